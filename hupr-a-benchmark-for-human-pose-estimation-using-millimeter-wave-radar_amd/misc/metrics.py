"""Arg-max decode on the GPU (reference misc/metrics.py:10-38)."""
import numpy as np
import torch

from .. import functional as F_


def get_max_preds(batch_heatmaps):
    """batch_heatmaps: GPU tensor (B,K,H,W) -> (preds ndarray (B,K,2) float32 [x,y], maxvals ndarray (B,K,1)).
    First maximum wins on ties (np.argmax); joints whose maximum is <= 0 decode to (0,0)."""
    if not isinstance(batch_heatmaps, torch.Tensor) or batch_heatmaps.dim() != 4:
        raise AssertionError("batch_heatmaps should be a 4-dim GPU tensor")
    B, K, H, W = batch_heatmaps.shape
    idx, mx = F_.argmax_rows(batch_heatmaps.reshape(B * K, H * W))
    idx = idx.cpu().numpy().reshape(B, K).astype(np.int64)
    mx = mx.cpu().numpy().reshape(B, K, 1)
    preds = np.stack([idx % W, idx // W], axis=2).astype(np.float32)
    preds *= (mx > 0.0).astype(np.float32)
    return preds, mx


DECODES = ("argmax", "subpixel")


def decode_setting(cfg):
    """``TEST.decode`` (not a key of the reference's YAML): absent or ``argmax`` = the reference's arg-max decode, ``subpixel`` =
    ``get_final_preds``.  Anything else raises here, where the config is read."""
    name = getattr(getattr(cfg, "TEST", None), "decode", "argmax")
    if name not in DECODES:
        raise ValueError("TEST.decode must be 'argmax' or 'subpixel', got %r" % (name,))
    return name


def get_final_preds(batch_heatmaps):
    """``get_max_preds`` with the arg-max refined to sub-pixel position (second-order Taylor step on the log heat-map, quarter-pixel
    fallback; functional.pose_decode): (B,K,H,W) GPU tensor -> (preds ndarray (B,K,2) float32 [x,y] in heat-map pixels, at most half a
    pixel from get_max_preds', maxvals ndarray (B,K,1))."""
    if not isinstance(batch_heatmaps, torch.Tensor) or batch_heatmaps.dim() != 4:
        raise AssertionError("batch_heatmaps should be a 4-dim GPU tensor")
    _, mx, raw, _, _ = F_.pose_decode(batch_heatmaps, 1.0, refine=True)
    return raw.cpu().numpy(), mx.cpu().numpy()[:, :, None]
