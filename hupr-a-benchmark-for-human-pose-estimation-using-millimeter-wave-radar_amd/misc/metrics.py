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


DECODES = ("argmax", "subpixel", "integral")
TARGET_SIGMA = {64: 2, 128: 3}          # the Gaussian targets' sigma per map size (LossComputer.targets); the patch radius is 3 sigma


def decode_setting(cfg):
    """``TEST.decode`` (not a key of the reference's YAML): absent or ``argmax`` = the reference's arg-max decode, ``subpixel`` =
    ``get_final_preds``, ``integral`` = ``get_integral_preds`` at ``decode_radius_setting``.  Anything else raises here, where the
    config is read."""
    name = getattr(getattr(cfg, "TEST", None), "decode", "argmax")
    if not isinstance(name, str) or name not in DECODES:
        raise ValueError("TEST.decode must be 'argmax', 'subpixel' or 'integral', got %r" % (name,))
    return name


def default_decode_radius(heatmap_size):
    """The integral decode's default window radius: the radius of the targets' patch, 3 sigma of the map size (6 at 64, 9 at 128)."""
    if heatmap_size not in TARGET_SIGMA:
        raise ValueError("no default decode radius for %r x %r heat-maps (the targets are defined for %s); give one"
                         % (heatmap_size, heatmap_size, " and ".join(str(s) for s in sorted(TARGET_SIGMA))))
    return 3 * TARGET_SIGMA[heatmap_size]


def check_decode_radius(radius, heatmap_size, what):
    """-> ``radius`` as an int: 0 (the whole plane) or an integer in [1, heatmap_size - 1]; a bool, a float, a string, a negative or a
    larger value is a ValueError naming ``what``."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= heatmap_size - 1:
        raise ValueError("%s must be 0 (the whole plane) or an integer in [1, %d], got %r" % (what, heatmap_size - 1, radius))
    return int(radius)


def decode_radius_setting(cfg):
    """``TEST.decodeRadius`` (not a key of the reference's YAML) -> None unless ``TEST.decode`` is ``integral``; then the window radius
    of the integral decode in heat-map pixels: absent = ``default_decode_radius``, 0 = the whole plane, else an integer in
    [1, heatmapSize - 1].  Anything else, and the key without ``TEST.decode: integral``, raises here, where the config is read."""
    test = getattr(cfg, "TEST", None)
    integral = decode_setting(cfg) == "integral"
    if not hasattr(test, "decodeRadius"):
        return default_decode_radius(cfg.DATASET.heatmapSize) if integral else None
    if not integral:
        raise ValueError("TEST.decodeRadius needs TEST.decode: integral, got TEST.decode %r" % (decode_setting(cfg),))
    return check_decode_radius(test.decodeRadius, cfg.DATASET.heatmapSize, "TEST.decodeRadius")


def get_final_preds(batch_heatmaps):
    """``get_max_preds`` with the arg-max refined to sub-pixel position (second-order Taylor step on the log heat-map, quarter-pixel
    fallback; functional.pose_decode): (B,K,H,W) GPU tensor -> (preds ndarray (B,K,2) float32 [x,y] in heat-map pixels, at most half a
    pixel from get_max_preds', maxvals ndarray (B,K,1))."""
    if not isinstance(batch_heatmaps, torch.Tensor) or batch_heatmaps.dim() != 4:
        raise AssertionError("batch_heatmaps should be a 4-dim GPU tensor")
    _, mx, raw, _, _ = F_.pose_decode(batch_heatmaps, 1.0, refine=True)
    return raw.cpu().numpy(), mx.cpu().numpy()[:, :, None]


def get_integral_preds(batch_heatmaps, radius):
    """``get_max_preds`` with the arg-max replaced by the mass centroid of the window of ``radius`` heat-map pixels around it (0: the
    whole plane) — functional.pose_decode_integral, the decode the integral coordinate loss trains: (B,K,H,W) GPU tensor -> (preds
    ndarray (B,K,2) float32 [x,y] in heat-map pixels, at most ``radius`` from get_max_preds', maxvals ndarray (B,K,1))."""
    if not isinstance(batch_heatmaps, torch.Tensor) or batch_heatmaps.dim() != 4:
        raise AssertionError("batch_heatmaps should be a 4-dim GPU tensor")
    _, mx, raw, _, _ = F_.pose_decode_integral(batch_heatmaps, 1.0, radius)
    return raw.cpu().numpy(), mx.cpu().numpy()[:, :, None]
