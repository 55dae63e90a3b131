"""LossComputer (reference misc/losses.py:8-48) with device-side targets, BCE and decode."""

import math

import numpy as np
import torch

from .. import functional as F_
from .metrics import decode_radius_setting, decode_setting, get_final_preds, get_integral_preds, get_max_preds

PAIR_BCE = True      # test aid: False = one BCE node per head, combined by torch

TARGETS = ("integer", "subpixel")


def targets_setting(cfg):
    """``TRAINING.targets`` (not a key of the reference's YAML): absent or ``integer`` = the reference's targets, a fixed patch
    centred on the whole heat-map pixel nearest the integer joint; ``subpixel`` = the Gaussian centred on the float joint's real
    position inside that window (``functional.gaussian_targets_subpixel``).  Anything else raises here, where the config is read."""
    name = getattr(getattr(cfg, "TRAINING", None), "targets", "integer")
    if not isinstance(name, str) or name not in TARGETS:
        raise ValueError("TRAINING.targets must be 'integer' or 'subpixel', got %r" % (name,))
    return name


def ohkm_setting(cfg):
    """``TRAINING.ohkm`` (not a key of the reference's YAML) -> None (absent or -1: off, the YAML's own "-1 = off" idiom) or ``k``, an
    int in [1, DATASET.numKeypoints]: online hard keypoint mining, per head and sample only the ``k`` joints with the largest loss
    carry loss and gradient (``functional.MinedBCEFn``).  Anything else (0, a bool, a float, a string, out of range) raises here,
    where the config is read."""
    v = getattr(getattr(cfg, "TRAINING", None), "ohkm", -1)
    K = cfg.DATASET.numKeypoints
    if isinstance(v, int) and not isinstance(v, bool):
        if v == -1:
            return None
        if 1 <= v <= K:
            return v
    raise ValueError("TRAINING.ohkm must be -1 (off) or an int in [1, numKeypoints = %d], got %r" % (K, v))


def joint_weights_setting(cfg):
    """``TRAINING.jointWeights`` (not a key of the reference's YAML) -> None (absent or -1: off) or the per-joint loss weights as a
    list of DATASET.numKeypoints floats in ``DATASET.idxToJoints`` order: finite, >= 0, not all zero.  Anything else raises here,
    where the config is read."""
    v = getattr(getattr(cfg, "TRAINING", None), "jointWeights", -1)
    K = cfg.DATASET.numKeypoints
    if isinstance(v, (int, float)) and not isinstance(v, bool) and v == -1:
        return None
    if isinstance(v, (list, tuple)) and len(v) == K and \
            all(isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x) and x >= 0 for x in v) and any(x > 0 for x in v):
        return [float(x) for x in v]
    raise ValueError("TRAINING.jointWeights must be -1 (off) or a list of numKeypoints = %d finite weights >= 0, not all zero, "
                     "got %r" % (K, v))


def coord_loss_setting(cfg):
    """``TRAINING.coordLoss`` (not a key of the reference's YAML) -> None (absent or -1: off) or the weight lambda, a finite number
    > 0, of the integral coordinate loss that computeLoss adds to the heat-map loss (``functional.CoordLossFn``).  Anything else (0, a
    negative, nan, inf, a bool, a string, a list) raises here, where the config is read."""
    v = getattr(getattr(cfg, "TRAINING", None), "coordLoss", -1)
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        if v == -1:
            return None
        if math.isfinite(v) and v > 0:
            return float(v)
    raise ValueError("TRAINING.coordLoss must be -1 (off) or a finite weight > 0, got %r" % (v,))


def bone_loss_setting(cfg):
    """``TRAINING.boneLoss`` (not a key of the reference's YAML) -> None (absent or -1: off) or the weight mu, a finite number > 0,
    of the bone-vector loss that computeLoss adds to the heat-map loss (``functional.BoneLossFn``).  Anything else (0, a negative,
    nan, inf, a bool, a string, a list) raises here, where the config is read."""
    v = getattr(getattr(cfg, "TRAINING", None), "boneLoss", -1)
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        if v == -1:
            return None
        if math.isfinite(v) and v > 0:
            return float(v)
    raise ValueError("TRAINING.boneLoss must be -1 (off) or a finite weight > 0, got %r" % (v,))


def bone_weights(joint_weights, bones):
    """Per-bone weights from per-joint ones: w_e = sqrt(w_u w_v), taken in fp64 and stored as fp32, so a joint of weight zero
    silences its bones and equal joint weights carry over unchanged."""
    return [float(np.float32(math.sqrt(float(joint_weights[u]) * float(joint_weights[v])))) for u, v in bones]


class LossComputer():
    def __init__(self, cfg, device):
        self.device = device
        self.cfg = cfg
        self.numFrames = cfg.DATASET.numFrames
        self.numGroupFrames = cfg.DATASET.numGroupFrames
        self.numKeypoints = cfg.DATASET.numKeypoints
        self.heatmapSize = self.width = self.height = cfg.DATASET.heatmapSize
        self.imgSize = self.imgWidth = self.imgHeight = cfg.DATASET.imgSize
        self.lossDecay = cfg.TRAINING.lossDecay
        self.decode = decode_setting(cfg)       # TEST.decode: how the host-decode branch below turns preds2 into pred2d
        self.decodeRadius = decode_radius_setting(cfg)      # TEST.decodeRadius: the integral decode's window (None for the others)
        self.targets_mode = targets_setting(cfg)    # TRAINING.targets: which joints computeLoss takes and how targets() encodes them
        # TRAINING.ohkm / TRAINING.jointWeights: with either set computeLoss takes the mined loss (k = numKeypoints for weights alone)
        self.ohkm = ohkm_setting(cfg)
        self.jointWeights = joint_weights_setting(cfg)
        self.mined = self.ohkm is not None or self.jointWeights is not None
        self.mined_k = (self.ohkm if self.ohkm is not None else self.numKeypoints) if self.mined else None
        # the weights and the (2, K) selection counters live on the device from the start: a captured step replays their updates
        self._joint_w = torch.tensor(self.jointWeights, dtype=torch.float32, device=device) if self.jointWeights is not None else None
        self.mining_counts = torch.zeros((2, self.numKeypoints), dtype=torch.int64, device=device) if self.mined else None
        self.plane_loss = None          # the last mined loss's (2, B, K) unweighted plane losses, on the device
        # TRAINING.coordLoss: computeLoss adds lambda times the integral coordinate loss of both heads (csrc/coord_loss.hip); its
        # accumulator {sum C_0, sum C_1, steps} lives on the device from the start, as the selection counters do
        self.coordLoss = coord_loss_setting(cfg)
        self.coord_acc = torch.zeros(3, dtype=torch.float64, device=device) if self.coordLoss is not None else None
        self.coord_residual = None      # the last coordinate loss's (2, B, K, 2) residuals in heat-map pixels, on the device
        if self.coordLoss is not None:
            self.computeLoss = self._computeLossWithCoord       # without the key computeLoss stays the method below, untouched
        # TRAINING.boneLoss: computeLoss adds mu times the bone-vector loss of both heads (csrc/bone_loss.hip) over the data set's
        # skeleton, on top of whatever the keys above made of it; the accumulator {sum B_0, sum B_1, steps} lives on the device
        self.boneLoss = bone_loss_setting(cfg)
        self.bone_acc = self.bones = self._bone_w = None
        self.bone_residual = None       # the last bone loss's (2, B, E, 2) bone residuals in heat-map pixels, on the device
        if self.boneLoss is not None:
            self.bones = F_.bone_table(None, self.numKeypoints)
            self.bone_acc = torch.zeros(3, dtype=torch.float64, device=device)
            if self.jointWeights is not None:
                self._bone_w = torch.tensor(bone_weights(self.jointWeights, self.bones), dtype=torch.float32, device=device)
            self._computeLossBeforeBone = self.computeLoss      # the method below, or the one with the coordinate term
            self.computeLoss = self._computeLossWithBone
        self.alpha = 0.0
        self.beta = 1.0

    def targets(self, gt):
        sigma = {64: 2, 128: 3}[self.heatmapSize]
        if self.targets_mode == "subpixel":
            return F_.gaussian_targets_subpixel(gt.to(self.device), self.heatmapSize, self.imgSize, sigma)
        return F_.gaussian_targets(gt.to(self.device), self.heatmapSize, self.imgSize, sigma)

    def computeLoss(self, preds, gt, decode=True):
        """preds = (heatmap (B,K,1,H,W), gcn_heatmap (B,1,K,H,W)); gt (B,K,2) integer joints — with
        ``TRAINING.targets: subpixel`` the float joints (an integer tensor is accepted there and means whole pixels).
        -> (loss, loss2, pred2d ndarray, gt2d ndarray) — same tuple as the reference."""
        heatmaps = self.targets(gt)
        preds1, preds2 = preds
        K, H, W = self.numKeypoints, self.height, self.width
        a1, a2 = preds1.reshape(-1, K, H, W), preds2.reshape(-1, K, H, W)
        if self.alpha < 1.0:
            self.alpha += self.lossDecay
            self.beta -= self.lossDecay
        if self.mined:
            # online hard keypoint mining / per-joint weights (csrc/bce_mined.hip): the launches of the pair loss below.  The
            # selection counters move only where gradients are recorded: evaluation shows the trained loss and does not count
            w = (self.alpha, self.beta) if self.lossDecay != -1 else (1.0, 1.0)
            loss, loss2 = F_.MinedBCEFn.apply(a1, a2, heatmaps, self.mined_k, self._joint_w, w[0], w[1],
                                              self.mining_counts if torch.is_grad_enabled() else None)
            self.plane_loss = F_.MinedBCEFn.last_plane_loss
        elif PAIR_BCE and a1.is_cuda and a1.dtype == a2.dtype == heatmaps.dtype == torch.float32 and a1.shape == a2.shape == heatmaps.shape:
            # both losses and their weighted sum as one node (two launches forward, one backward; the same floats)
            w = (self.alpha, self.beta) if self.lossDecay != -1 else (1.0, 1.0)
            loss, loss2 = F_.PairBCEFn.apply(a1, a2, heatmaps, w[0], w[1])
        else:
            loss1 = F_.BCEFn.apply(a1, heatmaps)
            loss2 = F_.BCEFn.apply(a2, heatmaps)
            if self.lossDecay != -1:
                loss = self.alpha * loss1 + self.beta * loss2
            else:
                loss = loss1 + loss2
        if not decode:
            return loss, loss2, None, None
        if decode == "device":
            # the reference decodes both arg-max sets every iteration (misc/losses.py:43-44); here the two decodes are
            # kernels on the step's stream and the (B,K) index / maximum tensors stay on the device (no sync, no D2H)
            return loss, loss2, F_.argmax_rows(preds2.detach().reshape(-1, H * W)), F_.argmax_rows(heatmaps.reshape(-1, H * W))
        if self.decode == "integral":
            pred2d, _ = get_integral_preds(preds2.detach().reshape(-1, K, H, W), self.decodeRadius)
        else:
            final = get_final_preds if self.decode == "subpixel" else get_max_preds
            pred2d, _ = final(preds2.detach().reshape(-1, K, H, W))
        gt2d, _ = get_max_preds(heatmaps)
        return loss, loss2, pred2d, gt2d

    def _computeLossWithCoord(self, preds, gt, decode=True):
        """computeLoss with ``TRAINING.coordLoss`` set: the same tuple, ``loss`` being the heat-map loss plus lambda times the
        coordinate term of both heads on every valid joint, whatever the mining keeps; ``loss2`` stays the second head's BCE.  The
        head weights are those the BCE pair just got.  The accumulator moves only where gradients are recorded, as the selection
        counters do."""
        loss, loss2, pred2d, gt2d = LossComputer.computeLoss(self, preds, gt, decode)
        K, H, W = self.numKeypoints, self.height, self.width
        w = (self.alpha, self.beta) if self.lossDecay != -1 else (1.0, 1.0)
        coord, _ = F_.CoordLossFn.apply(preds[0].reshape(-1, K, H, W), preds[1].reshape(-1, K, H, W), gt.to(self.device),
                                        self.imgSize / self.heatmapSize, self.targets_mode == "integer", self._joint_w,
                                        self.coordLoss * w[0], self.coordLoss * w[1],
                                        self.coord_acc if torch.is_grad_enabled() else None)
        self.coord_residual = F_.CoordLossFn.last_residual
        return loss + coord, loss2, pred2d, gt2d

    def _computeLossWithBone(self, preds, gt, decode=True):
        """computeLoss with ``TRAINING.boneLoss`` set: the same tuple, ``loss`` being the loss of the other keys plus mu times the
        bone-vector term of both heads on every valid bone, whatever the mining keeps; ``loss2`` stays the second head's BCE.  The
        head weights are those the BCE pair just got; with ``TRAINING.jointWeights`` a bone weighs sqrt(w_u w_v).  The accumulator
        moves only where gradients are recorded."""
        loss, loss2, pred2d, gt2d = self._computeLossBeforeBone(preds, gt, decode)
        K, H, W = self.numKeypoints, self.height, self.width
        w = (self.alpha, self.beta) if self.lossDecay != -1 else (1.0, 1.0)
        bone, _ = F_.BoneLossFn.apply(preds[0].reshape(-1, K, H, W), preds[1].reshape(-1, K, H, W), gt.to(self.device),
                                      self.imgSize / self.heatmapSize, self.targets_mode == "integer", self.bones, self._bone_w,
                                      self.boneLoss * w[0], self.boneLoss * w[1], self.bone_acc if torch.is_grad_enabled() else None)
        self.bone_residual = F_.BoneLossFn.last_residual
        return loss + bone, loss2, pred2d, gt2d
