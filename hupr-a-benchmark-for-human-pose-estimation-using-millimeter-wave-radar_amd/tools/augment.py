"""Radar augmentation on the device and the flip test (csrc/augment.hip, section (a14) of include/hupr.h).

Settings (none of them a key of the reference's YAML; each absent or ``-1`` = off, anything invalid raises where the config is read):

  ``TRAINING.augMirror``     probability in (0, 1] of mirroring a sample left/right
  ``TRAINING.augNoise``      sigma_max > 0: per sample sigma ~ U[0, sigma_max), Gaussian noise in units of the normalised input
  ``TRAINING.augMaskRange``  int in [1, rangeSize / 2]: per sample one band of up to that many range bins is zeroed in both maps
  ``TRAINING.augMaskAngle``  int in [1, azimuthSize / 2]: per sample and map one band of up to that many azimuth bins is zeroed
  ``TEST.flip``              bool: evaluate with the flip test (``TrainEngine.infer_from_adc(..., flip=True)``)
  ``DATASET.tdmCompensation`` bool (absent = false): Doppler phase compensation of the TDM-MIMO virtual array in the FFT chain
                             (``preprocessing.tdm_phase_table``; read here because it meets the mirror, below)

What "mirror" means for this radar.  Reversing the azimuth axis of the network input is wrong: the FFT chain's azimuth index is
``a -> (31 - a) mod 64`` in frequency, so a mirrored target lands on ``(62 - a) mod 64``, and a scene mirrored about the array centre
also carries the per-bin phase ``exp(-2 pi i 7 ((31 - a) mod 64) / 64)``, which cannot be applied behind ``Normalize`` (it takes mean
and std of the real and imaginary planes separately).  The exact operation is a permutation of the raw ADC cube in front of the
chain: reverse the receivers and swap transmitters 0 and 2 (``mirror_adc_host``; ``hupr_adc_mirror_i16`` on the device).  Hence the
mirror needs raw ADC cubes; stored, already normalised cubes can take the noise and the masks only.

Two approximations.  The vertical sensor's cube is left as it is: the mirrored scene would reflect that array's two-row axis, which
is not symmetric (8 antennas in one row, 4 in the other), and the network only ever sees the mean over that axis.  Swapping the two
transmitters also swaps their time slots: with ``DATASET.tdmCompensation`` off (the default; the reference compensates no TDM phase
either) a target in Doppler bin ``d`` keeps a residual phase of the order ``2 pi d / 96`` between the two antenna halves.  With the key
on the residual vanishes: the engine hands the plan's mirror flags to the chain, which compensates a mirrored frame with the slots of
transmitters 0 and 2 exchanged, and the mirror identity (index map times ramp) holds exactly on the compensated cube.

The labels are mirrored about the centre of the heat-map grid, ``x' = stride (H - 1) - x`` (252 - x), with ``L_*`` and ``R_*`` joints
exchanged: the decode maps heat-map pixel ``m`` to image ``4 m``, so only this axis makes the mirrored target the mirror
``m -> H - 1 - m`` of the target; where the radar's boresight falls in the image is not known to better than the 1.5 px between the two
choices.  One tie case: with integer targets a joint whose ``x / 4`` lies exactly on ``.5`` rounds up on both sides of the mirror, so
its mirrored target is one pixel off the mirror of its target.

The numpy half of this module (``philox4x32``, ``plan_reference``, ``noise_reference``, ``mirror_adc_host``) restates the device's
rules on the host; the tests compare the two.
"""
import ctypes
import math

import numpy as np
import torch

from .. import runtime as rt

MIRROR_NEEDS_ADC = ("TRAINING.augMirror needs raw ADC cubes (train_step_from_adc / a raw-ADC dataset): the mirror of this radar is a "
                    "permutation of the ADC cube in front of the FFT chain — reversing the azimuth axis of an already normalised input "
                    "is off by one bin and by a per-bin phase that cannot be applied behind Normalize")

# columns of the plan table (B, 8)
MIRROR, SIGMA, RANGE_LEN, RANGE_START, HORI_LEN, HORI_START, VERT_LEN, VERT_START = range(8)


# ---- settings -----------------------------------------------------------------------------------------------------------------
def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _off(v):
    return _number(v) and v == -1


def aug_mirror_setting(cfg):
    """``TRAINING.augMirror`` -> None (absent or -1: off) or the probability, a number in (0, 1]."""
    v = getattr(getattr(cfg, "TRAINING", None), "augMirror", -1)
    if _off(v):
        return None
    if _number(v) and 0 < v <= 1:                   # False for NaN
        return float(v)
    raise ValueError("TRAINING.augMirror must be -1 (off) or a probability in (0, 1], got %r" % (v,))


def aug_noise_setting(cfg):
    """``TRAINING.augNoise`` -> None (absent or -1: off) or sigma_max, a finite number > 0 that fp32 holds as one."""
    v = getattr(getattr(cfg, "TRAINING", None), "augNoise", -1)
    if _off(v):
        return None
    if _number(v) and math.isfinite(v) and 2.0 ** -149 <= v <= float(np.finfo(np.float32).max):
        return float(v)
    raise ValueError("TRAINING.augNoise must be -1 (off) or a finite sigma_max > 0, got %r" % (v,))


def _band_setting(cfg, key, size_key):
    v = getattr(getattr(cfg, "TRAINING", None), key, -1)
    size = getattr(cfg.DATASET, size_key)
    if isinstance(v, int) and not isinstance(v, bool):
        if v == -1:
            return None
        if 1 <= v <= size // 2:
            return v
    raise ValueError("TRAINING.%s must be -1 (off) or an int in [1, DATASET.%s / 2 = %d], got %r" % (key, size_key, size // 2, v))


def aug_mask_range_setting(cfg):
    """``TRAINING.augMaskRange`` -> None (absent or -1: off) or the longest range band, an int in [1, DATASET.rangeSize / 2]."""
    return _band_setting(cfg, "augMaskRange", "rangeSize")


def aug_mask_angle_setting(cfg):
    """``TRAINING.augMaskAngle`` -> None (absent or -1: off) or the longest azimuth band, an int in [1, DATASET.azimuthSize / 2]."""
    return _band_setting(cfg, "augMaskAngle", "azimuthSize")


def flip_setting(cfg):
    """``TEST.flip`` -> bool (absent: False).  Anything but a bool raises."""
    v = getattr(getattr(cfg, "TEST", None), "flip", False)
    if isinstance(v, bool):
        return v
    raise ValueError("TEST.flip must be true or false, got %r" % (v,))


TDM_NEEDS_RANGE_DOPPLER = ("DATASET.tdmCompensation is set, but this dataset reads stored cubes: the compensation acts on the range-Doppler map, "
                           "which a stored cube no longer has.  Cubes written with processRadarDataHoriVert(tdm_compensation=True) are already "
                           "compensated and are used with the key off")


def tdm_setting(cfg):
    """``DATASET.tdmCompensation`` -> bool (absent: False).  Anything but a bool raises."""
    v = getattr(getattr(cfg, "DATASET", None), "tdmCompensation", False)
    if isinstance(v, bool):
        return v
    raise ValueError("DATASET.tdmCompensation must be true or false, got %r" % (v,))


def augment_settings(cfg):
    """-> None when no training key is set, else {"p_mirror", "sigma_max", "max_range", "max_angle"} with 0 for a key that is off."""
    vals = (aug_mirror_setting(cfg), aug_noise_setting(cfg), aug_mask_range_setting(cfg), aug_mask_angle_setting(cfg))
    if all(v is None for v in vals):
        return None
    return dict(zip(("p_mirror", "sigma_max", "max_range", "max_angle"), (v if v is not None else 0 for v in vals)))


def mirror_pairs(names):
    """The joint exchanged with each joint by the left/right mirror: ``L_x`` <-> ``R_x``, every other name maps to itself.  A
    one-sided name (``L_x`` without ``R_x`` or the reverse) or a repeated name is an error."""
    names = list(names)
    index = {}
    for i, n in enumerate(names):
        if not isinstance(n, str) or n in index:
            raise ValueError("mirror_pairs: joint names must be distinct strings, got %r" % (names,))
        index[n] = i
    pairs = []
    for n in names:
        if n[:2] in ("L_", "R_"):
            other = ("R_" if n[0] == "L" else "L_") + n[2:]
            if other not in index:
                raise ValueError("mirror_pairs: joint %r has no counterpart %r" % (n, other))
            pairs.append(index[other])
        else:
            pairs.append(index[n])
    return pairs


# ---- host mirror of the device's rules (numpy) -----------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=10):
    """Philox4x32 (Salmon et al., SC 2011).  counter: (..., 4), key: (..., 2) broadcastable, unsigned 32-bit values -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(rounds):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2            # 32 x 32 -> 64 bits, no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def _words(step, seed, rank, domain, b, q):
    b, q = np.broadcast_arrays(np.asarray(b, dtype=np.uint64), np.asarray(q, dtype=np.uint64))
    ctr = np.stack([np.full(b.shape, step & 0xFFFFFFFF, dtype=np.uint64), np.full(b.shape, (step >> 32) & 0xFFFFFFFF, dtype=np.uint64), b, q],
                   axis=-1)
    return philox4x32(ctr, np.array([seed & 0xFFFFFFFF, (4 * rank + domain) & 0xFFFFFFFF], dtype=np.uint64))


def plan_reference(B, step, seed, rank, p_mirror, sigma_max, max_range, max_angle, R, A):
    """The plan ``hupr_augment_plan`` draws for ``B`` samples at counter ``step`` -> ((B, 8) int32 table with sigma's fp32 bits in
    column SIGMA, (B,) uint8 mirror flags)."""
    b = np.arange(B)
    w0, w1 = _words(step, seed, rank, 0, b, 0), _words(step, seed, rank, 0, b, 1)
    m0, m1 = (w0 >> 8).astype(np.int64), (w1 >> 8).astype(np.int64)
    table = np.zeros((B, 8), dtype=np.int32)
    table[:, MIRROR] = (m0[:, 0].astype(np.float32) * np.float32(2.0 ** -24)) < np.float32(p_mirror)
    sigma = (np.float32(sigma_max) * (m0[:, 1].astype(np.float32) * np.float32(2.0 ** -24))).astype(np.float32)
    table[:, SIGMA] = sigma.view(np.int32)
    table[:, RANGE_LEN] = (m0[:, 2] * (max_range + 1)) >> 24
    table[:, RANGE_START] = (m0[:, 3] * (R - table[:, RANGE_LEN] + 1)) >> 24
    table[:, HORI_LEN] = (m1[:, 0] * (max_angle + 1)) >> 24
    table[:, HORI_START] = (m1[:, 1] * (A - table[:, HORI_LEN] + 1)) >> 24
    table[:, VERT_LEN] = (m1[:, 2] * (max_angle + 1)) >> 24
    table[:, VERT_START] = (m1[:, 3] * (A - table[:, VERT_LEN] + 1)) >> 24
    return table, table[:, MIRROR].astype(np.uint8)


def plan_sigma(table):
    """Column SIGMA of a plan table as float32."""
    return np.ascontiguousarray(np.asarray(table)[:, SIGMA]).view(np.float32)


def noise_reference(step, seed, rank, sensor, b, n):
    """The ``n`` standard normal values of sample ``b`` that ``hupr_augment_apply_f32`` adds (times sigma) for the plan drawn at
    counter ``step``, in fp64 from the same Philox words: Box-Muller, two pairs per call."""
    nq = (n + 3) // 4
    w = _words(step, seed, rank, 1 + sensor, b, np.arange(nq)).astype(np.float64)
    m = np.floor(w / 256.0)
    z = np.empty((nq, 4), dtype=np.float64)
    for i in (0, 2):
        r = np.sqrt(-2.0 * np.log((m[:, i] + 0.5) * 2.0 ** -24))
        t = 2.0 * np.pi * (m[:, i + 1] * 2.0 ** -24)
        z[:, i], z[:, i + 1] = r * np.cos(t), r * np.sin(t)
    return z.reshape(-1)[:n]


def mirror_adc_host(cube):
    """The left/right mirror of ADC cubes (..., 4 rx, 192 = 3 cc + tx, 256, 2) on the host: receivers reversed, transmitters 0 and 2
    swapped."""
    cube = np.asarray(cube)
    c = np.arange(192)
    return np.ascontiguousarray(cube[..., ::-1, :, :, :][..., c + 2 - 2 * (c % 3), :, :])


def mirror_joints_host(joints, pairs, x_mirror):
    """(B, K, 2) joints of mirrored samples (torch or numpy): ``x' = x_mirror - x``, joint j taken from ``pairs[j]``."""
    out = joints[:, list(pairs)].clone() if isinstance(joints, torch.Tensor) else np.array(joints[:, list(pairs)])
    out[..., 0] = x_mirror - out[..., 0]
    return out


# ---- device entry points ---------------------------------------------------------------------------------------------------------
def _pair_array(pairs):
    return (ctypes.c_int * len(pairs))(*pairs)


def adc_mirror(adc, flags=None, G=1):
    """int16 GPU cubes (n, 4, 192, 256, 2) -> a new tensor with the frames of the flagged samples mirrored (``flags``: (n / G,) uint8 on
    the device, None = every frame)."""
    if adc.dtype != torch.int16 or tuple(adc.shape[1:]) != (4, 192, 256, 2):
        raise ValueError("adc must be int16 (n,4,192,256,2), got %s %r" % (adc.dtype, tuple(adc.shape)))
    n = adc.shape[0]
    if flags is not None and (flags.dtype != torch.uint8 or flags.numel() * G != n):
        raise ValueError("flags must be uint8 with one entry per %d frames, got %s %r for %d frames" % (G, flags.dtype, tuple(flags.shape), n))
    out = torch.empty_like(adc, memory_format=torch.contiguous_format)
    rt.check(rt.lib().hupr_adc_mirror_i16(rt.ptr(adc), rt.ptr(out), n, G, rt.ptr(flags), rt.stream()))
    return out


def mirror_joints(joints, pairs, x_mirror, flags=None):
    """(B, K, 2) int64 or float32 GPU joints -> a new tensor with the flagged samples' labels mirrored (None = every sample)."""
    if joints.dim() != 3 or joints.shape[2] != 2 or joints.dtype not in (torch.int64, torch.float32):
        raise ValueError("joints must be (B,K,2) int64 or float32, got %s %r" % (joints.dtype, tuple(joints.shape)))
    B, K = joints.shape[:2]
    if flags is not None and (flags.dtype != torch.uint8 or flags.numel() != B):
        raise ValueError("flags must be uint8 (B,), got %s %r" % (flags.dtype, tuple(flags.shape)))
    joints = joints.contiguous()
    out = torch.empty_like(joints)
    rt.check(rt.lib().hupr_augment_joints(rt.ptr(joints), rt.ptr(out), B, K, int(joints.is_floating_point()), rt.ptr(flags),
                                          _pair_array(pairs), int(x_mirror), rt.stream()))
    return out


def flip_merge(p, pm, pairs):
    """``0.5 * (p + mirror(pm))`` of one head's maps, ``p`` and ``pm`` fp32 GPU tensors of one shape whose last two axes are (H, W) and
    whose leading axes hold B x K planes in (b, k) order; the result has ``p``'s shape."""
    K = len(pairs)
    if p.dtype != torch.float32 or pm.dtype != torch.float32 or p.shape != pm.shape or p.dim() < 3 or p.numel() % (K * p.shape[-1] * p.shape[-2]):
        raise ValueError("flip_merge: p and pm must be fp32 of one shape (..., H, W) holding B x %d planes, got %r %r" % (K, tuple(p.shape), tuple(pm.shape)))
    H, W = p.shape[-2:]
    p, pm = p.contiguous(), pm.contiguous()
    out = torch.empty_like(p)
    rt.check(rt.lib().hupr_flip_merge_f32(rt.ptr(p), rt.ptr(pm), rt.ptr(out), p.numel() // (K * H * W), K, H, W, _pair_array(pairs), rt.stream()))
    return out


class Augmenter:
    """The training-time augmentation of one engine: the settings, the device state block {counter, mirrored, samples, sum of sigma},
    and the last plan.  ``plan(B)`` draws the step's plan (one launch); ``adc`` / ``apply`` / ``labels`` consume it."""

    def __init__(self, cfg, settings, device, seed=0, rank=0):
        self.p_mirror, self.sigma_max = settings["p_mirror"], settings["sigma_max"]
        self.max_range, self.max_angle = settings["max_range"], settings["max_angle"]
        self.R, self.A = cfg.DATASET.rangeSize, cfg.DATASET.azimuthSize
        self.G = cfg.DATASET.numGroupFrames
        self.pairs = mirror_pairs(cfg.DATASET.idxToJoints)
        self.x_mirror = (cfg.DATASET.imgSize // cfg.DATASET.heatmapSize) * (cfg.DATASET.heatmapSize - 1)
        self.seed, self.rank = int(seed) & 0xFFFFFFFF, int(rank)
        self.device = torch.device(device)
        assert rt.lib().hupr_augment_state_bytes() == 32
        self.state = torch.zeros(4, dtype=torch.int64, device=self.device)       # the f64 sum is viewed in stats()
        self.table = self.flags = None

    @property
    def mirrors(self):
        return self.p_mirror > 0

    @property
    def transforms_input(self):
        return self.sigma_max > 0 or self.max_range > 0 or self.max_angle > 0

    def plan(self, B):
        """Draw the plan of the next step for ``B`` samples on the current stream."""
        self.table = torch.empty((B, 8), dtype=torch.int32, device=self.device)
        self.flags = torch.empty((B,), dtype=torch.uint8, device=self.device)
        rt.check(rt.lib().hupr_augment_plan(B, rt.ptr(self.state), self.p_mirror, self.sigma_max, self.max_range, self.max_angle, self.R,
                                            self.A, self.seed, self.rank, rt.ptr(self.table), rt.ptr(self.flags), rt.stream()))

    def adc(self, adc_hori):
        """The horizontal cube with the plan's mirrored samples permuted (a new tensor); the cube itself when the mirror is off."""
        return adc_mirror(adc_hori, self.flags, self.G) if self.mirrors else adc_hori

    def labels(self, joints):
        """The joints of the plan's mirrored samples mirrored (a new tensor on the device); as they come when the mirror is off."""
        return mirror_joints(joints.to(self.device), self.pairs, self.x_mirror, self.flags) if self.mirrors else joints

    def apply(self, x, sensor):
        """Noise and masks of the last plan on a network input (B, ..., R, A) (elevation-mean planes) or (B, ..., R, A, E) (the
        reference-shaped 7-D tensor), in place; ``sensor`` 0 = horizontal, 1 = vertical."""
        if not self.transforms_input:
            return x
        B = x.shape[0]
        if x.dtype != torch.float32 or self.table is None or self.table.shape[0] != B:
            raise ValueError("Augmenter.apply: fp32 input with the plan's batch size expected, got %s %r" % (x.dtype, tuple(x.shape)))
        if x.dim() == 7 and tuple(x.shape[4:6]) == (self.R, self.A):
            E = x.shape[6]
        elif tuple(x.shape[-2:]) == (self.R, self.A):
            E = 1
        else:
            raise ValueError("Augmenter.apply: input must end in (R, A) = (%d, %d) or be the 7-D (B,G,F,2,R,A,E) tensor, got %r"
                             % (self.R, self.A, tuple(x.shape)))
        P = x[0].numel() // (self.R * self.A * E)
        rt.check(rt.lib().hupr_augment_apply_f32(rt.ptr(x), rt.ptr(x), B, P, self.R, self.A, E, rt.ptr(self.table), sensor, rt.ptr(self.state),
                                                 self.seed, self.rank, rt.stream()))
        return x

    # -- host bookkeeping ----------------------------------------------------------------------------------------------------------
    def stats(self):
        """{"steps", "samples", "mirrored", "mean_sigma", "last_plan"}: plans drawn so far, the samples they covered, how many of them
        were mirrored, the mean of their sigma, and the last plan's (B, 8) int32 table (sigma's fp32 bits in column 1; None before
        the first plan).  Synchronises the device: per epoch, not per step."""
        st = self.state.cpu().numpy()
        samples = int(st[2])
        return {"steps": int(st[0]), "samples": samples, "mirrored": int(st[1]),
                "mean_sigma": float(st[3:4].view(np.float64)[0]) / max(samples, 1),
                "last_plan": self.table.cpu().numpy() if self.table is not None else None}

    def set_step(self, step):
        """Resume: the next plan is drawn at counter ``step`` (the statistics are diagnostics and start over)."""
        step = int(step)
        if step < 0:
            raise ValueError("Augmenter.set_step: step must be >= 0, got %r" % (step,))
        self.state.copy_(torch.tensor([step, 0, 0, 0], dtype=torch.int64))
