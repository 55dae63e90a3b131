"""Scene occupancy, offline: cell-averaging CFAR detection on the (range, azimuth) maps of the loader's elevation-mean planes
(csrc/cfar.hip; the rule is stated beside hupr_cfar_ra_f32 in include/hupr.h).  The stage between the FFT chain and the estimator that
answers "is there a mover, and where".  ``pfa``, ``guard`` and ``train`` default to guesses: nobody has run this on a real capture.
"""
import math

import numpy as np
import torch

CFAR_DEFAULTS = {"pfa": 1e-5, "guard": 2, "train": 4}
CFAR_MAX_HALF = 8          # guard + train at most: the 17 x 17 window (csrc/cfar_host.h)


def check_cfar(pfa, guard, train):
    """The detector's three settings -> (float pfa, int guard, int train); ValueError for a ``pfa`` outside (0, 1), ``guard`` < 0,
    ``train`` < 1, ``guard + train`` > 8 or a value of the wrong kind."""
    if isinstance(pfa, bool) or not isinstance(pfa, (int, float, np.integer, np.floating)) or not math.isfinite(pfa) or not 0 < pfa < 1:
        raise ValueError("pfa must be a number in (0, 1), got %r" % (pfa,))
    for name, v, lo in (("guard", guard, 0), ("train", train, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError("%s must be an integer >= %d, got %r" % (name, lo, v))
    if guard + train > CFAR_MAX_HALF:
        raise ValueError("guard + train must not exceed %d, got %d + %d" % (CFAR_MAX_HALF, guard, train))
    return float(pfa), int(guard), int(train)


def cfar_window_cells(guard, train):
    """Training cells of an interior cell: (2 w + 1)^2 - (2 g + 1)^2, w = guard + train."""
    w = guard + train
    return (2 * w + 1) ** 2 - (2 * guard + 1) ** 2


def cfar_alpha_table(pfa=CFAR_DEFAULTS["pfa"], guard=CFAR_DEFAULTS["guard"], train=CFAR_DEFAULTS["train"]):
    """The CA-CFAR threshold factors in fp64: entry N = alpha[N] = N (pfa^(-1/N) - 1) for N = 1 .. (2 w + 1)^2 - (2 g + 1)^2 training
    cells, exact for exponentially distributed cells; entry 0 = +inf (no training cell, never a detection).  The device takes its
    fp32 rounding, and a cell near the border reads the entry of its own, smaller N."""
    pfa, guard, train = check_cfar(pfa, guard, train)
    n = np.arange(1, cfar_window_cells(guard, train) + 1, dtype=np.float64)
    return np.concatenate([[np.inf], n * np.expm1(-math.log(pfa) / n)])


def cfar_detect(x, pfa=CFAR_DEFAULTS["pfa"], guard=CFAR_DEFAULTS["guard"], train=CFAR_DEFAULTS["train"], want_mask=True, want_snr=False,
                zero_doppler=None, tdm_compensation=False):
    """The detector on ``x``: int16 ADC cubes (n, 4, 192, 256, 2) on the GPU, which go through ``fft_chain_loader_means`` first
    (``zero_doppler`` / ``tdm_compensation`` as there), or ready fp32 mean planes (..., 16, 64, 64) -> ``functional.CfarResult``
    (``summary`` (..., 8), ``mask`` uint8 and ``snr`` fp32 (..., 8, 64, 64) when asked for).  Device tensors, no sync."""
    from .. import functional as F_
    from .process_iwr1843 import fft_chain_loader_means
    if not isinstance(x, torch.Tensor):
        raise ValueError("cfar_detect needs a torch tensor, got %s" % type(x).__name__)
    if x.dtype == torch.int16:
        x = fft_chain_loader_means(x, zero_doppler=zero_doppler, tdm_compensation=tdm_compensation)
    elif zero_doppler is not None or tdm_compensation:
        raise ValueError("zero_doppler / tdm_compensation are settings of the FFT chain: they need int16 ADC cubes, got %s planes" % x.dtype)
    return F_.cfar_ra(x, pfa, guard, train, want_mask=want_mask, want_snr=want_snr)
