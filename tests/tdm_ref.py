"""The fp64 statement of the Doppler phase compensation for the TDM-MIMO virtual array (include/hupr.h, hupr_fft_chain_tdm), for the
tests: the oracle's demux, range-Doppler transform and angle transform with the rule applied between them, the output index map of
SURVEY.md App. A restated, and the loader forms (Normalize per (re/im, elevation) plane, the elevation mean) in fp64.

The rule.  Virtual antenna v in the chain's workspace order: v = 0..3 is TX0 in slot 0, v = 4..7 is TX2 in slot 2, v = 8..11 is TX1 — the
elevated row — in slot 1; a swapped sensor-frame has slots 2 and 0 on the two azimuth halves.  The range-Doppler value of antenna v at
signed Doppler bin d is multiplied by exp(-2 pi j d k(v) / 192)."""
import numpy as np

from oracle import fft_chain as offt

SLOTS = np.array([0, 0, 0, 0, 2, 2, 2, 2, 1, 1, 1, 1])
SLOTS_SWAPPED = np.array([2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 1, 1])


def slots(swapped=False):
    return SLOTS_SWAPPED if swapped else SLOTS


def table(swapped=False):
    """(12, 16) complex128: the factor of antenna v at kept Doppler index i (signed bin d = i - 8)."""
    d, k = np.arange(16) - 8, slots(swapped)
    out = np.exp(-2j * np.pi * d[None, :] * k[:, None] / 192.0)
    out[:, 8] = 1.0
    out[k == 0, :] = 1.0
    return out


def compensate(az, el, swapped=False):
    """The rule on the oracle's range-Doppler arrays az (8, 64 Doppler, 256), el (4, 64, 256): every FFT bin by its signed Doppler bin."""
    d = np.arange(64)
    d = np.where(d < 32, d, d - 64).astype(np.float64)
    k = slots(swapped).astype(np.float64)
    f = np.exp(-2j * np.pi * d[None, :] * k[:, None] / 192.0)            # (12, 64)
    f[:, 0] = 1.0
    f[k == 0, :] = 1.0
    return az * f[:8, :, None], el * f[8:, :, None]


def index_map(M5):
    """out[i, r, a, e] = M5[(3 - e) % 8, (31 - a) % 64, (56 + i) % 64, 94 - r]   """
    e = (3 - np.arange(8)) % 8
    a = (31 - np.arange(64)) % 64
    d = (56 + np.arange(16)) % 64
    r = 94 - np.arange(64)
    return np.ascontiguousarray(M5[e[None, None, None, :], a[None, None, :, None], d[:, None, None, None], r[None, :, None, None]])


def cube(frame, compensated=True, swapped=False, window=0, zero_doppler=None, iq=None):
    """frame: complex (4, 192, 256) -> complex128 (16, 64, 64, 8).  ``zero_doppler``: None = the fp64 residue of the transform,
    "dither" = the chain's default stand-in (needs the int16 cube ``iq`` (4, 192, 256, 2)), "exact" = zeros."""
    az, el = offt.demux(frame)
    az, el = offt.range_doppler(az, el, window)
    if zero_doppler == "dither":
        dz = np.fft.fft(offt.zero_doppler_dither(iq), axis=1)
        az[:, 0, :], el[:, 0, :] = dz[:8], dz[8:]
    elif zero_doppler == "exact":
        az[:, 0, :], el[:, 0, :] = 0.0, 0.0
    if compensated:
        az, el = compensate(az, el, swapped)
    return index_map(offt.angle_cube(az, el))


def cube_iq(iq, **kw):
    """int16 (4, 192, 256, 2) -> ``cube`` of its complex frame."""
    iq = np.asarray(iq)
    return cube(iq[..., 0].astype(np.float64) + 1j * iq[..., 1].astype(np.float64), iq=iq, **kw)


def normalize(plane):
    """Normalize (datasets/base.py:13-24) of one (range, azimuth) plane in fp64: (x - mean) / unbiased std — the min / max
    rescaling in front of it cancels."""
    plane = np.asarray(plane, dtype=np.float64)
    return (plane - plane.mean()) / plane.std(ddof=1)


def loader(c):
    """complex (16, 64, 64, 8) -> float64 (8 f, 2 re/im, 64, 64, 8): Doppler indices 4..11, every (re/im, elevation) plane normalised."""
    out = np.empty((8, 2, 64, 64, 8), dtype=np.float64)
    for f in range(8):
        for e in range(8):
            out[f, 0, :, :, e] = normalize(c[4 + f, :, :, e].real)
            out[f, 1, :, :, e] = normalize(c[4 + f, :, :, e].imag)
    return out


def means(ld):
    """(8, 2, 64, 64, 8) -> (16, 64, 64): plane 2 f + c, the mean over elevation."""
    return ld.mean(axis=-1).reshape(16, 64, 64)
