"""The fp64 answer of every form of the FFT chain (csrc/fft_chain.hip; include/hupr.h hupr_fft_chain_opts / hupr_fft_chain_tdm), for
tests/test_fft_fp64_gpu.py and tests/test_fft_route.py.  Nothing is restated here that tests/tdm_ref.py or oracle/fft_chain.py already
state: the demux, the windows, the transforms, the index map, the dither, the TDM rule and Normalize are theirs.

A form is (window bits 0..3, convention, loader 0 / 1 / 2, magnitude, tdm); a sensor-frame of a TDM form is swapped or not.

The zero-Doppler index (Doppler index 8, loader slot f = 4, mean planes 8 and 9) per form — ``zero_rule``:
  "dither"     Doppler-first without the Doppler window, default convention: the UNWINDOWED dither, whatever the range window;
  "exact"      Doppler-first without the Doppler window under HUPR_FFT_ZERO_DOPPLER_EXACT: zeros (a zero plane normalises to zeros);
  None         the range-first order, or any form with the Doppler window: the plain fp64 transform of the mean-free cube.  With the
               Doppler window that is honest leakage; without it (range-first) it is zero to ~1e-16 A.

The scale A of a (frame, form) is the L2 norm of the raw int16 samples times the window weights of the form — NOT mean-removed: the
clutter cancels inside the kernels in fp32, so their error scales with what goes in.  At a dithered zero-Doppler index the scale is
the L2 norm of the dither's input instead."""
import collections
import hashlib

import numpy as np

import tdm_ref
from oracle import fft_chain as offt

Form = collections.namedtuple("Form", "window convention loader magnitude tdm")
CONVENTIONS = ("dither", "exact", "range_first")
Answer = collections.namedtuple("Answer", "ref A scale std cube ld")
# ref    the fp64 answer in the form's layout: (16, 64, 64, 8) complex or |.|, (8, 2, 64, 64, 8), (16, 64, 64)
# A      the frame's scale (above)
# scale  (16,) the scale per Doppler index: A, and the dither's at index 8 of a dithered form
# std    loader forms: (8, 2, 8) the fp64 unbiased std of the reference plane (f, re/im, e) before Normalize; else None
# cube   the fp64 complex cube behind ref (read-only, shared)
# ld     loader forms: the fp64 loader tensor (8, 2, 64, 64, 8) behind ref; else None


def zero_rule(window, convention):
    assert convention in CONVENTIONS and 0 <= window <= 3
    return None if (window & 2) or convention == "range_first" else convention


def window_weights(window):
    """(64 chirp loops, 256 samples): the weights that multiply a sample of the form."""
    wd = np.hanning(offt.NUM_LOOPS) if window & 2 else np.ones(offt.NUM_LOOPS)
    wr = np.hanning(offt.NUM_SAMPLE) if window & 1 else np.ones(offt.NUM_SAMPLE)
    return wd[:, None] * wr[None, :]


def frame_scale(iq, window):
    iq = np.asarray(iq)
    assert iq.dtype == np.int16 and iq.shape == (4, 192, 256, 2)
    w = np.repeat(window_weights(window), 3, axis=0)                       # chirp 3 c + tx has the weight of loop c
    return float(np.sqrt(((iq.astype(np.float64) ** 2).sum(-1) * (w ** 2)[None]).sum()))


def dither_scale(iq):
    return float(np.linalg.norm(offt.zero_doppler_dither(np.asarray(iq))))


_CUBES = {}


def _key(iq):
    return hashlib.sha1(np.ascontiguousarray(iq).tobytes()).digest()


def cube(iq, window=0, convention="dither", compensated=False, swapped=False):
    """int16 (4, 192, 256, 2) -> complex128 (16, 64, 64, 8), computed once per (frame, window, zero rule, compensated, swapped) and
    never modified."""
    zd = zero_rule(window, convention)
    key = (_key(iq), window, zd, bool(compensated), bool(swapped) and bool(compensated))
    if key not in _CUBES:
        c = tdm_ref.cube_iq(iq, compensated=bool(compensated), swapped=bool(swapped), window=window, zero_doppler=zd)
        c.setflags(write=False)
        _CUBES[key] = c
    return _CUBES[key]


def drop_cache():
    """Forget the cached cubes (8 MiB each): the modules that use them call this when they are done."""
    _CUBES.clear()


def plane_std(c):
    """(8, 2, 8): the unbiased std of the (range, azimuth) plane of loader slot f, re / im, elevation e."""
    k = c[4:12]
    return np.stack([k.real.std(axis=(1, 2), ddof=1), k.imag.std(axis=(1, 2), ddof=1)], axis=1)


def loader(c):
    """tdm_ref.loader, with an exactly-zero plane normalised to zeros (include/hupr.h: "the loader epilogues then emit zeros")."""
    out = np.zeros((8, 2, 64, 64, 8), dtype=np.float64)
    for f in range(8):
        for e in range(8):
            for k, p in enumerate((c[4 + f, :, :, e].real, c[4 + f, :, :, e].imag)):
                if p.any():
                    out[f, k, :, :, e] = tdm_ref.normalize(p)
    return out


def answer(iq, form, swapped=False):
    """The fp64 answer of ``form`` on the int16 frame ``iq`` -> Answer."""
    c = cube(iq, form.window, form.convention, form.tdm, swapped)
    A = frame_scale(iq, form.window)
    scale = np.full(16, A)
    if zero_rule(form.window, form.convention) == "dither":
        scale[8] = dither_scale(iq)
    assert not (form.loader and form.magnitude)
    if form.loader == 0:
        return Answer(np.abs(c) if form.magnitude else c, A, scale, None, c, None)
    ld = loader(c)
    return Answer(ld if form.loader == 1 else tdm_ref.means(ld), A, scale, plane_std(c), c, ld)
