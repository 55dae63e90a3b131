"""The rule of hupr_cfar_ra_f32 and hupr_presence_update (include/hupr.h) restated in NumPy, in fp64, and the inputs the detector
tests share.  Written here: the reference project has no detector.  Imported by tests/test_cfar_cpu.py, tests/test_cfar_gpu.py,
tests/test_stream_presence_gpu.py; no GPU needed."""
import functools

import numpy as np

R = A = 64
DEAD_SLOT = 4                                    # the clutter-nulled zero-Doppler slot: never examined
SLOTS = tuple(f for f in range(8) if f != DEAD_SLOT)
PAIRS = ((0, 1), (1, 2), (2, 4), (0, 8))         # the (guard, train) pairs of the tests
DEFAULTS = dict(pfa=1e-5, guard=2, train=4, min_cells=3, confirm=2, hold=20)


def alpha(pfa, N):
    """The closed form N (pfa^(-1/N) - 1) in fp64, as written."""
    N = np.asarray(N, dtype=np.float64)
    return N * (np.float64(pfa) ** (-1.0 / N) - 1.0)


def ring_offsets(g, t):
    """[(dr, da)] of the training cells: g < max(|dr|, |da|) <= g + t."""
    w = g + t
    return [(dr, da) for dr in range(-w, w + 1) for da in range(-w, w + 1) if g < max(abs(dr), abs(da)) <= w]


@functools.lru_cache(maxsize=None)
def window_counts(g, t):
    """(R, A) int: the number of training cells of every cell, counted one by one (cells outside the map are not counted)."""
    n = np.zeros((R, A), dtype=np.int64)
    rr, aa = np.mgrid[0:R, 0:A]
    for dr, da in ring_offsets(g, t):
        n += ((rr + dr >= 0) & (rr + dr < R) & (aa + da >= 0) & (aa + da < A))
    return n


def border_cells(g, t):
    """(R, A) bool: the cells whose window leaves the map."""
    return window_counts(g, t) < len(ring_offsets(g, t))


def power(x32):
    """(n, 16, R, A) float32 planes -> (n, 8, R, A) fp64 power, slot 4 included (the callers leave it out)."""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64).reshape(-1, 8, 2, R, A)
    return x[:, :, 0] ** 2 + x[:, :, 1] ** 2


def ref_cfar(x32, pfa, g, t):
    """The detector on (n, 16, R, A) float32 planes -> dict of fp64 / int arrays, (n, 8, R, A) each unless noted:
    p, noise, snr, ratio = p / (alpha[N] noise), mask (uint8), N (R, A), summary (n, 8).  Slot 4: mask 0, snr 0, noise and ratio NaN."""
    p = power(x32)
    n = p.shape[0]
    N = window_counts(g, t)
    tot = np.zeros_like(p)
    pad = np.zeros((n, 8, R + 2 * (g + t), A + 2 * (g + t)))
    w = g + t
    pad[:, :, w:w + R, w:w + A] = p
    for dr, da in ring_offsets(g, t):
        tot += pad[:, :, w + dr:w + dr + R, w + da:w + da + A]
    with np.errstate(all="ignore"):
        noise = tot / N
        thr = alpha(pfa, N) * noise
        ratio = p / thr
        mask = (p > thr)
        snr = np.where((p == 0) & (noise == 0), 0.0, p / noise)
    mask[:, DEAD_SLOT] = False
    snr[:, DEAD_SLOT] = 0.0
    noise[:, DEAD_SLOT] = np.nan
    ratio[:, DEAD_SLOT] = np.nan
    return dict(p=p, noise=noise, snr=snr, ratio=ratio, mask=mask.astype(np.uint8), N=N, summary=ref_summary(mask, snr))


def ref_summary(mask, snr):
    """(n, 8, R, A) mask and SNR -> (n, 8) fp64: count, peak_snr, peak_f, peak_r, peak_a, centroid_r, centroid_a, doppler."""
    mask = np.asarray(mask).astype(bool)
    n = mask.shape[0]
    out = np.zeros((n, 8))
    ff, rr, aa = np.mgrid[0:8, 0:R, 0:A]
    for i in range(n):
        m = mask[i]
        if not m.any():
            out[i] = (0, 0, -1, -1, -1, 0, 0, 0)
            continue
        s = snr[i][m]
        k = int(np.argmax(s))                    # first maximum in (f, r, a) order
        with np.errstate(all="ignore"):
            out[i] = (m.sum(), s[k], ff[m][k], rr[m][k], aa[m][k], (s * rr[m]).sum() / s.sum(), (s * aa[m]).sum() / s.sum(),
                      (s * (ff[m] - 4)).sum() / s.sum())
    return out


def ref_gate(counts, min_cells, confirm, hold, state=None):
    """The presence gate over a sequence of per-frame counts -> (present per frame, state (present, hits, misses, frames))."""
    present, hits, misses, frames = state if state is not None else (0, 0, 0, 0)
    out = []
    for c in counts:
        hit = c >= min_cells
        hits = hits + 1 if hit else 0
        misses = 0 if hit else misses + 1
        if not present and hits >= confirm:
            present = 1
        elif present and misses > hold:
            present = 0
        frames += 1
        out.append(present)
    return np.asarray(out, dtype=np.int32), (present, hits, misses, frames)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
def noise_planes(n, seed):
    """(n, 16, R, A) float32: unit complex-Gaussian noise in every slot."""
    from hupr_amd import synth
    return synth.normal((n, 16, R, A), "cfar_noise", seed)


def spike_planes(n, seed, gain=1e4):
    """Noise plus, in every frame, one cell at ``gain`` times the mean noise power (2): what a difference of box sums would get wrong
    in its neighbourhood."""
    x = noise_planes(n, seed).copy()
    for i in range(n):
        f, r, a = (1, 6, 2)[i % 3], 20 + 7 * i, 31 - 5 * i
        x[i, 2 * f, r, a] = np.float32(np.sqrt(2.0 * gain))
        x[i, 2 * f + 1, r, a] = 0.0
    return x


def border_planes(n, seed, gain=300.0):
    """Noise plus strong cells in the four corners and on each edge, spread over the slots; their amplitudes differ, so no two SNRs tie."""
    x = noise_planes(n, seed).copy()
    spots = [(0, 0), (0, A - 1), (R - 1, 0), (R - 1, A - 1), (0, 29), (R - 1, 40), (17, 0), (45, A - 1)]
    for i in range(n):
        for k, (r, a) in enumerate(spots):
            f = SLOTS[(k + i) % 7]
            x[i, 2 * f, r, a] = np.float32(np.sqrt(2.0 * gain * (1.0 + 0.13 * k + 0.05 * i)))
            x[i, 2 * f + 1, r, a] = 0.0
    return x


INPUTS = {"noise": noise_planes, "spike": spike_planes, "border": border_planes}
