"""The rule of hupr_pose_decode_integral_f32 (include/hupr.h) restated in NumPy fp64, and the synthetic planes its tests share: sub-pixel
Gaussian targets as hupr_gaussian_targets_subpixel_f32 draws them, clean and under additive noise.  Written here: the reference project
has no integral decode.  Imported by tests/test_pose_integral_cpu.py and tests/test_pose_integral_gpu.py; no GPU needed."""
import functools

import numpy as np

U = 2.0 ** -24                          # the unit round-off of fp32


def ref_integral(h32, radius, dtype=np.float64):
    """h32 (rows, H, W) float32 maps -> dict of (rows, ...) arrays: idx, maxval (first maximum wins, a NaN is never the maximum), off =
    (Mx / m, My / m) over the window of ``radius`` around the peak clipped to the map (0: the whole map), pos = peak + off in heat-map
    pixels ((0, 0) where the maximum is not positive), spread = (sum w |x - px| / m, sum w |y - py| / m), the scale of the moments'
    rounding error, and cells, the number of window cells.  Weights w = max(h, 0), a NaN weighs 0; a window whose mass is not positive
    and finite, or whose offset is not finite, gives the offset (0, 0)."""
    h32 = np.asarray(h32)
    rows, H, W = h32.shape
    out = dict(idx=np.zeros(rows, np.int64), maxval=np.zeros(rows, np.float32), off=np.zeros((rows, 2), dtype), pos=np.zeros((rows, 2), dtype),
               spread=np.zeros((rows, 2), dtype), cells=np.zeros(rows, np.int64))
    rad = max(H, W) if radius == 0 else min(int(radius), max(H, W))
    for r in range(rows):
        flat = h32[r].reshape(-1)
        i = int(np.argmax(np.where(np.isnan(flat), -np.inf, flat)))
        mx = flat[i]
        out["idx"][r], out["maxval"][r] = i, mx
        if not mx > 0:
            continue
        px, py = i % W, i // W
        x0, x1, y0, y1 = max(px - rad, 0), min(px + rad, W - 1), max(py - rad, 0), min(py + rad, H - 1)
        w = h32[r, y0:y1 + 1, x0:x1 + 1].astype(dtype)
        w = np.where(np.isnan(w), dtype(0), np.maximum(w, dtype(0)))
        v, u = np.mgrid[y0 - py:y1 - py + 1, x0 - px:x1 - px + 1].astype(dtype)
        out["cells"][r] = w.size
        with np.errstate(all="ignore"):
            m = w.sum(dtype=dtype)
            off = np.array([(w * u).sum(dtype=dtype) / m, (w * v).sum(dtype=dtype) / m])
            spread = np.array([(w * np.abs(u)).sum(dtype=dtype) / m, (w * np.abs(v)).sum(dtype=dtype) / m])
        if m > 0 and np.isfinite(m) and np.isfinite(off).all():
            out["off"][r], out["spread"][r] = off, spread
        out["pos"][r] = (px + out["off"][r, 0], py + out["off"][r, 1])
    return out


def roundings(cells):
    """The fp32 roundings on the way to one moment of a window of ``cells`` cells in the stated summation shape: a lane adds at most
    ceil(cells / 64) terms in sequence (one rounding each: an addition for m, a fused multiply-add for Mx and My), then the 6 additions
    of the wave butterfly."""
    return -(-np.asarray(cells) // 64) + 6


def offset_bound(ref):
    """|fp32 offset - fp64 offset| per row and axis, to first order in U.  With D = roundings(cells): the numerator M is a sum of terms
    of one rounding each whose partial sums never exceed sum w |x - px| in magnitude, so |dM| <= D U sum w |x - px|; the weights are
    >= 0, so |dm| <= D U m; the quotient adds one rounding.  o = M / m then errs by at most D U spread + D U |o| + U |o|
    <= (D + 1) U (spread + |o|).  The bound is twice that: the second-order terms and nothing else."""
    D = roundings(ref["cells"])[:, None]
    return 2.0 * (D + 1) * U * (ref["spread"] + np.abs(ref["off"]))


def position_bound(ref, ratio):
    """|fp32 raw keypoint - ratio * fp64 pos|: the offset's bound plus the two roundings of (px + ox) * ratio, all times ratio."""
    return ratio * (offset_bound(ref) + 2.0 * U * np.abs(ref["pos"]) * (1 + 2 * U))


# ---- planes -----------------------------------------------------------------------------------------------------------------------------
def target_planes(centres, H=64, sigma=2.0, rad=6):
    """centres (n, 2) = (x, y) in heat-map pixels -> (n, H, H) float32: the planes hupr_gaussian_targets_subpixel_f32 draws for the
    joints centres * stride: exp(-((x - cx)^2 + (y - cy)^2) / (2 sigma^2)) on the (2 rad + 1)^2 patch around the pixel
    (int)(c + 0.5), zero elsewhere (fp64 arithmetic, rounded once)."""
    c = np.asarray(centres, dtype=np.float64)
    mu = np.floor(c + 0.5)
    g = np.arange(H, dtype=np.float64)
    dx, dy = g[None, :] - c[:, 0:1], g[None, :] - c[:, 1:2]                     # (n, H) each
    inx, iny = np.abs(g[None, :] - mu[:, 0:1]) <= rad, np.abs(g[None, :] - mu[:, 1:2]) <= rad
    ex, ey = np.where(inx, np.exp(-dx * dx / (2.0 * sigma * sigma)), 0.0), np.where(iny, np.exp(-dy * dy / (2.0 * sigma * sigma)), 0.0)
    return (ey[:, :, None] * ex[:, None, :]).astype(np.float32)


NOISE_LEVELS = (0.02, 0.05, 0.10)
N_PLANES, SEED = 2000, 20181012


@functools.lru_cache(maxsize=None)
def noise_case(level, n=N_PLANES):
    """``n`` 64 x 64 targets of sigma 2 with centres uniform in [8, 55] (seed fixed), as 0.8 * target + N(0, level), clipped to
    [1e-4, 1]; level 0 = the clean targets themselves -> (float32 planes, fp64 centres).  Read-only, shared."""
    rng = np.random.RandomState(SEED + int(round(level * 1000)))
    centres = rng.uniform(8.0, 55.0, (n, 2))
    t = target_planes(centres)
    if level > 0:
        t = np.clip(0.8 * t.astype(np.float64) + rng.normal(0.0, level, t.shape), 1e-4, 1.0).astype(np.float32)
    t.setflags(write=False)
    centres.setflags(write=False)
    return t, centres


def error_stats(pos, centres):
    """Euclidean error per plane in heat-map pixels -> (mean, 99th percentile)."""
    e = np.sqrt(((np.asarray(pos, dtype=np.float64) - centres) ** 2).sum(axis=1))
    return float(e.mean()), float(np.percentile(e, 99))
