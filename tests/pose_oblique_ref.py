"""The oblique scenario the pose-tracker family is tested on where x and y couple: 24 frames x 12 joints of 20 x 27 heat-maps, every map
one rotated anisotropic Gaussian, four of the joints at the map's borders, at two parameter points.  The scenarios of
tests/pose_track_ref.py and its descendants draw isotropic Gaussians well inside a 64 x 64 map: their window moment Sxy, and with it
every cross term of the filter and of the smoothers (P01, P03, P12, P23), is zero to rounding.  Here the median |Sxy| / sqrt(Sxx Syy) is
about 0.5 and the median |Pxy| / sqrt(Pxx Pyy) about 0.4.  Written here: the reference project has no tracker.  The rules themselves are
those of tests/pose_track_ref.py, pose_imm_ref.py, pose_nll_ref.py, pose_smooth_ref.py, pose_lag_ref.py, pose_assoc_ref.py and
pose_pairs_ref.py, used as they are.  Imported by tests/test_pose_oblique_cpu.py and tests/test_pose_oblique_gpu.py; no GPU and no
package needed."""
import functools
import types

import numpy as np

import pose_assoc_ref as A
import pose_imm_ref as ir
import pose_lag_ref as lr
import pose_nll_ref as nr
import pose_pairs_ref as Pr
import pose_smooth_ref as sr
import pose_track_ref as ref

T, ROWS, H, W = 24, 12, 20, 27                    # 540 pixels: no multiple of the 64 lanes of the arg-max
AMPLITUDE, FAINT, MIN_SCORE = 0.8, 0.05, 0.1
# Chosen so that the conditions of tests/test_pose_oblique_cpu.py hold with both decodes.  SEED draws the scenario, and the ghost variant
# is built on it with bumps from GHOST_SEED; the pair variant is built on the scenario of PAIR_SEED (with SEED's, the arg-max decode
# has a gate decision of the pair tracker 0.85 % from the gate at point B).
SEED, GHOST_SEED, PAIR_SEED = 3, 17, 4
LEFT, RIGHT, TOP, CORNER = 0, 1, 2, 3             # the border rows: by the left, right and top edge and in the bottom-right corner
BORDER = (LEFT, RIGHT, TOP, CORNER)
INTERIOR = tuple(range(4, ROWS))
DROP, DROP_FRAMES = 5, (6, 7, 8)                  # its score falls under MIN_SCORE for three frames
OUTLIER, OUTLIER_FRAME, OUTLIER_BY = 7, 11, (9.0, 4.0)       # heat-map pixels, towards the middle of the map
GONE, GONE_FRAMES = 9, tuple(range(5, 13))        # faint for eight frames: more than max_coast at both points
EVENT_ROWS = (DROP, OUTLIER, GONE)

POINTS = ("A", "B")
RATIO = dict(A=4.0, B=3.0)
SETTINGS = dict(A=dict(rate_hz=10.0, accel_psd=100.0, meas_std=1.0, heatmap_gain=1.0, gate=13.816, max_coast=5, init_speed_std=50.0,
                       horizon_s=0.3),
                B=dict(rate_hz=25.0, accel_psd=37.0, meas_std=1.5, heatmap_gain=0.37, gate=9.21, max_coast=2, init_speed_std=20.0,
                       horizon_s=0.12))
IMM = dict(accel_psd=5.0, accel_psd_moving=2000.0, switch_prob=0.05, moving_prior=0.5)
LAGS = (1, 4)
EXTENT = dict(A=(W * 4.0, H * 4.0), B=(W * 3.0, H * 3.0))    # the image of the map, in image pixels: what an outlier is uniform over

# The largest difference of the NumPy fp32 run of each restatement (window moments included; the smoothers behind an fp32 tracker run)
# from its fp64 run on this scenario, per rule and point: positions (image pixels), velocities (pixels / s), position covariance
# (pose_track_ref.cov_rel_diff), the tracker's whole covariance in its state after every frame (``state_cov_diff``), the probability
# ``moving``, the likelihood sum of a (candidate, row) cell relative to its magnitude.
# tests/test_pose_oblique_cpu.py measures them again and holds them; tests/test_pose_oblique_gpu.py allows each kernel 16 x them.
FP32 = {
    ("track", "A"): dict(pos=1.08e-5, vel=3.08e-5, cov=2.47e-7, state=6.26e-7),
    ("track", "B"): dict(pos=1.12e-5, vel=3.68e-5, cov=3.10e-7, state=7.89e-7),
    ("imm", "A"): dict(pos=1.09e-5, vel=2.86e-5, cov=8.49e-7, moving=6.61e-7),
    ("imm", "B"): dict(pos=1.15e-5, vel=6.09e-5, cov=1.45e-6, moving=1.71e-6),
    ("smooth", "A"): dict(pos=1.76e-5, vel=2.66e-5, cov=7.17e-6),
    ("smooth", "B"): dict(pos=1.28e-5, vel=2.25e-5, cov=3.06e-6),
    ("lag1", "A"): dict(pos=1.13e-5, vel=3.03e-5, cov=6.58e-7),
    ("lag1", "B"): dict(pos=1.12e-5, vel=3.78e-5, cov=5.31e-7),
    ("lag4", "A"): dict(pos=1.89e-5, vel=3.02e-5, cov=2.35e-6),
    ("lag4", "B"): dict(pos=1.31e-5, vel=3.96e-5, cov=2.54e-6),
    ("nll", "A"): dict(nll=9.31e-8),
    ("nll", "B"): dict(nll=4.96e-7),
}
MARGIN = 16                                       # the family's margin for FMA contraction and summation order (TOL_COV_REL = 16 x ...)


def bound(rule, point, what):
    """What tests/test_pose_oblique_gpu.py allows the kernel of ``rule`` at ``point``: MARGIN x the fp32-against-fp64 figure recorded above."""
    return MARGIN * FP32[rule, point][what]


def params(point, **kw):
    """The tracker parameters of ``point`` without importing the package: every attribute functional.pose_track and the restatements
    read (tools.PoseTracking's names)."""
    d = dict(SETTINGS[point], min_score=MIN_SCORE, candidates=1, min_separation=3, peak_ratio=0.25, gate_on_presence=False,
             pair_swap=False, swap_cost=0.0, pairs=None, accel_psd_moving=None, switch_prob=0.05, moving_prior=0.5)
    d.update(kw)
    return types.SimpleNamespace(**d)


def imm_params(point, **kw):
    return params(point, **dict(IMM, **kw))


# ---- the maps ----------------------------------------------------------------------------------------------------------------------------
def oblique_maps(centres, amplitude, major, minor, angle):
    """centres (rows, 2) (x, y) in heat-map pixels, amplitude, the sigmas along and across the major axis and its angle from x, each
    (rows,) -> (rows, H, W) float32: amplitude exp(-(a^2 / major^2 + b^2 / minor^2) / 2), a along and b across the major axis."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = xx[None] - centres[:, 0, None, None], yy[None] - centres[:, 1, None, None]
    c, s = np.cos(angle)[:, None, None], np.sin(angle)[:, None, None]
    a, b = dx * c + dy * s, -dx * s + dy * c
    return (amplitude[:, None, None] * np.exp(-0.5 * (a ** 2 / major[:, None, None] ** 2 + b ** 2 / minor[:, None, None] ** 2))).astype(np.float32)


def shapes(rng, rows):
    """-> (major in [2.2, 3.0], minor in [0.9, 1.3], angle of magnitude in [0.3, 1.2] rad with a random sign), each (rows,)."""
    return (rng.uniform(2.2, 3.0, rows), rng.uniform(0.9, 1.3, rows),
            rng.uniform(0.3, 1.2, rows) * np.where(rng.uniform(size=rows) < 0.5, -1.0, 1.0))


@functools.lru_cache(maxsize=None)
def scenario(events=True, seed=SEED):
    """-> (maps (T, ROWS, H, W) float32, truth (T, ROWS, 2), measured (T, ROWS, 2)), positions in heat-map pixels.  Tracks centre +
    amp sin(w t + phase) per axis, amp in [0.5, 2.5] pixels (0.5 on the border rows), w in [0.05, 0.2] rad / frame; every frame's map
    is one oblique Gaussian (``shapes``, drawn per row) of amplitude 0.8 at the track position plus N(0, sigma) noise, sigma in
    [0.25, 0.5] pixel per row (1 to 2 image pixels at ratio 4).  The border rows' measured positions are held within [0.3, 2.4] pixels
    of their edge, so their covariance window is clipped in every frame.  ``events``: the drop-out, outlier and gone rows."""
    rng = np.random.RandomState(seed)
    centre = np.stack([rng.uniform(8.0, 18.0, ROWS), rng.uniform(7.0, 12.0, ROWS)], axis=1)
    near = 1.35
    centre[LEFT, 0], centre[RIGHT, 0], centre[TOP, 1] = near, W - 1 - near, near
    centre[CORNER] = (W - 1 - near, H - 1 - near)
    amp, w, ph = rng.uniform(0.5, 2.5, (ROWS, 2)), rng.uniform(0.05, 0.2, (ROWS, 2)), rng.uniform(0.0, 2 * np.pi, (ROWS, 2))
    amp[list(BORDER)] = 0.5
    t = np.arange(T)[:, None, None]
    truth = centre[None] + amp[None] * np.sin(w[None] * t + ph[None])
    measured = truth + rng.normal(0.0, 1.0, truth.shape) * rng.uniform(0.25, 0.5, ROWS)[None, :, None]
    lo, hi = 0.3, 2.4
    measured[:, LEFT, 0] = np.clip(measured[:, LEFT, 0], lo, hi)
    measured[:, RIGHT, 0] = np.clip(measured[:, RIGHT, 0], W - 1 - hi, W - 1 - lo)
    measured[:, TOP, 1] = np.clip(measured[:, TOP, 1], lo, hi)
    measured[:, CORNER, 0] = np.clip(measured[:, CORNER, 0], W - 1 - hi, W - 1 - lo)
    measured[:, CORNER, 1] = np.clip(measured[:, CORNER, 1], H - 1 - hi, H - 1 - lo)
    major, minor, angle = shapes(rng, ROWS)
    amplitude = np.full((T, ROWS), AMPLITUDE)
    if events:
        middle = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
        measured[OUTLIER_FRAME, OUTLIER] += np.sign(middle - truth[OUTLIER_FRAME, OUTLIER]) * OUTLIER_BY
        amplitude[list(DROP_FRAMES), DROP] = FAINT
        amplitude[list(GONE_FRAMES), GONE] = FAINT
    maps = np.stack([oblique_maps(measured[k], amplitude[k], major, minor, angle) for k in range(T)])
    for a in (maps, truth, measured):
        a.setflags(write=False)
    return maps, truth, measured


GHOST_ROWS, GHOST_FRAMES, GHOST_AMPLITUDE = INTERIOR, tuple(range(4, 20)), 1.0


@functools.lru_cache(maxsize=None)
def ghost_scenario(seed=SEED, ghost_seed=GHOST_SEED):
    """``scenario(events=False)`` with a second oblique bump of amplitude 1.0 (the joint's is 0.8, so the ghost is the arg-max) on
    the interior rows in frames 4..19: 4.2 to 5.5 pixels beside the joint in x and 0.5 to 2.5 in y, towards the middle of the map, plus
    N(0, 0.3 pixel), with a shape of its own, merged by np.maximum -> (maps (T, ROWS, H, W) float32, truth (T, ROWS, 2))."""
    maps, truth, _ = scenario(False, seed)
    maps = maps.copy()
    rng = np.random.RandomState(ghost_seed)
    rows = list(GHOST_ROWS)
    middle = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    by = np.sign(middle[None] - truth[:, rows].mean(axis=0)) * np.stack([rng.uniform(4.2, 5.5, len(rows)), rng.uniform(0.5, 2.5, len(rows))], axis=1)
    major, minor, angle = shapes(rng, len(rows))
    for t in GHOST_FRAMES:
        at = truth[t, rows] + by + rng.normal(0.0, 0.3, (len(rows), 2))
        maps[t, rows] = np.maximum(maps[t, rows], oblique_maps(at, np.full(len(rows), GHOST_AMPLITUDE), major, minor, angle))
    maps.setflags(write=False)
    return maps, truth


PARTNER = (0, 1, 2, 3, 5, 4, 7, 6, 9, 8, 10, 11)  # three pairs among the interior rows, the rest their own partner
PAIRS = ((4, 5), (6, 7), (8, 9))
IDENTITY = tuple(range(ROWS))
SWAP_FRAMES = tuple(range(8, 16))


@functools.lru_cache(maxsize=None)
def pair_scenario(seed=PAIR_SEED):
    """``scenario(events=False, PAIR_SEED)`` with the two maps of every pair of ``PAIRS`` exchanged in frames 8..15 -> (maps, truth)."""
    maps, truth, _ = scenario(False, seed)
    maps = maps.copy()
    for t in SWAP_FRAMES:
        for a, b in PAIRS:
            maps[t, [a, b]] = maps[t, [b, a]]
    maps.setflags(write=False)
    return maps, truth


def ghost_run(point, refine=True):
    """The ghost variant through pose_assoc_ref with K = 2 -> (ref_assoc's dict, the candidates).  The restated peak finder refines its
    candidates unless told otherwise, so the arg-max decode goes through ref_peaks and ref_assoc, the two halves of ref_run."""
    maps, p = ghost_scenario()[0], params(point, candidates=2)
    if refine:
        return A.ref_run(maps, p, RATIO[point], 2)
    per = [A.ref_peaks(maps[t], 2, p.min_separation, p.peak_ratio, RATIO[point], False) for t in range(T)]
    c = {k: np.stack([o[k] for o in per]) for k in per[0]}
    return A.ref_assoc(c["xy"], c["score"], c["count"], c["mom"], p, RATIO[point]), c


def pair_run(point, refine=True):
    """The pair variant through pose_pairs_ref with K = 1 -> (ref_pairs' dict, the candidates)."""
    maps, p = pair_scenario()[0], params(point, pair_swap=True, pairs=PARTNER)
    c = None
    if not refine:
        per = [A.ref_peaks(maps[t], 1, p.min_separation, p.peak_ratio, RATIO[point], False) for t in range(T)]
        c = {k: np.stack([o[k] for o in per]) for k in per[0]}
    return Pr.ref_run(maps, p, PARTNER, 0.0, RATIO[point], 1, c=c)


# ---- the decode and the moments of a set of maps, restated ----------------------------------------------------------------------------------
def decode(maps, ratio, refine):
    """maps (T, rows, H, W) -> (idx (T, rows), maxval (T, rows) float32, raw (T, rows, 2) image pixels): np.argmax, first maximum wins,
    and the sub-pixel offset of pose_assoc_ref.refine_offset with ``refine`` — the fp64 stand-in of hupr_pose_decode_f32.  The GPU
    tests feed the rules the kernel's own decode instead."""
    Tn, rows = maps.shape[:2]
    flat = maps.reshape(Tn, rows, -1)
    idx = flat.argmax(axis=2)
    mx = np.take_along_axis(flat, idx[..., None], axis=2)[..., 0]
    raw = np.stack([idx % W, idx // W], axis=-1).astype(np.float64)
    if refine:
        for t in range(Tn):
            for r in range(rows):
                raw[t, r] += A.refine_offset(maps[t, r], int(idx[t, r] % W), int(idx[t, r] // W))
    return idx, mx, raw * ratio * (mx > 0)[..., None]


def moments(maps, idx, dtype=np.float64):
    """The window moments (pose_track_ref.window_moments) of every frame -> (T, rows, 4)."""
    return np.stack([ref.window_moments(maps[t], idx[t], dtype) for t in range(maps.shape[0])])


@functools.lru_cache(maxsize=None)
def inputs(point, refine=True, seed=SEED, events=True):
    """What the measurement-level rules read of the scenario at ``point`` -> (idx, maxval, raw (image pixels), moments fp64)."""
    maps = scenario(events, seed)[0]
    idx, mx, raw = decode(maps, RATIO[point], refine)
    return idx, mx, raw, moments(maps, idx)


@functools.lru_cache(maxsize=None)
def moments32(seed=SEED, events=True):
    maps = scenario(events, seed)[0]
    return moments(maps, maps.reshape(T, ROWS, -1).argmax(axis=2), np.float32)


def edge_distance(idx):
    """How many pixels the pixel ``idx`` lies from the nearest edge of the map; under 3 the covariance window is clipped."""
    px, py = idx % W, idx // W
    return np.minimum(np.minimum(px, W - 1 - px), np.minimum(py, H - 1 - py))


# ---- the runs ------------------------------------------------------------------------------------------------------------------------------
def track_run(point, raw, mx, mom, dtype=np.float64, **kw):
    """ref_track and its state after every frame -> (dict, states (T, rows, 16))."""
    return sr.track_with_states(raw.astype(dtype), mx, mom, params(point, **kw), RATIO[point], dtype)


def imm_run(point, raw, mx, mom, dtype=np.float64, **kw):
    return ir.ref_imm(raw.astype(dtype), mx, mom, imm_params(point, **kw), RATIO[point], dtype)


def smooth_run(point, states, status, kp, dtype=np.float64):
    p = params(point)
    return sr.ref_smooth(states, status, kp, p.rate_hz, p.accel_psd, dtype)


def lag_run(point, states, status, kp, L, dtype=np.float64):
    p = params(point)
    return lr.ref_lag(states, status, kp, p.rate_hz, p.accel_psd, L, dtype)


def nll_grid(point):
    """The 3 x 3 x 3 candidates around the point's (accel_psd, meas_std, heatmap_gain): factors (1/2, 1, 2), (1/sqrt 2, 1, sqrt 2) and
    (1/2, 1, 2), accel_psd the slow axis, rounded to fp32 as the launch reads them -> (27, 3) fp64; NLL_OWN is the point's own.  Every
    candidate has heatmap_gain > 0."""
    s = SETTINGS[point]
    q = s["accel_psd"] * np.array([0.5, 1.0, 2.0])
    m = s["meas_std"] * np.array([0.5 ** 0.5, 1.0, 2.0 ** 0.5])
    g = s["heatmap_gain"] * np.array([0.5, 1.0, 2.0])
    return np.stack([np.repeat(q, 9), np.tile(np.repeat(m, 3), 3), np.tile(g, 9)], axis=1).astype(np.float32).astype(np.float64)


NLL_OWN = 13


def nll_run(point, meas, dtype=np.float64):
    start = np.zeros(meas.shape[0], int)
    start[0] = 1
    return nr.ref_nll(meas, start, params(point), nll_grid(point), RATIO[point], EXTENT[point], dtype)


def state_cov_diff(states, states64):
    """Largest |Pij - Pij64| / sqrt(Pii64 Pjj64) over the ten covariance entries of the (..., 16) states whose fp64 track is live:
    every entry on the scale of its own two variances, so that the velocity block and the cross block count like the position block."""
    _, P = sr.unpack(states, np.float64)
    _, P64 = sr.unpack(states64, np.float64)
    live = np.asarray(states64)[..., 14] == 1
    d = np.sqrt(np.diagonal(P64, axis1=-2, axis2=-1))
    return float((np.abs(P - P64)[live] / (d[..., :, None] * d[..., None, :])[live]).max())


def nll_rel_diff(nll, o64):
    """Largest |nll - nll64| / |nll64| over the (candidate, row) cells that scored a frame."""
    keep = o64["counts"][..., 5] > 0
    return float((np.abs(np.asarray(nll, dtype=np.float64) - o64["nll"])[keep] / np.abs(o64["nll"][keep])).max())


# ---- what the sensitivity and the equivariance tests change ----------------------------------------------------------------------------------
CROSS = (5, 7, 9, 12)                             # P01, P03, P12, P23 in the 16 floats of a state


def without_sxy(mom):
    out = np.array(mom)
    out[..., 2] = np.where(np.isnan(out[..., 2]), np.nan, 0.0)
    return out


def without_cross(states):
    out = np.array(states)
    out[..., list(CROSS)] = 0
    return out


def rotation(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s], [s, c]])


def rotate_moments(mom, Q):
    """(..., 4) = (m, Sxx, Sxy, Syy) -> the same with S replaced by Q S Q^T."""
    S = np.stack([np.stack([mom[..., 1], mom[..., 2]], -1), np.stack([mom[..., 2], mom[..., 3]], -1)], -2)
    S = Q @ S @ Q.T
    return np.stack([mom[..., 0], S[..., 0, 0], 0.5 * (S[..., 0, 1] + S[..., 1, 0]), S[..., 1, 1]], axis=-1)


def rotate_cov(cov, Q):
    """(..., 3) = (Pxx, Pxy, Pyy) -> Q P Q^T in the same layout."""
    return rotate_moments(np.concatenate([cov[..., :1], cov], axis=-1), Q)[..., 1:]


def rotate_states(states, Q, floats=16):
    """(..., 16) tracker states, or (..., 32) two-model states, rotated by blockdiag(Q, Q): x -> B x, P -> B P B^T."""
    B = np.zeros((4, 4))
    B[:2, :2] = B[2:, 2:] = Q
    out = np.array(states, dtype=np.float64)
    for at in ((0,) if floats == 16 else (0, 14)):
        P = np.zeros(out.shape[:-1] + (4, 4))
        P[..., sr.IU[0], sr.IU[1]] = out[..., at + 4:at + 14]
        P[..., sr.IU[1], sr.IU[0]] = out[..., at + 4:at + 14]
        P = B @ P @ B.T
        out[..., at:at + 4] = out[..., at:at + 4] @ B.T
        out[..., at + 4:at + 14] = P[..., sr.IU[0], sr.IU[1]]
    return out
