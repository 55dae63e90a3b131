"""The rule of hupr_pose_track_f32 (include/hupr.h) restated in NumPy — fp64 by default, any float type on request — and the moving-
joint scenario the tracker tests share.  Written here: the reference project has no tracker.  Imported by tests/test_pose_track_cpu.py
and tests/test_pose_track_gpu.py; no GPU needed."""
import functools

import numpy as np

UPDATED, COASTED_MISSING, COASTED_GATED, STARTED, LOST = range(5)
RADIUS = 3


def window_moments(h32, idx, dtype=np.float64):
    """h32 (rows, H, W) float32 maps, idx (rows,) arg-max positions -> (rows, 4): mass m and the second central moments Sxx, Sxy, Syy
    (heat-map pixels squared) of w = max(h, 0) over the radius-3 window around the peak, clipped to the map, in window-relative
    coordinates.  A NaN pixel weighs 0; a row whose maximum is not positive has m = 0 and NaN moments."""
    rows, H, W = h32.shape
    out = np.zeros((rows, 4), dtype=dtype)
    for r in range(rows):
        i = int(idx[r])
        if not 0 <= i < H * W or not h32[r].reshape(-1)[i] > 0:
            out[r, 1:] = np.nan
            continue
        px, py = i % W, i // W
        x0, x1, y0, y1 = max(px - RADIUS, 0), min(px + RADIUS, W - 1), max(py - RADIUS, 0), min(py + RADIUS, H - 1)
        w = h32[r, y0:y1 + 1, x0:x1 + 1].astype(dtype)
        w = np.where(np.isnan(w), dtype(0), np.maximum(w, dtype(0)))
        v, u = np.mgrid[y0 - py:y1 - py + 1, x0 - px:x1 - px + 1].astype(dtype)
        with np.errstate(all="ignore"):
            m = w.sum(dtype=dtype)
            cu, cv = (w * u).sum(dtype=dtype) / m, (w * v).sum(dtype=dtype) / m
            out[r] = (m, (w * (u - cu) ** 2).sum(dtype=dtype) / m, (w * (u - cu) * (v - cv)).sum(dtype=dtype) / m,
                      (w * (v - cv) ** 2).sum(dtype=dtype) / m)
    return out


def ref_track(raw, maxval, mom, p, ratio, dtype=np.float64):
    """The recurrence over raw (T, rows, 2) keypoints, (T, rows) maxima and (T, rows, 4) window moments with the parameters ``p`` (a
    PoseTracking) -> dict of (T, rows, ...) arrays: kp, vel, cov (Pxx, Pxy, Pyy), fc, status, d2 (NaN where no gate was computed),
    usable; and state, the (rows, 16) state after the last frame.  All arithmetic in ``dtype``, in matrix form."""
    f = dtype
    T, rows = maxval.shape
    dt = f(1) / f(p.rate_hz)
    F = np.eye(4, dtype=f)
    F[0, 2] = F[1, 3] = dt
    q = f(p.accel_psd)
    Q = np.zeros((4, 4), dtype=f)
    Q[0, 0] = Q[1, 1] = q * dt * dt * dt / f(3)
    Q[0, 2] = Q[2, 0] = Q[1, 3] = Q[3, 1] = q * dt * dt / f(2)
    Q[2, 2] = Q[3, 3] = q * dt
    Hm = np.zeros((2, 4), dtype=f)
    Hm[0, 0] = Hm[1, 1] = 1
    I4, I2 = np.eye(4, dtype=f), np.eye(2, dtype=f)
    gain, floor2 = f(ratio) * f(ratio) * f(p.heatmap_gain), f(p.meas_std) * f(p.meas_std)
    x = np.zeros((rows, 4), dtype=f)
    P = np.zeros((rows, 4, 4), dtype=f)
    live = np.zeros(rows, bool)
    coast = np.zeros(rows, int)
    out = dict(kp=np.zeros((T, rows, 2), f), vel=np.zeros((T, rows, 2), f), cov=np.zeros((T, rows, 3), f), fc=np.zeros((T, rows, 2), f),
               status=np.zeros((T, rows), np.int32), d2=np.full((T, rows), np.nan), usable=np.zeros((T, rows), bool))
    for t in range(T):
        for r in range(rows):
            z = raw[t, r].astype(f)
            m, sxx, sxy, syy = (f(v) for v in mom[t, r])
            with np.errstate(all="ignore"):
                R = gain * np.array([[sxx, sxy], [sxy, syy]], dtype=f) + floor2 * I2
            usable = bool(maxval[t, r] > p.min_score and np.isfinite(z).all() and m > 0 and np.isfinite(R).all())
            out["usable"][t, r] = usable
            code = LOST
            if live[r]:
                xm, Pm = F @ x[r], F @ P[r] @ F.T + Q
                accepted = False
                if usable:
                    nu = z - Hm @ xm
                    S = Hm @ Pm @ Hm.T + R
                    det = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
                    if det > 0 and np.isfinite(det):
                        Si = np.array([[S[1, 1], -S[0, 1]], [-S[0, 1], S[0, 0]]], dtype=f) / det
                        d2 = nu @ Si @ nu
                        out["d2"][t, r] = d2
                        accepted = bool(d2 <= f(p.gate))
                if accepted:
                    K = Pm @ Hm.T @ Si
                    A = I4 - K @ Hm
                    Pn = A @ Pm @ A.T + K @ R @ K.T
                    x[r], P[r], coast[r], code = xm + K @ nu, f(0.5) * (Pn + Pn.T), 0, UPDATED
                elif coast[r] + 1 > p.max_coast:
                    live[r] = False
                else:
                    x[r], P[r], code = xm, Pm, COASTED_GATED if usable else COASTED_MISSING
                    coast[r] += 1
            if not live[r]:
                x[r], P[r], coast[r] = 0, 0, 0
                if usable:
                    x[r, :2] = z
                    P[r, :2, :2] = R
                    P[r, 2, 2] = P[r, 3, 3] = f(p.init_speed_std) * f(p.init_speed_std)
                    live[r], code = True, STARTED
            kp = x[r, :2] if live[r] else z
            out["kp"][t, r], out["vel"][t, r], out["cov"][t, r] = kp, x[r, 2:], (P[r, 0, 0], P[r, 0, 1], P[r, 1, 1])
            out["fc"][t, r] = kp + x[r, 2:] * f(p.horizon_s)
            out["status"][t, r] = code
    iu = np.triu_indices(4)
    out["state"] = np.concatenate([x, P[:, iu[0], iu[1]], live[:, None].astype(f), coast[:, None].astype(f)], axis=1)
    return out


# ---- the scenario: 60 frames x 28 joints at 10 Hz ------------------------------------------------------------------------------------------
T, ROWS, RATE, HM, RATIO = 60, 28, 10.0, 64, 4.0
SEED = 11
AMPLITUDE, FAINT, MIN_SCORE = 0.8, 0.05, 0.1
DROP, DROP_FRAMES = 4, (20, 21, 22)                # its score falls under MIN_SCORE for three frames
OUTLIER, OUTLIER_FRAME, OUTLIER_BY = 9, 30, (60.0, -45.0)
GONE, GONE_FRAMES = 15, tuple(range(25, 35))       # missing for ten frames
NEVER = 22                                         # never above MIN_SCORE


def gaussian_maps(centres, amplitude, sigma=2.0, H=HM, W=HM):
    """centres (rows, 2) (x, y) in heat-map pixels, amplitude (rows,) -> (rows, H, W) float32."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = (xx[None] - centres[:, 0, None, None]) ** 2 + (yy[None] - centres[:, 1, None, None]) ** 2
    return (amplitude[:, None, None] * np.exp(-r2 / (2.0 * sigma ** 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scenario(events=True, seed=SEED):
    """-> (maps (T, ROWS, 64, 64) float32, truth (T, ROWS, 2), measured (T, ROWS, 2)) in image pixels.  Tracks centre + amp sin(w t +
    phase) per axis, amp in [10, 40] image pixels, w in [0.3, 1.0] rad / s; every frame's map is a Gaussian of sigma 2 heat-map pixels
    and amplitude 0.8 at the track position plus N(0, 3 pixel) noise.  ``events``: the drop-out, outlier, gone and never-seen rows."""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(70.0, 186.0, (ROWS, 2))
    amp, w, ph = rng.uniform(10.0, 40.0, (ROWS, 2)), rng.uniform(0.3, 1.0, (ROWS, 2)), rng.uniform(0.0, 2 * np.pi, (ROWS, 2))
    t = np.arange(T)[:, None, None] / RATE
    truth = centre[None] + amp[None] * np.sin(w[None] * t + ph[None])
    measured = truth + rng.normal(0.0, 3.0, truth.shape)
    A = np.full((T, ROWS), AMPLITUDE)
    if events:
        measured[OUTLIER_FRAME, OUTLIER] += OUTLIER_BY
        A[list(DROP_FRAMES), DROP] = FAINT
        A[list(GONE_FRAMES), GONE] = FAINT
        A[:, NEVER] = FAINT
    maps = np.stack([gaussian_maps(measured[k] / RATIO, A[k]) for k in range(T)])
    for a in (maps, truth, measured):
        a.setflags(write=False)
    return maps, truth, measured


@functools.lru_cache(maxsize=None)
def scenario_moments(events=True, seed=SEED, dtype=np.float64):
    """-> (idx (T, ROWS), maxval (T, ROWS) float32, moments (T, ROWS, 4)) of the scenario's maps: np.argmax, first maximum wins."""
    maps = scenario(events, seed)[0]
    flat = maps.reshape(T, ROWS, -1)
    idx = flat.argmax(axis=2)
    mx = np.take_along_axis(flat, idx[..., None], axis=2)[..., 0]
    return idx, mx, np.stack([window_moments(maps[k], idx[k], dtype) for k in range(T)])


def cov_rel_diff(cov, cov64):
    """Largest difference of a (..., 3) covariance from the fp64 one, relative to the fp64 one's larger variance, over the entries
    where the fp64 one is not zero."""
    scale = np.maximum(cov64[..., 0], cov64[..., 2])
    keep = scale > 0
    return float((np.abs(cov.astype(np.float64) - cov64).max(axis=-1)[keep] / scale[keep]).max())
