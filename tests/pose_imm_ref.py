"""The rule of hupr_pose_track_imm_f32 (include/hupr.h) restated in NumPy matrix form — fp64 by default, any float type on request —
and the stop-and-go scenario its tests share: joints that rest, reach along a minimum-jerk path and rest again.  Written here: the
reference project has no tracker.  The window moments, the Gaussian maps and the status codes are tests/pose_track_ref.py's.
Imported by tests/test_pose_imm_cpu.py, tests/test_pose_imm_gpu.py and tests/test_stream_imm_gpu.py; no GPU needed."""
import functools

import numpy as np

from pose_track_ref import COASTED_GATED, COASTED_MISSING, LOST, STARTED, UPDATED, gaussian_maps, window_moments

FLOATS = 32                                        # per row: model 0's 4 + 10, model 1's 4 + 10, mu0, mu1, live, coast


def ref_imm(raw, maxval, mom, p, ratio, dtype=np.float64, present=None):
    """The recurrence over raw (T, rows, 2) keypoints, (T, rows) maxima and (T, rows, 4) window moments with the parameters ``p`` (a
    PoseTracking with ``accel_psd_moving``) -> dict of (T, rows, ...) arrays: kp, vel, cov (Pxx, Pxy, Pyy), fc, status, moving, d2
    (the decisive one: the smallest valid d2 among the models with c_j > 0, NaN where there is none), usable; and state, the
    (rows, 32) state after the last frame.  ``present`` (T, rows) bool or None: a row flagged absent has no measurement.  All
    arithmetic in ``dtype``."""
    f = dtype
    T, rows = maxval.shape
    dt = f(1) / f(p.rate_hz)
    F = np.eye(4, dtype=f)
    F[0, 2] = F[1, 3] = dt
    Q = []
    for q in (f(p.accel_psd), f(p.accel_psd_moving)):
        Qj = np.zeros((4, 4), dtype=f)
        Qj[0, 0] = Qj[1, 1] = q * dt * dt * dt / f(3)
        Qj[0, 2] = Qj[2, 0] = Qj[1, 3] = Qj[3, 1] = q * dt * dt / f(2)
        Qj[2, 2] = Qj[3, 3] = q * dt
        Q.append(Qj)
    Hm = np.zeros((2, 4), dtype=f)
    Hm[0, 0] = Hm[1, 1] = 1
    I4, I2 = np.eye(4, dtype=f), np.eye(2, dtype=f)
    gain, floor2 = f(ratio) * f(ratio) * f(p.heatmap_gain), f(p.meas_std) * f(p.meas_std)
    sp = f(p.switch_prob)
    pi = np.array([[f(1) - sp, sp], [sp, f(1) - sp]], dtype=f)
    prior = np.array([f(1) - f(p.moving_prior), f(p.moving_prior)], dtype=f)
    x = np.zeros((rows, 2, 4), dtype=f)
    P = np.zeros((rows, 2, 4, 4), dtype=f)
    mu = np.zeros((rows, 2), dtype=f)
    live = np.zeros(rows, bool)
    coast = np.zeros(rows, int)
    out = dict(kp=np.zeros((T, rows, 2), f), vel=np.zeros((T, rows, 2), f), cov=np.zeros((T, rows, 3), f), fc=np.zeros((T, rows, 2), f),
               status=np.zeros((T, rows), np.int32), moving=np.zeros((T, rows), f), d2=np.full((T, rows), np.nan),
               usable=np.zeros((T, rows), bool))
    for t in range(T):
        for r in range(rows):
            z = raw[t, r].astype(f)
            m, sxx, sxy, syy = (f(v) for v in mom[t, r])
            with np.errstate(all="ignore"):
                R = gain * np.array([[sxx, sxy], [sxy, syy]], dtype=f) + floor2 * I2
            usable = bool(maxval[t, r] > p.min_score and np.isfinite(z).all() and m > 0 and np.isfinite(R).all())
            usable = usable and (present is None or bool(present[t, r]))
            out["usable"][t, r] = usable
            code = LOST
            if live[r]:
                # 1. mixing
                c = mu[r].copy()
                xs, Ps = x[r].copy(), P[r].copy()
                if p.switch_prob != 0:
                    c = pi.T @ mu[r]
                    for j in range(2):
                        w = pi[:, j] * mu[r] / c[j]
                        xs[j] = w[0] * x[r, 0] + w[1] * x[r, 1]
                        d = x[r] - xs[j]
                        Ps[j] = sum(w[i] * (P[r, i] + np.outer(d[i], d[i])) for i in range(2))
                # 2. predict, 3. gate
                valid, d2, ldet, nu, Si = [False, False], [f(0), f(0)], [f(0), f(0)], [None, None], [None, None]
                for j in range(2):
                    xs[j], Ps[j] = F @ xs[j], F @ Ps[j] @ F.T + Q[j]
                    if usable:
                        nu[j] = z - Hm @ xs[j]
                        S = Hm @ Ps[j] @ Hm.T + R
                        det = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
                        if det > 0 and np.isfinite(det):
                            Si[j] = np.array([[S[1, 1], -S[0, 1]], [-S[0, 1], S[0, 0]]], dtype=f) / det
                            valid[j], d2[j], ldet[j] = True, nu[j] @ Si[j] @ nu[j], np.log(det)
                say = [j for j in range(2) if valid[j] and c[j] > 0]
                if say:
                    out["d2"][t, r] = min(d2[j] for j in say)
                if any(d2[j] <= f(p.gate) for j in say):
                    # 4. accepted
                    for j in range(2):
                        if valid[j]:
                            K = Ps[j] @ Hm.T @ Si[j]
                            A = I4 - K @ Hm
                            Pn = A @ Ps[j] @ A.T + K @ R @ K.T
                            xs[j], Ps[j] = xs[j] + K @ nu[j], f(0.5) * (Pn + Pn.T)
                    l = [d2[j] + ldet[j] for j in range(2)]
                    lo = min(l[j] for j in say)
                    w = np.array([c[j] * np.exp(-(l[j] - lo) / f(2)) if j in say else f(0) for j in range(2)], dtype=f)
                    x[r], P[r], mu[r], coast[r], code = xs, Ps, w / (w[0] + w[1]), 0, UPDATED
                elif coast[r] + 1 > p.max_coast:
                    live[r] = False
                else:
                    # 5. not accepted
                    x[r], P[r], mu[r], code = xs, Ps, c, COASTED_GATED if usable else COASTED_MISSING
                    coast[r] += 1
            if not live[r]:
                x[r], P[r], mu[r], coast[r] = 0, 0, 0, 0
                if usable:
                    x[r, :, :2] = z
                    P[r, :, :2, :2] = R
                    P[r, :, 2, 2] = P[r, :, 3, 3] = f(p.init_speed_std) * f(p.init_speed_std)
                    mu[r] = prior
                    live[r], code = True, STARTED
            # 7. the moment-matched mixture
            xm = x[r, 0] + mu[r, 1] * (x[r, 1] - x[r, 0])
            d = x[r] - xm
            Pm = sum(mu[r, j] * (P[r, j] + np.outer(d[j], d[j])) for j in range(2))
            kp = xm[:2] if live[r] else z
            out["kp"][t, r], out["vel"][t, r], out["cov"][t, r] = kp, xm[2:], (Pm[0, 0], Pm[0, 1], Pm[1, 1])
            out["fc"][t, r] = kp + xm[2:] * f(p.horizon_s)
            out["status"][t, r], out["moving"][t, r] = code, mu[r, 1]
    iu = np.triu_indices(4)
    out["state"] = np.concatenate([x[:, 0], P[:, 0][:, iu[0], iu[1]], x[:, 1], P[:, 1][:, iu[0], iu[1]], mu, live[:, None].astype(f),
                                   coast[:, None].astype(f)], axis=1)
    return out


# ---- the scenario: 120 frames x 28 joints at 10 Hz that stop and go ---------------------------------------------------------------------
T, ROWS, RATE, HM, RATIO = 120, 28, 10.0, 64, 4.0
SEED = 3
AMPLITUDE, FAINT, MIN_SCORE, NOISE = 0.8, 0.05, 0.1, 3.0
DROP, DROP_FRAMES = 4, (40, 41, 42)                # its score falls under MIN_SCORE for three frames
OUTLIER, OUTLIER_FRAME, OUTLIER_BY = 9, 50, (60.0, 45.0)      # towards the middle of the image, so the peak stays on the map
GONE, GONE_FRAMES = 15, tuple(range(60, 70))       # missing for ten frames
NEVER = 22                                         # never above MIN_SCORE
EVENT_ROWS = (DROP, OUTLIER, GONE, NEVER)
NORMAL = tuple(r for r in range(ROWS) if r not in EVENT_ROWS)


@functools.lru_cache(maxsize=None)
def stop_and_go(seed=SEED, events=True):
    """-> (maps (T, ROWS, 64, 64) float32, truth (T, ROWS, 2), measured (T, ROWS, 2), moving (T, ROWS) bool) in image pixels.  Every
    row starts uniform in [70, 186]^2 and alternates 10 to 30 still frames with a minimum-jerk reach (10 s^3 - 15 s^4 + 6 s^5) of 15 to
    50 pixels over 8 to 15 frames in a uniform direction, its target clipped to [20, 236]; ``moving`` marks the frames of a reach.
    Every frame's map is a Gaussian of sigma 2 heat-map pixels and amplitude 0.8 at truth + N(0, 3 pixel).  ``events``: the drop-out,
    outlier, gone and never-seen rows."""
    rng = np.random.RandomState(seed)
    truth = np.zeros((T, ROWS, 2))
    moving = np.zeros((T, ROWS), bool)
    start = rng.uniform(70.0, 186.0, (ROWS, 2))
    for r in range(ROWS):
        at, t = start[r], 0
        while t < T:
            n = rng.randint(10, 31)
            truth[t:t + n, r] = at
            t += n
            if t >= T:
                break
            reach, n, angle = rng.uniform(15.0, 50.0), rng.randint(8, 16), rng.uniform(0.0, 2 * np.pi)
            target = np.clip(at + reach * np.array([np.cos(angle), np.sin(angle)]), 20.0, 236.0)
            for k in range(1, n + 1):
                if t < T:
                    s = k / n
                    truth[t, r] = at + (10 * s ** 3 - 15 * s ** 4 + 6 * s ** 5) * (target - at)
                    moving[t, r] = True
                    t += 1
            at = target
    measured = truth + rng.normal(0.0, NOISE, truth.shape)
    A = np.full((T, ROWS), AMPLITUDE)
    if events:
        measured[OUTLIER_FRAME, OUTLIER] += np.sign(128.0 - truth[OUTLIER_FRAME, OUTLIER]) * OUTLIER_BY
        A[list(DROP_FRAMES), DROP] = FAINT
        A[list(GONE_FRAMES), GONE] = FAINT
        A[:, NEVER] = FAINT
    maps = np.stack([gaussian_maps(measured[k] / RATIO, A[k]) for k in range(T)])
    for a in (maps, truth, measured, moving):
        a.setflags(write=False)
    return maps, truth, measured, moving


@functools.lru_cache(maxsize=None)
def stop_and_go_moments(seed=SEED, events=True, dtype=np.float64):
    """-> (idx (T, ROWS), maxval (T, ROWS) float32, moments (T, ROWS, 4)) of the scenario's maps: np.argmax, first maximum wins."""
    maps = stop_and_go(seed, events)[0]
    flat = maps.reshape(T, ROWS, -1)
    idx = flat.argmax(axis=2)
    mx = np.take_along_axis(flat, idx[..., None], axis=2)[..., 0]
    return idx, mx, np.stack([window_moments(maps[k], idx[k], dtype) for k in range(T)])


def rel_gate_margin(d2, gate):
    """The smallest |d2 / gate - 1| over the finite entries of ``d2``: how close the closest decision came to the gate."""
    d = d2[np.isfinite(d2)]
    return float(np.abs(d / gate - 1.0).min())
