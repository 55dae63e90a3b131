"""The rule of hupr_pose_smooth_rts_f32 (include/hupr.h) restated in NumPy — fp64 by default, any float type on request — in matrix
form, on top of tests/pose_track_ref.py: the backward Rauch-Tung-Striebel pass over the states a tracker run left behind.  Written
here: the reference project has no tracker and no smoother.  Imported by tests/test_pose_smooth_cpu.py and
tests/test_pose_smooth_gpu.py; no GPU needed."""
import functools
import types

import numpy as np

import pose_track_ref as ref

SMOOTHED, END, PASSTHROUGH, DEGENERATE = range(4)
IU = np.triu_indices(4)
ACCEL_PSD = 200.0                  # the smoother tests' own tracker parameters: PoseTracking's default power, arg-max measurements
NORMAL = [r for r in range(ref.ROWS) if r not in (ref.DROP, ref.OUTLIER, ref.GONE, ref.NEVER)]
# NumPy fp32 vs fp64 runs of this restatement (tracker and smoother) on the scenario: largest difference of the smoothed positions (image
# pixels), velocities (pixels / s) and position covariances (cov_rel_diff).  tests/test_pose_smooth_cpu.py measures them again and holds
# them; tests/test_pose_smooth_gpu.py allows the kernel 16 x each.
POS_FP32, VEL_FP32, COV_REL_FP32 = 4.03e-5, 6.58e-5, 3.18e-6


def params(**kw):
    """The tracker parameters of the smoother tests without importing the package: PoseTracking's defaults, accel_psd 200, the
    scenario's rate and min_score."""
    d = dict(rate_hz=ref.RATE, accel_psd=ACCEL_PSD, meas_std=1.0, heatmap_gain=1.0, gate=13.816, max_coast=5, init_speed_std=50.0,
             min_score=ref.MIN_SCORE, horizon_s=0.0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def model(rate_hz, accel_psd, f):
    """-> (F, Q) of hupr_pose_track_f32 in the float type ``f``."""
    dt = f(1) / f(rate_hz)
    F = np.eye(4, dtype=f)
    F[0, 2] = F[1, 3] = dt
    q = f(accel_psd)
    Q = np.zeros((4, 4), dtype=f)
    Q[0, 0] = Q[1, 1] = q * dt * dt * dt / f(3)
    Q[0, 2] = Q[2, 0] = Q[1, 3] = Q[3, 1] = q * dt * dt / f(2)
    Q[2, 2] = Q[3, 3] = q * dt
    return F, Q


def unpack(states, f):
    """(..., 16) state entries -> (x (..., 4), P (..., 4, 4) symmetric) in the float type ``f``."""
    s = np.asarray(states).astype(f)
    P = np.zeros(s.shape[:-1] + (4, 4), dtype=f)
    P[..., IU[0], IU[1]] = s[..., 4:14]
    P[..., IU[1], IU[0]] = s[..., 4:14]
    return s[..., :4], P


def cholesky(A, f):
    """Lower factor of the 4 x 4 matrix A in the float type ``f``, column by column -> (L, ok); ok is False where a pivot is not
    positive and finite."""
    L = np.zeros((4, 4), dtype=f)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(4):
            d = A[j, j] - (L[j, :j] * L[j, :j]).sum(dtype=f)
            ok = ok and bool(d > 0 and np.isfinite(d))
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 4):
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum(dtype=f)) / L[j, j]
    return L, ok


def gain(P, F, L, f):
    """C = P F^T (L L^T)^-1: every row by a forward and a backward substitution."""
    A = P @ F.T
    C = np.zeros((4, 4), dtype=f)
    with np.errstate(all="ignore"):
        for i in range(4):
            y = np.zeros(4, dtype=f)
            for j in range(4):
                y[j] = (A[i, j] - (L[j, :j] * y[:j]).sum(dtype=f)) / L[j, j]
            for j in range(3, -1, -1):
                C[i, j] = (y[j] - (L[j + 1:, j] * C[i, j + 1:]).sum(dtype=f)) / L[j, j]
    return C


def ref_smooth(states, status, keypoints, rate_hz, accel_psd, dtype=np.float64):
    """The backward pass over states (T, rows, 16), status (T, rows) and the filtered keypoints (T, rows, 2) -> dict of kp (T, rows, 2),
    vel (T, rows, 2), cov (T, rows, 3) = (Pxx, Pxy, Pyy), flag (T, rows) int32, and the full x (T, rows, 4), P (T, rows, 4, 4).  All
    arithmetic in ``dtype``."""
    f = dtype
    T, rows = status.shape
    F, Q = model(rate_hz, accel_psd, f)
    x, P = unpack(states, f)
    xs, Ps = np.zeros((T, rows, 4), dtype=f), np.zeros((T, rows, 4, 4), dtype=f)
    flag = np.zeros((T, rows), dtype=np.int32)
    kp = np.zeros((T, rows, 2), dtype=f)
    for r in range(rows):
        for k in range(T - 1, -1, -1):
            if status[k, r] == ref.LOST:
                flag[k, r], kp[k, r] = PASSTHROUGH, keypoints[k, r]
                continue
            if k == T - 1 or status[k + 1, r] in (ref.STARTED, ref.LOST):
                flag[k, r], xs[k, r], Ps[k, r] = END, x[k, r], P[k, r]
            else:
                xp, Pp = F @ x[k, r], F @ P[k, r] @ F.T + Q
                L, ok = cholesky(Pp, f)
                with np.errstate(all="ignore"):
                    C = gain(P[k, r], F, L, f)
                    nx = x[k, r] + C @ (xs[k + 1, r] - xp)
                    nP = P[k, r] + C @ (Ps[k + 1, r] - Pp) @ C.T
                    nP = f(0.5) * (nP + nP.T)
                if ok and np.isfinite(nx).all() and np.isfinite(nP).all():
                    flag[k, r], xs[k, r], Ps[k, r] = SMOOTHED, nx, nP
                else:
                    flag[k, r], xs[k, r], Ps[k, r] = DEGENERATE, x[k, r], P[k, r]
            kp[k, r] = xs[k, r, :2]
    cov = np.stack([Ps[..., 0, 0], Ps[..., 0, 1], Ps[..., 1, 1]], axis=-1)
    return dict(kp=kp, vel=xs[..., 2:].copy(), cov=cov, flag=flag, x=xs, P=Ps)


def textbook_rts(x, P, F, Q):
    """Dense textbook RTS over one uninterrupted segment x (T, 4), P (T, 4, 4) in fp64 with np.linalg.inv -> (xs, Ps)."""
    T = x.shape[0]
    xs, Ps = x.astype(np.float64).copy(), P.astype(np.float64).copy()
    for k in range(T - 2, -1, -1):
        Pp = F @ P[k] @ F.T + Q
        C = P[k] @ F.T @ np.linalg.inv(Pp)
        xs[k] = x[k] + C @ (xs[k + 1] - F @ x[k])
        Ps[k] = P[k] + C @ (Ps[k + 1] - Pp) @ C.T
    return xs, Ps


def track_with_states(raw, maxval, mom, p, ratio, dtype=np.float64):
    """ref_track over the whole sequence, and its state after every frame: ref_track starts from the empty state and returns the state
    after its last frame only, so the state after frame k is that of a run over frames 0 .. k -> (ref_track's dict, states (T, rows,
    16))."""
    outs = [ref.ref_track(raw[:k + 1], maxval[:k + 1], mom[:k + 1], p, ratio, dtype) for k in range(maxval.shape[0])]
    return outs[-1], np.stack([o["state"] for o in outs])


def argmax_keypoints(idx, maxval, ratio=ref.RATIO, W=ref.HM):
    """The arg-max decode's raw keypoints in image pixels, (0, 0) where the maximum is not positive."""
    kp = np.stack([idx % W, idx // W], axis=-1).astype(np.float64) * ratio
    return kp * (maxval > 0)[..., None]


@functools.lru_cache(maxsize=None)
def scenario_run(dtype=np.float64, events=True):
    """The scenario of pose_track_ref through ref_track (arg-max measurements, ``params()``) and ref_smooth, all in ``dtype`` ->
    (track dict, states, smooth dict, raw keypoints)."""
    idx, mx, mom = ref.scenario_moments(events, dtype=dtype)
    raw = argmax_keypoints(idx, mx).astype(dtype)
    p = params()
    track, states = track_with_states(raw, mx, mom, p, ref.RATIO, dtype)
    smooth = ref_smooth(states, track["status"], track["kp"], p.rate_hz, p.accel_psd, dtype)
    return track, states, smooth, raw


def rms(a):
    """Root mean square over every frame, row and axis."""
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))


def second_difference(a):
    return a[2:] - 2.0 * a[1:-1] + a[:-2]
