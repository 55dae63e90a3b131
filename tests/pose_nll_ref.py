"""The rule of hupr_pose_track_nll_f32 (include/hupr.h) restated in NumPy — fp64 by default, any float type on request — and the
model-drawn record the fitting tests share.  Written here: the reference project has no tracker.  The recurrence is
pose_track_ref.ref_track's, frame for frame, in matrix form over all (candidate, row) cells at once; tests/test_pose_fit_cpu.py checks
the two against each other.  Imported by tests/test_pose_fit_cpu.py and tests/test_pose_fit_gpu.py; no GPU needed."""
import functools
import math

import numpy as np

import pose_track_ref as ref

MEAS_FLOATS = 8


def outlier_cost(extent):
    """2 ln(width height / 2 pi): a measurement as an outlier uniform over the image, in the units of d2 + ln det S."""
    return 2.0 * math.log(float(extent[0]) * float(extent[1]) / (2.0 * math.pi))


def record_of(raw, maxval, mom):
    """raw (T, rows, 2), maxval (T, rows), mom (T, rows, 4) = (m, Sxx, Sxy, Syy) -> the (T, rows, 8) float32 record."""
    T, rows = maxval.shape
    meas = np.zeros((T, rows, MEAS_FLOATS), np.float32)
    meas[..., 0:2], meas[..., 2], meas[..., 3:7] = raw, maxval, mom
    return meas


def ref_nll(meas, start, p, params, ratio, extent, dtype=np.float64):
    """meas (T, rows, 8) float32, start (T,) (non-zero: the tracks are zeroed in front of the frame), ``p`` the shared parameters (a
    PoseTracking: rate_hz, gate, max_coast, init_speed_std, min_score), params (G, 3) = (accel_psd, meas_std, heatmap_gain) -> dict:
    nll (G, rows) float64, the sum of min(d2 + ln det S, outlier cost) over the frames scored, every term computed in ``dtype`` and
    added in fp64 as the kernel does; counts (G, rows, 6); state (G, rows, 16); status (T, G, rows); kp (T, G, rows, 2); d2
    (T, G, rows), NaN where no gate was computed; near (G, rows), the smallest |d2 / gate - 1| of the cell's gate decisions."""
    f = dtype
    meas = np.asarray(meas)
    params = np.asarray(params, dtype=np.float64)
    T, rows = meas.shape[:2]
    G = params.shape[0]
    dt = f(1) / f(p.rate_hz)
    F = np.eye(4, dtype=f)
    F[0, 2] = F[1, 3] = dt
    q = params[:, 0].astype(f)
    Q = np.zeros((G, 1, 4, 4), dtype=f)
    Q[:, 0, 0, 0] = Q[:, 0, 1, 1] = q * dt * dt * dt / f(3)
    Q[:, 0, 0, 2] = Q[:, 0, 2, 0] = Q[:, 0, 1, 3] = Q[:, 0, 3, 1] = q * dt * dt / f(2)
    Q[:, 0, 2, 2] = Q[:, 0, 3, 3] = q * dt
    Hm = np.zeros((2, 4), dtype=f)
    Hm[0, 0] = Hm[1, 1] = 1
    I4, I2 = np.eye(4, dtype=f), np.eye(2, dtype=f)
    gain = (f(ratio) * f(ratio) * params[:, 2].astype(f))[:, None, None, None]
    floor2 = (params[:, 1].astype(f) * params[:, 1].astype(f))[:, None, None, None]
    cap, gate, speed2 = f(outlier_cost(extent)), f(p.gate), f(p.init_speed_std) * f(p.init_speed_std)
    x = np.zeros((G, rows, 4), dtype=f)
    P = np.zeros((G, rows, 4, 4), dtype=f)
    live = np.zeros((G, rows), bool)
    coast = np.zeros((G, rows), int)
    nll = np.zeros((G, rows), np.float64)
    counts = np.zeros((G, rows, 6), np.int32)
    near = np.full((G, rows), np.inf)
    out = dict(status=np.zeros((T, G, rows), np.int32), kp=np.zeros((T, G, rows, 2), f), d2=np.full((T, G, rows), np.nan))
    for t in range(T):
        if start[t]:
            x[:], P[:], live[:], coast[:] = 0, 0, False, 0
        z = meas[t, :, 0:2].astype(f)                                                   # (rows, 2)
        m, sxx, sxy, syy = (meas[t, :, k].astype(f) for k in (3, 4, 5, 6))
        Sw = np.stack([np.stack([sxx, sxy], -1), np.stack([sxy, syy], -1)], -2)          # (rows, 2, 2)
        with np.errstate(all="ignore"):
            R = gain * Sw[None] + floor2 * I2                                           # (G, rows, 2, 2)
            usable = ((meas[t, :, 2] > p.min_score) & np.isfinite(z).all(-1) & (m > 0))[None] & np.isfinite(R).all((-1, -2))
            was = live.copy()
            xm = x @ F.T
            Pm = F @ P @ F.T + Q
            nu = z[None] - xm[..., :2]
            S = Pm[..., :2, :2] + R
            det = S[..., 0, 0] * S[..., 1, 1] - S[..., 0, 1] * S[..., 0, 1]
            valid = was & usable & (det > 0) & np.isfinite(det)
            Si = np.stack([np.stack([S[..., 1, 1], -S[..., 0, 1]], -1), np.stack([-S[..., 0, 1], S[..., 0, 0]], -1)], -2) / det[..., None, None]
            d2 = np.einsum("gri,grij,grj->gr", nu, Si, nu)
            cost = np.minimum(d2 + np.log(det), cap)
            cost = np.where(np.isnan(cost), cap, cost)                                  # fminf returns the number
            K = Pm[..., :, :2] @ Si
            A = I4 - K @ Hm
            Pn = A @ Pm @ np.swapaxes(A, -1, -2) + K @ R @ np.swapaxes(K, -1, -2)
            Pn = f(0.5) * (Pn + np.swapaxes(Pn, -1, -2))
            xn = xm + np.einsum("grij,grj->gri", K, nu)
        nll += np.where(valid, cost.astype(np.float64), 0.0)
        counts[..., 5] += valid
        out["d2"][t] = np.where(valid, d2, np.nan)
        with np.errstate(all="ignore"):
            near = np.where(valid, np.minimum(near, np.abs(d2.astype(np.float64) / float(p.gate) - 1.0)), near)
        accepted = valid & (d2 <= gate)
        ends = was & ~accepted & (coast + 1 > p.max_coast)
        coasts = was & ~accepted & ~ends
        x = np.where(accepted[..., None], xn, np.where(coasts[..., None], xm, x))
        P = np.where(accepted[..., None, None], Pn, np.where(coasts[..., None, None], Pm, P))
        coast = np.where(accepted, 0, np.where(coasts, coast + 1, coast))
        code = np.where(accepted, ref.UPDATED, np.where(coasts, np.where(usable, ref.COASTED_GATED, ref.COASTED_MISSING), ref.LOST))
        live = was & ~ends
        begin = ~live & usable
        clear = ~live
        x = np.where(clear[..., None], f(0), x)
        P = np.where(clear[..., None, None], f(0), P)
        coast = np.where(clear, 0, coast)
        x0 = np.concatenate([np.broadcast_to(z[None], (G, rows, 2)), np.zeros((G, rows, 2), f)], -1)
        P0 = np.zeros((G, rows, 4, 4), f)
        P0[..., :2, :2] = np.where(np.isfinite(R), R, f(0))
        P0[..., 2, 2] = P0[..., 3, 3] = speed2
        x = np.where(begin[..., None], x0, x)
        P = np.where(begin[..., None, None], P0, P)
        code = np.where(begin, ref.STARTED, code)
        live = live | begin
        for c in range(5):
            counts[..., c] += code == c
        out["status"][t] = code
        out["kp"][t] = np.where(live[..., None], x[..., :2], z[None])
    iu = np.triu_indices(4)
    out["state"] = np.concatenate([x, P[..., iu[0], iu[1]], live[..., None].astype(f), coast[..., None].astype(f)], axis=-1)
    out.update(nll=nll, counts=counts, near=near)
    return out


# ---- the model-drawn record: tracks from the filter's own model ---------------------------------------------------------------------------
TRUE_Q, TRUE_STD, RATE, T, EXTENT, RATIO = 400.0, 2.5, 10.0, 48, (256.0, 256.0), 4.0
TRUE_INDEX = 40                                     # of model_grid(): the middle of the 9 x 9


@functools.lru_cache(maxsize=None)
def model_record(seed, rows=28, frames=T):
    """-> (meas (frames, rows, 8) float32, truth (frames, rows, 2)): white-acceleration tracks of power TRUE_Q pixel^2 / s^3 per axis,
    drawn exactly from the discrete model at RATE Hz (start uniform in the image's middle, speed N(0, 30 pixel / s)), observed with
    isotropic N(0, TRUE_STD pixel) noise.  Score 1, window mass 1 and a fixed isotropic window: with heatmap_gain = 0, R = meas_std^2 I."""
    rng = np.random.RandomState(seed)
    dt = 1.0 / RATE
    Lq = np.linalg.cholesky(TRUE_Q * np.array([[dt ** 3 / 3, dt ** 2 / 2], [dt ** 2 / 2, dt]]))
    pos = rng.uniform(70.0, 186.0, (rows, 2))
    vel = rng.normal(0.0, 30.0, (rows, 2))
    truth = np.zeros((frames, rows, 2))
    for t in range(frames):
        if t:
            w = rng.normal(0.0, 1.0, (rows, 2, 2)) @ Lq.T                               # per row and axis: (position, velocity) noise
            pos, vel = pos + dt * vel + w[..., 0], vel + w[..., 1]
        truth[t] = pos
    z = truth + rng.normal(0.0, TRUE_STD, truth.shape)
    mom = np.broadcast_to(np.array([1.0, 2.67, 0.0, 2.67]), (frames, rows, 4))
    meas = record_of(z, np.ones((frames, rows)), mom)
    meas.setflags(write=False)
    truth.setflags(write=False)
    return meas, truth


def model_grid():
    """The 9 x 9 candidates around the truth: accel_psd in factors of 2, meas_std in factors of sqrt 2, heatmap_gain 0; (81, 3),
    accel_psd the slow axis, so the truth is TRUE_INDEX."""
    q = TRUE_Q * 2.0 ** np.arange(-4, 5)
    s = TRUE_STD * 2.0 ** (0.5 * np.arange(-4, 5))
    return np.stack([np.repeat(q, 9), np.tile(s, 9), np.zeros(81)], axis=1)
