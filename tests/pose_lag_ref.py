"""The rule of hupr_pose_smooth_lag_f32 (include/hupr.h) restated in NumPy on top of tests/pose_smooth_ref.py: the fixed-lag smoother
is the Rauch-Tung-Striebel backward pass cut short — after frame n it runs over the frames max(n - L, 0) .. n only.  Written here: the
reference project has no tracker and no smoother.  Imported by tests/test_pose_lag_cpu.py and tests/test_pose_lag_gpu.py; no GPU
needed."""
import functools

import numpy as np

import pose_smooth_ref as sr

EMPTY = 4
OUT = ("kp", "vel", "cov", "flag")
# NumPy fp32 vs fp64 runs of this restatement (tracker and fixed-lag smoother, L = 4) on the scenario: largest difference of the
# lagged positions (image pixels), velocities (pixels / s) and position covariances (cov_rel_diff).  tests/test_pose_lag_cpu.py
# measures them again and holds them; tests/test_pose_lag_gpu.py allows the kernel 16 x each.
POS_FP32, VEL_FP32, COV_REL_FP32 = 3.69e-5, 6.93e-5, 2.24e-6


def ref_lag(states, status, keypoints, rate_hz, accel_psd, L, dtype=np.float64):
    """The fixed-lag smoother over states (T, rows, 16), status (T, rows) and the filtered keypoints (T, rows, 2), in ``dtype`` ->
    (answers, tails).  ``answers``: dict of kp (T, rows, 2), vel (T, rows, 2), cov (T, rows, 3), flag (T, rows): frame k as
    ``ref_smooth(states[:n + 1], ...)[k]`` gives it with n = min(k + L, T - 1) — the backward pass from frame n never looks in front
    of frame k, so the pass over the window max(n - L, 0) .. n is run instead.  ``tails``: after every frame n the dict of
    (L + 1, rows, ...) arrays the launch of that frame writes: slot j = frame n - j, zeros and EMPTY where j > n."""
    T, rows = status.shape
    answers = {k: [None] * T for k in OUT}
    tails = []
    for n in range(T):
        lo = max(n - L, 0)
        o = sr.ref_smooth(states[lo:n + 1], status[lo:n + 1], keypoints[lo:n + 1], rate_hz, accel_psd, dtype)
        tail = {}
        for k in OUT:
            a = o[k][::-1]                                                      # newest frame first
            pad = np.zeros((L + 1 - a.shape[0],) + a.shape[1:], dtype=a.dtype)
            tail[k] = np.concatenate([a, pad + EMPTY if k == "flag" else pad])
        tails.append(tail)
        due = range(n - L, n - L + 1) if n < T - 1 else range(max(n - L, 0), T)  # the last launch settles every frame still owed
        for f in due:
            if f >= 0:
                for k in OUT:
                    answers[k][f] = o[k][f - lo]
    return {k: np.stack(v) for k, v in answers.items()}, tails


@functools.lru_cache(maxsize=None)
def scenario_lag(L, dtype=np.float64, rows=None):
    """``ref_lag`` over ``pose_smooth_ref.scenario_run(dtype)``'s tracker run (all of its rows, or the tuple ``rows``), all in
    ``dtype`` -> (answers, tails)."""
    track, states, _, _ = sr.scenario_run(dtype)
    sel = slice(None) if rows is None else list(rows)
    p = sr.params()
    return ref_lag(states[:, sel], track["status"][:, sel], track["kp"][:, sel], p.rate_hz, p.accel_psd, L, dtype)
