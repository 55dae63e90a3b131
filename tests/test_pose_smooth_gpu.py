"""GPU (-m gpu): hupr_pose_smooth_rts_f32 (csrc/pose_smooth.hip) — the Rauch-Tung-Striebel backward pass over a recorded run of the
Kalman tracker — against the NumPy statement of the rule in tests/pose_smooth_ref.py.

The history.  The scenario of tests/pose_track_ref.py (60 frames x 28 rows of 64 x 64 maps at 10 Hz, seed 11, with its drop-out,
outlier, gone and never-seen rows) goes through functional.pose_track frame by frame (PoseTracking's defaults, accel_psd = 200,
min_score = 0.1, arg-max measurements), the state tensor copied after every launch.  The fp64 rule is fed that same fp32 history, so
only the backward pass is measured.  Wider row counts take further seeds of the same scenario beside it.

Bounds.  Flags: equal.  Smoothed position, velocity and position covariance (relative to the larger fp64 variance, cov_rel_diff):
16 x the differences of the NumPy fp32 run of the restatement from its fp64 run (pose_smooth_ref.POS_FP32 = 4.03e-5 pixel, VEL_FP32
= 6.58e-5 pixel / s, COV_REL_FP32 = 3.18e-6; tests/test_pose_smooth_cpu.py measures them), i.e. 6.4e-4 pixel, 1.05e-3 pixel / s and
5.1e-5: the kernel contracts to FMAs and may order sums differently from NumPy — the margin tests/test_pose_track_gpu.py gives its
covariance for the same reason.  The test prints what the GPU shows.  END and PASSTHROUGH frames, run-to-run, row permutation,
batching and the sequence split: bit equality.

Degenerate input.  P_k = 0 inside a live segment makes the predicted covariance Pp = Q: with accel_psd = 0 that is the zero matrix,
the first pivot is not positive and the frame is DEGENERATE; with accel_psd > 0 Q is positive definite, the gain is 0 and the rule
keeps the frame as SMOOTHED with the filter's values.  Both are checked, against the fp64 rule's flags."""
import functools

import numpy as np
import pytest
import torch

import pose_smooth_ref as sr
import pose_track_ref as ref

pytestmark = pytest.mark.gpu
TOL_POS, TOL_VEL, TOL_COV_REL = 16 * sr.POS_FP32, 16 * sr.VEL_FP32, 16 * sr.COV_REL_FP32
SEEDS = (ref.SEED, 12, 13)
OUT = ("kp", "vel", "cov", "flag")


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(dict(accel_psd=sr.ACCEL_PSD, min_score=ref.MIN_SCORE), **kw))


@functools.lru_cache(maxsize=None)
def history(seed=ref.SEED, accel_psd=sr.ACCEL_PSD, zero_at=None):
    """The scenario of ``seed`` through functional.pose_track frame by frame from a fresh state, the state zeroed in front of frame
    ``zero_at`` -> dict of (T, ROWS, ...) device tensors: states, status, kp (the filtered keypoints)."""
    from hupr_amd import functional as F_
    heat = torch.from_numpy(np.array(ref.scenario(True, seed)[0])).cuda()
    p, state = tracking(accel_psd=accel_psd), F_.pose_track_state(ref.ROWS, "cuda")
    states, status, kp = [], [], []
    for t in range(ref.T):
        if t == zero_at:
            state.zero_()
        o = F_.pose_track(heat[t], ref.RATIO, refine=False, track_state=state, tracking=p)
        states.append(state.clone())
        status.append(o[7])
        kp.append(o[3])
    return dict(states=torch.stack(states), status=torch.stack(status), kp=torch.stack(kp))


def wide(rows):
    """A history of ``rows`` <= 84 rows: the scenarios of SEEDS side by side."""
    hs = [history(s) for s in SEEDS[:(rows + ref.ROWS - 1) // ref.ROWS]]
    return {k: torch.cat([h[k] for h in hs], dim=1)[:, :rows].contiguous() for k in hs[0]}


def smooth(h, p=None):
    from hupr_amd import functional as F_
    return dict(zip(OUT, F_.pose_smooth_rts(h["states"], h["status"], h["kp"], p or tracking())))


def fp64(h, accel_psd=sr.ACCEL_PSD):
    return sr.ref_smooth(h["states"].cpu().numpy(), h["status"].cpu().numpy(), h["kp"].cpu().numpy(), ref.RATE, accel_psd)


def same(a, b, what):
    for k in OUT:
        assert torch.equal(a[k], b[k]), (what, k)


def compare(o, o64, what, bounds=True):
    """Flags equal, values within the bounds (they are the scenario's: ``bounds`` False where the history is another); prints what the
    GPU shows."""
    assert o["flag"].dtype == torch.int32
    flag = o["flag"].cpu().numpy()
    assert np.array_equal(flag, o64["flag"]), what
    e_kp = np.abs(o["kp"].cpu().numpy() - o64["kp"]).max()
    e_vel = np.abs(o["vel"].cpu().numpy() - o64["vel"]).max()
    e_cov = ref.cov_rel_diff(o["cov"].cpu().numpy(), o64["cov"]) if (o64["cov"][..., [0, 2]] > 0).any() else 0.0
    print("%s: max |smoothed - fp64| %.3e px (bound %.3e), |velocity - fp64| %.3e px/s (bound %.3e), covariance relative %.3e "
          "(bound %.3e); flags %s" % (what, e_kp, TOL_POS, e_vel, TOL_VEL, e_cov, TOL_COV_REL, np.bincount(flag.ravel(), minlength=4).tolist()))
    assert not bounds or (e_kp <= TOL_POS and e_vel <= TOL_VEL and e_cov <= TOL_COV_REL), what
    return flag


# ---- 1: against the fp64 rule ---------------------------------------------------------------------------------------------------------------
def test_the_backward_pass_follows_the_fp64_rule():
    h = history()
    o, o64 = smooth(h), fp64(h)
    flag = compare(o, o64, "scenario, %d frames x %d rows" % (ref.T, ref.ROWS))
    status = h["status"].cpu().numpy()
    # the history is the one the rule's tests describe
    want = [sr.SMOOTHED] * 29 + [sr.END] + [sr.PASSTHROUGH] * 5 + [sr.SMOOTHED] * 24 + [sr.END]
    assert flag[:, ref.GONE].tolist() == want and (flag[:, ref.NEVER] == sr.PASSTHROUGH).all()
    assert (status[list(ref.DROP_FRAMES), ref.DROP] == ref.COASTED_MISSING).all() and status[ref.OUTLIER_FRAME, ref.OUTLIER] == ref.COASTED_GATED
    # a real test: the smoother moves the keypoints, towards the truth, and tightens the coasted frames
    _, truth, _ = ref.scenario()
    kp, sm = h["kp"].cpu().numpy().astype(np.float64), o["kp"].cpu().numpy().astype(np.float64)
    e_f, e_s = sr.rms((kp - truth)[:, sr.NORMAL]), sr.rms((sm - truth)[:, sr.NORMAL])
    print("rms error on the %d normal rows: filter %.3f px, smoother %.3f px (ratio %.2f)" % (len(sr.NORMAL), e_f, e_s, e_s / e_f))
    assert np.abs(sm - kp)[:, sr.NORMAL].max() > 1.0 and e_s / e_f < 0.6
    cov_f = h["states"][:, :, 4].cpu().numpy()
    for t in ref.DROP_FRAMES:
        assert o["cov"][t, ref.DROP, 0].item() < 0.5 * cov_f[t, ref.DROP]


@pytest.mark.parametrize("T", [1, 2, 60])
@pytest.mark.parametrize("rows", [1, 28, 65])
def test_shapes(rows, T):
    """rows = 65 crosses a workgroup of 64; T = 1 is END / PASSTHROUGH only; the short slices start at frame 30, where the gone row is
    LOST.  Row 0 of the single-row case is the gone row, so that every flag occurs there too."""
    h = wide(max(rows, ref.ROWS))
    if rows == 1:
        h = {k: v[:, ref.GONE:ref.GONE + 1] for k, v in h.items()}
    first = 0 if T == ref.T else 30
    h = {k: v[first:first + T, :rows].contiguous() for k, v in h.items()}
    o = smooth(h)
    assert o["kp"].shape == (T, rows, 2) and o["vel"].shape == (T, rows, 2) and o["cov"].shape == (T, rows, 3) and o["flag"].shape == (T, rows)
    flag = compare(o, fp64(h), "rows %d, T %d" % (rows, T))
    if T == 1:
        assert np.isin(flag, (sr.END, sr.PASSTHROUGH)).all()
    if rows == 65:
        assert (flag[:, 64] != sr.PASSTHROUGH).any()                            # the row beyond the first workgroup is a live one


# ---- 2: bit equality -------------------------------------------------------------------------------------------------------------------------
def test_end_and_passthrough_frames_are_the_filters_bits():
    h = history()
    o = smooth(h)
    end, lost = o["flag"] == sr.END, o["flag"] == sr.PASSTHROUGH
    assert end.sum().item() >= ref.ROWS - 1 and lost.sum().item() == ref.T + 5
    assert torch.equal(lost, h["status"] == ref.LOST)
    st = h["states"]
    assert torch.equal(o["kp"][end], st[..., 0:2][end]) and torch.equal(o["vel"][end], st[..., 2:4][end])
    assert torch.equal(o["cov"][end], st[..., [4, 5, 8]][end])                   # P00, P01, P11 of the upper triangle
    assert torch.equal(o["kp"][end], h["kp"][end])
    assert torch.equal(o["kp"][lost], h["kp"][lost]) and h["kp"][lost].any().item()
    assert not o["vel"][lost].any().item() and not o["cov"][lost].any().item()


# ---- 3: determinism and row independence ----------------------------------------------------------------------------------------------------
def test_runs_are_identical_and_rows_are_independent():
    h = wide(65)
    a, b = smooth(h), smooth(h)
    same(a, b, "two runs")
    perm = torch.from_numpy(np.random.RandomState(4).permutation(65)).cuda()
    c = smooth({k: v[:, perm].contiguous() for k, v in h.items()})
    for k in OUT:
        assert torch.equal(c[k], a[k][:, perm]), ("row permutation", k)
    # two sequences batched along rows = the two launches
    h0, h1 = history(SEEDS[0]), history(SEEDS[1])
    both = smooth({k: torch.cat([h0[k], h1[k]], dim=1) for k in h0})
    o0, o1 = smooth(h0), smooth(h1)
    assert not torch.equal(o0["kp"], o1["kp"])
    for k in OUT:
        assert torch.equal(both[k][:, :ref.ROWS], o0[k]) and torch.equal(both[k][:, ref.ROWS:], o1[k]), ("batched", k)


def test_a_zeroed_state_splits_the_sequence():
    """The state zeroed in front of frame 30 (a second recording appended to the first): no frame before 30 is influenced by anything
    after it — the first 30 frames are those of a T = 30 launch, bit for bit."""
    h = history(zero_at=30)
    status = h["status"].cpu().numpy()
    assert np.isin(status[30], (ref.STARTED, ref.LOST)).all() and (status[30] == ref.STARTED).sum() == ref.ROWS - 2
    assert (status[29, sr.NORMAL] == ref.UPDATED).all()
    whole = smooth(h)
    head = smooth({k: v[:30].contiguous() for k, v in h.items()})
    for k in OUT:
        assert torch.equal(whole[k][:30], head[k]), k
    live = torch.from_numpy(status[29] != ref.LOST).cuda()
    assert torch.equal(whole["flag"][29][live], torch.full((int(live.sum()),), sr.END, dtype=torch.int32, device="cuda"))
    # and without the split frame 29 does see frame 30
    joined = smooth(history())
    assert (joined["flag"][29, sr.NORMAL] == sr.SMOOTHED).all().item()
    assert not torch.equal(joined["kp"][:30, sr.NORMAL], head["kp"][:, sr.NORMAL])


# ---- 4: degenerate input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel_psd,want", [(0.0, sr.DEGENERATE), (sr.ACCEL_PSD, sr.SMOOTHED)], ids=["no process noise", "accel_psd 200"])
def test_a_zero_covariance_inside_a_live_segment(accel_psd, want):
    h = {k: v.clone() for k, v in history(accel_psd=accel_psd).items()}
    r = sr.NORMAL[0]
    updated = (h["status"][:, r] == ref.UPDATED).cpu().numpy()
    k = next(t for t in range(5, ref.T - 1) if updated[t] and updated[t + 1])      # inside a live segment, a live successor
    h["states"][k, r, 4:14] = 0.0
    p = tracking(accel_psd=accel_psd)
    o = smooth(h, p)
    flag = compare(o, fp64(h, accel_psd), "P = 0 at frame %d of row %d, accel_psd %g" % (k, r, accel_psd), bounds=False)
    assert flag[k, r] == want
    assert np.argwhere(flag == sr.DEGENERATE).tolist() == ([[k, r]] if want == sr.DEGENERATE else [])
    assert torch.equal(o["kp"][k, r], h["states"][k, r, 0:2]) and torch.equal(o["vel"][k, r], h["states"][k, r, 2:4])
    assert not o["cov"][k, r].any().item()
    for key in ("kp", "vel", "cov"):
        assert torch.isfinite(o[key]).all().item(), key


# ---- 5: argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_minus_one_and_launch_nothing():
    from hupr_amd import runtime as rt
    L = rt.lib()
    T, rows = 4, 3
    st = torch.zeros((T, rows, 16), device="cuda")
    status = torch.zeros((T, rows), dtype=torch.int32, device="cuda")
    kp, sm, vel = (torch.zeros((T, rows, 2), device="cuda") for _ in range(3))
    cov = torch.zeros((T, rows, 3), device="cuda")
    flag = torch.full((T, rows), -7, dtype=torch.int32, device="cuda")
    good = [rt.ptr(st), rt.ptr(status), rt.ptr(kp), T, rows, 10.0, 200.0, rt.ptr(sm), rt.ptr(vel), rt.ptr(cov), rt.ptr(flag)]

    def call(**change):
        a = list(good)
        for i, v in change.items():
            a[int(i[1:])] = v
        return L.hupr_pose_smooth_rts_f32(*a, rt.stream())

    c0 = L.hupr_launch_count()
    for i in (0, 1, 2, 7, 8, 9, 10):
        assert call(**{"a%d" % i: None}) == -1, "null pointer %d" % i
    assert call(a3=0) == -1 and call(a3=-1) == -1                               # T < 1
    assert call(a4=-1) == -1                                                    # rows < 0
    assert call(a3=0, a4=0) == -1
    assert call(a3=1 << 16, a4=1 << 15) == -1 and call(a3=1 << 40, a4=1 << 40) == -1    # T * rows beyond 2^31
    assert call(a0=rt.ptr(st) + 4) == -1                                        # misaligned states
    for bad in (0.0, -10.0, float("inf"), float("nan")):
        assert call(a5=bad) == -1, "rate_hz %r" % bad
    for bad in (-1.0, float("inf"), float("nan")):
        assert call(a6=bad) == -1, "accel_psd %r" % bad
    assert "hupr_pose_smooth_rts_f32" in rt.last_error()
    assert call(a4=0) == 0                                                      # rows == 0 with T >= 1: a no-op
    assert L.hupr_launch_count() == c0
    torch.cuda.synchronize()
    assert (flag == -7).all().item()
    assert call() == 0 and L.hupr_launch_count() == c0 + 1
    torch.cuda.synchronize()
    assert (flag[-1] == sr.END).all().item() and (flag[:-1] == sr.SMOOTHED).all().item()    # status UPDATED throughout: one segment
