"""GPU (-m gpu): hupr_pose_smooth_lag_f32 (csrc/pose_lag.hip) — the fixed-lag Rauch-Tung-Striebel smoother behind the Kalman tracker,
one launch per frame over a ring of the last L + 1 tracker states — against hupr_pose_smooth_rts_f32 on the same windows, bit for bit,
and against the NumPy statement of the rule in tests/pose_lag_ref.py; then behind the live stream, the offline SequenceSmoother and
Runner.eval.

The history.  The scenario of tests/pose_track_ref.py (60 frames x 28 rows of 64 x 64 maps at 10 Hz, seed 11, with its drop-out,
outlier, gone and never-seen rows) goes through functional.pose_track frame by frame (PoseTracking's defaults, accel_psd = 200,
min_score = 0.1, arg-max measurements), the state and the outputs kept after every launch; the lag launch then runs after every frame
for L in {1, 4, 64}: 28 rows are no multiple of the 64 threads of a workgroup, and 60 frames wrap the rings of L = 1 and L = 4 many
times.

Bounds.  Against the fixed-interval kernel: torch.equal — both compile csrc/pose_rts.h.  Against the fp64 rule, fed the same fp32
history so that only the backward pass is measured: 16 x the differences of the NumPy fp32 run of the restatement from its fp64 run
at L = 4 (pose_lag_ref.POS_FP32 = 3.69e-5 pixel, VEL_FP32 = 6.93e-5 pixel / s, COV_REL_FP32 = 2.24e-6; tests/test_pose_lag_cpu.py
measures them), i.e. 5.9e-4 pixel, 1.1e-3 pixel / s and 3.6e-5 — the project's rule for the fixed-interval kernel."""
import functools

import numpy as np
import pytest
import torch

import pose_lag_ref as lr
import pose_smooth_ref as sr
import pose_track_ref as ref

pytestmark = pytest.mark.gpu
TOL_POS, TOL_VEL, TOL_COV_REL = 16 * lr.POS_FP32, 16 * lr.VEL_FP32, 16 * lr.COV_REL_FP32
LAGS = (1, 4, 64)
TAIL = ("kp", "vel", "cov", "flag", "filtered", "raw", "status", "scores")
HIST = ("states", "status", "kp", "raw", "scores")


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(dict(accel_psd=sr.ACCEL_PSD, min_score=ref.MIN_SCORE), **kw))


@functools.lru_cache(maxsize=None)
def history(rows=ref.ROWS, zero=None):
    """The scenario's rows, tiled to ``rows`` of them, through functional.pose_track frame by frame from a fresh state; ``zero`` =
    (frame, row): that row's tracker state is zeroed in front of that frame -> dict of (T, rows, ...) device tensors: states, status,
    kp (the filtered keypoints), raw, scores."""
    from hupr_amd import functional as F_
    heat = torch.from_numpy(np.array(ref.scenario(True, ref.SEED)[0])).cuda()
    pick = torch.arange(rows, device="cuda") % ref.ROWS
    p, state = tracking(), F_.pose_track_state(rows, "cuda")
    out = {k: [] for k in HIST}
    for t in range(ref.T):
        if zero is not None and t == zero[0]:
            state[zero[1]].zero_()
        o = F_.pose_track(heat[t][pick], ref.RATIO, refine=False, track_state=state, tracking=p)
        for k, v in zip(HIST, (state.clone(), o[7], o[3], o[2], o[1])):
            out[k].append(v)
    return {k: torch.stack(v) for k, v in out.items()}


def launch(h, t, lag_state, L, cols=slice(None), out=None):
    from hupr_amd import functional as F_
    return F_.pose_smooth_lag(*[h[k][t, cols].contiguous() for k in HIST], lag_state, tracking(), L, out=out)


def lag_run(h, L, lag_state=None, cols=slice(None)):
    """The lag launch after every frame of ``h`` -> (the T tails, each a dict of (L + 1, rows, ...) clones; the lag state)."""
    from hupr_amd import functional as F_
    rows = h["status"][0, cols].shape[0]
    lag_state = F_.pose_lag_state(rows, L, "cuda") if lag_state is None else lag_state
    tails, out = [], None
    for t in range(ref.T):
        out = launch(h, t, lag_state, L, cols, out)
        tails.append({k: v.clone() for k, v in zip(TAIL, out)})
    return tails, lag_state


@functools.lru_cache(maxsize=None)
def scenario_tails(L):
    return lag_run(history(), L)[0]


def answers(tails, L):
    """What a consumer keeps: frame k from slot L of the launch of frame k + L, the last L frames from the last launch's tail."""
    T = len(tails)
    return {k: torch.stack([tails[f + L][k][L] if f + L < T else tails[-1][k][T - 1 - f] for f in range(T)]) for k in TAIL}


def rts(h, lo, hi, cols=slice(None)):
    """functional.pose_smooth_rts over the recorded frames lo .. hi -> dict of (hi - lo + 1, rows, ...)."""
    from hupr_amd import functional as F_
    o = F_.pose_smooth_rts(*[h[k][lo:hi + 1, cols].contiguous() for k in ("states", "status", "kp")], tracking())
    return dict(zip(TAIL[:4], o))


# ---- 1: the window is the fixed-interval kernel's recording, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("L", LAGS)
def test_every_tail_is_the_fixed_interval_kernel_over_the_same_frames(L):
    h, tails, T = history(), scenario_tails(L), ref.T
    for n in range(T):
        lo = max(n - L, 0)
        want = rts(h, lo, n)
        for k in TAIL[:4]:
            assert torch.equal(tails[n][k][:n - lo + 1], want[k].flip(0)), (L, n, k)
        # the filter's record of the same frames
        for k, src in zip(TAIL[4:], ("kp", "raw", "status", "scores")):
            assert torch.equal(tails[n][k][:n - lo + 1], h[src][lo:n + 1].flip(0)), (L, n, k)
    # frame k is emitted from slot L once frame k + L is there, and that is the smoother over [k .. k + L] at index 0; the last L
    # frames come from the last tail, the smoother over [k .. T - 1] at index 0
    a = answers(tails, L)
    for f in range(T):
        want = rts(h, f, min(f + L, T - 1))
        for k in TAIL[:4]:
            assert torch.equal(a[k][f], want[k][0]), (L, f, k)
    # the whole tail after the last frame: the fixed-interval kernel over the last L + 1 frames
    lo = max(T - 1 - L, 0)
    want = rts(h, lo, T - 1)
    for k in TAIL[:4]:
        assert torch.equal(tails[-1][k][:T - lo], want[k].flip(0)), (L, k)
    # slot 0 is the filter itself, always
    for n in (0, 1, 29, 30, T - 1):
        assert torch.isin(tails[n]["flag"][0], torch.tensor([sr.END, sr.PASSTHROUGH], device="cuda", dtype=torch.int32)).all().item()
        assert torch.equal(tails[n]["kp"][0], h["kp"][n])


def test_a_lag_beyond_the_run_leaves_empty_slots_and_ends_as_the_whole_recording():
    L, T = 64, ref.T
    h, tails = history(), scenario_tails(64)
    for n in (0, 1, 30, T - 1):
        empty = {k: v[n + 1:] for k, v in tails[n].items()}
        assert (empty["flag"] == lr.EMPTY).all().item() and (tails[n]["flag"][:n + 1] != lr.EMPTY).all().item()
        for k in TAIL:
            if k != "flag":
                assert not empty[k].any().item(), (n, k)
    whole = rts(h, 0, T - 1)
    for k in TAIL[:4]:
        assert torch.equal(tails[-1][k][:T], whole[k].flip(0)), k
    # and a short lag never shows an EMPTY slot once the ring is full
    for n in range(ref.T):
        assert ((scenario_tails(4)[n]["flag"] == lr.EMPTY).sum(0) == max(4 - n, 0)).all().item(), n


# ---- 2: against the fp64 rule ---------------------------------------------------------------------------------------------------------------
def test_the_lagged_poses_follow_the_fp64_rule():
    L, h = 4, history()
    a = answers(scenario_tails(L), L)
    a64, tails64 = lr.ref_lag(h["states"].cpu().numpy(), h["status"].cpu().numpy(), h["kp"].cpu().numpy(), ref.RATE, sr.ACCEL_PSD, L)
    flag = a["flag"].cpu().numpy()
    assert np.array_equal(flag, a64["flag"])
    e_kp = np.abs(a["kp"].cpu().numpy() - a64["kp"]).max()
    e_vel = np.abs(a["vel"].cpu().numpy() - a64["vel"]).max()
    e_cov = ref.cov_rel_diff(a["cov"].cpu().numpy(), a64["cov"])
    print("L = 4: max |lagged - fp64| %.3e px (bound %.3e), |velocity - fp64| %.3e px/s (bound %.3e), covariance relative %.3e "
          "(bound %.3e); flags %s" % (e_kp, TOL_POS, e_vel, TOL_VEL, e_cov, TOL_COV_REL, np.bincount(flag.ravel(), minlength=5).tolist()))
    assert e_kp <= TOL_POS and e_vel <= TOL_VEL and e_cov <= TOL_COV_REL
    # every tail too, the EMPTY slots of the first frames included
    for n in (0, 2, 3, 4, 29, 31, ref.T - 1):
        t = scenario_tails(L)[n]
        assert np.array_equal(t["flag"].cpu().numpy(), tails64[n]["flag"]), n
        assert np.abs(t["kp"].cpu().numpy() - tails64[n]["kp"]).max() <= TOL_POS and np.abs(t["vel"].cpu().numpy() - tails64[n]["vel"]).max() <= TOL_VEL
    # a real test: the lag moves the keypoints towards the truth, by what the CPU table says
    truth = ref.scenario()[1]
    kp, lg = h["kp"].cpu().numpy().astype(np.float64), a["kp"].cpu().numpy().astype(np.float64)
    e_f, e_l = sr.rms((kp - truth)[:, sr.NORMAL]), sr.rms((lg - truth)[:, sr.NORMAL])
    print("rms error on the %d normal rows: filter %.3f px, lag 4 %.3f px (ratio %.3f)" % (len(sr.NORMAL), e_f, e_l, e_l / e_f))
    assert e_l / e_f < 0.6
    want = [sr.SMOOTHED] * 29 + [sr.END] + [sr.PASSTHROUGH] * 5 + [sr.SMOOTHED] * 24 + [sr.END]
    assert flag[:, ref.GONE].tolist() == want and (flag[:, ref.NEVER] == sr.PASSTHROUGH).all()


# ---- 3: 65 rows: a second workgroup, independent rows, a broken chain, a zeroed lag state ------------------------------------------------------
def test_rows_are_independent_and_a_zeroed_state_starts_anew():
    L, ROW, AT, T = 4, 64, 30, ref.T
    twin = ROW % ref.ROWS
    assert twin in sr.NORMAL
    h = history(65, zero=(AT, ROW))
    status = h["status"].cpu().numpy()
    assert status[AT, ROW] == ref.STARTED and status[AT, twin] == ref.UPDATED and status[AT - 1, ROW] == ref.UPDATED
    tails, state = lag_run(h, L)
    a = answers(tails, L)
    # against the fixed-interval kernel on the windows, across the workgroup boundary
    for f in (0, AT - L - 1, AT - L, AT - 1, AT, T - 2, T - 1):
        want = rts(h, f, min(f + L, T - 1))
        for k in TAIL[:4]:
            assert torch.equal(a[k][f], want[k][0]), (f, k)
    # rows are independent: the tiles are equal, bit for bit, except the one row whose tracker state was zeroed
    for k in TAIL:
        assert torch.equal(a[k][:, :ref.ROWS], a[k][:, ref.ROWS:2 * ref.ROWS]), k
        assert torch.equal(a[k][:, :ROW - 2 * ref.ROWS], a[k][:, 2 * ref.ROWS:ROW]), k
    # ... which alone in a launch of one row gives the same bits as in its place among 65
    alone = answers(lag_run(h, L, cols=slice(ROW, ROW + 1))[0], L)
    for k in TAIL:
        assert torch.equal(alone[k][:, 0], a[k][:, ROW]), k
    # STARTED breaks the chain: frame AT - 1 ends its segment with the filter's own bits, frames up to AT - 1 - L never see the break
    assert a["flag"][AT - 1, ROW].item() == sr.END and a["flag"][AT - 1, twin].item() == sr.SMOOTHED
    assert torch.equal(a["kp"][AT - 1, ROW], h["kp"][AT - 1, ROW]) and torch.equal(a["vel"][AT - 1, ROW], h["states"][AT - 1, ROW, 2:4])
    assert torch.equal(a["cov"][AT - 1, ROW], h["states"][AT - 1, ROW][[4, 5, 8]])
    for k in TAIL[:4]:
        assert torch.equal(a[k][:AT - L, ROW], a[k][:AT - L, twin]), k
    assert not torch.equal(a["kp"][AT - L:AT, ROW], a["kp"][AT - L:AT, twin])
    # a second pass over the same ring without zeroing sees the first pass's frames behind its first; zeroed, it is the first pass
    first = launch(h, 0, state.clone(), L)
    assert (first[3][1:] != lr.EMPTY).all().item()
    state.zero_()
    again, _ = lag_run(h, L, lag_state=state)
    assert (again[0]["flag"][1:] == lr.EMPTY).all().item()
    for n in range(T):
        for k in TAIL:
            assert torch.equal(again[n][k], tails[n][k]), ("after zeroing", n, k)


def test_argument_errors_return_minus_one_and_launch_nothing():
    from hupr_amd import functional as F_
    from hupr_amd import runtime as rt
    lib = rt.lib()
    rows, L = 3, 2
    st = torch.zeros((rows + 1, 16), device="cuda")
    status = torch.zeros(rows, dtype=torch.int32, device="cuda")
    kp, raw, mx = torch.zeros((rows, 2), device="cuda"), torch.zeros((rows, 2), device="cuda"), torch.zeros(rows, device="cuda")
    ls = torch.zeros(F_.pose_lag_state(rows, L, "cuda").numel() + 4, device="cuda")
    tail = [torch.zeros((L + 1, rows) + s, dtype=d, device="cuda") for s, d in (((2,), torch.float32), ((2,), torch.float32), ((3,), torch.float32),
            ((), torch.int32), ((2,), torch.float32), ((2,), torch.float32), ((), torch.int32), ((), torch.float32))]
    tail[3].fill_(-7)
    good = [rt.ptr(st), rt.ptr(status), rt.ptr(kp), rt.ptr(raw), rt.ptr(mx), rows, L, 10.0, 200.0, rt.ptr(ls)] + [rt.ptr(t) for t in tail]

    def call(**change):
        a = list(good)
        for i, v in change.items():
            a[int(i[1:])] = v
        return lib.hupr_pose_smooth_lag_f32(*a, rt.stream())

    c0 = lib.hupr_launch_count()
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 14, 15, 16, 17):
        assert call(**{"a%d" % i: None}) == -1, "null pointer %d" % i
    assert call(a5=-1) == -1 and call(a5=1 << 40) == -1                         # rows
    for bad in (0, -1, 65, 1 << 20):
        assert call(a6=bad) == -1, "lag %r" % bad
    assert call(a0=rt.ptr(st) + 4) == -1 and call(a9=rt.ptr(ls) + 4) == -1      # misaligned tracker state, misaligned lag state
    for bad in (0.0, -10.0, float("inf"), float("nan")):
        assert call(a7=bad) == -1, "rate_hz %r" % bad
    for bad in (-1.0, float("inf"), float("nan")):
        assert call(a8=bad) == -1, "accel_psd %r" % bad
    assert "hupr_pose_smooth_lag_f32" in rt.last_error()
    assert call(a5=0) == 0                                                      # rows == 0: a no-op
    assert lib.hupr_launch_count() == c0
    torch.cuda.synchronize()
    assert (tail[3] == -7).all().item() and not ls.any().item()
    assert call() == 0 and call(a0=rt.ptr(st) + 64, a9=rt.ptr(ls) + 16) == 0 and lib.hupr_launch_count() == c0 + 2
    torch.cuda.synchronize()
    assert tail[3].cpu().tolist() == [[sr.END] * rows, [lr.EMPTY] * rows, [lr.EMPTY] * rows]    # status UPDATED, a state with no frame behind it


# ---- 4: the offline route ---------------------------------------------------------------------------------------------------------------------
def test_a_sequence_smoother_with_a_lag_keeps_the_fixed_lag_answers():
    from hupr_amd.tools import SequenceSmoother, SmoothedSequence, TrackingError
    L, CUT, T = 4, 25, ref.T
    heat = torch.from_numpy(np.array(ref.scenario(True, ref.SEED)[0])).cuda()
    sm, plain = SequenceSmoother(tracking(), ref.ROWS, "cuda", lag=L), SequenceSmoother(tracking(), ref.ROWS, "cuda")
    with pytest.raises(TrackingError):
        plain.smooth_lagged()
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            SequenceSmoother(tracking(), ref.ROWS, "cuda", lag=bad)
    for t in range(T):
        if t == CUT:
            sm.new_sequence()
            plain.new_sequence()
        a, b = sm.track(heat[t], ref.RATIO, refine=False), plain.track(heat[t], ref.RATIO, refine=False)
        for x, y in zip(a, b):
            assert torch.equal(x, y)                                            # the smoother feeds nothing back
        if t in (3, CUT - 1, CUT + 2):                                          # asked in the middle of a sequence, and going on after it
            part = sm.smooth_lagged()
            assert len(part) == t + 1 and torch.equal(part.keypoints[t], part.filtered[t])
    seq, whole = sm.smooth_lagged(), sm.smooth()
    assert isinstance(seq, SmoothedSequence) and len(seq) == T and seq.keypoints.shape == (T, ref.ROWS, 2) and seq.flag.shape == (T, ref.ROWS)
    for k in ("filtered", "raw", "status", "scores"):
        assert torch.equal(getattr(seq, k), getattr(whole, k)), k
    h = dict(zip(HIST, (sm.history._views()[k] for k in ("states", "status", "filtered", "raw", "scores"))))
    for f in range(T):
        end = CUT - 1 if f < CUT else T - 1                                      # the last frame of f's sequence
        want = rts(h, f, min(f + L, end))
        for k, name in zip(TAIL[:4], ("keypoints", "velocity", "covariance", "flag")):
            assert torch.equal(getattr(seq, name)[f], want[k][0]), (f, name)
    assert (seq.flag[CUT - 1][seq.status[CUT - 1] != ref.LOST] == sr.END).all().item()
    assert not torch.equal(seq.keypoints, whole.keypoints) and not torch.equal(seq.keypoints, seq.filtered)
    sm.clear()
    assert len(sm) == 0
    sm.track(heat[0], ref.RATIO, refine=False)
    one = sm.smooth_lagged()
    assert len(one) == 1 and torch.equal(one.keypoints[0], seq.filtered[0])
    assert torch.isin(one.flag, torch.tensor([sr.END, sr.PASSTHROUGH], device="cuda", dtype=torch.int32)).all().item()


# ---- 5: the live session ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from test_stream_smooth_gpu import _Ctx
    c = _Ctx()
    yield c
    c.engine.close()


LAGGED = ("keypoints", "velocity", "covariance", "flag", "filtered", "raw_keypoints", "status", "scores")


def test_a_session_with_a_lag_emits_the_pose_of_two_frames_ago(ctx):
    from test_stream_smooth_gpu import FIELDS, N
    from hupr_amd import functional as F_
    from hupr_amd.tools import LaggedPose, LaggedTrackedPoseFrame, TrackedPoseFrame, TrackingError
    L = 2
    plain = ctx.session()
    as_today = ctx.play(plain)
    s = ctx.session(history=True, lag=L)
    frames = ctx.play(s)
    assert bool(s._graphs) and bool(plain._graphs)
    assert all(type(p) is TrackedPoseFrame and p.lagged is None for p in as_today) and all(type(p) is LaggedTrackedPoseFrame for p in frames)
    # the filter's outputs of every frame: those of a session without lag
    for a, b in zip(as_today, frames):
        for k in FIELDS:
            assert torch.equal(getattr(a, k), getattr(b, k)), (a.frame, k)
    with pytest.raises(TrackingError):
        plain.lag_tail()
    h = s._history._views()
    states, status, filtered = h["states"], h["status"], h["filtered"]

    def check(lp, k, hi):
        """``lp`` is the pose of frame k smoothed over the history's frames k .. hi."""
        assert type(lp) is LaggedPose and lp.frame == k
        want = F_.pose_smooth_rts(states[k:hi + 1], status[k:hi + 1], filtered[k:hi + 1], s.track)
        for name, w in zip(LAGGED[:4], want):
            assert getattr(lp, name).shape == w[0].shape and torch.equal(getattr(lp, name), w[0]), (k, name)
        assert torch.equal(lp.filtered, frames[k].keypoints) and torch.equal(lp.raw_keypoints, frames[k].raw_keypoints), k
        assert torch.equal(lp.status, frames[k].status) and torch.equal(lp.scores, frames[k].scores), k

    assert frames[0].lagged is None and frames[1].lagged is None
    for pf in frames[L:]:
        assert pf.lagged.frame == pf.frame - L
        check(pf.lagged, pf.frame - L, pf.frame)
    assert (frames[-1].lagged.flag == F_.SMOOTH_SMOOTHED).any().item()
    assert not torch.equal(frames[-1].lagged.keypoints, frames[-1].lagged.filtered)   # the smoother moves them
    tail = s.lag_tail()
    seq = s.smoothed()
    assert [lp.frame for lp in tail] == [N - 2, N - 1]
    for lp in tail:
        check(lp, lp.frame, N - 1)
        for name, w in zip(LAGGED[:4], (seq.keypoints, seq.velocity, seq.covariance, seq.flag)):
            assert torch.equal(getattr(lp, name), w[lp.frame]), (lp.frame, name)
    # reset() starts the ring anew: a second play gives the same bits
    kept = [(pf.lagged, pf.keypoints) for pf in frames]
    s.reset()
    again = ctx.play(s)
    for (lp, kp), pf in zip(kept, again):
        assert torch.equal(kp, pf.keypoints) and (lp is None) == (pf.lagged is None)
        if lp is not None:
            for name in LAGGED:
                assert torch.equal(getattr(lp, name), getattr(pf.lagged, name)), (pf.frame, name)
    for x, y in zip(tail, s.lag_tail()):
        for name in LAGGED:
            assert torch.equal(getattr(x, name), getattr(y, name)), (x.frame, name)


def test_stream_command_with_track_lag_adds_the_lagged_pose_to_every_record(ctx, tmp_path, monkeypatch):
    """python -m hupr_amd.tools.stream --track --rate 10 --track-lag 2 --rts on a tiny raw capture with a saved checkpoint: every record
    gains the four lagged fields, the last two from lag_tail(), and those two are the whole-recording smoother's."""
    import json
    import os
    from hupr_amd import synth
    from hupr_amd.tools import stream as st
    root = synth.write_tiny_dataset(str(tmp_path / "tinyraw"), cubes=False, raw=True)
    seq = synth.TINY["valName"][0]
    os.makedirs(tmp_path / "logs" / "streamtest")
    torch.save({"epoch": 3, "model_state_dict": ctx.model.state_dict(), "optimizer_state_dict": {}, "accuracy": 0.0},
               str(tmp_path / "logs" / "streamtest" / "model_best.pth"))
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "poses.json"
    st.main(["--dir", "streamtest", "--raw", os.path.join(root, "single_%d" % seq), "--math", "bf16", "--out", str(out),
             "--decode", "subpixel", "--track", "--rate", "10", "--track-lag", "2", "--rts"])
    records = json.load(open(out))
    n = synth.TINY["duration"]
    assert n > 2 and [r["frame"] for r in records] == list(range(n))
    for r in records:
        assert {"lagged", "lagged_velocity", "lagged_covariance", "lagged_flag", "smoothed", "smoothed_flag", "keypoints", "status"} <= set(r)
        assert np.array(r["lagged"]).shape == (14, 2) and np.array(r["lagged_velocity"]).shape == (14, 2)
        assert np.array(r["lagged_covariance"]).shape == (14, 3) and len(r["lagged_flag"]) == 14
        assert np.isfinite(r["lagged"]).all() and all(f in (0, 1, 2, 3) for f in r["lagged_flag"])
        for j, f in enumerate(r["lagged_flag"]):
            assert (f == 2) == (r["status"][j] == 4)                              # PASSTHROUGH where the tracker says LOST
            if f in (1, 2):                                                     # END / PASSTHROUGH: the filter's own keypoint
                assert r["lagged"][j] == r["keypoints"][j][:2]
    for r in records[-3:]:                                                      # smoothed over all the frames there are: the offline answer
        assert r["lagged"] == r["smoothed"] and r["lagged_flag"] == r["smoothed_flag"] and r["lagged_covariance"] == r["smoothed_covariance"]
    assert all(f in (1, 2) for f in records[-1]["lagged_flag"])
    assert any(f == 0 for r in records for f in r["lagged_flag"])


# ---- 6: Runner.eval -----------------------------------------------------------------------------------------------------------------------------
def test_eval_with_temporal_lag_scores_the_lagged_keypoints(tmp_path, monkeypatch, capsys):
    import re
    from test_stream_smooth_gpu import FRAMES, _eval
    lines, recs = _eval(tmp_path, monkeypatch, capsys, "lag", temporal="lag", temporalLag=2)
    assert len(recs) == FRAMES and [r["image_id"] for r in recs] == list(range(FRAMES))
    assert all(len(r["keypoints"]) == 42 and np.isfinite(r["keypoints"]).all() for r in recs)
    ap = next(i for i, l in enumerate(lines) if l.startswith("AP:"))
    tail = lines[ap + 1:]
    mp = [l for l in tail if l.startswith("MPJPE ")]
    assert [l.split(":")[0] for l in mp] == ["MPJPE raw", "MPJPE filtered", "MPJPE lagged"]
    for l in mp:
        m = re.fullmatch(r"MPJPE \w+: (\S+) px \(n = (\d+)\)", l)
        assert m and np.isfinite(float(m.group(1))) and int(m.group(2)) == FRAMES, l
    jt = [l for l in tail if l.startswith("Jitter ")]
    assert [l.split(":")[0] for l in jt] == ["Jitter raw", "Jitter filtered", "Jitter lagged", "Jitter truth"]
    for l in jt:
        m = re.fullmatch(r"Jitter \w+: (\S+) px", l)
        assert m and np.isfinite(float(m.group(1))), l
    assert tail.index(jt[0]) > tail.index(mp[-1])
