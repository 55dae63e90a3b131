"""GPU (-m gpu): hupr_pose_track_imm_f32 (csrc/pose_imm.hip) — the decode of hupr_pose_decode_f32, the tracker's measurement, and two
constant-velocity Kalman filters per row coupled as an interacting-multiple-model estimator — against functional.pose_decode, against
the plain tracker hupr_pose_track_f32, and against the NumPy statement of the rule in tests/pose_imm_ref.py.

Bounds.  Decode: bit equality with functional.pose_decode.  With switch_prob = 0 and moving_prior = 0: bit equality with the plain
tracker, outputs and state.  Filtered keypoints and forecast: TOL_FILTER = 2e-3 image pixel, the plain tracker's bound
(tests/test_pose_track_gpu.py); velocity rate_hz x that.  Covariance, relative to the larger variance of the fp64 one, and ``moving``:
the NumPy fp32 run of the restatement (window moments included) differs from the fp64 run by COV_REL_FP32 = 1.39e-5 and
MOVING_FP32 = 7.06e-6 on the stop-and-go scenario, seed 3 (measured on the CPU, tests/test_pose_imm_cpu.py prints them again and
holds them), and the bounds are 16 x those = 2.22e-4 and 1.13e-4: the kernel contracts to FMAs, mixes means as x_0 + w (x_1 - x_0)
and takes exp and ln from the device library.  The covariance figure is larger than the plain tracker's 3.02e-7 because the mixture
adds the spread of the two means, a difference of positions near 200 pixels, to variances of a few pixels squared.  The tests print
what the GPU shows.

The scenario (pose_imm_ref.stop_and_go, seed 3): in the fp64 run on the measurement-level stand-in the closest decisive d2 lies
7.6 % from the gate of 13.816; the test asserts > 1 % on the fp64 run fed the GPU's own decode.

At most 120 launches of 28 rows per test."""
import functools

import numpy as np
import pytest
import torch

import pose_imm_ref as ref
import pose_track_ref as plain

pytestmark = pytest.mark.gpu
TOL_FILTER = 2e-3
COV_REL_FP32, MOVING_FP32 = 1.39e-5, 7.06e-6
TOL_COV_REL, TOL_MOVING = 16 * COV_REL_FP32, 16 * MOVING_FP32
OUT = ("idx", "maxval", "raw", "kp", "vel", "cov", "fc", "status", "moving")
MODELS = dict(accel_psd=5.0, accel_psd_moving=5000.0, switch_prob=0.05, meas_std=3.0, heatmap_gain=0.0)


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(dict(MODELS, min_score=ref.MIN_SCORE), **kw))


def track(maps, ratio, state, p, refine=True, present=None):
    from hupr_amd import functional as F_
    heat = maps if isinstance(maps, torch.Tensor) else torch.from_numpy(np.array(maps)).cuda()
    return dict(zip(OUT, F_.pose_track(heat, ratio, refine=refine, track_state=state, tracking=p, present=present)))


def stacked(seq, key):
    return np.stack([o[key].cpu().numpy() for o in seq])


# ---- 1: decode anchor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 28])
@pytest.mark.parametrize("refine", [False, True], ids=["argmax", "subpixel"])
@pytest.mark.parametrize("H,W", [(64, 64), (24, 40)], ids=["64x64", "24x40"])
def test_the_decode_is_pose_decode_bit_for_bit(H, W, refine, rows):
    from hupr_amd import functional as F_
    ratio = 4.0
    maps = np.random.RandomState(3).uniform(-0.2, 1.0, (rows, H, W)).astype(np.float32)
    maps[0].reshape(-1)[[77, 300, 900]] = 2.0                  # tied maxima: the first wins
    if rows > 10:
        maps[9] = -np.abs(maps[9])                             # all <= 0 -> (0, 0)
        maps[10] = 0.0
    heat = torch.from_numpy(maps).cuda()
    idx, mx, raw, _, _ = F_.pose_decode(heat, ratio, refine=refine)
    state = F_.pose_imm_state(rows, "cuda")
    assert state.shape == (rows, 32) and not state.any().item()
    o = track(heat, ratio, state, tracking(min_score=0.0, moving_prior=0.25), refine=refine)
    assert o["idx"].dtype == torch.int32 and o["status"].dtype == torch.int32 and o["moving"].dtype == torch.float32
    assert torch.equal(o["idx"], idx) and torch.equal(o["maxval"], mx) and torch.equal(o["raw"], raw)
    assert idx[0].item() == 77
    usable = torch.ones(rows, dtype=torch.bool, device="cuda")
    if rows > 10:
        usable[[9, 10]] = False
        assert raw[9].tolist() == [0.0, 0.0] and raw[10].tolist() == [0.0, 0.0]
    assert torch.equal(o["status"], torch.where(usable, plain.STARTED, plain.LOST).to(torch.int32))
    assert torch.equal(o["kp"], raw) and torch.equal(o["fc"], raw) and not o["vel"].any().item()
    assert torch.equal(o["moving"], torch.where(usable, 0.25, 0.0).to(torch.float32))
    assert not state[~usable].any().item() and (state[usable][:, 30] == 1).all().item()
    assert torch.equal(state[usable][:, 0:2], raw[usable]) and torch.equal(state[usable][:, 14:16], raw[usable])
    assert torch.equal(state[usable][:, 28:30], torch.tensor([0.75, 0.25], device="cuda").expand(int(usable.sum()), 2))


# ---- 2: bit anchor to the plain tracker ----------------------------------------------------------------------------------------------------
def test_without_switching_and_prior_the_outputs_and_the_state_are_the_plain_trackers():
    """switch_prob = 0, moving_prior = 0: model 1 never has a say, and the eight outputs, state floats 0..13 and live / coast are
    hupr_pose_track_f32's on every frame of its own scenario with its events — the filter functions compiled into the two kernels are
    the same ones — and ``moving`` is exactly 0."""
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseTracking
    heat = torch.from_numpy(np.array(plain.scenario()[0])).cuda()
    kw = dict(accel_psd=100.0, min_score=plain.MIN_SCORE, horizon_s=0.3)
    p1, p2 = PoseTracking(plain.RATE, **kw), PoseTracking(plain.RATE, accel_psd_moving=5000.0, switch_prob=0.0, moving_prior=0.0, **kw)
    s1, s2 = F_.pose_track_state(plain.ROWS, "cuda"), F_.pose_imm_state(plain.ROWS, "cuda")
    seen = set()
    for t in range(plain.T):
        a = F_.pose_track(heat[t], plain.RATIO, track_state=s1, tracking=p1)
        b = F_.pose_track(heat[t], plain.RATIO, track_state=s2, tracking=p2)
        assert len(a) == 8 and len(b) == 9
        for k, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (t, OUT[k])
        assert torch.equal(s1[:, :14], s2[:, :14]) and torch.equal(s1[:, 14:], s2[:, 30:]), t
        assert not b[8].any().item(), t
        live = s2[:, 30] == 1
        assert torch.equal(s2[:, 28], live.float()) and not s2[:, 29].any().item(), t           # mu = (1, 0) on every live row
        seen |= set(a[7].cpu().numpy().tolist())
    assert seen == {plain.UPDATED, plain.COASTED_MISSING, plain.COASTED_GATED, plain.STARTED, plain.LOST}
    assert s2[:, 14:28].any().item()                                                       # model 1 did run


# ---- 3: recurrence ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scenario_on_gpu():
    return torch.from_numpy(np.array(ref.stop_and_go()[0])).cuda()


@functools.lru_cache(maxsize=None)
def gpu_run(run=0, first=0, last=ref.T, **kw):
    """Frames first .. last-1 of the scenario through the kernel from a fresh state -> [per frame: dict of cloned outputs and the state
    after the frame]."""
    from hupr_amd import functional as F_
    heat, p = scenario_on_gpu(), tracking(**kw)
    state = F_.pose_imm_state(ref.ROWS, "cuda")
    seq = []
    for t in range(first, last):
        o = track(heat[t], ref.RATIO, state, p)
        o["state"] = state.clone()
        seq.append(o)
    return seq


def fp64_run(seq, first=0, **kw):
    """The restatement fed the GPU's own raw keypoints and maxima and the fp64 window moments of the same float32 maps."""
    idx = stacked(seq, "idx")
    maps = ref.stop_and_go()[0]
    mom = np.stack([plain.window_moments(maps[first + t], idx[t]) for t in range(len(seq))])
    return ref.ref_imm(stacked(seq, "raw"), stacked(seq, "maxval"), mom, tracking(**kw), ref.RATIO)


def test_the_recurrence_follows_the_fp64_rule():
    seq, p = gpu_run(horizon_s=0.3), tracking(horizon_s=0.3)
    o64 = fp64_run(seq, horizon_s=0.3)
    status = stacked(seq, "status")
    # the condition on the inputs: no decisive d2 of the fp64 run is within 1 % of the gate
    margin = ref.rel_gate_margin(o64["d2"], p.gate)
    print("closest decisive d2: %.2f %% from the gate (%d decisions)" % (100 * margin, int(np.isfinite(o64["d2"]).sum())))
    assert np.isfinite(o64["d2"]).sum() > 3000 and margin > 0.01
    assert np.array_equal(status, o64["status"])                                           # every row, every frame
    e_kp, e_fc = np.abs(stacked(seq, "kp") - o64["kp"]).max(), np.abs(stacked(seq, "fc") - o64["fc"]).max()
    e_vel = np.abs(stacked(seq, "vel") - o64["vel"]).max()
    e_cov = plain.cov_rel_diff(stacked(seq, "cov"), o64["cov"])
    e_mov = np.abs(stacked(seq, "moving") - o64["moving"]).max()
    print("two models over %d frames x %d rows: max |filtered - fp64| %.3e px, |forecast - fp64| %.3e px, |velocity - fp64| %.3e px/s, "
          "covariance relative %.3e (bound %.3e), |moving - fp64| %.3e (bound %.3e); statuses %s"
          % (ref.T, ref.ROWS, e_kp, e_fc, e_vel, e_cov, TOL_COV_REL, e_mov, TOL_MOVING, np.bincount(status.ravel(), minlength=5).tolist()))
    assert e_kp <= TOL_FILTER and e_fc <= TOL_FILTER
    assert e_vel <= p.rate_hz * TOL_FILTER
    assert e_cov <= TOL_COV_REL
    assert e_mov <= TOL_MOVING
    # the layout of the state: two models, mu, live, coast
    last = seq[-1]["state"].cpu().numpy()
    assert np.abs(o64["state"] - last).max() <= 1.0 and np.array_equal(o64["state"][:, 30:], last[:, 30:])
    assert np.abs(o64["state"][:, 28:30] - last[:, 28:30]).max() <= TOL_MOVING
    assert np.array_equal(stacked(seq, "moving"), np.stack([o["state"][:, 29].cpu().numpy() for o in seq]))
    # a real test: both regimes occur, the moving model is the likelier one in a reach, and the mixture beats the raw keypoints
    _, truth, _, moving = ref.stop_and_go()
    N = list(ref.NORMAL)
    mv = stacked(seq, "moving")[:, N]
    in_reach, at_rest = float(mv[moving[:, N]].mean()), float(mv[~moving[:, N]].mean())
    rms = lambda a: float(np.sqrt(np.mean(np.sum(a.astype(np.float64) ** 2, axis=-1))))
    e_f, e_r = rms((stacked(seq, "kp") - truth)[:, N]), rms((stacked(seq, "raw") - truth)[:, N])
    print("rms error %.3f px filtered, %.3f px raw; moving %.3f in a reach, %.3f at rest" % (e_f, e_r, in_reach, at_rest))
    assert mv.max() > 0.9 and mv[1:].min() < 0.15 and in_reach > at_rest and e_f < e_r
    assert (status[0, N] == plain.STARTED).all()


# ---- 4: life cycle ---------------------------------------------------------------------------------------------------------------------------
def test_the_life_cycle_is_shared_by_both_models():
    """Frames 36 .. 75 of the scenario with moving_prior = 0.25: the drop-out row coasts with a growing covariance and resumes, the
    outlier is refused by the gate, the row gone for ten frames with max_coast = 5 shows five coasts, then LOST with a zero state and
    the raw keypoint, then STARTED with mu = (0.75, 0.25); the never-usable row stays zero."""
    first = 36
    seq = gpu_run(first=first, last=76, moving_prior=0.25)
    o64 = fp64_run(seq, first=first, moving_prior=0.25)
    status = stacked(seq, "status")
    assert np.array_equal(status, o64["status"])
    at = lambda t: seq[t - first]
    d0, d1 = ref.DROP_FRAMES[0], ref.DROP_FRAMES[-1]
    for t in ref.DROP_FRAMES:
        assert at(t)["maxval"][ref.DROP].item() <= ref.MIN_SCORE and at(t)["status"][ref.DROP].item() == plain.COASTED_MISSING
        assert at(t)["state"][ref.DROP, 31].item() == t - d0 + 1
        assert at(t)["cov"][ref.DROP, 0].item() > at(t - 1)["cov"][ref.DROP, 0].item()       # its uncertainty grows
        assert at(t)["cov"][ref.DROP, 2].item() > at(t - 1)["cov"][ref.DROP, 2].item()
        assert abs(at(t)["state"][ref.DROP, 28:30].sum().item() - 1.0) < 1e-6
    assert at(d1 + 1)["status"][ref.DROP].item() == plain.UPDATED and at(d1 + 1)["state"][ref.DROP, 31].item() == 0
    t = ref.OUTLIER_FRAME
    assert at(t)["status"][ref.OUTLIER].item() == plain.COASTED_GATED and at(t + 1)["status"][ref.OUTLIER].item() == plain.UPDATED
    assert (at(t)["raw"][ref.OUTLIER] - at(t)["kp"][ref.OUTLIER]).abs().max().item() > 30.0
    g0 = ref.GONE_FRAMES[0]
    p = tracking()
    assert p.max_coast == 5 and len(ref.GONE_FRAMES) == 10
    assert status[g0 - first:g0 - first + 11, ref.GONE].tolist() == [plain.COASTED_MISSING] * 5 + [plain.LOST] * 5 + [plain.STARTED]
    assert at(g0 + 11)["status"][ref.GONE].item() == plain.UPDATED
    for t in range(g0 + 5, g0 + 10):
        o = at(t)
        assert not o["state"][ref.GONE].any().item() and torch.equal(o["kp"][ref.GONE], o["raw"][ref.GONE])
        assert torch.equal(o["fc"][ref.GONE], o["raw"][ref.GONE]) and o["moving"][ref.GONE].item() == 0.0
        assert not o["vel"][ref.GONE].any().item() and not o["cov"][ref.GONE].any().item()
    o = at(g0 + 10)
    assert torch.equal(o["kp"][ref.GONE], o["raw"][ref.GONE]) and not o["vel"][ref.GONE].any().item()
    assert o["state"][ref.GONE, 28:30].tolist() == [0.75, 0.25] and o["moving"][ref.GONE].item() == 0.25
    assert torch.equal(o["state"][ref.GONE, 0:14], o["state"][ref.GONE, 14:28])              # both models start from z
    for o in seq:
        assert o["status"][ref.NEVER].item() == plain.LOST and not o["state"][ref.NEVER].any().item()
        assert torch.equal(o["kp"][ref.NEVER], o["raw"][ref.NEVER]) and o["moving"][ref.NEVER].item() == 0.0


# ---- 5: presence flags -------------------------------------------------------------------------------------------------------------------------
def test_a_group_flagged_absent_has_no_measurement():
    """2 groups of 14 rows over the first 20 frames; group 1 is flagged absent in frames 6 .. 13: its rows coast for five frames with
    COASTED_MISSING, then are LOST, and start again when the flag returns; group 0 is bit-equal to a run without flags."""
    from hupr_amd import functional as F_
    heat = scenario_on_gpu().view(ref.T, 2, 14, ref.HM, ref.HM)
    p = tracking()
    s_flag, s_none = F_.pose_imm_state(ref.ROWS, "cuda"), F_.pose_imm_state(ref.ROWS, "cuda")
    absent = range(6, 14)
    usable_rows = [r for r in range(14, 28) if r != ref.NEVER and r != ref.GONE]
    for t in range(20):
        flags = torch.tensor([1, 0 if t in absent else 1], dtype=torch.int32, device="cuda")
        a = track(heat[t], ref.RATIO, s_flag, p, present=flags)
        b = track(heat[t], ref.RATIO, s_none, p)
        for k in OUT:
            assert a[k].shape == b[k].shape and torch.equal(a[k][0], b[k][0]), (t, k)
        assert torch.equal(s_flag[:14], s_none[:14]), t
        for k in ("idx", "maxval", "raw"):                                                 # the decode does not read the flags
            assert torch.equal(a[k], b[k]), (t, k)
        st = a["status"].view(-1)[usable_rows]
        if t in absent:
            want = plain.COASTED_MISSING if t - absent[0] < 5 else plain.LOST
            assert (st == want).all().item(), (t, st.tolist())
            if want == plain.LOST:
                assert not s_flag[14:].any().item() and not a["moving"][1].any().item()
                assert torch.equal(a["kp"][1], a["raw"][1])
        elif t == absent[-1] + 1:
            assert (st == plain.STARTED).all().item(), t
        elif t > 0:
            assert (st == plain.UPDATED).all().item(), (t, st.tolist())
    # flags of the wrong shape or type are refused before the launch
    for bad in (torch.ones(3, dtype=torch.int32, device="cuda"), torch.ones(2, dtype=torch.int64, device="cuda"),
                torch.ones(2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            track(heat[0], ref.RATIO, s_flag, p, present=bad)


# ---- 6: run to run -----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_identical_and_a_zeroed_state_starts_again():
    a, b = gpu_run(run=0, last=40), gpu_run(run=1, last=40)
    assert a is not b
    for t in range(40):
        for k in OUT + ("state",):
            assert torch.equal(a[t][k], b[t][k]), (t, k)
    state = a[-1]["state"].clone()
    assert state.any().item()
    state.zero_()
    o = track(scenario_on_gpu()[12], ref.RATIO, state, tracking())
    usable = o["maxval"] > ref.MIN_SCORE
    assert usable.sum().item() == ref.ROWS - 1
    assert torch.equal(o["status"], torch.where(usable, plain.STARTED, plain.LOST).to(torch.int32))
    assert torch.equal(o["kp"], o["raw"]) and not o["vel"].any().item()
    assert torch.equal(o["moving"], torch.where(usable, 0.5, 0.0).to(torch.float32))


# ---- 7: offline ------------------------------------------------------------------------------------------------------------------------------
def test_the_sequence_smoother_tracks_and_records_with_two_models():
    """``tools.SequenceSmoother`` over frames 36 .. 75: its nine outputs and its record are the kernel's own run, the mean ``moving``
    is over the live joints, a new sequence starts new tracks, and it refuses to smooth."""
    from hupr_amd.tools import SequenceSmoother, TrackingError
    first, last = 36, 76
    seq, p = gpu_run(first=first, last=last, moving_prior=0.25), tracking(moving_prior=0.25)
    s = SequenceSmoother(p, ref.ROWS, "cuda", measurements=True)
    heat = scenario_on_gpu()
    for t in range(first, last):
        out = s.track(heat[t], ref.RATIO)
        assert len(out) == 9
        for k, got in zip(OUT, out):
            assert torch.equal(got, seq[t - first][k]), (t, k)
    assert torch.equal(s.state, seq[-1]["state"]) and len(s) == last - first and len(s.record) == last - first
    rec = s.history.record()
    assert rec.keypoints is None and torch.equal(rec.filtered, torch.stack([o["kp"] for o in seq]))
    assert torch.equal(rec.status, torch.stack([o["status"] for o in seq])) and torch.equal(rec.raw, torch.stack([o["raw"] for o in seq]))
    status, moving = stacked(seq, "status"), stacked(seq, "moving")
    mean, n = s.history.moving_mean()
    assert n == int((status != plain.LOST).sum()) and abs(mean - moving[status != plain.LOST].astype(np.float64).mean()) < 1e-9
    with pytest.raises(TrackingError):
        s.smooth()
    s.new_sequence()
    assert not s.state.any().item()
    assert (s.track(heat[first], ref.RATIO)[7] == plain.STARTED).sum().item() == ref.ROWS - 1
