"""CPU (-m "not gpu"): the two-model (interacting-multiple-model) joint tracker without a launch — the argument checks at every layer
(C ABI through ctypes, ``PoseTracking``, ``functional.pose_track``, ``PoseStream``, ``SequenceSmoother``, ``TEST.tracking``, the
command line), the register / scratch metadata of csrc/pose_imm.hip, the rule's own worth on its fp64 restatement
(tests/pose_imm_ref.py) against single-model filters, and the fp32 restatement against the fp64 one, whose printed differences are the
basis of the bounds in tests/test_pose_imm_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import pose_imm_ref as ref
import pose_track_ref as plain
from listing import kernel_metadata


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


#       rate_hz, accel_psd, meas_std, heatmap_gain, gate, max_coast, init_speed_std, min_score, horizon_s
GOOD = (10.0, 5.0, 1.0, 1.0, 13.816, 5, 50.0, 0.0, 0.0)
NAMES = ("rate_hz", "accel_psd", "meas_std", "heatmap_gain", "gate", "max_coast", "init_speed_std", "min_score", "horizon_s")
MODEL = (5000.0, 0.05, 0.5)                                # accel_psd_moving, switch_prob, moving_prior
P = 4096                                                   # any non-null address: every call below returns before it launches
NAN, INF = float("nan"), float("inf")


def _call(L, heat=P, rows=14, state=P, params=GOOD, model=MODEL, present=None, group=1, outs=(P,) * 9, H=64, W=64):
    return L.hupr_pose_track_imm_f32(heat, rows, H, W, 4.0, 1, state, *params, *model, present, group, *outs, None)


def _with(**kw):
    return tuple(kw.get(k, v) for k, v in zip(NAMES, GOOD))


def test_entry_points_check_their_arguments_on_the_host(L):
    assert L.hupr_pose_track_imm_state_bytes(0) == 0 and L.hupr_pose_track_imm_state_bytes(-3) == 0
    assert L.hupr_pose_track_imm_state_bytes(1) == 128 and L.hupr_pose_track_imm_state_bytes(28) == 28 * 32 * 4
    # rows == 0 is a no-op whatever else is passed
    assert _call(L, None, 0, None, (0.0,) * 5 + (0,) + (0.0,) * 3, (NAN, 2.0, -1.0), outs=(None,) * 9) == 0
    # null pointers: the heat-maps, the state, each of the nine outputs
    assert _call(L, heat=None) == -1 and b"null" in L.hupr_last_error()
    assert _call(L, state=None) == -1 and b"null" in L.hupr_last_error()
    for k in range(9):
        assert _call(L, outs=tuple(None if j == k else P for j in range(9))) == -1, k
        assert b"null" in L.hupr_last_error()
    # shapes and alignment
    assert _call(L, rows=-1) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, rows=1 << 31) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, H=0) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, W=-2) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, H=1 << 16, W=1 << 16) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, state=P + 4) == -1 and b"aligned" in L.hupr_last_error()
    # the nine tracker parameters go through the tracker's own check
    for bad in (dict(rate_hz=0.0), dict(accel_psd=-1.0), dict(meas_std=NAN), dict(gate=INF), dict(max_coast=-1), dict(min_score=NAN)):
        assert _call(L, params=_with(**bad)) == -1 and b"tracker parameter" in L.hupr_last_error(), bad
    # presence flags: the group size divides the rows
    assert _call(L, present=P, group=0) == -1 and b"rows_per_group" in L.hupr_last_error()
    assert _call(L, present=P, group=4) == -1 and b"rows_per_group" in L.hupr_last_error()


@pytest.mark.parametrize("model", [(4.0, 0.05, 0.5), (NAN, 0.05, 0.5), (INF, 0.05, 0.5), (5000.0, -0.01, 0.5), (5000.0, 0.51, 0.5),
                                   (5000.0, NAN, 0.5), (5000.0, 0.05, -0.1), (5000.0, 0.05, 1.1), (5000.0, 0.05, NAN)],
                         ids=lambda m: "%g-%g-%g" % m)
def test_a_bad_model_parameter_is_refused(L, model):
    assert _call(L, model=model) == -1
    assert b"model parameter" in L.hupr_last_error()


def test_pose_tracking_validates_the_three_new_settings_and_is_unchanged_without_them():
    from hupr_amd import tools
    from hupr_amd.tools import stream as st
    s = st.PoseTracking(10)
    assert s.__slots__ == NAMES and st.PoseTracking.ARGUMENTS == NAMES + ("candidates", "min_separation", "peak_ratio", "gate_on_presence")
    assert st.PoseTracking.MANEUVER_ARGUMENTS == ("accel_psd_moving", "switch_prob", "moving_prior")
    assert (s.accel_psd_moving, s.switch_prob, s.moving_prior) == (None, 0.05, 0.5) and not s.maneuvers
    assert repr(s) == ("PoseTracking(rate_hz=10.0, accel_psd=200.0, meas_std=1.0, heatmap_gain=1.0, gate=13.816, max_coast=5, "
                       "init_speed_std=50.0, min_score=0.0, horizon_s=0.0, candidates=1, min_separation=3, peak_ratio=0.25, "
                       "gate_on_presence=False)")
    assert "moving" not in repr(st.PoseTracking(10, switch_prob=0.1, moving_prior=0.2))             # shown only when on
    with pytest.raises(AttributeError):
        s.extra = 1                                                              # still no __dict__
    m = st.PoseTracking(10, accel_psd=5, accel_psd_moving=5000, switch_prob=0.1, moving_prior=0.25, gate_on_presence=True)
    assert m.maneuvers and not m.associates and type(m.accel_psd_moving) is float
    assert repr(m).endswith("gate_on_presence=True, accel_psd_moving=5000.0, switch_prob=0.1, moving_prior=0.25)")
    assert "unmeasured" in st.PoseTracking.__doc__ and "too high" in st.PoseTracking.__doc__
    st.PoseTracking(10, accel_psd=200, accel_psd_moving=200, switch_prob=0, moving_prior=0)          # the edges are allowed
    st.PoseTracking(10, accel_psd_moving=1e4, switch_prob=0.5, moving_prior=1)
    for bad in (dict(accel_psd_moving=100.0), dict(accel_psd_moving=NAN), dict(accel_psd_moving=INF), dict(accel_psd_moving=True),
                dict(accel_psd_moving="5000"), dict(switch_prob=-0.01), dict(switch_prob=0.51), dict(switch_prob=NAN),
                dict(switch_prob=True), dict(switch_prob=None), dict(moving_prior=-0.1), dict(moving_prior=1.5), dict(moving_prior=NAN),
                dict(moving_prior=False), dict(accel_psd_moving=5000.0, candidates=2), dict(accel_psd_moving=5000.0, pair_swap=True)):
        with pytest.raises(st.TrackingError):
            st.PoseTracking(10, **bad)
    # the copies carry the new fields
    h = m.with_horizon(0.3)
    assert (h.horizon_s, h.accel_psd_moving, h.switch_prob, h.moving_prior, h.gate_on_presence) == (0.3, 5000.0, 0.1, 0.25, True)
    assert m.for_joints(["L_a", "R_a"]) is m
    c = m._copy(meas_std=2.0)
    assert (c.meas_std, c.accel_psd, c.accel_psd_moving) == (2.0, 5.0, 5000.0)
    assert tools.ManeuveringPoseFrame is st.ManeuveringPoseFrame


def test_the_new_frame_class_is_a_tracked_pose_frame_with_moving():
    from hupr_amd.tools.stream import ManeuveringPoseFrame, TrackedPoseFrame
    assert TrackedPoseFrame.__slots__ == ("covariance", "forecast", "status") and ManeuveringPoseFrame.__slots__ == ("moving",)
    t = [torch.full((1,), float(i)) for i in range(9)] + [torch.full((1,), 3, dtype=torch.int32)]
    pf = ManeuveringPoseFrame(5, *t, moving=torch.full((1,), 0.25))
    assert isinstance(pf, TrackedPoseFrame) and not hasattr(pf, "__dict__") and pf.chosen is None and pf.source is None
    for c in (pf.clone(), pf.cpu()):
        assert type(c) is ManeuveringPoseFrame and c.frame == 5 and c.moving.item() == 0.25 and torch.equal(c.status, t[9])
    assert pf.clone().moving is not pf.moving
    assert TrackedPoseFrame(5, *t).clone().lagged is None and not hasattr(TrackedPoseFrame(5, *t), "moving")


def test_functional_pose_track_validates_the_two_model_state_and_refuses_cpu_tensors(L):
    from hupr_amd import functional as F_
    from hupr_amd.runtime import HuprError
    from hupr_amd.tools import PoseTracking
    heat, tr = torch.zeros((2, 8, 8)), PoseTracking(10.0, accel_psd=5.0, accel_psd_moving=5000.0)
    state = F_.pose_imm_state(2, "cpu")
    assert state.shape == (2, 32) and state.dtype == torch.float32 and not state.any().item()
    with pytest.raises(ValueError, match="pose_imm_state"):
        F_.pose_track(heat, 4.0, track_state=F_.pose_track_state(2, "cpu"), tracking=tr)           # the plain tracker's state
    with pytest.raises(ValueError, match="pose_track_state"):
        F_.pose_track(heat, 4.0, track_state=state, tracking=PoseTracking(10.0))                 # and the other way round
    with pytest.raises(ValueError):
        F_.pose_track(heat, 4.0, track_state=torch.zeros((3, 32)), tracking=tr)
    with pytest.raises(ValueError):
        F_.pose_track(heat, 4.0, track_state=state.double(), tracking=tr)
    with pytest.raises(ValueError):
        F_.pose_track(heat, 4.0, track_state=state, tracking=tr, out=(None,) * 8)                # out is the 9-tuple
    with pytest.raises(ValueError, match="present"):
        F_.pose_track(heat, 4.0, track_state=state, tracking=tr, present=torch.zeros(2, dtype=torch.int32))   # one flag per group: shape ()

    class Both:                                                                  # an object that asks for both: refused here too
        rate_hz, accel_psd, meas_std, heatmap_gain, gate, max_coast, init_speed_std, min_score, horizon_s = GOOD
        accel_psd_moving, switch_prob, moving_prior, candidates = 5000.0, 0.05, 0.5, 2
    with pytest.raises(ValueError, match="candidates"):
        F_.pose_track(heat, 4.0, track_state=state, tracking=Both)
    with pytest.raises(HuprError):                                               # no CPU fallback
        F_.pose_track(heat, 4.0, track_state=state, tracking=tr)
    with pytest.raises(HuprError):
        F_.pose_track(heat, 4.0, track_state=state, tracking=tr, present=torch.ones((), dtype=torch.int32))


def test_the_refused_combinations():
    from hupr_amd import tools
    from hupr_amd.config_tree import load_config
    from hupr_amd.runtime import HuprError
    from hupr_amd.tools import smooth as sm

    class _Cpu(torch.nn.Module):
        math_mode, numFilters = None, 32

        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    cfg = load_config()
    imm = tools.PoseTracking(10.0, accel_psd=5.0, accel_psd_moving=5000.0)
    with pytest.raises(tools.TrackingError, match="lag"):
        tools.PoseStream(_Cpu(), cfg, track=imm, lag=4)
    with pytest.raises(tools.TrackingError, match="history"):
        tools.PoseStream(_Cpu(), cfg, track=imm, history=True)
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, track=imm, smooth=tools.PoseSmoothing(10.0))
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, accel_psd_moving=5000.0, gate_on_presence=True))   # needs presence
    for ok in (dict(), dict(measurements=True), dict(predict_now=True), dict(decode="subpixel")):
        with pytest.raises(HuprError):                                           # valid arguments reach the GPU check
            tools.PoseStream(_Cpu(), cfg, track=imm, **ok)
    # offline: the smoother tracks and records, and refuses to smooth
    with pytest.raises(tools.TrackingError, match="lag"):
        tools.SequenceSmoother(imm, 14, "cpu", lag=4)
    s = tools.SequenceSmoother(imm, 14, "cpu")
    assert s.state.shape == (14, 32) and isinstance(s.history, sm.ManeuverHistory)
    with pytest.raises(tools.TrackingError):
        s.smooth()
    with pytest.raises(tools.TrackingError):
        s.smooth_lagged()
    assert tools.SequenceSmoother(tools.PoseTracking(10.0), 14, "cpu").state.shape == (14, 16)
    # the history of the two-model tracker: what it records, and the mean probability over live joints
    h = sm.ManeuverHistory((3,), "cpu")
    status = torch.tensor([plain.UPDATED, plain.LOST, plain.STARTED], dtype=torch.int32)
    h.append(None, status, torch.ones(3, 2), torch.zeros(3, 2), torch.full((3,), 0.5), torch.tensor([0.25, 0.0, 0.75]))
    rec = h.record()
    assert len(h) == 1 and torch.equal(rec.status[0], status) and rec.keypoints is None and h.moving_mean() == (0.5, 2)


def _cfg(**test):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in test.items():
        setattr(cfg.TEST, k, v)
    return cfg


def test_test_tracking_accepts_the_three_keys_and_refuses_the_smoothers():
    from hupr_amd.tools.smooth import temporal_setting
    keys = dict(accel_psd=5.0, accel_psd_moving=5000.0, switch_prob=0.1, moving_prior=0.3)
    s = temporal_setting(_cfg(temporal="track", tracking=keys))
    assert s.mode == "track" and (s.tracking.accel_psd_moving, s.tracking.switch_prob, s.tracking.moving_prior) == (5000.0, 0.1, 0.3)
    assert temporal_setting(_cfg(temporal="off", tracking=keys)) is None
    for mode in ("rts", "lag"):
        with pytest.raises(ValueError, match="accel_psd_moving"):
            temporal_setting(_cfg(temporal=mode, tracking=keys))
    with pytest.raises(ValueError, match="accel_psd_moving"):
        temporal_setting(_cfg(temporal="track", tracking=dict(accel_psd_moving=100.0)))            # below the default accel_psd
    with pytest.raises(ValueError):
        temporal_setting(_cfg(temporal="track", tracking=dict(accel_psd_moving=5000.0, candidates=2)))
    assert not temporal_setting(_cfg(temporal="rts", tracking=dict(switch_prob=0.1))).tracking.maneuvers   # off: as ever


def test_the_fit_leaves_both_acceleration_psds_alone():
    """``tools.calibrate.search`` on a two-model ``PoseTracking``: the single-model fit runs as ever, meas_std and heatmap_gain are
    carried over, accel_psd and accel_psd_moving stay the user's — also where the fitted accel_psd would exceed accel_psd_moving."""
    from hupr_amd.tools import PoseTracking, calibrate

    def evaluate(grid):                                                          # the best candidate: the largest of everything
        costs = -grid.sum(axis=1)
        counts = np.tile(np.array([5, 0, 0, 1, 0, 5]), (grid.shape[0], 1))
        return costs, counts, int(np.argmin(costs))

    fit = calibrate.search(evaluate, PoseTracking(10.0, accel_psd=5.0, accel_psd_moving=50.0), rounds=1)
    assert (fit.tracking.accel_psd, fit.tracking.accel_psd_moving) == (5.0, 50.0)
    assert fit.tracking.meas_std > 1.0 and fit.tracking.heatmap_gain > 1.0
    assert calibrate.search(evaluate, PoseTracking(10.0, accel_psd=5.0), rounds=1).tracking.accel_psd > 5.0    # without: fitted as ever


def test_stream_command_two_model_arguments():
    from hupr_amd.tools import stream as st
    t = st.tracking_from_args(st.parse(["--raw", "x", "--track", "--rate", "10"]))
    assert t.accel_psd_moving is None and not t.maneuvers
    a = st.parse(["--raw", "x", "--track", "--rate", "10", "--accel-psd", "5", "--track-moving-psd", "5000", "--track-switch-prob", "0.1",
                  "--track-moving-prior", "0.3", "--fit-tracker"])
    t = st.tracking_from_args(a)
    assert (t.accel_psd, t.accel_psd_moving, t.switch_prob, t.moving_prior) == (5.0, 5000.0, 0.1, 0.3)
    t = st.tracking_from_args(st.parse(["--raw", "x", "--track", "--rate", "10", "--track-moving-psd", "5000"]))
    assert (t.accel_psd_moving, t.switch_prob, t.moving_prior) == (5000.0, 0.05, 0.5)
    tr = ["--track", "--rate", "10"]
    for bad in (["--track-moving-psd", "5000"], tr + ["--track-switch-prob", "0.1"], tr + ["--track-moving-prior", "0.3"],
                tr + ["--track-moving-psd", "100"], tr + ["--track-moving-psd", "5000", "--track-switch-prob", "0.6"],
                tr + ["--track-moving-psd", "5000", "--track-moving-prior", "2"], tr + ["--track-moving-psd", "5000", "--rts"],
                tr + ["--track-moving-psd", "5000", "--track-lag", "4"], tr + ["--track-moving-psd", "5000", "--track-candidates", "2"],
                tr + ["--track-moving-psd", "5000", "--track-pairs"]):
        with pytest.raises(SystemExit):
            st.parse(["--raw", "x"] + bad)


def test_pose_imm_kernel_uses_no_scratch():
    """The listing the build keeps for csrc/pose_imm.hip: its one kernel, 64 threads, with 0 spilled registers, 0 bytes of scratch and
    no LDS — read from the code-object metadata only."""
    meta = kernel_metadata("pose_imm")
    assert len(meta) == 1 and "hupr_k_pose_track_imm" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    print(m)
    assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, m
    assert m["threads"] == 64, m


# ---- the claim, on the fp64 rule ---------------------------------------------------------------------------------------------------------
SEEDS = (3, 4, 5)
SINGLE_PSD = (200.0, 500.0, 1000.0, 2000.0, 3000.0, 5000.0, 10000.0)
SETTINGS = dict(accel_psd=5.0, meas_std=3.0, heatmap_gain=0.0, min_score=ref.MIN_SCORE)
MODELS = dict(accel_psd_moving=5000.0, switch_prob=0.05)


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(SETTINGS, **kw))


@functools.lru_cache(maxsize=None)
def imm64(seed, events=True):
    _, _, measured, _ = ref.stop_and_go(seed, events)
    _, mx, mom = ref.stop_and_go_moments(seed, events)
    return ref.ref_imm(measured, mx, mom, tracking(**MODELS), ref.RATIO)


def test_two_models_beat_every_single_model_on_joints_that_stop_and_go():
    """The fp64 restatement on the stop-and-go scenario (120 frames x 28 joints at 10 Hz, 3-pixel measurement noise), rows without
    events, seeds 3, 4 and 5, accel_psd = 5, accel_psd_moving = 5000, switch_prob = 0.05, meas_std = 3, heatmap_gain = 0; the decode is
    stood in for by the noisy position each map was drawn at, as in tests/test_pose_track_cpu.py.  On every seed: the two-model
    tracker's rms error is below that of every single-model run with accel_psd in {200 .. 10000}; its mean step from frame to frame
    while the joint is still is below that of the best-rms single filter; and the moving model is more probable during a reach than at
    rest.  Orderings only; the printed numbers are PAPERS.md's table."""
    rms = lambda a: float(np.sqrt(np.mean(np.sum(a ** 2, axis=-1))))
    N = list(ref.NORMAL)
    for seed in SEEDS:
        _, truth, measured, moving = ref.stop_and_go(seed)
        _, mx, mom = ref.stop_and_go_moments(seed)
        still = (~moving[1:] & ~moving[:-1])[:, N]
        step = lambda kp: float(np.mean(np.linalg.norm(kp[1:] - kp[:-1], axis=-1)[:, N][still]))
        o = imm64(seed)
        e_imm, s_imm = rms((o["kp"] - truth)[:, N]), step(o["kp"])
        mv, st = float(o["moving"][:, N][moving[:, N]].mean()), float(o["moving"][:, N][~moving[:, N]].mean())
        singles = {}
        for q in SINGLE_PSD:
            s = plain.ref_track(measured, mx, mom, tracking(accel_psd=q), ref.RATIO)
            singles[q] = (rms((s["kp"] - truth)[:, N]), step(s["kp"]), int((s["status"][:, N] == plain.COASTED_GATED).sum()))
        best = min(singles, key=lambda q: singles[q][0])
        print("seed %d: two models rms %.3f px, still step %.3f px, gated %d, moving %.3f in a reach / %.3f at rest; raw rms %.3f px"
              % (seed, e_imm, s_imm, int((o["status"][:, N] == plain.COASTED_GATED).sum()), mv, st, rms((measured - truth)[:, N])))
        print("        single model: " + "; ".join("psd %g rms %.3f step %.3f gated %d" % ((q,) + singles[q]) for q in SINGLE_PSD))
        print("        best single psd %g: rms ratio %.3f" % (best, e_imm / singles[best][0]))
        for q in SINGLE_PSD:
            assert e_imm < singles[q][0], (seed, q)
        assert s_imm < singles[best][1], seed
        assert mv > st, seed


def test_the_scenario_has_its_events_and_the_rule_handles_them():
    maps, truth, measured, moving = ref.stop_and_go()
    assert maps.shape == (ref.T, ref.ROWS, 64, 64) and maps.dtype == np.float32 and moving.dtype == bool
    assert 0.2 < moving[:, list(ref.NORMAL)].mean() < 0.6 and truth.min() >= 20.0 and truth.max() <= 236.0
    o = imm64(ref.SEED)
    s = o["status"]
    assert (s[list(ref.DROP_FRAMES), ref.DROP] == plain.COASTED_MISSING).all() and s[ref.DROP_FRAMES[-1] + 1, ref.DROP] == plain.UPDATED
    assert s[ref.OUTLIER_FRAME, ref.OUTLIER] == plain.COASTED_GATED and s[ref.OUTLIER_FRAME + 1, ref.OUTLIER] == plain.UPDATED
    g0 = ref.GONE_FRAMES[0]
    assert s[g0:g0 + 11, ref.GONE].tolist() == [plain.COASTED_MISSING] * 5 + [plain.LOST] * 5 + [plain.STARTED]
    assert o["moving"][g0 + 10, ref.GONE] == 0.5 and not o["moving"][g0 + 5:g0 + 10, ref.GONE].any()
    assert (s[:, ref.NEVER] == plain.LOST).all() and not o["state"][ref.NEVER].any() and not o["moving"][:, ref.NEVER].any()
    assert o["state"].shape == (ref.ROWS, ref.FLOATS)
    assert np.allclose(o["state"][list(ref.NORMAL), 28] + o["state"][list(ref.NORMAL), 29], 1.0, atol=1e-12)


def test_with_no_switching_and_no_prior_the_rule_is_the_plain_tracker():
    """switch_prob = 0 and moving_prior = 0: model 1 never has a say, and the fp64 rule gives the plain tracker's outputs exactly."""
    _, _, measured, _ = ref.stop_and_go()
    _, mx, mom = ref.stop_and_go_moments()
    p = tracking(accel_psd=100.0, accel_psd_moving=5000.0, switch_prob=0.0, moving_prior=0.0, horizon_s=0.3)
    a, b = ref.ref_imm(measured, mx, mom, p, ref.RATIO), plain.ref_track(measured, mx, mom, p, ref.RATIO)
    for k in ("kp", "vel", "cov", "fc", "status"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["state"][:, :14], b["state"][:, :14]) and np.array_equal(a["state"][:, 30:], b["state"][:, 14:])
    assert not a["moving"].any()


def test_the_fp32_restatement_agrees_with_the_fp64_one():
    """Where the covariance and ``moving`` bounds of tests/test_pose_imm_gpu.py come from: the restatement run in NumPy fp32 (window
    moments included) against its fp64 run on the stop-and-go scenario with its events, seed 3.  Measured here: positions 6.9e-5
    pixel, velocity 2.5e-4 pixel / s, covariance 1.39e-5 relative to the larger variance, moving 7.06e-6; the GPU test allows
    covariance and moving 16 x that.  This test prints the figures and holds them to the order of magnitude recorded there."""
    p = tracking(horizon_s=0.3, **MODELS)
    _, _, measured, _ = ref.stop_and_go()
    _, mx, mom = ref.stop_and_go_moments()
    _, _, mom32 = ref.stop_and_go_moments(dtype=np.float32)
    o64 = ref.ref_imm(measured, mx, mom, p, ref.RATIO)
    o32 = ref.ref_imm(measured.astype(np.float32), mx, mom32, p, ref.RATIO, np.float32)
    assert o32["kp"].dtype == np.float32 and o32["moving"].dtype == np.float32
    margin = ref.rel_gate_margin(o64["d2"], p.gate)
    e_kp, e_vel = np.abs(o32["kp"] - o64["kp"]).max(), np.abs(o32["vel"] - o64["vel"]).max()
    e_cov, e_mov = plain.cov_rel_diff(o32["cov"], o64["cov"]), np.abs(o32["moving"] - o64["moving"]).max()
    print("fp32 vs fp64 restatement: positions %.3e px, velocity %.3e px/s, covariance %.3e relative, moving %.3e; closest decision "
          "%.2f %% from the gate" % (e_kp, e_vel, e_cov, e_mov, 100 * margin))
    assert margin > 0.01                                                         # no decision near the gate: fp32 may not differ
    assert np.array_equal(o32["status"], o64["status"])
    assert e_kp < 2e-3 and e_vel < 2e-2
    assert COV_REL_FP32 / 4 <= e_cov <= COV_REL_FP32 * 4
    assert MOVING_FP32 / 4 <= e_mov <= MOVING_FP32 * 4


COV_REL_FP32, MOVING_FP32 = 1.39e-5, 7.06e-6                                     # tests/test_pose_imm_gpu.py holds the same two
