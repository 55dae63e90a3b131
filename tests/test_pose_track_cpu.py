"""CPU (-m "not gpu"): the argument checks of the Kalman joint tracker at every layer (C ABI through ctypes, ``PoseTracking``,
``functional.pose_track``, ``PoseStream``, the command line), ``TrackedPoseFrame``, the register / scratch metadata of
csrc/pose_track.hip, and the rule's own worth on its fp64 restatement (tests/pose_track_ref.py).  No launch."""

import numpy as np
import pytest
import torch

import pose_track_ref as ref
from listing import kernel_metadata


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


#       rate_hz, accel_psd, meas_std, heatmap_gain, gate, max_coast, init_speed_std, min_score, horizon_s
GOOD = (10.0, 200.0, 1.0, 1.0, 13.816, 5, 50.0, 0.0, 0.0)
NAMES = ("rate_hz", "accel_psd", "meas_std", "heatmap_gain", "gate", "max_coast", "init_speed_std", "min_score", "horizon_s")
P = 4096                                                   # any non-null address: every call below returns before it launches


def _call(L, heat=P, rows=14, state=P, params=GOOD, outs=(P,) * 8, H=64, W=64):
    return L.hupr_pose_track_f32(heat, rows, H, W, 4.0, 1, state, *params, *outs, None)


def _with(**kw):
    return tuple(kw.get(k, v) for k, v in zip(NAMES, GOOD))


def test_entry_points_check_their_arguments_on_the_host(L):
    assert L.hupr_pose_track_state_bytes(0) == 0 and L.hupr_pose_track_state_bytes(-3) == 0
    assert L.hupr_pose_track_state_bytes(1) == 64 and L.hupr_pose_track_state_bytes(28) == 28 * 16 * 4
    # rows == 0 is a no-op whatever else is passed
    assert _call(L, None, 0, None, (0.0,) * 5 + (0,) + (0.0,) * 3, (None,) * 8) == 0
    assert _call(L, None, 0, P, _with(rate_hz=-1.0, max_coast=-1), (None,) * 8) == 0
    # null pointers: the heat-maps, the state, each of the eight outputs
    assert _call(L, heat=None) == -1 and b"null" in L.hupr_last_error()
    assert _call(L, state=None) == -1 and b"null" in L.hupr_last_error()
    for k in range(8):
        assert _call(L, outs=tuple(None if j == k else P for j in range(8))) == -1, k
        assert b"null" in L.hupr_last_error()
    # shapes
    assert _call(L, rows=-1) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, rows=1 << 31) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, H=0) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, W=-2) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, H=1 << 16, W=1 << 16) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, state=P + 4) == -1 and b"aligned" in L.hupr_last_error()


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("bad", [dict(rate_hz=0.0), dict(rate_hz=-10.0), dict(rate_hz=NAN), dict(rate_hz=INF), dict(accel_psd=-1.0),
                                 dict(accel_psd=NAN), dict(accel_psd=INF), dict(meas_std=0.0), dict(meas_std=-1.0), dict(meas_std=NAN),
                                 dict(meas_std=INF), dict(heatmap_gain=-0.5), dict(heatmap_gain=NAN), dict(heatmap_gain=INF),
                                 dict(gate=0.0), dict(gate=-1.0), dict(gate=NAN), dict(gate=INF), dict(max_coast=-1),
                                 dict(init_speed_std=0.0), dict(init_speed_std=-5.0), dict(init_speed_std=NAN),
                                 dict(init_speed_std=INF), dict(min_score=NAN), dict(horizon_s=-0.1), dict(horizon_s=NAN),
                                 dict(horizon_s=INF)], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_a_bad_tracker_parameter_is_refused(L, bad):
    assert _call(L, params=_with(**bad)) == -1
    assert b"tracker parameter" in L.hupr_last_error()


def test_pose_tracking_validates_on_the_host():
    from hupr_amd import tools
    from hupr_amd.tools import stream as st
    assert tools.PoseTracking is st.PoseTracking and tools.TrackingError is st.TrackingError
    assert tools.TrackedPoseFrame is st.TrackedPoseFrame
    assert issubclass(st.TrackingError, st.StreamError)
    s = st.PoseTracking(10)
    assert tuple(getattr(s, k) for k in NAMES) == GOOD and s.__slots__ == NAMES
    assert all(isinstance(getattr(s, k), float) for k in NAMES if k != "max_coast") and type(s.max_coast) is int
    assert repr(s).startswith("PoseTracking(rate_hz=10.0, accel_psd=200.0,") and "max_coast=5" in repr(s)
    with pytest.raises(AttributeError):
        s.extra = 1                                                              # __slots__
    st.PoseTracking(30.0, accel_psd=0, meas_std=0.5, heatmap_gain=0.0, gate=9.21, max_coast=0, init_speed_std=10, min_score=-1.0,
                    horizon_s=0.3)
    assert st.PoseTracking(10, max_coast=np.int64(3)).max_coast == 3
    # the list of PoseSmoothing's test, on this class's parameters
    for bad in (dict(rate_hz=0), dict(rate_hz=-10.0), dict(rate_hz=NAN), dict(rate_hz=INF), dict(rate_hz="10"), dict(rate_hz=None),
                dict(rate_hz=True), dict(rate_hz=10, meas_std=0.0), dict(rate_hz=10, meas_std=-1.0), dict(rate_hz=10, accel_psd=-1e-3),
                dict(rate_hz=10, init_speed_std=0), dict(rate_hz=10, init_speed_std=NAN), dict(rate_hz=10, min_score=NAN),
                dict(rate_hz=10, min_score="0"),
                # and its own
                dict(rate_hz=10, max_coast=-1), dict(rate_hz=10, max_coast=1.5), dict(rate_hz=10, gate=0), dict(rate_hz=10, gate=-1.0),
                dict(rate_hz=10, max_coast=True), dict(rate_hz=10, max_coast=None), dict(rate_hz=10, heatmap_gain=-1.0),
                dict(rate_hz=10, heatmap_gain=INF), dict(rate_hz=10, horizon_s=-0.1), dict(rate_hz=10, horizon_s=NAN)):
        with pytest.raises(st.TrackingError):
            st.PoseTracking(**bad)


def test_functional_pose_track_refuses_bad_arguments_and_cpu_tensors(L):
    from hupr_amd import functional as F_
    from hupr_amd.runtime import HuprError
    from hupr_amd.tools import PoseTracking
    heat, tr = torch.zeros((2, 8, 8)), PoseTracking(10.0)
    state = F_.pose_track_state(2, "cpu")
    assert state.shape == (2, 16) and state.dtype == torch.float32 and not state.any().item()
    with pytest.raises(ValueError):
        F_.pose_track(torch.zeros(8), 4.0, track_state=state, tracking=tr)
    with pytest.raises(ValueError):
        F_.pose_track(heat.double(), 4.0, track_state=state, tracking=tr)
    with pytest.raises(ValueError):
        F_.pose_track(heat, 4.0, tracking=tr)                                    # the state is required
    with pytest.raises(ValueError):
        F_.pose_track(heat, 4.0, track_state=state)                              # and so are the parameters
    with pytest.raises(ValueError):
        F_.pose_track(heat, 4.0, track_state=torch.zeros((3, 16)), tracking=tr)
    with pytest.raises(ValueError):
        F_.pose_track(heat, 4.0, track_state=torch.zeros((2, 8)), tracking=tr)   # a One-Euro state
    with pytest.raises(ValueError):
        F_.pose_track(heat, 4.0, track_state=state.double(), tracking=tr)
    with pytest.raises(HuprError):                                               # no CPU fallback
        F_.pose_track(heat, 4.0, track_state=state, tracking=tr)


def test_session_argument_errors_come_before_the_gpu_check():
    from hupr_amd import tools
    from hupr_amd.config_tree import load_config
    from hupr_amd.runtime import HuprError

    class _Cpu(torch.nn.Module):
        math_mode, numFilters = None, 32

        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    cfg = load_config()
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, track=10.0)
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseSmoothing(10.0))
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0), smooth=tools.PoseSmoothing(10.0))
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, predict_now=True)
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, smooth=tools.PoseSmoothing(10.0), predict_now=True)
    with pytest.raises(tools.StreamError):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, gate=0))    # raised by PoseTracking itself
    with pytest.raises(HuprError):                                               # valid arguments reach the GPU check
        tools.PoseStream(_Cpu(), cfg, decode="subpixel", track=tools.PoseTracking(10.0), predict_now=True)
    with pytest.raises(HuprError):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, horizon_s=0.3))


def test_tracked_pose_frame_is_a_pose_frame_with_three_more_fields():
    from hupr_amd.tools.stream import PoseFrame, TrackedPoseFrame
    assert PoseFrame.__slots__ == ("frame", "keypoints", "scores", "indices", "heatmap", "gcn_heatmap", "raw_keypoints", "velocity")
    assert TrackedPoseFrame.__slots__ == ("covariance", "forecast", "status") and issubclass(TrackedPoseFrame, PoseFrame)
    t = [torch.full((1,), float(i)) for i in range(9)] + [torch.full((1,), 3, dtype=torch.int32)]
    pf = TrackedPoseFrame(5, *t)
    assert isinstance(pf, PoseFrame) and not hasattr(pf, "__dict__")
    assert pf.raw_keypoints is t[5] and pf.velocity is t[6] and pf.covariance is t[7] and pf.forecast is t[8] and pf.status is t[9]
    for c in (pf.clone(), pf.cpu()):
        assert type(c) is TrackedPoseFrame and c.frame == 5
        for k, want in zip(PoseFrame.__slots__[1:] + TrackedPoseFrame.__slots__, t):
            assert torch.equal(getattr(c, k), want) and getattr(c, k).dtype == want.dtype, k
    assert pf.clone().covariance is not pf.covariance
    assert TrackedPoseFrame.STATUS[ref.LOST] == "LOST" and TrackedPoseFrame.STATUS[ref.UPDATED] == "UPDATED"
    # the base class still constructs positionally, without the new fields
    assert type(PoseFrame(3, *t[:7]).clone()) is PoseFrame
    # cpu() and clone() round-trip every field of the class, whatever base class declares it, None included
    fields = [k for c in TrackedPoseFrame.__mro__ for k in getattr(c, "__slots__", ())]
    assert sorted(fields) == sorted(PoseFrame.__slots__ + TrackedPoseFrame.__slots__ + ("present", "occupancy", "interference", "candidates",
                                                                                        "candidate_scores", "candidate_count", "chosen"))
    full = TrackedPoseFrame(7, *t, present=torch.ones(1, dtype=torch.int32), occupancy=torch.full((1, 8), 2.0),
                            candidates=torch.full((1, 2, 2), 7.0), candidate_scores=torch.full((1, 2), 8.0),
                            candidate_count=torch.full((1,), 2, dtype=torch.int32), chosen=torch.full((1,), -1, dtype=torch.int32),
                            interference=torch.full((2, 1, 2), 9, dtype=torch.int32))
    for src in (pf, full):
        for c in (src.cpu(), src.clone()):
            assert type(c) is TrackedPoseFrame and c.frame == src.frame
            for k in fields:
                a, b = getattr(src, k), getattr(c, k)
                assert a == b if k == "frame" else (a is None and b is None) or (torch.equal(a, b) and a.dtype == b.dtype), k
    assert pf.cpu().chosen is None and pf.cpu().interference is None and full.cpu().chosen is not None


def test_stream_command_tracking_arguments():
    from hupr_amd.tools import stream as st
    a = st.parse(["--raw", "x"])
    assert not a.track and not a.predict_now and st.tracking_from_args(a) is None
    a = st.parse(["--raw", "x", "--decode", "subpixel", "--track", "--rate", "10", "--predict-now", "--accel-psd", "100", "--gate", "9.21",
                  "--max-coast", "3", "--lookahead", "2"])
    assert a.track and a.predict_now and a.rate == 10.0 and a.decode == "subpixel"
    t = st.tracking_from_args(a)
    assert (t.rate_hz, t.accel_psd, t.gate, t.max_coast, t.meas_std) == (10.0, 100.0, 9.21, 3, 1.0)
    t = st.tracking_from_args(st.parse(["--raw", "x", "--track", "--rate", "25"]))
    assert tuple(getattr(t, k) for k in NAMES) == (25.0,) + GOOD[1:]
    for bad in (["--track"], ["--track", "--smooth", "--rate", "10"], ["--predict-now"], ["--predict-now", "--smooth", "--rate", "10"],
                ["--accel-psd", "100"], ["--gate", "9"], ["--max-coast", "2"], ["--track", "--rate", "10", "--max-coast", "1.5"]):
        with pytest.raises(SystemExit):
            st.parse(["--raw", "x"] + bad)


def test_pose_track_kernel_uses_no_scratch():
    """The listing the build keeps for csrc/pose_track.hip: its one kernel, 64 threads, with 0 spilled registers, 0 bytes of scratch
    and no LDS — read from the code-object metadata only."""
    meta = kernel_metadata("pose_track")
    assert len(meta) == 1 and "hupr_k_pose_track" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    print(m)
    assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, m
    assert m["threads"] == 64, m


def test_the_rule_beats_the_raw_keypoints_and_its_forecast_beats_holding():
    """The fp64 restatement on the scenario without its drop-outs and outlier (60 frames x 28 joints at 10 Hz, 3-pixel measurement
    noise, accel_psd = 100): the filtered keypoints are closer to the truth than the raw ones, and the forecast 0.3 s ahead is closer
    to the truth 0.3 s later than the held filtered position and than the raw keypoint.  The decode is stood in for by the noisy
    position each map was drawn at (the sub-pixel decode recovers a Gaussian's centre to 1e-3 pixel, tests/test_pose_decode_gpu.py)."""
    from hupr_amd.tools import PoseTracking
    p = PoseTracking(ref.RATE, accel_psd=100.0, min_score=ref.MIN_SCORE, horizon_s=0.3)
    _, truth, measured = ref.scenario(events=False)
    _, mx, mom = ref.scenario_moments(events=False)
    o = ref.ref_track(measured, mx, mom, p, ref.RATIO)
    assert (o["status"][0] == ref.STARTED).all() and (o["status"][1:] == ref.UPDATED).all()
    rms = lambda a: float(np.sqrt(np.mean(np.sum(a ** 2, axis=-1))))
    ahead = int(round(0.3 * ref.RATE))
    filtered, raw = rms(o["kp"] - truth), rms(measured - truth)
    forecast, held, raw_held = rms(o["fc"][:-ahead] - truth[ahead:]), rms(o["kp"][:-ahead] - truth[ahead:]), rms(measured[:-ahead] - truth[ahead:])
    print("RMS error in pixels: filtered %.2f, raw %.2f; 0.3 s ahead: forecast %.2f, held filtered %.2f, raw %.2f"
          % (filtered, raw, forecast, held, raw_held))
    assert filtered < raw
    assert forecast < held and forecast < raw_held


def test_the_fp32_restatement_agrees_with_the_fp64_one():
    """Where the covariance bound of tests/test_pose_track_gpu.py comes from: the restatement run in NumPy fp32 (window moments
    included) against its fp64 run on the scenario with its events.  Measured here: positions 3.8e-5 pixel, velocity 7.1e-5 pixel / s,
    covariance 3.02e-7 relative to the larger variance; the GPU test allows the covariance 16 x that.  This test prints the figures
    and holds them to the order of magnitude recorded there."""
    from hupr_amd.tools import PoseTracking
    p = PoseTracking(ref.RATE, accel_psd=100.0, min_score=ref.MIN_SCORE, horizon_s=0.3)
    _, _, measured = ref.scenario()
    _, mx, mom = ref.scenario_moments()
    _, _, mom32 = ref.scenario_moments(dtype=np.float32)
    o64 = ref.ref_track(measured, mx, mom, p, ref.RATIO)
    o32 = ref.ref_track(measured.astype(np.float32), mx, mom32, p, ref.RATIO, np.float32)
    d2 = o64["d2"][o64["usable"] & np.isfinite(o64["d2"])]
    e_kp, e_vel, e_cov = np.abs(o32["kp"] - o64["kp"]).max(), np.abs(o32["vel"] - o64["vel"]).max(), ref.cov_rel_diff(o32["cov"], o64["cov"])
    print("fp32 vs fp64 restatement: positions %.3e px, velocity %.3e px/s, covariance %.3e relative; d2 accepted <= %.3f, refused >= %.3f"
          % (e_kp, e_vel, e_cov, d2[d2 <= p.gate].max(), d2[d2 > p.gate].min()))
    assert (np.abs(d2 / p.gate - 1.0) > 0.01).all()                              # no decision near the gate: fp32 may not differ
    assert np.array_equal(o32["status"], o64["status"])
    assert e_kp < 2e-3 and e_vel < 2e-2
    assert 3.02e-7 / 4 <= e_cov <= 3.02e-7 * 4
    for r, want in ((ref.DROP, ref.COASTED_MISSING), (ref.GONE, ref.COASTED_MISSING), (ref.OUTLIER, ref.COASTED_GATED)):
        assert (o64["status"][:, r] == want).any()
    assert (o64["status"][:, ref.NEVER] == ref.LOST).all() and not o64["state"][ref.NEVER].any()
