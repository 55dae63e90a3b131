"""CPU: the fixed-lag smoother's rule (include/hupr.h, hupr_pose_smooth_lag_f32) as restated in tests/pose_lag_ref.py — what a lag of L
frames buys on the tracker tests' scenario (60 frames x 28 rows at 10 Hz, seed 11; the table of PAPERS.md is printed here), that it is
the fixed-interval pass cut short, and the NumPy fp32 vs fp64 differences that set the bounds of tests/test_pose_lag_gpu.py — and the
host logic around it: TEST.temporal: lag / temporalLag, --track-lag, PoseStream(lag=...), functional.pose_smooth_lag's checks, the
kernel's listing.

Tracker parameters of these tests (pose_smooth_ref.params): PoseTracking's defaults with accel_psd = 200, min_score = 0.1, arg-max
measurements."""
import types

import numpy as np
import pytest

import pose_lag_ref as lr
import pose_smooth_ref as sr
import pose_track_ref as ref
from listing import kernel_metadata

LAGS = (1, 2, 3, 4, 6, 8)


def test_every_frame_of_lag_buys_position_error_on_the_scenario():
    track, _, smooth, _ = sr.scenario_run()
    truth, N = ref.scenario()[1], sr.NORMAL
    assert len(N) == 24
    err = lambda kp: sr.rms(kp - truth[:, N])
    jit = lambda kp: sr.rms(sr.second_difference(kp))
    e_f, j_f = err(track["kp"][:, N]), jit(track["kp"][:, N])
    e, j = {}, {}
    print("| lag L (frames) | rms error | share of the filter's | jitter (rms 2nd difference) |")
    print("| 0 = the filter | %.3f | 1.000 | %.3f |" % (e_f, j_f))
    for L in LAGS:
        kp = lr.scenario_lag(L, rows=tuple(N))[0]["kp"]
        e[L], j[L] = err(kp), jit(kp)
        print("| %d | %.3f | %.3f | %.3f |" % (L, e[L], e[L] / e_f, j[L]))
    print("| whole recording (RTS) | %.3f | %.3f | %.3f (truth %.3f) |" % (err(smooth["kp"][:, N]), err(smooth["kp"][:, N]) / e_f,
                                                                          jit(smooth["kp"][:, N]), jit(truth[:, N])))
    assert e[8] < e[4] < e[2] < e[1] < e_f
    assert e[4] / e_f < 0.6
    assert err(smooth["kp"][:, N]) < e[8]                                        # and the whole recording buys the rest


def test_a_lag_of_the_whole_run_is_the_fixed_interval_smoother():
    """L >= T - 1: nothing falls due before the last frame, whose tail is ref_smooth over the whole run — exactly."""
    rows = (sr.NORMAL[0], ref.DROP, ref.OUTLIER, ref.GONE, ref.NEVER)
    track, states, smooth, _ = sr.scenario_run()
    for L in (ref.T - 1, 64):
        answers, tails = lr.scenario_lag(L, rows=rows)
        for k in lr.OUT:
            assert np.array_equal(answers[k], smooth[k][:, rows]), (L, k)
            assert np.array_equal(tails[-1][k][:ref.T], smooth[k][::-1, rows]), (L, k)
        assert (tails[-1]["flag"][ref.T:] == lr.EMPTY).all() and not tails[-1]["kp"][ref.T:].any()
        assert (tails[0]["flag"][1:] == lr.EMPTY).all() and np.isin(tails[0]["flag"][0], (sr.END, sr.PASSTHROUGH)).all()


def test_the_last_tail_is_the_smoother_over_the_last_frames():
    track, states, _, _ = sr.scenario_run()
    p = sr.params()
    for L in (1, 4):
        answers, tails = lr.scenario_lag(L)
        o = sr.ref_smooth(states[-(L + 1):], track["status"][-(L + 1):], track["kp"][-(L + 1):], p.rate_hz, p.accel_psd)
        for k in lr.OUT:
            assert np.array_equal(tails[-1][k], o[k][::-1]), (L, k)
            assert np.array_equal(answers[k][-(L + 1):], o[k]), (L, k)
        # slot 0 is always the filter itself; an answer in front of the end has seen exactly L frames more
        for n in (0, 7, 31, ref.T - 1):
            assert np.isin(tails[n]["flag"][0], (sr.END, sr.PASSTHROUGH)).all()
            assert np.array_equal(tails[n]["kp"][0], track["kp"][n])
        k = 20
        o = sr.ref_smooth(states[:k + L + 1], track["status"][:k + L + 1], track["kp"][:k + L + 1], p.rate_hz, p.accel_psd)
        assert np.array_equal(answers["kp"][k], o["kp"][k]) and np.array_equal(answers["flag"][k], o["flag"][k])
    # the gone row: LOST frames pass through, and the frame in front of them ends its segment
    flag = lr.scenario_lag(4)[0]["flag"][:, ref.GONE]
    assert flag.tolist() == sr.scenario_run()[2]["flag"][:, ref.GONE].tolist()


def test_the_fp32_restatement_agrees_with_the_fp64_one():
    """Where the bounds of tests/test_pose_lag_gpu.py come from: the restatement (tracker and fixed-lag smoother, L = 4) run in NumPy
    fp32 against its fp64 run on the scenario.  Measured here: positions 3.69e-5 pixel, velocity 6.93e-5 pixel / s, covariance
    2.24e-6 relative to the larger variance (pose_lag_ref.POS_FP32, VEL_FP32, COV_REL_FP32); the GPU test allows 16 x each.  This
    test prints the figures and holds them to the recorded constants within a factor 2."""
    a64, a32 = lr.scenario_lag(4)[0], lr.scenario_lag(4, np.float32)[0]
    assert np.array_equal(a32["flag"], a64["flag"])
    e_kp, e_vel = np.abs(a32["kp"] - a64["kp"]).max(), np.abs(a32["vel"] - a64["vel"]).max()
    e_cov = ref.cov_rel_diff(a32["cov"], a64["cov"])
    print("fp32 vs fp64 fixed-lag restatement, L = 4: positions %.3e px, velocity %.3e px/s, covariance %.3e relative" % (e_kp, e_vel, e_cov))
    for got, rec in ((e_kp, lr.POS_FP32), (e_vel, lr.VEL_FP32), (e_cov, lr.COV_REL_FP32)):
        assert rec / 2 <= got <= rec * 2


def test_pose_lag_kernel_uses_no_scratch():
    """The listing the build keeps for csrc/pose_lag.hip: its one kernel, 64 threads, with 0 spilled registers, 0 bytes of scratch
    and no LDS — read from the code-object metadata only (DESIGN.md records the register count).  csrc/pose_smooth.hip, which now
    shares csrc/pose_rts.h with it, still holds exactly its one kernel."""
    meta = kernel_metadata("pose_lag")
    assert len(meta) == 1 and "hupr_k_pose_smooth_lag" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    print(m)
    assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, m
    assert m["threads"] == 64 and m["vgpr"] <= 128, m
    rts = kernel_metadata("pose_smooth")
    assert len(rts) == 1 and "hupr_k_pose_smooth_rts" in next(iter(rts)), sorted(rts)


# ---- host logic -----------------------------------------------------------------------------------------------------------------------------
def _cfg(decode=None, **test):
    if decode is not None:
        test["decode"] = decode
    return types.SimpleNamespace(TEST=types.SimpleNamespace(**test), DATASET=types.SimpleNamespace(heatmapSize=64))


def test_temporal_setting_reads_lag_and_temporal_lag():
    from hupr_amd.tools.smooth import temporal_setting
    t = temporal_setting(_cfg(temporal="lag"))
    assert t.mode == "lag" and t.lag == 4 and t.tracking.rate_hz == 10.0
    t = temporal_setting(_cfg(temporal="lag", temporalLag=2, temporalRate=25, tracking={"accel_psd": 50.0}))
    assert t.mode == "lag" and t.lag == 2 and isinstance(t.lag, int) and t.tracking.rate_hz == 25.0 and t.tracking.accel_psd == 50.0
    assert temporal_setting(_cfg(temporal="lag", temporalLag=np.int64(64))).lag == 64 and temporal_setting(_cfg(temporal="lag", temporalLag=1)).lag == 1
    assert temporal_setting(_cfg(temporal="rts", temporalLag=8)).mode == "rts"
    assert temporal_setting(_cfg(temporalLag=8)) is None and temporal_setting(_cfg(temporal="off", temporalLag=8)) is None
    for bad in (0, -1, 65, 4.0, 2.5, "4", True, None, [4], float("nan")):
        with pytest.raises(ValueError, match="TEST.temporalLag"):
            temporal_setting(_cfg(temporal="lag", temporalLag=bad))
        with pytest.raises(ValueError, match="TEST.temporalLag"):
            temporal_setting(_cfg(temporalLag=bad))                              # checked whatever TEST.temporal says
        with pytest.raises(ValueError, match="TEST.temporalLag"):
            temporal_setting(_cfg(temporal="rts", temporalLag=bad))
    for bad in ("Lag", "fixed-lag", "lagged", 4):
        with pytest.raises(ValueError, match="TEST.temporal"):
            temporal_setting(_cfg(temporal=bad))
    with pytest.raises(ValueError, match="integral"):
        temporal_setting(_cfg(temporal="lag", decode="integral"))
    assert temporal_setting(_cfg(temporal="lag", decode="subpixel")).mode == "lag"


def test_track_lag_needs_track_on_the_command_line():
    from hupr_amd.tools.stream import parse
    with pytest.raises(SystemExit):
        parse(["--raw", "x", "--track-lag", "2"])
    with pytest.raises(SystemExit):
        parse(["--raw", "x", "--track-lag", "2", "--smooth", "--rate", "10"])
    for bad in ("0", "65", "-1", "1.5", "x"):
        with pytest.raises(SystemExit):
            parse(["--raw", "x", "--track", "--rate", "10", "--track-lag", bad])
    args = parse(["--raw", "x", "--track", "--rate", "10", "--track-lag", "2"])
    assert args.track_lag == 2 and args.track
    assert parse(["--raw", "x", "--track", "--rate", "10", "--track-lag", "64", "--rts"]).track_lag == 64
    assert parse(["--raw", "x", "--track", "--rate", "10"]).track_lag is None


def test_lag_needs_track_and_a_number_of_frames():
    from hupr_amd.config_tree import load_config
    from hupr_amd.tools import PoseStream, PoseTracking, TrackingError
    cfg = load_config()
    with pytest.raises(TrackingError):
        PoseStream(None, cfg, lag=2)
    for bad in (0, 65, -1, 2.0, "2", True):
        with pytest.raises(TrackingError):
            PoseStream(None, cfg, track=PoseTracking(10.0), lag=bad)


def test_a_frame_without_lag_has_no_lagged_pose_and_a_lagged_frame_clones_it():
    import torch
    from hupr_amd.tools import LaggedPairedPoseFrame, LaggedPose, LaggedTrackedPoseFrame, PairedPoseFrame, PoseFrame, TrackedPoseFrame
    t = [torch.full((1,), float(i)) for i in range(9)] + [torch.full((1,), 3, dtype=torch.int32)]
    assert PoseFrame(3, *t[:7]).lagged is None and TrackedPoseFrame(5, *t).lagged is None and TrackedPoseFrame(5, *t).clone().lagged is None
    lp = LaggedPose(3, t[0], t[1], t[2], t[9], t[3], t[4], t[9], t[5])
    assert LaggedPose.__slots__ == ("frame", "keypoints", "velocity", "covariance", "flag", "filtered", "raw_keypoints", "status", "scores")
    for cls, base, more in ((LaggedTrackedPoseFrame, TrackedPoseFrame, {}), (LaggedPairedPoseFrame, PairedPoseFrame, {"source": t[9]})):
        assert issubclass(cls, base) and cls.__slots__ == ("lagged",)
        early = cls(2, *t, **more)
        assert early.lagged is None and early.clone().lagged is None and type(early.clone()) is cls
        pf = cls(5, *t, lagged=lp, **more)
        assert not hasattr(pf, "__dict__") and pf.clone().lagged.keypoints is not lp.keypoints
        for c in (pf.clone(), pf.cpu()):
            assert type(c) is cls and c.frame == 5 and type(c.lagged) is LaggedPose and c.lagged.frame == 3
            for k in LaggedPose.__slots__[1:]:
                assert torch.equal(getattr(c.lagged, k), getattr(lp, k)) and getattr(c.lagged, k).dtype == getattr(lp, k).dtype, k
            assert torch.equal(c.covariance, pf.covariance) and (c.source is None) == (pf.source is None)


def test_pose_smooth_lag_validates_its_arguments():
    import torch
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseTracking
    tr = PoseTracking(10.0)
    rows, L = 3, 2
    st, status, kp, raw, mx = (torch.zeros((rows, 16)), torch.zeros(rows, dtype=torch.int32), torch.zeros((rows, 2)), torch.zeros((rows, 2)),
                               torch.zeros(rows))
    ls = torch.zeros((rows, 22 * (L + 1) + 1))
    good = (st, status, kp, raw, mx, ls)
    assert F_.SMOOTH_EMPTY == 4 and F_.MAX_LAG == 64
    for i, bad in ((0, st.double()), (1, status.long()), (2, kp.double()), (3, raw.half()), (4, mx.double()), (5, ls.double()), (0, None),
                   (5, None), (0, st[:, :8]), (0, st[:2]), (2, kp[:2]), (3, raw[:, :1]), (4, mx[:2])):
        a = list(good)
        a[i] = bad
        with pytest.raises(ValueError):
            F_.pose_smooth_lag(*a, tr, L)
    with pytest.raises(ValueError):
        F_.pose_smooth_lag(*good, None, L)
    for bad in (0, 65, -1, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="lag"):
            F_.pose_smooth_lag(*good, tr, bad)
        with pytest.raises(ValueError, match="lag"):
            F_.pose_lag_state(rows, bad, "cpu")
    with pytest.raises(ValueError, match="GPU"):
        F_.pose_smooth_lag(*good, tr, L)                                         # no CPU fallback


def test_the_lag_state_is_sized_by_the_library():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime as rt
    L = rt.lib()
    assert L.hupr_pose_lag_state_bytes(3, 2) == 4 * 3 * (22 * 3 + 1) and L.hupr_pose_lag_state_bytes(0, 1) == 0
    assert L.hupr_pose_lag_state_bytes(14, 64) == 4 * 14 * (22 * 65 + 1)
    assert L.hupr_pose_lag_state_bytes(3, 0) == 0 and L.hupr_pose_lag_state_bytes(3, 65) == 0 and L.hupr_pose_lag_state_bytes(-1, 2) == 0
    # argument errors are found on the host, before any launch: no GPU is needed to see them
    c0 = L.hupr_launch_count()
    assert L.hupr_pose_smooth_lag_f32(*[None] * 5, 3, 2, 10.0, 200.0, *[None] * 9, None) == -1 and "null" in rt.last_error()
    assert L.hupr_pose_smooth_lag_f32(*[None] * 5, 0, 0, 10.0, 200.0, *[None] * 9, None) == -1 and "lag" in rt.last_error()
    assert L.hupr_pose_smooth_lag_f32(*[None] * 5, -1, 2, 10.0, 200.0, *[None] * 9, None) == -1
    assert L.hupr_pose_smooth_lag_f32(*[None] * 5, 0, 2, 0.0, 200.0, *[None] * 9, None) == -1
    assert L.hupr_pose_smooth_lag_f32(*[None] * 5, 0, 2, 10.0, 200.0, *[None] * 9, None) == 0      # rows == 0: a no-op
    assert L.hupr_launch_count() == c0
