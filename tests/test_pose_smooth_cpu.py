"""CPU: the Rauch-Tung-Striebel smoother's rule (include/hupr.h, hupr_pose_smooth_rts_f32) as restated in tests/pose_smooth_ref.py —
against a dense textbook RTS, for what it buys on the tracker tests' scenario (60 frames x 28 rows at 10 Hz, seed 11; the table of
PAPERS.md is printed here), its flags, and the NumPy fp32 vs fp64 differences that set the bounds of tests/test_pose_smooth_gpu.py —
and the host logic around it: TEST.temporal / temporalRate / tracking, imageId to sequence and frame, --rts, jitter.

Tracker parameters of these tests (pose_smooth_ref.params): PoseTracking's defaults with accel_psd = 200, min_score = 0.1, arg-max
measurements."""
import types

import numpy as np
import pytest

import pose_smooth_ref as sr
import pose_track_ref as ref
from listing import kernel_metadata


def _truth():
    return ref.scenario()[1]


def test_the_restatement_equals_a_dense_textbook_rts():
    """On a segment without events (a normal row: STARTED, then UPDATED throughout) the Cholesky / two-solve form is the textbook
    smoother with np.linalg.inv, to 1e-10."""
    track, states, smooth, _ = sr.scenario_run()
    p = sr.params()
    F, Q = sr.model(p.rate_hz, p.accel_psd, np.float64)
    worst = 0.0
    for r in sr.NORMAL[:6]:
        assert track["status"][0, r] == ref.STARTED and (track["status"][1:, r] == ref.UPDATED).all()
        x, P = sr.unpack(states[:, r], np.float64)
        xs, Ps = sr.textbook_rts(x, P, F, Q)
        worst = max(worst, np.abs(xs - smooth["x"][:, r]).max(), np.abs(Ps - smooth["P"][:, r]).max())
    print("restatement vs dense textbook RTS: %.3e" % worst)
    assert worst <= 1e-10


def test_the_smoother_beats_the_filter_on_the_scenario():
    track, _, smooth, raw = sr.scenario_run()
    truth, N = _truth(), sr.NORMAL
    assert len(N) == 24
    e_raw, e_f, e_s = (sr.rms((a - truth)[:, N]) for a in (raw, track["kp"], smooth["kp"]))
    j_raw, j_f, j_s, j_t = (sr.rms(sr.second_difference(a[:, N])) for a in (raw, track["kp"], smooth["kp"], truth))
    print("| quantity (image pixels) | raw decode | filter | smoother | truth |")
    print("| rms position error | %.2f | %.2f | %.2f | |" % (e_raw, e_f, e_s))
    print("| rms second difference (jitter) | %.2f | %.2f | %.3f | %.3f |" % (j_raw, j_f, j_s, j_t))
    assert e_s < e_f < e_raw
    assert e_s / e_f < 0.6
    assert j_t / 2 <= j_s <= j_t * 2
    for r in N:
        assert sr.rms((smooth["kp"] - truth)[:, r]) < sr.rms((track["kp"] - truth)[:, r]), r
    dist = lambda a, t, r: float(np.linalg.norm(a[t, r] - truth[t, r]))
    for t in ref.DROP_FRAMES:
        assert track["status"][t, ref.DROP] == ref.COASTED_MISSING and smooth["flag"][t, ref.DROP] == sr.SMOOTHED
        print("drop-out frame %d: filter %.2f px (Pxx %.1f), smoother %.2f px (Pxx %.1f)"
              % (t, dist(track["kp"], t, ref.DROP), track["cov"][t, ref.DROP, 0], dist(smooth["kp"], t, ref.DROP), smooth["cov"][t, ref.DROP, 0]))
        assert dist(smooth["kp"], t, ref.DROP) < dist(track["kp"], t, ref.DROP)
        assert smooth["cov"][t, ref.DROP, 0] < 0.5 * track["cov"][t, ref.DROP, 0]
    t = ref.OUTLIER_FRAME
    assert track["status"][t, ref.OUTLIER] == ref.COASTED_GATED
    print("outlier frame: filter %.2f px, smoother %.2f px" % (dist(track["kp"], t, ref.OUTLIER), dist(smooth["kp"], t, ref.OUTLIER)))
    assert dist(smooth["kp"], t, ref.OUTLIER) < dist(track["kp"], t, ref.OUTLIER)
    # the smoothed position variances never exceed the filter's, at every live frame
    live = track["status"] != ref.LOST
    assert (smooth["cov"][..., 0][live] <= track["cov"][..., 0][live] * (1 + 1e-12)).all()
    assert (smooth["cov"][..., 2][live] <= track["cov"][..., 2][live] * (1 + 1e-12)).all()
    # the predicted covariances are well conditioned: a 4 x 4 Cholesky in fp32 is safe
    p = sr.params()
    F, Q = sr.model(p.rate_hz, p.accel_psd, np.float64)
    _, P = sr.unpack(sr.scenario_run()[1], np.float64)
    cond = np.array([np.linalg.cond(F @ P[k, r] @ F.T + Q) for k in range(ref.T) for r in range(ref.ROWS) if live[k, r]])
    print("condition numbers of the predicted covariances: max %.1f, median %.1f" % (cond.max(), np.median(cond)))
    assert cond.max() < 1e3


def test_the_flags_follow_the_track_segments():
    track, _, smooth, _ = sr.scenario_run()
    flag = smooth["flag"]
    want = [sr.SMOOTHED] * 29 + [sr.END] + [sr.PASSTHROUGH] * 5 + [sr.SMOOTHED] * 24 + [sr.END]
    assert flag[:, ref.GONE].tolist() == want
    lost = track["status"][:, ref.GONE] == ref.LOST
    assert np.array_equal(smooth["kp"][lost, ref.GONE], track["kp"][lost, ref.GONE])
    assert not smooth["vel"][lost, ref.GONE].any() and not smooth["cov"][lost, ref.GONE].any()
    assert (flag[:, ref.NEVER] == sr.PASSTHROUGH).all()
    for r in sr.NORMAL:
        assert (flag[:-1, r] == sr.SMOOTHED).all() and flag[-1, r] == sr.END
    # an END frame is the filter's own state
    ends = flag == sr.END
    assert np.array_equal(smooth["kp"][ends], track["kp"][ends]) and np.array_equal(smooth["cov"][ends], track["cov"][ends])
    assert not (flag == sr.DEGENERATE).any()


def test_a_single_frame_is_an_end_or_a_passthrough():
    track, states, _, _ = sr.scenario_run()
    for k in (0, 30):
        o = sr.ref_smooth(states[k:k + 1], track["status"][k:k + 1], track["kp"][k:k + 1], ref.RATE, sr.ACCEL_PSD)
        lost = track["status"][k] == ref.LOST
        assert lost.any() and not lost.all()
        assert np.array_equal(o["flag"][0], np.where(lost, sr.PASSTHROUGH, sr.END))
        assert np.array_equal(o["kp"][0], track["kp"][k]) and np.array_equal(o["cov"][0], track["cov"][k])


def test_a_zero_covariance_is_degenerate_only_without_process_noise():
    """P_k = 0 inside a live segment: with accel_psd = 0 the predicted covariance is 0, the first pivot is not positive and the frame is
    DEGENERATE; with accel_psd > 0 the predicted covariance is Q, positive definite, the gain is 0 and the frame keeps the filter's
    state as SMOOTHED.  Every other frame stays finite."""
    track, states, _, _ = sr.scenario_run()
    r, k = sr.NORMAL[0], 17
    st = states[:, r:r + 1].copy()
    st[k, 0, 4:14] = 0.0
    for psd, want in ((0.0, sr.DEGENERATE), (sr.ACCEL_PSD, sr.SMOOTHED)):
        o = sr.ref_smooth(st, track["status"][:, r:r + 1], track["kp"][:, r:r + 1], ref.RATE, psd)
        assert o["flag"][k, 0] == want and (np.delete(o["flag"][:-1, 0], k) == sr.SMOOTHED).all()
        assert np.array_equal(o["x"][k, 0], st[k, 0, :4]) and not o["P"][k, 0].any()
        assert np.isfinite(o["x"]).all() and np.isfinite(o["P"]).all()


def test_the_fp32_restatement_agrees_with_the_fp64_one():
    """Where the bounds of tests/test_pose_smooth_gpu.py come from: the restatement (tracker and smoother) run in NumPy fp32 against
    its fp64 run on the scenario.  Measured here: positions 4.03e-5 pixel, velocity 6.58e-5 pixel / s, covariance 3.18e-6 relative
    to the larger variance (pose_smooth_ref.POS_FP32, VEL_FP32, COV_REL_FP32); the GPU test allows 16 x each.  This test prints the
    figures and holds them to the recorded constants within a factor 2."""
    t64, _, s64, _ = sr.scenario_run()
    t32, _, s32, _ = sr.scenario_run(np.float32)
    assert np.array_equal(t32["status"], t64["status"]) and np.array_equal(s32["flag"], s64["flag"])
    e_kp, e_vel = np.abs(s32["kp"] - s64["kp"]).max(), np.abs(s32["vel"] - s64["vel"]).max()
    e_cov = ref.cov_rel_diff(s32["cov"], s64["cov"])
    print("fp32 vs fp64 smoother restatement: positions %.3e px, velocity %.3e px/s, covariance %.3e relative" % (e_kp, e_vel, e_cov))
    for got, rec in ((e_kp, sr.POS_FP32), (e_vel, sr.VEL_FP32), (e_cov, sr.COV_REL_FP32)):
        assert rec / 2 <= got <= rec * 2


def test_pose_smooth_kernel_uses_no_scratch():
    """The listing the build keeps for csrc/pose_smooth.hip: its one kernel, 64 threads, with 0 spilled registers, 0 bytes of scratch
    and no LDS — read from the code-object metadata only (DESIGN.md records the register count)."""
    meta = kernel_metadata("pose_smooth")
    assert len(meta) == 1 and "hupr_k_pose_smooth_rts" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    print(m)
    assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, m
    assert m["threads"] == 64 and m["vgpr"] <= 128, m


# ---- host logic -----------------------------------------------------------------------------------------------------------------------------
def _cfg(decode=None, **test):
    if decode is not None:
        test["decode"] = decode
    return types.SimpleNamespace(TEST=types.SimpleNamespace(**test), DATASET=types.SimpleNamespace(heatmapSize=64))


def test_temporal_setting_validates_the_three_keys():
    from hupr_amd.config_tree import obj
    from hupr_amd.tools.smooth import temporal_setting
    assert temporal_setting(_cfg()) is None and temporal_setting(_cfg(temporal="off")) is None
    assert temporal_setting(_cfg(temporal=False)) is None                      # YAML's bare off
    assert temporal_setting(types.SimpleNamespace()) is None
    t = temporal_setting(_cfg(temporal="track"))
    assert t.mode == "track" and t.tracking.rate_hz == 10.0 and t.tracking.accel_psd == 200.0
    t = temporal_setting(_cfg(temporal="rts", temporalRate=25, tracking={"accel_psd": 50.0, "max_coast": 2}))
    assert t.mode == "rts" and t.tracking.rate_hz == 25.0 and t.tracking.accel_psd == 50.0 and t.tracking.max_coast == 2
    t = temporal_setting(_cfg(temporal="rts", decode="subpixel", tracking=obj({"gate": 9.21})))     # a YAML mapping as config_tree reads it
    assert t.tracking.gate == 9.21
    for bad in ("kalman", "RTS", 1, True, ["rts"]):
        with pytest.raises(ValueError, match="TEST.temporal"):
            temporal_setting(_cfg(temporal=bad))
    for bad in (0, -10.0, float("inf"), float("nan"), "10", True, None):
        with pytest.raises(ValueError, match="TEST.temporalRate"):
            temporal_setting(_cfg(temporal="rts", temporalRate=bad))
        with pytest.raises(ValueError, match="TEST.temporalRate"):
            temporal_setting(_cfg(temporalRate=bad))                           # checked whatever TEST.temporal says
    for bad in ({"rate_hz": 10.0}, {"accel": 1.0}, {"gate": -1.0}, {"max_coast": 1.5}, [1, 2], "x", 3):
        with pytest.raises(ValueError, match="TEST.tracking"):
            temporal_setting(_cfg(temporal="track", tracking=bad))
    for mode in ("track", "rts"):
        with pytest.raises(ValueError, match="integral"):
            temporal_setting(_cfg(temporal=mode, decode="integral"))
    assert temporal_setting(_cfg(temporal="off", decode="integral")) is None


def test_image_ids_become_sequences_and_a_gap_resets():
    from hupr_amd.tools.smooth import SequenceWalker, sequence_and_frame
    assert sequence_and_frame(0) == (0, 0) and sequence_and_frame(99999) == (0, 99999)
    assert sequence_and_frame(100000) == (1, 0) and sequence_and_frame(27600123) == (276, 123)
    with pytest.raises(ValueError):
        sequence_and_frame(-1)
    w = SequenceWalker()
    ids = [0, 1, 2, 4, 5, 100005, 100006, 200000, 200001, 200001, 200000]
    resets = [w.step(np.int64(i)) for i in ids]
    assert resets == [True, False, False, True, False, True, False, True, False, True, True]
    assert w.segments() == [(0, 3), (3, 5), (5, 7), (7, 9), (9, 10), (10, 11)]


def test_rts_needs_track_on_the_command_line():
    from hupr_amd.tools.stream import parse
    with pytest.raises(SystemExit):
        parse(["--raw", "x", "--rts"])
    with pytest.raises(SystemExit):
        parse(["--raw", "x", "--rts", "--smooth", "--rate", "10"])
    args = parse(["--raw", "x", "--track", "--rate", "10", "--rts"])
    assert args.rts and args.track
    assert parse(["--raw", "x", "--track", "--rate", "10"]).rts is False


def test_history_needs_track():
    from hupr_amd.config_tree import load_config
    from hupr_amd.tools import PoseStream, TrackingError
    with pytest.raises(TrackingError):
        PoseStream(None, load_config(), history=True)


def test_jitter_is_the_rms_second_difference():
    import torch
    from hupr_amd.tools import jitter
    t = np.arange(10, dtype=np.float64)
    line = np.stack([3.0 * t + 1.0, -2.0 * t], axis=-1)[:, None, :]              # (10, 1, 2): a steady motion has none
    assert jitter(line) == 0.0
    para = np.stack([0.5 * t * t, np.zeros_like(t)], axis=-1)[:, None, :]        # second difference (1, 0) throughout
    assert abs(jitter(para) - np.sqrt(0.5)) < 1e-12
    assert abs(jitter(torch.from_numpy(para).float()) - np.sqrt(0.5)) < 1e-6
    assert abs(jitter([para, line]) - np.sqrt(0.25)) < 1e-12                     # pooled over the sequences, not across their seam
    assert np.isnan(jitter(para[:2])) and abs(jitter([para[:2], para]) - np.sqrt(0.5)) < 1e-12
    # the restatement's metric
    kp = np.random.RandomState(0).normal(size=(12, 3, 2))
    assert abs(jitter(kp) - sr.rms(sr.second_difference(kp))) < 1e-12


def test_pose_smooth_rts_validates_its_arguments():
    import torch
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseTracking
    tr = PoseTracking(10.0)
    st, status, kp = torch.zeros((3, 2, 16)), torch.zeros((3, 2), dtype=torch.int32), torch.zeros((3, 2, 2))
    for bad in ((st.double(), status, kp), (st, status.long(), kp), (st, status, kp.double()), (st[:, :, :8], status, kp),
                (st, status, kp[:2]), (st[:0], status[:0], kp[:0]), (None, status, kp)):
        with pytest.raises(ValueError):
            F_.pose_smooth_rts(*bad, tr)
    with pytest.raises(ValueError):
        F_.pose_smooth_rts(st, status, kp, None)
    with pytest.raises(ValueError, match="GPU"):
        F_.pose_smooth_rts(st, status, kp, tr)                                   # no CPU fallback
