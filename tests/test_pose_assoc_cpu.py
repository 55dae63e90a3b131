"""CPU (-m "not gpu"): the tracker that chooses its measurement among several heat-map peaks (csrc/pose_assoc.hip) — the rule's own
worth on its fp64 restatement (tests/pose_assoc_ref.py), the conditions on the inputs that tests/test_pose_assoc_gpu.py relies on,
and the argument checks at every layer (C ABI through ctypes, ``PoseTracking``, ``functional``, ``TEST.tracking``, ``PoseStream``, the
command line), the frame's new fields and the register / scratch metadata of the kernel.  No launch.

Tracker parameters: those of the tracker tests (accel_psd = 100, min_score = 0.1), min_separation = 3 and peak_ratio = 0.25.
Measured on the distractor scenario (pose_assoc_ref.distractor_scenario), rms error in image pixels from frame 20 on: K = 1 46.75 on the
distracted rows (107 gated coasts, 19 restarts on the ghost), K = 2 3.75 and no coast, the untouched rows 3.39."""
import types

import numpy as np
import pytest
import torch

import pose_assoc_ref as A
import pose_track_ref as ref
from listing import kernel_metadata


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(dict(accel_psd=100.0, min_score=ref.MIN_SCORE), **kw))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


# ---- the rule on its restatement -----------------------------------------------------------------------------------------------------------
def test_one_candidate_is_the_plain_tracker_exactly():
    maps = ref.scenario()[0]
    o, c = A.ref_run(maps, tracking(), K=1)
    idx, mx, mom = ref.scenario_moments()
    assert np.array_equal(c["idx"][:, :, 0], idx) and np.array_equal(c["score"][:, :, 0], mx) and (c["count"] == 1).all()
    assert np.array_equal(c["mom"][:, :, 0], mom)
    want = ref.ref_track(c["xy"][:, :, 0], mx, mom, tracking(), ref.RATIO)
    for k in ("kp", "vel", "cov", "fc", "status", "state"):
        assert np.array_equal(o[k], want[k]), k
    assert np.array_equal(o["chosen"], np.where(np.isin(want["status"], (ref.UPDATED, ref.STARTED)), 0, -1))
    assert len(np.unique(want["status"])) == 5                                   # the events scenario shows every status


@pytest.mark.parametrize("H,W", A.HAND_SHAPES, ids=["8x12", "64x64"])
def test_hand_placed_maps_have_the_candidates_written_beside_them(H, W):
    maps, want = A.hand_maps(H, W)
    got = A.ref_peaks(maps, A.HAND_K, A.HAND_SEPARATION, A.HAND_PEAK_RATIO, 4.0)
    for i, w in enumerate(want):
        n = got["count"][i]
        assert [(int(p % W), int(p // W)) for p in got["idx"][i, :n]] == w, i
        assert not got["idx"][i, n:].any() and not got["score"][i, n:].any() and not got["xy"][i, n:].any()
    assert np.isnan(maps[4]).sum() == 2 and got["count"][5] == 0
    sub = got["xy"][6, :2] / 4.0                                                  # the smooth bumps decode to their centres
    off = (0, 0) if (H, W) == (8, 12) else (23, 31)
    assert np.abs(sub - (np.array([[3.3, 3.6], [8.4, 4.2]]) + off)).max() < 0.01
    fewer = A.ref_peaks(maps, 2, A.HAND_SEPARATION, A.HAND_PEAK_RATIO, 4.0)      # a smaller K is a prefix
    assert np.array_equal(fewer["idx"], got["idx"][:, :2] * (np.arange(2) < got["count"][:, None]))


@pytest.fixture(scope="module")
def distractor():
    maps, truth = A.distractor_scenario()
    runs = {K: A.ref_run(maps, tracking(candidates=K)) for K in (1, 2)}
    return maps, truth, runs


def test_two_candidates_keep_the_track_a_ghost_takes_from_one(distractor):
    maps, truth, runs = distractor
    (o1, _), (o2, c2) = runs[1], runs[2]
    e1, clean1 = A.distractor_errors(o1["kp"], truth)
    e2, clean2 = A.distractor_errors(o2["kp"], truth)
    t0, rows = A.GHOST_FRAMES[0], list(A.DISTRACTED)
    print("distractor scenario, rms error from frame %d on: K = 1 %.2f px on the distracted rows (statuses %s), K = 2 %.2f px (statuses "
          "%s, chosen %s), the untouched rows %.2f px"
          % (t0, e1, np.bincount(o1["status"][t0:, rows].ravel(), minlength=5).tolist(), e2,
             np.bincount(o2["status"][t0:, rows].ravel(), minlength=5).tolist(),
             np.bincount(o2["chosen"][t0:, rows].ravel() + 1, minlength=3).tolist(), clean2))
    assert clean1 == clean2                                                      # rows without a second peak do not notice K
    assert e2 <= 1.5 * clean2
    assert e1 >= 5.0 * e2
    assert (o2["status"][t0:, rows] == ref.UPDATED).all()                        # no coast at all
    assert (o2["chosen"][list(A.GHOST_FRAMES)][:, rows] == 1).sum() > 100       # and the second peak is what it took
    assert (c2["count"][list(A.GHOST_FRAMES)][:, rows] == 2).sum() > 200


def test_the_distractor_scenario_decides_nothing_on_a_rounding(distractor):
    """What tests/test_pose_assoc_gpu.py needs in order to ask for equal statuses and choices of an fp32 kernel."""
    maps, _, runs = distractor
    o, c = runs[2]
    p = tracking(candidates=2)
    d2 = o["d2"][np.isfinite(o["d2"])]
    margin = np.abs(d2 / p.gate - 1.0).min()
    cost = np.sort(np.where(np.isfinite(o["cost"]), o["cost"], np.inf), axis=-1)
    both = np.isfinite(cost[..., 1])
    gap = (cost[both][:, 1] - cost[both][:, 0]).min()
    flat = maps.reshape(ref.T, ref.ROWS, -1)
    floor = np.float32(p.peak_ratio) * flat.max(axis=-1)
    tops = np.stack([[A.local_maxima(m) for m in frame] for frame in maps]).reshape(flat.shape)
    rel = np.abs(flat / floor[..., None] - 1.0)[tops].min()
    print("%d gate decisions, the nearest %.3f of the gate away; %d frames x rows with two gated candidates, the closest costs %.3f "
          "apart; the local maximum nearest to peak_ratio x maximum is %.3f of it away" % (d2.size, margin, int(both.sum()), gap, rel))
    assert d2.size > 1500 and margin > 0.01
    assert both.sum() >= 10 and gap > 1e-3
    assert rel > 1e-4


def test_what_a_second_candidate_costs_under_noise():
    """Nearest-neighbour association takes the likeliest peak, and under additive noise that is now and then a noise peak: the honest
    cost of the rule and the reason ``candidates`` defaults to 1.  Printed (PAPERS.md holds the table); asserted only where it is
    exact: without noise a single bump has a single candidate and K changes nothing."""
    maps, truth, _ = ref.scenario()
    normal = [r for r in range(ref.ROWS) if r not in (ref.DROP, ref.OUTLIER, ref.GONE, ref.NEVER)]
    noisy = (maps + np.abs(np.random.RandomState(7).normal(0.0, 0.1, maps.shape))).astype(np.float32)
    table = {}
    for name, m in (("none", maps), ("|N(0, 0.1)|", noisy)):
        for K in (1, 3):
            o, c = A.ref_run(m, tracking(candidates=K))
            table[name, K] = A.rms((o["kp"] - truth)[:, normal]), float((c["count"][:, normal] > 1).mean())
    for name in ("none", "|N(0, 0.1)|"):
        print("additive noise %-12s normal rows: K = 1 rms %.3f px, K = 3 rms %.3f px (%.0f %% of the maps show a second candidate)"
              % (name, table[name, 1][0], table[name, 3][0], 100 * table[name, 3][1]))
    assert table["none", 1][0] == table["none", 3][0] and table["none", 3][1] == 0.0
    assert all(np.isfinite(v[0]) for v in table.values())


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
GOOD = (10.0, 200.0, 1.0, 1.0, 13.816, 5, 50.0, 0.0, 0.0)
P = 4096                                                   # any non-null address: every call below returns before it launches


def _assoc(L, heat=P, rows=28, state=P, params=GOOD, K=2, sep=3, floor=0.25, present=None, group=14, outs=(P,) * 12, H=64, W=64):
    return L.hupr_pose_track_assoc_f32(heat, rows, H, W, 4.0, 1, state, *params, K, sep, floor, present, group, *outs, None)


def _peaks(L, heat=P, rows=28, K=2, sep=3, floor=0.25, outs=(P,) * 4, H=64, W=64):
    return L.hupr_pose_peaks_f32(heat, rows, H, W, 4.0, 1, K, sep, floor, *outs, None)


def test_entry_points_check_their_arguments_on_the_host(L):
    assert _assoc(L, None, 0, None, (0.0,) * 5 + (0,) + (0.0,) * 3, 0, -1, 0.0, None, 0, (None,) * 12) == 0      # rows == 0: a no-op
    assert _peaks(L, None, 0, 0, -1, 0.0, (None,) * 4) == 0
    assert _assoc(L, heat=None) == -1 and b"null" in L.hupr_last_error()
    assert _assoc(L, state=None) == -1 and b"null" in L.hupr_last_error()
    for k in range(12):
        assert _assoc(L, outs=tuple(None if j == k else P for j in range(12))) == -1, k
        assert b"null" in L.hupr_last_error()
    for k in range(4):
        assert _peaks(L, outs=tuple(None if j == k else P for j in range(4))) == -1, k
        assert b"null" in L.hupr_last_error()
    assert _peaks(L, heat=None) == -1 and b"null" in L.hupr_last_error()
    for call in (_assoc, _peaks):
        assert call(L, rows=-1) == -1 and b"shape" in L.hupr_last_error()
        assert call(L, H=0) == -1 and b"shape" in L.hupr_last_error()
        assert call(L, H=1 << 16, W=1 << 16) == -1 and b"shape" in L.hupr_last_error()
        for bad in (dict(K=0), dict(K=5), dict(K=-1), dict(sep=-1), dict(floor=0.0), dict(floor=-0.5), dict(floor=1.5),
                    dict(floor=float("nan"))):
            assert call(L, **bad) == -1 and b"candidate parameter" in L.hupr_last_error(), bad
    assert _assoc(L, state=P + 4) == -1 and b"aligned" in L.hupr_last_error()
    assert _assoc(L, params=GOOD[:4] + (0.0,) + GOOD[5:]) == -1 and b"tracker parameter" in L.hupr_last_error()
    # the groups of the presence flags: only read with the pointer
    assert _assoc(L, present=P, group=0) == -1 and b"rows_per_group" in L.hupr_last_error()
    assert _assoc(L, present=P, group=-2) == -1 and b"rows_per_group" in L.hupr_last_error()
    assert _assoc(L, present=P, group=5) == -1 and b"rows_per_group" in L.hupr_last_error()


def test_pose_tracking_validates_the_association_settings():
    from hupr_amd.tools import stream as st
    s = st.PoseTracking(10)
    assert (s.candidates, s.min_separation, s.peak_ratio, s.gate_on_presence) == (1, 3, 0.25, False) and not s.associates
    assert type(s.candidates) is int and type(s.min_separation) is int and type(s.peak_ratio) is float
    assert st.PoseTracking.ARGUMENTS == st.PoseTracking.__slots__ + ("candidates", "min_separation", "peak_ratio", "gate_on_presence")
    assert "guesses" in st.PoseTracking.__doc__
    s = st.PoseTracking(10, candidates=np.int64(3), min_separation=0, peak_ratio=1, gate_on_presence=True)
    assert (s.candidates, s.min_separation, s.peak_ratio, s.gate_on_presence) == (3, 0, 1.0, True) and s.associates
    assert st.PoseTracking(10, candidates=2).associates and st.PoseTracking(10, gate_on_presence=True).associates
    assert repr(s).endswith("candidates=3, min_separation=0, peak_ratio=1.0, gate_on_presence=True)")
    h = s.with_horizon(0.3)
    assert h.horizon_s == 0.3 and all(getattr(h, k) == getattr(s, k) for k in st.PoseTracking.ARGUMENTS if k != "horizon_s")
    with pytest.raises(AttributeError):
        s.extra = 1
    for bad in (dict(candidates=0), dict(candidates=5), dict(candidates=2.0), dict(candidates=True), dict(candidates=None),
                dict(min_separation=-1), dict(min_separation=1.5), dict(min_separation=True), dict(peak_ratio=0), dict(peak_ratio=-0.1),
                dict(peak_ratio=1.01), dict(peak_ratio=float("nan")), dict(peak_ratio="0.25"), dict(peak_ratio=True),
                dict(gate_on_presence=1), dict(gate_on_presence=None)):
        with pytest.raises(st.TrackingError):
            st.PoseTracking(10, **bad)


def test_test_tracking_forwards_the_association_settings():
    from hupr_amd.tools.smooth import SequenceSmoother, temporal_setting
    from hupr_amd.tools import TrackingError
    cfg = lambda **test: types.SimpleNamespace(TEST=types.SimpleNamespace(**test), DATASET=types.SimpleNamespace(heatmapSize=64))
    t = temporal_setting(cfg(temporal="rts", tracking={"candidates": 3, "min_separation": 2, "peak_ratio": 0.5}))
    assert (t.tracking.candidates, t.tracking.min_separation, t.tracking.peak_ratio) == (3, 2, 0.5)
    assert temporal_setting(cfg(temporal="track")).tracking.candidates == 1
    for bad in ({"candidates": 5}, {"candidates": 1.5}, {"peak_ratio": 0}, {"min_separation": -1}, {"separation": 2}):
        with pytest.raises(ValueError, match="TEST.tracking"):
            temporal_setting(cfg(temporal="track", tracking=bad))
    # the offline walker has no presence gate to ask
    with pytest.raises(TrackingError, match="gate_on_presence"):
        SequenceSmoother(tracking(gate_on_presence=True), 14, "cpu")


def test_functional_refuses_bad_arguments_and_cpu_tensors(L):
    from hupr_amd import functional as F_
    from hupr_amd.runtime import HuprError
    heat = torch.zeros((2, 3, 8, 8))
    assert F_.MAX_CANDIDATES == 4 and F_.check_peaks(np.int64(2), 0, 1) == (2, 0, 1.0)
    for bad in (dict(K=0), dict(K=5), dict(K=2.0), dict(K=True), dict(K=2, min_separation=-1), dict(K=2, min_separation=1.5),
                dict(K=2, peak_ratio=0.0), dict(K=2, peak_ratio=1.5), dict(K=2, peak_ratio=float("nan")), dict(K=2, peak_ratio="x")):
        with pytest.raises(ValueError):
            F_.pose_peaks(heat, 4.0, **bad)
    with pytest.raises(ValueError):
        F_.pose_peaks(torch.zeros(8), 4.0, 2)
    with pytest.raises(ValueError):
        F_.pose_peaks(heat.double(), 4.0, 2)
    with pytest.raises(HuprError):                                               # no CPU fallback
        F_.pose_peaks(heat, 4.0, 2)
    state = F_.pose_track_state(6, "cpu")
    for present in (torch.ones(2), torch.ones(3, dtype=torch.int32), torch.ones((2, 3), dtype=torch.int32), [1, 1]):
        with pytest.raises(ValueError, match="present"):
            F_.pose_track(heat, 4.0, track_state=state, tracking=tracking(), present=present)
    with pytest.raises(HuprError):
        F_.pose_track(heat, 4.0, track_state=state, tracking=tracking(), present=torch.ones(2, dtype=torch.int32))
    with pytest.raises(HuprError):
        F_.pose_track(heat, 4.0, track_state=state, tracking=tracking(candidates=2))


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
    with pytest.raises(tools.TrackingError, match="presence"):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, gate_on_presence=True))
    with pytest.raises(HuprError):                                               # valid arguments reach the GPU check
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, gate_on_presence=True), presence=tools.PresenceGate())
    with pytest.raises(HuprError):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, candidates=2))


def test_tracked_pose_frame_carries_the_candidates():
    from hupr_amd.tools.stream import PoseFrame, TrackedPoseFrame
    t = [torch.full((1,), float(i)) for i in range(9)] + [torch.full((1,), 3, dtype=torch.int32)]
    plain = TrackedPoseFrame(5, *t)
    assert plain.candidates is None and plain.candidate_scores is None and plain.candidate_count is None and plain.chosen is None
    assert plain.clone().chosen is None and not hasattr(plain, "__dict__")
    extra = [torch.full((1, 2, 2), 7.0), torch.full((1, 2), 8.0), torch.full((1,), 2, dtype=torch.int32), torch.full((1,), -1, dtype=torch.int32)]
    pf = TrackedPoseFrame(5, *t, None, None, *extra)
    assert pf.candidates is extra[0] and pf.candidate_scores is extra[1] and pf.candidate_count is extra[2] and pf.chosen is extra[3]
    for c in (pf.clone(), pf.cpu()):
        assert type(c) is TrackedPoseFrame and c.present is None and c.frame == 5
        for k, want in zip(("candidates", "candidate_scores", "candidate_count", "chosen"), extra):
            assert torch.equal(getattr(c, k), want) and getattr(c, k).dtype == want.dtype, k
    assert pf.clone().candidates is not pf.candidates
    assert isinstance(pf, PoseFrame)


def test_stream_command_association_arguments():
    from hupr_amd.tools import stream as st
    t = st.tracking_from_args(st.parse(["--raw", "x", "--track", "--rate", "10"]))
    assert (t.candidates, t.min_separation, t.peak_ratio, t.gate_on_presence) == (1, 3, 0.25, False)
    a = st.parse(["--raw", "x", "--track", "--rate", "10", "--track-candidates", "3", "--track-separation", "2", "--track-peak-ratio", "0.5",
                  "--presence", "--track-on-presence"])
    t = st.tracking_from_args(a)
    assert (t.candidates, t.min_separation, t.peak_ratio, t.gate_on_presence) == (3, 2, 0.5, True)
    track = ["--track", "--rate", "10"]
    for bad in (["--track-candidates", "2"], ["--track-separation", "2"], ["--track-peak-ratio", "0.5"], ["--track-on-presence"],
                ["--presence", "--track-on-presence"], track + ["--track-on-presence"], track + ["--track-candidates", "5"],
                track + ["--track-candidates", "0"], track + ["--track-candidates", "1.5"], track + ["--track-separation", "-1"],
                track + ["--track-peak-ratio", "0"], track + ["--track-peak-ratio", "2"]):
        with pytest.raises(SystemExit):
            st.parse(["--raw", "x"] + bad)


def test_pose_assoc_kernel_uses_no_scratch():
    """The listing the build keeps for csrc/pose_assoc.hip: its one kernel, 64 threads, with 0 spilled vector registers, 0 bytes of
    scratch and no LDS — read from the code-object metadata only."""
    meta = kernel_metadata("pose_assoc")
    assert len(meta) == 1 and "hupr_k_pose_track_assoc" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    print(m)
    assert m["spill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, m
    assert m["threads"] == 64 and m["vgpr"] <= 128, m
