"""CPU (-m "not gpu"): the tracker that assigns the left / right partners of a skeleton jointly (csrc/pose_pairs.hip) — the rule's own
worth on its fp64 restatement (tests/pose_pairs_ref.py), what it costs where nothing is swapped, the conditions on the inputs that
tests/test_pose_pairs_gpu.py relies on, the hand-placed maps, the argument checks at every layer (C ABI through ctypes,
``PoseTracking``, ``functional``, ``TEST.tracking``, ``PoseStream``, the command line), the frame's new field and the scratch metadata
of the kernel.  No launch.

Tracker parameters: those of the tracker tests (accel_psd = 100, min_score = 0.1, one candidate per map).  Measured on the swap scenario
(pose_pairs_ref.swap_scenario: the maps of the six L / R pairs of lane 0 exchanged in frames 20..35), rms error in image pixels from
frame 20 on: the plain tracker 26.88 on the swapped rows (84 gated coasts, 12 restarts), the paired one 3.89 with swap_cost = 0 (all
480 UPDATED, 194 measurements from the partner's map) and 21.82 with swap_cost = 2; the untouched lane 3.39 throughout."""
import ctypes
import types

import numpy as np
import pytest
import torch

import pose_assoc_ref as A
import pose_pairs_ref as Pr
import pose_track_ref as ref
from listing import kernel_metadata

GATE = 9.21                  # the 99 % quantile: at the default 13.816 a cross-pair d2 of the swap scenario lies 1.9e-5 from the gate


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(dict(accel_psd=100.0, min_score=ref.MIN_SCORE), **kw))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


@pytest.fixture(scope="module")
def swapped():
    maps, truth = Pr.swap_scenario()
    return maps, truth, Pr.candidates(maps, tracking())


@pytest.fixture(scope="module")
def unswapped():
    maps, truth = Pr.swap_scenario(frames=())
    return maps, truth, Pr.candidates(maps, tracking())


def run(c, p, partner, swap_cost=0.0, present=None):
    return Pr.ref_pairs(c["xy"], c["score"], c["count"], c["mom"], p, ref.RATIO, partner, swap_cost, present)


# ---- the rule on its restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 2))
def test_the_identity_table_is_the_associating_tracker_exactly(K):
    maps = A.distractor_scenario()[0] if K == 2 else ref.scenario()[0]
    p = tracking(candidates=K)
    want, c = A.ref_run(maps, p)
    got = run(c, p, Pr.IDENTITY)
    for k in ("kp", "vel", "cov", "fc", "status", "chosen", "state", "usable"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["d2"][..., :K], want["d2"], equal_nan=True) and np.array_equal(got["cost"][..., :K], want["cost"], equal_nan=True)
    assert np.isnan(got["d2"][..., K:]).all()
    assert np.array_equal(got["source"], np.where(want["chosen"] >= 0, 0, -1))
    assert (want["chosen"] == K - 1).any()


def test_a_left_right_swap_is_followed(swapped):
    maps, truth, c = swapped
    p = tracking()
    plain, paired = run(c, p, Pr.IDENTITY), run(c, p, Pr.PARTNER)
    costly = run(c, p, Pr.PARTNER, 2.0)
    t0, rows = Pr.SWAP_FRAMES[0], list(Pr.swapped_rows())
    (e_plain, clean_plain), (e_pair, clean_pair) = Pr.swap_errors(plain["kp"], truth), Pr.swap_errors(paired["kp"], truth)
    st_plain, st_pair = plain["status"][t0:, rows], paired["status"][t0:, rows]
    taken = int((paired["source"][:, rows] == 1).sum())
    print("swap scenario, rms error from frame %d on: plain %.2f px on the swapped rows (statuses %s of %d), paired with swap_cost 0 "
          "%.2f px (statuses %s, %d measurements from the partner's map), with swap_cost 2 %.2f px; the untouched lane %.2f px"
          % (t0, e_plain, np.bincount(st_plain.ravel(), minlength=5).tolist(), st_plain.size, e_pair,
             np.bincount(st_pair.ravel(), minlength=5).tolist(), taken, Pr.swap_errors(costly["kp"], truth)[0], clean_pair))
    assert clean_plain == clean_pair                                             # the other lane does not notice
    assert e_pair <= 1.5 * clean_pair
    assert e_plain >= 5.0 * e_pair
    assert (st_pair == ref.UPDATED).all()                                        # no coast at all
    assert taken > 150
    inside = paired["source"][list(Pr.SWAP_FRAMES)][:, rows]
    assert (inside == 1).mean() > 0.95                                           # and the partner's map is where it took them, while swapped
    single = [r for r in range(Pr.GROUP) if Pr.PARTNER[r] == r]
    for k in ("kp", "status", "chosen", "source"):                               # a joint without a partner is tracked as before
        assert np.array_equal(paired[k][:, single], plain[k][:, single]), k


def test_what_the_pairing_costs_where_nothing_is_swapped(unswapped):
    """The synthetic tracks are independent and cross (down to a few pixels apart), and with swap_cost = 0 the paired rule then takes
    the partner's peak now and then: the honest cost of the rule and the reason it is off by default.  Printed (PAPERS.md holds the
    figures); asserted only where it is exact: swap_cost = 2 takes none, and is then the plain tracker."""
    maps, truth, c = unswapped
    p = tracking()
    plain = run(c, p, Pr.IDENTITY)
    lane0 = list(range(Pr.GROUP))
    apart = min(np.linalg.norm(truth[:, a] - truth[:, b], axis=-1).min() for a, b in Pr.PAIRS)
    picks = {}
    for cost in (0.0, 2.0):
        o = run(c, p, Pr.PARTNER, cost)
        picks[cost] = int((o["source"] == 1).sum())
        print("no swap, swap_cost %.1f: paired %.3f px against plain %.3f px rms over lane 0, %d measurements taken from the partner's map "
              "(partners come as close as %.1f px)" % (cost, A.rms((o["kp"] - truth)[:, lane0]), A.rms((plain["kp"] - truth)[:, lane0]),
                                                      picks[cost], apart))
    assert picks[2.0] == 0
    for k in ("kp", "status", "chosen"):
        assert np.array_equal(o[k], plain[k]), k


def test_the_swap_scenario_decides_nothing_on_a_rounding(swapped):
    """What tests/test_pose_pairs_gpu.py needs in order to ask for equal statuses, choices and sources of an fp32 kernel: at
    gate = 9.21 no d2 within 1e-3 (relative) of the gate and no two assignments of equal cardinality within 1e-3 in cost."""
    maps, truth, c = swapped
    p = tracking(gate=GATE)
    o = run(c, p, Pr.PARTNER)
    d2 = o["d2"][np.isfinite(o["d2"])]
    margin = np.abs(d2 / p.gate - 1.0).min()
    alt = o["alt"][np.isfinite(o["alt"])]
    default = run(c, tracking(), Pr.PARTNER)
    d2_default = default["d2"][np.isfinite(default["d2"])]
    print("gate %.3f: %d gate decisions, the nearest %.1e of the gate away (at the default 13.816: %.1e); %d units x frames with a second "
          "assignment of the same cardinality, the closest %.3f apart in cost"
          % (p.gate, d2.size, margin, np.abs(d2_default / 13.816 - 1.0).min(), alt.size, alt.min()))
    assert d2.size > 2500 and margin > 1e-3
    assert alt.size >= 10 and alt.min() > 1e-3                                  # not vacuous: some units do have a choice
    e, clean = Pr.swap_errors(o["kp"], truth)                                    # and the scenario shows the same at this gate
    assert e <= 1.5 * clean and (o["status"][Pr.SWAP_FRAMES[0]:, list(Pr.swapped_rows())] == ref.UPDATED).all()
    assert Pr.swap_errors(run(c, p, Pr.IDENTITY)["kp"], truth)[0] >= 5.0 * e and (o["source"] == 1).sum() > 150


# ---- hand-placed maps ------------------------------------------------------------------------------------------------------------------------
def test_one_peak_goes_to_the_cheaper_track_and_the_other_coasts_gated():
    maps = Pr.hand_one_peak()
    o, c = Pr.ref_run(maps, tracking(), Pr.HAND_PARTNER)
    assert o["status"][0].tolist() == [ref.STARTED, ref.STARTED] and c["count"][1].tolist() == [1, 1]
    assert o["usable"][1, :, 0].tolist() == [True, False]
    assert np.isfinite(o["cost"][1, 0, 0]) and np.isfinite(o["cost"][1, 1, 1])   # admissible for both: its own slot for row 0, the partner's for row 1
    assert o["cost"][1, 0, 0] < o["cost"][1, 1, 1]
    assert o["status"][1].tolist() == [ref.UPDATED, ref.COASTED_GATED]
    assert o["chosen"][1].tolist() == [0, -1] and o["source"][1].tolist() == [0, -1]
    alone = Pr.ref_run(maps, tracking(), (0, 1))[0]                              # by itself row 1 sees nothing usable
    assert alone["status"][1].tolist() == [ref.UPDATED, ref.COASTED_MISSING]


def test_a_dead_row_whose_candidate_was_taken_by_its_partner_stays_lost():
    maps = Pr.hand_taken_start()
    o, c = Pr.ref_run(maps, tracking(), Pr.HAND_PARTNER)
    assert o["status"][0].tolist() == [ref.LOST, ref.STARTED]
    for t in (1, 2):
        assert o["usable"][t, :, 0].tolist() == [True, False]
        assert o["status"][t].tolist() == [ref.LOST, ref.UPDATED], t
        assert o["chosen"][t].tolist() == [-1, 0] and o["source"][t].tolist() == [-1, 1]
        assert np.array_equal(o["kp"][t, 0], c["xy"][t, 0, 0])                   # LOST: the raw keypoint
    assert not o["state"][0].any()
    alone = Pr.ref_run(maps, tracking(), (0, 1))[0]                              # unpaired, row 0 starts from it
    assert alone["status"][1].tolist() == [ref.STARTED, ref.COASTED_MISSING]


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
GOOD = (10.0, 200.0, 1.0, 1.0, 13.816, 5, 50.0, 0.0, 0.0)
P = 4096                                                   # any non-null address: every call below returns before it launches


def table(*entries):
    return (ctypes.c_int * len(entries))(*entries)


def _pairs(L, heat=P, rows=28, state=P, params=GOOD, K=2, sep=3, floor=0.25, present=None, group=14, partner=Pr.PARTNER, swap=0.0,
           outs=(P,) * 13, H=64, W=64):
    return L.hupr_pose_track_pairs_f32(heat, rows, H, W, 4.0, 1, state, *params, K, sep, floor, present, group,
                                       None if partner is None else table(*partner), swap, *outs, None)


def test_the_entry_point_checks_its_arguments_on_the_host(L):
    assert _pairs(L, None, 0, None, (0.0,) * 5 + (0,) + (0.0,) * 3, 0, -1, 0.0, None, 0, None, -1.0, (None,) * 13) == 0     # rows == 0
    for bad in (dict(heat=None), dict(state=None), dict(partner=None)):
        assert _pairs(L, **bad) == -1 and b"null" in L.hupr_last_error(), bad
    for k in range(13):
        assert _pairs(L, outs=tuple(None if j == k else P for j in range(13))) == -1, k
        assert b"null" in L.hupr_last_error()
    assert _pairs(L, rows=-14) == -1 and b"shape" in L.hupr_last_error()
    assert _pairs(L, H=0) == -1 and b"shape" in L.hupr_last_error()
    for bad in (dict(K=0), dict(K=5), dict(sep=-1), dict(floor=0.0), dict(floor=1.5), dict(floor=float("nan"))):
        assert _pairs(L, **bad) == -1 and b"candidate parameter" in L.hupr_last_error(), bad
    assert _pairs(L, state=P + 4) == -1 and b"aligned" in L.hupr_last_error()
    assert _pairs(L, params=GOOD[:4] + (0.0,) + GOOD[5:]) == -1 and b"tracker parameter" in L.hupr_last_error()
    # the groups are read with or without presence flags
    for group, partner in ((0, ()), (-2, ()), (5, (0, 1, 2, 3, 4)), (33, tuple(range(33)))):
        assert _pairs(L, rows=28 if group != 33 else 66, group=group, partner=partner or (0,)) == -1, group
        assert b"rows_per_group" in L.hupr_last_error()
    for partner in ((14,) + Pr.PARTNER[1:], (-1,) + Pr.PARTNER[1:], (1, 2, 0) + tuple(range(3, 14)), (1,) + tuple(range(1, 14))):
        assert _pairs(L, partner=partner) == -1 and b"partner" in L.hupr_last_error(), partner
    for swap in (-0.5, float("nan"), float("inf")):
        assert _pairs(L, swap=swap) == -1 and b"swap_cost" in L.hupr_last_error(), swap


def test_pose_tracking_validates_the_pair_settings():
    from hupr_amd.tools import stream as st
    s = st.PoseTracking(10)
    assert (s.pair_swap, s.swap_cost, s.pairs) == (False, 0.0, None) and not s.associates and type(s.swap_cost) is float
    assert st.PoseTracking.PAIR_ARGUMENTS == ("pair_swap", "swap_cost", "pairs") and "unmeasured" in st.PoseTracking.__doc__
    assert "pair_swap" not in repr(s) and s.for_joints(Pr.JOINTS) is s
    s = st.PoseTracking(10, pair_swap=True, swap_cost=2, candidates=2, gate_on_presence=True)
    assert s.associates and s.pairs is None and s.swap_cost == 2.0
    assert repr(s).endswith("pair_swap=True, swap_cost=2.0, pairs=None)")
    r = s.for_joints(Pr.JOINTS)
    assert r.pairs == Pr.PARTNER and (r.pair_swap, r.swap_cost, r.candidates, r.gate_on_presence) == (True, 2.0, 2, True)
    h = r.with_horizon(0.3)
    assert h.horizon_s == 0.3 and h.pairs == Pr.PARTNER and h.pair_swap and h.swap_cost == 2.0
    own = st.PoseTracking(10, pair_swap=True, pairs=np.array([1, 0, 2]))
    assert own.pairs == (1, 0, 2) and type(own.pairs[0]) is int and own.for_joints("abc").pairs == (1, 0, 2)
    with pytest.raises(AttributeError):
        s.extra = 1
    for bad in (dict(pair_swap=1), dict(pair_swap=None), dict(swap_cost=-0.1), dict(swap_cost=float("nan")), dict(swap_cost=float("inf")),
                dict(swap_cost="0"), dict(swap_cost=True), dict(pairs=3), dict(pairs=()), dict(pairs=(1, 2, 0)), dict(pairs=(0, 2)),
                dict(pairs=(0, -1)), dict(pairs=(0.0, 1.0)), dict(pairs=(True, False)), dict(pairs=tuple(range(33)))):
        with pytest.raises(st.TrackingError):
            st.PoseTracking(10, **bad)
    with pytest.raises(st.TrackingError, match="pairs"):                        # a table for another skeleton
        own.for_joints(Pr.JOINTS)
    with pytest.raises(st.TrackingError, match="counterpart"):                  # a one-sided name
        s.for_joints(("L_Hip", "Neck"))


def test_test_tracking_forwards_the_pair_settings():
    from hupr_amd.tools.smooth import SequenceSmoother, temporal_setting
    from hupr_amd.tools import TrackingError
    cfg = lambda **test: types.SimpleNamespace(TEST=types.SimpleNamespace(**test),
                                               DATASET=types.SimpleNamespace(heatmapSize=64, idxToJoints=list(Pr.JOINTS)))
    t = temporal_setting(cfg(temporal="rts", tracking={"pair_swap": True, "swap_cost": 1.5}))
    assert t.tracking.pair_swap and t.tracking.swap_cost == 1.5 and t.tracking.pairs == Pr.PARTNER
    t = temporal_setting(cfg(temporal="track", tracking={"pair_swap": True, "pairs": list(Pr.IDENTITY)}))
    assert t.tracking.pairs == Pr.IDENTITY
    assert not temporal_setting(cfg(temporal="track")).tracking.pair_swap
    for bad in ({"pair_swap": 1}, {"swap_cost": -1}, {"pair_swap": True, "pairs": [1, 0]}, {"pairs": [1, 2, 0]}, {"swap": 2}):
        with pytest.raises(ValueError, match="TEST.tracking"):
            temporal_setting(cfg(temporal="track", tracking=bad))
    # the offline walker takes a table that fits its rows
    with pytest.raises(TrackingError, match="pairs"):
        SequenceSmoother(tracking(pair_swap=True), 14, "cpu")
    with pytest.raises(TrackingError, match="pairs"):
        SequenceSmoother(tracking(pair_swap=True, pairs=(1, 0)), 14, "cpu")
    assert SequenceSmoother(tracking(pair_swap=True).for_joints(Pr.JOINTS), 14, "cpu").tracking.pairs == Pr.PARTNER


def test_functional_refuses_bad_pair_arguments_and_cpu_tensors(L):
    from hupr_amd import functional as F_
    from hupr_amd.runtime import HuprError
    heat = torch.zeros((2, 3, 8, 8))
    state = F_.pose_track_state(6, "cpu")
    assert F_.MAX_GROUP_ROWS == 32 and F_.check_pair_table(np.array([1, 0, 2]), 1, 3) == ([1, 0, 2], 1.0)
    settings = lambda **kw: types.SimpleNamespace(**dict({k: getattr(tracking(), k) for k in F_._TRACK_PARAMS}, pair_swap=True, **kw))
    for bad in (dict(), dict(pairs=None), dict(pairs=(1, 0)), dict(pairs=(1, 2, 0)), dict(pairs=(0, 1, 3)), dict(pairs=(0.0, 1.0, 2.0)),
                dict(pairs=(0, 1, 2), swap_cost=-1.0), dict(pairs=(0, 1, 2), swap_cost=float("nan")), dict(pairs=(0, 1, 2), swap_cost=1e39),
                dict(pairs=(0, 1, 2), swap_cost="1")):
        with pytest.raises(ValueError, match="pairs|swap_cost"):
            F_.pose_track(heat, 4.0, track_state=state, tracking=settings(**bad))
    with pytest.raises(ValueError, match="groups of 1..32"):
        F_.pose_track(torch.zeros((40, 8, 8)), 4.0, track_state=F_.pose_track_state(40, "cpu"), tracking=settings(pairs=tuple(range(40))))
    with pytest.raises(HuprError):                                               # no CPU fallback
        F_.pose_track(heat, 4.0, track_state=state, tracking=settings(pairs=(1, 0, 2)))
    with pytest.raises(HuprError):
        F_.pose_track(heat, 4.0, track_state=state, tracking=tracking(pair_swap=True, pairs=(1, 0, 2), candidates=2))


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
    assert tuple(cfg.DATASET.idxToJoints) == Pr.JOINTS
    with pytest.raises(tools.TrackingError, match="pairs"):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, pair_swap=True, pairs=(1, 0)))
    with pytest.raises(HuprError):                                               # valid arguments reach the GPU check
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, pair_swap=True))
    with pytest.raises(HuprError):
        tools.PoseStream(_Cpu(), cfg, track=tools.PoseTracking(10.0, pair_swap=True, pairs=Pr.IDENTITY, swap_cost=1.0), predict_now=True)


def test_the_paired_frame_carries_the_source():
    from hupr_amd import tools
    from hupr_amd.tools.stream import PairedPoseFrame, PoseFrame, TrackedPoseFrame
    assert tools.PairedPoseFrame is PairedPoseFrame
    t = [torch.full((1,), float(i)) for i in range(9)] + [torch.full((1,), 3, dtype=torch.int32)]
    plain = TrackedPoseFrame(5, *t)
    assert plain.source is None and plain.clone().source is None and not hasattr(plain, "__dict__")
    source, chosen = torch.tensor([1, 0, -1], dtype=torch.int32), torch.tensor([0, 1, -1], dtype=torch.int32)
    pf = PairedPoseFrame(5, *t, chosen=chosen, source=source)
    assert pf.source is source and pf.chosen is chosen and pf.candidates is None and not hasattr(pf, "__dict__")
    assert isinstance(pf, TrackedPoseFrame) and isinstance(pf, PoseFrame) and torch.equal(pf.status, t[9])
    for c in (pf.clone(), pf.cpu()):
        assert type(c) is PairedPoseFrame and c.frame == 5 and torch.equal(c.source, source) and c.source.dtype == torch.int32
        assert torch.equal(c.chosen, chosen) and torch.equal(c.covariance, pf.covariance)
    assert pf.clone().source is not source
    assert PairedPoseFrame(5, *t).source is None and "source" in TrackedPoseFrame.__doc__


def test_stream_command_pair_arguments():
    from hupr_amd.tools import stream as st
    t = st.tracking_from_args(st.parse(["--raw", "x", "--track", "--rate", "10"]))
    assert (t.pair_swap, t.swap_cost, t.pairs) == (False, 0.0, None)
    t = st.tracking_from_args(st.parse(["--raw", "x", "--track", "--rate", "10", "--track-pairs"]))
    assert (t.pair_swap, t.swap_cost) == (True, 0.0)
    t = st.tracking_from_args(st.parse(["--raw", "x", "--track", "--rate", "10", "--track-pairs", "--track-swap-cost", "1.5",
                                        "--track-candidates", "2"]))
    assert (t.pair_swap, t.swap_cost, t.candidates) == (True, 1.5, 2)
    track = ["--track", "--rate", "10"]
    for bad in (["--track-pairs"], ["--track-swap-cost", "1"], track + ["--track-swap-cost", "1"],
                track + ["--track-pairs", "--track-swap-cost", "-1"], track + ["--track-pairs", "--track-swap-cost", "nan"],
                track + ["--track-pairs", "--track-swap-cost", "x"]):
        with pytest.raises(SystemExit):
            st.parse(["--raw", "x"] + bad)


def test_pose_pairs_kernel_uses_no_scratch():
    """The listing the build keeps for csrc/pose_pairs.hip: its one kernel, 64 threads, with 0 spilled vector registers and 0 bytes of
    scratch; the pool of at most 8 measurements and the two cost rows are its LDS — read from the code-object metadata only."""
    meta = kernel_metadata("pose_pairs")
    assert len(meta) == 1 and "hupr_k_pose_track_pairs" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    print(m)
    assert m["spill"] == 0 and m["scratch"] == 0, m
    assert m["threads"] == 64 and m["vgpr"] <= 128 and 0 < m["lds"] <= 1024, m
