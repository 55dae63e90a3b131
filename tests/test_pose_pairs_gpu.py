"""GPU (-m gpu): hupr_pose_track_pairs_f32 (csrc/pose_pairs.hip) — the Kalman joint tracker that assigns the left / right partners of a
skeleton jointly — against hupr_pose_track_assoc_f32 and against the NumPy statement of the rule in tests/pose_pairs_ref.py.

Bounds.  With every joint its own partner: bit equality with hupr_pose_track_assoc_f32, the twelve outputs and the state.  Recurrence:
TOL_FILTER and TOL_COV_REL of tests/test_pose_track_gpu.py, for the same reasons: the filter is the same code
(csrc/pose_track_model.h).  Statuses, choices and sources are asked to be equal because tests/test_pose_pairs_cpu.py asserts that the
swap scenario at gate = 9.21 decides nothing on a rounding: no d2 within 1e-3 of the gate (the nearest is 6.0e-3 away), no two
assignments of equal cardinality within 1e-3 in cost (the closest are 0.078 apart; an fp32 sum of two d2 + ln det S errs by about
1e-5).  Hand maps: the restatement runs on its own fp64 candidates, which lie within TOL_PX = 1e-3 pixel of the kernel's (the bound of
tests/test_pose_decode_gpu.py), so the filtered positions agree within TOL_PX + TOL_FILTER."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pose_assoc_ref as A
import pose_pairs_ref as Pr
import pose_track_ref as ref

pytestmark = pytest.mark.gpu
TOL_PX = 1e-3
TOL_FILTER = 2e-3
TOL_COV_REL = 16 * 3.02e-7
GATE = 9.21                  # tests/test_pose_pairs_cpu.py: the default gate has a d2 of the swap scenario 1.9e-5 from it
OUT = ("idx", "maxval", "raw", "kp", "vel", "cov", "fc", "status")
CAND = ("cand_xy", "cand_score", "cand_count", "chosen")
ALL = OUT + CAND + ("source",)


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(dict(accel_psd=100.0, min_score=ref.MIN_SCORE), **kw))


def on_gpu(a):
    return torch.from_numpy(np.array(a)).cuda()


def entry(heat, state, p, K, partner=None, swap_cost=0.0, group=1):
    """One frame of (rows, H, W) maps through hupr_pose_track_pairs_f32 itself, or with ``partner`` None through
    hupr_pose_track_assoc_f32."""
    from hupr_amd import functional as F_, runtime as rt
    rows, H, W = heat.shape
    new = lambda shape, dtype: torch.empty((rows,) + shape, dtype=dtype, device="cuda")
    o = dict(idx=new((), torch.int32), maxval=new((), torch.float32), raw=new((2,), torch.float32), kp=new((2,), torch.float32),
             vel=new((2,), torch.float32), cov=new((3,), torch.float32), fc=new((2,), torch.float32), status=new((), torch.int32),
             cand_xy=new((K, 2), torch.float32), cand_score=new((K,), torch.float32), cand_count=new((), torch.int32),
             chosen=new((), torch.int32))
    params = tuple(int(getattr(p, k)) if k == "max_coast" else float(getattr(p, k)) for k in F_._TRACK_PARAMS)
    head = (rt.ptr(heat), rows, H, W, ref.RATIO, 1, rt.ptr(state)) + params + (K, p.min_separation, p.peak_ratio, None)
    if partner is None:
        rt.check(rt.lib().hupr_pose_track_assoc_f32(*head, group, *[rt.ptr(o[k]) for k in OUT + CAND], rt.stream()))
    else:
        o["source"] = new((), torch.int32)
        rt.check(rt.lib().hupr_pose_track_pairs_f32(*head, group, (ctypes.c_int * group)(*partner), swap_cost,
                                                    *[rt.ptr(o[k]) for k in ALL], rt.stream()))
    return o


def track(heat, state, p, present=None):
    from hupr_amd import functional as F_
    out = F_.pose_track(heat, ref.RATIO, refine=True, track_state=state, tracking=p, present=present)
    assert len(out) == (13 if p.pair_swap else 12 if p.candidates > 1 or present is not None else 8)
    return dict(zip(ALL, out))


def stacked(seq, key, lead=2):
    """The outputs ``key`` of every frame, their ``lead`` leading axes flattened into rows -> (T, rows, ...)."""
    return np.stack([o[key].cpu().numpy() for o in seq]).reshape((len(seq), -1) + tuple(seq[0][key].shape[lead:]))


def lanes(maps):
    """(T, 28, H, W) -> (T, 2, 14, H, W): the last lead axis is the group of joints."""
    return on_gpu(maps).reshape(maps.shape[0], 2, Pr.GROUP, *maps.shape[2:])


# ---- (1): every joint its own partner is the associating tracker ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 2))
def test_the_identity_table_is_pose_track_assoc_bit_for_bit(K):
    from hupr_amd import functional as F_
    heat, p = on_gpu(ref.scenario()[0]), tracking(horizon_s=0.3)
    s_old, s_new = F_.pose_track_state(ref.ROWS, "cuda"), F_.pose_track_state(ref.ROWS, "cuda")
    seen = set()
    for t in range(ref.T):
        old, new = entry(heat[t], s_old, p, K), entry(heat[t], s_new, p, K, Pr.IDENTITY, 0.0, Pr.GROUP)
        for k in OUT + CAND:
            assert torch.equal(old[k], new[k]), (t, k)
        assert torch.equal(s_old, s_new), t
        assert torch.equal(new["source"], torch.where(new["chosen"] >= 0, 0, -1).int()), t
        seen |= set(old["status"].tolist())
    assert seen == {ref.UPDATED, ref.COASTED_MISSING, ref.COASTED_GATED, ref.STARTED, ref.LOST}


# ---- (2): the swap scenario ---------------------------------------------------------------------------------------------------------------------
def paired_settings():
    return tracking(gate=GATE, horizon_s=0.3, pair_swap=True, pairs=Pr.PARTNER)


@functools.lru_cache(maxsize=None)
def swap_run(paired=True, run=0):
    from hupr_amd import functional as F_
    heat = lanes(Pr.swap_scenario()[0])
    p = paired_settings() if paired else tracking(gate=GATE, horizon_s=0.3)
    state = F_.pose_track_state(ref.ROWS, "cuda")
    seq = []
    for t in range(ref.T):
        o = track(heat[t], state, p)
        o["state"] = state.clone()
        seq.append(o)
    return seq


def test_a_swap_follows_the_fp64_rule_and_keeps_both_tracks():
    from hupr_amd import functional as F_
    maps, truth = Pr.swap_scenario()
    p = paired_settings()
    seq = swap_run(True, 0)
    # the candidates' pixels from the peak finder, and the launch reports the same candidates
    xy, score, idx, count = F_.pose_peaks(on_gpu(maps).reshape(ref.T * ref.ROWS, ref.HM, ref.HM), ref.RATIO, 1, p.min_separation, p.peak_ratio)
    g_xy, g_score, g_count = stacked(seq, "cand_xy"), stacked(seq, "cand_score"), stacked(seq, "cand_count")
    assert np.array_equal(xy.cpu().numpy().reshape(g_xy.shape), g_xy) and np.array_equal(score.cpu().numpy().reshape(g_score.shape), g_score)
    assert np.array_equal(count.cpu().numpy().reshape(g_count.shape), g_count)
    idx = idx.cpu().numpy().reshape(ref.T, ref.ROWS, 1)
    # the restatement fed the GPU's own candidates and the fp64 window moments at their pixels
    mom = np.stack([A.candidate_moments(maps[t], idx[t], g_count[t]) for t in range(ref.T)])
    o64 = Pr.ref_pairs(g_xy, g_score, g_count, mom, p, ref.RATIO, Pr.PARTNER, 0.0)
    status, chosen, source = stacked(seq, "status"), stacked(seq, "chosen"), stacked(seq, "source")
    assert np.array_equal(status, o64["status"]) and np.array_equal(chosen, o64["chosen"]) and np.array_equal(source, o64["source"])
    e_kp, e_fc = np.abs(stacked(seq, "kp") - o64["kp"]).max(), np.abs(stacked(seq, "fc") - o64["fc"]).max()
    e_vel = np.abs(stacked(seq, "vel") - o64["vel"]).max()
    e_cov = ref.cov_rel_diff(stacked(seq, "cov"), o64["cov"])
    print("joint assignment over %d frames x %d rows: max |filtered - fp64| %.3e px, |forecast - fp64| %.3e px, |velocity - fp64| %.3e "
          "px/s, covariance relative %.3e (bound %.3e); source %s" % (ref.T, ref.ROWS, e_kp, e_fc, e_vel, e_cov, TOL_COV_REL,
                                                                       np.bincount(source.ravel() + 1, minlength=3).tolist()))
    assert e_kp <= TOL_FILTER and e_fc <= TOL_FILTER
    assert e_vel <= p.rate_hz * TOL_FILTER
    assert e_cov <= TOL_COV_REL
    assert np.array_equal(o64["state"][:, 14:], seq[-1]["state"][:, 14:].cpu().numpy())
    assert np.array_equal(stacked(seq, "raw"), g_xy[:, :, 0]) and np.array_equal(stacked(seq, "maxval"), g_score[:, :, 0])
    # the orderings of tests/test_pose_pairs_cpu.py on the kernel's own output
    rows, t0 = list(Pr.swapped_rows()), Pr.SWAP_FRAMES[0]
    e_pair, clean = Pr.swap_errors(stacked(seq, "kp"), truth)
    plain = swap_run(False, 0)
    e_plain, clean_plain = Pr.swap_errors(stacked(plain, "kp"), truth)
    print("rms error from frame %d on: plain %.2f px, paired %.2f px on the swapped rows, %.2f px on the untouched lane" % (t0, e_plain, e_pair, clean))
    assert e_pair <= 1.5 * clean
    assert e_plain >= 5.0 * e_pair
    assert clean_plain == clean
    assert (status[t0:, rows] == ref.UPDATED).all()
    assert (source[:, rows] == 1).sum() > 150
    # the row's own decode does not depend on the option
    for k in ("idx", "maxval", "raw"):
        assert np.array_equal(stacked(seq, k), stacked(plain, k)), k


# ---- (3): the hand maps ---------------------------------------------------------------------------------------------------------------------------
def hand_run(maps, partner):
    from hupr_amd import functional as F_
    p = tracking(pair_swap=True, pairs=partner)
    heat, state = on_gpu(maps), F_.pose_track_state(2, "cuda")
    seq = [track(heat[t], state, p) for t in range(len(maps))]
    want = Pr.ref_run(maps, p, partner)[0]
    for k in ("status", "chosen", "source"):
        assert np.array_equal(stacked(seq, k, 1), want[k]), k
    assert np.abs(stacked(seq, "kp", 1) - want["kp"]).max() <= TOL_PX + TOL_FILTER
    return seq, state


def test_one_peak_goes_to_the_cheaper_track_and_the_other_coasts_gated():
    seq, _ = hand_run(Pr.hand_one_peak(), Pr.HAND_PARTNER)
    assert seq[1]["status"].tolist() == [ref.UPDATED, ref.COASTED_GATED]
    assert seq[1]["chosen"].tolist() == [0, -1] and seq[1]["source"].tolist() == [0, -1]
    alone, _ = hand_run(Pr.hand_one_peak(), (0, 1))
    assert alone[1]["status"].tolist() == [ref.UPDATED, ref.COASTED_MISSING]


def test_a_dead_row_whose_candidate_was_taken_by_its_partner_stays_lost():
    seq, state = hand_run(Pr.hand_taken_start(), Pr.HAND_PARTNER)
    for t in (1, 2):
        assert seq[t]["status"].tolist() == [ref.LOST, ref.UPDATED], t
        assert seq[t]["chosen"].tolist() == [-1, 0] and seq[t]["source"].tolist() == [-1, 1]
        assert torch.equal(seq[t]["kp"][0], seq[t]["raw"][0])
    assert not state[0].any().item() and state[1, 14].item() == 1.0
    alone, _ = hand_run(Pr.hand_taken_start(), (0, 1))
    assert alone[1]["status"].tolist() == [ref.STARTED, ref.COASTED_MISSING]


# ---- (4): the presence flags ----------------------------------------------------------------------------------------------------------------------
def test_a_group_flagged_absent_coasts_and_the_other_does_not_notice():
    from hupr_amd import functional as F_
    heat = lanes(ref.scenario(events=False)[0])
    p, gone = tracking(pair_swap=True, pairs=Pr.PARTNER), range(20, 25)
    s_flag, s_plain = F_.pose_track_state(ref.ROWS, "cuda"), F_.pose_track_state(ref.ROWS, "cuda")
    there, away = on_gpu(np.array([1, 1], np.int32)), on_gpu(np.array([0, 7], np.int32))
    for t in range(26):
        flagged, plain = track(heat[t], s_flag, p, present=away if t in gone else there), track(heat[t], s_plain, p)
        for k in ALL:                                                            # group 1 is never flagged
            assert torch.equal(flagged[k][1], plain[k][1]), (t, k)
        assert torch.equal(s_flag[14:], s_plain[14:]), t
        if t in gone:
            assert (flagged["status"][0] == ref.COASTED_MISSING).all().item(), t
            assert (flagged["chosen"][0] == -1).all().item() and (flagged["source"][0] == -1).all().item()
            assert torch.equal(flagged["raw"][0], plain["raw"][0])               # the decode does not depend on the flag
        elif t in (19, 25):
            assert (flagged["status"][0] == ref.UPDATED).all().item(), t


def test_the_offline_walker_tracks_pairs_and_its_history_smooths():
    """tools.SequenceSmoother (what Runner.eval walks the test set with under TEST.temporal) on lane 0 of the swap scenario: the pair
    tracker's 13 outputs, those of functional.pose_track on a state of its own, and a history the RTS pass reads as it is."""
    from hupr_amd import functional as F_
    from hupr_amd.tools import SequenceSmoother
    heat = lanes(Pr.swap_scenario()[0])[:, 0]
    p = tracking(pair_swap=True).for_joints(Pr.JOINTS)
    walker, state = SequenceSmoother(p, Pr.GROUP, "cuda"), F_.pose_track_state(Pr.GROUP, "cuda")
    taken = 0
    for t in range(30):
        got, want = walker.track(heat[t], ref.RATIO), track(heat[t], state, p)
        assert len(got) == 13
        for g, k in zip(got, ALL):
            assert torch.equal(g, want[k]), (t, k)
        taken += int((want["source"] == 1).sum().item())
    assert torch.equal(walker.state, state) and taken > 50
    seq = walker.smooth()
    assert len(seq) == 30 and seq.keypoints.shape == (30, Pr.GROUP, 2) and torch.isfinite(seq.keypoints).all().item()


# ---- (5): determinism -------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_identical():
    a, b = swap_run(True, 0), swap_run(True, 1)
    assert a is not b
    for t in range(ref.T):
        for k in ALL + ("state",):
            assert torch.equal(a[t][k], b[t][k]), (t, k)
