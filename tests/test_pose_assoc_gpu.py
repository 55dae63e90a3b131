"""GPU (-m gpu): hupr_pose_track_assoc_f32 and hupr_pose_peaks_f32 (csrc/pose_assoc.hip) — the Kalman joint tracker that chooses its
measurement among up to four peaks of the heat-map — against the NumPy statement of the rule in tests/pose_assoc_ref.py.

Bounds.  With one candidate and no presence flags: bit equality with functional.pose_track, outputs and state.  Candidates: equal
counts, order and pixel indices; scores are the map's own floats; positions within TOL_PX = 1e-3 image pixel, the bound of
tests/test_pose_decode_gpu.py.  Recurrence: TOL_FILTER and TOL_COV_REL of tests/test_pose_track_gpu.py, for the same reasons: the
filter is the same code (csrc/pose_track_model.h).  Statuses and choices are asked to be equal because tests/test_pose_assoc_cpu.py
asserts that the distractor scenario decides nothing on a rounding: no d2 within 1 % of the gate, no two gated costs within 1e-3 (the
closest are 0.46 apart; an fp32 d2 + ln det S errs by about 1e-5), no local maximum within 1e-4 of the floor."""
import functools

import numpy as np
import pytest
import torch

import pose_assoc_ref as A
import pose_track_ref as ref

pytestmark = pytest.mark.gpu
TOL_PX = 1e-3
TOL_FILTER = 2e-3
TOL_COV_REL = 16 * 3.02e-7
OUT = ("idx", "maxval", "raw", "kp", "vel", "cov", "fc", "status")
CAND = ("cand_xy", "cand_score", "cand_count", "chosen")


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(dict(accel_psd=100.0, min_score=ref.MIN_SCORE), **kw))


def on_gpu(a):
    return torch.from_numpy(np.array(a)).cuda()


def assoc_entry(heat, state, p, K, present=None, group=1, ratio=ref.RATIO):
    """One frame through hupr_pose_track_assoc_f32 itself (functional.pose_track routes K = 1 without flags to the plain tracker)."""
    from hupr_amd import functional as F_, runtime as rt
    lead, (H, W) = tuple(heat.shape[:-2]), heat.shape[-2:]
    rows = int(np.prod(lead))
    new = lambda shape, dtype: torch.empty(lead + shape, dtype=dtype, device="cuda")
    o = dict(idx=new((), torch.int32), maxval=new((), torch.float32), raw=new((2,), torch.float32), kp=new((2,), torch.float32),
             vel=new((2,), torch.float32), cov=new((3,), torch.float32), fc=new((2,), torch.float32), status=new((), torch.int32),
             cand_xy=new((K, 2), torch.float32), cand_score=new((K,), torch.float32), cand_count=new((), torch.int32),
             chosen=new((), torch.int32))
    params = tuple(int(getattr(p, k)) if k == "max_coast" else float(getattr(p, k)) for k in F_._TRACK_PARAMS)
    rt.check(rt.lib().hupr_pose_track_assoc_f32(rt.ptr(heat), rows, H, W, ratio, 1, rt.ptr(state), *params, K, p.min_separation,
                                                p.peak_ratio, rt.ptr(present), group, *[rt.ptr(o[k]) for k in OUT + CAND], rt.stream()))
    return o


def track(heat, state, p, present=None):
    from hupr_amd import functional as F_
    out = F_.pose_track(heat, ref.RATIO, refine=True, track_state=state, tracking=p, present=present)
    assert len(out) == (12 if p.candidates > 1 or present is not None else 8)
    return dict(zip(OUT + CAND, out))


def stacked(seq, key):
    return np.stack([o[key].cpu().numpy() for o in seq])


# ---- (a): one candidate is the plain tracker ---------------------------------------------------------------------------------------------
def test_one_candidate_without_flags_is_pose_track_bit_for_bit():
    from hupr_amd import functional as F_
    heat, p = on_gpu(ref.scenario()[0]), tracking(horizon_s=0.3)
    s_old, s_new = F_.pose_track_state(ref.ROWS, "cuda"), F_.pose_track_state(ref.ROWS, "cuda")
    seen = set()
    for t in range(ref.T):
        old, new = track(heat[t], s_old, p), assoc_entry(heat[t], s_new, p, 1)
        for k in OUT:
            assert torch.equal(old[k], new[k]), (t, k)
        assert torch.equal(s_old, s_new), t
        seen |= set(old["status"].tolist())
        assert torch.equal(new["cand_xy"][:, 0], new["raw"]) and torch.equal(new["cand_score"][:, 0], new["maxval"])
        assert (new["cand_count"] == 1).all().item()
        assert torch.equal(new["chosen"], torch.where((new["status"] == ref.UPDATED) | (new["status"] == ref.STARTED), 0, -1).int())
    assert seen == {ref.UPDATED, ref.COASTED_MISSING, ref.COASTED_GATED, ref.STARTED, ref.LOST}


def test_a_map_without_a_positive_pixel_has_no_candidate_and_decodes_as_before():
    from hupr_amd import functional as F_
    maps = np.random.RandomState(3).uniform(-0.2, 1.0, (6, 8, 12)).astype(np.float32)
    maps[1] = -np.abs(maps[1])
    maps[2] = 0.0
    maps[3] = np.nan
    heat, p = on_gpu(maps), tracking(min_score=-1.0)
    s_old, s_new = F_.pose_track_state(6, "cuda"), F_.pose_track_state(6, "cuda")
    for t in range(2):
        old, new = track(heat, s_old, p), assoc_entry(heat, s_new, p, 3)
        rows = slice(0, 6) if t == 0 else slice(1, 4)     # the first frame starts every track from candidate 0; then K = 3 may choose
        for k in OUT:
            assert torch.equal(old[k][rows], new[k][rows]), (t, k)
        assert torch.equal(s_old[rows], s_new[rows])
        assert new["maxval"][3].item() == -np.inf and new["idx"][3].item() == 0x7fffffff          # all NaN: no maximum
        assert new["cand_count"][1:4].tolist() == [0, 0, 0] and new["chosen"][1:4].tolist() == [-1, -1, -1]
        assert not new["cand_xy"][1:4].any().item() and not new["cand_score"][1:4].any().item()
        assert new["status"][1:4].tolist() == [ref.LOST] * 3


# ---- (b): the peak finder alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", A.HAND_SHAPES, ids=["8x12", "64x64"])
def test_pose_peaks_finds_the_hand_placed_candidates(H, W):
    from hupr_amd import functional as F_
    maps, _ = A.hand_maps(H, W)
    want = A.ref_peaks(maps, A.HAND_K, A.HAND_SEPARATION, A.HAND_PEAK_RATIO, ref.RATIO)
    xy, score, idx, count = F_.pose_peaks(on_gpu(maps), ref.RATIO, A.HAND_K, A.HAND_SEPARATION, A.HAND_PEAK_RATIO)
    assert xy.shape == (len(maps), A.HAND_K, 2) and idx.dtype == torch.int32 and count.dtype == torch.int32
    assert np.array_equal(count.cpu().numpy(), want["count"])
    assert np.array_equal(idx.cpu().numpy(), want["idx"])                        # order and indices; zeros past the count
    assert np.array_equal(score.cpu().numpy(), want["score"])                    # the map's own floats
    err = np.abs(xy.cpu().numpy() - want["xy"]).max()
    print("%d x %d: %d candidates on %d maps, max |position - fp64| %.3e px" % (H, W, int(want["count"].sum()), len(maps), err))
    assert err <= TOL_PX
    assert want["count"].tolist() == [2, 2, 3, 2, 2, 0, 2, 4, 3]
    # without refinement the positions are the pixels; a smaller K is a prefix
    xy0, _, idx0, count0 = F_.pose_peaks(on_gpu(maps), ref.RATIO, 2, A.HAND_SEPARATION, A.HAND_PEAK_RATIO, refine=False)
    assert torch.equal(idx0, idx[:, :2]) and torch.equal(count0, count.clamp(max=2))
    px = torch.stack([idx0 % W, idx0 // W], dim=-1).float() * ref.RATIO
    assert torch.equal(xy0, px)


# ---- (c): the distractor scenario ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def distractor_run(K, run=0):
    from hupr_amd import functional as F_
    heat, p = on_gpu(A.distractor_scenario()[0]), tracking(candidates=K, horizon_s=0.3)
    state = F_.pose_track_state(ref.ROWS, "cuda")
    seq = []
    for t in range(ref.T):
        o = track(heat[t], state, p) if K > 1 else assoc_entry(heat[t], state, p, 1)
        o["state"] = state.clone()
        seq.append(o)
    return seq


def test_two_candidates_follow_the_fp64_rule_and_keep_the_track():
    from hupr_amd import functional as F_
    maps, truth = A.distractor_scenario()
    p = tracking(candidates=2, horizon_s=0.3)
    seq = distractor_run(2)
    # the candidates' pixels from the peak finder: the same kernel, and the tracker's launch must report the same candidates
    heat = on_gpu(maps)
    xy, score, idx, count = F_.pose_peaks(heat.reshape(ref.T * ref.ROWS, ref.HM, ref.HM), ref.RATIO, 2, p.min_separation, p.peak_ratio)
    g_xy, g_score, g_count = stacked(seq, "cand_xy"), stacked(seq, "cand_score"), stacked(seq, "cand_count")
    assert np.array_equal(xy.cpu().numpy().reshape(g_xy.shape), g_xy) and np.array_equal(score.cpu().numpy().reshape(g_score.shape), g_score)
    assert np.array_equal(count.cpu().numpy().reshape(g_count.shape), g_count)
    idx = idx.cpu().numpy().reshape(ref.T, ref.ROWS, 2)
    _, c64 = A.ref_run(maps, p)
    assert np.array_equal(idx, c64["idx"]) and np.array_equal(g_count, c64["count"]) and np.array_equal(g_score, c64["score"])
    assert np.abs(g_xy - c64["xy"]).max() <= TOL_PX
    # the restatement fed the GPU's own candidates and the fp64 window moments at their pixels
    mom = np.stack([A.candidate_moments(maps[t], idx[t], g_count[t]) for t in range(ref.T)])
    o64 = A.ref_assoc(g_xy, g_score, g_count, mom, p, ref.RATIO)
    status, chosen = stacked(seq, "status"), stacked(seq, "chosen")
    assert np.array_equal(status, o64["status"]) and np.array_equal(chosen, o64["chosen"])
    e_kp, e_fc = np.abs(stacked(seq, "kp") - o64["kp"]).max(), np.abs(stacked(seq, "fc") - o64["fc"]).max()
    e_vel = np.abs(stacked(seq, "vel") - o64["vel"]).max()
    e_cov = ref.cov_rel_diff(stacked(seq, "cov"), o64["cov"])
    print("association over %d frames x %d rows: max |filtered - fp64| %.3e px, |forecast - fp64| %.3e px, |velocity - fp64| %.3e px/s, "
          "covariance relative %.3e (bound %.3e); chosen %s" % (ref.T, ref.ROWS, e_kp, e_fc, e_vel, e_cov, TOL_COV_REL,
                                                                np.bincount(chosen.ravel() + 1, minlength=3).tolist()))
    assert e_kp <= TOL_FILTER and e_fc <= TOL_FILTER
    assert e_vel <= p.rate_hz * TOL_FILTER
    assert e_cov <= TOL_COV_REL
    assert np.array_equal(o64["state"][:, 14:], seq[-1]["state"][:, 14:].cpu().numpy())
    assert np.array_equal(stacked(seq, "raw"), g_xy[:, :, 0]) and np.array_equal(stacked(seq, "maxval"), g_score[:, :, 0])
    # the two orderings of tests/test_pose_assoc_cpu.py on the kernel's own output
    e2, clean = A.distractor_errors(stacked(seq, "kp"), truth)
    e1, clean1 = A.distractor_errors(stacked(distractor_run(1), "kp"), truth)
    print("rms error from frame %d on: K = 1 %.2f px, K = 2 %.2f px on the distracted rows, %.2f px on the untouched ones"
          % (A.GHOST_FRAMES[0], e1, e2, clean))
    assert e2 <= 1.5 * clean
    assert e1 >= 5.0 * e2
    assert clean1 == clean
    assert (chosen[list(A.GHOST_FRAMES)][:, list(A.DISTRACTED)] == 1).sum() > 100


# ---- (d): the presence flags ----------------------------------------------------------------------------------------------------------------------
def test_a_group_flagged_absent_coasts_and_resumes_and_the_others_do_not_notice():
    from hupr_amd import functional as F_
    heat = on_gpu(ref.scenario(events=False)[0]).reshape(ref.T, 2, 14, ref.HM, ref.HM)
    p, gone = tracking(), range(20, 25)
    s_flag, s_plain = F_.pose_track_state(ref.ROWS, "cuda"), F_.pose_track_state(ref.ROWS, "cuda")
    there, away = on_gpu(np.array([1, 1], np.int32)), on_gpu(np.array([0, 7], np.int32))
    seq, plain = [], []
    for t in range(ref.T):
        seq.append(track(heat[t], s_flag, p, present=away if t in gone else there))
        plain.append(track(heat[t], s_plain, p))
        for k in OUT:                                                            # group 1 is never flagged
            assert torch.equal(seq[t][k][1], plain[t][k][1]), (t, k)
        assert torch.equal(s_flag[14:], s_plain[14:]), t
    for t in gone:
        assert (seq[t]["status"][0] == ref.COASTED_MISSING).all().item(), t
        assert (seq[t]["chosen"][0] == -1).all().item() and (seq[t]["cand_count"][0] == 1).all().item()
        assert torch.equal(seq[t]["vel"][0], seq[19]["vel"][0]), t              # on the track's own velocity
        assert (seq[t]["cov"][0][:, [0, 2]] > seq[t - 1]["cov"][0][:, [0, 2]]).all().item(), t
        assert torch.equal(seq[t]["raw"][0], plain[t]["raw"][0])                 # the decode does not depend on the flag
    assert (seq[19]["status"][0] == ref.UPDATED).all().item() and (seq[25]["status"][0] == ref.UPDATED).all().item()
    assert (seq[25]["chosen"][0] == 0).all().item()
    # a row without a track stays LOST while its group is away, and starts when it is back
    state = F_.pose_track_state(ref.ROWS, "cuda")
    o = track(heat[0], state, p, present=away)
    assert (o["status"][0] == ref.LOST).all().item() and (o["status"][1] == ref.STARTED).all().item() and not state[:14].any().item()
    assert torch.equal(o["kp"][0], o["raw"][0]) and (o["chosen"][0] == -1).all().item() and (o["chosen"][1] == 0).all().item()
    assert (track(heat[1], state, p, present=there)["status"][0] == ref.STARTED).all().item()


# ---- (e): determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_identical_and_unused_slots_are_zero():
    a, b = distractor_run(2, run=0), distractor_run(2, run=1)
    assert a is not b
    holes = 0
    for t in range(ref.T):
        for k in OUT + CAND + ("state",):
            assert torch.equal(a[t][k], b[t][k]), (t, k)
        empty = torch.arange(2, device="cuda")[None] >= a[t]["cand_count"][:, None]
        holes += int(empty.sum().item())
        assert not a[t]["cand_xy"][empty].any().item() and not a[t]["cand_score"][empty].any().item()
    assert holes > ref.T * ref.ROWS // 2                                         # most maps show one peak
