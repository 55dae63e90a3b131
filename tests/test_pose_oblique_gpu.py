"""GPU (-m gpu): every kernel of the pose-tracker family on the oblique scenario of tests/pose_oblique_ref.py — 24 frames x 12 rows of
20 x 27 maps, each one rotated anisotropic Gaussian, four rows at the map's borders, at the parameter points A and B, with both
decodes — against the fp64 restatements: hupr_pose_measure_f32, hupr_pose_track_f32, hupr_pose_track_assoc_f32,
hupr_pose_track_pairs_f32, hupr_pose_track_imm_f32, hupr_pose_track_nll_f32, hupr_pose_smooth_rts_f32, hupr_pose_smooth_lag_f32.

The family's other scenarios are isotropic Gaussians inside a 64 x 64 map: Sxy, Pxy and the state's P03, P12, P23 are zero to rounding
there, and about half of the filter's arithmetic is multiplied by 1e-8.  Here the median |Sxy| / sqrt(Sxx Syy) is 0.54 and the state's
cross correlations 0.2 to 0.45; tests/test_pose_oblique_cpu.py asserts that, and that forcing any of them to 0 moves the answers by
at least 100 x the bounds below.

Each fp64 rule is fed the kernel's own idx, maxval and raw keypoints (first asserted bit-equal to functional.pose_decode) and the fp64
window moments of the same float32 maps, so only the moments and the filter are measured; the smoothers are fed the recorded fp32
states of the tracker's run.

Bounds.  Statuses, flags, counts, choices and sources: equal — tests/test_pose_oblique_cpu.py asserts that no decision sits on a
rounding, and every test here asserts it again on the fp64 run fed the kernel's decode.  Window moments: TOL_MOMENT of
tests/test_pose_track_gpu.py (49 terms, values <= 9).  Positions, velocities, covariance (pose_track_ref.cov_rel_diff), the tracker's
whole state covariance (pose_oblique_ref.state_cov_diff), ``moving`` and the likelihood sums: 16 x what the NumPy fp32 run of that rule
differs from its fp64 run at that point (pose_oblique_ref.FP32; tests/test_pose_oblique_cpu.py measures and holds it) — the family's
margin for FMA contraction, the order of sums and the device's exp and ln.  The forecast kp + horizon_s vel: the position bound plus
horizon_s x the velocity bound.  The associating and the pair tracker have no fp32 restatement; they compile the tracker's filter
(csrc/pose_track_model.h) and are held to the tracker's figures.  Candidate positions: TOL_PX = 1e-3 pixel, the bound of
tests/test_pose_decode_gpu.py.  The fixed-lag kernel's cross terms are carried by its covariance and by the bit equality of every
window of its ring with the fixed-interval kernel: its lagged keypoints move too little with them (tests/test_pose_oblique_cpu.py).
Every test prints what the GPU shows beside its bound; DESIGN.md has the table.

Every test is at most a few runs of 24 launches of 12 rows."""
import functools

import numpy as np
import pytest
import torch

import pose_assoc_ref as A
import pose_oblique_ref as ob
import pose_pairs_ref as Pr
import pose_smooth_ref as sr
import pose_track_ref as ref

pytestmark = pytest.mark.gpu
POINT = pytest.mark.parametrize("point", ob.POINTS)
REFINE = pytest.mark.parametrize("refine", [False, True], ids=["argmax", "subpixel"])
TOL_PX = 1e-3
OUT = ("idx", "maxval", "raw", "kp", "vel", "cov", "fc", "status")
CAND = ("cand_xy", "cand_score", "cand_count", "chosen")
NAMES = {8: OUT, 9: OUT + ("moving",), 12: OUT + CAND, 13: OUT + CAND + ("source",)}
ALL_CODES = {ref.UPDATED, ref.COASTED_MISSING, ref.COASTED_GATED, ref.STARTED, ref.LOST}
# kind -> (maps, what the point's parameters are changed by, whether a presence flag goes with the launch)
KINDS = {"plain": ("plain", {}, False),
         "flagged": ("plain", {}, True),
         "ghost2": ("ghost", dict(candidates=2), False),
         "ghost2 identity": ("ghost", dict(candidates=2, pair_swap=True, pairs=ob.IDENTITY), False),
         "pairs": ("pair", dict(pair_swap=True, pairs=ob.PARTNER), False),
         "imm": ("plain", dict(ob.IMM), False),
         "imm off": ("plain", dict(accel_psd_moving=ob.IMM["accel_psd_moving"], switch_prob=0.0, moving_prior=0.0), False)}


def tracking(point, **kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(**vars(ob.params(point, **kw)))


def maps_of(which):
    return {"plain": ob.scenario, "ghost": ob.ghost_scenario, "pair": ob.pair_scenario}[which]()[0]


@functools.lru_cache(maxsize=None)
def heat(which):
    return torch.from_numpy(np.array(maps_of(which))).cuda()


@functools.lru_cache(maxsize=None)
def gpu_run(kind, point, refine, run=0):
    """The maps of ``kind`` through functional.pose_track from a fresh state, one launch per frame -> [per frame: dict of the launch's
    outputs and a copy of the state after it]."""
    from hupr_amd import functional as F_
    which, change, flagged = KINDS[kind]
    h, p = heat(which), tracking(point, **change)
    state = (F_.pose_imm_state if p.maneuvers else F_.pose_track_state)(ob.ROWS, "cuda")
    present = torch.ones(1, dtype=torch.int32, device="cuda") if flagged else None
    seq = []
    for t in range(ob.T):
        out = F_.pose_track(h[t][None] if flagged else h[t], ob.RATIO[point], refine=refine, track_state=state, tracking=p, present=present)
        o = {k: (v[0] if flagged else v) for k, v in zip(NAMES[len(out)], out)}
        o["state"] = state.clone()
        seq.append(o)
    return seq


def stacked(seq, key):
    return np.stack([o[key].cpu().numpy() for o in seq])


def same_bits(a, b, keys, what):
    for t in range(ob.T):
        for k in keys:
            assert torch.equal(a[t][k], b[t][k]), (what, t, k)


def the_decode_is_pose_decode(seq, which, point, refine):
    """idx, maxval and the raw keypoints of every launch of ``seq`` are functional.pose_decode's bits."""
    from hupr_amd import functional as F_
    idx, mx, raw, _, _ = F_.pose_decode(heat(which), ob.RATIO[point], refine=refine)
    for t in range(ob.T):
        assert torch.equal(seq[t]["idx"], idx[t]) and torch.equal(seq[t]["maxval"], mx[t]) and torch.equal(seq[t]["raw"], raw[t]), t


def shown(rule, point, refine, figures):
    """Prints every (what, shown, bound) of ``figures`` as a line of the table, then asserts them all."""
    for what, got, tol in figures:
        print("| %-14s | %s | %-8s | %-18s | %.2e | %.2e |" % (rule, point, "subpixel" if refine else "arg-max", what, got, tol))
    for what, got, tol in figures:
        assert got <= tol, (rule, point, what, got, tol)


def filter_figures(seq, o64, rule, point, p):
    """The four figures every tracker shows against its fp64 run: keypoints, forecast, velocity, covariance."""
    pos, vel = ob.bound(rule, point, "pos"), ob.bound(rule, point, "vel")
    return [("keypoints px", np.abs(stacked(seq, "kp") - o64["kp"]).max(), pos),
            ("forecast px", np.abs(stacked(seq, "fc") - o64["fc"]).max(), pos + p.horizon_s * vel),
            ("velocity px/s", np.abs(stacked(seq, "vel") - o64["vel"]).max(), vel),
            ("covariance rel", ref.cov_rel_diff(stacked(seq, "cov"), o64["cov"]), ob.bound(rule, point, "cov"))]


def gate_margin(d2, gate):
    d = d2[np.isfinite(d2)]
    return float(np.abs(d / gate - 1.0).min())


# ---- pose_measure ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measured(point, refine, run=0):
    """functional.pose_measure over all 24 x 12 maps in one launch -> (idx, maxval, raw, meas (T, ROWS, 8))."""
    from hupr_amd import functional as F_
    return F_.pose_measure(heat("plain"), ob.RATIO[point], refine=refine)


@REFINE
@POINT
def test_pose_measure_gives_the_fp64_window_moments_at_the_borders_too(point, refine):
    from hupr_amd import functional as F_
    from test_pose_track_gpu import TOL_MOMENT
    idx, mx, raw, meas = measured(point, refine)
    d_idx, d_mx, d_raw, _, _ = F_.pose_decode(heat("plain"), ob.RATIO[point], refine=refine)
    assert torch.equal(idx, d_idx) and torch.equal(mx, d_mx) and torch.equal(raw, d_raw)
    assert torch.equal(meas[..., 0:2], raw) and torch.equal(meas[..., 2], mx) and not meas[..., 7].any().item()
    idx = idx.cpu().numpy()
    want = ob.moments(maps_of("plain"), idx)
    got = meas[..., 3:7].cpu().numpy().astype(np.float64)
    assert np.isfinite(want).all() and (want[..., 0] > 0).all()                 # every map has a positive peak, the faint ones too
    edge = ob.edge_distance(idx)
    assert (edge[:, list(ob.BORDER)] < ref.RADIUS).all() and (edge[:, list(ob.INTERIOR)] >= ref.RADIUS).all()
    err = np.abs(got[..., 1:] - want[..., 1:])
    rho = np.abs(want[..., 2]) / np.sqrt(want[..., 1] * want[..., 3])
    assert np.median(rho) >= 0.3
    shown("pose_measure", point, refine, [("moments border", err[:, list(ob.BORDER)].max(), TOL_MOMENT),
                                          ("moments interior", err[:, list(ob.INTERIOR)].max(), TOL_MOMENT),
                                          ("mass rel", np.abs(got[..., 0] / want[..., 0] - 1.0).max(), 1e-5)])


# ---- pose_track --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fp64_track(point, refine):
    """ref_track and its state after every frame, fed the kernel's decode and the fp64 moments at its pixels."""
    seq = gpu_run("plain", point, refine)
    mom = ob.moments(maps_of("plain"), stacked(seq, "idx"))
    return ob.track_run(point, stacked(seq, "raw"), stacked(seq, "maxval"), mom)


@REFINE
@POINT
def test_the_tracker_follows_the_fp64_rule(point, refine):
    seq, p = gpu_run("plain", point, refine), ob.params(point)
    the_decode_is_pose_decode(seq, "plain", point, refine)
    o64, states64 = fp64_track(point, refine)
    margin = gate_margin(o64["d2"], p.gate)
    status = stacked(seq, "status")
    print("%s: statuses %s; the nearest gate decision %.1f %% of the gate away" % (point, np.bincount(status.ravel(), minlength=5).tolist(), 100 * margin))
    assert margin > 0.01 and set(np.unique(o64["status"])) == ALL_CODES
    assert np.array_equal(status, o64["status"])                                # every row, every frame, the border rows too
    states = stacked(seq, "state")
    assert np.array_equal(states[..., 14:], states64[..., 14:])                 # live and coast after every frame
    figures = filter_figures(seq, o64, "track", point, p)
    figures += [("state xy px", np.abs(states[..., 0:2] - states64[..., 0:2]).max(), ob.bound("track", point, "pos")),
                ("state v px/s", np.abs(states[..., 2:4] - states64[..., 2:4]).max(), ob.bound("track", point, "vel")),
                ("state P rel", ob.state_cov_diff(states, states64), ob.bound("track", point, "state"))]
    # row by row, so that a residual names its rows: the border rows and the interior ones
    for name, rows in (("border", list(ob.BORDER)), ("interior", list(ob.INTERIOR))):
        print("%s rows: keypoints %.2e px, covariance %.2e" % (name, np.abs(stacked(seq, "kp") - o64["kp"])[:, rows].max(),
                                                               ref.cov_rel_diff(stacked(seq, "cov")[:, rows], o64["cov"][:, rows])))
    shown("pose_track", point, refine, figures)
    assert np.array_equal(o64["state"], states64[-1]) and p.horizon_s > 0
    # the outputs are the state's own entries
    for o in seq:
        live = o["state"][:, 14] == 1
        assert torch.equal(o["kp"][live], o["state"][live][:, 0:2]) and torch.equal(o["vel"], o["state"][:, 2:4])
        assert torch.equal(o["cov"], o["state"][:, [4, 5, 8]])
        assert torch.equal(o["kp"][~live], o["raw"][~live])


# ---- pose_track with candidates ----------------------------------------------------------------------------------------------------------
def candidates_of(seq, which, point, refine, K, p):
    """The launch's candidates against functional.pose_peaks (the same kernel) and against the restated peak finder -> (xy, score,
    count, idx) of the GPU as (T, ROWS, K, ...) arrays."""
    from hupr_amd import functional as F_
    xy, score, idx, count = F_.pose_peaks(heat(which), ob.RATIO[point], K, p.min_separation, p.peak_ratio, refine=refine)
    g_xy, g_score, g_count = stacked(seq, "cand_xy"), stacked(seq, "cand_score"), stacked(seq, "cand_count")
    assert np.array_equal(xy.cpu().numpy(), g_xy) and np.array_equal(score.cpu().numpy(), g_score) and np.array_equal(count.cpu().numpy(), g_count)
    idx = idx.cpu().numpy()
    maps = maps_of(which)
    per = [A.ref_peaks(maps[t], K, p.min_separation, p.peak_ratio, ob.RATIO[point], refine) for t in range(ob.T)]
    c64 = {k: np.stack([o[k] for o in per]) for k in per[0]}
    assert np.array_equal(idx, c64["idx"]) and np.array_equal(g_count, c64["count"]) and np.array_equal(g_score, c64["score"])
    assert np.abs(g_xy - c64["xy"]).max() <= (TOL_PX if refine else 0.0)
    assert np.array_equal(stacked(seq, "raw"), g_xy[:, :, 0]) and np.array_equal(stacked(seq, "maxval"), g_score[:, :, 0])
    return g_xy, g_score, g_count, idx


@REFINE
@POINT
def test_two_candidates_on_the_ghost_variant_follow_the_fp64_rule(point, refine):
    seq, p = gpu_run("ghost2", point, refine), ob.params(point, candidates=2)
    the_decode_is_pose_decode(seq, "ghost", point, refine)
    g_xy, g_score, g_count, idx = candidates_of(seq, "ghost", point, refine, 2, p)
    maps = maps_of("ghost")
    mom = np.stack([A.candidate_moments(maps[t], idx[t], g_count[t]) for t in range(ob.T)])
    o64 = A.ref_assoc(g_xy, g_score, g_count, mom, p, ob.RATIO[point])
    cost = np.sort(np.where(np.isfinite(o64["cost"]), o64["cost"], np.inf), axis=-1)
    both = np.isfinite(cost[..., 1])
    margin, gap = gate_margin(o64["d2"], p.gate), (cost[both][:, 1] - cost[both][:, 0]).min()
    chosen = stacked(seq, "chosen")
    print("%s: the nearest gate decision %.1f %% of the gate away, %d frames x rows with two gated candidates, the closest costs %.3f "
          "apart; chosen %s" % (point, 100 * margin, int(both.sum()), gap, np.bincount(chosen.ravel() + 1, minlength=3).tolist()))
    assert margin > 0.01 and both.sum() >= 10 and gap > 1e-3
    assert np.array_equal(stacked(seq, "status"), o64["status"]) and np.array_equal(chosen, o64["chosen"])
    assert (g_count[list(ob.GHOST_FRAMES)][:, list(ob.GHOST_ROWS)] == 2).sum() >= 100
    assert (chosen[list(ob.GHOST_FRAMES)][:, list(ob.GHOST_ROWS)] == 1).sum() >= 100         # the ghost is the arg-max, the joint is taken
    shown("pose_track K=2", point, refine, filter_figures(seq, o64, "track", point, p)
          + [("state P rel", ob.state_cov_diff(seq[-1]["state"].cpu().numpy(), o64["state"]), ob.bound("track", point, "state"))])
    assert np.array_equal(o64["state"][:, 14:], seq[-1]["state"][:, 14:].cpu().numpy())


@REFINE
@POINT
def test_one_candidate_with_presence_flags_is_the_tracker_bit_for_bit(point, refine):
    plain, flagged = gpu_run("plain", point, refine), gpu_run("flagged", point, refine)
    assert "chosen" in flagged[0] and "chosen" not in plain[0]                   # the associating kernel's launch
    same_bits(plain, flagged, OUT + ("state",), "one candidate")
    assert {int(s) for o in plain for s in o["status"].tolist()} == ALL_CODES
    for o in flagged:
        assert (o["cand_count"] == 1).all().item() and torch.equal(o["cand_xy"][:, 0], o["raw"])
        assert torch.equal(o["chosen"], torch.where((o["status"] == ref.UPDATED) | (o["status"] == ref.STARTED), 0, -1).int())


# ---- pose_track with pair_swap -----------------------------------------------------------------------------------------------------------
@REFINE
@POINT
def test_the_pair_tracker_on_the_pair_variant_follows_the_fp64_rule(point, refine):
    seq, p = gpu_run("pairs", point, refine), ob.params(point, pair_swap=True, pairs=ob.PARTNER)
    the_decode_is_pose_decode(seq, "pair", point, refine)
    g_xy, g_score, g_count, idx = candidates_of(seq, "pair", point, refine, 1, p)
    maps = maps_of("pair")
    mom = np.stack([A.candidate_moments(maps[t], idx[t], g_count[t]) for t in range(ob.T)])
    o64 = Pr.ref_pairs(g_xy, g_score, g_count, mom, p, ob.RATIO[point], ob.PARTNER, 0.0)
    alt = o64["alt"][np.isfinite(o64["alt"])]
    margin = gate_margin(o64["d2"], p.gate)
    source = stacked(seq, "source")
    print("%s: the nearest gate decision %.1f %% of the gate away, %d units with a second assignment of equal cardinality, the closest "
          "%.3f apart; source %s" % (point, 100 * margin, alt.size, alt.min(), np.bincount(source.ravel() + 1, minlength=3).tolist()))
    assert margin > 0.01 and alt.size >= 10 and alt.min() > 1e-3
    assert np.array_equal(stacked(seq, "status"), o64["status"]) and np.array_equal(stacked(seq, "chosen"), o64["chosen"])
    assert np.array_equal(source, o64["source"])
    swapped = [r for pair in ob.PAIRS for r in pair]
    assert (source[list(ob.SWAP_FRAMES)][:, swapped] == 1).sum() >= 40 and (source[:, list(ob.BORDER)] <= 0).all()
    shown("pose_track pairs", point, refine, filter_figures(seq, o64, "track", point, p)
          + [("state P rel", ob.state_cov_diff(seq[-1]["state"].cpu().numpy(), o64["state"]), ob.bound("track", point, "state"))])
    assert np.array_equal(o64["state"][:, 14:], seq[-1]["state"][:, 14:].cpu().numpy())


@REFINE
@POINT
def test_the_identity_table_is_the_associating_tracker_bit_for_bit(point, refine):
    assoc, pairs = gpu_run("ghost2", point, refine), gpu_run("ghost2 identity", point, refine)
    assert "source" in pairs[0] and "source" not in assoc[0]
    same_bits(assoc, pairs, OUT + CAND + ("state",), "identity table")
    for o in pairs:
        assert torch.equal(o["source"], torch.where(o["chosen"] >= 0, 0, -1).int())
    assert sum(int((o["chosen"] == 1).sum().item()) for o in assoc) >= 100


# ---- pose_track with accel_psd_moving ----------------------------------------------------------------------------------------------------
@REFINE
@POINT
def test_the_two_model_tracker_follows_the_fp64_rule(point, refine):
    seq, p = gpu_run("imm", point, refine), ob.imm_params(point)
    the_decode_is_pose_decode(seq, "plain", point, refine)
    mom = ob.moments(maps_of("plain"), stacked(seq, "idx"))
    o64 = ob.imm_run(point, stacked(seq, "raw"), stacked(seq, "maxval"), mom)
    margin = gate_margin(o64["d2"], p.gate)
    status, moving = stacked(seq, "status"), stacked(seq, "moving")
    print("%s: statuses %s; the nearest decisive d2 %.1f %% of the gate away; moving %.3f to %.3f on the live rows"
          % (point, np.bincount(status.ravel(), minlength=5).tolist(), 100 * margin, moving[status != ref.LOST].min(), moving.max()))
    assert margin > 0.01 and set(np.unique(o64["status"])) == ALL_CODES
    assert np.array_equal(status, o64["status"])
    last = seq[-1]["state"].cpu().numpy()
    shown("pose_track imm", point, refine, filter_figures(seq, o64, "imm", point, p)
          + [("moving", np.abs(moving - o64["moving"]).max(), ob.bound("imm", point, "moving")),
             ("state mu", np.abs(last[:, 28:30] - o64["state"][:, 28:30]).max(), ob.bound("imm", point, "moving")),
             ("state xy px", np.abs(last[:, [0, 1, 14, 15]] - o64["state"][:, [0, 1, 14, 15]]).max(), ob.bound("imm", point, "pos")),
             ("state v px/s", np.abs(last[:, [2, 3, 16, 17]] - o64["state"][:, [2, 3, 16, 17]]).max(), ob.bound("imm", point, "vel"))])
    assert np.array_equal(o64["state"][:, 30:], last[:, 30:])
    assert np.array_equal(moving, np.stack([o["state"][:, 29].cpu().numpy() for o in seq]))
    assert moving.max() - moving[status != ref.LOST].min() > 0.2                 # the probabilities move


@REFINE
@POINT
def test_without_switching_and_prior_the_two_model_tracker_is_the_tracker_bit_for_bit(point, refine):
    plain, off = gpu_run("plain", point, refine), gpu_run("imm off", point, refine)
    same_bits(plain, off, OUT, "imm without switching")
    for t in range(ob.T):
        s1, s2 = plain[t]["state"], off[t]["state"]
        assert torch.equal(s1[:, :14], s2[:, :14]) and torch.equal(s1[:, 14:], s2[:, 30:]), t
        assert not off[t]["moving"].any().item() and not s2[:, 29].any().item(), t
    assert off[-1]["state"][:, 14:28].any().item()                               # model 1 did run


# ---- pose_track_nll ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nll_launch(point, refine, run=0):
    from hupr_amd import functional as F_
    start = torch.zeros(ob.T, dtype=torch.int32, device="cuda")
    start[0] = 1
    return F_.pose_track_nll(measured(point, refine)[3], start, tracking(point), ob.nll_grid(point), ob.EXTENT[point], ob.RATIO[point])


@REFINE
@POINT
def test_the_likelihood_of_the_runs_record_follows_the_fp64_rule(point, refine):
    seq = gpu_run("plain", point, refine)
    idx, mx, raw, meas = measured(point, refine)
    for t in range(ob.T):                                                       # the record is the run's own measurements
        assert torch.equal(raw[t], seq[t]["raw"]) and torch.equal(mx[t], seq[t]["maxval"])
    nll, counts, final = nll_launch(point, refine)
    assert nll.shape == (27, ob.ROWS) and counts.shape == (27, ob.ROWS, 6) and final.shape == (27, ob.ROWS, 16)
    # the candidate with the tracker's parameters ends in the tracker's state, bit for bit, and counts its statuses
    assert torch.equal(final[ob.NLL_OWN], seq[-1]["state"])
    status = torch.stack([o["status"] for o in seq])
    assert torch.equal(counts[ob.NLL_OWN, :, :5], torch.stack([(status == c).sum(0) for c in range(5)], dim=1).to(torch.int32))
    assert not torch.equal(final[ob.NLL_OWN - 1], seq[-1]["state"]) and not torch.equal(final[ob.NLL_OWN + 9], seq[-1]["state"])
    # all 27 against the fp64 rule on the same fp32 record
    o64 = ob.nll_run(point, meas.cpu().numpy())
    print("%s: the nearest gate decision of %d cells %.1f %% of the gate away" % (point, o64["near"].size, 100 * o64["near"].min()))
    assert o64["near"].min() > 0.01 and (ob.nll_grid(point)[:, 2] > 0).all()
    assert np.array_equal(counts.cpu().numpy(), o64["counts"])                  # the five statuses and the frames scored, every cell
    final = final.cpu().numpy()
    assert np.array_equal(final[..., 14:], o64["state"][..., 14:])
    shown("pose_track_nll", point, refine,
          [("nll rel", ob.nll_rel_diff(nll.cpu().numpy(), o64), ob.bound("nll", point, "nll")),
           ("final xy px", np.abs(final[..., 0:2] - o64["state"][..., 0:2]).max(), ob.bound("track", point, "pos")),
           ("final v px/s", np.abs(final[..., 2:4] - o64["state"][..., 2:4]).max(), ob.bound("track", point, "vel")),
           ("final P rel", ob.state_cov_diff(final, o64["state"]), ob.bound("track", point, "state"))])
    assert nll.cpu().numpy().sum(1).argmin() == o64["nll"].sum(1).argmin()


# ---- the smoothers -----------------------------------------------------------------------------------------------------------------------
HIST = ("state", "status", "kp", "raw", "maxval")
TAIL = ("kp", "vel", "cov", "flag")


def history(point, refine):
    """The recorded fp32 run of the tracker -> dict of (T, ROWS, ...) device tensors."""
    seq = gpu_run("plain", point, refine)
    return {k: torch.stack([o[k] for o in seq]) for k in HIST}


def rts(h, point, lo=0, hi=ob.T - 1):
    from hupr_amd import functional as F_
    return dict(zip(TAIL, F_.pose_smooth_rts(h["state"][lo:hi + 1], h["status"][lo:hi + 1], h["kp"][lo:hi + 1], tracking(point))))


def smoother_figures(o, o64, rule, point):
    return [("keypoints px", np.abs(o["kp"] - o64["kp"]).max(), ob.bound(rule, point, "pos")),
            ("velocity px/s", np.abs(o["vel"] - o64["vel"]).max(), ob.bound(rule, point, "vel")),
            ("covariance rel", ref.cov_rel_diff(o["cov"], o64["cov"]), ob.bound(rule, point, "cov"))]


@REFINE
@POINT
def test_the_backward_pass_over_the_recorded_states_follows_the_fp64_rule(point, refine):
    h = history(point, refine)
    o = {k: v.cpu().numpy() for k, v in rts(h, point).items()}
    o64 = ob.smooth_run(point, h["state"].cpu().numpy(), h["status"].cpu().numpy(), h["kp"].cpu().numpy())
    print("%s: flags %s" % (point, np.bincount(o["flag"].ravel(), minlength=4).tolist()))
    assert np.array_equal(o["flag"], o64["flag"]) and set(np.unique(o["flag"])) == {sr.SMOOTHED, sr.END, sr.PASSTHROUGH}
    shown("pose_smooth_rts", point, refine, smoother_figures(o, o64, "smooth", point))
    assert np.abs(o["kp"] - h["kp"].cpu().numpy()).max() > 0.3                   # the smoother moves the keypoints
    assert np.abs(o["cov"][..., 1]).max() > 0.5                                  # and its covariance is oblique


LAG_TAIL = TAIL + ("filtered", "raw", "status", "scores")


@functools.lru_cache(maxsize=None)
def lag_tails(point, refine, L, run=0):
    """The lag launch after every frame of the recorded run, from a fresh ring -> [per frame: dict of the launch's eight tails]."""
    from hupr_amd import functional as F_
    h, p = history(point, refine), tracking(point)
    lag_state = F_.pose_lag_state(ob.ROWS, L, "cuda")
    return [dict(zip(LAG_TAIL, F_.pose_smooth_lag(*[h[k][n] for k in HIST], lag_state, p, L))) for n in range(ob.T)]


@pytest.mark.parametrize("L", ob.LAGS)
@REFINE
@POINT
def test_the_fixed_lag_smoother_follows_the_fp64_rule_and_the_fixed_interval_kernel(point, refine, L):
    h, tails = history(point, refine), lag_tails(point, refine, L)
    # every window of the ring is the fixed-interval kernel's output over the same frames, bit for bit
    for n in range(ob.T):
        lo = max(n - L, 0)
        want = rts(h, point, lo, n)
        for k in TAIL:
            assert torch.equal(tails[n][k][:n - lo + 1], want[k].flip(0)), (n, k)
    a = {k: np.stack([(tails[f + L][k][L] if f + L < ob.T else tails[-1][k][ob.T - 1 - f]).cpu().numpy() for f in range(ob.T)]) for k in TAIL}
    a64, _ = ob.lag_run(point, h["state"].cpu().numpy(), h["status"].cpu().numpy(), h["kp"].cpu().numpy(), L)
    assert np.array_equal(a["flag"], a64["flag"])
    shown("pose_smooth_lag %d" % L, point, refine, smoother_figures(a, a64, "lag%d" % L, point))


# ---- run to run --------------------------------------------------------------------------------------------------------------------------
@POINT
def test_two_runs_of_everything_are_identical(point):
    for refine in (False, True):
        for kind in KINDS:
            a, b = gpu_run(kind, point, refine, 0), gpu_run(kind, point, refine, 1)
            assert a is not b
            same_bits(a, b, tuple(a[0]), kind)
        for x, y in zip(nll_launch(point, refine, 0), nll_launch(point, refine, 1)):
            assert torch.equal(x, y)
        h = history(point, refine)
        one, two = rts(h, point), rts(h, point)
        for k in TAIL:
            assert torch.equal(one[k], two[k]), k
        for x, y in zip(measured(point, refine, 0), measured(point, refine, 1)):
            assert x is not y and torch.equal(x.nan_to_num(-1.0), y.nan_to_num(-1.0))
        for L in ob.LAGS:
            a, b = lag_tails(point, refine, L, 0), lag_tails(point, refine, L, 1)
            assert a is not b
            same_bits(a, b, LAG_TAIL, "lag %d" % L)
