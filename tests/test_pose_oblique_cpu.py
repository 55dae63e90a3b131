"""CPU (-m "not gpu"): the oblique scenario of tests/pose_oblique_ref.py and the fp64 restatements of the pose-tracker family on it.  No
launch, no package.

1. The conditions on the inputs that tests/test_pose_oblique_gpu.py relies on, asserted on the fp64 rules alone, at both parameter
   points and with both decodes: every status occurs; no gate decision of the tracker, of the two-model tracker, of any of the 27
   likelihood candidates, of the ghost and of the pair variant lies within 1 % of the gate; the ghost variant has no two gated costs
   within 1e-3 and no local maximum within 1e-4 of the floor; the pair variant has no two assignments of equal cardinality within 1e-3
   in cost.  The coupling is material: the median |Sxy| / sqrt(Sxx Syy) is >= 0.3, the median |Pxy| / sqrt(Pxx Pyy) >= 0.2, and the
   border rows' arg-max stays within 3 pixels of their edge.  And it shows: the rules with Sxy forced to 0, and the smoothers fed
   states without P01, P03, P12, P23, differ from the true ones by at least 100 x the GPU tests' bounds.
2. The restatements' own cross terms.  The model is isotropic (one accel_psd and one init_speed_std for both axes), so every rule is
   rotation-equivariant at the measurement level: raw keypoints rotated by Q and moments by Q S Q^T give Q-rotated keypoints and
   velocities and Q P Q^T, with equal statuses, flags and ``moving``, and equal likelihood sums and counts — to 1e-10 in fp64.  A
   kernel and a restatement that shared a misreading of a cross term would both fail this.  ref_smooth is also held against the dense
   textbook smoother on an uninterrupted oblique row.
3. The fp32 figures pose_oblique_ref.FP32 records, measured again and held."""
import functools

import numpy as np
import pytest

import pose_assoc_ref as A
import pose_nll_ref as nr
import pose_oblique_ref as ob
import pose_smooth_ref as sr
import pose_track_ref as ref

POINT = pytest.mark.parametrize("point", ob.POINTS)
REFINE = pytest.mark.parametrize("refine", [False, True], ids=["argmax", "subpixel"])
ALL_CODES = {ref.UPDATED, ref.COASTED_MISSING, ref.COASTED_GATED, ref.STARTED, ref.LOST}


def gate_margin(d2, gate):
    """-> (the smallest |d2 / gate - 1| over the gate decisions, their number)."""
    d = d2[np.isfinite(d2)]
    return float(np.abs(d / gate - 1.0).min()), d.size


@functools.lru_cache(maxsize=None)
def runs(point, refine=True, dtype=np.float64):
    """Every measurement-level rule over the scenario at ``point`` in ``dtype`` (fp32: window moments included, the smoothers behind
    the fp32 tracker run) -> dict: track, states, imm, smooth, lag (by L), nll."""
    idx, mx, raw, mom = ob.inputs(point, refine)
    if dtype is np.float32:
        mom = ob.moments32()
    track, states = ob.track_run(point, raw, mx, mom, dtype)
    meas = nr.record_of(raw, mx, ob.inputs(point, refine)[3])                   # one fp32 record for both float types, as on the GPU
    return dict(track=track, states=states, imm=ob.imm_run(point, raw, mx, mom, dtype),
                smooth=ob.smooth_run(point, states, track["status"], track["kp"], dtype),
                lag={L: ob.lag_run(point, states, track["status"], track["kp"], L, dtype)[0] for L in ob.LAGS},
                nll=ob.nll_run(point, meas, dtype))


# ---- 1: the conditions on the inputs -----------------------------------------------------------------------------------------------------
@REFINE
@POINT
def test_every_status_occurs_and_no_decision_is_near_the_gate(point, refine):
    o, p = runs(point, refine), ob.params(point)
    for name in ("track", "imm"):
        status = o[name]["status"]
        margin, n = gate_margin(o[name]["d2"], p.gate)
        print("%s %s: statuses %s, %d gate decisions, the nearest %.1f %% of the gate away"
              % (point, name, np.bincount(status.ravel(), minlength=5).tolist(), n, 100 * margin))
        assert set(np.unique(status)) == ALL_CODES
        assert n > 200 and margin > 0.01
    assert np.array_equal(o["track"]["status"], o["imm"]["status"])
    status = o["track"]["status"]
    # the events are what they are meant to be
    assert (status[list(ob.DROP_FRAMES)[:2], ob.DROP] == ref.COASTED_MISSING).all()
    assert status[ob.OUTLIER_FRAME, ob.OUTLIER] == ref.COASTED_GATED
    g0, g1 = ob.GONE_FRAMES[0], ob.GONE_FRAMES[-1]
    assert len(ob.GONE_FRAMES) > p.max_coast
    assert status[g0:g1 + 2, ob.GONE].tolist() == ([ref.COASTED_MISSING] * p.max_coast + [ref.LOST] * (len(ob.GONE_FRAMES) - p.max_coast)
                                                   + [ref.STARTED])
    # the 27 likelihood candidates: no cell has a decision within 1 % of the gate, and every status occurs under the point's own
    nll = o["nll"]
    print("%s likelihood: the nearest decision of %d cells %.1f %% of the gate away; the own candidate's counts %s"
          % (point, nll["near"].size, 100 * nll["near"].min(), nll["counts"][ob.NLL_OWN].sum(0).tolist()))
    assert nll["near"].min() > 0.01
    assert np.array_equal(nll["status"][:, ob.NLL_OWN], status) and (ob.nll_grid(point)[:, 2] > 0).all()
    assert tuple(ob.nll_grid(point)[ob.NLL_OWN]) == tuple(float(np.float32(v)) for v in (p.accel_psd, p.meas_std, p.heatmap_gain))
    assert (nll["counts"][..., 5] > 0).all() and (nll["counts"][..., :5].sum(0).sum(0) > 0).all()


@REFINE
@POINT
def test_the_coupling_is_material_and_the_border_rows_stay_at_their_edge(point, refine):
    idx, mx, raw, mom = ob.inputs(point, refine)
    o = runs(point, refine)["track"]
    use = o["usable"]
    rho_s = np.abs(mom[..., 2][use]) / np.sqrt(mom[..., 1][use] * mom[..., 3][use])
    cov = o["cov"][o["status"] == ref.UPDATED]
    rho_p = np.abs(cov[:, 1]) / np.sqrt(cov[:, 0] * cov[:, 2])
    edge = ob.edge_distance(idx)
    print("%s: median |Sxy| / sqrt(Sxx Syy) %.2f over %d measurements, median |Pxy| / sqrt(Pxx Pyy) %.2f over %d updates; border rows at "
          "most %d pixels from an edge, interior rows at least %d" % (point, np.median(rho_s), rho_s.size, np.median(rho_p), rho_p.size,
                                                                       edge[:, list(ob.BORDER)].max(), edge[:, list(ob.INTERIOR)].min()))
    assert use.sum() > 250 and np.median(rho_s) >= 0.3
    assert np.median(rho_p) >= 0.2
    assert (edge[:, list(ob.BORDER)] < ref.RADIUS).all()                         # the window is clipped in every frame
    px, py = idx % ob.W, idx // ob.W
    assert (px[:, ob.LEFT] < 3).all() and (px[:, ob.RIGHT] > ob.W - 4).all() and (py[:, ob.TOP] < 3).all()
    assert (px[:, ob.CORNER] > ob.W - 4).all() and (py[:, ob.CORNER] > ob.H - 4).all()
    assert (mx[:, list(ob.BORDER)] > ob.MIN_SCORE).all()
    # the cross entries of the state are no rounding either
    states = runs(point, refine)["states"]
    live = states[..., 14] == 1
    _, P = sr.unpack(states[live], np.float64)
    d = np.sqrt(np.diagonal(P, axis1=-2, axis2=-1))
    rho = np.abs(P) / (d[:, :, None] * d[:, None, :])
    print("%s: median correlation of the live states: P01 %.2f, P03 %.2f, P12 %.2f, P23 %.2f"
          % (point, np.median(rho[:, 0, 1]), np.median(rho[:, 0, 3]), np.median(rho[:, 1, 2]), np.median(rho[:, 2, 3])))
    assert min(np.median(rho[:, i, j]) for i, j in ((0, 1), (0, 3), (1, 2), (2, 3))) > 0.05


@REFINE
@POINT
def test_the_ghost_variant_decides_nothing_on_a_rounding(point, refine):
    maps, _ = ob.ghost_scenario()
    p = ob.params(point, candidates=2)
    o, c = ob.ghost_run(point, refine)
    margin, n = gate_margin(o["d2"], p.gate)
    cost = np.sort(np.where(np.isfinite(o["cost"]), o["cost"], np.inf), axis=-1)
    both = np.isfinite(cost[..., 1])
    gap = (cost[both][:, 1] - cost[both][:, 0]).min()
    flat = maps.reshape(ob.T, ob.ROWS, -1)
    floor = np.float32(p.peak_ratio) * flat.max(axis=-1)
    tops = np.stack([[A.local_maxima(m) for m in frame] for frame in maps]).reshape(flat.shape)
    rel = np.abs(flat / floor[..., None] - 1.0)[tops].min()
    chosen = o["chosen"][list(ob.GHOST_FRAMES)][:, list(ob.GHOST_ROWS)]
    print("%s ghost: %d gate decisions, the nearest %.1f %% of the gate away; %d frames x rows with two gated candidates, the closest "
          "costs %.3f apart; the local maximum nearest to the floor %.3f of it away; chosen in the ghost frames %s"
          % (point, n, 100 * margin, int(both.sum()), gap, rel, np.bincount(chosen.ravel() + 1, minlength=3).tolist()))
    assert n > 300 and margin > 0.01
    assert both.sum() >= 10 and gap > 1e-3
    assert rel > 1e-4
    assert (c["count"][list(ob.GHOST_FRAMES)][:, list(ob.GHOST_ROWS)] == 2).sum() >= 100 and (chosen == 1).sum() >= 100


@REFINE
@POINT
def test_the_pair_variant_decides_nothing_on_a_rounding(point, refine):
    p = ob.params(point, pair_swap=True, pairs=ob.PARTNER)
    o, _ = ob.pair_run(point, refine)
    margin, n = gate_margin(o["d2"], p.gate)
    alt = o["alt"][np.isfinite(o["alt"])]
    swapped = [r for pair in ob.PAIRS for r in pair]
    source = o["source"][list(ob.SWAP_FRAMES)][:, swapped]
    print("%s pairs: %d gate decisions, the nearest %.1f %% of the gate away; %d units with a second assignment of equal cardinality, the "
          "closest %.3f apart; source in the swapped frames %s" % (point, n, 100 * margin, alt.size, alt.min(),
                                                                   np.bincount(source.ravel() + 1, minlength=3).tolist()))
    assert n > 300 and margin > 0.01
    assert alt.size >= 10 and alt.min() > 1e-3
    assert (source == 1).sum() >= 40                                            # the swap is followed


@POINT
def test_forcing_the_cross_terms_to_zero_shows(point):
    """Sxy = 0 in the tracker and the two-model tracker, and P01 = P03 = P12 = P23 = 0 in the states the smoothers read, against the
    true rules: the keypoints, the covariance and ``moving`` differ by at least 100 x the bounds of tests/test_pose_oblique_gpu.py.  The fixed-lag
    smoother is held to this in its covariance only: see below."""
    idx, mx, raw, mom = ob.inputs(point)
    o = runs(point)
    flat = ob.without_sxy(mom)
    t0, _ = ob.track_run(point, raw, mx, flat)
    i0 = ob.imm_run(point, raw, mx, flat)
    bare = ob.without_cross(o["states"])
    s0 = ob.smooth_run(point, bare, o["track"]["status"], o["track"]["kp"])
    shown = {"track": (t0, o["track"]), "imm": (i0, o["imm"]), "smooth": (s0, o["smooth"])}
    for L in ob.LAGS:
        shown["lag%d" % L] = (ob.lag_run(point, bare, o["track"]["status"], o["track"]["kp"], L)[0], o["lag"][L])
    for rule, (zeroed, true) in shown.items():
        d_cov = ref.cov_rel_diff(zeroed["cov"], true["cov"])
        print("%s %s without its cross terms: covariance %.3f relative (%.0f x the bound)" % (point, rule, d_cov, d_cov / ob.bound(rule, point, "cov")))
        assert d_cov >= 100 * ob.bound(rule, point, "cov"), rule
        if rule.startswith("lag"):
            # The lagged keypoints are no check of the cross terms and are not used as one: one to four backward steps move a keypoint
            # by a fraction of an innovation, and at point B, L = 1 the cross terms move it by 3 x the bound only, whatever the seed.
            # For the lag kernel they are carried by its covariance (here) and by the bit equality of every window of its ring with the
            # fixed-interval kernel (tests/test_pose_oblique_gpu.py), whose keypoints are held below.
            continue
        d_kp = np.abs(zeroed["kp"] - true["kp"]).max()
        print("%s %s without its cross terms: keypoints %.3f px (%.0f x the bound)" % (point, rule, d_kp, d_kp / ob.bound(rule, point, "pos")))
        assert d_kp >= 100 * ob.bound(rule, point, "pos"), rule
    d_mv = np.abs(i0["moving"] - o["imm"]["moving"]).max()
    print("%s imm without Sxy: moving %.3f (%.0f x the bound)" % (point, d_mv, d_mv / ob.bound("imm", point, "moving")))
    assert d_mv >= 100 * ob.bound("imm", point, "moving")


# ---- 2: the restatements' own cross terms ------------------------------------------------------------------------------------------------
THETA = 0.7
TOL_ROT = 1e-10


def close(a, b, what):
    err = np.abs(np.asarray(a) - np.asarray(b)).max()
    assert err <= TOL_ROT, (what, err)
    return err


@POINT
def test_the_tracker_restatements_are_rotation_equivariant(point):
    Q = ob.rotation(THETA)
    idx, mx, raw, mom = ob.inputs(point)
    o = runs(point)
    raw_q, mom_q = raw @ Q.T, ob.rotate_moments(mom, Q)
    assert np.abs(mom_q[..., 2] - mom[..., 2]).max() > 0.5                      # the rotation does mix the moments
    t_q, states_q = ob.track_run(point, raw_q, mx, mom_q)
    i_q = ob.imm_run(point, raw_q, mx, mom_q)
    worst = 0.0
    for name, got, want in (("ref_track", t_q, o["track"]), ("ref_imm", i_q, o["imm"])):
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["usable"], want["usable"]), name
        for k in ("kp", "vel", "fc"):
            worst = max(worst, close(got[k], want[k] @ Q.T, (name, k)))
        worst = max(worst, close(got["cov"], ob.rotate_cov(want["cov"], Q), (name, "cov")))
        both = np.isfinite(want["d2"])
        assert np.array_equal(np.isfinite(got["d2"]), both)
        worst = max(worst, close(got["d2"][both], want["d2"][both], (name, "d2")))
        floats = want["state"].shape[-1]
        worst = max(worst, close(got["state"], ob.rotate_states(want["state"], Q, floats), (name, "state")))
    worst = max(worst, close(i_q["moving"], o["imm"]["moving"], "moving"))
    worst = max(worst, close(states_q, ob.rotate_states(o["states"], Q), "states"))
    print("%s: ref_track and ref_imm under a rotation by %.1f rad: largest deviation from equivariance %.2e" % (point, THETA, worst))


@POINT
def test_the_smoother_restatements_are_rotation_equivariant(point):
    Q = ob.rotation(THETA)
    o = runs(point)
    states_q, kp_q, status = ob.rotate_states(o["states"], Q), o["track"]["kp"] @ Q.T, o["track"]["status"]
    got = {"ref_smooth": ob.smooth_run(point, states_q, status, kp_q)}
    want = {"ref_smooth": o["smooth"]}
    for L in ob.LAGS:
        got["ref_lag %d" % L], want["ref_lag %d" % L] = ob.lag_run(point, states_q, status, kp_q, L)[0], o["lag"][L]
    worst = 0.0
    for name in got:
        assert np.array_equal(got[name]["flag"], want[name]["flag"]), name
        assert set(np.unique(want[name]["flag"])) == {sr.SMOOTHED, sr.END, sr.PASSTHROUGH}
        for k in ("kp", "vel"):
            worst = max(worst, close(got[name][k], want[name][k] @ Q.T, (name, k)))
        worst = max(worst, close(got[name]["cov"], ob.rotate_cov(want[name]["cov"], Q), (name, "cov")))
    B = np.zeros((4, 4))
    B[:2, :2] = B[2:, 2:] = Q
    worst = max(worst, close(got["ref_smooth"]["P"], B @ o["smooth"]["P"] @ B.T, "the full smoothed covariance"))
    print("%s: ref_smooth and ref_lag under a rotation by %.1f rad: largest deviation from equivariance %.2e" % (point, THETA, worst))


@POINT
def test_the_likelihood_restatement_is_rotation_invariant(point):
    Q = ob.rotation(THETA)
    idx, mx, raw, mom = ob.inputs(point)
    record = lambda z, m: np.concatenate([z, mx[..., None].astype(np.float64), m, np.zeros(mx.shape + (1,))], axis=-1)   # fp64: no rounding
    a, b = ob.nll_run(point, record(raw, mom)), ob.nll_run(point, record(raw @ Q.T, ob.rotate_moments(mom, Q)))
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["status"], b["status"])
    err = (np.abs(a["nll"] - b["nll"]) / np.maximum(np.abs(a["nll"]), 1.0)).max()
    print("%s: ref_nll under a rotation by %.1f rad: sums differ by %.2e relative, %d cells" % (point, THETA, err, a["nll"].size))
    assert err <= TOL_ROT
    close(b["state"], ob.rotate_states(a["state"], Q), "final states")
    # and frame for frame it is ref_track at the point's own candidate
    own, p = runs(point)["track"], ob.params(point)
    start = np.arange(ob.T) == 0
    exact = nr.ref_nll(record(raw, mom), start, p, [[p.accel_psd, p.meas_std, p.heatmap_gain]], ob.RATIO[point], ob.EXTENT[point])
    assert np.array_equal(exact["status"][:, 0], own["status"])
    close(exact["kp"][:, 0], own["kp"], "ref_nll against ref_track")
    close(exact["state"][0], own["state"], "ref_nll's final state against ref_track's")


@POINT
def test_ref_smooth_is_the_textbook_smoother_on_an_oblique_row(point):
    o = runs(point)
    p = ob.params(point)
    quiet = [r for r in range(ob.ROWS) if r not in ob.EVENT_ROWS]
    status = o["track"]["status"]
    assert (status[0, quiet] == ref.STARTED).all() and (status[1:, quiet] == ref.UPDATED).all()      # uninterrupted, border rows included
    F, Q = sr.model(p.rate_hz, p.accel_psd, np.float64)
    worst = 0.0
    for r in quiet:
        x, P = sr.unpack(o["states"][:, r], np.float64)
        assert np.abs(P[:, 0, 1]).max() > 0.5 and np.abs(P[:, 0, 3]).max() > 0.05
        xs, Ps = sr.textbook_rts(x, P, F, Q)
        worst = max(worst, np.abs(xs - o["smooth"]["x"][:, r]).max(), np.abs(Ps - o["smooth"]["P"][:, r]).max())
    print("%s: ref_smooth against the dense textbook smoother on %d uninterrupted rows: %.2e" % (point, len(quiet), worst))
    assert worst <= 1e-8                                                        # np.linalg.inv of a 4 x 4 with condition ~1e4


# ---- 3: the fp32 figures --------------------------------------------------------------------------------------------------------------------
def fp32_figures(point):
    """The figures of pose_oblique_ref.FP32 at ``point``: the larger of the two decodes'."""
    out = {}

    def put(rule, what, v):
        out.setdefault(rule, {})
        out[rule][what] = max(out[rule].get(what, 0.0), float(v))

    for refine in (False, True):
        o64, o32 = runs(point, refine), runs(point, refine, np.float32)
        pairs = [("track", o32["track"], o64["track"]), ("imm", o32["imm"], o64["imm"]), ("smooth", o32["smooth"], o64["smooth"])]
        pairs += [("lag%d" % L, o32["lag"][L], o64["lag"][L]) for L in ob.LAGS]
        for rule, a, b in pairs:
            assert np.array_equal(a["status" if "status" in a else "flag"], b["status" if "status" in b else "flag"]), rule
            put(rule, "pos", np.abs(a["kp"] - b["kp"]).max())
            put(rule, "vel", np.abs(a["vel"] - b["vel"]).max())
            put(rule, "cov", ref.cov_rel_diff(a["cov"], b["cov"]))
        put("track", "state", ob.state_cov_diff(o32["states"], o64["states"]))
        put("imm", "moving", np.abs(o32["imm"]["moving"] - o64["imm"]["moving"]).max())
        assert np.array_equal(o32["nll"]["counts"], o64["nll"]["counts"])
        put("nll", "nll", ob.nll_rel_diff(o32["nll"]["nll"], o64["nll"]))
    return out


@POINT
def test_the_fp32_restatements_agree_with_the_fp64_ones(point):
    """Where the bounds of tests/test_pose_oblique_gpu.py come from: every restatement run in NumPy fp32 (window moments included)
    against its fp64 run.  Prints the figures and holds the recorded ones: none is exceeded, none is more than twice what is measured."""
    got = fp32_figures(point)
    for rule, figures in got.items():
        want = ob.FP32[rule, point]
        print("%s %-6s measured %s | recorded %s" % (point, rule, ", ".join("%s %.3e" % kv for kv in sorted(figures.items())),
                                                    ", ".join("%s %.3e" % kv for kv in sorted(want.items()))))
    for rule, figures in got.items():
        want = ob.FP32[rule, point]
        assert set(figures) == set(want), rule
        for what, v in figures.items():
            assert want[what] / 2 <= v <= want[what] * 1.01, (rule, what, v, want[what])
    assert set(r for r, _ in ob.FP32) == set(got)
