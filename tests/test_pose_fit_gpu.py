"""GPU (-m gpu): hupr_pose_measure_f32 and hupr_pose_track_nll_f32 (csrc/pose_fit.hip) — the tracker's measurement without a filter, and
the likelihood of a whole recording under many parameter candidates in one launch — against functional.pose_decode and
functional.pose_track bit for bit and against the NumPy statement of the rule in tests/pose_nll_ref.py; then tools.calibrate.fit_tracking,
the live session, the offline SequenceSmoother and Runner.eval.

Bounds.  Decode: bit equality with functional.pose_decode.  Window moments: the tracker test's TOL_MOMENT = 1e-4 heat-map pixel^2
(tests/test_pose_track_gpu.py derives it).  A candidate that equals a pose_track run's parameters: the final state is that run's,
torch.equal — both kernels compile the device functions of csrc/pose_track_model.h.  Against fp64: a (candidate, row) cell is left
out where the fp64 run has a gate decision within 1e-3 of the gate, relative (an fp32 run may decide it the other way, and then differs
by a frame's whole cost); at most 2 % of the cells may be left out (the fp64 reference alone: 0.8 to 1.4 % on the 28-row records,
tests/test_pose_fit_cpu.py asserts it).  On the others the counts are equal and |nll - nll64| / scored <= 16 x NLL_REL_FP32 = 3.5e-4,
NLL_REL_FP32 = 2.17e-5 being what the NumPy fp32 run of the restatement shows against its fp64 run (measured in
tests/test_pose_fit_cpu.py) — the project's rule for an fp32 kernel, which contracts to FMAs and uses the device's logf."""
import functools
import re

import numpy as np
import pytest
import torch

import pose_nll_ref as nr
import pose_track_ref as ref
from test_pose_fit_cpu import NEAR_GATE, NLL_REL_FP32

pytestmark = pytest.mark.gpu
TOL_NLL_REL = 16 * NLL_REL_FP32
EXTENT = (256.0, 256.0)


def tracking(rate=ref.RATE, **kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(rate, **kw)


def launches():
    from hupr_amd import runtime as rt
    return rt.lib().hupr_launch_count()


# ---- 1: the measurement -----------------------------------------------------------------------------------------------------------------------
def measure_maps(which):
    from test_pose_track_gpu import covariance_maps
    if which == "6x8x12":
        return covariance_maps(8, 12)[0]
    maps = np.random.RandomState(3).uniform(-0.2, 1.0, (28, 64, 64)).astype(np.float32)
    maps[5].reshape(-1)[[77, 1300, 4000]] = 2.0                # tied maxima: the first wins
    maps[9] = -np.abs(maps[9])                                 # all <= 0: no measurement
    maps[10] = 0.0
    return maps


@pytest.mark.parametrize("refine", [False, True], ids=["argmax", "subpixel"])
@pytest.mark.parametrize("which", ["28x64x64", "6x8x12"])
def test_pose_measure_is_the_decode_and_the_window_moments(which, refine):
    from hupr_amd import functional as F_
    from test_pose_track_gpu import TOL_MOMENT
    maps, ratio = measure_maps(which), 4.0
    heat = torch.from_numpy(maps).cuda()
    idx, mx, raw, _, _ = F_.pose_decode(heat, ratio, refine=refine)
    n0 = launches()
    midx, mmx, mraw, meas = F_.pose_measure(heat, ratio, refine=refine)
    assert launches() - n0 == 1
    assert midx.dtype == torch.int32 and meas.shape == (maps.shape[0], 8) and meas.dtype == torch.float32
    assert torch.equal(midx, idx) and torch.equal(mmx, mx) and torch.equal(mraw, raw)
    assert torch.equal(meas[:, 0:2], raw) and torch.equal(meas[:, 2], mx) and not meas[:, 7].any().item()
    want = ref.window_moments(maps, idx.cpu().numpy())
    got = meas[:, 3:7].cpu().numpy().astype(np.float64)
    positive = mx.cpu().numpy() > 0
    assert positive.sum() >= maps.shape[0] - 2
    err = np.abs(got[positive, 1:] - want[positive, 1:]).max()
    mass = np.abs(got[positive, 0] / want[positive, 0] - 1.0).max()
    print("%s refine %d: max |moment - fp64| %.3e heat-map pixel^2 (bound %.0e), mass relative %.3e" % (which, refine, err, TOL_MOMENT, mass))
    assert err <= TOL_MOMENT and mass <= 1e-5
    assert (got[~positive, 0] == 0).all() and (want[~positive, 0] == 0).all()
    if which == "28x64x64":
        assert not positive[9] and not positive[10] and idx[5].item() == 77
    # into the caller's own tensors
    out = tuple(torch.empty_like(t) for t in (midx, mmx, mraw, meas))
    back = F_.pose_measure(heat, ratio, refine=refine, out=out)
    assert all(a is b for a, b in zip(back, out)) and torch.equal(out[3].nan_to_num(-1.0), meas.nan_to_num(-1.0))


# ---- 2: the bit anchor ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scenario_walk():
    """The scenario through functional.pose_track (accel_psd 100, min_score 0.1) and through functional.pose_measure -> (the state after
    the last frame, status (T, ROWS), meas (T, ROWS, 8), the tracking)."""
    from hupr_amd import functional as F_
    heat = torch.from_numpy(np.array(ref.scenario()[0])).cuda()
    p = tracking(accel_psd=100.0, min_score=ref.MIN_SCORE)
    state = F_.pose_track_state(ref.ROWS, "cuda")
    status, meas = [], []
    for t in range(ref.T):
        o = F_.pose_track(heat[t], ref.RATIO, track_state=state, tracking=p)
        m = F_.pose_measure(heat[t], ref.RATIO)
        assert torch.equal(m[2], o[2]) and torch.equal(m[1], o[1])
        status.append(o[7].clone())
        meas.append(m[3])
    return state.clone(), torch.stack(status), torch.stack(meas), p


def zeros_start(T, *ones):
    s = torch.zeros(T, dtype=torch.int32, device="cuda")
    for k in ones:
        s[k] = 1
    return s


def test_a_candidate_with_the_trackers_parameters_ends_in_the_trackers_state():
    from hupr_amd import functional as F_
    live, status, meas, p = scenario_walk()
    G = 65                                                                              # a second block of candidates, one lane of it used
    params = np.stack([100.0 * 1.05 ** (np.arange(G) - 30.5), np.full(G, 1.5), np.full(G, 0.5)], axis=1)
    params[1] = params[64] = (p.accel_psd, p.meas_std, p.heatmap_gain)
    n0 = launches()
    nll, counts, final = F_.pose_track_nll(meas, zeros_start(ref.T, 0), p, params, EXTENT, ref.RATIO)
    assert launches() - n0 == 1
    assert nll.shape == (G, ref.ROWS) and nll.dtype == torch.float64 and counts.shape == (G, ref.ROWS, 6) and final.shape == (G, ref.ROWS, 16)
    assert live.any().item() and torch.equal(final[1], live) and torch.equal(final[64], live)
    hist = torch.stack([(status == c).sum(0) for c in range(5)], dim=1).to(torch.int32)
    assert torch.equal(counts[1, :, :5], hist) and torch.equal(counts[64, :, :5], hist)
    assert torch.equal(nll[1], nll[64]) and torch.equal(counts[1], counts[64])
    assert (counts[..., :5].sum(-1) == ref.T).all().item()
    assert not torch.equal(final[0], live) and not torch.equal(final[63], live) and not torch.equal(nll[0], nll[1])
    assert (hist > 0).any(0).all().item()                                                # every status occurs
    # the frames scored are the fp64 rule's on the same record (no decision of the scenario is near the gate, tests/test_pose_track_gpu.py);
    # the cost is printed beside it — the bound of the fp64 test below belongs to the model-drawn record it was measured on
    o64 = nr.ref_nll(meas.cpu().numpy(), [1] + [0] * (ref.T - 1), p, params[[1]], ref.RATIO, EXTENT)
    assert np.array_equal(o64["counts"][0], counts[1].cpu().numpy())
    scored = np.maximum(o64["counts"][0, :, 5], 1)
    print("the tracker's own candidate: max |nll - nll64| / scored %.3e" % (np.abs(nll[1].cpu().numpy() - o64["nll"][0]) / scored).max())


# ---- 3: against fp64 -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_on_gpu(seed, rows, frames=nr.T):
    return torch.from_numpy(np.array(nr.model_record(seed, rows)[0][:frames])).cuda()


@pytest.mark.parametrize("rows", [28, 3])
def test_the_likelihood_follows_the_fp64_rule(rows):
    from hupr_amd import functional as F_
    p, grid = tracking(nr.RATE), nr.model_grid()
    meas = model_on_gpu(0, rows)
    nll, counts, _ = F_.pose_track_nll(meas, zeros_start(nr.T), p, grid, nr.EXTENT, nr.RATIO)
    o64 = nr.ref_nll(meas.cpu().numpy(), np.zeros(nr.T, int), p, grid, nr.RATIO, nr.EXTENT)
    near = o64["near"] < NEAR_GATE
    keep = ~near
    assert near.mean() <= 0.02
    nll, counts = nll.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(counts[keep], o64["counts"][keep])
    scored = o64["counts"][..., 5]
    assert (scored[keep] > 0).all()
    rel = (np.abs(nll - o64["nll"])[keep] / scored[keep]).max()
    print("rows %d: %.2f %% of %d cells left out; max |nll - nll64| / scored %.3e (bound %.3e); argmin %d, the reference's %d"
          % (rows, 100 * near.mean(), near.size, rel, TOL_NLL_REL, nll.sum(1).argmin(), o64["nll"].sum(1).argmin()))
    assert rel <= TOL_NLL_REL
    assert nll.sum(1).argmin() == o64["nll"].sum(1).argmin()
    if rows == 28:
        assert nll.sum(1).argmin() == nr.TRUE_INDEX


# ---- 4: sequence starts ---------------------------------------------------------------------------------------------------------------------
def test_a_start_flag_zeroes_the_tracks_between_two_sequences():
    from hupr_amd import functional as F_
    p, grid = tracking(nr.RATE), nr.model_grid()
    a, b = model_on_gpu(0, 28, 24), model_on_gpu(1, 28, 24)
    na, ca, _ = F_.pose_track_nll(a, zeros_start(24), p, grid, nr.EXTENT, nr.RATIO)
    nb, cb, fb = F_.pose_track_nll(b, zeros_start(24, 0), p, grid, nr.EXTENT, nr.RATIO)
    both = torch.cat([a, b])
    n, c, f = F_.pose_track_nll(both, zeros_start(48, 24), p, grid, nr.EXTENT, nr.RATIO)
    assert torch.equal(f, fb) and torch.equal(c, ca + cb)
    assert ((n - (na + nb)).abs() <= 1e-9 * (na + nb).abs()).all().item()
    # without the flag the second sequence inherits the first one's tracks
    n2, c2, f2 = F_.pose_track_nll(both, zeros_start(48), p, grid, nr.EXTENT, nr.RATIO)
    assert not torch.equal(f2, fb) and not torch.equal(c2, c) and (c2[..., 3].sum() < c[..., 3].sum()).item()
    # a bool start is taken too
    flags = torch.zeros(48, dtype=torch.bool, device="cuda")
    flags[24] = True
    n3, c3, f3 = F_.pose_track_nll(both, flags, p, grid, nr.EXTENT, nr.RATIO)
    assert torch.equal(n3, n) and torch.equal(c3, c) and torch.equal(f3, f)


# ---- 5: run to run, edges ---------------------------------------------------------------------------------------------------------------------
def test_two_launches_are_identical_and_the_edges_work():
    from hupr_amd import functional as F_
    p, grid = tracking(nr.RATE), nr.model_grid()
    meas = model_on_gpu(0, 28)
    one = F_.pose_track_nll(meas, zeros_start(nr.T), p, grid, nr.EXTENT, nr.RATIO)
    two = F_.pose_track_nll(meas, zeros_start(nr.T), p, grid, nr.EXTENT, nr.RATIO)
    for x, y in zip(one, two):
        assert torch.equal(x, y)
    # G = 1: the candidate's column of the grid launch; a row alone: its row
    g1 = F_.pose_track_nll(meas, zeros_start(nr.T), p, grid[[nr.TRUE_INDEX]], nr.EXTENT, nr.RATIO)
    for x, y in zip(one, g1):
        assert torch.equal(x[nr.TRUE_INDEX], y[0])
    r1 = F_.pose_track_nll(meas[:, 5:6].contiguous(), zeros_start(nr.T), p, grid, nr.EXTENT, nr.RATIO)
    for x, y in zip(one, r1):
        assert torch.equal(x[:, 5], y[:, 0])
    # T = 1: every row starts a track and nothing is scored
    nll, counts, final = F_.pose_track_nll(meas[:1], zeros_start(1), p, grid, nr.EXTENT, nr.RATIO)
    assert not nll.any().item() and (counts[..., 3] == 1).all().item() and (counts.sum(-1) == 1).all().item()
    assert torch.equal(final[..., 0:2], meas[0, :, 0:2].expand(81, 28, 2)) and (final[..., 14] == 1).all().item()
    # T = 0 zeroes the outputs without a launch
    n0 = launches()
    nll, counts, final = F_.pose_track_nll(meas[:0], zeros_start(0), p, grid, nr.EXTENT, nr.RATIO)
    assert launches() == n0 and nll.shape == (81, 28) and not nll.any().item() and not counts.any().item() and not final.any().item()
    # a lead of two axes, as a live session's (lanes, K)
    lead2 = F_.pose_track_nll(meas.reshape(nr.T, 2, 14, 8), zeros_start(nr.T), p, grid, nr.EXTENT, nr.RATIO)
    assert lead2[0].shape == (81, 2, 14) and torch.equal(lead2[0].reshape(81, 28), one[0]) and lead2[2].shape == (81, 2, 14, 16)
    # a bad candidate raises in Python, before any launch
    n0 = launches()
    for bad in ([-1.0, 1.0, 1.0], [100.0, 0.0, 1.0]):
        with pytest.raises(ValueError):
            F_.pose_track_nll(meas, zeros_start(nr.T), p, np.vstack([grid, [bad]]), nr.EXTENT, nr.RATIO)
    assert launches() == n0


# ---- 6: the fit ---------------------------------------------------------------------------------------------------------------------------------
def test_fit_tracking_recovers_the_models_noise():
    from hupr_amd.tools import MeasurementRecord, TrackingFit, fit_tracking
    meas = model_on_gpu(0, 28)
    rec = MeasurementRecord((28,), "cuda", ratio=nr.RATIO, extent=nr.EXTENT, capacity=4)
    for t in range(nr.T):
        rec.append(meas[t], start=t == 0)
    assert len(rec) == nr.T and torch.equal(rec.views()[0], meas) and rec.views()[1].tolist() == [1] + [0] * (nr.T - 1)
    p = tracking(nr.RATE, heatmap_gain=0.0)
    n0 = launches()
    fit = fit_tracking(rec, p, fit=("accel_psd", "meas_std"))
    assert launches() - n0 == 3                                                         # one launch per round
    assert isinstance(fit, TrackingFit)
    print(fit.line())
    assert nr.TRUE_Q / 2 <= fit.tracking.accel_psd <= nr.TRUE_Q * 2 and nr.TRUE_STD / 2 <= fit.tracking.meas_std <= nr.TRUE_STD * 2
    assert fit.tracking.heatmap_gain == 0.0 and fit.tracking.rate_hz == p.rate_hz and fit.tracking.gate == p.gate
    assert fit.cost_per_measurement[1] <= fit.cost_per_measurement[0]
    assert fit.grid[0].shape == (81, 3) and fit.grid[1].shape == (81,) and fit.counts[5] > 0 and sum(fit.counts[:5]) == nr.T * 28
    # what it reports is what a launch at the fitted values gives
    from hupr_amd import functional as F_
    v = fit.tracking
    nll, counts, _ = F_.pose_track_nll(meas, rec.views()[1], p, [[v.accel_psd, v.meas_std, v.heatmap_gain]], nr.EXTENT, nr.RATIO)
    assert tuple(counts.sum(dim=(0, 1)).tolist()) == fit.counts
    total = nll.sum().item()                                                            # fp64 sums of 28 terms, in whatever order
    assert abs(fit.cost_per_measurement[1] * fit.counts[5] - total) <= 1e-12 * total and abs(fit.grid[1].min() - total) <= 1e-12 * total


# ---- 7: the offline route, the live session, Runner.eval ----------------------------------------------------------------------------------------
def test_a_sequence_smoother_with_measurements_records_them():
    from hupr_amd import functional as F_
    from hupr_amd.tools import SequenceSmoother, TrackingError
    heat = torch.from_numpy(np.array(ref.scenario()[0][:12])).cuda()
    p = tracking(accel_psd=100.0, min_score=ref.MIN_SCORE)
    sm, plain = SequenceSmoother(p, ref.ROWS, "cuda", measurements=True), SequenceSmoother(p, ref.ROWS, "cuda")
    assert plain.record is None
    with pytest.raises(TrackingError):
        plain.fit_tracking()
    n0 = launches()
    for t in range(12):
        plain.track(heat[t], ref.RATIO)
    n1 = launches()
    for t in range(12):
        if t == 7:
            sm.new_sequence()
        sm.track(heat[t], ref.RATIO)
    assert n1 - n0 == 12 and launches() - n1 == 24                                      # one more launch per frame, none without the flag
    meas, start = sm.record.views()
    assert start.tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0] and sm.record.extent == (256.0, 256.0) and sm.record.ratio == 4.0
    h = sm.history._views()
    assert torch.equal(meas[..., 0:2], h["raw"]) and torch.equal(meas[..., 2], h["scores"])
    assert torch.equal(meas[3], F_.pose_measure(heat[3], ref.RATIO)[3])
    fit = sm.fit_tracking(rounds=1)
    assert fit.cost_per_measurement[1] <= fit.cost_per_measurement[0] and fit.counts[3] >= 2 * (ref.ROWS - 1)
    sm.clear()
    assert len(sm.record) == 0


@pytest.fixture(scope="module")
def ctx():
    from test_stream_smooth_gpu import _Ctx
    c = _Ctx()
    yield c
    c.engine.close()


def test_a_session_with_measurements_records_what_it_emitted(ctx):
    from test_stream_smooth_gpu import FIELDS, N
    from hupr_amd.tools import TrackingError, stream as st
    n0 = launches()
    off = ctx.session(measurements=False)                                               # the first session of a model also packs its weights
    ctx.play(off)
    n1 = launches()
    plain = ctx.session()
    as_today = ctx.play(plain)
    n2 = launches()
    s = ctx.session(measurements=True)
    frames = ctx.play(s)
    n3 = launches()
    assert bool(s._graphs) and bool(plain._graphs) and plain.measurements is None and off.measurements is None
    # without the flag nothing is added; with it one launch per pose that is not a graph replay (the warm-up, the capture, the flush)
    assert n1 - n0 >= n2 - n1
    assert (n3 - n2) - (n2 - n1) == st.WARMUP_PUSHES + 1 + s.lookahead
    for a, b in zip(as_today, frames):
        for k in FIELDS:
            assert torch.equal(getattr(a, k), getattr(b, k)), (a.frame, k)
    with pytest.raises(TrackingError):
        plain.fit_tracking()
    meas, start = s.measurements.views()
    assert meas.shape == (N, 1, 14, 8) and start.tolist() == [1] + [0] * (N - 1)
    assert torch.equal(meas[..., 0:2], torch.stack([f.raw_keypoints for f in frames]))
    assert torch.equal(meas[..., 2], torch.stack([f.scores for f in frames]))
    assert torch.isfinite(meas[..., 0:3]).all().item()
    fit = s.fit_tracking()
    print(fit.line())
    assert fit.cost_per_measurement[1] <= fit.cost_per_measurement[0] and sum(fit.counts[:5]) == N * 14
    assert fit.tracking.rate_hz == s.track.rate_hz and s.track.accel_psd == 200.0      # the session goes on as it was built
    s.reset()                                                                           # the record stays, the next pose starts a sequence
    ctx.play(s)
    assert s.measurements.views()[1].tolist() == ([1] + [0] * (N - 1)) * 2
    with pytest.raises(TrackingError):
        from hupr_amd.tools import PoseStream
        PoseStream(ctx.model, ctx.cfg, measurements=True)


def test_eval_with_temporal_fit_prints_the_fitted_values(tmp_path, monkeypatch, capsys):
    from test_stream_smooth_gpu import FRAMES, _eval
    lines, recs = _eval(tmp_path, monkeypatch, capsys, "fit", temporal="track", temporalFit=True)
    assert len(recs) == FRAMES
    fit = [l for l in lines if l.startswith("tracker fit:")]
    assert len(fit) == 1 and lines.index(fit[0]) > max(i for i, l in enumerate(lines) if l.startswith("Jitter "))
    m = re.fullmatch(r"tracker fit: accel_psd (\S+), meas_std (\S+), heatmap_gain (\S+) \| cost per measurement (\S+) configured, (\S+) "
                     r"fitted \| updated (\d+), missing (\d+), gated (\d+), started (\d+), lost (\d+), scored (\d+)", fit[0])
    assert m, fit[0]
    q, s, h, before, after = (float(m.group(k)) for k in range(1, 6))
    assert q >= 0 and s > 0 and h >= 0 and np.isfinite([q, s, h, before, after]).all() and after <= before
    assert sum(int(m.group(k)) for k in range(6, 11)) == FRAMES * 14
    # off without the key: no line; a non-bool raises where the config is read
    lines, _ = _eval(tmp_path, monkeypatch, capsys, "nofit", temporal="track")
    assert not [l for l in lines if l.startswith("tracker fit:")]
    with pytest.raises(ValueError, match="temporalFit"):
        _eval(tmp_path, monkeypatch, capsys, "badfit", temporal="track", temporalFit="yes")
