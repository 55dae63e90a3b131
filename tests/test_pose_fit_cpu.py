"""CPU (-m "not gpu"): the maximum-likelihood fit of the tracker's noise parameters (csrc/pose_fit.hip, tools/calibrate.py) on its NumPy
restatement (tests/pose_nll_ref.py): the restatement against pose_track_ref.ref_track, the likelihood's minimum on records drawn from
the filter's own model, the outlier cap, the fit on the tracker tests' scenario, the fp32 run against the fp64 run; then the argument
checks of the two entries and of the Python layers, and the kernels' metadata.  No launch.

The model-drawn record (pose_nll_ref.model_record): white-acceleration tracks, q = 400 pixel^2 / s^3, isotropic measurement noise of
2.5 pixel, 28 rows x 48 frames at 10 Hz, seeds 0 to 2; the 9 x 9 grid (pose_nll_ref.model_grid): accel_psd in factors of 2 and meas_std
in factors of sqrt 2 around the truth, heatmap_gain 0.  Measured here (fp64):

    seed   cost at the truth   runner-up behind by   cells with a gate decision within 1e-3   |nll32 - nll64| / scored (max)
       0        9 423.3               66.1                      1.41 %                                 1.16e-5
       1        9 413.6               75.8                      0.84 %                                 2.17e-5
       2        9 561.2               55.1                      1.10 %                                 1.05e-5

NLL_REL_FP32 = 2.17e-5 is the largest of the last column, over the cells that have no gate decision within 1e-3 of the gate (a cell
with one may decide differently in fp32, and then differs by a whole frame's cost); tests/test_pose_fit_gpu.py allows the kernel 16 x
that.

The scenario (pose_track_ref.scenario, arg-max measurements, min_score 0.1, PoseTracking's defaults as the start), three rounds:

                                   accel_psd   meas_std   heatmap_gain   summed cost   rms error on the 24 event-free rows
    defaults                          200        1           1            14 154.6          3.057 px
    the tracker tests' accel_psd      100        1           1            14 161.7          3.456 px
    fitted                            168.2      6.9e-4      0.25         12 226.9          2.901 px

The fitted meas_std is the smallest value the three rounds can reach from 1: with heatmap_gain 0.25 the window term alone is the
measurement noise (R about 13 pixel^2 against the scene's 9 plus the 4-pixel grid's quantisation), and the floor no longer matters."""
import numpy as np
import pytest
import torch

import pose_nll_ref as nr
import pose_track_ref as ref
from listing import kernel_metadata

NLL_REL_FP32 = 2.17e-5
NEAR_GATE = 1e-3
SEEDS = (0, 1, 2)


def shared(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(nr.RATE, **kw)


def model_run(seed, dtype=np.float64):
    return nr.ref_nll(nr.model_record(seed)[0], np.zeros(nr.T, int), shared(), nr.model_grid(), nr.RATIO, nr.EXTENT, dtype=dtype)


def scenario_record():
    """The scenario's arg-max measurements -> (meas (T, ROWS, 8), start)."""
    idx, mx, mom = ref.scenario_moments()
    raw = np.stack([idx % ref.HM, idx // ref.HM], -1).astype(np.float64) * ref.RATIO
    start = np.zeros(ref.T, int)
    start[0] = 1
    return nr.record_of(np.where((mx > 0)[..., None], raw, 0.0), mx, mom), start


def test_one_candidate_is_ref_track():
    from hupr_amd.tools import PoseTracking
    p = PoseTracking(ref.RATE, accel_psd=100.0, min_score=ref.MIN_SCORE)
    meas, start = scenario_record()
    o = nr.ref_nll(meas, start, p, [[p.accel_psd, p.meas_std, p.heatmap_gain]], ref.RATIO, (256, 256))
    t = ref.ref_track(meas[..., :2], meas[..., 2], meas[..., 3:7], p, ref.RATIO)
    assert np.array_equal(o["status"][:, 0], t["status"])
    assert np.abs(o["kp"][:, 0] - t["kp"]).max() < 1e-9 and np.abs(o["state"][0] - t["state"]).max() < 1e-9
    assert np.array_equal(o["counts"][0, :, :5], np.stack([(t["status"] == c).sum(0) for c in range(5)], -1))
    d2 = t["d2"]
    assert np.array_equal(o["counts"][0, :, 5], np.isfinite(d2).sum(0))
    assert len(set(np.unique(t["status"]))) == 5                                        # the scenario shows every status
    cap = nr.outlier_cost((256, 256))
    assert abs(cap - 18.505) < 0.001                                                    # 2 ln(65536 / 2 pi)
    assert (o["nll"][0] <= o["counts"][0, :, 5] * cap + 1e-9).all() and o["nll"][0, ref.NEVER] == 0 and o["counts"][0, ref.NEVER, 5] == 0
    assert o["nll"][0, ref.OUTLIER] > 0 and t["status"][ref.OUTLIER_FRAME, ref.OUTLIER] == ref.COASTED_GATED


@pytest.mark.parametrize("seed", SEEDS)
def test_the_minimum_on_a_model_drawn_record_is_the_truth(seed):
    o = model_run(seed)
    cost = o["nll"].sum(1)
    order = np.argsort(cost, kind="stable")
    near = o["near"] < NEAR_GATE
    print("seed %d: cost at the truth %.1f, runner-up (candidate %d) behind by %.1f, %.2f %% of the cells with a gate decision within "
          "%g" % (seed, cost[nr.TRUE_INDEX], order[1], cost[order[1]] - cost[order[0]], 100 * near.mean(), NEAR_GATE))
    assert order[0] == nr.TRUE_INDEX
    assert tuple(nr.model_grid()[nr.TRUE_INDEX]) == (nr.TRUE_Q, nr.TRUE_STD, 0.0)
    assert near.mean() <= 0.02


@pytest.mark.parametrize("seed", SEEDS)
def test_the_cap_makes_a_candidate_that_gates_everything_out_pay(seed):
    meas = nr.model_record(seed)[0]
    o = nr.ref_nll(meas, np.zeros(nr.T, int), shared(), [[nr.TRUE_Q / 4096, nr.TRUE_STD / 64, 0.0], [nr.TRUE_Q, nr.TRUE_STD, 0.0]],
                   nr.RATIO, nr.EXTENT)
    tiny, truth = o["nll"].sum(1)
    counts = o["counts"].sum(1)
    print("seed %d: tiny R and Q cost %.1f with counts %s, the truth %.1f with %s" % (seed, tiny, counts[0].tolist(), truth, counts[1].tolist()))
    assert counts[0, ref.COASTED_GATED] > 4 * counts[0, ref.UPDATED] and counts[1, ref.COASTED_GATED] <= 2    # it refuses most frames: five of six, then the track ends ...
    assert tiny > truth                                                                 # ... and pays for it
    uncapped = nr.ref_nll(meas, np.zeros(nr.T, int), shared(), [[nr.TRUE_Q / 4096, nr.TRUE_STD / 64, 0.0]], nr.RATIO, (1e30, 1e30))
    assert uncapped["nll"].sum() > 10 * tiny                                            # what the refused frames would cost without it


def test_the_fit_on_the_scenario_costs_and_errs_no_more_than_the_defaults():
    from hupr_amd.tools import PoseTracking, TrackingError
    from hupr_amd.tools import calibrate as cal
    meas, start = scenario_record()
    p0 = PoseTracking(ref.RATE, min_score=ref.MIN_SCORE)
    launches = []

    def evaluate(grid):
        launches.append(grid.shape[0])
        r = nr.ref_nll(meas, start, p0, grid, ref.RATIO, (256, 256))
        c = r["nll"].sum(1)
        return c, r["counts"].sum(1), int(np.argmin(c))

    fit = cal.search(evaluate, p0)
    assert launches == [810, 810, 810]
    normal = [r for r in range(ref.ROWS) if r not in (ref.DROP, ref.OUTLIER, ref.GONE, ref.NEVER)]
    truth = ref.scenario()[1]

    def run(p):
        r = nr.ref_nll(meas, start, p, [[p.accel_psd, p.meas_std, p.heatmap_gain]], ref.RATIO, (256, 256))
        e = (r["kp"][:, 0] - truth)[:, normal]
        return float(r["nll"].sum()), float(np.sqrt(np.mean(np.sum(e ** 2, -1)))), r["counts"].sum(1)[0]

    rows = [("defaults", p0), ("accel_psd 100", PoseTracking(ref.RATE, accel_psd=100.0, min_score=ref.MIN_SCORE)), ("fitted", fit.tracking)]
    got = {}
    for name, p in rows:
        got[name] = run(p)
        print("%-14s accel_psd %-8.6g meas_std %-10.4g heatmap_gain %-6.4g cost %.1f  rms %.3f px" % (
            (name, p.accel_psd, p.meas_std, p.heatmap_gain) + got[name][:2]))
    print(fit.line())
    assert len(normal) == 24
    assert got["fitted"][0] <= got["defaults"][0] and got["fitted"][1] <= got["defaults"][1]
    # what the TrackingFit says is what a run at those values gives
    scored = int(got["fitted"][2][5])
    assert fit.counts == tuple(int(c) for c in got["fitted"][2])
    assert abs(fit.cost_per_measurement[1] - got["fitted"][0] / scored) < 1e-9
    assert abs(fit.cost_per_measurement[0] - got["defaults"][0] / int(got["defaults"][2][5])) < 1e-9
    assert fit.cost_per_measurement[1] <= fit.cost_per_measurement[0]
    assert fit.grid[0].shape == (810, 3) and fit.grid[1].shape == (810,) and fit.grid[1].min() == got["fitted"][0]
    # the other settings are carried over, and so are the association settings of a tracking that has them
    for k in ("rate_hz", "gate", "max_coast", "init_speed_std", "min_score", "horizon_s", "candidates", "pair_swap"):
        assert getattr(fit.tracking, k) == getattr(p0, k), k
    # a parameter not in fit stays fixed; round 1 holds the start
    part = cal.search(evaluate, p0, fit=("accel_psd",), rounds=1)
    assert launches[-1] == 9 and (part.tracking.meas_std, part.tracking.heatmap_gain) == (p0.meas_std, p0.heatmap_gain)
    assert part.cost_per_measurement[1] <= part.cost_per_measurement[0]
    for bad in ((), ("gate",), ("accel_psd", "accel_psd"), 3):
        with pytest.raises(TrackingError):
            cal.search(evaluate, p0, fit=bad)
    for bad in (0, 1.5, True):
        with pytest.raises(TrackingError):
            cal.search(evaluate, p0, rounds=bad)


def test_the_candidate_axes_are_nine_log_spaced_values_and_a_zero_gain():
    from hupr_amd.tools import calibrate as cal
    values = dict(accel_psd=200.0, meas_std=1.0, heatmap_gain=1.0)
    axes = cal.candidate_axes(values, values, cal.FITTED, 4.0)
    assert [len(a) for a in axes] == [9, 9, 10] and axes[2][-1] == 0.0 and axes[0][4] == 200.0
    assert np.allclose(axes[1], 4.0 ** np.arange(-4, 5)) and np.allclose(axes[0][1:] / axes[0][:-1], 4.0)
    grid = cal.candidate_grid(axes)
    assert grid.shape == (810, 3) and tuple(grid[0]) == (axes[0][0], axes[1][0], axes[2][0]) and tuple(grid[1][:2]) == tuple(grid[0][:2])
    # the next round spans one step of this one on both sides
    finer = cal.candidate_axes(values, values, cal.FITTED, 4.0 ** 0.25)
    assert np.isclose(finer[0][0], 200.0 / 4.0) and np.isclose(finer[0][-1], 200.0 * 4.0)
    # held out of the fit: one value; a current value of 0 is searched around the fallback and stays a candidate
    held = cal.candidate_axes(dict(values, heatmap_gain=0.0), values, ("accel_psd", "meas_std"), 4.0)
    assert held[2].tolist() == [0.0]
    zero = cal.candidate_axes(dict(values, accel_psd=0.0), values, cal.FITTED, 4.0)
    assert len(zero[0]) == 10 and zero[0][-1] == 0.0 and zero[0][4] == 200.0


@pytest.mark.parametrize("seed", SEEDS)
def test_the_fp32_restatement_agrees_with_the_fp64_one(seed):
    """Where NLL_REL_FP32 comes from."""
    o64, o32 = model_run(seed), model_run(seed, np.float32)
    keep = (o64["near"] >= NEAR_GATE) & (o64["counts"][..., 5] > 0)
    assert np.array_equal(o32["counts"][keep], o64["counts"][keep])
    rel = (np.abs(o32["nll"] - o64["nll"])[keep] / o64["counts"][..., 5][keep]).max()
    print("seed %d: max |nll32 - nll64| / scored %.3e over %d of %d cells (NLL_REL_FP32 = %.3e)" % (seed, rel, keep.sum(), keep.size, NLL_REL_FP32))
    assert rel <= NLL_REL_FP32 * 1.01 and (seed != 1 or rel >= NLL_REL_FP32 / 4)
    assert o32["nll"].sum(1).argmin() == o64["nll"].sum(1).argmin()


# ---- the entries, the Python layers, the listing -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


P = 4096                                                   # any non-null, 16-byte aligned address: every call below returns before it launches
NAN, INF = float("nan"), float("inf")


def test_entry_points_check_their_arguments_on_the_host(L):
    def measure(heat=P, rows=14, H=64, W=64, outs=(P,) * 4):
        return L.hupr_pose_measure_f32(heat, rows, H, W, 4.0, 1, *outs, None)

    def nll(meas=P, start=P, T=10, rows=14, ratio=4.0, rate=10.0, gate=13.816, max_coast=5, speed=50.0, min_score=0.0, cap=18.5,
            params=P, G=81, outs=(P, P, P)):
        return L.hupr_pose_track_nll_f32(meas, start, T, rows, ratio, rate, gate, max_coast, speed, min_score, cap, params, G, *outs, None)

    c0 = L.hupr_launch_count()
    assert measure(None, 0, 0, 0, (None,) * 4) == 0                                     # rows == 0: a no-op
    assert measure(heat=None) == -1 and b"null" in L.hupr_last_error()
    for k in range(4):
        assert measure(outs=tuple(None if j == k else P for j in range(4))) == -1 and b"null" in L.hupr_last_error()
    for bad in (dict(rows=-1), dict(rows=1 << 31), dict(H=0), dict(W=-2), dict(H=1 << 16, W=1 << 16)):
        assert measure(**bad) == -1 and b"shape" in L.hupr_last_error(), bad
    assert measure(outs=(P, P, P, P + 4)) == -1 and b"aligned" in L.hupr_last_error()

    assert nll(None, None, 10, 14, params=None, G=0, outs=(None,) * 3) == 0             # G == 0 and rows == 0: no-ops
    assert nll(None, None, 10, 0, params=None, outs=(None,) * 3) == 0
    for bad in (dict(T=-1), dict(rows=-1), dict(G=-1), dict(T=1 << 31), dict(rows=1 << 31), dict(G=(1 << 22) + 1)):
        assert nll(**bad) == -1 and b"shape" in L.hupr_last_error(), bad
    for bad in (dict(meas=None), dict(start=None), dict(params=None), dict(outs=(None, P, P)), dict(outs=(P, None, P))):
        assert nll(**bad) == -1 and b"null" in L.hupr_last_error(), bad
    assert nll(meas=P + 4) == -1 and b"aligned" in L.hupr_last_error()
    assert nll(outs=(P, P, P + 8)) == -1 and b"aligned" in L.hupr_last_error()
    for bad in (dict(rate=0.0), dict(rate=NAN), dict(rate=INF), dict(gate=0.0), dict(gate=NAN), dict(max_coast=-1), dict(speed=0.0),
                dict(speed=INF), dict(min_score=NAN)):
        assert nll(**bad) == -1 and b"bad tracker parameter" in L.hupr_last_error(), bad
    for bad in (dict(ratio=0.0), dict(ratio=NAN), dict(ratio=INF), dict(cap=NAN)):
        assert nll(**bad) == -1 and b"ratio" in L.hupr_last_error(), bad
    assert b"hupr_pose_track_nll_f32" in L.hupr_last_error()
    assert L.hupr_launch_count() == c0


def test_candidates_are_checked_in_python_before_the_upload():
    from hupr_amd import functional as F_
    ok = F_.check_track_candidates([[200.0, 1.0, 1.0], [0.0, 1e-3, 0.0]])
    assert ok.dtype == np.float32 and ok.shape == (2, 3)
    assert F_.check_track_candidates(torch.tensor([[1.0, 2.0, 3.0]])).tolist() == [[1.0, 2.0, 3.0]]
    for bad in ([[-1.0, 1.0, 1.0]], [[1.0, 0.0, 1.0]], [[1.0, -1.0, 1.0]], [[1.0, 1.0, -0.5]], [[NAN, 1.0, 1.0]], [[1.0, INF, 1.0]],
                [[1e39, 1.0, 1.0]], [[1.0, 1e-50, 1.0]], [1.0, 1.0, 1.0], [[1.0, 1.0]], "abc", [[200.0, 1.0, 1.0], [1.0, 1.0, NAN]]):
        with pytest.raises(ValueError):
            F_.check_track_candidates(bad)
    assert abs(F_.outlier_cost((256, 256)) - nr.outlier_cost((256, 256))) == 0
    for bad in ((0, 256), (256,), None, (INF, 1)):
        with pytest.raises(ValueError):
            F_.outlier_cost(bad)
    # no CPU fallback, and the argument errors come first
    meas, start = torch.zeros((4, 3, 8)), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        F_.pose_track_nll(meas, start, shared(), [[1.0, 1.0, 1.0]], (256, 256), 4.0)
    with pytest.raises(ValueError):
        F_.pose_track_nll(torch.zeros((4, 3, 7)), start, shared(), [[1.0, 1.0, 1.0]], (256, 256), 4.0)


def test_temporal_fit_is_read_where_the_config_is_read():
    from hupr_amd.config_tree import load_config
    from hupr_amd.tools.smooth import temporal_setting
    cfg = load_config()
    assert temporal_setting(cfg) is None
    cfg.TEST.temporal = "track"
    assert temporal_setting(cfg).fit is False
    cfg.TEST.temporalFit = True
    assert temporal_setting(cfg).fit is True
    for bad in (1, 0, "true", "yes", None, 1.0):
        cfg.TEST.temporalFit = bad
        with pytest.raises(ValueError, match="temporalFit"):
            temporal_setting(cfg)
    cfg.TEST.temporalFit, cfg.TEST.temporal = True, "off"
    with pytest.raises(ValueError, match="temporalFit"):
        temporal_setting(cfg)
    cfg.TEST.temporalFit = False
    assert temporal_setting(cfg) is None


def test_sessions_and_the_command_check_the_new_arguments():
    from hupr_amd.tools import stream as st
    from hupr_amd.tools import MeasurementRecord, PoseTracking, SequenceSmoother, TrackingError, fit_tracking
    a = st.parse(["--raw", "x", "--track", "--rate", "10", "--fit-tracker"])
    assert a.fit_tracker and not st.parse(["--raw", "x", "--track", "--rate", "10"]).fit_tracker
    with pytest.raises(SystemExit):
        st.parse(["--raw", "x", "--fit-tracker"])
    with pytest.raises(ValueError):
        SequenceSmoother(PoseTracking(10.0), 3, "cpu", measurements=1)
    with pytest.raises(TrackingError):
        fit_tracking(object(), PoseTracking(10.0))
    rec = MeasurementRecord((3,), "cpu")
    with pytest.raises(TrackingError):
        fit_tracking(rec, PoseTracking(10.0))                                           # no ratio, no extent
    rec = MeasurementRecord((3,), "cpu", ratio=4.0, extent=(256.0, 256.0), capacity=2)
    with pytest.raises(ValueError):
        rec.views()
    for k in range(5):                                                                  # grows by doubling, keeps what it held
        rec.append(torch.full((3, 8), float(k)), start=k in (0, 3))
    meas, start = rec.views()
    assert len(rec) == 5 and meas.shape == (5, 3, 8) and start.tolist() == [1, 0, 0, 1, 0]
    assert meas[:, 0, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    rec.clear()
    assert len(rec) == 0


def test_pose_fit_kernels_use_no_scratch():
    """The listing the build keeps for csrc/pose_fit.hip: its two kernels, 64 threads each, with 0 spilled registers, 0 bytes of scratch
    and no LDS — read from the code-object metadata only."""
    meta = kernel_metadata("pose_fit")
    assert len(meta) == 2 and any("hupr_k_pose_measure" in k for k in meta) and any("hupr_k_pose_track_nll" in k for k in meta), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, (name, m)
        assert m["threads"] == 64, (name, m)
