"""GPU (-m gpu): the two kernels of csrc/radar_points.hip against their NumPy statement (tests/radar_points_ref.py).  Every equality
case feeds the statement the detector kernel's own mask and SNR (``functional.cfar_ra`` on the same planes), so counts, cells, order,
power and SNR compare bit for bit; the refined range is held to the header's bound, the refined azimuth to twice the measured
distance of the rule in fp32 from the rule in fp64 (``AZ_TOL``, tests/test_radar_points_cpu.py), on the points whose lobe has a
curvature of at least 0.05.  At most 3 frames per call."""
import functools

import numpy as np
import pytest
import torch

import cfar_ref
import radar_points_ref as P
from hupr_amd import functional as F_
from hupr_amd import preprocessing
from hupr_amd import simulate as sim
from hupr_amd.preprocessing.points import radar_geometry

pytestmark = pytest.mark.gpu
D = cfar_ref.DEFAULTS
DEFAULT_CFAR = (D["pfa"], D["guard"], D["train"])
MODEL = sim.RadarModel()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _input(name):
    """-> (planes, cfar settings, peak settings), shared and never modified."""
    if name == "noise":
        return cfar_ref.noise_planes(3, P.NOISE_SEED), (P.NOISE_PFA, D["guard"], D["train"]), dict(max_points=256)
    if name == "planted":
        return P.planted_planes()[0], P.PLANTED_CFAR, dict(max_points=64)
    if name == "checker":
        return P.checker_planes(), P.CHECKER_CFAR, dict(max_points=256, sep_range=0, sep_azimuth=0)
    x, _, kw = P.hand_cases()[name]
    return x, DEFAULT_CFAR, dict(max_points=8, **kw)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (RadarPeaks of the kernel, the statement on the kernel's own mask and SNR, the detector's result)."""
    x, cfar, kw = _input(name)
    planes = _dev(x)
    det = F_.cfar_ra(planes, *cfar, want_mask=True, want_snr=True)
    got = F_.radar_peaks(planes, det.mask, det.snr, **kw)
    want = P.ref_peaks(x, det.mask.cpu().numpy(), det.snr.cpu().numpy().astype(np.float64), **kw)
    return got, want, det


def _assert_equal_fields(got, want):
    counts = got.counts.cpu().numpy()
    pts = got.points.cpu().numpy()
    assert got.points.dtype == torch.float32 and got.counts.dtype == torch.int32
    assert np.array_equal(counts, want["counts"]), (counts.tolist(), want["counts"].tolist())
    w = want["points"]
    for col in (2, 3, 4, 5):                                    # Doppler bin, power, SNR, cell: the same bits, the same order
        assert np.array_equal(pts[..., col], w[..., col].astype(np.float32)), col
    for i in range(pts.shape[0]):                               # the zero / -1 tail
        assert np.all(pts[i, counts[i, 0]:] == np.array([0, 0, 0, 0, 0, -1], dtype=np.float32))
    assert torch.equal(got.cell, got.points[..., 5]) and torch.equal(got.count, got.counts[..., 0]) and torch.equal(got.found, got.counts[..., 1])


def _assert_float_fields(got, want, name):
    pts = got.points.cpu().numpy().astype(np.float64)
    total = excluded = 0
    worst_r = worst_a = 0.0
    for i in range(pts.shape[0]):
        k = want["counts"][i, 0]
        g, w, cv = pts[i, :k], want["points"][i, :k], want["curv"][i, :k]
        r = (w[:, 5].astype(np.int64) % P.CELLS) // P.A
        err_r = np.abs(g[:, 0] - w[:, 0])
        assert np.all(err_r <= 4 * P.U32 * np.abs(w[:, 0]) + P.range_bound(w[:, 0], r)), (name, i)
        worst_r = max(worst_r, float(err_r.max()))
        flat = cv < P.CURV_MIN
        total, excluded = total + k, excluded + int(flat.sum())
        by_rule = np.isnan(cv) | (w[:, 1] == w[:, 5] % P.A)     # offset 0 by rule: exact
        assert np.all(g[by_rule & ~flat, 1] == w[by_rule & ~flat, 1]), (name, i)
        err_a = np.abs(g[:, 1] - w[:, 1])[~flat]
        assert np.all(err_a <= P.AZ_TOL), (name, i, float(err_a.max()))
        worst_a = max(worst_a, float(err_a.max()))
        assert np.all(np.abs(g[:, 1] - w[:, 5] % P.A) <= 0.5)
    print("%s: %d points, %d excluded (flat lobe), range within %.3e, azimuth within %.3e (tolerance %.3e)"
          % (name, total, excluded, worst_r, worst_a, P.AZ_TOL))
    assert excluded <= 0.1 * total


@pytest.mark.parametrize("name", ["plateau", "corners", "slots", "separation", "nan"])
def test_hand_built_planes(name):
    got, want, det = _case(name)
    _assert_equal_fields(got, want)
    _assert_float_fields(got, want, name)
    cells = [(int(c) // P.CELLS, (int(c) % P.CELLS) // P.A, int(c) % P.A) for c in got.cell[0, :int(got.count[0])].cpu().numpy()]
    assert cells == P.hand_cases()[name][1]
    for f, r, a in cells:
        assert int(det.mask[0, f, r, a]) == 1


def test_noise_planes_counts_cells_and_order():
    """Unit complex-Gaussian planes at pfa = 1e-2: about 290 detections and 200 points per frame."""
    got, want, det = _case("noise")
    assert want["counts"][:, 0].min() >= 150 and np.all(want["counts"][:, 1] <= 256)
    _assert_equal_fields(got, want)


def test_noise_planes_float_fields():
    got, want, _ = _case("noise")
    _assert_float_fields(got, want, "noise")


def test_capacity_keeps_the_strongest_in_order():
    """300 planted peaks, 64 rows: the 64 strongest in order, found == 300."""
    got, want, _ = _case("planted")
    assert want["counts"][0].tolist() == [64, 300]
    _assert_equal_fields(got, want)
    _assert_float_fields(got, want, "planted")
    power = got.power[0].cpu().numpy()
    assert np.all(np.diff(power) < 0)
    x, cfar, _ = _input("planted")
    planes = _dev(x)
    det = F_.cfar_ra(planes, *cfar, want_mask=True)
    small = F_.radar_peaks(planes, det.mask, max_points=5)      # fewer rows, and no SNR given: zeros
    assert small.counts[0].tolist() == [5, 300] and torch.equal(small.points[0][:, [0, 1, 2, 3, 5]], got.points[0, :5][:, [0, 1, 2, 3, 5]])
    assert not small.snr.any()
    wide = F_.radar_peaks(planes, det.mask, det.snr, max_points=256, sep_range=4, sep_azimuth=8)      # the largest box, and a tail
    ref = P.ref_peaks(x, det.mask.cpu().numpy(), None, max_points=256, sep_range=4, sep_azimuth=8)
    assert np.array_equal(wide.counts.cpu().numpy(), ref["counts"]) and 0 < ref["counts"][0, 1] < 256
    assert np.array_equal(wide.cell.cpu().numpy(), ref["points"][..., 5].astype(np.float32))


def test_overflow_ranks_the_first_4096_and_reports_the_true_count():
    """A checkerboard with more than 4096 peaks: found is the true count, the first 4096 in cell order are ranked, and a second run
    gives the same bits."""
    got, want, _ = _case("checker")
    assert want["counts"][0, 0] == 256 and want["counts"][0, 1] > 2 * P.STAGE
    _assert_equal_fields(got, want)
    _assert_float_fields(got, want, "checker")
    x, cfar, kw = _input("checker")
    planes = _dev(x)
    det = F_.cfar_ra(planes, *cfar, want_mask=True, want_snr=True)
    again = F_.radar_peaks(planes, det.mask, det.snr, **kw)
    assert torch.equal(again.points, got.points) and torch.equal(again.counts, got.counts)


def test_frames_do_not_depend_on_their_neighbours_and_no_frame_is_a_no_op():
    from hupr_amd import runtime
    got, _, det = _case("noise")
    x, cfar, kw = _input("noise")
    planes = _dev(x)
    n = runtime.lib().hupr_launch_count()
    one = F_.radar_peaks(planes[1:2], det.mask[1:2], det.snr[1:2], **kw)
    assert runtime.lib().hupr_launch_count() == n + 1                                  # one launch per call
    assert torch.equal(one.points[0], got.points[1]) and torch.equal(one.counts[0], got.counts[1])
    lead = F_.radar_peaks(planes.reshape(3, 1, 16, 64, 64), det.mask.reshape(3, 1, 8, 64, 64), det.snr.reshape(3, 1, 8, 64, 64), **kw)
    assert lead.points.shape == (3, 1, 256, 6) and torch.equal(lead.points.reshape(3, 256, 6), got.points)
    n = runtime.lib().hupr_launch_count()
    empty = F_.radar_peaks(planes[:0], det.mask[:0], det.snr[:0], **kw)
    assert empty.points.shape == (0, 256, 6) and empty.counts.shape == (0, 2)
    cloud = F_.radar_points_fuse(empty, empty, radar_geometry(MODEL))
    assert cloud.cloud.shape == (0, 256, 8) and cloud.counts.shape == (0,) and runtime.lib().hupr_launch_count() == n


# ---- fusion ------------------------------------------------------------------------------------------------------------------------------
def _peaks(rows, max_points=8):
    pts, counts = P.points_list(rows, max_points)
    return F_.RadarPeaks(_dev(pts), _dev(counts), max_points, 1, 4), pts, counts


@pytest.mark.parametrize("name", ["contend", "gate", "doppler", "radicand", "nearest"])
def test_fusion_lists_through_the_kernel(name):
    rows_h, rows_v, pairs = P.fuse_cases(MODEL)[name]
    (gh, ph, ch), (gv, pv, cv) = _peaks(rows_h), _peaks(rows_v, 5)
    geo = radar_geometry(MODEL)
    got = F_.radar_points_fuse(gh, gv, geo)
    want, counts = P.ref_fuse(ph, ch, pv, cv, geo)
    cloud = got.cloud.cpu().numpy()
    assert got.cloud.shape == (1, 8, 8) and got.counts.dtype == torch.int32 and got.counts.cpu().numpy().tolist() == counts.tolist()
    k = counts[0]
    assert [(int(r[6]), int(r[7])) for r in cloud[0, :k]] == pairs
    assert np.array_equal(cloud[0, :, 4:], want[0, :, 4:].astype(np.float32))          # both SNRs, both rows, the -1 tail
    assert np.all(cloud[0, k:, :4] == 0)
    assert np.all(np.abs(cloud[0, :k, :4] - want[0, :k, :4]) <= 1e-5 * np.abs(want[0, :k, :4]))      # metres and m/s
    assert torch.equal(got.xyz, got.cloud[..., :3]) and torch.equal(got.row_v, got.cloud[..., 7]) and got.peaks_h is gh
    again = F_.radar_points_fuse(gh, gv, geo)
    assert torch.equal(again.cloud, got.cloud)
    if name == "gate":                                                                  # a wider gate takes the second pair too
        assert F_.radar_points_fuse(gh, gv, geo, range_gate=1.6).counts.tolist() == [2]
    if name == "doppler":
        assert F_.radar_points_fuse(gh, gv, geo, doppler_gate=0).counts.tolist() == [0]
        assert F_.radar_points_fuse(gh, gv, geo, doppler_gate=2).counts.tolist() == [2]


def test_fusion_of_full_lists():
    """256 rows a sensor, three frames: every horizontal point of the noise planes against a shuffled copy of its own list as the
    vertical one — the serial pass at its longest, against the statement."""
    got, _, _ = _case("noise")
    pts, counts = got.points.cpu().numpy(), got.counts.cpu().numpy()
    perm = np.argsort(cfar_ref.noise_planes(1, 77).ravel()[:256], kind="stable")
    pv = pts.copy()
    for i in range(3):
        k = counts[i, 0]
        pv[i, :k] = pts[i, :k][np.argsort(perm[:k], kind="stable")]
    gv = F_.RadarPeaks(_dev(pv), got.counts, 256, 1, 4)
    geo = radar_geometry(MODEL)
    fused = F_.radar_points_fuse(got, gv, geo, range_gate=0.75)
    want, wc = P.ref_fuse(pts, counts, pv, counts, geo, range_gate=0.75)
    cloud = fused.cloud.cpu().numpy()
    assert fused.counts.cpu().numpy().tolist() == wc.tolist() and wc.min() > 50
    assert np.array_equal(cloud[..., 4:], want[..., 4:].astype(np.float32))
    assert np.all(np.abs(cloud[..., :4] - want[..., :4]) <= 1e-5 * np.abs(want[..., :4]))


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def _e2e_cloud(scale):
    pos, vel, amp = P.e2e_scene(MODEL)
    cubes = []
    for si, sensor in enumerate(("hori", "vert")):
        tx, rx = MODEL.array(sensor)
        cubes.append(F_.radar_scene(_dev(pos), _dev(vel), _dev(amp * np.float32(scale)), tx, rx, MODEL.wavelength, MODEL.range_bin_m,
                                    MODEL.chirp_period_s, add=_dev(P.e2e_noise(si))))
    return preprocessing.radar_point_cloud(cubes[0], cubes[1], MODEL, tdm_compensation=True), pos


def test_two_simulated_movers_come_back_in_metres():
    """``functional.radar_scene`` for both sensors of ``RadarModel()``, three frames of two movers 0.8 m apart in x at 2.2 m and 2.9 m
    with radial speeds of two and minus three Doppler bins under seeded noise, TDM compensation on: ``radar_point_cloud`` returns two
    points per frame, each within ``E2E_BOUND_M`` = 0.1319 m of its mover — 1.5 times the 0.0879 m that the fp64 statement of the
    whole chain leaves on the same scene (tests/test_radar_points_cpu.py::test_end_to_end_statement_figure) — and with its mover's
    radial velocity.  The same noise without the movers gives no point."""
    rc, pos = _e2e_cloud(1.0)
    counts, cloud = rc.counts.cpu().numpy(), rc.cloud.cpu().numpy()
    d = P.match_distances(cloud, counts, pos)
    print("points per frame %s, distances %s m (statement: at most %.4f, bound %.4f)" % (counts.tolist(), np.round(d, 4).tolist(),
                                                                                         P.E2E_STATEMENT_MAX_M, P.E2E_BOUND_M))
    assert counts.tolist() == [2, 2, 2]
    assert d.max() <= P.E2E_BOUND_M
    dv = radar_geometry(MODEL)[1]
    for i in range(P.E2E_FRAMES):
        for s, bins in enumerate((2.0, -3.0)):
            k = int(np.argmin(np.linalg.norm(cloud[i, :2, :3] - pos[i, s], axis=1)))
            assert cloud[i, k, 3] == np.float32(bins * dv)
        assert sorted(cloud[i, :2, 6].tolist()) == [0.0, 1.0] and np.all(cloud[i, 2:, 6:] == -1)
    assert rc.peaks_h.points.shape == (3, 64, 6) and rc.peaks_v.counts.shape == (3, 2)
    empty, _ = _e2e_cloud(0.0)
    assert empty.counts.cpu().numpy().tolist() == [0, 0, 0] and not empty.cloud[..., :6].any()


def test_the_command_on_a_simulated_tree(tmp_path, capsys):
    """``python -m hupr_amd.tools.points`` on a simulated recording of 4 frames, frames 1:4 in blocks of 2: the arrays it writes are
    those of one ``radar_point_cloud`` call on the same cubes, one .ply per frame with as many vertices as the frame has points."""
    from hupr_amd.tools import points as tp
    root = sim.write_simulated_dataset(str(tmp_path / "data"), {"test": [1]}, 4, 3)
    out, ply = str(tmp_path / "cloud.npz"), str(tmp_path / "ply")
    tp.main(["--data", root, "--seq", "single_1", "--out", out, "--ply", ply, "--frames", "1:4", "--tdm-compensation", "--block", "2",
             "--max-points", "32"])
    line = capsys.readouterr().out
    z = np.load(out)
    assert z["frames"].tolist() == [1, 2, 3] and z["cloud"].shape == (3, 32, 8) and z["counts"].shape == (3,)
    assert z["points_h"].shape == z["points_v"].shape == (3, 32, 6) and z["counts_h"].shape == z["counts_v"].shape == (3, 2)
    assert "3 frames" in line and "%.2f points per frame" % z["counts"].mean() in line
    seed = sim.sequence_seed(3, 1)
    cubes = sim.simulate_sequence(MODEL, sim.walking_body(4, MODEL.frame_rate_hz, seed), noise_std=2.0, seed=seed)
    rc = preprocessing.radar_point_cloud(cubes[0][1:4], cubes[1][1:4], settings=preprocessing.PointCloudSettings(max_points=32),
                                         tdm_compensation=True)
    assert np.array_equal(z["cloud"], rc.cloud.cpu().numpy()) and np.array_equal(z["counts"], rc.counts.cpu().numpy())
    assert np.array_equal(z["points_h"], rc.peaks_h.points.cpu().numpy()) and np.array_equal(z["counts_v"], rc.peaks_v.counts.cpu().numpy())
    assert z["counts_h"][:, 0].min() > 0                                               # the walker is detected in every frame
    for k, f in enumerate((1, 2, 3)):
        lines = open("%s/%09d.ply" % (ply, f)).read().splitlines()
        assert "element vertex %d" % z["counts"][k] in lines and len(lines) == lines.index("end_header") + 1 + z["counts"][k]
