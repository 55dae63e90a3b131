"""CPU (-m "not gpu"): the radar point cloud as tests/radar_points_ref.py states it — the peak rule on hand-built planes, one mover
through the oracle chain, the association and the geometry on hand-built lists — the figures the device test takes its tolerances
from, and the host side of csrc/radar_points.hip (argument checks; no launch), the settings and the command's arguments."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import cfar_ref
import radar_points_ref as P
from test_cfar_cpu import oracle_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = cfar_ref.DEFAULTS


def _cells(points, count):
    return [(int(c) // P.CELLS, (int(c) % P.CELLS) // P.A, int(c) % P.A) for c in points[:count, 5]]


# ---- the peak rule -------------------------------------------------------------------------------------------------------------------
def _round32(exact):
    """A rational -> the nearest float32, ties to the even mantissa."""
    import fractions
    c = np.float32(float(exact))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    return min(cands, key=lambda v: (abs(fractions.Fraction(float(v)) - exact), int(np.float32(v).view(np.int32)) & 1))


def test_power32_is_the_fused_rounding():
    """``power32`` against exact rational arithmetic: fl32(re^2 + fl32(im^2)), on noise cells and on a half-way case, where the fp64
    sum alone would round the other way: re = 1 + 2^-12, so re^2 = 1 + 2^-11 + 2^-24 lies half way between two fp32 values; with
    im = 2^-30 the fused sum lies above the middle and rounds up, with im = 0 it is a tie and goes to the even value below."""
    import fractions
    x = cfar_ref.noise_planes(1, 5)
    x[0, 0, 0, 0], x[0, 1, 0, 0] = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -30)
    x[0, 0, 0, 1], x[0, 1, 0, 1] = np.float32(1 + 2.0 ** -12), 0.0
    p = P.power32(x)
    assert p.dtype == np.float32 and p.shape == (1, 8, 64, 64)
    assert p[0, 0, 0, 0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and p[0, 0, 0, 1] == np.float32(1 + 2.0 ** -11)
    for a in range(64):
        for f in (0, 4, 7):
            re, im = float(x[0, 2 * f, 0, a]), float(x[0, 2 * f + 1, 0, a])
            exact = fractions.Fraction(re) ** 2 + fractions.Fraction(float(_round32(fractions.Fraction(im) ** 2)))
            assert p[0, f, 0, a] == _round32(exact), (f, a)
    assert np.all(np.abs(p.astype(np.float64) - cfar_ref.power(x)) <= 2.0 ** -23 * cfar_ref.power(x))


@pytest.mark.parametrize("name", ["plateau", "corners", "slots", "separation", "nan"])
def test_the_statement_on_hand_built_planes(name):
    """plateau: four cells of equal power over two slots give their lowest cell, once.  corners: a peak in each corner of the map.
    slots: peaks in slots 3 and 5 at one cell, slot 4 between them holding 1e6 and a NaN — never read.  separation: 4 azimuth
    cells apart the weaker peak goes, 5 apart both stay.  nan: a NaN two cells from a peak — inside the guard area, so the
    detector flags the peak, and inside the box, so it is no point."""
    x, want, kw = P.hand_cases()[name]
    det = cfar_ref.ref_cfar(x, D["pfa"], D["guard"], D["train"])
    out = P.ref_peaks(x, det["mask"], det["snr"], max_points=8, **kw)
    count, found = out["counts"][0]
    assert count == found == len(want) and _cells(out["points"][0], count) == want
    pts = out["points"][0]
    assert np.all(pts[count:] == (0, 0, 0, 0, 0, -1))
    assert np.all(np.diff(pts[:count, 3]) <= 0)
    for k, (f, r, a) in enumerate(want):
        assert det["mask"][0, f, r, a] == 1 and pts[k, 2] == f - 4 and pts[k, 4] == det["snr"][0, f, r, a]
        assert abs(pts[k, 0] - r) < 1 and abs(pts[k, 1] - a) <= 0.5
    if name == "separation":
        assert det["mask"][0, 2, 10, 24] == 1 and not out["peaks"][0, 2, 10, 24]      # detected, and suppressed by its neighbour
    if name == "nan":
        assert det["mask"][0, 2, 30, 30] == 1 and not out["peaks"][0, 2, 30, 30]
    if name == "corners":
        assert np.all(pts[:4, 1] == [63, 63, 0, 0])                                   # no azimuth offset at the map's edge


TRIAL_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 9, 13, 15)
TRIAL_RANGE_MAX, TRIAL_AZ_MAX = 0.304, 1.180      # measured (docstring below); the bounds are 1.5 times these


def _trial_target(seed):
    from hupr_amd import synth
    u = synth.uniform01(3, "points_trial", seed)
    return dict(range_bin=40.0 + 45.0 * u[0], az_bin=-20.0 + 40.0 * u[1], el_bin=0.0, doppler_bin=float((-3, -2, -1, 1, 2, 3)[seed % 6]), amp=15.0)


@functools.lru_cache(maxsize=None)
def _trial(seed):
    from hupr_amd import synth
    t = _trial_target(seed)
    x = oracle_planes(synth.point_target_cube([t], noise=300.0, seed=seed, tdm=True))[None]
    det = cfar_ref.ref_cfar(x, D["pfa"], D["guard"], D["train"])
    return t, det, P.ref_peaks(x, det["mask"], det["snr"])


@pytest.mark.parametrize("seed", TRIAL_SEEDS)
def test_one_mover_through_the_oracle_chain_is_one_point(seed):
    """One mover at a random fractional range and azimuth bin (amp 15 under noise 300 per component) through the oracle chain without
    TDM compensation, default detector: 6 to 13 detected cells, exactly one peak, in the mover's slot.  Of the seeds 0..15 the
    detector fires on twelve; these are eleven of them — seed 14 also fires on one far noise cell, a second (false) point, and is
    left out.  Measured with this statement on these seeds: refined range off by 0.304 bins at most (0.127 rms), refined azimuth by
    1.180 cells at most (0.638 rms); asserted with 1.5 times the maxima.  The azimuth error holds the known shift of d / 6 of a
    cell that the uncompensated TDM phase causes at Doppler bin d (up to half a cell here), on top of the noise on a lobe that is
    8 cells wide.  PAPERS.md."""
    t, det, out = _trial(seed)
    count, found = out["counts"][0]
    rng, az, d = out["points"][0, 0, :3]
    err_r, err_a = rng - (94.0 - t["range_bin"]), az - (31.0 - t["az_bin"])
    print("seed %d: %d cells, %d peaks, range error %.3f, azimuth error %.3f" % (seed, det["mask"].sum(), found, err_r, err_a))
    assert det["mask"].sum() >= 3 and count == found == 1 and d == t["doppler_bin"]
    assert abs(err_r) <= 1.5 * TRIAL_RANGE_MAX and abs(err_a) <= 1.5 * TRIAL_AZ_MAX


def test_the_trials_recorded_maxima_are_the_measured_ones():
    errs = np.array([[_trial(s)[2]["points"][0, 0, 0] - (94.0 - _trial(s)[0]["range_bin"]),
                      _trial(s)[2]["points"][0, 0, 1] - (31.0 - _trial(s)[0]["az_bin"])] for s in TRIAL_SEEDS])
    print("range: max %.3f rms %.3f; azimuth: max %.3f rms %.3f" % (np.abs(errs[:, 0]).max(), np.sqrt((errs[:, 0] ** 2).mean()),
                                                                   np.abs(errs[:, 1]).max(), np.sqrt((errs[:, 1] ** 2).mean())))
    assert abs(np.abs(errs[:, 0]).max() - TRIAL_RANGE_MAX) < 1e-3 and abs(np.abs(errs[:, 1]).max() - TRIAL_AZ_MAX) < 1e-3


# ---- the figures the device test rests on ------------------------------------------------------------------------------------------------
def _device_inputs():
    yield "noise", cfar_ref.noise_planes(3, P.NOISE_SEED), (P.NOISE_PFA, D["guard"], D["train"]), dict(max_points=256)
    for name, (x, _, kw) in P.hand_cases().items():
        yield name, x, (D["pfa"], D["guard"], D["train"]), dict(max_points=8, **kw)
    yield "planted", P.planted_planes()[0], P.PLANTED_CFAR, dict(max_points=64)
    yield "checker", P.checker_planes(), P.CHECKER_CFAR, dict(max_points=256, sep_range=0, sep_azimuth=0)


def test_fp32_refinement_against_fp64_on_the_device_tests_planes():
    """The reference alone, on the planes of tests/test_radar_points_gpu.py: the share of points whose curvature is under 0.05 stays
    under 10 % (it is 0), the fp32 statement of the azimuth lies within ``AZ32_MEASURED`` of the fp64 one on the others, and the fp32
    range within the header's bound."""
    worst, total, excluded = 0.0, 0, 0
    for name, x, cfar, kw in _device_inputs():
        det = cfar_ref.ref_cfar(x, *cfar)
        out = P.ref_peaks(x, det["mask"], det["snr"], **kw)
        for i in range(x.shape[0]):
            k = out["counts"][i, 0]
            assert k > 0
            pts, cv = out["points"][i, :k], out["curv"][i, :k]
            flat = cv < P.CURV_MIN
            total, excluded = total + k, excluded + int(flat.sum())
            worst = max(worst, float(np.abs(pts[:, 1] - out["az32"][i, :k])[~flat].max()))
            r = (pts[:, 5].astype(np.int64) % P.CELLS) // P.A
            assert np.all(np.abs(pts[:, 0] - out["range32"][i, :k]) <= P.range_bound(pts[:, 0], r)), name
    print("%d points, %d with a flat lobe, fp32 azimuth within %.3e of fp64" % (total, excluded, worst))
    assert excluded <= 0.1 * total
    assert 0.5 * P.AZ32_MEASURED <= worst <= P.AZ32_MEASURED


def test_capacity_and_overflow_planes_hold_what_the_device_test_expects():
    x, spots = P.planted_planes()
    det = cfar_ref.ref_cfar(x, *P.PLANTED_CFAR)
    out = P.ref_peaks(x, det["mask"], max_points=64)
    assert out["counts"][0].tolist() == [64, 300] and set(_cells(out["points"][0], 64)) <= set(spots)
    x = P.checker_planes()
    det = cfar_ref.ref_cfar(x, *P.CHECKER_CFAR)
    out = P.ref_peaks(x, det["mask"], max_points=256, sep_range=0, sep_azimuth=0)
    count, found = out["counts"][0]
    assert count == 256 and found > 2 * P.STAGE
    keys = np.flatnonzero(out["peaks"][0].ravel())
    assert set(out["points"][0, :, 5].astype(np.int64)) <= set(keys[:P.STAGE])      # only the first 4096 in cell order are ranked
    assert out["p32"][0].ravel()[keys[P.STAGE:]].max() > out["points"][0, -1, 3]    # a later, stronger peak is left out


# ---- fusion ------------------------------------------------------------------------------------------------------------------------------
def _model():
    from hupr_amd import simulate as sim
    return sim.RadarModel()


@pytest.mark.parametrize("name", ["contend", "gate", "doppler", "radicand", "nearest"])
def test_fusion_on_hand_built_lists(name):
    from hupr_amd.preprocessing.points import radar_geometry
    rows_h, rows_v, want = P.fuse_cases(_model())[name]
    (ph, ch), (pv, cv) = P.points_list(rows_h), P.points_list(rows_v)
    cloud, counts = P.ref_fuse(ph, ch, pv, cv, radar_geometry(_model()))
    k = counts[0]
    assert [(int(r[6]), int(r[7])) for r in cloud[0, :k]] == want
    assert np.all(cloud[0, k:] == (0, 0, 0, 0, 0, 0, -1, -1))
    assert np.all(cloud[0, :k, 1] > 0)                                                 # in front of the radar
    for r in cloud[0, :k]:
        assert r[3] == rows_h[int(r[6])][2] * radar_geometry(_model())[1]
    if name == "contend":
        assert cloud[0, 0, 4] == 9.0 and cloud[0, 0, 5] == 7.0
    if name == "radicand":                                                             # the dropped pair's vertical point stays taken
        assert abs((31.0 - 1.0) / 32.0) ** 2 + abs((31.0 - 2.0) / 32.0) ** 2 > 1


@pytest.mark.parametrize("p", [(-0.5, 1.1, 0.2), (0.3, 1.9, -0.4), (0.0, 2.5, 0.0), (0.9, 2.9, 0.5), (-1.2, 3.2, -0.3)])
def test_geometry_inverts_expected_cell(p):
    """A scatterer at ``p`` (1.2 to 3.5 m away) -> ``expected_cell`` of both sensors -> the rule: the range |p - o_h| comes back to
    1e-9 m, and so does the position.  ``expected_cell`` is itself the far-field statement — range and direction cosine from each
    sensor's ORIGIN — and for it the rule is exact algebra: c_h = p . a_h, c_v = p . a_v (the vertical range goes with the vertical
    cosine, each about o_v), c_b from the horizontal range about o_h.  Measured: 2.2e-16 m at most, an angle error of 0.  The far-field
    error proper — the antennas sit up to 12 mm from the origin, a parallax of 12 mm / R — is not in ``expected_cell``; it is measured
    through the simulator, where it is part of the 0.0879 m of the end-to-end case (``E2E_STATEMENT_MAX_M``), most of which is noise
    on the 8-cell lobe.  Through the fp32 lists the position keeps the lists' rounding: 2^-24 of a cell index below 64 is 4e-6
    cells, 1.4e-7 m of range and 1.2e-7 of a cosine, under 2e-6 m at 3.5 m; asserted with 2e-5."""
    from hupr_amd.preprocessing.points import radar_geometry
    m = _model()
    v = np.array(p) / np.linalg.norm(p) * 0.2
    cells = [m.expected_cell(s, p, v) for s in ("hori", "vert")]
    geo = radar_geometry(m)
    ph = np.array([[[cells[0][0], cells[0][1], cells[0][2], 1, 1, -1]]])
    pv = np.array([[[cells[1][0], cells[1][1], cells[1][2], 1, 1, -1]]])
    one = np.array([[1, 1]], dtype=np.int32)
    # fp64 rows: the rule itself, without the fp32 storage of the lists
    rb, dv, a_h, o_h, a_v, o_v, b = P.fuse_axes(geo)
    Rh, uh = (94.0 - ph[0, 0, 0]) * rb, (31.0 - ph[0, 0, 1]) / 32.0
    Rv, uv = (94.0 - pv[0, 0, 0]) * rb, (31.0 - pv[0, 0, 1]) / 32.0
    c_h, c_v = o_h @ a_h + Rh * uh, o_v @ a_v + Rv * uv
    pos = c_h * a_h + c_v * a_v + (o_h @ b + np.sqrt(Rh * Rh - (c_h - o_h @ a_h) ** 2 - (c_v - o_h @ a_v) ** 2)) * b
    assert abs(Rh - np.linalg.norm(np.array(p) - o_h)) < 1e-9
    assert np.abs(pos - np.array(p)).max() < 1e-9
    assert abs(ph[0, 0, 2] * dv - 0.2) < 1e-9                                          # doppler_mps_per_bin inverts expected_cell
    print("position error %.1e m" % np.abs(pos - np.array(p)).max())
    cloud, counts = P.ref_fuse(ph.astype(np.float32), one, pv.astype(np.float32), one, geo, range_gate=4.0)
    assert counts[0] == 1 and np.abs(cloud[0, 0, :3] - np.array(p)).max() < 2e-5


def test_end_to_end_statement_figure():
    """The fp64 statement of the device test's end-to-end case: two points in each of the three frames, each mover within
    ``E2E_STATEMENT_MAX_M`` of one; without the movers, no point."""
    cloud, counts, pos = P.e2e_statement(_model())
    d = P.match_distances(cloud, counts, pos)
    print("points per frame %s, distances %s" % (counts.tolist(), np.round(d, 4).tolist()))
    assert counts.tolist() == [2, 2, 2]
    assert abs(d.max() - P.E2E_STATEMENT_MAX_M) < 5e-4
    _, empty, _ = P.e2e_statement(_model(), 0.0)
    assert empty.tolist() == [0, 0, 0]


# ---- settings --------------------------------------------------------------------------------------------------------------------------
BAD_POINTS = [dict(sep_range=-1), dict(sep_range=5), dict(sep_range=1.0), dict(sep_range=True), dict(sep_azimuth=-1), dict(sep_azimuth=9),
              dict(sep_azimuth="4"), dict(range_gate=-0.5), dict(range_gate=float("nan")), dict(range_gate=float("inf")), dict(range_gate="1"),
              dict(range_gate=True), dict(doppler_gate=-1), dict(doppler_gate=8), dict(doppler_gate=1.0), dict(max_points=0),
              dict(max_points=257), dict(max_points=64.0), dict(max_points=None), dict(separation=1)]


@pytest.mark.parametrize("kw", BAD_POINTS, ids=lambda kw: "-".join("%s=%r" % kv for kv in kw.items()))
def test_check_points_refuses_bad_values(kw):
    from hupr_amd.preprocessing import PointCloudSettings, check_points
    with pytest.raises(ValueError):
        check_points(**kw)
    if "separation" not in kw:
        with pytest.raises(ValueError):
            PointCloudSettings(**kw)


def test_point_cloud_settings_defaults_and_frozen():
    from hupr_amd.preprocessing import PointCloudSettings, check_points
    s = PointCloudSettings()
    assert {k: getattr(s, k) for k in s.__slots__} == dict(pfa=1e-5, guard=2, train=4, **P.DEFAULTS)
    assert check_points(sep_range=np.int64(4), range_gate=2) == {"sep_range": 4, "range_gate": 2.0}
    assert s == PointCloudSettings() and s != PointCloudSettings(max_points=8) and hash(s) == hash(PointCloudSettings())
    with pytest.raises(AttributeError):
        s.max_points = 3
    assert "sep_azimuth=4" in repr(s)
    for bad in (dict(pfa=0.0), dict(guard=5, train=4), dict(train=0)):
        with pytest.raises(ValueError):
            PointCloudSettings(**bad)


def test_radar_geometry_of_the_default_model():
    from hupr_amd.preprocessing.points import geometry_vector, radar_geometry
    m = _model()
    rb, dv, a_h, o_h, a_v, o_v = radar_geometry(m)
    assert rb == m.range_bin_m and dv == m.wavelength / (64 * 6 * m.chirp_period_s)
    assert a_h.tolist() == [1, 0, 0] and a_v.tolist() == [0, 0, 1] and o_h.tolist() == [0, 0, 0] and o_v.tolist() == [0, 0, -0.10]
    assert geometry_vector(radar_geometry(m)).shape == (14,)
    for bad in (None, (1.0, 2.0), (rb, dv, a_h, o_h, a_v), (rb, dv, a_h[:2], o_h, a_v, o_v), (rb, dv, "x", o_h, a_v, o_v)):
        with pytest.raises(ValueError):
            geometry_vector(bad)


def test_command_arguments():
    from hupr_amd.preprocessing import PointCloudSettings
    from hupr_amd.tools import points as tp
    a = tp.parse(["--data", "d", "--seq", "single_1", "--out", "o.npz"])
    assert a.settings == PointCloudSettings() and a.frames == (0, None) and a.ply is None and not a.tdm_compensation
    a = tp.parse(["--data", "d", "--seq", "s", "--out", "o.npz", "--frames", "3:9", "--ply", "p", "--tdm-compensation", "--pfa", "1e-4",
                  "--cfar-guard", "1", "--cfar-train", "3", "--sep-range", "2", "--sep-azimuth", "6", "--range-gate", "2.5",
                  "--doppler-gate", "0", "--max-points", "16"])
    assert a.settings == PointCloudSettings(1e-4, 1, 3, 2, 6, 2.5, 0, 16) and a.frames == (3, 9) and a.ply == "p" and a.tdm_compensation
    assert tp.parse(["--data", "d", "--seq", "s", "--out", "o", "--frames", ":5"]).frames == (0, 5)
    assert tp.parse(["--data", "d", "--seq", "s", "--out", "o", "--frames", "2:"]).frames == (2, None)
    for extra in (["--pfa", "2"], ["--sep-range", "5"], ["--max-points", "0"], ["--frames", "5:3"], ["--frames", "x"], ["--range-gate", "-1"],
                  ["--cfar-guard", "6", "--cfar-train", "3"], ["--block", "0"]):
        with pytest.raises(SystemExit):
            tp.parse(["--data", "d", "--seq", "s", "--out", "o"] + extra)
    for missing in (["--seq", "s", "--out", "o"], ["--data", "d", "--out", "o"], ["--data", "d", "--seq", "s"]):
        with pytest.raises(SystemExit):
            tp.parse(missing)


def test_ply_file(tmp_path):
    from hupr_amd.tools import points as tp
    rows = np.array([[0.5, 2.0, -0.25, 0.25, 20.0, 18.0, 0, 1], [-1.0, 3.0, 0.5, -0.3, 15.0, 13.0, 1, 0]], dtype=np.float32)
    path = str(tmp_path / "f.ply")
    tp.write_ply(path, rows)
    lines = open(path).read().splitlines()
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0" and "element vertex 2" in lines and lines[-3] == "end_header"
    assert [float(v) for v in lines[-2].split()] == [0.5, 2.0, -0.25, 0.25, 20.0, 18.0]
    tp.write_ply(path, rows[:0])
    assert "element vertex 0" in open(path).read() and open(path).read().endswith("end_header\n")


# ---- the library's host side -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


def _geo(**change):
    from hupr_amd.preprocessing.points import geometry_vector, radar_geometry
    v = geometry_vector(radar_geometry(_model())).copy()
    for k, val in change.items():
        v[int(k[1:])] = val
    return v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), v


def test_library_argument_errors_before_any_launch(lib):
    """Every refusal comes back as HUPR_ERR_ARG from the host checks: nothing is launched (there is no GPU here)."""
    one = ctypes.c_void_p(16)                      # a non-null pointer that is never followed: the checks come first
    peaks = lambda n=1, mp=64, sr=1, sa=4, planes=one, mask=one, points=one, counts=one: lib.hupr_radar_peaks_f32(
        planes, mask, None, n, mp, sr, sa, points, counts, None)
    for kw in (dict(n=-1), dict(mp=0), dict(mp=257), dict(sr=-1), dict(sr=5), dict(sa=-1), dict(sa=9), dict(n=(1 << 20) + 1)):
        assert peaks(**kw) == -1
    assert peaks(sa=9) == -1 and b"sep_azimuth" in lib.hupr_last_error()
    for kw in (dict(planes=None), dict(mask=None), dict(points=None), dict(counts=None)):
        assert peaks(**kw) == -1 and b"null" in lib.hupr_last_error()
    assert peaks(n=0, planes=None, mask=None, points=None, counts=None) == 0          # no frame: a no-op
    assert peaks(n=0, mp=0, planes=None, mask=None, points=None, counts=None) == -1   # ... with valid settings only

    good, keep = _geo()
    fuse = lambda n=1, mh=64, mv=64, geo=good, rg=1.5, dg=1, ph=one, ch=one, pv=one, cv=one, cloud=one, cc=one: \
        lib.hupr_radar_points_fuse_f32(ph, ch, mh, pv, cv, mv, n, geo, rg, dg, cloud, cc, None)
    for kw in (dict(n=-1), dict(mh=0), dict(mh=257), dict(mv=0), dict(mv=300), dict(rg=-1.0), dict(rg=float("nan")), dict(rg=float("inf")),
               dict(dg=-1), dict(dg=8), dict(geo=None)):
        assert fuse(**kw) == -1
    for change, word in ((dict(i0=0.0), b"range_bin_m"), (dict(i0=-1.0), b"range_bin_m"), (dict(i1=0.0), b"doppler"),
                         (dict(i5=float("nan")), b"finite"), (dict(i2=0.9), b"unit"), (dict(i10=1.001), b"unit"),
                         (dict(i8=1.0, i10=0.0), b"orthogonal"), (dict(i8=1e-6), b"orthogonal"),
                         (dict(i8=0.0, i9=1.0, i10=0.0), b"boresight")):
        bad, hold = _geo(**change)
        assert fuse(geo=bad) == -1 and word in lib.hupr_last_error(), (change, lib.hupr_last_error())
    for kw in (dict(ph=None), dict(ch=None), dict(pv=None), dict(cv=None), dict(cloud=None), dict(cc=None)):
        assert fuse(**kw) == -1 and b"null" in lib.hupr_last_error()
    assert fuse(n=0, ph=None, ch=None, pv=None, cv=None, cloud=None, cc=None) == 0
    assert keep.shape == (14,)


def test_no_cpu_fallback():
    import torch
    from hupr_amd import functional as F_, preprocessing
    from hupr_amd.preprocessing.points import radar_geometry
    from hupr_amd.runtime import HuprError
    planes, mask = torch.zeros((1, 16, 64, 64)), torch.zeros((1, 8, 64, 64), dtype=torch.uint8)
    with pytest.raises(HuprError):
        F_.radar_peaks(planes, mask)
    for bad in ((planes[:, :, :32], mask), (planes, mask.float()), (planes, mask[:, :7]), (planes.double(), mask)):
        with pytest.raises(ValueError):
            F_.radar_peaks(*bad)
    with pytest.raises(ValueError):
        F_.radar_peaks(planes, mask, snr=torch.zeros((1, 8, 64, 32)))
    with pytest.raises(ValueError):
        F_.radar_peaks(planes, mask, max_points=0)
    pk = F_.RadarPeaks(torch.zeros((1, 4, 6)), torch.zeros((1, 2), dtype=torch.int32), 4, 1, 4)
    assert pk.range.shape == (1, 4) and pk.found.shape == (1,) and not hasattr(pk, "__dict__")
    with pytest.raises(HuprError):
        F_.radar_points_fuse(pk, pk, radar_geometry(_model()))
    with pytest.raises(ValueError):
        F_.radar_points_fuse(pk, pk.points, radar_geometry(_model()))
    with pytest.raises(ValueError):
        F_.radar_points_fuse(pk, pk, radar_geometry(_model()), range_gate=-1)
    cube = torch.zeros((1, 4, 192, 256, 2), dtype=torch.int16)
    with pytest.raises(HuprError):
        preprocessing.radar_point_cloud(cube, cube)
    for bad in (dict(settings=1e-5), dict(model="iwr1843")):
        with pytest.raises(ValueError):
            preprocessing.radar_point_cloud(cube, cube, **bad)
    with pytest.raises(ValueError):
        preprocessing.radar_point_cloud(cube, cube.float())
    with pytest.raises(ValueError):
        preprocessing.radar_point_cloud(cube, torch.zeros((2, 4, 192, 256, 2), dtype=torch.int16))


def test_host_code_is_clean_under_the_sanitizers(tmp_path):
    """The argument checks and the derived geometry of csrc/radar_points_host.h in a stand-alone program
    (scripts/radar_points_host_check.cpp) built with the address and undefined-behaviour sanitizers: it runs to the end and reports
    nothing."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "radar_points_host_check")
    src = os.path.join(ROOT, "scripts", "radar_points_host_check.cpp")
    inc = os.path.join(ROOT, "hupr-a-benchmark-for-human-pose-estimation-using-millimeter-wave-radar_amd", "csrc")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc,
                            src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("sanitize" in build.stderr or "asan" in build.stderr.lower()):
        pytest.skip("this compiler cannot link the sanitizer runtimes")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ok" in run.stdout and not run.stderr, run.stdout + run.stderr
