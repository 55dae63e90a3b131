"""CPU (-m "not gpu"): the radar scene simulator's model and host side.  The fp64 statement (tests/radar_scene_ref.py) against the
bin-domain scene of ``synth.point_target_scene(tdm=True)`` in the far field — the anchor of the array's sign conventions — and through
the oracle's FFT chain; the entry points' argument checks, which return before any launch; the body, the camera, the data-set writer
and the command line.  The device kernel is compared with the same statement in tests/test_radar_scene_gpu.py."""
import json
import os

import numpy as np
import pytest

import radar_scene_ref as R
import tdm_ref
from hupr_amd import simulate as sim
from hupr_amd import synth
from oracle import fft_chain as offt

# ---- the far-field anchor ---------------------------------------------------------------------------------------------------------------
WAVELENGTH, FAR_BIN_M, CHIRP = 3.9e-3, 5.0, 1e-4                  # 5 m range bins put range bin 60 at 300 m
FAR_TARGETS = (dict(range_bin=60, az_bin=9, el_bin=1, doppler_bin=7, amp=400.0),
               dict(range_bin=50, az_bin=-11, el_bin=-2, doppler_bin=-5, amp=300.0),
               dict(range_bin=72, az_bin=5, el_bin=3, doppler_bin=-8, amp=500.0),
               dict(range_bin=44, az_bin=-20, el_bin=-1, doppler_bin=3, amp=250.0))


def _scatterer(t, wavelength, range_bin_m, chirp):
    """The scatterer whose far field is bin-domain target ``t``: range range_bin * range_bin_m, direction cosines dx = 2 az_bin / 64
    and dz = 2 el_bin / 8, radial speed doppler_bin / 64 * wavelength / (6 chirp), receding positive."""
    rng = t["range_bin"] * range_bin_m
    dx, dz = 2.0 * t["az_bin"] / 64.0, 2.0 * t["el_bin"] / 8.0
    u = np.array([dx, np.sqrt(1.0 - dx * dx - dz * dz), dz])
    speed = t["doppler_bin"] / 64.0 * wavelength / (6.0 * chirp)
    return rng * u, speed * u, t["amp"] * rng * rng, rng, speed


def _anchor(t, tx, rx):
    """-> (largest |model - f * scene| over the cube relative to the target's amplitude, |f|), f the common complex factor fitted by
    least squares."""
    p, v, a, _, _ = _scatterer(t, WAVELENGTH, FAR_BIN_M, CHIRP)
    model, _ = R.radar_scene_ref(p[None, None], v[None, None], [[a]], tx, rx, WAVELENGTH, FAR_BIN_M, CHIRP, physics=True)
    scene = synth.point_target_scene([t], tdm=True)
    f = np.vdot(scene, model[0]) / np.vdot(scene, scene)
    return np.abs(model[0] - f * scene).max() / t["amp"], abs(f)


def _anchor_tolerance(t):
    """Two terms, both phase errors in radians of what the bin-domain scene does not model.  Curvature: an element D off the origin
    sees the path D^2 / (2 R) longer than the plane wave says, D at most the virtual aperture 3.5 wavelengths (tx[2] + rx[3]), so
    2 pi D^2 / (2 R wavelength).  Range migration: over the burst of 191 chirp periods the path grows by 2 |speed| 191 T, which moves
    the beat frequency; at the last sample that is 2 pi 255 (path change) / (2 * 256 * range_bin_m)."""
    _, _, _, rng, speed = _scatterer(t, WAVELENGTH, FAR_BIN_M, CHIRP)
    D = 3.5 * WAVELENGTH
    curvature = 2 * np.pi * D * D / (2 * rng * WAVELENGTH)
    migration = 2 * np.pi * 255 * (2 * abs(speed) * 191 * CHIRP) / (2 * 256 * FAR_BIN_M)
    return curvature + migration


@pytest.mark.parametrize("t", FAR_TARGETS, ids=lambda t: "az%d_el%d_d%d" % (t["az_bin"], t["el_bin"], t["doppler_bin"]))
def test_far_field_is_the_bin_domain_scene(t):
    tx, rx = sim.iwr1843_array(WAVELENGTH)
    err, f = _anchor(t, tx, rx)
    tol = _anchor_tolerance(t)
    print("target %r: max difference %.4f of the amplitude, tolerance %.4f, |common factor| %.4f" % (t, err, tol, f))
    assert err <= tol                      # curvature + range migration, computed above from this target's geometry
    assert abs(f - 1.0) <= tol


def test_the_elevated_transmitter_on_the_wrong_side_loses_the_agreement():
    tx, rx = sim.iwr1843_array(WAVELENGTH)
    wrong = tx.copy()
    wrong[1, 2] = -wrong[1, 2]
    assert wrong[1, 2] > 0 > tx[1, 2]
    for t in FAR_TARGETS:
        err, f = _anchor(t, wrong, rx)
        print("target %r, tx[1] at +z: max difference %.3f of the amplitude, |common factor| %.3f" % (t, err, f))
        assert err > 10 * _anchor_tolerance(t) and f < 0.95
    mirrored = -rx                                                  # the receivers on the other side: azimuth flips
    assert _anchor(FAR_TARGETS[0], tx, mirrored)[0] > 10 * _anchor_tolerance(FAR_TARGETS[0])


def test_array_builder():
    tx, rx = sim.iwr1843_array(WAVELENGTH)
    h = WAVELENGTH / 2
    assert np.allclose(rx, [[-k * h, 0, 0] for k in range(4)], atol=0) and np.array_equal(tx[0], [0, 0, 0])
    assert np.array_equal(tx[2], [-4 * h, 0, 0]) and np.array_equal(tx[1], [-2 * h, 0, -h])
    vt, vr = sim.iwr1843_array(WAVELENGTH, sim.QUARTER_TURN, (0.0, 0.0, -0.1))
    assert np.allclose(vr, [[0, 0, -0.1 - k * h] for k in range(4)], atol=1e-18) and np.allclose(vt[1], [h, 0, -0.1 - 2 * h], atol=1e-18)
    assert abs(np.linalg.det(sim.QUARTER_TURN) - 1.0) < 1e-15
    m = sim.RadarModel()
    assert (m.wavelength, m.range_bin_m, m.chirp_period_s) == (3.9e-3, 0.0375, 1e-4)
    assert np.array_equal(m.array("hori")[0], tx) and np.array_equal(m.array("vert")[1], sim.iwr1843_array(WAVELENGTH, sim.QUARTER_TURN, sim.DEFAULT_VERT_ORIGIN)[1])
    for bad in (dict(wavelength=0.0), dict(range_bin_m=-1.0), dict(chirp_period_s=float("nan")), dict(frame_rate_hz=100.0)):
        with pytest.raises(ValueError):
            sim.RadarModel(**bad)
    with pytest.raises(ValueError):
        sim.iwr1843_array(WAVELENGTH, np.eye(2))


# ---- through the oracle chain -----------------------------------------------------------------------------------------------------------
def _human_range_cube(range_bin, az_bin, el_bin, doppler_bin, sensor="hori", amp=400.0):
    """One scatterer of the default model built from bins (range 2 to 3 m) -> (int16 (4, 192, 256, 2), position, velocity)."""
    m = sim.RadarModel()
    p, v, a, _, _ = _scatterer(dict(range_bin=range_bin, az_bin=az_bin, el_bin=el_bin, doppler_bin=doppler_bin, amp=amp),
                               m.wavelength, m.range_bin_m, m.chirp_period_s)
    tx, rx = m.array(sensor)
    z, _ = R.radar_scene_ref(p[None, None], v[None, None], [[a]], tx, rx, m.wavelength, m.range_bin_m, m.chirp_period_s)
    return R.quantise(z)[0], p, v


def test_a_moving_scatterer_peaks_in_the_predicted_cell_of_the_oracle_chain():
    """The reference's chain as it is (no TDM compensation) moves the azimuth peak by -d / 6 of a cell at Doppler bin d (two chirp
    periods between the two azimuth halves: 2 pi 2 d / 192 over four antennas), so the slow movers go through it and the faster ones
    through the compensated chain."""
    m = sim.RadarModel()
    # (range bin, azimuth bin, elevation bin, Doppler bin: receding positive), compensated, the predicted (range, azimuth) indices
    for bins, comp, cell in (((64, 6, 0, 1), False, (30, 25)), ((70, -10, 1, -2), False, (24, 41)),
                             ((64, 6, 0, 3), True, (30, 25)), ((70, -10, 1, -4), True, (24, 41))):
        iq, p, v = _human_range_cube(*bins)                             # 2.4 m and 2.6 m away, 0.1 to 0.4 m/s
        want = m.expected_cell("hori", p, v)
        assert np.allclose(want, cell + (bins[3],), atol=1e-9)
        heat = np.abs(tdm_ref.cube(synth.adc_cube_complex(iq), compensated=comp))
        if not comp:
            assert np.array_equal(heat, np.abs(offt.generate_heatmap(synth.adc_cube_complex(iq))))
        i, r, a, e = np.unravel_index(heat.argmax(), heat.shape)
        assert (i, r, a) == (bins[3] + 8,) + cell, (bins, comp)


@pytest.mark.parametrize("d", [7, -8])
def test_tdm_compensation_puts_a_fast_movers_azimuth_peak_on_the_predicted_cell(d):
    """The geometry of tests/test_tdm_cpu.py (range bin 60, azimuth bin 9: azimuth index 22) as a physical scatterer 2.25 m away."""
    iq, p, v = _human_range_cube(60, 9, 1, d)
    frame = synth.adc_cube_complex(iq)
    want_a = sim.RadarModel().expected_cell("hori", p, v)[1]
    assert abs(want_a - 22) < 1e-9
    peaks = {}
    for comp in (True, False):
        plane = np.abs(tdm_ref.cube(frame, compensated=comp)[d + 8])
        r, a, e = np.unravel_index(plane.argmax(), plane.shape)
        peaks[comp] = int(a)
    print("d = %d: azimuth peak %d with the compensation, %d without" % (d, peaks[True], peaks[False]))
    assert peaks[True] == 22
    assert abs(peaks[False] - 22) == 1


def test_the_statement_hides_what_the_header_says_it_hides():
    m = sim.RadarModel()
    tx, rx = m.array("hori")
    pos = np.array([[[0.3, 2.0, 0.1], [0.1, 2.5, 0.0], [np.nan, 2.0, 0.0], [0.0, 0.0, 0.0], [0.2, 2.2, 0.0], [0.2, 2.2, 0.0]]])
    vel = np.zeros_like(pos)
    vel[0, 4, 1] = np.inf
    amp = np.array([[100.0, 0.0, 100.0, 100.0, 100.0, np.nan]], dtype=np.float32)
    full, A = R.radar_scene_ref(pos, vel, amp, tx, rx, m.wavelength, m.range_bin_m, m.chirp_period_s)
    one, A1 = R.radar_scene_ref(pos[:, :1], vel[:, :1], amp[:, :1], tx, rx, m.wavelength, m.range_bin_m, m.chirp_period_s)
    # scatterer 3 sits on tx[0] = rx[0]: hidden from the chirps of transmitter 0 and from receiver 0, seen elsewhere
    assert np.array_equal(full[0, 0, 0::3], one[0, 0, 0::3]) and np.array_equal(full[0, 0], one[0, 0]) and np.isfinite(full).all()
    assert not np.array_equal(full[0, 1, 1::3], one[0, 1, 1::3]) and np.array_equal(A[0, 0], A1[0, 0])


# ---- host-side argument checks ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


@pytest.mark.parametrize("entry", ["hupr_radar_scene_i16", "hupr_radar_scene_f32"])
def test_argument_checks_return_before_any_launch(lib, entry):
    import ctypes
    fn = getattr(lib, entry)
    tx, rx = sim.iwr1843_array(3.9e-3)
    f64p = ctypes.POINTER(ctypes.c_double)
    ptx, prx = tx.ctypes.data_as(f64p), rx.ctypes.data_as(f64p)
    launches = lib.hupr_launch_count()
    good = (3.9e-3, 0.0375, 1e-4)
    assert fn(None, None, None, ptx, prx, 0, 1, *good, None, None, None) == 0             # frames == 0: a no-op
    fake = 4096                                                                         # never dereferenced: every call below is refused

    def refused(word, *args):
        assert fn(*args) == -1
        assert word in lib.hupr_last_error().decode(), lib.hupr_last_error()

    refused("null", None, None, None, ptx, prx, 1, 1, *good, None, None, None)
    refused("null", fake, fake, None, ptx, prx, 1, 1, *good, None, fake, None)
    refused("null", fake, fake, fake, ptx, prx, 1, 1, *good, None, None, None)
    refused("null", fake, fake, fake, None, prx, 1, 1, *good, None, fake, None)
    refused("null", fake, fake, fake, ptx, None, 0, 1, *good, None, fake, None)
    refused("frames", fake, fake, fake, ptx, prx, -1, 1, *good, None, fake, None)
    refused("S 0", fake, fake, fake, ptx, prx, 1, 0, *good, None, fake, None)
    refused("S 4097", fake, fake, fake, ptx, prx, 1, 4097, *good, None, fake, None)
    for k in range(3):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            s = list(good)
            s[k] = bad
            refused("positive and finite", fake, fake, fake, ptx, prx, 1, 1, *s, None, fake, None)
    nan_tx = tx.copy()
    nan_tx[2, 1] = np.nan
    refused("tx[2][1]", fake, fake, fake, nan_tx.ctypes.data_as(f64p), prx, 1, 1, *good, None, fake, None)
    inf_rx = rx.copy()
    inf_rx[3, 0] = np.inf
    refused("rx[3][0]", fake, fake, fake, ptx, inf_rx.ctypes.data_as(f64p), 1, 1, *good, None, fake, None)
    refused("aligned", fake + 4, fake, fake, ptx, prx, 1, 1, *good, None, fake, None)
    refused("aligned", fake, fake, fake, ptx, prx, 1, 1, *good, fake + 4, fake, None)
    refused("misaligned", fake, fake, fake + 2, ptx, prx, 1, 1, *good, None, fake, None)
    refused("misaligned", fake, fake, fake, ptx, prx, 1, 1, *good, None, fake + 2, None)
    assert lib.hupr_launch_count() == launches


def test_the_python_wrapper_refuses_before_it_touches_the_device(lib):
    import torch
    from hupr_amd import functional as F_, runtime
    tx, rx = sim.iwr1843_array(3.9e-3)
    pos, amp = torch.zeros((1, 2, 3), dtype=torch.float64), torch.ones((1, 2), dtype=torch.float32)
    args = (tx, rx, 3.9e-3, 0.0375, 1e-4)
    with pytest.raises(runtime.HuprError, match="no CPU fallback"):
        F_.radar_scene(pos, pos, amp, *args)
    for bad in ((pos.float(), pos, amp), (pos, pos[:, :1], amp), (pos, pos, amp.double()), (pos, pos, amp[:, :1]), (pos[0], pos[0], amp)):
        with pytest.raises(ValueError):
            F_.radar_scene(*bad, *args)
    with pytest.raises(ValueError):
        F_.radar_scene(pos, pos, amp, tx[:2], rx, 3.9e-3, 0.0375, 1e-4)
    with pytest.raises(ValueError):
        F_.radar_scene(pos, pos, amp, *args, add=torch.zeros((1, 4, 192, 256), dtype=torch.float32))
    with pytest.raises(ValueError):
        F_.radar_scene(pos, pos, amp, *args, out_dtype=torch.float16)


# ---- the body, the camera, the writer, the command -------------------------------------------------------------------------------------
def test_walking_body_keeps_every_bone_length_and_stays_in_range():
    from hupr_amd.datasets.base import SKELETON
    m = sim.RadarModel()
    for seed in (0, 1, 2):
        b = sim.walking_body(120, m.frame_rate_hz, seed)
        assert b.joints3d.shape == (120, 14, 3) and b.pos.shape == b.vel.shape == (120, sim.S_BODY, 3) and sim.S_BODY == 46
        assert b.amp.shape == (120, 46) and b.amp.dtype == np.float32 and np.array_equal(b.pos[:, :14], b.joints3d)
        for u, v in SKELETON:
            ln = np.linalg.norm(b.joints3d[:, u - 1] - b.joints3d[:, v - 1], axis=-1)
            assert ln.max() - ln.min() <= 1e-9 and 0.1 < ln.mean() < 0.7
        rng = np.linalg.norm(b.pos, axis=-1) / m.range_bin_m
        assert 31 < rng.min() and rng.max() < 94                                        # the range bins the chain keeps
        assert (b.amp[:, b.torso] > b.amp[:, :1]).all() and len(b.torso) == sim.TORSO_POINTS
        # the velocities are central differences of the positions over 2 ms: the same walk sampled at 1 kHz holds both neighbours
        fine = sim.walking_body(3, 1000.0, seed)
        assert np.array_equal(fine.pos[0], b.pos[0]) and np.abs(fine.vel[1] - (fine.pos[2] - fine.pos[0]) / 2e-3).max() <= 1e-9
        assert np.abs(b.vel).max() < 4.0
    a, c = sim.walking_body(4, 10.0, 5), sim.walking_body(4, 10.0, 6)
    assert np.array_equal(a.pos, sim.walking_body(4, 10.0, 5).pos) and not np.array_equal(a.pos, c.pos)
    assert not sim.walking_body(3, 10.0, 0).with_amp(0.0).amp.any()


def test_project_joints_keeps_the_labels_inside_the_image():
    for seed in range(4):
        uv = sim.project_joints(sim.walking_body(100, 10.0, seed).joints3d)
        assert uv.shape == (100, 14, 2) and uv.min() > 0.0 and uv.max() < 255.0          # strictly: nothing was clipped
        assert (uv[:, 7, 1] < uv[:, 6, 1]).all() and (uv[:, 2, 1] > uv[:, 0, 1]).all()   # the head above the neck, ankles below hips
        assert (uv[:, 8, 0] > uv[:, 11, 0]).all()                                        # the left shoulder on the image's right
    assert np.array_equal(sim.project_joints(np.array([[50.0, 1.0, 0.0], [0.1, 2.0, -50.0]])), [[255.0, 128.0], [128.0, 255.0]])
    with pytest.raises(ValueError):
        sim.project_joints(np.array([[0.0, -1.0, 0.0]]))


def _host_simulate(model, body, noise_std, seed):
    """The fp64 statement on three of the body's scatterers, for the writer's test (the device path is tests/test_simulate_dataset_gpu.py)."""
    keep = [6, 20, 44]
    return tuple(R.quantise(R.radar_scene_ref(body.pos[:, keep], body.vel[:, keep], body.amp[:, keep], *model.array(s), model.wavelength,
                                              model.range_bin_m, model.chirp_period_s)[0]) for s in ("hori", "vert"))


def test_written_tree_has_the_tiny_datasets_layout(tmp_path):
    dur = synth.TINY["duration"]
    tiny = synth.write_tiny_dataset(str(tmp_path / "tiny"), cubes=False, raw=True)
    got = sim.write_simulated_dataset(str(tmp_path / "sim"), {"train": synth.TINY["trainName"], "val": synth.TINY["valName"]}, dur, 3,
                                      simulate=_host_simulate)
    files = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    assert files(got) == files(tiny)
    for f in files(tiny):
        if f.endswith(".bin"):
            assert os.path.getsize(os.path.join(got, f)) == os.path.getsize(os.path.join(tiny, f)) == dur * 4 * 192 * 256 * 2 * 2
        else:
            a, b = json.load(open(os.path.join(got, f))), json.load(open(os.path.join(tiny, f)))
            assert len(a) == len(b) and all(len(x) == len(y) == dur for x, y in zip(a, b))
            for x, y in zip(a[0], b[0]):
                assert set(x) == set(y) and x["image"] == y["image"] and np.shape(x["joints"]) == (14, 2) and len(x["bbox"]) == 4
                assert all(isinstance(v, float) for v in x["bbox"]) and x["bbox"][0] < x["bbox"][2] and x["bbox"][1] < x["bbox"][3]
    # the capture decodes to the cube that went in
    seq = synth.TINY["valName"][0]
    s = sim.sequence_seed(3, seq)
    want = _host_simulate(sim.RadarModel(), sim.walking_body(dur, 10.0, s), 0.0, s)[1]
    raw = np.fromfile(os.path.join(got, "single_%d" % seq, "vert", "adc_data.bin"), dtype=np.int16)
    assert np.array_equal(raw, synth.dca1000_encode(want)) and want.any()
    assert sim.sequence_names(2) == {"train": [1, 2], "val": [3], "test": [3]}
    for bad in (0, True, {}, "3"):
        with pytest.raises(ValueError):
            sim.sequence_names(bad)


def test_the_command_parses_its_arguments():
    from hupr_amd.tools import simulate as cmd
    a = cmd.parse(["--out", "d", "--sequences", "2", "--frames", "600", "--seed", "4"])
    assert (a.out, a.sequences, a.frames, a.seed, a.noise, a.interference) == ("d", 2, 600, 4, 2.0, False)
    a = cmd.parse(["--out", "d", "--sequences", "1", "--frames", "6", "--seed", "0", "--noise", "0", "--interference"])
    assert a.noise == 0.0 and a.interference is True
    for argv in (["--sequences", "2", "--frames", "6", "--seed", "0"], ["--out", "d", "--sequences", "0", "--frames", "6", "--seed", "0"],
                 ["--out", "d", "--sequences", "1", "--frames", "0", "--seed", "0"],
                 ["--out", "d", "--sequences", "1", "--frames", "6", "--seed", "0", "--noise", "-1"],
                 ["--out", "d", "--sequences", "1", "--frames", "6"]):
        with pytest.raises(SystemExit):
            cmd.parse(argv)
