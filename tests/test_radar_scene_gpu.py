"""GPU (-m gpu): the radar scene kernel (csrc/radar_scene.hip) against its fp64 statement (tests/radar_scene_ref.py).  The cube's inner
shape is fixed by the layout; frames in {1, 2} and S in {1, 3, 65} (65 crosses a 64-scatterer chunk), and one S = 130 scene whose last
66 amplitudes are zero.  Amplitudes are scaled so that the largest per-row sum of received amplitudes A is about 2000: the int16
comparison needs the zone around the half-integers, (1e-6 + 6e-8 S) A wide, to hold under 5 % of the samples."""
import numpy as np
import pytest
import torch

import radar_scene_ref as R
from hupr_amd import simulate as sim
from hupr_amd import synth

pytestmark = pytest.mark.gpu
MODEL = sim.RadarModel()
TX, RX = MODEL.array("hori")
SCALARS = (MODEL.wavelength, MODEL.range_bin_m, MODEL.chirp_period_s)
CASES = [(f, s) for s in (1, 3, 65) for f in (1, 2)] + [(1, 130)]
A_TARGET = 2000.0


def _scene(frames, S):
    """Scatterers at human range, up to 1.5 m/s; S = 130: the last 66 hidden by a zero amplitude."""
    pos = np.stack([synth.uniform((frames, S), -1.0, 1.0, "rs_x", frames, S, dtype=np.float64),
                    synth.uniform((frames, S), 1.5, 3.3, "rs_y", frames, S, dtype=np.float64),
                    synth.uniform((frames, S), -1.0, 1.0, "rs_z", frames, S, dtype=np.float64)], -1)
    vel = synth.uniform((frames, S, 3), -1.5, 1.5, "rs_v", frames, S, dtype=np.float64)
    amp = synth.uniform((frames, S), 0.5, 1.5, "rs_a", frames, S, dtype=np.float32)
    if S == 130:
        amp[:, 64:] = 0.0
    _, _, A = R.scene_terms(pos, vel, amp, TX, RX, *SCALARS)
    amp = (amp * np.float32(A_TARGET / A.sum(axis=-1).max())).astype(np.float32)
    return pos, vel, amp


_cache = {}


def _case(frames, S):
    """-> (pos, vel, amp, the fp64 statement's cube, A); computed once per case and shared, never modified."""
    if (frames, S) not in _cache:
        pos, vel, amp = _scene(frames, S)
        ref, A = R.radar_scene_ref(pos, vel, amp, TX, RX, *SCALARS)
        _cache[(frames, S)] = (pos, vel, amp, ref, float(A.max()))
    return _cache[(frames, S)]


def _run(pos, vel, amp, tx=TX, rx=RX, **kw):
    from hupr_amd import functional as F_
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return F_.radar_scene(dev(pos), dev(vel), dev(amp), tx, rx, *SCALARS, **kw)


def _complex(t):
    x = t.cpu().numpy().astype(np.float64)
    return x[..., 0] + 1j * x[..., 1]


def _bound(S, A):
    """Each term is at most 6.2e-7 of its amplitude off (6e-8 turn of phase rounding, a 2-ulp sine and cosine); on top, the worst case
    of S fp32 additions."""
    return (1e-6 + 6e-8 * S) * A


@pytest.mark.parametrize("frames,S", CASES)
def test_fp32_sums_against_the_fp64_statement(frames, S):
    pos, vel, amp, ref, A = _case(frames, S)
    got = _run(pos, vel, amp, out_dtype=torch.float32)
    assert got.shape == (frames, 4, 192, 256, 2) and got.dtype == torch.float32
    d = _complex(got) - ref
    err = max(np.abs(d.real).max(), np.abs(d.imag).max())
    print("frames %d S %d: A %.1f, max |difference| %.3e = %.3e A, bound %.3e A" % (frames, S, A, err, err / A, _bound(S, A) / A))
    assert 0.9 * A_TARGET < A < 1.1 * A_TARGET
    assert err <= _bound(S, A)


@pytest.mark.parametrize("frames,S", CASES)
def test_int16_cube_is_the_rounded_statement(frames, S):
    pos, vel, amp, ref, A = _case(frames, S)
    got = _run(pos, vel, amp)
    assert got.shape == (frames, 4, 192, 256, 2) and got.dtype == torch.int16
    got = got.cpu().numpy().astype(np.int64)
    val = np.stack([ref.real, ref.imag], -1)
    want = np.rint(val).astype(np.int64)
    zone = np.abs(np.abs(val - np.floor(val)) - 0.5) <= _bound(S, A)           # within the bound of a half-integer
    share = zone.mean()
    flips = (got != want)
    print("frames %d S %d: %.2f %% of the samples in the zone, %d of %d differ" % (frames, S, 100 * share, flips.sum(), flips.size))
    assert share < 0.05                                                          # or the comparison below is vacuous
    assert np.array_equal(got[~zone], want[~zone])
    assert np.abs(got - want).max() <= 1
    assert np.abs(val).max() < 32000                                             # nothing here clips


def test_an_overflowing_amplitude_clips_at_both_rails():
    pos, vel, amp, _, _ = _case(1, 3)
    big = amp * np.float32(40.0)                                                 # A about 80 000
    ref, _ = R.radar_scene_ref(pos, vel, big, TX, RX, *SCALARS)
    got = _run(pos, vel, big).cpu().numpy()
    val = np.stack([ref.real, ref.imag], -1)
    assert (val > 40000).any() and (val < -40000).any()
    assert got.max() == 32767 and got.min() == -32768
    assert (got[val > 32768] == 32767).all() and (got[val < -32769] == -32768).all()
    inside = np.abs(val) < 32000
    assert np.abs(got[inside] - np.rint(val[inside])).max() <= 1


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_hidden_scatterers_leave_the_bits_of_the_cube_without_them(dtype):
    pos, vel, amp, _, _ = _case(2, 3)
    plain = _run(pos, vel, amp, out_dtype=dtype)
    # a zero amplitude at index 1, a NaN position at index 3, an infinite velocity at 5, a NaN amplitude at 6, among the three
    idx = [0, None, 1, None, 2, None, None]
    p5, v5, a5 = (np.stack([a[:, i] if i is not None else np.ones_like(a[:, 0]) for i in idx], 1) for a in (pos, vel, amp))
    a5[:, 1] = 0.0
    p5[:, 3, 2] = np.nan
    v5[:, 5, 0] = np.inf
    a5[:, 6] = np.nan
    assert torch.equal(_run(p5, v5, a5, out_dtype=dtype), plain)
    # hidden in one frame only
    a3 = amp.copy()
    a3[1, 2] = 0.0
    one = _run(pos, vel, a3, out_dtype=dtype)
    assert torch.equal(one[0], plain[0]) and not torch.equal(one[1], plain[1])
    assert torch.equal(one[1], _run(pos[1:, :2], vel[1:, :2], amp[1:, :2], out_dtype=dtype)[0])
    # a scatterer on an antenna is hidden from that antenna's rows and seen by the others
    p4 = np.concatenate([pos, np.broadcast_to(TX[1], (2, 1, 3))], 1)
    v4, a4 = np.concatenate([vel, np.zeros((2, 1, 3))], 1), np.concatenate([amp, np.full((2, 1), 1e-4, np.float32)], 1)
    on = _run(p4, v4, a4, out_dtype=dtype)
    assert torch.equal(on[:, :, 1::3], plain[:, :, 1::3]) and not torch.equal(on[:, :, 0::3], plain[:, :, 0::3])
    assert bool(torch.isfinite(on.float()).all())


def test_add_is_honoured():
    pos, vel, amp, _, _ = _case(2, 3)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    add = torch.randn((2, 4, 192, 256, 2), generator=gen, device="cuda") * 300.0
    plain = _run(pos, vel, amp, out_dtype=torch.float32)
    got = _run(pos, vel, amp, add=add, out_dtype=torch.float32)
    want = plain.double() + add.double()
    ulp = torch.from_numpy(np.spacing(np.abs(want.cpu().numpy()).astype(np.float32))).cuda().double()
    assert bool(((got.double() - want).abs() <= ulp).all())                      # 1 ulp of the sum
    # the int16 entry rounds the same sums
    q = _run(pos, vel, amp, add=add)
    assert torch.equal(q, torch.clamp(torch.round(got), -32768, 32767).to(torch.int16))
    assert not torch.equal(q, _run(pos, vel, amp))


def test_two_runs_are_bit_equal():
    pos, vel, amp, _, _ = _case(2, 65)
    for dtype in (torch.int16, torch.float32):
        assert torch.equal(_run(pos, vel, amp, out_dtype=dtype), _run(pos, vel, amp, out_dtype=dtype))


def test_no_frames_is_a_no_op_and_a_frame_does_not_depend_on_its_neighbours():
    from hupr_amd import runtime
    pos, vel, amp, _, _ = _case(2, 65)
    n = runtime.lib().hupr_launch_count()
    for dtype in (torch.int16, torch.float32):
        empty = _run(pos[:0], vel[:0], amp[:0], out_dtype=dtype)
        assert empty.shape == (0, 4, 192, 256, 2) and empty.dtype == dtype
    assert runtime.lib().hupr_launch_count() == n
    both = _run(pos, vel, amp)
    assert runtime.lib().hupr_launch_count() == n + 1                            # one launch per call
    for f in (0, 1):
        assert torch.equal(_run(pos[f:f + 1], vel[f:f + 1], amp[f:f + 1])[0], both[f])


def test_the_device_chain_finds_the_walkers_torso_in_both_sensors():
    """Frames 14 and 38 of ``walking_body(40, 10 Hz, seed 0)``: the torso recedes at Doppler bin 3.1 and approaches at -3.1.  In the
    Doppler plane of the torso's predicted bin, summed over elevation, the strongest (range, azimuth) cell of the device FFT chain
    lies within one cell of the torso's predicted cell, in both sensors.  (Point scatterers a few wavelengths apart add with random
    phases, so the peak of a frame can sit on another part of the trunk: through the fp64 oracle chain about one frame in ten of
    this walker does; these two do not.)"""
    from hupr_amd import preprocessing
    body = sim.walking_body(40, MODEL.frame_rate_hz, 0)
    pick = [14, 38]
    part = sim.Body(body.joints3d[pick], body.pos[pick], body.vel[pick], body.amp[pick], body.torso, body.rate_hz)
    cubes = sim.simulate_sequence(MODEL, part, noise_std=2.0, seed=1)
    for sensor, cube in zip(("hori", "vert"), cubes):
        assert cube.shape == (2, 4, 192, 256, 2) and cube.dtype == torch.int16 and cube.is_cuda
        heat = preprocessing.fft_chain(cube).abs().cpu().numpy().astype(np.float64) ** 2          # (2, 16, 64, 64, 8)
        for k in range(2):
            c, v = part.pos[k, part.torso].mean(0), part.vel[k, part.torso].mean(0)
            want_r, want_a, want_d = MODEL.expected_cell(sensor, c, v)
            assert abs(want_d - round(want_d)) < 0.2 and 2 <= abs(want_d) <= 7
            plane = heat[k, int(round(want_d)) + 8].sum(axis=-1)
            r, a = np.unravel_index(plane.argmax(), plane.shape)
            print("%s frame %d: peak (%d, %d), predicted (%.2f, %.2f) at Doppler bin %.2f" % (sensor, pick[k], r, a, want_r, want_a, want_d))
            assert abs(r - round(want_r)) <= 1 and abs(a - round(want_a)) <= 1
