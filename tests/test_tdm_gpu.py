"""GPU (-m gpu): the Doppler phase compensation for the TDM-MIMO virtual array (hupr_fft_chain_tdm, csrc/fft_chain.hip) against its
fp64 statement (tests/tdm_ref.py), its bit-level promises (the zero-Doppler index, the table forms, modes 1 and 3), and the layers
above it: TrainEngine with ``DATASET.tdmCompensation``, the mirror, the flip test, and one PoseStream session.

The numeric yardstick is measured here: e0 = the rel-L2 error of the unchanged, uncompensated call against the oracle on the same
inputs; the compensated call must stay within 2 e0 of its own oracle (one more fp32 rounding on top of the chain's own)."""
import os

import numpy as np
import pytest
import torch

import tdm_ref
from hupr_amd import synth
from hupr_amd.tools import augment as aug

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = 8
N_SF, FRAMES_PER_FLAG, FLAGS = 4, 2, (1, 0)
TARGET = dict(range_bin=60, az_bin=9, el_bin=1, amp=400.0)


def _dev():
    return torch.device("cuda", 0)


def _pre():
    from hupr_amd.preprocessing import process_iwr1843 as pre
    return pre


def _rt():
    from hupr_amd import runtime as rt
    return rt


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def frames():
    """Four sensor-frames — the physical point target at d = 7, a random cube, the physical point target at d = -5, a random cube — on
    the host and the device, and the swap flags [1, 0] (two frames per flag: the first target and the first random cube are swapped).
    The targets sit in receiver noise: the int16 rounding of a noise-free exponential is periodic, which leaves whole Doppler planes
    of its cube empty, and Normalize of an empty plane is 0 / 0 in the oracle and amplified rounding in the chain."""
    host = np.concatenate([synth.point_target_cube([dict(TARGET, doppler_bin=7)], noise=30.0, seed=1, tdm=True), synth.adc_cube_int16(41),
                           synth.point_target_cube([dict(TARGET, doppler_bin=-5)], noise=30.0, seed=2, tdm=True), synth.adc_cube_int16(42)])
    assert host.shape[0] == N_SF
    return host, torch.from_numpy(host).to(_dev()), torch.tensor(FLAGS, dtype=torch.uint8, device=_dev())


_REF = {}


def _reference(host, window, zero_doppler, compensated):
    """The fp64 cubes of the four frames (computed once per form, never modified): (4, 16, 64, 64, 8) complex128."""
    key = (window, zero_doppler, compensated)
    if key not in _REF:
        _REF[key] = np.stack([tdm_ref.cube_iq(host[n], compensated=compensated, swapped=bool(FLAGS[n // FRAMES_PER_FLAG]), window=window,
                                              zero_doppler=zero_doppler) for n in range(N_SF)])
        _REF[key].setflags(write=False)
    return _REF[key]


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=ref.dtype), np.asarray(ref)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


# name -> (python keywords of the chain, loader form, oracle window, oracle zero-Doppler form)
CASES = {
    "cube": (dict(), 0, 0, "dither"),
    "loader": (dict(), 1, 0, "dither"),
    "means": (dict(), 2, 0, "dither"),
    "hann": (dict(window="hann"), 0, 3, None),
    "zero_doppler_exact": (dict(zero_doppler="exact"), 0, 0, "exact"),
    "range_first": (dict(zero_doppler="range_first"), 0, 0, None),
    "magnitude": (dict(magnitude=True), 0, 0, "dither"),
}


def _call(pre, dev, loader, kw, **tdm):
    if loader == 0:
        return pre.fft_chain(dev, **kw, **tdm)
    if loader == 1:
        return pre.fft_chain_loader(dev, **kw, **tdm)
    return pre.fft_chain_loader_means(dev, **kw, **tdm)


def _oracle_form(c, loader, magnitude):
    """fp64 cubes (4, 16, 64, 64, 8) -> the form the call returns, the zero-Doppler index (8; loader slot f = 4) left out."""
    if loader == 0:
        keep = np.arange(16) != 8
        return np.abs(c[:, keep]) if magnitude else c[:, keep]
    ld = np.stack([tdm_ref.loader(x) for x in c])                        # (4, 8, 2, 64, 64, 8)
    keep = np.arange(8) != 4
    if loader == 1:
        return ld[:, keep]
    return np.stack([tdm_ref.means(x) for x in ld]).reshape(N_SF, 8, 2, 64, 64)[:, keep]


def _got_form(t, loader):
    a = t.cpu().numpy()
    if loader == 0:
        return a[:, np.arange(16) != 8]
    if loader == 1:
        return a[:, np.arange(8) != 4]
    return a.reshape(N_SF, 8, 2, 64, 64)[:, np.arange(8) != 4]


@pytest.mark.parametrize("name", list(CASES))
def test_compensated_call_against_the_fp64_rule(frames, name):
    """Measured on an MI355X ("Doppler phase compensation"): e0 and the compensated call's error per form."""
    host, dev, flags = frames
    pre = _pre()
    kw, loader, window, zd = CASES[name]
    magnitude = bool(kw.get("magnitude"))
    plain = _call(pre, dev, loader, kw)
    comp = _call(pre, dev, loader, kw, tdm_compensation=True, tx_swapped=flags, frames_per_flag=FRAMES_PER_FLAG)
    assert comp.shape == plain.shape and comp.dtype == plain.dtype
    e0 = _rel(_got_form(plain, loader), _oracle_form(_reference(host, window, zd, False), loader, magnitude))
    e1 = _rel(_got_form(comp, loader), _oracle_form(_reference(host, window, zd, True), loader, magnitude))
    # the compensation is not a no-op: against the OTHER oracle the call is far off
    cross = _rel(_got_form(comp, loader), _oracle_form(_reference(host, window, zd, False), loader, magnitude))
    print("%s: uncompensated call vs oracle e0 = %.3e, compensated call vs its oracle %.3e (%.2f e0); vs the uncompensated oracle %.3e"
          % (name, e0, e1, e1 / e0, cross))
    assert np.isfinite(comp.cpu().numpy().view(np.float32)).all()
    assert e0 <= 1e-4                          # the yardstick itself is the chain's known error
    assert e1 <= 2.0 * e0
    assert cross >= 1e-2
    # Doppler index 8 (loader slot f = 4) is the uncompensated call's, bit for bit
    zero = {0: lambda t: t[:, 8], 1: lambda t: t[:, 4], 2: lambda t: t[:, 8:10]}[loader]
    assert torch.equal(_bits(zero(comp)), _bits(zero(plain)))
    assert not torch.equal(_bits(comp), _bits(plain))


def _raw(dev, loader, table, n_swapped, frames_per_flag, flags=0):
    """hupr_fft_chain_tdm as the C ABI takes it -> (return code, output)."""
    rt, pre = _rt(), _pre()
    n = dev.shape[0]
    shape = {0: (n, 16, 64, 64, 8), 1: (n, 8, 2, 64, 64, 8), 2: (n, 16, 64, 64)}[loader]
    out = torch.zeros(shape, dtype=torch.complex64 if loader == 0 else torch.float32, device=dev.device)
    ws, nbytes = pre._workspace(n, dev.device)
    rc = rt.lib().hupr_fft_chain_tdm(rt.ptr(dev), n, rt.ptr(out), flags, loader, rt.ptr(table), n_swapped, frames_per_flag, rt.ptr(ws),
                                     nbytes, rt.stream())
    return rc, out


@pytest.mark.parametrize("loader", [0, 1, 2])
def test_table_forms_that_mean_the_same_give_the_same_bits(frames, loader):
    _, dev, flags = frames
    zeros = torch.zeros(2, dtype=torch.uint8, device=_dev())
    rc, null = _raw(dev, loader, None, 0, 1)
    assert rc == 0
    for what, (table, n_swapped, fpf) in {"zeros": (zeros, 2, 2), "zeros, one flag per frame": (torch.zeros(4, dtype=torch.uint8, device=_dev()), 4, 1),
                                          "null with a count": (None, 3, 2), "null, frames_per_flag = 7": (None, 0, 7)}.items():
        rc, out = _raw(dev, loader, table, n_swapped, fpf)
        assert rc == 0 and torch.equal(_bits(out), _bits(null)), what
    # rows past n_swapped are not swapped: [1] with n_swapped = 1 is [1, 0]
    rc, full = _raw(dev, loader, flags, 2, FRAMES_PER_FLAG)
    rc2, short = _raw(dev, loader, flags, 1, FRAMES_PER_FLAG)
    assert rc == 0 and rc2 == 0 and torch.equal(_bits(full), _bits(short))
    assert not torch.equal(_bits(full), _bits(null))
    assert torch.equal(_bits(full[2:]), _bits(null[2:]))                             # the unswapped frames are the null table's
    # any non-zero byte is a flag
    rc, other = _raw(dev, loader, torch.tensor([200, 0], dtype=torch.uint8, device=_dev()), 2, FRAMES_PER_FLAG)
    assert rc == 0 and torch.equal(_bits(other), _bits(full))
    # the Python entry is the same call
    py = _call(_pre(), dev, loader, {}, tdm_compensation=True, tx_swapped=flags, frames_per_flag=FRAMES_PER_FLAG)
    assert torch.equal(_bits(py), _bits(full))


def test_means_are_the_elevation_mean_of_the_loader_tensor_bit_for_bit(frames):
    _, dev, flags = frames
    pre = _pre()
    kw = dict(tdm_compensation=True, tx_swapped=flags, frames_per_flag=FRAMES_PER_FLAG)
    n = pre.fft_chain_loader(dev, **kw)                                               # (4, 8, 2, 64, 64, 8)
    m = pre.fft_chain_loader_means(dev, **kw)                                         # (4, 16, 64, 64)
    e = [n[..., k] for k in range(8)]
    want = ((((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]))) * 0.125).reshape(N_SF, 16, 64, 64)
    assert torch.equal(_bits(m), _bits(want))


def test_three_launches_give_the_same_bits(frames):
    _, dev, flags = frames
    pre = _pre()
    kw = dict(tdm_compensation=True, tx_swapped=flags, frames_per_flag=FRAMES_PER_FLAG)
    for fn in (pre.fft_chain, pre.fft_chain_loader, pre.fft_chain_loader_means):
        a, b, c = fn(dev, **kw), fn(dev, **kw), fn(dev, **kw)
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c)), fn.__name__


def test_argument_errors_return_minus_one_and_launch_nothing(frames):
    _, dev, flags = frames
    rt = _rt()
    L = rt.lib()
    out = torch.zeros((N_SF, 16, 64, 64, 8), dtype=torch.complex64, device=_dev())     # large enough for every form
    big, nbytes = _pre()._workspace(N_SF, _dev())
    torch.cuda.synchronize()
    n0 = L.hupr_launch_count()
    for what, (table, n_swapped, fpf, loader, fl) in {"frames_per_flag = 0": (flags, 2, 0, 0, 0), "frames_per_flag < 0": (None, 0, -1, 0, 0),
                                                       "n_swapped < 0": (flags, -1, 2, 0, 0), "a table with n_swapped = 0": (flags, 0, 2, 0, 0),
                                                       "loader = 3": (None, 0, 1, 3, 0), "loader = -1": (None, 0, 1, -1, 0),
                                                       "unknown flag": (None, 0, 1, 0, 64), "loader + magnitude": (None, 0, 1, 1, 4),
                                                       "exact + range-first": (None, 0, 1, 0, 24)}.items():
        rc = L.hupr_fft_chain_tdm(rt.ptr(dev), N_SF, rt.ptr(out), fl, loader, rt.ptr(table), n_swapped, fpf, rt.ptr(big), nbytes, rt.stream())
        assert rc == -1 and L.hupr_last_error(), what
    assert L.hupr_launch_count() == n0
    assert not out.cpu().numpy().view(np.float32).any()
    assert L.hupr_fft_chain_tdm(None, 1, None, 0, 0, None, 0, 1, None, 0, None) == -1 and b"null" in L.hupr_last_error()
    assert L.hupr_fft_chain_tdm(None, 0, None, 0, 0, None, 0, 1, None, 0, None) == 0           # the empty batch is a no-op, as in _opts
    ws = torch.empty(16, dtype=torch.uint8, device=_dev())
    assert L.hupr_fft_chain_tdm(rt.ptr(dev), N_SF, rt.ptr(out), 0, 0, None, 0, 1, rt.ptr(ws), 16, None) == -2     # workspace too small
    assert L.hupr_launch_count() == n0
    # the Python entry refuses what it can see
    pre = _pre()
    with pytest.raises(ValueError, match="frames_per_flag"):
        pre.fft_chain(dev, tdm_compensation=True, tx_swapped=flags, frames_per_flag=0)
    with pytest.raises(ValueError, match="tx_swapped"):
        pre.fft_chain(dev, tdm_compensation=True, tx_swapped=flags, frames_per_flag=1)          # two flags for four frames
    with pytest.raises(ValueError, match="tx_swapped"):
        pre.fft_chain(dev, tx_swapped=flags, frames_per_flag=2)                                 # flags without the compensation
    assert L.hupr_launch_count() == n0


def test_physical_target_peaks_at_azimuth_22_once_compensated():
    pre = _pre()
    dev = torch.from_numpy(synth.point_target_cube([dict(TARGET, doppler_bin=7)], tdm=True)).to(_dev())

    def peak(out):
        m = out[0].abs().cpu().numpy()
        return tuple(int(x) for x in np.unravel_index(m.argmax(), m.shape))
    plain, comp = peak(pre.fft_chain(dev)), peak(pre.fft_chain(dev, tdm_compensation=True))
    print("physical target at d = 7: arg-max (doppler, range, azimuth, elevation) %r today, %r compensated" % (plain, comp))
    assert comp[:3] == (15, 34, 22)
    assert plain[:2] == (15, 34) and plain[2] == 21                                   # today's chain: one bin off (tests/test_tdm_cpu.py)
    obj = pre.RadarObject(device="cuda")
    frame = synth.adc_cube_complex(dev.cpu().numpy())[0]
    assert np.array_equal(obj.generateHeatmap(frame, tdm_compensation=True), pre.fft_chain(dev, tdm_compensation=True)[0].cpu().numpy().astype(np.complex128))
    assert np.array_equal(obj.generateHeatmap(frame), pre.fft_chain(dev)[0].cpu().numpy().astype(np.complex128))


# ---- the engine (B = 2, the model of tests/test_augment_gpu.py) ----------------------------------------------------------------------
def _cfg(tdm=None, **training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    if tdm is not None:
        cfg.DATASET.tdmCompensation = tdm
    return cfg


@pytest.fixture(scope="module")
def batch():
    B = 2
    host_h = synth.adc_cube_int16(31, sensor=0, nframes=B * G)
    return (torch.from_numpy(host_h).to(_dev()), torch.from_numpy(aug.mirror_adc_host(host_h)).to(_dev()),
            torch.from_numpy(synth.adc_cube_int16(31, sensor=1, nframes=B * G)).to(_dev()), torch.from_numpy(synth.keypoints(B, 32)).to(_dev()))


@pytest.fixture()
def bf16():
    from hupr_amd import functional as F_
    F_.set_math("bf16")
    yield F_
    F_.set_math("f32")


def _count(fn):
    L = _rt().lib()
    torch.cuda.synchronize()
    n0 = L.hupr_launch_count()
    out = fn()
    return L.hupr_launch_count() - n0, out


def test_engine_honours_the_key_and_leaves_todays_path_alone(batch, bf16):
    from hupr_amd.tools.engine import TrainEngine
    pre = _pre()
    adc_h, adc_hm, adc_v, joints = batch
    B = 2
    off = TrainEngine(_cfg(), device=_dev(), seed=0)
    assert off.tdm is False
    n_off, (h0, v0) = _count(lambda: off.preprocess(adc_h, adc_v))
    assert n_off == 4                                                                  # two chains of two kernels, as ever
    assert torch.equal(_bits(h0), _bits(pre.fft_chain_loader_means(adc_h).view(B, G, 16, 64, 64)))
    assert torch.equal(_bits(v0), _bits(pre.fft_chain_loader_means(adc_v).view(B, G, 16, 64, 64)))
    off.close()
    with pytest.raises(ValueError, match="DATASET.tdmCompensation"):
        TrainEngine(_cfg(tdm=1), device=_dev(), seed=0)

    on = TrainEngine(_cfg(tdm=True, augMirror=1.0), device=_dev(), seed=0)
    assert on.tdm is True
    n_on, (h1, v1) = _count(lambda: on.preprocess(adc_h, adc_v))
    assert n_on == 4
    assert torch.equal(_bits(h1), _bits(pre.fft_chain_loader_means(adc_h, tdm_compensation=True).view(B, G, 16, 64, 64)))
    assert torch.equal(_bits(v1), _bits(pre.fft_chain_loader_means(adc_v, tdm_compensation=True).view(B, G, 16, 64, 64)))
    assert not torch.equal(h1, h0)
    # augMirror 1.0: the chain on the permuted cube with every flag set; the vertical cube is never swapped
    ones = torch.ones(B, dtype=torch.uint8, device=_dev())
    hm, vm, jm = on._augmented_from_adc(adc_h, adc_v, joints)
    want = pre.fft_chain_loader_means(adc_hm, tdm_compensation=True, tx_swapped=ones, frames_per_flag=G).view(B, G, 16, 64, 64)
    assert torch.equal(_bits(hm), _bits(want)) and torch.equal(_bits(vm), _bits(v1))
    assert not torch.equal(hm, pre.fft_chain_loader_means(adc_hm, tdm_compensation=True).view(B, G, 16, 64, 64))
    assert torch.equal(jm, aug.mirror_joints_host(joints, on.augment.pairs, 252))
    # the reference-shaped hand-over takes the same route
    on.fuse_elevation_mean = False
    h7, v7 = on.preprocess(adc_h, adc_v, hori_swapped=ones)
    assert torch.equal(_bits(h7), _bits(pre.fft_chain_loader(adc_h, tdm_compensation=True, tx_swapped=ones, frames_per_flag=G).view(B, G, 8, 2, 64, 64, 8)))
    assert torch.equal(_bits(v7), _bits(pre.fft_chain_loader(adc_v, tdm_compensation=True).view(B, G, 8, 2, 64, 64, 8)))
    on.fuse_elevation_mean = True
    # the flip test's second pass marks every frame swapped
    plain = on.infer_from_adc(adc_h, adc_v)
    second = on.infer(*on.preprocess(adc_hm, adc_v, hori_swapped=ones))
    flipped = on.infer_from_adc(adc_h, adc_v, flip=True)
    pairs = aug.mirror_pairs(on.cfg.DATASET.idxToJoints)
    for k in range(2):
        assert torch.equal(_bits(flipped[k]), _bits(aug.flip_merge(plain[k], second[k], pairs)))
    on.close()


def test_sequence_cache_follows_the_key(batch):
    from hupr_amd.datasets.dataset import SequenceFFTCache
    pre = _pre()
    adc_h, _, adc_v, _ = batch
    on, off = SequenceFFTCache(adc_h[:4], adc_v[:4], G, tdm_compensation=True), SequenceFFTCache(adc_h[:4], adc_v[:4], G)
    assert torch.equal(_bits(on.hori), _bits(pre.fft_chain_loader(adc_h[:4], tdm_compensation=True)))
    assert torch.equal(_bits(on.vert), _bits(pre.fft_chain_loader(adc_v[:4], tdm_compensation=True)))
    assert torch.equal(_bits(off.hori), _bits(pre.fft_chain_loader(adc_h[:4]))) and not torch.equal(on.hori, off.hori)


def test_one_stream_session_with_the_option_equals_the_offline_route(bf16):
    """Pushes 0 .. 3 of a zero-lookahead session (two eager emits, the capture, one replay) against engine.preprocess + engine.infer
    with the key on, on the windows the session sees; and the session without the option is today's."""
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseStream
    from hupr_amd.tools.engine import TrainEngine
    from hupr_amd.tools.stream import stream_window_sources
    g = np.load(os.path.join(GOLD, "model_eval.npz"))
    cfg = _cfg(tdm=True)
    engine = TrainEngine(cfg, device=_dev(), seed=0)
    engine.model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.hupr_state(int(g["model_seed"]), gain=float(g["gain"])).items()})
    engine.model.eval()
    engine.model.math_mode = "bf16"
    seq = [torch.from_numpy(np.concatenate([synth.adc_cube_int16(5, seq=0, frame=f, sensor=s) for f in range(4)])).to(_dev()) for s in range(2)]

    def offline(eng, c):
        idx = torch.tensor(stream_window_sources(c, c, G), device=_dev())
        p1, p2 = eng.infer(*eng.preprocess(seq[0].index_select(0, idx), seq[1].index_select(0, idx)))
        am, mx = F_.argmax_rows(p2.reshape(-1, 64 * 64))
        return p1, p2, am.view(1, -1), mx.view(1, -1)

    s = PoseStream(engine.model, cfg, lanes=1, lookahead=0, tdm_compensation=True)
    for c in range(4):
        pf = s.push(seq[0][c:c + 1], seq[1][c:c + 1])
        p1, p2, am, mx = offline(engine, c)
        assert pf.frame == c and torch.equal(pf.heatmap, p1) and torch.equal(pf.gcn_heatmap, p2), c
        assert torch.equal(pf.indices, am) and torch.equal(pf.scores, mx), c
    assert s._graphs                                                                   # the last push was a graph replay
    # without the option: today's chain, which the key-on offline route does not reproduce
    engine.tdm = False
    s0 = PoseStream(engine.model, cfg, lanes=1, lookahead=0)
    pf = s0.push(seq[0][0:1], seq[1][0:1])
    p1, p2, _, _ = offline(engine, 0)
    assert torch.equal(pf.heatmap, p1) and torch.equal(pf.gcn_heatmap, p2)
    engine.tdm = True
    q1, _, _, _ = offline(engine, 0)
    assert not torch.equal(q1, p1)
    with pytest.raises(Exception, match="tdm_compensation"):
        PoseStream(engine.model, cfg, tdm_compensation=1)
    engine.close()
