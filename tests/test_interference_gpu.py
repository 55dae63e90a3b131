"""GPU (-m gpu): interference blanking of the raw ADC cube (csrc/interference.hip) against the numpy statement of its rule
(tests/interference_ref.py) with torch.equal — output cube, bit mask, group counts and summed counts, no tolerances — and the layers
above it: the FFT chain's ``interference=``, the live stream and the training engine, each against the same path fed the
reference-filtered cubes."""
import functools

import numpy as np
import pytest
import torch

import interference_ref as R
from hupr_amd import synth

pytestmark = pytest.mark.gpu

SETTINGS = [(32, 2, "clutter"), (32, 2, "zero"), (2, 0, "clutter"), (1024, 8, "zero"), (2, 8, "clutter")]


def _dev():
    return torch.device("cuda", 0)


def _rt():
    from hupr_amd import runtime as rt
    return rt


def _F():
    from hupr_amd import functional as F_
    return F_


def _bits(t):
    return t.contiguous().view(torch.int32)


def _edge_cubes():
    """Three sensor-frames of placement and range edge cases on the clean scene (seeds 1..3)."""
    cube = np.concatenate([R.clean_scene(s) for s in (1, 2, 3)])
    ph = np.exp(2j * np.pi * synth.uniform01(256, "edge_phase"))
    # frame 0: bursts touching samples 0 and 255 (the guard is clipped there, and never enters the next chirp)
    for chirp, sl in ((10, slice(0, 6)), (100, slice(250, 256)), (101, slice(0, 1)), (191, slice(255, 256))):
        z = 9000.0 * ph[sl]
        cube[0, :, chirp, sl, 0] += np.rint(z.real).astype(np.int16)
        cube[0, :, chirp, sl, 1] += np.rint(z.imag).astype(np.int16)
    # frame 1: sample 77 of group (rx 1, tx 2) hit in all 64 loops with alternating sign (the same value in every loop would be
    # clutter): with a guard no loop is left at 75..79 and the clutter fill is 0; chirp 50 of rx 2 with 161 of its 256 samples hit
    sign = np.where(np.arange(64) % 2 == 0, 1, -1).astype(np.int16)
    cube[1, 1, 2::3, 77, 0] = 20000 * sign
    cube[1, 1, 2::3, 77, 1] = -15000 * sign
    z = 8000.0 * ph[40:201]
    cube[1, 2, 50, 40:201, 0] += np.rint(z.real).astype(np.int16)
    cube[1, 2, 50, 40:201, 1] += np.rint(z.imag).astype(np.int16)
    # frame 2: the ends of the int16 range, single samples and a whole column of a group
    cube[2, 0, 7, 100] = (-32768, 32767)
    cube[2, 0, 7, 101] = (32767, -32768)
    cube[2, 3, 0::3, 200, 0] = np.where(np.arange(64) % 2 == 0, 32767, -32768).astype(np.int16)
    cube[2, 3, 0::3, 200, 1] = np.where(np.arange(64) % 2 == 0, -32768, 32767).astype(np.int16)
    cube[2, 3, 1::3, 13] = (-32768, -32768)                      # the same extreme in every loop but one: the largest residual
    cube[2, 3, 4, 13] = (32767, 32767)
    return cube


@functools.lru_cache(maxsize=None)
def _host(name):
    if name == "burst":
        return R.burst_scene(0)[0]
    if name == "clean_zero":
        return np.concatenate([R.clean_scene(0), np.zeros((1, 4, 192, 256, 2), dtype=np.int16)])
    return _edge_cubes()


@functools.lru_cache(maxsize=None)
def _device(name):
    return torch.from_numpy(_host(name)).to(_dev())


@functools.lru_cache(maxsize=None)
def _ref(name, K, guard, fill):
    return R.interference_ref(_host(name), K, guard, fill)


def _assert_equals_ref(got, ref):
    cube, stats, mask = got
    dev = cube.device
    assert cube.dtype == torch.int16 and stats.frames.dtype == torch.int32 and stats.groups.dtype == torch.int32
    assert torch.equal(cube, torch.from_numpy(ref["cube"]).to(dev))
    assert torch.equal(stats.groups, torch.from_numpy(ref["groups"]).to(dev))
    assert torch.equal(stats.frames, torch.from_numpy(ref["frames"]).to(dev))
    if mask is not None:
        assert mask.dtype == torch.uint8 and torch.equal(mask, torch.from_numpy(ref["mask"]).to(dev))


@pytest.mark.parametrize("K,guard,fill", SETTINGS)
@pytest.mark.parametrize("name", ["burst", "clean_zero", "edges"])
def test_cube_mask_and_counts_equal_the_rule(name, K, guard, fill):
    adc, keep = _device(name), _device(name).clone()
    ref = _ref(name, K, guard, fill)
    got = _F().adc_interference(adc, K, guard, fill, want_mask=True)
    _assert_equals_ref(got, ref)
    assert got[0].data_ptr() != adc.data_ptr() and torch.equal(adc, keep)          # out of place: the source is unchanged
    print("%s K=%d guard=%d %s: frames %s" % (name, K, guard, fill, ref["frames"].tolist()))


def test_the_known_answers():
    """The burst scene: every injected sample is flagged, the extras are the guard; a clean scene passes bit for bit; an all-zero
    cube has no flag; the edge cases do what they were built for (so the comparisons above cover them)."""
    _, _, injected = R.burst_scene(0)
    ref = _ref("burst", 32, 2, "clutter")
    assert not (injected & ~ref["flags"]).any() and not (ref["flags"] & ~R.dilate(injected, 2)).any()
    cube, stats, mask = _F().adc_interference(_device("clean_zero"), 32, 2, "clutter", want_mask=True)
    assert torch.equal(cube, _device("clean_zero")) and int(stats.frames.sum()) == 0 and int(mask.sum()) == 0
    e = _ref("edges", 32, 2, "clutter")
    f = e["flags"]
    assert f[0, :, 10, :8].all() and not f[0, :, 10, 8:].any() and not f[0, :, 11].any()            # clipped at 0, no wrap
    assert f[0, :, 100, 248:].all() and f[0, :, 101, :3].all() and not f[0, :, 101, 3:].any() and f[0, :, 191, 253:].all()
    assert f[1, 1, 2::3, 75:80].all() and (e["cube"][1, 1, 2::3, 75:80] == 0).all()                 # no loop left: fill 0
    assert not f[1, 2, 50].any()                                   # more than half the chirp hit: the median is the burst's own
    assert f[2, 0, 7, 100] and f[2, 0, 7, 101] and f[2, 3, 0::3, 200].all() and f[2, 3, 4, 13]


def test_in_place_and_without_mask():
    F_ = _F()
    for name in ("burst", "edges"):
        ref = _ref(name, 32, 2, "clutter")
        buf = _device(name).clone()
        cube, stats, mask = F_.adc_interference(buf, 32, 2, "clutter", out=buf)      # the mask pointer is null
        assert mask is None and cube.data_ptr() == buf.data_ptr()
        _assert_equals_ref((cube, stats, mask), ref)
        other = torch.empty_like(buf)
        got = F_.adc_interference(_device(name), 32, 2, "clutter", out=other)
        assert got[0].data_ptr() == other.data_ptr()
        _assert_equals_ref(got, ref)


def test_three_launches_are_bit_equal():
    runs = [_F().adc_interference(_device("edges"), 2, 8, "clutter", want_mask=True) for _ in range(3)]
    for cube, stats, mask in runs[1:]:
        assert torch.equal(cube, runs[0][0]) and torch.equal(mask, runs[0][2])
        assert torch.equal(stats.groups, runs[0][1].groups) and torch.equal(stats.frames, runs[0][1].frames)


def test_argument_errors_launch_nothing():
    rt = _rt()
    L, s = rt.lib(), None
    adc = _device("edges")
    out = torch.full_like(adc[:2], 7)
    counts = torch.full((2, 12, 2), 7, dtype=torch.int32, device=_dev())
    stats = torch.full((2, 2), 7, dtype=torch.int32, device=_dev())
    mask = torch.full((2, 4, 192, 32), 7, dtype=torch.uint8, device=_dev())
    p, o, c, m, st = adc.data_ptr(), out.data_ptr(), counts.data_ptr(), mask.data_ptr(), stats.data_ptr()
    n0 = L.hupr_launch_count()
    assert L.hupr_adc_interference_i16(None, None, 0, 32, 2, 0, None, None, s) == 0              # an empty batch is a no-op
    assert L.hupr_adc_interference_stats(None, 0, None, s) == 0
    bad = [(None, o, 2, 32, 2, 0, m, c), (p, None, 2, 32, 2, 0, m, c), (p, o, 2, 32, 2, 0, m, None), (p, o, -1, 32, 2, 0, m, c),
           (p, o, 2, 1, 2, 0, m, c), (p, o, 2, 1025, 2, 0, m, c), (p, o, 2, 32, -1, 0, m, c), (p, o, 2, 32, 9, 0, m, c),
           (p, o, 2, 32, 2, 2, m, c), (p, o, 2, 32, 2, -1, m, c), (p + 2, o, 2, 32, 2, 0, m, c), (p, o + 8, 1, 32, 2, 0, m, c),
           (p, p + 786432, 2, 32, 2, 0, m, c), (p, p + 16, 1, 32, 2, 0, m, c), (p, o, 2, 32, 2, 0, m + 1, c), (p, o, 2, 32, 2, 0, m, c + 2),
           (p, o, 2, 32, 2, 0, o, c), (p, o, 2, 32, 2, 0, m, o), (p, o, 2, 32, 2, 0, m, p), (p, o, 2, 32, 2, 0, c, c),
           (None, None, 0, 1, 2, 0, None, None)]
    for args in bad:
        assert L.hupr_adc_interference_i16(*args, s) == -1, args
        assert b"hupr_adc_interference_i16" in L.hupr_last_error()
    for args in ((None, 2, st), (c, 2, None), (c, -1, st), (c + 2, 2, st), (c, 2, c + 8)):
        assert L.hupr_adc_interference_stats(*args, s) == -1, args
        assert b"hupr_adc_interference_stats" in L.hupr_last_error()
    assert L.hupr_launch_count() == n0
    F_ = _F()
    for kw in (dict(K=1), dict(K=32.0), dict(K=True), dict(guard=9), dict(guard=-1), dict(fill="mean"), dict(fill=0)):
        with pytest.raises(ValueError):
            F_.adc_interference(adc, **kw)
    with pytest.raises(ValueError):
        F_.adc_interference(adc.float())
    with pytest.raises(ValueError):
        F_.adc_interference(adc, out=out)
    with pytest.raises(rt.HuprError):
        F_.adc_interference(adc.cpu())
    assert L.hupr_launch_count() == n0
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (out, counts, stats, mask))


def test_the_filter_commutes_with_the_mirror():
    from hupr_amd.tools import augment as aug
    F_ = _F()
    for name in ("burst", "edges"):
        adc = _device(name)
        a, sa, ma = F_.adc_interference(aug.adc_mirror(adc), 32, 2, "clutter", want_mask=True)
        b, sb, mb = F_.adc_interference(adc, 32, 2, "clutter", want_mask=True)
        assert torch.equal(a, aug.adc_mirror(b)) and torch.equal(sa.frames, sb.frames)
        c = torch.arange(192, device=adc.device)
        assert torch.equal(ma, mb.flip(1)[:, :, c + 2 - 2 * (c % 3)])
        g = torch.tensor([3 * (3 - r) + 2 - t for r in range(4) for t in range(3)], device=adc.device)
        assert torch.equal(sa.groups, sb.groups[:, g])


# ---- the layers above: FFT chain, training engine, live stream -------------------------------------------------------------------------
GOLD = __import__("os").path.join(__import__("os").path.dirname(__file__), "golden")
G, B, N_PUSH = 8, 2, 6
BURST_PUSHES = (1, 4)                 # an eager push and a replayed one


def _filter(**kw):
    from hupr_amd.preprocessing import InterferenceFilter
    return InterferenceFilter(**kw)


def _cfg(interference=None, **training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    if interference is not None:
        cfg.DATASET.interference = interference
    return cfg


@functools.lru_cache(maxsize=None)
def _batch():
    """B G sensor-frames per sensor with bursts in a few of them, their reference-filtered versions and the reference's counts, on
    the device; joints."""
    out = []
    for sensor in range(2):
        host = synth.adc_cube_int16(41, sensor=sensor, nframes=B * G)
        for f in (1, 6, 11) if sensor == 0 else (3, 11):
            host[f] = synth.interference_bursts(host[f], range(2 + f, 192, 17), amp=24000.0, length=(6, 30), seed=10 * f + sensor)[0]
        ref = R.interference_ref(host, 32, 2, "clutter")
        assert (ref["frames"][:, 0] > 0).sum() == (3 if sensor == 0 else 2)
        out.append((torch.from_numpy(host).to(_dev()), torch.from_numpy(ref["cube"]).to(_dev()), torch.from_numpy(ref["frames"]).to(_dev())))
    return out[0], out[1], torch.from_numpy(synth.keypoints(B, 32)).to(_dev())


def _count(fn):
    L = _rt().lib()
    torch.cuda.synchronize()
    n0 = L.hupr_launch_count()
    out = fn()
    return L.hupr_launch_count() - n0, out


def test_fft_chain_with_the_filter_equals_the_chain_on_the_reference_filtered_cube():
    from hupr_amd import preprocessing as pre
    (adc, filtered, _), _, _ = _batch()
    adc, filtered, keep = adc[:3], filtered[:3], adc[:3].clone()
    f = _filter()
    n_on, got = _count(lambda: pre.fft_chain_loader_means(adc, interference=f))
    n_off, want = _count(lambda: pre.fft_chain_loader_means(filtered))
    assert n_on == n_off + 2 and torch.equal(_bits(got), _bits(want)) and torch.equal(adc, keep)
    assert not torch.equal(got, pre.fft_chain_loader_means(adc))
    assert torch.equal(_bits(pre.fft_chain_loader(adc, interference=f)), _bits(pre.fft_chain_loader(filtered)))
    assert torch.equal(pre.fft_chain(adc, interference=f).view(torch.float32), pre.fft_chain(filtered).view(torch.float32))
    assert torch.equal(_bits(pre.fft_chain_loader_means(adc, interference=_filter(K=2, guard=8, fill="zero"))),
                       _bits(pre.fft_chain_loader_means(_F().adc_interference(adc, 2, 8, "zero")[0])))
    with pytest.raises(ValueError, match="InterferenceFilter"):
        pre.fft_chain_loader_means(adc, interference=True)


@pytest.fixture()
def bf16():
    F_ = _F()
    F_.set_math("bf16")
    yield F_
    F_.set_math("f32")


def test_train_step_with_the_key_equals_the_step_on_the_reference_filtered_cubes(bf16):
    from hupr_amd.tools.engine import TrainEngine
    (adc_h, ref_h, frames_h), (adc_v, ref_v, frames_v), joints = _batch()
    with pytest.raises(ValueError, match="DATASET.interference"):
        TrainEngine(_cfg(interference=3), device=_dev(), seed=0)
    on = TrainEngine(_cfg(interference=True), device=_dev(), seed=0)
    off = TrainEngine(_cfg(), device=_dev(), seed=0)
    assert off.interference is None and off.interference_stats() is None and on.interference == _filter()
    n_off, _ = _count(lambda: off.preprocess(adc_h, adc_v))
    assert n_off == 4                                                               # off: two chains of two kernels, as ever
    lo, lo2 = on.train_step_from_adc(adc_h, adc_v, joints)
    lr, lr2 = off.train_step_from_adc(ref_h, ref_v, joints)
    assert torch.equal(_bits(lo), _bits(lr)) and torch.equal(_bits(lo2), _bits(lr2))
    for (name, p), q in zip(on.model.named_parameters(), off.model.parameters()):
        assert torch.equal(_bits(p), _bits(q)), name
    assert torch.equal(on.last_interference[0], frames_h) and torch.equal(on.last_interference[1], frames_v)
    st = on.interference_stats()
    assert st["hori"] == {"frames": B * G, "touched": 3, "samples": int(frames_h[:, 0].sum())}
    assert st["vert"] == {"frames": B * G, "touched": 2, "samples": int(frames_v[:, 0].sum())}
    # inference and the flip test: the filter first, then the mirror
    for flip in (False, True):
        for a, b in zip(on.infer_from_adc(adc_h, adc_v, flip=flip), off.infer_from_adc(ref_h, ref_v, flip=flip)):
            assert torch.equal(_bits(a), _bits(b)), flip
    assert on.interference_stats()["hori"]["frames"] == 3 * B * G
    on.close()
    off.close()
    # under augMirror the filter runs in front of the mirror
    on = TrainEngine(_cfg(interference={"threshold": 32, "guard": 2}, augMirror=1.0), device=_dev(), seed=0)
    off = TrainEngine(_cfg(augMirror=1.0), device=_dev(), seed=0)
    for a, b in zip(on._augmented_from_adc(adc_h, adc_v, joints), off._augmented_from_adc(ref_h, ref_v, joints)):
        assert torch.equal(a, b)
    on.close()
    off.close()


class _Stream:
    def __init__(self):
        from hupr_amd.tools.engine import TrainEngine
        g = np.load(__import__("os").path.join(GOLD, "model_eval.npz"))
        self.cfg = _cfg()
        self.engine = TrainEngine(self.cfg, device="cuda")
        self.model = self.engine.model
        self.model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.hupr_state(int(g["model_seed"]), gain=float(g["gain"])).items()})
        self.model.eval()
        self.model.math_mode = "bf16"
        self.raw, self.ref, self.counts = [], [], []
        for sensor in range(2):
            host = np.concatenate([synth.adc_cube_int16(7, seq=0, frame=f, sensor=sensor) for f in range(N_PUSH)])
            for f in BURST_PUSHES:
                host[f] = synth.interference_bursts(host[f], range(3 + sensor, 192, 11), amp=24000.0, length=(6, 30), seed=f + sensor)[0]
            ref = R.interference_ref(host, 32, 2, "clutter")
            self.raw.append(torch.from_numpy(host).cuda())
            self.ref.append(torch.from_numpy(ref["cube"]).cuda())
            self.counts.append(torch.from_numpy(ref["frames"]).cuda())
        from hupr_amd.tools import PoseStream
        PoseStream(self.model, self.cfg, lanes=1, lookahead=0, graph=False).push(self.ref[0][:1], self.ref[1][:1])      # packs the weights once

    def play(self, frames, host=False, **kw):
        from hupr_amd.tools import PoseStream
        s = PoseStream(self.model, self.cfg, lanes=1, lookahead=1, **kw)
        out, launches = [], []
        for n in range(N_PUSH):
            a, b = frames[0][n:n + 1], frames[1][n:n + 1]
            k, pf = _count(lambda: s.push(a.cpu(), b.cpu()) if host else s.push(a, b))
            launches.append(k)
            if pf is not None:
                out.append(pf.clone())
        return s, out + s.flush(), launches


@pytest.fixture(scope="module")
def stream():
    c = _Stream()
    yield c
    c.engine.close()


@pytest.mark.parametrize("graph", [True, False])
def test_stream_with_the_filter_equals_a_session_fed_the_reference_filtered_frames(stream, graph):
    keep = [t.clone() for t in stream.raw]
    s, got, n_on = stream.play(stream.raw, graph=graph, interference=_filter())
    s0, want, n_off = stream.play(stream.ref, graph=graph)
    assert bool(s._graphs) == graph and len(got) == len(want) == N_PUSH
    assert all(torch.equal(a, b) for a, b in zip(stream.raw, keep))                 # the caller's device frames are left alone
    touched = 0
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.frame == b.frame == i
        for k in ("keypoints", "scores", "indices", "heatmap", "gcn_heatmap"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (i, k)
        assert b.interference is None
        if i < N_PUSH - 1:                     # emitted by push i + 1 (lookahead 1): the counts describe the frame that push brought in
            want_counts = torch.stack([stream.counts[0][i + 1], stream.counts[1][i + 1]]).view(2, 1, 2)
            assert a.interference.dtype == torch.int32 and torch.equal(a.interference, want_counts), i
            touched += int(a.interference[0, 0, 0] > 0)
        else:
            assert a.interference is None      # the flush pushes nothing
    assert touched == len(BURST_PUSHES)
    # eager pushes: the filter's two launches on top of today's; a replay launches nothing through the library's counter
    print("launches per push, filter off: %s  on: %s" % (n_off, n_on))
    eager = [i for i in range(N_PUSH) if not graph or i < 3]
    assert all(n_on[i] == n_off[i] + 2 for i in eager), (n_on, n_off)
    # without the filter: what a push launched before there was one (FFT chain 2 + MNet 1 + advance 1; an emitting push 134)
    assert [n_off[i] for i in eager] == [4] + [134] * (len(eager) - 1), n_off


def test_stream_from_host_frames_and_bad_arguments(stream):
    from hupr_amd.tools import PoseStream
    from hupr_amd.tools.stream import InterferenceError, StreamError
    _, got, _ = stream.play(stream.raw, host=True, interference=_filter())
    _, want, _ = stream.play(stream.ref)
    for a, b in zip(got, want):
        assert torch.equal(a.keypoints, b.keypoints) and torch.equal(a.gcn_heatmap, b.gcn_heatmap)
    assert issubclass(InterferenceError, StreamError)
    for bad in (True, 32, {"threshold": 32}):
        with pytest.raises(InterferenceError):
            PoseStream(stream.model, stream.cfg, interference=bad)


def test_runner_prints_the_share_of_labelled_frames_touched(tmp_path, monkeypatch, capsys):
    """``DATASET.interference`` through main(): one line per epoch, one per evaluation, the checkpoint's keys as ever.  The synthetic
    dataset's cubes are uniform noise, so the share is 0."""
    import yaml
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    cfgd = yaml.safe_load(open(__import__("os").path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"].update(dataDir="synthetic", interference={"threshold": 16, "guard": 1})
    cfgd["TRAINING"].update(batchSize=2, epochs=1)
    cfgd["TEST"].update(batchSize=2)
    for d in ("config", "logs", "visualization"):
        (tmp_path / d).mkdir(exist_ok=True)
    yaml.safe_dump(cfgd, open(tmp_path / "config" / "itf.yaml", "w"))
    monkeypatch.chdir(tmp_path)
    hmain.main(["--config", "itf.yaml", "--dir", "itf", "--synthetic_length", "4", "--max_steps", "2"])
    out = capsys.readouterr().out.splitlines()
    want = "share of 4 labelled frames touched: hori 0.000 (0 samples replaced)  vert 0.000 (0 samples replaced)"
    assert [l for l in out if l.startswith("==========>Interference in epoch 0: ")] == ["==========>Interference in epoch 0: " + want]
    assert [l for l in out if l.startswith("Interference: ")] == ["Interference: " + want]
    assert set(torch.load(tmp_path / "logs" / "itf" / "checkpoint.pth")) == {"epoch", "model_state_dict", "optimizer_state_dict", "accuracy"}
