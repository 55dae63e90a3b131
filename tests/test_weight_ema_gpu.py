"""GPU (-m gpu): TRAINING.emaDecay — the weight average: hupr_ema_tick_f32 (the warm-up ramp and the update count on the device,
obeying the gradient guard), hupr_ema_update_f32 (ema += w (p - ema)) and hupr_swap_f32, through the C ABI, then through
TrainEngine (eager, skipped steps, graph replay, averaged_weights(), resume) and main.py / the stream's loader.

Tolerances.  The tick's weight is one fp64 expression rounded to fp32 and is compared exactly.  One update is one fp32 subtraction
and one fused multiply-add, so it commits at most about one fp32 ulp of |ema| (2^-23 relative); the tests run 3 to 5 updates against
the fp64 recurrence on the same fp32 weights, 5 x 2^-23 = 6e-7, and compare at 1e-6 of the largest value.  Everything else (the
path taken, a skipped step, a swap, a replayed graph, a resumed run) is compared bit for bit."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from hupr_amd import synth

pytestmark = pytest.mark.gpu
SIZES = [1, 3, 4, 5, 1023, 10007, (1 << 20) + 3]
DECAY = 0.999
CANARY = -12345.5
INF = float("inf")


def close(got, ref, tol, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-30
    print("%s: max err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / scale))
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / scale)


def f32(x):
    return float(np.float32(x))


def weight64(k, decay=DECAY):
    """The tick's weight after k earlier updates, restated in numpy fp64 and rounded to fp32 (decay as the kernel receives it)."""
    d = min(np.float64(np.float32(decay)), (np.float64(1.0) + k) / (np.float64(10.0) + k))
    return f32(np.float64(1.0) - d)


def _rnd(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _lib():
    from hupr_amd import runtime as rt
    return rt, rt.lib()


def _tick(state, guard=None, decay=DECAY):
    rt, L = _lib()
    rt.check(L.hupr_ema_tick_f32(rt.ptr(state), decay, rt.ptr(guard), rt.stream()))


def _update(ema, p, state):
    rt, L = _lib()
    rt.check(L.hupr_ema_update_f32(rt.ptr(ema), rt.ptr(p), ema.numel(), rt.ptr(state), rt.stream()))


def _swap(a, b):
    rt, L = _lib()
    rt.check(L.hupr_swap_f32(rt.ptr(a), rt.ptr(b), a.numel(), rt.stream()))


def _bits(t):
    return t.view(torch.int32)


def _bits_equal(a, b):
    return torch.equal(_bits(a), _bits(b))


def _in_canaries(data, off, pad=8):
    """``data`` at element offset ``off`` of a larger buffer filled with the canary -> (buffer, view)."""
    big = torch.full((data.numel() + pad,), CANARY, device="cuda")
    view = big[off:off + data.numel()]
    view.copy_(data)
    assert view.data_ptr() % 16 == 4 * off
    return big, view


def _canaries_intact(big, off, n):
    return bool((torch.cat([big[:off], big[off + n:]]) == CANARY).all())


# ---- the kernels through the C ABI ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    """Per size: a start value and five parameter vectors, made once and left unchanged."""
    return {n: (_rnd(n, 2000 + i).cuda(), [_rnd(n, 3000 + 10 * i + k).cuda() for k in range(5)]) for i, n in enumerate(SIZES)}


@pytest.mark.parametrize("n", SIZES)
def test_five_updates_match_the_fp64_recurrence(n, data):
    e0, ps = data[n]
    ema = e0.clone()
    state = torch.zeros(2, device="cuda")
    ref = e0.double()
    for k, p in enumerate(ps):
        _tick(state)
        w = weight64(k)
        assert w == f32(1 - min(0.999, (1 + k) / (10 + k)))          # the ramp, not the decay, rules the first updates
        assert state.tolist() == [float(k + 1), w], (k, state.tolist(), w)
        _update(ema, p, state)
        ref = ref + w * (p.double() - ref)
    torch.cuda.synchronize()
    close(ema, ref, 1e-6, "n=%d: ema after 5 updates" % n)
    assert not torch.equal(ema, e0)


def test_the_ramp_ends_at_the_decay():
    """k = 8990: (1 + k) / (10 + k) = 0.999 in exact arithmetic; from there on the weight is 1 - decay, decay as an fp32 number."""
    state = torch.zeros(2, device="cuda")
    for k in (0, 9, 8000, 8990, 8991, 100000):
        state.copy_(torch.tensor([float(k), 0.25]))
        _tick(state)
        assert state.tolist() == [float(k + 1), weight64(k)], k
    assert weight64(100000) == f32(1.0 - float(np.float32(DECAY))) and weight64(8000) > weight64(100000)
    for decay, end in ((0.5, 8), (0.9, 80)):                         # (1 + k) / (10 + k) reaches 0.5 at k = 8, 0.9 at k = 80
        for k in (0, end - 1, end, end + 1, 1000):
            state.copy_(torch.tensor([float(k), 0.25]))
            _tick(state, decay=decay)
            assert state.tolist() == [float(k + 1), weight64(k, decay)], (decay, k)
        assert weight64(end - 1, decay) > weight64(end + 1, decay) == weight64(1000, decay) == f32(1.0 - float(np.float32(decay)))


OFFSETS = [(1, 0), (0, 1), (1, 1), (3, 3), (2, 1)]          # (ema / a, p / b): alone, both, and further boundaries


@pytest.mark.parametrize("n", [5, 10007, (1 << 20) + 3])
def test_unaligned_update_equals_the_aligned_one(n, data):
    """The same data at element offsets of larger buffers — equal offsets: scalar head, float4 body, scalar tail; different ones:
    the 4-byte launch — gives the bits of the aligned launch, and nothing around either array is touched."""
    e0, ps = data[n]
    state = torch.zeros(2, device="cuda")
    _tick(state)
    want = e0.clone()
    _update(want, ps[0], state)
    assert not torch.equal(want, e0)
    for oe, op in OFFSETS:
        ebig, ev = _in_canaries(e0, oe)
        pbig, pv = _in_canaries(ps[0], op)
        pcopy = pbig.clone()
        sbig = torch.full((6,), CANARY, device="cuda")
        sbig[2:4].copy_(state)
        _update(ev, pv, sbig[2:4])
        torch.cuda.synchronize()
        assert torch.equal(ev, want), (oe, op)
        assert _canaries_intact(ebig, oe, n), (oe, op)
        assert _bits_equal(pbig, pcopy) and _bits_equal(sbig[2:4], state) and bool((sbig[:2] == CANARY).all()) \
            and bool((sbig[4:] == CANARY).all()), (oe, op)


def _patterns(n, seed):
    """n random 32-bit patterns as fp32, among them quiet and signalling NaNs with payloads, -0.0, infinities and denormals."""
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    special = torch.tensor([0x7fc00001, 0xffc12345 - (1 << 32), 0x7f800001, 0x80000000 - (1 << 32), 0x7f800000, 0x00000001, 0xff800000 - (1 << 32)])
    k = min(n, special.numel())
    bits[torch.arange(k) * (n // k)] = special.roll(seed)[:k]                # another order per seed: two arrays differ from n = 2 on
    return bits.to(torch.int32).view(torch.float32).cuda()


@pytest.mark.parametrize("n", SIZES)
def test_swap_is_exact_and_twice_is_the_identity(n):
    a0, b0 = _patterns(n, 11), _patterns(n, 12)
    a, b = a0.clone(), b0.clone()
    _swap(a, b)
    torch.cuda.synchronize()
    assert _bits_equal(a, b0) and _bits_equal(b, a0)
    assert n < 2 or not _bits_equal(a, a0)
    _swap(a, b)
    torch.cuda.synchronize()
    assert _bits_equal(a, a0) and _bits_equal(b, b0)


@pytest.mark.parametrize("n", [5, 10007, (1 << 20) + 3])
def test_unaligned_swap_equals_the_aligned_one(n):
    a0, b0 = _patterns(n, 13), _patterns(n, 14)
    for oa, ob in OFFSETS:
        abig, av = _in_canaries(a0, oa)
        bbig, bv = _in_canaries(b0, ob)
        _swap(av, bv)
        torch.cuda.synchronize()
        assert _bits_equal(av, b0) and _bits_equal(bv, a0), (oa, ob)
        assert _canaries_intact(abig, oa, n) and _canaries_intact(bbig, ob, n), (oa, ob)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [5, 10007])
def test_a_skipped_step_stores_nothing(n, off):
    """guard = {0, inf, 1, 0}: the tick keeps the count and sets the weight to 0, the update keeps every bit of ema although p is
    all NaN.  guard = {1, 1, 0, 1} and no guard: the update runs."""
    ebig, ev = _in_canaries(_patterns(n, 21), off)
    before = ebig.clone()
    p = torch.full((n,), float("nan"), device="cuda")
    state = torch.tensor([3.0, 0.5], device="cuda")
    skipped = torch.tensor([0.0, INF, 1.0, 0.0], device="cuda")
    _tick(state, skipped)
    assert state.tolist() == [3.0, 0.0] and skipped.tolist() == [0.0, INF, 1.0, 0.0]
    _update(ev, p, state)
    pv = _in_canaries(p, 1 - off)[1]                                 # and through the 4-byte launch
    _update(ev, pv, state)
    torch.cuda.synchronize()
    assert _bits_equal(ebig, before)
    for guard in (torch.tensor([1.0, 1.0, 0.0, 1.0], device="cuda"), None):
        e0 = _rnd(n, 22)
        ebig, ev = _in_canaries(e0.cuda(), off)
        p = _rnd(n, 23).cuda()
        state = torch.tensor([3.0, 0.0], device="cuda")
        _tick(state, guard)
        assert state.tolist() == [4.0, weight64(3)]
        _update(ev, p, state)
        torch.cuda.synchronize()
        close(ev, e0.double() + weight64(3) * (p.double().cpu() - e0.double()), 1e-6, "update behind a finite step")
        assert not torch.equal(ev.cpu(), e0) and _canaries_intact(ebig, off, n)


def test_ema_entries_refuse_bad_arguments_before_any_launch():
    rt, L = _lib()
    t = torch.zeros(64, device="cuda")
    a, s = rt.ptr(t), rt.stream()
    b, st = a + 128, a + 192
    before = L.hupr_launch_count()
    for state, decay, guard in [(None, DECAY, None), (None, DECAY, a)] + [(st, d, g) for d in (0.0, 1.0, 1.5, -0.1, float("nan"))
                                                                          for g in (None, a)]:
        assert L.hupr_ema_tick_f32(state, decay, guard, s) == -1 and b"hupr_ema_tick_f32" in L.hupr_last_error()
    for e, p, n, state in [(None, b, 16, st), (a, None, 16, st), (a, b, 16, None), (a, b, 0, st), (a, b, -4, st), (a + 2, b, 8, st)]:
        assert L.hupr_ema_update_f32(e, p, n, state, s) == -1 and b"hupr_ema_update_f32" in L.hupr_last_error()
    for x, y, n in [(None, b, 16), (a, None, 16), (a, b, 0), (a, b, -4), (a, a, 16), (a, a + 4, 16), (a + 60, a, 16), (a, a + 60, 16),
                    (a + 2, b, 8)]:
        assert L.hupr_swap_f32(x, y, n, s) == -1 and b"hupr_swap_f32" in L.hupr_last_error()
    assert L.hupr_launch_count() == before
    assert L.hupr_swap_f32(a, a + 64, 16, s) == 0                    # adjacent ranges do not overlap
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ---- the engine with TRAINING.emaDecay (bf16, B = 2 synthetic cubes) --------------------------------------------------------
def _setup(optimizer, clip=None, ema=None, B=2, seed=51):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    cfg.TRAINING.optimizer = optimizer
    if clip is not None:
        cfg.TRAINING.gradClip = clip
    if ema is not None:
        cfg.TRAINING.emaDecay = ema
    dev = torch.device("cuda", 0)
    G = cfg.DATASET.numGroupFrames
    adc_h = torch.from_numpy(synth.adc_cube_int16(seed, sensor=0, nframes=B * G)).to(dev)
    adc_v = torch.from_numpy(synth.adc_cube_int16(seed, sensor=1, nframes=B * G)).to(dev)
    joints = torch.from_numpy(synth.keypoints(B, seed + 1)).to(dev)
    return cfg, dev, (adc_h, adc_v, joints)


def _engine(optimizer, clip=None, ema=None, seed=51):
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, batch = _setup(optimizer, clip, ema, seed=seed)
    return TrainEngine(cfg, device=dev, seed=0), batch


def _flat(eng):
    return torch.cat([p.detach().flatten() for p in eng.model.parameters()])


def _state(eng):
    return [st[k] for st in eng.optimizer._flat_state for k in eng.optimizer._state_keys]


def _params(eng):
    """Clones of the flat parameter buckets."""
    return [p.clone() for p, _ in eng.optimizer._flat]


def _same_training_state(a, b):
    assert _bits_equal(_flat(a), _flat(b))
    for x, y in zip(_state(a), _state(b)):
        assert _bits_equal(x, y)


def _same_average(a, b):
    assert len(a.ema.flat) == len(b.ema.flat) >= 2
    for x, y in zip(a.ema.flat, b.ema.flat):
        assert _bits_equal(x, y)
    assert a.ema_stats() == b.ema_stats()


@pytest.fixture
def bf16():
    from hupr_amd import functional as F_
    F_.set_math("bf16")
    yield F_
    F_.set_math("f32")


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_engine_average_is_transparent_to_training_and_matches_fp64(optimizer, bf16):
    e0, batch = _engine(optimizer, seed=71)
    assert e0.ema is None and e0.ema_stats() is None
    with pytest.raises(RuntimeError, match="emaDecay"):
        with e0.averaged_weights():
            pass
    e1, _ = _engine(optimizer, ema=DECAY, seed=71)
    assert e1.ema is not None and e1.ema.decay == DECAY and e1.ema_stats() == {"updates": 0, "weight": 0.0}
    ref = [p.double() for p in _params(e1)]
    for e, r in zip(e1.ema.flat, ref):
        assert torch.equal(e.double(), r)                            # starts as a copy of the parameters
    for k in range(3):
        l0, _ = e0.train_step_from_adc(*batch)
        l1, _ = e1.train_step_from_adc(*batch)
        w = weight64(k)
        ref = [r + w * (p.double() - r) for r, p in zip(ref, _params(e1))]
    torch.cuda.synchronize()
    assert float(l0.detach()) == float(l1.detach())
    _same_training_state(e0, e1)
    assert e1.ema_stats() == {"updates": 3, "weight": weight64(2)}
    for i, (e, r, (p, _)) in enumerate(zip(e1.ema.flat, ref, e1.optimizer._flat)):
        close(e, r, 1e-6, "%s bucket %d" % (optimizer, i))
        assert not torch.equal(e, p)                                 # the average lags the parameters


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_engine_average_stands_still_across_a_skipped_step(optimizer, bf16):
    eng, batch = _engine(optimizer, INF, DECAY, seed=73)
    eng.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    a1 = [e.clone() for e in eng.ema.flat]
    assert eng.ema_stats() == {"updates": 1, "weight": weight64(0)}
    eng._seed.fill_(INF)
    eng.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    assert eng.guard_stats()["skipped"] == 1
    assert eng.ema_stats() == {"updates": 1, "weight": 0.0}
    for e, a in zip(eng.ema.flat, a1):
        assert _bits_equal(e, a)
    eng._seed.fill_(1.0)
    eng.train_step_from_adc(*batch)
    twin, _ = _engine(optimizer, INF, DECAY, seed=73)
    for _ in range(2):
        twin.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.cat(eng.ema.flat)).all())
    _same_training_state(eng, twin)
    _same_average(eng, twin)
    assert eng.ema_stats() == {"updates": 2, "weight": weight64(1)}


def test_engine_average_replays_inside_the_graph(bf16):
    """Eager: ok, ok, skip, ok.  Graph: ok, capture (1 warm-up step), a replay with the inf seed, a replay.  Bit-equal: the count, the
    weight and the guard's decision all live on the device."""
    def run(graph):
        eng, batch = _engine("adam", INF, DECAY, seed=75)
        eng.train_step_from_adc(*batch)
        if graph:
            eng.capture(*batch, warmup=1)
        else:
            eng.train_step_from_adc(*batch)
        eng._seed.fill_(INF)
        eng.train_step_from_adc(*batch)
        eng._seed.fill_(1.0)
        eng.train_step_from_adc(*batch)
        torch.cuda.synchronize()
        assert (eng._graph is not None) == graph
        return eng
    e1, e2 = run(False), run(True)
    _same_training_state(e1, e2)
    _same_average(e1, e2)
    assert e2.ema_stats() == {"updates": 3, "weight": weight64(2)} and e2.guard_stats()["skipped"] == 1
    assert bool(torch.isfinite(torch.cat(e2.ema.flat)).all())


def test_engine_averaged_weights_swap_in_and_out(bf16):
    from hupr_amd.models import HuPRNet
    eng, batch = _engine("adam", ema=DECAY, seed=77)
    twin, _ = _engine("adam", ema=DECAY, seed=77)
    for _ in range(2):
        eng.train_step_from_adc(*batch)
        twin.train_step_from_adc(*batch)
    hv = eng.preprocess(batch[0], batch[1])
    live_out = eng.infer(*hv)                                        # fills every derived-weight cache with the live weights
    live, avg = _params(eng), [e.clone() for e in eng.ema.flat]
    sd = eng.ema.state_dict(eng.model)
    assert list(sd) == list(eng.model.state_dict())
    with eng.averaged_weights():
        assert eng.ema.swapped
        for (p, _), e, l, a in zip(eng.optimizer._flat, eng.ema.flat, live, avg):
            assert _bits_equal(p, a) and _bits_equal(e, l)
        got = eng.infer(*hv)
        with pytest.raises(RuntimeError, match="averaged_weights"):
            eng.train_step_from_adc(*batch)
        with pytest.raises(RuntimeError, match="averaged_weights"):
            eng.train_step(*hv, batch[2])
        with pytest.raises(RuntimeError, match="averaged_weights"):
            eng.capture(*batch)
        with pytest.raises(RuntimeError, match="nesting"):
            with eng.averaged_weights():
                pass
        with pytest.raises(RuntimeError, match="swapped"):
            eng.ema.state_dict(eng.model)
        assert eng.ema.swapped                                       # the refused calls changed nothing
    assert not eng.ema.swapped
    for (p, _), e, l, a in zip(eng.optimizer._flat, eng.ema.flat, live, avg):
        assert _bits_equal(p, l) and _bits_equal(e, a)
    fresh = HuPRNet(eng.cfg).to(eng.device).eval()
    fresh.load_state_dict(sd, strict=True)
    bf16.invalidate_packed()
    with torch.no_grad():
        want = fresh(*hv)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not (torch.equal(got[0], live_out[0]) and torch.equal(got[1], live_out[1]))     # the average is not the live weights
    back = eng.infer(*hv)                                            # and the live weights are back behind the block
    assert torch.equal(back[0], live_out[0]) and torch.equal(back[1], live_out[1])
    eng.train_step_from_adc(*batch)
    twin.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    _same_training_state(eng, twin)
    _same_average(eng, twin)


def test_engine_average_resumes_from_a_checkpoint(bf16):
    full, batch = _engine("adam", ema=DECAY, seed=79)
    for _ in range(3):
        full.train_step_from_adc(*batch)
    first, _ = _engine("adam", ema=DECAY, seed=79)
    for _ in range(2):
        first.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    saved = {"model": {k: v.clone() for k, v in first.model.state_dict().items()}, "optimizer": first.optimizer.state_dict(),
             "ema": first.ema.state_dict(first.model), "updates": first.ema_stats()["updates"]}
    assert saved["updates"] == 2
    second, _ = _engine("adam", ema=DECAY, seed=80)
    second.model.load_state_dict(saved["model"])
    second.optimizer.load_state_dict(saved["optimizer"])
    second.ema.load_state_dict(saved["ema"], saved["updates"])
    assert second.ema_stats() == {"updates": 2, "weight": 0.0}
    second.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    _same_training_state(full, second)
    _same_average(full, second)
    assert second.ema_stats() == {"updates": 3, "weight": weight64(2)}


def test_bucket_update_time(bf16):
    """Prints what the average costs per step on the engine's own buckets: the tick and the per-bucket updates, timed with HIP
    events around the whole group on a quiet stream — warm-up, then the median of 20.  A figure, not a bound."""
    eng, _ = _engine("adam", ema=DECAY, seed=81)
    ema = eng.ema
    nbytes = sum(e.numel() for e in ema.flat) * 4
    for _ in range(5):
        ema.update()
    torch.cuda.synchronize()
    times = []
    for _ in range(20):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ema.update()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3)
    us = float(np.median(times))
    print("weight average: %d buckets, %.1f MB of parameters, tick + updates %.1f us per step (median of 20, min %.1f, max %.1f; "
          "%.2f TB/s over 12 B per element)" % (len(ema.flat), nbytes / 1e6, us, min(times), max(times), 3 * nbytes / us / 1e6))
    assert math.isfinite(us) and us > 0


# ---- main.py and the stream's loader -------------------------------------------------------------------------------------------
def test_main_train_resume_eval_with_ema(tmp_path, monkeypatch, capsys):
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR, load_config
    from hupr_amd.models import HuPRNet
    from hupr_amd.tools.stream import load_model_best
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"]["dataDir"] = "synthetic"
    cfgd["TRAINING"]["batchSize"] = 2
    cfgd["TRAINING"]["epochs"] = 1
    cfgd["TEST"]["batchSize"] = 2
    (tmp_path / "config").mkdir()
    yaml.safe_dump(cfgd, open(tmp_path / "config" / "plain.yaml", "w"))
    cfgd["TRAINING"]["emaDecay"] = 0.999
    yaml.safe_dump(cfgd, open(tmp_path / "config" / "tiny.yaml", "w"))
    (tmp_path / "logs").mkdir()
    (tmp_path / "visualization").mkdir()
    monkeypatch.chdir(tmp_path)
    four = ["epoch", "model_state_dict", "optimizer_state_dict", "accuracy"]

    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--max_steps", "2"])
    out = capsys.readouterr().out
    assert "averaged weights" in out
    run = tmp_path / "logs" / "run0"
    ck = torch.load(run / "checkpoint.pth")
    assert list(ck) == four + ["ema_state_dict", "ema_updates"] and ck["ema_updates"] == 2
    model = HuPRNet(load_config()).eval()
    assert list(ck["ema_state_dict"]) == list(model.state_dict())
    model.load_state_dict(ck["ema_state_dict"], strict=True)
    pnames = [k for k, _ in model.named_parameters()]
    assert any(not torch.equal(ck["ema_state_dict"][k], ck["model_state_dict"][k]) for k in pnames)
    assert all(bool(torch.isfinite(ck["ema_state_dict"][k]).all()) for k in pnames)

    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--max_steps", "1"])   # resumes
    out = capsys.readouterr().out
    assert "previous weight average (2 updates)" in out
    assert torch.load(run / "checkpoint.pth")["ema_updates"] == 3

    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--eval"])
    out = capsys.readouterr().out
    assert "Load the averaged weights" in out
    assert len(json.load(open(run / "test_results.json"))) == 4

    best = torch.load(run / "model_best.pth")
    dev = torch.device("cuda", 0)
    model = HuPRNet(load_config()).to(dev).eval()
    load_model_best(model, str(run), dev, weights="averaged")
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), best["ema_state_dict"][k].cpu()), k
    load_model_best(model, str(run), dev)                            # the default: the weights as trained
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), best["model_state_dict"][k].cpu()), k
    with pytest.raises(ValueError, match="weights"):
        load_model_best(model, str(run), dev, weights="best")

    # without the key: the reference's four checkpoint keys, no word about an average, and no averaged weights to stream
    capsys.readouterr()
    hmain.main(["--config", "plain.yaml", "--dir", "run1", "--synthetic_length", "4", "--max_steps", "2"])
    out = capsys.readouterr().out
    assert "averaged" not in out and "average" not in out
    assert list(torch.load(tmp_path / "logs" / "run1" / "checkpoint.pth")) == four
    with pytest.raises(KeyError, match="ema_state_dict"):
        load_model_best(model, str(tmp_path / "logs" / "run1"), dev, weights="averaged")
    # emaDecay set, resuming a checkpoint that has no average: it starts from the loaded weights
    hmain.main(["--config", "tiny.yaml", "--dir", "run1", "--synthetic_length", "4", "--max_steps", "1"])
    out = capsys.readouterr().out
    assert "starts from the loaded weights at 0 updates" in out
    assert torch.load(tmp_path / "logs" / "run1" / "checkpoint.pth")["ema_updates"] == 1
