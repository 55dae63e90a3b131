"""GPU (-m gpu): TRAINING.gradClip — the gradient guard: hupr_grad_sumsq_f32 + hupr_grad_guard_f32 (global L2 norm of the flat
gradients, clip_grad_norm_'s coefficient, the finite / skip decision, all on the device) and the optimiser steps that obey it
(hupr_adam_step_guard_f32, hupr_sgd_step_guard_f32), through the C ABI, then through TrainEngine, graph capture, the forced
collective and main.py.

Tolerances.  The sum of squares is accumulated in fp64 from the first element on, so norm and coef are compared with the fp64
restatement ROUNDED TO fp32 and may differ from it by at most 1 fp32 ulp: the only difference between kernel and restatement is
the order of an fp64 sum (relative ~1e-13), which can move the final rounding to fp32 across a tie and nothing else.  The step
kernels are compared at 1e-6 of the largest value, the tolerance of the fused optimisers' own tests (tests/test_sgd_gpu.py).
Injected inf / NaN values are ordinary arithmetic."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from hupr_amd import synth

pytestmark = pytest.mark.gpu
SIZES = [1, 3, 255, 1025, 10007, (1 << 20) + 3]
LR, MOM, WD, B1, B2, EPS = 1e-2, 0.9, 1e-4, 0.9, 0.999, 1e-8
CANARY = -12345.5
INF = float("inf")


def close(got, ref, tol, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-30
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / scale)


def ulps(a, b):
    """Distance of two finite fp32 values of equal sign in units in the last place."""
    ia, ib = (int(np.array(x, dtype=np.float32).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def f32(x):
    return float(np.float32(x))


def _rnd(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _lib():
    from hupr_amd import runtime as rt
    return rt, rt.lib()


def _sumsq(g, partials):
    rt, L = _lib()
    rt.check(L.hupr_grad_sumsq_f32(rt.ptr(g), g.numel(), rt.ptr(partials), rt.stream()))


def _guard(partials, gscale, max_norm, state, guard):
    rt, L = _lib()
    rt.check(L.hupr_grad_guard_f32(rt.ptr(partials), partials.numel(), gscale, max_norm, rt.ptr(state), rt.ptr(guard), rt.stream()))


def _new_partials(buckets=1, fill=7.0):
    """Pre-filled with a value that is neither 0 nor a sum: every slot must be written by the launch."""
    _, L = _lib()
    return torch.full((buckets * L.hupr_grad_sumsq_partials(),), fill, dtype=torch.float64, device="cuda")


def _norm_coef64(gs, gscale, max_norm):
    """The fp64 restatement: norm = gscale sqrt(sum g^2), coef = min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_'s rule)."""
    total = sum(float((g.detach().double() ** 2).sum()) for g in gs)
    norm = gscale * math.sqrt(total)
    return norm, min(1.0, max_norm / (norm + 1e-6))


# ---- the reduction and the decision through the C ABI ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def gradients():
    """One random gradient per size, made once and left unchanged."""
    return {n: _rnd(n, 1000 + i).cuda() for i, n in enumerate(SIZES)}


@pytest.mark.parametrize("n", SIZES)
def test_norm_and_coefficient_match_fp64_within_one_ulp(n, gradients):
    g = gradients[n]
    partials = _new_partials()
    _sumsq(g, partials)
    torch.cuda.synchronize()
    total64 = float((g.double().cpu() ** 2).sum())
    assert abs(float(partials.sum()) - total64) <= 1e-12 * total64
    assert int((partials != 0).sum()) <= (n + 3) // 4 + 2          # slots without an element hold 0.0, none the pre-fill
    assert bool((partials != 7.0).all())
    for gscale in (1.0, 0.5):
        norm0, _ = _norm_coef64([g], gscale, INF)
        for max_norm in (INF, f32(2 * norm0), f32(norm0 / 2)):
            state = torch.tensor([LR, 4.0], device="cuda")
            guard = torch.zeros(4, device="cuda")
            _guard(partials, gscale, max_norm, state, guard)
            coef, norm, skipped, finite = guard.tolist()
            nref, cref = _norm_coef64([g], gscale, max_norm)
            print("n=%d gscale=%g max_norm=%g: norm %.9g (fp64 %.17g), coef %.9g (fp64 %.17g)" % (n, gscale, max_norm, norm, nref, coef, cref))
            assert ulps(norm, f32(nref)) <= 1, (norm, nref)
            assert ulps(coef, f32(cref)) <= 1, (coef, cref)
            if max_norm == INF or max_norm > 1.5 * nref:
                assert coef == 1.0                                   # exactly: the unclipped step keeps gscale's bits
            else:
                assert 0.49 < coef < 0.51
            assert (skipped, finite) == (0.0, 1.0)
            assert state.tolist() == [f32(LR), 5.0]                  # the guard kernel owns the step increment


@pytest.mark.parametrize("n", SIZES)
def test_unaligned_gradient_gives_the_same_norm(n, gradients):
    """The same data at element offset 1 of a larger buffer (scalar head, float4 body from the first 16-byte boundary, scalar
    tail) gives the same fp32 norm; nothing around the gradient, the partials, the state or the guard is touched."""
    _, L = _lib()
    K = L.hupr_grad_sumsq_partials()
    g = gradients[n]
    out = {}
    for off in (0, 1, 2, 3):
        big = torch.full((n + 8,), CANARY, device="cuda")
        view = big[off:off + n]
        view.copy_(g)
        assert view.data_ptr() % 16 == 4 * off
        pbig = torch.full((K + 2,), CANARY, dtype=torch.float64, device="cuda")
        sbig = torch.full((2 + 4,), CANARY, device="cuda")
        gbig = torch.full((4 + 4,), CANARY, device="cuda")
        state, guard = sbig[2:4], gbig[2:6]
        state.copy_(torch.tensor([LR, 0.0]))
        guard.zero_()
        _sumsq(view, pbig[1:1 + K])
        _guard(pbig[1:1 + K], 1.0, INF, state, guard)
        torch.cuda.synchronize()
        out[off] = guard.tolist()
        assert torch.equal(view, g)
        assert bool((torch.cat([big[:off], big[off + n:]]) == CANARY).all())
        assert pbig[0].item() == CANARY and pbig[-1].item() == CANARY
        assert bool((sbig[:2] == CANARY).all()) and bool((sbig[4:] == CANARY).all()) and state.tolist() == [f32(LR), 1.0]
        assert bool((gbig[:2] == CANARY).all()) and bool((gbig[6:] == CANARY).all())
    assert out[1] == out[0] and out[2] == out[0] and out[3] == out[0], out


@pytest.mark.parametrize("n", [10007, (1 << 20) + 3])
def test_partials_are_bit_identical_from_launch_to_launch(n, gradients):
    runs = []
    for _ in range(3):
        partials = _new_partials()
        _sumsq(gradients[n], partials)
        runs.append(partials)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("n", [1, 3, 10007, (1 << 20) + 3])
def test_non_finite_gradient_is_a_skip(n, gradients):
    """One inf, -inf or NaN at the first, a middle or the last element: finite = 0, coef = 0, skipped + 1, the step count stays
    (and the learning rate beside it).  Two buckets: the bad value sits in either."""
    other = gradients[255]
    for k, pos in enumerate(sorted({0, n // 2, n - 1})):
        for j, bad in enumerate((INF, float("nan"), -INF)):
            g = gradients[n].clone()
            g[pos] = bad
            partials = _new_partials(2)
            K = partials.numel() // 2
            first = (k + j) % 2 == 0
            _sumsq(g if first else other, partials[:K])
            _sumsq(other if first else g, partials[K:])
            state = torch.tensor([LR, 4.0], device="cuda")
            guard = torch.tensor([0.25, 1.0, 2.0, 1.0], device="cuda")      # an earlier step's decision, two skips so far
            _guard(partials, 1.0, 1.0, state, guard)
            coef, norm, skipped, finite = guard.tolist()
            assert (coef, skipped, finite) == (0.0, 3.0, 0.0) and not math.isfinite(norm), (pos, bad, guard.tolist())
            assert state.tolist() == [f32(LR), 4.0]


def test_a_square_beyond_fp32_is_still_a_finite_norm():
    """3e38^2 overflows fp32, not the fp64 accumulator: the step is clipped, not skipped."""
    g = _rnd(10007, 7).cuda()
    g[5003] = 3e38
    partials = _new_partials()
    _sumsq(g, partials)
    state = torch.tensor([LR, 0.0], device="cuda")
    guard = torch.zeros(4, device="cuda")
    _guard(partials, 1.0, 1.0, state, guard)
    coef, norm, skipped, finite = guard.tolist()
    nref, cref = _norm_coef64([g], 1.0, 1.0)
    assert math.isfinite(norm) and ulps(norm, f32(nref)) <= 1 and ulps(coef, f32(cref)) <= 1 and coef > 0
    assert (skipped, finite) == (0.0, 1.0) and state.tolist() == [f32(LR), 1.0]


# ---- the guarded optimiser steps through the C ABI ------------------------------------------------------------------------
def _adam_dev(p, g, m, v, state, gscale=1.0):
    rt, L = _lib()
    rt.check(L.hupr_adam_step_dev_f32(rt.ptr(p), rt.ptr(g), rt.ptr(m), rt.ptr(v), p.numel(), rt.ptr(state), B1, B2, EPS, WD, gscale,
                                      rt.stream()))


def _adam_guard(p, g, m, v, state, guard, gscale=1.0):
    rt, L = _lib()
    rt.check(L.hupr_adam_step_guard_f32(rt.ptr(p), rt.ptr(g), rt.ptr(m), rt.ptr(v), p.numel(), rt.ptr(state), rt.ptr(guard), B1, B2,
                                        EPS, WD, gscale, rt.stream()))


def _sgd_dev(p, g, buf, state, gscale=1.0):
    rt, L = _lib()
    rt.check(L.hupr_sgd_step_dev_f32(rt.ptr(p), rt.ptr(g), rt.ptr(buf), p.numel(), rt.ptr(state), MOM, WD, gscale, rt.stream()))


def _sgd_guard(p, g, buf, state, guard, gscale=1.0):
    rt, L = _lib()
    rt.check(L.hupr_sgd_step_guard_f32(rt.ptr(p), rt.ptr(g), rt.ptr(buf), p.numel(), rt.ptr(state), rt.ptr(guard), MOM, WD, gscale,
                                       rt.stream()))


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("n", [5, 10007])
def test_guarded_steps_with_coef_one_are_the_dev_entries_bit_for_bit(n, gscale):
    """4 steps, the learning rate halved after step 2, the guard taken by the real kernels with max_norm = inf (coef exactly 1,
    the step count advanced by the guard kernel): the bits of hupr_adam_step_dev_f32 / hupr_sgd_step_dev_f32, whose step
    count the host sets."""
    z = lambda: torch.zeros(n, device="cuda")
    ref = dict(pa=_rnd(n, 5).cuda(), m=z(), v=z(), ps=_rnd(n, 6).cuda(), buf=torch.empty(n, device="cuda"))
    got = dict(pa=_rnd(n, 5).cuda(), m=z(), v=z(), ps=_rnd(n, 6).cuda(), buf=torch.empty(n, device="cuda"))
    sref = torch.zeros(2, device="cuda")
    sgot = torch.tensor([LR, 0.0], device="cuda")
    guard = torch.zeros(4, device="cuda")
    partials = _new_partials()
    lr = LR
    for step in range(1, 5):
        if step == 3:
            lr = LR / 2
            sgot[0] = lr
        g = _rnd(n, 20 + step).cuda()
        sref.copy_(torch.tensor([lr, float(step)]))
        _adam_dev(ref["pa"], g, ref["m"], ref["v"], sref, gscale)
        _sgd_dev(ref["ps"], g, ref["buf"], sref, gscale)
        _sumsq(g, partials)
        _guard(partials, gscale, INF, sgot, guard)
        _adam_guard(got["pa"], g, got["m"], got["v"], sgot, guard, gscale)
        _sgd_guard(got["ps"], g, got["buf"], sgot, guard, gscale)
    torch.cuda.synchronize()
    assert guard[0].item() == 1.0 and sgot.tolist() == sref.tolist()
    for k in ref:
        assert torch.equal(ref[k], got[k]), k


@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_clipped_steps_match_torch_and_fp64(gscale):
    """Two buckets (10007 and 1025 elements, one global norm), max_norm = 40 against norms of ~105 gscale: 5 steps with a new
    gradient each, against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / SGD on the GPU and against an fp64 restatement
    (coef from the fp64 norm).  The restatement works on the hyper-parameters as the kernel receives them, rounded to fp32:
    Adam's 1 - beta2 is then 0.99998713e-3 where torch, which subtracts in double, has 1e-3, so exp_avg_sq stands 1.29e-5
    beside torch's (the update body shared with hupr_adam_step_f32; it moves the parameters by < 1e-8) and is compared with the
    restatement only; parameters and exp_avg are compared with both."""
    ns, max_norm = (10007, 1025), 40.0
    p0 = [_rnd(n, 40 + i) for i, n in enumerate(ns)]
    z = lambda t: torch.zeros_like(t)
    # ours
    pa, ps = [t.cuda() for t in p0], [t.cuda() for t in p0]
    m, v, buf = [z(t) for t in pa], [z(t) for t in pa], [torch.empty_like(t) for t in pa]
    sa, ss = torch.tensor([1e-3, 0.0], device="cuda"), torch.tensor([LR, 0.0], device="cuda")
    ga, gs_ = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    partials = _new_partials(2)
    K = partials.numel() // 2
    # torch
    ta = [t.cuda().requires_grad_(True) for t in p0]
    ts = [t.cuda().requires_grad_(True) for t in p0]
    oa = torch.optim.Adam(ta, lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD)
    os_ = torch.optim.SGD(ts, lr=LR, momentum=MOM, weight_decay=WD)
    # fp64
    a64, s64 = [t.double() for t in p0], [t.double() for t in p0]
    m64, v64, b64 = [z(t) for t in a64], [z(t) for t in a64], None
    for step in range(1, 6):
        gr = [_rnd(n, 100 * step + i) for i, n in enumerate(ns)]
        gd = [t.cuda() for t in gr]
        for i in range(2):
            _sumsq(gd[i], partials[i * K:(i + 1) * K])
        _guard(partials, gscale, max_norm, sa, ga)
        _guard(partials, gscale, max_norm, ss, gs_)
        for i in range(2):
            _adam_guard(pa[i], gd[i], m[i], v[i], sa, ga, gscale)
            _sgd_guard(ps[i], gd[i], buf[i], ss, gs_, gscale)
        for params, opt in ((ta, oa), (ts, os_)):
            for t, g in zip(params, gd):
                t.grad = g * gscale
            torch.nn.utils.clip_grad_norm_(params, max_norm)
            opt.step()
        _, coef = _norm_coef64(gr, gscale, max_norm)
        assert 0.3 < coef < 0.9
        b1, b2, wd, eps, lra = f32(B1), f32(B2), f32(WD), f32(EPS), f32(1e-3)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        d_s = [g.double() * gscale * coef + WD * p for g, p in zip(gr, s64)]
        b64 = d_s if b64 is None else [MOM * b + d for b, d in zip(b64, d_s)]
        s64 = [p - LR * b for p, b in zip(s64, b64)]
        for i in range(2):
            d = gr[i].double() * gscale * coef + wd * a64[i]
            m64[i] = b1 * m64[i] + (1 - b1) * d
            v64[i] = b2 * v64[i] + (1 - b2) * d * d
            a64[i] = a64[i] - (lra / bc1) * m64[i] / (v64[i].sqrt() / math.sqrt(bc2) + eps)
    torch.cuda.synchronize()
    assert sa[1].item() == 5.0 and ss[1].item() == 5.0 and ga[2].item() == 0.0
    for i in range(2):
        close(pa[i], ta[i], 1e-6, "adam p vs torch")
        close(m[i], oa.state[ta[i]]["exp_avg"], 1e-6, "adam m vs torch")
        close(ps[i], ts[i], 1e-6, "sgd p vs torch")
        close(buf[i], os_.state[ts[i]]["momentum_buffer"], 1e-6, "sgd buf vs torch")
        close(pa[i], a64[i], 1e-6, "adam p vs fp64")
        close(m[i], m64[i], 1e-6, "adam m vs fp64")
        close(v[i], v64[i], 1e-6, "adam v vs fp64")
        close(ps[i], s64[i], 1e-6, "sgd p vs fp64")
        close(buf[i], b64[i], 1e-6, "sgd buf vs fp64")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [5, 10007])
def test_guarded_steps_write_nothing_when_the_gradient_was_not_finite(n, off):
    """finite = 0: parameters, optimiser state and the canaries around them keep their bits, for the aligned (float4) and the
    scalar launch alike, whatever the gradient holds."""
    names = ("pa", "m", "v", "ps", "buf")
    big = {k: torch.full((n + 8,), CANARY, device="cuda") for k in names}
    for i, k in enumerate(names):
        big[k][off:off + n].copy_(_rnd(n, 60 + i))
    before = {k: t.clone() for k, t in big.items()}
    view = {k: t[off:off + n] for k, t in big.items()}
    g = _rnd(n, 70).cuda()
    g[n // 2] = float("nan")
    state = torch.tensor([LR, 3.0], device="cuda")
    guard = torch.tensor([0.0, INF, 1.0, 0.0], device="cuda")
    _adam_guard(view["pa"], g, view["m"], view["v"], state, guard)
    _sgd_guard(view["ps"], g, view["buf"], state, guard)
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(big[k].view(torch.int32), before[k].view(torch.int32)), k
    assert state.tolist() == [f32(LR), 3.0] and guard.tolist() == [0.0, INF, 1.0, 0.0]


def test_guard_entries_refuse_bad_arguments_before_any_launch():
    rt, L = _lib()
    t = torch.zeros(16, device="cuda")
    d = torch.zeros(L.hupr_grad_sumsq_partials(), dtype=torch.float64, device="cuda")
    a, pd, s = rt.ptr(t), rt.ptr(d), rt.stream()
    before = L.hupr_launch_count()
    for g, n, p in [(None, 16, pd), (a, 16, None), (a, 0, pd), (a, -4, pd), (a + 2, 8, pd), (a, 16, pd + 4)]:
        assert L.hupr_grad_sumsq_f32(g, n, p, s) == -1
        assert b"hupr_grad_sumsq_f32" in L.hupr_last_error()
    for p, count, max_norm, st, gd in [(None, 4, 1.0, a, a), (pd, 4, 1.0, None, a), (pd, 4, 1.0, a, None), (pd, 0, 1.0, a, a),
                                       (pd, -1, 1.0, a, a), (pd, 4, 0.0, a, a), (pd, 4, -1.0, a, a), (pd, 4, float("nan"), a, a)]:
        assert L.hupr_grad_guard_f32(p, count, 1.0, max_norm, st, gd, s) == -1
        assert b"hupr_grad_guard_f32" in L.hupr_last_error()
    for i in range(6):                                               # p, g, exp_avg, exp_avg_sq, dev_state, guard
        ptrs = [None if j == i else a for j in range(6)]
        assert L.hupr_adam_step_guard_f32(*ptrs[:4], 16, ptrs[4], ptrs[5], B1, B2, EPS, WD, 1.0, s) == -1
        assert b"hupr_adam_step_guard_f32" in L.hupr_last_error()
    for i in range(5):                                               # p, g, momentum_buf, dev_state, guard
        ptrs = [None if j == i else a for j in range(5)]
        assert L.hupr_sgd_step_guard_f32(*ptrs[:3], 16, ptrs[3], ptrs[4], MOM, WD, 1.0, s) == -1
        assert b"hupr_sgd_step_guard_f32" in L.hupr_last_error()
    for n in (0, -4):
        assert L.hupr_adam_step_guard_f32(a, a, a, a, n, a, a, B1, B2, EPS, WD, 1.0, s) == -1
        assert L.hupr_sgd_step_guard_f32(a, a, a, n, a, a, MOM, WD, 1.0, s) == -1
    assert L.hupr_launch_count() == before
    torch.cuda.synchronize()
    assert bool((t == 0).all()) and bool((d == 0).all())


# ---- the engine with TRAINING.gradClip (bf16, B = 2 synthetic cubes) --------------------------------------------------------
def _setup(optimizer, clip=None, B=2, seed=51):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    cfg.TRAINING.optimizer = optimizer
    if clip is not None:
        cfg.TRAINING.gradClip = clip
    dev = torch.device("cuda", 0)
    G = cfg.DATASET.numGroupFrames
    adc_h = torch.from_numpy(synth.adc_cube_int16(seed, sensor=0, nframes=B * G)).to(dev)
    adc_v = torch.from_numpy(synth.adc_cube_int16(seed, sensor=1, nframes=B * G)).to(dev)
    joints = torch.from_numpy(synth.keypoints(B, seed + 1)).to(dev)
    return cfg, dev, (adc_h, adc_v, joints)


def _engine(optimizer, clip=None, seed=51):
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, batch = _setup(optimizer, clip, seed=seed)
    return TrainEngine(cfg, device=dev, seed=0), batch


def _flat(eng):
    return torch.cat([p.detach().flatten() for p in eng.model.parameters()])


def _state(eng):
    """Every flat optimiser state tensor, in bucket order."""
    return [st[k] for st in eng.optimizer._flat_state for k in eng.optimizer._state_keys]


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture
def bf16():
    from hupr_amd import functional as F_
    F_.set_math("bf16")
    yield F_
    F_.set_math("f32")


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_engine_guard_only_is_the_unguarded_step_bit_for_bit(optimizer, bf16):
    """gradClip = inf: 3 steps land on the bits of an engine without the key whose optimiser keeps {lr, step} on the device;
    the reported norm is the fp64 norm of the flat gradients times grad_scale, nothing is skipped."""
    e0, batch = _engine(optimizer, seed=61)
    assert e0.optimizer._guard is None and e0.guard_stats() is None
    e0.optimizer.use_device_state()
    e1, _ = _engine(optimizer, INF, seed=61)
    assert e1.optimizer._guard is not None and e1.optimizer._guard_max_norm == INF
    for _ in range(3):
        l0, _ = e0.train_step_from_adc(*batch)
        l1, _ = e1.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    assert float(l0.detach()) == float(l1.detach())
    assert torch.equal(_flat(e0), _flat(e1))
    for a, b in zip(_state(e0), _state(e1)):
        assert torch.equal(a, b)
    stats = e1.guard_stats()
    nref, _ = _norm_coef64([g for _, g in e1.optimizer._flat], e1.optimizer.grad_scale, INF)
    print("%s: norm %.9g (fp64 %.17g)" % (optimizer, stats["norm"], nref))
    assert set(stats) == {"norm", "coef", "skipped"}
    assert ulps(stats["norm"], f32(nref)) <= 1 and stats["coef"] == 1.0 and stats["skipped"] == 0
    assert e1.optimizer._host_step(0) == 3 and e0.optimizer._host_step(0) == 3


def test_engine_clipped_first_sgd_step(bf16):
    """gradClip = half the first gradient's norm: every bucket's momentum buffer is g gscale coef + wd p0 in fp64."""
    e0, batch = _engine("sgd", seed=63)
    e0.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    n0, _ = _norm_coef64([g for _, g in e0.optimizer._flat], e0.optimizer.grad_scale, INF)
    assert n0 > 0 and math.isfinite(n0)
    e1, _ = _engine("sgd", n0 / 2, seed=63)
    opt = e1.optimizer
    before = [p.clone() for p, _ in opt._flat]
    e1.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    for (_, g0), (_, g1) in zip(e0.optimizer._flat, opt._flat):
        assert torch.equal(g0, g1)                                   # same weights, same data: the same first gradient
    _, cref = _norm_coef64([g for _, g in opt._flat], opt.grad_scale, f32(n0 / 2))
    stats = e1.guard_stats()
    print("norm %.9g (fp64 %.17g), coef %.9g (fp64 %.17g)" % (stats["norm"], n0, stats["coef"], cref))
    assert ulps(stats["norm"], f32(n0)) <= 1 and ulps(stats["coef"], f32(cref)) <= 1 and 0.49 < cref < 0.51
    lr = opt.param_groups[0]["lr"]
    for (p, g), st, p0 in zip(opt._flat, opt._flat_state, before):
        buf = st["momentum_buffer"]
        close(buf, g.double() * opt.grad_scale * cref + WD * p0.double(), 1e-6, "buffer")
        close(p, p0.double() - lr * buf.double(), 1e-6, "parameters")
        assert not torch.equal(p, p0)
    assert opt._host_step(0) == 1


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_engine_skips_a_non_finite_step(optimizer, bf16):
    """A good step, then one whose backward is seeded with inf: parameters, optimiser state and step count keep their bits and
    skipped == 1; the next good step lands where a twin lands that took only the two good steps."""
    eng, batch = _engine(optimizer, INF, seed=65)
    eng.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    p1, s1 = _flat(eng).clone(), [t.clone() for t in _state(eng)]
    eng._seed.fill_(INF)
    eng.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    stats = eng.guard_stats()
    assert not all(bool(torch.isfinite(g).all()) for _, g in eng.optimizer._flat)      # the bad values did reach the buckets
    assert stats["skipped"] == 1 and stats["coef"] == 0.0 and not math.isfinite(stats["norm"])
    assert _bits_equal(_flat(eng), p1)
    for a, b in zip(_state(eng), s1):
        assert _bits_equal(a, b)
    assert eng.optimizer._host_step(0) == 1
    eng._seed.fill_(1.0)
    eng.train_step_from_adc(*batch)
    twin, _ = _engine(optimizer, INF, seed=65)
    for _ in range(2):
        twin.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(_flat(eng)).all())
    assert torch.equal(_flat(eng), _flat(twin))
    for a, b in zip(_state(eng), _state(twin)):
        assert torch.equal(a, b)
    assert eng.optimizer._host_step(0) == 2 and eng.guard_stats()["skipped"] == 1 and twin.guard_stats()["skipped"] == 0


def test_engine_guard_replays_inside_the_graph(bf16):
    """Eager: ok, ok, skip, ok.  Graph: ok, capture (1 warm-up step), a replay with the inf seed, a replay.  Bit-equal: the guard,
    the step count and the decision all live on the device."""
    def run(graph):
        eng, batch = _engine("adam", 1.0, seed=67)
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
    assert bool(torch.isfinite(_flat(e2)).all())
    assert torch.equal(_flat(e1), _flat(e2))
    for a, b in zip(_state(e1), _state(e2)):
        assert torch.equal(a, b)
    for eng in (e1, e2):
        assert eng.optimizer._host_step(0) == 3 and eng.guard_stats()["skipped"] == 1
    assert e1.guard_stats() == e2.guard_stats()


def test_engine_guard_with_single_rank_collective_is_bit_transparent(monkeypatch, bf16):
    """HUPR_FORCE_ALLREDUCE=1 on one compute stream (every bucket through hupr_allreduce_bucket on a single-rank communicator,
    joined before the norm is taken) and the guard clipping: 3 SGD steps == 3 steps without any collective, bit for bit."""
    saved = bf16.TWO_STREAMS
    try:
        bf16.TWO_STREAMS = False
        monkeypatch.delenv("HUPR_FORCE_ALLREDUCE", raising=False)
        e0, batch = _engine("sgd", 1.0, seed=69)
        assert not e0.buckets.active
        monkeypatch.setenv("HUPR_FORCE_ALLREDUCE", "1")
        e1, _ = _engine("sgd", 1.0, seed=69)
        assert e1.buckets.active and e1.buckets.transport.name.startswith("rccl"), e1.buckets.transport.name
        for _ in range(3):
            l0, _ = e0.train_step_from_adc(*batch)
            l1, _ = e1.train_step_from_adc(*batch)
        torch.cuda.synchronize()
        assert float(l0.detach()) == float(l1.detach())
        assert torch.equal(_flat(e0), _flat(e1))
        for a, b in zip(_state(e0), _state(e1)):
            assert torch.equal(a, b)
        assert e0.guard_stats() == e1.guard_stats() and e0.guard_stats()["skipped"] == 0
        e1.buckets.transport.close()
    finally:
        bf16.TWO_STREAMS = saved


def test_main_train_resume_eval_with_grad_clip(tmp_path, monkeypatch):
    """main.py with TRAINING.gradClip: 1.0 — trains, checkpoints torch.optim.Adam's state with the step count the guard kernel
    kept on the device, resumes from it and evaluates."""
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"]["dataDir"] = "synthetic"
    cfgd["TRAINING"]["batchSize"] = 2
    cfgd["TRAINING"]["epochs"] = 1
    cfgd["TRAINING"]["gradClip"] = 1.0
    cfgd["TEST"]["batchSize"] = 2
    (tmp_path / "config").mkdir()
    yaml.safe_dump(cfgd, open(tmp_path / "config" / "tiny.yaml", "w"))
    (tmp_path / "logs").mkdir()
    (tmp_path / "visualization").mkdir()
    monkeypatch.chdir(tmp_path)
    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--max_steps", "2"])
    run = tmp_path / "logs" / "run0"
    osd = torch.load(run / "checkpoint.pth")["optimizer_state_dict"]
    assert len(osd["state"]) == len(osd["param_groups"][0]["params"])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 2.0 for s in osd["state"].values())
    assert all(bool(torch.isfinite(s["exp_avg"]).all()) for s in osd["state"].values())
    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--max_steps", "1"])   # resumes
    osd2 = torch.load(run / "checkpoint.pth")["optimizer_state_dict"]
    assert all(float(s["step"]) == 3.0 for s in osd2["state"].values())
    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--eval"])
    assert len(json.load(open(run / "test_results.json"))) == 4
