"""GPU (-m gpu): TRAINING.optimizer = lamb — the three LAMB launches over a flat bucket (hupr_lamb_stage1_f32, hupr_lamb_ratio_f32,
hupr_lamb_stage2_f32) against a float64 restatement of the rule, then the engine, graph capture, checkpoint resume, the gradient
guard, the collective, accumulation and main.py with it.

The rule, per parameter tensor (a segment of the bucket), k the 1-based step count, g' = g * gscale * coef:
    m <- b1 m + (1 - b1) g'          v <- b2 v + (1 - b2) g'^2
    d = (m / (1 - b1^k)) / (sqrt(v) / sqrt(1 - b2^k) + eps)
    adapted:  u = d + wd p,  r = |p| / |u| if both norms > 0 else 1;      not adapted:  u = d,  r = 1;      p <- p - lr r u
with b = (0.9, 0.999), eps = 1e-6.  New, no reference counterpart."""
import json
import math
import os

import pytest
import torch
import yaml

from hupr_amd import synth

pytestmark = pytest.mark.gpu
B1, B2, EPS = 0.9, 0.999, 1e-6
LR, WD, GSCALE, STEPS = 1e-2, 0.01, 0.5, 3
INF = float("inf")


def _rnd(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _chunk():
    from hupr_amd import runtime as rt
    return rt.lib().hupr_lamb_chunk()


def _segments(lengths, adapted):
    out, at = [], 0
    for n, a in zip(lengths, adapted):
        out.append((at, n, a))
        at += n
    return out


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------
def rule(dtype, segments, p0, grads, lr=LR, wd=WD, gscale=GSCALE, coef=1.0):
    """The rule in ``dtype`` on the CPU.  -> per step (p, m, v, stats), stats = (S, 3) float64 rows (|p|, |u|, r)."""
    p, m, v = p0.to(dtype), torch.zeros_like(p0, dtype=dtype), torch.zeros_like(p0, dtype=dtype)
    out = []
    for k, g in enumerate(grads, 1):
        gp = g.to(dtype) * (gscale * coef)
        m = B1 * m + (1 - B1) * gp
        v = B2 * v + (1 - B2) * gp * gp
        d = (m / (1 - B1 ** k)) / (v.sqrt() / math.sqrt(1 - B2 ** k) + EPS)
        new, stats = p.clone(), []
        for start, n, adapted in segments:
            ps, ds = p[start:start + n], d[start:start + n]
            u = ds + wd * ps if adapted else ds
            pn, un = ps.norm(), u.norm()
            r = pn / un if adapted and pn > 0 and un > 0 else torch.ones((), dtype=dtype)
            new[start:start + n] = ps - lr * r * u
            stats.append([float(pn), float(un), float(r)])
        p = new
        out.append((p.clone(), m.clone(), v.clone(), torch.tensor(stats, dtype=torch.float64)))
    return out


# ---- the kernels through the C ABI ----------------------------------------------------------------------------------------------
def lamb(segments, p0, grads, lr=LR, wd=WD, gscale=GSCALE, guard=None, shift=0, shift_g=None, seed_state=None):
    """``len(grads)`` LAMB steps over one bucket.  shift / shift_g: element offset of p, m, v / of g inside larger canary-filled
    buffers.  guard: None or the 4 floats.  seed_state: (p, m, v, stats) bits to start from instead of (p0, 0, 0, 0).
    -> per step (p, m, v, stats (3, S)) on the CPU."""
    from hupr_amd import runtime as rt
    from hupr_amd.tools.optim import lamb_chunk_table
    L, s = rt.lib(), rt.stream()
    n = p0.numel()
    canary = -12345.5
    shift_g = shift if shift_g is None else shift_g
    big = {k: torch.full((n + 8,), canary, device="cuda") for k in "pgmv"}
    off = {"p": shift, "m": shift, "v": shift, "g": shift_g}
    view = {k: big[k][off[k]:off[k] + n] for k in big}
    assert all(view[k].data_ptr() % 16 == 4 * (off[k] % 4) for k in view)
    host = torch.tensor(lamb_chunk_table(segments, L.hupr_lamb_chunk()), dtype=torch.int64)
    dev = host.cuda()
    S, K = int(host[0]), int(host[1])
    partials = torch.zeros(2 * K, dtype=torch.float64, device="cuda")
    stats = torch.zeros(3 * S, device="cuda")
    view["p"].copy_(p0)
    view["m"].zero_()
    view["v"].zero_()
    if seed_state is not None:
        for k, t in zip("pmv", seed_state[:3]):
            view[k].copy_(t)
        stats.copy_(seed_state[3].reshape(-1))
    state = torch.zeros(2, device="cuda")
    gd = None if guard is None else torch.tensor(guard, dtype=torch.float32, device="cuda")
    table = (host.data_ptr(), host.numel(), rt.ptr(dev))
    out = []
    for k, g in enumerate(grads, 1):
        view["g"].copy_(g)
        state.copy_(torch.tensor([lr, float(k)]))
        rt.check(L.hupr_lamb_stage1_f32(rt.ptr(view["p"]), rt.ptr(view["g"]), rt.ptr(view["m"]), rt.ptr(view["v"]), n, *table,
                                        rt.ptr(state), rt.ptr(gd), B1, B2, EPS, wd, gscale, rt.ptr(partials), s))
        rt.check(L.hupr_lamb_ratio_f32(rt.ptr(partials), n, *table, rt.ptr(gd), rt.ptr(stats), s))
        rt.check(L.hupr_lamb_stage2_f32(rt.ptr(view["p"]), rt.ptr(view["m"]), rt.ptr(view["v"]), n, *table, rt.ptr(state),
                                        rt.ptr(gd), B1, B2, EPS, wd, rt.ptr(stats), s))
        out.append(tuple(view[k].cpu() for k in "pmv") + (stats.view(3, S).cpu(),))
    torch.cuda.synchronize()
    for k, t in big.items():                                # nothing outside the bucket was written
        assert bool((torch.cat([t[:off[k]], t[off[k] + n:]]) == canary).all()), k
    return out


def _ulp(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


@pytest.fixture(scope="module")
def big():
    """The hand-built bucket of the kernel tests: inputs, the float64 rule, the float32 rule and one run of the kernels."""
    C = _chunk()
    lengths = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C, 2 * C + 3, 10007]
    segments = _segments(lengths, [i % 2 == 0 for i in range(len(lengths))])
    assert segments[0][2] and segments[8][1] == 2 * C + 3 and segments[8][2]
    n = sum(lengths)
    p0 = 0.1 * _rnd(n, 1)
    grads = [_rnd(n, 10 + k) * 10.0 ** -k for k in range(STEPS)]
    return dict(segments=segments, p0=p0, grads=grads, r64=rule(torch.float64, segments, p0, grads),
                r32=rule(torch.float32, segments, p0, grads), got=lamb(segments, p0, grads))


def test_three_steps_agree_with_the_float64_rule(big):
    """Per tensor and per array x of p, m, v, after each of the 3 steps: |kernel - fp64| <= max(4 d32, 2 ulp of max|p|), d32 the
    largest deviation of the float32 restatement from float64 on that tensor and array, max|p| that tensor's largest parameter.
    (The factor 4: the device's fused multiply-adds and division order differ from torch's.  On the MI355X the kernel sat on the
    float32 restatement's own deviation, or below it, for nearly every tensor.)
    The stored ratios agree to 1e-5 relative; an adapted tensor moves by lr |p|: |dp| / (lr |p_before|) = 1 to 1e-5."""
    worst = 0.0
    before = big["p0"].double()
    for k in range(STEPS):
        got, r64, r32 = big["got"][k], big["r64"][k], big["r32"][k]
        for s, (start, n, adapted) in enumerate(big["segments"]):
            sl = slice(start, start + n)
            pmax = r64[0][sl].abs().max().item()
            for name, x, x64, x32 in zip("pmv", got[:3], r64[:3], r32[:3]):
                d32 = (x32[sl].double() - x64[sl]).abs().max().item()
                err = (x[sl].double() - x64[sl]).abs().max().item()
                tol = max(4 * d32, 2 * _ulp(pmax))
                worst = max(worst, err / tol)
                print("step %d segment %d (n = %d) %s: err %.3e  d32 %.3e  tol %.3e" % (k + 1, s, n, name, err, d32, tol))
                assert err <= tol, (k + 1, s, name, err, d32, tol)
            ref = r64[3][s]
            stats = got[3][:, s].double()
            print("step %d segment %d: |p| %.9g |u| %.9g r %.9g (fp64 %.12g %.12g %.12g)" % ((k + 1, s) + tuple(stats.tolist()) + tuple(ref.tolist())))
            assert ((stats - ref).abs() <= 1e-5 * ref.abs()).all(), (k + 1, s, stats, ref)
            if not adapted:
                assert stats[2] == 1.0
            elif ref[0] > 0 and ref[1] > 0:
                moved = (got[0][sl].double() - before[sl]).norm().item() / (LR * before[sl].norm().item())
                print("step %d segment %d: |dp| / (lr |p|) = %.9g" % (k + 1, s, moved))
                assert abs(moved - 1.0) <= 1e-5, (k + 1, s, moved)
        before = got[0].double()
    print("worst err / tol %.3f" % worst)


# -- degenerate tensors: one bucket, the special segment between two normal ones
def _degenerate(p_mid, g_mid, adapted, wd):
    n = 37
    segments = _segments([n, n, n], [True, adapted, False])
    p0 = 0.1 * _rnd(3 * n, 3)
    g = _rnd(3 * n, 4)
    if p_mid is not None:
        p0[n:2 * n] = p_mid
    if g_mid is not None:
        g[n:2 * n] = g_mid
    got = lamb(segments, p0, [g], wd=wd)[0]
    ref = rule(torch.float64, segments, p0, [g], wd=wd)[0]
    for name, x, x64 in zip("pmv", got[:3], ref[:3]):
        err = (x.double() - x64).abs().max().item()
        assert err <= 1e-6 * x64.abs().max().item(), (name, err)
    assert ((got[3].double().T - ref[3]).abs() <= 1e-5 * ref[3].abs()).all()
    return p0[n:2 * n], got[0][n:2 * n], got[3][:, 1]


def test_an_adapted_tensor_of_zeros_has_ratio_one():
    p0, p1, stats = _degenerate(0.0, None, True, WD)
    assert stats[0] == 0.0 and stats[1] > 0 and stats[2] == 1.0
    assert bool((p1 != 0).all())                            # it moves by lr u, Adam's step


def test_an_adapted_tensor_with_zero_gradient_has_ratio_one_over_wd():
    p0, p1, stats = _degenerate(None, 0.0, True, WD)
    assert abs(stats[2].item() * WD - 1.0) <= 1e-5 and stats[0] > 0
    assert ((p1.double() - p0.double() * (1 - LR)).abs() <= 1e-6 * p0.abs().max().item()).all()      # u = wd p, r = 1 / wd


def test_zero_gradient_and_zero_decay_keep_the_bits():
    p0, p1, stats = _degenerate(None, 0.0, True, 0.0)
    assert stats[1] == 0.0 and stats[2] == 1.0 and stats[0] > 0
    assert _bits_equal(p0, p1)


def test_a_tensor_that_is_not_adapted_takes_adams_step():
    """Against torch.optim.Adam(eps=1e-6, weight_decay=0) on the GPU, 3 steps, to 1e-6 of the scale (test_adam_step_matches_torch's
    gate)."""
    n = 10007
    segments = [(0, n, False)]
    p0 = 0.1 * _rnd(n, 5)
    grads = [_rnd(n, 20 + k) * 10.0 ** -k for k in range(STEPS)]
    pt = p0.cuda().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0)
    for g in grads:
        pt.grad = g.cuda()
        opt.step()
    got = lamb(segments, p0, grads, gscale=1.0)
    ref = rule(torch.float64, segments, p0, grads, gscale=1.0)
    for name, x, xt, x64 in zip("pmv", got[-1][:3], (pt.detach(), opt.state[pt]["exp_avg"], opt.state[pt]["exp_avg_sq"]), ref[-1][:3]):
        for what, y in (("torch", xt.cpu().double()), ("fp64", x64)):
            err = (x.double() - y).abs().max().item()
            assert err <= 1e-6 * y.abs().max().item(), (name, what, err)
    assert all(step[3][2, 0] == 1.0 for step in got)


def test_every_segment_alone_gives_the_bits_it_gets_in_the_bucket(big):
    """A norm that leaks over a tensor boundary, or a chunk that straddles one, shows here: p, m, v and r of every segment run as a
    bucket of its own equal its bits inside the big bucket."""
    for s, (start, n, adapted) in enumerate(big["segments"]):
        sl = slice(start, start + n)
        alone = lamb([(0, n, adapted)], big["p0"][sl].clone(), [g[sl].clone() for g in big["grads"]])
        for k in range(STEPS):
            for name, x, y in zip("pmv", alone[k][:3], big["got"][k][:3]):
                assert _bits_equal(x, y[sl]), (s, k + 1, name)
            assert _bits_equal(alone[k][3][:, 0], big["got"][k][3][:, s]), (s, k + 1, alone[k][3][:, 0], big["got"][k][3][:, s])


@pytest.mark.parametrize("only_g", [False, True])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_a_shifted_bucket_gives_the_same_bits(big, shift, only_g):
    got = lamb(big["segments"], big["p0"], big["grads"], shift=0 if only_g else shift, shift_g=shift)
    for k in range(STEPS):
        for name, x, y in zip("pmvs", got[k], big["got"][k]):
            assert _bits_equal(x, y), (k + 1, name)


def test_two_runs_are_bit_identical(big):
    again = lamb(big["segments"], big["p0"], big["grads"])
    for k in range(STEPS):
        for x, y in zip(again[k], big["got"][k]):
            assert torch.equal(x, y)


def test_a_skipped_step_writes_nothing(big):
    """guard = {0, ., ., 0}: p, m, v and the three per-segment arrays keep their bits, whatever the gradient holds."""
    start = big["got"][1]
    bad = big["grads"][2].clone()
    bad[::7] = INF
    got = lamb(big["segments"], big["p0"], [bad], guard=[0.0, INF, 1.0, 0.0], seed_state=start)[0]
    for name, x, y in zip("pmvs", got, start):
        assert _bits_equal(x, y), name


def test_the_guards_coefficient_is_a_gradient_scale(big):
    """guard[0] = 0.5 with gscale = 1 is gscale = 0.5 without a guard, bit for bit."""
    got = lamb(big["segments"], big["p0"], big["grads"], gscale=1.0, guard=[0.5, 1.0, 0.0, 1.0])
    for k in range(STEPS):
        for name, x, y in zip("pmvs", got[k], big["got"][k]):
            assert _bits_equal(x, y), (k + 1, name)


def test_lamb_entries_refuse_bad_arguments_before_any_launch():
    from hupr_amd import runtime as rt
    from hupr_amd.tools.optim import lamb_chunk_table
    L, s = rt.lib(), rt.stream()
    C = L.hupr_lamb_chunk()
    n = C + 6
    t = torch.zeros(n, device="cuda")
    part = torch.zeros(8, dtype=torch.float64, device="cuda")
    stats = torch.zeros(6, device="cuda")
    state = torch.tensor([LR, 1.0], device="cuda")
    good = lamb_chunk_table([(0, 5, True), (5, C + 1, False)], C)
    gap, overlap, past = list(good), list(good), list(good)
    gap[4 + 5] = 6
    overlap[4 + 5] = 4
    past[4 + 5 + 1] = C + 2
    host = torch.tensor(good, dtype=torch.int64)
    dev = host.cuda()
    a, st, pp, ss, h, d, w = rt.ptr(t), rt.ptr(state), rt.ptr(part), rt.ptr(stats), host.data_ptr(), rt.ptr(dev), host.numel()
    torch.cuda.synchronize()
    before = L.hupr_launch_count()

    def stage1(p=a, g=a, m=a, v=a, n=n, h=h, w=w, d=d, st=st, pp=pp):
        return L.hupr_lamb_stage1_f32(p, g, m, v, n, h, w, d, st, None, B1, B2, EPS, WD, 1.0, pp, s)

    def ratio(pp=pp, n=n, h=h, w=w, d=d, ss=ss):
        return L.hupr_lamb_ratio_f32(pp, n, h, w, d, None, ss, s)

    def stage2(p=a, m=a, v=a, n=n, h=h, w=w, d=d, st=st, ss=ss):
        return L.hupr_lamb_stage2_f32(p, m, v, n, h, w, d, st, None, B1, B2, EPS, WD, ss, s)
    calls = [("hupr_lamb_stage1_f32", stage1, ["p", "g", "m", "v", "h", "d", "st", "pp"]),
             ("hupr_lamb_ratio_f32", ratio, ["pp", "h", "d", "ss"]),
             ("hupr_lamb_stage2_f32", stage2, ["p", "m", "v", "h", "d", "st", "ss"])]
    for name, fn, pointers in calls:
        for k in pointers:
            assert fn(**{k: None}) == -1 and name.encode() in L.hupr_last_error(), (name, k)
        for bad_n in (0, -4):
            assert fn(n=bad_n) == -1 and name.encode() in L.hupr_last_error(), (name, bad_n)
        if "pp" in pointers:
            assert fn(pp=pp + 4) == -1 and b"aligned" in L.hupr_last_error(), name
        for table, word in ((gap, b"gap"), (overlap, b"overlap"), (past, b"past n")):      # finite tables, the host-side check
            bad = torch.tensor(table, dtype=torch.int64)
            assert fn(h=bad.data_ptr()) == -1, (name, word)
            assert name.encode() in L.hupr_last_error() and word in L.hupr_last_error(), L.hupr_last_error()
            assert L.hupr_lamb_table_check(bad.data_ptr(), bad.numel(), n) == -1 and word in L.hupr_last_error()
        assert fn(n=n + 1) == -1 and fn(w=w - 1) == -1, name
    assert L.hupr_launch_count() == before
    torch.cuda.synchronize()
    assert bool((t == 0).all()) and bool((part == 0).all()) and bool((stats == 0).all())


# ---- the engine with TRAINING.optimizer = lamb (bf16, B = 2 synthetic cubes) -----------------------------------------------------
def _setup(seed=51, B=2, **training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    cfg.TRAINING.optimizer = "lamb"
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    dev = torch.device("cuda", 0)
    G = cfg.DATASET.numGroupFrames
    adc_h = torch.from_numpy(synth.adc_cube_int16(seed, sensor=0, nframes=B * G)).to(dev)
    adc_v = torch.from_numpy(synth.adc_cube_int16(seed, sensor=1, nframes=B * G)).to(dev)
    joints = torch.from_numpy(synth.keypoints(B, seed + 1)).to(dev)
    return cfg, dev, (adc_h, adc_v, joints)


def _flat(eng):
    return torch.cat([p.detach().flatten() for p in eng.model.parameters()])


def _state(eng):
    return [st[k] for st in eng.optimizer._flat_state for k in eng.optimizer._state_keys]


def _ratios(eng):
    return [st["lamb"]["stats"] for st in eng.optimizer._flat_state]


@pytest.fixture
def bf16():
    from hupr_amd import functional as F_
    F_.set_math("bf16")
    yield F_
    F_.set_math("f32")


def test_engine_first_lamb_step(bf16):
    """From the parameters before and the gradients after: every parameter tensor, its moments and its (|p|, |u|, r) follow the
    float64 rule (1e-6 of the tensor's scale; 1e-5 relative for the norms and ratios); ndim <= 1 means r == 1."""
    from hupr_amd.tools.engine import TrainEngine
    from hupr_amd.tools.optim import FusedLAMB
    cfg, dev, batch = _setup(seed=91)
    eng = TrainEngine(cfg, device=dev, seed=0)
    opt = eng.optimizer
    assert type(opt) is FusedLAMB and opt._dev_state is not None
    group = {k: v for k, v in opt.param_groups[0].items() if k != "params"}
    assert group == dict(lr=cfg.TRAINING.lr, betas=(B1, B2), eps=EPS, weight_decay=0.01, trust_ratio=True)
    assert eng.guard_stats() is None
    lr = group["lr"]
    before = [p.clone() for p, _ in opt._flat]
    eng.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    stats = eng.lamb_stats()
    names = {id(p): name for name, p in eng.model.named_parameters()}
    assert sorted(stats) == sorted(names.values()) and opt._host_step(0) == 1
    adapted = 0
    for (p, g), st, p0, entries in zip(opt._flat, opt._flat_state, before, eng.buckets.layout()):
        segments = [(off, n, q.ndim > 1) for q, off, n in entries]
        ref = rule(torch.float64, segments, p0.cpu(), [g.cpu()], lr=lr, wd=0.01, gscale=opt.grad_scale)[0]
        for (q, off, n), row in zip(entries, ref[3]):
            sl = slice(off, off + n)
            for name, x, x64 in (("p", p, ref[0]), ("m", st["exp_avg"], ref[1]), ("v", st["exp_avg_sq"], ref[2])):
                err = (x[sl].cpu().double() - x64[sl]).abs().max().item()
                assert err <= 1e-6 * (x64[sl].abs().max().item() + 1e-30), (names[id(q)], name, err)
            got = torch.tensor(stats[names[id(q)]], dtype=torch.float64)
            assert ((got - row).abs() <= 1e-5 * row.abs()).all(), (names[id(q)], got, row)
            assert q.ndim > 1 or got[2] == 1.0
            adapted += q.ndim > 1
        assert not torch.equal(p, p0)
    assert 0 < adapted < len(stats)


def test_engine_lamb_loss_falls(bf16):
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, batch = _setup(seed=93)
    eng = TrainEngine(cfg, device=dev, seed=0, lr=1e-2)
    losses = [float(eng.train_step_from_adc(*batch)[0]) for _ in range(10)]
    print(losses)
    assert losses[-1] < losses[0], losses
    assert bool(torch.isfinite(_flat(eng)).all())


def test_engine_lamb_graph_replay_equals_eager_steps(bf16):
    """5 eager steps == 2 eager + capture (1 warm-up) + 2 replays, bit for bit, with the learning rate halved after step 3."""
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, batch = _setup(seed=95)

    def halve(eng):
        for group in eng.optimizer.param_groups:
            group["lr"] *= 0.5
    e1 = TrainEngine(cfg, device=dev, seed=0)
    for s in range(5):
        if s == 3:
            halve(e1)
        e1.train_step_from_adc(*batch)
    e2 = TrainEngine(cfg, device=dev, seed=0)
    for _ in range(2):
        e2.train_step_from_adc(*batch)
    e2.capture(*batch, warmup=1)
    halve(e2)
    e2.sync_lr()
    for _ in range(2):
        e2.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    assert e2.optimizer._host_step(0) == 5 and e1.optimizer._host_step(0) == 5
    assert torch.equal(_flat(e1), _flat(e2))
    for a, b in zip(_state(e1) + _ratios(e1), _state(e2) + _ratios(e2)):
        assert torch.equal(a, b)


def test_engine_lamb_checkpoint_resume_is_bit_exact(tmp_path, bf16):
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, batch = _setup(seed=97)
    e1 = TrainEngine(cfg, device=dev, seed=0)
    for _ in range(2):
        e1.train_step_from_adc(*batch)
    torch.save({"model_state_dict": e1.model.state_dict(), "optimizer_state_dict": e1.optimizer.state_dict()}, tmp_path / "checkpoint.pth")
    e1.train_step_from_adc(*batch)
    n_params = sum(1 for _ in e1.model.parameters())
    ck = torch.load(tmp_path / "checkpoint.pth", map_location="cuda")
    st = ck["optimizer_state_dict"]["state"]
    assert len(st) == n_params and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 2.0 for s in st.values())
    assert ck["optimizer_state_dict"]["param_groups"][0]["trust_ratio"] is True
    e2 = TrainEngine(cfg, device=dev, seed=123)              # different init on purpose
    e2.model.load_state_dict(ck["model_state_dict"])
    e2.optimizer.load_state_dict(ck["optimizer_state_dict"])
    bf16.invalidate_packed()
    e2.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    assert e2.optimizer._host_step(0) == 3
    assert torch.equal(_flat(e1), _flat(e2))
    for a, b in zip(_state(e1), _state(e2)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ema", [False, True])
def test_engine_lamb_skips_a_non_finite_step(ema, bf16):
    """gradClip = inf: a good step, then one whose backward is seeded with inf.  Parameters, moments, step count and trust ratios
    keep their bits and skipped == 1; with TRAINING.emaDecay the average does not move either."""
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, batch = _setup(seed=65, gradClip=INF, **({"emaDecay": 0.9} if ema else {}))
    eng = TrainEngine(cfg, device=dev, seed=0)
    assert (eng.ema is not None) == ema
    eng.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    keep = [t.clone() for t in [_flat(eng)] + _state(eng) + _ratios(eng) + (eng.ema.flat if ema else [])]
    assert all(bool((r.view(3, -1)[2] > 0).all()) for r in _ratios(eng))
    eng._seed.fill_(INF)
    eng.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    stats = eng.guard_stats()
    assert not all(bool(torch.isfinite(g).all()) for _, g in eng.optimizer._flat)      # the bad values did reach the buckets
    assert stats["skipped"] == 1 and stats["coef"] == 0.0
    now = [_flat(eng)] + _state(eng) + _ratios(eng) + (eng.ema.flat if ema else [])
    for a, b in zip(now, keep):
        assert _bits_equal(a, b)
    assert eng.optimizer._host_step(0) == 1
    if ema:
        assert eng.ema_stats()["updates"] == 1
    eng._seed.fill_(1.0)
    eng.train_step_from_adc(*batch)
    torch.cuda.synchronize()
    assert eng.optimizer._host_step(0) == 2 and bool(torch.isfinite(_flat(eng)).all()) and not _bits_equal(_flat(eng), keep[0])


def test_engine_lamb_rccl_exchange_single_rank_is_bit_transparent(monkeypatch, bf16):
    from hupr_amd.tools.engine import TrainEngine
    saved = bf16.TWO_STREAMS
    try:
        bf16.TWO_STREAMS = False
        cfg, dev, batch = _setup(seed=99)
        monkeypatch.delenv("HUPR_FORCE_ALLREDUCE", raising=False)
        e0 = TrainEngine(cfg, device=dev, seed=0)
        assert not e0.buckets.active
        monkeypatch.setenv("HUPR_FORCE_ALLREDUCE", "1")
        e1 = TrainEngine(cfg, device=dev, seed=0)
        assert e1.buckets.active and e1.buckets.transport.name.startswith("rccl"), e1.buckets.transport.name
        for _ in range(3):
            l0, _ = e0.train_step_from_adc(*batch)
            l1, _ = e1.train_step_from_adc(*batch)
        torch.cuda.synchronize()
        assert float(l0) == float(l1)
        assert torch.equal(_flat(e0), _flat(e1))
        for a, b in zip(_state(e0) + _ratios(e0), _state(e1) + _ratios(e1)):
            assert torch.equal(a, b)
        e1.buckets.transport.close()
    finally:
        bf16.TWO_STREAMS = saved


def test_engine_lamb_accumulated_step_equals_the_plain_step(bf16):
    """train_step_accumulated over two copies of the batch == one train_step on it, to 1e-6 on the parameters."""
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, batch = _setup(seed=101)
    e1 = TrainEngine(cfg, device=dev, seed=0)
    e1.train_step_from_adc(*batch)
    e2 = TrainEngine(cfg, device=dev, seed=0)
    e2.train_step_accumulated([batch] * 2)
    torch.cuda.synchronize()
    a, b = _flat(e1).double(), _flat(e2).double()
    err = (a - b).abs().max().item()
    print("accumulated vs plain: max err %.3e, scale %.3e" % (err, a.abs().max().item()))
    assert err <= 1e-6 * a.abs().max().item()


def test_main_train_then_resume_with_lamb(tmp_path, monkeypatch, capsys):
    """main.py with TRAINING.optimizer: lamb — trains 2 steps, resumes 1; the checkpoint's group carries trust_ratio and the
    trust-ratio line is printed each epoch."""
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"]["dataDir"] = "synthetic"
    cfgd["TRAINING"]["batchSize"] = 2
    cfgd["TRAINING"]["epochs"] = 1
    cfgd["TRAINING"]["optimizer"] = "lamb"
    cfgd["TRAINING"]["lambWeightDecay"] = 0.02
    cfgd["TEST"]["batchSize"] = 2
    (tmp_path / "config").mkdir()
    yaml.safe_dump(cfgd, open(tmp_path / "config" / "tiny.yaml", "w"))
    (tmp_path / "logs").mkdir()
    (tmp_path / "visualization").mkdir()
    monkeypatch.chdir(tmp_path)
    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--max_steps", "2"])
    out = capsys.readouterr().out
    line = [l for l in out.splitlines() if "Trust ratios in epoch 0" in l]
    assert len(line) == 1 and all(w in line[0] for w in ("min ", "median ", "max ", "adapted tensors")), out[-2000:]
    run = tmp_path / "logs" / "run0"
    osd = torch.load(run / "checkpoint.pth")["optimizer_state_dict"]
    g = osd["param_groups"][0]
    assert g["trust_ratio"] is True and g["weight_decay"] == 0.02 and g["eps"] == 1e-6
    assert len(osd["state"]) == len(g["params"])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 2.0 for s in osd["state"].values())
    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--max_steps", "1"])   # resumes
    out = capsys.readouterr().out
    assert "Load the previous optimizer" in out and "Trust ratios in epoch" in out
    osd2 = torch.load(run / "checkpoint.pth")["optimizer_state_dict"]
    assert osd2["param_groups"][0]["trust_ratio"] is True
    assert all(float(s["step"]) == 3.0 for s in osd2["state"].values())
    assert json.load(open(run / "val_results.json"))
