"""CPU (no GPU needed): the case table of test_norm_act_fp64_gpu.py reaches every launch regime of csrc/norm_act.hip (by the
module's mirror of the host arithmetic), and its fp64 gates accept a float32 emulation of the kernels' own summation order
(per-thread fp32 runs of n_t rows, then fp64) while they reject results of subtly wrong kernels."""
import numpy as np
import pytest
import torch

import test_norm_act_fp64_gpu as N

f32 = np.float32


def R(c):
    return N.regime(c.dt, c.M, c.C)


# ---- the table reaches every regime ------------------------------------------------------------------------------------------
def test_mirror_matches_the_model_shapes():
    r = N.regime("f32", 1 << 20, 64)
    assert (r.nblk, r.rows_per_pass, r.n_t, r.grid, r.passes, r.fixed) == (512, 16, 128, 4096, 16, True)
    r = N.regime("bf16", 1 << 20, 64)
    assert (r.rows_per_pass, r.n_t, r.passes) == (32, 64, 8)
    r = N.regime("f32", 32769, 64)
    assert (r.nblk, r.rows_per_block, r.empty) == (512, 65, 7)
    assert N.regime("f32", 1000 * 3, 1000).rows_per_pass == 1 and N.regime("f32", 64, 4).rows_per_pass == 256


def test_table_reaches_every_regime():
    rs = [(c, R(c)) for c in N.CASES]
    for dt in ("f32", "bf16"):
        sub = [r for c, r in rs if c.dt == dt]
        assert any(r.nblk < 512 for r in sub) and any(r.nblk == 512 for r in sub), dt
        assert any(r.empty > 0 for r in sub), dt
        assert any(r.n_t == 1 for r in sub) and any(r.n_t >= 64 for r in sub), dt
        assert any(r.rows_per_pass == 256 for r in sub), dt
        assert any(r.idle > 0 for r in sub), dt
        assert any(r.passes > 1 for r in sub), dt
        assert any(not r.fixed for r in sub) and any(not r.fixed and r.passes > 1 for r in sub), dt
        assert {c.data for c in N.CASES if c.dt == dt} >= {"normal", "shifted", "const", "half"}, dt
    assert any(r.rows_per_pass == 1 for c, r in rs)
    assert {(c.M, c.C) for c in N.CASES} >= {(1, 64), (37, 64), (63, 64), (4096, 64), (32769, 64), (131072, 128), (16384, 256),
                                             (1 << 20, 64), (4096, 4), (4096, 8), (3000, 1000), (2048, 1024)}
    assert {c.C for c in N.CASES} >= {24, 40, 96}
    assert len({N.case_id(c) for c in N.CASES}) == len(N.CASES)
    # every case row is a legal call: C a multiple of V, at most 1024
    assert all(c.C % R(c).V == 0 and c.C <= 1024 and c.M >= 1 for c in N.CASES)


def test_entry_table_covers_both_dtypes_of_every_entry():
    for tab in (N.STATS, N.COLSUM, N.SSA, N.EVAL_ACT, N.BWD, N.BWD_REMASK, N.BWD2, N.BWD2_REMASK, N.PRELU_FWD, N.PRELU_BWD,
                N.PRELU_PARTIALS):
        assert set(tab) == {"f32", "bf16"} and len(set(tab.values())) == 2


# ---- float32 emulation of the kernels --------------------------------------------------------------------------------------
def runs(dt, T1, A, B):
    """Per-workgroup partial rows [nblk][2][C] of the statistics kernels: thread (row subgroup, channel) adds T1 with fp32 adds and
    A * B with fp32 fmas over its rows r0 + rsub + k rows_per_pass, k < n_t, in order; the subgroups then combine in fp64."""
    M, C = T1.shape
    r = N.regime(dt, M, C)
    out = np.zeros((r.nblk, 2, C))
    for b in range(r.nblk):
        r0, r1 = b * r.rows_per_block, min(M, (b + 1) * r.rows_per_block)
        s1 = np.zeros((r.rows_per_pass, C), f32)
        s2 = np.zeros((r.rows_per_pass, C), f32)
        for k in range(r.n_t):
            rows = r0 + np.arange(r.rows_per_pass) + k * r.rows_per_pass
            ok = rows < r1
            if not ok.any():
                break
            rr = rows[ok]
            s1[ok] = s1[ok] + T1[rr]
            s2[ok] = (s2[ok].astype(np.float64) + A[rr].astype(np.float64) * B[rr].astype(np.float64)).astype(f32)
        out[b, 0] = s1.astype(np.float64).sum(0)
        out[b, 1] = s2.astype(np.float64).sum(0)
    return out


def emulate_finalize(part, M, gamma, beta, rm, rv, biased=False, eps=N.EPS):
    s1, s2 = part[:, 0].sum(0), part[:, 1].sum(0)
    mean = s1 / M
    var = np.maximum(s2 / M - mean * mean, 0)
    inv = (1 / np.sqrt(var + float(f32(eps)))).astype(f32)
    sm = mean.astype(f32)
    sc = (gamma * inv).astype(f32)
    sh = (beta - sm * sc).astype(f32)
    unb = var * M / (M - 1) if M > 1 and not biased else var
    m = f32(N.MOM)
    nrm = (f32(1) - m) * rm + m * sm
    nrv = (f32(1) - m) * rv + m * unb.astype(f32)
    return [torch.from_numpy(np.asarray(t, dtype=f32)) for t in (sm, inv, sc, sh, nrm, nrv)]


def data(M, C, seed, mean=0.0, sd=1.0):
    g = np.random.default_rng(seed)
    return (g.standard_normal((M, C)) * sd + mean + g.uniform(-0.5, 0.5, C)).astype(f32)


def params(C, seed):
    g = np.random.default_rng(seed)
    return [g.uniform(0.5, 1.5, C).astype(f32), (0.5 * g.standard_normal(C)).astype(f32), g.standard_normal(C).astype(f32),
            g.uniform(0.5, 2, C).astype(f32)]


def stats_ok(x, dt, outs, p):
    """Which outputs of the statistics meet their gates."""
    G = N.stats_gate(torch.from_numpy(x).double(), N.regime(dt, *x.shape).n_t, *[torch.from_numpy(t).double() for t in p])
    sm, si, sc, sh, rm, rv = outs
    return dict(mean=bool(N.within(sm, *G["mean"]).all()), invstd=bool(N.within_interval(si, *G["invstd"][1:]).all()),
                scale=bool(N.within(sc, *G["scale"]).all()), shift=bool(N.within(sh, *G["shift"]).all()),
                running_mean=bool(N.within(rm, *G["running_mean"]).all()),
                running_var=bool(N.within(rv, *G["running_var"]).all()))


SHAPES = [("f32", 37, 64), ("bf16", 63, 64), ("f32", 4096, 8), ("f32", 1000, 24), ("bf16", 2000, 40), ("f32", 32769, 4)]


@pytest.mark.parametrize("dt,M,C", SHAPES)
@pytest.mark.parametrize("mean", [0.0, 32.0])
def test_stats_gate_accepts_emulation(dt, M, C, mean):
    x = data(M, C, M + C, mean=mean)
    if dt == "bf16":
        x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    p = params(C, 1)
    outs = emulate_finalize(runs(dt, x, x, x), M, *p)
    assert all(stats_ok(x, dt, outs, p).values())
    G = N.stats_gate(torch.from_numpy(x).double(), N.regime(dt, M, C).n_t, *[torch.from_numpy(t).double() for t in p])
    assert bool(N.within(torch.from_numpy(runs(dt, x, x, x)[:, 0].sum(0).astype(f32)), *G["colsum"]).all())


def test_stats_gate_accepts_constant_channels():
    x = np.tile(np.array([0.1, -3.7, 1000.0, 0.1], f32), (4096, 2))
    p = params(8, 2)
    assert all(stats_ok(x, "f32", emulate_finalize(runs("f32", x, x, x), 4096, *p), p).values())


def test_stats_gate_rejects_a_dropped_block():
    x = data(4096, 8, 1, mean=3.0)
    p = params(8, 1)
    part = runs("f32", x, x, x)
    part[17] = 0
    ok = stats_ok(x, "f32", emulate_finalize(part, 4096, *p), p)
    assert not ok["mean"] and not ok["running_mean"]


def test_stats_gate_rejects_a_block_counted_twice():
    x = data(32769, 4, 2, mean=3.0)
    p = params(4, 1)
    part = runs("f32", x, x, x)
    part[504] *= 2                                   # the short last block
    ok = stats_ok(x, "f32", emulate_finalize(part, 32769, *p), p)
    assert not ok["mean"]


def test_stats_gate_rejects_biased_running_variance():
    x = data(37, 64, 3)
    p = params(64, 1)
    ok = stats_ok(x, "f32", emulate_finalize(runs("f32", x, x, x), 37, *p, biased=True), p)
    assert not ok["running_var"] and ok["mean"] and ok["invstd"]


def test_stats_gate_rejects_eps_omitted():
    x = data(4096, 8, 4, sd=0.003)
    p = params(8, 1)
    ok = stats_ok(x, "f32", emulate_finalize(runs("f32", x, x, x), 4096, *p, eps=0.0), p)
    assert not ok["invstd"] and not ok["scale"]


# ---- backward --------------------------------------------------------------------------------------------------------------
def emulate_bwd(dt, x, g, mask, mean, inv, gamma, train, shift_group=0):
    """The one-branch backward in float32 (colstats<1> runs, finalize_bwd's fp32 coefficients, bwd_apply's fmas); shift_group
    reads the coefficients of the channel group that many groups over."""
    M, C = x.shape
    V = N.regime(dt, M, C).V
    gp = np.where(mask, g, f32(0)) if mask is not None else g
    xm = (x - mean).astype(f32)
    xh = (xm * inv).astype(f32)
    part = runs(dt, gp, gp, xh)
    s1, s2 = part[:, 0].sum(0).astype(f32), part[:, 1].sum(0).astype(f32)
    inv_m = f32(1) / f32(M)
    w = (gamma * inv).astype(f32)
    cB = ((-w * inv).astype(f32) * (s2 * inv_m)).astype(f32) if train else np.zeros(C, f32)
    cD = (-w * (s1 * inv_m)).astype(f32) if train else np.zeros(C, f32)
    sel = (np.arange(C) + shift_group * V) % C
    w, cB, cD, mu = w[sel], cB[sel], cD[sel], mean[sel]
    inner = (cB.astype(np.float64) * (x - mu).astype(f32) + cD).astype(f32)
    dx = (w.astype(np.float64) * gp + inner).astype(f32)
    return torch.from_numpy(dx), torch.from_numpy(s2), torch.from_numpy(s1)


def bwd_inputs(dt, M, C, seed):
    x = data(M, C, seed, mean=1.0)
    g = data(M, C, seed + 1)
    if dt == "bf16":
        x, g = (torch.from_numpy(t).to(torch.bfloat16).float().numpy() for t in (x, g))
    mean = x.mean(0).astype(f32)
    inv = (1 / np.sqrt(x.var(0) + 1e-5)).astype(f32)
    gamma = params(C, seed)[0]
    return x, g, mean, inv, gamma


def bwd_ok(dt, x, g, mask, mean, inv, gamma, train, got):
    r = N.regime(dt, *x.shape)
    ref = N.bwd_gate(*(torch.from_numpy(t).double() for t in (x, g)), None if mask is None else torch.from_numpy(mask),
                     *(torch.from_numpy(t).double() for t in (mean, inv, gamma)), r.n_t, train, dt == "bf16")
    dx, dg, db = got
    if dt == "bf16":
        dx = dx.to(torch.bfloat16)
    return dict(dx=bool(N.within(dx, *ref["dx"]).all()), dgamma=bool(N.within(dg, *ref["dgamma"]).all()),
                dbeta=bool(N.within(db, *ref["dbeta"]).all()))


@pytest.mark.parametrize("dt,M,C", SHAPES[:5])
@pytest.mark.parametrize("train", [1, 0])
def test_bwd_gate_accepts_emulation(dt, M, C, train):
    x, g, mean, inv, gamma = bwd_inputs(dt, M, C, 5)
    mask = (x - mean) * inv > 0.3
    for m in (mask, None):
        assert all(bwd_ok(dt, x, g, m, mean, inv, gamma, train, emulate_bwd(dt, x, g, m, mean, inv, gamma, train)).values())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bwd_gate_rejects_next_channel_groups_coefficients(dt):
    x, g, mean, inv, gamma = bwd_inputs(dt, 4096, 64, 6)
    mask = (x - mean) * inv > 0
    ok = bwd_ok(dt, x, g, mask, mean, inv, gamma, 1, emulate_bwd(dt, x, g, mask, mean, inv, gamma, 1, shift_group=1))
    assert not ok["dx"]


def test_bwd_gate_rejects_a_one_branch_mask():
    """Two-branch backward: the mask of y = relu(bn_a(x1) + bn_b(x2)) taken from branch a alone."""
    x1, g, m1, i1, ga = bwd_inputs("f32", 4096, 64, 7)
    x2, _, m2, i2, _ = bwd_inputs("f32", 4096, 64, 9)
    pa = (x1 - m1) * i1
    both = pa + (x2 - m2) * i2 > 0
    assert all(bwd_ok("f32", x1, g, both, m1, i1, ga, 1, emulate_bwd("f32", x1, g, both, m1, i1, ga, 1)).values())
    ok = bwd_ok("f32", x1, g, both, m1, i1, ga, 1, emulate_bwd("f32", x1, g, pa > 0, m1, i1, ga, 1))
    assert not ok["dx"] and not ok["dbeta"]


# ---- PReLU slope gradient --------------------------------------------------------------------------------------------------
def emulate_dalpha(dt, x, g, where):
    """prelu_bwd's slope gradient: each thread adds passes V products in fp32, the wave and the grid combine (here in fp64)."""
    n = x.size
    r = N.regime(dt, n // 8, 8)          # the element-wise grid depends on n = M C only
    V, grid = r.V, r.grid
    t = np.where(where(x), (g * x).astype(f32), f32(0)).reshape(-1, V)      # [nv][V]
    acc = np.zeros(grid * 256, f32)
    for p in range(r.passes):
        blk = t[p * grid * 256:(p + 1) * grid * 256]
        for k in range(V):
            acc[:blk.shape[0]] = acc[:blk.shape[0]] + blk[:, k]
    return torch.tensor([acc.astype(np.float64).sum()], dtype=torch.float32)


@pytest.mark.parametrize("dt,n", [("f32", 4096 * 64), ("bf16", 200000 * 8), ("f32", 1 << 22)])
def test_dalpha_gate(dt, n):
    g0 = np.random.default_rng(n)
    x = (g0.standard_normal(n) + 0.3).astype(f32)
    g = g0.standard_normal(n).astype(f32)
    if dt == "bf16":
        x, g = (torch.from_numpy(t).to(torch.bfloat16).float().numpy() for t in (x, g))
    r = N.regime(dt, n // 8, 8)          # the element-wise grid depends on n = M C only
    ref, b = N.dalpha_gate(torch.from_numpy(x).double(), torch.from_numpy(g).double(), r.passes, r.V)
    assert bool(N.within(emulate_dalpha(dt, x, g, lambda v: v <= 0), ref.reshape(1), b.reshape(1)).all())
    assert not bool(N.within(emulate_dalpha(dt, x, g, lambda v: v > 0), ref.reshape(1), b.reshape(1)).all())


def test_apply_gate():
    """The apply gate accepts fp32 fmas (and their bf16 rounding) and rejects the second branch's shift dropped."""
    g0 = np.random.default_rng(3)
    x1, x2 = g0.standard_normal((512, 16)).astype(f32), g0.standard_normal((512, 16)).astype(f32)
    s1, t1, s2, t2 = (g0.standard_normal(16).astype(f32) for _ in range(4))
    v = (x1.astype(np.float64) * s1 + t1).astype(f32)
    v = (v + (x2.astype(np.float64) * s2 + t2).astype(f32)).astype(f32)
    v = np.maximum(v, 0)
    T = [torch.from_numpy(t).double() for t in (x1, s1, t1, x2, s2, t2)]
    ref, b = N.apply_gate(*T, relu=True)
    assert bool(N.within(torch.from_numpy(v), ref, b).all())
    refb, bb = N.apply_gate(*T, relu=True, bf16=True)
    assert bool(N.within(torch.from_numpy(v).to(torch.bfloat16), refb, bb).all())
    bad = np.maximum((x1.astype(np.float64) * s1 + t1 + x2.astype(np.float64) * s2).astype(f32), 0)
    assert not bool(N.within(torch.from_numpy(bad), ref, b).all())
