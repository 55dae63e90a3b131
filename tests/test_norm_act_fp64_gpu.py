"""GPU (-m gpu): every entry point of csrc/norm_act.hip (BatchNorm statistics, finalizes, apply and backward passes, PReLU, the
bias-gradient column sums, the inference tails and the fp32 / bf16 casts) against fp64 references of exactly the values the kernels
read (bf16 inputs widened), at the shapes where the launch arithmetic changes regime, called through the C ABI.

Regime mirror (``regime``): the host arithmetic of norm_act.hip.  With V = 4 (fp32) or 8 (bf16) channels per thread:
    nblk = min(512, ceil(M / 64)) statistics workgroups of rows_per_block = ceil(M / nblk) rows, of which the trailing
    nblk - ceil(M / rows_per_block) are empty; rows_per_pass = 256 // (C / V) row subgroups (256 - rows_per_pass C / V threads
    idle); each thread adds n_t = ceil(rows_per_block / rows_per_pass) rows in fp32.  Element-wise kernels: grid =
    min(4096, ceil(nv / 256)) over nv = M C / V vectors, passes = ceil(nv / (256 grid)) loop passes, and the channel
    coefficients are loaded once when fixed = (256 grid V) % C == 0, reloaded every pass otherwise.
Each case row states the regime it reaches; tests/test_norm_act_gate.py asserts that the table reaches all of them.  The GPU
observes nblk (the statistics kernel writes exactly nblk 2 C doubles of a NaN-filled workspace, the empty blocks 0.0) and the
element-wise grid (hupr_prelu_bwd_partials_* returns it).

Gates (u = 2^-24; A1 = sum |x|, A2 = sum x^2 per channel):
  statistics   fp32 runs of n_t terms: dS1 = (n_t + 1) u A1, dS2 = (n_t + 2) u A2 (the fp64 combination adds < 2^-40 A).
               save_mean: dS1 / M + u |mean|.  dvar = dS2 / M + (2 |mean| + dS1 / M) dS1 / M (+ 2^-49 A2 / M, the fp64 finalize).
               save_invstd in [1 / sqrt(var + dvar + eps), 1 / sqrt(max(0, var - dvar) + eps)] widened by 2u (covers constant
               channels, var = 0).  scale, shift, running mean / var carry dmean, dinvstd, dvar through a few fp32 roundings (3u
               per term); running_var uses the unbiased M / (M - 1) for M > 1.  colsum: dS1 + u |S1|.
  apply        y = act(x1 s1 + t1 [+ x2 s2 + t2]) with the call's own fp32 s, t: 2u (|x1 s1| + |t1| + |x2 s2| + |t2|) + u |ref|,
               plus 2^-8 (|ref| + that) for a bf16 output (8 significant bits: a rounding to bf16 moves a value by up to
               2^-8 of itself).
  backward     g' = dy [mask], xhat = (x - save_mean) save_invstd from the call's own fp32 values, S1 = sum g', S2 = sum g' xhat.
               dbeta: dS1 + u |S1|, dS1 = (n_t + 1) u sum |g'|;  dgamma: dS2 + u |S2|, dS2 = (n_t + 3) u sum |g' xhat|.
               dx (w = gamma invstd): 8 u (|w g'| + |w| |xhat| |S2| / M + |w| |S1| / M) + |w| (|xhat| dS2 + dS1) / M, plus 2^-8
               (|ref| + that) for bf16 (8u: the coefficients cA, cB, cD are formed in at most five fp32 roundings, x - mean and the two fmas
               add three).  train = 0: dx = w g', 2u |w g'|.
  PReLU        y and dx are one correctly rounded multiply: bit-exact against torch (fp32, then .to(bfloat16)), NaN as NaN-ness.
               dalpha = sum dy x [x <= 0]: (passes V + 7) u sum |dy x [x <= 0]| + u |ref| (per-thread fp32 run, 6 wave steps).
  casts        bit-exact against torch .to(); NaN in gives NaN out.
  infer tail   bit-identical to the device composition its kernel comment names, and within an fp64 gate of 2^-8 relative terms.
Bit-for-bit identities between entries: finalize of bn_train_stats's own workspace = bn_train_stats; finalize2 = two finalizes;
bn_eval_act = bn_eval_params + scale_shift_act; y_mask form = remask form; dbeta1 = dbeta2; prelu_bwd_partials +
sum_partials_multi = prelu_bwd; two runs of every statistics entry at 1M rows.  Launch counts are asserted, a 4 KiB pattern
guard behind every workspace must come back unchanged, and refused calls return their code, launch nothing and leave NaN-filled
outputs untouched.  References: torch fp64 on the device for 1M-row cases, on the CPU otherwise."""
import collections
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG, HUPR_ERR_WORKSPACE = -1, -2
U = 2.0 ** -24
BF16_U = 2.0 ** -8                         # bf16 keeps 8 significant bits: one rounding moves a value by up to 2^-8 of it
TINY = 2.0 ** -40
C_DX = 8.0
MOM, EPS = 0.1, 1e-5
GUARD = 4096
PAT = 0x7FF8DEADBEEF0001                   # a NaN payload (as a double) no kernel writes
WORST = {}                                 # quantity -> (worst err / bound, case)
PRECISION = {}                             # case -> measured save_invstd precision (printed by the last test)
CURRENT = [""]

STATS = {"f32": "hupr_bn_train_stats_f32", "bf16": "hupr_bn_train_stats_bf16act"}
COLSUM = {"f32": "hupr_colsum_f32", "bf16": "hupr_colsum_bf16act"}
SSA = {"f32": "hupr_scale_shift_act_f32", "bf16": "hupr_scale_shift_act_bf16act"}
EVAL_ACT = {"f32": "hupr_bn_eval_act_f32", "bf16": "hupr_bn_eval_act_bf16act"}
BWD = {"f32": "hupr_bn_bwd_f32", "bf16": "hupr_bn_bwd_bf16act"}
BWD_REMASK = {"f32": "hupr_bn_bwd_remask_f32", "bf16": "hupr_bn_bwd_remask_bf16act"}
BWD2 = {"f32": "hupr_bn_bwd2_f32", "bf16": "hupr_bn_bwd2_bf16act"}
BWD2_REMASK = {"f32": "hupr_bn_bwd2_remask_f32", "bf16": "hupr_bn_bwd2_remask_bf16act"}
PRELU_FWD = {"f32": "hupr_prelu_fwd_f32", "bf16": "hupr_prelu_fwd_bf16act"}
PRELU_BWD = {"f32": "hupr_prelu_bwd_f32", "bf16": "hupr_prelu_bwd_bf16act"}
PRELU_PARTIALS = {"f32": "hupr_prelu_bwd_partials_f32", "bf16": "hupr_prelu_bwd_partials_bf16act"}
# the other entries: hupr_bn_ws_bytes, hupr_prelu_ws_bytes, hupr_bn_train_finalize_f32, hupr_bn_train_finalize2_f32,
# hupr_bn_eval_params_f32, hupr_infer_tail_bf16act, hupr_sum_partials_multi, hupr_cast_f32_to_bf16, hupr_cast_bf16_to_f32


def cdiv(a, b):
    return -(-a // b)


Regime = collections.namedtuple("Regime", "V nblk rows_per_block rows_per_pass idle n_t empty grid passes fixed")


def regime(dt, M, C):
    """The launch arithmetic of norm_act.hip's host code for M rows of C channels (see the module docstring)."""
    V = 4 if dt == "f32" else 8
    nblk = min(512, cdiv(M, 64))
    rpb = cdiv(M, nblk)
    cvn = C // V
    rpp = 256 // cvn
    nv = M * C // V
    grid = min(4096, cdiv(nv, 256))
    return Regime(V, nblk, rpb, rpp, 256 - rpp * cvn, cdiv(rpb, rpp), nblk - cdiv(M, rpb), grid, cdiv(nv, 256 * grid),
                  (256 * grid * V) % C == 0)


Case = collections.namedtuple("Case", "dt M C data why")
CASES = [
    Case("f32", 1, 64, "normal", "one row: biased-variance branch of the running update"),
    Case("bf16", 1, 64, "normal", "one row"),
    Case("f32", 37, 64, "normal", "one short block"),
    Case("bf16", 63, 64, "normal", "one short block"),
    Case("f32", 4096, 64, "normal", "64 blocks, n_t = 4"),
    Case("bf16", 4096, 64, "shifted", "|mean| = 32 std"),
    Case("f32", 4096, 64, "half", "ReLU mask about half on"),
    Case("f32", 4096, 64, "const", "constant channels: var = 0"),
    Case("bf16", 4096, 64, "const", "constant channels: var = 0"),
    Case("f32", 32769, 64, "normal", "nblk = 512 with 7 empty trailing blocks"),
    Case("bf16", 32769, 64, "half", "nblk = 512 with 7 empty trailing blocks"),
    Case("f32", 32769, 64, "shifted", "|mean| = 32 std at nblk = 512"),
    Case("f32", 131072, 128, "normal", "C = 128, 2 loop passes"),
    Case("bf16", 16384, 256, "normal", "C = 256, rows_per_pass = 8"),
    Case("f32", 1048576, 64, "normal", "the model's largest BatchNorm: n_t = 128, 16 passes"),
    Case("bf16", 1048576, 64, "normal", "the model's largest BatchNorm: n_t = 64, 8 passes"),
    Case("f32", 1048576, 64, "shifted", "|mean| = 32 std at n_t = 128"),
    Case("f32", 4096, 4, "normal", "rows_per_pass = 256"),
    Case("bf16", 4096, 8, "normal", "rows_per_pass = 256"),
    Case("f32", 200000, 24, "normal", "idle threads, coefficient reload over 2 passes"),
    Case("bf16", 250000, 40, "normal", "idle threads, coefficient reload over 2 passes"),
    Case("f32", 5000, 96, "shifted", "16 idle threads, coefficient reload"),
    Case("bf16", 7001, 96, "normal", "idle threads, coefficient reload"),
    Case("bf16", 4099, 24, "half", "idle thread, short last block"),
    Case("f32", 3000, 1000, "normal", "rows_per_pass = 1, 6 idle threads, reload"),
    Case("f32", 2048, 1024, "normal", "C = 1024, rows_per_pass = 1"),
    Case("bf16", 2048, 1024, "shifted", "C = 1024, rows_per_pass = 2"),
]


def case_id(c):
    return "%s-M%d-C%d-%s" % (c.dt, c.M, c.C, c.data)


# ---- the fp64 references and the gates (device-agnostic torch; also used without a GPU by test_norm_act_gate.py) ----------
def stats_gate(X, n_t, gamma, beta, rm0, rv0, momentum=MOM, eps=EPS, dS1=None, dS2=None):
    """fp64 references and bounds of every output of the BatchNorm statistics for X [M, C] (fp64) summed in fp32 runs of n_t
    (or with the given sum errors dS1, dS2).  gamma, beta, rm0, rv0: fp64 [C]."""
    M = X.shape[0]
    m = float(torch.tensor(momentum, dtype=torch.float32))
    e = float(torch.tensor(eps, dtype=torch.float32))
    S1 = X.sum(0)
    A1 = X.abs().sum(0)
    A2 = (X * X).sum(0)
    mean = S1 / M
    var = ((X - mean) ** 2).sum(0) / M
    if dS1 is None:
        dS1 = (n_t + 1) * U * A1 + TINY * A1
        dS2 = (n_t + 2) * U * A2 + TINY * A2
    dmean = dS1 / M + U * mean.abs() + TINY * A1 / M
    dvar = dS2 / M + (2 * mean.abs() + dS1 / M) * dS1 / M + 2.0 ** -49 * A2 / M
    inv = 1 / torch.sqrt(var + e)
    lo = (1 - 2 * U) / torch.sqrt(var + dvar + e)
    hi = (1 + 2 * U) / torch.sqrt((var - dvar).clamp(min=0) + e)
    dinv = torch.maximum(hi - inv, inv - lo)
    ag = gamma.abs()
    f = M / (M - 1) if M > 1 else 1.0
    return dict(
        mean=(mean, dmean),
        invstd=(inv, lo, hi),
        scale=(gamma * inv, ag * dinv + 2 * U * ag * hi),
        shift=(beta - mean * gamma * inv,
               ag * hi * dmean + mean.abs() * ag * dinv + 3 * U * (beta.abs() + mean.abs() * ag * hi)),
        running_mean=((1 - m) * rm0 + m * mean, m * dmean + 3 * U * ((1 - m) * rm0.abs() + m * mean.abs()) + U * rm0.abs()),
        running_var=((1 - m) * rv0 + m * f * var,
                     m * f * dvar + 3 * U * ((1 - m) * rv0.abs() + m * f * (var + dvar)) + U * rv0.abs()),
        colsum=(S1, dS1 + U * S1.abs()),
        var=var)


def apply_gate(X1, s1, t1, X2=None, s2=None, t2=None, relu=False, bf16=False):
    """y = act(x1 s1 + t1 [+ x2 s2 + t2]) from the call's own fp32 s, t (fp64 [C]); X fp64 [M, C] -> (ref, bound)."""
    pre = X1 * s1 + t1
    A = (X1 * s1).abs() + t1.abs()
    if X2 is not None:
        pre = pre + X2 * s2 + t2
        A = A + (X2 * s2).abs() + t2.abs()
    ref = pre.clamp(min=0) if relu else pre
    b = 2 * U * A + U * ref.abs()
    if bf16:
        b = b + BF16_U * (ref.abs() + b)
    return ref, b


def bwd_gate(X, G, mask, mean, inv, gamma, n_t, train, bf16=False):
    """One branch of the BatchNorm backward: X, G fp64 [M, C], mask bool [M, C] or None, mean, inv, gamma fp64 [C] (the call's own
    fp32 values) -> dict of (ref, bound) for dx, dgamma, dbeta."""
    M = X.shape[0]
    gp = G if mask is None else G * mask
    xh = (X - mean) * inv
    S1 = gp.sum(0)
    S2 = (gp * xh).sum(0)
    A1 = gp.abs().sum(0)
    A2 = (gp * xh).abs().sum(0)
    dS1 = (n_t + 1) * U * A1 + TINY * A1
    dS2 = (n_t + 3) * U * A2 + TINY * A2
    w = gamma * inv
    if train:
        dx = w * (gp - S1 / M - xh * S2 / M)
        b = C_DX * U * ((w * gp).abs() + w.abs() * xh.abs() * S2.abs() / M + w.abs() * S1.abs() / M) \
            + w.abs() * (xh.abs() * dS2 + dS1) / M
    else:
        dx = w * gp
        b = 2 * U * (w * gp).abs()
    if bf16:
        b = b + BF16_U * (dx.abs() + b)
    return dict(dx=(dx, b), dgamma=(S2, dS2 + U * S2.abs()), dbeta=(S1, dS1 + U * S1.abs()))


def dalpha_gate(X, G, passes, V):
    """dalpha = sum dy x [x <= 0] over all elements (fp64) -> (ref, bound)."""
    t = torch.where(X <= 0, G * X, torch.zeros_like(X))
    ref = t.sum()
    A = t.abs().sum()
    return ref, (passes * V + 7) * U * A + U * ref.abs() + TINY * A


def within(got, ref, bound):
    """True where got meets |got - ref| <= bound (a NaN never does)."""
    return (got.to(ref.device).double() - ref).abs() <= bound


def within_interval(got, lo, hi):
    g = got.to(lo.device).double()
    return (g >= lo) & (g <= hi)


def _note(what, w):
    if what not in WORST or w > WORST[what][0]:
        WORST[what] = (w, CURRENT[0])


def check(what, got, ref, bound):
    got = got.to(ref.device).double()
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).nan_to_num(float("inf"))
    _note(what, ratio.max().item())
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s [%s]: %d of %d outside the gate, first at %s (got %r, ref %r, bound %r)"
                             % (what, CURRENT[0], bad.shape[0], ok.numel(), i, got[i].item(), ref[i].item(), bound[i].item()))


def check_interval(what, got, ref, lo, hi):
    got = got.to(ref.device).double()
    side = torch.where(got >= ref, hi - ref, ref - lo)
    err = (got - ref).abs()
    _note(what, torch.where(err == 0, torch.zeros_like(err), err / side).nan_to_num(float("inf")).max().item())
    ok = (got >= lo) & (got <= hi)
    assert bool(ok.all()), "%s [%s]: %d of %d outside [lo, hi]" % (what, CURRENT[0], int((~ok).sum()), ok.numel())


def check_stats(G, sm, si, sc, sh, rm=None, rv=None):
    check("mean", sm, *G["mean"])
    check_interval("invstd", si, *G["invstd"])
    check("scale", sc, *G["scale"])
    check("shift", sh, *G["shift"])
    if rm is not None:
        check("running_mean", rm, *G["running_mean"])
        check("running_var", rv, *G["running_var"])


# ---- device helpers --------------------------------------------------------------------------------------------------------
def act_dtype(dt):
    return torch.float32 if dt == "f32" else torch.bfloat16


def ref_device(M):
    return "cuda" if M >= 1 << 20 else "cpu"


def make_x(dt, M, C, data, seed):
    """[M, C] activations in the case's storage type on the GPU."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if data == "const":
        vals = torch.tensor([0.1, -3.7, 1000.0], device="cuda")[torch.arange(C, device="cuda") % 3]
        x = vals.expand(M, C).contiguous()
    else:
        sd = 0.5 + 1.5 * torch.rand(C, generator=g, device="cuda")
        if data == "shifted":
            mu = 32 * sd * torch.where(torch.rand(C, generator=g, device="cuda") < 0.5, -1.0, 1.0)
        else:
            mu = torch.rand(C, generator=g, device="cuda") - 0.5
        x = torch.randn(M, C, generator=g, device="cuda") * sd + mu
    return x.to(act_dtype(dt)).contiguous()


def bn_params(C, seed, half=False):
    g = torch.Generator().manual_seed(seed)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = torch.zeros(C) if half else 0.5 * torch.randn(C, generator=g)
    rm = torch.randn(C, generator=g)
    rv = 0.5 + 1.5 * torch.rand(C, generator=g)
    return [t.cuda() for t in (gamma, beta, rm, rv)]


def nan32(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def nan_act(dt, *shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=act_dtype(dt))


def ws_buf(nbytes):
    """nbytes of workspace followed by a GUARD-byte pattern guard, all filled with the NaN pattern PAT."""
    assert nbytes % 8 == 0
    return torch.full(((nbytes + GUARD) // 8,), PAT, dtype=torch.int64, device="cuda")


def guard_intact(ws, nbytes):
    return bool((ws[nbytes // 8:] == PAT).all())


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4 else torch.int64))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


@pytest.fixture(scope="module")
def L():
    from hupr_amd import runtime
    return runtime.lib()


class Launches:
    def __init__(self, L):
        self.L = L

    def __enter__(self):
        self.n0 = self.L.hupr_launch_count()
        return self

    def __exit__(self, *a):
        self.n = self.L.hupr_launch_count() - self.n0


def run_stats(L, dt, x, M, C, p, rm=None, rv=None, ws=None):
    from hupr_amd import runtime as rt
    wsb = L.hupr_bn_ws_bytes(C)
    ws = ws_buf(wsb) if ws is None else ws
    sm, si, sc, sh = (nan32(C) for _ in range(4))
    with Launches(L) as n:
        rt.check(getattr(L, STATS[dt])(x.data_ptr(), M, C, p[0].data_ptr(), p[1].data_ptr(), rt.ptr(rm), rt.ptr(rv), MOM, EPS,
                                       sm.data_ptr(), si.data_ptr(), sc.data_ptr(), sh.data_ptr(), ws.data_ptr(), wsb, rt.stream()))
    assert n.n == 2
    return sm, si, sc, sh, ws


def ssa(L, dt, x1, s1, t1, x2, s2, t2, M, C, act):
    from hupr_amd import runtime as rt
    y = nan_act(dt, M, C)
    rt.check(getattr(L, SSA[dt])(x1.data_ptr(), s1.data_ptr(), t1.data_ptr(), rt.ptr(x2), rt.ptr(s2), rt.ptr(t2), y.data_ptr(),
                                 M, C, act, rt.stream()))
    return y


def d64(t, dev):
    return t.to(dev).double()


# ---- BatchNorm statistics, column sums, finalize ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_bn_stats_colsum_finalize(c, L):
    from hupr_amd import runtime as rt
    CURRENT[0] = case_id(c)
    R = regime(c.dt, c.M, c.C)
    M, C, rd = c.M, c.C, ref_device(c.M)
    x = make_x(c.dt, M, C, c.data, 1)
    p = bn_params(C, 2, c.data == "half")
    rm, rv = p[2].clone(), p[3].clone()
    sm, si, sc, sh, ws = run_stats(L, c.dt, x, M, C, p, rm, rv)
    wsb = L.hupr_bn_ws_bytes(C)
    assert wsb == 512 * 3 * C * 8 + 8 * C * 4
    torch.cuda.synchronize()
    # the statistics kernel wrote exactly nblk partial rows; the empty trailing blocks hold 0.0; the guard is intact
    part = ws[:wsb // 8]
    written = int((part != PAT).sum())
    assert written == R.nblk * 2 * C and bool((part[:written] != PAT).all()), (written, R.nblk)
    pd = part.view(torch.float64)[:written].view(R.nblk, 2, C)
    if R.empty:
        assert bool((pd[R.nblk - R.empty:] == 0).all())
    assert bool(torch.isfinite(pd).all())
    assert guard_intact(ws, wsb)

    X = d64(x, rd)
    P = [d64(t, rd) for t in p]
    G = stats_gate(X, R.n_t, *P)
    check_stats(G, sm, si, sc, sh, rm, rv)

    # null running pointers: same outputs, running buffers not read or written
    sm2, si2, sc2, sh2, _ = run_stats(L, c.dt, x, M, C, p)
    assert all(same_bits(a, b) for a, b in ((sm, sm2), (si, si2), (sc, sc2), (sh, sh2)))

    # finalize of the statistics kernel's own partial rows = bn_train_stats, bit for bit (running statistics included)
    rm3, rv3 = p[2].clone(), p[3].clone()
    fo = [nan32(C) for _ in range(4)]
    with Launches(L) as n:
        rt.check(L.hupr_bn_train_finalize_f32(ws.data_ptr(), R.nblk, M, C, p[0].data_ptr(), p[1].data_ptr(), rm3.data_ptr(),
                                              rv3.data_ptr(), MOM, EPS, *[t.data_ptr() for t in fo], rt.stream()))
    assert n.n == 1
    assert all(same_bits(a, b) for a, b in zip(fo + [rm3, rv3], (sm, si, sc, sh, rm, rv)))

    # colsum: its own gate, 2 launches, workspace guard
    out = nan32(C)
    ws2 = ws_buf(wsb)
    with Launches(L) as n:
        rt.check(getattr(L, COLSUM[c.dt])(x.data_ptr(), M, C, out.data_ptr(), ws2.data_ptr(), wsb, rt.stream()))
    assert n.n == 2
    check("colsum", out, *G["colsum"])
    torch.cuda.synchronize()
    assert guard_intact(ws2, wsb)

    if M >= 1 << 20:       # determinism: a second run gives the same bits (partial rows included)
        rm4, rv4 = p[2].clone(), p[3].clone()
        again = run_stats(L, c.dt, x, M, C, p, rm4, rv4)
        assert all(same_bits(a, b) for a, b in zip(again[:4] + (rm4, rv4), (sm, si, sc, sh, rm, rv)))
        assert same_bits(again[4], ws)
        out2 = nan32(C)
        rt.check(getattr(L, COLSUM[c.dt])(x.data_ptr(), M, C, out2.data_ptr(), ws2.data_ptr(), wsb, rt.stream()))
        assert same_bits(out, out2)

    if c.data in ("shifted", "const"):     # measured precision of save_invstd, next to torch's fp32 BatchNorm on the same data
        xf = x.float()
        tsm, tsi = torch.native_batch_norm(xf, p[0], p[1], None, None, True, MOM, EPS)[1:3]
        inv, _, _ = G["invstd"]
        k_rel = ((d64(si, rd) - inv).abs() / inv).max().item()
        t_rel = ((d64(tsi, rd) - inv).abs() / inv).max().item()
        var_k = (1 / d64(si, rd) ** 2 - EPS).abs().max().item()
        var_t = (1 / d64(tsi, rd) ** 2 - EPS).abs().max().item()
        PRECISION[case_id(c)] = (k_rel, t_rel, var_k, var_t)


# ---- finalize from host-built partial rows; finalize2 = two finalizes ------------------------------------------------------
@pytest.mark.parametrize("nblk,C", [(1, 64), (37, 20), (37, 52), (512, 1000)], ids=lambda v: str(v))
def test_bn_finalize_host_partials(nblk, C, L):
    from hupr_amd import runtime as rt
    CURRENT[0] = "finalize-nblk%d-C%d" % (nblk, C)
    M = nblk * 50 + 3
    g = torch.Generator().manual_seed(nblk * 7 + C)
    X = (torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + torch.randn(C, generator=g, dtype=torch.float64))
    rows = torch.arange(M) % nblk
    part = torch.zeros(nblk, 2, C, dtype=torch.float64)
    part[:, 0].index_add_(0, rows, X)
    part[:, 1].index_add_(0, rows, X * X)
    A1, A2 = X.abs().sum(0), (X * X).sum(0)
    err = (nblk + 16) * 2.0 ** -53
    p = bn_params(C, 5)
    P = [t.cpu().double() for t in p]
    Gt = stats_gate(X, 0, *P, dS1=err * A1, dS2=err * A2)
    pa = part.cuda()
    rm, rv = p[2].clone(), p[3].clone()
    o = [nan32(C) for _ in range(4)]
    rt.check(L.hupr_bn_train_finalize_f32(pa.data_ptr(), nblk, M, C, p[0].data_ptr(), p[1].data_ptr(), rm.data_ptr(),
                                          rv.data_ptr(), MOM, EPS, *[t.data_ptr() for t in o], rt.stream()))
    check_stats(Gt, *o, rm, rv)
    # a second BatchNorm of the same shape (other partials, nblk, parameters, momentum, eps)
    nb2 = max(1, nblk // 2)
    X2 = torch.randn(M, C, generator=g, dtype=torch.float64) * 0.3 - 1
    part2 = torch.zeros(nb2, 2, C, dtype=torch.float64)
    part2[:, 0].index_add_(0, torch.arange(M) % nb2, X2)
    part2[:, 1].index_add_(0, torch.arange(M) % nb2, X2 * X2)
    pa2 = part2.cuda()
    q = bn_params(C, 6)
    rmq, rvq = q[2].clone(), q[3].clone()
    o2 = [nan32(C) for _ in range(4)]
    rt.check(L.hupr_bn_train_finalize_f32(pa2.data_ptr(), nb2, M, C, q[0].data_ptr(), q[1].data_ptr(), rmq.data_ptr(),
                                          rvq.data_ptr(), 0.25, 1e-3, *[t.data_ptr() for t in o2], rt.stream()))
    r1, r2 = p[2].clone(), p[3].clone()
    r3, r4 = q[2].clone(), q[3].clone()
    f1 = [nan32(C) for _ in range(4)]
    f2 = [nan32(C) for _ in range(4)]
    with Launches(L) as n:
        rt.check(L.hupr_bn_train_finalize2_f32(pa.data_ptr(), nblk, p[0].data_ptr(), p[1].data_ptr(), r1.data_ptr(), r2.data_ptr(),
                                               MOM, EPS, *[t.data_ptr() for t in f1], pa2.data_ptr(), nb2, q[0].data_ptr(),
                                               q[1].data_ptr(), r3.data_ptr(), r4.data_ptr(), 0.25, 1e-3,
                                               *[t.data_ptr() for t in f2], M, C, rt.stream()))
    assert n.n == 1
    assert all(same_bits(a, b) for a, b in zip(f1 + [r1, r2] + f2 + [r3, r4], o + [rm, rv] + o2 + [rmq, rvq]))


# ---- apply: scale_shift_act, bn_eval_act = bn_eval_params + scale_shift_act ------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_bn_apply(c, L):
    from hupr_amd import runtime as rt
    CURRENT[0] = case_id(c)
    M, C, rd = c.M, c.C, ref_device(c.M)
    bf = c.dt == "bf16"
    x1 = make_x(c.dt, M, C, c.data, 1)
    x2 = make_x(c.dt, M, C, "normal", 3)
    p1, p2 = bn_params(C, 2, c.data == "half"), bn_params(C, 4)
    _, _, s1, t1, _ = run_stats(L, c.dt, x1, M, C, p1)
    _, _, s2, t2, _ = run_stats(L, c.dt, x2, M, C, p2)
    X1, X2 = d64(x1, rd), d64(x2, rd)
    S1, T1, S2, T2 = (d64(t, rd) for t in (s1, t1, s2, t2))
    for two in (False, True):
        for act in (0, 1):
            with Launches(L) as n:
                y = ssa(L, c.dt, x1, s1, t1, x2 if two else None, s2 if two else None, t2 if two else None, M, C, act)
            assert n.n == 1
            ref, b = apply_gate(X1, S1, T1, X2 if two else None, S2, T2, relu=bool(act), bf16=bf)
            check("y", y, ref, b)
            del y
    # eval mode from running statistics: one launch, the same bits as eval_params + scale_shift_act
    sc, sh, sc2, sh2 = (nan32(C) for _ in range(4))
    rt.check(L.hupr_bn_eval_params_f32(*[t.data_ptr() for t in p1], EPS, C, sc.data_ptr(), sh.data_ptr(), rt.stream()))
    rt.check(L.hupr_bn_eval_params_f32(*[t.data_ptr() for t in p2], 1e-3, C, sc2.data_ptr(), sh2.data_ptr(), rt.stream()))
    P1 = [t.cpu().double() for t in p1]
    inv = 1 / torch.sqrt(P1[3] + float(torch.tensor(EPS, dtype=torch.float32)))
    check("eval_scale", sc.cpu(), P1[0] * inv, 4 * U * (P1[0] * inv).abs())
    check("eval_shift", sh.cpu(), P1[1] - P1[2] * P1[0] * inv, 6 * U * (P1[1].abs() + (P1[2] * P1[0] * inv).abs()))
    for two in (False, True):
        for act in (0, 1):
            want = ssa(L, c.dt, x1, sc, sh, x2 if two else None, sc2 if two else None, sh2 if two else None, M, C, act)
            y = nan_act(c.dt, M, C)
            q = [t.data_ptr() for t in p2] if two else [None] * 4
            with Launches(L) as n:
                rt.check(getattr(L, EVAL_ACT[c.dt])(x1.data_ptr(), *[t.data_ptr() for t in p1], EPS, rt.ptr(x2) if two else None,
                                                    *q, 1e-3, y.data_ptr(), M, C, act, rt.stream()))
            assert n.n == 1
            assert same_bits(y, want), "bn_eval_act != bn_eval_params + scale_shift_act (two=%s act=%d)" % (two, act)
            del want, y


# ---- backward: all eight BatchNorm backward entries ------------------------------------------------------------------------
def _bwd_outputs(dt, M, C, two):
    n = 2 if two else 1
    return [nan_act(dt, M, C) for _ in range(n)], [nan32(C) for _ in range(2 * n)]


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_bn_bwd(c, L):
    from hupr_amd import runtime as rt
    CURRENT[0] = case_id(c)
    R = regime(c.dt, c.M, c.C)
    M, C, rd = c.M, c.C, ref_device(c.M)
    bf = c.dt == "bf16"
    x1 = make_x(c.dt, M, C, c.data, 1)
    x2 = make_x(c.dt, M, C, "normal", 3)
    dy = make_x(c.dt, M, C, "normal", 5)
    p1, p2 = bn_params(C, 2, c.data == "half"), bn_params(C, 4)
    m1, i1, s1, t1, _ = run_stats(L, c.dt, x1, M, C, p1)
    m2, i2, s2, t2, _ = run_stats(L, c.dt, x2, M, C, p2)
    y1 = ssa(L, c.dt, x1, s1, t1, None, None, None, M, C, 1)
    y12 = ssa(L, c.dt, x1, s1, t1, x2, s2, t2, M, C, 1)
    X1, X2, G = d64(x1, rd), d64(x2, rd), d64(dy, rd)
    M1, I1, S1, T1, M2, I2, S2, T2 = (d64(t, rd) for t in (m1, i1, s1, t1, m2, i2, s2, t2))
    G1, G2 = d64(p1[0], rd), d64(p2[0], rd)
    # precondition: no pre-activation so small that a bf16 rounding of y could turn a positive into zero
    pre1 = X1 * S1 + T1
    pre12 = pre1 + X2 * S2 + T2
    assert float(pre1.abs().min()) >= 2.0 ** -120 and float(pre12.abs().min()) >= 2.0 ** -120
    mask1, mask12 = d64(y1, rd) > 0, d64(y12, rd) > 0
    if c.data == "half":
        assert 0.35 < float(mask1.double().mean()) < 0.65
    del pre1, pre12
    wsb = L.hupr_bn_ws_bytes(C)
    s = rt.stream()
    for train in (1, 0):
        ref = bwd_gate(X1, G, mask1, M1, I1, G1, R.n_t, train, bf)
        runs = []
        for name, mask_args in ((BWD[c.dt], (y1.data_ptr(),)), (BWD_REMASK[c.dt], (s1.data_ptr(), t1.data_ptr()))):
            (dx,), (dg, db) = _bwd_outputs(c.dt, M, C, False)
            ws = ws_buf(wsb)
            with Launches(L) as n:
                rt.check(getattr(L, name)(dy.data_ptr(), *mask_args, x1.data_ptr(), m1.data_ptr(), i1.data_ptr(), p1[0].data_ptr(),
                                          dx.data_ptr(), dg.data_ptr(), db.data_ptr(), M, C, train, ws.data_ptr(), wsb, s))
            assert n.n == 3
            torch.cuda.synchronize()
            assert guard_intact(ws, wsb), name
            runs.append((dx, dg, db))
        check("dx", runs[0][0], *ref["dx"])
        check("dgamma", runs[0][1], *ref["dgamma"])
        check("dbeta", runs[0][2], *ref["dbeta"])
        assert all(same_bits(a, b) for a, b in zip(*runs)), "y_mask form != remask form"
        del runs, ref
        # no ReLU (null mask)
        (dx,), (dg, db) = _bwd_outputs(c.dt, M, C, False)
        ws = ws_buf(wsb)
        rt.check(getattr(L, BWD[c.dt])(dy.data_ptr(), None, x1.data_ptr(), m1.data_ptr(), i1.data_ptr(), p1[0].data_ptr(),
                                       dx.data_ptr(), dg.data_ptr(), db.data_ptr(), M, C, train, ws.data_ptr(), wsb, s))
        ref = bwd_gate(X1, G, None, M1, I1, G1, R.n_t, train, bf)
        check("dx", dx, *ref["dx"])
        check("dgamma", dg, *ref["dgamma"])
        check("dbeta", db, *ref["dbeta"])
        del dx, ref
        # two branches, shared dy and mask
        ra = bwd_gate(X1, G, mask12, M1, I1, G1, R.n_t, train, bf)
        rb = bwd_gate(X2, G, mask12, M2, I2, G2, R.n_t, train, bf)
        runs = []
        for name in (BWD2[c.dt], BWD2_REMASK[c.dt]):
            (dx1, dx2), (dg1, db1, dg2, db2) = _bwd_outputs(c.dt, M, C, True)
            ws = ws_buf(wsb)
            outs = [t.data_ptr() for t in (dx1, dx2, dg1, db1, dg2, db2)]
            with Launches(L) as n:
                if name == BWD2[c.dt]:
                    rt.check(getattr(L, name)(dy.data_ptr(), y12.data_ptr(), x1.data_ptr(), m1.data_ptr(), i1.data_ptr(),
                                              p1[0].data_ptr(), x2.data_ptr(), m2.data_ptr(), i2.data_ptr(), p2[0].data_ptr(), *outs,
                                              M, C, train, ws.data_ptr(), wsb, s))
                else:
                    rt.check(getattr(L, name)(dy.data_ptr(), x1.data_ptr(), s1.data_ptr(), t1.data_ptr(), m1.data_ptr(),
                                              i1.data_ptr(), p1[0].data_ptr(), x2.data_ptr(), s2.data_ptr(), t2.data_ptr(),
                                              m2.data_ptr(), i2.data_ptr(), p2[0].data_ptr(), *outs, M, C, train, ws.data_ptr(),
                                              wsb, s))
            assert n.n == 3
            torch.cuda.synchronize()
            assert guard_intact(ws, wsb), name
            runs.append((dx1, dx2, dg1, db1, dg2, db2))
        dx1, dx2, dg1, db1, dg2, db2 = runs[0]
        check("dx", dx1, *ra["dx"])
        check("dx", dx2, *rb["dx"])
        check("dgamma", dg1, *ra["dgamma"])
        check("dgamma", dg2, *rb["dgamma"])
        check("dbeta", db1, *ra["dbeta"])
        assert same_bits(db1, db2), "dbeta1 != dbeta2"
        assert all(same_bits(a, b) for a, b in zip(*runs)), "two-branch y_mask form != remask form"
        if M >= 1 << 20 and train:      # determinism of the backward statistics: a second run gives the same bits
            (ex1, ex2), eg = _bwd_outputs(c.dt, M, C, True)
            ws = ws_buf(wsb)
            rt.check(getattr(L, BWD2[c.dt])(dy.data_ptr(), y12.data_ptr(), x1.data_ptr(), m1.data_ptr(), i1.data_ptr(),
                                            p1[0].data_ptr(), x2.data_ptr(), m2.data_ptr(), i2.data_ptr(), p2[0].data_ptr(),
                                            ex1.data_ptr(), ex2.data_ptr(), *[t.data_ptr() for t in eg], M, C, train, ws.data_ptr(),
                                            wsb, s))
            assert all(same_bits(a, b) for a, b in zip([ex1, ex2] + eg, runs[0])), "bn_bwd2 not deterministic"
            del ex1, ex2
        del runs, ra, rb, dx1, dx2


# ---- PReLU -----------------------------------------------------------------------------------------------------------------
def prelu_ref_cpu(x, a):
    """torch's PReLU on the CPU: where(x > 0, x, a x) in fp32, then rounded to the storage type."""
    xf = x.cpu().float()
    return torch.where(xf > 0, xf, a * xf).to(x.dtype)


def prelu_dx_ref_cpu(g, x, a):
    gf, xf = g.cpu().float(), x.cpu().float()
    return torch.where(xf > 0, gf, a * gf).to(x.dtype)


def same_or_both_nan(got, ref):
    got, ref = got.cpu(), ref.cpu()
    nan_g, nan_r = torch.isnan(got.float()), torch.isnan(ref.float())
    return bool((nan_g == nan_r).all()) and bool((bits(got)[~nan_g] == bits(ref)[~nan_r]).all())


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_prelu(c, L):
    from hupr_amd import runtime as rt
    CURRENT[0] = case_id(c)
    R = regime(c.dt, c.M, c.C)
    n = c.M * c.C
    x = make_x(c.dt, c.M, c.C, c.data, 1).view(-1)
    dy = make_x(c.dt, c.M, c.C, "normal", 5).view(-1)
    alpha = torch.tensor([0.25], device="cuda")
    s = rt.stream()
    y = nan_act(c.dt, n)
    with Launches(L) as k:
        rt.check(getattr(L, PRELU_FWD[c.dt])(x.data_ptr(), alpha.data_ptr(), y.data_ptr(), n, s))
    assert k.n == 1
    assert same_or_both_nan(y, prelu_ref_cpu(x, 0.25))
    del y
    wsb = L.hupr_prelu_ws_bytes()
    assert wsb == 4096 * 8
    dx, da, ws = nan_act(c.dt, n), nan32(1), ws_buf(wsb)
    with Launches(L) as k:
        rt.check(getattr(L, PRELU_BWD[c.dt])(dy.data_ptr(), x.data_ptr(), alpha.data_ptr(), dx.data_ptr(), da.data_ptr(), n,
                                             ws.data_ptr(), wsb, s))
    assert k.n == 2
    torch.cuda.synchronize()
    assert guard_intact(ws, wsb)
    assert same_or_both_nan(dx, prelu_dx_ref_cpu(dy, x, 0.25))
    rd = ref_device(c.M)
    ref, b = dalpha_gate(d64(x, rd), d64(dy, rd), R.passes, R.V)
    check("dalpha", da, ref.reshape(1), b.reshape(1))
    # partials + sum_partials_multi = prelu_bwd; the partial count is the mirrored element-wise grid
    dx2, part = nan_act(c.dt, n), ws_buf(wsb)
    npart = __import__("ctypes").c_int(-1)
    with Launches(L) as k:
        rt.check(getattr(L, PRELU_PARTIALS[c.dt])(dy.data_ptr(), x.data_ptr(), alpha.data_ptr(), dx2.data_ptr(), n,
                                                  part.data_ptr(), wsb, npart, s))
    assert k.n == 1 and npart.value == R.grid, (npart.value, R.grid)
    torch.cuda.synchronize()
    assert guard_intact(part, wsb) and bool((part[R.grid:wsb // 8] == PAT).all())
    assert same_bits(dx2, dx)
    out = nan32(1)
    items = (rt.SumItem * 1)()
    items[0].partial, items[0].n, items[0].out = part.data_ptr(), npart.value, out.data_ptr()
    with Launches(L) as k:
        rt.check(L.hupr_sum_partials_multi(items, 1, s))
    assert k.n == 1 and same_bits(out, da)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_prelu_special_values(dt, L):
    """-0.0, subnormals, +-Inf, NaN, and slopes whose products are subnormal or overflow: one correctly rounded multiply."""
    from hupr_amd import runtime as rt
    sub = 1e-40 if dt == "f32" else 1e-39
    vals = torch.tensor([0.0, -0.0, sub, -sub, 1.2e-38, -1.2e-38, float("inf"), float("-inf"), float("nan"), -float("nan"),
                         1.0, -1.0, 3.4e38, -3.4e38, 1e-30, -1e-30, 1.00390625, -1.00390625])
    g = torch.Generator().manual_seed(9)
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (8192,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    x = torch.cat([vals, vals.flip(0), rnd]).to(act_dtype(dt))
    x = x[: x.numel() - x.numel() % 8]
    n = x.numel()
    xg = x.cuda()
    dy = torch.randn(n, generator=g).to(act_dtype(dt))
    dy[: vals.numel()] = vals.to(act_dtype(dt))
    dyg = dy.cuda()
    wsb = L.hupr_prelu_ws_bytes()
    for a in (0.25, -0.5, 1e-30, 3.0e10, 0.0):
        alpha = torch.tensor([a], device="cuda")
        y = nan_act(dt, n)
        rt.check(getattr(L, PRELU_FWD[dt])(xg.data_ptr(), alpha.data_ptr(), y.data_ptr(), n, rt.stream()))
        assert same_or_both_nan(y, prelu_ref_cpu(x, float(alpha.item()))), "prelu fwd alpha=%g" % a
        dx, da, ws = nan_act(dt, n), nan32(1), ws_buf(wsb)
        rt.check(getattr(L, PRELU_BWD[dt])(dyg.data_ptr(), xg.data_ptr(), alpha.data_ptr(), dx.data_ptr(), da.data_ptr(), n,
                                           ws.data_ptr(), wsb, rt.stream()))
        assert same_or_both_nan(dx, prelu_dx_ref_cpu(dy, x, float(alpha.item()))), "prelu dx alpha=%g" % a


@pytest.mark.parametrize("n_items", [1, 16, 17])
def test_sum_partials_multi(n_items, L):
    """n_items PReLU slope gradients finished by one hupr_sum_partials_multi call in ceil(n / 16) launches: each = prelu_bwd."""
    from hupr_amd import runtime as rt
    import ctypes
    s = rt.stream()
    wsb = L.hupr_prelu_ws_bytes()
    items = (rt.SumItem * n_items)()
    keep, want = [], []
    for i in range(n_items):
        dt = "f32" if i % 2 == 0 else "bf16"
        M = 64 + 997 * i
        x = make_x(dt, M, 8, "normal", 20 + i).view(-1)
        dy = make_x(dt, M, 8, "normal", 40 + i).view(-1)
        alpha = torch.tensor([0.1 * i], device="cuda")
        dx, da, ws = nan_act(dt, M * 8), nan32(1), ws_buf(wsb)
        rt.check(getattr(L, PRELU_BWD[dt])(dy.data_ptr(), x.data_ptr(), alpha.data_ptr(), dx.data_ptr(), da.data_ptr(), M * 8,
                                           ws.data_ptr(), wsb, s))
        part, npart, out = ws_buf(wsb), ctypes.c_int(-1), nan32(1)
        rt.check(getattr(L, PRELU_PARTIALS[dt])(dy.data_ptr(), x.data_ptr(), alpha.data_ptr(), dx.data_ptr(), M * 8,
                                                part.data_ptr(), wsb, npart, s))
        items[i].partial, items[i].n, items[i].out = part.data_ptr(), npart.value, out.data_ptr()
        keep += [x, dy, alpha, dx, ws, part]
        want.append((out, da))
    with Launches(L) as k:
        rt.check(L.hupr_sum_partials_multi(items, n_items, s))
    assert k.n == cdiv(n_items, 16)
    assert all(same_bits(o, d) for o, d in want)


# ---- casts -----------------------------------------------------------------------------------------------------------------
def test_casts(L):
    """Round-to-nearest-even ties, overflow to Inf, subnormals, +-0 and NaN, over more elements than one grid-stride pass."""
    from hupr_amd import runtime as rt
    g = torch.Generator().manual_seed(3)
    n = 4 * (4096 * 256 * 2 + 333)
    r = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    k = torch.arange(n)
    # every 4th element a tie (low half 0x8000), every 7th a value near the bf16 overflow threshold
    r = torch.where(k % 4 == 1, (r & ~0xFFFF) | 0x8000, r)
    r = torch.where(k % 7 == 2, (r & -0x80000000) | 0x7F7F0000 | (r & 0xFFFF), r)
    r = torch.where(k % 11 == 3, r & -0x7F800001, r)                    # sign | mantissa: subnormals and +-0
    x = r.view(torch.float32)
    x[:8] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.3895314e38, 3.3961776e38, -1e-45])
    xg = x.cuda()
    y = torch.full((n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    with Launches(L) as c:
        rt.check(L.hupr_cast_f32_to_bf16(xg.data_ptr(), y.data_ptr(), n, rt.stream()))
    assert c.n == 1
    assert same_or_both_nan(y, x.to(torch.bfloat16))
    assert bool(torch.isinf(y.cpu()[x.abs() >= 3.3961776e38]).all())
    hb = torch.randint(-2 ** 15, 2 ** 15 - 1, (n,), generator=g, dtype=torch.int32).to(torch.int16)
    hb[:6] = torch.tensor([0, -32768, 0x7F80, -128, 0x7FC0, 0x0001], dtype=torch.int16)  # +0, -0, Inf, -Inf, NaN, subnormal
    xb = hb.view(torch.bfloat16)
    y32 = nan32(n)
    rt.check(L.hupr_cast_bf16_to_f32(xb.cuda().data_ptr(), y32.data_ptr(), n, rt.stream()))
    assert same_or_both_nan(y32, xb.float())


# ---- inference tails -------------------------------------------------------------------------------------------------------
TAIL_CASES = [(mode, n1, n2) for mode in (0, 1) for n1 in range(4) for n2 in (None, 0, 1, 2, 3)]


def _tail_side(n, M, C, seed, scale):
    """A bf16 tensor (n = 0) or n fp32 slices [n][M][C]; returns (device tensor, its fp32 / bf16 value as the tail sees it before
    rounding, its exact fp64 sum, the fp64 sum of the slices' magnitudes)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if n == 0:
        t = (torch.randn(M, C, generator=g, device="cuda") * scale).to(torch.bfloat16)
        return t, t.float(), t.double(), t.double().abs()
    t = torch.randn(n, M, C, generator=g, device="cuda") * scale
    acc = t[0].clone()
    for j in range(1, n):
        acc = acc + t[j]
    return t, acc, t.double().sum(0), t.double().abs().sum(0)


@pytest.mark.parametrize("mode,n1,n2", TAIL_CASES, ids=["m%d-n%d-%s" % (m, a, "none" if b is None else "n%d" % b)
                                                        for m, a, b in TAIL_CASES])
def test_infer_tail(mode, n1, n2, L):
    from hupr_amd import runtime as rt
    CURRENT[0] = "tail-m%d-n%d-%s" % (mode, n1, n2)
    M, C = 1000, 64
    s = rt.stream()
    x1, v1, e1, a1 = _tail_side(n1, M, C, 1 + n1, 2.0)
    x2, v2, e2, a2 = (None,) * 4 if n2 is None else _tail_side(n2, M, C, 11 + n2, 1.5)
    p1, p2 = bn_params(C, 7), bn_params(C, 8)
    alpha = torch.tensor([0.3], device="cuda")
    y = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device="cuda")
    bn = lambda p: [t.data_ptr() for t in p]
    with Launches(L) as k:
        rt.check(L.hupr_infer_tail_bf16act(mode, x1.data_ptr(), n1, *(bn(p1) if mode == 0 else [None] * 4), EPS,
                                           rt.ptr(x2), n2 or 0, *(bn(p2) if mode == 0 and x2 is not None else [None] * 4), 1e-3,
                                           alpha.data_ptr() if mode == 1 else None, 1, y.data_ptr(), M, C, s))
    assert k.n == 1
    two = x2 is not None
    if mode == 0:       # the composition: slices summed in order in fp32, rounded to bf16, then bn_eval_act
        r1, r2 = v1.to(torch.bfloat16), (v2.to(torch.bfloat16) if two else None)
        want = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device="cuda")
        rt.check(L.hupr_bn_eval_act_bf16act(r1.data_ptr(), *bn(p1), EPS, rt.ptr(r2), *(bn(p2) if two else [None] * 4), 1e-3,
                                            want.data_ptr(), M, C, 1, s))
        assert same_bits(y, want), "infer_tail mode 0 != bf16 rounding + hupr_bn_eval_act_bf16act"
        P1, P2 = [t.double() for t in p1], [t.double() for t in p2]
        sc1 = P1[0] / torch.sqrt(P1[3] + float(torch.tensor(EPS, dtype=torch.float32)))
        ref = e1 * sc1 + (P1[1] - P1[2] * sc1)
        A = a1 * sc1.abs()
        B = (P1[1] - P1[2] * sc1).abs() + (P1[2] * sc1).abs()
        if two:
            sc2 = P2[0] / torch.sqrt(P2[3] + float(torch.tensor(1e-3, dtype=torch.float32)))
            ref = ref + e2 * sc2 + (P2[1] - P2[2] * sc2)
            A = A + a2 * sc2.abs()
            B = B + (P2[1] - P2[2] * sc2).abs() + (P2[2] * sc2).abs()
        ref = ref.clamp(min=0)
        b = (BF16_U + (n1 + (n2 or 0) + 6) * U) * A + 6 * U * B
        check("tail_y", y, ref, b + BF16_U * (ref.abs() + b))
    else:               # prelu(c1 + c2): c2 rounded as stored, the sum rounded once, then hupr_prelu_fwd_bf16act
        z = (v1 + v2.to(torch.bfloat16).float() if two else v1).to(torch.bfloat16)
        want = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device="cuda")
        rt.check(L.hupr_prelu_fwd_bf16act(z.data_ptr(), alpha.data_ptr(), want.data_ptr(), M * C, s))
        assert same_bits(y, want), "infer_tail mode 1 != bf16 rounding + hupr_prelu_fwd_bf16act"
        e = e1 + (e2 if two else 0)
        a = float(alpha.item())
        ref = torch.where(e > 0, e, a * e)
        A = a1 + (2 * a2 if two else 0)
        nsl = max(n1, 1) + max(n2 or 0, 1)
        b = max(1.0, abs(a)) * (BF16_U * A + nsl * U * A)
        check("tail_y", y, ref, b + BF16_U * (ref.abs() + b))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(L):
    """Each refused call returns its documented code, launches nothing and leaves its NaN-filled outputs untouched."""
    from hupr_amd import runtime as rt
    s = rt.stream()
    M, C = 256, 64
    x = make_x("f32", M, C, "normal", 1)
    xb = make_x("bf16", M, C, "normal", 1)
    p = bn_params(1024 + 8, 2)
    g, b, rm, rv = (t.data_ptr() for t in p)
    o = [nan32(1032) for _ in range(8)]
    y, yb = nan_act("f32", M, C), nan_act("bf16", M, C)
    wsb = L.hupr_bn_ws_bytes(1032)
    ws = ws_buf(wsb)
    keep = [t.clone() for t in o + [y, yb, ws] + p]

    def refused(code, rc, why):
        assert rc == code, "%s: rc %d" % (why, rc)

    def untouched():
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip(o + [y, yb, ws] + p, keep)), "a refused call wrote its outputs"

    n0 = L.hupr_launch_count()
    st = lambda L_fn, xp, M_, C_, wsb_=wsb, sm=o[0].data_ptr(): L_fn(xp, M_, C_, g, b, rm, rv, MOM, EPS, sm, o[1].data_ptr(),
                                                                     o[2].data_ptr(), o[3].data_ptr(), ws.data_ptr(), wsb_, s)
    refused(HUPR_ERR_ARG, st(L.hupr_bn_train_stats_bf16act, xb.data_ptr(), M, 12), "bf16 C % 8")
    refused(HUPR_ERR_ARG, st(L.hupr_bn_train_stats_f32, x.data_ptr(), M, 6), "f32 C % 4")
    refused(HUPR_ERR_ARG, st(L.hupr_bn_train_stats_f32, x.data_ptr(), 16, 1028), "C = 1028")
    refused(HUPR_ERR_ARG, st(L.hupr_bn_train_stats_f32, x.data_ptr(), 0, C), "M = 0")
    refused(HUPR_ERR_ARG, st(L.hupr_bn_train_stats_f32, x.data_ptr(), M, C, sm=None), "null save_mean")
    refused(HUPR_ERR_WORKSPACE, st(L.hupr_bn_train_stats_f32, x.data_ptr(), M, C, L.hupr_bn_ws_bytes(C) - 1), "ws one byte short")
    refused(HUPR_ERR_WORKSPACE, st(L.hupr_bn_train_stats_bf16act, xb.data_ptr(), M, C, L.hupr_bn_ws_bytes(C) - 1), "ws short")
    refused(HUPR_ERR_ARG, L.hupr_colsum_f32(x.data_ptr(), M, 1028, o[0].data_ptr(), ws.data_ptr(), wsb, s), "colsum C = 1028")
    refused(HUPR_ERR_ARG, L.hupr_colsum_bf16act(xb.data_ptr(), M, 12, o[0].data_ptr(), ws.data_ptr(), wsb, s), "colsum bf16 C % 8")
    refused(HUPR_ERR_WORKSPACE, L.hupr_colsum_f32(x.data_ptr(), M, C, o[0].data_ptr(), ws.data_ptr(), L.hupr_bn_ws_bytes(C) - 1, s),
            "colsum ws short")
    refused(HUPR_ERR_ARG, L.hupr_bn_train_finalize_f32(ws.data_ptr(), 0, M, C, g, b, rm, rv, MOM, EPS,
                                                       *[t.data_ptr() for t in o[:4]], s), "finalize nblk = 0")
    refused(HUPR_ERR_ARG, L.hupr_bn_train_finalize2_f32(ws.data_ptr(), 1, g, b, rm, rv, MOM, EPS, *[t.data_ptr() for t in o[:4]],
                                                        None, 1, g, b, rm, rv, MOM, EPS, *[t.data_ptr() for t in o[4:]], M, C, s),
            "finalize2 null partial2")
    refused(HUPR_ERR_ARG, L.hupr_bn_eval_params_f32(g, b, rm, None, EPS, C, o[0].data_ptr(), o[1].data_ptr(), s), "eval_params null")
    for fn, xp, yp in ((L.hupr_scale_shift_act_f32, x.data_ptr(), y.data_ptr()), (L.hupr_scale_shift_act_bf16act, xb.data_ptr(),
                                                                                  yb.data_ptr())):
        refused(HUPR_ERR_ARG, fn(xp, g, b, xp, None, b, yp, M, C, 1, s), "second branch without scale")
        refused(HUPR_ERR_ARG, fn(xp, g, b, None, None, None, yp, M, 1028, 1, s), "C = 1028")
        refused(HUPR_ERR_ARG, fn(xp, g, b, None, None, None, yp, 0, C, 1, s), "M = 0")
    refused(HUPR_ERR_ARG, L.hupr_scale_shift_act_bf16act(xb.data_ptr(), g, b, None, None, None, yb.data_ptr(), M, 12, 1, s), "C % 8")
    for fn, xp, yp in ((L.hupr_bn_eval_act_f32, x.data_ptr(), y.data_ptr()), (L.hupr_bn_eval_act_bf16act, xb.data_ptr(),
                                                                              yb.data_ptr())):
        refused(HUPR_ERR_ARG, fn(xp, g, b, rm, rv, EPS, xp, g, b, None, rv, EPS, yp, M, C, 1, s), "second branch without mean")
        refused(HUPR_ERR_ARG, fn(xp, g, b, rm, rv, EPS, None, None, None, None, None, EPS, yp, M, 1028, 1, s), "C = 1028")
    # backward: the forms without a y_mask parameter refuse a missing scale / shift; bn_bwd2 refuses a missing mask; C, M, ws
    dx, dxb = y, yb
    d = [t.data_ptr() for t in o]
    for dt, xp, dxp in (("f32", x.data_ptr(), dx.data_ptr()), ("bf16", xb.data_ptr(), dxb.data_ptr())):
        bwd = getattr(L, BWD[dt])
        refused(HUPR_ERR_ARG, bwd(xp, xp, xp, rm, rv, g, dxp, d[0], d[1], M, 1028, 1, ws.data_ptr(), wsb, s), "bwd C = 1028")
        refused(HUPR_ERR_ARG, bwd(xp, xp, xp, rm, rv, g, dxp, d[0], d[1], 0, C, 1, ws.data_ptr(), wsb, s), "bwd M = 0")
        refused(HUPR_ERR_ARG, bwd(xp, xp, xp, rm, rv, None, dxp, d[0], d[1], M, C, 1, ws.data_ptr(), wsb, s), "bwd null gamma")
        refused(HUPR_ERR_WORKSPACE, bwd(xp, xp, xp, rm, rv, g, dxp, d[0], d[1], M, C, 1, ws.data_ptr(), L.hupr_bn_ws_bytes(C) - 1, s),
                "bwd ws short")
        rem = getattr(L, BWD_REMASK[dt])
        refused(HUPR_ERR_ARG, rem(xp, g, None, xp, rm, rv, g, dxp, d[0], d[1], M, C, 1, ws.data_ptr(), wsb, s), "remask null shift")
        refused(HUPR_ERR_ARG, rem(xp, g, b, xp, rm, rv, g, dxp, d[0], d[1], M, C + 2, 1, ws.data_ptr(), wsb, s), "remask C % V")
        b2 = getattr(L, BWD2[dt])
        args2 = lambda mask, C_=C, wsb_=wsb: b2(xp, mask, xp, rm, rv, g, xp, rm, rv, g, dxp, dxp, *d[:4], M, C_, 1, ws.data_ptr(),
                                                wsb_, s)
        refused(HUPR_ERR_ARG, args2(None), "bwd2 without a mask")
        refused(HUPR_ERR_ARG, args2(xp, 1028), "bwd2 C = 1028")
        refused(HUPR_ERR_WORKSPACE, args2(xp, C, L.hupr_bn_ws_bytes(C) - 1), "bwd2 ws short")
        r2 = getattr(L, BWD2_REMASK[dt])
        refused(HUPR_ERR_ARG, r2(xp, xp, g, b, rm, rv, g, xp, g, None, rm, rv, g, dxp, dxp, *d[:4], M, C, 1, ws.data_ptr(), wsb, s),
                "bwd2 remask missing shift2")
        refused(HUPR_ERR_WORKSPACE, r2(xp, xp, g, b, rm, rv, g, xp, g, b, rm, rv, g, dxp, dxp, *d[:4], M, C, 1, ws.data_ptr(),
                                       L.hupr_bn_ws_bytes(C) - 1, s), "bwd2 remask ws short")
        # PReLU
        pw = L.hupr_prelu_ws_bytes()
        refused(HUPR_ERR_ARG, getattr(L, PRELU_FWD[dt])(xp, g, dxp, 6, s), "prelu n % V")
        refused(HUPR_ERR_ARG, getattr(L, PRELU_FWD[dt])(xp, None, dxp, M * C, s), "prelu null alpha")
        refused(HUPR_ERR_WORKSPACE, getattr(L, PRELU_BWD[dt])(xp, xp, g, dxp, d[0], M * C, ws.data_ptr(), pw - 1, s), "prelu ws short")
        refused(HUPR_ERR_ARG, getattr(L, PRELU_BWD[dt])(xp, xp, g, dxp, None, M * C, ws.data_ptr(), pw, s), "prelu null dalpha")
        npart = __import__("ctypes").c_int(-1)
        refused(HUPR_ERR_ARG, getattr(L, PRELU_PARTIALS[dt])(xp, xp, g, dxp, 0, ws.data_ptr(), pw, npart, s), "partials n = 0")
        refused(HUPR_ERR_WORKSPACE, getattr(L, PRELU_PARTIALS[dt])(xp, xp, g, dxp, M * C, ws.data_ptr(), pw - 1, npart, s),
                "partials ws short")
    # casts
    refused(HUPR_ERR_ARG, L.hupr_cast_f32_to_bf16(x.data_ptr(), yb.data_ptr(), 6, s), "cast n % 4")
    refused(HUPR_ERR_ARG, L.hupr_cast_bf16_to_f32(xb.data_ptr(), None, M * C, s), "cast null y")
    # sum_partials_multi: a bad item anywhere refuses the whole call, also when it lies in the second launch's 16
    items = (rt.SumItem * 17)()
    for i in range(17):
        items[i].partial, items[i].n, items[i].out = ws.data_ptr(), 4, o[i % 8].data_ptr()
    items[16].out = None
    refused(HUPR_ERR_ARG, L.hupr_sum_partials_multi(items, 17, s), "item 16 without out")
    items[16].out, items[3].n = o[0].data_ptr(), 0
    refused(HUPR_ERR_ARG, L.hupr_sum_partials_multi(items, 17, s), "item 3 with n = 0")
    refused(HUPR_ERR_ARG, L.hupr_sum_partials_multi(items, 0, s), "no items")
    # infer_tail: misaligned pointers, mode 0 without BatchNorm tensors, mode 1 without a slope
    yt = yb.view(-1)
    sl = torch.zeros(2, M, C, device="cuda")
    keep.append(sl.clone())
    tail = lambda mode, x1, n1, x2, n2, yp, bnp=(g, b, rm, rv), al=None: L.hupr_infer_tail_bf16act(
        mode, x1, n1, *bnp, EPS, x2, n2, *bnp, EPS, al, 1, yp, M - 1, C, s)
    refused(HUPR_ERR_ARG, tail(0, xb.data_ptr() + 2, 0, None, 0, yt.data_ptr()), "x1 misaligned")
    refused(HUPR_ERR_ARG, tail(0, xb.data_ptr(), 0, xb.data_ptr() + 4, 0, yt.data_ptr()), "x2 misaligned")
    refused(HUPR_ERR_ARG, tail(0, xb.data_ptr(), 0, None, 0, yt.data_ptr() + 2), "y misaligned")
    refused(HUPR_ERR_ARG, tail(0, sl.data_ptr() + 8, 2, None, 0, yt.data_ptr()), "slices misaligned")
    refused(HUPR_ERR_ARG, tail(0, xb.data_ptr(), 0, sl.data_ptr() + 8, 1, yt.data_ptr()), "x2 slices misaligned")
    refused(HUPR_ERR_ARG, tail(0, xb.data_ptr(), 0, None, 0, yt.data_ptr(), bnp=(g, b, None, rv)), "mode 0 without mean")
    refused(HUPR_ERR_ARG, tail(1, xb.data_ptr(), 0, None, 0, yt.data_ptr(), bnp=(None,) * 4), "mode 1 without alpha")
    refused(HUPR_ERR_ARG, tail(2, xb.data_ptr(), 0, None, 0, yt.data_ptr(), al=g), "mode 2")
    refused(HUPR_ERR_ARG, tail(0, xb.data_ptr(), -1, None, 0, yt.data_ptr()), "n1 < 0")
    assert L.hupr_launch_count() == n0, "a refused call launched a kernel"
    untouched()
    assert bool((sl == 0).all())


def test_zz_report_worst_ratios():
    """Prints the worst error-to-bound ratio per quantity and the measured save_invstd precision (run with -s to see it)."""
    for k in sorted(WORST):
        print("\nworst err / bound of %s: %.3g (%s)" % (k, WORST[k][0], WORST[k][1]), end="")
    for k in sorted(PRECISION):
        kr, tr, vk, vt = PRECISION[k]
        print("\n%s: save_invstd max rel err %.3g (torch fp32 BatchNorm %.3g); max |1/invstd^2 - eps| %.3g (torch %.3g)"
              % (k, kr, tr, vk, vt), end="")
    print()
    assert all(v <= 1.0 for v, _ in WORST.values())
