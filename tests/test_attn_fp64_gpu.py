"""GPU (-m gpu): every entry point and kernel route of the fused MSCSA attention (csrc/attention_bf16.hip) against an fp64 attention
of exactly the operands the kernels see, element by element, with the route of every case asserted first (hupr_attn_route).

Operands: bf16 K, V, dO; the query is Q' = log2(e) Q rounded to bf16 for the QS entries (the reference uses Q' / log2(e)) and bf16 Q
otherwise; the fp32-operand entries get fp32 tensors and the reference rounds them to bf16 as the kernels do.  The exact terms (the
residual V, the fp32 gradient of the row sum and of the residual dV) are the fp32 tensors the call is given.

Gate (``within_gate``), with P the fp64 softmax over keys j of s_jk = K_j . Q_k, dP_jk = V_j . dO_k, D_k = sum_c dO_kc out_kc and
E_jk = |dP_jk| + |D_k| + sum_c |dO_kc| A_out,kc:
    |got - ref| <= c A + 2^-22 |ref| (+ 2^-24 |term| for a residual or accumulated term) + 2^-126 U
    out  A_out = P^T |V|                  c = 2^-7
    dV   A_dV  = sum_k P_jk |dO_k|        c = 2^-7
    dQ   A_dQ  = sum_j P_jk E_jk |K_j|    c = 2^-6
    dK   A_dK  = sum_k P_jk E_jk |Q_k|    c = 2^-6
    lse  |got - ref| <= 2^-14 (1 + max_j |s_jk|)
U is the same sum with every P_jk replaced by 1 (E_jk by max E): probabilities below 2^-126 (the moving-maximum profile reaches
e^-100) are subnormal in fp32 and bf16 and lose their relative precision, never more than 2^-126 each.
The bf16 roundings of P and dS the kernels make stay within 2^-9 A; tests/test_attn_route.py shows that the gate accepts them and
rejects a missing key tile, swapped log-sum-exps, a missing query tile of dK and a wrong dV epilogue — without a GPU.
Batch items {0, 1, B // 2, B - 1} are compared.  Strided inputs hold NaN past their C columns; strided outputs are NaN-filled and
their padding must come back NaN bit for bit.  The batch entries must match the same items issued as single calls bit for bit."""
import collections
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG = -1
# hupr_attn_route codes (include/hupr.h)
PP64, ONE_PASS, SPLIT = 1, 2, 3
DKV512, NH1, NH2 = 4, 8, 12
XMAP = 16
LOG2E = math.log2(math.e)
C_OUT, C_DV, C_DQ, C_DK = 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6
NAN16, NAN32 = 0x7FC1, 0x7FC00001          # quiet NaNs with a payload no arithmetic produces
WORST = {}                                 # quantity -> (worst |got - ref| / bound seen, case) (printed by the last test)
CURRENT = [""]                             # the case being checked


def route(fwd, dkv, xmap=False, S=1):
    return fwd | dkv | (XMAP if xmap else 0) | (S << 8)


# ---- the fp64 reference and the gate (CPU) -----------------------------------------------------------------------------
def reference(k, q, v, g, g32=None, vres=None, keep=False):
    """fp64 attention of one batch item: k, q, v, g [N, C] as the matrix pipe sees them (q unscaled), g32 the gradient of the exact
    terms (row sum D, residual dV; default g), vres the residual added to out (or None).  Returns references and bound weights."""
    k, q, v, g = (t.double() for t in (k, q, v, g))
    g32 = g if g32 is None else g32.double()
    s = k @ q.T                                             # [keys j, queries k]
    lse = torch.logsumexp(s, 0)
    P = torch.exp(s - lse)
    out = P.T @ v
    A_out = P.T @ v.abs()
    dP = v @ g.T
    D = (g32 * out).sum(1)
    E = dP.abs() + D.abs() + (g32.abs() * A_out).sum(1)
    dS = P * (dP - D)
    PE = P * E
    Emax = E.max()
    r = dict(out=out, lse=lse, dV=P @ g, dQ=dS.T @ k, dK=dS @ q, A_out=A_out, A_dV=P @ g.abs(), A_dQ=PE.T @ k.abs(),
             A_dK=PE @ q.abs(), smax=s.abs().amax(0), g32=g32, U_out=v.abs().sum(0), U_dV=g.abs().sum(0),
             U_dQ=Emax * k.abs().sum(0), U_dK=Emax * q.abs().sum(0))
    if vres is not None:
        r["out"] = out + vres.double()
        r["res"] = vres.double()
    if keep:
        r.update(P=P, dS=dS, s=s, dP=dP, D=D, k=k, q=q, v=v, g=g)
    return r


def gate_bound(ref, A, c, terms=(), U=0.0):
    b = c * A + 2.0 ** -22 * ref.abs() + 2.0 ** -126 * U
    for t in terms:
        b = b + 2.0 ** -24 * t.double().abs()
    return b


def within_gate(got, ref, A, c, terms=(), U=0.0):
    """True where got meets the gate (a NaN never does)."""
    return (got.double() - ref).abs() <= gate_bound(ref, A, c, terms, U)


def lse_within(got, r):
    return (got.double() - r["lse"]).abs() <= 2.0 ** -14 * (1.0 + r["smax"])


def _ratio(err, b):
    return torch.where(err == 0, torch.zeros_like(err), err / b).nan_to_num(float("inf"))


def _note(what, ratio):
    w = ratio.max().item()
    if what not in WORST or w > WORST[what][0]:
        WORST[what] = (w, CURRENT[0])


def assert_gate(what, got, ref, A, c, terms=(), U=0.0):
    got = got.detach().cpu()
    b = gate_bound(ref, A, c, terms, U)
    ratio = _ratio((got.double() - ref).abs(), b)
    _note(what, ratio)
    ok = within_gate(got, ref, A, c, terms, U)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d outside the gate, first at %s (got %r, ref %r), worst err / bound %.3g"
                             % (what, bad.shape[0], ok.numel(), i, got[i].item(), ref[i].item(), ratio.max().item()))


def assert_lse(got, r):
    got = got.detach().cpu()
    ratio = _ratio((got.double() - r["lse"]).abs(), 2.0 ** -14 * (1.0 + r["smax"]))
    _note("lse", ratio)
    assert bool(lse_within(got, r).all()), "lse: worst err / bound %.3g" % ratio.max().item()


def items(B):
    return sorted({0, 1, B // 2, B - 1}) if B > 4 else list(range(B))


# ---- operands ----------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def moving_profile(N):
    """Key norms that grow slowly, jump, stay high and fall along the key axis (test_flash_attention_qs_deferred_maximum at
    N = 1024): the running maximum keeps moving, deferred and rescaled."""
    q = N // 4
    return torch.cat([torch.linspace(0.05, 0.3, q), torch.linspace(0.3, 3.0, q), torch.full((q,), 6.0), torch.linspace(6.0, 0.1, q)])


def operands(B, N, C, regime, seed, qs):
    """fp32 K, Q, V, dO of one attention in a logit regime -> dict with the bf16 operands and the matrix-pipe values of the reference
    (qr: the unscaled query the kernels effectively multiply by)."""
    ks = {"mild": C ** -0.25, "peaky": (12.0 / C ** 0.5) ** 0.5, "moving": 1.0, "zero": C ** -0.25}[regime]
    k, q = rnd(B, N, C, seed=seed, scale=ks), rnd(B, N, C, seed=seed + 1, scale=ks)
    v, g = rnd(B, N, C, seed=seed + 2), rnd(B, N, C, seed=seed + 3)
    if regime == "moving":
        k = k * moving_profile(N)[None, :, None]
    if regime == "zero":
        k = torch.zeros_like(k)
    kb, vb, gb = k.bfloat16(), v.bfloat16(), g.bfloat16()
    if qs:
        qb = (q * LOG2E).bfloat16()
        qr = qb.double() / LOG2E
    else:
        qb = q.bfloat16()
        qr = qb.double()
    return dict(k32=k, q32=q, v32=v, g32=g, kb=kb, qb=qb, vb=vb, gb=gb, qr=qr)


def nan_buffer(shape, dtype):
    n = 1
    for d in shape:
        n *= d
    if dtype == torch.bfloat16:
        return torch.full((n,), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16).view(*shape)
    return torch.full((n,), NAN32, dtype=torch.int32, device="cuda").view(torch.float32).view(*shape)


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def assert_nan_outside(buf, blocks, what):
    """Every column of the NaN-filled buffer [B, N, ld] outside the written column blocks [(start, width)] is still NaN, bit for bit."""
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    for c0, w in blocks:
        keep[c0:c0 + w] = False
    nan = NAN16 if buf.dtype == torch.bfloat16 else NAN32
    assert bool((bits(buf[..., keep]) == nan).all()), "%s: a padding column was written" % what


def col(buf, slot, C):
    """Address of column block `slot` (width C) of a [B, N, ld] buffer."""
    return buf.data_ptr() + slot * C * buf.element_size()


# ---- the case table ----------------------------------------------------------------------------------------------------
# fwd: "f32" hupr_attn_fwd_bf16 + hupr_attn_bwd_bf16 (fp32 operands); "bf16in" the _bf16in pair; "ld" hupr_attn_fwd_bf16in_ld +
# hupr_attn_bwd_bf16in_ld; "ld_ws" / "ld_ws_qs" hupr_attn_fwd_bf16in_ld_ws(_qs) + hupr_attn_bwd_bf16in_ld(_qs).
# bwd: "dout32" (the fp32 gradient given: prep<float>, add32 residual), "bf16" (dout32 = NULL: prep<bf16>, add16 residual), "acc"
# (accumulate = 1 onto a prefilled dV).  strided: K and Q in slots 0 / 1 of 4C-wide bf16 rows (slots 2 / 3 NaN), dO in slot 1 of a
# NaN-filled 4C-wide bf16 gradient, dK / dQ in slots 2 / 0 of NaN-filled 4C-wide fp32 tensors, out16 in slot 3 of a NaN-filled
# 4C-wide bf16 tensor.  split: the hupr_debug_attn_split mode for a call given a workspace (None: no workspace).
Case = collections.namedtuple("Case", "fwd B N C regime residual bwd strided split route")
CASES = [
    # fp32 operands (TI = float): no ping-pong / 512-thread kernels at any shape
    Case("f32", 2, 256, 64, "mild", True, "dout32", False, None, route(ONE_PASS, NH1)),
    Case("f32", 3, 128, 128, "peaky", False, "dout32", False, None, route(ONE_PASS, NH1)),
    Case("f32", 2, 256, 256, "mild", True, "dout32", False, None, route(ONE_PASS, NH2)),
    # pre-rounded bf16 operands, contiguous
    Case("bf16in", 2, 384, 64, "mild", True, "dout32", False, None, route(ONE_PASS, NH1)),
    Case("bf16in", 2, 1024, 64, "peaky", False, "dout32", False, None, route(PP64, DKV512)),
    # strided (the level's layout), rounds-1-4 kernels
    Case("ld", 3, 384, 64, "mild", True, "dout32", True, None, route(ONE_PASS, NH1)),
    Case("ld", 8, 512, 64, "mild", True, "bf16", True, None, route(PP64, DKV512, xmap=True)),
    Case("ld", 2, 256, 128, "peaky", False, "acc", True, None, route(ONE_PASS, NH1)),
    Case("ld", 3, 256, 256, "mild", False, "bf16", True, None, route(ONE_PASS, NH2)),
    # key-split forward: forced at Bn > 1, the default at Bn = 1, switched off (-1)
    Case("ld_ws", 3, 256, 128, "mild", True, "dout32", True, 1, route(SPLIT, NH1, S=4)),
    Case("ld_ws", 1, 1024, 64, "peaky", False, "bf16", False, 0, route(SPLIT, DKV512, S=16)),
    Case("ld_ws", 1, 1024, 64, "mild", True, "bf16", True, -1, route(PP64, DKV512)),
    # QS kernels (the training default)
    Case("ld_ws_qs", 2, 4096, 64, "mild", True, "bf16", True, None, route(PP64, DKV512)),
    Case("ld_ws_qs", 8, 512, 64, "mild", False, "acc", True, None, route(PP64, DKV512, xmap=True)),
    Case("ld_ws_qs", 8, 1024, 64, "moving", False, "bf16", False, None, route(PP64, DKV512, xmap=True)),
    Case("ld_ws_qs", 2, 384, 64, "mild", True, "dout32", True, None, route(ONE_PASS, NH1)),
    Case("ld_ws_qs", 3, 384, 64, "peaky", True, "bf16", True, None, route(ONE_PASS, NH1)),
    Case("ld_ws_qs", 2, 128, 64, "zero", False, "bf16", True, None, route(ONE_PASS, NH1)),
    Case("ld_ws_qs", 2, 1024, 64, "zero", True, "dout32", False, None, route(PP64, DKV512)),
    Case("ld_ws_qs", 3, 1024, 128, "peaky", False, "acc", True, None, route(ONE_PASS, NH1)),
    Case("ld_ws_qs", 8, 128, 128, "peaky", True, "bf16", True, None, route(ONE_PASS, NH1, xmap=True)),
    Case("ld_ws_qs", 2, 256, 256, "mild", True, "dout32", True, None, route(ONE_PASS, NH2)),
    Case("ld_ws_qs", 8, 256, 256, "moving", False, "acc", True, None, route(ONE_PASS, NH2, xmap=True)),
    Case("ld_ws_qs", 1, 384, 256, "mild", False, "bf16", True, 0, route(SPLIT, NH2, S=2)),
    Case("ld_ws_qs", 3, 256, 64, "peaky", True, "bf16", True, 1, route(SPLIT, DKV512, S=4)),
    Case("ld_ws_qs", 1, 128, 128, "moving", True, "dout32", False, -1, route(ONE_PASS, NH1)),
]


def case_id(c):
    return "%s-B%d-N%d-C%d-%s-%s-%s%s%s" % (c.fwd, c.B, c.N, c.C, c.regime, "res" if c.residual else "nores", c.bwd,
                                           "-strided" if c.strided else "", "" if c.split is None else "-split%d" % c.split)


def route_of(L, c):
    ldk = 4 * c.C if c.strided else c.C
    return L.hupr_attn_route(c.B, c.N, c.C, ldk, int(c.fwd != "f32"), int(c.split is not None))


@pytest.fixture(scope="module")
def L():
    from hupr_amd import runtime
    L = runtime.lib()
    L.hupr_debug_attn_split(0)
    return L


def _qs(c):
    return c.fwd.endswith("_qs")


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_attention_case_vs_fp64(c, L):
    from hupr_amd import runtime as rt
    assert c.fwd in ("f32", "bf16in", "ld", "ld_ws", "ld_ws_qs") and c.bwd in ("dout32", "bf16", "acc")
    assert not (c.bwd == "acc" and c.residual) and (c.fwd in ("ld", "ld_ws", "ld_ws_qs") or (c.bwd == "dout32" and not c.strided))
    CURRENT[0] = case_id(c)
    try:
        L.hupr_debug_attn_split(c.split or 0)
        assert route_of(L, c) == c.route
        _run_case(c, L, rt)
    finally:
        L.hupr_debug_attn_split(0)


def _run_case(c, L, rt):
    B, N, C = c.B, c.N, c.C
    o = operands(B, N, C, c.regime, 1000 + 17 * CASES.index(c), _qs(c))
    dev = lambda t: t.cuda().contiguous()
    W = 4 * C if c.strided else C
    # operands
    if c.fwd == "f32":
        kd, qd, vd, gd = dev(o["k32"]), dev(o["q32"]), dev(o["v32"]), dev(o["g32"])
        kp, qp = kd.data_ptr(), qd.data_ptr()
    else:
        vd, gd = dev(o["vb"]), dev(o["gb"])
        if c.strided:
            proj = nan_buffer((B, N, W), torch.bfloat16)
            proj[..., :C] = o["kb"].cuda()
            proj[..., C:2 * C] = o["qb"].cuda()
            kp, qp = col(proj, 0, C), col(proj, 1, C)
            gbuf = nan_buffer((B, N, W), torch.bfloat16)
            gbuf[..., C:2 * C] = o["gb"].cuda()
            gp = col(gbuf, 1, C)
        else:
            kd, qd = dev(o["kb"]), dev(o["qb"])
            kp, qp, gp = kd.data_ptr(), qd.data_ptr(), gd.data_ptr()
    v32d, g32d = dev(o["v32"]), dev(o["g32"])
    out = nan_buffer((B, N, C), torch.float32)
    lse = nan_buffer((B, N), torch.float32)
    o16, ld16 = None, 0
    if c.fwd in ("ld", "ld_ws", "ld_ws_qs"):
        o16, ld16 = nan_buffer((B, N, W), torch.bfloat16), W
    vres = v32d if c.residual else None
    s = rt.stream()
    # forward
    if c.fwd == "f32":
        rt.check(L.hupr_attn_fwd_bf16(kp, qp, vd.data_ptr(), rt.ptr(out), rt.ptr(lse), B, N, C, int(c.residual), s))
    elif c.fwd == "bf16in":
        rt.check(L.hupr_attn_fwd_bf16in(kp, qp, rt.ptr(vd), rt.ptr(vres), rt.ptr(out), rt.ptr(lse), B, N, C, s))
    elif c.fwd == "ld":
        rt.check(L.hupr_attn_fwd_bf16in_ld(kp, W, qp, W, rt.ptr(vd), rt.ptr(vres), rt.ptr(out), rt.ptr(lse), col(o16, W // C - 1, C),
                                           ld16, B, N, C, s))
    else:
        nbytes = L.hupr_attn_fwd_split_ws_bytes(B, N, C) if c.split is not None else 0
        assert (nbytes > 0) == ((c.route & 3) == SPLIT)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda") if c.split is not None else None
        fwd = L.hupr_attn_fwd_bf16in_ld_ws_qs if _qs(c) else L.hupr_attn_fwd_bf16in_ld_ws
        rt.check(fwd(kp, W, qp, W, rt.ptr(vd), rt.ptr(vres), rt.ptr(out), rt.ptr(lse), col(o16, W // C - 1, C), ld16, B, N, C,
                     rt.ptr(ws), nbytes, s))
    # backward
    slot_dk, slot_dq = (2, 0) if c.strided else (0, 0)
    dK, dQ = nan_buffer((B, N, W), torch.float32), nan_buffer((B, N, W), torch.float32)
    dv0 = rnd(B, N, C, seed=77 + B * N)
    dV = dv0.cuda() if c.bwd == "acc" else nan_buffer((B, N, C), torch.float32)
    scr = torch.empty((B, N), device="cuda")
    res, acc = int(c.residual), int(c.bwd == "acc")
    g32p = rt.ptr(g32d) if c.bwd in ("dout32",) or c.fwd in ("f32", "bf16in") else None
    if c.fwd == "f32":
        rt.check(L.hupr_attn_bwd_bf16(kp, qp, vd.data_ptr(), rt.ptr(out), g32p, rt.ptr(lse), rt.ptr(dK), rt.ptr(dQ), rt.ptr(dV),
                                      rt.ptr(scr), B, N, C, res, s))
    elif c.fwd == "bf16in":
        rt.check(L.hupr_attn_bwd_bf16in(kp, qp, rt.ptr(vd), rt.ptr(gd), rt.ptr(v32d), rt.ptr(out), g32p, rt.ptr(lse), rt.ptr(dK),
                                        rt.ptr(dQ), rt.ptr(dV), rt.ptr(scr), B, N, C, res, s))
    else:
        bwd = L.hupr_attn_bwd_bf16in_ld_qs if _qs(c) else L.hupr_attn_bwd_bf16in_ld
        rt.check(bwd(kp, W, qp, W, rt.ptr(vd), gp, W, rt.ptr(v32d), rt.ptr(out), g32p, rt.ptr(lse), col(dK, slot_dk, C), W,
                     col(dQ, slot_dq, C), W, rt.ptr(dV), rt.ptr(scr), B, N, C, res, acc, s))
    torch.cuda.synchronize()
    # exact pins: the bf16 copy of out, untouched padding
    if o16 is not None:
        blk = W // C - 1
        assert torch.equal(bits(o16[..., blk * C:(blk + 1) * C]), bits(out.bfloat16())), "out16 != out rounded to bf16"
        assert_nan_outside(o16, [(blk * C, C)], "out16")
    if c.strided:
        assert_nan_outside(dK, [(slot_dk * C, C)], "dK")
        assert_nan_outside(dQ, [(slot_dq * C, C)], "dQ")
    dK, dQ = dK[..., slot_dk * C:(slot_dk + 1) * C].cpu(), dQ[..., slot_dq * C:(slot_dq + 1) * C].cpu()
    out, lse, dV = out.cpu(), lse.cpu(), dV.cpu()
    g32 = o["g32"] if g32p is not None else o["gb"].float()
    for b in items(B):
        r = reference(o["kb"][b], o["qr"][b], o["vb"][b], o["gb"][b], g32[b], o["v32"][b] if c.residual else None)
        tag = "%s item %d" % (case_id(c), b)
        assert_gate("out", out[b], r["out"], r["A_out"], C_OUT, [r["res"]] if c.residual else (), r["U_out"])
        assert_lse(lse[b], r)
        refv, terms = r["dV"], []
        if c.residual:
            refv, terms = refv + r["g32"], [r["g32"]]
        if c.bwd == "acc":
            refv, terms = refv + dv0[b].double(), [dv0[b]]
        assert_gate("dV", dV[b], refv, r["A_dV"], C_DV, terms, r["U_dV"])
        assert_gate("dQ", dQ[b], r["dQ"], r["A_dQ"], C_DQ, (), r["U_dQ"])
        assert_gate("dK", dK[b], r["dK"], r["A_dK"], C_DK, (), r["U_dK"])
        if c.regime == "zero":
            assert bool((dQ[b] == 0).all()), "%s: K = 0 must give dQ = 0 exactly" % tag
            mean = o["vb"][b].double().mean(0) + (o["v32"][b].double() if c.residual else 0)
            assert_gate("out", out[b], mean.expand(N, C) if not c.residual else mean, r["A_out"], C_OUT,
                        [r["res"]] if c.residual else ())


# ---- the batch entries: an MSCSA level's layout ------------------------------------------------------------------------
#            K source/slot, Q source/slot, V map (0: ra, 1: re), residual  (functional.MSCSALevelFn.SPEC)
SPEC = ((0, 0, 1, 1, 0, True), (0, 2, 0, 3, 0, False), (1, 0, 0, 1, 1, True), (1, 2, 1, 3, 1, False))
LAYOUTS = {
    1: SPEC[:1],                                         # one residual item
    2: (SPEC[0], SPEC[2]),                                # two maps, distinct dV: one dK / dV round
    3: (SPEC[0], SPEC[1], (1, 2, 1, 3, 0, False)),       # one dV shared by a writer and two accumulating items: three rounds
    4: SPEC,                                             # the level: two rounds of two
}
ROUNDS = {1: 1, 2: 1, 3: 3, 4: 2}
# qs, B, N, C, n_items, regime, ld of the incoming gradient (>= 4C: a column slice of a wider one), split (the forwards get a workspace
# under the default split policy), route
BatchCase = collections.namedtuple("BatchCase", "qs B N C n regime ldg split route")
BATCH_CASES = [
    BatchCase(True, 2, 256, 128, 4, "mild", 4 * 128, False, route(ONE_PASS, NH1)),
    BatchCase(False, 2, 256, 128, 4, "peaky", 4 * 128 + 8, False, route(ONE_PASS, NH1)),
    BatchCase(False, 3, 384, 64, 3, "mild", 4 * 64 + 8, False, route(ONE_PASS, NH1)),
    BatchCase(True, 3, 384, 64, 2, "peaky", 4 * 64, False, route(ONE_PASS, NH1)),
    BatchCase(True, 8, 256, 64, 4, "mild", 4 * 64 + 16, False, route(PP64, DKV512, xmap=True)),
    BatchCase(False, 8, 256, 64, 3, "moving", 4 * 64, False, route(PP64, DKV512, xmap=True)),
    BatchCase(True, 2, 1024, 64, 1, "mild", 4 * 64, False, route(PP64, DKV512)),
    BatchCase(True, 8, 128, 128, 3, "peaky", 4 * 128 + 8, False, route(ONE_PASS, NH1, xmap=True)),
    BatchCase(True, 2, 256, 256, 4, "mild", 4 * 256, False, route(ONE_PASS, NH2)),
    BatchCase(False, 3, 256, 256, 1, "mild", 4 * 256 + 8, False, route(ONE_PASS, NH2)),
    BatchCase(True, 1, 512, 128, 4, "mild", 4 * 128, False, route(ONE_PASS, NH1)),
    BatchCase(True, 1, 512, 128, 4, "peaky", 4 * 128, True, route(SPLIT, NH1, S=8)),
    BatchCase(False, 1, 256, 256, 3, "mild", 4 * 256 + 8, True, route(SPLIT, NH2, S=4)),
    BatchCase(True, 1, 1024, 64, 2, "moving", 4 * 64, True, route(SPLIT, DKV512, S=16)),
]


def batch_id(c):
    return "%s-B%d-N%d-C%d-n%d-%s-ldg%d%s" % ("qs" if c.qs else "plain", c.B, c.N, c.C, c.n, c.regime, c.ldg, "-split" if c.split else "")


def batch_route_of(L, c):
    return L.hupr_attn_route(c.B, c.N, c.C, 4 * c.C, 1, int(c.split))


def expected_bwd_launches(c):
    return 2 + (c.n if (c.route & 12) == DKV512 else ROUNDS[c.n])


def _level(c, seed):
    """Two maps and their 4C-wide bf16 projections (the level's K / Q slots), fp32 maps, bf16 maps, the bf16 gradient of the
    concatenated output (column blocks, row stride ldg; NaN past 4C)."""
    B, N, C = c.B, c.N, c.C
    ks = {"mild": C ** -0.25, "peaky": (12.0 / C ** 0.5) ** 0.5, "moving": 1.0}[c.regime]
    Y = []
    for m in range(2):
        y = rnd(B, N, 4 * C, seed=seed + m, scale=ks)
        if c.regime == "moving":           # the key slots 0 and 2
            y[..., :C] *= moving_profile(N)[None, :, None]
            y[..., 2 * C:3 * C] *= moving_profile(N)[None, :, None]
        if c.qs:           # query slots 1 and 3 carry log2(e) before their rounding
            y[..., C:2 * C] *= LOG2E
            y[..., 3 * C:] *= LOG2E
        Y.append(y.bfloat16())
    maps = [rnd(B, N, C, seed=seed + 2 + m) for m in range(2)]
    g = rnd(B, N, 4 * C, seed=seed + 4).bfloat16()
    return Y, maps, g


def _slot_val(Y, src, slot, C, qs, query):
    t = Y[src][..., slot * C:(slot + 1) * C]
    return t.double() / LOG2E if (qs and query) else t.double()


@pytest.mark.parametrize("c", BATCH_CASES, ids=[batch_id(c) for c in BATCH_CASES])
def test_batch_entries_vs_single_calls_and_fp64(c, L):
    """hupr_attn_fwd_bf16in_ld_ws_batch(_qs) and hupr_attn_bwd_bf16in_ld_batch(_qs) on the level's layout: the same bits as the items
    issued as single calls in array order (dout32 = NULL), the fp64 gate on every item, the launch count of the backward."""
    from hupr_amd import runtime as rt
    CURRENT[0] = batch_id(c)
    assert batch_route_of(L, c) == c.route
    B, N, C, n = c.B, c.N, c.C, c.n
    spec = LAYOUTS[n]
    Y, maps, g = _level(c, 5000 + 31 * BATCH_CASES.index(c))
    Yd = [y.cuda() for y in Y]
    mapd = [m.cuda() for m in maps]
    vbd = [m.bfloat16().cuda() for m in maps]
    gbuf = nan_buffer((B, N, c.ldg), torch.bfloat16)
    gbuf[..., :4 * C] = g.cuda()
    s = rt.stream()
    fwd_batch = L.hupr_attn_fwd_bf16in_ld_ws_batch_qs if c.qs else L.hupr_attn_fwd_bf16in_ld_ws_batch
    fwd_one = L.hupr_attn_fwd_bf16in_ld_ws_qs if c.qs else L.hupr_attn_fwd_bf16in_ld_ws
    bwd_batch = L.hupr_attn_bwd_bf16in_ld_batch_qs if c.qs else L.hupr_attn_bwd_bf16in_ld_batch
    bwd_one = L.hupr_attn_bwd_bf16in_ld_qs if c.qs else L.hupr_attn_bwd_bf16in_ld
    ld16 = 4 * C + 8                                     # strided bf16 copy: a column slice of a wider concatenation

    def forward(batch):
        outs = [nan_buffer((B, N, C), torch.float32) for _ in range(n)]
        lses = [nan_buffer((B, N), torch.float32) for _ in range(n)]
        cat = nan_buffer((B, N, ld16), torch.bfloat16)
        its = (rt.AttnItem * n)()
        for i, (ks, kslot, qsrc, qslot, vs, residual) in enumerate(spec):
            its[i].K, its[i].Q = col(Yd[ks], kslot, C), col(Yd[qsrc], qslot, C)
            its[i].V, its[i].Vres = rt.ptr(vbd[vs]), (rt.ptr(mapd[vs]) if residual else None)
            its[i].out, its[i].lse, its[i].out16 = rt.ptr(outs[i]), rt.ptr(lses[i]), col(cat, i, C)
        nbytes = L.hupr_attn_fwd_split_ws_bytes(B, N, C) if c.split else 0
        assert (nbytes > 0) == bool(c.split)
        ws = torch.empty(max(n * nbytes, 16), dtype=torch.uint8, device="cuda") if c.split else None
        if batch:
            rt.check(fwd_batch(its, n, 4 * C, 4 * C, ld16, B, N, C, rt.ptr(ws), n * nbytes, s))
        else:
            for t in its:
                rt.check(fwd_one(t.K, 4 * C, t.Q, 4 * C, t.V, t.Vres, t.out, t.lse, t.out16, ld16, B, N, C, rt.ptr(ws), nbytes, s))
        return outs, lses, cat

    def backward(batch, outs, lses):
        dY = [nan_buffer((B, N, 4 * C), torch.float32) for _ in range(2)]
        dV = [nan_buffer((B, N, C), torch.float32) for _ in range(2)]
        scr = torch.empty((n, B, N), device="cuda")
        its = (rt.AttnBwdItem * n)()
        for i, (ks, kslot, qsrc, qslot, vs, residual) in enumerate(spec):
            t = its[i]
            t.K, t.Q, t.V, t.dO = col(Yd[ks], kslot, C), col(Yd[qsrc], qslot, C), rt.ptr(vbd[vs]), col(gbuf, i, C)
            t.V32, t.out, t.lse = rt.ptr(mapd[vs]), rt.ptr(outs[i]), rt.ptr(lses[i])
            t.dK, t.dQ, t.dV, t.Dq = col(dY[ks], kslot, C), col(dY[qsrc], qslot, C), rt.ptr(dV[vs]), scr[i].data_ptr()
            t.residual, t.accumulate = (1, 0) if residual else (0, 1)
        if batch:
            n0 = L.hupr_launch_count()
            rt.check(bwd_batch(its, n, 4 * C, 4 * C, c.ldg, 4 * C, 4 * C, B, N, C, s))
            assert L.hupr_launch_count() - n0 == expected_bwd_launches(c)
        else:
            for t in its:
                rt.check(bwd_one(t.K, 4 * C, t.Q, 4 * C, t.V, t.dO, c.ldg, t.V32, t.out, None, t.lse, t.dK, 4 * C, t.dQ, 4 * C, t.dV,
                                 t.Dq, B, N, C, t.residual, t.accumulate, s))
        return dY, dV

    fo, fl, fc = forward(True)
    so, sl, sc = forward(False)
    for i in range(n):
        assert torch.equal(bits(fo[i]), bits(so[i])) and torch.equal(bits(fl[i]), bits(sl[i])), "batch forward item %d" % i
    assert torch.equal(bits(fc), bits(sc)), "batch forward bf16 copies"
    assert_nan_outside(fc, [(i * C, C) for i in range(n)], "out16")
    for i in range(n):
        assert torch.equal(bits(fc[..., i * C:(i + 1) * C]), bits(fo[i].bfloat16())), "out16 of item %d" % i
    bY, bV = backward(True, fo, fl)
    sY, sV = backward(False, so, sl)
    torch.cuda.synchronize()
    for m in range(2):
        assert torch.equal(bits(bY[m]), bits(sY[m])), "batch dK / dQ of map %d != single calls" % m
        assert torch.equal(bits(bV[m]), bits(sV[m])), "batch dV of map %d != single calls" % m
        written = [(kslot * C, C) for ks, kslot, _, _, _, _ in spec if ks == m] + [(qslot * C, C) for _, _, qs, qslot, _, _ in spec if qs == m]
        assert_nan_outside(bY[m], written, "dY[%d]" % m)
        if not any(vs == m for *_, vs, _ in spec):
            assert_nan_outside(bV[m], [], "dV[%d]" % m)
    # fp64 gate per item (dV: the sum over the items of a map plus the residual items' dO)
    dY = [t.cpu() for t in bY]
    dV = [t.cpu() for t in bV]
    outs, lses = [t.cpu() for t in fo], [t.cpu() for t in fl]
    for b in items(B):
        vref = [0.0, 0.0]
        vA = [0.0, 0.0]
        vU = [0.0, 0.0]
        vterms = [[], []]
        for i, (ks, kslot, qsrc, qslot, vs, residual) in enumerate(spec):
            kk = _slot_val(Y, ks, kslot, C, c.qs, False)[b]
            qq = _slot_val(Y, qsrc, qslot, C, c.qs, True)[b]
            go = g[b, :, i * C:(i + 1) * C]
            r = reference(kk, qq, maps[vs][b].bfloat16(), go, None, maps[vs][b] if residual else None)
            assert_gate("out", outs[i][b], r["out"], r["A_out"], C_OUT, [r["res"]] if residual else (), r["U_out"])
            assert_lse(lses[i][b], r)
            assert_gate("dK", dY[ks][b, :, kslot * C:(kslot + 1) * C], r["dK"], r["A_dK"], C_DK, (), r["U_dK"])
            assert_gate("dQ", dY[qsrc][b, :, qslot * C:(qslot + 1) * C], r["dQ"], r["A_dQ"], C_DQ, (), r["U_dQ"])
            vref[vs] = vref[vs] + r["dV"] + (r["g32"] if residual else 0.0)
            vA[vs] = vA[vs] + r["A_dV"]
            vU[vs] = vU[vs] + r["U_dV"]
            if residual:
                vterms[vs].append(r["g32"])
        for m in range(2):
            if any(vs == m for *_, vs, _ in spec):
                assert_gate("dV", dV[m][b], vref[m], vA[m], C_DV, vterms[m], vU[m])


# ---- refused calls --------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_every_output_untouched(L):
    """HUPR_ERR_ARG, and no output written: N % 128 != 0, C = 96, ldk % 8 != 0, residual with accumulate, n_items = 5, an item with
    a null pointer (at the level-1 shape the batch forward launches per item: every item is checked before the first launch)."""
    from hupr_amd import runtime as rt
    s = rt.stream()

    def bufs(B, N, C):
        kq = torch.zeros((B, N, 4 * C + 8), dtype=torch.bfloat16, device="cuda")
        v, g = torch.zeros((B, N, C), dtype=torch.bfloat16, device="cuda"), torch.zeros((B, N, 4 * C), dtype=torch.bfloat16, device="cuda")
        v32 = torch.zeros((B, N, C), device="cuda")
        outs = [nan_buffer((B, N, C), torch.float32) for _ in range(6)]
        lse = [nan_buffer((B, N), torch.float32) for _ in range(6)]
        return kq, v, g, v32, outs, lse

    def untouched(ts):
        torch.cuda.synchronize()
        for t in ts:
            assert bool((bits(t) == NAN32).all()), "a refused call wrote an output"

    for B, N, C, ldk, why in ((2, 192, 64, 256, "N % 128"), (2, 256, 96, 384, "C = 96"), (2, 256, 64, 68, "ldk % 8")):
        if why != "C = 96":
            assert L.hupr_attn_route(B, N, C, ldk, 1, 0) == HUPR_ERR_ARG, why
        else:
            assert L.hupr_attn_route(B, N, C, 4 * C, 1, 0) == HUPR_ERR_ARG, why
        kq, v, g, v32, outs, lse = bufs(B, N, C)
        ldq = max(C, ldk - ldk % 8)
        for fwd in (L.hupr_attn_fwd_bf16in_ld_ws, L.hupr_attn_fwd_bf16in_ld_ws_qs):
            assert fwd(kq.data_ptr(), ldk, kq.data_ptr(), ldq, v.data_ptr(), None, rt.ptr(outs[0]), rt.ptr(lse[0]), None, 0, B, N, C,
                       None, 0, s) == HUPR_ERR_ARG, why
        for bwd in (L.hupr_attn_bwd_bf16in_ld, L.hupr_attn_bwd_bf16in_ld_qs):
            assert bwd(kq.data_ptr(), ldk, kq.data_ptr(), ldq, v.data_ptr(), g.data_ptr(), 4 * C, v32.data_ptr(), v32.data_ptr(), None,
                       rt.ptr(lse[5]), rt.ptr(outs[1]), C, rt.ptr(outs[2]), C, rt.ptr(outs[3]), rt.ptr(lse[1]), B, N, C, 0, 0,
                       s) == HUPR_ERR_ARG, why
        untouched(outs[:4] + lse[:2])

    # residual with accumulate (single and batch), n_items = 5, null pointers — at the level-1 shape and at a level-2 shape
    for B, N, C in ((2, 512, 64), (2, 256, 128)):
        kq, v, g, v32, outs, lse = bufs(B, N, C)
        W = 4 * C
        for bwd in (L.hupr_attn_bwd_bf16in_ld, L.hupr_attn_bwd_bf16in_ld_qs):
            assert bwd(kq.data_ptr(), W, kq.data_ptr(), W, v.data_ptr(), g.data_ptr(), W, v32.data_ptr(), v32.data_ptr(), None,
                       rt.ptr(lse[5]), rt.ptr(outs[1]), C, rt.ptr(outs[2]), C, rt.ptr(outs[3]), rt.ptr(lse[1]), B, N, C, 1, 1,
                       s) == HUPR_ERR_ARG
        untouched(outs[1:4] + lse[1:2])
        fits = (rt.AttnItem * 5)()
        for i in range(5):
            fits[i].K, fits[i].Q, fits[i].V = kq.data_ptr(), kq.data_ptr() + 2 * C, v.data_ptr()
            fits[i].out, fits[i].lse, fits[i].out16 = rt.ptr(outs[i]), rt.ptr(lse[i]), None
        for fwd_batch in (L.hupr_attn_fwd_bf16in_ld_ws_batch, L.hupr_attn_fwd_bf16in_ld_ws_batch_qs):
            assert fwd_batch(fits, 5, W + 8, W + 8, 0, B, N, C, None, 0, s) == HUPR_ERR_ARG, "n_items = 5"
            fits[2].lse = None
            assert fwd_batch(fits, 4, W + 8, W + 8, 0, B, N, C, None, 0, s) == HUPR_ERR_ARG, "null lse in item 2"
            fits[2].lse = rt.ptr(lse[2])
            fits[3].V = None
            assert fwd_batch(fits, 4, W + 8, W + 8, 0, B, N, C, None, 0, s) == HUPR_ERR_ARG, "null V in item 3"
            fits[3].V = v.data_ptr()
        untouched(outs[:5] + lse[:5])
        bitems = (rt.AttnBwdItem * 5)()
        for i in range(5):
            t = bitems[i]
            t.K, t.Q, t.V, t.dO = kq.data_ptr(), kq.data_ptr() + 2 * C, v.data_ptr(), g.data_ptr()
            t.V32, t.out, t.lse = v32.data_ptr(), v32.data_ptr(), rt.ptr(lse[5])
            t.dK, t.dQ, t.dV, t.Dq = rt.ptr(outs[0]), rt.ptr(outs[1]), rt.ptr(outs[2 + i % 2]), rt.ptr(lse[i % 2])
            t.residual, t.accumulate = (1, 0) if i % 2 == 0 else (0, 1)
        for bwd_batch in (L.hupr_attn_bwd_bf16in_ld_batch, L.hupr_attn_bwd_bf16in_ld_batch_qs):
            assert bwd_batch(bitems, 5, W + 8, W + 8, W, C, C, B, N, C, s) == HUPR_ERR_ARG, "n_items = 5"
            bitems[3].dV = None
            assert bwd_batch(bitems, 4, W + 8, W + 8, W, C, C, B, N, C, s) == HUPR_ERR_ARG, "null dV in item 3"
            bitems[3].dV = rt.ptr(outs[3])
            bitems[1].residual = 1
            assert bwd_batch(bitems, 4, W + 8, W + 8, W, C, C, B, N, C, s) == HUPR_ERR_ARG, "residual with accumulate"
            bitems[1].residual = 0
        untouched(outs[:4] + lse[:2])


def test_zz_report_worst_ratios():
    """Prints the worst error-to-bound ratio per quantity over this module's cases (run with -s to see it)."""
    for k in sorted(WORST):
        print("\nworst err / bound of %s: %.3g (%s)" % (k, WORST[k][0], WORST[k][1]), end="")
    print()
    assert all(v <= 1.0 for v, _ in WORST.values())
