"""GPU (-m gpu): every kernel of the network's last stage (csrc/head.hip, csrc/gcn_products.hip and the nodes of functional.py that
call them) against an fp64 reference of exactly the operands the kernel reads, element by element, at the shapes where each kernel
takes another branch: the PRGCN products on v_mfma_f32_32x32x2_f32 (both instantiations of hupr_k_gcn_wx and hupr_k_gcn_dw with every
prefetch branch of their software pipelines), the adjacency epilogue forward (both ld branches, K slices summed), backward and bias
gradient with dense non-symmetric and the model's adjacency, GCNLayerFn on its three routes with the entry points counted, the fp32
1x1 head (forward, input gradient, weight gradient and its reduce with one-chunk, two-chunk, ragged and empty workgroups), the
sigmoid head both ways, BCE and pair BCE both ways, Gaussian targets, arg-max rows and softmax rows both ways, each kernel with a
grid-stride loop at a size where the loop wraps.

Every case (CASES) runs three times.  Outputs are views at 16-byte-aligned offsets inside NaN-pattern buffers with guards before and
after; workspaces have exactly the byte count the library asks for, followed by a guard; operands end in NaN guard tails; every guard
must come back bit-identical and no output element may stay NaN.  The second launch (fresh buffers, same operands) must give the same
bits.  The input pad columns (k >= K of x, t, dy and the logits) hold a large finite sentinel — not NaN: hupr_k_gcn_adj_fwd multiplies
its pad columns by an exact 0 — and the third launch, with another sentinel, must give the same bits again; output pad columns must be
exactly 0.0 (the product kernels have none: they carry all 16 columns).

Gates.  Sums (products, adjacency epilogues, bias gradient, head forward, dgrad, wgrad, softmax backward, the scalar losses):
|out - ref| <= c A  with A the same sum over absolute values, bias included (for a loss the mean of the absolute terms: below 1 for
probabilities away from saturation, so the gate is then tighter than the same c taken absolutely).  Element-wise:  sigmoid
|p - ref| <= c;  sigmoid backward, BCE gradient  |out - ref| <= c |ref|;  softmax  |p - ref| <= c max_row(ref).  (The softmax
backward gets 2^-149 on top, the spacing of fp32 denormals: behind logits of magnitude 80 some of its outputs are denormal.)  c per operation and route
(GATE_C) is the smallest power of two that is at least 8 x the worst value measured over this table against fp64 on an MI355X, never
above the caps (CAPS: 2^-16 for the sums, the project's gate of an fp32-output convolution, and what tests/test_ops_gpu.py asserts
for the element-wise ones: 1e-6 sigmoid, 1e-5 loss and gradient, 2e-5 max softmax).  Measured worst values (pytest -s prints them per
case and as a table at the end):

    operation                                 route / branch        worst      8 x        c
    product W x, W^T dt (wx)                                        2^-22.27   2^-19.27   2^-19
    product dW (dw)                                                 2^-21.69   2^-18.69   2^-18
    adjacency forward (adj_fwd)               ld = 16               2^-21.75   2^-18.75   2^-18
                                              scalar (ld != 16)     2^-21.75   2^-18.75   2^-18
    adjacency forward over K slices           ld = 16               2^-22.69   2^-19.69   2^-19
    (adj_sliced)                              scalar                2^-22.09   2^-19.09   2^-19
    adjacency backward, dt (adj_bwd)                                2^-21.84   2^-18.84   2^-18
    bias gradient (dbias)                                           2^-22.77   2^-19.77   2^-19
    GCNLayerFn forward (layer_fwd)            sliced                2^-24.94   2^-21.94   2^-21
                                              products              2^-23.54   2^-20.54   2^-20
                                              generic               2^-22.99   2^-19.99   2^-19
    GCNLayerFn dx (layer_dx)                  products              2^-23.35   2^-20.35   2^-20
                                              generic               2^-22.26   2^-19.26   2^-19
    GCNLayerFn dW (layer_dw)                  products              2^-22.14   2^-19.14   2^-19
                                              generic               2^-21.88   2^-18.88   2^-18
    head forward (head_fwd)                                         2^-21.63   2^-18.63   2^-18
    head input gradient (head_dgrad)                                2^-21.78   2^-18.78   2^-18
    head weight gradient (head_wgrad)                               2^-22.72   2^-19.72   2^-19
    sigmoid, absolute                                               2^-23.42   2^-20.42   2^-20
    sigmoid backward, relative                                      2^-22.49   2^-19.49   2^-19
    BCE and pair BCE losses (bce)                                   2^-23.38   2^-20.38   2^-20
    BCE and pair BCE gradients, relative                            2^-21.52   2^-18.52   2^-18
    softmax, of the row maximum                                     2^-22.43   2^-19.43   2^-19
    softmax backward                                                2^-22.54   2^-19.54   2^-19

(The layer rows are measured against the product of all three factors, so their A is larger than that of the single kernels and the
figures smaller; a single sample's backward is the generic engine's.  None of the 8 x values reaches a cap.)

tests/test_head_route.py checks the routes, the coverage of this table and the refusals without a GPU, and that these gates reject
the results of subtly wrong kernels."""
import collections
import functools
import math

import numpy as np
import pytest
import torch

from test_conv_halo_fp64_gpu import GUARD, NAN32, bits, nan_buffer, rnd

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG, HUPR_ERR_WORKSPACE = -1, -2
CAP = 2.0 ** -16                                        # the project's gate of an fp32-output sum (tests/test_tmerge_fp64_gpu.py)
SENT = (2.0 ** 100, -3.0e4)                             # what the input pad columns hold in the first two / the third launch
SUM_OPS = ("wx", "dw", "adj_fwd", "adj_sliced", "adj_bwd", "dbias", "head_fwd", "head_dgrad", "head_wgrad", "layer_fwd", "layer_dx",
           "layer_dw", "softmax_bwd")
# the element-wise gates may not be looser than tests/test_ops_gpu.py: 1e-6 (sigmoid), 1e-5 (loss, gradients), 2e-5 max (softmax)
CAPS = {"sigmoid": 2.0 ** -20, "sigmoid_bwd": 2.0 ** -17, "bce": 2.0 ** -17, "bce_bwd": 2.0 ** -17, "softmax": 2.0 ** -16}
CAPS.update({op: CAP for op in SUM_OPS})
assert CAPS["sigmoid"] <= 1e-6 and CAPS["bce"] <= 1e-5 and CAPS["bce_bwd"] <= 1e-5 and CAPS["sigmoid_bwd"] <= 1e-5 and CAPS["softmax"] <= 2e-5

# (operation, route) -> c
GATE_C = {
    ("wx", "any"): 2.0 ** -19, ("dw", "any"): 2.0 ** -18,
    ("adj_fwd", "ld16"): 2.0 ** -18, ("adj_fwd", "scalar"): 2.0 ** -18, ("adj_sliced", "ld16"): 2.0 ** -19, ("adj_sliced", "scalar"): 2.0 ** -19,
    ("adj_bwd", "any"): 2.0 ** -18, ("dbias", "any"): 2.0 ** -19,
    ("layer_fwd", "sliced"): 2.0 ** -21, ("layer_fwd", "products"): 2.0 ** -20, ("layer_fwd", "generic"): 2.0 ** -19,
    ("layer_dx", "products"): 2.0 ** -20, ("layer_dx", "generic"): 2.0 ** -19, ("layer_dw", "products"): 2.0 ** -19, ("layer_dw", "generic"): 2.0 ** -18,
    ("head_fwd", "any"): 2.0 ** -18, ("head_dgrad", "any"): 2.0 ** -18, ("head_wgrad", "any"): 2.0 ** -19,
    ("sigmoid", "any"): 2.0 ** -20, ("sigmoid_bwd", "any"): 2.0 ** -19,
    ("bce", "any"): 2.0 ** -20, ("bce_bwd", "any"): 2.0 ** -18,
    ("softmax", "any"): 2.0 ** -19, ("softmax_bwd", "any"): 2.0 ** -19,
}
assert all(c <= CAPS[op] for (op, _), c in GATE_C.items())

# op: what runs (OPS below).  entry: the entry points of the library the case calls.  route: the kernel branch it must take ("ld16" /
# "scalar" of the adjacency forward, "sliced" / "products" / "generic" of GCNLayerFn, else "any").  p: the shape, per operation.
Case = collections.namedtuple("Case", "op entry route p")
CASES = []

# ---- PRGCN products: p = (F, Bn, trans_w, exact) / (F, Bn, exact) -----------------------------------------------------------------
WX_SHAPES = [(F, Bn) for F in (64, 128, 192) for Bn in (1, 2, 5)] + [(1024, 2), (1024, 3)]
CASES += [Case("wx", ("hupr_gcn_wx_f32",), "any", (F, Bn, tw, False)) for tw in (0, 1) for (F, Bn) in WX_SHAPES]
CASES += [Case("wx", ("hupr_gcn_wx_f32",), "any", (128, 3, tw, True)) for tw in (0, 1)]
DW_SHAPES = [(64, Bn) for Bn in range(1, 9)] + [(192, 3), (1024, 2)]
CASES += [Case("dw", ("hupr_gcn_dw_f32",), "any", (F, Bn, False)) for (F, Bn) in DW_SHAPES]
CASES += [Case("dw", ("hupr_gcn_dw_f32",), "any", (128, 3, True))]

# ---- adjacency epilogues: p = (F, Bn, K, ld, relu, adjacency) ------------------------------------------------------------------------
K_LD = [(14, 16), (14, 14), (5, 8), (16, 16), (1, 4)]
ADJ_SHAPES = [(F, Bn, K, ld, relu, adj) for adj in ("dense", "model") for (K, ld) in K_LD if adj == "dense" or K == 14
              for relu in (0, 1) for F in (64, 1024) for Bn in (1, 3)]
ADJ_FWD_WRAP = [(64, 1041, 14, 16, 1, "dense"), (64, 1041, 14, 14, 0, "dense")]          # 66 624 rows > 4096 workgroups x 16
ADJ_BWD_WRAP = [(64, 16385, 14, 16, 1, "dense")]                                          # 1 048 640 rows > 4096 x 256


def ld_route(ld):
    return "ld16" if ld == 16 else "scalar"


CASES += [Case("adj_fwd", ("hupr_gcn_adj_fwd_f32",), ld_route(p[3]), p) for p in ADJ_SHAPES + ADJ_FWD_WRAP]
CASES += [Case("adj_bwd", ("hupr_gcn_adj_bwd_f32",), "any", p) for p in ADJ_SHAPES + ADJ_BWD_WRAP]
# p = (F, Bn, K, ld, relu, adjacency, slices)
CASES += [Case("adj_sliced", ("hupr_gcn_adj_fwd_sliced_f32",), ld_route(ld), (64, 3, K, ld, relu, "dense", S))
          for S in (1, 2, 8, 64) for (K, ld, relu) in ((14, 16, 1), (14, 14, 0), (5, 8, 1))]

# ---- GCNLayerFn: p = (B, F, relu, GCN_PRODUCTS) -----------------------------------------------------------------------------------------
LAYER_ENTRIES = ("hupr_gcn_wx_f32", "hupr_gcn_dw_f32", "hupr_gemm_f32", "hupr_gcn_adj_fwd_f32", "hupr_gcn_adj_fwd_sliced_f32")
CASES += [Case("layer", ("hupr_gemm_f32", "hupr_gcn_adj_fwd_sliced_f32", "hupr_gcn_adj_bwd_f32"), "sliced", (1, 1024, 1, True)),
          Case("layer", ("hupr_gemm_f32", "hupr_gcn_adj_fwd_sliced_f32", "hupr_gcn_adj_bwd_f32"), "sliced", (1, 1024, 0, True)),
          Case("layer", ("hupr_gcn_wx_f32", "hupr_gcn_dw_f32", "hupr_gcn_adj_fwd_f32", "hupr_gcn_adj_bwd_f32"), "products", (3, 128, 1, True)),
          Case("layer", ("hupr_gcn_wx_f32", "hupr_gcn_dw_f32", "hupr_gcn_adj_fwd_f32", "hupr_gcn_adj_bwd_f32"), "products", (2, 1024, 0, True)),
          # a single sample whose F is no multiple of 1024: the product forward with Bn = 1, the generic backward
          Case("layer", ("hupr_gcn_wx_f32", "hupr_gemm_f32", "hupr_gcn_adj_fwd_f32", "hupr_gcn_adj_bwd_f32"), "products", (1, 192, 1, True)),
          Case("layer", ("hupr_gemm_f32", "hupr_gcn_adj_fwd_f32", "hupr_gcn_adj_bwd_f32"), "generic", (2, 128, 1, False)),
          Case("layer", ("hupr_gemm_f32", "hupr_gcn_adj_fwd_f32", "hupr_gcn_adj_bwd_f32"), "generic", (2, 96, 0, True))]

# ---- the fp32 1x1 head: p = (M, out_rows, null) with null in "", "dx", "dw" -----------------------------------------------------------
HEAD_M = (1, 127, 129, 256, 257, 65537, 65664)
HEAD16 = ("hupr_head1x1_fwd_f32", "hupr_head1x1_bwd_f32")
HEAD14 = ("hupr_head1x1_fwd_f32", "hupr_head1x1_bwd_rows_f32")
CASES += [Case("head", HEAD14 if rows == 14 else HEAD16, "any", (M, rows, "")) for M in HEAD_M for rows in (14, 16)]
CASES += [Case("head", HEAD14, "any", (257, 14, "dx")), Case("head", HEAD14, "any", (257, 14, "dw")),
          Case("head", HEAD16, "any", (129, 16, "dx")), Case("head", HEAD16, "any", (129, 16, "dw"))]

# ---- sigmoid head: p = (Bn, K, ld, HW) ---------------------------------------------------------------------------------------------------
SIGMOID = ("hupr_sigmoid_to_nchw_f32", "hupr_sigmoid_to_nchw_bwd_f32")
CASES += [Case("sigmoid", SIGMOID, "any", (2, K, ld, HW)) for (K, ld) in ((14, 16), (14, 14), (3, 8)) for HW in (1, 63, 4096)]
CASES += [Case("sigmoid", SIGMOID, "any", (19, 14, 16, 4096))]                              # 1 089 536 elements > 4096 x 256

# ---- BCE and pair BCE: p = (n, kind) with kind "random" (against fp64) or "saturated" (against torch on the CPU) ----------------------
BCE_N = (1, 255, 257, 262144, 262145, 19 * 14 * 4096)
BCE = ("hupr_bce_fwd_f32", "hupr_bce_bwd_f32")
PAIR = ("hupr_bce_pair_fwd_f32", "hupr_bce_pair_bwd_f32")
CASES += [Case(op, e, "any", (n, "random")) for (op, e) in (("bce", BCE), ("bce_pair", PAIR)) for n in BCE_N]
CASES += [Case(op, e, "any", (n, "saturated")) for (op, e) in (("bce", BCE), ("bce_pair", PAIR)) for n in (6, 257)]

# ---- targets, arg-max, softmax -------------------------------------------------------------------------------------------------------------
CASES += [Case("targets", ("hupr_gaussian_targets_f32",), "any", (19, 14, 64))]             # 1 089 536 elements: the loop wraps
CASES += [Case("argmax", ("hupr_argmax_rows_f32",), "any", (n,)) for n in (1, 63, 64, 65, 4096)]
SOFTMAX = ("hupr_softmax_rows_f32", "hupr_softmax_rows_bwd_f32")
CASES += [Case("softmax", SOFTMAX, "any", (rows, n, 3.0)) for n in (4, 1020, 1024, 1028, 4096) for rows in (1, 3)]
CASES += [Case("softmax", SOFTMAX, "any", (3, 1028, 80.0))]                                 # logits of magnitude 80


def case_id(c):
    return "%s-%s-%s" % (c.op, c.route, "-".join(str(v) for v in c.p))


# ---- gates (any device) ----------------------------------------------------------------------------------------------------------------
DENORMAL = 2.0 ** -149                                  # the spacing of fp32 below 2^-126: what one rounding there may cost, whatever A


def ratio(out, ref, A, floor=0.0):
    """(err - floor) / A element by element; 0 where err <= floor; inf for a NaN."""
    err = ((out.double() - ref).abs() - floor).clamp_min(0.0)
    return torch.where(err == 0, torch.zeros_like(err), err / A).nan_to_num(float("inf"))


def within(out, ref, A, c, floor=0.0):
    """True where out meets |out - ref| <= c A + floor (a NaN never does)."""
    return (out.double() - ref).abs() <= c * A + floor


WORST = {}             # (op, route) -> worst measured value of this session


def log2(v):
    return math.log2(v) if v > 0 else float("-inf")


def check(out, ref, A, key, what, floor=0.0):
    """Assert the gate GATE_C[key] on every element; print and record the measured worst err / A."""
    A = A if isinstance(A, torch.Tensor) else torch.full_like(ref, A)
    assert out.shape == ref.shape == A.shape, (what, out.shape, ref.shape, A.shape)
    worst = ratio(out, ref, A, floor).max().item() if out.numel() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("head fp64: %-58s %-24s worst %.3g = 2^%.2f" % (what, "%s/%s" % key, worst, log2(worst)))
    ok = within(out, ref, A, GATE_C[key], floor)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s [%s/%s]: %d of %d outside the gate, first at %s (out %r, ref %r, A %r), measured worst %.3g (c %.3g)"
                             % ((what,) + key + (bad.shape[0], ok.numel(), i, out[i].item(), ref[i].item(), A[i].item(), worst, GATE_C[key])))


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if WORST:
        print("\nhead fp64: measured worst values of this session (operation/route, 2^x; 8 x that; the committed c)")
        for key in sorted(WORST):
            w = WORST[key]
            print("    %-28s 2^%7.2f   2^%7.2f   2^%d" % ("%s/%s" % key, log2(w), log2(8 * w), round(log2(GATE_C[key]))))


# ---- operands (CPU, seeded; pad columns zero) and fp64 references (any device) -----------------------------------------------------------
def seed_of(c):
    return sum((i + 1) * int(v) for i, v in enumerate(c.p) if isinstance(v, (int, float))) % 100003


def make_wx(c):
    """W [F, F], x [Bn, F, 16] and K (the number of real columns of x)."""
    F, Bn, tw, exact = c.p
    if exact:
        # W: a permutation matrix with entries +-1 .. +-4; x: distinct integers 1 .. Bn F 16 (every product is exact in fp32)
        g = torch.Generator().manual_seed(7 + tw)
        perm = torch.randperm(F, generator=g)
        vals = torch.randint(1, 5, (F,), generator=g).float() * (torch.randint(0, 2, (F,), generator=g).float() * 2 - 1)
        W = torch.zeros(F, F)
        W[torch.arange(F), perm] = vals
        x = (torch.arange(Bn * F * 16) + 1).float().view(Bn, F, 16)
        return {"W": W, "x": x, "K": 16}
    s = seed_of(c)
    x = rnd(Bn, F, 16, seed=s)
    x[..., 14:] = 0
    return {"W": rnd(F, F, seed=s + 1, scale=F ** -0.5), "x": x, "K": 14}


def wx_ref(W, x, tw):
    """fp64 (ref, A): t[b][f][n] = sum_g W[f][g] x[b][g][n], or with trans_w dx[b][g][n] = sum_f W[f][g] x[b][f][n]."""
    eq = "fg,bfn->bgn" if tw else "fg,bgn->bfn"
    W, x = W.double(), x.double()
    return torch.einsum(eq, W, x), torch.einsum(eq, W.abs(), x.abs())


def make_dw(c):
    """dt, x [Bn, F, 16]; the pad columns of dt are zero (hupr_k_gcn_adj_bwd writes them so), those of x take the sentinel."""
    F, Bn, exact = c.p
    s = seed_of(c)
    if exact:
        g = torch.Generator().manual_seed(11)
        return {"dt": torch.randint(-4, 5, (Bn, F, 16), generator=g).float(), "x": torch.randint(-4, 5, (Bn, F, 16), generator=g).float(),
                "K": 16}
    dt, x = rnd(Bn, F, 16, seed=s), rnd(Bn, F, 16, seed=s + 1)
    dt[..., 14:] = 0
    x[..., 14:] = 0
    return {"dt": dt, "x": x, "K": 14}


def dw_ref(dt, x):
    dt, x = dt.double(), x.double()
    return torch.einsum("bfn,bgn->fg", dt, x), torch.einsum("bfn,bgn->fg", dt.abs(), x.abs())


def adjacency_of(kind, K, seed=5):
    if kind == "model":
        from oracle.model import adjacency
        assert K == 14
        return adjacency()
    return rnd(K, K, seed=seed + K)                     # dense, not symmetric


def make_adj(c):
    """t (forward) [S, Bn, F, ld] or [Bn, F, ld], dy and y (backward) [Bn, F, ld], adj [K, K], bias [F, K].  y holds exact zeros and
    negative zeros, and elsewhere the sign pattern of an independent draw: the ReLU mask must come from y > 0, not from dy."""
    F, Bn, K, ld, relu, kind = c.p[:6]
    S = c.p[6] if c.op == "adj_sliced" else None
    s = seed_of(c)
    lead = (S, Bn, F) if S else (Bn, F)
    t = torch.zeros(*lead, ld)
    t[..., :K] = rnd(*lead, K, seed=s)
    o = {"t": t, "adj": adjacency_of(kind, K), "bias": rnd(F, K, seed=s + 1), "K": K}
    if c.op == "adj_bwd":
        dy, y = torch.zeros(Bn, F, ld), torch.zeros(Bn, F, ld)
        dy[..., :K] = rnd(Bn, F, K, seed=s + 2)
        yv = rnd(Bn, F, K, seed=s + 3)
        flat = yv.view(-1)
        flat[0::7] = 0.0
        flat[3::7] = -0.0
        y[..., :K] = yv
        o.update(dy=dy, y=y)
        del o["t"]
    return o


def adj_fwd_ref(t, adj, bias, K, relu):
    """fp64 (ref, A) [Bn, F, K] of y = act(sum_k t[..., k] adj[k][k'] + bias); t [S, Bn, F, ld] is summed over its slices first."""
    t, adj, bias = t.double()[..., :K], adj.double(), bias.double()
    ta = t.abs()
    if t.dim() == 4:
        t, ta = t.sum(0), ta.sum(0)
    ref = torch.einsum("bfk,kj->bfj", t, adj) + bias
    A = torch.einsum("bfk,kj->bfj", ta, adj.abs()) + bias.abs()
    return (ref.clamp_min(0.0) if relu else ref), A


def adj_bwd_ref(dy, y, adj, K, relu):
    """fp64 g [Bn, F, K] (exact: dy or 0), (dt, A), (dbias, A): g = dy [y > 0], dt[.., k] = sum_k' g[k'] adj[k][k'], dbias = sum_b g."""
    g = dy.double()[..., :K]
    if relu:
        g = g * (y[..., :K] > 0)
    adj = adj.double()
    return (g, (torch.einsum("bfj,kj->bfk", g, adj), torch.einsum("bfj,kj->bfk", g.abs(), adj.abs())), (g.sum(0), g.abs().sum(0)))


def make_layer(c):
    B, F, relu, _ = c.p
    s = seed_of(c)
    x, dy = torch.zeros(B, F, 16), torch.zeros(B, F, 16)
    x[..., :14] = rnd(B, F, 14, seed=s)
    dy[..., :14] = rnd(B, F, 14, seed=s + 3)
    return {"x": x, "W": rnd(F, F, seed=s + 1, scale=F ** -0.5), "bias": rnd(F, 14, seed=s + 2, scale=0.5), "dy": dy,
            "adj": adjacency_of("model", 14), "K": 14}


def layer_fwd_ref(x, W, bias, adj, relu):
    """fp64 (ref, A) [B, F, K] of act((W x) adj + bias)."""
    K = adj.shape[0]
    x, W, adj, bias = x.double()[..., :K], W.double(), adj.double(), bias.double()
    ref = torch.einsum("fg,bgk,kj->bfj", W, x, adj) + bias
    A = torch.einsum("fg,bgk,kj->bfj", W.abs(), x.abs(), adj.abs()) + bias.abs()
    return (ref.clamp_min(0.0) if relu else ref), A


def layer_bwd_ref(x, W, adj, g):
    """g [B, F, K] fp64, the masked output gradient: (dx, A), (dW, A) of the layer."""
    K = adj.shape[0]
    x, W, adj = x.double()[..., :K], W.double(), adj.double()
    dt, dta = torch.einsum("bfj,kj->bfk", g, adj), torch.einsum("bfj,kj->bfk", g.abs(), adj.abs())
    return ((torch.einsum("fg,bfk->bgk", W, dt), torch.einsum("fg,bfk->bgk", W.abs(), dta)),
            (torch.einsum("bfk,bgk->fg", dt, x), torch.einsum("bfk,bgk->fg", dta, x.abs())))


def make_head(c):
    """x [M, 32], w16 [16, 32] (rows >= out_rows zero), dy [M, 16] (columns >= out_rows take the sentinel)."""
    M, rows, _ = c.p
    s = seed_of(c)
    w = rnd(16, 32, seed=s + 1, scale=32 ** -0.5)
    w[rows:] = 0
    dy = rnd(M, 16, seed=s + 2)
    dy[:, rows:] = 0
    return {"x": rnd(M, 32, seed=s), "w": w, "dy": dy, "K": rows}


def head_ref(x, w, dy, rows):
    """fp64 (y, A) [M, 16], (dx, A) [M, 32], (dw, A) [rows, 32] — dy's columns >= rows do not enter (their filters are zero)."""
    x, w, dy = x.double(), w.double(), dy.double()[:, :rows]
    return ((x @ w.t(), x.abs() @ w.abs().t()), (dy @ w[:rows], dy.abs() @ w[:rows].abs()), (dy.t() @ x, dy.abs().t() @ x.abs()))


SPECIAL_LOGITS = (0.0, -0.0, 20.0, -20.0, 90.0, -90.0)


def make_sigmoid(c):
    """Logits x [Bn, HW, ld] whose first real elements are +-0, +-20 and +-90, and dy [Bn, K, HW]."""
    Bn, K, ld, HW = c.p
    s = seed_of(c)
    v = rnd(Bn, HW, K, seed=s) * 3
    flat = v.view(-1)
    n = min(flat.numel(), len(SPECIAL_LOGITS))
    flat[:n] = torch.tensor(SPECIAL_LOGITS[:n])
    x = torch.zeros(Bn, HW, ld)
    x[..., :K] = v
    return {"x": x, "dy": rnd(Bn, K, HW, seed=s + 1), "K": K}


def sigmoid_ref(x, K):
    """fp64 probabilities [Bn, K, HW] of channels-last logits [Bn, HW, ld]."""
    return torch.sigmoid(x.double()[..., :K]).permute(0, 2, 1).contiguous()


def make_bce(c):
    """p1, p2, t [n].  random: p in (0.05, 0.95), t in (0, 1).  saturated: p exactly 0 and 1 against t in {0, 1, 0.5}."""
    n, kind = c.p
    s = seed_of(c) + (1 if c.op == "bce_pair" else 0)
    if kind == "saturated":
        i = torch.arange(n)
        p1 = (i % 2).float()
        t = torch.tensor([0.0, 1.0, 0.5])[(i // 2) % 3]
        return {"p1": p1, "p2": 1.0 - p1, "t": t}
    g = torch.Generator().manual_seed(s)
    return {"p1": 0.05 + 0.9 * torch.rand(n, generator=g), "p2": 0.05 + 0.9 * torch.rand(n, generator=g), "t": torch.rand(n, generator=g)}


def bce_ref(p, t):
    """fp64 mean BCE with the logarithms clamped at -100, as (ref, A) of shape (1,): A is the mean over the absolute values of the
    terms (with p and t in [0, 1] every term is positive: A = ref)."""
    p, t = p.double(), t.double()
    a, b = t * torch.log(p).clamp_min(-100.0), (1 - t) * torch.log(1 - p).clamp_min(-100.0)
    return -(a + b).mean().view(1), (a.abs() + b.abs()).mean().view(1)


def bce_grad_ref(p, t, scale):
    """fp64 scale (p - t) / max(p (1 - p), 1e-12) / n."""
    p, t = p.double(), t.double()
    return scale * (p - t) / (p * (1 - p)).clamp_min(1e-12) / p.numel()


ALPHA, BETA = float(np.float32(0.3)), float(np.float32(0.7))
G_OUT, G_OUT2 = float(np.float32(1.7)), float(np.float32(-0.6))


def make_argmax(c):
    """Rows of length n and the index each must give: a random row, ties across lanes and inside one lane (the lowest index wins), NaNs
    in front of and between two equal maxima (skipped), all -inf (index 0)."""
    (n,) = c.p
    rows = [rnd(n, seed=40 + n)]
    if n >= 2:
        r = rnd(n, seed=41 + n)
        r[n // 3] = r[n - 1] = 50.0                            # two lanes (n // 3 != n - 1 mod 64 for the table's n)
        rows.append(r)
        r = rnd(n, seed=42 + n)
        r[0] = float("nan")
        r[n // 2] = float("nan")
        r[1] = r[n - 1] = 60.0
        rows.append(r)
    if n > 64:
        r = rnd(n, seed=43 + n)
        r[n - 1] = r[n - 65] = 50.0                            # one lane, two trips of its loop
        rows.append(r)
        r = rnd(n, seed=44 + n)
        r[0] = r[64] = r[n - 1] = 50.0
        rows.append(r)
    rows.append(torch.full((n,), float("-inf")))
    p = torch.stack(rows)
    clean = torch.where(p.isnan(), torch.full_like(p, float("-inf")), p)
    return {"p": p, "idx": torch.from_numpy(clean.numpy().argmax(axis=1).astype(np.int32)), "max": clean.max(dim=1).values}


def make_softmax(c):
    rows, n, mag = c.p
    s = seed_of(c)
    return {"x": rnd(rows, n, seed=s) * mag, "dp": rnd(rows, n, seed=s + 1)}


def softmax_ref(x):
    return torch.softmax(x.double(), dim=1)


def softmax_bwd_ref(p, dp):
    """fp64 (ds, A): ds = p (dp - sum_j dp_j p_j)."""
    p, dp = p.double(), dp.double()
    return p * (dp - (dp * p).sum(1, keepdim=True)), p.abs() * (dp.abs() + (dp * p).abs().sum(1, keepdim=True))


def make_targets(c):
    """Joints (B, K, 2) in image pixels: random ones, the four corners, and patches clipped by or wholly outside the map."""
    B, K, H = c.p
    g = np.random.RandomState(19)
    gt = g.randint(0, 256, size=(B, K, 2)).astype(np.int64)
    gt[0, :6] = [[0, 0], [255, 255], [0, 255], [-40, 100], [400, 400], [270, 10]]
    return {"joints": gt}


MAKE = {"wx": make_wx, "dw": make_dw, "adj_fwd": make_adj, "adj_sliced": make_adj, "adj_bwd": make_adj, "layer": make_layer,
        "head": make_head, "sigmoid": make_sigmoid, "bce": make_bce, "bce_pair": make_bce, "argmax": make_argmax, "softmax": make_softmax,
        "targets": make_targets}


@functools.lru_cache(maxsize=2)
def made(c):
    """The CPU operands of a case (left unchanged by everyone), kept for its three launches."""
    return MAKE[c.op](c)


# ---- buffers (GPU) ----------------------------------------------------------------------------------------------------------------------
def dev(t, K=None, sent=None, dtype=torch.float32):
    """t copied into a fresh device buffer that ends in a NaN guard tail; columns >= K of its last axis set to the sentinel."""
    n = t.numel()
    if dtype == torch.float32:
        buf = nan_buffer(n + GUARD, torch.float32)
    else:
        buf = torch.full((n + GUARD,), -1, dtype=dtype, device="cuda")
    v = buf[:n].view(t.shape)
    v.copy_(t)
    if K is not None and K < t.shape[-1]:
        v[..., K:] = sent
    assert v.data_ptr() % 16 == 0
    return v


class Out:
    """guard | n fp32 (or int32) elements | guard in the NaN pattern; the view starts 1024 bytes into the allocation."""

    def __init__(self, *shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.buf = nan_buffer(GUARD + self.n + GUARD, torch.float32)
        self.v = self.buf[GUARD:GUARD + self.n].view(*shape)
        self.ptr = self.v.data_ptr()
        self.dtype = dtype
        assert self.ptr % 16 == 0

    def done(self, what, nan_ok=False):
        """After the launch: guards untouched, nothing left NaN; the output (as its dtype)."""
        assert bool((bits(self.buf[:GUARD]) == NAN32).all()), "%s: the guard in front of the output was written" % what
        assert bool((bits(self.buf[GUARD + self.n:]) == NAN32).all()), "%s: the guard past the output was written" % what
        if self.dtype == torch.int32:
            assert not bool((bits(self.v) == NAN32).any()), "%s: an output element was not written" % what
            return self.v.view(torch.int32)
        if not nan_ok:
            assert not bool(self.v.isnan().any()), "%s: an output element was left NaN" % what
        return self.v


class Workspace:
    """Exactly nbytes in the NaN pattern (a partial that is read before it is written shows) + a guard."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.nbytes = nbytes
        self.buf = nan_buffer(nbytes // 4 + GUARD, torch.float32)
        self.ptr = self.buf.data_ptr()

    def done(self, what):
        assert bool((bits(self.buf[self.nbytes // 4:]) == NAN32).all()), "%s: the guard past the workspace was written" % what


def pads_zero(out, K, what):
    if K < out.shape[-1]:
        assert bool((bits(out[..., K:].contiguous()) == 0).all()), "%s: an output pad column is not +0.0" % what


def ok(L, rc):
    torch.cuda.synchronize()
    assert rc == 0, L.hupr_last_error()


def stream():
    from hupr_amd import runtime as rt
    return rt.stream()


# ---- one launch of a case with pad sentinel `sent`: {name: output}, verified against fp64 if `verify` -----------------------------------
def run_wx(L, c, sent, verify):
    F, Bn, tw, exact = c.p
    o = made(c)
    K, what = o["K"], case_id(c)
    W, x = dev(o["W"]), dev(o["x"], K, sent)
    t = Out(Bn, F, 16)
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_gcn_wx_f32(W.data_ptr(), x.data_ptr(), t.ptr, Bn, F, 16, tw, stream()))
    assert L.hupr_launch_count() - n0 == 1
    out = t.done(what)
    real = out[..., :K].contiguous()
    if verify:
        ref, A = wx_ref(W, x, tw)
        if exact:
            bad = (real.double() != ref).nonzero()
            assert bad.numel() == 0, "%s: %d elements differ, first (b, row, n) = %s" % (what, bad.shape[0], bad[0].tolist())
        else:
            check(real, ref[..., :K], A[..., :K], ("wx", "any"), what)
    return {"t": real}                                   # (the pad columns of the product carry W x_pad: no contract)


def run_dw(L, c, sent, verify):
    F, Bn, exact = c.p
    o = made(c)
    K, what = o["K"], case_id(c)
    dt, x = dev(o["dt"]), dev(o["x"], K, sent)
    dW = Out(F, F)
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_gcn_dw_f32(dt.data_ptr(), x.data_ptr(), dW.ptr, Bn, F, 16, stream()))
    assert L.hupr_launch_count() - n0 == 1
    out = dW.done(what)
    if verify:
        ref, A = dw_ref(dt, x)
        if exact:
            bad = (out.double() != ref).nonzero()
            assert bad.numel() == 0, "%s: %d elements differ, first (f, g) = %s" % (what, bad.shape[0], bad[0].tolist())
        else:
            check(out, ref, A, ("dw", "any"), what)
    return {"dW": out}


def run_adj_fwd(L, c, sent, verify):
    F, Bn, K, ld, relu, _ = c.p[:6]
    S = c.p[6] if c.op == "adj_sliced" else None
    o = made(c)
    what = case_id(c)
    t, adj, bias = dev(o["t"], K, sent), dev(o["adj"]), dev(o["bias"])
    y = Out(Bn, F, ld)
    n0 = L.hupr_launch_count()
    if S:
        ok(L, L.hupr_gcn_adj_fwd_sliced_f32(t.data_ptr(), S, adj.data_ptr(), bias.data_ptr(), y.ptr, Bn, F, K, ld, relu, stream()))
    else:
        ok(L, L.hupr_gcn_adj_fwd_f32(t.data_ptr(), adj.data_ptr(), bias.data_ptr(), y.ptr, Bn, F, K, ld, relu, stream()))
    assert L.hupr_launch_count() - n0 == 1
    out = y.done(what)
    pads_zero(out, K, what)
    if verify:
        ref, A = adj_fwd_ref(t, adj, bias, K, relu)
        check(out[..., :K], ref, A, (c.op, c.route), what)
    return {"y": out}


def run_adj_bwd(L, c, sent, verify):
    F, Bn, K, ld, relu, _ = c.p
    o = made(c)
    what = case_id(c)
    dy, y, adj = dev(o["dy"], K, sent), dev(o["y"], K, sent), dev(o["adj"])
    dt, gm, db = Out(Bn, F, ld), Out(Bn, F, ld), Out(F, K)
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_gcn_adj_bwd_f32(dy.data_ptr(), y.data_ptr(), adj.data_ptr(), dt.ptr, gm.ptr, db.ptr, Bn, F, K, ld, relu, stream()))
    assert L.hupr_launch_count() - n0 == 2
    outs = {"dt": dt.done(what + " dt"), "gmasked": gm.done(what + " gmasked"), "dbias": db.done(what + " dbias")}
    pads_zero(outs["dt"], K, what + " dt")
    pads_zero(outs["gmasked"], K, what + " gmasked")
    if verify:
        g, (ref, A), (bref, bA) = adj_bwd_ref(dy, y, adj, K, relu)
        if relu:                                          # (the zeros of both signs in y are really there, and dy is not zero on them)
            zero = y[..., :K] == 0
            assert bool(zero.any()) and bool((dy[..., :K][zero] != 0).all()) and bool((g[zero] == 0).all())
        assert torch.equal(outs["gmasked"][..., :K].double(), g), "%s: the masked gradient is not dy [y > 0] exactly" % what
        check(outs["dt"][..., :K], ref, A, ("adj_bwd", "any"), what + " dt")
        check(outs["dbias"], bref, bA, ("dbias", "any"), what + " dbias")
    return outs


class Counted:
    """The PRGCN entry points of rt.lib() wrapped by call counters for the block."""

    def __init__(self, L, names=LAYER_ENTRIES + ("hupr_gcn_adj_bwd_f32",)):
        self.L, self.names, self.n, self.orig = L, names, collections.Counter(), {}

    def __enter__(self):
        for name in self.names:
            self.orig[name] = orig = getattr(self.L, name)

            def f(*a, _name=name, _orig=orig):
                self.n[_name] += 1
                return _orig(*a)
            setattr(self.L, name, f)
        return self

    def __exit__(self, *exc):
        for name, orig in self.orig.items():
            setattr(self.L, name, orig)

    def take(self):
        n, self.n = dict(self.n), collections.Counter()
        return n


# what each forward route calls forward, and what its backward calls (a single sample's backward is the generic engine's)
LAYER_CALLS = {"sliced": ({"hupr_gemm_f32": 1, "hupr_gcn_adj_fwd_sliced_f32": 1}, {"hupr_gcn_adj_bwd_f32": 1, "hupr_gemm_f32": 2}),
               "products": ({"hupr_gcn_wx_f32": 1, "hupr_gcn_adj_fwd_f32": 1}, {"hupr_gcn_adj_bwd_f32": 1, "hupr_gcn_wx_f32": 1, "hupr_gcn_dw_f32": 1}),
               "generic": ({"hupr_gemm_f32": 1, "hupr_gcn_adj_fwd_f32": 1}, {"hupr_gcn_adj_bwd_f32": 1, "hupr_gemm_f32": 2})}


def counted_route(calls):
    """The forward route that a dictionary of counted calls shows."""
    if calls.get("hupr_gcn_adj_fwd_sliced_f32"):
        return "sliced"
    return "products" if calls.get("hupr_gcn_wx_f32") else "generic"


def run_layer(L, c, sent, verify):
    from hupr_amd import functional as F_
    B, F, relu, products = c.p
    o = made(c)
    K, what = 14, case_id(c)
    x, W, bias = (dev(o["x"], K, sent).requires_grad_(True), dev(o["W"]).requires_grad_(True), dev(o["bias"]).requires_grad_(True))
    dy, adj = dev(o["dy"], K, sent), dev(o["adj"])
    was = F_.GCN_PRODUCTS
    F_.GCN_PRODUCTS = products
    try:
        want = F_.gcn_route(B, F, 16, W.shape, torch.float32), F_.gcn_route(B, F, 16, W.shape, torch.float32, backward=True)
        with Counted(L) as n:
            y = F_.GCNLayerFn.apply(x, W, bias, adj, bool(relu))
            fwd = n.take()
            y.backward(dy)
            bwd = n.take()
    finally:
        F_.GCN_PRODUCTS = was
    torch.cuda.synchronize()
    assert want[0] == c.route == counted_route(fwd), (want, c.route, fwd)
    assert fwd == LAYER_CALLS[c.route][0], fwd
    assert bwd == LAYER_CALLS[want[1] if want[1] == "products" else "generic"][1], bwd
    assert want[1] == ("products" if bwd.get("hupr_gcn_dw_f32") else "generic")
    y = y.detach()
    outs = {"y": y, "dx": x.grad[..., :K].contiguous(), "dW": W.grad, "dbias": bias.grad}
    for name, t in outs.items():
        assert not bool(t.isnan().any()), "%s: %s holds a NaN" % (what, name)
    pads_zero(y, K, what)
    if verify:
        ref, A = layer_fwd_ref(x.detach(), W.detach(), bias.detach(), adj, relu)
        check(y[..., :K], ref, A, ("layer_fwd", c.route), what + " y")
        g = dy.double()[..., :K] * (y[..., :K] > 0) if relu else dy.double()[..., :K]            # the mask of the kernel's own y
        (dx, dxA), (dw, dwA) = layer_bwd_ref(x.detach(), W.detach(), adj, g)
        check(outs["dx"], dx, dxA, ("layer_dx", want[1]), what + " dx")
        check(outs["dW"], dw, dwA, ("layer_dw", want[1]), what + " dW")
        check(outs["dbias"], g.sum(0), g.abs().sum(0), ("dbias", "any"), what + " dbias")
    return outs


def run_head(L, c, sent, verify):
    M, rows, null = c.p
    o = made(c)
    what = case_id(c)
    x, w, dy = dev(o["x"]), dev(o["w"]), dev(o["dy"], rows, sent)
    y, dx, dw = Out(M, 16), Out(M, 32), Out(16, 32)
    ws = Workspace(L.hupr_head1x1_ws_bytes())
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_head1x1_fwd_f32(x.data_ptr(), w.data_ptr(), y.ptr, M, stream()))
    assert L.hupr_launch_count() - n0 == 1
    args = (dx.ptr if null != "dx" else None, dw.ptr if null != "dw" else None)
    if rows == 16:
        ok(L, L.hupr_head1x1_bwd_f32(x.data_ptr(), w.data_ptr(), dy.data_ptr(), *args, M, ws.ptr, ws.nbytes, stream()))
    else:
        ok(L, L.hupr_head1x1_bwd_rows_f32(x.data_ptr(), w.data_ptr(), dy.data_ptr(), *args, rows, M, ws.ptr, ws.nbytes, stream()))
    assert L.hupr_launch_count() - n0 == 1 + (null != "dx") + 2 * (null != "dw")
    ws.done(what)
    outs = {"y": y.done(what + " y")}
    pads_zero(outs["y"], rows, what + " y")
    (yr, yA), (dxr, dxA), (dwr, dwA) = head_ref(x, w, dy, rows) if verify else ((None,) * 2,) * 3
    if null == "dx":
        assert bool((bits(dx.buf) == NAN32).all()), "%s: dx was written though its pointer was null" % what
    else:
        outs["dx"] = dx.done(what + " dx")
    if null == "dw":
        assert bool((bits(dw.buf) == NAN32).all()), "%s: dw was written though its pointer was null" % what
    else:
        full = dw.done(what + " dw", nan_ok=True)
        assert bool((bits(full[rows:]) == NAN32).all()), "%s: a row of dw past out_rows was written" % what
        outs["dw"] = full[:rows]
        assert not bool(outs["dw"].isnan().any()), "%s: an element of dw was left NaN" % what
    if verify:
        check(outs["y"][:, :rows], yr[:, :rows], yA[:, :rows], ("head_fwd", "any"), what + " y")
        if "dx" in outs:
            check(outs["dx"], dxr, dxA, ("head_dgrad", "any"), what + " dx")
        if "dw" in outs:
            check(outs["dw"], dwr, dwA, ("head_wgrad", "any"), what + " dw")
    return outs


def run_sigmoid(L, c, sent, verify):
    Bn, K, ld, HW = c.p
    o = made(c)
    what = case_id(c)
    x, dy = dev(o["x"], K, sent), dev(o["dy"])
    y, dx = Out(Bn, K, HW), Out(Bn, HW, ld)
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_sigmoid_to_nchw_f32(x.data_ptr(), y.ptr, Bn, HW, K, ld, stream()))
    p = y.done(what + " p")
    ok(L, L.hupr_sigmoid_to_nchw_bwd_f32(dy.data_ptr(), p.data_ptr(), dx.ptr, Bn, HW, K, ld, stream()))
    assert L.hupr_launch_count() - n0 == 2
    outs = {"p": p, "dx": dx.done(what + " dx")}
    pads_zero(outs["dx"], K, what + " dx")
    if verify:
        ref = sigmoid_ref(x, K)
        check(p, ref, 1.0, ("sigmoid", "any"), what + " p")
        # the saturated logits: p exactly 0.5 at +-0, exactly 1 / 0 at +-90 (expf overflows to inf), and their gradients exactly 0
        v = x[..., :K].reshape(-1)[:len(SPECIAL_LOGITS)]
        pv = p.permute(0, 2, 1).reshape(-1)[:v.numel()]
        want = {0.0: 0.5, 90.0: 1.0, -90.0: 0.0}
        for i, lv in enumerate(v.tolist()):
            assert lv == SPECIAL_LOGITS[i]
            if lv in want:
                assert pv[i].item() == want[lv], "%s: sigmoid(%r) = %r" % (what, lv, pv[i].item())
            if abs(lv) == 90.0:
                assert outs["dx"][..., :K].reshape(-1)[i].item() == 0.0
        # the backward against fp64 of exactly what it reads: dy and the kernel's own p
        gref = (dy.double() * p.double() * (1 - p.double())).permute(0, 2, 1)
        check(outs["dx"][..., :K], gref, gref.abs(), ("sigmoid_bwd", "any"), what + " dx")
    return outs


def torch_bce_cpu(p, t, scale):
    """torch's own fp32 BCE on the CPU: (loss, scale x its gradient)."""
    pc = p.cpu().clone().requires_grad_(True)
    loss = torch.nn.functional.binary_cross_entropy(pc, t.cpu())
    (loss * scale).backward()
    return loss.detach(), pc.grad


def run_bce(L, c, sent, verify):
    n, kind = c.p
    o = made(c)
    what = case_id(c)
    p, t, g = dev(o["p1"]), dev(o["t"]), dev(torch.tensor([G_OUT]))
    loss, dp = Out(1), Out(n)
    ws = Workspace(L.hupr_bce_ws_bytes())
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_bce_fwd_f32(p.data_ptr(), t.data_ptr(), n, loss.ptr, ws.ptr, ws.nbytes, stream()))
    ok(L, L.hupr_bce_bwd_f32(p.data_ptr(), t.data_ptr(), g.data_ptr(), dp.ptr, n, stream()))
    assert L.hupr_launch_count() - n0 == 3
    ws.done(what)
    outs = {"loss": loss.done(what + " loss"), "dp": dp.done(what + " dp")}
    assert bool(outs["loss"].isfinite().all()) and bool(outs["dp"].isfinite().all()), what
    if verify:
        ref, A = bce_ref(p, t)
        check(outs["loss"], ref, A, ("bce", "any"), what + " loss")
        gref = bce_grad_ref(p, t, G_OUT)
        check(outs["dp"], gref, gref.abs(), ("bce_bwd", "any"), what + " dp")
        if kind == "saturated":                          # the -100 clamp and the 1e-12 floor as torch has them, in fp32
            lt, gt = torch_bce_cpu(p, t, G_OUT)
            check(outs["loss"].cpu(), lt.double().view(1), A.cpu(), ("bce", "any"), what + " loss vs torch")
            check(outs["dp"].cpu(), gt.double(), gt.double().abs(), ("bce_bwd", "any"), what + " dp vs torch")
    return outs


def run_bce_pair(L, c, sent, verify):
    n, kind = c.p
    o = made(c)
    what = case_id(c)
    p1, p2, t = dev(o["p1"]), dev(o["p2"]), dev(o["t"])
    g, g2 = dev(torch.tensor([G_OUT])), dev(torch.tensor([G_OUT2]))
    loss3, d1, d2, e1, e2 = Out(3), Out(n), Out(n), Out(n), Out(n)
    ws = Workspace(2 * L.hupr_bce_ws_bytes())
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_bce_pair_fwd_f32(p1.data_ptr(), p2.data_ptr(), t.data_ptr(), n, ALPHA, BETA, loss3.ptr, ws.ptr, ws.nbytes, stream()))
    ok(L, L.hupr_bce_pair_bwd_f32(p1.data_ptr(), p2.data_ptr(), t.data_ptr(), g.data_ptr(), None, ALPHA, BETA, d1.ptr, d2.ptr, n, stream()))
    ok(L, L.hupr_bce_pair_bwd_f32(p1.data_ptr(), p2.data_ptr(), t.data_ptr(), g.data_ptr(), g2.data_ptr(), ALPHA, BETA, e1.ptr, e2.ptr, n,
                                  stream()))
    assert L.hupr_launch_count() - n0 == 4
    ws.done(what)
    outs = {"loss3": loss3.done(what + " losses"), "dp1": d1.done(what + " dp1"), "dp2": d2.done(what + " dp2"),
            "dp1 (grad_loss2)": e1.done(what + " dp1"), "dp2 (grad_loss2)": e2.done(what + " dp2")}
    assert all(bool(v.isfinite().all()) for v in outs.values()), what
    assert torch.equal(bits(outs["dp1"]), bits(outs["dp1 (grad_loss2)"])), "%s: grad_loss2 reached dp1" % what
    if verify:
        (l1, A1), (l2, A2) = bce_ref(p1, t), bce_ref(p2, t)
        A3 = torch.cat([ALPHA * A1 + BETA * A2, A1, A2])
        check(outs["loss3"], torch.cat([ALPHA * l1 + BETA * l2, l1, l2]), A3, ("bce", "any"), what + " loss, loss1, loss2")
        for name, p, scale in (("dp1", p1, G_OUT * ALPHA), ("dp2", p2, G_OUT * BETA), ("dp2 (grad_loss2)", p2, G_OUT * BETA + G_OUT2)):
            gref = bce_grad_ref(p, t, scale)
            check(outs[name], gref, gref.abs(), ("bce_bwd", "any"), "%s %s" % (what, name))
        if kind == "saturated":
            for name, p, scale, i in (("dp1", p1, G_OUT * ALPHA, 1), ("dp2", p2, G_OUT * BETA, 2)):
                lt, gt = torch_bce_cpu(p, t, float(np.float32(scale)))
                check(outs["loss3"][i:i + 1].cpu(), lt.double().view(1), A3[i:i + 1].cpu(), ("bce", "any"), "%s loss%d vs torch" % (what, i))
                check(outs[name].cpu(), gt.double(), gt.double().abs(), ("bce_bwd", "any"), "%s %s vs torch" % (what, name))
    return outs


def run_targets(L, c, sent, verify):
    from hupr_amd import functional as F_
    B, K, H = c.p
    o = made(c)
    what = case_id(c)
    joints = dev(torch.from_numpy(o["joints"]), dtype=torch.int64)
    F_.gaussian_targets(joints[:1])                       # (fills the patch table of sigma = 2)
    patch = dev(F_._PATCH_CACHE[(2, joints.device)])
    t = Out(B, K, H, H)
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_gaussian_targets_f32(joints.data_ptr(), patch.data_ptr(), t.ptr, B * K, H, 6, 256.0 / H, stream()))
    assert L.hupr_launch_count() - n0 == 1
    out = t.done(what)
    if verify:
        from oracle import loss as oloss
        want, _ = oloss.batch_targets(o["joints"])
        assert torch.equal(bits(out.cpu()), bits(torch.from_numpy(want))), "%s: the targets are not the oracle's bits" % what
    return {"t": out}


def run_argmax(L, c, sent, verify):
    (n,) = c.p
    o = made(c)
    what = case_id(c)
    rows = o["p"].shape[0]
    p = dev(o["p"])
    idx, mx = Out(rows, dtype=torch.int32), Out(rows)
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_argmax_rows_f32(p.data_ptr(), rows, n, idx.ptr, mx.ptr, stream()))
    assert L.hupr_launch_count() - n0 == 1
    outs = {"idx": idx.done(what + " idx"), "max": mx.done(what + " max")}
    if verify:
        assert outs["idx"].cpu().tolist() == o["idx"].tolist(), (what, outs["idx"].cpu().tolist(), o["idx"].tolist())
        assert torch.equal(bits(outs["max"].cpu()), bits(o["max"])), what
    return outs


def run_softmax(L, c, sent, verify):
    rows, n, mag = c.p
    o = made(c)
    what = case_id(c)
    x, dp = dev(o["x"]), dev(o["dp"])
    s, d = Out(rows, n), Out(rows, n)
    s.v.copy_(x)
    d.v.copy_(dp)
    n0 = L.hupr_launch_count()
    ok(L, L.hupr_softmax_rows_f32(s.ptr, rows, n, stream()))
    p = s.done(what + " p")
    ok(L, L.hupr_softmax_rows_bwd_f32(p.data_ptr(), d.ptr, rows, n, stream()))
    assert L.hupr_launch_count() - n0 == 2
    outs = {"p": p, "ds": d.done(what + " ds")}
    if verify:
        ref = softmax_ref(x)
        check(p, ref, ref.max(dim=1, keepdim=True).values.expand_as(ref), ("softmax", "any"), what + " p")
        gref, A = softmax_bwd_ref(p, dp)                  # of exactly what the backward reads: the kernel's own p
        # (behind logits of magnitude 80 some p, and their ds, are denormal: one rounding there costs up to 2^-149 whatever A is)
        check(outs["ds"], gref, A, ("softmax_bwd", "any"), what + " ds", floor=DENORMAL)
    return outs


OPS = {"wx": run_wx, "dw": run_dw, "adj_fwd": run_adj_fwd, "adj_sliced": run_adj_fwd, "adj_bwd": run_adj_bwd, "layer": run_layer,
       "head": run_head, "sigmoid": run_sigmoid, "bce": run_bce, "bce_pair": run_bce_pair, "targets": run_targets, "argmax": run_argmax,
       "softmax": run_softmax}
assert {c.op for c in CASES} == set(OPS)


@pytest.fixture
def lib():
    from hupr_amd import runtime
    return runtime.lib()


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_head_case_matches_fp64(c, lib):
    """The case against fp64 under its gate (or exactly, where the case is exact), every element; guards untouched, nothing left NaN,
    output pads +0.0; the same bits from a second launch, and from a third whose input pad columns hold another sentinel."""
    run = OPS[c.op]
    first = run(lib, c, SENT[0], True)
    for sent, why in ((SENT[0], "two launches differ"), (SENT[1], "the result depends on the input pad columns")):
        again = run(lib, c, sent, False)
        assert again.keys() == first.keys()
        for name in first:
            assert torch.equal(bits(again[name]), bits(first[name])), "%s: %s (%s)" % (case_id(c), why, name)


def test_head_of_no_voxels_launches_nothing(lib):
    """M = 0: HUPR_OK and not one launch, whatever the pointers."""
    n0 = lib.hupr_launch_count()
    assert lib.hupr_head1x1_fwd_f32(None, None, None, 0, stream()) == 0
    assert lib.hupr_head1x1_bwd_rows_f32(None, None, None, None, None, 14, 0, None, 0, stream()) == 0
    assert lib.hupr_head1x1_bwd_f32(None, None, None, None, None, 0, None, 0, stream()) == 0
    assert lib.hupr_launch_count() == n0


# ---- the other nodes of functional.py, entry points counted ----------------------------------------------------------------------------
NODE_ENTRIES = ("hupr_head1x1_fwd_f32", "hupr_head1x1_bwd_rows_f32", "hupr_head1x1_bwd_f32", "hupr_sigmoid_to_nchw_f32",
                "hupr_sigmoid_to_nchw_bwd_f32", "hupr_bce_fwd_f32", "hupr_bce_bwd_f32", "hupr_bce_pair_fwd_f32", "hupr_bce_pair_bwd_f32")


def test_head_conv_node_runs_the_dedicated_kernels_inside_a_switched_head_region_only(lib):
    """head_conv inside the "head" region of a bf16 run: Head1x1Fn, one call of the forward and one of the 14-row backward, all three
    results inside the gates of the C-ABI cases; in an fp32 run: none of these entry points (the generic convolution)."""
    from hupr_amd import functional as F_
    B, H, K = 2, 9, 14                                   # 162 voxels: one workgroup of two chunks, the second ragged
    c = Case("head", HEAD14, "any", (B * H * H, K, ""))
    o = make_head(c)
    x = o["x"].view(B, 1, H, H, 32).cuda().requires_grad_(True)
    w = o["w"][:K].reshape(K, 32, 1, 1).cuda().requires_grad_(True)
    dy = dev(o["dy"], K, SENT[0]).view(B, 1, H, H, 16)
    assert F_.head_route(True, True, torch.float32, 32, w.shape, K) == "head1x1"
    F_.set_math("bf16")
    try:
        with Counted(lib, NODE_ENTRIES) as n:
            with F_.region("head"):
                y = F_.head_conv(x, w, K)
            assert n.take() == {"hupr_head1x1_fwd_f32": 1}
            y.backward(dy)
            assert n.take() == {"hupr_head1x1_bwd_rows_f32": 1}
    finally:
        F_.set_math("f32")
    torch.cuda.synchronize()
    (yr, yA), (dxr, dxA), (dwr, dwA) = head_ref(x.detach().view(-1, 32), o["w"].cuda(), dy.view(-1, 16), K)
    pads_zero(y.detach(), K, "head_conv")
    check(y.detach().view(-1, 16)[:, :K], yr[:, :K], yA[:, :K], ("head_fwd", "any"), "head_conv y")
    check(x.grad.view(-1, 32), dxr, dxA, ("head_dgrad", "any"), "head_conv dx")
    assert tuple(w.grad.shape) == (K, 32, 1, 1)
    check(w.grad.view(K, 32), dwr, dwA, ("head_wgrad", "any"), "head_conv dw")
    with Counted(lib, NODE_ENTRIES) as n:                # an fp32 run: the parity path keeps the generic convolution
        assert F_.MATH == "f32"
        with F_.region("head"):
            y2 = F_.head_conv(x.detach(), w.detach(), K)
        assert n.take() == {}
    assert bool(within(y2.view(-1, 16)[:, :K], yr[:, :K], yA[:, :K], CAP).all()), "head_conv y, generic convolution"


def test_sigmoid_and_loss_nodes_call_each_entry_once_and_match_fp64(lib):
    """SigmoidHeadFn, BCEFn and PairBCEFn: the entry points of each forward and backward counted, every result inside the gates of the
    C-ABI cases."""
    from hupr_amd import functional as F_
    c = Case("sigmoid", SIGMOID, "any", (2, 14, 16, 63))
    o = make_sigmoid(c)
    x = dev(o["x"], 14, SENT[0]).requires_grad_(True)
    dy = o["dy"].cuda()
    with Counted(lib, NODE_ENTRIES) as n:
        p = F_.SigmoidHeadFn.apply(x, 14)
        assert n.take() == {"hupr_sigmoid_to_nchw_f32": 1}
        p.backward(dy)
        assert n.take() == {"hupr_sigmoid_to_nchw_bwd_f32": 1}
        p = p.detach()
        check(p, sigmoid_ref(x.detach(), 14), 1.0, ("sigmoid", "any"), "SigmoidHeadFn p")
        gref = (dy.double() * p.double() * (1 - p.double())).permute(0, 2, 1)
        check(x.grad[..., :14], gref, gref.abs(), ("sigmoid_bwd", "any"), "SigmoidHeadFn dx")
        pads_zero(x.grad, 14, "SigmoidHeadFn dx")
        ob = make_bce(Case("bce_pair", PAIR, "any", (2 * 14 * 63, "random")))
        t = ob["t"].cuda().view(2, 14, 63)
        p1, p2 = p.clone().requires_grad_(True), ob["p2"].cuda().view(2, 14, 63).requires_grad_(True)
        loss = F_.BCEFn.apply(p1, t)
        assert n.take() == {"hupr_bce_fwd_f32": 1}
        (loss * G_OUT).backward()
        assert n.take() == {"hupr_bce_bwd_f32": 1}
        (l1, A1), (l2, A2) = bce_ref(p1.detach(), t), bce_ref(p2.detach(), t)
        check(loss.detach().view(1), l1, A1, ("bce", "any"), "BCEFn loss")
        g1 = bce_grad_ref(p1.detach(), t, G_OUT)
        check(p1.grad, g1, g1.abs(), ("bce_bwd", "any"), "BCEFn dp")
        p1.grad = None
        both, second = F_.PairBCEFn.apply(p1, p2, t, ALPHA, BETA)
        assert n.take() == {"hupr_bce_pair_fwd_f32": 1}
        (both * G_OUT + second * G_OUT2).backward()
        assert n.take() == {"hupr_bce_pair_bwd_f32": 1}
    check(torch.stack([both.detach(), second.detach()]), torch.cat([ALPHA * l1 + BETA * l2, l2]), torch.cat([ALPHA * A1 + BETA * A2, A2]),
          ("bce", "any"), "PairBCEFn loss, loss2")
    g1, g2 = bce_grad_ref(p1.detach(), t, G_OUT * ALPHA), bce_grad_ref(p2.detach(), t, G_OUT * BETA + G_OUT2)
    check(p1.grad, g1, g1.abs(), ("bce_bwd", "any"), "PairBCEFn dp1")
    check(p2.grad, g2, g2.abs(), ("bce_bwd", "any"), "PairBCEFn dp2")


# ---- refused calls: (what, entry point, arguments as a function of the base addresses (x, w, y, ws) and the workspace size) --------------
def _refused():
    r = []
    for ld, F in ((14, 64), (16, 96)):
        r.append(("wx: ld = %d, F = %d" % (ld, F), lambda L, a, ld=ld, F=F: L.hupr_gcn_wx_f32(a[1], a[0], a[2], 2, F, ld, 0, None)))
        r.append(("dw: ld = %d, F = %d" % (ld, F), lambda L, a, ld=ld, F=F: L.hupr_gcn_dw_f32(a[0], a[1], a[2], 2, F, ld, None)))
    for K, ld in ((17, 17), (14, 12), (14, 20)):
        r.append(("adj fwd: K = %d, ld = %d" % (K, ld), lambda L, a, K=K, ld=ld: L.hupr_gcn_adj_fwd_f32(a[0], a[1], a[1], a[2], 2, 64, K, ld, 1, None)))
        r.append(("adj sliced: K = %d, ld = %d" % (K, ld),
                  lambda L, a, K=K, ld=ld: L.hupr_gcn_adj_fwd_sliced_f32(a[0], 2, a[1], a[1], a[2], 2, 64, K, ld, 1, None)))
        r.append(("adj bwd: K = %d, ld = %d" % (K, ld),
                  lambda L, a, K=K, ld=ld: L.hupr_gcn_adj_bwd_f32(a[0], a[0], a[1], a[2], a[2], a[2], 2, 64, K, ld, 1, None)))
    for S in (0, 65):
        r.append(("adj sliced: slices = %d" % S, lambda L, a, S=S: L.hupr_gcn_adj_fwd_sliced_f32(a[0], S, a[1], a[1], a[2], 1, 64, 14, 16, 1, None)))
    wsb = lambda L: L.hupr_head1x1_ws_bytes()
    for rows in (0, 17):
        r.append(("head bwd: out_rows = %d" % rows,
                  lambda L, a, rows=rows: L.hupr_head1x1_bwd_rows_f32(a[0], a[1], a[0], a[2], a[2], rows, 64, a[3], wsb(L), None)))
    r.append(("head fwd: x misaligned by 4 bytes", lambda L, a: L.hupr_head1x1_fwd_f32(a[0] + 4, a[1], a[2], 64, None)))
    r.append(("head bwd: x misaligned by 4 bytes", lambda L, a: L.hupr_head1x1_bwd_rows_f32(a[0] + 4, a[1], a[0], a[2], a[2], 14, 64, a[3], wsb(L), None)))
    r.append(("head bwd: dy misaligned by 4 bytes", lambda L, a: L.hupr_head1x1_bwd_rows_f32(a[0], a[1], a[0] + 4, a[2], a[2], 14, 64, a[3], wsb(L), None)))
    r.append(("head bwd: workspace one byte short",
              lambda L, a: L.hupr_head1x1_bwd_rows_f32(a[0], a[1], a[0], None, a[2], 14, 64, a[3], wsb(L) - 1, None)))
    r.append(("head bwd (16 rows): workspace one byte short",
              lambda L, a: L.hupr_head1x1_bwd_f32(a[0], a[1], a[0], None, a[2], 64, a[3], wsb(L) - 1, None)))
    r.append(("softmax: n = 6", lambda L, a: L.hupr_softmax_rows_f32(a[2], 2, 6, None)))
    r.append(("softmax bwd: n = 6", lambda L, a: L.hupr_softmax_rows_bwd_f32(a[0], a[2], 2, 6, None)))
    r.append(("bce: workspace one byte short", lambda L, a: L.hupr_bce_fwd_f32(a[0], a[1], 64, a[2], a[3], L.hupr_bce_ws_bytes() - 1, None)))
    r.append(("pair bce: workspace one byte short",
              lambda L, a: L.hupr_bce_pair_fwd_f32(a[0], a[0], a[1], 64, 0.5, 0.5, a[2], a[3], 2 * L.hupr_bce_ws_bytes() - 1, None)))
    return r


REFUSED = _refused()


@pytest.mark.parametrize("r", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_calls_leave_everything_untouched(r, lib):
    """Calls the launchers refuse return HUPR_ERR_ARG or HUPR_ERR_WORKSPACE before any launch: the output, the workspace and their
    guards keep the NaN pattern bit for bit and hupr_launch_count() does not move.  (tests/test_head_route.py verifies without a device
    that the refusals are host checks.)"""
    what, call = r
    n = 1 << 16
    x, w = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    out, ws = nan_buffer(n, torch.float32), nan_buffer(1 << 18, torch.float32)
    n0 = lib.hupr_launch_count()
    rc = call(lib, (x.data_ptr(), w.data_ptr(), out.data_ptr(), ws.data_ptr()))
    torch.cuda.synchronize()
    assert rc in (HUPR_ERR_ARG, HUPR_ERR_WORKSPACE), (what, rc)
    assert lib.hupr_launch_count() == n0, what
    assert bool((bits(out) == NAN32).all()) and bool((bits(ws) == NAN32).all()), what
