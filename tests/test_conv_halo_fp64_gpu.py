"""GPU (-m gpu): every form of the halo-tiled 3x3(x3) convolution (hupr_conv3x3_halo_bf16(act)(_ws|_stats)) against an fp64
convolution of exactly the operands the kernel sees, element by element, with the route of every launch asserted first
(hupr_debug_halo_route): each instantiation of the 256-voxel kernel, each of the 128-voxel kernel and its K-sliced form.

Gate (``within_bound``), with A the same convolution over absolute values (+ |bias| + |res|):
  bf16-stored output  |y - ref| <= 2^-8 |ref| + 2^-16 A   (one round-to-nearest-even bf16 store + fp32 accumulation slack;
                                                           the bf16 x bf16 products are exact in fp32)
  fp32 output         |y - ref| <= 2^-16 A
Batch items {0, 1, B // 2, B - 1} are compared entirely (the last one holds the tail of the tile sequence).  Output buffers are
NaN-filled with their padding columns and a guard tail, which must come back NaN bit for bit; input channels beyond Ci and residual
columns beyond Co are NaN and must not reach the output.  tests/test_conv_halo_route.py checks the routes of this table and that
the gate rejects a kernel that drops one (tap, 8-channel) product slice or one bias channel — without a GPU."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG = -1
# route codes of hupr_debug_halo_route (include/hupr_debug.h): the 256-voxel kernel's instantiations ...
CI32, CO32, T1X16X16, STATS_ONE, STATS_TWO, STATS_2X8X16, T4X8X8, T2X8X16 = range(1, 9)


def r128(bn, kc, kd, abf, slices=1):
    """... and the 128-voxel kernel's hupr_k_conv_halo_bf16<BN, KC, abf, kd == 3> over `slices` K slices."""
    return 256 + 16 * slices + 8 * (bn == 64) + 4 * (kc == 64) + 2 * (kd == 3) + int(abf)


# act: "bf16" hupr_conv3x3_halo_bf16act, "f32" hupr_conv3x3_halo_bf16 (fp32-stored activations), "ws" the _ws entry with a
# workspace, "stats" the _stats entry.  epi: bias / res / inplace (the output written over the residual: out_ld == res_ld).
# pad: (in_ld - Ci, out_ld - Co, res_ld - Co).  out_ld % 8 == 0: the 256-voxel kernel's deferred ("parked") epilogue where bias and
# residual allow it; out_ld = Co + 4: the immediate one.
Case = collections.namedtuple("Case", "B Ci Co D H W kd act epi pad route")
S = (8, 8, 12)           # strided, deferred epilogue, res_ld != Co
I = (8, 4, 12)           # strided, immediate epilogue
P = (0, 0, 0)            # dense
CASES = [
    # 4 x 8 x 8: 1, 2, 4 channel chunks x 1, 2, 4 output tiles; the level-1 bench shape; 288 tiles over 256 workgroups
    Case(32, 64, 64, 8, 64, 64, 3, "bf16", "", P, T4X8X8),
    Case(9, 128, 128, 4, 32, 32, 3, "bf16", "res", S, T4X8X8),
    Case(9, 128, 128, 4, 32, 32, 3, "bf16", "res", I, T4X8X8),
    Case(16, 256, 256, 4, 16, 16, 3, "bf16", "bias res", S, T4X8X8),
    Case(8, 64, 256, 4, 16, 32, 3, "bf16", "inplace", (8, 12, 12), T4X8X8),
    Case(64, 256, 64, 4, 16, 16, 3, "bf16", "inplace", (8, 8, 8), T4X8X8),
    Case(4, 64, 128, 8, 32, 64, 3, "bf16", "bias", I, T4X8X8),
    Case(4, 64, 128, 8, 32, 64, 3, "bf16", "", S, T4X8X8),
    Case(9, 128, 128, 4, 32, 32, 3, "bf16", "", I, T4X8X8),
    # Ci = 32 (the encoders' first convolution, 64-byte rows): none, bias, res, bias + res, in place; the level-1 bench shape
    Case(32, 32, 64, 8, 64, 64, 3, "bf16", "bias", P, CI32),
    Case(16, 32, 64, 4, 32, 32, 3, "bf16", "", S, CI32),
    Case(16, 32, 64, 4, 32, 32, 3, "bf16", "", I, CI32),
    Case(16, 32, 64, 4, 32, 32, 3, "bf16", "bias", I, CI32),
    Case(7, 32, 128, 4, 32, 48, 3, "bf16", "res", S, CI32),
    Case(7, 32, 128, 4, 32, 48, 3, "bf16", "res", I, CI32),
    Case(7, 32, 128, 4, 32, 48, 3, "bf16", "bias res", S, CI32),
    Case(7, 32, 128, 4, 32, 48, 3, "bf16", "bias res", I, CI32),
    Case(16, 32, 64, 4, 32, 32, 3, "bf16", "bias inplace", (8, 8, 8), CI32),
    Case(16, 32, 64, 4, 32, 32, 3, "bf16", "inplace", (8, 4, 4), CI32),
    # Co = 32 (the first layer's input gradient, 8 x 8 x 8 tile): one and two channel chunks; out_ld % 8 != 0 leaves it
    Case(4, 64, 32, 8, 64, 64, 3, "bf16", "", S, CO32),
    Case(9, 128, 32, 8, 32, 64, 3, "bf16", "res", S, CO32),
    Case(4, 64, 32, 8, 64, 64, 3, "bf16", "", I, r128(32, 64, 3, 1)),
    # 2 x 8 x 16 (depth 2): 1, 2, 4 channel chunks at >= 256 tiles
    Case(64, 64, 64, 2, 16, 32, 3, "bf16", "bias", S, T2X8X16),
    Case(33, 128, 128, 2, 16, 32, 3, "bf16", "", S, T2X8X16),
    Case(32, 256, 256, 2, 16, 16, 3, "bf16", "res", S, T2X8X16),
    # 1 x 16 x 16 (the decoder's 1 x 3 x 3 taps): Ci = 320 -> 64, Co = 192
    Case(16, 320, 64, 1, 64, 64, 1, "bf16", "res", S, T1X16X16),
    Case(17, 320, 64, 1, 64, 64, 1, "bf16", "", I, T1X16X16),
    Case(15, 64, 192, 1, 32, 48, 1, "bf16", "inplace", (8, 8, 8), T1X16X16),
    # fused BatchNorm statistics: one / two output tiles per workgroup, the 2 x 8 x 16 tile
    Case(16, 64, 64, 4, 32, 32, 3, "stats", "", S, STATS_ONE),
    Case(8, 128, 128, 4, 32, 32, 3, "stats", "", I, STATS_ONE),
    Case(12, 128, 128, 4, 32, 32, 3, "stats", "", P, STATS_TWO),
    Case(32, 128, 256, 2, 16, 16, 3, "stats", "", S, STATS_2X8X16),
    # the 128-voxel kernel: BN 32 / 64 x KC 32 / 64 x kd 3 / 1, bf16- and fp32-stored activations; a Co that is not a multiple of 8
    Case(2, 32, 32, 4, 16, 16, 3, "bf16", "bias res", S, r128(32, 32, 3, 1)),
    Case(2, 32, 32, 4, 16, 16, 3, "f32", "bias res", (4, 4, 8), r128(32, 32, 3, 0)),
    Case(9, 96, 64, 4, 32, 32, 3, "bf16", "res", S, r128(64, 32, 3, 1)),
    Case(9, 96, 64, 4, 32, 32, 3, "f32", "res", (4, 4, 8), r128(64, 32, 3, 0)),
    Case(2, 64, 64, 4, 16, 16, 3, "bf16", "inplace", (8, 8, 8), r128(32, 64, 3, 1)),
    Case(2, 64, 64, 4, 16, 16, 3, "f32", "bias", (4, 4, 4), r128(32, 64, 3, 0)),
    Case(5, 64, 96, 4, 32, 32, 3, "bf16", "bias res", S, r128(64, 64, 3, 1)),
    Case(5, 64, 96, 4, 32, 32, 3, "f32", "", (4, 4, 4), r128(64, 64, 3, 0)),
    Case(2, 32, 32, 1, 16, 16, 1, "bf16", "bias", I, r128(32, 32, 1, 1)),
    Case(2, 32, 32, 1, 16, 16, 1, "f32", "res", (4, 4, 8), r128(32, 32, 1, 0)),
    Case(9, 96, 64, 1, 64, 64, 1, "bf16", "bias res", S, r128(64, 32, 1, 1)),
    Case(9, 96, 64, 1, 64, 64, 1, "f32", "inplace", (4, 4, 4), r128(64, 32, 1, 0)),
    Case(2, 64, 64, 1, 16, 32, 1, "bf16", "res", S, r128(32, 64, 1, 1)),
    Case(2, 64, 64, 1, 16, 32, 1, "f32", "bias", (4, 4, 4), r128(32, 64, 1, 0)),
    Case(9, 64, 96, 1, 64, 64, 1, "bf16", "", S, r128(64, 64, 1, 1)),
    Case(9, 64, 96, 1, 64, 64, 1, "f32", "bias res", (4, 4, 8), r128(64, 64, 1, 0)),
    Case(2, 32, 36, 2, 8, 8, 3, "bf16", "bias res", (8, 4, 4), r128(64, 32, 3, 1)),
    # the K-sliced form (single-sample grids, caller's workspace) with bias + residual
    Case(1, 128, 256, 2, 16, 16, 3, "ws", "bias res", S, r128(32, 64, 3, 1, slices=6)),
]


def case_id(c):
    return "%s-B%d-%dto%d-%dx%dx%d-k%d-%s-ld%d.%d.%d" % (c.act, c.B, c.Ci, c.Co, c.D, c.H, c.W, c.kd, c.epi.replace(" ", "+") or "plain",
                                                       *c.pad)


def lds(c):
    in_ld, out_ld, res_ld = c.Ci + c.pad[0], c.Co + c.pad[1], c.Co + c.pad[2]
    if "inplace" in c.epi:
        assert out_ld == res_ld, c
    return in_ld, out_ld, res_ld


def route_of(L, c):
    in_ld, out_ld, _ = lds(c)
    return L.hupr_debug_halo_route(c.B, c.D, c.H, c.W, c.Ci, in_ld, c.Co, out_ld, c.kd, int(c.act != "f32"), int(c.act == "stats"),
                                   int(c.act == "ws"))


def items(B):
    return sorted({0, 1, B // 2, B - 1}) if B > 4 else list(range(B))


# ---- the fp64 reference and the gate (CPU) -----------------------------------------------------------------------------
def conv_ref(x, w, bias, res, kd):
    """fp64 convolution of channels-last x [n, D, H, W, Ci] with w [Co, Ci, kd, 3, 3] (+ bias [Co]) (+ res [n, D, H, W, Co]), all
    given as the exact values the kernel reads; returns (ref, A) channels-last, A over absolute values."""
    xd = x.double().permute(0, 4, 1, 2, 3)
    wd = w.double()
    pad = (kd // 2, 1, 1)
    ref = F.conv3d(xd, wd, None, 1, pad).permute(0, 2, 3, 4, 1)
    A = F.conv3d(xd.abs(), wd.abs(), None, 1, pad).permute(0, 2, 3, 4, 1)
    if bias is not None:
        ref = ref + bias.double()
        A = A + bias.double().abs()
    if res is not None:
        ref = ref + res.double()
        A = A + res.double().abs()
    return ref, A


def bound(ref, A, bf16_store):
    return (2.0 ** -8 * ref.abs() if bf16_store else 0.0) + 2.0 ** -16 * A


def within_bound(y, ref, A, bf16_store):
    """True where y meets the gate (a NaN never does)."""
    return (y.double() - ref).abs() <= bound(ref, A, bf16_store)


def assert_within(y, ref, A, bf16_store, what):
    ok = within_bound(y, ref, A, bf16_store)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        err = ((y.double() - ref).abs() / bound(ref, A, bf16_store)).nan_to_num(float("inf"))
        raise AssertionError("%s: %d of %d outside the bound, first at %s (y %r, ref %r), worst err / bound %.3g"
                             % (what, bad.shape[0], ok.numel(), tuple(bad[0].tolist()), y[tuple(bad[0])].item(),
                                ref[tuple(bad[0])].item(), err.max().item()))


# ---- operands and NaN-padded buffers (GPU) --------------------------------------------------------------------------------
NAN16, NAN32 = 0x7FC1, 0x7FC00001          # quiet NaNs with a payload no arithmetic produces


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def nan_buffer(n, dtype):
    if dtype == torch.bfloat16:
        return torch.full((n,), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full((n,), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)


def padded(vals, ld, dtype):
    """[B, D, H, W, C] values -> a [B, D, H, W, ld] buffer of dtype whose columns >= C hold NaN (+ a NaN guard tail)."""
    *lead, C = vals.shape
    n = int(np.prod(lead)) * ld
    buf = nan_buffer(n + GUARD, dtype)
    buf[:n].view(*lead, ld)[..., :C] = vals.to("cuda", dtype)
    return buf


GUARD = 256


def view(buf, c, ld):
    return buf[:c.B * c.D * c.H * c.W * ld].view(c.B, c.D, c.H, c.W, ld)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def assert_padding_untouched(buf, c, ld):
    nan = NAN16 if buf.dtype == torch.bfloat16 else NAN32
    v = view(buf, c, ld)
    assert bool((bits(v[..., c.Co:].contiguous()) == nan).all()), "a padding column of the output was written"
    assert bool((bits(buf[-GUARD:]) == nan).all()), "the guard tail past the output was written"


def operands(c, seed):
    """The operands of a case, as the exact values the kernel reads: x bf16-representable, packed weights bf16-rounded, bias fp32,
    residual in the storage type."""
    from hupr_amd import functional as F_
    dt = torch.float32 if c.act == "f32" else torch.bfloat16
    x = rnd(c.B, c.D, c.H, c.W, c.Ci, seed=seed).to(torch.bfloat16).float()
    w = rnd(c.Co, c.Ci, c.kd, 3, 3, seed=seed + 1, scale=(c.Ci * 9 * c.kd) ** -0.5)
    wq = w.to(torch.bfloat16).float()
    wp = F_.pack_weights_bf16(w.cuda(), 0)
    bias = rnd(c.Co, seed=seed + 2).cuda() if "bias" in c.epi else None
    res = None
    if "res" in c.epi or "inplace" in c.epi:
        res = rnd(c.B, c.D, c.H, c.W, c.Co, seed=seed + 3)
        res = res.to(torch.bfloat16).float() if dt == torch.bfloat16 else res
    return dt, x, wq, wp, bias, res


def launch(c, dt, x, wp, bias, res, inplace=None, stats=None, part=None):
    """One call of the case's entry on NaN-padded buffers; returns (rc, output buffer, fused statistics or None)."""
    from hupr_amd import functional as F_
    L, rt = F_.rt.lib(), F_.rt
    in_ld, out_ld, res_ld = lds(c)
    inplace = "inplace" in c.epi if inplace is None else inplace
    xb = padded(x, in_ld, dt)
    rb = padded(res, res_ld, dt) if res is not None else None
    yb = rb if inplace else nan_buffer(c.B * c.D * c.H * c.W * out_ld + GUARD, dt)
    args = (c.B, c.D, c.H, c.W, c.Ci, in_ld, c.Co, out_ld)
    bp, rp = rt.ptr(bias) if bias is not None else None, rt.ptr(rb) if rb is not None else None
    st = None
    if c.act == "stats":
        st = torch.full((L.hupr_conv3x3_halo_stats_rows(), 2, c.Co), float("nan"), dtype=torch.float64, device="cuda")
        rc = L.hupr_conv3x3_halo_bf16act_stats(rt.ptr(xb), rt.ptr(wp), rt.ptr(yb), *args, c.kd, rt.ptr(st), rt.stream())
    elif c.act == "ws":
        nws = L.hupr_conv3x3_halo_splitk_ws_bytes(c.B, c.D, c.H, c.W, c.Ci, c.Co, c.kd)
        assert nws > 0
        ws = torch.empty(nws // 4, dtype=torch.float32, device="cuda")
        rc = L.hupr_conv3x3_halo_bf16act_ws(rt.ptr(xb), rt.ptr(wp), bp, rp, rt.ptr(yb), *args, res_ld, c.kd, rt.ptr(ws), nws,
                                            rt.stream())
    else:
        fn = L.hupr_conv3x3_halo_bf16act if dt == torch.bfloat16 else L.hupr_conv3x3_halo_bf16
        rc = fn(rt.ptr(xb), rt.ptr(wp), bp, rp, rt.ptr(yb), *args, res_ld, c.kd, rt.stream())
    torch.cuda.synchronize()
    return rc, yb, st


@pytest.fixture
def lib():
    from hupr_amd import functional as F_
    L = F_.rt.lib()
    yield L
    L.hupr_debug_halo_res_prefetch(1)


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_halo_conv_form_matches_fp64(c, lib):
    """The routed instantiation against fp64, element by element on items {0, 1, B/2, B-1}; padding and guard untouched; the
    same bits from a second launch; fused statistics against the exact sums of the stored outputs."""
    assert route_of(lib, c) == c.route, (route_of(lib, c), c.route)
    dt, x, wq, wp, bias, res = operands(c, seed=c.B * 131 + c.Ci + c.Co)
    _, out_ld, _ = lds(c)
    rc, yb, st = launch(c, dt, x, wp, bias, res)
    assert rc == 0, lib.hupr_last_error()
    assert_padding_untouched(yb, c, out_ld)
    y = view(yb, c, out_ld)[..., :c.Co].cpu()
    sel = items(c.B)
    ref, A = conv_ref(x[sel], wq, bias.cpu() if bias is not None else None, res[sel] if res is not None else None, c.kd)
    assert_within(y[sel], ref, A, dt == torch.bfloat16, "%s (route %d)" % (case_id(c), c.route))
    rc2, yb2, st2 = launch(c, dt, x, wp, bias, res)
    assert rc2 == 0 and torch.equal(bits(view(yb2, c, out_ld)[..., :c.Co].cpu()), bits(y)), "two launches differ"
    if st is not None:
        tot = st.sum(0).cpu()                   # [2][Co]: column sums and sums of squares over the workgroups' rows
        yd = y.double().reshape(-1, c.Co)
        s, q = yd.sum(0), (yd * yd).sum(0)
        assert bool(((tot[0] - s).abs() <= 2.0 ** -20 * yd.abs().sum(0)).all()), "fused column sums"
        assert bool(((tot[1] - q).abs() <= 2.0 ** -20 * q).all()), "fused sums of squares"
        assert torch.equal(st, st2)


EQ_CASES = [c for c in CASES if c.route in (T4X8X8, CI32) and c.pad[1] % 8 == 0 and c.act == "bf16"]


@pytest.mark.parametrize("c", EQ_CASES, ids=[case_id(c) for c in EQ_CASES])
def test_deferred_and_immediate_epilogues_store_the_same_bits(c, lib):
    """The 256-voxel kernel's deferred epilogue (parked tile, residual prefetched under the last stage, bias added in front of the
    rounding) and its immediate one — forced by out_ld % 8 != 0 and, with a residual, by hupr_debug_halo_res_prefetch(0) — round the
    same fp32 sums once: identical bits; in place (out is res) as out of place."""
    dt, x, wq, wp, bias, res = operands(c, seed=c.B * 131 + c.Ci + c.Co)
    _, out_ld, _ = lds(c)
    rc, yb, _ = launch(c, dt, x, wp, bias, res)
    assert rc == 0
    y = bits(view(yb, c, out_ld)[..., :c.Co].cpu())
    imm = c._replace(pad=(c.pad[0], 4, 4 if "inplace" in c.epi else c.pad[2]))
    assert route_of(lib, imm) == c.route
    rc, yb4, _ = launch(imm, dt, x, wp, bias, res)
    assert rc == 0
    assert_padding_untouched(yb4, imm, imm.Co + 4)
    assert torch.equal(bits(view(yb4, imm, imm.Co + 4)[..., :c.Co].cpu()), y), "out_ld = Co + 4 (immediate epilogue)"
    if res is not None:
        lib.hupr_debug_halo_res_prefetch(0)
        try:
            rc, ybn, _ = launch(c, dt, x, wp, bias, res)
        finally:
            lib.hupr_debug_halo_res_prefetch(1)
        assert rc == 0 and torch.equal(bits(view(ybn, c, out_ld)[..., :c.Co].cpu()), y), "residual read in the immediate epilogue"
        other = c._replace(pad=(c.pad[0], c.pad[2], c.pad[2]))            # the other placement: out of place <-> in place
        rc, ybo, _ = launch(other, dt, x, wp, bias, res, inplace="inplace" not in c.epi)
        assert rc == 0 and torch.equal(bits(view(ybo, other, other.Co + other.pad[1])[..., :c.Co].cpu()), y), "in place vs out of place"


def test_k_sliced_partial_sums_match_fp64(lib):
    """hupr_conv3x3_halo_bf16act_partial: the fp32 partial sums of the K-sliced form, summed over the slices, against fp64
    (the fp32 gate); nothing past the slices is written."""
    from hupr_amd import functional as F_
    rt = F_.rt
    c = [c for c in CASES if c.act == "ws"][0]
    dt, x, wq, wp, _, _ = operands(c, seed=7)
    in_ld, _, _ = lds(c)
    nws = lib.hupr_conv3x3_halo_splitk_ws_bytes(c.B, c.D, c.H, c.W, c.Ci, c.Co, c.kd)
    M = c.B * c.D * c.H * c.W
    slices = nws // (M * c.Co * 4)
    assert slices == (c.route - 256) // 16 and slices * M * c.Co * 4 == nws
    part = nan_buffer(nws // 4 + GUARD, torch.float32)
    xb = padded(x, in_ld, dt)
    rc = lib.hupr_conv3x3_halo_bf16act_partial(rt.ptr(xb), rt.ptr(wp), c.B, c.D, c.H, c.W, c.Ci, in_ld, c.Co, c.kd, rt.ptr(part),
                                               nws, rt.stream())
    assert rc == 0, lib.hupr_last_error()
    assert bool((bits(part[-GUARD:]) == NAN32).all())
    got = part[:nws // 4].view(slices, c.B, c.D, c.H, c.W, c.Co).double().sum(0).cpu()
    ref, A = conv_ref(x, wq, None, None, c.kd)
    assert_within(got, ref, A, False, "K-sliced partial sums")


REFUSED = [  # (what, B, Ci, Co, D, H, W, kd, in_ld, out_ld, res_ld, has_res, stats)
    ("Co % 4 != 0", 2, 64, 62, 4, 16, 16, 3, 64, 64, 64, False, False),
    ("bf16 in_ld % 8 != 0", 2, 64, 64, 4, 16, 16, 3, 68, 64, 64, False, False),
    ("out_ld % 4 != 0", 2, 64, 64, 4, 16, 16, 3, 64, 66, 64, False, False),
    ("res_ld % 4 != 0", 2, 64, 64, 4, 16, 16, 3, 64, 64, 66, True, False),
    ("H % 8 != 0", 2, 64, 64, 4, 12, 16, 3, 64, 64, 64, False, False),
    ("odd depth", 2, 64, 64, 3, 16, 16, 3, 64, 64, 64, False, False),
    ("Ci % 32 != 0", 2, 48, 64, 4, 16, 16, 3, 48, 64, 64, False, False),
    ("statistics on 32 input channels", 16, 32, 64, 4, 32, 32, 3, 32, 64, 64, False, True),
    ("statistics on three output tiles", 16, 64, 192, 4, 32, 32, 3, 64, 192, 192, False, True),
    ("statistics below 256 tiles", 2, 64, 64, 4, 16, 16, 3, 64, 64, 64, False, True),
]


@pytest.mark.parametrize("r", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_calls_leave_the_output_untouched(r, lib):
    """Calls the launcher refuses return HUPR_ERR_ARG before any launch: y keeps its NaN fill bit for bit.  (Statistics together with
    a bias or a residual cannot be asked for: the _stats entry has neither argument.)"""
    from hupr_amd import functional as F_
    rt = F_.rt
    what, B, Ci, Co, D, H, W, kd, in_ld, out_ld, res_ld, has_res, stats = r
    x = nan_buffer(B * D * H * W * in_ld, torch.bfloat16).zero_()
    wp = torch.zeros(Co * Ci * 9 * kd, dtype=torch.bfloat16, device="cuda")
    res = torch.zeros(B * D * H * W * res_ld, dtype=torch.bfloat16, device="cuda") if has_res else None
    y = nan_buffer(B * D * H * W * max(out_ld, Co) + GUARD, torch.bfloat16)
    if stats:
        st = torch.full((lib.hupr_conv3x3_halo_stats_rows(), 2, Co), float("nan"), dtype=torch.float64, device="cuda")
        rc = lib.hupr_conv3x3_halo_bf16act_stats(rt.ptr(x), rt.ptr(wp), rt.ptr(y), B, D, H, W, Ci, in_ld, Co, out_ld, kd, rt.ptr(st),
                                                 rt.stream())
        torch.cuda.synchronize()
        assert bool(st.isnan().all())
    else:
        rc = lib.hupr_conv3x3_halo_bf16act(rt.ptr(x), rt.ptr(wp), None, rt.ptr(res) if has_res else None, rt.ptr(y), B, D, H, W, Ci,
                                           in_ld, Co, out_ld, res_ld, kd, rt.stream())
        torch.cuda.synchronize()
    assert rc == HUPR_ERR_ARG, (what, rc)
    assert bool((bits(y) == NAN16).all()), what


# ---- autograd at shapes where the 256-voxel kernel engages ---------------------------------------------------------------
@pytest.mark.parametrize("Ci,with_bias", [(64, False), (32, True)])
def test_conv_autograd_at_256_voxel_shapes_matches_fp64(Ci, with_bias, lib):
    """ConvFn at a level-1 shape (B = 4, Ci -> 64, 8 x 64 x 64): the forward (4 x 8 x 8 / Ci = 32 tile), the input gradient — mode-1
    packed weights through the 4 x 8 x 8 (Ci = 64) or the 8 x 8 x 8 Co = 32 form (Ci = 32) — against fp64 autograd on the same bf16
    operands under the bf16 gate; weight (and bias) gradient within 1e-5 of the largest entry."""
    from hupr_amd import functional as F_
    B, Co, D, H, W = 4, 64, 8, 64, 64
    fwd = Case(B, Ci, Co, D, H, W, 3, "bf16", "bias" if with_bias else "", P, CI32 if Ci == 32 else T4X8X8)
    bwd = Case(B, Co, Ci, D, H, W, 3, "bf16", "", P, CO32 if Ci == 32 else T4X8X8)
    assert route_of(lib, fwd) == fwd.route and route_of(lib, bwd) == bwd.route
    x = rnd(B, D, H, W, Ci, seed=300 + Ci).to(torch.bfloat16)
    w = rnd(Co, Ci, 3, 3, 3, seed=301, scale=(Ci * 27) ** -0.5)
    b = rnd(Co, seed=302) if with_bias else None
    gy = rnd(B, D, H, W, Co, seed=303).to(torch.bfloat16)
    F_.set_math("bf16")
    try:
        xg = x.cuda().requires_grad_(True)
        wg = w.cuda().requires_grad_(True)
        bg = b.cuda().requires_grad_(True) if with_bias else None
        y = F_.conv(xg, wg, bg, None, (1, 1, 1))
        y.backward(gy.cuda())
    finally:
        F_.set_math("f32")
    wq = w.to(torch.bfloat16).double()
    xr = x.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    wr = wq.clone().requires_grad_(True)
    br = b.double().requires_grad_(True) if with_bias else None
    yr = F.conv3d(xr, wr, br, 1, 1)
    yr.backward(gy.double().permute(0, 4, 1, 2, 3))
    A = F.conv3d(xr.detach().abs(), wq.abs(), br.detach().abs() if with_bias else None, 1, 1)
    xa = xr.detach().abs().requires_grad_(True)
    F.conv3d(xa, wq.abs(), None, 1, 1).backward(gy.double().abs().permute(0, 4, 1, 2, 3))
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    assert_within(y.detach().float().cpu(), cl(yr.detach()), cl(A), True, "ConvFn forward")
    assert xg.grad.dtype == torch.bfloat16
    assert_within(xg.grad.float().cpu(), cl(xr.grad), cl(xa.grad), True, "ConvFn input gradient")
    scale = wr.grad.abs().max().item()
    assert (wg.grad.cpu().double() - wr.grad).abs().max().item() <= 1e-5 * scale, "ConvFn weight gradient"
    if with_bias:
        assert (bg.grad.cpu().double() - br.grad).abs().max().item() <= 1e-5 * br.grad.abs().max().item(), "ConvFn bias gradient"


def test_dual_conv_input_gradient_in_place_matches_fp64(lib):
    """DualConvFn: the second input gradient is added in place into the first (its residual epilogue, out is res) — against fp64:
    the first one is rounded to bf16 on its way through memory, so its own bf16 step joins the gate."""
    from hupr_amd import functional as F_
    B, C, D, H, W = 4, 64, 8, 32, 64
    bwd = Case(B, C, C, D, H, W, 3, "bf16", "inplace", P, T4X8X8)
    assert route_of(lib, bwd) == T4X8X8
    x = rnd(B, D, H, W, C, seed=310).to(torch.bfloat16)
    wa, wb = (rnd(C, C, 3, 3, 3, seed=311 + i, scale=(C * 27) ** -0.5) for i in range(2))
    ga, gb = (rnd(B, D, H, W, C, seed=313 + i).to(torch.bfloat16) for i in range(2))
    F_.set_math("bf16")
    try:
        xg = x.cuda().requires_grad_(True)
        ya, yb = F_.DualConvFn.apply(xg, wa.cuda().requires_grad_(True), wb.cuda().requires_grad_(True), (1, 1, 1))
        torch.autograd.backward([ya, yb], [ga.cuda(), gb.cuda()])
    finally:
        F_.set_math("f32")
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    refs = []
    for w, g in ((wa, ga), (wb, gb)):
        wq = w.to(torch.bfloat16).double()
        xr = x.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
        F.conv3d(xr, wq, None, 1, 1).backward(g.double().permute(0, 4, 1, 2, 3))
        xa = xr.detach().abs().requires_grad_(True)
        F.conv3d(xa, wq.abs(), None, 1, 1).backward(g.double().abs().permute(0, 4, 1, 2, 3))
        refs.append((cl(xr.grad), cl(xa.grad)))
    (ra, Aa), (rb, Ab) = refs
    ref = ra + rb
    got = xg.grad.float().cpu().double()
    lim = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * (1 + 2.0 ** -7) * ra.abs() + 2.0 ** -16 * (Aa + Ab)
    ok = (got - ref).abs() <= lim
    assert bool(ok.all()), "DualConvFn input gradient: %d outside, worst err / bound %.3g" % (
        (~ok).sum().item(), ((got - ref).abs() / lim).max().item())
