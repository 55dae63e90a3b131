"""GPU (-m gpu): every form of the halo-tiled weight gradient (hupr_conv3x3_wgrad_halo_bf16 / _bf16act / _bf16act_dual,
csrc/wgrad_halo_bf16.hip) against an fp64 reference of exactly the operands the kernel sees, element by element, with the route
and the partial-tensor count of every launch asserted first (hupr_debug_wgrad_route): the three instantiations of the
16 x 16 x 32 LDS-DMA kernel, the four of the 32 x 32 x 16 one, the four of the register-staged one; the 3-D and the XCD-aware grid;
padded rows (in_ld != Ci, dy_ld != Co); workspace-limited plans; two gradients in one launch; refused calls.

Reference: dw[:, :, a, b, c] = dy_flat.T @ x_shift_flat over the 9 kd shifted views of the zero-padded x, in fp64; A the same over
absolute values.  fp32-stored operands are NOT bf16-representable: the reference rounds them to nearest even, as the kernel must.

Gate (``within``): |dw - ref| <= GATE_C * A per element.  The bf16 x bf16 products are exact in fp32 and the output is fp32: only the
fp32 summation order is free, so there is no relative term.  GATE_C is the smallest power of two that is at least 8 x the worst
err / A measured over this table against fp64 on an MI355X (never above 2^-16, the gate of the fp32-output forward convolution);
the 8 x is room for legitimate changes of slice and group counts.  Measured worst err / A per route (route code & 15, see
include/hupr_debug.h), single and dual launches, 16 x 16 x 32 kernel on both grids:

    route                                   3-D grid   XCD grid   dual launch
     1 hupr_k_wgrad_halo_m16<true>            2^-22.9    2^-25.4    2^-24.2
     2 hupr_k_wgrad_halo_m16<false>           2^-23.5    2^-27.0    2^-25.3
     3 hupr_k_wgrad_halo_m16<true, true>      2^-25.9    2^-28.0    2^-28.0
     4 hupr_k_wgrad_halo_glds<false, false>   2^-25.3
     5 hupr_k_wgrad_halo_glds<false, true>    2^-25.9    2^-27.6
     6 hupr_k_wgrad_halo_glds<true, false>    2^-24.8
     7 hupr_k_wgrad_halo_glds<true, true>     2^-25.7
     8 hupr_k_wgrad_halo_bf16<false, false>   2^-24.5
     9 hupr_k_wgrad_halo_bf16<false, true>    2^-23.4
    10 hupr_k_wgrad_halo_bf16<true, false>    2^-23.8
    11 hupr_k_wgrad_halo_bf16<true, true>     2^-23.2

Worst of all: 2^-22.94 (1.24e-7; the short sums of the one- and two-tile cases, where the fp32 rounding of the result itself is
2^-24 of it); 8 x that is 2^-19.94, hence GATE_C = 2^-19.

Every x / dy buffer holds payload NaNs in its padding columns and its guard tail; dw is a view at a 12-byte offset inside a
NaN-pattern buffer and the workspace has exactly the byte count the case names, both followed (dw: also preceded) by NaN-pattern
guards that must come back bit-identical.  A second launch into a fresh dw must give the same bits (the split-K reduction is
deterministic).  tests/test_wgrad_halo_route.py checks the routes of this table, and that the gate rejects faulty sums, without a
GPU.

Register-staged bf16 kernel at in_ld = 2^23 (a 2 GiB x): its offsets are 32-bit element offsets (((b D + d) H + h) W + w) in_ld + c.
At the 128-voxel shapes used here a load that is kept has voxel index <= 127: offset <= 127 * 2^23 + 63 < 2^30.  A masked halo load
computes d <= D, h <= H, w <= W, voxel index <= 200 (3-D) / 144 (2-D): 200 * 2^23 < 2^31, no wrap, and its offset is replaced by 0
before the load."""
import collections
import ctypes
import functools

import pytest
import torch

from test_conv_halo_fp64_gpu import GUARD, NAN32, bits, nan_buffer, padded, rnd

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG, HUPR_ERR_WORKSPACE = -1, -2
GATE_C = 2.0 ** -19

# route codes of hupr_debug_wgrad_route (include/hupr_debug.h)
M16_3D, M16_2D, M16_KQ = 1, 2, 3                    # hupr_k_wgrad_halo_m16<true> / <false> / <true, true> (K quarters)
GLDS_2D, GLDS_2D_KQ, GLDS_3D, GLDS_3D_KQ = 4, 5, 6, 7    # hupr_k_wgrad_halo_glds<IS3D, CI32> (the 32 x 32 x 16 kernel)
REG_F32_2D, REG_F32_3D, REG_BF16_2D, REG_BF16_3D = 8, 9, 10, 11      # hupr_k_wgrad_halo_bf16<ABF, IS3D> (register-staged)
XCD, DUAL = 16, 32
ROUTE_NAMES = {1: "m16<true>", 2: "m16<false>", 3: "m16<true,true>", 4: "glds<false,false>", 5: "glds<false,true>",
               6: "glds<true,false>", 7: "glds<true,true>", 8: "bf16<false,false>", 9: "bf16<false,true>", 10: "bf16<true,false>",
               11: "bf16<true,true>"}

# act: "bf16" hupr_conv3x3_wgrad_halo_bf16act, "f32" hupr_conv3x3_wgrad_halo_bf16 (fp32-stored activations).  pad: (in_ld - Ci,
# dy_ld - Co).  ws: "full" = hupr_conv3x3_wgrad_halo_ws_bytes (twice that for a dual launch), "one" / an int n = exactly one / n
# partial tensors.  mode: None or (hupr_debug_wgrad_m16, hupr_debug_wgrad_ci32) settings.  route, groups: what
# hupr_debug_wgrad_route answers.
Case = collections.namedtuple("Case", "B Ci Co D H W kd act pad ws mode route groups")
P, P8, PX = (0, 0), (8, 8), (24, 40)                # dense; padded; padded, in_ld != dy_ld, neither a multiple of 64
F4 = (4, 12)                                        # fp32 storage: leading dimensions stay multiples of 4
BIG = 1 << 23                                       # in_ld of the register-staged bf16 cases: 128 voxels x 2^23 x 2 B = 2 GiB


def C(shape, route, groups, act="bf16", pad=P, ws="full", mode=None):
    return Case(*shape, act, pad, ws, mode, route, groups)


CASES = [
    # ---- m16<true>, 3-D grid: one tile and one group (all 27 taps see only borders) ... 192 pairs, one group walking two tiles
    C((1, 64, 64, 2, 8, 8, 3), M16_3D, 1),
    C((1, 64, 64, 2, 8, 8, 3), M16_3D, 1, pad=P8),
    C((2, 64, 64, 4, 8, 8, 3), M16_3D, 4),
    C((2, 128, 128, 2, 16, 16, 3), M16_3D, 8),
    C((2, 256, 256, 2, 8, 16, 3), M16_3D, 4),
    C((3, 96, 72, 4, 8, 16, 3), M16_3D, 12),
    C((3, 96, 72, 4, 8, 16, 3), M16_3D, 12, pad=P8),
    C((3, 96, 72, 4, 8, 16, 3), M16_3D, 12, pad=PX),
    C((2, 72, 136, 2, 16, 16, 3), M16_3D, 8),
    C((2, 72, 136, 2, 16, 16, 3), M16_3D, 8, pad=PX),
    C((3, 8, 8, 2, 8, 8, 3), M16_3D, 3),
    C((3, 8, 8, 2, 8, 8, 3), M16_3D, 3, pad=P8),
    C((2, 512, 512, 2, 8, 8, 3), M16_3D, 1),
    # ---- m16<true>, XCD grid: n_spatial = 80 = gw; 132 tiles over 80 groups; 6 members per group; Ci = 32 below the K-quarter threshold
    C((5, 64, 64, 4, 16, 32, 3), M16_3D + XCD, 80),
    C((5, 64, 64, 4, 16, 32, 3), M16_3D + XCD, 80, pad=PX),
    C((33, 64, 64, 2, 16, 16, 3), M16_3D + XCD, 80),
    C((5, 96, 64, 4, 16, 16, 3), M16_3D + XCD, 40),
    C((5, 96, 64, 4, 16, 16, 3), M16_3D + XCD, 40, pad=P8),
    C((9, 32, 64, 4, 32, 32, 3), M16_3D + XCD, 80),
    # ---- m16<false>
    C((2, 320, 64, 1, 16, 32, 1), M16_2D, 8),
    C((2, 320, 64, 1, 16, 32, 1), M16_2D, 8, pad=P8),
    C((3, 64, 192, 1, 16, 32, 1), M16_2D, 12),
    C((7, 128, 64, 1, 16, 48, 1), M16_2D, 42),
    C((1, 320, 320, 1, 8, 16, 1), M16_2D, 1),
    C((2, 24, 40, 1, 16, 32, 1), M16_2D, 8),
    C((2, 24, 40, 1, 16, 32, 1), M16_2D, 8, pad=PX),
    C((18, 32, 64, 1, 64, 64, 1), M16_2D + XCD, 128),          # 4.5 tiles per group
    C((18, 32, 64, 1, 64, 64, 1), M16_2D + XCD, 128, pad=P8),
    # ---- m16<true, true> by default (n_spatial >= 16 gw): XCD grid, 16 tiles per group; 3-D grid; the same layer just under the threshold
    C((5, 32, 64, 8, 64, 64, 3), M16_KQ + XCD, 80),
    C((5, 32, 64, 8, 64, 64, 3), M16_KQ + XCD, 80, pad=PX),
    C((5, 24, 512, 4, 32, 32, 3), M16_KQ, 10),
    C((5, 24, 512, 4, 32, 32, 3), M16_KQ, 10, pad=P8),
    C((3, 32, 512, 4, 32, 32, 3), M16_3D, 10),
    # ---- glds<false, true> by default (1 x 3 x 3 taps, Ci <= 32, n_spatial >= 16 gw) and just under the threshold
    C((8, 16, 512, 1, 64, 128, 1), GLDS_2D_KQ + XCD, 32),
    C((8, 16, 512, 1, 64, 128, 1), GLDS_2D_KQ + XCD, 32, pad=PX),
    C((4, 32, 512, 1, 64, 128, 1), M16_2D + XCD, 32),
    # ---- the remaining forms of the 32 x 32 x 16 kernel and forced K quarters at small shapes (debug settings)
    C((2, 64, 64, 4, 8, 8, 3), GLDS_3D, 4, mode=(0, 1)),
    C((2, 64, 64, 4, 8, 8, 3), GLDS_3D, 4, mode=(0, 1), pad=P8),
    C((2, 320, 64, 1, 16, 32, 1), GLDS_2D, 8, mode=(0, 1)),
    C((2, 320, 64, 1, 16, 32, 1), GLDS_2D, 8, mode=(0, 1), pad=PX),
    C((3, 32, 72, 4, 8, 24, 3), GLDS_3D, 18, mode=(0, 0)),
    C((3, 32, 72, 4, 8, 24, 3), GLDS_3D_KQ, 18, mode=(1, 3)),
    C((3, 32, 72, 4, 8, 24, 3), GLDS_3D_KQ, 18, mode=(0, 2), pad=PX),
    C((3, 32, 72, 4, 8, 24, 3), M16_KQ, 18, mode=(1, 2)),
    C((3, 32, 72, 4, 8, 24, 3), M16_KQ, 18, mode=(1, 2), pad=P8),
    C((3, 32, 72, 4, 8, 24, 3), M16_3D, 18, mode=(1, 0)),
    C((2, 24, 40, 1, 16, 32, 1), GLDS_2D_KQ, 8, mode=(1, 2)),
    C((2, 24, 40, 1, 16, 32, 1), GLDS_2D_KQ, 8, mode=(0, 3), pad=P8),
    C((2, 24, 40, 1, 16, 32, 1), GLDS_2D, 8, mode=(0, 0)),
    # ---- fp32 storage: bf16<false, *>; 256 partial tensors on 2-D maps, 128 under hupr_debug_wgrad_ci32(16 + mode)
    C((2, 64, 64, 4, 8, 8, 3), REG_F32_3D, 4, act="f32"),
    C((2, 64, 64, 4, 8, 8, 3), REG_F32_3D, 4, act="f32", pad=F4),
    C((3, 96, 72, 2, 8, 16, 3), REG_F32_3D, 6, act="f32"),
    C((3, 96, 72, 2, 8, 16, 3), REG_F32_3D, 6, act="f32", pad=F4),
    C((2, 320, 64, 1, 16, 32, 1), REG_F32_2D, 8, act="f32"),
    C((2, 320, 64, 1, 16, 32, 1), REG_F32_2D, 8, act="f32", pad=F4),
    C((2, 32, 40, 1, 8, 16, 1), REG_F32_2D, 2, act="f32"),
    C((2, 32, 40, 1, 8, 16, 1), REG_F32_2D, 2, act="f32", pad=F4),
    C((8, 32, 40, 1, 64, 64, 1), REG_F32_2D, 256, act="f32"),
    C((8, 32, 40, 1, 64, 64, 1), REG_F32_2D, 128, act="f32", mode=(1, 17)),
    # ---- workspace-limited plans: gw halved until it fits, the XCD grid dropped, one workgroup walking every tile
    C((5, 64, 64, 4, 16, 32, 3), M16_3D, 1, ws="one"),
    C((5, 64, 64, 4, 16, 32, 3), M16_3D, 2, ws=3),
    C((5, 64, 64, 4, 16, 32, 3), M16_3D, 20, ws=20),
    C((2, 64, 64, 4, 8, 8, 3), REG_F32_3D, 1, act="f32", ws="one"),
    C((2, 64, 64, 4, 8, 8, 3), REG_F32_3D, 2, act="f32", ws=3),
    # ---- register-staged bf16 (a tensor of 2 GiB): bf16<true, true> and <true, false>
    C((1, 64, 64, 2, 8, 8, 3), REG_BF16_3D, 1, pad=(BIG - 64, 0)),
    C((1, 64, 64, 1, 8, 16, 1), REG_BF16_2D, 1, pad=(BIG - 64, 0)),
]

# two gradients in one launch (hupr_conv3x3_wgrad_halo_bf16act_dual); ws "full" = 2 x hupr_conv3x3_wgrad_halo_ws_bytes
DUAL_CASES = [
    C((2, 64, 64, 4, 8, 8, 3), M16_3D + DUAL, 4),
    C((3, 96, 64, 2, 8, 8, 3), M16_3D + DUAL, 3),
    C((3, 96, 64, 2, 8, 8, 3), M16_3D + DUAL, 3, pad=PX),
    C((2, 128, 128, 2, 16, 16, 3), M16_3D + DUAL, 8),
    C((2, 64, 64, 1, 16, 32, 1), M16_2D + DUAL, 8),
    C((5, 64, 64, 4, 16, 32, 3), M16_3D + XCD + DUAL, 80),
    C((5, 32, 64, 8, 64, 64, 3), M16_KQ + XCD + DUAL, 80),
    C((5, 32, 64, 8, 64, 64, 3), M16_KQ + XCD + DUAL, 80, pad=P8),
]


def case_id(c):
    ws = c.ws if isinstance(c.ws, str) else "%dparts" % c.ws
    pad = "big.0" if c.pad[0] >= BIG // 2 else "%d.%d" % c.pad
    mode = "" if c.mode is None else "-m16.%d-ci32.%d" % c.mode
    return "%s-B%d-%dto%d-%dx%dx%d-k%d-ld%s-ws%s%s" % (c.act, c.B, c.Ci, c.Co, c.D, c.H, c.W, c.kd, pad, ws, mode)


def lds(c):
    return c.Ci + c.pad[0], c.Co + c.pad[1]


def ws_bytes_of(L, c, dual=False):
    nt = 2 if dual else 1
    if c.ws == "full":
        return nt * L.hupr_conv3x3_wgrad_halo_ws_bytes(c.Ci, c.Co, c.kd)
    return (1 if c.ws == "one" else c.ws) * nt * c.Co * c.kd * 9 * c.Ci * 4


class Modes:
    """The debug settings of a case, restored to the defaults on exit."""

    def __init__(self, L, mode):
        self.L, self.mode = L, mode

    def __enter__(self):
        if self.mode is not None:
            self.L.hupr_debug_wgrad_m16(self.mode[0])
            self.L.hupr_debug_wgrad_ci32(self.mode[1])

    def __exit__(self, *exc):
        self.L.hupr_debug_wgrad_m16(1)
        self.L.hupr_debug_wgrad_ci32(1)


def route_of(L, c, dual=False, ws_bytes=None):
    """(route code or HUPR_ERR_*, partial-tensor count) of the case under its debug settings."""
    in_ld, dy_ld = lds(c)
    g = ctypes.c_int(-1)
    with Modes(L, c.mode):
        r = L.hupr_debug_wgrad_route(c.B, c.D, c.H, c.W, c.Ci, in_ld, c.Co, dy_ld, c.kd, int(c.act != "f32"), int(dual),
                                     ws_bytes_of(L, c, dual) if ws_bytes is None else ws_bytes, ctypes.byref(g))
    return r, g.value


# ---- the fp64 reference and the gate (any device) ----------------------------------------------------------------------------
def zero_padded(x, kd):
    """[B, D, H, W, C] -> [B, D + kd - 1, H + 2, W + 2, C] in fp64 with the convolution's zero border."""
    pd = kd // 2
    B, D, H, W, Ci = x.shape
    xp = torch.zeros(B, D + 2 * pd, H + 2, W + 2, Ci, dtype=torch.float64, device=x.device)
    xp[:, pd:pd + D, 1:H + 1, 1:W + 1] = x.double()
    return xp


def wgrad_ref(x, dy, kd, xp=None):
    """fp64 weight gradient of channels-last x [B, D, H, W, Ci] and dy [B, D, H, W, Co], given as the exact values the kernel
    multiplies: 9 kd matmuls over shifted views of the zero-padded x (xp: that padded tensor, if the caller built it).  Returns
    (ref, A) in parameter layout [Co, Ci, kd, 3, 3]; A over absolute values."""
    B, D, H, W, Ci = x.shape
    Co = dy.shape[-1]
    xp = zero_padded(x, kd) if xp is None else xp
    dyt = dy.double().reshape(-1, Co).t().contiguous()
    dya = dyt.abs()
    ref = torch.empty(Co, Ci, kd, 3, 3, dtype=torch.float64, device=x.device)
    A = torch.empty_like(ref)
    for a in range(kd):
        for b in range(3):
            for c in range(3):
                xs = xp[:, a:a + D, b:b + H, c:c + W].reshape(-1, Ci)
                ref[:, :, a, b, c] = dyt @ xs
                A[:, :, a, b, c] = dya @ xs.abs()
    return ref, A


def within(dw, ref, A, c=None):
    """True where dw meets the gate (a NaN never does)."""
    return (dw.double() - ref).abs() <= (GATE_C if c is None else c) * A


WORST = {}             # route & 15 -> worst err / A seen in this session (printed per case: pytest -s shows the measurements)


def assert_within(dw, ref, A, what, route):
    ok = within(dw, ref, A)
    err = ((dw.double() - ref).abs() / A).nan_to_num(float("inf"))
    worst = err.max().item()
    WORST[route & 15] = max(WORST.get(route & 15, 0.0), worst)
    print("wgrad fp64: %-60s route %2d (%s) worst err / A = %.3g = 2^%.2f" % (
        what, route, ROUTE_NAMES[route & 15], worst, torch.log2(err.max()).item()))
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d outside the gate, first at %s (dw %r, ref %r), worst err / A %.3g (gate %.3g)"
                             % (what, bad.shape[0], ok.numel(), i, dw[i].item(), ref[i].item(), worst, GATE_C))


# ---- operands, NaN-guarded buffers, the launch (GPU) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(shape, act, n_dy=1):
    """Seeded operands of a shape, shared (and left unchanged) by every case on it: x and the dy tensors as stored — bf16, or fp32
    that is NOT bf16-representable — and per dy the fp64 reference over the values the kernel multiplies (rounded to nearest even)."""
    B, Ci, Co, D, H, W, kd = shape
    seed = 1000 * B + 7 * Ci + Co + D + H + W
    dt = torch.float32 if act == "f32" else torch.bfloat16
    x = rnd(B, D, H, W, Ci, seed=seed).cuda().to(dt)
    dys = [rnd(B, D, H, W, Co, seed=seed + 1 + i).cuda().to(dt) for i in range(n_dy)]
    xq = x.bfloat16()
    xp = zero_padded(xq, kd)
    refs = [wgrad_ref(xq, dy.bfloat16(), kd, xp) for dy in dys]
    return dt, x, dys, refs


def dw_buffer(n):
    """A NaN-pattern buffer with dw as a view at a 12-byte offset: guard | 3 floats | dw | guard."""
    buf = nan_buffer(GUARD + 3 + n + GUARD, torch.float32)
    return buf, buf[GUARD + 3:GUARD + 3 + n]


def assert_guards(buf, n, what):
    assert bool((bits(buf[:GUARD + 3]) == NAN32).all()), "%s: the guard in front of dw was written" % what
    assert bool((bits(buf[GUARD + 3 + n:]) == NAN32).all()), "%s: the guard past dw was written" % what


def ws_buffer(nbytes):
    """Exactly nbytes of workspace (NaN pattern, so a partial sum that is read before it is written shows) + a NaN-pattern guard."""
    assert nbytes % 4 == 0
    return nan_buffer(nbytes // 4 + GUARD, torch.float32)


def assert_ws_guard(ws, nbytes):
    assert bool((bits(ws[nbytes // 4:]) == NAN32).all()), "the guard past the workspace was written"


def stored(c, x, dys):
    """x and the dy tensors in [B, D, H, W, ld] buffers whose padding columns and guard tail hold payload NaNs."""
    in_ld, dy_ld = lds(c)
    try:
        return padded(x, in_ld, x.dtype), [padded(dy, dy_ld, dy.dtype) for dy in dys]
    except torch.OutOfMemoryError:
        pytest.skip("the card refused the %.1f GiB allocation of this case" % (x.numel() / c.Ci * in_ld * x.element_size() / 2 ** 30))


def call(L, c, xb, dybs, dws, ws, nbytes):
    from hupr_amd import runtime as rt
    in_ld, dy_ld = lds(c)
    geo = (c.B, c.D, c.H, c.W, c.Ci, in_ld, c.Co, dy_ld, c.kd)
    with Modes(L, c.mode):
        if len(dybs) == 2:
            rc = L.hupr_conv3x3_wgrad_halo_bf16act_dual(rt.ptr(xb), rt.ptr(dybs[0]), rt.ptr(dybs[1]), dws[0].data_ptr(), dws[1].data_ptr(),
                                                        *geo, rt.ptr(ws), nbytes, rt.stream())
        else:
            fn = L.hupr_conv3x3_wgrad_halo_bf16 if c.act == "f32" else L.hupr_conv3x3_wgrad_halo_bf16act
            rc = fn(rt.ptr(xb), rt.ptr(dybs[0]), dws[0].data_ptr(), *geo, rt.ptr(ws), nbytes, rt.stream())
    torch.cuda.synchronize()
    return rc


@pytest.fixture
def lib():
    from hupr_amd import runtime
    L = runtime.lib()
    yield L
    L.hupr_debug_wgrad_m16(1)
    L.hupr_debug_wgrad_ci32(1)


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_wgrad_halo_form_matches_fp64(c, lib):
    """The routed instantiation and grid plan against fp64 under the gate, every element; the guards around dw and past the workspace
    untouched; the same bits from a second launch."""
    assert route_of(lib, c) == (c.route, c.groups)
    dt, x, dys, refs = operands(tuple(c[:7]), c.act)
    xb, dybs = stored(c, x, dys)
    n = c.Co * c.Ci * c.kd * 9
    nbytes = ws_bytes_of(lib, c)
    ws = ws_buffer(nbytes)
    buf, dw = dw_buffer(n)
    rc = call(lib, c, xb, dybs, [dw], ws, nbytes)
    assert rc == 0, lib.hupr_last_error()
    ref, A = refs[0]
    assert_within(dw.view(c.Co, c.Ci, c.kd, 3, 3), ref, A, case_id(c), c.route)
    assert_guards(buf, n, case_id(c))
    assert_ws_guard(ws, nbytes)
    buf2, dw2 = dw_buffer(n)
    assert call(lib, c, xb, dybs, [dw2], ws, nbytes) == 0
    assert torch.equal(bits(dw2), bits(dw)), "two launches differ"
    assert_guards(buf2, n, case_id(c))


@pytest.mark.parametrize("c", DUAL_CASES, ids=[case_id(c) for c in DUAL_CASES])
def test_two_gradients_in_one_launch_match_fp64_and_two_single_calls(c, lib):
    """hupr_conv3x3_wgrad_halo_bf16act_dual on exactly 2 x hupr_conv3x3_wgrad_halo_ws_bytes: each output against fp64 under the gate
    and bit-equal to a single call; guards untouched; a workspace one byte short of two partial tensors is refused."""
    assert route_of(lib, c, dual=True) == (c.route, c.groups)
    assert route_of(lib, c) == (c.route - DUAL, c.groups)
    assert lib.hupr_conv3x3_wgrad_halo_dual_supported(c.B, c.D, c.H, c.W, c.Ci, c.Co, c.kd)
    dt, x, dys, refs = operands(tuple(c[:7]), c.act, 2)
    xb, dybs = stored(c, x, dys)
    n = c.Co * c.Ci * c.kd * 9
    nbytes = ws_bytes_of(lib, c, dual=True)
    assert nbytes == 2 * lib.hupr_conv3x3_wgrad_halo_ws_bytes(c.Ci, c.Co, c.kd)
    ws = ws_buffer(nbytes)
    (bufa, dwa), (bufb, dwb) = dw_buffer(n), dw_buffer(n)
    n0 = lib.hupr_launch_count()
    rc = call(lib, c, xb, dybs, [dwa, dwb], ws, nbytes)
    assert rc == 0, lib.hupr_last_error()
    assert lib.hupr_launch_count() - n0 == 2
    for i, (buf, dw) in enumerate(((bufa, dwa), (bufb, dwb))):
        what = "%s gradient %d" % (case_id(c), i)
        assert_within(dw.view(c.Co, c.Ci, c.kd, 3, 3), *refs[i], what, c.route)
        assert_guards(buf, n, what)
        buf1, dw1 = dw_buffer(n)
        assert call(lib, c, xb, [dybs[i]], [dw1], ws, nbytes // 2) == 0
        assert torch.equal(bits(dw1), bits(dw)), "%s: the dual launch and a single call differ" % what
        assert_guards(buf1, n, what)
    assert_ws_guard(ws, nbytes)
    # one byte short of two partial tensors (= one partial tensor of each gradient): refused, nothing launched or written
    short = 2 * n * 4 - 1
    assert route_of(lib, c, dual=True, ws_bytes=short) == (HUPR_ERR_WORKSPACE, 0)
    (bufa, dwa), (bufb, dwb) = dw_buffer(n), dw_buffer(n)
    ws = ws_buffer(2 * n * 4)
    n0 = lib.hupr_launch_count()
    assert call(lib, c, xb, dybs, [dwa, dwb], ws, short) == HUPR_ERR_WORKSPACE
    assert lib.hupr_launch_count() == n0
    assert bool((bits(bufa) == NAN32).all() and (bits(bufb) == NAN32).all() and (bits(ws) == NAN32).all())


# (what, error, shape, act, (in_ld - Ci, dy_ld - Co), dual, workspace bytes or None = hupr_conv3x3_wgrad_halo_ws_bytes)
REFUSED = [
    ("Ci % 8 != 0", HUPR_ERR_ARG, (2, 60, 64, 4, 8, 8, 3), "bf16", (4, 0), False, None),
    ("H % 8 != 0", HUPR_ERR_ARG, (2, 64, 64, 4, 12, 8, 3), "bf16", P, False, None),
    ("kd 3, odd D", HUPR_ERR_ARG, (2, 64, 64, 3, 8, 8, 3), "bf16", P, False, None),
    ("kd 3, W % 8 != 0", HUPR_ERR_ARG, (2, 64, 64, 4, 8, 12, 3), "bf16", P, False, None),
    ("kd 1, D != 1", HUPR_ERR_ARG, (2, 64, 64, 2, 8, 16, 1), "bf16", P, False, None),
    ("kd 1, W % 16 != 0", HUPR_ERR_ARG, (2, 64, 64, 1, 8, 24, 1), "bf16", P, False, None),
    ("bf16 in_ld % 8 != 0", HUPR_ERR_ARG, (2, 64, 64, 4, 8, 8, 3), "bf16", (4, 0), False, None),
    ("f32 in_ld % 4 != 0", HUPR_ERR_ARG, (2, 64, 64, 4, 8, 8, 3), "f32", (2, 0), False, None),
    ("f32 dy_ld % 4 != 0", HUPR_ERR_ARG, (2, 64, 64, 4, 8, 8, 3), "f32", (0, 2), False, None),
    ("dual, Co % 64 != 0", HUPR_ERR_ARG, (2, 64, 72, 4, 8, 8, 3), "bf16", P, True, None),
    ("workspace below one partial tensor", HUPR_ERR_WORKSPACE, (2, 64, 64, 4, 8, 8, 3), "bf16", P, False, 64 * 64 * 27 * 4 - 1),
    ("f32 workspace below one partial tensor", HUPR_ERR_WORKSPACE, (2, 64, 64, 1, 8, 16, 1), "f32", P, False, 64 * 64 * 9 * 4 - 4),
]


def refused_route(L, r):
    what, err, shape, act, pad, dual, wsb = r
    c = Case(*shape, act, pad, "full", None, err, 0)
    return route_of(L, c, dual=dual, ws_bytes=wsb)


@pytest.mark.parametrize("r", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_calls_leave_everything_untouched(r, lib):
    """Calls the launcher refuses return their error before any launch: dw, the workspace and their guards keep the NaN pattern bit
    for bit and hupr_launch_count() does not move."""
    what, err, shape, act, pad, dual, wsb = r
    c = Case(*shape, act, pad, "full", None, err, 0)
    assert refused_route(lib, r) == (err, 0), what
    dt = torch.float32 if act == "f32" else torch.bfloat16
    in_ld, dy_ld = lds(c)
    vox = c.B * c.D * c.H * c.W
    xb = torch.zeros(vox * in_ld, dtype=dt, device="cuda")
    dybs = [torch.zeros(vox * dy_ld, dtype=dt, device="cuda") for _ in range(2 if dual else 1)]
    n = c.Co * c.Ci * c.kd * 9
    full = ws_bytes_of(lib, c, dual)
    ws = ws_buffer(full)
    bufs = [dw_buffer(n) for _ in dybs]
    n0 = lib.hupr_launch_count()
    rc = call(lib, c, xb, dybs, [dw for _, dw in bufs], ws, full if wsb is None else wsb)
    assert rc == err, (what, rc)
    assert lib.hupr_launch_count() == n0, what
    assert bool((bits(ws) == NAN32).all()), what
    for buf, _ in bufs:
        assert bool((bits(buf) == NAN32).all()), what
