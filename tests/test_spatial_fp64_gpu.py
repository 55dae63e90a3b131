"""GPU (-m gpu): every form of the spatial kernels (csrc/spatial.hip: align_corners=True linear resampling forward, backward and
accumulating backward; the MNet front end fed by x or by elevation-mean planes, and its weight gradient fed by either) against an fp64
reference of exactly the operands the kernel uses, element by element, with the route of every launch asserted first from the
library's own plan (hupr_debug_interp_route, hupr_debug_mnet_grid) against the literal (vpt, grid) of the case table.

Resampling reference: per axis scale, src (the ROUNDED fp32 product), i0, i1, w1 = src - i0 and w0 = 1 - w1 in float32, as lin_coord
and ATen compute them; the three-axis weight product and the sum over the 8 taps in fp64; the backward is the adjoint of that same
sparse map (index_add_ in fp64 on the 8 taps), never autograd of a float32 op.  A is the same sum over absolute values (the accumulate
forms add |dx0|).  Gates, all derived: fp32-stored forward |y - ref| <= 2^-20 A (two roundings in the weight product, eight FMAs:
10 x 2^-24 < 2^-20); fp32-stored backward |dx - ref| <= (T + 2) 2^-24 A with T the case's largest contributor count per input voxel,
taken from the reference map; a bf16 store adds 2^-8 |ref|; a NaN never passes.  The bf16 forward must also equal, bit for bit, the
round-to-nearest-even of the fp32 forward on the same bf16-representable input.  An input voxel without a contributor must come back
as +0 (backward) or with dx0's bits untouched (accumulating backward).  On the dense small cases the fp32 forward is compared with
F.interpolate(align_corners=True) in float64 as well: |y - torch64| <= 2^-20 A + 3 x 2^-23 max(in - 1) R, R the largest difference
between neighbouring input voxels along any axis (the second term covers the fp32 rounding of src, which the fp64 op does not have).

Outputs are channel slices of NaN-pattern buffers between guards; every column outside the slice and every guard must come back
bit-identical, no output element may stay NaN, and a second launch into fresh buffers must give the same bits.  x and dy sit in
NaN-pattern buffers too (NaN columns, NaN guard tails), so a read outside the slice shows.

MNet reference: the reference model's .view reinterpretation (plane j = 2 f + c is read as ch2 = j / 8, t = j % 8: not a permute),
Conv3d(2 -> 32, (2, 1, 1), stride (2, 1, 1)), the maximum over the four steps, the first maximum taking the gradient; all fp64.  x is
drawn as multiples of 2^-10 below 4, so the eight-term sum and the multiply by 0.125 are exact in fp32: the means output must equal
the reference means bit for bit, and the four forward forms and the two backward feeds see identical operands.  Gates: fp32-stored
forward |out - ref| <= 2^-22 A with A = |bias| + sum |w| |m| at the winning step (four FMAs; derived); the bf16 store must be bit-equal
to the round-to-nearest-even of the fp32 form; dW and dbias |d - ref| <= c A_d with A_d = sum |dy| |m| and sum |dy|.  c is not
derivable (per-thread run length, shuffle order): the smallest power of two that is at least 8 x the worst err / A_d measured over this
table against fp64 on an MI355X, never above 2^-16.  Measured worst values per form (the four forms of a case — fed by the means or
by x, fp32 or bf16 dy of the same values — return the same bits, which the test asserts, hence the same figures):

    quantity   from means, f32 / bf16 dy   from x, f32 / bf16 dy   at
    dW         2^-24.41                    2^-24.41                37 pixels (5 x 63: 2^-25.32; 65 536 pixels and more: 2^-29.5 .. 2^-30.2)
    dbias      2^-30.75                    2^-30.75                65 745 pixels (37 pixels: exact; the others 2^-30.9 .. 2^-31.9)

(The short sums of the 37-pixel case carry the fp32 rounding of the result itself, up to 2^-24 of it; the long ones are summed in
fp32 over a thread's few pixels and in fp64 from there.)  8 x these: 2^-21.41 and 2^-27.75, hence MNET_C = 2^-21 (dW), 2^-27 (dbias).

The arg-max is discontinuous: where the fp64 margin between the best and the second-best step is below 2^-21 A (A the largest of the
four steps' sums) either step is a legitimate choice.  A case may hold no such (pixel, channel) entry: after drawing, the pixels that
contain one are re-drawn in a deterministic loop until none is left (asserted here; tests/test_spatial_route.py asserts it on the CPU).
The exact-tie case has small-integer means and weights, two or more steps tie exactly in at least a quarter of its entries, and its
forward and both gradients are compared exactly, with the fp64 reference and with F.max_pool3d + autograd in float64 on the CPU.

The forward wrap at 2^21 + 192 pixels runs the means-fed forms only (134 MB of mean planes): the x-fed form would read a 1 GiB
input that takes longer to draw and to reduce in fp64 than a test may take; its loop is the same statement as the means-fed one
and wraps nowhere in the model (4096 workgroups at batch 32).

tests/test_spatial_route.py checks the routes of this table, its coverage and the refusals without a GPU, and that the gates reject
the results of subtly wrong kernels."""
import collections
import ctypes
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_conv_halo_fp64_gpu import GUARD, NAN16, NAN32, bits, nan_buffer, padded, rnd

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG, HUPR_ERR_WORKSPACE = -1, -2
OPS = ("fwd", "bwd", "acc")                                   # hupr_debug_interp_route's op numbers
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ENTRY = {("fwd", "f32"): "hupr_interp_linear_fwd_f32", ("fwd", "bf16"): "hupr_interp_linear_fwd_bf16act",
         ("bwd", "f32"): "hupr_interp_linear_bwd_f32", ("bwd", "bf16"): "hupr_interp_linear_bwd_bf16act",
         ("acc", "f32"): "hupr_interp_linear_bwd_acc_f32", ("acc", "bf16"): "hupr_interp_linear_bwd_acc_bf16act"}

# ---- the resampling table ------------------------------------------------------------------------------------------------------
# fwd / bwd32 / bwd16: the literal (channel vectors per thread, workgroups) of the forward launch (the same for both storage types:
# it walks 4-channel items) and of the backward and accumulating-backward launches per storage type.  in_ld / out_ld: voxel strides
# of x, dx / of y, dy; off: channel offset of the y / dy slice inside its out_ld-wide buffer.  dev: the reference runs on the device.
Case = collections.namedtuple("Case", "name B din dout C in_ld out_ld off types ops dev fwd bwd32 bwd16")
BOTH, ALL = ("f32", "bf16"), OPS


def _case(name, B, din, dout, C, fwd, bwd32, bwd16, in_ld=None, out_ld=None, off=0, types=BOTH, ops=ALL, dev=False):
    return Case(name, B, din, dout, C, in_ld or C, out_ld or C, off, types, ops, dev, fwd, bwd32, bwd16)


CASES = [
    # ---- ratios: the backward gather's candidate window away from 2:1
    _case("7to13-13to7", 2, (1, 7, 13), (1, 13, 7), 16, (1, 3), (1, 3), (1, 2)),
    _case("31to17", 2, (1, 31, 31), (1, 17, 17), 8, (1, 5), (1, 16), (1, 8)),
    _case("5to64-many-contributors", 2, (1, 5, 5), (1, 64, 64), 8, (1, 64), (1, 1), (1, 1)),
    _case("64to5-most-without", 2, (1, 64, 64), (1, 5, 5), 8, (1, 1), (1, 64), (1, 32)),
    _case("n-to-1-takes-plane-0", 2, (4, 6, 5), (1, 6, 1), 8, (1, 1), (1, 2), (1, 1)),
    _case("1-to-n", 2, (1, 6, 1), (4, 6, 5), 8, (1, 2), (1, 1), (1, 1)),
    _case("trilinear-3-ratios", 2, (3, 7, 10), (5, 4, 16), 24, (1, 15), (1, 10), (1, 5)),
    # ---- the model's own maps, at the smallest batch that keeps the route of the training batch (32): all VPT = 4 there but the
    # PRGCN up-sampling, which stays on VPT = 1 up to batch 63
    _case("level1-half-B1", 1, (8, 64, 64), (4, 32, 32), 64, (1, 256), (4, 512), (4, 256), dev=True),      # bf16: exactly 65536
    _case("level2-half-B4", 4, (4, 32, 32), (2, 16, 16), 128, (1, 256), (4, 512), (4, 256), dev=True),     # bf16: exactly 65536
    _case("decoder-16to32-C256-B32", 32, (1, 16, 16), (1, 32, 32), 256, (1, 8192), (4, 512), (4, 256), dev=True),
    _case("decoder-32to64-C128-B16", 16, (1, 32, 32), (1, 64, 64), 128, (1, 8192), (4, 512), (4, 256), dev=True),
    _case("decoder-32to64-C64-B32", 32, (1, 32, 32), (1, 64, 64), 64, (1, 8192), (4, 512), (4, 256), dev=True),
    _case("prgcn-64to32-C16-B16", 16, (1, 64, 64), (1, 32, 32), 16, (1, 256), (4, 256), None, types=("f32",), dev=True),
    _case("prgcn-32to64-C16-B2", 2, (1, 32, 32), (1, 64, 64), 16, (1, 128), (1, 32), None, types=("f32",)),
    # ---- the VPT threshold voxels * C / (4 V) >= 65536 from below, at and above it: C = 16 for fp32 (V = 4), C = 32 for bf16 (V = 8)
    _case("vpt-below-C16", 1, (1, 257, 255), (1, 129, 128), 16, (1, 258), (1, 1024), (1, 512), dev=True),   # bf16: C % 32 != 0 on a large map
    _case("vpt-at-C16", 1, (1, 256, 256), (1, 128, 128), 16, (1, 256), (4, 256), (1, 512), dev=True),
    _case("vpt-above-C16", 1, (1, 256, 257), (1, 128, 129), 16, (1, 258), (4, 257), (1, 514), dev=True),
    _case("vpt-below-C32", 1, (1, 257, 255), (1, 129, 128), 32, (1, 516), (4, 512), (1, 1024), dev=True),
    _case("vpt-at-C32", 1, (1, 256, 256), (1, 128, 128), 32, (1, 512), (4, 512), (4, 256), dev=True),
    _case("vpt-above-C32", 1, (1, 256, 257), (1, 128, 129), 32, (1, 516), (4, 514), (4, 257), dev=True),
    _case("vpt1-C8-large-map", 1, (1, 256, 257), (1, 128, 129), 8, (1, 129), (1, 514), (1, 257), dev=True),   # fp32: C % 16 != 0
    # ---- grid-stride loops that wrap: forward above 2^21 (voxel, 4-channel) items (8192 workgroups), backward above 2^22 items
    # (16384 workgroups) at VPT = 1 and at VPT = 4
    _case("fwd-wrap", 1, (1, 9, 9), (1, 1024, 1025), 8, (1, 8192), None, None, ops=("fwd",), dev=True),
    _case("bwd-wrap-vpt1", 1, (1, 1448, 1450), (1, 724, 725), 8, None, (1, 16384), None, types=("f32",), ops=("bwd", "acc"), dev=True),
    _case("bwd-wrap-vpt4", 1, (1, 2048, 2050), (1, 1024, 1025), 16, None, (4, 16384), None, types=("f32",), ops=("bwd", "acc"), dev=True),
    # ---- leading dimensions: the decoder's concatenation buffer (out_ld > C, a slice at a 16-byte-aligned channel offset) and in_ld > C
    _case("out_ld-C+8", 2, (2, 5, 6), (3, 7, 9), 16, (1, 6), (1, 2), (1, 1), out_ld=24),
    _case("out-slice-of-320", 2, (2, 5, 6), (3, 7, 9), 16, (1, 6), (1, 2), (1, 1), out_ld=320, off=40),
    _case("in_ld-C+8", 2, (2, 5, 6), (3, 7, 9), 16, (1, 6), (1, 2), (1, 1), in_ld=24),
    _case("both-ld", 2, (1, 16, 16), (1, 32, 32), 64, (1, 128), (1, 32), (1, 16), in_ld=72, out_ld=320, off=64),
]
assert 1024 * 1025 * 2 > 1 << 21 and 1448 * 1450 * 2 > 1 << 22 and 2048 * 2050 > 1 << 22


def case_id(c):
    return c.name


def vox(ext):
    return ext[0] * ext[1] * ext[2]


def expected_route(c, T, op):
    return c.fwd if op == "fwd" else (c.bwd16 if T == "bf16" else c.bwd32)


def route_of(L, op, T, B, din, dout, C, in_ld, out_ld):
    """(vpt, grid) of the launch from the library's plan, or its error code."""
    g = ctypes.c_int(-1)
    vpt = L.hupr_debug_interp_route(OPS.index(op), int(T == "bf16"), B, *din, *dout, C, in_ld, out_ld, ctypes.byref(g))
    return (vpt, g.value) if vpt > 0 else vpt


def case_route(L, c, T, op):
    return route_of(L, op, T, c.B, c.din, c.dout, c.C, c.in_ld, c.out_ld)


# ---- the fp64 resampling reference and its gates (any device) --------------------------------------------------------------------
def axis_map(n_in, n_out, device="cpu"):
    """((i0, i1), (w0, w1)) of an axis: indices int64, weights the float32 values of lin_coord, returned as fp64."""
    f32 = torch.float32
    o = torch.arange(n_out, dtype=f32, device=device)
    if n_out > 1:
        scale = torch.tensor(float(n_in - 1), dtype=f32, device=device) / torch.tensor(float(n_out - 1), dtype=f32, device=device)
    else:
        scale = torch.zeros((), dtype=f32, device=device)
    src = scale * o                                           # rounded to fp32 before the subtraction below
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    w1 = src - i0.to(f32)
    w0 = 1 - w1
    assert w0.dtype == f32 and w1.dtype == f32
    return (i0, i1), (w0.double(), w1.double())


def taps_of(din, dout, device="cpu", axis_map=axis_map):
    """The sparse map as 8 (flat input voxel index [Vo], fp64 weight [Vo]) pairs; the weight is the fp64 product of the three fp32 axis
    weights."""
    (Di, Hi, Wi), (Do, Ho, Wo) = din, dout
    md, mh, mw = axis_map(Di, Do, device), axis_map(Hi, Ho, device), axis_map(Wi, Wo, device)
    out = []
    for a in range(2):
        for b in range(2):
            for c in range(2):
                idx = (md[0][a].view(Do, 1, 1) * Hi + mh[0][b].view(1, Ho, 1)) * Wi + mw[0][c].view(1, 1, Wo)
                w = md[1][a].view(Do, 1, 1) * mh[1][b].view(1, Ho, 1) * mw[1][c].view(1, 1, Wo)
                out.append((idx.reshape(-1), w.reshape(-1)))
    return out


def fwd_ref(x, taps):
    """x [B, Vi, C] -> (ref, A) [B, Vo, C] in fp64."""
    xd = x.double()
    ref = A = None
    for idx, w in taps:
        g = xd[:, idx]
        t, ta = w.view(1, -1, 1) * g, w.abs().view(1, -1, 1) * g.abs()
        ref, A = (t, ta) if ref is None else (ref + t, A + ta)
    return ref, A


def bwd_ref(dy, taps, Vi, dx0=None):
    """dy [B, Vo, C] -> (ref, A) [B, Vi, C] in fp64: the adjoint of the map of fwd_ref, plus dx0 for the accumulating form."""
    dyd = dy.double()
    ref = torch.zeros(dy.shape[0], Vi, dy.shape[2], dtype=torch.float64, device=dy.device)
    A = torch.zeros_like(ref)
    for idx, w in taps:
        ref.index_add_(1, idx, w.view(1, -1, 1) * dyd)
        A.index_add_(1, idx, w.abs().view(1, -1, 1) * dyd.abs())
    if dx0 is not None:
        ref, A = ref + dx0.double(), A + dx0.double().abs()
    return ref, A


def axis_contributors(n_in, n_out):
    """[n_in]: how many output indices reach each input index with a non-zero weight (both taps on one index count once)."""
    (i0, i1), (w0, w1) = axis_map(n_in, n_out)
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    r = torch.arange(n_out)
    M.index_put_((r, i0), w0, accumulate=True)
    M.index_put_((r, i1), w1, accumulate=True)
    return (M != 0).sum(0)


def contributors(din, dout):
    """(T, has [Vi] bool): the largest contributor count of an input voxel and which input voxels have a contributor at all."""
    n = [axis_contributors(i, o) for i, o in zip(din, dout)]
    cnt = (n[0].view(-1, 1, 1) * n[1].view(1, -1, 1) * n[2].view(1, 1, -1)).reshape(-1)
    return int(cnt.max()), cnt > 0


def within_fwd(y, ref, A, bf16_store):
    lim = 2.0 ** -20 * A
    if bf16_store:
        lim = lim + 2.0 ** -8 * ref.abs()
    return (y.double() - ref).abs() <= lim                 # (a NaN never is)


def within_bwd(dx, ref, A, T, bf16_store):
    lim = (T + 2) * 2.0 ** -24 * A
    if bf16_store:
        lim = lim + 2.0 ** -8 * ref.abs()
    return (dx.double() - ref).abs() <= lim


def assert_all(ok, out, ref, A, what):
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d outside the gate, first at %s (out %r, ref %r, A %r), worst err / A 2^%.2f" % (
            what, bad.shape[0], ok.numel(), i, out[i].item(), ref[i].item(), A[i].item(),
            torch.log2(((out.double() - ref).abs() / A.clamp_min(1e-300)).nan_to_num(float("inf")).max()).item()))


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def make_operands(c, device="cpu"):
    """Seeded x [B, Vi, C], dy [B, Vo, C] and dx0 [B, Vi, C] (fp32) of a case, drawn on `device`."""
    g = torch.Generator(device=device).manual_seed(seed_of(c.name))
    Vi, Vo = vox(c.din), vox(c.dout)
    mk = lambda *s: torch.randn(*s, generator=g, device=device)
    return {"x": mk(c.B, Vi, c.C) if "fwd" in c.ops else None, "dy": mk(c.B, Vo, c.C) if any(op != "fwd" for op in c.ops) else None,
            "dx0": mk(c.B, Vi, c.C) if "acc" in c.ops else None}


# ---- NaN-guarded buffers and the launches (GPU) --------------------------------------------------------------------------------
def placed(vals, nvox, C, ld, off, dtype):
    """guard | nvox x ld | guard in the NaN pattern with vals (or nothing, for an output) in columns off .. off + C; -> (buffer, the
    address of the slice's first element)."""
    buf = nan_buffer(GUARD + nvox * ld + GUARD, dtype)
    if vals is not None:
        buf[GUARD:GUARD + nvox * ld].view(nvox, ld)[:, off:off + C] = vals.reshape(nvox, C).to("cuda", dtype)
    return buf, buf.data_ptr() + (GUARD + off) * buf.element_size()


def taken(buf, nvox, C, ld, off, what):
    """The slice of a buffer of `placed` after a launch, with everything around it verified bit-identical and no NaN left inside."""
    nan = NAN16 if buf.dtype == torch.bfloat16 else NAN32
    body = buf[GUARD:GUARD + nvox * ld].view(nvox, ld)
    assert bool((bits(buf[:GUARD]) == nan).all()), "%s: the guard in front was written" % what
    assert bool((bits(buf[GUARD + nvox * ld:]) == nan).all()), "%s: the guard behind was written" % what
    if off:
        assert bool((bits(body[:, :off].contiguous()) == nan).all()), "%s: a column in front of the slice was written" % what
    if off + C < ld:
        assert bool((bits(body[:, off + C:].contiguous()) == nan).all()), "%s: a column behind the slice was written" % what
    out = body[:, off:off + C]
    assert not bool(out.isnan().any()), "%s: an output element was left NaN" % what
    return out.contiguous()


def launch(L, c, T, op, src, dst, geo=None):
    from hupr_amd import runtime as rt
    B, din, dout, C, in_ld, out_ld = geo or (c.B, c.din, c.dout, c.C, c.in_ld, c.out_ld)
    rc = getattr(L, ENTRY[(op, T)])(src, dst, B, *din, *dout, C, in_ld, out_ld, rt.stream())
    torch.cuda.synchronize()
    return rc


def run(L, c, T, op, o, what, twice=True):
    """One guarded launch (and a second one into fresh buffers, bit-compared) of op in storage type T on the operands o: x / dy / dx0
    as fp32 tensors holding the values the kernel is to read.  -> the output [B, V, C] in its storage type."""
    dt = DT[T]
    ni, no = c.B * vox(c.din), c.B * vox(c.dout)
    outs = []
    for _ in range(2 if twice else 1):
        if op == "fwd":
            sbuf, src = placed(o["x"], ni, c.C, c.in_ld, 0, dt)
            dbuf, dst = placed(None, no, c.C, c.out_ld, c.off, dt)
            geo = (no, c.out_ld, c.off)
        else:
            sbuf, src = placed(o["dy"], no, c.C, c.out_ld, c.off, dt)
            dbuf, dst = placed(o["dx0"] if op == "acc" else None, ni, c.C, c.in_ld, 0, dt)
            geo = (ni, c.in_ld, 0)
        n0 = L.hupr_launch_count()
        assert launch(L, c, T, op, src, dst) == 0, L.hupr_last_error()
        assert L.hupr_launch_count() - n0 == 1
        outs.append(taken(dbuf, geo[0], c.C, geo[1], geo[2], what))
        del sbuf, dbuf
    if twice:
        assert torch.equal(bits(outs[0]), bits(outs[1])), "%s: two launches differ" % what
    return outs[0].view(c.B, -1, c.C)


def operands_for(c, T, dev):
    """The case's operands as the values a kernel of storage type T reads (bf16: rounded to bf16), fp32 tensors on `dev`."""
    o = make_operands(c, "cuda" if c.dev else "cpu")
    if T == "bf16":
        o = {k: None if v is None else v.to(torch.bfloat16).float() for k, v in o.items()}
    return {k: None if v is None else v.to(dev) for k, v in o.items()}


def check_case(L, c, T, twice=True, torch64=False):
    """Every op of the case in storage type T: route, guarded launches, the gate against the fp64 reference (on the device for the large
    cases, on the CPU for the small ones), the exact properties of voxels without a contributor and of the bf16 store."""
    dev = "cuda" if c.dev else "cpu"
    bf = T == "bf16"
    o = operands_for(c, T, dev)
    taps = taps_of(c.din, c.dout, dev)
    Tn, has = contributors(c.din, c.dout)
    none = (~has).to(dev)
    Vi = vox(c.din)
    for op in c.ops:
        what = "%s %s %s" % (c.name, T, op)
        assert case_route(L, c, T, op) == expected_route(c, T, op), what
        out = run(L, c, T, op, {k: None if v is None else v.cuda() for k, v in o.items()}, what, twice).to(dev)
        if op == "fwd":
            ref, A = fwd_ref(o["x"], taps)
            assert_all(within_fwd(out, ref, A, bf), out, ref, A, what)
            if bf:                                        # the same kernel arithmetic, one more rounding: RNE of the fp32 form
                y32 = run(L, c, "f32", "fwd", {"x": o["x"].cuda()}, what + " (fp32 form on the bf16-representable x)", False)
                assert torch.equal(bits(out.cuda()), bits(y32.to(torch.bfloat16))), "%s: not the nearest-even rounding of the fp32 form" % what
            elif torch64:
                assert_matches_torch64(c, o["x"], out, A, what)
        else:
            dx0 = o["dx0"] if op == "acc" else None
            ref, A = bwd_ref(o["dy"], taps, Vi, dx0)
            assert_all(within_bwd(out, ref, A, Tn, bf), out, ref, A, what)
            if bool(none.any()):
                got = bits(out[:, none].contiguous())
                if op == "acc":
                    assert torch.equal(got, bits(dx0[:, none].to(DT[T]).contiguous())), "%s: a voxel without a contributor lost dx0's bits" % what
                else:
                    assert bool((got == 0).all()), "%s: a voxel without a contributor is not +0" % what
    return Tn


def assert_matches_torch64(c, x, y, A, what):
    """The independent check of the semantics: F.interpolate(align_corners=True) in float64 on the same x."""
    xr = x.double().view(c.B, *c.din, c.C).permute(0, 4, 1, 2, 3)
    yr = F.interpolate(xr, size=c.dout, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1).reshape(c.B, -1, c.C)
    R = max([(xr.diff(dim=d).abs().max().item() if xr.shape[d] > 1 else 0.0) for d in (2, 3, 4)])
    lim = 2.0 ** -20 * A + 3 * 2.0 ** -23 * max(n - 1 for n in c.din) * R
    ok = (y.double() - yr).abs() <= lim
    assert bool(ok.all()), "%s against F.interpolate in float64: %d outside, worst err / bound %.3g" % (
        what, int((~ok).sum()), ((y.double() - yr).abs() / lim.clamp_min(1e-300)).max().item())


@pytest.fixture
def lib():
    from hupr_amd import runtime
    return runtime.lib()


PARAMS = [(c, T) for c in CASES for T in c.types]


@pytest.mark.parametrize("c,T", PARAMS, ids=["%s-%s" % (c.name, T) for c, T in PARAMS])
def test_resampling_form_matches_fp64(c, T, lib):
    dense_small = not c.dev and c.in_ld == c.C and c.out_ld == c.C
    check_case(lib, c, T, torch64=dense_small)


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", BOTH)
def test_same_extent_is_a_bitwise_copy_both_ways(T, lib):
    c = _case("identity", 2, (2, 3, 5), (2, 3, 5), 8, (1, 1), (1, 1), (1, 1), ops=("fwd", "bwd"))
    o = operands_for(c, "bf16", "cuda")                       # bf16-representable in both storage types
    for op, key in (("fwd", "x"), ("bwd", "dy")):
        assert case_route(lib, c, T, op) == (1, 1)
        out = run(lib, c, T, op, o, "identity " + op)
        assert torch.equal(bits(out), bits(o[key].to(DT[T]))), op


@pytest.mark.parametrize("T", BOTH)
def test_one_hot_at_scale_one_half_is_exact(T, lib):
    """out = 2 in - 1: scale is exactly 0.5, every weight is 0, 0.5 or 1.  x holds one few-bit value per (sample, channel) at its own
    voxel, dy likewise: every result is one product, exact in fp32 and in bf16; the kernel must equal the fp64 reference exactly."""
    c = _case("one-hot-half", 2, (3, 4, 5), (5, 7, 9), 8, (1, 5), (1, 1), (1, 1), ops=("fwd", "bwd"))
    vals = torch.tensor([1.0, 1.5, -2.0, 0.75, -1.25, 3.0, -0.5, 1.75])
    taps = taps_of(c.din, c.dout)
    for op, V, key in (("fwd", vox(c.din), "x"), ("bwd", vox(c.dout), "dy")):
        assert case_route(lib, c, T, op) == expected_route(c, T, op)
        t = torch.zeros(c.B, V, c.C)
        for b in range(c.B):
            for k in range(c.C):
                t[b, (7 * k + 13 * b + 5) % V, k] = vals[(k + 3 * b) % 8]
        out = run(lib, c, T, op, {key: t.cuda()}, "one-hot " + op).cpu()
        ref = fwd_ref(t, taps)[0] if op == "fwd" else bwd_ref(t, taps, vox(c.din))[0]
        assert int((ref != 0).sum()) > 2 * c.B * c.C
        assert torch.equal(out.double(), ref), op


# ---- the small-extent sweep of the candidate window -----------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["W", "H"])
@pytest.mark.parametrize("T", BOTH)
def test_every_extent_pair_up_to_12(T, axis, lib):
    """Every (in, out) in 1..12 squared along W (D = H = 1) and along H (W = 3, so the middle axis is not always degenerate): forward,
    backward and accumulating backward against the reference."""
    for n_in in range(1, 13):
        for n_out in range(1, 13):
            din, dout = ((1, 1, n_in), (1, 1, n_out)) if axis == "W" else ((1, n_in, 3), (1, n_out, 3))
            c = _case("sweep-%s-%d-%d" % (axis, n_in, n_out), 2, din, dout, 8, (1, 1), (1, 1), (1, 1))
            check_case(lib, c, T, twice=False, torch64=True)


# ---- refused calls ---------------------------------------------------------------------------------------------------------------------
OK_GEO = (2, (2, 4, 4), (3, 5, 6), 8, 8, 8)
# (what, T, op, (B, din, dout, C, in_ld, out_ld), which pointer is null: None, "src" or "dst")
REFUSED = []
for _T in BOTH:
    for _op in OPS:
        REFUSED += [("%s %s: C = 6" % (_T, _op), _T, _op, (2, (2, 4, 4), (3, 5, 6), 6, 8, 8), None),
                    ("%s %s: in_ld < C" % (_T, _op), _T, _op, (2, (2, 4, 4), (3, 5, 6), 8, 4, 8), None),
                    ("%s %s: out_ld %% 4 != 0" % (_T, _op), _T, _op, (2, (2, 4, 4), (3, 5, 6), 8, 8, 10), None),
                    ("%s %s: an input extent of 0" % (_T, _op), _T, _op, (2, (2, 0, 4), (3, 5, 6), 8, 8, 8), None),
                    ("%s %s: an output extent of 0" % (_T, _op), _T, _op, (2, (2, 4, 4), (3, 5, 0), 8, 8, 8), None),
                    ("%s %s: batch 0" % (_T, _op), _T, _op, (0, (2, 4, 4), (3, 5, 6), 8, 8, 8), None),
                    ("%s %s: null source" % (_T, _op), _T, _op, OK_GEO, "src"),
                    ("%s %s: null destination" % (_T, _op), _T, _op, OK_GEO, "dst")]
for _op in ("bwd", "acc"):
    REFUSED += [("bf16 %s: C = 12" % _op, "bf16", _op, (2, (2, 4, 4), (3, 5, 6), 12, 12, 12), None),
                ("bf16 %s: in_ld = 12" % _op, "bf16", _op, (2, (2, 4, 4), (3, 5, 6), 8, 12, 8), None),
                ("bf16 %s: out_ld = 12" % _op, "bf16", _op, (2, (2, 4, 4), (3, 5, 6), 8, 8, 12), None)]


def refused_call(L, r, src, dst, stream):
    """The refused call on the given addresses (integers): rejected by host checks, nothing is dereferenced."""
    what, T, op, (B, din, dout, C, in_ld, out_ld), null = r
    return getattr(L, ENTRY[(op, T)])(None if null == "src" else src, None if null == "dst" else dst, B, *din, *dout, C, in_ld, out_ld, stream)


@pytest.mark.parametrize("r", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_resampling_calls_leave_everything_untouched(r, lib):
    from hupr_amd import runtime as rt
    what, T, op, geo, null = r
    if null is None:
        assert route_of(lib, op, T, *geo) == HUPR_ERR_ARG, what
    n = 1 << 14
    src = torch.zeros(n, dtype=DT[T], device="cuda")
    dst = nan_buffer(n, DT[T])
    n0 = lib.hupr_launch_count()
    rc = refused_call(lib, r, src.data_ptr(), dst.data_ptr(), rt.stream())
    torch.cuda.synchronize()
    assert rc == HUPR_ERR_ARG, (what, rc)
    assert lib.hupr_launch_count() == n0, what
    assert bool((bits(dst) == (NAN16 if T == "bf16" else NAN32)).all()), what


def test_bf16_map_with_12_channels_resamples_forward_only(lib):
    """bf16act forward accepts C % 4 == 0, the backward forms need C % 8 == 0: C = 12 goes forward (and matches the reference) and is
    refused on the way back."""
    c = _case("bf16-C12", 2, (2, 4, 4), (3, 5, 6), 12, (1, 3), (1, 1), None, ops=("fwd",))
    check_case(lib, c, "bf16")
    check_case(lib, c._replace(ops=ALL), "f32")
    for op in ("bwd", "acc"):
        assert case_route(lib, c, "bf16", op) == HUPR_ERR_ARG


# ---- through functional.py -----------------------------------------------------------------------------------------------------------
def spatial_entries():
    """The entry points of csrc/spatial.hip, from the binding table."""
    from hupr_amd import runtime as rt
    return sorted(n for n in rt.SIGNATURES
                  if n.startswith("hupr_interp_linear_") or (n.startswith("hupr_mnet_") and not n.startswith("hupr_mnet_stream")))


class Counted:
    """The callable entry points of csrc/spatial.hip on rt.lib() wrapped by call counters for the block."""

    def __init__(self, L):
        self.L, self.n, self.orig = L, collections.Counter(), {}

    def __enter__(self):
        for name in spatial_entries():
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


NODE = _case("node", 2, (2, 5, 6), (3, 7, 9), 16, (1, 6), (1, 2), (1, 1))


@pytest.mark.parametrize("placement", ["own-output", "out-slice"])
@pytest.mark.parametrize("T", BOTH)
def test_interp_node_calls_each_entry_once(T, placement, lib):
    """functional.interp without and with out= (a slice at channel 40 of a 320-wide buffer, whose other channels must survive; the
    gradient arrives as such a slice too): one forward and one backward entry call, both results inside the gates."""
    from hupr_amd import functional as F_
    c, dt = NODE, DT[T]
    o = operands_for(c, T, "cuda")
    x = o["x"].view(c.B, *c.din, c.C).to(dt).clone().requires_grad_(True)
    wide = gwide = None
    if placement == "out-slice":
        wide = nan_buffer(c.B * vox(c.dout) * 320, dt).view(c.B, *c.dout, 320)
        gwide = nan_buffer(c.B * vox(c.dout) * 320, dt).view(c.B, *c.dout, 320)
        gwide[..., 40:56] = o["dy"].view(c.B, *c.dout, c.C).to(dt)
    with Counted(lib) as n:
        y = F_.interp(x, c.dout, out=None if wide is None else wide[..., 40:56])
        assert n.take() == {ENTRY[("fwd", T)]: 1}
        y.backward(o["dy"].view(c.B, *c.dout, c.C).to(dt) if gwide is None else gwide[..., 40:56])
        assert n.take() == {ENTRY[("bwd", T)]: 1}
    torch.cuda.synchronize()
    if wide is not None:
        nan = NAN16 if T == "bf16" else NAN32
        assert y.data_ptr() == wide.data_ptr() + 40 * wide.element_size()
        assert bool((bits(wide[..., :40].contiguous()) == nan).all()) and bool((bits(wide[..., 56:].contiguous()) == nan).all())
    taps = taps_of(c.din, c.dout, "cuda")
    Tn, _ = contributors(c.din, c.dout)
    got = y.detach().reshape(c.B, -1, c.C)
    ref, A = fwd_ref(o["x"], taps)
    assert_all(within_fwd(got, ref, A, T == "bf16"), got, ref, A, "interp node forward")
    assert x.grad.dtype == dt
    got = x.grad.reshape(c.B, -1, c.C)
    ref, A = bwd_ref(o["dy"], taps, vox(c.din))
    assert_all(within_bwd(got, ref, A, Tn, T == "bf16"), got, ref, A, "interp node backward")


@pytest.fixture
def bf16_math():
    from hupr_amd import functional as F_
    F_.set_math("bf16")
    yield
    F_.set_math("f32")


def test_merge_down_node_accumulates_onto_the_merge_gradient(lib, bf16_math):
    """MergeDownFn at (G = 4, 16 x 16, C = 64) -> (2, 8, 8): one bf16act forward call, one accumulating-backward call.  With a zero
    gradient of the down-sampled map the node returns the merge's own input gradient M (bf16); with the real one it must return
    M + the resampling adjoint inside the accumulating gate, and M's bits where a voxel has no contributor."""
    from hupr_amd import functional as F_
    B, G, H, W, C = 2, 4, 16, 16, 64
    size = (2, 8, 8)
    x = rnd(B, G, H, W, C, seed=901).to(torch.bfloat16).cuda()
    w = rnd(C, C, G, 1, 1, seed=902, scale=(C * G) ** -0.5).cuda()
    dm = rnd(B, 1, H, W, C, seed=903).cuda()
    dd = rnd(B, *size, C, seed=904).to(torch.bfloat16).cuda()
    grads = []
    for g_down in (torch.zeros_like(dd), dd):
        xi, wi = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        with Counted(lib) as n:
            merged, down = F_.MergeDownFn.apply(xi, wi, size)
            assert n.take() == {ENTRY[("fwd", "bf16")]: 1}
            torch.autograd.backward((merged, down), (dm, g_down))
            assert n.take() == {ENTRY[("acc", "bf16")]: 1}
        grads.append(xi.grad.reshape(B, -1, C))
    torch.cuda.synchronize()
    M, dx = grads
    din = (G, H, W)
    taps = taps_of(din, size, "cuda")
    Tn, has = contributors(din, size)
    got = down.detach().reshape(B, -1, C)
    ref, A = fwd_ref(x.view(B, -1, C), taps)
    assert_all(within_fwd(got, ref, A, True), got, ref, A, "MergeDownFn down-sampled map")
    ref, A = bwd_ref(dd.view(B, -1, C), taps, vox(din), M)
    assert_all(within_bwd(dx, ref, A, Tn, True), dx, ref, A, "MergeDownFn dx")
    none = (~has).cuda()
    assert bool(none.any()) and torch.equal(bits(dx[:, none].contiguous()), bits(M[:, none].contiguous()))


# ==== MNet ================================================================================================================================
MNET_CAP = 2.0 ** -16
MNET_C = {"dw": 2.0 ** -21, "db": 2.0 ** -27}              # see the table in the module docstring
assert max(MNET_C.values()) <= MNET_CAP

# name, n_bg, pixels, x_fed (False: the case runs the means-fed forward only), bwd, and the literal workgroups of hupr_mnet_fwd_*,
# hupr_mnet_fwd_means_* and hupr_mnet_bwd_*
MCase = collections.namedtuple("MCase", "name n_bg pixels x_fed bwd g_fwd g_means g_bwd")
MCASES = [
    MCase("37px", 1, 37, True, True, 1, 1, 1),                                       # one partly idle workgroup
    MCase("5x63", 5, 63, True, True, 2, 2, 5),                                       # the bg / pixel split, a ragged total
    MCase("total-65536", 2, 32768, True, True, 256, 256, 1024),                      # backward: exactly one pass for each of 1024
    MCase("total-65536+209", 5, 13149, True, True, 257, 257, 1024),                  # backward wraps unevenly, ragged last wave
    MCase("model-64x64-bg16", 16, 4096, True, True, 256, 256, 1024),                 # the model's map at B G = 16: one pass each
    MCase("model-64x64-bg32", 32, 4096, True, True, 512, 512, 1024),                 # backward wraps evenly (twice)
    MCase("fwd-wrap-2^21+192", 8, 262168, False, False, None, 8192, None),           # forward wraps (means-fed only: see the docstring)
]
assert 5 * 13149 == 65536 + 3 * 64 + 17 and 8 * 262168 == (1 << 21) + 192
MNET_OP = {"fwd": 0, "means": 1, "bwd": 2}


def mnet_grids(L, c):
    return tuple(L.hupr_debug_mnet_grid(op, c.n_bg, c.pixels) for op in (0, 1, 2))


def mnet_steps(m, w, b):
    """m [N, 16] fp64 means of N pixels (plane j = 2 f + c), w [32, 2, 2], b [32] fp64 -> (o, Ao) [N, 32, 4]: the convolution output of
    the four steps and the same sum over absolute values.  The .view: plane j is (ch2 = j / 8, t = j % 8)."""
    v = m.view(-1, 2, 4, 2)                                    # [N, ch2, t2, kt]: t = 2 t2 + kt
    o = torch.einsum("nctk,ock->not", v, w) + b.view(1, 32, 1)
    Ao = torch.einsum("nctk,ock->not", v.abs(), w.abs()) + b.abs().view(1, 32, 1)
    return o, Ao


def first_max(o):
    """Index of the first maximum along the last axis (torch.max does not promise which one it returns)."""
    best = o.max(-1, keepdim=True).values
    return (o == best).to(torch.int8).argmax(-1)               # argmax of a 0/1 tensor of ...: the FIRST 1, asserted below


assert first_max(torch.tensor([[1.0, 3.0, 3.0, 3.0], [2.0, 2.0, 1.0, 2.0]])).tolist() == [1, 0]


def mnet_fwd_ref(m, w, b, pick=first_max):
    """-> (out [N, 32], A [N, 32] at the winning step, t* [N, 32])."""
    o, Ao = mnet_steps(m, w, b)
    t = pick(o)
    return o.gather(2, t.unsqueeze(-1)).squeeze(-1), Ao.gather(2, t.unsqueeze(-1)).squeeze(-1), t


def mnet_bwd_ref(m, t, dy):
    """m [N, 16], t [N, 32] winning steps, dy [N, 32] fp64 -> (dW [32, 2, 2], A_dW, dbias [32], A_db)."""
    v = m.view(-1, 2, 4, 2)
    sel = v.permute(0, 2, 1, 3)                                # [N, t2, ch2, kt]
    taken_ = sel.gather(1, t.view(-1, 32, 1, 1).expand(-1, 32, 2, 2))       # [N, 32, ch2, kt]: the winning step's operands
    dyd = dy.view(-1, 32, 1, 1)
    return (dyd * taken_).sum(0), (dyd.abs() * taken_.abs()).sum(0), dy.sum(0), dy.abs().sum(0)


def near_ties(m, w, b):
    """[N] bool: pixels with a (pixel, channel) entry whose best and second-best step are closer than 2^-21 A (A: the largest of the
    four steps' sums of absolute values) — there the arg-max of an fp32 kernel may legitimately differ."""
    o, Ao = mnet_steps(m, w, b)
    top = o.topk(2, dim=-1).values
    return ((top[..., 0] - top[..., 1]) < 2.0 ** -21 * Ao.max(-1).values).any(-1)


def exact_ties(m, w, b):
    """[N, 32] bool: entries where two or more steps reach the maximum exactly."""
    o, _ = mnet_steps(m, w, b)
    return (o == o.max(-1, keepdim=True).values).sum(-1) >= 2


def mnet_weights(name):
    s = seed_of("mnet-" + name)
    return rnd(32, 2, 2, seed=s, scale=0.5), rnd(32, seed=s + 1, scale=0.5)


def draw_mnet(c, device="cpu", chunk=1 << 18):
    """The operands of an MNet case: x [n_bg, 16, pixels, 8] fp32 (multiples of 2^-10 below 4; None where the case is not x-fed: then the
    means themselves are drawn, as multiples of 2^-13 below 4), its exact means as pixel-major m [N, 16] fp32, w, b, dy [N, 32] (bf16-
    representable).  Draws come from a seeded CPU generator; the pixels holding a near-tie are re-drawn until none is left (the
    search runs on `device` in chunks).  -> dict, with "redrawn" the number of pixels drawn again."""
    g = torch.Generator().manual_seed(seed_of("mnet-x-" + c.name))
    N = c.n_bg * c.pixels
    w, b = mnet_weights(c.name)
    wd, bd = w.double().to(device), b.double().to(device)

    def draw(n):                                               # -> (x [n, 16, 8] or None, m [n, 16]), CPU fp32
        if c.x_fed:
            x = torch.randint(-4095, 4096, (n, 16, 8), generator=g).float() * 2.0 ** -10
            return x, x.sum(-1) * 0.125                        # exact: 8 x 13-bit integers, then a power of two
        return None, torch.randint(-32767, 32768, (n, 16), generator=g).float() * 2.0 ** -13

    x, m = draw(N)                                             # pixel-major [N, ...]: pixel index = bg * pixels + pix
    redrawn = 0
    for _ in range(64):
        bad = torch.cat([near_ties(m[i:i + chunk].double().to(device), wd, bd).cpu() for i in range(0, N, chunk)]).nonzero().view(-1)
        if bad.numel() == 0:
            break
        redrawn += bad.numel()
        xn, mn = draw(bad.numel())
        m[bad] = mn
        if x is not None:
            x[bad] = xn
    else:
        raise AssertionError("near-ties left after 64 rounds")
    dy = torch.randn(N, 32, generator=g).to(torch.bfloat16).float() if c.bwd else None
    if x is not None:                                          # [N, 16, 8] -> the kernel's [n_bg, 16, pixels, 8]
        x = x.view(c.n_bg, c.pixels, 16, 8).permute(0, 2, 1, 3).contiguous()
    return {"x": x, "m": m, "w": w, "b": b, "dy": dy, "redrawn": redrawn, "left": int(bad.numel())}


def mnet_planes(m, c):
    """Pixel-major means [N, 16] -> the fused loader's planes [n_bg, 16, pixels]."""
    return m.view(c.n_bg, c.pixels, 16).permute(0, 2, 1).contiguous()


def mnet_within(out, ref, A):
    return (out.double() - ref).abs() <= 2.0 ** -22 * A


def grad_within(d, ref, A, c):
    return (d.double() - ref).abs() <= c * A


MNET_WORST = {}


def mnet_forward(L, c, o, feed, T, with_means):
    """One guarded launch of hupr_mnet_fwd_* (feed "x") or hupr_mnet_fwd_means_* (feed "means"): -> (out [N, 32], means [N, 16] | None)."""
    from hupr_amd import runtime as rt
    N = c.n_bg * c.pixels
    src = o["xbuf"] if feed == "x" else o["pbuf"]
    obuf, optr = placed(None, N, 32, 32, 0, DT[T])
    mbuf, mptr = placed(None, N, 16, 16, 0, torch.float32) if with_means else (None, None)
    fn = getattr(L, "hupr_mnet_fwd%s_%s" % ("" if feed == "x" else "_means", "bf16act" if T == "bf16" else "f32"))
    n0 = L.hupr_launch_count()
    rc = fn(src.data_ptr(), o["wd"].data_ptr(), o["bd"].data_ptr(), optr, mptr, c.n_bg, c.pixels, rt.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.hupr_last_error()
    assert L.hupr_launch_count() - n0 == 1
    what = "%s %s-fed %s" % (c.name, feed, T)
    return taken(obuf, N, 32, 32, 0, what), (taken(mbuf, N, 16, 16, 0, what + " means") if with_means else None)


def mnet_backward(L, c, o, feed, T, ws_short=0, both_null=False):
    """One guarded launch of hupr_mnet_bwd_*: -> (rc, dW [32, 2, 2], dbias [32], their buffers)."""
    from hupr_amd import runtime as rt
    nbytes = L.hupr_mnet_bwd_ws_bytes()
    assert nbytes == 1024 * 160 * 4
    ws = nan_buffer(nbytes // 4 + GUARD, torch.float32)
    wbuf, wptr = placed(None, 1, 128, 128, 0, torch.float32)
    bbuf, bptr = placed(None, 1, 32, 32, 0, torch.float32)
    dy = o["dy16"] if T == "bf16" else o["dy32"]
    xp = None if (feed == "means" or both_null) else o["xbuf"].data_ptr()
    mp = None if (feed == "x" or both_null) else o["mbuf"].data_ptr()
    fn = getattr(L, "hupr_mnet_bwd_" + ("bf16act" if T == "bf16" else "f32"))
    rc = fn(xp, mp, o["wd"].data_ptr(), o["bd"].data_ptr(), dy.data_ptr(), wptr, bptr, c.n_bg, c.pixels, ws.data_ptr(), nbytes - ws_short,
            rt.stream())
    torch.cuda.synchronize()
    assert bool((bits(ws[nbytes // 4:]) == NAN32).all()), "the guard past the workspace was written"
    return rc, wbuf, bbuf


@functools.lru_cache(maxsize=2)
def mnet_device_operands(name):
    (c,) = [c for c in MCASES + [TIE_CASE] if c.name == name]
    o = draw_ties() if c is TIE_CASE else draw_mnet(c, "cuda")
    N = c.n_bg * c.pixels
    o["xbuf"] = padded(o["x"].view(-1, 8), 8, torch.float32) if o["x"] is not None else None
    o["pbuf"] = padded(mnet_planes(o["m"], c).view(-1, 1), 1, torch.float32)
    o["mbuf"] = padded(o["m"], 16, torch.float32)
    o["wd"], o["bd"] = o["w"].cuda().contiguous(), o["b"].cuda().contiguous()
    if o["dy"] is not None:
        o["dy32"], o["dy16"] = padded(o["dy"], 32, torch.float32), padded(o["dy"], 32, torch.bfloat16)
    md = o["m"].cuda().double()
    o["ref"] = mnet_fwd_ref(md, o["wd"].double(), o["bd"].double())
    assert not bool(near_ties(md, o["wd"].double(), o["bd"].double()).any()) or c is TIE_CASE
    return o


@pytest.mark.parametrize("c", MCASES, ids=[c.name for c in MCASES])
def test_mnet_forward_forms_match_fp64(c, lib):
    """x-fed and means-fed, fp32 and bf16act, with and without the means output: the grids the table names; the means bit-equal to the
    reference's; every fp32 form inside the gate and bit-equal to the others; every bf16 form the nearest-even rounding of it."""
    g = mnet_grids(lib, c)
    assert g[1] == c.g_means and (not c.x_fed or g[0] == c.g_fwd)
    o = mnet_device_operands(c.name)
    ref, A, _ = o["ref"]
    m_bits = bits(o["m"].cuda())
    first = None
    for feed in (("x", "means") if c.x_fed else ("means",)):
        for with_means in (True, False):
            out, means = mnet_forward(lib, c, o, feed, "f32", with_means)
            if with_means:
                assert torch.equal(bits(means), m_bits), "%s %s-fed: the means output is not the exact mean" % (c.name, feed)
            assert_all(mnet_within(out, ref, A), out, ref, A, "%s %s-fed f32" % (c.name, feed))
            first = out if first is None else first
            assert torch.equal(bits(out), bits(first)), "%s: the %s-fed form differs (means output %s)" % (c.name, feed, with_means)
            out16, means = mnet_forward(lib, c, o, feed, "bf16", with_means)
            if with_means:
                assert torch.equal(bits(means), m_bits)
            assert torch.equal(bits(out16), bits(first.to(torch.bfloat16))), "%s %s-fed bf16: not the rounding of the fp32 form" % (c.name, feed)


BWD_CASES = [c for c in MCASES if c.bwd]


@pytest.mark.parametrize("c", BWD_CASES, ids=[c.name for c in BWD_CASES])
def test_mnet_backward_feeds_match_fp64(c, lib):
    """dW and dbias from the means and from x, fp32 and bf16 dy (the same bf16-representable values): the grid the table names, a
    workspace of exactly hupr_mnet_bwd_ws_bytes() with a guard, both feeds bit-equal, every result inside c A_d."""
    assert mnet_grids(lib, c)[2] == c.g_bwd
    o = mnet_device_operands(c.name)
    _, _, t = o["ref"]
    dw_ref, dw_A, db_ref, db_A = mnet_bwd_ref(o["m"].cuda().double(), t, o["dy"].cuda().double())
    first = None
    for feed in ("means", "x"):
        for T in BOTH:
            n0 = lib.hupr_launch_count()
            rc, wbuf, bbuf = mnet_backward(lib, c, o, feed, T)
            assert rc == 0, lib.hupr_last_error()
            assert lib.hupr_launch_count() - n0 == 2
            what = "%s backward from %s, %s dy" % (c.name, feed, T)
            dw, db = taken(wbuf, 1, 128, 128, 0, what).view(32, 2, 2), taken(bbuf, 1, 32, 32, 0, what).view(32)
            for key, d, r, A in (("dw", dw, dw_ref, dw_A), ("db", db, db_ref, db_A)):
                worst = ((d.double() - r).abs() / A).nan_to_num(float("inf")).max().item()
                MNET_WORST[(key, feed)] = max(MNET_WORST.get((key, feed), 0.0), worst)
                print("mnet fp64: %-52s %s worst err / A_d %.3g = 2^%.2f" % (what, key, worst, torch.log2(torch.tensor(worst)).item()))
                assert_all(grad_within(d, r, A, MNET_C[key]), d, r, A, what + " " + key)
            first = (dw, db) if first is None else first
            assert torch.equal(bits(dw), bits(first[0])) and torch.equal(bits(db), bits(first[1])), what + ": differs from the first form"


def test_mnet_backward_refusals(lib):
    """One byte of workspace fewer: HUPR_ERR_WORKSPACE; x and means both null: HUPR_ERR_ARG; dW and dbias keep the NaN pattern."""
    c = MCASES[0]
    o = mnet_device_operands(c.name)
    for T in BOTH:
        for kw, want in (({"ws_short": 1}, HUPR_ERR_WORKSPACE), ({"both_null": True}, HUPR_ERR_ARG)):
            n0 = lib.hupr_launch_count()
            rc, wbuf, bbuf = mnet_backward(lib, c, o, "means", T, **kw)
            assert rc == want, (T, kw, rc)
            assert lib.hupr_launch_count() == n0
            assert bool((bits(wbuf) == NAN32).all()) and bool((bits(bbuf) == NAN32).all())


# ---- exact ties ---------------------------------------------------------------------------------------------------------------------------
TIE_CASE = MCase("exact-ties", 3, 50, True, True, 1, 1, 3)
TIE_SHARE = 0.25


def draw_ties():
    """Small-integer means (every elevation holds the mean itself), weights in {-1, 0, 1}, integer bias and dy: every step value and
    every gradient sum is a small integer, exact in fp32 in any order, and steps tie exactly in a large share of the entries."""
    c = TIE_CASE
    g = torch.Generator().manual_seed(seed_of("mnet-ties"))
    N = c.n_bg * c.pixels
    m = torch.randint(-1, 2, (N, 16), generator=g).float()
    x = m.view(c.n_bg, c.pixels, 16, 1).expand(-1, -1, -1, 8).permute(0, 2, 1, 3).contiguous()
    w = torch.randint(-1, 2, (32, 2, 2), generator=g).float()
    b = torch.randint(-3, 4, (32,), generator=g).float()
    dy = torch.randint(-4, 5, (N, 32), generator=g).float()
    return {"x": x, "m": m, "w": w, "b": b, "dy": dy, "redrawn": 0, "left": 0}


def tie_torch64(o):
    """F.conv3d + F.max_pool3d + autograd in float64 on the CPU (max_pool3d hands the gradient to the first maximum) of the tie case:
    -> (out [N, 32], dW [32, 2, 2], dbias [32])."""
    c = TIE_CASE
    w = o["w"].double().view(32, 2, 2, 1, 1).requires_grad_(True)
    b = o["b"].double().requires_grad_(True)
    v = mnet_planes(o["m"], c).double().view(c.n_bg, 2, 8, c.pixels, 1)           # the .view: 16 planes -> (ch2, t)
    y = F.max_pool3d(F.conv3d(v, w, b, (2, 1, 1)), (4, 1, 1), (4, 1, 1)).view(c.n_bg, 32, c.pixels)
    y.backward(o["dy"].double().view(c.n_bg, c.pixels, 32).permute(0, 2, 1))
    return y.detach().permute(0, 2, 1).reshape(-1, 32), w.grad.view(32, 2, 2), b.grad


def test_exact_ties_go_to_the_first_maximum(lib):
    c = TIE_CASE
    assert mnet_grids(lib, c) == (c.g_fwd, c.g_means, c.g_bwd)
    o = mnet_device_operands(c.name)
    cpu = {k: o[k] for k in ("m", "w", "b", "dy")}
    share = exact_ties(cpu["m"].double(), cpu["w"].double(), cpu["b"].double()).float().mean().item()
    assert share >= TIE_SHARE, share
    ref, _, t = mnet_fwd_ref(cpu["m"].double(), cpu["w"].double(), cpu["b"].double())
    dw_ref, _, db_ref, _ = mnet_bwd_ref(cpu["m"].double(), t, cpu["dy"].double())
    y64, dw64, db64 = tie_torch64(cpu)
    assert torch.equal(ref, y64) and torch.equal(dw_ref, dw64) and torch.equal(db_ref, db64)
    for feed in ("x", "means"):
        for T in BOTH:
            out, _ = mnet_forward(lib, c, o, feed, T, True)
            assert torch.equal(out.cpu().double(), ref), (feed, T)         # (small integers: exact in bf16 too)
            rc, wbuf, bbuf = mnet_backward(lib, c, o, feed, T)
            assert rc == 0, lib.hupr_last_error()
            dw, db = taken(wbuf, 1, 128, 128, 0, "ties dW").view(32, 2, 2), taken(bbuf, 1, 32, 32, 0, "ties dbias").view(32)
            assert torch.equal(dw.cpu().double(), dw_ref), (feed, T)
            assert torch.equal(db.cpu().double(), db_ref), (feed, T)


@pytest.mark.parametrize("rank", [7, 5])
@pytest.mark.parametrize("T", BOTH)
def test_mnet_node_calls_each_entry_once(T, rank, lib):
    """MNetFn fed by x (B, G, 8, 2, R, A, 8) and by mean planes (B, G, 16, R, A), fp32 and bf16 output: one forward and one backward
    entry call; output, dW and dbias inside the gates."""
    from hupr_amd import functional as F_
    c = MCASES[1]
    o = mnet_device_operands(c.name)
    B, G, R, A_ = 1, 5, 7, 9
    assert (B * G, R * A_) == (c.n_bg, c.pixels)
    src = o["x"].view(B, G, 8, 2, R, A_, 8).cuda() if rank == 7 else mnet_planes(o["m"], c).view(B, G, 16, R, A_).cuda()
    w = o["w"].view(32, 2, 2, 1, 1).cuda().requires_grad_(True)
    b = o["b"].cuda().requires_grad_(True)
    stem = "hupr_mnet_fwd%s_%s" % ("" if rank == 7 else "_means", "bf16act" if T == "bf16" else "f32")
    with Counted(lib) as n:
        y = F_.MNetFn.apply(src, w, b, DT[T])
        assert n.take() == {stem: 1}
        y.backward(o["dy"].view(B, G, R, A_, 32).to(DT[T]).cuda())
        assert n.take() == {"hupr_mnet_bwd_ws_bytes": 1, "hupr_mnet_bwd_" + ("bf16act" if T == "bf16" else "f32"): 1}
    torch.cuda.synchronize()
    ref, A, t = o["ref"]
    got = y.detach().reshape(-1, 32)
    assert y.dtype == DT[T]
    if T == "bf16":
        assert_all((got.double() - ref).abs() <= 2.0 ** -22 * A + 2.0 ** -8 * ref.abs(), got, ref, A, "MNetFn forward")
    else:
        assert_all(mnet_within(got, ref, A), got, ref, A, "MNetFn forward")
    dw_ref, dw_A, db_ref, db_A = mnet_bwd_ref(o["m"].cuda().double(), t, o["dy"].cuda().double())
    assert_all(grad_within(w.grad.view(32, 2, 2), dw_ref, dw_A, MNET_C["dw"]), w.grad.view(32, 2, 2), dw_ref, dw_A, "MNetFn dW")
    assert_all(grad_within(b.grad, db_ref, db_A, MNET_C["db"]), b.grad, db_ref, db_A, "MNetFn dbias")
