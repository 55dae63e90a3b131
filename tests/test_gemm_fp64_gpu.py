"""GPU (-m gpu): every form of the two GEMM engines (csrc/gemm_f32.hip, csrc/gemm_bf16.hip: batched GEMM in three operand modes, forward
convolution / input gradient, the batched input gradient of a temporal merge, split-K weight gradient with its four reduce kernels,
weight packing) and of the streaming MSCSA
projections (csrc/projection.hip) against an fp64 reference of exactly the operands the kernel multiplies, element by element, with
the route of every launch asserted first from the library's own plan (hupr_debug_gemm_route, hupr_debug_mscsa_proj_grid: the host
functions the launchers themselves call) against the literal in the case table.

Reference: the fp32 engine multiplies the fp32 values; the bf16 engine and the projections round both operands to bf16 (nearest
even), so the reference is the fp64 sum over the rounded values (operands stored as bf16 are drawn bf16-representable).  A is the
same sum over absolute values, with |bias|, |res| and the old |C| of an accumulate added.  Convolutions, input gradients and weight
gradients are explicit fp64 sums over taps of shifted slices (zero outside), computed on the device.

Gate (``within``): fp32 output |out - ref| <= c A; bf16-stored output |out - ref| <= 2^-8 |ref| + c A; a NaN never passes.  c per
(engine, operation) (GATE_C) is the smallest power of two that is at least 8 x the worst err / A measured over this table against
fp64 on an MI355X, never above 2^-16; the 8 x is room for legitimate changes of tile and slot order.  Behind a bf16 store the
measured figure is the part of the error the store cannot explain (``measured``, as in test_tmerge_fp64_gpu.py).  Measured worst
values per (engine, operation, route):

    engine operation    route: worst err / A                                                                     8 x worst   c
    f32    gemm         128x128 2^-21.37  64x128 2^-21.42  128x64 2^-21.23  64x64 2^-21.52  128x32 2^-21.46     2^-18.23    2^-18
    bf16   gemm         128x128 2^-22.59  64x128 2^-22.58  128x64 2^-22.63  64x64 2^-22.69                      2^-19.58    2^-19
    f32    conv / dgrad 128x128 2^-21.56  64x128 2^-21.63  128x64 2^-21.67  64x64 2^-21.68  128x32 2^-21.98     2^-18.56    2^-18
    bf16   conv / dgrad 128x128 2^-22.97  64x128 2^-23.45  128x64 2^-23.13  64x64 2^-23.04                      2^-19.97    2^-19
    f32    wgrad        reduce_t bm64 2^-22.23, bm128 2^-22.24  reduce4<4> 2^-23.25  reduce4<16> 2^-25.23
                        scalar 2^-23.16                                                                          2^-19.23    2^-19
    bf16   wgrad        reduce_t 2^-23.60  reduce4<4> bm64 2^-24.84, bm128 2^-23.94  reduce4<16> bm64 2^-26.40,
                        bm128 2^-26.33  scalar 2^-25.14                                                          2^-20.60    2^-20
    bf16   proj fwd     C64 one step 2^-25.12, wrapping 2^-24.43  C128 one step 2^-25.00, wrapping 2^-24.70      2^-21.43    2^-21
    bf16   proj dgrad   C64 one step 2^-23.13, wrapping 2^-23.11                                                 2^-20.11    2^-20

(The fp32 engine's figures are the fp32 rounding of its own long sums — up to 1 728 terms in one MFMA chain —, the bf16 engine's
products are exact and only the fp32 accumulation shows; the many-slice weight gradients sum short chains and are the most accurate.
No route needs more than 2^-18: all are far inside the 2^-16 cap.)

Every output is a slice inside a NaN-pattern buffer between guards; every operand has NaN padding columns and NaN guards around it;
the workspace has exactly the bytes the library asks for (or the case names), pre-filled with the NaN pattern and followed by a guard;
guards and padding must come back bit-identical, no output element may stay NaN, and a second launch into fresh buffers must give the
same bits.  The exact cases use small integers or one-hot rows (bf16-exact, sums exact in fp32): the output must equal the fp64
reference bit for bit, so a slip in a transpose, tap order, tap reversal, LDS swizzle, lane pairing or MFMA output mapping is an exact
mismatch.

hupr_debug_splitk_slices: forcing the slice class the automatic choice takes (4 or 16), with or without the scattered-store kernel
(+ 256), must give the bits of the automatic choice on the same partials; the other class sums the same partials in another order (it
is inside the gate, and bit-identical too where there are at most four partial tensors: both then add them in index order).

tests/test_gemm_route.py checks the routes of these tables, their coverage, the model's own shapes and the refusals without a GPU,
and that the gates reject the results of subtly wrong kernels."""
import collections
import ctypes
import functools
import math

import pytest
import torch

from test_conv_halo_fp64_gpu import GUARD, NAN16, NAN32, bits, nan_buffer, rnd

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG, HUPR_ERR_WORKSPACE = -1, -2
CAP = 2.0 ** -16                                       # the project's gate of an fp32-output convolution
ENGINES = ("f32", "bf16")
GATE_C = {("f32", "gemm"): 2.0 ** -18, ("bf16", "gemm"): 2.0 ** -19, ("f32", "conv"): 2.0 ** -18, ("bf16", "conv"): 2.0 ** -19,
          ("f32", "wgrad"): 2.0 ** -19, ("bf16", "wgrad"): 2.0 ** -20, ("bf16", "proj_fwd"): 2.0 ** -21, ("bf16", "proj_dgrad"): 2.0 ** -20}
SCALAR, REDUCE4_4, REDUCE4_16, REDUCE_T = range(4)      # reduce kernels of hupr_debug_gemm_route


# ---- the library's plan ----------------------------------------------------------------------------------------------------------
def plan(L, engine, op, v, ws_bytes=0, misalign=0):
    """hupr_debug_gemm_route: the six answers, or the error code."""
    a = (ctypes.c_int * len(v))(*v)
    o = (ctypes.c_int * 6)()
    rc = L.hupr_debug_gemm_route(ENGINES.index(engine), op, a, ws_bytes, misalign, o)
    return rc if rc else tuple(o)


def proj_grid(L, op, M, C):
    o = (ctypes.c_int * 3)()
    rc = L.hupr_debug_mscsa_proj_grid(op, M, C, o)
    return rc if rc else tuple(o)


def vox(d):
    return d[0] * d[1] * d[2]


def out_extent(din, k, pad):
    return tuple(i + 2 * p - t + 1 for i, t, p in zip(din, k, pad))


# ---- batched GEMM: the case table --------------------------------------------------------------------------------------------------
# (M, N, batch, tile of the fp32 engine, tile of the bf16 engine): every tile of dispatch_tiles / dispatch_h, the 512-workgroup
# threshold reached through the batch from below and at it, N = 64 / 65 and 32 / 33, M = 64 / 65, several tiles per batch item
TILE_SHAPES = [(72, 72, 512, (128, 128), (128, 128)), (72, 72, 511, (64, 128), (64, 128)), (72, 72, 3, (64, 128), (64, 64)),
               (40, 72, 512, (64, 128), (64, 128)), (40, 72, 511, (64, 128), (64, 64)),
               (72, 40, 512, (128, 64), (128, 64)), (72, 40, 511, (64, 64), (64, 64)), (72, 40, 3, (64, 64), (64, 64)),
               (72, 20, 512, (128, 32), (128, 64)), (70, 22, 3, (128, 32), (64, 64)),
               (65, 65, 512, (128, 128), (128, 128)), (64, 65, 512, (64, 128), (64, 128)), (65, 64, 512, (128, 64), (128, 64)),
               (65, 33, 512, (128, 64), (128, 64)), (65, 32, 512, (128, 32), (128, 64)), (64, 64, 512, (64, 64), (64, 64)),
               (130, 131, 1, (64, 128), (64, 64)), (201, 150, 128, (128, 128), (128, 128)), (133, 30, 256, (128, 32), (128, 64))]
MODES = ((0, 1), (0, 0), (1, 0))                        # C = A B^T, A B, A^T B
K_LIST = (1, 3, 31, 32, 33, 40, 64, 65, 128, 7, 130)    # K = 1, K % 4 != 0, below / at / one past / a multiple of a K tile (32 and 64)
PADS = ((0, 0, 0, 0), (4, 8, 4, 8), (1, 3, 1, 3), (3, 1, 0, 1), (0, 0, 3, 0))      # lda, ldb, ldc, res_ld beyond the dense extent
EPIS = ("", "res", "acc", "res acc")
GCase = collections.namedtuple("GCase", "ta tb M N K batch pads epi bcast tile")


def _gemm_cases():
    cases, i = [], 0
    for M, N, batch, t32, t16 in TILE_SHAPES:
        for ta, tb in MODES:
            cases.append(GCase(ta, tb, M, N, K_LIST[i % 11], batch, PADS[(i // 2) % 5], EPIS[(i // 3) % 4], i % 7 == 1,
                               {"f32": t32, "bf16": t16}))
            i += 1
    return cases


GEMM_CASES = _gemm_cases()


def gemm_id(c):
    return "%s-%dx%dx%d-b%d-ld%d.%d.%d.%d-%s%s" % ("NT" if c.tb else ("TN" if c.ta else "NN"), c.M, c.N, c.K, c.batch, *c.pads,
                                                   c.epi.replace(" ", "+") or "plain", "-bcast" if c.bcast else "")


def gemm_lds(c):
    """(rows of A, rows of B, lda, ldb, ldc, res_ld)."""
    ra, ca = (c.M, c.K) if c.ta == 0 else (c.K, c.M)
    rb, cb = (c.N, c.K) if c.tb == 1 else (c.K, c.N)
    return ra, rb, ca + c.pads[0], cb + c.pads[1], c.N + c.pads[2], c.N + c.pads[3]


def gemm_expected(c, engine):
    bm, bn = c.tile[engine]
    return bm, bn, -(-c.M // bm) * -(-c.N // bn), c.batch, 0, 0


def gemm_plan_of(L, c, engine):
    return plan(L, engine, 0, [c.ta, c.tb, c.M, c.N, c.K, c.batch])


# ---- convolutions: the case tables ------------------------------------------------------------------------------------------------
# eng: the engine; din: the forward input extents; lds: (in_ld - Ci, channel offset of x in its rows, out_ld - Co, channel offset of y,
# res_ld - Co); epi: bias / res / acc / inplace (y written over the residual); store: "" the plain entry point, else the _mixed one with
# "x16" / "y16" (stored as bf16) or "f32" (neither); dgrad: the input gradient — the same entry point on mode-1 weights with pad
# k - 1 - p, dy (extents of the forward output, Co channels) in, dx (din, Ci channels) out; tile: the literal (BM, BN).
CCase = collections.namedtuple("CCase", "name eng B din Ci Co k pad lds epi store dgrad tile")
DENSE = (0, 0, 0, 0, 0)
K333, K133, K111 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
SAME3, NOPAD = (1, 1, 1), (0, 0, 0)


def _conv_cases():
    c = []
    for eng, ca, cb, v in (("f32", 32, 64, 4), ("bf16", 8, 24, 8)):       # the input channels of the engine; v: channels per 16 bytes of x
        small = (128, 32) if eng == "f32" else (64, 64)
        wide = (64, 128) if eng == "f32" else (64, 64)
        big = (64, 128)
        c += [
            CCase("333-same", eng, 2, (3, 5, 7), ca, 16, K333, SAME3, DENSE, "", "", False, small),
            CCase("333-nopad-strided", eng, 1, (5, 6, 7), cb, 20, K333, NOPAD, (v, v, 4, 4, 8), "bias", "", False, small),
            CCase("333-pad-hw", eng, 2, (4, 5, 7), ca, 40, K333, (0, 1, 1), (2 * v, 0, 8, 0, 3), "res", "", False, (64, 64)),
            CCase("133-ragged63", eng, 1, (1, 7, 9), cb, 72, K133, (0, 1, 1), (v, 0, 1, 0, 5), "bias res acc", "", False, wide),
            CCase("G11", eng, 2, (4, 5, 7), ca, 16, (4, 1, 1), NOPAD, (0, 0, 4, 4, 0), "acc", "", False, small),
            CCase("111-inplace", eng, 1, (1, 7, 9), ca, 20, K111, NOPAD, (v, v, 4, 0, 4), "bias inplace", "", False, small),
            CCase("111-inplace-odd-ld", eng, 2, (3, 5, 7), cb, 40, K111, NOPAD, (0, 0, 3, 0, 3), "inplace", "", False, (64, 64)),
            CCase("333-d1023", eng, 1, (1023, 1, 2), ca, 16, K333, SAME3, DENSE, "bias", "", False, small),
            CCase("333-h1023", eng, 1, (2, 1023, 1), ca, 20, K333, SAME3, (0, 0, 1, 0, 0), "res", "", False, small),
            CCase("133-w1023", eng, 1, (1, 2, 1023), ca, 40, K133, (0, 1, 1), DENSE, "", "", False, (64, 64)),
            # the 128-row tiles: 512 workgroups of 128 rows at 65 536 and 65 535 voxels, 511 at 65 408
            CCase("111-65536-co72", eng, 1, (1, 256, 256), ca, 72, K111, NOPAD, DENSE, "bias", "", False, (128, 128)),
            CCase("111-65535-co72", eng, 1, (1, 255, 257), ca, 72, K111, NOPAD, DENSE, "res", "", False, (128, 128)),
            CCase("111-65408-co72", eng, 1, (1, 224, 292), ca, 72, K111, NOPAD, DENSE, "", "", False, big),
            CCase("111-65536-co40", eng, 1, (1, 256, 256), ca, 40, K111, NOPAD, DENSE, "acc", "", False, (128, 64)),
            CCase("111-65408-co40", eng, 1, (1, 224, 292), ca, 40, K111, NOPAD, DENSE, "bias", "", False, (64, 64)),
            # input gradients (Co plays the engine's input channels)
            CCase("333-same-dgrad", eng, 2, (3, 5, 7), 16, ca, K333, SAME3, DENSE, "", "", True, small),
            CCase("333-nopad-dgrad", eng, 1, (5, 6, 7), 20, cb, K333, NOPAD, (v, 0, 4, 0, 0), "", "", True, small),
            CCase("133-dgrad", eng, 2, (1, 7, 9), 40, cb, K133, (0, 1, 1), DENSE, "res", "", True, (64, 64)),
            CCase("G11-dgrad", eng, 2, (4, 5, 7), 72, ca, (4, 1, 1), NOPAD, DENSE, "", "", True, wide),
        ]
    # the _mixed entry point (bf16 engine): x stored as bf16, y stored as bf16, both, neither
    c += [CCase("mixed-x16", "bf16", 2, (3, 5, 7), 8, 20, K333, SAME3, (8, 8, 4, 4, 0), "bias", "x16", False, (64, 64)),
          CCase("mixed-y16", "bf16", 2, (3, 5, 7), 24, 20, K133, (0, 1, 1), (8, 0, 4, 4, 0), "bias", "y16", False, (64, 64)),
          CCase("mixed-y16-odd-ld", "bf16", 1, (1, 7, 9), 8, 18, K111, NOPAD, (0, 0, 3, 0, 0), "", "y16", False, (64, 64)),
          CCase("mixed-x16-y16", "bf16", 1, (4, 5, 7), 24, 72, (4, 1, 1), NOPAD, (8, 8, 8, 8, 0), "", "x16 y16", False, (64, 64)),
          CCase("mixed-x16-y16-65536", "bf16", 1, (1, 256, 256), 8, 72, K111, NOPAD, DENSE, "bias", "x16 y16", False, (128, 128)),
          CCase("mixed-f32", "bf16", 2, (3, 5, 7), 8, 40, K333, NOPAD, DENSE, "", "f32", False, (64, 64)),
          CCase("mixed-x16-dgrad", "bf16", 2, (3, 5, 7), 16, 8, K333, SAME3, (8, 0, 0, 0, 0), "", "x16", True, (64, 64))]
    return c


CONV_CASES = _conv_cases()


def conv_id(c):
    return "%s-%s" % (c.eng, c.name)


def conv_call_geometry(c):
    """The call as the entry point sees it: (input extents, input channels, output extents, output channels, pad)."""
    dout = out_extent(c.din, c.k, c.pad)
    if c.dgrad:
        return dout, c.Co, c.din, c.Ci, tuple(t - 1 - p for t, p in zip(c.k, c.pad))
    return c.din, c.Ci, dout, c.Co, c.pad


def conv_entry(c):
    if c.eng == "f32":
        return "hupr_conv_fwd_f32"
    return "hupr_conv_fwd_bf16_mixed" if c.store else "hupr_conv_fwd_bf16"


def conv_route_args(c):
    i_ext, ci, o_ext, co, pad = conv_call_geometry(c)
    return [c.B, *i_ext, ci, ci + c.lds[0], *o_ext, co, *c.k, *pad, int("x16" in c.store), int("y16" in c.store), int("acc" in c.epi),
            int("res" in c.epi or "inplace" in c.epi)]


def conv_expected(c):
    _, _, o_ext, co, _ = conv_call_geometry(c)
    bm, bn = c.tile
    return bm, bn, -(-c.B * vox(o_ext) // bm) * -(-co // bn), 1, 0, 0


# eng, lds: (in_ld - Ci, dy_ld - Co); xbf: x stored as bf16 (the _mixed entry); ws: "lib" (hupr_conv_wgrad_ws_bytes), ("parts", n) n
# partial tensors, ("misalign", n) the library's bytes behind a pointer 4 bytes off; route: the literal (BM, grid.x, slices, reduce
# kernel, its workgroups); why: the cap that sets the slice count.
WCase = collections.namedtuple("WCase", "name eng B din Ci Co k pad lds xbf ws route why")


def _wgrad_cases():
    return [
        # ---- fp32 engine: 32-deep K tiles, Ci % 32 == 0
        WCase("333-ktiles7", "f32", 2, (3, 5, 7), 32, 16, K333, SAME3, (0, 0), 0, "lib", (64, 7, 7, REDUCE_T, 16), "ktiles"),
        WCase("133-bm128-odd-dy", "f32", 1, (1, 7, 9), 64, 65, K133, (0, 1, 1), (4, 2), 0, "lib", (128, 5, 2, REDUCE_T, 130), "ktiles"),
        WCase("111-co64", "f32", 1, (1, 7, 9), 32, 64, K111, NOPAD, (4, 4), 0, "lib", (64, 1, 2, REDUCE4_4, 8), "ktiles"),
        WCase("333-nopad-co18", "f32", 1, (5, 6, 7), 32, 18, K333, NOPAD, (0, 1), 0, "lib", (64, 7, 2, REDUCE_T, 18), "ktiles"),
        WCase("G11-3slices", "f32", 1, (4, 8, 12), 32, 20, (4, 1, 1), NOPAD, (0, 0), 0, "lib", (64, 1, 3, REDUCE_T, 20), "ktiles"),
        WCase("111-33slices", "f32", 1, (1, 32, 33), 32, 16, K111, NOPAD, (0, 0), 0, "lib", (64, 1, 33, REDUCE4_16, 8), "ktiles"),
        WCase("111-256", "f32", 1, (16, 32, 32), 32, 16, K111, NOPAD, (0, 0), 0, "lib", (64, 1, 256, REDUCE4_16, 8), "256"),
        WCase("333-1024/tiles", "f32", 2, (8, 16, 32), 32, 64, K333, SAME3, (0, 0), 0, "lib", (64, 7, 147, REDUCE4_16, 864), "1024/tiles"),
        WCase("133-tiles2x3", "f32", 2, (1, 16, 16), 32, 130, K133, (0, 1, 1), (0, 0), 0, "lib", (128, 6, 16, REDUCE_T, 130), "ktiles"),
        WCase("111-empty-slice", "f32", 1, (1, 11, 25), 32, 16, K111, NOPAD, (0, 0), 0, ("parts", 4), (64, 1, 4, REDUCE4_4, 2), "shrink"),
        WCase("133-empty-slice", "f32", 1, (1, 12, 24), 32, 16, K133, (0, 1, 1), (0, 0), 0, ("parts", 4), (64, 3, 4, REDUCE_T, 16), "shrink"),
        WCase("333-shrink-to-1", "f32", 2, (3, 5, 7), 32, 16, K333, SAME3, (0, 0), 0, ("parts", 1), (64, 7, 1, REDUCE_T, 16), "shrink"),
        WCase("333-shrink-to-3", "f32", 2, (3, 5, 7), 32, 16, K333, SAME3, (0, 0), 0, ("parts", 3), (64, 7, 3, REDUCE_T, 16), "shrink"),
        WCase("111-shrink-to-2", "f32", 1, (1, 11, 25), 32, 16, K111, NOPAD, (0, 0), 0, ("parts", 3), (64, 1, 2, REDUCE4_4, 2), "shrink"),
        WCase("333-scalar", "f32", 2, (3, 5, 7), 32, 16, K333, SAME3, (0, 0), 0, ("misalign", 4), (64, 7, 7, SCALAR, 54), "ktiles"),
        WCase("111-scalar", "f32", 1, (1, 7, 9), 32, 64, K111, NOPAD, (0, 0), 0, ("misalign", 4), (64, 1, 2, SCALAR, 8), "ktiles"),
        # ---- bf16 engine: 64-deep K tiles, Ci % 4 == 0, the in-bytes cap and its floor
        WCase("333-ci8", "bf16", 2, (3, 5, 7), 8, 16, K333, SAME3, (4, 0), 0, "lib", (64, 2, 4, REDUCE4_4, 14), "ktiles"),
        WCase("133-ci24-bm128-odd-dy", "bf16", 1, (1, 7, 9), 24, 65, K133, (0, 1, 1), (0, 2), 0, "lib", (128, 2, 1, REDUCE4_4, 55), "ktiles"),
        WCase("333-ci32-x16", "bf16", 2, (3, 5, 7), 32, 18, K333, NOPAD, (8, 1), 1, "lib", (64, 7, 1, REDUCE_T, 18), "ktiles"),
        WCase("111-33slices", "bf16", 1, (2, 32, 33), 32, 16, K111, NOPAD, (0, 0), 0, "lib", (64, 1, 33, REDUCE4_16, 8), "ktiles"),
        WCase("111-256", "bf16", 1, (16, 32, 32), 32, 16, K111, NOPAD, (0, 0), 0, "lib", (64, 1, 256, REDUCE4_16, 8), "256"),
        WCase("333-1024/tiles", "bf16", 4, (8, 32, 32), 32, 64, K333, SAME3, (0, 0), 0, "lib", (64, 7, 147, REDUCE4_16, 864), "1024/tiles"),
        WCase("111-in-bytes-cap", "bf16", 8, (1, 32, 32), 256, 1024, K111, NOPAD, (0, 0), 0, "lib", (128, 16, 20, REDUCE4_4, 1024), "cap"),
        WCase("111-in-bytes-cap-x16", "bf16", 8, (1, 32, 32), 256, 1024, K111, NOPAD, (0, 0), 1, "lib", (128, 16, 18, REDUCE4_4, 1024), "cap"),
        WCase("111-cap-floor", "bf16", 8, (1, 32, 32), 256, 256, K111, NOPAD, (0, 0), 0, "lib", (128, 4, 64, REDUCE4_16, 1024), "floor"),
        WCase("111-empty-slice", "bf16", 1, (1, 22, 25), 32, 16, K111, NOPAD, (0, 0), 0, ("parts", 4), (64, 1, 4, REDUCE4_4, 2), "shrink"),
        WCase("133-ci8-scalar", "bf16", 2, (1, 16, 16), 8, 20, K133, (0, 1, 1), (0, 0), 0, ("misalign", 4), (64, 1, 8, SCALAR, 6), "ktiles"),
        WCase("G11-x16", "bf16", 3, (4, 16, 16), 64, 64, (4, 1, 1), NOPAD, (0, 0), 1, "lib", (64, 2, 12, REDUCE_T, 128), "ktiles"),
    ]


WGRAD_CASES = _wgrad_cases()


def wgrad_id(c):
    return "%s-%s" % (c.eng, c.name)


def wgrad_entry(c):
    return "hupr_conv_wgrad_f32" if c.eng == "f32" else ("hupr_conv_wgrad_bf16_mixed" if c.xbf else "hupr_conv_wgrad_bf16")


def wgrad_ws(L, c):
    """(bytes handed to the call, byte offset of the pointer)."""
    dout = out_extent(c.din, c.k, c.pad)
    lib_bytes = L.hupr_conv_wgrad_ws_bytes(c.B, *dout, c.Ci, c.Co, *c.k)
    if c.ws == "lib":
        return lib_bytes, 0
    if c.ws[0] == "parts":
        return c.ws[1] * c.Co * vox(c.k) * c.Ci * 4, 0
    return lib_bytes, c.ws[1]


def wgrad_route_args(c):
    dout = out_extent(c.din, c.k, c.pad)
    return [c.B, *c.din, c.Ci, c.Ci + c.lds[0], *dout, c.Co, *c.k, *c.pad, c.xbf]


def wgrad_plan_of(L, c):
    nbytes, off = wgrad_ws(L, c)
    return plan(L, c.eng, 2, wgrad_route_args(c), nbytes, off)


def wgrad_expected(c):
    return c.route + (c.route[2] * c.Co * vox(c.k) * c.Ci * 4,)


# ---- projections ------------------------------------------------------------------------------------------------------------------
# (op, C, M, (threads, row groups, column blocks)): 16, 17, 31 rows; one full step and one row past it; the last non-wrapping count;
# an uneven wrap whose last wave is partial and the same wrap with whole waves
PCase = collections.namedtuple("PCase", "op C M grid res")


def _proj_cases():
    c = []
    for M in (16, 17, 31, 256, 257, 65536, 65813, 65808):
        c.append(PCase("fwd", 64, M, (1024, min(256, -(-M // 256)), 1), False))
    for M in (16, 17, 31, 128, 129, 32768, 32917, 32912):
        c.append(PCase("fwd", 128, M, (512, min(256, -(-M // 128)), 2), False))
        c.append(PCase("dgrad", 64, M, (512, min(256, -(-M // 128)), 1), M % 2 == 0))
    c += [PCase("dgrad", 64, 272, (512, 3, 1), True), PCase("dgrad", 64, 32917, (512, 256, 1), True)]
    return c


PROJ_CASES = _proj_cases()


def proj_id(c):
    return "%s-C%d-M%d%s" % (c.op, c.C, c.M, "-res" if c.res else "")


# ---- the gate (any device) ---------------------------------------------------------------------------------------------------------
def q(t):
    """Rounded to bf16 (nearest even), as fp64."""
    return t.to(torch.bfloat16).double()


def operand(t, engine):
    """What the engine multiplies of the stored values t, as fp64."""
    return t.double() if engine == "f32" else q(t)


def within(out, ref, A, c, bf16_store):
    """True where out meets the gate (a NaN never does)."""
    lim = c * A
    if bf16_store:
        lim = lim + 2.0 ** -8 * ref.abs()
    return (out.double() - ref).abs() <= lim


def measured(out, ref, A, bf16_store):
    """Worst err / A.  Behind a bf16 store the error of the fp32 sum shows only where it moved the sum across a rounding border: where
    the stored value is not the bf16 nearest to ref, the sum was at least |ref - midpoint of the two| off; together with any excess of
    the error over 2^-8 |ref|, over A.  A NaN gives inf; where A is 0 the output must equal ref (0 / 0 counts as 0)."""
    err = (out.double() - ref).abs()
    if bf16_store:
        nearest = ref.to(torch.bfloat16).double()
        moved = (ref - (out.double() + nearest) / 2).abs() * (out.double() != nearest)
        err = torch.maximum(moved, err - 2.0 ** -8 * ref.abs()).clamp_min(0.0)
    r = torch.where((err == 0) & (A == 0), torch.zeros_like(err), err / A)
    return r.nan_to_num(float("inf")).max().item()


WORST = {}             # (engine, op, route) -> worst measured value of this session (printed per case: pytest -s shows the measurements)


def assert_within(out, ref, A, engine, op, bf16_store, what, route=None):
    worst = measured(out, ref, A, bf16_store)
    if route is not None:
        key = (engine, op, route)
        WORST[key] = max(WORST.get(key, 0.0), worst)
        print("gemm fp64: %-58s worst %.3g = 2^%.2f   (so far %s: 2^%.2f)" % (
            what, worst, math.log2(worst) if worst > 0 else -99.0, key, math.log2(WORST[key]) if WORST[key] > 0 else -99.0))
    c = GATE_C[(engine, op)]
    ok = within(out, ref, A, c, bf16_store)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d outside the gate, first at %s (out %r, ref %r, A %r), measured worst %.3g (c %.3g)"
                             % (what, bad.shape[0], ok.numel(), i, out[i].item(), ref[i].item(), A[i].item(), worst, c))


def assert_exact(out, ref, what):
    assert ref.dtype == torch.float64
    want = ref.to(out.dtype)
    assert torch.equal(want.double(), ref), "%s: the reference is not representable" % what
    bad = (bits(out.contiguous()) != bits(want.contiguous())).nonzero()
    assert bad.numel() == 0, "%s: %d of %d elements differ, first at %s (out %r, want %r)" % (
        what, bad.shape[0], out.numel(), bad[0].tolist(), out[tuple(bad[0].tolist())].item(), want[tuple(bad[0].tolist())].item())


# ---- fp64 references: explicit sums over taps of shifted slices ------------------------------------------------------------------------
def taps_of(k):
    return [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]


def _span(n_out, n_in, t, p):
    """The outputs o whose input index o + t - p lies inside [0, n_in)."""
    return max(0, p - t), min(n_out, n_in + p - t)


def _slices(dout, din, tap, pad):
    """(output slices, input slices) of a tap, or None where no output sees it."""
    so, si = [], []
    for n_out, n_in, t, p in zip(dout, din, tap, pad):
        lo, hi = _span(n_out, n_in, t, p)
        if lo >= hi:
            return None
        so.append(slice(lo, hi))
        si.append(slice(lo + t - p, hi + t - p))
    return tuple(so), tuple(si)


def conv_ref(x, w, k, pad, tap_map=None):
    """x [B, Di, Hi, Wi, Ci], w [Co, Ci, kd, kh, kw], both fp64 -> (ref, A) [B, Do, Ho, Wo, Co].  tap_map (the route tests' mutations):
    tap -> the tap whose weights it is multiplied by."""
    din = tuple(x.shape[1:4])
    dout = out_extent(din, k, pad)
    ref = torch.zeros((x.shape[0],) + dout + (w.shape[0],), dtype=torch.float64, device=x.device)
    A = torch.zeros_like(ref)
    for tap in taps_of(k):
        s = _slices(dout, din, tap, pad)
        if s is None:
            continue
        (od, oh, ow), (i_d, ih, iw) = s
        wt = w[(slice(None), slice(None)) + (tap_map(tap) if tap_map else tap)].t()
        xs = x[:, i_d, ih, iw]
        ref[:, od, oh, ow] += xs @ wt
        A[:, od, oh, ow] += xs.abs() @ wt.abs()
    return ref, A


def dgrad_ref(dy, w, k, pad, din):
    """The adjoint of conv_ref in x: dy [B, Do, Ho, Wo, Co], w [Co, Ci, kd, kh, kw] -> (ref, A) [B, Di, Hi, Wi, Ci]."""
    dout = tuple(dy.shape[1:4])
    ref = torch.zeros((dy.shape[0],) + tuple(din) + (w.shape[1],), dtype=torch.float64, device=dy.device)
    A = torch.zeros_like(ref)
    for tap in taps_of(k):
        s = _slices(dout, din, tap, pad)
        if s is None:
            continue
        (od, oh, ow), (i_d, ih, iw) = s
        wt = w[(slice(None), slice(None)) + tap]
        ds = dy[:, od, oh, ow]
        ref[:, i_d, ih, iw] += ds @ wt
        A[:, i_d, ih, iw] += ds.abs() @ wt.abs()
    return ref, A


def wgrad_ref(x, dy, k, pad):
    """The adjoint of conv_ref in w: -> (ref, A) in the parameter layout [Co, Ci, kd, kh, kw]."""
    din, dout = tuple(x.shape[1:4]), tuple(dy.shape[1:4])
    ref = torch.zeros((dy.shape[-1], x.shape[-1]) + tuple(k), dtype=torch.float64, device=x.device)
    A = torch.zeros_like(ref)
    for tap in taps_of(k):
        s = _slices(dout, din, tap, pad)
        if s is None:
            continue
        (od, oh, ow), (i_d, ih, iw) = s
        ds = dy[:, od, oh, ow].reshape(-1, dy.shape[-1])
        xs = x[:, i_d, ih, iw].reshape(-1, x.shape[-1])
        ref[(slice(None), slice(None)) + tap] = ds.t() @ xs
        A[(slice(None), slice(None)) + tap] = ds.abs().t() @ xs.abs()
    return ref, A


def gemm_ref(c, A_, B_, res=None, old=None):
    """A_ [batch, rows, cols], B_ [batch or 1, rows, cols] fp64 as stored (already the engine's operands) -> (ref, A) [batch, M, N]."""
    a = A_ if c.ta == 0 else A_.transpose(1, 2)
    b = B_.transpose(1, 2) if c.tb == 1 else B_
    ref, A = a @ b, a.abs() @ b.abs()
    for t in (res, old):
        if t is not None:
            ref, A = ref + t, A + t.abs()
    return ref, A


# ---- NaN-guarded buffers (GPU) --------------------------------------------------------------------------------------------------------
class Slab:
    """rows x C values in columns [off, off + C) of rows of ld elements, inside a NaN-pattern buffer between two guards: everything
    but the values is NaN and must stay so.  ptr: the address of element (0, off) plus `byte_off`."""

    def __init__(self, rows, C, ld, dtype, vals=None, off=0):
        assert off + C <= ld or rows == 1
        self.rows, self.C, self.ld, self.off, self.dtype = rows, C, ld, off, dtype
        self.buf = nan_buffer(GUARD + rows * ld + GUARD, dtype)
        self.mat = self.buf[GUARD:GUARD + rows * ld].view(rows, ld)
        self.view = self.mat[:, off:off + C]
        if vals is not None:
            self.view.copy_(vals.reshape(rows, C))
        self.ptr = self.buf.data_ptr() + (GUARD + off) * self.buf.element_size()

    def assert_rest_untouched(self, what):
        nan = NAN16 if self.dtype == torch.bfloat16 else NAN32
        b = bits(self.buf) == nan
        b[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.C] = True
        assert bool(b.all()), "%s: %d elements outside the output slice were written (padding columns or guards)" % (what, int((~b).sum()))

    def assert_written(self, what):
        assert not bool(self.view.isnan().any()), "%s: an output element was left NaN" % what


def drnd(*shape, seed, ints=False):
    """Seeded operands drawn on the device: standard normal, or small integers in [-4, 4] (exact in bf16; sums exact in fp32)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if ints:
        return torch.randint(-4, 5, shape, generator=g, device="cuda").float()
    return torch.randn(*shape, generator=g, device="cuda")


@pytest.fixture
def lib():
    from hupr_amd import runtime
    return runtime.lib()


def stream():
    from hupr_amd import runtime
    return runtime.stream()


# ---- batched GEMM ----------------------------------------------------------------------------------------------------------------------
def gemm_operands(c, ints):
    ra, rb, lda, ldb, ldc, res_ld = gemm_lds(c)
    seed = 7 * c.M + 11 * c.N + 13 * c.K + c.batch + 100 * c.ta + 200 * c.tb
    o = {"A": drnd(c.batch, ra, lda - c.pads[0], seed=seed, ints=ints),
         "B": drnd(1 if c.bcast else c.batch, rb, ldb - c.pads[1], seed=seed + 1, ints=ints),
         "res": drnd(c.batch, c.M, c.N, seed=seed + 2, ints=ints) if "res" in c.epi else None,
         "old": drnd(c.batch, c.M, c.N, seed=seed + 3, ints=ints) if "acc" in c.epi else None}
    o["sA"] = Slab(c.batch * ra, lda - c.pads[0], lda, torch.float32, o["A"])
    o["sB"] = Slab(o["B"].shape[0] * rb, ldb - c.pads[1], ldb, torch.float32, o["B"])
    o["sR"] = Slab(c.batch * c.M, c.N, res_ld, torch.float32, o["res"]) if o["res"] is not None else None
    return o


def gemm_launch(L, c, engine, o, what):
    ra, rb, lda, ldb, ldc, res_ld = gemm_lds(c)
    out = Slab(c.batch * c.M, c.N, ldc, torch.float32, o["old"])
    fn = getattr(L, "hupr_gemm_" + engine)
    sR = o["sR"]
    rc = fn(c.ta, c.tb, o["sA"].ptr, o["sB"].ptr, out.ptr, c.M, c.N, c.K, lda, ldb, ldc, c.batch, ra * lda, 0 if c.bcast else rb * ldb,
            c.M * ldc, sR.ptr if sR else None, res_ld, c.M * res_ld, int("acc" in c.epi), stream())
    torch.cuda.synchronize()
    assert rc == 0, L.hupr_last_error()
    out.assert_rest_untouched(what)
    out.assert_written(what)
    return out.view.reshape(c.batch, c.M, c.N)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("c", GEMM_CASES, ids=[gemm_id(c) for c in GEMM_CASES])
def test_batched_gemm_matches_fp64(c, engine, lib):
    """Route first; then random operands against fp64 under the gate and integer operands bit for bit; guards, padding, NaN, the same
    bits from a second launch, one launch per call."""
    assert gemm_plan_of(lib, c, engine) == gemm_expected(c, engine)
    what = "%s %s" % (engine, gemm_id(c))
    for ints in (False, True):
        o = gemm_operands(c, ints)
        ref, A = gemm_ref(c, operand(o["A"], engine), operand(o["B"], engine), *(None if t is None else t.double() for t in (o["res"], o["old"])))
        n0 = lib.hupr_launch_count()
        out = gemm_launch(lib, c, engine, o, what)
        assert lib.hupr_launch_count() - n0 == 1
        if ints:
            assert_exact(out, ref, what + " (integers)")
        else:
            assert_within(out, ref, A, engine, "gemm", False, what, "%dx%d" % c.tile[engine])
        assert torch.equal(bits(gemm_launch(lib, c, engine, o, what)), bits(out)), "two launches differ"


# (Bn, G, HW, Ci, Co, dx stored as bf16, tile): hupr_tmerge_dgrad_bf16 — Bn G batched GEMMs dx[b, g] = dy[b] . W_g on mode-1 packed weights
TMERGE_DGRAD = [(2, 4, 63, 24, 40, 0, (64, 64)), (64, 8, 72, 40, 16, 1, (128, 64)), (3, 2, 130, 72, 33, 0, (64, 64)), (3, 2, 130, 72, 33, 1, (64, 64))]


@pytest.mark.parametrize("Bn,G_,HW,Ci,Co,dx16,tile", TMERGE_DGRAD)
def test_tmerge_input_gradient_matches_fp64(Bn, G_, HW, Ci, Co, dx16, tile, lib):
    """The generic input gradient of a temporal merge (z = (b, g) batching, negative weight stride) against the fp64 adjoint of the
    (G, 1, 1) convolution; fp32 dx also with integer operands, bit for bit."""
    assert plan(lib, "bf16", 0, [0, 1, HW, Ci, Co, Bn * G_])[:4] == tile + (-(-HW // tile[0]) * -(-Ci // tile[1]), Bn * G_)
    for ints in ((False,) if dx16 else (False, True)):
        dy = drnd(Bn, 1, 1, HW, Co, seed=HW + Co, ints=ints)
        w = drnd(Co, Ci, G_, 1, 1, seed=HW + Ci, ints=ints) * (1.0 if ints else Co ** -0.5)
        sDy, wp = Slab(1, dy.numel(), dy.numel(), torch.float32, dy), pack(lib, w, 1)
        n = Bn * G_ * HW * Ci
        out = Slab(1, n, n, torch.bfloat16 if dx16 else torch.float32)
        n0 = lib.hupr_launch_count()
        assert lib.hupr_tmerge_dgrad_bf16(sDy.ptr, wp.ptr, out.ptr, dx16, Bn, G_, HW, Ci, Co, stream()) == 0, lib.hupr_last_error()
        torch.cuda.synchronize()
        assert lib.hupr_launch_count() - n0 == 1
        out.assert_rest_untouched("tmerge dgrad")
        out.assert_written("tmerge dgrad")
        ref, A = dgrad_ref(q(dy), q(w), (G_, 1, 1), NOPAD, (G_, 1, HW))
        got = out.view.view(Bn, G_, 1, HW, Ci)
        if ints:
            assert_exact(got, ref, "tmerge dgrad (integers)")
        else:
            assert_within(got, ref, A, "bf16", "gemm", bool(dx16), "tmerge dgrad %dx%dx%d b%d" % (HW, Ci, Co, Bn * G_), "%dx%d" % tile)


# ---- weight packing ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [27, 9, 1])
def test_weight_packing_is_an_exact_permutation(taps, lib):
    """hupr_pack_conv_weights_f32 / _bf16, mode 0 [co][tap][ci] and mode 1 [ci][taps - 1 - tap][co], at (Co, Ci) = (20, 24): the fp32
    packing of a weight whose elements are all different integers, the bf16 packing of bf16-exact integers (neighbouring elements
    differ); no element may land anywhere else, guards untouched."""
    Co, Ci = 20, 24
    n = Co * Ci * taps
    w = (torch.randperm(n, generator=torch.Generator().manual_seed(taps)).float() - n // 2).view(Co, Ci, taps).cuda()
    w16 = (w / 64).round()                      # |values| <= 102: exact in bf16
    for fn, dt, src in ((lib.hupr_pack_conv_weights_f32, torch.float32, w), (lib.hupr_pack_conv_weights_bf16, torch.bfloat16, w16)):
        for mode in (0, 1):
            wp = Slab(1, n, n, dt)
            assert fn(src.data_ptr(), wp.ptr, Co, Ci, taps, mode, stream()) == 0, lib.hupr_last_error()
            torch.cuda.synchronize()
            wp.assert_rest_untouched("pack")
            want = src.permute(0, 2, 1) if mode == 0 else src.permute(1, 2, 0).flip(1)
            assert torch.equal(wp.view.view(want.shape), want.contiguous().to(dt)), (dt, mode)
    for bad in ((0, Ci, taps, 0), (Co, 0, taps, 0), (Co, Ci, 0, 0), (Co, Ci, taps, 2)):
        assert lib.hupr_pack_conv_weights_f32(w.data_ptr(), w.data_ptr(), *bad, stream()) == HUPR_ERR_ARG


def pack(L, w, mode):
    """w [Co, Ci, kd, kh, kw] fp32 -> the fp32 packing both engines read (mode 0 forward, 1 input gradient), in a guarded buffer."""
    Co, Ci = w.shape[:2]
    taps = w[0, 0].numel()
    wp = Slab(1, w.numel(), w.numel(), torch.float32)
    assert L.hupr_pack_conv_weights_f32(w.contiguous().data_ptr(), wp.ptr, Co, Ci, taps, mode, stream()) == 0, L.hupr_last_error()
    return wp


# ---- forward convolution and input gradient ------------------------------------------------------------------------------------------
def conv_operands(c, ints):
    i_ext, ci, o_ext, co, pad = conv_call_geometry(c)
    seed = sum(ord(ch) for ch in c.name) + 1000 * (c.eng == "bf16")
    xdt = torch.bfloat16 if "x16" in c.store else torch.float32
    o = {"x": drnd(c.B, *i_ext, ci, seed=seed, ints=ints).to(xdt),
         "w": drnd(c.Co, c.Ci, *c.k, seed=seed + 1, ints=ints) * (1.0 if ints else (vox(c.k) * ci) ** -0.5),
         "bias": drnd(co, seed=seed + 2, ints=ints) if "bias" in c.epi else None,
         "res": drnd(c.B, *o_ext, co, seed=seed + 3, ints=ints) if ("res" in c.epi or "inplace" in c.epi) else None,
         "old": drnd(c.B, *o_ext, co, seed=seed + 4, ints=ints) if "acc" in c.epi else None}
    o["sX"] = Slab(c.B * vox(i_ext), ci, ci + c.lds[0], xdt, o["x"], off=c.lds[1])
    if o["res"] is not None and "inplace" not in c.epi:
        o["sR"] = Slab(c.B * vox(o_ext), co, co + c.lds[4], torch.float32, o["res"])
    if o["bias"] is not None:
        o["sBias"] = Slab(1, co, co, torch.float32, o["bias"])
    return o


def conv_reference(c, o):
    i_ext, ci, o_ext, co, pad = conv_call_geometry(c)
    xd, wd = operand(o["x"].float(), c.eng), operand(o["w"], c.eng)
    ref, A = dgrad_ref(xd, wd, c.k, c.pad, c.din) if c.dgrad else conv_ref(xd, wd, c.k, c.pad)
    for t in (o["bias"], o["res"], o["old"]):
        if t is not None:
            ref, A = ref + t.double(), A + t.double().abs()
    return ref, A


def conv_launch(L, c, o, what):
    i_ext, ci, o_ext, co, pad = conv_call_geometry(c)
    ydt = torch.bfloat16 if "y16" in c.store else torch.float32
    rows, out_ld = c.B * vox(o_ext), co + c.lds[2]
    inplace = "inplace" in c.epi
    out = Slab(rows, co, out_ld, ydt, o["res"] if inplace else o["old"], off=c.lds[3])
    sR = out if inplace else o.get("sR")
    wp = pack(L, o["w"], 1 if c.dgrad else 0)
    bias = o["sBias"].ptr if "sBias" in o else None
    geo = (c.B, *i_ext, ci, ci + c.lds[0], *o_ext, co, out_ld)
    if c.store:
        rc = L.hupr_conv_fwd_bf16_mixed(o["sX"].ptr, int("x16" in c.store), wp.ptr, bias, out.ptr, int("y16" in c.store), *geo, *c.k, *pad, stream())
    else:
        fn = L.hupr_conv_fwd_f32 if c.eng == "f32" else L.hupr_conv_fwd_bf16
        rc = fn(o["sX"].ptr, wp.ptr, bias, sR.ptr if sR else None, out.ptr, *geo, sR.ld if sR else 0, *c.k, *pad, int("acc" in c.epi), stream())
    torch.cuda.synchronize()
    assert rc == 0, L.hupr_last_error()
    out.assert_rest_untouched(what)
    out.assert_written(what)
    wp.assert_rest_untouched(what + " (packed weights)")
    return out.view.reshape(c.B, *o_ext, co)


@pytest.mark.parametrize("c", CONV_CASES, ids=[conv_id(c) for c in CONV_CASES])
def test_convolution_matches_fp64(c, lib):
    """Forward convolutions and input gradients of both engines: route first, random operands under the gate, integer operands bit for
    bit (a bf16-stored output holds integers up to 256 exactly: the integer draw of those cases has one non-zero input channel and unit weights)."""
    assert plan(lib, c.eng, 1, conv_route_args(c)) == conv_expected(c)
    what = conv_id(c)
    for ints in (False, True):
        o = conv_operands(c, ints)
        if ints and "y16" in c.store:            # keep the sums inside bf16's 8 bits: one non-zero input channel per voxel, weights of -1, 0, 1
            keep = torch.zeros_like(o["x"])
            keep[..., 0] = 1
            o["x"] = o["x"] * keep
            o["sX"].view.copy_(o["x"].reshape(o["sX"].rows, -1))
            o["w"] = o["w"].sign()
        ref, A = conv_reference(c, o)
        n0 = lib.hupr_launch_count()
        out = conv_launch(lib, c, o, what)
        assert lib.hupr_launch_count() - n0 == 2                  # the packing and the convolution
        if ints:
            assert_exact(out, ref, what + " (integers)")
        else:
            assert_within(out, ref, A, c.eng, "conv", out.dtype == torch.bfloat16, what, "%dx%d" % c.tile)
        assert torch.equal(bits(conv_launch(lib, c, o, what).contiguous()), bits(out.contiguous())), "two launches differ"


def test_one_hot_convolution_reads_every_tap_exactly(lib):
    """x one-hot in the channels with the hot channel a function of the voxel, w all different integers: every output is a sum of 27
    single weights picked by (tap, channel) — exact, and wrong for any slip in tap order, tap reversal (mode 1) or channel chunking."""
    for eng, Ci in (("f32", 32), ("bf16", 24)):
        for dgrad in (False, True):
            c = CCase("one-hot", eng, 2, (3, 5, 7), 16 if dgrad else Ci, Ci if dgrad else 16, K333, SAME3, DENSE, "", "", dgrad, None)
            i_ext, ci, o_ext, co, pad = conv_call_geometry(c)
            n = c.B * vox(i_ext)
            hot = (torch.arange(n, device="cuda") * 5) % ci
            x = torch.zeros(n, ci, device="cuda").scatter_(1, hot.view(-1, 1), 1.0).view(c.B, *i_ext, ci)
            w = ((torch.arange(c.Co * c.Ci * 27, device="cuda") * 37) % 251 - 125).float().view(c.Co, c.Ci, 3, 3, 3)
            o = {"x": x, "w": w, "bias": None, "res": None, "old": None, "sX": Slab(n, ci, ci, torch.float32, x)}
            ref, _ = conv_reference(c, o)
            assert_exact(conv_launch(lib, c, o, "one-hot"), ref, "one-hot %s dgrad=%s" % (eng, dgrad))


# ---- weight gradient -------------------------------------------------------------------------------------------------------------------
def wgrad_operands(c, ints):
    dout = out_extent(c.din, c.k, c.pad)
    seed = sum(ord(ch) for ch in c.name) + 2000 * (c.eng == "bf16")
    xdt = torch.bfloat16 if c.xbf else torch.float32
    x = drnd(c.B, *c.din, c.Ci, seed=seed, ints=ints).to(xdt)
    dy = drnd(c.B, *dout, c.Co, seed=seed + 1, ints=ints)
    assert c.B * vox(dout) * 16 < 1 << 24          # the integer sums stay exact in fp32
    return {"x": x, "dy": dy, "sX": Slab(c.B * vox(c.din), c.Ci, c.Ci + c.lds[0], xdt, x),
            "sDy": Slab(c.B * vox(dout), c.Co, c.Co + c.lds[1], torch.float32, dy)}


def wgrad_launch(L, c, o, what, nbytes=None, off=None):
    """One guarded launch: dW [Co, Ci, kd, kh, kw]; the workspace holds exactly nbytes behind its pointer, NaN before and after."""
    dout = out_extent(c.din, c.k, c.pad)
    lib_bytes, lib_off = wgrad_ws(L, c)
    nbytes, off = lib_bytes if nbytes is None else nbytes, lib_off if off is None else off
    assert nbytes % 4 == 0 and off % 4 == 0
    n = c.Co * c.Ci * vox(c.k)
    dw = Slab(1, n, n, torch.float32)
    ws = Slab(1, nbytes // 4, nbytes // 4 + off // 4, torch.float32, off=off // 4)
    args = (dw.ptr, c.B, *c.din, c.Ci, c.Ci + c.lds[0], *dout, c.Co, c.Co + c.lds[1], *c.k, *c.pad, ws.ptr, nbytes, stream())
    if c.eng == "f32":
        rc = L.hupr_conv_wgrad_f32(o["sX"].ptr, o["sDy"].ptr, *args)
    elif c.xbf:
        rc = L.hupr_conv_wgrad_bf16_mixed(o["sX"].ptr, 1, o["sDy"].ptr, *args)
    else:
        rc = L.hupr_conv_wgrad_bf16(o["sX"].ptr, o["sDy"].ptr, *args)
    torch.cuda.synchronize()
    assert rc == 0, L.hupr_last_error()
    dw.assert_rest_untouched(what)
    dw.assert_written(what)
    ws.assert_rest_untouched(what + " (workspace)")
    return dw.view.view(c.Co, c.Ci, *c.k)


def wgrad_route_name(c):
    return "%s-%s" % (("scalar", "reduce4<4>", "reduce4<16>", "reduce_t<4,8>")[c.route[3]], "bm%d" % c.route[0])


@pytest.mark.parametrize("c", WGRAD_CASES, ids=[wgrad_id(c) for c in WGRAD_CASES])
def test_weight_gradient_matches_fp64(c, lib):
    """Route first (tile, slices after every cap and the shrink loop, reduce kernel and grid, bytes written); the workspace is NaN on
    entry, so a slice that skips its partial tensor — an empty one must still write zeros — shows; random and integer operands."""
    assert wgrad_plan_of(lib, c) == wgrad_expected(c)
    nbytes, _ = wgrad_ws(lib, c)
    dout = out_extent(c.din, c.k, c.pad)
    lib_bytes = lib.hupr_conv_wgrad_ws_bytes(c.B, *dout, c.Ci, c.Co, *c.k)
    assert c.ws != "lib" or wgrad_expected(c)[5] <= lib_bytes                    # never below what the engine then uses
    what = wgrad_id(c)
    for ints in (False, True):
        o = wgrad_operands(c, ints)
        ref, A = wgrad_ref(operand(o["x"].float(), c.eng), operand(o["dy"], c.eng), c.k, c.pad)
        n0 = lib.hupr_launch_count()
        out = wgrad_launch(lib, c, o, what)
        assert lib.hupr_launch_count() - n0 == 2                  # the sliced product and the reduction
        if ints:
            assert_exact(out, ref, what + " (integers)")
        else:
            assert_within(out, ref, A, c.eng, "wgrad", False, what, wgrad_route_name(c))
        assert torch.equal(bits(wgrad_launch(lib, c, o, what).contiguous()), bits(out.contiguous())), "two launches differ"


FORCED = [c for c in WGRAD_CASES if c.name in ("333-ktiles7", "111-33slices", "111-256", "333-1024/tiles", "111-empty-slice", "133-empty-slice",
                                               "333-ci8", "G11-x16")]


@pytest.mark.parametrize("c", FORCED, ids=[wgrad_id(c) for c in FORCED])
def test_forced_slice_classes_sum_the_same_partials(c, lib):
    """hupr_debug_splitk_slices: the class the automatic choice takes, with and without the scattered-store kernel, gives its bits; the
    other class is inside the gate, and bit-identical at four partial tensors or fewer."""
    o = wgrad_operands(c, False)
    ref, A = wgrad_ref(operand(o["x"].float(), c.eng), operand(o["dy"], c.eng), c.k, c.pad)
    what = wgrad_id(c)
    auto = wgrad_launch(lib, c, o, what).clone()
    mine = 16 if c.route[3] == REDUCE4_16 else 4
    try:
        for forced in (4, 16, 4 + 256, 16 + 256):
            lib.hupr_debug_splitk_slices(forced)
            kernel = wgrad_plan_of(lib, c)[3]
            if forced & 256:
                assert kernel == (REDUCE4_16 if forced & 255 == 16 else REDUCE4_4)
            elif forced == 16:
                assert kernel == REDUCE4_16
            else:
                assert kernel in (REDUCE4_4, REDUCE_T)
            out = wgrad_launch(lib, c, o, "%s forced %d" % (what, forced))
            if forced & 255 == mine or c.route[2] <= 4:
                assert torch.equal(bits(out.contiguous()), bits(auto)), "forced %d differs from the automatic choice" % forced
            else:
                assert_within(out, ref, A, c.eng, "wgrad", False, "%s forced %d" % (what, forced))
    finally:
        lib.hupr_debug_splitk_slices(0)
    assert wgrad_plan_of(lib, c) == wgrad_expected(c)


# ---- projections -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def proj_weights(C, ints=False):
    w = drnd(4 * C, C, seed=600 + C, ints=ints)
    return w if ints else w * C ** -0.5


def proj_reference(c, x, wc, res):
    xd, wd = q(x), q(wc)
    if c.op == "fwd":
        return xd @ wd.t(), xd.abs() @ wd.abs().t()
    ref, A = xd @ wd, xd.abs() @ wd.abs()
    if res is not None:
        ref, A = ref + res.double(), A + res.double().abs()
    return ref, A


def proj_launch(L, c, x, wc, res, what):
    """x: X [M, C] (forward) or dY [M, 4C] (input gradient), behind and in front of NaN guards."""
    sX = Slab(1, x.numel(), x.numel(), torch.float32, x)
    sW = Slab(1, wc.numel(), wc.numel(), torch.float32, wc)
    if c.op == "fwd":
        out = Slab(1, c.M * 4 * c.C, c.M * 4 * c.C, torch.bfloat16)
        rc = L.hupr_mscsa_proj_fwd_bf16(sX.ptr, sW.ptr, out.ptr, c.M, c.C, stream())
    else:
        out = Slab(1, c.M * c.C, c.M * c.C, torch.float32)
        sR = Slab(1, res.numel(), res.numel(), torch.float32, res) if res is not None else None
        rc = L.hupr_mscsa_proj_dgrad_f32(sX.ptr, sW.ptr, sR.ptr if sR else None, out.ptr, c.M, c.C, stream())
    torch.cuda.synchronize()
    assert rc == 0, L.hupr_last_error()
    out.assert_rest_untouched(what)
    out.assert_written(what)
    return out.view.view(c.M, -1)


def proj_plan_of(L, c):
    return proj_grid(L, int(c.op == "dgrad"), c.M, c.C)


@pytest.mark.parametrize("c", PROJ_CASES, ids=[proj_id(c) for c in PROJ_CASES])
def test_projection_matches_fp64(c, lib):
    assert proj_plan_of(lib, c) == c.grid
    assert (lib.hupr_mscsa_proj_supported if c.op == "fwd" else lib.hupr_mscsa_proj_dgrad_supported)(c.M, c.C) == 1
    wc = proj_weights(c.C)
    x = drnd(c.M, c.C if c.op == "fwd" else 4 * c.C, seed=c.M + c.C)
    res = drnd(c.M, c.C, seed=c.M + 1) if c.res else None
    ref, A = proj_reference(c, x, wc, res)
    what = proj_id(c)
    n0 = lib.hupr_launch_count()
    out = proj_launch(lib, c, x, wc, res, what)
    assert lib.hupr_launch_count() - n0 == 1
    wrap = "wrap" if c.M > c.grid[1] * c.grid[0] // 4 else "one-step"
    assert_within(out, ref, A, "bf16", "proj_" + c.op, c.op == "fwd", what, "C%d-%s" % (c.C, wrap))
    assert torch.equal(bits(proj_launch(lib, c, x, wc, res, what).contiguous()), bits(out.contiguous())), "two launches differ"


@pytest.mark.parametrize("op,C", [("fwd", 64), ("fwd", 128), ("dgrad", 64)])
def test_projection_exact_cases(op, C, lib):
    """M = 272 (a partial last step).  Forward: x one-hot in the channels (value p[m] at channel (3 m) % C) against integer weights —
    y[m][n] = p[m] Wc[n][(3 m) % C], at most 32 in magnitude, exact in bf16; and bf16-representable x against one-hot weight rows
    (+-1 at channel (7 n) % C) — y[m][n] = +-x[m][(7 n) % C].  Input gradient: integer operands and residual, sums exact in fp32."""
    M = 272
    c = PCase(op, C, M, None, op == "dgrad")
    m = torch.arange(M, device="cuda")
    if op == "fwd":
        p = ((m * 5) % 17 - 8).float()
        x = torch.zeros(M, C, device="cuda").scatter_(1, ((3 * m) % C).view(-1, 1), p.view(-1, 1))
        wc = proj_weights(C, True)
        assert_exact(proj_launch(lib, c, x, wc, None, "one-hot rows"), proj_reference(c, x, wc, None)[0], "%s C = %d one-hot rows" % (op, C))
        n = torch.arange(4 * C, device="cuda")
        sign = (1 - 2 * (n % 2)).float()
        wc = torch.zeros(4 * C, C, device="cuda").scatter_(1, ((7 * n) % C).view(-1, 1), sign.view(-1, 1))
        x = drnd(M, C, seed=9).to(torch.bfloat16).float()
        want = x[:, (7 * n) % C] * sign
        out = proj_launch(lib, c, x, wc, None, "one-hot weights")
        assert_exact(out, want.double(), "%s C = %d one-hot weights" % (op, C))
        assert torch.equal(proj_reference(c, x, wc, None)[0], want.double())
    else:
        x, wc, res = drnd(M, 4 * C, seed=10, ints=True), proj_weights(C, True), drnd(M, C, seed=11, ints=True)
        assert_exact(proj_launch(lib, c, x, wc, res, "integers"), proj_reference(c, x, wc, res)[0], "dgrad integers")
        assert_exact(proj_launch(lib, PCase(op, C, M, None, False), x, wc, None, "integers"), proj_reference(c, x, wc, None)[0],
                     "dgrad integers, no residual")


@pytest.mark.parametrize("C", [64, 128])
def test_projection_of_prescaled_query_rows(C, lib):
    """The forward multiplies by the concatenation functional._proj_cat builds: query (theta) rows pre-scaled by log2 e in fp32.  The
    reference rounds those scaled fp32 rows to bf16, as the kernel does."""
    from hupr_amd import functional as F_
    M = 272
    ws = [torch.nn.Parameter(proj_weights(C)[j * C:(j + 1) * C].clone().view(C, C, 1, 1)) for j in range(4)]
    wc, wq = F_._proj_cat(ws, C)
    assert torch.equal(wc, proj_weights(C))
    scaled = wc.clone()
    scaled[C:2 * C] *= 1.4426950408889634
    scaled[3 * C:] *= 1.4426950408889634
    assert torch.equal(wq, scaled)
    c = PCase("fwd", C, M, None, False)
    x = drnd(M, C, seed=12)
    ref, A = proj_reference(c, x, wq, None)
    assert_within(proj_launch(lib, c, x, wq, None, "pre-scaled"), ref, A, "bf16", "proj_fwd", True, "fwd C = %d pre-scaled query rows" % C)


# ---- refused calls ------------------------------------------------------------------------------------------------------------------
# (what, kind, engine, arguments): refused by the plan alone — test_gemm_route.py asserts that without a device
G_OK = [0, 1, 8, 8, 8, 1]
C_OK = [1, 2, 4, 4, 32, 32, 2, 4, 4, 16, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]


def _with(v, **kw):
    names = {"ta": 0, "tb": 1, "M": 2, "N": 3, "K": 4, "batch": 5} if len(v) == 6 else {
        "Bn": 0, "Di": 1, "Hi": 2, "Wi": 3, "Ci": 4, "in_ld": 5, "Do": 6, "Ho": 7, "Wo": 8, "Co": 9, "kd": 10, "pd": 13, "x16": 16, "y16": 17,
        "acc": 18, "res": 19}
    v = list(v)
    for k_, val in kw.items():
        v[names[k_]] = val
    return v


REFUSED = []
for _e in ENGINES:
    REFUSED += [("%s gemm: batch 65536" % _e, "gemm", _e, _with(G_OK, batch=65536)), ("%s gemm: batch 0" % _e, "gemm", _e, _with(G_OK, batch=0)),
                ("%s gemm: M = 0" % _e, "gemm", _e, _with(G_OK, M=0)), ("%s gemm: N = -1" % _e, "gemm", _e, _with(G_OK, N=-1)),
                ("%s gemm: K = 0" % _e, "gemm", _e, _with(G_OK, K=0)), ("%s gemm: A^T B^T" % _e, "gemm", _e, _with(G_OK, ta=1, tb=1)),
                ("%s conv: extent 1024" % _e, "conv", _e, _with(C_OK, Di=1024, Do=1024)),
                ("%s conv: Ci not a multiple" % _e, "conv", _e, _with(C_OK, Ci=16 if _e == "f32" else 12, in_ld=16)),
                ("%s conv: in_ld not a multiple of 4" % _e, "conv", _e, _with(C_OK, in_ld=34)),
                ("%s conv: output extent" % _e, "conv", _e, _with(C_OK, Do=3)),
                ("%s conv: Co = 0" % _e, "conv", _e, _with(C_OK, Co=0)), ("%s conv: Bn = 0" % _e, "conv", _e, _with(C_OK, Bn=0)),
                ("%s wgrad: extent 1024" % _e, "wgrad", _e, _with(C_OK, Di=1024, Do=1024)[:17]),
                ("%s wgrad: Ci not a multiple" % _e, "wgrad", _e, _with(C_OK, Ci=16 if _e == "f32" else 6, in_ld=16)[:17]),
                ("%s wgrad: workspace below one partial tensor" % _e, "wgrad-ws", _e, C_OK[:17])]
REFUSED += [("bf16 conv: bf16 output with accumulate", "conv", "bf16", _with(C_OK, y16=1, acc=1)),
            ("bf16 conv: bf16 output with a residual", "conv", "bf16", _with(C_OK, y16=1, res=1))]


def refused_plan(L, r):
    what, kind, e, v = r
    if kind == "wgrad-ws":
        return plan(L, e, 2, v, v[9] * v[4] * 4 - 4)
    return plan(L, e, {"gemm": 0, "conv": 1, "wgrad": 2}[kind], v, 1 << 20)


def refused_call(L, r, x, w, out, ws, s):
    """The refused call through its entry point on the given addresses (None: the plan has no entry point that takes this combination)."""
    what, kind, e, v = r
    if kind == "gemm":
        return getattr(L, "hupr_gemm_" + e)(v[0], v[1], x, w, out, v[2], v[3], v[4], 8, 8, 8, v[5], 64, 64, 64, None, 0, 0, 0, s)
    if kind == "conv":
        if v[17]:
            return None
        fn = L.hupr_conv_fwd_f32 if e == "f32" else L.hupr_conv_fwd_bf16
        return fn(x, w, None, None, out, *v[:10], v[9], v[9], *v[10:16], 0, s)
    nbytes = (v[9] * v[4] * 4 - 4) if kind == "wgrad-ws" else (1 << 20)
    fn = L.hupr_conv_wgrad_f32 if e == "f32" else L.hupr_conv_wgrad_bf16
    return fn(x, w, out, *v[:10], v[9], *v[10:16], ws, nbytes, s)


@pytest.mark.parametrize("r", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_calls_leave_everything_untouched(r, lib):
    want = HUPR_ERR_WORKSPACE if r[1] == "wgrad-ws" else HUPR_ERR_ARG
    assert refused_plan(lib, r) == want
    x = torch.zeros(1 << 16, device="cuda")
    out, ws = Slab(1, 1 << 16, 1 << 16, torch.float32), Slab(1, 1 << 18, 1 << 18, torch.float32)
    n0 = lib.hupr_launch_count()
    rc = refused_call(lib, r, x.data_ptr(), x.data_ptr(), out.ptr, ws.ptr, stream())
    torch.cuda.synchronize()
    assert rc in (want, None), (r[0], rc)
    assert lib.hupr_launch_count() == n0
    assert bool((bits(out.buf) == NAN32).all()) and bool((bits(ws.buf) == NAN32).all()), r[0]


PROJ_REFUSED = [("fwd C = 256", "fwd", 64, 256, 0), ("fwd C = 32", "fwd", 64, 32, 0), ("fwd M = 15", "fwd", 15, 64, 0), ("dgrad M = 15", "dgrad", 15, 64, 0),
                ("dgrad C = 128", "dgrad", 64, 128, 0), ("fwd: pointers 4 bytes off", "fwd", 64, 64, 4), ("fwd: pointers 8 bytes off", "fwd", 64, 64, 8),
                ("dgrad: pointers 4 bytes off", "dgrad", 64, 64, 4), ("dgrad: pointers 8 bytes off", "dgrad", 64, 64, 8)]


def proj_refused_call(L, r, x, w, out, s):
    """Every pointer in turn carries the offset; all of the calls must be refused."""
    what, op, M, C, off = r
    rcs = []
    for i in range(4 if (off and op == "dgrad") else 3 if off else 1):
        p = [x, w, out, x]
        p[i] += off
        rcs.append(L.hupr_mscsa_proj_fwd_bf16(p[0], p[1], p[2], M, C, s) if op == "fwd" else
                   L.hupr_mscsa_proj_dgrad_f32(p[0], p[1], p[3], p[2], M, C, s))
    return rcs


@pytest.mark.parametrize("r", PROJ_REFUSED, ids=[r[0] for r in PROJ_REFUSED])
def test_refused_projections_leave_everything_untouched(r, lib):
    x = torch.zeros(1 << 16, device="cuda")
    out = Slab(1, 1 << 16, 1 << 16, torch.float32)
    n0 = lib.hupr_launch_count()
    rcs = proj_refused_call(lib, r, x.data_ptr(), x.data_ptr(), out.ptr, stream())
    torch.cuda.synchronize()
    assert rcs and all(rc == HUPR_ERR_ARG for rc in rcs), (r[0], rcs)
    assert lib.hupr_launch_count() == n0 and bool((bits(out.buf) == NAN32).all())
    if not r[4]:
        assert proj_grid(lib, int(r[1] == "dgrad"), r[2], r[3]) == HUPR_ERR_ARG
        assert (lib.hupr_mscsa_proj_supported if r[1] == "fwd" else lib.hupr_mscsa_proj_dgrad_supported)(r[2], r[3]) == 0


# ---- through functional.py ------------------------------------------------------------------------------------------------------------
ENTRIES = ("hupr_gemm_f32", "hupr_gemm_bf16", "hupr_conv_fwd_f32", "hupr_conv_fwd_bf16", "hupr_conv_fwd_bf16_mixed", "hupr_conv_wgrad_f32",
           "hupr_conv_wgrad_bf16", "hupr_conv_wgrad_bf16_mixed", "hupr_tmerge_dgrad_bf16", "hupr_mscsa_proj_fwd_bf16", "hupr_mscsa_proj_dgrad_f32",
           "hupr_conv3x3_halo_bf16", "hupr_conv3x3_halo_bf16act", "hupr_conv3x3_wgrad_halo_bf16")


class Counted:
    """The engines' entry points of rt.lib() (and the halo kernels' a convolution could take instead) wrapped by call counters."""

    def __init__(self, L, spy=None):
        self.L, self.n, self.orig, self.spy = L, collections.Counter(), {}, spy or {}

    def __enter__(self):
        for name in ENTRIES:
            self.orig[name] = orig = getattr(self.L, name)

            def f(*a, _name=name, _orig=orig):
                self.n[_name] += 1
                if _name in self.spy:
                    return self.spy[_name](_orig, *a)
                return _orig(*a)
            setattr(self.L, name, f)
        return self

    def __exit__(self, *exc):
        for name, orig in self.orig.items():
            setattr(self.L, name, orig)

    def take(self):
        n, self.n = dict(self.n), collections.Counter()
        return n


@pytest.fixture
def math_mode():
    from hupr_amd import functional as F_
    yield F_.set_math
    F_.set_math("f32")


@pytest.mark.parametrize("engine", ENGINES)
def test_functional_gemm_reaches_its_engine(engine, lib, math_mode):
    from hupr_amd import functional as F_
    math_mode(engine)
    c = GCase(0, 0, 70, 66, 33, 3, (0, 0, 0, 0), "res acc", False, None)
    A_, B_ = drnd(3, 70, 33, seed=1), drnd(3, 33, 66, seed=2)
    res, old = drnd(3, 70, 66, seed=3), drnd(3, 70, 66, seed=4)
    out = old.clone()
    with Counted(lib) as n:
        got = F_.gemm(0, 0, A_, B_, 70, 66, 33, 33, 66, 3, 70 * 33, 33 * 66, out=out, res=res, accumulate=True)
        assert n.take() == {"hupr_gemm_" + engine: 1}
        other = ENGINES[1 - ENGINES.index(engine)]
        got2 = F_.gemm(0, 0, A_, B_, 70, 66, 33, 33, 66, 3, 70 * 33, 33 * 66, math=other)
        assert n.take() == {"hupr_gemm_" + other: 1}
    torch.cuda.synchronize()
    assert got is out
    assert_within(got, *gemm_ref(c, operand(A_, engine), operand(B_, engine), res.double(), old.double()), engine, "gemm", False, "functional.gemm")
    assert_within(got2, *gemm_ref(c, operand(A_, other), operand(B_, other)), other, "gemm", False, "functional.gemm math=")


@pytest.mark.parametrize("engine", ENGINES)
def test_functional_conv_reaches_its_engine(engine, lib, math_mode):
    """functional.conv at a shape the halo kernel refuses (a 3 x 3 x 3 kernel without padding) in fp32 and in bf16 math: forward, input
    gradient (mode-1 weights) and weight gradient through autograd, one call of the engine's entry point each, none of the halo kernels."""
    from hupr_amd import functional as F_
    math_mode(engine)
    B, din, Ci, Co = 2, (4, 6, 7), 32, 32
    x = drnd(B, *din, Ci, seed=21).requires_grad_(True)
    w = (drnd(Co, Ci, 3, 3, 3, seed=22) * (27 * Ci) ** -0.5).requires_grad_(True)
    bias = drnd(Co, seed=23).requires_grad_(True)
    dout = out_extent(din, K333, NOPAD)
    dy = drnd(B, *dout, Co, seed=24)
    with Counted(lib) as n:
        y = F_.conv(x, w, bias, pad=NOPAD)
        assert n.take() == {"hupr_conv_fwd_" + engine: 1}
        y.backward(dy)
        assert n.take() == {"hupr_conv_fwd_" + engine: 1, "hupr_conv_wgrad_" + engine: 1}
    torch.cuda.synchronize()
    xd, wd, dyd = operand(x.detach(), engine), operand(w.detach(), engine), operand(dy, engine)
    ref, A = conv_ref(xd, wd, K333, NOPAD)
    assert_within(y.detach(), ref + bias.detach().double(), A + bias.detach().double().abs(), engine, "conv", False, "functional.conv forward")
    assert_within(x.grad, *dgrad_ref(dyd, wd, K333, NOPAD, din), engine, "conv", False, "functional.conv dx")
    assert_within(w.grad, *wgrad_ref(xd, dyd, K333, NOPAD), engine, "wgrad", False, "functional.conv dW")


def test_mscsa_level_node_projects_through_the_streaming_kernels(lib, math_mode):
    """MSCSALevelFn at level-1 geometry (C = 64, N = 16 x 8 = 128 keys, B = 3: M = 384 rows): two forward projections, two input
    gradients, two weight gradients (hupr_conv_wgrad_bf16) and none of the engine's other entry points; every projection call is
    checked against fp64 on the operands it was handed (copied out around the call)."""
    from hupr_amd import functional as F_
    math_mode("bf16")
    B, H, W, C = 3, 16, 8, 64
    M = B * H * W
    if not lib.hupr_attn_flash_supported(H * W, C):
        pytest.fail("the fused attention kernels refuse N = %d, C = %d: choose another level-1 shape" % (H * W, C))
    ra, re = (drnd(B, 1, H, W, C, seed=s).requires_grad_(True) for s in (31, 32))
    weights = [torch.nn.Parameter(drnd(C, C, 1, 1, seed=40 + j) * C ** -0.5) for j in range(8)]
    seen = []

    class Raw:
        def __init__(self, ptr, n, typestr):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}

    def grab(ptr, n, dtype):
        """A copy of n elements of device memory at a raw address."""
        t = torch.as_tensor(Raw(ptr, n, "<f4" if dtype == torch.float32 else "<i2"), device="cuda").clone()
        torch.cuda.synchronize()
        return t if dtype == torch.float32 else t.view(torch.bfloat16)

    def spy_fwd(orig, X, Wc, Y, M_, C_, s):
        x, wc = grab(X, M_ * C_, torch.float32).view(M_, C_), grab(Wc, 4 * C_ * C_, torch.float32).view(4 * C_, C_)
        rc = orig(X, Wc, Y, M_, C_, s)
        seen.append(("fwd", x, wc, None, grab(Y, M_ * 4 * C_, torch.bfloat16).view(M_, 4 * C_)))
        return rc

    def spy_dgrad(orig, dY, Wc, res, dX, M_, C_, s):
        dy, wc = grab(dY, M_ * 4 * C_, torch.float32).view(M_, 4 * C_), grab(Wc, 4 * C_ * C_, torch.float32).view(4 * C_, C_)
        r = grab(res, M_ * C_, torch.float32).view(M_, C_) if res else None
        rc = orig(dY, Wc, res, dX, M_, C_, s)
        seen.append(("dgrad", dy, wc, r, grab(dX, M_ * C_, torch.float32).view(M_, C_)))
        return rc

    spies = {"hupr_mscsa_proj_fwd_bf16": spy_fwd, "hupr_mscsa_proj_dgrad_f32": spy_dgrad}
    with Counted(lib, spies) as n:
        outs = F_.MSCSALevelFn.apply(ra, re, 0, *weights)
        assert n.take() == {"hupr_mscsa_proj_fwd_bf16": 2}
        torch.autograd.backward(outs, [drnd(B, 1, H, W, C, seed=50 + i) for i in range(4)])
        assert n.take() == {"hupr_mscsa_proj_dgrad_f32": 2, "hupr_conv_wgrad_bf16": 2}
    torch.cuda.synchronize()
    assert ra.grad is not None and not bool(ra.grad.isnan().any()) and all(w.grad is not None for w in weights)
    # the concatenations the calls were handed: forward the pre-scaled one, backward the plain one
    plain = [torch.cat([w.detach().view(C, C) for w in weights[4 * i:4 * i + 4]]) for i in range(2)]
    scaled = [p.clone() for p in plain]
    for s_ in scaled:
        s_[C:2 * C] *= 1.4426950408889634
        s_[3 * C:] *= 1.4426950408889634
    assert [k[0] for k in seen] == ["fwd", "fwd", "dgrad", "dgrad"]
    for i, (op, x, wc, r, out) in enumerate(seen):
        assert torch.equal(wc, (scaled if (op == "fwd" and F_.QS_ATTN) else plain)[i % 2]), (op, i)
        c = PCase(op, C, M, None, r is not None)
        assert op == "fwd" or r is not None                            # the value gradient rides as the residual term
        assert_within(out, *proj_reference(c, x, wc, r), "bf16", "proj_" + op, op == "fwd", "MSCSALevelFn %s %d" % (op, i))
    for i, x in enumerate((ra, re)):
        assert torch.equal(seen[i][1], x.detach().view(M, C)) and torch.equal(seen[2 + i][4].view_as(x), x.grad)


# ---- what this session measured (pytest -s) -----------------------------------------------------------------------------------------
def test_zz_print_the_worst_measured_values():
    for key in sorted(WORST):
        print("gemm fp64 WORST %-40s 2^%.2f" % (key, math.log2(WORST[key]) if WORST[key] > 0 else -99.0))
    for (engine, op), c in GATE_C.items():
        worst = max([v for (e, o, _), v in WORST.items() if (e, o) == (engine, op)], default=0.0)
        assert c <= CAP and worst <= c
