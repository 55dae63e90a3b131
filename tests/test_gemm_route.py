"""CPU (no GPU needed): the launch plans of the GEMM engines and of the MSCSA projections (hupr_debug_gemm_route,
hupr_debug_mscsa_proj_grid: the host functions the launchers of csrc/gemm_f32.hip, csrc/gemm_bf16.hip and csrc/projection.hip
themselves call) send every case of the fp64 tables (test_gemm_fp64_gpu.py) to the literal route it names — the rules are restated
here (the two tile dispatchers, wgrad_splits with the workspace-shrink loop, the reduce-kernel choice, the projection grids) and must
give the same answer; the model's own GEMM-engine shapes at batch 1, 3 and 32 are pinned to today's routes, so a change that silently
moves a training shape to another tile or slice count fails; the tables reach every template instantiation launch<...> / launch_h<...>
can reach, every reduce kernel, every branch of the split rule and every exported entry point of the three sources; the refused
calls are refused by the plans alone; and the gates reject the results of subtly wrong kernels (mutated copies of the fp64 reference)
while they accept an honest fp32 evaluation of the same sums in another order."""
import os
import re

import pytest
import torch

import test_gemm_fp64_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hupr-a-benchmark-for-human-pose-estimation-using-millimeter-wave-radar_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


# ---- the rules, restated ----------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def tile_rule(engine, M, N, batch):
    """dispatch_tiles (fp32) / dispatch_h (bf16): the largest tile that still gives 512 workgroups."""
    blocks = lambda bm, bn: cdiv(M, bm) * cdiv(N, bn) * batch
    if N > 64:
        if M > 64 and blocks(128, 128) >= 512:
            t = (128, 128)
        elif engine == "f32" or blocks(64, 128) >= 512:
            t = (64, 128)
        else:
            t = (64, 64)
    elif N > 32 or engine == "bf16":
        t = (128, 64) if M > 64 and blocks(128, 64) >= 512 else (64, 64)
    else:
        t = (128, 32)
    return t + (cdiv(M, t[0]) * cdiv(N, t[1]), batch, 0, 0)


def splits_rule(tiles, ktiles, one, in_bytes=0):
    """wgrad_splits; -> (slices, the cap that set them)."""
    s, why = cdiv(1024, tiles), "1024/tiles"
    if in_bytes:
        cap, floor = in_bytes // (2 * one), cdiv(256, tiles)
        if s > cap:
            s, why = (cap, "cap") if cap > floor else (floor, "floor")
    if s > 256:
        s, why = 256, "256"
    if s > ktiles:
        s, why = ktiles, "ktiles"
    while s > 1 and s * one > 256 << 20:
        s >>= 1
    return max(s, 1), why


def reduce_rule(n, splits, taps, ci, aligned, forced=0):
    """launch_splitk_reduce for one gradient: (kernel, workgroups)."""
    if not (n % 4 == 0 and ci % 4 == 0 and aligned):
        return G.SCALAR, cdiv(n, 256)
    s16 = (forced & 255) == 16 if forced & 255 else (splits >= 32 and n // 4 <= 1 << 17)
    if not s16 and 1 < taps <= 27 and ci % 32 == 0 and not forced & 256:
        return G.REDUCE_T, n // (taps * ci) * (ci // 32)
    return (G.REDUCE4_16, cdiv(n // 4, 16)) if s16 else (G.REDUCE4_4, cdiv(n // 4, 64))


def wgrad_rule(engine, B, dout, Ci, Co, k, xbf, ws_bytes, misalign=0, forced=0):
    """-> (BM, grid.x, slices, reduce kernel, its workgroups, bytes written), the cap that set the slices."""
    Mv, taps = B * G.vox(dout), G.vox(k)
    bm = 64 if Co <= 64 else 128
    tiles = cdiv(Co, bm) * cdiv(taps * Ci, 128)
    one = Co * taps * Ci * 4
    in_bytes = 0 if engine == "f32" else Mv * (Co * 4 + taps * Ci * (2 if xbf else 4))
    s, why = splits_rule(tiles, cdiv(Mv, 32 if engine == "f32" else 64), one, in_bytes)
    while s > 1 and s * one > ws_bytes:
        s, why = s >> 1, "shrink"
    return (bm, tiles, s) + reduce_rule(Co * taps * Ci, s, taps, Ci, misalign % 16 == 0, forced) + (s * one,), why


def proj_rule(op, M, C):
    threads = 1024 if (op == "fwd" and C == 64) else 512
    return threads, min(256, cdiv(M, threads // 4)), 4 * C // 256 if op == "fwd" else 1


# ---- every case of the tables goes to its literal route ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.GEMM_CASES, ids=[G.gemm_id(c) for c in G.GEMM_CASES])
def test_gemm_case_routes(c, L):
    for e in G.ENGINES:
        assert G.gemm_plan_of(L, c, e) == G.gemm_expected(c, e) == tile_rule(e, c.M, c.N, c.batch), (e, G.gemm_id(c))


def test_tmerge_input_gradient_case_routes(L):
    for Bn, G_, HW, Ci, Co, dx16, tile in G.TMERGE_DGRAD:
        assert G.plan(L, "bf16", 0, [0, 1, HW, Ci, Co, Bn * G_]) == tile_rule("bf16", HW, Ci, Bn * G_) and tile_rule("bf16", HW, Ci, Bn * G_)[:2] == tile
    assert {c[5] for c in G.TMERGE_DGRAD} == {0, 1} and any(c[4] % 4 for c in G.TMERGE_DGRAD)


@pytest.mark.parametrize("c", G.CONV_CASES, ids=[G.conv_id(c) for c in G.CONV_CASES])
def test_conv_case_routes(c, L):
    i_ext, ci, o_ext, co, pad = G.conv_call_geometry(c)
    assert G.plan(L, c.eng, 1, G.conv_route_args(c)) == G.conv_expected(c) == tile_rule(c.eng, c.B * G.vox(o_ext), co, 1)
    assert o_ext == G.out_extent(i_ext, c.k, pad) and all(e >= 1 for e in o_ext)
    assert ci % (32 if c.eng == "f32" else 8) == 0 and c.lds[1] <= c.lds[0] and c.lds[3] <= c.lds[2] and c.lds[1] % 4 == 0
    assert hasattr(L, G.conv_entry(c))
    if "y16" in c.store:
        assert not set(c.epi.split()) & {"res", "acc", "inplace"}


@pytest.mark.parametrize("c", G.WGRAD_CASES, ids=[G.wgrad_id(c) for c in G.WGRAD_CASES])
def test_wgrad_case_routes(c, L):
    nbytes, off = G.wgrad_ws(L, c)
    dout = G.out_extent(c.din, c.k, c.pad)
    want, why = wgrad_rule(c.eng, c.B, dout, c.Ci, c.Co, c.k, c.xbf, nbytes, off)
    assert G.wgrad_plan_of(L, c) == G.wgrad_expected(c) == want, G.wgrad_id(c)
    assert why == c.why, (G.wgrad_id(c), why)
    # hupr_conv_wgrad_ws_bytes: the fp32 engine's own count, and never below what either engine uses with it
    lib_bytes = L.hupr_conv_wgrad_ws_bytes(c.B, *dout, c.Ci, c.Co, *c.k)
    f32, _ = wgrad_rule("f32", c.B, dout, c.Ci, c.Co, c.k, 0, 1 << 40)
    assert lib_bytes == f32[5]
    for e, xbf in (("f32", 0), ("bf16", 0), ("bf16", 1)):
        assert wgrad_rule(e, c.B, dout, c.Ci, c.Co, c.k, xbf, lib_bytes)[0][5] <= lib_bytes
    # the forced slice classes of hupr_debug_splitk_slices
    try:
        for forced in (4, 16, 4 + 256, 16 + 256):
            L.hupr_debug_splitk_slices(forced)
            assert G.wgrad_plan_of(L, c) == wgrad_rule(c.eng, c.B, dout, c.Ci, c.Co, c.k, c.xbf, nbytes, off, forced)[0], forced
    finally:
        L.hupr_debug_splitk_slices(0)
    assert G.wgrad_plan_of(L, c) == want


@pytest.mark.parametrize("c", G.PROJ_CASES, ids=[G.proj_id(c) for c in G.PROJ_CASES])
def test_projection_case_grids(c, L):
    assert G.proj_plan_of(L, c) == c.grid == proj_rule(c.op, c.M, c.C)
    assert L.hupr_mscsa_proj_supported(c.M, c.C) if c.op == "fwd" else L.hupr_mscsa_proj_dgrad_supported(c.M, c.C)


# ---- the model's own shapes -----------------------------------------------------------------------------------------------------------
K333, K133, K111, SAME3, NOPAD = G.K333, G.K133, G.K111, G.SAME3, G.NOPAD
HW = (0, 1, 1)
# (name, input extents, Ci, Co, kernel, pad): every convolution of HuPRNet at numFilters = 32, 8 group frames, 64 x 64 maps
MODEL_CONVS = [("enc1 first 32->64", (8, 64, 64), 32, 64, K333, SAME3), ("enc1 64->64", (8, 64, 64), 64, 64, K333, SAME3),
               ("enc2 64->128", (4, 32, 32), 64, 128, K333, SAME3), ("enc2 128->128", (4, 32, 32), 128, 128, K333, SAME3),
               ("enc3 128->256", (2, 16, 16), 128, 256, K333, SAME3), ("enc3 256->256", (2, 16, 16), 256, 256, K333, SAME3),
               ("merge1", (8, 64, 64), 64, 64, (8, 1, 1), NOPAD), ("merge2", (4, 32, 32), 128, 128, (4, 1, 1), NOPAD),
               ("merge3", (2, 16, 16), 256, 256, (2, 1, 1), NOPAD),
               ("proj level 3", (1, 16, 16), 256, 256, K111, NOPAD), ("proj level 2", (1, 32, 32), 128, 128, K111, NOPAD),
               ("proj level 1", (1, 64, 64), 64, 64, K111, NOPAD),
               ("dec3 1024->256", (1, 16, 16), 1024, 256, K133, HW), ("dec3 256->256", (1, 16, 16), 256, 256, K133, HW),
               ("dec3 256->128", (1, 16, 16), 256, 128, K133, HW), ("dec3 128->128", (1, 16, 16), 128, 128, K133, HW),
               ("dec2 640->128", (1, 32, 32), 640, 128, K133, HW), ("dec2 128->128", (1, 32, 32), 128, 128, K133, HW),
               ("dec2 128->64", (1, 32, 32), 128, 64, K133, HW), ("dec2 64->64", (1, 32, 32), 64, 64, K133, HW),
               ("dec1 320->64", (1, 64, 64), 320, 64, K133, HW), ("dec1 64->64", (1, 64, 64), 64, 64, K133, HW),
               ("dec1 64->32", (1, 64, 64), 64, 32, K133, HW), ("dec1 32->32", (1, 64, 64), 32, 32, K133, HW),
               ("head 32->16", (1, 64, 64), 32, 16, K111, NOPAD)]
BATCHES = (1, 3, 32)
SC, R4, R16, RT = G.SCALAR, G.REDUCE4_4, G.REDUCE4_16, G.REDUCE_T
# fp32 math, per batch 1 / 3 / 32: (forward tile, input-gradient tile, (BM, slices, reduce kernel) of the weight gradient)
F32_PINS = {
    'enc1 first 32->64': (((64, 64), (128, 32), (64, 147, R16)), ((128, 64), (128, 32), (64, 147, R16)), ((128, 64), (128, 32), (64, 147, R16))),
    'enc1 64->64': (((64, 64), (64, 64), (64, 74, R16)), ((128, 64), (128, 64), (64, 74, R16)), ((128, 64), (128, 64), (64, 74, R16))),
    'enc2 64->128': (((64, 128), (64, 64), (128, 74, R16)), ((64, 128), (64, 64), (128, 74, R16)), ((128, 128), (128, 64), (128, 74, R16))),
    'enc2 128->128': (((64, 128), (64, 128), (128, 38, R16)), ((64, 128), (64, 128), (128, 38, R16)), ((128, 128), (128, 128), (128, 38, R16))),
    'enc3 128->256': (((64, 128), (64, 128), (128, 16, RT)), ((64, 128), (64, 128), (128, 19, RT)), ((64, 128), (64, 128), (128, 19, RT))),
    'enc3 256->256': (((64, 128), (64, 128), (128, 10, RT)), ((64, 128), (64, 128), (128, 10, RT)), ((64, 128), (64, 128), (128, 10, RT))),
    'merge1': (((64, 64), (64, 64), (64, 128, R16)), ((64, 64), (128, 64), (64, 256, R16)), ((128, 64), (128, 64), (64, 256, R16))),
    'merge2': (((64, 128), (64, 128), (128, 32, R16)), ((64, 128), (64, 128), (128, 96, R16)), ((64, 128), (128, 128), (128, 256, R16))),
    'merge3': (((64, 128), (64, 128), (128, 8, RT)), ((64, 128), (64, 128), (128, 24, RT)), ((64, 128), (64, 128), (128, 128, R16))),
    'proj level 3': (((64, 128), (64, 128), (128, 8, R4)), ((64, 128), (64, 128), (128, 24, R4)), ((64, 128), (64, 128), (128, 256, R16))),
    'proj level 2': (((64, 128), (64, 128), (128, 32, R16)), ((64, 128), (64, 128), (128, 96, R16)), ((64, 128), (64, 128), (128, 256, R16))),
    'proj level 1': (((64, 64), (64, 64), (64, 128, R16)), ((64, 64), (64, 64), (64, 256, R16)), ((128, 64), (128, 64), (64, 256, R16))),
    'dec3 1024->256': (((64, 128), (64, 128), (128, 8, RT)), ((64, 128), (64, 128), (128, 8, RT)), ((64, 128), (128, 128), (128, 8, RT))),
    'dec3 256->256': (((64, 128), (64, 128), (128, 8, RT)), ((64, 128), (64, 128), (128, 24, RT)), ((64, 128), (64, 128), (128, 29, RT))),
    'dec3 256->128': (((64, 128), (64, 128), (128, 8, RT)), ((64, 128), (64, 128), (128, 24, RT)), ((64, 128), (64, 128), (128, 57, R16))),
    'dec3 128->128': (((64, 128), (64, 128), (128, 8, RT)), ((64, 128), (64, 128), (128, 24, RT)), ((64, 128), (64, 128), (128, 114, R16))),
    'dec2 640->128': (((64, 128), (64, 128), (128, 23, RT)), ((64, 128), (64, 128), (128, 23, RT)), ((64, 128), (128, 128), (128, 23, RT))),
    'dec2 128->128': (((64, 128), (64, 128), (128, 32, R16)), ((64, 128), (64, 128), (128, 96, R16)), ((64, 128), (64, 128), (128, 114, R16))),
    'dec2 128->64': (((64, 64), (64, 128), (64, 32, R16)), ((64, 64), (64, 128), (64, 96, R16)), ((64, 64), (64, 128), (64, 114, R16))),
    'dec2 64->64': (((64, 64), (64, 64), (64, 32, R16)), ((64, 64), (64, 64), (64, 96, R16)), ((64, 64), (64, 64), (64, 205, R16))),
    'dec1 320->64': (((64, 64), (64, 128), (64, 45, R16)), ((64, 64), (64, 128), (64, 45, R16)), ((128, 64), (128, 128), (64, 45, R16))),
    'dec1 64->64': (((64, 64), (64, 64), (64, 128, R16)), ((64, 64), (64, 64), (64, 205, R16)), ((128, 64), (128, 64), (64, 205, R16))),
    'dec1 64->32': (((128, 32), (64, 64), (64, 128, R16)), ((128, 32), (64, 64), (64, 205, R16)), ((128, 32), (128, 64), (64, 205, R16))),
    'dec1 32->32': (((128, 32), (128, 32), (64, 128, R16)), ((128, 32), (128, 32), (64, 256, R16)), ((128, 32), (128, 32), (64, 256, R16))),
    'head 32->16': (((128, 32), (128, 32), (64, 128, R16)), ((128, 32), (128, 32), (64, 256, R16)), ((128, 32), (128, 32), (64, 256, R16))),
}
# bf16 math: the level-3 projections (hupr_conv_fwd_bf16_mixed, C = 256 -> 4 C) and their input gradient (hupr_gemm_bf16, K = 4 C), the
# projection weight gradients of the three levels (hupr_conv_wgrad_bf16, C -> 4 C), the unfused 1 x 1 projections and the head through
# the bf16 engine, the attention fall-back GEMMs of level 3 (N = C = 256).  Same triple layout where a convolution, else the tile.
BF16_PINS = {
    'proj weight gradient level 3': ((128, 4, R4), (128, 12, R4), (128, 20, R4)),
    'unfused 1x1 level 3': (((64, 64), (64, 64), (128, 4, R4)), ((64, 64), (64, 64), (128, 12, R4)), ((64, 64), (64, 64), (128, 64, R16))),
    'proj weight gradient level 2': ((128, 16, R4), (128, 48, R16), (128, 160, R16)),
    'unfused 1x1 level 2': (((64, 64), (64, 64), (128, 16, R4)), ((64, 64), (64, 64), (128, 48, R16)), ((64, 128), (64, 128), (128, 256, R16))),
    'proj weight gradient level 1': ((128, 64, R16), (128, 128, R16), (128, 256, R16)),
    'unfused 1x1 level 1': (((64, 64), (64, 64), (64, 64, R16)), ((64, 64), (64, 64), (64, 192, R16)), ((128, 64), (128, 64), (64, 256, R16))),
    'proj level 3 forward': ((64, 64), (64, 64), (128, 128)),
    'proj level 3 input gradient': ((64, 64), (64, 64), (64, 64)),
    'head 32->16': (((64, 64), (64, 64), (64, 64, R16)), ((64, 64), (64, 64), (64, 192, R16)), ((128, 64), (128, 64), (64, 256, R16))),
    'attention fall-back (0, 1)': ((64, 64), (64, 64), (64, 64)),
    'attention fall-back (0, 0)': ((64, 64), (64, 64), (64, 64)),
    'attention fall-back (1, 0)': ((64, 64), (64, 64), (64, 64)),
}


def conv_routes(L, eng, B, din, Ci, Co, k, pad):
    """(forward tile, input-gradient tile, (BM, slices, reduce kernel)) of one convolution, library and rule agreeing."""
    dout = G.out_extent(din, k, pad)
    cog = cdiv(Co, 32) * 32                          # functional.ConvFn zero-pads the input gradient's K axis to a multiple of 32
    fw = G.plan(L, eng, 1, [B, *din, Ci, Ci, *dout, Co, *k, *pad, 0, 0, 0, 0])
    dg = G.plan(L, eng, 1, [B, *dout, cog, cog, *din, Ci, *k, *(t - 1 - p for t, p in zip(k, pad)), 0, 0, 0, 0])
    ws = L.hupr_conv_wgrad_ws_bytes(B, *dout, Ci, Co, *k)
    wg = G.plan(L, eng, 2, [B, *din, Ci, Ci, *dout, Co, *k, *pad, 0], ws)
    assert fw == tile_rule(eng, B * G.vox(dout), Co, 1) and dg == tile_rule(eng, B * G.vox(din), Ci, 1)
    assert wg == wgrad_rule(eng, B, dout, Ci, Co, k, 0, ws)[0]
    return fw[:2], dg[:2], (wg[0], wg[2], wg[3])


def test_model_shapes_keep_their_routes_fp32_math(L):
    assert [m[0] for m in MODEL_CONVS] == list(F32_PINS)
    for name, din, Ci, Co, k, pad in MODEL_CONVS:
        got = tuple(conv_routes(L, "f32", B, din, Ci, Co, k, pad) for B in BATCHES)
        assert got == F32_PINS[name], (name, got)


def test_model_shapes_keep_their_routes_bf16_math(L):
    got = {}
    for lvl, (H, C) in ((3, (16, 256)), (2, (32, 128)), (1, (64, 64))):
        got["proj weight gradient level %d" % lvl] = tuple(conv_routes(L, "bf16", B, (1, H, H), C, 4 * C, K111, NOPAD)[2] for B in BATCHES)
        got["unfused 1x1 level %d" % lvl] = tuple(conv_routes(L, "bf16", B, (1, H, H), C, C, K111, NOPAD) for B in BATCHES)
    got["proj level 3 forward"] = tuple(conv_routes(L, "bf16", B, (1, 16, 16), 256, 1024, K111, NOPAD)[0] for B in BATCHES)
    got["proj level 3 input gradient"] = tuple(G.plan(L, "bf16", 0, [0, 0, B * 256, 256, 1024, 1])[:2] for B in BATCHES)
    got["head 32->16"] = tuple(conv_routes(L, "bf16", B, (1, 64, 64), 32, 16, K111, NOPAD) for B in BATCHES)
    for ta, tb in G.MODES:
        r = tuple(G.plan(L, "bf16", 0, [ta, tb, 256, 256, 256, B]) for B in BATCHES)
        assert r == tuple(tile_rule("bf16", 256, 256, B) for B in BATCHES)
        got["attention fall-back (%d, %d)" % (ta, tb)] = tuple(x[:2] for x in r)
    assert got == BF16_PINS, got
    # the fused kernels take the projections of levels 1 and 2 and the input gradient of level 1; level 3 (C = 256) stays on the engine
    for B in BATCHES:
        assert L.hupr_mscsa_proj_supported(B * 4096, 64) and L.hupr_mscsa_proj_supported(B * 1024, 128) and not L.hupr_mscsa_proj_supported(B * 256, 256)
        assert L.hupr_mscsa_proj_dgrad_supported(B * 4096, 64) and not L.hupr_mscsa_proj_dgrad_supported(B * 1024, 128)
        assert G.proj_grid(L, 0, B * 4096, 64) == proj_rule("fwd", B * 4096, 64) == (1024, min(256, 16 * B), 1)
        assert G.proj_grid(L, 0, B * 1024, 128) == proj_rule("fwd", B * 1024, 128) == (512, min(256, 8 * B), 2)
        assert G.proj_grid(L, 1, B * 4096, 64) == proj_rule("dgrad", B * 4096, 64) == (512, min(256, 32 * B), 1)


# ---- coverage of the tables ---------------------------------------------------------------------------------------------------------
def test_the_tables_reach_every_template_instantiation():
    f32_tiles, bf16_tiles = {(128, 128), (64, 128), (128, 64), (64, 64), (128, 32)}, {(128, 128), (64, 128), (128, 64), (64, 64)}
    for e, tiles in (("f32", f32_tiles), ("bf16", bf16_tiles)):
        # launch<BM, BN, .., A_ROWK | A_KM, B_NK | B_KN>: every tile in every operand mode
        assert {(c.ta, c.tb, c.tile[e]) for c in G.GEMM_CASES} == {(ta, tb, t) for ta, tb in G.MODES for t in tiles}, e
        # <.., A_CONV, B_NK>
        assert {c.tile for c in G.CONV_CASES if c.eng == e} == tiles, e
        # <64 | 128, 128, .., A_KM, B_CONVK>
        assert {c.route[0] for c in G.WGRAD_CASES if c.eng == e} == {64, 128}, e
    src = open(os.path.join(CSRC, "gemm_f32.hip")).read() + open(os.path.join(CSRC, "gemm_bf16.hip")).read()
    inst = set(re.findall(r"launch(?:_h)?<(\d+), (\d+), \d, \d, (\w+), (\w+)>", src))
    assert {(int(bm), int(bn)) for bm, bn, am, bmd in inst if am == "AM"} == f32_tiles          # the dispatchers name no other tile
    assert {(bm, bn) for bm, bn, am, bmd in inst if am == "A_KM" and bmd == "B_CONVK"} == {("64", "128"), ("128", "128")}


def test_the_tables_reach_every_reduce_kernel_split_branch_and_edge():
    for e in G.ENGINES:
        mine = [c for c in G.WGRAD_CASES if c.eng == e]
        assert {c.route[3] for c in mine} == {G.SCALAR, G.REDUCE4_4, G.REDUCE4_16, G.REDUCE_T}, e
        assert {"ktiles", "256", "1024/tiles", "shrink"} <= {c.why for c in mine}
        assert any(c.Co % 4 for c in mine) and any(c.lds[1] % 2 for c in mine) and any(c.lds[1] and not c.lds[1] % 2 for c in mine)
        assert all(c.Ci < 128 for c in mine if G.vox(c.k) > 1 and c.why == "ktiles")          # N tiles that span several taps
        # an empty slice: fewer K tiles than slices x tiles per slice
        empty = [c for c in mine if "empty-slice" in c.name]
        for c in empty:
            kt = cdiv(c.B * G.vox(G.out_extent(c.din, c.k, c.pad)), 32 if e == "f32" else 64)
            assert kt == 9 and c.route[2] == 4 and 3 * cdiv(kt, 4) >= kt
        assert empty
    assert {"cap", "floor"} <= {c.why for c in G.WGRAD_CASES if c.eng == "bf16"}
    assert any(c.xbf and c.why == "cap" for c in G.WGRAD_CASES) and any(c.xbf for c in G.WGRAD_CASES if G.vox(c.k) > 1)
    slices = {c.route[2] for c in G.WGRAD_CASES}
    assert {1, 2, 3, 33, 256} <= slices
    assert {(c.route[3], G.vox(c.k) > 1) for c in G.WGRAD_CASES} >= {(G.SCALAR, True), (G.SCALAR, False), (G.REDUCE4_4, True), (G.REDUCE4_4, False)}
    assert {G.vox(c.k) for c in G.WGRAD_CASES if c.route[3] == G.REDUCE_T} >= {27, 9}
    assert any(c.Ci == 8 and G.vox(c.k) > 1 and c.route[3] == G.REDUCE4_4 for c in G.WGRAD_CASES)
    # the eight-loads-in-flight loop k += S * U wraps at 33 slices for S = 4 (forced) and at 256 for S = 16
    assert {c.route[2] for c in G.FORCED} >= {4, 33, 256, 147} and any(c.route[3] == G.REDUCE_T for c in G.FORCED)
    # batched GEMM: K edges in every operand mode, leading dimensions, epilogues
    for ta, tb in G.MODES:
        ks = {c.K for c in G.GEMM_CASES if (c.ta, c.tb) == (ta, tb)}
        assert 1 in ks and any(k % 4 for k in ks) and {33, 65} & ks and {32, 64, 128} & ks and any(k < 32 for k in ks), (ta, tb, ks)
    assert {c.K for c in G.GEMM_CASES} >= {1, 3, 31, 32, 33, 64, 65, 128}
    assert any(c.M % 4 and c.N % 4 for c in G.GEMM_CASES)
    lds = [G.gemm_lds(c) for c in G.GEMM_CASES]
    assert any(l[2] % 4 for l in lds) and any(l[2] % 4 == 0 for l in lds) and any(l[3] % 4 for l in lds) and any(l[3] % 4 == 0 for l in lds)
    for epi in ("res", "acc", "res acc"):
        mine = [(c, G.gemm_lds(c)) for c in G.GEMM_CASES if c.epi == epi]
        assert any(l[4] % 2 for _, l in mine) and any(l[4] % 4 == 0 for _, l in mine), epi
    assert any(l[5] % 2 and "res" in c.epi for c, l in zip(G.GEMM_CASES, lds)) and any(c.bcast for c in G.GEMM_CASES)
    blocks = {cdiv(c.M, 128) * cdiv(c.N, 128) * c.batch for c in G.GEMM_CASES if c.N > 64 and c.M > 64}
    assert {511, 512} <= blocks
    assert {c.N for c in G.GEMM_CASES} >= {64, 65, 32, 33} and {c.M for c in G.GEMM_CASES} >= {64, 65}
    # convolutions
    for e in G.ENGINES:
        mine = [c for c in G.CONV_CASES if c.eng == e]
        assert {c.k for c in mine} >= {K333, K133, K111, (4, 1, 1)} and {c.pad for c in mine if c.k == K333} >= {SAME3, NOPAD, (0, 1, 1)}
        assert any(c.dgrad and c.pad != SAME3 for c in mine) and any(c.dgrad and c.k == (4, 1, 1) for c in mine)
        ext = [c.din for c in mine]
        assert (3, 5, 7) in ext and any(1023 in d and 1 in d for d in ext) and {d.index(1023) for d in ext if 1023 in d} == {0, 1, 2}
        assert any(c.B * G.vox(G.out_extent(c.din, c.k, c.pad)) == 63 for c in mine)
        assert {c.B * G.vox(c.din) for c in mine} >= {65536, 65535, 65408}
        assert {c.Co for c in mine if not c.dgrad} >= {16, 20, 40, 72}
        epis = {w for c in mine for w in c.epi.split()}
        assert epis >= {"bias", "res", "acc", "inplace"} and any(c.epi == "bias res acc" for c in mine)
        assert any(c.lds[0] and c.lds[1] for c in mine) and any(c.lds[2] and c.lds[3] for c in mine) and any(c.lds[4] % 2 for c in mine)
        assert any(c.lds[2] % 2 for c in mine)
    assert {c.Ci for c in G.CONV_CASES if c.eng == "bf16" and not c.dgrad} >= {8, 24}
    assert {c.store for c in G.CONV_CASES} >= {"x16", "y16", "x16 y16", "f32"}
    # projections
    for op, C, step in (("fwd", 64, 256), ("fwd", 128, 128), ("dgrad", 64, 128)):
        ms = {c.M for c in G.PROJ_CASES if (c.op, c.C) == (op, C)}
        wrap = 256 * step
        assert {16, 17, 31, step, step + 1, wrap} <= ms
        uneven = [m for m in ms if m > wrap]
        assert any(m % 16 for m in uneven) and any(m % 16 == 0 and m % step for m in uneven)
    assert {c.res for c in G.PROJ_CASES if c.op == "dgrad"} == {True, False}


def exported(source):
    txt = open(os.path.join(CSRC, source)).read()
    return set(re.findall(r'extern "C" \w[\w \*]*?\b(hupr_\w+)\(', txt))


def test_every_entry_point_of_the_three_sources_is_named():
    names = exported("gemm_f32.hip") | exported("gemm_bf16.hip") | exported("projection.hip")
    assert len(names) == 18, sorted(names)
    src = open(os.path.join(ROOT, "tests", "test_gemm_fp64_gpu.py")).read()
    called = set(re.findall(r"\b(hupr_\w+)\b", src))
    called |= {"hupr_gemm_" + e for e in G.ENGINES}                            # (spelled "hupr_gemm_" + engine there)
    assert names <= called, sorted(names - called)
    assert {G.conv_entry(c) for c in G.CONV_CASES} == {"hupr_conv_fwd_f32", "hupr_conv_fwd_bf16", "hupr_conv_fwd_bf16_mixed"}
    assert {G.wgrad_entry(c) for c in G.WGRAD_CASES} == {"hupr_conv_wgrad_f32", "hupr_conv_wgrad_bf16", "hupr_conv_wgrad_bf16_mixed"}


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", G.REFUSED, ids=[r[0] for r in G.REFUSED])
def test_refused_calls_are_refused_by_the_plan_alone(r, L):
    """The plan refuses; and the entry point, on made-up addresses and without a device, returns the same code before anything is
    launched or dereferenced."""
    want = G.HUPR_ERR_WORKSPACE if r[1] == "wgrad-ws" else G.HUPR_ERR_ARG
    assert G.refused_plan(L, r) == want, r[0]
    n0 = L.hupr_launch_count()
    assert G.refused_call(L, r, 1 << 24, 2 << 24, 3 << 24, 4 << 24, None) in (want, None), (r[0], L.hupr_last_error())
    assert L.hupr_launch_count() == n0


@pytest.mark.parametrize("r", G.PROJ_REFUSED, ids=[r[0] for r in G.PROJ_REFUSED])
def test_refused_projections_are_refused_by_host_checks(r, L):
    n0 = L.hupr_launch_count()
    rcs = G.proj_refused_call(L, r, 1 << 24, 2 << 24, 3 << 24, None)
    assert rcs and all(rc == G.HUPR_ERR_ARG for rc in rcs), (r[0], rcs)
    assert L.hupr_launch_count() == n0
    if not r[4]:
        assert G.proj_grid(L, int(r[1] == "dgrad"), r[2], r[3]) == G.HUPR_ERR_ARG


def test_refusal_tables_cover_the_issue_list(L):
    whats = " | ".join(r[0] for r in G.REFUSED)
    for e in G.ENGINES:
        for frag in ("gemm: batch 65536", "gemm: M = 0", "gemm: N = -1", "gemm: K = 0", "gemm: batch 0", "gemm: A^T B^T", "conv: extent 1024",
                     "conv: Ci not a multiple", "wgrad: workspace below one partial tensor"):
            assert "%s %s" % (e, frag) in whats
    assert "bf16 output with accumulate" in whats and "bf16 output with a residual" in whats
    pw = " | ".join(r[0] for r in G.PROJ_REFUSED)
    for frag in ("fwd C = 256", "fwd C = 32", "fwd M = 15", "dgrad C = 128", "4 bytes off", "8 bytes off"):
        assert frag in pw
    # the bounds themselves: batch 65 535 and an extent of 1023 pass
    assert G.plan(L, "f32", 0, [0, 1, 8, 8, 8, 65535]) == (128, 32, 1, 65535, 0, 0)
    assert G.plan(L, "bf16", 1, G._with(G.C_OK, Di=1023, Do=1023))[:2] == (64, 64)
    assert G.plan(L, "f32", 3, G.G_OK) == G.HUPR_ERR_ARG and G.plan(L, "f32", -1, G.G_OK) == G.HUPR_ERR_ARG
    assert L.hupr_debug_gemm_route(2, 0, None, 0, 0, None) == G.HUPR_ERR_ARG and G.proj_grid(L, 2, 64, 64) == G.HUPR_ERR_ARG


# ---- gate sensitivity, on CPU fp64 data ----------------------------------------------------------------------------------------------
def stored(t, bf16=False):
    """What a kernel would leave in memory of the sums t: one rounding to fp32, one more to bf16 behind a bf16 store."""
    return t.float().to(torch.bfloat16) if bf16 else t.float()


def _rejects(ok, bad, ref, what, frac):
    """ok: the gate on the stored faulty result; it must fail at >= frac of the outputs the fault touches (at one at least) and nowhere else."""
    touched = (bad != ref) | bad.isnan()
    n, caught = int(touched.sum()), int((~ok & touched).sum())
    assert n > 0, what
    assert caught >= max(1, frac * n), (what, caught, n)
    assert not bool((~ok & ~touched).any()), what


def gate(engine, op, out, ref, A, bf16=False):
    return G.within(stored(out, bf16), ref, A, G.GATE_C[(engine, op)], bf16)


@pytest.fixture(scope="module")
def gemm_data():
    c = G.GCase(0, 1, 70, 66, 65, 2, (0, 0, 0, 0), "res acc", False, None)
    A_, B_ = G.rnd(2, 70, 65, seed=1), G.rnd(2, 66, 65, seed=2)
    res, old = G.rnd(2, 70, 66, seed=3).double(), G.rnd(2, 70, 66, seed=4).double()
    return c, A_, B_, res, old


@pytest.mark.parametrize("engine", G.ENGINES)
def test_gemm_gate_accepts_honest_fp32_and_rejects_wrong_results(engine, gemm_data):
    c, A_, B_, res, old = gemm_data
    a, b = G.operand(A_, engine), G.operand(B_, engine)
    ref, A = G.gemm_ref(c, a, b, res, old)
    assert bool(gate(engine, "gemm", ref, ref, A).all())
    # an honest fp32 evaluation in another order: k descending, one fp32 accumulator, the epilogue terms first
    acc = (res + old).float()
    for k in reversed(range(c.K)):
        acc = acc + a[:, :, k:k + 1].float() * b[:, :, k].float().unsqueeze(1)
    assert bool((acc.double() != ref).any()) and bool(gate(engine, "gemm", acc.double(), ref, A).all())
    # one k term dropped from one element
    bad = ref.clone()
    bad[1, 69, 65] -= a[1, 69, 64] * b[1, 65, 64]
    _rejects(gate(engine, "gemm", bad, ref, A), bad, ref, "one k term dropped", 1.0)
    # residual omitted / added twice; accumulate ignoring the old value; the last row unwritten (it keeps the old C)
    for what, bad in (("residual omitted", ref - res), ("residual twice", ref + res), ("old value ignored", ref - old)):
        _rejects(gate(engine, "gemm", bad, ref, A), bad, ref, what, 0.99)
    bad = ref.clone()
    bad[:, -1] = old[:, -1]
    _rejects(gate(engine, "gemm", bad, ref, A), bad, ref, "last row unwritten", 0.95)
    bad[:, -1] = float("nan")
    _rejects(gate(engine, "gemm", bad, ref, A), bad, ref, "last row left NaN", 1.0)
    if engine == "bf16":
        # one operand left un-rounded
        bad = G.gemm_ref(c, A_.double(), b, res, old)[0]
        _rejects(gate(engine, "gemm", bad, ref, A), bad, ref, "A not rounded to bf16", 0.5)


@pytest.fixture(scope="module")
def conv_data():
    B, din, Ci, Co, k, pad = 2, (3, 5, 7), 8, 20, K333, SAME3
    x, w = G.rnd(B, *din, Ci, seed=5), G.rnd(Co, Ci, *k, seed=6) * (27 * Ci) ** -0.5
    bias, res = G.rnd(Co, seed=7).double(), G.rnd(B, *din, Co, seed=8).double()
    dy = G.rnd(B, *din, Co, seed=9)
    return din, k, pad, x, w, bias, res, dy


@pytest.mark.parametrize("engine", G.ENGINES)
def test_conv_gates_accept_honest_fp32_and_reject_wrong_results(engine, conv_data):
    din, k, pad, x, w, bias, res, dy = conv_data
    xd, wd, dyd = G.operand(x, engine), G.operand(w, engine), G.operand(dy, engine)
    ref, A = G.conv_ref(xd, wd, k, pad)
    ref, A = ref + bias + res, A + bias.abs() + res.abs()
    for bf16 in (False, True):
        assert bool(gate(engine, "conv", ref, ref, A, bf16).all())
    # an honest fp32 evaluation: taps in reversed order, channels summed in fp32
    acc = (bias + res).float()
    for tap in reversed(G.taps_of(k)):
        (od, oh, ow), (i_d, ih, iw) = G._slices(din, din, tap, pad)
        acc[:, od, oh, ow] += (xd[:, i_d, ih, iw].float().unsqueeze(-2) * wd[(slice(None), slice(None)) + tap].float()).flip(-1).sum(-1)
    assert bool((acc.double() != ref).any()) and bool(gate(engine, "conv", acc.double(), ref, A).all())
    extra = bias + res
    swap = lambda t: {(0, 1, 2): (2, 1, 0), (2, 1, 0): (0, 1, 2)}.get(t, t)
    mutations = [("two taps swapped", G.conv_ref(xd, wd, k, pad, tap_map=swap)[0] + extra, 0.9),
                 ("taps reversed", G.conv_ref(xd, wd, k, pad, tap_map=lambda t: tuple(2 - i for i in t))[0] + extra, 0.95),
                 ("bias shifted by one column", ref - bias + bias.roll(1), 0.95), ("residual omitted", ref - res, 0.99),
                 ("residual twice", ref + res, 0.99)]
    dropped = ref.clone()                                      # one border voxel loses one tap: the (0, 0, 0) tap of the last voxel
    dropped[1, 2, 4, 6] -= xd[1, 1, 3, 5] @ wd[:, :, 0, 0, 0].t()
    mutations.append(("one tap dropped on one border voxel", dropped, 0.9))
    for what, bad, frac in mutations:
        _rejects(gate(engine, "conv", bad, ref, A), bad, ref, what, frac)
        _rejects(gate(engine, "conv", bad, ref, A, True), bad, ref, what + " (bf16 store)", 0.5 * frac)
    # the input gradient with the tap reversal of pack mode 1 missing
    rd, Ad = G.dgrad_ref(dyd, wd, k, pad, din)
    bad = G.dgrad_ref(dyd, wd.flip(2, 3, 4), k, pad, din)[0]
    assert bool(gate(engine, "conv", rd, rd, Ad).all())
    _rejects(gate(engine, "conv", bad, rd, Ad), bad, rd, "mode 1 without tap reversal", 0.95)
    # weight gradient: two taps swapped, one empty slice contributing the NaN pattern, one voxel dropped from one element
    rw, Aw = G.wgrad_ref(xd, dyd, k, pad)
    assert bool(gate(engine, "wgrad", rw, rw, Aw).all())
    acc = torch.zeros_like(rw, dtype=torch.float32)             # fp32 partial sums per sample, then added: another slice order
    for b_ in reversed(range(xd.shape[0])):
        acc = acc + G.wgrad_ref(xd[b_:b_ + 1], dyd[b_:b_ + 1], k, pad)[0].float()
    assert bool(gate(engine, "wgrad", acc.double(), rw, Aw).all())
    bad = rw.clone()
    bad[:, :, 0, 1, 2], bad[:, :, 2, 1, 0] = rw[:, :, 2, 1, 0], rw[:, :, 0, 1, 2]
    _rejects(gate(engine, "wgrad", bad, rw, Aw), bad, rw, "wgrad: two taps swapped", 0.95)
    bad = rw + torch.tensor(G.NAN32, dtype=torch.int32).view(torch.float32).double()
    assert not bool(gate(engine, "wgrad", bad, rw, Aw).any())
    bad = rw.clone()
    bad[19, 7, 1, 1, 1] -= dyd[0, 1, 2, 3, 19] * xd[0, 1, 2, 3, 7]
    _rejects(gate(engine, "wgrad", bad, rw, Aw), bad, rw, "wgrad: one voxel dropped from one element", 1.0)
    if engine == "bf16":
        bad = G.conv_ref(x.double(), wd, k, pad)[0] + extra
        _rejects(gate(engine, "conv", bad, ref, A), bad, ref, "x not rounded to bf16", 0.5)
        bad = G.wgrad_ref(xd, dy.double(), k, pad)[0]
        _rejects(gate(engine, "wgrad", bad, rw, Aw), bad, rw, "dy not rounded to bf16", 0.5)


def test_projection_gates_accept_honest_fp32_and_reject_wrong_results():
    C, M = 64, 48
    x, wc = G.rnd(M, C, seed=10), G.rnd(4 * C, C, seed=11) * C ** -0.5
    dy, res = G.rnd(M, 4 * C, seed=12), G.rnd(M, C, seed=13)
    fw, dg = G.PCase("fwd", C, M, None, False), G.PCase("dgrad", C, M, None, True)
    ref, A = G.proj_reference(fw, x, wc, None)
    rd, Ad = G.proj_reference(dg, dy, wc, res)
    assert bool(gate("bf16", "proj_fwd", ref, ref, A, True).all()) and bool(gate("bf16", "proj_dgrad", rd, rd, Ad).all())
    acc = torch.zeros(M, 4 * C)
    for k in reversed(range(C)):
        acc = acc + G.q(x)[:, k:k + 1].float() * G.q(wc)[:, k].float()
    assert bool(gate("bf16", "proj_fwd", acc.double(), ref, A, True).all())
    acc = res.clone()
    for k in reversed(range(4 * C)):
        acc = acc + G.q(dy)[:, k:k + 1].float() * G.q(wc)[k].float()
    assert bool((acc.double() != rd).any()) and bool(gate("bf16", "proj_dgrad", acc.double(), rd, Ad).all())

    def groups_swapped(t):                                     # two 4-channel groups exchanged within every 16-channel block
        t = t.clone().view(t.shape[0], -1, 4, 4)
        t[:, :, [1, 2]] = t[:, :, [2, 1]]
        return t.view(t.shape[0], -1)
    for what, bad, r_, A_, op, bf16, frac in (
            ("fwd: 4-channel groups swapped", groups_swapped(ref), ref, A, "proj_fwd", True, 0.9),
            ("dgrad: 4-channel groups swapped", groups_swapped(rd), rd, Ad, "proj_dgrad", False, 0.99),
            ("dgrad: residual omitted", rd - res.double(), rd, Ad, "proj_dgrad", False, 0.99),
            ("dgrad: residual twice", rd + res.double(), rd, Ad, "proj_dgrad", False, 0.99),
            ("fwd: x not rounded", x.double() @ G.q(wc).t(), ref, A, "proj_fwd", True, 0.15),
            ("dgrad: dY not rounded", dy.double() @ G.q(wc) + res.double(), rd, Ad, "proj_dgrad", False, 0.5)):
        _rejects(gate("bf16", op, bad, r_, A_, bf16), bad, r_, what, frac)
    for r_, A_, op, bf16 in ((ref, A, "proj_fwd", True), (rd, Ad, "proj_dgrad", False)):
        bad = r_.clone()
        bad[-1] = float("nan")                                  # the last row unwritten
        _rejects(gate("bf16", op, bad, r_, A_, bf16), bad, r_, op + ": last row unwritten", 1.0)
        bad = r_.clone()
        bad[5, 9] -= (G.q(x)[5, 63] * G.q(wc)[9, 63]) if op == "proj_fwd" else (G.q(dy)[5, 255] * G.q(wc)[255, 9])
        if not bf16:
            _rejects(gate("bf16", op, bad, r_, A_, bf16), bad, r_, op + ": one k term dropped", 1.0)


def test_gate_constants_are_powers_of_two_inside_the_cap():
    for key, c in G.GATE_C.items():
        assert 0 < c <= G.CAP and float(torch.log2(torch.tensor(c))).is_integer(), key
