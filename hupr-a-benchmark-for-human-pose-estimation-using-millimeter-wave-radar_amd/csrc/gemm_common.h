// Shared argument structures of the GEMM / implicit-GEMM convolution engines (fp32 and bf16 MFMA).
#pragma once
#include "hupr_common.h"

namespace hupr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum AMode { A_ROWK = 0, A_CONV = 1, A_KM = 2 };
enum BMode { B_NK = 0, B_KN = 1, B_CONVK = 2 };

struct ConvGeom {
    int Di, Hi, Wi, Ci;       // input voxels / channels taken part in the GEMM
    int in_ld;                // floats between consecutive voxels of the input buffer
    int Do, Ho, Wo;           // output voxels
    int kd, kh, kw;           // taps
    int pd, ph, pw;           // zero padding
};

struct GemmArgs {
    const float* A;
    const float* B;
    float* C;
    int M, N, K;
    long lda, ldb, ldc;
    // batch: z -> (z / zdiv, z % zdiv), pointer += z0 * bs0 + z1 * bs1
    int zdiv;
    long a_bs0, a_bs1, b_bs0, b_bs1, c_bs0, c_bs1;
    ConvGeom g;
    const float* bias;        // [N] or null
    const float* res;         // residual added in the epilogue, same indexing as C with res_ld
    long res_ld, res_bs0, res_bs1;
    int ksplit;               // >1: grid.y slices K, partial tiles go to C + slice*M*ldc... (see host)
    long split_stride;        // floats between partial outputs
    int accumulate;           // 1: C += result (read-modify-write; not with ksplit)
    int flags;                // bf16 engine only: GEMM_A_BF16 / GEMM_B_BF16 / GEMM_C_BF16 (tensor stored as bf16 in HBM)
};
enum { GEMM_A_BF16 = 1, GEMM_B_BF16 = 2, GEMM_C_BF16 = 4 };


inline void fill_common(GemmArgs& a) {
    a.zdiv = 1;
    a.a_bs0 = a.a_bs1 = a.b_bs0 = a.b_bs1 = a.c_bs0 = a.c_bs1 = 0;
    a.bias = nullptr;
    a.res = nullptr;
    a.res_ld = a.res_bs0 = a.res_bs1 = 0;
    a.ksplit = 1;
    a.split_stride = 0;
    a.accumulate = 0;
    a.flags = 0;
    a.g = ConvGeom{};
}

inline int check_geom(const char* who, int Bn, const ConvGeom& g, int Co, int ci_mult) {
    HUPR_REQUIRE(Bn > 0 && g.Di > 0 && g.Hi > 0 && g.Wi > 0 && g.Do > 0 && g.Ho > 0 && g.Wo > 0,
                 "%s: bad geometry", who);
    HUPR_REQUIRE(g.Ci % ci_mult == 0, "%s: Cin=%d must be a multiple of %d", who, g.Ci, ci_mult);
    HUPR_REQUIRE(g.Do < 1024 && g.Ho < 1024 && g.Wo < 1024, "%s: extent >= 1024", who);
    HUPR_REQUIRE(g.in_ld % 4 == 0, "%s: input voxel stride %d not a multiple of 4 floats", who, g.in_ld);
    HUPR_REQUIRE(Co > 0, "%s: Cout=%d", who, Co);
    return HUPR_OK;
}

// split-K partial reduction + optional [Co][taps][Ci] -> (Co,Ci,taps) relayout (gemm_f32.hip)
// Voxel-axis slices of the GEMM-form weight gradient: enough workgroups for ~4 per CU, at most 256 slices and at most
// 256 MiB of partials (a 64x64 1x1 weight over 131k voxels used to run on 64 workgroups: a quarter of the chip).
// in_bytes (optional): bytes of the two operands.  Every slice writes one partial tensor that the reduction reads back, so the
// slices are also capped where that round trip would exceed the operands themselves (a 1024 x 256 gradient over 8 192 voxels
// ran 64 slices: 134 MB of partial traffic against 42 MB of input) — but never below one workgroup per CU.
inline int wgrad_splits(long tiles, long ktiles, size_t one_bytes, size_t in_bytes = 0) {
    long s = (1024 + tiles - 1) / tiles;
    if (in_bytes) {
        const long cap = (long)(in_bytes / (2 * one_bytes));
        const long floor_ = (256 + tiles - 1) / tiles;
        if (s > cap) s = cap > floor_ ? cap : floor_;
    }
    if (s > 256) s = 256;
    if (s > ktiles) s = ktiles;
    while (s > 1 && (size_t)s * one_bytes > ((size_t)256 << 20)) s >>= 1;
    return (int)(s < 1 ? 1 : s);
}
void launch_splitk_reduce(const float* part, float* out, long n, int splits, long split_stride, int taps, int ci,
                          hipStream_t s, float* out2 = nullptr, long n_first = 0);

// ---- launch plans ---------------------------------------------------------------------------------------------------------------
// Every launch decision of the two engines is made once, here, for the launchers and for hupr_debug_gemm_route: the argument checks
// (all but the pointers), the tile, the grid, and for a weight gradient the K slices, the workspace it needs and the reduce kernel.
// engine: 0 = gemm_f32.hip (32-deep K tiles), 1 = gemm_bf16.hip (64-deep).

struct GemmPlan {
    int bm, bn;               // block tile
    int grid_x, grid_z;       // output tiles, batch
};

// Largest tile that still gives >= ~2 workgroups per CU (256 CUs); N tile from N.  The fp32 engine has a 128 x 32 tile for N <= 32
// and keeps 64 x 128 for a small wide problem; the bf16 engine sends small problems (level-0 attention GEMMs) to 64 x 64.
inline void gemm_tile_plan(int engine, int M, int N, int batch, GemmPlan* p) {
    auto blocks = [&](int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * batch; };
    int bm, bn;
    if (N > 64) {
        if (M > 64 && blocks(128, 128) >= 512) { bm = 128; bn = 128; }
        else if (engine == 0 || blocks(64, 128) >= 512) { bm = 64; bn = 128; }
        else { bm = 64; bn = 64; }
    } else if (N > 32 || engine == 1) {
        if (M > 64 && blocks(128, 64) >= 512) { bm = 128; bn = 64; }
        else { bm = 64; bn = 64; }
    } else {
        bm = 128; bn = 32;
    }
    p->bm = bm; p->bn = bn;
    p->grid_x = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
    p->grid_z = batch;
}

// batched GEMM (hupr_gemm_f32 / hupr_gemm_bf16): C = op(A) op(B), (ta, tb) in {(0, 1), (0, 0), (1, 0)}
inline int gemm_plan(const char* who, int engine, int ta, int tb, int M, int N, int K, int batch, GemmPlan* p) {
    HUPR_REQUIRE(M > 0 && N > 0 && K > 0 && batch > 0, "%s: bad shape %d %d %d x%d", who, M, N, K, batch);
    HUPR_REQUIRE(batch <= 65535, "%s: batch %d > 65535", who, batch);
    HUPR_REQUIRE((ta == 0 && (tb == 0 || tb == 1)) || (ta == 1 && tb == 0), "%s: unsupported transpose combination %d %d", who, ta, tb);
    gemm_tile_plan(engine, M, N, batch, p);
    return HUPR_OK;
}

// forward convolution / input gradient (A_CONV x B_NK): M = output voxels, N = Co.  flags: GEMM_A_BF16 / GEMM_C_BF16 (bf16 engine)
inline int conv_fwd_plan(const char* who, int engine, int Bn, const ConvGeom& g, int Co, int flags, int accumulate, bool has_res,
                         GemmPlan* p) {
    int rc = check_geom(who, Bn, g, Co, engine == 0 ? 32 : 8);
    if (rc) return rc;
    HUPR_REQUIRE(g.Do == g.Di + 2 * g.pd - g.kd + 1 && g.Ho == g.Hi + 2 * g.ph - g.kh + 1 && g.Wo == g.Wi + 2 * g.pw - g.kw + 1,
                 "%s: output extent does not match stride-1 convolution", who);
    HUPR_REQUIRE(!(flags & GEMM_C_BF16) || (!accumulate && !has_res), "%s: bf16 output excludes accumulate/residual", who);
    const long M = (long)Bn * g.Do * g.Ho * g.Wo;
    HUPR_REQUIRE(M < (1L << 31), "%s: too many output voxels", who);
    gemm_tile_plan(engine, (int)M, Co, 1, p);
    return HUPR_OK;
}

enum SplitkKernel { SPLITK_SCALAR = 0, SPLITK_REDUCE4_4 = 1, SPLITK_REDUCE4_16 = 2, SPLITK_REDUCE_T_4_8 = 3 };
struct SplitkPlan {
    int kernel;               // SplitkKernel
    int grid;
};
// the reduce kernel of launch_splitk_reduce (gemm_f32.hip) and its workgroups, under hupr_debug_splitk_slices as set.  n_one: the
// elements of ONE gradient (n, or n_first where two gradients share the tensor); part_aligned: the partials start on 16 bytes
SplitkPlan splitk_reduce_plan(long n, long n_one, int splits, long split_stride, int taps, int ci, bool part_aligned, bool rows_ok);

struct WgradPlan {
    int bm, grid_x;           // 64 x 128 or 128 x 128 tiles over (Co, taps * Ci)
    int splits;               // K slices = partial tensors (grid.y), after the caps and the workspace-shrink loop
    size_t ws_need;           // bytes of workspace the launch writes
    SplitkPlan red;
};
// weight gradient (A_KM x B_CONVK): M = Co, N = taps * Ci, K = output voxels, sliced so the grid fills the chip.  Returns
// HUPR_ERR_WORKSPACE (with ws_need = one partial tensor) where even one slice does not fit.
inline int wgrad_plan(const char* who, int engine, int Bn, const ConvGeom& g, int Co, int x_bf16, size_t ws_bytes, bool ws_aligned,
                      WgradPlan* p) {
    int rc = check_geom(who, Bn, g, Co, engine == 0 ? 32 : 4);
    if (rc) return rc;
    const long Mv = (long)Bn * g.Do * g.Ho * g.Wo;
    HUPR_REQUIRE(Mv < (1L << 31), "%s: too many output voxels", who);
    const int taps = g.kd * g.kh * g.kw, N = taps * g.Ci, bk = engine == 0 ? 32 : 64;
    p->bm = (Co <= 64) ? 64 : 128;
    // 128-wide n tiles (spanning taps when Ci < 128); slice the voxel axis so the grid fills the chip
    p->grid_x = ((Co + p->bm - 1) / p->bm) * ((N + 127) / 128);
    const long tiles = p->grid_x;
    const int ktiles = (int)((Mv + bk - 1) / bk);
    const long stride = (long)Co * N;
    const size_t one = (size_t)stride * sizeof(float);
    const size_t in_bytes = engine == 0 ? 0 : (size_t)Mv * ((size_t)Co * sizeof(float) + (size_t)taps * g.Ci * (x_bf16 ? 2 : 4));
    int splits = wgrad_splits(tiles, ktiles, one, in_bytes);
    while (splits > 1 && (size_t)splits * one > ws_bytes) splits >>= 1;
    p->splits = splits;
    p->ws_need = (size_t)splits * one;
    if (ws_bytes < p->ws_need) return fail(HUPR_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, p->ws_need);
    p->red = splitk_reduce_plan(stride, stride, splits, stride, taps, g.Ci, ws_aligned, true);
    return HUPR_OK;
}

}  // namespace hupr
