/* hupr_debug.h — test and profiling aids of libhupr_hip.so.  NOT part of the operator contract (include/hupr.h): process-wide
 * switches that select an alternative kernel for a parity comparison in tests/ (same products, another summation order or launch
 * shape) or arm a profiling hook.  Every default is the product path; nothing in the package calls these outside tests/ and scripts/.
 */
#ifndef HUPR_DEBUG_H
#define HUPR_DEBUG_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

void hupr_debug_attn_trace(void* dev_buf); /* profiling aid: device buffer of 3 x 2 x 4096 uint64 s_memtime stamps written by workgroup 0 of the ping-pong attention kernels, or null */
void hupr_debug_halo_variant(int v);  /* A/B aid: 0 auto, 1 force the 128-voxel kernel */
void hupr_debug_halo_res_prefetch(int on);  /* A/B aid: 0 = the 256-voxel 16 x 16 x 32 convolution reads a residual in its immediate epilogue (rounds 4-5a); default 1: prefetched, deferred epilogue */
void hupr_debug_splitk_slices(int s);     /* test aid: slices per workgroup of the split-K reduction: 0 auto, 4, 16; + 256: the scattered-store kernel (hupr_k_splitk_reduce4) for convolution weight gradients too — same sums, the comparison the parity test makes */
void hupr_debug_wgrad_m16(int on);        /* A/B aid: 0 = the LDS-DMA weight gradient on v_mfma_f32_32x32x16_bf16 (rounds 2-4); default 1: v_mfma_f32_16x16x32_bf16 (round 5) */
void hupr_debug_wgrad_ci32(int on);       /* A/B aid: 0 sends Ci <= 32 weight gradients through the two-quadrant kernel (K halves only), 2 forces the K-quarter mode at any size, 3 the same on the 32 x 32 x 16 kernel (the rounds-3-5 path), 1 = default */
void hupr_debug_halo_trace(void* device_u64_4096); /* profiling aid: per-tile s_memtime stamps of workgroup 0 (null = off) */
void hupr_debug_attn_split(int mode);    /* 0 (default): split for Bn == 1 only; 1: every grid below 128 workgroups; -1: never */
void hupr_debug_halo_split_k(int on);     /* A/B aid: 0 = never slice the reduction of small grids */
void hupr_debug_halo_tiles(int mask);     /* test aid: which tiles of the 256-voxel convolution kernel (conv_halo256m_bf16.hip) are in use — bit 0: 4 x 8 x 8, bit 1: 2 x 8 x 16 (D % 4 != 0), bit 2: 1 x 16 x 16 (1 x 3 x 3 taps), bit 3: 8 x 8 x 8 (32 output channels, D = 8), bit 4: 4 x 8 x 8 on 64-byte rows (32 input channels); default 31.  A cleared bit sends those layers to the 128-voxel kernel (the comparison the parity tests make) */
void hupr_debug_halo_two_plane(int on);   /* A/B aid: 0 = depth-2 layers (D == 2, the 2 x 8 x 16 tile spans the depth) run the general four-plane instantiation of that tile, which also multiplies the two zero padding planes; default 1: the two-plane form.  Same route codes (6, 8), same bits for finite weights */

int hupr_debug_halo_route(int Bn, int D, int H, int W, int Ci, int in_ld, int Co, int out_ld, int kd, int abf, int stats, int sliced_ws);
    /* test aid: which kernel instantiation hupr_conv3x3_halo_bf16 (abf = 0) / _bf16act (abf = 1) would launch for this call (stats: the _stats
     * entry; sliced_ws: the _ws entry with a large enough workspace), under the switches above; nothing is launched.  HUPR_ERR_ARG where the
     * call is refused.  1-8: the 256-voxel kernel — 1 the 4 x 8 x 8 tile on 64-byte rows (32 input channels), 2 the 8 x 8 x 8 tile (32 output
     * channels), 3 the 1 x 16 x 16 tile, 4 / 5 the 4 x 8 x 8 tile with fused statistics of one / two output tiles per workgroup, 6 the 2 x 8 x 16
     * tile with fused statistics, 7 the 4 x 8 x 8 tile, 8 the 2 x 8 x 16 tile; else the 128-voxel kernel: 256 + 16 * slices + 8 * (BN == 64)
     * + 4 * (KC == 64) + 2 * (kd == 3) + abf (slices > 1: the K-sliced form) */
int hupr_debug_wgrad_route(int Bn, int D, int H, int W, int Ci, int in_ld, int Co, int dy_ld, int kd, int abf, int dual, size_t ws_bytes,
                           int* groups_out);
    /* test aid: which kernel instantiation hupr_conv3x3_wgrad_halo_bf16 (abf = 0) / _bf16act (abf = 1) / _bf16act_dual (dual = 1) would launch
     * with a workspace of ws_bytes, under hupr_debug_wgrad_m16 / _ci32 as set; *groups_out (may be null): its partial-tensor count.  Nothing is
     * launched.  HUPR_ERR_ARG / HUPR_ERR_WORKSPACE where the call is refused.  route & 15: 1 hupr_k_wgrad_halo_m16<true> (3-D taps), 2
     * m16<false>, 3 m16<true, true> (K quarters); 4-7 hupr_k_wgrad_halo_glds<IS3D, CI32> = 4 + 2 * IS3D + CI32 (the 32 x 32 x 16 kernel);
     * 8-11 the register-staged hupr_k_wgrad_halo_bf16<ABF, IS3D> = 8 + 2 * ABF + IS3D.  + 16: the XCD-aware 1-D grid; + 32: two gradients */
int hupr_debug_interp_route(int op, int bf16, int Bn, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int C, int in_ld, int out_ld,
                            int* grid_out);
    /* test aid: the launch hupr_interp_linear_fwd_* (op 0), _bwd_* (op 1) or _bwd_acc_* (op 2) would make, _f32 (bf16 = 0) or _bf16act
     * (bf16 = 1), from the plan the launchers themselves use (csrc/spatial.hip: interp_plan).  Nothing is launched.  Returns the channel
     * vectors per thread of the kernel (forward: 1; backward: 1 or 4), HUPR_ERR_ARG where the call is refused; *grid_out (may be null): its
     * workgroups. */
int hupr_debug_mnet_grid(int op, long n_bg, int pixels);
    /* test aid: the workgroups of hupr_mnet_fwd_* (op 0), hupr_mnet_fwd_means_* (op 1) or hupr_mnet_bwd_* (op 2) on n_bg x pixels, from the
     * function the launchers themselves use; HUPR_ERR_ARG for another op or an empty extent.  Nothing is launched. */
int hupr_debug_gemm_route(int engine, int op, const int* v, size_t ws_bytes, int ws_misalign, int* out);
    /* test aid: the launch the GEMM engines (engine 0: csrc/gemm_f32.hip, 1: csrc/gemm_bf16.hip) would make, from the plans the launchers
     * themselves use (csrc/gemm_common.h); nothing is launched, the pointers of a call aside every check of the entry point is made.
     * op 0, hupr_gemm_*: v = {ta, tb, M, N, K, batch} (hupr_tmerge_dgrad_bf16: {0, 1, HW, Ci, Co, Bn G}); out = {BM, BN, grid.x, grid.z}.
     * op 1, hupr_conv_fwd_* : v = {Bn, Di, Hi, Wi, Ci, in_ld, Do, Ho, Wo, Co, kd, kh, kw, pd, ph, pw, x_bf16, y_bf16, accumulate, residual
     * given}; out as for op 0.  op 2, hupr_conv_wgrad_*: v = the same first 16 and x_bf16, with a workspace of ws_bytes whose address
     * is ws_misalign modulo 16; out = {BM, grid.x, K slices (partial tensors), reduce kernel, its workgroups, workspace bytes written}
     * — reduce kernel 0 hupr_k_splitk_reduce, 1 hupr_k_splitk_reduce4<4>, 2 hupr_k_splitk_reduce4<16>, 3 hupr_k_splitk_reduce_t<4, 8>,
     * under hupr_debug_splitk_slices as set.  Returns 0, or HUPR_ERR_ARG / HUPR_ERR_WORKSPACE where the call is refused (out[5] is then
     * one partial tensor's bytes, or 0). */
int hupr_debug_mscsa_proj_grid(int op, long M, int C, int* out);
    /* test aid: out = {threads per workgroup, row groups, column blocks} of hupr_mscsa_proj_fwd_bf16 (op 0) or hupr_mscsa_proj_dgrad_f32
     * (op 1) on M rows of C channels, from the plan the launchers themselves use (grid = row groups x column blocks); HUPR_ERR_ARG where
     * the call is refused.  Nothing is launched. */
#ifdef __cplusplus
}
#endif
#endif /* HUPR_DEBUG_H */
