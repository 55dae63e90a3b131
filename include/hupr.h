/*
 * hupr.h — C ABI of the MI355X (gfx950) radar->pose hot path.
 *
 * The reference (robert80203/HuPR-...) is pure Python with no native layer, so there is no
 * FFI in it to mirror symbol-for-symbol.  Each entry point below therefore cites the
 * reference *Python* interface it replaces (file:line relative to the reference root); the
 * Python host in hupr-..._amd/ binds these with ctypes (runtime.py) and re-exposes the
 * reference's own names (RadarObject.generateHeatmap, Normalize, HuPRNet.forward, ...).
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes; no torch types; the caller owns every buffer
 *   - stream-ordered on `stream` (a hipStream_t passed as void*); never synchronises,
 *     never allocates; scratch comes from the caller (`ws`, `ws_bytes`)
 *   - returns 0 on success, a negative HUPR_ERR_* otherwise; hupr_last_error() gives a
 *     thread-local message
 */
#ifndef HUPR_H
#define HUPR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HUPR_OK 0
#define HUPR_ERR_ARG (-1)       /* bad argument (null pointer, unsupported shape)   */
#define HUPR_ERR_WORKSPACE (-2) /* workspace too small                               */
#define HUPR_ERR_LAUNCH (-3)    /* hipLaunch / runtime error                         */
#define HUPR_ERR_COMM (-4)      /* librccl missing / RCCL returned an error          */

typedef void* hupr_stream_t; /* hipStream_t */

int hupr_version(void);
const char* hupr_last_error(void);
/* kernels launched by this library in this process so far (every launch goes through one counting macro, csrc/hupr_common.h):
 * bench.py prints the difference over a step as `launches_per_step` — measurement aid, nothing in the reference to replace */
unsigned long long hupr_launch_count(void);

/* ------------------------------------------------------------------------------------------
 * (a1) FFT chain — replaces RadarObject.generateHeatmap, preprocessing/process_iwr1843.py:106-173
 *      (+ clutterRemoval :85-104, postProcessFFT3D :48-52).
 *
 * adc_iq : int16  [n_sf][4 rx][192 chirp][256 sample][2 (I,Q)]      786 432 B / sensor-frame
 * out    : float2 [n_sf][16 doppler][64 range][64 az][8 el]          complex64, 4 194 304 B
 * Window = rectangular, output = complex (the reference applies no window / magnitude).
 * ws must hold hupr_fft_chain_ws_bytes(n_sf) bytes.
 * ---------------------------------------------------------------------------------------- */
size_t hupr_fft_chain_ws_bytes(int n_sf);
int hupr_fft_chain_c64(const int16_t* adc_iq, int n_sf, void* out_c64, void* ws, size_t ws_bytes,
                       hupr_stream_t stream);

/* (a1+a2) FFT chain fused with the loader glue — replaces generateHeatmap + np.save/np.load +
 *      datasets/dataset.py:144-150 (keep Doppler 4..11, re/im split) + Normalize
 *      (datasets/base.py:13-24; per elevation channel (x-mean)/std, unbiased std).
 * out    : float  [n_sf][8 f][2 re/im][64 range][64 az][8 el]        2 097 152 B / sensor-frame
 *          == one (F,2,R,A,E) group-frame of HuPRNet's input. */
int hupr_fft_chain_loader_f32(const int16_t* adc_iq, int n_sf, float* out, void* ws, size_t ws_bytes,
                              hupr_stream_t stream);

/* (a1+a2+a3 seam) the same, with HuPRNet's elevation mean (models/networks.py:26-27, the first thing forward_chirp does to the
 *      loader tensor) folded in: means[n_sf][16 = 2 f + c][64 range][64 az] = mean over the 8 elevation bins of the normalised
 *      plane — 262 144 B / sensor-frame instead of 2 097 152 B (1 048 576 B algorithmic incl. the ADC read).
 *      Consumed by hupr_mnet_fwd_means_*; bit-identical to hupr_fft_chain_loader_f32 followed by hupr_mnet_fwd_*. */
int hupr_fft_chain_loader_means_f32(const int16_t* adc_iq, int n_sf, float* means, void* ws, size_t ws_bytes,
                                    hupr_stream_t stream);

/* (a1, opt-in variants) north_star asks for "Hanning windowing and magnitude"; the reference has neither
 *      (process_iwr1843.py:130-151 is bare np.fft.fft2 / np.fft.fft, np.abs only in the plotting helper :207-208), so
 *      both are flags that are OFF on every parity path:
 *        HUPR_FFT_HANN_RANGE    x[c,s] *= hann256[s]            before the range FFT   (np.hanning(256), symmetric)
 *        HUPR_FFT_HANN_DOPPLER  (x - mean_c x)[c] *= hann64[c]  before the Doppler FFT (after clutter removal :122-128)
 *        HUPR_FFT_MAGNITUDE     out = |X| as float [n_sf][16][64][64][8] (2 097 152 B) instead of complex64
 *      loader: 0 = complex cube, 1 = the fused loader epilogue of hupr_fft_chain_loader_f32, 2 = the elevation-mean planes of
 *      hupr_fft_chain_loader_means_f32 (window / zero-Doppler / order flags only).
 *      flags == 0 is exactly hupr_fft_chain_c64 / hupr_fft_chain_loader_f32 / hupr_fft_chain_loader_means_f32.
 *
 *      The zero-Doppler bin (Doppler index 8; the loader's slot f = 4).  Clutter removal (process_iwr1843.py:122-128) cancels
 *      it analytically; the reference keeps the fp64 rounding residue of its fft2 there (~2e-16 of the other bins, white, a
 *      pure function of the frame) and its Normalize (datasets/base.py:17-24) inflates that plane to a unit-variance input
 *      channel — an exactly-zero plane would be 0/0 = NaN in that Normalize.  Default: the bin carries a frame-keyed dither
 *      with the reference residue's statistics (integer hash of the exact chirp sums, 2^-53 of an ADC LSB per sample, restated
 *      bit for bit by oracle/fft_chain.py::zero_doppler_dither), transformed and normalised like every other bin.
 *        HUPR_FFT_ZERO_DOPPLER_EXACT  the bin is exactly 0 (round 3's behaviour; the loader epilogues then emit zeros in f = 4)
 *        HUPR_FFT_RANGE_FIRST         the range-first order of rounds 1-2 (the reference's order of operations in fp32: the bin
 *                                     holds that order's own fp32 rounding residue, ~1e-7 relative); slower (2.6 vs 4 TB/s)
 *      Under a window, in the default (Doppler-first) order:
 *        no Doppler window (no window at all, or HUPR_FFT_HANN_RANGE alone)  the bin is still analytically zero (the range window
 *                 commutes with the chirp mean) and follows the convention: by default the SAME unwindowed dither as without a
 *                 window, under HUPR_FFT_ZERO_DOPPLER_EXACT exactly 0, and the loader epilogues then emit zeros in f = 4;
 *        HUPR_FFT_HANN_DOPPLER (alone or with HUPR_FFT_HANN_RANGE)  the window un-nulls the bin: index 8 is ordinary leakage of the
 *                 neighbouring bins, computed like every other bin.  HUPR_FFT_ZERO_DOPPLER_EXACT is accepted and has NO effect on it,
 *                 and no dither is inserted (a process-wide convention must not make a windowed call fail);
 *        HUPR_FFT_RANGE_FIRST  as without a window: whatever that order's arithmetic leaves. */
#define HUPR_FFT_HANN_RANGE 1
#define HUPR_FFT_HANN_DOPPLER 2
#define HUPR_FFT_MAGNITUDE 4
#define HUPR_FFT_ZERO_DOPPLER_EXACT 8
#define HUPR_FFT_RANGE_FIRST 16
int hupr_fft_chain_opts(const int16_t* adc_iq, int n_sf, void* out, int flags, int loader, void* ws, size_t ws_bytes,
                        hupr_stream_t stream);

/* (a1, opt-in) Doppler phase compensation for the TDM-MIMO virtual array.  The reference has none (process_iwr1843.py:113-120
 *      demultiplexes the three transmitters and goes on as if they had fired together); this is the Doppler compensation step of
 *      a TDM-MIMO pipeline (TI mmWave SDK, AoA DPU, "Doppler compensation").  OFF on every parity path.
 *
 *      Virtual antenna v in the chain's workspace order:
 *
 *        v      transmitter             slot k
 *        0..3   TX0                     0
 *        4..7   TX2                     2
 *        8..11  TX1, the elevated row   1
 *
 *      - The kept Doppler index i = 0..15 has the signed bin d = i - 8.
 *      - The range-Doppler value of (v, i, range) is multiplied by exp(-2 pi j d k(v) / 192) before the pruned angle DFT and
 *        before the loader statistics.
 *      - For a sensor-frame marked swapped, k is 2 for v in 0..3 and 0 for v in 4..7.  k stays 1 for the elevated row.
 *      - The 48 factors are the fp32 roundings of the fp64 cosine and sine.  A factor with d == 0 or k == 0 is exactly (1, 0).
 *      - Doppler index 8 and the k = 0 rows must therefore keep today's bits.  This holds under all three zero-Doppler
 *        conventions: the dither, ZERO_DOPPLER_EXACT and RANGE_FIRST.
 *
 *      flags, loader, the buffers, the workspace and the error rules are those of hupr_fft_chain_opts.  Sensor-frame sf is swapped
 *      when tx_swapped_or_null is non-null, sf / frames_per_flag < n_swapped and that byte is non-zero (the ADC mirror of
 *      hupr_adc_mirror_i16 exchanges TX0 and TX2, and with them their slots).  The table is device memory, read by the kernel at
 *      launch time: a step replayed from a hipGraph follows the table's current content.  HUPR_ERR_ARG before any launch for
 *      frames_per_flag < 1, n_swapped < 0, or a non-null table with n_swapped == 0.
 *      A Doppler bin aliased past +-32 is compensated with the wrong sign, as in every such pipeline. */
int hupr_fft_chain_tdm(const int16_t* adc_iq, int n_sf, void* out, int flags, int loader,
                       const unsigned char* tx_swapped_or_null, int n_swapped, int frames_per_flag,
                       void* ws, size_t ws_bytes, hupr_stream_t stream);

/* (a2) loader glue alone on a precomputed cube (the .npy hand-off of the reference):
 * cube_c64 : float2 [n_sf][16][64][64][8]  ->  out float [n_sf][8][2][64][64][8]            */
int hupr_loader_normalize_c64(const void* cube_c64, int n_sf, float* out, hupr_stream_t stream);

/* (f1) DCA1000 raw capture -> ADC layout above — replaces RadarObject.getadcDataFromDCA1000,
 *      preprocessing/process_iwr1843.py:54-83 (2-lane LVDS groups [I0,I1,Q0,Q1]; per chirp [rx0][rx1][rx2][rx3] x 256).
 * raw : int16 stream of n_frames * 786 432 / 2 values;  adc_iq: int16 [n_frames][4][192][256][2]. */
int hupr_dca1000_deinterleave(const int16_t* raw, int16_t* adc_iq, int n_frames, hupr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * HuPRNet operators.  Activations are CHANNELS-LAST fp32: x[b][d][h][w][c] ("voxel stride" =
 * floats between consecutive voxels, >= c, lets an op read/write a channel slice of a wider
 * concat buffer).  Parameters keep the reference's state_dict shapes.
 * ---------------------------------------------------------------------------------------- */

/* Generic batched fp32 MFMA GEMM, row-major.  ta/tb: 0 = as stored, 1 = transposed.
 *   (ta,tb) = (0,1): C[m][n] = sum_k A[m][k] B[n][k]      attention S = Q K^T, dP = dO V^T   (models/layers.py:129)
 *   (0,0):          C[m][n] = sum_k A[m][k] B[k][n]      O = P V (:131), dQ = dS K, PRGCN W.x  (gcn_networks.py:25)
 *   (1,0):          C[m][n] = sum_k A[k][m] B[k][n]      dV = P^T dO, dK = dS^T Q
 * res (optional) is added in the epilogue (cross-attention residual, models/layers.py:146,148).
 * accumulate != 0: C += result. */
int hupr_gemm_f32(int ta, int tb, const float* A, const float* B, float* C, int M, int N, int K, long lda,
                  long ldb, long ldc, int batch, long a_batch_stride, long b_batch_stride, long c_batch_stride,
                  const float* res, long res_ld, long res_batch_stride, int accumulate, hupr_stream_t stream);

/* (a4,a6) stride-1 convolution as implicit GEMM — replaces nn.Conv3d / nn.Conv2d forward and, with
 * weights packed in mode 1, their input-gradient (models/layers.py:10-23,42-62,81-95,115-123,194-210).
 * x : [Bn][Di][Hi][Wi] voxels, in_ld floats apart, first Ci channels used (Ci % 32 == 0)
 * wp: packed weights [Co][kd*kh*kw][Ci]   (hupr_pack_conv_weights_f32)
 * y : [Bn][Do][Ho][Wo] voxels, out_ld floats apart, first Co channels written
 * bias [Co] and res (same voxel indexing, res_ld) optional. */
int hupr_conv_fwd_f32(const float* x, const float* wp, const float* bias, const float* res, float* y, int Bn,
                      int Di, int Hi, int Wi, int Ci, int in_ld, int Do, int Ho, int Wo, int Co, int out_ld,
                      int res_ld, int kd, int kh, int kw, int pd, int ph, int pw, int accumulate,
                      hupr_stream_t stream);

/* weight gradient of the same convolution: dw in the PARAMETER layout (Co, Ci, kd, kh, kw). */
size_t hupr_conv_wgrad_ws_bytes(int Bn, int Do, int Ho, int Wo, int Ci, int Co, int kd, int kh, int kw);
int hupr_conv_wgrad_f32(const float* x, const float* dy, float* dw, int Bn, int Di, int Hi, int Wi, int Ci,
                        int in_ld, int Do, int Ho, int Wo, int Co, int dy_ld, int kd, int kh, int kw, int pd,
                        int ph, int pw, void* ws, size_t ws_bytes, hupr_stream_t stream);

/* w (Co, Ci, taps) parameter layout -> mode 0: [Co][taps][Ci] (forward), mode 1: [Ci][taps reversed][Co] (dgrad) */
int hupr_pack_conv_weights_f32(const float* w, float* wp, int Co, int Ci, int taps, int mode, hupr_stream_t stream);

/* bf16-MFMA variants of the three entry points above: identical signatures and fp32 tensors in HBM;
 * operands are rounded to bf16 while staged into LDS, products accumulate in fp32 (16x the matrix rate).
 * The fp32 entry points remain the parity path (north_star: fp32 within 1e-3; bf16 for configs C2/C4). */
int hupr_gemm_bf16(int ta, int tb, const float* A, const float* B, float* C, int M, int N, int K, long lda,
                   long ldb, long ldc, int batch, long a_batch_stride, long b_batch_stride, long c_batch_stride,
                   const float* res, long res_ld, long res_batch_stride, int accumulate, hupr_stream_t stream);
int hupr_conv_fwd_bf16(const float* x, const float* wp, const float* bias, const float* res, float* y, int Bn,
                       int Di, int Hi, int Wi, int Ci, int in_ld, int Do, int Ho, int Wo, int Co, int out_ld,
                       int res_ld, int kd, int kh, int kw, int pd, int ph, int pw, int accumulate,
                       hupr_stream_t stream);
int hupr_conv_wgrad_bf16(const float* x, const float* dy, float* dw, int Bn, int Di, int Hi, int Wi, int Ci,
                         int in_ld, int Do, int Ho, int Wo, int Co, int dy_ld, int kd, int kh, int kw, int pd,
                         int ph, int pw, void* ws, size_t ws_bytes, hupr_stream_t stream);

/* Streaming form of the temporal merge Conv3d(C, C, (G,1,1)) for 64-channel maps (reference models/layers.py:208,218: the
 * level-1 merge): x bf16 (Bn, G, HW, 64) -> y fp32 (Bn, HW, 64).  The operand travels global -> LDS by LDS-DMA through a ring of
 * four 16 KB stages per persistent workgroup (three in flight while one is multiplied); the generic engine keeps one 8 KB tile
 * in flight and ran this 64 flop/B product at 2.2 TB/s.  wp_bf16: the weight packed [Co][G][Ci] (hupr_pack_conv_weights_bf16). */
int hupr_tmerge_stream_supported(int G, int HW, int Ci, int Co);
int hupr_tmerge_fwd_stream_bf16(const void* x, const void* wp_bf16, float* y, int Bn, int G, int HW, int Ci, int Co,
                                hupr_stream_t stream);
/* Its input gradient dx (bf16, (Bn,G,HW,64)) from dy (fp32, (Bn,HW,64)) — write-bound: the dy tile is converted to bf16 in LDS
 * once and multiplied by the G resident weight slices; wp1_bf16 = the mode-1 bf16 packing ([Ci][taps reversed][Co]) — and its
 * weight gradient dw (fp32, parameter layout (Co,Ci,G), overwritten; deterministic): x and dy both stream through the LDS-DMA
 * ring, the voxel axis is put along the MFMA K of both operands by ds_read_b64_tr_b16, every persistent workgroup leaves one
 * fp32 partial in `ws` (hupr_tmerge_wgrad_stream_ws_bytes) and a second kernel sums them in a fixed order. */
int hupr_tmerge_dgrad_stream_bf16(const float* dy, const void* wp1_bf16, void* dx, int Bn, int G, int HW, int Ci, int Co,
                                  hupr_stream_t stream);
int hupr_tmerge_wgrad_stream_supported(int G, int HW, int Ci, int Co);  /* the weight gradient also takes C = 128 / 256 (Ci == Co, G * C / 64 in {2,4,8}):
                                                                        a frame is C / 64 virtual 64-channel frames, the Co / 64 output blocks go to different workgroups */
size_t hupr_tmerge_wgrad_stream_ws_bytes(int Bn, int G, int HW, int Ci, int Co);
int hupr_tmerge_wgrad_stream_bf16(const void* x, const float* dy, float* dw, int Bn, int G, int HW, int Ci, int Co, void* ws,
                                  size_t ws_bytes, hupr_stream_t stream);
/* Mixed-storage variants for the temporal merges of Encoder3D (reference models/layers.py:195-197: Conv3d with
 * kernel (G,1,1) collapsing the frame axis): the feature maps arrive bf16-stored from the bf16-activation encoder,
 * the merged maps and all gradients of the parameters stay fp32.  x_bf16 / y_bf16 / dx_bf16 select the HBM storage
 * type of that tensor (0: fp32, 1: bf16); everything else as in the entry points above.
 * hupr_tmerge_dgrad_bf16: input gradient of such a merge (one output slice, no padding) as Bn*G batched GEMMs
 * dx[b,d] = dy[b] . W_d  with wp1 the mode-1 packed fp32 weights ([Ci][taps reversed][Co]). */
int hupr_conv_fwd_bf16_mixed(const void* x, int x_bf16, const float* wp, const float* bias, void* y, int y_bf16,
                             int Bn, int Di, int Hi, int Wi, int Ci, int in_ld, int Do, int Ho, int Wo, int Co,
                             int out_ld, int kd, int kh, int kw, int pd, int ph, int pw, hupr_stream_t stream);
int hupr_conv_wgrad_bf16_mixed(const void* x, int x_bf16, const float* dy, float* dw, int Bn, int Di, int Hi,
                               int Wi, int Ci, int in_ld, int Do, int Ho, int Wo, int Co, int dy_ld, int kd,
                               int kh, int kw, int pd, int ph, int pw, void* ws, size_t ws_bytes,
                               hupr_stream_t stream);
int hupr_tmerge_dgrad_bf16(const float* dy, const float* wp1, void* dx, int dx_bf16, int Bn, int G, int HW,
                           int Ci, int Co, hupr_stream_t stream);

/* LDS halo-tiled 3x3x3 / 1x3x3 "same" convolution on the bf16 matrix pipe (forward, and input gradient
 * with mode-1 packed weights): the input halo of a 128-voxel tile is staged once as bf16 and all taps
 * run from LDS.  wp_bf16 from hupr_pack_conv_weights_bf16 ([Co][kd*9][Ci] bf16). */
/* BatchNorm statistics fused into the convolution epilogue (BasicBlock3D: every 3x3x3 convolution is followed by a
 * BatchNorm3d, reference models/layers.py:55-65): bf16 activations, the 256-voxel persistent kernel, no bias / residual.
 * `stats`: hupr_conv3x3_halo_stats_rows() x [2][Co] doubles — per-workgroup column sums and sums of squares of the stored
 * (bf16-rounded) outputs; hupr_bn_train_finalize_f32 (below, with the BatchNorm entry points) turns them into the
 * BatchNorm coefficients, so the separate statistics pass over y is skipped. */
int hupr_conv3x3_halo_stats_supported(int Bn, int D, int H, int W, int Ci, int Co, int kd);
int hupr_conv3x3_halo_stats_rows(void);
int hupr_conv3x3_halo_bf16act_stats(const void* x, const void* wp_bf16, void* y, int Bn, int D, int H, int W, int Ci,
                                    int in_ld, int Co, int out_ld, int kd, void* stats, hupr_stream_t stream);
int hupr_pack_conv_weights_bf16(const float* w, void* wp_bf16, int Co, int Ci, int taps, int mode,
                                hupr_stream_t stream);
/* Repack many weights (both layouts each) in ONE launch.  descs_dev: device array of 48-byte records
 * { const float* w; void* wp0; void* wp1; int64 first; int32 co, ci, taps, kind } with kind 0 = fp32 layouts
 * (hupr_pack_conv_weights_f32 modes 0 and 1), 1 = bf16 layouts.  blocks_dev: one 16-byte record per workgroup
 * { int32 entry, layout; int64 start }: the workgroup writes destination elements [start, start + 2048) of that layout. */
int hupr_pack_conv_weights_table(const void* descs_dev, const void* blocks_dev, int n_blocks, hupr_stream_t stream);
int hupr_conv3x3_halo_supported(int D, int H, int W, int Ci, int kd, int kh, int kw, int pd, int ph, int pw);
int hupr_conv3x3_halo_bf16(const float* x, const void* wp_bf16, const float* bias, const float* res, float* y,
                           int Bn, int D, int H, int W, int Ci, int in_ld, int Co, int out_ld, int res_ld, int kd,
                           hupr_stream_t stream);

/* Weight gradient of the same 3x3(x3) convolutions, halo-tiled (x halo + dy tile staged once per 128-voxel tile,
 * operands transposed by ds_read_b64_tr_b16).  Requires Ci % 64 == 0; dw in parameter layout (Co,Ci,kd,3,3). */
size_t hupr_conv3x3_wgrad_halo_ws_bytes(int Ci, int Co, int kd);
int hupr_conv3x3_wgrad_halo_bf16(const float* x, const float* dy, float* dw, int Bn, int D, int H, int W, int Ci,
                                 int in_ld, int Co, int dy_ld, int kd, void* ws, size_t ws_bytes, hupr_stream_t stream);

/* (a4) BatchNorm3d pieces (models/layers.py:46,49,53); x is [M voxels][C]. */
size_t hupr_bn_ws_bytes(int C);
int hupr_bn_train_stats_f32(const float* x, long M, int C, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                            float* save_invstd, float* scale, float* shift, void* ws, size_t ws_bytes,
                            hupr_stream_t stream);
int hupr_bn_eval_params_f32(const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, int C, float* scale, float* shift,
                            hupr_stream_t stream);
/* y = act(x1*scale1+shift1 [+ x2*scale2+shift2]); act: 0 identity, 1 ReLU  (BasicBlock3D.forward :66-70) */
int hupr_scale_shift_act_f32(const float* x1, const float* scale1, const float* shift1, const float* x2,
                             const float* scale2, const float* shift2, float* y, long M, int C, int act,
                             hupr_stream_t stream);
/* Eval-mode BatchNorm(s) + optional ReLU from the module's own tensors (models/layers.py:57,60,64 in eval mode): the
 * coefficient launch (hupr_bn_eval_params_f32) and the apply launch as one — single-sample inference is launch-bound.
 * x2 (and its BatchNorm) may be null.  The bf16act form takes bf16-stored x1 / x2 / y. */
int hupr_bn_eval_act_f32(const float* x1, const float* gamma1, const float* beta1, const float* mean1, const float* var1,
                         float eps1, const float* x2, const float* gamma2, const float* beta2, const float* mean2,
                         const float* var2, float eps2, float* y, long M, int C, int act, hupr_stream_t stream);
int hupr_bn_eval_act_bf16act(const void* x1, const float* gamma1, const float* beta1, const float* mean1, const float* var1,
                             float eps1, const void* x2, const float* gamma2, const float* beta2, const float* mean2,
                             const float* var2, float eps2, void* y, long M, int C, int act, hupr_stream_t stream);
/* finalize only, from nblk rows of [2][C] double column sums produced elsewhere (hupr_conv3x3_halo_bf16act_stats) */
int hupr_bn_train_finalize_f32(const void* partial, int nblk, long M, int C, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                               float* save_invstd, float* scale, float* shift, hupr_stream_t stream);
/* ... of two BatchNorms over tensors of one shape in one launch (the tail of a BasicBlock3D, reference models/layers.py:66-70) */
int hupr_bn_train_finalize2_f32(const void* partial1, int nblk1, const float* gamma1, const float* beta1, float* running_mean1,
                                float* running_var1, float momentum1, float eps1, float* save_mean1, float* save_invstd1,
                                float* scale1, float* shift1, const void* partial2, int nblk2, const float* gamma2,
                                const float* beta2, float* running_mean2, float* running_var2, float momentum2, float eps2,
                                float* save_mean2, float* save_invstd2, float* scale2, float* shift2, long M, int C,
                                hupr_stream_t stream);
int hupr_bn_bwd_f32(const float* dy, const float* y_mask, const float* x, const float* save_mean,
                    const float* save_invstd, const float* gamma, float* dx, float* dgamma, float* dbeta, long M,
                    int C, int train, void* ws, size_t ws_bytes, hupr_stream_t stream);

/* out[c] = sum_rows x[row][c] — bias gradient of Encoder3D.layer1.0 (models/layers.py:195); ws as hupr_bn_ws_bytes */
/* both branches of y = relu(bn_a(x1) + bn_b(x2)) (BasicBlock3D tail) in one statistics pass + one apply pass */
int hupr_bn_bwd2_f32(const float* dy, const float* y_mask, const float* x1, const float* mean1, const float* invstd1,
                     const float* gamma1, const float* x2, const float* mean2, const float* invstd2, const float* gamma2,
                     float* dx1, float* dx2, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, long M, int C,
                     int train, void* ws, size_t ws_bytes, hupr_stream_t stream);
/* The same two backward passes with the ReLU mask RECOMPUTED from x (x1, x2) and the forward pass's scale / shift
 * (the outputs of hupr_bn_train_stats_* / hupr_bn_eval_params_f32, i.e. exactly the expression
 * hupr_scale_shift_act_* evaluated) instead of read back from the activation: one tensor read less per pass. */
int hupr_bn_bwd_remask_f32(const float* dy, const float* fwd_scale, const float* fwd_shift, const float* x,
                           const float* save_mean, const float* save_invstd, const float* gamma, float* dx, float* dgamma,
                           float* dbeta, long M, int C, int train, void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_bn_bwd2_remask_f32(const float* dy, const float* x1, const float* fwd_scale1, const float* fwd_shift1,
                            const float* mean1, const float* invstd1, const float* gamma1, const float* x2,
                            const float* fwd_scale2, const float* fwd_shift2, const float* mean2, const float* invstd2,
                            const float* gamma2, float* dx1, float* dx2, float* dgamma1, float* dbeta1, float* dgamma2,
                            float* dbeta2, long M, int C, int train, void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_colsum_f32(const float* x, long M, int C, float* out, void* ws, size_t ws_bytes, hupr_stream_t stream);

/* (a6) nn.PReLU() with one shared slope (models/layers.py:26,32) */
int hupr_prelu_fwd_f32(const float* x, const float* alpha, float* y, long n, hupr_stream_t stream);
size_t hupr_prelu_ws_bytes(void);
int hupr_prelu_bwd_f32(const float* dy, const float* x, const float* alpha, float* dx, float* dalpha, long n,
                       void* ws, size_t ws_bytes, hupr_stream_t stream);

/* (a3) MNet front end — replaces HuPRNet.forward_chirp + MNet.forward (models/networks.py:23-33,
 * models/chirp_networks.py:17-21): elevation mean, the (F,2)->(2,F) .view, Conv3d(2->32,(2,1,1),s(2,1,1)),
 * MaxPool3d((4,1,1)).  x: (n_bg=B*G, 8, 2, pixels=R*A, 8) fp32; out: (n_bg, pixels, 32) channels-last.
 * means_or_null: (n_bg, pixels, 16) fp32 — the 16 elevation means per pixel; they are all the backward pass needs of
 * x (1/8 of its bytes), so a training forward saves them and the backward takes them instead of x. */
int hupr_mnet_fwd_f32(const float* x, const float* w, const float* bias, float* out, float* means_or_null, long n_bg,
                      int pixels, hupr_stream_t stream);
size_t hupr_mnet_bwd_ws_bytes(void);
int hupr_mnet_bwd_f32(const float* x_or_null, const float* means_or_null, const float* w, const float* bias,
                      const float* dy, float* dw, float* dbias, long n_bg, int pixels, void* ws, size_t ws_bytes,
                      hupr_stream_t stream);

/* (a3, live stream) the MNet front end over a sliding window — replaces forward_chirp (models/networks.py:23-33) on the G-frame
 *      window the loader gathers around a frame (datasets/dataset.py:120-139) when the frames arrive one at a time.
 * The session state (hupr_stream_state_bytes() bytes on the device; hupr_stream_reset zeroes it) counts the sensor-frames pushed
 * and the poses emitted.  With n = frames pushed so far, a push (flush == 0) files the new frame n and serves the centre frame
 * c = n - lookahead with newest = n; a flush serves c = poses emitted with newest = n - 1.  Window position j reads frame
 * clamp(c - G/2 + j, 0, newest): the new frame from `staging`, any other from ring slot (frame mod G).
 * staging : float [2 sensors][lanes][16][pixels]  the new frame's elevation-mean planes (hupr_fft_chain_loader_means_f32 on the
 *           2 * lanes new sensor-frames, hori first); null for a flush.  Copied into ring slot n mod G by the same launch.
 * ring    : float [2][lanes][G][16][pixels]       the session's mean planes of the last G frames
 * out_*   : [lanes][G][pixels][32] channels-last, fp32 or (bf16act) bf16 — what Encoder3D consumes; bit-identical to
 *           hupr_mnet_fwd_means_* on the gathered planes.  0 <= lookahead <= G/2 - 1, G even; lanes == 0 is a no-op.
 * hupr_stream_advance follows on the same stream: a push counts the frame (and the pose once n >= lookahead), a flush the pose.
 * No argument of either launch depends on the frame number, so one captured graph serves every frame. */
size_t hupr_stream_state_bytes(void);
int hupr_stream_reset(void* state, hupr_stream_t stream);
int hupr_stream_advance(void* state, int lookahead, int flush, hupr_stream_t stream);
int hupr_mnet_stream_f32(const float* staging_or_null, float* ring, const void* state, int lookahead, int flush,
                         const float* w_hori, const float* bias_hori, const float* w_vert, const float* bias_vert,
                         float* out_hori, float* out_vert, int lanes, int G, int pixels, hupr_stream_t stream);
int hupr_mnet_stream_bf16act(const float* staging_or_null, float* ring, const void* state, int lookahead, int flush,
                             const float* w_hori, const float* bias_hori, const float* w_vert, const float* bias_vert,
                             void* out_hori, void* out_vert, int lanes, int G, int pixels, hupr_stream_t stream);
/* arg-max rows (hupr_argmax_rows_f32) -> keypoints[rows][2] = (idx % W, idx / W) * ratio in image pixels, (0, 0) where the
 * maximum is <= 0 — the decode of misc/metrics.py:10-38 scaled as tools/run.py:47-53 hands it to saveKeypoints */
int hupr_stream_keypoints_f32(const int* idx, const float* maxval, float* keypoints, long rows, int W, float ratio,
                              hupr_stream_t stream);
/* Keypoint decode in one launch (csrc/pose_decode.hip): arg-max, sub-pixel refinement and, with a filter state, One-Euro smoothing.
 * Extends the decode of misc/metrics.py:10-38; one 64-lane wave per row, no scratch, no LDS.
 * heat : float [rows][H][W].  idx / maxval [rows]: the bits of hupr_argmax_rows_f32 (first maximum wins).
 * With the peak at (px, py) = (idx % W, idx / W) and h the row as H x W, the offset (ox, oy) in heat-map pixels is
 *   (0, 0) when refine == 0, when maxval <= 0, or when the peak lies on the map border (px in {0, W-1} or py in {0, H-1});
 *   else, with l = logf(fmaxf(h, 1e-10f)) on the 3 x 3 neighbourhood (a NaN neighbour counts as a non-finite log),
 *     dx = 0.5 (l[x+1] - l[x-1]), dxx = l[x+1] - 2 l[x] + l[x-1] (dy, dyy likewise),
 *     dxy = 0.25 (l[x+1,y+1] - l[x-1,y+1] - l[x+1,y-1] + l[x-1,y-1]), det = dxx dyy - dxy^2:
 *     if dxx < 0 and det > 0, the Taylor step (-(dyy dx - dxy dy) / det, -(dxx dy - dxy dx) / det), each component clamped to
 *     [-0.5, 0.5] (Zhang et al., DARK); otherwise the quarter rule 0.25 sign(h[x+1] - h[x-1]) per axis, sign(0) = 0;
 *   (0, 0) when one of the nine logs or an unclamped offset is not finite.
 * raw_keypoints [rows][2] = ((px + ox) * ratio, (py + oy) * ratio), (0, 0) where maxval <= 0.  With refine == 0 these are the floats of
 * hupr_argmax_rows_f32 followed by hupr_stream_keypoints_f32.
 * filter_state_or_null : float [rows][8] = (x^, y^, dx^, dy^, valid, 3 x pad), hupr_pose_filter_state_bytes(rows) bytes; all zero =
 *   never seen.  Null: no filter, keypoints_or_null and velocity_or_null must be null and the five parameters are ignored.
 *   Otherwise rate_hz, min_cutoff, d_cutoff > 0 and beta >= 0 (One-Euro filter, Casiez et al.), a(fc) = 1 / (1 + rate_hz / (2 pi fc)).
 *   A joint is missing when maxval <= min_score or its raw keypoint is not finite: keypoints = (x^, y^) if the state is valid, else
 *   the raw keypoint; velocity = 0; the state is untouched.  The first sample that is not missing sets x^ = x, dx^ = 0, valid = 1.
 *   After that, per axis: dx = (x - x^) rate_hz; dx^ = a(d_cutoff) dx + (1 - a(d_cutoff)) dx^; fc = min_cutoff + beta |dx^|;
 *   x^ = a(fc) x + (1 - a(fc)) x^.  keypoints_or_null [rows][2] = (x^, y^), velocity_or_null [rows][2] = (dx^, dy^) in image pixels
 *   per second.  The parameters are launch arguments, i.e. constants of a captured graph; the state advances with every launch.
 * rows == 0 is a no-op. */
size_t hupr_pose_filter_state_bytes(long rows);
int hupr_pose_decode_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* filter_state_or_null,
                         float rate_hz, float min_cutoff, float beta, float d_cutoff, float min_score, int* idx, float* maxval,
                         float* raw_keypoints, float* keypoints_or_null, float* velocity_or_null, hupr_stream_t stream);
/* Integral keypoint decode in one launch (csrc/pose_integral.hip): arg-max, the mass centroid of a window around it and, with a filter
 * state, One-Euro smoothing.  The decode of Sun et al., "Integral Human Pose Regression" (ECCV 2018) and Nibali et al. (DSNT), which
 * hupr_coord_loss_fwd_f32 trains, restricted to a window so that a floor under the map does not pull it to the map centre.  New, no
 * reference counterpart; one 64-lane wave per row, no scratch, no LDS, no atomics: every output is bit-identical from run to run.
 * heat : float [rows][H][W].  idx / maxval [rows]: the bits of hupr_argmax_rows_f32 (first maximum wins).
 * With the peak at (px, py) = (idx % W, idx / W), h the row as H x W and radius r >= 0:
 *   Window    x in [max(px - r, 0), min(px + r, W - 1)] = [x0, x1], y in [max(py - r, 0), min(py + r, H - 1)] = [y0, y1].  r == 0 means
 *             the whole map, enumerated as the window [0, W-1] x [0, H-1]; any r >= max(H, W) - 1 clips to that window and gives the
 *             bits of r == 0.
 *   Weights   w = fmaxf(h, 0): a negative pixel and a NaN pixel weigh 0 (the weights of hupr_pose_track_f32's covariance window).
 *   Moments   m = sum w, Mx = sum w (x - px), My = sum w (y - py) over the window, in fp32, in this order: with ww = x1 - x0 + 1 the
 *             window cell c = 0 .. ww (y1 - y0 + 1) - 1 is the pixel (x0 + c % ww, y0 + c / ww); lane l of the wave takes the cells
 *             c = l, l + 64, l + 128, ... and adds them in increasing c, starting from 0: m = m + w, Mx = fmaf(w, x - px, Mx),
 *             My = fmaf(w, y - py, My) (x - px and y - py are exact integers); then the three lane sums go through the wave butterfly,
 *             v = v + v[lane ^ 32], then ^ 16, 8, 4, 2, 1.
 *   Offset    (ox, oy) = (Mx / m, My / m) in heat-map pixels.  No clamp: the window bounds each component by r.  (0, 0) where
 *             maxval <= 0 (the window is then not read), where m is not positive and finite, or where Mx / m or My / m is not finite.
 * raw_keypoints [rows][2] = ((px + ox) * ratio, (py + oy) * ratio), (0, 0) where maxval <= 0, as in hupr_pose_decode_f32.
 * filter_state_or_null, rate_hz, min_cutoff, beta, d_cutoff, min_score, keypoints_or_null, velocity_or_null: the One-Euro stage of
 *   hupr_pose_decode_f32 on this raw keypoint: one definition of the filter serves both entries (csrc/pose_filter.h), so the state is
 *   the same [rows][8] of hupr_pose_filter_state_bytes(rows) bytes, missing means the same, and equal raw keypoints give equal
 *   outputs and equal states, bit for bit.  A state may pass from one decode to the other; the filter then goes on from it, on raw
 *   keypoints that differ between the two decodes.
 * Returns -1 (HUPR_ERR_ARG) before any launch for a null required pointer, radius < 0, H or W below 1, rows or H * W beyond 2^31, and
 * the filter-argument errors of hupr_pose_decode_f32.  rows == 0 is a no-op. */
int hupr_pose_decode_integral_f32(const float* heat, long rows, int H, int W, float ratio, int radius, float* filter_state_or_null,
                                  float rate_hz, float min_cutoff, float beta, float d_cutoff, float min_score, int* idx, float* maxval,
                                  float* raw_keypoints, float* keypoints_or_null, float* velocity_or_null, hupr_stream_t stream);
/* Keypoint decode with a constant-velocity Kalman filter per row in one launch (csrc/pose_track.hip): arg-max, sub-pixel refinement,
 * a measurement covariance read off the heat-map, predict / gate / update, and a forecast.  One 64-lane wave per row, no scratch, no
 * LDS.  All positions are image pixels, all times seconds; one call is one frame, dt = 1 / rate_hz.
 * Decode.  heat, idx, maxval and raw_keypoints = z are those of hupr_pose_decode_f32 for the same refine, bit for bit, the (0, 0) of a
 *   non-positive maximum included.
 * Measurement covariance.  On the window of radius 3 around the arg-max pixel (px, py), clipped to the map, with window-relative
 *   coordinates u, v in -3..3 (u = x - px, v = y - py) and weights w = fmaxf(h, 0) (a NaN pixel weighs 0; all 0 where maxval <= 0):
 *     m = sum w;  cu = sum w u / m, cv = sum w v / m;
 *     Sxx = sum w (u - cu)^2 / m,  Sxy = sum w (u - cu)(v - cv) / m,  Syy = sum w (v - cv)^2 / m   (heat-map pixels squared)
 *     R = ratio^2 heatmap_gain [[Sxx, Sxy], [Sxy, Syy]] + meas_std^2 I.
 *   heatmap_gain = 0 gives the constant isotropic R.  S is a spread measure, not an estimate of the peak's width: the window truncates
 *   a wide peak (a Gaussian of sigma 2 measures about 2.67 per axis, not 4), and heatmap_gain scales it.
 * Usable measurement: maxval > min_score, z finite, m > 0 and R finite.
 * state : float [rows][16] = (x, y, vx, vy, P00, P01, P02, P03, P11, P12, P13, P22, P23, P33, live, coast): the state vector in the
 *   order (x, y, vx, vy), the upper triangle of its symmetric 4 x 4 covariance P row by row, live = 1 while a track exists, coast =
 *   the number of consecutive frames it went without an accepted measurement.  hupr_pose_track_state_bytes(rows) bytes, 16-byte
 *   aligned; all zero = never seen.  Required; it advances with every launch.
 * Predict (live track only): x- = F x, P- = F P F^T + Q with the constant-velocity F = [[I, dt I], [0, I]] and, per axis, the white-
 *   acceleration Q = accel_psd [[dt^3 / 3, dt^2 / 2], [dt^2 / 2, dt]] (Bar-Shalom, Li & Kirubarajan 2001, section 6.2.2).
 * Gate and update (live track only), H = [I 0]: nu = z - H x-, S = H P- H^T + R, d2 = nu^T S^-1 nu through the closed-form 2 x 2
 *   inverse.  The measurement is accepted iff it is usable, det S > 0 and finite, and d2 <= gate (a chi-square quantile, 2 d.o.f.).
 *   Accepted: K = P- H^T S^-1, x = x- + K nu, P = (I - K H) P- (I - K H)^T + K R K^T (Joseph form), then P = (P + P^T) / 2;
 *     coast = 0; status HUPR_TRACK_UPDATED.
 *   Not accepted, coast < max_coast: x = x-, P = P-, coast += 1; status HUPR_TRACK_COASTED_MISSING (not usable) or
 *     HUPR_TRACK_COASTED_GATED (usable, refused by the gate).
 *   Not accepted, coast == max_coast (it would coast for the (max_coast + 1)-th consecutive frame): the track ends, and the row
 *     goes on as one without a live track, in the same frame.
 * No live track: a usable measurement starts one, x = (z, 0, 0), P = diag-blocks(R, init_speed_std^2 I), live = 1, coast = 0, status
 *   HUPR_TRACK_STARTED; otherwise the state is all zero and the status HUPR_TRACK_LOST.
 * Outputs per row: keypoints [rows][2] = (x, y); velocity [rows][2] = (vx, vy) per second; covariance [rows][3] = (P00, P01, P11),
 *   the position block; forecast [rows][2] = (x + vx horizon_s, y + vy horizon_s), with horizon_s = 0 the keypoints bit for bit;
 *   status [rows] int.  STARTED: keypoints = z bit for bit, velocity 0, covariance R.  LOST: keypoints = forecast = z, velocity and
 *   covariance 0.
 * Parameters: rate_hz, meas_std, gate, init_speed_std > 0 and finite; accel_psd (pixel^2 / s^3), heatmap_gain, horizon_s >= 0 and
 *   finite; max_coast >= 0; min_score not NaN.  They are launch arguments, i.e. constants of a captured graph.
 * rows == 0 is a no-op. */
#define HUPR_TRACK_UPDATED 0
#define HUPR_TRACK_COASTED_MISSING 1
#define HUPR_TRACK_COASTED_GATED 2
#define HUPR_TRACK_STARTED 3
#define HUPR_TRACK_LOST 4
size_t hupr_pose_track_state_bytes(long rows);
int hupr_pose_track_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* state, float rate_hz,
                        float accel_psd, float meas_std, float heatmap_gain, float gate, int max_coast, float init_speed_std,
                        float min_score, float horizon_s, int* idx, float* maxval, float* raw_keypoints, float* keypoints,
                        float* velocity, float* covariance, float* forecast, int* status, hupr_stream_t stream);
/* hupr_pose_track_f32 with a choice of measurement (csrc/pose_assoc.hip): up to K <= 4 peaks of every heat-map are decoded, and a live
 * track is updated with the one inside its gate that it finds most likely — the nearest-neighbour standard filter (Bar-Shalom, Li &
 * Kirubarajan 2001) — instead of the strongest.  New, no reference counterpart.  One 64-lane wave per row, no scratch, no LDS, no
 * atomics: the same maps and the same state give the same bits.  Everything not said here is hupr_pose_track_f32's: the arguments up
 * to horizon_s, the state and its layout (so a state may pass between the two entries, and hupr_pose_smooth_rts_f32 reads either's),
 * predict, gate, update, coasting, the eight outputs and the status codes.  With K = 1 and present_or_null = NULL the eight outputs
 * and the state are hupr_pose_track_f32's bit for bit.
 * Candidates of a row (one H x W map, pixel index p = y W + x):
 *   Candidate 0 is the arg-max: idx, maxval and raw_keypoints are its index, value and refined keypoint, those of
 *     hupr_pose_track_f32 bit for bit.  A row whose maximum is not > 0 has no candidate (cand_count 0) and no measurement.
 *   A pixel q stands in front of a pixel p when h[q] > h[p], or h[q] == h[p] and q < p.  A NaN pixel stands in front of nothing, and
 *     nothing stands in front of it.  p is a local maximum when h[p] > 0 and none of its up to eight neighbours inside the map stands
 *     in front of it (for maps without NaN: h[p] > h[q], or h[p] == h[q] and p < q, for every neighbour q).  A NaN pixel is never one.
 *   Candidates 1 .. K-1 are taken greedily: the next one is the local maximum in front of all others (value descending, index
 *     ascending) among those with h[p] >= peak_ratio * maxval (the fp32 product) and at Chebyshev distance > min_separation heat-map
 *     pixels from every candidate already taken.  The list ends early when nothing qualifies.
 *   Every candidate gets the sub-pixel refinement of hupr_pose_decode_f32 (for the same refine) and its own measurement covariance
 *     R_k from the radius-3 window around its pixel, exactly as candidate 0 does in hupr_pose_track_f32.  Its score is h[p].
 *   Usable candidate: score > min_score, keypoint finite, window mass > 0, R_k finite — and its group is present (below).
 * Association (live track only), after the prediction: every usable candidate k gets nu_k, S_k = H P- H^T + R_k and d2_k as in
 *   hupr_pose_track_f32.  Those with det S_k > 0 and finite and d2_k <= gate compete on c_k = d2_k + ln det S_k — minus twice the
 *   log-likelihood of nu_k up to a constant, so a broad bump does not win on its inflated R alone.  The smallest c_k is the
 *   measurement of the update; a tie goes to the lower k.  No such candidate: the track coasts or ends as in hupr_pose_track_f32,
 *   with status HUPR_TRACK_COASTED_GATED if any candidate was usable, else HUPR_TRACK_COASTED_MISSING.
 * No live track (also one that ended in this frame): candidate 0 starts one if it is usable, as in hupr_pose_track_f32.
 * Presence coupling.  present_or_null : int [rows / rows_per_group], one flag per group of rows_per_group consecutive rows (the joints
 *   of a lane).  Where the flag is 0 no candidate of the group is usable in this frame: a live track coasts with
 *   HUPR_TRACK_COASTED_MISSING (or ends), a row without one stays HUPR_TRACK_LOST.  NULL: no coupling, rows_per_group is not read.
 * Outputs beside hupr_pose_track_f32's eight: cand_xy [rows][K][2] the candidates' keypoints in image pixels, cand_score [rows][K]
 *   their heat-map values, cand_count [rows] int, chosen [rows] int: the candidate whose measurement went into the state in this frame
 *   (the update's; 0 with HUPR_TRACK_STARTED), -1 when none did.  Slots k >= cand_count hold zeros.
 * Returns -1 (HUPR_ERR_ARG) before any launch for hupr_pose_track_f32's errors, a null output, K outside 1..4, min_separation < 0,
 * peak_ratio outside (0, 1] or NaN, and, with present_or_null, rows_per_group < 1 or rows no multiple of it.  rows == 0 is a no-op. */
int hupr_pose_track_assoc_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* state, float rate_hz,
                              float accel_psd, float meas_std, float heatmap_gain, float gate, int max_coast, float init_speed_std,
                              float min_score, float horizon_s, int K, int min_separation, float peak_ratio,
                              const int* present_or_null, int rows_per_group, int* idx, float* maxval, float* raw_keypoints,
                              float* keypoints, float* velocity, float* covariance, float* forecast, int* status, float* cand_xy,
                              float* cand_score, int* cand_count, int* chosen, hupr_stream_t stream);
/* The candidates of hupr_pose_track_assoc_f32 alone, without a tracker (the same kernel with no state): cand_xy [rows][K][2],
 * cand_score [rows][K], cand_idx [rows][K] int (the pixel index p) and cand_count [rows] int, slots k >= cand_count zero.  The same
 * argument errors; rows == 0 is a no-op. */
int hupr_pose_peaks_f32(const float* heat, long rows, int H, int W, float ratio, int refine, int K, int min_separation,
                        float peak_ratio, float* cand_xy, float* cand_score, int* cand_idx, int* cand_count, hupr_stream_t stream);
/* hupr_pose_track_assoc_f32 with the left / right partners of a skeleton resolved together (csrc/pose_pairs.hip): a network that
 * exchanges a left and a right limb puts each track's peak into its partner's heat-map, and the two tracks then share the peaks of
 * both maps by global nearest neighbour on the two-track problem (Blackman 1986; Bar-Shalom, Li & Kirubarajan 2001).  New, no
 * reference counterpart.  One 64-lane wave per unit (below), which owns the states of its one or two rows; the pool of at most 8
 * measurements is in LDS; no scratch, no atomics: the same maps and the same state give the same bits.  Everything not said here is
 * hupr_pose_track_assoc_f32's: the arguments up to rows_per_group, the state and its layout (so a state may pass between the three
 * entries, and hupr_pose_smooth_rts_f32 reads any of them), the candidates of a map with their refinement and R_k, the usable rule, the
 * presence flags, predict, gate, update, coasting, the end of a track, the eight outputs and the four candidate outputs.  idx, maxval
 * and raw_keypoints are the row's own decode, bit for bit.
 * partner_host : HOST memory, int [rows_per_group]: the partner of joint j inside its group of rows_per_group consecutive rows, or j
 *   itself for a joint without one.  It is copied into the launch arguments, so there is no device table and the entry captures into a
 *   graph.  rows_per_group is always read here (1..32), with or without present_or_null.
 * Unit: one row without a partner, or two partner rows a < b of one group.
 * Pool of a unit: the candidates of a's map in the slots 0 .. K-1, then (two rows) those of b's map in K .. 2K-1.
 * Admissible measurements.  For every live track of the unit, after its prediction, every usable pool entry e gets nu, S, det S and d2
 *   as in hupr_pose_track_f32.  e is admissible for the track when det S > 0 and finite and d2 <= gate; its cost is
 *   c = d2 + ln det S, plus swap_cost when e comes from the other row's map.
 * Assignment.  Every live track gets one of its admissible entries or none, and no entry goes to two tracks.  Among all such
 *   assignments the one that updates the most tracks is taken; among those the one with the smallest fp32 sum c_a + c_b (the one cost
 *   where one track is updated); a tie goes to the lexicographically smaller (entry of a, entry of b) in pool order, "none" last.
 * Update or coast.  An assigned track is updated with its entry.  Every other live track coasts or ends as in hupr_pose_track_f32,
 *   with status HUPR_TRACK_COASTED_GATED if any pool entry was usable, else HUPR_TRACK_COASTED_MISSING.
 * Start.  A row without a live track (also one whose track ended in this frame) starts one from its OWN map's candidate 0 iff that is
 *   usable and was not assigned to a track in this frame; otherwise the row is HUPR_TRACK_LOST.
 * Outputs beside hupr_pose_track_assoc_f32's twelve: source [rows] int, the map the measurement that went into the state came from:
 *   0 the row's own, 1 its partner's, -1 when none did.  chosen is the slot inside that map.
 * With partner_host[j] == j for every j and swap_cost = 0 the twelve outputs and the state are hupr_pose_track_assoc_f32's bit for
 *   bit, and source = (chosen >= 0 ? 0 : -1).
 * swap_cost >= 0 prices a measurement from the partner's map: 0 (no preference) follows a swap at once but lets two partners that
 *   pass close to each other take each other's peak now and then; a larger value keeps close partners apart and follows a swap late.
 * Returns -1 (HUPR_ERR_ARG) before any launch for hupr_pose_track_assoc_f32's errors, a null partner_host or source, rows_per_group
 * outside 1..32, rows no multiple of it, an entry of partner_host outside 0 .. rows_per_group-1 or partner_host[partner_host[j]] != j,
 * swap_cost negative or not finite.  rows == 0 is a no-op. */
int hupr_pose_track_pairs_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* state, float rate_hz,
                              float accel_psd, float meas_std, float heatmap_gain, float gate, int max_coast, float init_speed_std,
                              float min_score, float horizon_s, int K, int min_separation, float peak_ratio,
                              const int* present_or_null, int rows_per_group, const int* partner_host, float swap_cost, int* idx,
                              float* maxval, float* raw_keypoints, float* keypoints, float* velocity, float* covariance,
                              float* forecast, int* status, float* cand_xy, float* cand_score, int* cand_count, int* chosen,
                              int* source, hupr_stream_t stream);
/* hupr_pose_track_f32 with two motion models per row (csrc/pose_imm.hip): the interacting-multiple-model estimator (Blom & Bar-Shalom,
 * IEEE TAC 33(8), 1988; Bar-Shalom, Li & Kirubarajan 2001, section 11.6) for joints that rest, reach and rest again.  Model 0 ("still")
 * filters with accel_psd, model 1 ("moving") with accel_psd_moving; everything else of the nine tracker parameters is shared.  New, no
 * reference counterpart.  One 64-lane wave per row, no scratch, no LDS, no atomics: the same maps and the same state give the same
 * bits.  Everything not said here is hupr_pose_track_f32's: the arguments up to horizon_s, the decode (idx, maxval and raw_keypoints
 * are hupr_pose_decode_f32's bits), the measurement z with its covariance R and the usable rule, F, Q, the gate quantities, the Joseph
 * update, coasting and the status codes.  Predict, gate, update, coast and start are the same device functions, run once per model.
 * state : float [rows][32] = (model 0's x, y, vx, vy, P00, P01, P02, P03, P11, P12, P13, P22, P23, P33; model 1's same 14; mu0, mu1;
 *   live, coast): floats 0..13 in the order of hupr_pose_track_f32's state, mu_j the probability of model j, one live / coast shared by
 *   both models.  hupr_pose_track_imm_state_bytes(rows) bytes, 16-byte aligned; all zero = never seen.  It advances with every launch.
 * A live row, with p = switch_prob and the Markov chain pi = [[1 - p, p], [p, 1 - p]]:
 *   1. Mixing.  c_j = sum_i pi_ij mu_i;  w_{i|j} = pi_ij mu_i / c_j;  x0_j = sum_i w_{i|j} x_i (computed as x_0 + w_{1|j} (x_1 - x_0));
 *      P0_j = sum_i w_{i|j} (P_i + (x_i - x0_j)(x_i - x0_j)^T), all 4 x 4.  With switch_prob == 0 the step is skipped: c = mu, and
 *      every model goes on from its own estimate.
 *   2. Predict.  Each model as in hupr_pose_track_f32 from (x0_j, P0_j), with its own accel_psd in Q.
 *   3. Gate.  Each model j gets nu_j, S_j, det S_j and d2_j against z; its gate is valid when z is usable and det S_j > 0 and finite.
 *      The frame's measurement is accepted iff some model with c_j > 0 has a valid gate and d2_j <= gate.
 *   4. Accepted.  Every model with a valid gate takes the Joseph update (whatever its d2_j and c_j); one whose gate is not valid keeps
 *      its prediction.  l_j = d2_j + ln det S_j (minus twice the log-likelihood of nu_j up to a constant, the cost of
 *      hupr_pose_track_assoc_f32);  m = min l_j over the models with a valid gate and c_j > 0;  w_j = c_j exp(-(l_j - m) / 2) for those
 *      models and 0 for the others;  mu_j = w_j / (w_0 + w_1).  coast = 0; status HUPR_TRACK_UPDATED.
 *   5. Not accepted.  mu = c; both models keep their predictions; the shared counter coasts or the track ends exactly as in
 *      hupr_pose_track_f32: HUPR_TRACK_COASTED_GATED if z is usable, else HUPR_TRACK_COASTED_MISSING, and past max_coast the track ends.
 * No live track (also one that ended in this frame): a usable z starts both models as hupr_pose_track_f32 starts its one, with
 *   mu = (1 - moving_prior, moving_prior), status HUPR_TRACK_STARTED; otherwise the whole state is zero, status HUPR_TRACK_LOST.
 * Outputs: the moment-matched mixture.  x = x_0 + mu_1 (x_1 - x_0) for all four components; keypoints = its position, velocity its
 *   velocity; covariance (P00, P01, P11) of sum_j mu_j (P_j + d_j d_j^T), d_j = x_j - x; forecast = keypoints + horizon_s velocity.
 *   LOST: keypoints = forecast = z, velocity and covariance 0.  moving [rows] = mu_1, 0 without a live track.
 * With switch_prob = 0 and moving_prior = 0 model 1 never has a say: the eight outputs, state floats 0..13 and live / coast are those of
 *   hupr_pose_track_f32 (state floats 0..15) bit for bit, and moving is 0.
 * present_or_null, rows_per_group : the presence flags of hupr_pose_track_assoc_f32: int [rows / rows_per_group]; where the flag is 0
 *   the rows of the group have no usable measurement in this frame.  NULL: no coupling, rows_per_group is not read.
 * Returns -1 (HUPR_ERR_ARG) before any launch for hupr_pose_track_f32's errors, a null moving, accel_psd_moving not finite or below
 * accel_psd, switch_prob outside [0, 0.5], moving_prior outside [0, 1] (NaN included) and, with present_or_null, rows_per_group < 1 or
 * rows no multiple of it.  rows == 0 is a no-op. */
size_t hupr_pose_track_imm_state_bytes(long rows);
int hupr_pose_track_imm_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* state, float rate_hz,
                            float accel_psd, float meas_std, float heatmap_gain, float gate, int max_coast, float init_speed_std,
                            float min_score, float horizon_s, float accel_psd_moving, float switch_prob, float moving_prior,
                            const int* present_or_null, int rows_per_group, int* idx, float* maxval, float* raw_keypoints,
                            float* keypoints, float* velocity, float* covariance, float* forecast, int* status, float* moving,
                            hupr_stream_t stream);
/* Fixed-interval Rauch-Tung-Striebel smoother over a recorded run of hupr_pose_track_f32 in one launch (csrc/pose_smooth.hip; Rauch,
 * Tung & Striebel 1965): the backward pass over the states the filter left behind, so that the answer for frame k uses the frames
 * after it too.  New, no reference counterpart.  One thread per row, sequential in the frame: a latency-bound recurrence of T
 * dependent steps, the rows axis being there so that many sequences (sequences x joints) share one launch.  No LDS, no atomics, no
 * scratch: every output is bit-identical from run to run and independent of the other rows.
 * states    : float [T][rows][16].  Entry k is a copy of the tracker's state tensor right after the hupr_pose_track_f32 launch of
 *             frame k, in that entry's layout (x, y, vx, vy, the upper triangle of P row by row, live, coast).  16-byte aligned.
 * status    : int [T][rows], keypoints : float [T][rows][2]: the tracker's status and filtered keypoints of every frame.
 * rate_hz, accel_psd : those of the filter run; F and Q below are hupr_pose_track_f32's, dt = 1 / rate_hz.
 * Per row, for k = T-1 down to 0, with x_k, P_k the state of entry k and xs, Ps the smoothed state:
 *   status[k] == HUPR_TRACK_LOST: smoothed = keypoints[k] bit for bit, velocity and covariance 0, flag HUPR_SMOOTH_PASSTHROUGH; frame
 *     k-1 has no successor.
 *   Otherwise, and k == T-1 or status[k+1] is HUPR_TRACK_STARTED or HUPR_TRACK_LOST: the end of a track segment.  xs_k = x_k,
 *     Ps_k = P_k bit for bit, flag HUPR_SMOOTH_END.  (A caller separates two recordings by zeroing the tracker state between them: the
 *     next status is then STARTED or LOST, and the chain breaks by itself.)
 *   Otherwise, in this order:
 *     xp = F x_k, Pp = F P_k F^T + Q;
 *     Cholesky Pp = L L^T;
 *     C = P_k F^T Pp^-1, every row by a forward and a backward triangular solve with L;
 *     xs_k = x_k + C (xs_{k+1} - xp);
 *     Ps_k = P_k + C (Ps_{k+1} - Pp) C^T, then (Ps_k + Ps_k^T) / 2;
 *     flag HUPR_SMOOTH_SMOOTHED.
 *     If a pivot of the Cholesky factorisation is not positive and finite, or an entry of xs_k or Ps_k is not finite: xs_k = x_k,
 *     Ps_k = P_k, flag HUPR_SMOOTH_DEGENERATE, and the chain goes on from those values.  (P_k = 0 alone is not degenerate while
 *     accel_psd > 0: Pp = Q is then positive definite, C = 0 and the frame keeps x_k, P_k as SMOOTHED.)
 * Outputs: smoothed [T][rows][2] = (xs[0], xs[1]); velocity [T][rows][2] = (xs[2], xs[3]) per second; covariance [T][rows][3] =
 *   (Ps00, Ps01, Ps11), the position block; flag [T][rows] int.
 * Returns -1 (HUPR_ERR_ARG) before any launch for a null pointer, T < 1, rows < 0, T * rows beyond 2^31, states not 16-byte aligned,
 * rate_hz not positive and finite, accel_psd negative or not finite.  rows == 0 with T >= 1 is a no-op. */
#define HUPR_SMOOTH_SMOOTHED 0
#define HUPR_SMOOTH_END 1
#define HUPR_SMOOTH_PASSTHROUGH 2
#define HUPR_SMOOTH_DEGENERATE 3
int hupr_pose_smooth_rts_f32(const float* states, const int* status, const float* keypoints, long T, long rows, float rate_hz,
                             float accel_psd, float* smoothed, float* velocity, float* covariance, int* flag, hupr_stream_t stream);
/* Fixed-lag Rauch-Tung-Striebel smoother behind the tracker, one launch per tracked frame (csrc/pose_lag.hip; Moore 1973; Simon,
 * Optimal State Estimation, ch. 9): the frame is filed in a ring of the last L + 1 tracker states in device memory, and the backward
 * pass of hupr_pose_smooth_rts_f32 runs over the ring only.  The oldest frame of the ring is the fixed-lag answer: the pose of L = lag
 * frames ago, smoothed with the L frames seen since.  New, no reference counterpart.  One thread per row, 64 per workgroup, a
 * latency-bound recurrence of at most L dependent steps.  No LDS, no atomics, no scratch: every output is bit-identical from run to
 * run and independent of the other rows.  No argument depends on the frame number — the counter is in the lag state —, so the launch
 * captures into a graph and replays.
 * track_state : float [rows][16], the tracker's state tensor right after the launch of this frame, whichever of hupr_pose_track_f32,
 *             hupr_pose_track_assoc_f32 and hupr_pose_track_pairs_f32 wrote it (one layout).  16-byte aligned.  Read only.
 * status : int [rows], keypoints : float [rows][2], raw_keypoints : float [rows][2], maxval : float [rows]: that launch's status,
 *             filtered keypoints, raw keypoints and maxima.  Read only: the smoother reports, it feeds nothing back.
 * lag_state : hupr_pose_lag_state_bytes(rows, lag) bytes, opaque, 16-byte aligned, advanced in place: the ring — [L + 1][rows][16]
 *             states and, in the same [slot][rows] order, the four other inputs — and a frame counter per row.  All zero means a new
 *             sequence; a state belongs to one (rows, lag).  hupr_pose_lag_state_bytes returns 0 for rows < 0 or beyond 2^31 / 65 and
 *             for lag outside 1..64.
 * rate_hz, accel_psd : those of the filter run, as in hupr_pose_smooth_rts_f32.
 * Per row, with n the number of frames of this row filed since its lag state was zeroed (the row's own counter; a counter the entry
 * did not write counts as 0):
 *   File.  The five inputs of the row are copied into slot n mod (L + 1) of the ring, and the counter becomes n + 1.  (It is kept
 *     below 2 (L + 1) by subtracting L + 1: n mod (L + 1) and min(n, L) are all that is read of it.)
 *   Window.  The frames n, n-1, ..., max(n - L, 0) — the ring's slots (n - j) mod (L + 1) — are a recording of T = min(n, L) + 1
 *     frames, and the backward pass over it is hupr_pose_smooth_rts_f32's word for word, frame n being its frame T-1:
 *     HUPR_SMOOTH_PASSTHROUGH where the status is HUPR_TRACK_LOST; HUPR_SMOOTH_END at frame n and in front of a successor that is
 *     HUPR_TRACK_STARTED or HUPR_TRACK_LOST, with xs = x, Ps = P bit for bit; otherwise predict, Cholesky, the two triangular solves,
 *     xs and Ps, HUPR_SMOOTH_SMOOTHED, or HUPR_SMOOTH_DEGENERATE with the filter's own state, from which the chain goes on.  The two
 *     kernels compile the same expressions (csrc/pose_rts.h): the tail below is hupr_pose_smooth_rts_f32 over the same T frames bit
 *     for bit.  Gains are recomputed in every launch, none is kept in the ring.
 * Outputs, the tail: slot j = 0..L is frame n - j.  tail_keypoints [L+1][rows][2] = (xs[0], xs[1]), tail_velocity [L+1][rows][2] =
 *   (xs[2], xs[3]) per second, tail_covariance [L+1][rows][3] = (Ps00, Ps01, Ps11), tail_flag [L+1][rows] int; and the filter's record
 *   of the same frames as it was filed: tail_filtered [L+1][rows][2], tail_raw [L+1][rows][2], tail_status [L+1][rows] int,
 *   tail_scores [L+1][rows].  Slot 0 is the newest frame, always HUPR_SMOOTH_END or HUPR_SMOOTH_PASSTHROUGH: the filter itself.  Slot
 *   L is the fixed-lag answer, the pose of frame n - L.  A slot j > n — the frame does not exist yet — holds zeros in all eight and
 *   the flag HUPR_SMOOTH_EMPTY.  After the last frame of a sequence the slots L-1 .. 0 are the answers still owed, each smoothed with
 *   all the frames there are.
 * Returns -1 (HUPR_ERR_ARG) before any launch for a null pointer, lag outside 1..64, rows < 0 or beyond 2^31 / 65, track_state or
 * lag_state not 16-byte aligned, rate_hz not positive and finite, accel_psd negative or not finite.  rows == 0 is a no-op. */
#define HUPR_SMOOTH_EMPTY 4
size_t hupr_pose_lag_state_bytes(long rows, int lag);
int hupr_pose_smooth_lag_f32(const float* track_state, const int* status, const float* keypoints, const float* raw_keypoints,
                             const float* maxval, long rows, int lag, float rate_hz, float accel_psd, float* lag_state,
                             float* tail_keypoints, float* tail_velocity, float* tail_covariance, int* tail_flag, float* tail_filtered,
                             float* tail_raw, int* tail_status, float* tail_scores, hupr_stream_t stream);
/* The measurement half of hupr_pose_track_f32 without a filter, in one launch (csrc/pose_fit.hip): what a recording has to keep of a
 * frame so that the tracker can be run over it again, under any parameters.  New, no reference counterpart.  One 64-lane wave per
 * row, no scratch, no LDS.
 * heat, idx, maxval and raw_keypoints are those of hupr_pose_decode_f32 for the same refine, bit for bit.
 * meas : float [rows][8] = (zx, zy, score, m, Sxx, Sxy, Syy, 0), 16-byte aligned: z = raw_keypoints and score = maxval of the row, and
 *   the mass m and the second central moments of the radius-3 window around the arg-max pixel exactly as hupr_pose_track_f32 computes
 *   them (m = 0 and NaN moments where maxval <= 0).  With these eight floats and (ratio, meas_std, heatmap_gain, min_score) the
 *   measurement of hupr_pose_track_f32 — z, R = ratio^2 heatmap_gain S + meas_std^2 I, usable or not — is determined, bit for bit.
 * Returns -1 (HUPR_ERR_ARG) before any launch for a null pointer, H or W below 1, rows or H * W beyond 2^31, meas not 16-byte aligned.
 * rows == 0 is a no-op. */
int hupr_pose_measure_f32(const float* heat, long rows, int H, int W, float ratio, int refine, int* idx, float* maxval,
                          float* raw_keypoints, float* meas, hupr_stream_t stream);
/* The likelihood of a whole recording of hupr_pose_measure_f32 under G candidate parameter triples, in one launch (csrc/pose_fit.hip):
 * the search of a maximum-likelihood fit of the tracker's noise parameters (Bar-Shalom, Li & Kirubarajan 2001, ch. 5 and 11.6; Abbeel
 * et al., RSS 2005).  New, no reference counterpart.  One thread per (candidate, row), a wave being 64 candidates of one row: the
 * record is read with wave-uniform loads, and each thread runs a recurrence of T dependent frames on registers.  No LDS, no atomics, no
 * scratch: each thread adds its costs in frame order, and every output is bit-identical from run to run.
 * meas  : float [T][rows][8], frame by frame what hupr_pose_measure_f32 wrote; 16-byte aligned.  Read only.
 * start : int [T]; a non-zero entry marks the first frame of a sequence: every row's track is zeroed in front of it (what a caller of
 *   hupr_pose_track_f32 does by zeroing the state between two recordings).  The tracks are all zero in front of frame 0 in any case.
 * ratio, rate_hz, gate, max_coast, init_speed_std, min_score : hupr_pose_track_f32's, shared by all candidates; horizon_s plays no part.
 * params : DEVICE memory, float [G][3] = (accel_psd, meas_std, heatmap_gain) of candidate g.  hupr_pose_track_f32's rule for the three
 *   (accel_psd and heatmap_gain >= 0, meas_std > 0, all finite) is the caller's to check before the upload: the entry cannot read them.
 * Per (candidate g, row r), for t = 0 .. T-1, the frame of hupr_pose_track_f32 with the same device functions in the same order:
 *   1. start[t] != 0: the track becomes all zero.
 *   2. The measurement z, R and usable from meas[t][r] under the candidate's meas_std and heatmap_gain.
 *   3. Live track: predict; nu, S, det S and d2; ``valid`` iff usable, det S > 0 and finite.  Accepted iff valid and d2 <= gate: the
 *      Joseph update; otherwise the track coasts or ends as in hupr_pose_track_f32.
 *   4. No live track (also one that ended in this frame): a usable measurement starts one, otherwise the state is all zero.
 *   Cost: on every frame where the track was live in front of step 3 and the gate was valid, accepted or not,
 *     c = fminf(d2 + logf(det S), outlier_cost)  (fp32)
 *   is added to a double.  d2 + ln det S is minus twice the Gaussian log-likelihood of the innovation up to 2 ln 2 pi; outlier_cost is
 *   what a measurement costs as an outlier uniform over the image, 2 ln(image area / 2 pi) in the same units, so that a candidate
 *   whose tiny R and Q gate everything out pays outlier_cost per frame instead of nothing.  A frame that starts a track or has no
 *   usable measurement adds nothing.
 * Outputs: nll [G][rows] double, the sums; counts [G][rows][6] int = the number of frames with status HUPR_TRACK_UPDATED,
 *   COASTED_MISSING, COASTED_GATED, STARTED, LOST (code order), then the number of frames scored; final_state_or_null
 *   [G][rows][16], the state after the last frame in hupr_pose_track_f32's layout, 16-byte aligned: for a candidate that equals the
 *   parameters of a hupr_pose_track_f32 run over the same frames, that run's state bit for bit.
 * G == 0 or rows == 0 is a no-op; T == 0 with G > 0 zeroes the outputs and launches nothing.
 * Returns -1 (HUPR_ERR_ARG) before any launch for a null required pointer, T, rows or G negative, T or rows beyond 2^31, G beyond 2^22,
 * meas or final_state not 16-byte aligned, hupr_pose_track_f32's errors for the shared parameters, ratio not positive and finite,
 * outlier_cost NaN. */
int hupr_pose_track_nll_f32(const float* meas, const int* start, long T, long rows, float ratio, float rate_hz, float gate, int max_coast,
                            float init_speed_std, float min_score, float outlier_cost, const float* params, long G, double* nll,
                            int* counts, float* final_state_or_null, hupr_stream_t stream);
/* Scene occupancy (csrc/cfar.hip): cell-averaging constant-false-alarm-rate detection on the (range, azimuth) maps of a sensor-frame's
 * elevation-mean planes, a per-frame summary of the detections, and a presence gate over the summaries (Rohling 1983; Richards,
 * Fundamentals of Radar Signal Processing, ch. 6).  New, no reference counterpart.  One workgroup per frame, 48 KB of LDS, no atomics,
 * fixed reduction order: every output is bit-identical from run to run.
 * planes : float [n][16][64][64], what hupr_fft_chain_loader_means_f32 writes: plane 2 f + c is Doppler slot f = 0..7, c = re / im, the
 *          spatial axes are (range r, azimuth a).  Clutter removal has nulled everything static: the planes hold movers plus noise, and
 *          under noise a cell is complex Gaussian, its power exponentially distributed.
 * Slot 4.  The clutter-nulled zero-Doppler slot f = 4 (planes 8 and 9) is never read: its mask is 0, its SNR 0, whatever it holds.
 * Power.   For the other seven slots p_f[r][a] = x[2f][r][a]^2 + x[2f+1][r][a]^2.
 * Training cells.  guard = g >= 0, train = t >= 1, w = g + t <= 8.  Inside one slot T(r, a) = {(r', a') inside the map :
 *          g < max(|r' - r|, |a' - a|) <= w}; neither axis wraps, cells outside the map are not counted, so N = |T| is smaller near the
 *          border (N >= 3).  noise = (sum of p over T) / N.  The sum is built from training cells only, never as a difference of sums
 *          that hold the cell under test: per row the cells of the columns a - w .. a + w beyond the guard columns, in increasing a',
 *          and those of the guard columns; then over the rows r - w .. r + w in increasing r', a row beyond the guard rows adding both
 *          of its sums, a guard row the first.  With p's two roundings and the division this bounds the relative error of noise by
 *          (4 w + 3) 2^-24 and that of snr by (4 w + 6) 2^-24.
 * Threshold.  alpha[N] = N (pfa^(-1/N) - 1), the exact factor for exponential cells at false-alarm probability pfa.
 *          alpha_table : float [table_len] on the device, entry N = alpha[N] computed in fp64 and rounded to fp32, entry 0 unused
 *          (+inf); table_len >= (2 w + 1)^2 - (2 g + 1)^2 + 1.  hupr_cfar_table_len / hupr_cfar_alpha_table_f32 size and fill a HOST
 *          table.  The kernel reads entry N of the cell's own window, so the design rate also holds at the border.
 *          A cell detects iff p > alpha[N] * noise (both sides fp32; a NaN on either side does not detect).
 *          snr = p / noise, 0 where p and noise are both 0.
 * mask_or_null : unsigned char [n][8][64][64], 1 = detection.  snr_or_null : float, the same shape.  Either may be null.
 * summary : float [n][8] = (count, peak_snr, peak_f, peak_r, peak_a, centroid_r, centroid_a, doppler): the number of detections over
 *          the seven slots; the SNR and the slot, range and azimuth of the detection with the largest SNR, ties to the lowest (f, r, a)
 *          in that order; the SNR-weighted mean range and azimuth of all detections; the SNR-weighted mean of the signed Doppler bin
 *          d = f - 4 (its sign tells approaching from receding).  Without a detection (0, 0, -1, -1, -1, 0, 0, 0).  The weighted sums
 *          are accumulated in fp64.
 * hupr_cfar_ra_stream_f32 runs the same kernel on the centre frame of a live-stream session (hupr_mnet_stream_f32 above), read from
 * the session's ring: frame `lane` is the horizontal sensor's ring slot (centre mod G) of that lane, centre = flush ? poses emitted :
 * frames pushed - lookahead, read from the session state on the device.  It goes behind the hupr_mnet_stream_* launch of the same push
 * or flush, which has filed the newest frame, and in front of hupr_stream_advance; no argument depends on the frame number.
 * hupr_presence_update, one call per emitted frame: gate_state int [lanes][4] = (present, hits, misses, frames), all zero = a new
 * sequence.  hit = count >= min_cells (count = summary[lane][0]); hits = hit ? hits + 1 : 0; misses = hit ? 0 : misses + 1; an absent
 * lane becomes present when hits >= confirm, a present lane absent when misses > hold; frames += 1 (the three counters saturate at
 * 2^31 - 1).  present_out int [lanes].  hold bridges the pauses of a person who stands still and so vanishes under clutter removal.
 * All entries return -1 (HUPR_ERR_ARG) before any launch for guard < 0, train < 1, guard + train > 8, a table shorter than the window
 * needs, pfa outside (0, 1), min_cells < 1, confirm < 1, hold < 0, a negative count and null pointers; n == 0 / lanes == 0 is a no-op. */
int hupr_cfar_table_len(int guard, int train);
int hupr_cfar_alpha_table_f32(double pfa, int guard, int train, float* host_table, int table_len);
int hupr_cfar_ra_f32(const float* planes, int n, int guard, int train, const float* alpha_table, int table_len,
                     unsigned char* mask_or_null, float* snr_or_null, float* summary, hupr_stream_t stream);
int hupr_cfar_ra_stream_f32(const float* ring, const void* stream_state, int lookahead, int flush, int lanes, int G, int guard,
                            int train, const float* alpha_table, int table_len, unsigned char* mask_or_null, float* snr_or_null,
                            float* summary, hupr_stream_t stream);
int hupr_presence_update(const float* summary, int lanes, int min_cells, int confirm, int hold, int* gate_state, int* present_out,
                         hupr_stream_t stream);
/* Radar point cloud, one sensor (csrc/radar_points.hip): the detections of hupr_cfar_ra_f32 thinned to local power maxima and refined to
 * sub-cell (range, azimuth) points (Rohling 1983; Jacobsen & Kootsookos 2007 for the range estimator; Richards ch. 6).  New, no
 * reference counterpart.  One workgroup per frame, 49 KB of LDS, no atomics, a block prefix scan and fixed orders: every output is
 * bit-identical from run to run.
 * planes : float [n][16][64][64] and mask : unsigned char [n][8][64][64], what hupr_cfar_ra_f32 reads and writes.
 * Power.   p_f[r][a] = fmaf(x[2f], x[2f], x[2f+1] * x[2f+1]) in fp32, the rounding of the CFAR kernel.  Slot 4 is never read.
 * Peak.    Cell c = (f, r, a) is a point iff mask[c] == 1 and p[c] dominates its box.  The box: the slots f' with |f' - f| <= 1, slot 4
 *          and slots outside 0..7 left out; in each, the cells with |r' - r| <= sep_range and |a' - a| <= sep_azimuth inside the map
 *          (no axis wraps).  Every cell of the box counts, detected or not.  p[c] dominates when p[c] > p[c'] for every c' of the box
 *          below c in (f, r, a) order and p[c] >= p[c'] for every c' above it: a plateau yields its lowest cell, once.  A NaN fails
 *          every comparison: a NaN power is no point, and no cell with a NaN in its box is one.
 *          0 <= sep_range <= 4, 0 <= sep_azimuth <= 8; the Python layer's defaults are 1 and 4 (half the 8-antenna main lobe).
 * Refinement, in fp32, every operation rounded on its own (sqrt and the divisions correctly rounded; log is evaluated in fp64 and
 *          rounded to fp32, so it is the correctly rounded fp32 logarithm but for a double rounding):
 *          range.   A0 = sqrt(p[c]), A- = sqrt(p at (f, r - 1, a)), A+ = sqrt(p at (f, r + 1, a)); a neighbour outside the map or
 *                   NaN counts as 0.  range = A+ >= A- ? r + A+ / (A0 + A+) : r - A- / (A0 + A-)  — the two-point amplitude
 *                   estimator of an unwindowed, unpadded DFT.  Against exact arithmetic on the same fp32 powers the error is at most
 *                   2^-24 (4 |range - r| + |range|): one rounding in each root, one in the sum, one in the quotient, one in the
 *                   last sum.
 *          azimuth. l = log(p) at (f, r, a - 1), c and (f, r, a + 1); den = (l- - 2 l0) + l+;
 *                   azimuth = a + clip(0.5 * ((l- - l+) / den), -0.5, 0.5), the three-point parabola of a zero-padded transform's
 *                   lobe; the offset is 0 for a = 0 or 63, where a neighbour's power is not > 0, or where den is not < 0.  The
 *                   quotient cancels where the lobe is flat (|den| small): no bound is stated.
 *          Doppler is not refined: d = f - 4.
 * points : float [n][max_points][6] = (range index, azimuth index, signed Doppler bin d, power p[c], snr, cell), cell = (f * 64 + r) *
 *          64 + a as a float; snr = snr_or_null[c] (float [n][8][64][64], what hupr_cfar_ra_f32 writes) or 0 without it.  Sorted by
 *          descending power, ties to the lower cell.  The rows beyond the points written hold (0, 0, 0, 0, 0, -1).
 * counts : int [n][2] = (points written, peaks found).  The first 4096 peaks of a frame in (f, r, a) order are staged and ranked; a
 *          frame with more ranks those and still reports the true number found, so the caller sees found > 4096.
 * max_points in 1..256.  Returns -1 (HUPR_ERR_ARG) before any launch for a bad count or separation, n < 0 or beyond 2^20 and null
 * pointers (snr_or_null may be null); n == 0 is a no-op.
 *
 * Two sensors to metres: hupr_radar_points_fuse_f32 pairs the horizontal sensor's points of a frame with the vertical sensor's and
 * solves for the position.  One wave per frame, no atomics, fixed orders.
 * points_h [n][max_h][6], counts_h [n][2], points_v [n][max_v][6], counts_v [n][2] : the outputs of hupr_radar_peaks_f32 for the same
 *          frames of the two sensors (of counts only "points written" is read, clamped to the list).
 * geometry_host : HOST double [14] = (range_bin_m, doppler_mps_per_bin, a_h[3], o_h[3], a_v[3], o_v[3]): metres per range bin, metres
 *          per second per Doppler bin, and per sensor the unit vector a_s along its array and its origin o_s (metres; x right, y
 *          boresight, z up).  |a_s| = 1 and a_h . a_v = 0 to 1e-9, all values finite, both scalars positive, and b = a_v x a_h must
 *          have a y component (b is signed so that b . y > 0).
 * Association.  The horizontal points are walked in their order (strongest first).  Each takes, among the vertical points not yet
 *          taken whose Doppler bin differs by at most doppler_gate (0..7) and whose range index differs by at most range_gate
 *          (|r_h - r_v| <= range_gate, the difference exact in fp64), the one with the smallest |r_h - r_v|, ties to the lower row.  A
 *          horizontal point without a partner is not emitted.
 * Geometry, fp64, stored as fp32.  R_s = (94 - range index) * range_bin_m, u_s = (31 - azimuth index) / 32 (the index conventions of
 *          the FFT chain).  c_h = o_h . a_h + R_h u_h, c_v = o_v . a_v + R_v u_v,
 *          c_b = o_h . b + sqrt(R_h^2 - (c_h - o_h . a_h)^2 - (c_v - o_h . a_v)^2); position = c_h a_h + c_v a_v + c_b b.  A radicand
 *          that is negative (or NaN) drops the pair; its vertical point stays taken.
 * cloud : float [n][max_h][8] = (x, y, z, radial velocity = d_h * doppler_mps_per_bin in m/s, receding positive, snr_h, snr_v, row_h,
 *          row_v): eight fields, 32-byte rows, in the order of the horizontal points.  The rows beyond the pairs written hold
 *          (0, 0, 0, 0, 0, 0, -1, -1).  cloud_counts : int [n].
 * max_h, max_v in 1..256.  Returns -1 before any launch for a refused geometry, gate or count and null pointers; n == 0 is a no-op. */
int hupr_radar_peaks_f32(const float* planes, const unsigned char* mask, const float* snr_or_null, int n, int max_points, int sep_range,
                         int sep_azimuth, float* points, int* counts, hupr_stream_t stream);
int hupr_radar_points_fuse_f32(const float* points_h, const int* counts_h, int max_h, const float* points_v, const int* counts_v, int max_v,
                               int n, const double* geometry_host, double range_gate, int doppler_gate, float* cloud, int* cloud_counts,
                               hupr_stream_t stream);

/* tri-/bilinear align_corners=True resampling (models/layers.py:84,89,199,204; gcn_networks.py:49,63) */
int hupr_interp_linear_fwd_f32(const float* x, float* y, int Bn, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                               int C, int in_ld, int out_ld, hupr_stream_t stream);
int hupr_interp_linear_bwd_f32(const float* dy, float* dx, int Bn, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                               int C, int in_ld, int out_ld, hupr_stream_t stream);

/* (a5) softmax over the key axis, in place on rows of length n (models/layers.py:131), and its backward */
int hupr_softmax_rows_f32(float* s, long rows, int n, hupr_stream_t stream);
int hupr_softmax_rows_bwd_f32(const float* p, float* dp_inout, long rows, int n, hupr_stream_t stream);

/* (a5) fused flash-style attention on the bf16 matrix pipe (C in {64,128}, N % 128 == 0): no N x N matrix in HBM.
 * K, Q, V, out, dout, dK, dQ, dV: (B,N,C) fp32 token-major; lse, Dq_scratch: (B,N) fp32. */
int hupr_attn_flash_supported(int N, int C);
int hupr_attn_fwd_bf16(const float* K, const float* Q, const float* V, float* out, float* lse, int Bn, int N, int C,
                       int residual, hupr_stream_t stream);
int hupr_attn_bwd_bf16(const float* K, const float* Q, const float* V, const float* out, const float* dout,
                       const float* lse, float* dK, float* dQ, float* dV, float* Dq_scratch, int Bn, int N, int C,
                       int residual, hupr_stream_t stream);

/* Same kernels fed with pre-rounded bf16 copies of the MFMA operands (hupr_cast_f32_to_bf16): every workgroup re-reads
 * all of K/V (or Q/dO), so the copies halve that traffic and drop the per-tile fp32->bf16 conversions; results are
 * bit-identical to the fp32-input entry points.  Vres / V32 / dout32: the fp32 tensors of the exact residual terms. */
int hupr_attn_fwd_bf16in(const void* K, const void* Q, const void* V, const float* Vres, float* out, float* lse, int Bn,
                         int N, int C, hupr_stream_t stream);
int hupr_attn_bwd_bf16in(const void* K, const void* Q, const void* V, const void* dO, const float* V32, const float* out,
                         const float* dout32, const float* lse, float* dK, float* dQ, float* dV, float* Dq_scratch,
                         int Bn, int N, int C, int residual, hupr_stream_t stream);
/* Strided forms for one MSCSA level (models/layers.py:150-163: eight 1x1 projections of the two maps feed four attentions):
 * the four projections of a map are one GEMM into a (B, N, 4C) bf16 tensor, K / Q point at column blocks of it with
 * row strides ldk / ldq (elements), and the backward writes dK / dQ into column blocks (lddk / lddq) of the matching
 * fp32 gradient tensors.  accumulate != 0 (non-residual form) adds onto the dV another attention left in place.
 * out16: optional bf16 copy of the output with row stride ld16 (a column block of the decoder's concatenated input);
 * dO: bf16, row stride lddo; dout32 null: the gradient arrived bf16-stored and dO is used for the exact terms too. */
int hupr_attn_fwd_bf16in_ld(const void* K, int ldk, const void* Q, int ldq, const void* V, const float* Vres, float* out,
                            float* lse, void* out16_or_null, int ld16, int Bn, int N, int C, hupr_stream_t stream);
/* Small batches (BASELINE config C2, B = 1 inference: N / 128 x Bn workgroups leave most of the 256 CUs idle): the same forward
 * with the keys split over a third grid dimension and a merge launch (flash-decoding).  hupr_attn_fwd_split_ws_bytes returns
 * the workspace that needs, or 0 when the one-pass kernel is used (ws may then be null): by default the split is taken for
 * single-sample calls only, so that batched runs keep the rounding their parity gates were measured with. */
size_t hupr_attn_fwd_split_ws_bytes(int Bn, int N, int C);
/* Which kernels an attention call of this shape launches (nothing is launched): bf16_operands = 0 for hupr_attn_fwd_bf16 /
 * hupr_attn_bwd_bf16 (fp32 operands), else 1; split_ws != 0 for a forward given a workspace (the _ws entries with ws != NULL).  The
 * single, batch, plain and _qs entries of one shape take the same route.  HUPR_ERR_ARG where (Bn, N, C, ldk) is refused.  Otherwise
 *   route & 3  : the forward kernel — HUPR_ATTN_FWD_PP64 (the 512-thread ping-pong kernel), _ONE_PASS (hupr_k_attn_fwd<C>), _SPLIT
 *                (hupr_k_attn_fwd<C> over key shares + hupr_k_attn_combine<C>)
 *   route & 12 : the dK / dV kernel — HUPR_ATTN_DKV512 (512 threads, C = 64), _DKV_NH1 (hupr_k_attn_bwd_dkv<C, 1>), _DKV_NH2 (<256, 2>)
 *   route & 16 : HUPR_ATTN_XMAP, the backward's batch-to-XCD remap (Bn % 8 == 0)
 *   route >> 8 : the forward's key shares S (1 unless split)
 * A backward batch call launches 2 + (dK / dV rounds) kernels, 2 + n_items with HUPR_ATTN_DKV512. */
#define HUPR_ATTN_FWD_PP64 1
#define HUPR_ATTN_FWD_ONE_PASS 2
#define HUPR_ATTN_FWD_SPLIT 3
#define HUPR_ATTN_DKV512 4
#define HUPR_ATTN_DKV_NH1 8
#define HUPR_ATTN_DKV_NH2 12
#define HUPR_ATTN_XMAP 16
int hupr_attn_route(int Bn, int N, int C, int ldk, int bf16_operands, int split_ws);
/* Up to four independent attentions of one shape (the four of an MSCSA level, reference models/layers.py:150-163) in as few launches as
 * fill the chip.  Where hupr_attn_fwd_split_ws_bytes() > 0 (single-sample inference — bound by launches, not work): ONE split launch and
 * ONE merge launch, ws: n_items times that size.  Otherwise (training batches; ws may be NULL): ONE launch of the one-pass kernel over all
 * items (levels 2 and 3), or one ping-pong launch per item (level-1 shape).  K / Q / V: bf16 with row strides ldk / ldq / C; Vres (fp32 V for the residual) and out16 (bf16 copy, stride ld16) may be null. */
typedef struct hupr_attn_item { const void* K; const void* Q; const void* V; const float* Vres; float* out; float* lse; void* out16; } hupr_attn_item;
int hupr_attn_fwd_bf16in_ld_ws_batch(const hupr_attn_item* items, int n_items, int ldk, int ldq, int ld16, int Bn, int N, int C,
                                     void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_attn_fwd_bf16in_ld_ws(const void* K, int ldk, const void* Q, int ldq, const void* V, const float* Vres, float* out,
                               float* lse, void* out16_or_null, int ld16, int Bn, int N, int C, void* ws, size_t ws_bytes,
                               hupr_stream_t stream);
int hupr_attn_bwd_bf16in_ld(const void* K, int ldk, const void* Q, int ldq, const void* V, const void* dO, int lddo,
                            const float* V32, const float* out, const float* dout32_or_null, const float* lse, float* dK,
                            int lddk, float* dQ, int lddq, float* dV, float* Dq_scratch, int Bn, int N, int C,
                            int residual, int accumulate, hupr_stream_t stream);
/* The "QS" forms (round 5): the query operand arrives pre-scaled, Qs = log2(e) Q as bf16 (the level's query projections multiply by
 * log2(e)-scaled weight rows: hupr_pack_conv_weights_table, block layout 3), so that K . Qs^T is the exponent of 2 and the score
 * leaves the matrix pipe as the argument of v_exp_f32: the MFMA chain of a score tile starts from minus the running maximum
 * (forward; kept until a tile exceeds it by more than 8 binary orders) or minus the stored log-sum-exp (backward) instead of 0.
 * Same semantics as the entry points above: out / lse (natural units) of softmax_keys(K Q^T), gradients with respect to K, the
 * UNSCALED Q and V.  Same reference lines (models/layers.py:126-133). */
int hupr_attn_fwd_bf16in_ld_ws_qs(const void* K, int ldk, const void* Qs, int ldq, const void* V, const float* Vres, float* out,
                                  float* lse, void* out16_or_null, int ld16, int Bn, int N, int C, void* ws, size_t ws_bytes,
                                  hupr_stream_t stream);
int hupr_attn_fwd_bf16in_ld_ws_batch_qs(const hupr_attn_item* items, int n_items, int ldk, int ldq, int ld16, int Bn, int N, int C,
                                        void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_attn_bwd_bf16in_ld_qs(const void* K, int ldk, const void* Qs, int ldq, const void* V, const void* dO, int lddo,
                               const float* V32, const float* out, const float* dout32_or_null, const float* lse, float* dK,
                               int lddk, float* dQ, int lddq, float* dV, float* Dq_scratch, int Bn, int N, int C, int residual,
                               int accumulate, hupr_stream_t stream);
/* The backward passes of up to four attentions of one shape and one set of strides (the four of an MSCSA level, reference
 * models/layers.py:150-163 under autograd) with a bf16-stored gradient dO: one row-sum launch, one dQ launch, and dK / dV launches
 * in as many rounds as the dV targets need (an item with `accumulate` adds onto the dV an EARLIER item writes).  Same results as n
 * calls of hupr_attn_bwd_bf16in_ld(_qs) with dout32 == NULL in array order; the level-1 shape is launched per item as before.
 * hupr_attn_fwd_bf16in_ld_ws_batch(_qs) is the forward counterpart (ws may be NULL for training batches). */
typedef struct hupr_attn_bwd_item {
    const void* K; const void* Q; const void* V; const void* dO;      /* bf16 operands (Q: Qs for the _qs form) */
    const float* V32; const float* out; const float* lse;             /* fp32: values, forward output, log-sum-exp */
    float* dK; float* dQ; float* dV; float* Dq;                        /* outputs (row strides lddk / lddq / C) and a (Bn, N) scratch of its own */
    int residual, accumulate;
} hupr_attn_bwd_item;
int hupr_attn_bwd_bf16in_ld_batch(const hupr_attn_bwd_item* items, int n_items, int ldk, int ldq, int lddo, int lddk, int lddq,
                                  int Bn, int N, int C, hupr_stream_t stream);
int hupr_attn_bwd_bf16in_ld_batch_qs(const hupr_attn_bwd_item* items, int n_items, int ldk, int ldq, int lddo, int lddk, int lddq,
                                     int Bn, int N, int C, hupr_stream_t stream);

/* (a7) PRGCN: y = act(t . A + bias) with t = W . x computed by hupr_gemm_f32 (gcn_networks.py:23-29,53-58) */
/* The 1x1 key-point head nn.Conv2d(32, 14, 1, bias=False) (reference models/layers.py:94) in plain fp32 FMAs: x [M][32],
 * w16 [16][32] (the 14 filters zero-padded to 16 output channels), y / dy [M][16]; backward writes dx [M][32] and / or
 * dw16 [16][32] (either may be null).  Used for the "head" precision region of bf16 runs (functional.PRECISION). */
size_t hupr_head1x1_ws_bytes(void);
int hupr_head1x1_fwd_f32(const float* x, const float* w16, float* y, long M, hupr_stream_t stream);
int hupr_head1x1_bwd_f32(const float* x, const float* w16, const float* dy, float* dx_or_null, float* dw16_or_null, long M,
                         void* ws, size_t ws_bytes, hupr_stream_t stream);
/* ... writing only the first out_rows (<= 16) filter rows of dw: out_rows = 14 lets dw be the (14, 32, 1, 1) parameter's own gradient
 * slot in a flat bucket (reference models/layers.py:94: nn.Conv2d(nf, numKeypoints, 1)) */
int hupr_head1x1_bwd_rows_f32(const float* x, const float* w16, const float* dy, float* dx_or_null, float* dw_or_null, int out_rows,
                              long M, void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_gcn_adj_fwd_f32(const float* t, const float* adj, const float* bias, float* y, int Bn, int F, int K,
                         int ld, int relu, hupr_stream_t stream);
/* t as `slices` partial products [slices][Bn*F][ld] (the K slices of W x of a single-sample forward), summed here in slice order */
int hupr_gcn_adj_fwd_sliced_f32(const float* t, int slices, const float* adj, const float* bias, float* y, int Bn, int F,
                                int K, int ld, int relu, hupr_stream_t stream);
int hupr_gcn_adj_bwd_f32(const float* dy, const float* y, const float* adj, float* dt, float* gmasked,
                         float* dbias, int Bn, int F, int K, int ld, int relu, hupr_stream_t stream);
/* The feature products of a PRGCN layer on the fp32 matrix pipe, batch folded into the MFMA column axis in place (x, t, dt: (Bn, F, 16),
 * W: (F, F) as nn.Parameter of gcn_networks.py:18 stores it; ld must be 16, F a multiple of 64):
 *   hupr_gcn_wx_f32, trans_w = 0:  t[b][f][n]  = sum_g W[f][g] x[b][g][n]       support = W . x          (gcn_networks.py:25)
 *   hupr_gcn_wx_f32, trans_w = 1:  t[b][g][n]  = sum_f W[f][g] x[b][f][n]       its input gradient W^T . dt
 *   hupr_gcn_dw_f32:               dW[f][g]    = sum_{b,n} dt[b][f][n] x[b][g][n]                     its weight gradient */
int hupr_gcn_wx_f32(const float* W, const float* x, float* t, int Bn, int F, int ld, int trans_w, hupr_stream_t stream);
int hupr_gcn_dw_f32(const float* dt, const float* x, float* dW, int Bn, int F, int ld, hupr_stream_t stream);

/* (a8) sigmoid heads: channels-last logits (B,HW,ld) -> NCHW probabilities (B,K,HW)  (networks.py:40, gcn_networks.py:64) */
int hupr_sigmoid_to_nchw_f32(const float* x, float* y, int Bn, int HW, int K, int ld, hupr_stream_t stream);
int hupr_sigmoid_to_nchw_bwd_f32(const float* dy, const float* y, float* dx, int Bn, int HW, int K, int ld,
                                 hupr_stream_t stream);

/* (a9) loss / targets / decode (misc/losses.py:23-45, misc/utils.py:6-66, misc/metrics.py:10-38) */
size_t hupr_bce_ws_bytes(void);
int hupr_bce_fwd_f32(const float* p, const float* t, long n, float* loss, void* ws, size_t ws_bytes,
                     hupr_stream_t stream);
int hupr_bce_bwd_f32(const float* p, const float* t, const float* grad_out, float* dp, long n, hupr_stream_t stream);
/* Both losses of a step and their weighted sum (reference misc/losses.py:24-33: loss = alpha * BCE(heatmap, target) + beta * BCE(gcn
 * heatmap, target)) in two launches: loss3 = {loss, loss1, loss2}, the same floats as two hupr_bce_fwd_f32 calls and torch's scalar
 * arithmetic; the backward takes the gradient of `loss` (and optionally of loss2) and writes both dp.  ws: 2 x hupr_bce_ws_bytes(). */
int hupr_bce_pair_fwd_f32(const float* p1, const float* p2, const float* t, long n, float alpha, float beta, float* loss3, void* ws,
                          size_t ws_bytes, hupr_stream_t stream);
int hupr_bce_pair_bwd_f32(const float* p1, const float* p2, const float* t, const float* grad_loss, const float* grad_loss2_or_null,
                          float alpha, float beta, float* dp1, float* dp2, long n, hupr_stream_t stream);
/* The pair loss with online hard keypoint mining (the top-k joint selection of CPN's RefineNet and HRNet's JointsOHKMMSELoss) and
 * per-joint weights (HRNet's target_weight), csrc/bce_mined.hip.  New, no reference counterpart; with k = K and no weights it is
 * hupr_bce_pair_fwd_f32 up to the order of summation.  Two launches forward, one backward, no workspace, no atomics: every output
 * is bit-identical from run to run.  p1, p2, t: float [B][K][HW]; head h = 0 is p1, h = 1 is p2.
 *   Plane loss   l[h,b,j] = the mean over the plane's HW cells of -(t log p + (1 - t) log(1 - p)), both logs clamped at -100 (the
 *                term of hupr_bce_fwd_f32 for every number; a NaN cell, or p outside [0, 1], gives a NaN plane loss), summed by one workgroup in an order fixed by HW alone: planes with equal contents give
 *                equal bits.  v[h,b,j] = w[j] * l[h,b,j], with w = joint_w_or_null (K floats) or all ones when it is null.
 *                plane_loss (2, B, K) receives l, not v.
 *   Selection    the K planes of one (head, sample) are ordered by v descending; a NaN ranks above every number (a non-finite
 *                forward reaches the loss, it is not mined away); equal values, and two NaNs, order by lower joint index first.
 *                sel[h,b,j] = 1 for the first k planes in that order and 0 for the rest.  Each head mines on its own.
 *   Losses       L_h = (1 / (B k)) sum_b sum_j sel * v, summed in fp64 in an order fixed by (B, K).
 *                loss3 = {alpha L_0 + beta L_1, L_0, L_1}; the two products and the sum are rounded separately, as in
 *                hupr_bce_pair_fwd_f32.
 *   Coefficients coef[h,b,j] (2, B, K) = sel ? w[j] / (B k HW) : 0  — what the backward scales a plane by.
 *   Counters     with counts_or_null non-null (2, K) int64: counts[h,j] += sum_b sel[h,b,j].  Plain adds by one workgroup; the
 *                caller zeroes the array once.
 *   Backward     dp_h[b,j,x] = G_h * coef[h,b,j] * (p - t) / max(p (1 - p), 1e-12), G_0 = g * alpha, G_1 = g * beta (+ g2): the
 *                arithmetic of hupr_bce_pair_bwd_f32 with a per-plane scale.  No gradient flows through the selection.  A plane
 *                whose scale G_h * coef is zero is written as zeros without being read; every cell of dp1 and dp2 is written.
 * Both return -1 (HUPR_ERR_ARG) before any launch for a null pointer (the two _or_null ones excepted), K outside [1, 64], B < 1,
 * HW < 1, B * K * HW beyond the 64-bit index arithmetic, and the forward for k outside [1, K].  16-byte loads and stores where
 * HW % 4 == 0 and the maps are 16-byte aligned, 4-byte ones otherwise. */
int hupr_bce_mined_fwd_f32(const float* p1, const float* p2, const float* t, long B, int K, long HW, int k,
                           const float* joint_w_or_null, float alpha, float beta, float* loss3, float* plane_loss, float* coef,
                           long long* counts_or_null, hupr_stream_t stream);
int hupr_bce_mined_bwd_f32(const float* p1, const float* p2, const float* t, const float* coef, const float* grad_loss,
                           const float* grad_loss2_or_null, float alpha, float beta, float* dp1, float* dp2, long B, int K, long HW,
                           hupr_stream_t stream);
/* Integral (soft-arg-max) coordinate loss on both heads (Sun et al., "Integral Human Pose Regression", ECCV 2018; Nibali et al., DSNT),
 * csrc/coord_loss.hip: an L1 on the offset of each plane's mass centroid from its joint, in heat-map pixels.  New, no reference
 * counterpart.  Two launches forward, one backward, no workspace, no atomics, no scratch: every output is bit-identical from run to
 * run, and equal planes with equal joints give equal bits.  p1, p2: float [B][K][H][H] probabilities, p[b][j][y][x]; head h = 0 is
 * p1, h = 1 is p2.  joints_xy: float [B][K][2] = (x, y) in image pixels.  Per row (h, b, j) and axis, in fp32:
 *   Position     a = joint / stride; with snap != 0, a = (float)(int)(a + 0.5f): the pixel hupr_gaussian_targets_f32 centres its
 *                patch on, with the truncating cast and the guard of hupr_gaussian_targets_subpixel_f32 (decided in float
 *                arithmetic, the cast is not executed on a NaN, an infinity or a + 0.5f outside [-2^31, 2^31): the row is invalid).
 *   Validity     the row is valid iff both a are finite and 0 <= a <= H - 1.
 *   Residual     S = sum p, N_x = sum p (x - a_x), N_y = sum p (y - a_y) over the plane, r = N / (S + eps): the offset of the mass
 *                centroid from the joint, shrunk by S / (S + eps).  Relative to the joint, so eps biases nothing at the optimum
 *                (r = 0 exactly when the centroid is on the joint), and the gradient stays bounded by about H / eps on a nearly
 *                empty plane.  A NaN cell in a valid plane gives a NaN residual; it is not masked.
 *   Row loss     l = w[j] (|r_x| + |r_y|) for a valid row and exactly 0 for an invalid one, whose plane is not read; w =
 *                joint_w_or_null (K floats) or all ones when it is null.
 *   Head loss    C_h = (1 / (2 B K)) sum_b sum_j l: a fixed denominator, invalid rows count as zeros; summed in fp64 in an order
 *                fixed by (B, K).
 *   Outputs      loss3 = {a0 C_0 + a1 C_1, C_0, C_1}, the two products and the sum rounded separately as in hupr_bce_pair_fwd_f32;
 *                resid (2, B, K, 2) receives r (zeros for an invalid row); scale (2, B, K) receives w[j] / (S + eps) for a valid row
 *                and 0 for an invalid one.
 *   Accumulator  with acc_or_null non-null (3 doubles): acc[0] += C_0, acc[1] += C_1, acc[2] += 1.  Plain adds by one workgroup;
 *                the caller zeroes the array once.
 *   Backward     dp_h[b,j,y,x] = G_h scale[h,b,j] / (2 B K) * (sgn(r_x) (x - a_x - r_x) + sgn(r_y) (y - a_y - r_y)), G_0 = g a0,
 *                G_1 = g a1, sgn(0) = 0.  It reads resid, scale, the joints and g, never the maps: a store-only kernel.  Every cell
 *                of dp1 and dp2 is written; a row whose factor G_h scale / (2 B K) is zero is written as zeros; a NaN factor or
 *                residual reaches every cell of its plane.  No gradient flows to the joints.
 * Reduction shape: one 256-thread workgroup (four wave64) per plane; a thread adds its H * H / 256 cells (16 at H = 64, 64 at
 * H = 128) in index order into fp32 partials of S, N_x, N_y; then the wave butterfly (6 additions) and the four waves through LDS in
 * wave order.  16-byte loads and stores where H % 4 == 0 and the maps are 16-byte aligned, 4-byte ones otherwise.
 * Both return -1 (HUPR_ERR_ARG) before any launch for a null pointer (the two _or_null ones excepted), B < 1, K outside [1, 64],
 * H outside [1, 4096], B * K * H * H beyond the 64-bit index arithmetic, stride not finite or not positive, and the forward for eps
 * not finite or not positive. */
int hupr_coord_loss_fwd_f32(const float* p1, const float* p2, const float* joints_xy, long B, int K, int H, float stride, int snap,
                            const float* joint_w_or_null, float eps, float a0, float a1, float* loss3, float* resid, float* scale,
                            double* acc_or_null, hupr_stream_t stream);
int hupr_coord_loss_bwd_f32(const float* resid, const float* scale, const float* joints_xy, const float* grad_loss, long B, int K, int H,
                            float stride, int snap, float a0, float a1, float* dp1, float* dp2, hupr_stream_t stream);
/* Bone-vector loss on both heads (Sun et al., "Compositional Human Pose Regression", ICCV 2017), csrc/bone_loss.hip: an L1 on the
 * error of the vector between the mass centroids of the two planes at the ends of every bone of a skeleton table, in heat-map pixels.
 * New, no reference counterpart.  Two launches forward, one backward, no workspace, no atomics, no scratch: every output is
 * bit-identical from run to run, and equal planes with equal joints give equal bits.  p1, p2, joints_xy, stride, snap, eps: as in
 * hupr_coord_loss_fwd_f32, with its Position and Validity; a joint is valid iff both axes are valid.
 *   Residual     per (h, b, j): S = sum p, N = sum p (x - a_x, y - a_y), den = S + eps, r = N / den: hupr_coord_loss_fwd_f32's
 *                residual by the same arithmetic in the same summation order (one body, csrc/coord_plane.h); for equal inputs and
 *                eps the bits equal that entry's resid.  inv_den = 1 / den.  An invalid joint gives r = 0 and inv_den = 0, and its
 *                plane is not read.  A NaN cell in a valid plane gives a NaN r and inv_den; it is not masked.
 *   Bones        bones_host: a HOST table of 2 E ints, bone e = (u_e, v_e); 1 <= E <= 32, every index in [0, K), u_e != v_e.  It is
 *                checked on the host and copied into the kernel's arguments.  A bone is valid iff both its joints are valid.
 *   Bone error   d[h,b,e] = r[h,b,v_e] - r[h,b,u_e], two fp32 subtractions; exactly 0 for an invalid bone.  Up to the eps damping
 *                this is (c_v - c_u) - (a_v - a_u), the error of the predicted bone vector: a pose whose every joint is displaced by
 *                the same offset costs nothing.
 *   Head loss    B_h = (1 / (2 B E)) sum_b sum_e w_e (|d_x| + |d_y|), w = bone_w_or_null (E floats on the device) or all ones when
 *                it is null: a fixed denominator, invalid bones count as zeros; summed in fp64 in an order fixed by (B, E).
 *   Coefficient  gcoef[h,b,j] = sum_{e: v_e = j} w_e sgn(d_e) - sum_{e: u_e = j} w_e sgn(d_e) per axis, accumulated in fp32 in bone-
 *                index order over the valid bones; sgn(0) = 0 and a NaN d stays a NaN: nothing is masked, so a NaN cell reaches both
 *                of the bone's joints.  A weight of zero is plain arithmetic, not a mask.
 *   Outputs      loss3 = {a0 B_0 + a1 B_1, B_0, B_1}, the two products and the sum rounded separately as in
 *                hupr_coord_loss_fwd_f32; resid (2, B, K, 2); inv_den (2, B, K); bone_resid (2, B, E, 2) receives d; gcoef
 *                (2, B, K, 2).
 *   Accumulator  with acc_or_null non-null (3 doubles): acc[0] += B_0, acc[1] += B_1, acc[2] += 1.  Plain adds by one workgroup;
 *                the caller zeroes the array once.
 *   Backward     dp_h[b,j,y,x] = f (gcoef_x ((x - a_x) - r_x) + gcoef_y ((y - a_y) - r_y)), f = (g a_h) inv_den[h,b,j] / (2 B E).
 *                It reads resid, inv_den, gcoef, the joints and g, never the maps: a store-only kernel.  Every cell of dp1 and dp2 is
 *                written; a plane whose f is zero, or whose two coefficients are both zero, is written as zeros; a NaN factor or
 *                coefficient is not zero and fills its plane.  No gradient flows to the joints.
 * Launches: the plane pass of hupr_coord_loss_fwd_f32 (one 256-thread workgroup per plane; 16-byte loads and stores where
 * H % 4 == 0 and the maps are 16-byte aligned, 4-byte ones otherwise), then one workgroup that writes bone_resid, gcoef and loss3 and
 * moves acc; each gcoef thread recomputes the d of its incident bones from resid, which gives the same bits.
 * Both return -1 (HUPR_ERR_ARG) before any launch for a null pointer (the two _or_null ones excepted), B < 1, K outside [1, 64],
 * H outside [1, 4096], B * K * H * H beyond the 64-bit index arithmetic, stride not finite or not positive, E outside [1, 32], and the
 * forward for eps not finite or not positive and for a bone with an index outside [0, K) or with u == v. */
int hupr_bone_loss_fwd_f32(const float* p1, const float* p2, const float* joints_xy, long B, int K, int H, float stride, int snap,
                           const int* bones_host, int E, const float* bone_w_or_null, float eps, float a0, float a1, float* loss3,
                           float* resid, float* inv_den, float* bone_resid, float* gcoef, double* acc_or_null, hupr_stream_t stream);
int hupr_bone_loss_bwd_f32(const float* resid, const float* inv_den, const float* gcoef, const float* joints_xy, const float* grad_loss,
                           long B, int K, int E, int H, float stride, int snap, float a0, float a1, float* dp1, float* dp2,
                           hupr_stream_t stream);
int hupr_gaussian_targets_f32(const long long* joints, const float* patch, float* t, int BK, int H, int rad,
                              float stride, hupr_stream_t stream);
int hupr_argmax_rows_f32(const float* p, long rows, int n, int* idx, float* maxval, hupr_stream_t stream);
/* Sub-pixel Gaussian targets in one launch (csrc/targets.hip): the unbiased encoding of Zhang et al., "Distribution-Aware Coordinate
 * Representation for Human Pose Estimation" (CVPR 2020), inside the window and in-bounds rule of the reference's targets
 * (misc/utils.py:6-66, hupr_gaussian_targets_f32 above).  hupr_pose_decode_f32 with refine != 0 inverts it.  No host table, no
 * workspace, no LDS, no scratch; every element of t is written exactly once, zeros included, so t may be uninitialised.
 * joints_xy : float [BK][2] = (x, y) in image pixels.  t : float [BK][H][H], t[r][y][x].  For row r and each axis, in fp32:
 *   ac = joint / stride;  mu = (int)(ac + 0.5f) (the truncating cast of hupr_gaussian_targets_f32);  f = ac - (float)mu.
 * The plane of row r is all zeros
 *   when mu_x - rad >= H, mu_y - rad >= H, mu_x + rad + 1 < 0 or mu_y + rad + 1 < 0 (the window lies outside the map), or
 *   when a coordinate is NaN or infinite, or ac + 0.5f is outside [-2^31, 2^31): decided in float arithmetic, the cast is not
 *   executed then, and a NaN never reaches t.
 * Otherwise cell (x, y), with dx = x - mu_x, dy = y - mu_y, |dx| <= rad, |dy| <= rad, 0 <= x, y < H, holds
 *   expf(-((dx - f_x)^2 + (dy - f_y)^2) / (2 sigma^2))
 * and every other cell holds exactly 0.0f.  A joint on a whole map pixel (f == 0) gives the support of hupr_gaussian_targets_f32
 * exactly and its values up to the rounding of expf.  (The cast truncates towards zero, so for ac < -0.5 the window's middle is the
 * pixel above the nearest one and f lies in (-1.5, -0.5]: the window is still that of hupr_gaussian_targets_f32, the Gaussian is on
 * the joint.)
 * Returns -1 (HUPR_ERR_ARG) before any launch for a null pointer, BK < 0 or BK * H * H beyond the 64-bit index arithmetic, H outside
 * [1, 4096], rad < 1, sigma or stride not finite or not positive (or 2 sigma^2 not a positive finite float).  Any other H is accepted:
 * 16-byte stores where H % 4 == 0 and t is 16-byte aligned, 4-byte stores otherwise; H may be smaller than the window.
 * BK == 0 is a no-op. */
int hupr_gaussian_targets_subpixel_f32(const float* joints_xy, float* t, long BK, int H, float sigma, int rad, float stride,
                                       hupr_stream_t stream);

/* (a10) Adam with coupled L2 weight decay (tools/base.py:47), one flat launch */
int hupr_adam_step_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int step, float gscale, hupr_stream_t stream);
/* same, {learning rate, step count} read from device memory (2 floats): for steps replayed from a captured hipGraph */
int hupr_adam_step_dev_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, const float* dev_state,
                           float beta1, float beta2, float eps, float weight_decay, float gscale, hupr_stream_t stream);
/* (a10) SGD with momentum and coupled L2 weight decay (tools/base.py:44-45; torch.optim.SGD with dampening 0, no Nesterov),
 * one flat launch.  first != 0 on the parameter's first step: the buffer is set to the decayed gradient (old contents
 * ignored). */
int hupr_sgd_step_f32(float* p, const float* g, float* momentum_buf, long n, float lr, float momentum,
                      float weight_decay, int first, float gscale, hupr_stream_t stream);
/* same, {learning rate, step count} read from device memory (the 2 floats of hupr_adam_step_dev_f32); step 1 is the first */
int hupr_sgd_step_dev_f32(float* p, const float* g, float* momentum_buf, long n, const float* dev_state,
                          float momentum, float weight_decay, float gscale, hupr_stream_t stream);

/* (a11) Gradient guard: global-norm clipping and the skip of a non-finite step, decided on the device (csrc/optim.hip).
 * New, no reference counterpart: the reference steps on whatever backward left (tools/run.py:78-79).  Per optimiser step and
 * stream: hupr_grad_sumsq_f32 once per gradient bucket, hupr_grad_guard_f32 once, then the *_step_guard_f32 entry per bucket.
 * No atomics: results are bit-identical from run to run.  All of it is stream-ordered and capturable in a hipGraph. */
/* number of fp64 partials one hupr_grad_sumsq_f32 call writes */
int hupr_grad_sumsq_partials(void);
/* partials[0 .. hupr_grad_sumsq_partials()) <- partial sums of g[i]^2 over g[0 .. n), accumulated in fp64 (slots without an
 * element hold 0.0).  g may start at any 4-byte boundary: float4 loads from its first 16-byte boundary, scalar ends. */
int hupr_grad_sumsq_f32(const float* g, long n, double* partials, hupr_stream_t stream);
/* total = sum of partials[0 .. count) (the partials of all buckets, fixed order, fp64);  norm = gscale * sqrt(total);
 * coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; max_norm = +inf: exactly 1).
 * guard[0 .. 4) <- {coef, norm, skipped, finite}.  total finite: finite = 1 and dev_state[1] (the step count of
 * hupr_adam_step_dev_f32) += 1.  total not finite: coef = 0, finite = 0, skipped (guard[2], zeroed by the caller once) += 1
 * and dev_state[1] stays. */
int hupr_grad_guard_f32(const double* partials, int count, float gscale, float max_norm, float* dev_state, float* guard,
                        hupr_stream_t stream);
/* hupr_adam_step_dev_f32 / hupr_sgd_step_dev_f32 obeying guard: nothing is written when guard[3] == 0, otherwise the update
 * runs on g * (gscale * guard[0]) (one fp32 product; with coef = 1 the bits of the _dev entries). */
int hupr_adam_step_guard_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, const float* dev_state,
                             const float* guard, float beta1, float beta2, float eps, float weight_decay, float gscale,
                             hupr_stream_t stream);
int hupr_sgd_step_guard_f32(float* p, const float* g, float* momentum_buf, long n, const float* dev_state, const float* guard,
                            float momentum, float weight_decay, float gscale, hupr_stream_t stream);

/* (a12) Exponential moving average of the weights, kept and swapped on the device (csrc/optim.hip; TRAINING.emaDecay).
 * New, no reference counterpart: the reference evaluates `self.model` as trained, `tools/run.py:35-63`.  Per optimiser step and
 * stream, behind the optimiser's launches: hupr_ema_tick_f32 once, then hupr_ema_update_f32 once per parameter bucket.
 * No atomics: results are bit-identical from run to run.  All of it is stream-ordered and capturable in a hipGraph. */
/* ema_state[0 .. 2) = {updates, weight} in device memory.  guard: null, or the 4 floats of hupr_grad_guard_f32.  guard given and
 * guard[3] == 0 (the step was skipped): weight = 0, updates stays.  Otherwise, k = updates: d = min(decay, (1 + k) / (10 + k)) in
 * fp64 (the warm-up ramp: the first updates are not dominated by the initial weights), weight = (float)(1 - d), updates = k + 1.
 * One thread.  decay must be inside (0, 1). */
int hupr_ema_tick_f32(float* ema_state, float decay, const float* guard, hupr_stream_t stream);
/* ema[i] += w * (p[i] - ema[i]) over [0, n), w = ema_state[1]: one fp32 subtraction and one fused multiply-add per element, the
 * same bits whichever path runs.  w == 0 stores nothing (the bits of ema are kept, whatever p holds).  ema and p may start at any
 * 4-byte boundary: float4 accesses from the first 16-byte boundary and scalar ends when both share their offset to it, 4-byte
 * accesses otherwise.  ema and p must not overlap. */
int hupr_ema_update_f32(float* ema, const float* p, long n, const float* ema_state, hupr_stream_t stream);
/* a[0 .. n) <-> b[0 .. n), every bit pattern kept.  Alignment handled as in hupr_ema_update_f32; overlapping ranges are refused. */
int hupr_swap_f32(float* a, float* b, long n, hupr_stream_t stream);

/* (a13) LAMB: Adam's direction rescaled per parameter tensor by the trust ratio |p| / |u| (csrc/optim.hip; TRAINING.optimizer:
 * lamb).  New, no reference counterpart: the reference's choice is SGD or Adam, `tools/base.py:44-47`.  Per tensor, k = dev_state[1],
 * g' = g * gscale * (guard ? guard[0] : 1) (one fp32 product), bias corrections as hupr_adam_step_dev_f32 forms them:
 *   m <- b1 m + (1 - b1) g',  v <- b2 v + (1 - b2) g'^2,  d = (m / (1 - b1^k)) / (sqrt(v) / sqrt(1 - b2^k) + eps)
 *   adapted tensor: u = d + wd p, r = |p| / |u| if both norms > 0 else 1;  other tensor: u = d, r = 1;  p <- p - lr r u
 * No clamp on r; |p| is taken before the update.  The parameter tensors are the segments of a flat bucket, described by a chunk
 * table of int64 words that the caller builds once per bucket and keeps in host AND device memory:
 *   {segments S, chunks K, hupr_lamb_chunk(), n},  S x {start, length, first chunk, chunk count, adapted (0 | 1)},
 *   K x {segment, start relative to the segment}
 * The segments tile [0, n) in order; a segment is cut from its own start into ceil(length / hupr_lamb_chunk()) chunks, consecutive
 * in the table, so no chunk spans two tensors.  Every entry checks the host copy in front of its launch and the kernels read the
 * device copy.  Per optimiser step, bucket and stream: stage1, ratio, stage2.  {lr, step} are always read from dev_state (the 2
 * floats of hupr_adam_step_dev_f32); guard is null or the 4 floats of hupr_grad_guard_f32, and guard[3] == 0 makes all three
 * launches return before their first store.  The betas are doubles: 1 - beta is rounded to fp32 once (1.f - 0.999f is 1.3e-5 away
 * from 0.001).  fp32 data, fp64 norms, no atomics; which thread adds which element depends on the
 * segment lengths only, never on the addresses: the bits repeat from run to run and do not change when a bucket moves by a few
 * floats.  All of it is stream-ordered and capturable in a hipGraph. */
/* elements per chunk */
int hupr_lamb_chunk(void);
/* host only, launches nothing: 0 when table_host[0 .. words) is such a table over [0, n), -1 with a message otherwise */
int hupr_lamb_table_check(const long* table_host, long words, long n);
/* new exp_avg, exp_avg_sq over [0, n); partials[2c], partials[2c + 1] <- {sum p^2, sum u^2} of chunk c in fp64 (8-byte aligned) */
int hupr_lamb_stage1_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, const long* table_host, long words,
                         const long* table_dev, const float* dev_state, const float* guard, double beta1, double beta2, float eps,
                         float weight_decay, float gscale, double* partials, hupr_stream_t stream);
/* per segment s the pairs of its chunks added in table order: seg_stats[s] <- |p|, seg_stats[S + s] <- |u|, seg_stats[2 S + s] <- r */
int hupr_lamb_ratio_f32(const double* partials, long n, const long* table_host, long words, const long* table_dev,
                        const float* guard, float* seg_stats, hupr_stream_t stream);
/* u recomputed from p and the new exp_avg, exp_avg_sq (stage 1's bits); p <- p - (lr * seg_stats[2 S + s]) * u, one fused multiply-add */
int hupr_lamb_stage2_f32(float* p, const float* exp_avg, const float* exp_avg_sq, long n, const long* table_host, long words,
                         const long* table_dev, const float* dev_state, const float* guard, double beta1, double beta2, float eps,
                         float weight_decay, const float* seg_stats, hupr_stream_t stream);

/* (a14) Radar augmentation on the device (csrc/augment.hip; TRAINING.augMirror / augNoise / augMaskRange / augMaskAngle, TEST.flip).
 * New, no reference counterpart: the reference augments nothing and has no flip test.  One plan per training step, drawn by a
 * launch from a counter in device memory, so a step replayed from a hipGraph draws a fresh plan although its launch arguments are
 * frozen; the ADC mirror, the noise and masks and the labels consume that plan.  No atomics: every output is bit-identical from
 * run to run.  All of it is stream-ordered and capturable in a hipGraph.
 *
 * Generator: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key (seed, 4 rank + domain),
 * counter (step_lo, step_hi, b, q) for sample b.  A word w gives m = w >> 8 and u = m 2^-24 (exact in fp32); floor(u n) is formed
 * exactly, as (m n) >> 24 in 64-bit integers.
 *
 * state: {counter (u64), mirrored samples (u64), samples (u64), sum of sigma (f64)} in device memory, 8-byte aligned,
 * hupr_augment_state_bytes() bytes; the caller zeroes it (or sets the counter to resume).
 * table: (B, 8) 32-bit words per sample: {mirror (int 0 | 1), sigma (float), range band length, range band start, azimuth band length,
 * start of the horizontal map, azimuth band length, start of the vertical map}; a band covers [start, start + length). */
size_t hupr_augment_state_bytes(void);
/* Domain 0, step = state.counter.  Call q = 0 yields {mirror = u0 < p_mirror, sigma = sigma_max * u1 (one fp32 product), range length =
 * floor(u2 (max_range + 1)), range start = floor(u3 (R - length + 1))}; call q = 1 the two azimuth bands the same way from max_angle
 * and A.  Also flags[b] = mirror as a byte.  Then one thread adds, in sample order: counter += 1, mirrored += sum of mirror, samples
 * += B, sum of sigma += sigma in fp64.  One launch of one workgroup.  A setting that is off is passed as 0 (p_mirror 0, sigma_max 0,
 * a maximal band length 0).  p_mirror in [0, 1], sigma_max finite >= 0, max_range <= R / 2, max_angle <= A / 2, B in [1, 65535]. */
int hupr_augment_plan(int B, void* state, float p_mirror, float sigma_max, int max_range, int max_angle, int R, int A, unsigned seed,
                      int rank, void* table, unsigned char* flags, hupr_stream_t stream);
/* The left/right mirror of the scene as a permutation of the raw cube adc[n_sf][4 rx][192 = 3 cc + tx][256][2] int16, in front of the
 * FFT chain: out[f][rx][3 cc + tx] = adc[f][3 - rx][3 cc + 2 - tx] for the frames f with flags[f / G] != 0 (null: every frame), a
 * plain copy for the others.  Reversing the receivers and swapping transmitters 0 and 2 reverses the 8 azimuth antennas and the
 * elevated row on its columns 2..5; the chain's output for the permuted cube is its output at azimuth bin (62 - a) mod 64 times
 * exp(-2 pi i 7 ((31 - a) mod 64) / 64), which no operation behind the chain's Normalize can form.  Out of place (overlap is
 * refused); 16-byte accesses, both pointers 16-byte aligned; 786 432 B per frame each way. */
int hupr_adc_mirror_i16(const void* adc, void* out, int n_sf, int G, const unsigned char* flags_or_null, hupr_stream_t stream);
/* Noise and band masks on a contiguous network input x[B][P][R][A][E] (E = 1: the elevation-mean planes, E = 8: the reference-shaped
 * tensor with P = G 8 2), y = x allowed.  sensor 0 | 1 = horizontal | vertical: generator domain 1 + sensor and that map's azimuth
 * band.  step = state.counter - 1, the plan drawn last.  Elements 4 q .. 4 q + 3 of sample b (flat index inside the sample) take the four
 * words {w0, w1, w2, w3} of call q: z0, z1 = r(w0) * {cospif, sinpif}(2 u(w1)), z2, z3 likewise from (w2, w3), r(w) = sqrtf(-2 ln u1)
 * with u1 = ((w >> 8) + 0.5) 2^-24; the logarithm is logf(u1) for m < 2^23 and log1pf(-(1 - u1)) above, 1 - u1 = (2^24 - 1 - m + 0.5)
 * 2^-24, so that its argument is exact in fp32 either way.  Precise library functions, no fast intrinsics.  y = fmaf(sigma_b, z, x);
 * sigma_b == 0 reads no generator and keeps the element's bits.  Then every element with r inside the range band or a inside the
 * map's azimuth band is set to 0.0f.  16-byte accesses when P R A E % 4 == 0 and x, y are 16-byte aligned, 4-byte accesses of the
 * same quads otherwise: the same bits.  B in [1, 65535], a sample of at most 2^33 elements. */
int hupr_augment_apply_f32(const float* x, float* y, int B, int P, int R, int A, int E, const void* table, int sensor, const void* state,
                           unsigned seed, int rank, hupr_stream_t stream);
/* The labels: joints (B, K, 2) = (x, y) in image pixels, int64 (is_float 0) or float32 (1), written out of place.  A sample with
 * flags[b] != 0 (null: every sample): out[b][j] = (x_mirror - x, y) of joints[b][pair[j]]; others are copied.  x_mirror = stride (H - 1),
 * the image column of the heat-map grid's centre doubled (252 for stride 4, H = 64): the decode maps heat-map pixel m to image 4 m, so
 * only this axis makes the mirrored target the mirror m -> H - 1 - m of the target.  pair_host: K ints in HOST memory (K <= 64), an
 * involution of [0, K); it travels by value with the launch.  No clamp: a coordinate beyond x_mirror goes negative. */
int hupr_augment_joints(const void* joints, void* out, long B, int K, int is_float, const unsigned char* flags_or_null,
                        const int* pair_host, long x_mirror, hupr_stream_t stream);
/* The flip-test merge of a head's maps p (B, K, H, W) and the maps pm of the mirrored input:
 * out[b][k][y][x] = 0.5f * (p[b][k][y][x] + pm[b][pair[k]][y][W - 1 - x]), the sum first.  pair_host as above.  out overlaps no input. */
int hupr_flip_merge_f32(const float* p, const float* pm, float* out, long B, int K, int H, int W, const int* pair_host,
                        hupr_stream_t stream);

/* (a15) Interference blanking of the raw cube in front of the FFT chain (csrc/interference.hip; DATASET.interference, the live
 * stream's `interference=`).  New, no reference counterpart: the reference transforms the cube as it comes.  A second FMCW radar in
 * the band (every HuPR capture runs two) leaves short high-amplitude bursts in single chirps wherever the ramps cross inside the IF
 * bandwidth; the range transform smears one over all 64 range bins.  The rule is integer arithmetic on the int16 samples: every
 * output is exact, repeats bit for bit, and no launch uses an atomic.  Stream-ordered and capturable in a hipGraph.
 *
 * adc[n_sf][4 rx][192 = 3 cc + tx][256][2] int16.  A group is one (sensor-frame, rx, tx): 64 chirp loops cc of 256 complex samples,
 * 64 rows of 1 KiB, 3 KiB apart; group index 3 rx + tx.  Groups are independent.  Per group:
 *   1. S[s] = sum over the 64 loops of x[cc][s], per component, int32.
 *   2. r[cc][s] = 64 x[cc][s] - S[s] per component (64 times the clutter-removed sample, |r| < 2^22) and p[cc][s] = r_I^2 + r_Q^2 as an
 *      unsigned 64-bit integer (< 2^45).
 *   3. med[cc] = the lower median of the loop's 256 values of p: the 128th smallest, sorted index 127.
 *   4. sample (cc, s) is flagged when p > K max(med, 1), compared in 64 bits; K is a power ratio, an integer in [2, 1024].
 *   5. the flags are dilated along s by `guard` samples on each side (guard in [0, 8]), clipped at samples 0 and 255; never into
 *      another loop.
 *   6. an unflagged sample is copied.  A flagged one is replaced, per component, by
 *        fill = HUPR_INTERFERENCE_FILL_CLUTTER: floor((2 Sc + n) / (2 n)), Sc the sum of x[cc'][s] over the n loops cc' NOT flagged at s
 *               (the clutter estimate rounded half up; 0 when n = 0) - behind the chain's clutter null that is a zero in the
 *               clutter-removed domain;
 *        fill = HUPR_INTERFERENCE_FILL_ZERO: 0.
 * Under complex Gaussian noise alone the flag rate is close to 2^-K, a little above it because the 256-sample median is itself noisy.
 * mask_or_null: uint8 [n_sf][4][192][32], bit s % 8 of byte s / 8 of a row = sample s flagged (after dilation), 4-byte aligned.
 * group_counts: int32 [n_sf][12][2] = {samples replaced, loops touched} per group.  out == adc exactly is allowed (a workgroup holds
 * its whole group before it writes); any other overlap between the buffers is refused.  adc and out 16-byte aligned.  One launch,
 * one workgroup per group; 786 432 B per sensor-frame each way.  n_sf == 0 is a no-op; n_sf at most 2^20. */
#define HUPR_INTERFERENCE_FILL_CLUTTER 0
#define HUPR_INTERFERENCE_FILL_ZERO 1
int hupr_adc_interference_i16(const void* adc, void* out, int n_sf, int K, int guard, int fill, unsigned char* mask_or_null,
                              int* group_counts, hupr_stream_t stream);
/* stats[n_sf][2] int32 = the sums of group_counts over a sensor-frame's 12 groups, in group order: {samples replaced, chirps touched}.
 * One small launch.  stats does not overlap group_counts. */
int hupr_adc_interference_stats(const int* group_counts, int n_sf, int* stats, hupr_stream_t stream);

/* (a16) Radar scene simulator: moving point scatterers -> the raw ADC cube of one sensor (csrc/radar_scene.hip; hupr_amd.simulate,
 * `python -m hupr_amd.tools.simulate`).  New, no reference counterpart: the reference only reads recorded captures.  NOT real data:
 * isotropic points of fixed amplitude, no multipath, no occlusion, no antenna pattern.
 *
 * The model.  A scene holds `frames` frames of S scatterers; per frame f and scatterer s a position p0 = pos[f][s][0..2] (metres), a
 * velocity v = vel[f][s][0..2] (metres per second), both at the start of that frame's burst, and an amplitude a = amp[f][s] >= 0.
 * The sensor is three transmitter positions tx[0..2][3] and four receiver positions rx[0..3][3] (metres, same coordinates), and three
 * scalars: wavelength (metres), range_bin_m (metres per bin of the 256-point range transform) and chirp_period_s.  Chirp c in 0..191
 * fires at t = c * chirp_period_s from transmitter c % 3 (the reference's demultiplexing); within a chirp nothing
 * moves (stop-and-hop).  For receiver r and sample n in 0..255:
 *     p    = p0 + v * t
 *     path = |p - tx[c % 3]| + |p - rx[r]|
 *     value(r, c, n) = sum over s of  a / (|p - tx| * |p - rx|) * exp(2 pi i (path / wavelength + n * path / (2 * 256 * range_bin_m)))
 * A receding scatterer's phase grows from chirp to chirp.  I is the real part, Q the imaginary part.
 *
 * The arithmetic.  In fp64, every operation rounded on its own (no fused multiply-add), in this order:
 *     p[k] = p0[k] + v[k] * t,  t = (double)c * chirp_period_s;     d(q) = sqrt((dx * dx + dy * dy) + dz * dz), dk = p[k] - q[k];
 *     path = d(tx) + d(rx);   u = path / wavelength;   w = path / (512.0 * range_bin_m);
 *     phi0 = rint((u - floor(u)) * 2^32) mod 2^32,   dphi = rint((w - floor(w)) * 2^32) mod 2^32       (ties to even; uint32)
 *     A    = (float)((double)a / (d(tx) * d(rx)))
 * The phase of sample n is phi0 + n * dphi in wrapping uint32 arithmetic — a numerically controlled oscillator, so the reduction
 * modulo one turn is exact.  Read as a signed int32 and converted to fp32 (nearest even), times 2^-32, it is a fraction x of a turn in
 * [-0.5, 0.5]; cs = cos(2 pi x), sn = sin(2 pi x) in fp32 (at most 2 ulp); re = fmaf(A, cs, re), im = fmaf(A, sn, im) in fp32 from
 * 0, in scatterer order.  add_or_null: fp32 in the cube's own layout [frames][4][192][256][2], added to (re, im) after the sum (the
 * Python layer's seeded receiver noise; the entry stays a pure function of its arguments).  hupr_radar_scene_f32 stores (re, im);
 * hupr_radar_scene_i16 stores rint (ties to even) clipped to [-32768, 32767] (a NaN, possible only through add, gives -32768).
 *
 * Hidden scatterers.  A scatterer contributes nothing to a (frame, chirp, receiver) — exactly: the bits are those of the scene
 * without it — unless its amplitude is finite and > 0, its position and velocity are finite and both distances are non-zero.
 *
 * pos, vel: device fp64 [frames][S][3], amp: device fp32 [frames][S]; tx_host [3][3], rx_host [4][3]: HOST fp64, finite, they travel by
 * value with the launch.  out: device, int16 or fp32 [frames][4][192][256][2].  One launch, one workgroup per (frame, chirp), no
 * workspace, no atomics: the same inputs give the same bits.  S in [1, 4096]; frames in [0, 2^20], 0 is a no-op; the three scalars
 * positive and finite.  Stream-ordered and capturable in a hipGraph.  9.4e6 complex exponentials per sensor-frame at S = 48. */
int hupr_radar_scene_i16(const double* pos, const double* vel, const float* amp, const double* tx_host, const double* rx_host, int frames,
                         int S, double wavelength, double range_bin_m, double chirp_period_s, const float* add_or_null, void* out,
                         hupr_stream_t stream);
int hupr_radar_scene_f32(const double* pos, const double* vel, const float* amp, const double* tx_host, const double* rx_host, int frames,
                         int S, double wavelength, double range_bin_m, double chirp_period_s, const float* add_or_null, float* out,
                         hupr_stream_t stream);

/* ---- bf16-activation variants ("bf16act") -------------------------------------------------------------
 * Same operators with the ACTIVATION tensors (x, y, dy, dx, residual) stored as bf16 in HBM; parameters,
 * statistics, weight gradients and all arithmetic stay fp32 (fp32 accumulate on the matrix pipe).  The
 * 3-D encoders (models/layers.py:160-191) run on them in bf16 mode: the layer-1 convolution sits at the
 * HBM/MFMA ridge with fp32 tensors (453 flop/B vs 312), bf16 storage doubles its intensity and halves every
 * BatchNorm / resampling pass.  Leading dimensions are in elements; bf16 conv inputs need in_ld % 8 == 0. */
int hupr_conv3x3_halo_bf16act(const void* x, const void* wp_bf16, const float* bias, const void* res, void* y,
                              int Bn, int D, int H, int W, int Ci, int in_ld, int Co, int out_ld, int res_ld, int kd,
                              hupr_stream_t stream);
/* The same operator with a caller-supplied workspace.  Grids that would leave most of the chip idle (single-sample inference,
 * config C2 of BASELINE.json: a level-3 layer is 32 workgroups walking 36 weight stages each) split the reduction over
 * (channel chunk, kz plane) slices on blockIdx.y; every slice leaves fp32 partial sums [slice][voxel][Co] in ws and a second
 * launch sums them in slice order (+ bias, + residual) and rounds once.  hupr_conv3x3_halo_splitk_ws_bytes() returns 0 where
 * the one-launch form is used anyway (ws may then be null).  Same products as the plain form; the fp32 summation order differs. */
size_t hupr_conv3x3_halo_splitk_ws_bytes(int Bn, int D, int H, int W, int Ci, int Co, int kd);
int hupr_conv3x3_halo_bf16act_ws(const void* x, const void* wp_bf16, const float* bias, const void* res, void* y,
                                 int Bn, int D, int H, int W, int Ci, int in_ld, int Co, int out_ld, int res_ld, int kd,
                                 void* ws, size_t ws_bytes, hupr_stream_t stream);
/* First half only: the fp32 partial sums [slices][voxel][Co] stay in `part` (slices = hupr_conv3x3_halo_splitk_ws_bytes() /
 * (voxels * Co * 4), which must be > 0) for a consumer that sums them itself.  No bias, no residual. */
int hupr_conv3x3_halo_bf16act_partial(const void* x, const void* wp_bf16, int Bn, int D, int H, int W, int Ci, int in_ld,
                                      int Co, int kd, void* part, size_t part_bytes, hupr_stream_t stream);
/* Inference tails that sum K-sliced partials themselves, in slice order and rounded where the stored tensor would have been
 * (bit-identical to convolution -> reduce -> tail, one launch per convolution less).  x*: bf16 tensor (n* == 0) or n* fp32 slices
 * [n][M][C]; x2 may be null.  mode 0: y = relu?(bn1_eval(x1) [+ bn2_eval(x2)]) — the BasicBlock3D tails, reference
 * models/layers.py:55-70 in eval mode; mode 1: y = prelu(x1 [+ x2]) — the BasicBlock2D tails, :30-37. */
int hupr_infer_tail_bf16act(int mode, const void* x1, int n1, const float* gamma1, const float* beta1, const float* mean1,
                            const float* var1, float eps1, const void* x2, int n2, const float* gamma2, const float* beta2,
                            const float* mean2, const float* var2, float eps2, const float* alpha, int relu, void* y, long M,
                            int C, hupr_stream_t stream);
int hupr_conv3x3_wgrad_halo_bf16act(const void* x, const void* dy, float* dw, int Bn, int D, int H, int W, int Ci,
                                    int in_ld, int Co, int dy_ld, int kd, void* ws, size_t ws_bytes,
                                    hupr_stream_t stream);
/* The weight gradients of TWO convolutions of one input (main[0] and downsample[0] of a residual block, reference models/layers.py:55-65;
 * same weight shape, same dy stride) in one launch of the LDS-DMA kernel over 2 Co output channels and one reduction: the same partial
 * sums, element for element, as two hupr_conv3x3_wgrad_halo_bf16act calls.  Applies where ..._dual_supported returns 1 (bf16 storage,
 * Co % 64 == 0); ws: 2 x hupr_conv3x3_wgrad_halo_ws_bytes(Ci, Co, kd). */
int hupr_conv3x3_wgrad_halo_dual_supported(int Bn, int D, int H, int W, int Ci, int Co, int kd);
int hupr_conv3x3_wgrad_halo_bf16act_dual(const void* x, const void* dy_a, const void* dy_b, float* dw_a, float* dw_b, int Bn, int D, int H,
                                         int W, int Ci, int in_ld, int Co, int dy_ld, int kd, void* ws, size_t ws_bytes,
                                         hupr_stream_t stream);
int hupr_bn_train_stats_bf16act(const void* x, long M, int C, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                                float* save_invstd, float* scale, float* shift, void* ws, size_t ws_bytes,
                                hupr_stream_t stream);
int hupr_scale_shift_act_bf16act(const void* x1, const float* scale1, const float* shift1, const void* x2,
                                 const float* scale2, const float* shift2, void* y, long M, int C, int act,
                                 hupr_stream_t stream);
int hupr_bn_bwd_bf16act(const void* dy, const void* y_mask, const void* x, const float* save_mean,
                        const float* save_invstd, const float* gamma, void* dx, float* dgamma, float* dbeta, long M,
                        int C, int train, void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_bn_bwd2_bf16act(const void* dy, const void* y_mask, const void* x1, const float* mean1, const float* invstd1,
                         const float* gamma1, const void* x2, const float* mean2, const float* invstd2, const float* gamma2,
                         void* dx1, void* dx2, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, long M, int C,
                         int train, void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_bn_bwd_remask_bf16act(const void* dy, const float* fwd_scale, const float* fwd_shift, const void* x,
                               const float* save_mean, const float* save_invstd, const float* gamma, void* dx,
                               float* dgamma, float* dbeta, long M, int C, int train, void* ws, size_t ws_bytes,
                               hupr_stream_t stream);
int hupr_bn_bwd2_remask_bf16act(const void* dy, const void* x1, const float* fwd_scale1, const float* fwd_shift1,
                                const float* mean1, const float* invstd1, const float* gamma1, const void* x2,
                                const float* fwd_scale2, const float* fwd_shift2, const float* mean2, const float* invstd2,
                                const float* gamma2, void* dx1, void* dx2, float* dgamma1, float* dbeta1, float* dgamma2,
                                float* dbeta2, long M, int C, int train, void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_colsum_bf16act(const void* x, long M, int C, float* out, void* ws, size_t ws_bytes, hupr_stream_t stream);
int hupr_prelu_fwd_bf16act(const void* x, const float* alpha, void* y, long n, hupr_stream_t stream);
int hupr_prelu_bwd_bf16act(const void* dy, const void* x, const float* alpha, void* dx, float* dalpha, long n, void* ws,
                           size_t ws_bytes, hupr_stream_t stream);
/* The PReLU backward with the final sum of its slope gradient deferred (nn.PReLU under autograd, reference models/layers.py:21-37): dx now,
 * *n_partials partial sums left in the caller's `partials` buffer (>= hupr_prelu_ws_bytes()); hupr_sum_partials_multi finishes any number
 * of them in one launch per 16 — the twelve slope gradients of a step when their gradient bucket is complete.  Same sums. */
typedef struct hupr_sum_item { const void* partial; int n; float* out; } hupr_sum_item;
int hupr_prelu_bwd_partials_f32(const float* dy, const float* x, const float* alpha, float* dx, long n, void* partials,
                                size_t partials_bytes, int* n_partials, hupr_stream_t stream);
int hupr_prelu_bwd_partials_bf16act(const void* dy, const void* x, const float* alpha, void* dx, long n, void* partials,
                                    size_t partials_bytes, int* n_partials, hupr_stream_t stream);
int hupr_sum_partials_multi(const hupr_sum_item* items, int n_items, hupr_stream_t stream);
int hupr_mnet_fwd_bf16act(const float* x, const float* w, const float* bias, void* out, float* means_or_null, long n_bg,
                          int pixels, hupr_stream_t stream);
/* MNet front end from the fused loader's elevation-mean planes [n_bg][16][pixels] (hupr_fft_chain_loader_means_f32); also
 * leaves the pixel-major means [n_bg][pixels][16] hupr_mnet_bwd_* reads (means_or_null). */
int hupr_mnet_fwd_means_f32(const float* mean_planes, const float* w, const float* bias, float* out, float* means_or_null,
                            long n_bg, int pixels, hupr_stream_t stream);
int hupr_mnet_fwd_means_bf16act(const float* mean_planes, const float* w, const float* bias, void* out, float* means_or_null,
                                long n_bg, int pixels, hupr_stream_t stream);
int hupr_mnet_bwd_bf16act(const float* x_or_null, const float* means_or_null, const float* w, const float* bias,
                          const void* dy, float* dw, float* dbias, long n_bg, int pixels, void* ws, size_t ws_bytes,
                          hupr_stream_t stream);
int hupr_interp_linear_fwd_bf16act(const void* x, void* y, int Bn, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                   int C, int in_ld, int out_ld, hupr_stream_t stream);
int hupr_interp_linear_bwd_bf16act(const void* dy, void* dx, int Bn, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                   int C, int in_ld, int out_ld, hupr_stream_t stream);
/* the same with dx += ...: dx already holds another consumer's gradient of the tensor (Encoder3D's level maps feed both a temporal
 * merge and the next level's down-sampling, models/layers.py:212-217) — replaces autograd's separate accumulation kernel */
int hupr_interp_linear_bwd_acc_f32(const float* dy, float* dx, int Bn, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int C,
                                   int in_ld, int out_ld, hupr_stream_t stream);
int hupr_interp_linear_bwd_acc_bf16act(const void* dy, void* dx, int Bn, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                       int C, int in_ld, int out_ld, hupr_stream_t stream);
/* boundary casts of the bf16-activation region (n % 4 == 0) */
int hupr_cast_f32_to_bf16(const float* x, void* y, long n, hupr_stream_t stream);
int hupr_cast_bf16_to_f32(const void* x, float* y, long n, hupr_stream_t stream);

/* (a5) The four 1 x 1 projections of one map of an MSCSA level (models/layers.py:150-157: phi / theta, cross / self — bias-free
 *      nn.Conv2d(C, C, 1)) as ONE streaming product: Y (M, 4 C) bf16 = X (M, C) fp32 . Wc^T with Wc (4 C, C) fp32 the four weight
 *      matrices stacked in the order the caller reads their column blocks (functional.MSCSALevelFn: [phi_cross | theta_cross | phi_self |
 *      theta_self], query rows pre-scaled by log2 e for the QS attention kernels); M = B H W channels-last rows.  Same operand roundings
 *      as hupr_conv_fwd_bf16_mixed with a bf16 epilogue (which it replaces for C in {64, 128}: levels 1 and 2); HBM-bound. */
int hupr_mscsa_proj_supported(long M, int C);
int hupr_mscsa_proj_fwd_bf16(const float* X, const float* Wc, void* Y, long M, int C, hupr_stream_t stream);
/* its input gradient: dX (M, C) fp32 = dY (M, 4 C) fp32 . Wc (+ res (M, C) fp32 or null — the map's value gradient dV) */
int hupr_mscsa_proj_dgrad_supported(long M, int C);      /* C == 64 (level 1) */
int hupr_mscsa_proj_dgrad_f32(const float* dY, const float* Wc, const float* res, float* dX, long M, int C, hupr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (e) Data-parallel exchange over RCCL / xGMI.  Nothing in the reference to mirror: it trains on one
 *     device (tools/base.py:14 `self.device = 'cuda'`, tools/run.py:76-79 forward / backward / step with no
 *     collective); BASELINE.json's configs 4-5 add 8-GPU data parallelism, whose only exchange is the sum
 *     all-reduce of the flat gradient buckets between `loss.backward()` (run.py:78) and `optimizer.step()`
 *     (run.py:79), plus one parameter broadcast at start-up.
 *
 *     librccl.so.1 is bound at run time (hupr_comm_load: the copy already mapped into the process wins, so
 *     the library never brings a second RCCL next to PyTorch's); one communicator per process = per GPU.
 *     hupr_comm_unique_id() is called on rank 0 and the HUPR_COMM_ID_BYTES blob is handed to every rank
 *     out of band (the Python host uses the torch.distributed store); hupr_comm_init_rank() is collective
 *     and binds the communicator to the CURRENT HIP device.  The two data entry points are in place,
 *     stream-ordered and capturable in a hipGraph; they never synchronise the host.
 * ---------------------------------------------------------------------------------------- */
#define HUPR_COMM_ID_BYTES 128
#define HUPR_COMM_F32 0
#define HUPR_COMM_BF16 1
typedef void* hupr_comm_t; /* ncclComm_t */
int hupr_comm_load(const char* librccl_path_or_null);
int hupr_comm_unique_id(void* id_out /* HUPR_COMM_ID_BYTES */);
int hupr_comm_init_rank(hupr_comm_t* comm_out, const void* id, int n_ranks, int rank);
int hupr_comm_destroy(hupr_comm_t comm);
/* ncclCommCount / ncclCommUserRank of a live communicator (what the bench line reports as rccl_ranks). */
int hupr_comm_info(hupr_comm_t comm, int* n_ranks_out, int* rank_out);
/* bucket[i] <- sum over ranks of bucket[i]  (count elements of dtype HUPR_COMM_F32 / HUPR_COMM_BF16) */
int hupr_allreduce_bucket(hupr_comm_t comm, void* bucket, size_t count, int dtype, hupr_stream_t stream);
/* bucket <- rank `root`'s bucket (initial parameter synchronisation) */
int hupr_broadcast_bucket(hupr_comm_t comm, void* bucket, size_t count, int dtype, int root, hupr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HUPR_H */
