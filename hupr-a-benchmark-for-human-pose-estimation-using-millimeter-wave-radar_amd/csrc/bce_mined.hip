// Heat-map BCE with online hard keypoint mining (the top-k joint selection of CPN's RefineNet, Chen et al., "Cascaded Pyramid Network
// for Multi-Person Pose Estimation", CVPR 2018, and of HRNet's JointsOHKMMSELoss) and per-joint loss weights (HRNet's target_weight),
// on both heads of a step.  The BCE term, its clamps and the backward's floor are those of hupr_k_bce_pair_fwd / _bwd in head.hip;
// what changes is the reduction: one mean per (head, sample, joint) plane, a device-side selection of the k largest weighted planes of
// each (head, sample), and a backward scaled per plane.  The rule is stated in full beside hupr_bce_mined_fwd_f32 in include/hupr.h.
// No atomics and no data-dependent summation order: every output is bit-identical from run to run.
#include "hupr_common.h"

namespace hupr {

// hupr_k_bce_fwd's term for every number; the clamps are comparisons, not fmaxf, so that a NaN cell stays a NaN (fmaxf would turn it
// into -100 and the plane would look finite to the selection and to the gradient guard)
__device__ __forceinline__ float bce_term(float pv, float tv) {
    const float a = logf(pv), b = logf(1.f - pv);
    const float l1 = a < -100.f ? -100.f : a, l0 = b < -100.f ? -100.f : b;
    return tv * l1 + (1.f - tv) * l0;
}

// One 256-thread workgroup per plane (grid-stride over the 2 B K planes, head-major): a thread sums its cells in index order, the
// wave butterfly and the four-wave sum are fixed, so equal planes give equal bits.  At HW = 4096 that is 16 + 6 fp32 additions deep
// and one rounding of the mean.  VEC: 16-byte loads (HW % 4 == 0 and aligned bases), otherwise one float per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_bce_mined_plane(const float* __restrict__ p1, const float* __restrict__ p2,
                                                              const float* __restrict__ t, long planes /* B K */, long HW,
                                                              float* __restrict__ plane_loss /* (2, B K) */) {
    __shared__ double red[4];
    for (long r = blockIdx.x; r < 2 * planes; r += gridDim.x) {
        const long q = r < planes ? r : r - planes;
        const float* __restrict__ pp = (r < planes ? p1 : p2) + q * HW;
        const float* __restrict__ tp = t + q * HW;
        float acc = 0.f;
        if (VEC) {
            const long n4 = HW >> 2;
            for (long g = threadIdx.x; g < n4; g += 256) {
                const float4 a = reinterpret_cast<const float4*>(pp)[g], b = reinterpret_cast<const float4*>(tp)[g];
                acc -= bce_term(a.x, b.x);
                acc -= bce_term(a.y, b.y);
                acc -= bce_term(a.z, b.z);
                acc -= bce_term(a.w, b.w);
            }
        } else {
            for (long i = threadIdx.x; i < HW; i += 256) acc -= bce_term(pp[i], tp[i]);
        }
        acc = wave_sum(acc);
        __syncthreads();        // the previous plane's red[] has been read
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)acc;
        __syncthreads();
        if (threadIdx.x == 0) plane_loss[r] = (float)((red[0] + red[1] + red[2] + red[3]) / (double)HW);
    }
}

// a ranks before b in the selection order: v descending, a NaN above every number, equal values and two NaNs by lower joint index
__device__ __forceinline__ bool mined_before(float va, int ia, float vb, int ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na && (!nb || ia < ib);
    return va > vb || (va == vb && ia < ib);
}

// One workgroup of four waves.  A wave ranks the K planes of one (head, sample) at a time, lane j holding joint j, and keeps lane j's
// selected sum (fp64) and count over the samples it visits (b = wave, wave + 4, ...); the four waves' partials are then added in
// wave order, the K lanes by the fixed butterfly: the order of every sum depends on the shape alone.
__global__ __launch_bounds__(256) void hupr_k_bce_mined_select(const float* __restrict__ plane_loss, const float* __restrict__ joint_w,
                                                               long B, int K, int k, double inv_bk, double inv_bkhw, float alpha,
                                                               float beta, float* __restrict__ loss3, float* __restrict__ coef,
                                                               long long* __restrict__ counts) {
    __shared__ double ssum[2][4][64];
    __shared__ int scnt[2][4][64];
    __shared__ float l[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool live = lane < K;
    const float w = live ? (joint_w ? joint_w[lane] : 1.f) : 0.f;
    const float cf = (float)((double)w * inv_bkhw);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double sum = 0.0;
        int cnt = 0;
        for (long b = wave; b < B; b += 4) {
            const long row = ((long)h * B + b) * K;
            // only lanes 0 .. K-1 are compared; what the others hold is never read
            const float v = live ? w * plane_loss[row + lane] : -INFINITY;
            int rank = 0;
            for (int i = 0; i < K; ++i) rank += mined_before(__shfl(v, i, 64), i, v, lane) ? 1 : 0;
            const bool sel = live && rank < k;
            if (live) coef[row + lane] = sel ? cf : 0.f;
            if (sel) {
                sum += (double)v;
                ++cnt;
            }
        }
        ssum[h][wave][lane] = sum;
        scnt[h][wave][lane] = cnt;
    }
    __syncthreads();
    if (wave < 2) {
        double s = ((ssum[wave][0][lane] + ssum[wave][1][lane]) + ssum[wave][2][lane]) + ssum[wave][3][lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) l[wave] = (float)(s * inv_bk);
        if (counts && live)
            counts[wave * K + lane] += (long long)scnt[wave][0][lane] + scnt[wave][1][lane] + scnt[wave][2][lane] + scnt[wave][3][lane];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        loss3[1] = l[0];
        loss3[2] = l[1];
        loss3[0] = __fadd_rn(__fmul_rn(alpha, l[0]), __fmul_rn(beta, l[1]));
    }
}

// dp_h = G_h coef[h, plane] (p - t) / max(p (1 - p), 1e-12): hupr_k_bce_pair_bwd with a per-plane scale.  blockIdx.y = head, one
// workgroup per plane (grid-stride); a plane whose scale is zero (not selected, or weight 0) is written as zeros without being read.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_bce_mined_bwd(const float* __restrict__ p1, const float* __restrict__ p2,
                                                            const float* __restrict__ t, const float* __restrict__ coef,
                                                            const float* __restrict__ g, const float* __restrict__ g2, float alpha,
                                                            float beta, float* __restrict__ dp1, float* __restrict__ dp2,
                                                            long planes /* B K */, long HW) {
    const bool second = blockIdx.y != 0;
    const float* __restrict__ p = second ? p2 : p1;
    float* __restrict__ dp = second ? dp2 : dp1;
    float go = __fmul_rn(g[0], second ? beta : alpha);
    if (second && g2) go = __fadd_rn(go, g2[0]);
    for (long r = blockIdx.x; r < planes; r += gridDim.x) {
        const float gs = go * coef[(second ? planes : 0) + r];
        const bool zero = gs == 0.f;        // false for a NaN scale, which must reach the gradient guard
        const float* __restrict__ pp = p + r * HW;
        const float* __restrict__ tp = t + r * HW;
        float* __restrict__ dq = dp + r * HW;
        if (VEC) {
            const long n4 = HW >> 2;
            for (long i = threadIdx.x; i < n4; i += 256) {
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!zero) {
                    const float4 a = reinterpret_cast<const float4*>(pp)[i], b = reinterpret_cast<const float4*>(tp)[i];
                    o.x = gs * (a.x - b.x) / fmaxf(a.x * (1.f - a.x), 1e-12f);
                    o.y = gs * (a.y - b.y) / fmaxf(a.y * (1.f - a.y), 1e-12f);
                    o.z = gs * (a.z - b.z) / fmaxf(a.z * (1.f - a.z), 1e-12f);
                    o.w = gs * (a.w - b.w) / fmaxf(a.w * (1.f - a.w), 1e-12f);
                }
                reinterpret_cast<float4*>(dq)[i] = o;
            }
        } else {
            for (long i = threadIdx.x; i < HW; i += 256) {
                float o = 0.f;
                if (!zero) {
                    const float pv = pp[i];
                    o = gs * (pv - tp[i]) / fmaxf(pv * (1.f - pv), 1e-12f);
                }
                dq[i] = o;
            }
        }
    }
}

static inline bool aligned16(const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

}  // namespace hupr

using namespace hupr;

// the shape rule shared by both entries; the byte offset of the last cell must fit the kernels' 64-bit index arithmetic
static int mined_shape(const char* name, long B, int K, long HW) {
    HUPR_REQUIRE(K >= 1 && K <= 64, "%s: bad shape (K %d must be in [1, 64])", name, K);
    HUPR_REQUIRE(B >= 1 && HW >= 1, "%s: bad shape (B %ld and HW %ld must be >= 1)", name, B, HW);
    HUPR_REQUIRE(B <= (INT64_MAX / 8) / K && B * K <= (INT64_MAX / 8) / HW, "%s: bad shape (%ld x %d planes of %ld cells)", name, B, K, HW);
    return HUPR_OK;
}

extern "C" int hupr_bce_mined_fwd_f32(const float* p1, const float* p2, const float* t, long B, int K, long HW, int k,
                                      const float* joint_w_or_null, float alpha, float beta, float* loss3, float* plane_loss,
                                      float* coef, long long* counts_or_null, hupr_stream_t stream) {
    HUPR_REQUIRE(p1 && p2 && t && loss3 && plane_loss && coef, "hupr_bce_mined_fwd_f32: null pointer");
    if (int e = mined_shape("hupr_bce_mined_fwd_f32", B, K, HW)) return e;
    HUPR_REQUIRE(k >= 1 && k <= K, "hupr_bce_mined_fwd_f32: bad selection (k %d must be in [1, K = %d])", k, K);
    hipStream_t s = as_stream(stream);
    const long planes = B * K;
    const dim3 grid((unsigned)min(2 * planes, 8192L));
    if (HW % 4 == 0 && aligned16(p1, p2, t)) {
        HUPR_LAUNCH(hupr_k_bce_mined_plane<true>, grid, dim3(256), 0, s, p1, p2, t, planes, HW, plane_loss);
    } else {
        HUPR_LAUNCH(hupr_k_bce_mined_plane<false>, grid, dim3(256), 0, s, p1, p2, t, planes, HW, plane_loss);
    }
    HUPR_LAUNCH_OK("hupr_k_bce_mined_plane");
    const double bk = (double)B * (double)k;
    HUPR_LAUNCH(hupr_k_bce_mined_select, dim3(1), dim3(256), 0, s, plane_loss, joint_w_or_null, B, K, k, 1.0 / bk, 1.0 / (bk * (double)HW),
                alpha, beta, loss3, coef, counts_or_null);
    HUPR_LAUNCH_OK("hupr_k_bce_mined_select");
    return HUPR_OK;
}

extern "C" int hupr_bce_mined_bwd_f32(const float* p1, const float* p2, const float* t, const float* coef, const float* grad_loss,
                                      const float* grad_loss2_or_null, float alpha, float beta, float* dp1, float* dp2, long B, int K,
                                      long HW, hupr_stream_t stream) {
    HUPR_REQUIRE(p1 && p2 && t && coef && grad_loss && dp1 && dp2, "hupr_bce_mined_bwd_f32: null pointer");
    if (int e = mined_shape("hupr_bce_mined_bwd_f32", B, K, HW)) return e;
    const long planes = B * K;
    const dim3 grid((unsigned)min(planes, 8192L), 2);
    if (HW % 4 == 0 && aligned16(p1, p2, t) && aligned16(dp1, dp2, t)) {
        HUPR_LAUNCH(hupr_k_bce_mined_bwd<true>, grid, dim3(256), 0, as_stream(stream), p1, p2, t, coef, grad_loss, grad_loss2_or_null,
                    alpha, beta, dp1, dp2, planes, HW);
    } else {
        HUPR_LAUNCH(hupr_k_bce_mined_bwd<false>, grid, dim3(256), 0, as_stream(stream), p1, p2, t, coef, grad_loss, grad_loss2_or_null,
                    alpha, beta, dp1, dp2, planes, HW);
    }
    HUPR_LAUNCH_OK("hupr_k_bce_mined_bwd");
    return HUPR_OK;
}
