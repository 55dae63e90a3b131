// Integral (soft-arg-max) coordinate loss on both heads of a step: an L1 on the offset of each heat-map's mass centroid from its joint
// (Sun et al., "Integral Human Pose Regression", ECCV 2018; Nibali et al., "Numerical Coordinate Regression with Convolutional Neural
// Networks", DSNT), written relative to the joint and damped by eps so that a nearly empty plane has a bounded gradient.  The rule is
// stated in full beside hupr_coord_loss_fwd_f32 in include/hupr.h.  No atomics, no workspace and no data-dependent summation order:
// every output is bit-identical from run to run, and equal planes with equal joints give equal bits.
#include "coord_plane.h"

namespace hupr {

// One 256-thread workgroup per plane (grid-stride over the 2 B K rows, head-major).  A thread adds its cells' p, p (x - a_x) and
// p (y - a_y) in index order into three fp32 partials (H * H / 256 terms: 16 at H = 64, 64 at H = 128), then the wave butterfly
// (6 additions) and the four waves through LDS in wave order (thread 0).  VEC: 16-byte loads of four columns of one row (H % 4 == 0
// and aligned bases), otherwise one float per lane.  An invalid row's plane is not read.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_coord_loss_plane(const float* __restrict__ p1, const float* __restrict__ p2,
                                                               const float* __restrict__ joints, const float* __restrict__ joint_w,
                                                               long planes /* B K */, int K, int H, float stride, int snap, float eps,
                                                               float* __restrict__ resid /* (2, B K, 2) */,
                                                               float* __restrict__ scale /* (2, B K) */) {
    __shared__ float red[3][4];
    const long HW = (long)H * H;
    for (long r = blockIdx.x; r < 2 * planes; r += gridDim.x) {
        const long q = r < planes ? r : r - planes;
        const float ax = coord_axis(joints[q * 2 + 0], stride, snap, H);
        const float ay = coord_axis(joints[q * 2 + 1], stride, snap, H);
        if (!(ax == ax && ay == ay)) {      // workgroup-uniform
            if (threadIdx.x == 0) {
                resid[r * 2 + 0] = 0.f;
                resid[r * 2 + 1] = 0.f;
                scale[r] = 0.f;
            }
            continue;
        }
        const float* __restrict__ pp = (r < planes ? p1 : p2) + q * HW;
        float S, Nx, Ny;
        coord_plane_sums<VEC>(pp, ax, ay, H, red, S, Nx, Ny);
        if (threadIdx.x == 0) {
            const float den = S + eps;
            resid[r * 2 + 0] = Nx / den;
            resid[r * 2 + 1] = Ny / den;
            scale[r] = (joint_w ? joint_w[q % K] : 1.f) / den;
        }
    }
}

// One workgroup of four waves.  Thread t adds the row losses l = w_j (|r_x| + |r_y|) of rows t, t + 256, ... of each head in fp64, then
// the wave butterfly and the four waves in wave order: the order of every sum depends on (B, K) alone.  An invalid row's residual
// is zero, so it adds exactly zero.  Thread 0 alone writes loss3 and moves the accumulator (plain adds, no atomics).
__global__ __launch_bounds__(256) void hupr_k_coord_loss_sum(const float* __restrict__ resid, const float* __restrict__ joint_w,
                                                             long planes /* B K */, int K, float a0, float a1,
                                                             float* __restrict__ loss3, double* __restrict__ acc) {
    __shared__ double red[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double s = 0.0;
        for (long i = threadIdx.x; i < planes; i += 256) {
            const long r = (long)h * planes + i;
            const float w = joint_w ? joint_w[i % K] : 1.f;
            s += (double)(w * (fabsf(resid[r * 2 + 0]) + fabsf(resid[r * 2 + 1])));
        }
        s = wave_sum_f64(s);
        if ((threadIdx.x & 63) == 0) red[h][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double den = 2.0 * (double)planes;
        const double c0 = (((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) / den;
        const double c1 = (((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]) / den;
        const float l0 = (float)c0, l1 = (float)c1;
        loss3[1] = l0;
        loss3[2] = l1;
        loss3[0] = __fadd_rn(__fmul_rn(a0, l0), __fmul_rn(a1, l1));
        if (acc) {
            acc[0] += c0;
            acc[1] += c1;
            acc[2] += 1.0;
        }
    }
}

// dp_h[b,j,y,x] = f (sgn(r_x) ((x - a_x) - r_x) + sgn(r_y) ((y - a_y) - r_y)), f = G_h scale[h,b,j] / (2 B K): a store-only kernel,
// blockIdx.y = head, one workgroup per plane (grid-stride).  A plane whose f is zero (invalid row, weight 0, head weight 0) is
// written as zeros; a NaN f is not zero and reaches every cell of its plane.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_coord_loss_bwd(const float* __restrict__ resid, const float* __restrict__ scale,
                                                             const float* __restrict__ joints, const float* __restrict__ g, float a0,
                                                             float a1, float inv2bk, float* __restrict__ dp1, float* __restrict__ dp2,
                                                             long planes /* B K */, int H, float stride, int snap) {
    const bool second = blockIdx.y != 0;
    float* __restrict__ dp = second ? dp2 : dp1;
    const float go = __fmul_rn(g[0], second ? a1 : a0);
    const long HW = (long)H * H;
    for (long q = blockIdx.x; q < planes; q += gridDim.x) {
        const long r = (second ? planes : 0) + q;
        const float f = (go * scale[r]) * inv2bk;
        const bool zero = f == 0.f;         // false for a NaN factor, which must reach the gradient guard
        float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, sx = 0.f, sy = 0.f;
        if (!zero) {
            ax = coord_axis(joints[q * 2 + 0], stride, snap, H);
            ay = coord_axis(joints[q * 2 + 1], stride, snap, H);
            rx = resid[r * 2 + 0];
            ry = resid[r * 2 + 1];
            sx = rx > 0.f ? f : (rx < 0.f ? -f : rx * f);       // sgn(0) = 0; a NaN residual stays a NaN
            sy = ry > 0.f ? f : (ry < 0.f ? -f : ry * f);
        }
        float* __restrict__ dq = dp + q * HW;
        if (VEC) {
            const int w4 = H >> 2, n4 = H * w4;
            for (int i = threadIdx.x; i < n4; i += 256) {
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!zero) {
                    const int y = i / w4, x = (i - y * w4) << 2;
                    const float ty = sy * (((float)y - ay) - ry);
                    o.x = fmaf(sx, ((float)x - ax) - rx, ty);
                    o.y = fmaf(sx, ((float)(x + 1) - ax) - rx, ty);
                    o.z = fmaf(sx, ((float)(x + 2) - ax) - rx, ty);
                    o.w = fmaf(sx, ((float)(x + 3) - ax) - rx, ty);
                }
                reinterpret_cast<float4*>(dq)[i] = o;
            }
        } else {
            const int n = H * H;
            for (int i = threadIdx.x; i < n; i += 256) {
                float o = 0.f;
                if (!zero) {
                    const int y = i / H, x = i - y * H;
                    o = fmaf(sx, ((float)x - ax) - rx, sy * (((float)y - ay) - ry));
                }
                dq[i] = o;
            }
        }
    }
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_coord_loss_fwd_f32(const float* p1, const float* p2, const float* joints_xy, long B, int K, int H, float stride,
                                       int snap, const float* joint_w_or_null, float eps, float a0, float a1, float* loss3, float* resid,
                                       float* scale, double* acc_or_null, hupr_stream_t stream) {
    HUPR_REQUIRE(p1 && p2 && joints_xy && loss3 && resid && scale, "hupr_coord_loss_fwd_f32: null pointer");
    if (int e = coord_shape("hupr_coord_loss_fwd_f32", B, K, H, stride)) return e;
    HUPR_REQUIRE(eps > 0.f && eps < INFINITY, "hupr_coord_loss_fwd_f32: bad parameter (eps %g must be positive and finite)", eps);
    hipStream_t s = as_stream(stream);
    const long planes = B * K;
    const dim3 grid((unsigned)min(2 * planes, 8192L));
    if (H % 4 == 0 && coord_aligned16(p1, p2)) {
        HUPR_LAUNCH(hupr_k_coord_loss_plane<true>, grid, dim3(256), 0, s, p1, p2, joints_xy, joint_w_or_null, planes, K, H, stride, snap, eps,
                    resid, scale);
    } else {
        HUPR_LAUNCH(hupr_k_coord_loss_plane<false>, grid, dim3(256), 0, s, p1, p2, joints_xy, joint_w_or_null, planes, K, H, stride, snap, eps,
                    resid, scale);
    }
    HUPR_LAUNCH_OK("hupr_k_coord_loss_plane");
    HUPR_LAUNCH(hupr_k_coord_loss_sum, dim3(1), dim3(256), 0, s, resid, joint_w_or_null, planes, K, a0, a1, loss3, acc_or_null);
    HUPR_LAUNCH_OK("hupr_k_coord_loss_sum");
    return HUPR_OK;
}

extern "C" int hupr_coord_loss_bwd_f32(const float* resid, const float* scale, const float* joints_xy, const float* grad_loss, long B,
                                       int K, int H, float stride, int snap, float a0, float a1, float* dp1, float* dp2,
                                       hupr_stream_t stream) {
    HUPR_REQUIRE(resid && scale && joints_xy && grad_loss && dp1 && dp2, "hupr_coord_loss_bwd_f32: null pointer");
    if (int e = coord_shape("hupr_coord_loss_bwd_f32", B, K, H, stride)) return e;
    const long planes = B * K;
    const float inv2bk = (float)(1.0 / (2.0 * (double)planes));
    const dim3 grid((unsigned)min(planes, 8192L), 2);
    if (H % 4 == 0 && coord_aligned16(dp1, dp2)) {
        HUPR_LAUNCH(hupr_k_coord_loss_bwd<true>, grid, dim3(256), 0, as_stream(stream), resid, scale, joints_xy, grad_loss, a0, a1, inv2bk,
                    dp1, dp2, planes, H, stride, snap);
    } else {
        HUPR_LAUNCH(hupr_k_coord_loss_bwd<false>, grid, dim3(256), 0, as_stream(stream), resid, scale, joints_xy, grad_loss, a0, a1, inv2bk,
                    dp1, dp2, planes, H, stride, snap);
    }
    HUPR_LAUNCH_OK("hupr_k_coord_loss_bwd");
    return HUPR_OK;
}
