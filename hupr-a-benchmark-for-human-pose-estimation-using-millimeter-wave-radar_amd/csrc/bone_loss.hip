// Bone-vector loss on both heads of a step (Sun et al., "Compositional Human Pose Regression", ICCV 2017): an L1 on the error of the
// vector between the mass centroids of the two heat-maps at the ends of every bone of a skeleton table, in heat-map pixels.  A
// centroid is taken relative to its joint with the plane pass of the integral coordinate loss (coord_plane.h), so the bone's
// error is the difference of two of that loss's residuals and a pose displaced as a whole costs nothing.  The rule is stated in full
// beside hupr_bone_loss_fwd_f32 in include/hupr.h.  No atomics, no workspace and no data-dependent summation order: every output is
// bit-identical from run to run, and equal planes with equal joints give equal bits.
#include "coord_plane.h"

namespace hupr {

// the skeleton, copied into the kernel's arguments: bone e joins joint uv[2 e] to joint uv[2 e + 1]
struct BoneTable {
    int E;
    int uv[64];
};

// One 256-thread workgroup per plane (grid-stride over the 2 B K rows, head-major): the coordinate loss's residual r = N / (S + eps)
// and 1 / (S + eps).  An invalid row is a zero row and its plane is not read.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_bone_loss_plane(const float* __restrict__ p1, const float* __restrict__ p2,
                                                              const float* __restrict__ joints, long planes /* B K */, int H, float stride,
                                                              int snap, float eps, float* __restrict__ resid /* (2, B K, 2) */,
                                                              float* __restrict__ inv_den /* (2, B K) */) {
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
                inv_den[r] = 0.f;
            }
            continue;
        }
        float S, Nx, Ny;
        coord_plane_sums<VEC>((r < planes ? p1 : p2) + q * HW, ax, ay, H, red, S, Nx, Ny);
        if (threadIdx.x == 0) {
            const float den = S + eps;
            resid[r * 2 + 0] = Nx / den;
            resid[r * 2 + 1] = Ny / den;
            inv_den[r] = 1.f / den;
        }
    }
}

__device__ __forceinline__ bool bone_joint_valid(const float* __restrict__ joints, long q, float stride, int snap, int H) {
    const float ax = coord_axis(joints[q * 2 + 0], stride, snap, H);
    const float ay = coord_axis(joints[q * 2 + 1], stride, snap, H);
    return ax == ax && ay == ay;
}

// sgn(0) = 0; a NaN stays a NaN
__device__ __forceinline__ float bone_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : d); }

// One workgroup of four waves, three passes over resid.  (1) bone_resid: thread t takes bones t, t + 256, ... of the 2 B E.
// (2) gcoef: thread t takes joints t, t + 256, ... of the 2 B K, walks the table in bone-index order and recomputes the d of its
// incident bones from resid: the same two subtractions, so the same bits as pass 1 without a hand-off between threads.  (3) the
// loss: thread t adds w_e (|d_x| + |d_y|) of bones t, t + 256, ... of each head in fp64, then the wave butterfly and the four waves
// in wave order: the order of every sum depends on (B, E) alone.  Thread 0 alone writes loss3 and moves the accumulator.
__global__ __launch_bounds__(256) void hupr_k_bone_loss_sum(const float* __restrict__ resid, const float* __restrict__ joints,
                                                            const float* __restrict__ bone_w, BoneTable bt, long B, int K, int H,
                                                            float stride, int snap, float a0, float a1, float* __restrict__ bone_resid,
                                                            float* __restrict__ gcoef, float* __restrict__ loss3,
                                                            double* __restrict__ acc) {
    __shared__ double red[2][4];
    const int E = bt.E;
    const long bones = B * E, planes = B * K;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double s = 0.0;
        for (long i = threadIdx.x; i < bones; i += 256) {
            const long b = i / E;
            const int e = (int)(i - b * E);
            const int u = bt.uv[2 * e], v = bt.uv[2 * e + 1];
            float dx = 0.f, dy = 0.f;
            if (bone_joint_valid(joints, b * K + u, stride, snap, H) && bone_joint_valid(joints, b * K + v, stride, snap, H)) {
                const long ru = (long)h * planes + b * K + u, rv = (long)h * planes + b * K + v;
                dx = resid[rv * 2 + 0] - resid[ru * 2 + 0];
                dy = resid[rv * 2 + 1] - resid[ru * 2 + 1];
            }
            const long o = (long)h * bones + i;
            bone_resid[o * 2 + 0] = dx;
            bone_resid[o * 2 + 1] = dy;
            const float w = bone_w ? bone_w[e] : 1.f;
            s += (double)(w * (fabsf(dx) + fabsf(dy)));
        }
        s = wave_sum_f64(s);
        if ((threadIdx.x & 63) == 0) red[h][threadIdx.x >> 6] = s;
    }
    for (long i = threadIdx.x; i < 2 * planes; i += 256) {
        const long q = i < planes ? i : i - planes;
        const long b = q / K;
        const int j = (int)(q - b * K);
        const long row0 = i - j;            // row of joint 0 of this head and sample
        float gx = 0.f, gy = 0.f;
        if (bone_joint_valid(joints, q, stride, snap, H)) {
            for (int e = 0; e < E; ++e) {
                const int u = bt.uv[2 * e], v = bt.uv[2 * e + 1];
                if (u != j && v != j) continue;
                if (!bone_joint_valid(joints, b * K + (u == j ? v : u), stride, snap, H)) continue;
                const float w = bone_w ? bone_w[e] : 1.f;
                const float dx = resid[(row0 + v) * 2 + 0] - resid[(row0 + u) * 2 + 0];
                const float dy = resid[(row0 + v) * 2 + 1] - resid[(row0 + u) * 2 + 1];
                const float sx = w * bone_sign(dx), sy = w * bone_sign(dy);
                gx = v == j ? gx + sx : gx - sx;
                gy = v == j ? gy + sy : gy - sy;
            }
        }
        gcoef[i * 2 + 0] = gx;
        gcoef[i * 2 + 1] = gy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double den = 2.0 * (double)bones;
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

// dp_h[b,j,y,x] = f (gcoef_x ((x - a_x) - r_x) + gcoef_y ((y - a_y) - r_y)), f = (g a_h) inv_den[h,b,j] / (2 B E): a store-only
// kernel, blockIdx.y = head, one workgroup per plane (grid-stride).  A plane whose f is zero (invalid row, head weight 0) or whose two
// coefficients are both zero is written as zeros; a NaN f or coefficient is not zero and reaches every cell of its plane.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_bone_loss_bwd(const float* __restrict__ resid, const float* __restrict__ inv_den,
                                                            const float* __restrict__ gcoef, const float* __restrict__ joints,
                                                            const float* __restrict__ g, float a0, float a1, float inv2be,
                                                            float* __restrict__ dp1, float* __restrict__ dp2, long planes /* B K */,
                                                            int H, float stride, int snap) {
    const bool second = blockIdx.y != 0;
    float* __restrict__ dp = second ? dp2 : dp1;
    const float go = __fmul_rn(g[0], second ? a1 : a0);
    const long HW = (long)H * H;
    for (long q = blockIdx.x; q < planes; q += gridDim.x) {
        const long r = (second ? planes : 0) + q;
        const float f = (go * inv_den[r]) * inv2be;
        const float gx = gcoef[r * 2 + 0], gy = gcoef[r * 2 + 1];
        const bool zero = f == 0.f || (gx == 0.f && gy == 0.f);     // false for a NaN, which must reach the gradient guard
        float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, sx = 0.f, sy = 0.f;
        if (!zero) {
            ax = coord_axis(joints[q * 2 + 0], stride, snap, H);
            ay = coord_axis(joints[q * 2 + 1], stride, snap, H);
            rx = resid[r * 2 + 0];
            ry = resid[r * 2 + 1];
            sx = gx * f;
            sy = gy * f;
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

static int bone_count(const char* name, int E) {
    HUPR_REQUIRE(E >= 1 && E <= 32, "%s: bad bone table (E %d must be in [1, 32])", name, E);
    return HUPR_OK;
}

extern "C" int hupr_bone_loss_fwd_f32(const float* p1, const float* p2, const float* joints_xy, long B, int K, int H, float stride,
                                      int snap, const int* bones_host, int E, const float* bone_w_or_null, float eps, float a0, float a1,
                                      float* loss3, float* resid, float* inv_den, float* bone_resid, float* gcoef, double* acc_or_null,
                                      hupr_stream_t stream) {
    HUPR_REQUIRE(p1 && p2 && joints_xy && bones_host && loss3 && resid && inv_den && bone_resid && gcoef,
                 "hupr_bone_loss_fwd_f32: null pointer");
    if (int e = coord_shape("hupr_bone_loss_fwd_f32", B, K, H, stride)) return e;
    if (int e = bone_count("hupr_bone_loss_fwd_f32", E)) return e;
    HUPR_REQUIRE(eps > 0.f && eps < INFINITY, "hupr_bone_loss_fwd_f32: bad parameter (eps %g must be positive and finite)", eps);
    BoneTable bt;
    bt.E = E;
    for (int e = 0; e < 32; ++e) {
        const int u = e < E ? bones_host[2 * e] : 0, v = e < E ? bones_host[2 * e + 1] : 0;
        HUPR_REQUIRE(e >= E || (u >= 0 && u < K && v >= 0 && v < K && u != v),
                     "hupr_bone_loss_fwd_f32: bad bone table (bone %d = (%d, %d); two different joints of [0, %d))", e, u, v, K);
        bt.uv[2 * e] = u;
        bt.uv[2 * e + 1] = v;
    }
    hipStream_t s = as_stream(stream);
    const long planes = B * K;
    const dim3 grid((unsigned)min(2 * planes, 8192L));
    if (H % 4 == 0 && coord_aligned16(p1, p2)) {
        HUPR_LAUNCH(hupr_k_bone_loss_plane<true>, grid, dim3(256), 0, s, p1, p2, joints_xy, planes, H, stride, snap, eps, resid, inv_den);
    } else {
        HUPR_LAUNCH(hupr_k_bone_loss_plane<false>, grid, dim3(256), 0, s, p1, p2, joints_xy, planes, H, stride, snap, eps, resid, inv_den);
    }
    HUPR_LAUNCH_OK("hupr_k_bone_loss_plane");
    HUPR_LAUNCH(hupr_k_bone_loss_sum, dim3(1), dim3(256), 0, s, resid, joints_xy, bone_w_or_null, bt, B, K, H, stride, snap, a0, a1,
                bone_resid, gcoef, loss3, acc_or_null);
    HUPR_LAUNCH_OK("hupr_k_bone_loss_sum");
    return HUPR_OK;
}

extern "C" int hupr_bone_loss_bwd_f32(const float* resid, const float* inv_den, const float* gcoef, const float* joints_xy,
                                      const float* grad_loss, long B, int K, int E, int H, float stride, int snap, float a0, float a1,
                                      float* dp1, float* dp2, hupr_stream_t stream) {
    HUPR_REQUIRE(resid && inv_den && gcoef && joints_xy && grad_loss && dp1 && dp2, "hupr_bone_loss_bwd_f32: null pointer");
    if (int e = coord_shape("hupr_bone_loss_bwd_f32", B, K, H, stride)) return e;
    if (int e = bone_count("hupr_bone_loss_bwd_f32", E)) return e;
    const long planes = B * K;
    const float inv2be = (float)(1.0 / (2.0 * (double)B * (double)E));
    const dim3 grid((unsigned)min(planes, 8192L), 2);
    if (H % 4 == 0 && coord_aligned16(dp1, dp2)) {
        HUPR_LAUNCH(hupr_k_bone_loss_bwd<true>, grid, dim3(256), 0, as_stream(stream), resid, inv_den, gcoef, joints_xy, grad_loss, a0, a1,
                    inv2be, dp1, dp2, planes, H, stride, snap);
    } else {
        HUPR_LAUNCH(hupr_k_bone_loss_bwd<false>, grid, dim3(256), 0, as_stream(stream), resid, inv_den, gcoef, joints_xy, grad_loss, a0, a1,
                    inv2be, dp1, dp2, planes, H, stride, snap);
    }
    HUPR_LAUNCH_OK("hupr_k_bone_loss_bwd");
    return HUPR_OK;
}
