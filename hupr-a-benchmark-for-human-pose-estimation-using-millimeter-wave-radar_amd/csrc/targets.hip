// Sub-pixel Gaussian training targets: the encoding half of distribution-aware coordinate representation (Zhang et al.,
// "Distribution-Aware Coordinate Representation for Human Pose Estimation", CVPR 2020).  The window and its in-bounds rule are the
// reference's (misc/utils.py:6-66, as hupr_k_gaussian_targets in head.hip pastes it); the Gaussian inside the window is centred on
// the joint's real position instead of the window's middle pixel, so that hupr_pose_decode_f32 (pose_decode.hip) inverts it.
// The rule is stated in full beside hupr_gaussian_targets_subpixel_f32 in include/hupr.h.
#include "hupr_common.h"

namespace hupr {

// One axis of one joint: the clipped window [lo, hi] of map pixels (empty as lo > hi), its middle pixel mu and the fraction f.
struct TargetAxis {
    int lo, hi, mu;
    float f;
};

__device__ __forceinline__ TargetAxis target_axis(float joint, float stride, int rad, int H) {
    const float ac = joint / stride;
    const float t = ac + 0.5f;
    TargetAxis a = {1, 0, 0, 0.f};
    // decided in float arithmetic: the cast below is executed only where it is defined (a NaN fails both comparisons)
    if (t >= -2147483648.f && t < 2147483648.f) {
        a.mu = (int)t;
        a.f = ac - (float)a.mu;
        // mu - rad >= H or mu + rad + 1 < 0 (the reference's test) leave an empty clipped window; 64-bit: rad is any positive int
        const long long lo = (long long)a.mu - rad, hi = (long long)a.mu + rad;
        a.lo = (int)max(lo, 0LL);
        a.hi = (int)max(min(hi, (long long)H - 1), -1LL);
    }
    return a;
}

__device__ __forceinline__ float target_cell(const TargetAxis& ax, const TargetAxis& ay, int x, int y, bool row_in, float two_s2) {
    if (!row_in || x < ax.lo || x > ax.hi) return 0.f;
    const float ddx = (float)(x - ax.mu) - ax.f, ddy = (float)(y - ay.mu) - ay.f;
    return expf(-(ddx * ddx + ddy * ddy) / two_s2);
}

// One workgroup per (sample, joint) plane (grid-stride over the planes), so the joint, its windows and fractions are wave-uniform.
// Every element of the plane is stored exactly once: VEC = 16-byte stores of four columns of one row (H % 4 == 0 and an aligned t),
// otherwise one float per lane.  expf runs only for cells inside the window.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_gaussian_targets_subpixel(const float* __restrict__ joints, float* __restrict__ t,
                                                                        long BK, int H, float two_s2, int rad, float stride) {
    for (long r = blockIdx.x; r < BK; r += gridDim.x) {
        const TargetAxis ax = target_axis(joints[r * 2 + 0], stride, rad, H);
        const TargetAxis ay = target_axis(joints[r * 2 + 1], stride, rad, H);
        float* plane = t + r * ((long)H * H);
        if (VEC) {
            const int q = H >> 2, n4 = H * q;
            for (int g = threadIdx.x; g < n4; g += 256) {
                const int y = g / q, x = (g - y * q) << 2;
                const bool row_in = y >= ay.lo && y <= ay.hi;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row_in && x + 3 >= ax.lo && x <= ax.hi) {
                    v.x = target_cell(ax, ay, x, y, true, two_s2);
                    v.y = target_cell(ax, ay, x + 1, y, true, two_s2);
                    v.z = target_cell(ax, ay, x + 2, y, true, two_s2);
                    v.w = target_cell(ax, ay, x + 3, y, true, two_s2);
                }
                reinterpret_cast<float4*>(plane)[g] = v;
            }
        } else {
            const int n = H * H;
            for (int i = threadIdx.x; i < n; i += 256) {
                const int y = i / H, x = i - y * H;
                plane[i] = target_cell(ax, ay, x, y, y >= ay.lo && y <= ay.hi, two_s2);
            }
        }
    }
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_gaussian_targets_subpixel_f32(const float* joints_xy, float* t, long BK, int H, float sigma, int rad, float stride,
                                                  hupr_stream_t stream) {
    if (BK == 0) return HUPR_OK;
    HUPR_REQUIRE(joints_xy && t, "hupr_gaussian_targets_subpixel_f32: null pointer");
    HUPR_REQUIRE(H >= 1 && H <= 4096, "hupr_gaussian_targets_subpixel_f32: bad shape (H %d must be in [1, 4096])", H);
    // the byte offset of the last plane must fit the kernel's 64-bit index arithmetic
    HUPR_REQUIRE(BK > 0 && BK <= (INT64_MAX / 4) / ((long)H * H),
                 "hupr_gaussian_targets_subpixel_f32: bad shape (BK %ld planes of %d x %d)", BK, H, H);
    HUPR_REQUIRE(rad >= 1, "hupr_gaussian_targets_subpixel_f32: bad window (rad %d must be >= 1)", rad);
    HUPR_REQUIRE(sigma > 0.f && sigma < INFINITY && stride > 0.f && stride < INFINITY,
                 "hupr_gaussian_targets_subpixel_f32: bad parameter (sigma %g and stride %g must be positive and finite)", sigma, stride);
    const float two_s2 = 2.f * sigma * sigma;
    HUPR_REQUIRE(two_s2 > 0.f && two_s2 < INFINITY, "hupr_gaussian_targets_subpixel_f32: bad parameter (2 sigma^2 = %g for sigma %g)",
                 two_s2, sigma);
    const dim3 grid((unsigned)min(BK, 8192L));
    if (H % 4 == 0 && (reinterpret_cast<uintptr_t>(t) & 15) == 0) {
        HUPR_LAUNCH(hupr_k_gaussian_targets_subpixel<true>, grid, dim3(256), 0, as_stream(stream), joints_xy, t, BK, H, two_s2, rad, stride);
    } else {
        HUPR_LAUNCH(hupr_k_gaussian_targets_subpixel<false>, grid, dim3(256), 0, as_stream(stream), joints_xy, t, BK, H, two_s2, rad, stride);
    }
    HUPR_LAUNCH_OK("hupr_k_gaussian_targets_subpixel");
    return HUPR_OK;
}
