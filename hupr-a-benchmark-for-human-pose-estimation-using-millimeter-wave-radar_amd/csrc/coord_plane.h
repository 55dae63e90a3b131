// The plane pass shared by the integral coordinate loss (coord_loss.hip) and the bone-vector loss (bone_loss.hip): a joint's position
// in heat-map pixels and the three sums S = sum p, N_x = sum p (x - a_x), N_y = sum p (y - a_y) of one plane by one 256-thread
// workgroup.  One body, so both losses take the same arithmetic in the same order and their residuals N / (S + eps) are equal bit
// for bit on equal inputs.
#pragma once
#include "hupr_common.h"

namespace hupr {

// One axis of one joint in heat-map pixels; a NaN where the row is invalid.  snap: the pixel hupr_k_gaussian_targets centres its patch
// on, (int)(a + 0.5f) with the truncating cast, which is executed only where it is defined (decided in float arithmetic as in
// target_axis of targets.hip: a NaN fails both comparisons).  Valid iff finite and 0 <= a <= H - 1.
__device__ __forceinline__ float coord_axis(float joint, float stride, int snap, int H) {
    float a = joint / stride;
    if (snap) {
        const float t = a + 0.5f;
        if (!(t >= -2147483648.f && t < 2147483648.f)) return NAN;
        a = (float)(int)t;
    }
    return (a >= 0.f && a <= (float)(H - 1)) ? a : NAN;
}

// The sums of the H x H plane pp around (ax, ay), called by all 256 threads of a workgroup; S, Nx and Ny are written in thread 0
// alone.  A thread adds its cells' p, p (x - a_x) and p (y - a_y) in index order into three fp32 partials (H * H / 256 terms: 16 at
// H = 64, 64 at H = 128), then the wave butterfly (6 additions) and the four waves through LDS in wave order.  VEC: 16-byte loads of
// four columns of one row (H % 4 == 0 and an aligned base), otherwise one float per lane.  The first barrier also orders the
// previous call's reads of red[] before this call's writes.
template <bool VEC>
__device__ __forceinline__ void coord_plane_sums(const float* __restrict__ pp, float ax, float ay, int H, float (*red)[4], float& S,
                                                 float& Nx, float& Ny) {
    float s = 0.f, nx = 0.f, ny = 0.f;
    if (VEC) {
        const int w4 = H >> 2, n4 = H * w4;
        for (int g = threadIdx.x; g < n4; g += 256) {
            const float4 v = reinterpret_cast<const float4*>(pp)[g];
            const int y = g / w4, x = (g - y * w4) << 2;
            const float dy = (float)y - ay, dx = (float)x - ax;
            s += v.x;
            nx = fmaf(v.x, dx, nx);
            ny = fmaf(v.x, dy, ny);
            s += v.y;
            nx = fmaf(v.y, (float)(x + 1) - ax, nx);
            ny = fmaf(v.y, dy, ny);
            s += v.z;
            nx = fmaf(v.z, (float)(x + 2) - ax, nx);
            ny = fmaf(v.z, dy, ny);
            s += v.w;
            nx = fmaf(v.w, (float)(x + 3) - ax, nx);
            ny = fmaf(v.w, dy, ny);
        }
    } else {
        const int n = H * H;
        for (int i = threadIdx.x; i < n; i += 256) {
            const float v = pp[i];
            const int y = i / H, x = i - y * H;
            s += v;
            nx = fmaf(v, (float)x - ax, nx);
            ny = fmaf(v, (float)y - ay, ny);
        }
    }
    s = wave_sum(s);
    nx = wave_sum(nx);
    ny = wave_sum(ny);
    __syncthreads();        // the previous row's red[] has been read
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        red[0][wv] = s;
        red[1][wv] = nx;
        red[2][wv] = ny;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        S = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        Nx = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        Ny = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    }
}

static inline bool coord_aligned16(const void* a, const void* b) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

// the shape rule shared by the entries of both losses; the byte offset of the last cell must fit the kernels' 64-bit index arithmetic
static inline int coord_shape(const char* name, long B, int K, int H, float stride) {
    HUPR_REQUIRE(K >= 1 && K <= 64, "%s: bad shape (K %d must be in [1, 64])", name, K);
    HUPR_REQUIRE(H >= 1 && H <= 4096, "%s: bad shape (H %d must be in [1, 4096])", name, H);
    HUPR_REQUIRE(B >= 1, "%s: bad shape (B %ld must be >= 1)", name, B);
    HUPR_REQUIRE(B <= (INT64_MAX / 8) / K && B * K <= (INT64_MAX / 8) / ((long)H * H), "%s: bad shape (%ld x %d planes of %d x %d cells)",
                 name, B, K, H, H);
    HUPR_REQUIRE(stride > 0.f && stride < INFINITY, "%s: bad parameter (stride %g must be positive and finite)", name, stride);
    return HUPR_OK;
}

}  // namespace hupr
