// Sub-pixel refinement of a heat-map peak, shared by hupr_k_pose_decode (pose_decode.hip) and hupr_k_pose_track (pose_track.hip) so
// that the two decode to the same bits, and the tail of those two and of hupr_k_pose_decode_integral (pose_integral.hip): the keypoint
// with its stores, and the entries' shape rule.  The rule is stated beside hupr_pose_decode_f32 in include/hupr.h.
#pragma once
#include "hupr_common.h"

namespace hupr {

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN too
__device__ __forceinline__ float signf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Offset (ox, oy) in heat-map pixels from the arg-max pixel (px, py) of ``row`` (H x W) to the refined peak: a second-order Taylor
// step on the log heat-map, the quarter-pixel rule where the Hessian is not negative definite, (0, 0) without refinement, for a
// non-positive maximum and on the map border.  Called by the whole wave; every lane ends with the same offset.
__device__ __forceinline__ void peak_offset(const float* row, int H, int W, int px, int py, bool positive, int refine, int lane,
                                            float& ox, float& oy) {
    const bool interior = px > 0 && px < W - 1 && py > 0 && py < H - 1;
    ox = 0.f;
    oy = 0.f;
    if (refine && positive && interior) {
        // lane k < 9 holds neighbour (px + k % 3 - 1, py + k / 3 - 1); a NaN neighbour stays NaN through the log
        float h = 1.f;
        if (lane < 9) h = row[(long)(py + lane / 3 - 1) * W + (px + lane % 3 - 1)];
        const float lg = (h != h) ? h : logf(fmaxf(h, 1e-10f));
        float l[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) l[k] = __shfl(lg, k, 64);
        const float hxm = __shfl(h, 3, 64), hxp = __shfl(h, 5, 64), hym = __shfl(h, 1, 64), hyp = __shfl(h, 7, 64);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) ok = ok && finitef(l[k]);
        if (ok) {
            const float dx = 0.5f * (l[5] - l[3]), dy = 0.5f * (l[7] - l[1]);
            const float dxx = l[5] - 2.f * l[4] + l[3], dyy = l[7] - 2.f * l[4] + l[1];
            const float dxy = 0.25f * (l[8] - l[6] - l[2] + l[0]);
            const float det = dxx * dyy - dxy * dxy;
            float tx, ty;
            if (dxx < 0.f && det > 0.f) {
                tx = -(dyy * dx - dxy * dy) / det;
                ty = -(dxx * dy - dxy * dx) / det;
            } else {
                tx = 0.25f * signf(hxp - hxm);
                ty = 0.25f * signf(hyp - hym);
            }
            if (finitef(tx) && finitef(ty)) {
                ox = fminf(fmaxf(tx, -0.5f), 0.5f);
                oy = fminf(fmaxf(ty, -0.5f), 0.5f);
            }
        }
    }
}

// The decoded keypoint of row r, called by lane 0: stores index, maximum and the image-pixel (x, y) and returns (x, y).  A joint whose
// maximum is <= 0 decodes to (0, 0) (misc/metrics.py); with a zero offset these are the floats of hupr_k_stream_keypoints.
__device__ __forceinline__ float2 store_keypoint(long r, int bi, float best, int px, int py, float ox, float oy, bool positive,
                                                 float ratio, int* idx, float* maxval, float* raw) {
    const float keep = positive ? 1.f : 0.f;
    const float2 k = make_float2(((float)px + ox) * keep * ratio, ((float)py + oy) * keep * ratio);
    idx[r] = bi;
    maxval[r] = best;
    *reinterpret_cast<float2*>(raw + r * 2) = k;
    return k;
}

// the shape rule shared by the entries of the three decodes: the kernels index a row's H * W pixels with an int
static inline int pose_shape(const char* name, long rows, int H, int W) {
    HUPR_REQUIRE(rows > 0 && rows < (1L << 31) && H > 0 && W > 0 && (long)H * W < (1L << 31), "%s: bad shape (rows %ld, H %d, W %d)",
                 name, rows, H, W);
    return HUPR_OK;
}

}  // namespace hupr
