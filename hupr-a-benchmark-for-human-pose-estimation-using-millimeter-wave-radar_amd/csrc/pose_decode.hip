// Keypoint decode with sub-pixel refinement and a device-side One-Euro filter: the tail of the inference path.
//   * arg-max of every (sample, joint) heat-map row — the reduction of hupr_k_argmax_rows (hupr_common.h, wave_argmax_row), so the
//     index and the maximum are its bits                                                       [misc/metrics.py:10-38]
//   * a second-order Taylor step on the log heat-map around the peak (Zhang et al., "Distribution-Aware Coordinate Representation
//     for Human Pose Estimation", CVPR 2020), the quarter-pixel offset of the HRNet decode where the Hessian is not negative definite
//   * optionally the One-Euro filter (Casiez et al., CHI 2012) on the image-pixel keypoint, its state on the device, so that the
//     smoothed pose and its velocity come out of the same launch — and of the same captured graph — as the decode
// The rule is stated in full beside hupr_pose_decode_f32 in include/hupr.h.
#include "hupr_common.h"
#include "pose_refine.h"

namespace hupr {

constexpr int kFilterFloats = 8;      // per row: x, y, dx, dy (filtered position and velocity), valid, 3 x pad

struct OneEuro {
    float rate, min_cutoff, beta, d_cutoff, min_score;
};

__device__ __forceinline__ float euro_alpha(float rate, float cutoff) { return 1.f / (1.f + rate / (6.283185307179586f * cutoff)); }

// One wave = one row.  Nothing is shared between workgroups; the filter state of a row is read and written by lane 0 of its wave.
__global__ __launch_bounds__(64) void hupr_k_pose_decode(const float* __restrict__ heat, int H, int W, float ratio, int refine,
                                                         float* __restrict__ state, OneEuro f, int* __restrict__ idx,
                                                         float* __restrict__ maxval, float* __restrict__ raw,
                                                         float* __restrict__ filtered, float* __restrict__ velocity) {
    const long r = blockIdx.x;
    const int lane = threadIdx.x;
    const float* row = heat + r * ((long)H * W);
    float best;
    int bi;
    wave_argmax_row(row, H * W, lane, best, bi);

    // ---- refinement: every lane ends with the same offset (pose_refine.h) ---------------------------------------------------------
    const int px = bi % W, py = bi / W;
    const bool positive = best > 0.f;                     // implies 0 <= bi < H * W
    float ox, oy;
    peak_offset(row, H, W, px, py, positive, refine, lane, ox, oy);
    if (lane != 0) return;

    // a joint whose maximum is <= 0 decodes to (0, 0) (misc/metrics.py); with a zero offset these are the floats of
    // hupr_k_stream_keypoints
    const float keep = positive ? 1.f : 0.f;
    const float x = ((float)px + ox) * keep * ratio, y = ((float)py + oy) * keep * ratio;
    idx[r] = bi;
    maxval[r] = best;
    *reinterpret_cast<float2*>(raw + r * 2) = make_float2(x, y);
    if (!state) return;

    // ---- One-Euro filter ---------------------------------------------------------------------------------------------------------
    float* s = state + r * kFilterFloats;
    const float sx = s[0], sy = s[1], svx = s[2], svy = s[3];
    const bool valid = s[4] != 0.f;
    const bool missing = !(best > f.min_score) || !finitef(x) || !finitef(y);
    float fx = x, fy = y, vx = 0.f, vy = 0.f;
    if (missing) {
        if (valid) { fx = sx; fy = sy; }                  // the joint holds its place; the state is left as it is
    } else {
        if (valid) {
            const float ad = euro_alpha(f.rate, f.d_cutoff);
            const float rx = (x - sx) * f.rate, ry = (y - sy) * f.rate;
            vx = ad * rx + (1.f - ad) * svx;
            vy = ad * ry + (1.f - ad) * svy;
            const float ax = euro_alpha(f.rate, f.min_cutoff + f.beta * fabsf(vx));
            const float ay = euro_alpha(f.rate, f.min_cutoff + f.beta * fabsf(vy));
            fx = ax * x + (1.f - ax) * sx;
            fy = ay * y + (1.f - ay) * sy;
        }
        s[0] = fx;
        s[1] = fy;
        s[2] = vx;
        s[3] = vy;
        s[4] = 1.f;
    }
    if (filtered) *reinterpret_cast<float2*>(filtered + r * 2) = make_float2(fx, fy);
    if (velocity) *reinterpret_cast<float2*>(velocity + r * 2) = make_float2(vx, vy);
}

}  // namespace hupr

using namespace hupr;

extern "C" size_t hupr_pose_filter_state_bytes(long rows) {
    return rows > 0 ? (size_t)rows * kFilterFloats * sizeof(float) : 0;
}

extern "C" int hupr_pose_decode_f32(const float* heat, long rows, int H, int W, float ratio, int refine,
                                    float* filter_state_or_null, float rate_hz, float min_cutoff, float beta, float d_cutoff,
                                    float min_score, int* idx, float* maxval, float* raw_keypoints, float* keypoints_or_null,
                                    float* velocity_or_null, hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(heat && idx && maxval && raw_keypoints, "hupr_pose_decode_f32: null pointer");
    HUPR_REQUIRE(rows > 0 && rows < (1L << 31) && H > 0 && W > 0 && (long)H * W < (1L << 31),
                 "hupr_pose_decode_f32: bad shape (rows %ld, H %d, W %d)", rows, H, W);
    if (filter_state_or_null) {
        HUPR_REQUIRE(rate_hz > 0.f && rate_hz < INFINITY && min_cutoff > 0.f && min_cutoff < INFINITY && d_cutoff > 0.f &&
                         d_cutoff < INFINITY && beta >= 0.f && beta < INFINITY && min_score == min_score,
                     "hupr_pose_decode_f32: bad filter parameter (rate_hz %g, min_cutoff %g and d_cutoff %g must be positive, beta %g "
                     "non-negative, min_score %g a number)", rate_hz, min_cutoff, d_cutoff, beta, min_score);
    } else {
        HUPR_REQUIRE(!keypoints_or_null && !velocity_or_null,
                     "hupr_pose_decode_f32: filtered keypoints / velocity asked for without a filter state");
    }
    const OneEuro f = {rate_hz, min_cutoff, beta, d_cutoff, min_score};
    HUPR_LAUNCH(hupr_k_pose_decode, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0,
                filter_state_or_null, f, idx, maxval, raw_keypoints, keypoints_or_null, velocity_or_null);
    HUPR_LAUNCH_OK("hupr_k_pose_decode");
    return HUPR_OK;
}
