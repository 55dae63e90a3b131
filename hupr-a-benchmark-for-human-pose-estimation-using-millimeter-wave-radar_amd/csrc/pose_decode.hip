// Keypoint decode with sub-pixel refinement and a device-side One-Euro filter: the tail of the inference path.
//   * arg-max of every (sample, joint) heat-map row — the reduction of hupr_k_argmax_rows (hupr_common.h, wave_argmax_row), so the
//     index and the maximum are its bits                                                       [misc/metrics.py:10-38]
//   * a second-order Taylor step on the log heat-map around the peak (Zhang et al., "Distribution-Aware Coordinate Representation
//     for Human Pose Estimation", CVPR 2020), the quarter-pixel offset of the HRNet decode where the Hessian is not negative definite
//   * optionally the One-Euro filter (Casiez et al., CHI 2012; pose_filter.h) on the image-pixel keypoint, its state on the device, so
//     that the smoothed pose and its velocity come out of the same launch — and of the same captured graph — as the decode
// The rule is stated in full beside hupr_pose_decode_f32 in include/hupr.h.
#include "hupr_common.h"
#include "pose_filter.h"

namespace hupr {

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
    const float2 k = store_keypoint(r, bi, best, px, py, ox, oy, positive, ratio, idx, maxval, raw);
    euro_step(state, r, f, best, k.x, k.y, filtered, velocity);
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
    if (int e = pose_shape("hupr_pose_decode_f32", rows, H, W)) return e;
    const OneEuro f = {rate_hz, min_cutoff, beta, d_cutoff, min_score};
    if (int e = euro_check("hupr_pose_decode_f32", filter_state_or_null, f, keypoints_or_null, velocity_or_null)) return e;
    HUPR_LAUNCH(hupr_k_pose_decode, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0,
                filter_state_or_null, f, idx, maxval, raw_keypoints, keypoints_or_null, velocity_or_null);
    HUPR_LAUNCH_OK("hupr_k_pose_decode");
    return HUPR_OK;
}
