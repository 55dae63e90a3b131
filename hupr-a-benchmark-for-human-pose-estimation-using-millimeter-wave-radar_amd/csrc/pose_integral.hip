// Integral keypoint decode: the mass centroid of a window around the heat-map peak, the decode that goes with the integral coordinate
// loss (Sun et al., "Integral Human Pose Regression", ECCV 2018; Nibali et al., DSNT; csrc/coord_loss.hip trains that centroid).
//   * arg-max of every (sample, joint) heat-map row through wave_argmax_row (hupr_common.h): the index and the maximum are the bits of
//     hupr_k_argmax_rows, hupr_k_pose_decode and hupr_k_pose_track
//   * first moments of the weights max(h, 0) over the window of the given radius around the peak, clipped to the map (radius 0: the
//     whole map), in a summation order fixed by the window alone
//   * optionally the One-Euro filter of hupr_k_pose_decode on the image-pixel keypoint: the one body and the one [rows][8] state of
//     pose_filter.h (this decode stays a source of its own because pose_decode.hip is pinned to one kernel)
// The rule is stated in full beside hupr_pose_decode_integral_f32 in include/hupr.h.
#include "hupr_common.h"
#include "pose_filter.h"

namespace hupr {

// One wave = one row.  Nothing is shared between workgroups; the filter state of a row is read and written by lane 0 of its wave.
__global__ __launch_bounds__(64) void hupr_k_pose_decode_integral(const float* __restrict__ heat, int H, int W, float ratio, int radius,
                                                                  float* __restrict__ state, OneEuro f, int* __restrict__ idx,
                                                                  float* __restrict__ maxval, float* __restrict__ raw,
                                                                  float* __restrict__ filtered, float* __restrict__ velocity) {
    const long r = blockIdx.x;
    const int lane = threadIdx.x;
    const float* row = heat + r * ((long)H * W);
    float best;
    int bi;
    wave_argmax_row(row, H * W, lane, best, bi);

    // ---- window moments: cell c of the window is (x0 + c % ww, y0 + c / ww); lane l adds cells l, l + 64, ... in that order -------------
    const bool positive = best > 0.f;                     // implies 0 <= bi < H * W
    const int px = positive ? bi % W : 0, py = positive ? bi / W : 0;
    const int x0 = max(px - radius, 0), x1 = min(px + radius, W - 1), y0 = max(py - radius, 0), y1 = min(py + radius, H - 1);
    const int ww = x1 - x0 + 1, cells = positive ? ww * (y1 - y0 + 1) : 0;
    float m = 0.f, mx = 0.f, my = 0.f;
    for (int c = lane; c < cells; c += 64) {
        const int gy = y0 + c / ww, gx = x0 + c - (c / ww) * ww;
        const float w = fmaxf(row[(long)gy * W + gx], 0.f);              // a NaN pixel weighs 0 (fmaxf returns the number)
        m += w;
        mx = fmaf(w, (float)(gx - px), mx);
        my = fmaf(w, (float)(gy - py), my);
    }
    m = wave_sum(m);
    mx = wave_sum(mx);
    my = wave_sum(my);
    if (lane != 0) return;

    float ox = 0.f, oy = 0.f;
    if (positive && m > 0.f && finitef(m)) {
        const float tx = mx / m, ty = my / m;
        if (finitef(tx) && finitef(ty)) { ox = tx; oy = ty; }
    }
    const float2 k = store_keypoint(r, bi, best, px, py, ox, oy, positive, ratio, idx, maxval, raw);
    euro_step(state, r, f, best, k.x, k.y, filtered, velocity);
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_pose_decode_integral_f32(const float* heat, long rows, int H, int W, float ratio, int radius,
                                             float* filter_state_or_null, float rate_hz, float min_cutoff, float beta, float d_cutoff,
                                             float min_score, int* idx, float* maxval, float* raw_keypoints, float* keypoints_or_null,
                                             float* velocity_or_null, hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(heat && idx && maxval && raw_keypoints, "hupr_pose_decode_integral_f32: null pointer");
    if (int e = pose_shape("hupr_pose_decode_integral_f32", rows, H, W)) return e;
    HUPR_REQUIRE(radius >= 0, "hupr_pose_decode_integral_f32: bad radius %d (0 = the whole map, else >= 1)", radius);
    const OneEuro f = {rate_hz, min_cutoff, beta, d_cutoff, min_score};
    if (int e = euro_check("hupr_pose_decode_integral_f32", filter_state_or_null, f, keypoints_or_null, velocity_or_null)) return e;
    // radius 0 is the whole map; any radius >= max(H, W) - 1 clips to the same window, so both become max(H, W) (no overflow in px + r)
    const int whole = H > W ? H : W;
    const int rad = (radius == 0 || radius > whole) ? whole : radius;
    HUPR_LAUNCH(hupr_k_pose_decode_integral, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, rad,
                filter_state_or_null, f, idx, maxval, raw_keypoints, keypoints_or_null, velocity_or_null);
    HUPR_LAUNCH_OK("hupr_k_pose_decode_integral");
    return HUPR_OK;
}
