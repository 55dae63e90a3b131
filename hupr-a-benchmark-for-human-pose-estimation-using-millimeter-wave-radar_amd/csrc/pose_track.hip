// Keypoint decode with a constant-velocity Kalman filter per joint: the tracking tail of the live stream.
//   * arg-max, sub-pixel refinement and the keypoint's stores exactly as hupr_k_pose_decode (wave_argmax_row, pose_refine.h): the
//     same index, maximum and raw keypoint, bit for bit
//   * the measurement covariance read off the heat-map: second central moments of the 7 x 7 window around the peak
//   * predict / gate / update of a constant-velocity Kalman filter (Kalman 1960) with the white-acceleration process noise and the
//     chi-square gate of Bar-Shalom, Li & Kirubarajan (2001), its state on the device, so that the filtered pose, its velocity, its
//     covariance and a forecast come out of the same launch — and of the same captured graph — as the decode
// The rule is stated in full beside hupr_pose_track_f32 in include/hupr.h; pose_track_model.h holds the filter itself, which the
// associating tracker (pose_assoc.hip) runs too, and what the smoother shares.
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"

namespace hupr {

// One wave = one row.  Nothing is shared between workgroups; the track state of a row is read and written by lane 0 of its wave.
__global__ __launch_bounds__(64) void hupr_k_pose_track(const float* __restrict__ heat, int H, int W, float ratio, int refine,
                                                        float* __restrict__ state, Tracker f, int* __restrict__ idx,
                                                        float* __restrict__ maxval, float* __restrict__ raw,
                                                        float* __restrict__ filtered, float* __restrict__ velocity,
                                                        float* __restrict__ covariance, float* __restrict__ forecast,
                                                        int* __restrict__ status) {
    const long r = blockIdx.x;
    const int lane = threadIdx.x;
    const float* row = heat + r * ((long)H * W);
    float best;
    int bi;
    wave_argmax_row(row, H * W, lane, best, bi);

    const int px = bi % W, py = bi / W;
    const bool positive = best > 0.f;                     // implies 0 <= bi < H * W
    float ox, oy;
    peak_offset(row, H, W, px, py, positive, refine, lane, ox, oy);

    const WindowMoments wm = window_moments(row, H, W, px, py, positive, lane);
    if (lane != 0) return;

    const float2 kp = store_keypoint(r, bi, best, px, py, ox, oy, positive, ratio, idx, maxval, raw);
    const Measurement z = measurement(best, kp.x, kp.y, wm, ratio, f);

    Track t = load_track(state, r);
    int code = HUPR_TRACK_LOST;
    if (t.live) {
        track_predict(t, f);
        const Gate g = track_gate(t, z);
        if (g.valid && g.d2 <= f.gate) {
            track_update(t, z, g);
            code = HUPR_TRACK_UPDATED;
        } else {
            code = track_coast(t, f, z.usable ? HUPR_TRACK_COASTED_GATED : HUPR_TRACK_COASTED_MISSING);
        }
    }
    track_finish(t, z, f, code, r, state, filtered, velocity, covariance, forecast, status);
}

}  // namespace hupr

using namespace hupr;

extern "C" size_t hupr_pose_track_state_bytes(long rows) {
    return rows > 0 ? (size_t)rows * kTrackFloats * sizeof(float) : 0;
}

extern "C" int hupr_pose_track_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* state, float rate_hz,
                                   float accel_psd, float meas_std, float heatmap_gain, float gate, int max_coast,
                                   float init_speed_std, float min_score, float horizon_s, int* idx, float* maxval,
                                   float* raw_keypoints, float* keypoints, float* velocity, float* covariance, float* forecast,
                                   int* status, hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(heat && state && idx && maxval && raw_keypoints && keypoints && velocity && covariance && forecast && status,
                 "hupr_pose_track_f32: null pointer");
    if (int e = pose_shape("hupr_pose_track_f32", rows, H, W)) return e;
    HUPR_REQUIRE(((uintptr_t)state & 15) == 0, "hupr_pose_track_f32: the state must be 16-byte aligned");
    const Tracker f = {rate_hz, accel_psd, meas_std, heatmap_gain, gate, max_coast, init_speed_std, min_score, horizon_s};
    if (int e = tracker_parameters("hupr_pose_track_f32", f)) return e;
    HUPR_LAUNCH(hupr_k_pose_track, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0, state, f,
                idx, maxval, raw_keypoints, keypoints, velocity, covariance, forecast, status);
    HUPR_LAUNCH_OK("hupr_k_pose_track");
    return HUPR_OK;
}
