// Fixed-interval Rauch-Tung-Striebel smoother (Rauch, Tung & Striebel 1965) over a recorded run of the Kalman tracker of
// csrc/pose_track.hip: the backward pass over the states the filter left behind, frame T-1 down to frame 0.
//   * one thread per row, sequential in the frame: a latency-bound recurrence of T dependent steps; the rows axis exists so that many
//     sequences (sequences x joints) share one launch
//   * the successor's smoothed state (4 + 10 values) stays in registers; the filter's state of a frame is read as four float4
//   * no LDS, no atomics, no scratch: every output is bit-identical from run to run and independent of the other rows
// The rule is stated in full beside hupr_pose_smooth_rts_f32 in include/hupr.h; the tracker's model is pose_track_model.h's.
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"
#include "pose_rts.h"

namespace hupr {

// One thread = one row, frames T-1 .. 0.  Nothing is shared between threads.
__global__ __launch_bounds__(64) void hupr_k_pose_smooth_rts(const float* __restrict__ states, const int* __restrict__ status,
                                                             const float* __restrict__ keypoints, long T, long rows, float rate,
                                                             float accel_psd, float* __restrict__ smoothed,
                                                             float* __restrict__ velocity, float* __restrict__ covariance,
                                                             int* __restrict__ flag) {
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    const float dt = 1.f / rate;
    const ProcessNoise q = process_noise(accel_psd, dt);
    float xs[4] = {0.f, 0.f, 0.f, 0.f};
    float ps[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool chained = false;                      // frame k + 1 exists and continues the track of frame k
    for (long k = T - 1; k >= 0; --k) {
        const long e = k * rows + r;
        const int code = status[e];
        int fl;
        if (code == HUPR_TRACK_LOST) {
            *reinterpret_cast<float2*>(smoothed + e * 2) = *reinterpret_cast<const float2*>(keypoints + e * 2);
            *reinterpret_cast<float2*>(velocity + e * 2) = make_float2(0.f, 0.f);
            covariance[e * 3 + 0] = 0.f;
            covariance[e * 3 + 1] = 0.f;
            covariance[e * 3 + 2] = 0.f;
            fl = HUPR_SMOOTH_PASSTHROUGH;
        } else {
            const float4* s = reinterpret_cast<const float4*>(states + e * kTrackFloats);
            const float4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
            const float x[4] = {s0.x, s0.y, s0.z, s0.w};
            const float p[10] = {s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y};
            fl = HUPR_SMOOTH_END;
            if (chained) fl = rts_step(x, p, xs, ps, dt, q) ? HUPR_SMOOTH_SMOOTHED : HUPR_SMOOTH_DEGENERATE;
            if (fl != HUPR_SMOOTH_SMOOTHED) {  // the end of a segment and a degenerate frame: the filter's own state, and the chain goes on from it
#pragma unroll
                for (int j = 0; j < 4; ++j) xs[j] = x[j];
#pragma unroll
                for (int j = 0; j < 10; ++j) ps[j] = p[j];
            }
            *reinterpret_cast<float2*>(smoothed + e * 2) = make_float2(xs[0], xs[1]);
            *reinterpret_cast<float2*>(velocity + e * 2) = make_float2(xs[2], xs[3]);
            covariance[e * 3 + 0] = ps[tri(0, 0)];
            covariance[e * 3 + 1] = ps[tri(0, 1)];
            covariance[e * 3 + 2] = ps[tri(1, 1)];
        }
        flag[e] = fl;
        chained = code != HUPR_TRACK_LOST && code != HUPR_TRACK_STARTED;
    }
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_pose_smooth_rts_f32(const float* states, const int* status, const float* keypoints, long T, long rows,
                                        float rate_hz, float accel_psd, float* smoothed, float* velocity, float* covariance, int* flag,
                                        hupr_stream_t stream) {
    HUPR_REQUIRE(T >= 1 && rows >= 0, "hupr_pose_smooth_rts_f32: bad shape (T %ld, rows %ld)", T, rows);
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(states && status && keypoints && smoothed && velocity && covariance && flag, "hupr_pose_smooth_rts_f32: null pointer");
    HUPR_REQUIRE(T < (1L << 31) && rows < (1L << 31) && T * rows < (1L << 31),
                 "hupr_pose_smooth_rts_f32: T * rows beyond 2^31 (T %ld, rows %ld)", T, rows);
    HUPR_REQUIRE(((uintptr_t)states & 15) == 0, "hupr_pose_smooth_rts_f32: the states must be 16-byte aligned");
    HUPR_REQUIRE(rate_hz > 0.f && rate_hz < INFINITY && accel_psd >= 0.f && accel_psd < INFINITY,
                 "hupr_pose_smooth_rts_f32: bad tracker parameter (rate_hz %g must be positive, accel_psd %g non-negative, both finite)",
                 rate_hz, accel_psd);
    HUPR_LAUNCH(hupr_k_pose_smooth_rts, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, as_stream(stream), states, status, keypoints, T,
                rows, rate_hz, accel_psd, smoothed, velocity, covariance, flag);
    HUPR_LAUNCH_OK("hupr_k_pose_smooth_rts");
    return HUPR_OK;
}
