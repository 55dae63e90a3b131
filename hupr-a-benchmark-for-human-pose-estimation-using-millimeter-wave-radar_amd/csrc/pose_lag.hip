// Fixed-lag Rauch-Tung-Striebel smoother (Moore 1973; Simon, Optimal State Estimation, ch. 9) behind the Kalman tracker of
// csrc/pose_track.hip, one launch per tracked frame: the frame is filed in a ring of the last L + 1 tracker states in device memory,
// and the backward pass of csrc/pose_smooth.hip runs over that ring only, newest frame first.  The oldest frame of the ring is the
// fixed-lag answer: the pose of L frames ago, smoothed with everything seen since.
//   * one thread per row, sequential in the frame: a latency-bound recurrence of at most L dependent steps
//   * the frame counter is the row's own and lives in the lag state, so no launch argument depends on the frame number and the
//     launch replays inside a captured graph; no thread reads what another writes
//   * the ring is [slot][rows][...], a slot's states being read as four float4 per row like a frame of the fixed-interval kernel
//   * the backward step is pose_rts.h's, the very expressions of the fixed-interval kernel: the tail of a launch is that kernel's
//     output over the same frames bit for bit.  The gains are recomputed, not cached: a cached gain would change which products the
//     compiler contracts
//   * no LDS, no atomics, no scratch: every output is bit-identical from run to run and independent of the other rows
// The rule is stated in full beside hupr_pose_smooth_lag_f32 in include/hupr.h.
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"
#include "pose_rts.h"

namespace hupr {

constexpr int kMaxLag = 64;
// the lag state per row and slot: the tracker's state, the filtered and the raw keypoints, status, maximum; and one counter per row
constexpr int kLagSlotFloats = kTrackFloats + 2 + 2 + 1 + 1;

// The sections of the lag state of ``rows`` rows and ``slots`` = L + 1 slots, in floats from its start.  Every section starts at an
// even offset, the states at 0: float4 and float2 accesses stay aligned.
struct LagLayout {
    long states, filtered, raw, status, scores, count, total;
};
__host__ __device__ inline LagLayout lag_layout(long rows, long slots) {
    const long n = rows * slots;
    return {0, n * kTrackFloats, n * (kTrackFloats + 2), n * (kTrackFloats + 4), n * (kTrackFloats + 5), n * kLagSlotFloats,
            n * kLagSlotFloats + rows};
}

// One thread = one row: file the frame, then the window newest frame first.  Nothing is shared between threads.
__global__ __launch_bounds__(64) void hupr_k_pose_smooth_lag(const float* __restrict__ track_state, const int* __restrict__ status,
                                                             const float* __restrict__ keypoints, const float* __restrict__ raw_keypoints,
                                                             const float* __restrict__ maxval, long rows, int lag, float rate,
                                                             float accel_psd, float* lag_state, float* __restrict__ tail_keypoints,
                                                             float* __restrict__ tail_velocity, float* __restrict__ tail_covariance,
                                                             int* __restrict__ tail_flag, float* __restrict__ tail_filtered,
                                                             float* __restrict__ tail_raw, int* __restrict__ tail_status,
                                                             float* __restrict__ tail_scores) {
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    const int slots = lag + 1;
    const LagLayout at = lag_layout(rows, slots);
    float* ring_states = lag_state + at.states;
    float* ring_filtered = lag_state + at.filtered;
    float* ring_raw = lag_state + at.raw;
    int* ring_status = reinterpret_cast<int*>(lag_state + at.status);
    float* ring_scores = lag_state + at.scores;
    int* count = reinterpret_cast<int*>(lag_state + at.count);

    // ---- file the frame: n frames of this row were filed before it; n stays below 2 (L + 1) with n mod (L + 1) and n >= L kept ----------
    int n = count[r];
    if (n < 0 || n >= 2 * slots) n = 0;        // no counter this kernel wrote: a new sequence, and no index leaves the ring
    const int newest = n % slots;
    {
        const long e = (long)newest * rows + r;
        const float4* s = reinterpret_cast<const float4*>(track_state + r * kTrackFloats);
        float4* d = reinterpret_cast<float4*>(ring_states + e * kTrackFloats);
        d[0] = s[0];
        d[1] = s[1];
        d[2] = s[2];
        d[3] = s[3];
        *reinterpret_cast<float2*>(ring_filtered + e * 2) = *reinterpret_cast<const float2*>(keypoints + r * 2);
        *reinterpret_cast<float2*>(ring_raw + e * 2) = *reinterpret_cast<const float2*>(raw_keypoints + r * 2);
        ring_status[e] = status[r];
        ring_scores[e] = maxval[r];
        count[r] = n + 1 >= 2 * slots ? n + 1 - slots : n + 1;
    }
    const int have = n < lag ? n : lag;        // frames in front of this one that the ring still holds

    // ---- the backward pass of hupr_k_pose_smooth_rts over the window, tail slot j = frame n - j -------------------------------------------
    const float dt = 1.f / rate;
    const ProcessNoise q = process_noise(accel_psd, dt);
    float xs[4] = {0.f, 0.f, 0.f, 0.f};
    float ps[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool chained = false;                      // frame k + 1 exists and continues the track of frame k
    int slot = newest;
    for (int j = 0; j <= have; ++j) {
        const long e = (long)slot * rows + r;  // in the ring
        const long o = (long)j * rows + r;     // in the tail
        const int code = ring_status[e];
        const float2 kp = *reinterpret_cast<const float2*>(ring_filtered + e * 2);
        int fl;
        if (code == HUPR_TRACK_LOST) {
            *reinterpret_cast<float2*>(tail_keypoints + o * 2) = kp;
            *reinterpret_cast<float2*>(tail_velocity + o * 2) = make_float2(0.f, 0.f);
            tail_covariance[o * 3 + 0] = 0.f;
            tail_covariance[o * 3 + 1] = 0.f;
            tail_covariance[o * 3 + 2] = 0.f;
            fl = HUPR_SMOOTH_PASSTHROUGH;
        } else {
            const float4* s = reinterpret_cast<const float4*>(ring_states + e * kTrackFloats);
            const float4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
            const float x[4] = {s0.x, s0.y, s0.z, s0.w};
            const float p[10] = {s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y};
            fl = HUPR_SMOOTH_END;
            if (chained) fl = rts_step(x, p, xs, ps, dt, q) ? HUPR_SMOOTH_SMOOTHED : HUPR_SMOOTH_DEGENERATE;
            if (fl != HUPR_SMOOTH_SMOOTHED) {  // the end of a segment and a degenerate frame: the filter's own state, and the chain goes on from it
#pragma unroll
                for (int i = 0; i < 4; ++i) xs[i] = x[i];
#pragma unroll
                for (int i = 0; i < 10; ++i) ps[i] = p[i];
            }
            *reinterpret_cast<float2*>(tail_keypoints + o * 2) = make_float2(xs[0], xs[1]);
            *reinterpret_cast<float2*>(tail_velocity + o * 2) = make_float2(xs[2], xs[3]);
            tail_covariance[o * 3 + 0] = ps[tri(0, 0)];
            tail_covariance[o * 3 + 1] = ps[tri(0, 1)];
            tail_covariance[o * 3 + 2] = ps[tri(1, 1)];
        }
        tail_flag[o] = fl;
        *reinterpret_cast<float2*>(tail_filtered + o * 2) = kp;
        *reinterpret_cast<float2*>(tail_raw + o * 2) = *reinterpret_cast<const float2*>(ring_raw + e * 2);
        tail_status[o] = code;
        tail_scores[o] = ring_scores[e];
        chained = code != HUPR_TRACK_LOST && code != HUPR_TRACK_STARTED;
        slot = slot == 0 ? lag : slot - 1;
    }
    // ---- the frames that do not exist yet ------------------------------------------------------------------------------------------------
    for (int j = have + 1; j <= lag; ++j) {
        const long o = (long)j * rows + r;
        *reinterpret_cast<float2*>(tail_keypoints + o * 2) = make_float2(0.f, 0.f);
        *reinterpret_cast<float2*>(tail_velocity + o * 2) = make_float2(0.f, 0.f);
        tail_covariance[o * 3 + 0] = 0.f;
        tail_covariance[o * 3 + 1] = 0.f;
        tail_covariance[o * 3 + 2] = 0.f;
        tail_flag[o] = HUPR_SMOOTH_EMPTY;
        *reinterpret_cast<float2*>(tail_filtered + o * 2) = make_float2(0.f, 0.f);
        *reinterpret_cast<float2*>(tail_raw + o * 2) = make_float2(0.f, 0.f);
        tail_status[o] = 0;
        tail_scores[o] = 0.f;
    }
}

}  // namespace hupr

using namespace hupr;

extern "C" size_t hupr_pose_lag_state_bytes(long rows, int lag) {
    if (rows < 0 || rows >= (1L << 31) / (kMaxLag + 1) || lag < 1 || lag > kMaxLag) return 0;
    return (size_t)lag_layout(rows, lag + 1).total * sizeof(float);
}

extern "C" int hupr_pose_smooth_lag_f32(const float* track_state, const int* status, const float* keypoints,
                                        const float* raw_keypoints, const float* maxval, long rows, int lag, float rate_hz,
                                        float accel_psd, float* lag_state, float* tail_keypoints, float* tail_velocity,
                                        float* tail_covariance, int* tail_flag, float* tail_filtered, float* tail_raw, int* tail_status,
                                        float* tail_scores, hupr_stream_t stream) {
    HUPR_REQUIRE(rows >= 0, "hupr_pose_smooth_lag_f32: bad shape (rows %ld)", rows);
    HUPR_REQUIRE(lag >= 1 && lag <= kMaxLag, "hupr_pose_smooth_lag_f32: lag %d outside 1..%d", lag, kMaxLag);
    HUPR_REQUIRE(rate_hz > 0.f && rate_hz < INFINITY && accel_psd >= 0.f && accel_psd < INFINITY,
                 "hupr_pose_smooth_lag_f32: bad tracker parameter (rate_hz %g must be positive, accel_psd %g non-negative, both finite)",
                 rate_hz, accel_psd);
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(track_state && status && keypoints && raw_keypoints && maxval && lag_state && tail_keypoints && tail_velocity &&
                     tail_covariance && tail_flag && tail_filtered && tail_raw && tail_status && tail_scores,
                 "hupr_pose_smooth_lag_f32: null pointer");
    HUPR_REQUIRE(rows < (1L << 31) / (kMaxLag + 1), "hupr_pose_smooth_lag_f32: rows * (lag + 1) beyond 2^31 (rows %ld)", rows);
    HUPR_REQUIRE(((uintptr_t)track_state & 15) == 0 && ((uintptr_t)lag_state & 15) == 0,
                 "hupr_pose_smooth_lag_f32: the tracker state and the lag state must be 16-byte aligned");
    HUPR_LAUNCH(hupr_k_pose_smooth_lag, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, as_stream(stream), track_state, status, keypoints,
                raw_keypoints, maxval, rows, lag, rate_hz, accel_psd, lag_state, tail_keypoints, tail_velocity, tail_covariance, tail_flag,
                tail_filtered, tail_raw, tail_status, tail_scores);
    HUPR_LAUNCH_OK("hupr_k_pose_smooth_lag");
    return HUPR_OK;
}
