// The Kalman joint tracker of pose_track.hip with a choice of measurement: up to four peaks of the heat-map are decoded, and the track
// takes the one inside its gate that it finds most likely (the nearest-neighbour standard filter of Bar-Shalom, Li & Kirubarajan 2001)
// instead of the strongest.  A mirrored limb or a multipath ghost that outshines the joint then no longer stops the track.
//   * candidate 0 is the arg-max of hupr_k_pose_track, bit for bit; candidates 1.. are the next 3 x 3 local maxima in the order (value
//     descending, index ascending) that lie far enough from the candidates taken and high enough beside the maximum
//   * every candidate is refined (pose_refine.h) and gets its own covariance from its 7 x 7 window, by the wave code of the tracker
//   * predict, gate, Joseph update, coasting and the stores are the tracker's own functions (pose_track_model.h)
//   * an optional presence flag per group of rows takes the measurement away: the track coasts
// With a null state the kernel is the peak finder alone (hupr_pose_peaks_f32).  The rule is stated in full beside
// hupr_pose_track_assoc_f32 in include/hupr.h.
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"

namespace hupr {

constexpr int kMaxCandidates = 4;

struct Peaks {
    int K, min_separation;
    float peak_ratio;
};

// (a, ia) stands in front of (b, ib) in the order (value descending, index ascending); never with a NaN on either side
__device__ __forceinline__ bool in_front(float a, long ia, float b, long ib) { return a > b || (a == b && ia < ib); }

// Pixel i = (x, y) of value v > 0 is a 3 x 3 local maximum: none of its up to eight neighbours inside the map stands in front of it.
__device__ __forceinline__ bool local_maximum(const float* row, int H, int W, int x, int y, float v, long i) {
    bool top = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if ((dx != 0 || dy != 0) && qx >= 0 && qx < W && qy >= 0 && qy < H) {
                const long qi = (long)qy * W + qx;
                top = top && !in_front(row[qi], qi, v, i);
            }
        }
    }
    return top;
}

// One wave = one row.  Nothing is shared between workgroups, nothing is accumulated in memory: the same map gives the same bits.
// Rounds 1 .. K - 1 are a masked wave arg-max each; the mask (behind the last candidate in the order, above the floor, far from the
// candidates taken, a local maximum) is evaluated where a pixel would otherwise win its lane, the neighbours read from global memory.
// The taken set only grows, so a pixel refused for its distance stays refused, and every round's winner stands behind the last one's.
// Lane 0 runs the recurrence between the rounds.
__global__ __launch_bounds__(64) void hupr_k_pose_track_assoc(const float* __restrict__ heat, int H, int W, float ratio, int refine,
                                                              float* __restrict__ state, Tracker f, Peaks c,
                                                              const int* __restrict__ present, int rows_per_group,
                                                              int* __restrict__ idx, float* __restrict__ maxval, float* __restrict__ raw,
                                                              float* __restrict__ filtered, float* __restrict__ velocity,
                                                              float* __restrict__ covariance, float* __restrict__ forecast,
                                                              int* __restrict__ status, float* __restrict__ cand_xy,
                                                              float* __restrict__ cand_score, int* __restrict__ cand_idx,
                                                              int* __restrict__ cand_count, int* __restrict__ chosen) {
    const long r = blockIdx.x;
    const int lane = threadIdx.x;
    const long n = (long)H * W;
    const float* row = heat + r * n;
    const bool tracking = state != nullptr;
    const bool seen = present == nullptr || present[r / rows_per_group] != 0;
    float best;
    int bi;
    wave_argmax_row(row, (int)n, lane, best, bi);
    const bool positive = best > 0.f;                     // implies 0 <= bi < H * W
    const float floor_v = c.peak_ratio * best;

    // lane 0's: the predicted track, candidate 0's measurement and the best gated one so far
    Track t = {};
    Measurement z0 = {}, zc = {};
    Gate gc = {};
    float cost = INFINITY;
    int pick = -1;
    bool any_usable = false;
    if (tracking && lane == 0) {
        t = load_track(state, r);
        if (t.live) track_predict(t, f);
    }

    int tx[kMaxCandidates], ty[kMaxCandidates];           // the candidates taken; indexed by unrolled constants only
    float pv = best;                                      // the last candidate taken
    long pi = bi;
    int count = 0;
    bool more = positive;
#pragma unroll
    for (int k = 0; k < kMaxCandidates; ++k) {
        tx[k] = ty[k] = 0;
        if (k >= c.K || !more) continue;
        if (k > 0) {
            // ---- masked arg-max: a lane walks its pixels upwards, so only a larger value can replace its best -------------------------
            float cv = -INFINITY;
            long ci = 0x7fffffff;
            for (long i = lane; i < n; i += 64) {
                const float v = row[i];
                if (!(v > 0.f && v >= floor_v && v > cv && in_front(pv, pi, v, i))) continue;
                const int x = (int)i % W, y = (int)i / W;                                   // i < H * W < 2^31
                bool far = true;
#pragma unroll
                for (int j = 0; j < kMaxCandidates; ++j)
                    if (j < k) far = far && max(abs(x - tx[j]), abs(y - ty[j])) > c.min_separation;
                if (far && local_maximum(row, H, W, x, y, v, i)) { cv = v; ci = i; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(cv, o, 64);
                const int oi = __shfl_xor((int)ci, o, 64);
                if (in_front(ov, oi, cv, ci)) { cv = ov; ci = oi; }
            }
            if (ci == 0x7fffffff) { more = false; continue; }                          // nothing qualifies: the list ends here
            pv = cv;
            pi = ci;
        }
        const int px = (int)pi % W, py = (int)pi / W;
        tx[k] = px;
        ty[k] = py;
        count = k + 1;
        float ox, oy;
        peak_offset(row, H, W, px, py, true, refine, lane, ox, oy);
        WindowMoments wm = {};
        if (tracking) wm = window_moments(row, H, W, px, py, true, lane);
        if (lane == 0) {
            float2 kp;
            if (k == 0 && tracking) kp = store_keypoint(r, bi, best, px, py, ox, oy, true, ratio, idx, maxval, raw);
            else kp = make_float2(((float)px + ox) * ratio, ((float)py + oy) * ratio);
            *reinterpret_cast<float2*>(cand_xy + (r * c.K + k) * 2) = kp;
            cand_score[r * c.K + k] = pv;
            if (cand_idx) cand_idx[r * c.K + k] = (int)pi;
            if (tracking) {
                Measurement z = measurement(pv, kp.x, kp.y, wm, ratio, f);
                z.usable = z.usable && seen;
                if (k == 0) z0 = z;
                any_usable = any_usable || z.usable;
                if (t.live) {
                    // ---- association: the gated candidate of the smallest d2 + ln det S, the lower k on a tie ---------------------------
                    const Gate g = track_gate(t, z);
                    const float ck = g.d2 + logf(g.det);
                    if (g.valid && g.d2 <= f.gate && ck < cost) { cost = ck; pick = k; zc = z; gc = g; }
                }
            }
        }
    }
    if (lane != 0) return;

#pragma unroll
    for (int k = 0; k < kMaxCandidates; ++k) {
        if (k < c.K && k >= count) {                                                   // slots past the count hold zeros
            *reinterpret_cast<float2*>(cand_xy + (r * c.K + k) * 2) = make_float2(0.f, 0.f);
            cand_score[r * c.K + k] = 0.f;
            if (cand_idx) cand_idx[r * c.K + k] = 0;
        }
    }
    cand_count[r] = count;
    if (!tracking) return;

    if (!positive) {                                      // no candidate: the tracker's decode of a non-positive maximum, (0, 0), not usable
        const WindowMoments none = {0.f, 0.f, 0.f, 0.f};
        const float2 kp = store_keypoint(r, bi, best, bi % W, bi / W, 0.f, 0.f, false, ratio, idx, maxval, raw);
        z0 = measurement(best, kp.x, kp.y, none, ratio, f);
    }
    int code = HUPR_TRACK_LOST;
    if (t.live) {
        if (pick >= 0) {
            track_update(t, zc, gc);
            code = HUPR_TRACK_UPDATED;
        } else {
            code = track_coast(t, f, any_usable ? HUPR_TRACK_COASTED_GATED : HUPR_TRACK_COASTED_MISSING);
        }
    }
    code = track_finish(t, z0, f, code, r, state, filtered, velocity, covariance, forecast, status);
    chosen[r] = code == HUPR_TRACK_UPDATED ? pick : (code == HUPR_TRACK_STARTED ? 0 : -1);
}

static int peaks_arguments(const char* name, int K, int min_separation, float peak_ratio) {
    HUPR_REQUIRE(K >= 1 && K <= kMaxCandidates && min_separation >= 0 && peak_ratio > 0.f && peak_ratio <= 1.f,
                 "%s: bad candidate parameter (K %d must be in 1..%d, min_separation %d non-negative, peak_ratio %g in (0, 1])", name, K,
                 kMaxCandidates, min_separation, peak_ratio);
    return HUPR_OK;
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_pose_track_assoc_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* state, float rate_hz,
                                         float accel_psd, float meas_std, float heatmap_gain, float gate, int max_coast,
                                         float init_speed_std, float min_score, float horizon_s, int K, int min_separation,
                                         float peak_ratio, const int* present_or_null, int rows_per_group, int* idx, float* maxval,
                                         float* raw_keypoints, float* keypoints, float* velocity, float* covariance, float* forecast,
                                         int* status, float* cand_xy, float* cand_score, int* cand_count, int* chosen,
                                         hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(heat && state && idx && maxval && raw_keypoints && keypoints && velocity && covariance && forecast && status &&
                     cand_xy && cand_score && cand_count && chosen,
                 "hupr_pose_track_assoc_f32: null pointer");
    if (int e = pose_shape("hupr_pose_track_assoc_f32", rows, H, W)) return e;
    HUPR_REQUIRE(((uintptr_t)state & 15) == 0, "hupr_pose_track_assoc_f32: the state must be 16-byte aligned");
    const Tracker f = {rate_hz, accel_psd, meas_std, heatmap_gain, gate, max_coast, init_speed_std, min_score, horizon_s};
    if (int e = tracker_parameters("hupr_pose_track_assoc_f32", f)) return e;
    if (int e = peaks_arguments("hupr_pose_track_assoc_f32", K, min_separation, peak_ratio)) return e;
    HUPR_REQUIRE(!present_or_null || (rows_per_group >= 1 && rows % rows_per_group == 0),
                 "hupr_pose_track_assoc_f32: rows %ld is no multiple of rows_per_group %d", rows, rows_per_group);
    const Peaks c = {K, min_separation, peak_ratio};
    HUPR_LAUNCH(hupr_k_pose_track_assoc, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0, state, f,
                c, present_or_null, present_or_null ? rows_per_group : 1, idx, maxval, raw_keypoints, keypoints, velocity, covariance,
                forecast, status, cand_xy, cand_score, (int*)nullptr, cand_count, chosen);
    HUPR_LAUNCH_OK("hupr_k_pose_track_assoc");
    return HUPR_OK;
}

extern "C" int hupr_pose_peaks_f32(const float* heat, long rows, int H, int W, float ratio, int refine, int K, int min_separation,
                                   float peak_ratio, float* cand_xy, float* cand_score, int* cand_idx, int* cand_count,
                                   hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(heat && cand_xy && cand_score && cand_idx && cand_count, "hupr_pose_peaks_f32: null pointer");
    if (int e = pose_shape("hupr_pose_peaks_f32", rows, H, W)) return e;
    if (int e = peaks_arguments("hupr_pose_peaks_f32", K, min_separation, peak_ratio)) return e;
    const Tracker none = {};
    const Peaks c = {K, min_separation, peak_ratio};
    HUPR_LAUNCH(hupr_k_pose_track_assoc, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0,
                (float*)nullptr, none, c, (const int*)nullptr, 1, (int*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                (float*)nullptr, (float*)nullptr, (float*)nullptr, (int*)nullptr, cand_xy, cand_score, cand_idx, cand_count,
                (int*)nullptr);
    HUPR_LAUNCH_OK("hupr_k_pose_track_assoc");
    return HUPR_OK;
}
