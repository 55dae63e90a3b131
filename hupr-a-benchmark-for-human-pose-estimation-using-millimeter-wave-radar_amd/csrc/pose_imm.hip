// The Kalman joint tracker of pose_track.hip with two motion models per row: the interacting-multiple-model estimator (Blom &
// Bar-Shalom 1988; Bar-Shalom, Li & Kirubarajan 2001, section 11.6).  A joint rests, reaches and rests again, and one accel_psd is
// wrong for one of the two regimes; here a "still" filter (accel_psd) and a "moving" one (accel_psd_moving) run on the same
// measurement, a two-state Markov chain couples them, and the output is their probability-weighted mixture.
//   * arg-max, refinement, the measurement and its covariance are the tracker's own wave code: idx, maxval and the raw keypoint are
//     hupr_k_pose_decode's bits
//   * predict, gate, Joseph update, coasting and the start of a track are the device functions of pose_track_model.h, called once per
//     model with a Tracker whose accel_psd is that model's; only the mixing and the mixture are new arithmetic (imm_mix below)
//   * one life cycle (live, coast, status) per row, shared by both models
// The rule is stated in full beside hupr_pose_track_imm_f32 in include/hupr.h.
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"

namespace hupr {

constexpr int kImmFloats = 32;        // per row: model 0's x, y, vx, vy and 10 covariance entries, model 1's same 14, mu0, mu1, live, coast

struct Imm {
    float accel_psd_moving, switch_prob, moving_prior;
};

// The moment-matched mixture wa N(a) + wb N(b), wa + wb = 1: mean xa + wb (xb - xa), covariance sum_i w_i (P_i + d_i d_i^T) with d_i the
// component's mean minus the mixture's.  With (wa, wb) = (1, 0) the result is ``a`` bit for bit (``b`` finite).  live / coast are a's.
__device__ __forceinline__ Track imm_mix(const Track& a, const Track& b, float wa, float wb) {
    HUPR_EXACT_FP
    Track m = a;
    m.x0 = fmaf(wb, b.x0 - a.x0, a.x0);
    m.x1 = fmaf(wb, b.x1 - a.x1, a.x1);
    m.x2 = fmaf(wb, b.x2 - a.x2, a.x2);
    m.x3 = fmaf(wb, b.x3 - a.x3, a.x3);
    const float a0 = a.x0 - m.x0, a1 = a.x1 - m.x1, a2 = a.x2 - m.x2, a3 = a.x3 - m.x3;
    const float b0 = b.x0 - m.x0, b1 = b.x1 - m.x1, b2 = b.x2 - m.x2, b3 = b.x3 - m.x3;
#define HUPR_MIX(i, j) m.p##i##j = fmaf(wb, fmaf(b##i, b##j, b.p##i##j), wa * fmaf(a##i, a##j, a.p##i##j));
    HUPR_MIX(0, 0) HUPR_MIX(0, 1) HUPR_MIX(0, 2) HUPR_MIX(0, 3) HUPR_MIX(1, 1) HUPR_MIX(1, 2) HUPR_MIX(1, 3) HUPR_MIX(2, 2) HUPR_MIX(2, 3)
    HUPR_MIX(3, 3)
#undef HUPR_MIX
    return m;
}

// One wave = one row, as hupr_k_pose_track.  Nothing is shared between workgroups; the state of a row is read and written by lane 0.
__global__ __launch_bounds__(64) void hupr_k_pose_track_imm(const float* __restrict__ heat, int H, int W, float ratio, int refine,
                                                            float* __restrict__ state, Tracker f, Imm c,
                                                            const int* __restrict__ present, int rows_per_group,
                                                            int* __restrict__ idx, float* __restrict__ maxval, float* __restrict__ raw,
                                                            float* __restrict__ filtered, float* __restrict__ velocity,
                                                            float* __restrict__ covariance, float* __restrict__ forecast,
                                                            int* __restrict__ status, float* __restrict__ moving) {
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
    Measurement z = measurement(best, kp.x, kp.y, wm, ratio, f);
    z.usable = z.usable && (present == nullptr || present[r / rows_per_group] != 0);

    Tracker fm = f;                                       // the moving model's parameters: the still model's but for the process noise
    fm.accel_psd = c.accel_psd_moving;

    float4* s = reinterpret_cast<float4*>(state + r * kImmFloats);
    const float4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3], s4 = s[4], s5 = s[5], s6 = s[6], s7 = s[7];
    const bool live = s7.z != 0.f;
    Track a = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y, live, s7.w};
    Track b = {s3.z, s3.w, s4.x, s4.y, s4.z, s4.w, s5.x, s5.y, s5.z, s5.w, s6.x, s6.y, s6.z, s6.w, live, s7.w};
    float mu0 = s7.x, mu1 = s7.y;

    int code = HUPR_TRACK_LOST;
    if (live) {
        HUPR_EXACT_FP
        // ---- mixing: the models exchange their estimates in proportion to the chain's switching prior ---------------------------------
        float c0 = mu0, c1 = mu1;
        if (c.switch_prob != 0.f) {
            const float p = c.switch_prob, q = 1.f - p;
            c0 = fmaf(q, mu0, p * mu1);
            c1 = fmaf(p, mu0, q * mu1);
            const Track a0 = imm_mix(a, b, q * mu0 / c0, p * mu1 / c0), b0 = imm_mix(a, b, p * mu0 / c1, q * mu1 / c1);
            a = a0;
            b = b0;
        }
        track_predict(a, f);
        track_predict(b, fm);
        const Gate g0 = track_gate(a, z), g1 = track_gate(b, z);
        const bool in0 = c0 > 0.f && g0.valid, in1 = c1 > 0.f && g1.valid;              // the models that have a say
        if ((in0 && g0.d2 <= f.gate) || (in1 && g1.d2 <= f.gate)) {
            if (g0.valid) track_update(a, z, g0);
            if (g1.valid) track_update(b, z, g1);
            // ---- mode probabilities from the innovation likelihoods, exp(-l / 2) with l = d2 + ln det S ----------------------------------
            const float l0 = g0.d2 + logf(g0.det), l1 = g1.d2 + logf(g1.det);
            const float m = in0 && in1 ? fminf(l0, l1) : (in0 ? l0 : l1);
            const float w0 = in0 ? c0 * expf(-0.5f * (l0 - m)) : 0.f, w1 = in1 ? c1 * expf(-0.5f * (l1 - m)) : 0.f;
            const float sum = w0 + w1;
            mu0 = w0 / sum;
            mu1 = w1 / sum;
            a.coast = 0.f;
            code = HUPR_TRACK_UPDATED;
        } else {
            mu0 = c0;
            mu1 = c1;
            code = track_coast(a, f, z.usable ? HUPR_TRACK_COASTED_GATED : HUPR_TRACK_COASTED_MISSING);
        }
    }
    if (!a.live) {                                        // no live track, also one that ended in this frame: both models start from z
        b.live = false;
        code = track_end(a, z, f, code);
        track_end(b, z, fm, code);
        mu0 = a.live ? 1.f - c.moving_prior : 0.f;
        mu1 = a.live ? c.moving_prior : 0.f;
    }

    s[0] = make_float4(a.x0, a.x1, a.x2, a.x3);
    s[1] = make_float4(a.p00, a.p01, a.p02, a.p03);
    s[2] = make_float4(a.p11, a.p12, a.p13, a.p22);
    s[3] = make_float4(a.p23, a.p33, b.x0, b.x1);
    s[4] = make_float4(b.x2, b.x3, b.p00, b.p01);
    s[5] = make_float4(b.p02, b.p03, b.p11, b.p12);
    s[6] = make_float4(b.p13, b.p22, b.p23, b.p33);
    s[7] = make_float4(mu0, mu1, a.live ? 1.f : 0.f, a.coast);

    const Track x = imm_mix(a, b, mu0, mu1);
    const float kx = a.live ? x.x0 : z.zx, ky = a.live ? x.x1 : z.zy;                  // LOST: the raw keypoint, nothing else
    *reinterpret_cast<float2*>(filtered + r * 2) = make_float2(kx, ky);
    *reinterpret_cast<float2*>(velocity + r * 2) = make_float2(x.x2, x.x3);
    covariance[r * 3 + 0] = x.p00;
    covariance[r * 3 + 1] = x.p01;
    covariance[r * 3 + 2] = x.p11;
    *reinterpret_cast<float2*>(forecast + r * 2) = make_float2(fmaf(x.x2, f.horizon, kx), fmaf(x.x3, f.horizon, ky));
    status[r] = code;
    moving[r] = mu1;
}

}  // namespace hupr

using namespace hupr;

extern "C" size_t hupr_pose_track_imm_state_bytes(long rows) {
    return rows > 0 ? (size_t)rows * kImmFloats * sizeof(float) : 0;
}

extern "C" int hupr_pose_track_imm_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* state, float rate_hz,
                                       float accel_psd, float meas_std, float heatmap_gain, float gate, int max_coast,
                                       float init_speed_std, float min_score, float horizon_s, float accel_psd_moving, float switch_prob,
                                       float moving_prior, const int* present_or_null, int rows_per_group, int* idx, float* maxval,
                                       float* raw_keypoints, float* keypoints, float* velocity, float* covariance, float* forecast,
                                       int* status, float* moving, hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(heat && state && idx && maxval && raw_keypoints && keypoints && velocity && covariance && forecast && status && moving,
                 "hupr_pose_track_imm_f32: null pointer");
    if (int e = pose_shape("hupr_pose_track_imm_f32", rows, H, W)) return e;
    HUPR_REQUIRE(((uintptr_t)state & 15) == 0, "hupr_pose_track_imm_f32: the state must be 16-byte aligned");
    const Tracker f = {rate_hz, accel_psd, meas_std, heatmap_gain, gate, max_coast, init_speed_std, min_score, horizon_s};
    if (int e = tracker_parameters("hupr_pose_track_imm_f32", f)) return e;
    HUPR_REQUIRE(accel_psd_moving >= accel_psd && accel_psd_moving < INFINITY && switch_prob >= 0.f && switch_prob <= 0.5f &&
                     moving_prior >= 0.f && moving_prior <= 1.f,
                 "hupr_pose_track_imm_f32: bad model parameter (accel_psd_moving %g must be finite and >= accel_psd %g, switch_prob %g in "
                 "[0, 0.5], moving_prior %g in [0, 1])",
                 accel_psd_moving, accel_psd, switch_prob, moving_prior);
    HUPR_REQUIRE(!present_or_null || (rows_per_group >= 1 && rows % rows_per_group == 0),
                 "hupr_pose_track_imm_f32: rows %ld is no multiple of rows_per_group %d", rows, rows_per_group);
    const Imm c = {accel_psd_moving, switch_prob, moving_prior};
    HUPR_LAUNCH(hupr_k_pose_track_imm, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0, state, f,
                c, present_or_null, present_or_null ? rows_per_group : 1, idx, maxval, raw_keypoints, keypoints, velocity, covariance,
                forecast, status, moving);
    HUPR_LAUNCH_OK("hupr_k_pose_track_imm");
    return HUPR_OK;
}
