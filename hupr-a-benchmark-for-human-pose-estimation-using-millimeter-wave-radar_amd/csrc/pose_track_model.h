// The constant-velocity model shared by the Kalman tracker (pose_track.hip), the tracker that picks its measurement among several
// heat-map peaks (pose_assoc.hip), the one that assigns left / right partner rows jointly (pose_pairs.hip) and the Rauch-Tung-Striebel
// smoother that runs backwards over their recorded states (pose_smooth.hip).  The status codes are the HUPR_TRACK_* / HUPR_SMOOTH_*
// of include/hupr.h.  The trackers share one statement of the filter: the measurement read off the heat-map, predict, gate, Joseph
// update, the end of the frame and its stores.  The likelihood
// kernel behind tools/calibrate.py (pose_fit.hip) runs the same frame for many parameter candidates at once.
#pragma once
#include "hupr_common.h"
#include "pose_refine.h"

namespace hupr {

constexpr int kTrackFloats = 16;      // per row: x, y, vx, vy, the 10 upper-triangle entries of P (row-major), live, coast

// white-acceleration process noise of one frame of dt seconds: per axis [[q11, q12], [q12, q22]] on (position, velocity)
struct ProcessNoise {
    float q11, q12, q22;
};
__device__ __forceinline__ ProcessNoise process_noise(float accel_psd, float dt) {
    return {accel_psd * dt * dt * dt * (1.f / 3.f), accel_psd * dt * dt * 0.5f, accel_psd * dt};
}

constexpr int kWindowRadius = 3;      // the covariance window: 7 x 7 pixels around the peak, clipped to the map
constexpr int kWindowSide = 2 * kWindowRadius + 1;

struct Tracker {
    float rate, accel_psd, meas_std, heatmap_gain, gate;
    int max_coast;
    float init_speed_std, min_score, horizon;
};

// the entries' check of the nine tracker parameters, in ``name``'s name
static inline int tracker_parameters(const char* name, const Tracker& f) {
    HUPR_REQUIRE(f.rate > 0.f && f.rate < INFINITY && f.meas_std > 0.f && f.meas_std < INFINITY && f.gate > 0.f && f.gate < INFINITY &&
                     f.init_speed_std > 0.f && f.init_speed_std < INFINITY && f.accel_psd >= 0.f && f.accel_psd < INFINITY &&
                     f.heatmap_gain >= 0.f && f.heatmap_gain < INFINITY && f.horizon >= 0.f && f.horizon < INFINITY && f.max_coast >= 0 &&
                     f.min_score == f.min_score,
                 "%s: bad tracker parameter (rate_hz %g, meas_std %g, gate %g and init_speed_std %g must be positive, "
                 "accel_psd %g, heatmap_gain %g, horizon_s %g and max_coast %d non-negative, min_score %g a number)",
                 name, f.rate, f.meas_std, f.gate, f.init_speed_std, f.accel_psd, f.heatmap_gain, f.horizon, f.max_coast, f.min_score);
    return HUPR_OK;
}

// Mass and second central moments of max(h, 0) over the 7 x 7 window around pixel (px, py) of ``row`` (H x W), clipped to the map, in
// window-relative coordinates; a NaN weighs 0, and without ``positive`` every weight is 0 (mass 0, NaN moments).  Called by the whole
// wave: lane k < 49 holds pixel (px + k % 7 - 3, py + k / 7 - 3); every lane ends with the same sums.
struct WindowMoments {
    float m, mxx, mxy, myy;
};
__device__ __forceinline__ WindowMoments window_moments(const float* row, int H, int W, int px, int py, bool positive, int lane) {
    const int wx = lane % kWindowSide - kWindowRadius, wy = lane / kWindowSide - kWindowRadius;
    const int gx = px + wx, gy = py + wy;
    float w = 0.f;
    if (positive && lane < kWindowSide * kWindowSide && gx >= 0 && gx < W && gy >= 0 && gy < H) w = fmaxf(row[(long)gy * W + gx], 0.f);
    const float fx = (float)wx, fy = (float)wy;
    const float m = wave_sum(w);
    const float cx = wave_sum(w * fx) / m, cy = wave_sum(w * fy) / m;
    const float ex = fx - cx, ey = fy - cy;
    return {m, wave_sum(w * ex * ex) / m, wave_sum(w * ex * ey) / m, wave_sum(w * ey * ey) / m};
}

// The filter's arithmetic below is written with its fused multiply-adds spelled out and the compiler's own contraction switched off:
// which products the compiler fuses depends on the code around an expression (it moved with the kernel's block structure), and the
// two trackers must agree bit for bit wherever they see the same measurement.  The fusions spelled out are the ones hupr_k_pose_track
// has always computed with.
#define HUPR_EXACT_FP _Pragma("clang fp contract(off)")

// One measurement: the keypoint z in image pixels, its covariance R = ratio^2 heatmap_gain S + meas_std^2 I, and whether it counts.
struct Measurement {
    float zx, zy, r00, r01, r11;
    bool usable;
};
__device__ __forceinline__ Measurement measurement(float score, float zx, float zy, const WindowMoments& w, float ratio, const Tracker& f) {
    HUPR_EXACT_FP
    const float gain = ratio * ratio * f.heatmap_gain, floor2 = f.meas_std * f.meas_std;
    const float r00 = fmaf(gain, w.mxx, floor2), r01 = gain * w.mxy, r11 = fmaf(gain, w.myy, floor2);
    const bool usable = score > f.min_score && finitef(zx) && finitef(zy) && w.m > 0.f && finitef(r00) && finitef(r01) && finitef(r11);
    return {zx, zy, r00, r01, r11, usable};
}

// The state of one row, in the layout of kTrackFloats.
struct Track {
    float x0, x1, x2, x3;                                                              // x, y, vx, vy
    float p00, p01, p02, p03, p11, p12, p13, p22, p23, p33;
    bool live;
    float coast;
};
__device__ __forceinline__ Track load_track(const float* state, long r) {
    const float4* s = reinterpret_cast<const float4*>(state + r * kTrackFloats);
    const float4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
    return {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y, s3.z != 0.f, s3.w};
}

// predict: x- = F x, P- = F P F^T + Q
__device__ __forceinline__ void track_predict(Track& t, const Tracker& f) {
    HUPR_EXACT_FP
    const float dt = 1.f / f.rate, dt2 = dt * dt;
    // process_noise(accel_psd, dt): q11 = a3 / 3 and q22 = accel_psd dt enter through the multiply-adds, q12 is rounded by itself
    const float a2 = f.accel_psd * dt * dt, a3 = a2 * dt, third = 1.f / 3.f, q12 = a2 * 0.5f;
    t.x0 = fmaf(dt, t.x2, t.x0);
    t.x1 = fmaf(dt, t.x3, t.x1);
    t.p00 += fmaf(a3, third, fmaf(dt, 2.f * t.p02, dt2 * t.p22));
    t.p01 += fmaf(dt, t.p03 + t.p12, dt2 * t.p23);
    t.p11 += fmaf(a3, third, fmaf(dt, 2.f * t.p13, dt2 * t.p33));
    t.p02 += fmaf(dt, t.p22, q12);
    t.p03 = fmaf(dt, t.p23, t.p03);
    t.p12 = fmaf(dt, t.p23, t.p12);
    t.p13 += fmaf(dt, t.p33, q12);
    t.p22 = fmaf(f.accel_psd, dt, t.p22);
    t.p33 = fmaf(f.accel_psd, dt, t.p33);
}

// gate: the innovation nu, S^-1 through the closed-form 2 x 2 inverse, d2 = nu^T S^-1 nu and det S of a usable measurement against the
// predicted track; ``valid`` iff det S > 0 and finite (everything else is 0 otherwise)
struct Gate {
    float nx, ny, i00, i01, i11, d2, det;
    bool valid;
};
__device__ __forceinline__ Gate track_gate(const Track& t, const Measurement& z) {
    HUPR_EXACT_FP
    Gate g = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
    if (z.usable) {
        g.nx = z.zx - t.x0;
        g.ny = z.zy - t.x1;
        const float a00 = t.p00 + z.r00, a01 = t.p01 + z.r01, a11 = t.p11 + z.r11;
        const float det = fmaf(a00, a11, -(a01 * a01));
        if (det > 0.f && finitef(det)) {
            g.i00 = a11 / det;
            g.i01 = -a01 / det;
            g.i11 = a00 / det;
            g.d2 = fmaf(g.ny * g.ny, g.i11, fmaf(g.nx * g.nx, g.i00, 2.f * (g.nx * g.ny * g.i01)));
            g.det = det;
            g.valid = true;
        }
    }
    return g;
}

// update: K = P- H^T S^-1, Joseph form, symmetrised; coast = 0
__device__ __forceinline__ void track_update(Track& t, const Measurement& z, const Gate& g) {
    HUPR_EXACT_FP
    const float p00 = t.p00, p01 = t.p01, p02 = t.p02, p03 = t.p03, p11 = t.p11, p12 = t.p12, p13 = t.p13, p22 = t.p22, p23 = t.p23,
                p33 = t.p33;
    const float r00 = z.r00, r01 = z.r01, r11 = z.r11, i00 = g.i00, i01 = g.i01, i11 = g.i11, nx = g.nx, ny = g.ny;
    const float p10 = p01, p20 = p02, p21 = p12, p30 = p03, p31 = p13, p32 = p23;
    const float p01i01 = p01 * i01;                                                    // shared by k00 and k11
    const float k00 = fmaf(p00, i00, p01i01), k01 = fmaf(p00, i01, p01 * i11);
    const float k10 = fmaf(p10, i00, p11 * i01), k11 = fmaf(p11, i11, p01i01);
    const float k20 = fmaf(p20, i00, p21 * i01), k21 = fmaf(p20, i01, p21 * i11);
    const float k30 = fmaf(p30, i00, p31 * i01), k31 = fmaf(p30, i01, p31 * i11);
    t.x0 += fmaf(k00, nx, k01 * ny);
    t.x1 += fmaf(k10, nx, k11 * ny);
    t.x2 += fmaf(k20, nx, k21 * ny);
    t.x3 += fmaf(k30, nx, k31 * ny);
    // t = (I - K H) P-;  n = t (I - K H)^T + K R K^T
#define HUPR_T(i, j) const float t##i##j = fmaf(-k##i##1, p1##j, fmaf(-k##i##0, p0##j, p##i##j));
#define HUPR_N(i, j)                                                                                                  \
    const float n##i##j = fmaf(k##i##1, fmaf(r01, k##j##0, r11 * k##j##1),                                            \
                               fmaf(k##i##0, fmaf(r00, k##j##0, r01 * k##j##1),                                       \
                                    fmaf(-t##i##1, k##j##1, fmaf(-t##i##0, k##j##0, t##i##j))));
#define HUPR_ROWS(M) M(0, 0) M(0, 1) M(0, 2) M(0, 3) M(1, 0) M(1, 1) M(1, 2) M(1, 3) M(2, 0) M(2, 1) M(2, 2) M(2, 3) M(3, 0) M(3, 1) M(3, 2) M(3, 3)
    HUPR_ROWS(HUPR_T)
    HUPR_ROWS(HUPR_N)
#undef HUPR_ROWS
#undef HUPR_N
#undef HUPR_T
    t.p00 = n00;
    t.p11 = n11;
    t.p22 = n22;
    t.p33 = n33;
    t.p01 = 0.5f * (n01 + n10);
    t.p02 = 0.5f * (n02 + n20);
    t.p03 = 0.5f * (n03 + n30);
    t.p12 = 0.5f * (n12 + n21);
    t.p13 = 0.5f * (n13 + n31);
    t.p23 = 0.5f * (n23 + n32);
    t.coast = 0.f;
}

// A live track that got no measurement this frame coasts, or ends once it would coast for the (max_coast + 1)-th frame in a row.
// -> the status of a track that coasts (``coasted``); a track that ends leaves HUPR_TRACK_LOST for track_finish to replace.
__device__ __forceinline__ int track_coast(Track& t, const Tracker& f, int coasted) {
    if (t.coast + 1.f > (float)f.max_coast) {
        t.live = false;                                                                // the track ends; a usable sample starts the next
        return HUPR_TRACK_LOST;
    }
    t.coast += 1.f;
    return coasted;
}

// The end of the frame's state logic: a row without a live track starts one from ``z`` if that is usable, else its state is all zero.
// ``code`` is the status so far (HUPR_TRACK_LOST without a live track); -> the frame's status.  Nothing is stored: the likelihood
// kernel (pose_fit.hip) runs the frame on registers alone.
__device__ __forceinline__ int track_end(Track& t, const Measurement& z, const Tracker& f, int code) {
    HUPR_EXACT_FP
    if (!t.live) {
        if (z.usable) {
            t.x0 = z.zx; t.x1 = z.zy; t.x2 = 0.f; t.x3 = 0.f;
            t.p00 = z.r00; t.p01 = z.r01; t.p11 = z.r11;
            t.p22 = t.p33 = f.init_speed_std * f.init_speed_std;
            t.p02 = t.p03 = t.p12 = t.p13 = t.p23 = 0.f;
            t.live = true;
            code = HUPR_TRACK_STARTED;
        } else {
            t.x0 = t.x1 = t.x2 = t.x3 = 0.f;
            t.p00 = t.p01 = t.p02 = t.p03 = t.p11 = t.p12 = t.p13 = t.p22 = t.p23 = t.p33 = 0.f;
        }
        t.coast = 0.f;
    }
    return code;
}

// The end of the frame, by one lane: ``track_end``, then the state and the five outputs of row r are stored.  -> the status stored.
__device__ __forceinline__ int track_finish(Track& t, const Measurement& z, const Tracker& f, int code, long r, float* state, float* filtered,
                                             float* velocity, float* covariance, float* forecast, int* status) {
    HUPR_EXACT_FP
    code = track_end(t, z, f, code);
    float4* s = reinterpret_cast<float4*>(state + r * kTrackFloats);
    s[0] = make_float4(t.x0, t.x1, t.x2, t.x3);
    s[1] = make_float4(t.p00, t.p01, t.p02, t.p03);
    s[2] = make_float4(t.p11, t.p12, t.p13, t.p22);
    s[3] = make_float4(t.p23, t.p33, t.live ? 1.f : 0.f, t.coast);

    const float kx = t.live ? t.x0 : z.zx, ky = t.live ? t.x1 : z.zy;                  // LOST: the raw keypoint, nothing else
    *reinterpret_cast<float2*>(filtered + r * 2) = make_float2(kx, ky);
    *reinterpret_cast<float2*>(velocity + r * 2) = make_float2(t.x2, t.x3);
    covariance[r * 3 + 0] = t.p00;
    covariance[r * 3 + 1] = t.p01;
    covariance[r * 3 + 2] = t.p11;
    *reinterpret_cast<float2*>(forecast + r * 2) = make_float2(fmaf(t.x2, f.horizon, kx), fmaf(t.x3, f.horizon, ky));
    status[r] = code;
    return code;
}

}  // namespace hupr
