// Keypoint decode with a constant-velocity Kalman filter per joint: the tracking tail of the live stream.
//   * arg-max, sub-pixel refinement and the keypoint's stores exactly as hupr_k_pose_decode (wave_argmax_row, pose_refine.h): the
//     same index, maximum and raw keypoint, bit for bit
//   * the measurement covariance read off the heat-map: second central moments of the 7 x 7 window around the peak
//   * predict / gate / update of a constant-velocity Kalman filter (Kalman 1960) with the white-acceleration process noise and the
//     chi-square gate of Bar-Shalom, Li & Kirubarajan (2001), its state on the device, so that the filtered pose, its velocity, its
//     covariance and a forecast come out of the same launch — and of the same captured graph — as the decode
// The rule is stated in full beside hupr_pose_track_f32 in include/hupr.h; pose_track_model.h holds what the smoother shares.
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"

namespace hupr {

constexpr int kWindowRadius = 3;      // the covariance window: 7 x 7 pixels around the peak, clipped to the map
constexpr int kWindowSide = 2 * kWindowRadius + 1;

struct Tracker {
    float rate, accel_psd, meas_std, heatmap_gain, gate;
    int max_coast;
    float init_speed_std, min_score, horizon;
};

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

    // ---- window moments: lane k < 49 holds pixel (px + k % 7 - 3, py + k / 7 - 3), weight max(h, 0); a NaN weighs 0 -------------------
    const int wx = lane % kWindowSide - kWindowRadius, wy = lane / kWindowSide - kWindowRadius;
    const int gx = px + wx, gy = py + wy;
    float w = 0.f;
    if (positive && lane < kWindowSide * kWindowSide && gx >= 0 && gx < W && gy >= 0 && gy < H) w = fmaxf(row[(long)gy * W + gx], 0.f);
    const float fx = (float)wx, fy = (float)wy;
    const float m = wave_sum(w);
    const float cx = wave_sum(w * fx) / m, cy = wave_sum(w * fy) / m;
    const float ex = fx - cx, ey = fy - cy;
    const float mxx = wave_sum(w * ex * ex) / m, mxy = wave_sum(w * ex * ey) / m, myy = wave_sum(w * ey * ey) / m;
    if (lane != 0) return;

    const float2 z = store_keypoint(r, bi, best, px, py, ox, oy, positive, ratio, idx, maxval, raw);
    const float zx = z.x, zy = z.y;

    // ---- measurement noise and whether there is a measurement at all --------------------------------------------------------------
    const float gain = ratio * ratio * f.heatmap_gain, floor2 = f.meas_std * f.meas_std;
    const float r00 = gain * mxx + floor2, r01 = gain * mxy, r11 = gain * myy + floor2;
    const bool usable = best > f.min_score && finitef(zx) && finitef(zy) && m > 0.f && finitef(r00) && finitef(r01) && finitef(r11);

    float4* s = reinterpret_cast<float4*>(state + r * kTrackFloats);
    const float4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
    float x0 = s0.x, x1 = s0.y, x2 = s0.z, x3 = s0.w;                                  // x, y, vx, vy
    float p00 = s1.x, p01 = s1.y, p02 = s1.z, p03 = s1.w, p11 = s2.x, p12 = s2.y, p13 = s2.z, p22 = s2.w, p23 = s3.x, p33 = s3.y;
    bool live = s3.z != 0.f;
    float coast = s3.w;
    int code = HUPR_TRACK_LOST;

    if (live) {
        // ---- predict: x- = F x, P- = F P F^T + Q ------------------------------------------------------------------------------------
        const float dt = 1.f / f.rate;
        const ProcessNoise q = process_noise(f.accel_psd, dt);
        x0 += dt * x2;
        x1 += dt * x3;
        p00 += dt * (2.f * p02) + dt * dt * p22 + q.q11;
        p01 += dt * (p03 + p12) + dt * dt * p23;
        p11 += dt * (2.f * p13) + dt * dt * p33 + q.q11;
        p02 += dt * p22 + q.q12;
        p03 += dt * p23;
        p12 += dt * p23;
        p13 += dt * p33 + q.q12;
        p22 += q.q22;
        p33 += q.q22;

        // ---- gate: d2 = nu^T S^-1 nu through the closed-form 2 x 2 inverse ----------------------------------------------------------------
        bool accepted = false;
        float nx = 0.f, ny = 0.f, i00 = 0.f, i01 = 0.f, i11 = 0.f;
        if (usable) {
            nx = zx - x0;
            ny = zy - x1;
            const float a00 = p00 + r00, a01 = p01 + r01, a11 = p11 + r11;
            const float det = a00 * a11 - a01 * a01;
            if (det > 0.f && finitef(det)) {
                i00 = a11 / det;
                i01 = -a01 / det;
                i11 = a00 / det;
                const float d2 = nx * nx * i00 + 2.f * (nx * ny * i01) + ny * ny * i11;
                accepted = d2 <= f.gate;
            }
        }
        if (accepted) {
            // ---- update: K = P- H^T S^-1, Joseph form, symmetrised ---------------------------------------------------------------------
            const float p10 = p01, p20 = p02, p21 = p12, p30 = p03, p31 = p13, p32 = p23;
            const float k00 = p00 * i00 + p01 * i01, k01 = p00 * i01 + p01 * i11;
            const float k10 = p10 * i00 + p11 * i01, k11 = p10 * i01 + p11 * i11;
            const float k20 = p20 * i00 + p21 * i01, k21 = p20 * i01 + p21 * i11;
            const float k30 = p30 * i00 + p31 * i01, k31 = p30 * i01 + p31 * i11;
            x0 += k00 * nx + k01 * ny;
            x1 += k10 * nx + k11 * ny;
            x2 += k20 * nx + k21 * ny;
            x3 += k30 * nx + k31 * ny;
            // t = (I - K H) P-;  n = t (I - K H)^T + K R K^T
#define HUPR_T(i, j) const float t##i##j = p##i##j - k##i##0 * p0##j - k##i##1 * p1##j;
#define HUPR_N(i, j)                                                                                                  \
    const float n##i##j = t##i##j - t##i##0 * k##j##0 - t##i##1 * k##j##1 + k##i##0 * (r00 * k##j##0 + r01 * k##j##1) + \
                          k##i##1 * (r01 * k##j##0 + r11 * k##j##1);
#define HUPR_ROWS(M) M(0, 0) M(0, 1) M(0, 2) M(0, 3) M(1, 0) M(1, 1) M(1, 2) M(1, 3) M(2, 0) M(2, 1) M(2, 2) M(2, 3) M(3, 0) M(3, 1) M(3, 2) M(3, 3)
            HUPR_ROWS(HUPR_T)
            HUPR_ROWS(HUPR_N)
#undef HUPR_ROWS
#undef HUPR_N
#undef HUPR_T
            p00 = n00;
            p11 = n11;
            p22 = n22;
            p33 = n33;
            p01 = 0.5f * (n01 + n10);
            p02 = 0.5f * (n02 + n20);
            p03 = 0.5f * (n03 + n30);
            p12 = 0.5f * (n12 + n21);
            p13 = 0.5f * (n13 + n31);
            p23 = 0.5f * (n23 + n32);
            coast = 0.f;
            code = HUPR_TRACK_UPDATED;
        } else if (coast + 1.f > (float)f.max_coast) {
            live = false;                                                              // the track ends; a usable sample starts the next
        } else {
            coast += 1.f;
            code = usable ? HUPR_TRACK_COASTED_GATED : HUPR_TRACK_COASTED_MISSING;
        }
    }
    if (!live) {
        if (usable) {
            x0 = zx; x1 = zy; x2 = 0.f; x3 = 0.f;
            p00 = r00; p01 = r01; p11 = r11;
            p22 = p33 = f.init_speed_std * f.init_speed_std;
            p02 = p03 = p12 = p13 = p23 = 0.f;
            live = true;
            code = HUPR_TRACK_STARTED;
        } else {
            x0 = x1 = x2 = x3 = 0.f;
            p00 = p01 = p02 = p03 = p11 = p12 = p13 = p22 = p23 = p33 = 0.f;
        }
        coast = 0.f;
    }
    s[0] = make_float4(x0, x1, x2, x3);
    s[1] = make_float4(p00, p01, p02, p03);
    s[2] = make_float4(p11, p12, p13, p22);
    s[3] = make_float4(p23, p33, live ? 1.f : 0.f, coast);

    const float kx = live ? x0 : zx, ky = live ? x1 : zy;                              // LOST: the raw keypoint, nothing else
    *reinterpret_cast<float2*>(filtered + r * 2) = make_float2(kx, ky);
    *reinterpret_cast<float2*>(velocity + r * 2) = make_float2(x2, x3);
    covariance[r * 3 + 0] = p00;
    covariance[r * 3 + 1] = p01;
    covariance[r * 3 + 2] = p11;
    *reinterpret_cast<float2*>(forecast + r * 2) = make_float2(kx + x2 * f.horizon, ky + x3 * f.horizon);
    status[r] = code;
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
    HUPR_REQUIRE(rate_hz > 0.f && rate_hz < INFINITY && meas_std > 0.f && meas_std < INFINITY && gate > 0.f && gate < INFINITY &&
                     init_speed_std > 0.f && init_speed_std < INFINITY && accel_psd >= 0.f && accel_psd < INFINITY &&
                     heatmap_gain >= 0.f && heatmap_gain < INFINITY && horizon_s >= 0.f && horizon_s < INFINITY && max_coast >= 0 &&
                     min_score == min_score,
                 "hupr_pose_track_f32: bad tracker parameter (rate_hz %g, meas_std %g, gate %g and init_speed_std %g must be positive, "
                 "accel_psd %g, heatmap_gain %g, horizon_s %g and max_coast %d non-negative, min_score %g a number)",
                 rate_hz, meas_std, gate, init_speed_std, accel_psd, heatmap_gain, horizon_s, max_coast, min_score);
    const Tracker f = {rate_hz, accel_psd, meas_std, heatmap_gain, gate, max_coast, init_speed_std, min_score, horizon_s};
    HUPR_LAUNCH(hupr_k_pose_track, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0, state, f,
                idx, maxval, raw_keypoints, keypoints, velocity, covariance, forecast, status);
    HUPR_LAUNCH_OK("hupr_k_pose_track");
    return HUPR_OK;
}
