// Fitting the Kalman tracker's noise parameters by maximum likelihood (Bar-Shalom, Li & Kirubarajan 2001, ch. 5 and 11.6; Abbeel et
// al., "Discriminative Training of Kalman Filters", RSS 2005): the innovations of the filter have a likelihood, and the parameters that
// maximise it over a recording are the fit.  No labels are needed.  Two kernels:
//   * hupr_k_pose_measure: the measurement half of hupr_k_pose_track without a filter — the decode of hupr_k_pose_decode and the
//     window moments, 32 bytes per row and frame, which is all that measurement() (pose_track_model.h) consumes
//   * hupr_k_pose_track_nll: the live tracker's frame (the device functions of pose_track_model.h, in hupr_k_pose_track's order) over a
//     whole recording, one thread per (parameter candidate, row), summing minus twice the log-likelihood of the innovations
// The rules are stated in full beside hupr_pose_measure_f32 and hupr_pose_track_nll_f32 in include/hupr.h; tools/calibrate.py searches.
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"

namespace hupr {

constexpr int kMeasFloats = 8;        // per row and frame: zx, zy, score, m, mxx, mxy, myy, 0

// One wave = one row, as in hupr_k_pose_track up to the measurement.
__global__ __launch_bounds__(64) void hupr_k_pose_measure(const float* __restrict__ heat, int H, int W, float ratio, int refine,
                                                          int* __restrict__ idx, float* __restrict__ maxval, float* __restrict__ raw,
                                                          float* __restrict__ meas) {
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
    float4* m = reinterpret_cast<float4*>(meas + r * kMeasFloats);
    m[0] = make_float4(kp.x, kp.y, best, wm.m);
    m[1] = make_float4(wm.mxx, wm.mxy, wm.myy, 0.f);
}

// A wave = 64 candidates of one row: the record's address depends on the block and the frame alone, so its loads are wave-uniform
// (scalar) and only the candidate's three parameters, its track and its sums are per lane.  Frame t + 1 is fetched under frame t's
// arithmetic.  Registers only: no LDS, no atomics, and every thread adds its costs in frame order.
__global__ __launch_bounds__(64) void hupr_k_pose_track_nll(const float4* __restrict__ meas, const int* __restrict__ start, int T, int rows,
                                                            float ratio, Tracker f, float outlier_cost,
                                                            const float* __restrict__ params, int G, double* __restrict__ nll,
                                                            int* __restrict__ counts, float* __restrict__ final_state) {
    const int row = blockIdx.x;
    const int g = blockIdx.y * 64 + threadIdx.x;
    if (g >= G) return;
    f.accel_psd = params[g * 3 + 0];
    f.meas_std = params[g * 3 + 1];
    f.heatmap_gain = params[g * 3 + 2];

    Track t = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false, 0.f};
    double sum = 0.0;
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0, scored = 0;

    const float4* rec = meas + (long)row * 2;
    const long stride = (long)rows * 2;
    float4 a = rec[0], b = rec[1];
    int fresh = start[0];
    for (int k = 0; k < T; ++k) {
        const float4 ca = a, cb = b;
        const int cfresh = fresh;
        if (k + 1 < T) {
            const float4* next = rec + (long)(k + 1) * stride;
            a = next[0];
            b = next[1];
            fresh = start[k + 1];
        }
        if (cfresh != 0) t = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false, 0.f};
        const WindowMoments wm = {ca.w, cb.x, cb.y, cb.z};
        const Measurement z = measurement(ca.z, ca.x, ca.y, wm, ratio, f);
        int code = HUPR_TRACK_LOST;
        if (t.live) {
            track_predict(t, f);
            const Gate gt = track_gate(t, z);
            if (gt.valid) {
                sum += (double)fminf(gt.d2 + logf(gt.det), outlier_cost);
                ++scored;
            }
            if (gt.valid && gt.d2 <= f.gate) {
                track_update(t, z, gt);
                code = HUPR_TRACK_UPDATED;
            } else {
                code = track_coast(t, f, z.usable ? HUPR_TRACK_COASTED_GATED : HUPR_TRACK_COASTED_MISSING);
            }
        }
        code = track_end(t, z, f, code);
        n0 += code == HUPR_TRACK_UPDATED;
        n1 += code == HUPR_TRACK_COASTED_MISSING;
        n2 += code == HUPR_TRACK_COASTED_GATED;
        n3 += code == HUPR_TRACK_STARTED;
        n4 += code == HUPR_TRACK_LOST;
    }

    const long cell = (long)g * rows + row;
    nll[cell] = sum;
    int* c = counts + cell * 6;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3; c[4] = n4; c[5] = scored;
    if (final_state) {
        float4* s = reinterpret_cast<float4*>(final_state + cell * kTrackFloats);
        s[0] = make_float4(t.x0, t.x1, t.x2, t.x3);
        s[1] = make_float4(t.p00, t.p01, t.p02, t.p03);
        s[2] = make_float4(t.p11, t.p12, t.p13, t.p22);
        s[3] = make_float4(t.p23, t.p33, t.live ? 1.f : 0.f, t.coast);
    }
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_pose_measure_f32(const float* heat, long rows, int H, int W, float ratio, int refine, int* idx, float* maxval,
                                     float* raw_keypoints, float* meas, hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(heat && idx && maxval && raw_keypoints && meas, "hupr_pose_measure_f32: null pointer");
    if (int e = pose_shape("hupr_pose_measure_f32", rows, H, W)) return e;
    HUPR_REQUIRE(((uintptr_t)meas & 15) == 0, "hupr_pose_measure_f32: meas must be 16-byte aligned");
    HUPR_LAUNCH(hupr_k_pose_measure, dim3((unsigned)rows), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0, idx, maxval,
                raw_keypoints, meas);
    HUPR_LAUNCH_OK("hupr_k_pose_measure");
    return HUPR_OK;
}

extern "C" int hupr_pose_track_nll_f32(const float* meas, const int* start, long T, long rows, float ratio, float rate_hz, float gate,
                                       int max_coast, float init_speed_std, float min_score, float outlier_cost, const float* params,
                                       long G, double* nll, int* counts, float* final_state_or_null, hupr_stream_t stream) {
    const char* name = "hupr_pose_track_nll_f32";
    HUPR_REQUIRE(T >= 0 && G >= 0 && rows >= 0 && T < (1L << 31) && rows < (1L << 31) && G <= (1L << 22),
                 "%s: bad shape (T %ld, rows %ld, G %ld; G at most 2^22)", name, T, rows, G);
    if (G == 0 || rows == 0) return HUPR_OK;
    HUPR_REQUIRE(params && nll && counts, "%s: null pointer", name);
    // the shared parameters through the tracker's own check, the candidates' three at values that pass it: those are device memory
    const Tracker f = {rate_hz, 0.f, 1.f, 0.f, gate, max_coast, init_speed_std, min_score, 0.f};
    if (int e = tracker_parameters(name, f)) return e;
    HUPR_REQUIRE(ratio > 0.f && ratio < INFINITY && outlier_cost == outlier_cost, "%s: ratio %g must be positive and finite, outlier_cost %g a number",
                 name, ratio, outlier_cost);
    HUPR_REQUIRE(((uintptr_t)final_state_or_null & 15) == 0, "%s: final_state must be 16-byte aligned", name);
    if (T == 0) {
        const size_t cells = (size_t)G * rows;
        hipError_t e = hipMemsetAsync(nll, 0, cells * sizeof(double), as_stream(stream));
        if (e == hipSuccess) e = hipMemsetAsync(counts, 0, cells * 6 * sizeof(int), as_stream(stream));
        if (e == hipSuccess && final_state_or_null)
            e = hipMemsetAsync(final_state_or_null, 0, cells * kTrackFloats * sizeof(float), as_stream(stream));
        if (e != hipSuccess) return fail(HUPR_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e));
        return HUPR_OK;
    }
    HUPR_REQUIRE(meas && start, "%s: null pointer", name);
    HUPR_REQUIRE(((uintptr_t)meas & 15) == 0, "%s: meas must be 16-byte aligned", name);
    HUPR_LAUNCH(hupr_k_pose_track_nll, dim3((unsigned)rows, (unsigned)((G + 63) / 64)), dim3(64), 0, as_stream(stream),
                reinterpret_cast<const float4*>(meas), start, (int)T, (int)rows, ratio, f, outlier_cost, params, (int)G, nll, counts,
                final_state_or_null);
    HUPR_LAUNCH_OK("hupr_k_pose_track_nll");
    return HUPR_OK;
}
