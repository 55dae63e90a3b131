// The associating Kalman joint tracker of pose_assoc.hip with the left / right partners of a skeleton resolved together: the network's
// best-known mistake is to exchange a left and a right limb, and then the peak a track needs stands in its partner's heat-map.  Two
// partner rows form one unit; their candidates go into one pool of at most 2 K measurements, and the two tracks share it by global
// nearest neighbour (Blackman 1986): the assignment that updates the most tracks, then the smallest summed cost, no measurement twice.
//   * the candidates of a map, their refinement and covariance are those of hupr_k_pose_track_assoc (the same masked arg-max rounds)
//   * predict, gate, Joseph update, coasting and the stores are the tracker's own functions (pose_track_model.h)
//   * one 64-lane wave owns a unit and with it both rows' states, which advance in place; lane 0 runs the recurrence
//   * the pool lives in LDS (lane 0 writes and reads it), so nothing is indexed dynamically in registers: no scratch
// With every joint its own partner the kernel computes hupr_pose_track_assoc_f32's bits.  The rule is stated in full beside
// hupr_pose_track_pairs_f32 in include/hupr.h.
#include "hupr_common.h"
#include "pose_refine.h"
#include "pose_track_model.h"

namespace hupr {

constexpr int kMaxCandidates = 4;                         // per map, as in pose_assoc.hip
constexpr int kMaxPool = 2 * kMaxCandidates;
constexpr int kMaxGroupRows = 32;

struct Peaks {
    int K, min_separation;
    float peak_ratio;
};

// The units of one group, by value in the launch arguments: unit u owns row a[u] of its group and, where b[u] >= 0, its partner b[u].
struct PairTable {
    int units;
    signed char a[kMaxGroupRows], b[kMaxGroupRows];
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

// the pool in LDS: per entry (zx, zy, r00, r01, r11, usable)
constexpr int kEntryFloats = 6;
__device__ __forceinline__ void put_entry(float* pool, int e, const Measurement& z) {
    float* p = pool + e * kEntryFloats;
    p[0] = z.zx; p[1] = z.zy; p[2] = z.r00; p[3] = z.r01; p[4] = z.r11; p[5] = z.usable ? 1.f : 0.f;
}
__device__ __forceinline__ Measurement get_entry(const float* pool, int e) {
    const float* p = pool + e * kEntryFloats;
    return {p[0], p[1], p[2], p[3], p[4], p[5] != 0.f};
}

// By the whole wave: the candidates of row r (hupr_k_pose_track_assoc's, round for round), its decode and its four candidate outputs
// stored, its K pool entries from ``base`` on written by lane 0 (the slots past the count not usable).  -> lane 0's ``z0``: candidate
// 0's measurement, or the (0, 0) of a non-positive maximum, which is not usable.
__device__ __forceinline__ void row_candidates(const float* __restrict__ heat, long r, int H, int W, float ratio, int refine,
                                               const Tracker& f, const Peaks& c, bool seen, int lane, float* pool, int base,
                                               Measurement& z0, int* __restrict__ idx, float* __restrict__ maxval,
                                               float* __restrict__ raw, float* __restrict__ cand_xy, float* __restrict__ cand_score,
                                               int* __restrict__ cand_count) {
    const long n = (long)H * W;
    const float* row = heat + r * n;
    float best;
    int bi;
    wave_argmax_row(row, (int)n, lane, best, bi);
    const bool positive = best > 0.f;                     // implies 0 <= bi < H * W
    const float floor_v = c.peak_ratio * best;

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
        const WindowMoments wm = window_moments(row, H, W, px, py, true, lane);
        if (lane == 0) {
            float2 kp;
            if (k == 0) kp = store_keypoint(r, bi, best, px, py, ox, oy, true, ratio, idx, maxval, raw);
            else kp = make_float2(((float)px + ox) * ratio, ((float)py + oy) * ratio);
            *reinterpret_cast<float2*>(cand_xy + (r * c.K + k) * 2) = kp;
            cand_score[r * c.K + k] = pv;
            Measurement z = measurement(pv, kp.x, kp.y, wm, ratio, f);
            z.usable = z.usable && seen;
            if (k == 0) z0 = z;
            put_entry(pool, base + k, z);
        }
    }
    if (lane != 0) return;

    const Measurement hole = {0.f, 0.f, 0.f, 0.f, 0.f, false};
#pragma unroll
    for (int k = 0; k < kMaxCandidates; ++k) {
        if (k < c.K && k >= count) {                                                   // slots past the count hold zeros
            *reinterpret_cast<float2*>(cand_xy + (r * c.K + k) * 2) = make_float2(0.f, 0.f);
            cand_score[r * c.K + k] = 0.f;
            put_entry(pool, base + k, hole);
        }
    }
    cand_count[r] = count;
    if (!positive) {                                      // no candidate: the tracker's decode of a non-positive maximum, (0, 0), not usable
        const WindowMoments none = {0.f, 0.f, 0.f, 0.f};
        const float2 kp = store_keypoint(r, bi, best, bi % W, bi / W, 0.f, 0.f, false, ratio, idx, maxval, raw);
        z0 = measurement(best, kp.x, kp.y, none, ratio, f);
    }
}

// Lane 0: the costs of the ``n`` pool entries for the predicted track ``t`` into cost[0 .. n): d2 + ln det S of an admissible entry,
// plus ``swap_cost`` for the entries of the other row's map, [other, other + K); INFINITY for every other entry.
__device__ __forceinline__ void entry_costs(const Track& t, const Tracker& f, const float* pool, int n, int other, int K, float swap_cost,
                                            float* cost) {
    for (int e = 0; e < n; ++e) {
        float ce = INFINITY;
        if (t.live) {
            const Gate g = track_gate(t, get_entry(pool, e));
            if (g.valid && g.d2 <= f.gate) {
                ce = g.d2 + logf(g.det);
                if (e >= other && e < other + K) ce += swap_cost;
            }
        }
        cost[e] = ce;
    }
}

// Lane 0: the rest of the frame for one row, after the assignment gave its live track pool entry ``e`` (``n``: none).
__device__ __forceinline__ void row_finish(Track& t, Measurement z0, bool z0_taken, int e, int n, int own, int K, bool any_usable,
                                           const Tracker& f, const float* pool, long r, float* state, float* filtered, float* velocity,
                                           float* covariance, float* forecast, int* status, int* chosen, int* source) {
    int code = HUPR_TRACK_LOST;
    if (t.live) {
        if (e < n) {
            const Measurement z = get_entry(pool, e);
            track_update(t, z, track_gate(t, z));
            code = HUPR_TRACK_UPDATED;
        } else {
            code = track_coast(t, f, any_usable ? HUPR_TRACK_COASTED_GATED : HUPR_TRACK_COASTED_MISSING);
        }
    }
    z0.usable = z0.usable && !z0_taken;                   // a measurement that went into a track this frame starts no second one
    code = track_finish(t, z0, f, code, r, state, filtered, velocity, covariance, forecast, status);
    const bool mine = e >= own && e < own + K;
    chosen[r] = code == HUPR_TRACK_UPDATED ? (e >= K ? e - K : e) : (code == HUPR_TRACK_STARTED ? 0 : -1);
    source[r] = code == HUPR_TRACK_UPDATED ? (mine ? 0 : 1) : (code == HUPR_TRACK_STARTED ? 0 : -1);
}

// One wave = one unit.  Nothing is shared between workgroups, nothing is accumulated in memory: the same maps give the same bits.
__global__ __launch_bounds__(64) void hupr_k_pose_track_pairs(const float* __restrict__ heat, int H, int W, float ratio, int refine,
                                                              float* __restrict__ state, Tracker f, Peaks c,
                                                              const int* __restrict__ present, int rows_per_group, PairTable table,
                                                              float swap_cost, int* __restrict__ idx, float* __restrict__ maxval,
                                                              float* __restrict__ raw, float* __restrict__ filtered,
                                                              float* __restrict__ velocity, float* __restrict__ covariance,
                                                              float* __restrict__ forecast, int* __restrict__ status,
                                                              float* __restrict__ cand_xy, float* __restrict__ cand_score,
                                                              int* __restrict__ cand_count, int* __restrict__ chosen,
                                                              int* __restrict__ source) {
    __shared__ float pool[kMaxPool * kEntryFloats];
    __shared__ float cost_a[kMaxPool], cost_b[kMaxPool];
    const long group = blockIdx.x / table.units;
    const int u = blockIdx.x % table.units;
    const int lane = threadIdx.x;
    const long ra = group * rows_per_group + table.a[u];
    const bool paired = table.b[u] >= 0;
    const long rb = group * rows_per_group + (paired ? table.b[u] : table.a[u]);
    const bool seen = present == nullptr || present[group] != 0;
    const int K = c.K, n = paired ? 2 * K : K;             // the pool: a's candidates in [0, K), b's in [K, 2 K)

    Measurement za = {}, zb = {};
    row_candidates(heat, ra, H, W, ratio, refine, f, c, seen, lane, pool, 0, za, idx, maxval, raw, cand_xy, cand_score, cand_count);
    if (paired)
        row_candidates(heat, rb, H, W, ratio, refine, f, c, seen, lane, pool, K, zb, idx, maxval, raw, cand_xy, cand_score, cand_count);
    if (lane != 0) return;

    Track ta = load_track(state, ra), tb = {};
    if (ta.live) track_predict(ta, f);
    if (paired) {
        tb = load_track(state, rb);
        if (tb.live) track_predict(tb, f);
    }
    bool any_usable = false;
    for (int e = 0; e < n; ++e) any_usable = any_usable || pool[e * kEntryFloats + 5] != 0.f;
    entry_costs(ta, f, pool, n, K, K, swap_cost, cost_a);
    entry_costs(tb, f, pool, n, 0, K, swap_cost, cost_b);

    // ---- assignment: most tracks updated, then the smallest c_a + c_b; walked in the order (entry of a, entry of b) with "none" = n
    // last and only a strictly better one taken, so a tie stays with the lexicographically smaller pair ------------------------------------
    int ea = n, eb = n, most = -1;
    float least = INFINITY;
    for (int ia = 0; ia <= n; ++ia) {
        const float ca = ia < n ? cost_a[ia] : 0.f;
        if (!(ca < INFINITY)) continue;
        for (int ib = 0; ib <= n; ++ib) {
            const float cb = ib < n ? cost_b[ib] : 0.f;
            if (!(cb < INFINITY) || (ia == ib && ia < n)) continue;
            const int tracks = (ia < n ? 1 : 0) + (ib < n ? 1 : 0);
            const float sum = ca + cb;
            if (tracks > most || (tracks == most && sum < least)) { most = tracks; least = sum; ea = ia; eb = ib; }
        }
    }

    const bool a0_taken = ea == 0 || eb == 0, b0_taken = ea == K || eb == K;
    row_finish(ta, za, a0_taken, ea, n, 0, K, any_usable, f, pool, ra, state, filtered, velocity, covariance, forecast, status, chosen,
               source);
    if (paired)
        row_finish(tb, zb, b0_taken, eb, n, K, K, any_usable, f, pool, rb, state, filtered, velocity, covariance, forecast, status, chosen,
                   source);
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_pose_track_pairs_f32(const float* heat, long rows, int H, int W, float ratio, int refine, float* state, float rate_hz,
                                         float accel_psd, float meas_std, float heatmap_gain, float gate, int max_coast,
                                         float init_speed_std, float min_score, float horizon_s, int K, int min_separation,
                                         float peak_ratio, const int* present_or_null, int rows_per_group, const int* partner_host,
                                         float swap_cost, int* idx, float* maxval, float* raw_keypoints, float* keypoints, float* velocity,
                                         float* covariance, float* forecast, int* status, float* cand_xy, float* cand_score,
                                         int* cand_count, int* chosen, int* source, hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(heat && state && partner_host && idx && maxval && raw_keypoints && keypoints && velocity && covariance && forecast &&
                     status && cand_xy && cand_score && cand_count && chosen && source,
                 "hupr_pose_track_pairs_f32: null pointer");
    if (int e = pose_shape("hupr_pose_track_pairs_f32", rows, H, W)) return e;
    HUPR_REQUIRE(((uintptr_t)state & 15) == 0, "hupr_pose_track_pairs_f32: the state must be 16-byte aligned");
    const Tracker f = {rate_hz, accel_psd, meas_std, heatmap_gain, gate, max_coast, init_speed_std, min_score, horizon_s};
    if (int e = tracker_parameters("hupr_pose_track_pairs_f32", f)) return e;
    HUPR_REQUIRE(K >= 1 && K <= kMaxCandidates && min_separation >= 0 && peak_ratio > 0.f && peak_ratio <= 1.f,
                 "hupr_pose_track_pairs_f32: bad candidate parameter (K %d must be in 1..%d, min_separation %d non-negative, peak_ratio %g "
                 "in (0, 1])", K, kMaxCandidates, min_separation, peak_ratio);
    HUPR_REQUIRE(rows_per_group >= 1 && rows_per_group <= kMaxGroupRows && rows % rows_per_group == 0,
                 "hupr_pose_track_pairs_f32: rows_per_group %d must be in 1..%d and divide rows %ld", rows_per_group, kMaxGroupRows, rows);
    HUPR_REQUIRE(swap_cost >= 0.f && swap_cost < INFINITY, "hupr_pose_track_pairs_f32: swap_cost %g must be finite and not negative",
                 swap_cost);
    PairTable table = {};
    for (int j = 0; j < rows_per_group; ++j) {
        const int q = partner_host[j];
        HUPR_REQUIRE(q >= 0 && q < rows_per_group && partner_host[q] == j,
                     "hupr_pose_track_pairs_f32: partner[%d] = %d: the partner table must map 0..%d onto itself and be its own inverse", j, q,
                     rows_per_group - 1);
        if (q >= j) {
            table.a[table.units] = (signed char)j;
            table.b[table.units] = (signed char)(q > j ? q : -1);
            ++table.units;
        }
    }
    const Peaks c = {K, min_separation, peak_ratio};
    const long grid = rows / rows_per_group * table.units;
    HUPR_LAUNCH(hupr_k_pose_track_pairs, dim3((unsigned)grid), dim3(64), 0, as_stream(stream), heat, H, W, ratio, refine ? 1 : 0, state, f,
                c, present_or_null, rows_per_group, table, swap_cost, idx, maxval, raw_keypoints, keypoints, velocity, covariance, forecast,
                status, cand_xy, cand_score, cand_count, chosen, source);
    HUPR_LAUNCH_OK("hupr_k_pose_track_pairs");
    return HUPR_OK;
}
