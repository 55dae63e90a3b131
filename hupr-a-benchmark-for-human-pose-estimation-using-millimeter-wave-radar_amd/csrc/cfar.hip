// Scene occupancy: cell-averaging CFAR detection on the (range, azimuth) planes of the seven moving Doppler slots of a sensor-frame's
// elevation-mean planes, the per-frame summary of the detections, and the presence gate over it.  The rule is stated beside
// hupr_cfar_ra_f32 in include/hupr.h (Rohling 1983; Richards, Fundamentals of Radar Signal Processing, ch. 6).  New, no reference
// counterpart.
//   * one workgroup of 1024 threads per frame walks the seven slots: the 64 x 64 power plane goes to LDS, a horizontal pass leaves
//     two row sums per cell there (the 2 w + 1 cells around it, and those of them beyond the guard columns), a vertical pass adds
//     the first over the rows beyond the guard rows and the second over the guard rows.  Every partial sum holds training cells only:
//     the cell under test and its guard cells never enter a sum that is later corrected (a mover 40 dB above the noise would leave a
//     cancellation error of the order of the noise).
//   * thread = one azimuth column and four consecutive ranges: every LDS access of a wave reads or writes 64 consecutive floats of
//     one row (conflict-free on 32 or 64 banks, the shifted reads a + const included), every global access 256 consecutive bytes.
//   * the summary is reduced in a fixed order (thread: slot, then range; wave: xor butterfly; workgroup: wave 0 .. 15), in fp64,
//     without atomics: the same planes give the same bits.
#include "hupr_common.h"
#include "cfar_host.h"
#include "stream_state.h"

namespace hupr {

constexpr int kCfarR = 64, kCfarA = 64, kCfarCells = kCfarR * kCfarA;
constexpr int kCfarThreads = 1024, kCfarWaves = kCfarThreads / 64, kCfarRows = kCfarR / kCfarWaves;      // 4 ranges per thread

struct GateState {      // hupr_presence_update's state of one lane
    int present;
    int hits;
    int misses;
    int frames;
};

__device__ __forceinline__ double wave_sum_xor_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// planes: frame `blockIdx.x` starts at planes + blockIdx.x * frame_stride (+ slot * 16 planes when a session state is given: the
// ring slot of the centre frame, by the arithmetic of hupr_k_mnet_stream).
__global__ __launch_bounds__(kCfarThreads) void hupr_k_cfar_ra(const float* __restrict__ planes, long frame_stride,
                                                                const StreamState* __restrict__ state, int lookahead, int flush, int G,
                                                                int g, int w, const float* __restrict__ alpha,
                                                                unsigned char* __restrict__ mask, float* __restrict__ snr_out,
                                                                float* __restrict__ summary) {
    __shared__ float sp[kCfarCells];         // power
    __shared__ float sfull[kCfarCells];      // row sum over the columns a - w .. a + w
    __shared__ float sside[kCfarCells];      // row sum over the columns a - w .. a - g - 1 and a + g + 1 .. a + w
    __shared__ double red_sum[kCfarWaves][4];
    __shared__ int red_count[kCfarWaves], red_key[kCfarWaves];
    __shared__ float red_best[kCfarWaves];
    const long frame = blockIdx.x;
    const float* x = planes + frame * frame_stride;
    if (state) {
        const int centre = flush ? state->emitted : state->frames - lookahead;
        x += (long)(((centre % G) + G) % G) * 16 * kCfarCells;      // in range whatever the state holds
    }
    const int a = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * kCfarRows;
    const int a_lo = max(a - w, 0), a_hi = min(a + w, kCfarA - 1);
    const int na_full = a_hi - a_lo + 1, na_guard = min(a + g, kCfarA - 1) - max(a - g, 0) + 1;

    double sum_w = 0.0, sum_r = 0.0, sum_a = 0.0, sum_d = 0.0;
    int count = 0, best_key = 0x7fffffff;
    float best = 0.f;
#pragma unroll 1
    for (int f = 0; f < 8; ++f) {
        const long out0 = (frame * 8 + f) * kCfarCells;
        if (f == 4) {      // the clutter-nulled zero-Doppler slot: never read
#pragma unroll
            for (int k = 0; k < kCfarRows; ++k) {
                const int cell = (r0 + k) * kCfarA + a;
                if (mask) mask[out0 + cell] = 0;
                if (snr_out) snr_out[out0 + cell] = 0.f;
            }
            continue;
        }
        const float* re = x + (long)(2 * f) * kCfarCells;
        const float* im = re + kCfarCells;
#pragma unroll
        for (int k = 0; k < kCfarRows; ++k) {
            const int cell = (r0 + k) * kCfarA + a;
            const float vr = re[cell], vi = im[cell];
            sp[cell] = fmaf(vr, vr, vi * vi);
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < kCfarRows; ++k) {
            const float* row = sp + (r0 + k) * kCfarA;
            float side = 0.f, mid = 0.f;
#pragma unroll 4
            for (int a2 = a_lo; a2 <= a_hi; ++a2) {
                const float v = row[a2];
                if (abs(a2 - a) > g) side += v; else mid += v;
            }
            sside[(r0 + k) * kCfarA + a] = side;
            sfull[(r0 + k) * kCfarA + a] = side + mid;
        }
        __syncthreads();
#pragma unroll 1      // rolled: 1024 threads leave 128 registers a thread
        for (int k = 0; k < kCfarRows; ++k) {
            const int r = r0 + k, cell = r * kCfarA + a;
            const int r_lo = max(r - w, 0), r_hi = min(r + w, kCfarR - 1);
            float acc = 0.f;
#pragma unroll 4
            for (int r2 = r_lo; r2 <= r_hi; ++r2) acc += (abs(r2 - r) > g ? sfull : sside)[r2 * kCfarA + a];
            const int N = (r_hi - r_lo + 1) * na_full - (min(r + g, kCfarR - 1) - max(r - g, 0) + 1) * na_guard;
            const float noise = acc / (float)N;
            const float p = sp[cell];
            const float thr = alpha[N] * noise;
            const bool det = p > thr;                                   // false for a NaN on either side
            const float s = (p == 0.f && noise == 0.f) ? 0.f : p / noise;
            if (mask) mask[out0 + cell] = det ? 1 : 0;
            if (snr_out) snr_out[out0 + cell] = s;
            if (det) {
                const int key = f * kCfarCells + cell;                  // (f, r, a) in that order
                ++count;
                sum_w += (double)s;
                sum_r += (double)s * (double)r;
                sum_a += (double)s * (double)a;
                sum_d += (double)s * (double)(f - 4);
                if (s > best || (s == best && key < best_key)) { best = s; best_key = key; }
            }
        }
        __syncthreads();      // the next slot overwrites the three planes
    }

    sum_w = wave_sum_xor_f64(sum_w);
    sum_r = wave_sum_xor_f64(sum_r);
    sum_a = wave_sum_xor_f64(sum_a);
    sum_d = wave_sum_xor_f64(sum_d);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        count += __shfl_xor(count, o, 64);
        const float ob = __shfl_xor(best, o, 64);
        const int ok = __shfl_xor(best_key, o, 64);
        if (ob > best || (ob == best && ok < best_key)) { best = ob; best_key = ok; }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_sum[wave][0] = sum_w; red_sum[wave][1] = sum_r; red_sum[wave][2] = sum_a; red_sum[wave][3] = sum_d;
        red_count[wave] = count; red_best[wave] = best; red_key[wave] = best_key;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tw = 0.0, tr = 0.0, ta = 0.0, td = 0.0;
        int tc = 0, tk = 0x7fffffff;
        float tb = 0.f;
#pragma unroll 1
        for (int v = 0; v < kCfarWaves; ++v) {
            tw += red_sum[v][0]; tr += red_sum[v][1]; ta += red_sum[v][2]; td += red_sum[v][3];
            tc += red_count[v];
            if (red_best[v] > tb || (red_best[v] == tb && red_key[v] < tk)) { tb = red_best[v]; tk = red_key[v]; }
        }
        float* o = summary + frame * 8;
        const bool any = tc > 0;
        o[0] = (float)tc;
        o[1] = any ? tb : 0.f;
        o[2] = any ? (float)(tk / kCfarCells) : -1.f;
        o[3] = any ? (float)((tk % kCfarCells) / kCfarA) : -1.f;
        o[4] = any ? (float)(tk % kCfarA) : -1.f;
        o[5] = any ? (float)(tr / tw) : 0.f;
        o[6] = any ? (float)(ta / tw) : 0.f;
        o[7] = any ? (float)(td / tw) : 0.f;
    }
}

// One thread per lane: the hysteresis of the presence gate.  The counters saturate instead of wrapping.
__global__ __launch_bounds__(64) void hupr_k_presence_update(const float* __restrict__ summary, int lanes, int min_cells, int confirm,
                                                             int hold, GateState* __restrict__ gate, int* __restrict__ present_out) {
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= lanes) return;
    GateState s = gate[lane];
    const bool hit = summary[(long)lane * 8] >= (float)min_cells;
    const int top = 0x7fffffff;
    s.hits = hit ? (s.hits < top ? s.hits + 1 : top) : 0;
    s.misses = hit ? 0 : (s.misses < top ? s.misses + 1 : top);
    if (!s.present && s.hits >= confirm) s.present = 1;
    else if (s.present && s.misses > hold) s.present = 0;
    s.frames = s.frames < top ? s.frames + 1 : top;
    gate[lane] = s;
    present_out[lane] = s.present;
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_cfar_table_len(int guard, int train) {
    const int cells = cfar_window_cells(guard, train);
    HUPR_REQUIRE(cells > 0, "hupr_cfar_table_len: guard %d, train %d: need guard >= 0, train >= 1 and guard + train <= %d", guard, train,
                 kCfarMaxHalf);
    return cells + 1;
}

extern "C" int hupr_cfar_alpha_table_f32(double pfa, int guard, int train, float* host_table, int table_len) {
    HUPR_REQUIRE(pfa > 0.0 && pfa < 1.0, "hupr_cfar_alpha_table_f32: pfa %g outside (0, 1)", pfa);
    const char* bad = cfar_check_window(guard, train, host_table, table_len);
    HUPR_REQUIRE(!bad, "hupr_cfar_alpha_table_f32: %s (guard %d, train %d, table_len %d)", bad, guard, train, table_len);
    return cfar_fill_alpha_table(pfa, guard, train, host_table, table_len) == 0 ? HUPR_OK : HUPR_ERR_ARG;
}

static int cfar_launch(const char* who, const float* planes, long frame_stride, const void* state, int lookahead, int flush, int G,
                       int n, int guard, int train, const float* alpha_table, int table_len, unsigned char* mask, float* snr,
                       float* summary, hupr_stream_t stream) {
    HUPR_REQUIRE(n >= 0, "%s: negative frame count %d", who, n);
    const char* bad = cfar_check_window(guard, train, alpha_table, table_len);
    HUPR_REQUIRE(!bad, "%s: %s (guard %d, train %d, table_len %d)", who, bad, guard, train, table_len);
    if (n == 0) return HUPR_OK;
    HUPR_REQUIRE(planes && summary, "%s: null pointer", who);
    HUPR_LAUNCH(hupr_k_cfar_ra, dim3((unsigned)n), dim3(kCfarThreads), 0, as_stream(stream), planes, frame_stride,
                static_cast<const StreamState*>(state), lookahead, flush ? 1 : 0, G, guard, guard + train, alpha_table, mask, snr,
                summary);
    HUPR_LAUNCH_OK("hupr_k_cfar_ra");
    return HUPR_OK;
}

extern "C" int hupr_cfar_ra_f32(const float* planes, int n, int guard, int train, const float* alpha_table, int table_len,
                                unsigned char* mask_or_null, float* snr_or_null, float* summary, hupr_stream_t stream) {
    return cfar_launch("hupr_cfar_ra_f32", planes, 16L * kCfarCells, nullptr, 0, 0, 2, n, guard, train, alpha_table, table_len,
                       mask_or_null, snr_or_null, summary, stream);
}

extern "C" int hupr_cfar_ra_stream_f32(const float* ring, const void* stream_state, int lookahead, int flush, int lanes, int G,
                                       int guard, int train, const float* alpha_table, int table_len, unsigned char* mask_or_null,
                                       float* snr_or_null, float* summary, hupr_stream_t stream) {
    const char* who = "hupr_cfar_ra_stream_f32";
    HUPR_REQUIRE(G >= 2 && G % 2 == 0 && G <= 64, "%s: the window must hold an even number of 2..64 frames, got %d", who, G);
    HUPR_REQUIRE(lookahead >= 0 && lookahead <= G / 2 - 1, "%s: lookahead %d outside 0..%d", who, lookahead, G / 2 - 1);
    HUPR_REQUIRE(lanes == 0 || stream_state, "%s: null session state", who);
    // the horizontal sensor's half of the ring: lane l's G slots of 16 planes start at l * G * 16 planes
    return cfar_launch(who, ring, (long)G * 16 * kCfarCells, stream_state, lookahead, flush, G, lanes, guard, train, alpha_table,
                       table_len, mask_or_null, snr_or_null, summary, stream);
}

extern "C" int hupr_presence_update(const float* summary, int lanes, int min_cells, int confirm, int hold, int* gate_state,
                                    int* present_out, hupr_stream_t stream) {
    const char* bad = presence_check(lanes, min_cells, confirm, hold);
    HUPR_REQUIRE(!bad, "hupr_presence_update: %s (lanes %d, min_cells %d, confirm %d, hold %d)", bad, lanes, min_cells, confirm, hold);
    if (lanes == 0) return HUPR_OK;
    HUPR_REQUIRE(summary && gate_state && present_out, "hupr_presence_update: null pointer");
    HUPR_LAUNCH(hupr_k_presence_update, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, as_stream(stream), summary, lanes, min_cells,
                confirm, hold, reinterpret_cast<GateState*>(gate_state), present_out);
    HUPR_LAUNCH_OK("hupr_k_presence_update");
    return HUPR_OK;
}
