// Radar point cloud: the CA-CFAR detections of one sensor (cfar.hip) thinned to local power maxima and refined to sub-cell (range,
// azimuth) points, and the two sensors' points of a frame associated and turned into metres.  The rules are stated beside
// hupr_radar_peaks_f32 and hupr_radar_points_fuse_f32 in include/hupr.h (Rohling 1983; Jacobsen & Kootsookos 2007 for the two-point
// range estimator; Richards, Fundamentals of Radar Signal Processing, ch. 6).  New, no reference counterpart.
//   * peaks: one workgroup of 1024 threads per frame, thread = one azimuth column and four consecutive ranges as in cfar.hip.  The
//     power planes of the slots f - 1, f, f + 1 sit in a ring of three LDS planes (48 KB); a cell that the mask flags walks its box
//     there (every wave access reads 64 consecutive floats of one row) and leaves one bit in a register.  A ballot per row, a scan
//     over the 8 x 16 (slot, wave) counts and the ballots again give every peak its place in (f, r, a) order; the first 4096 are
//     staged (power, cell) in the LDS the ring has left, ranked by counting, and the strongest max_points are refined from the planes
//     in global memory.  No atomics, fixed orders: the same planes give the same bits.
//   * fuse: one wave per frame; both lists go to LDS, the horizontal points are walked in their order, the lanes search the vertical
//     list and a butterfly picks the partner (smallest range difference, ties to the lower row).  Geometry in fp64.
#include <math.h>

#include "hupr_common.h"
#include "radar_points_host.h"

namespace hupr {

constexpr int kPkR = 64, kPkA = 64, kPkCells = kPkR * kPkA;
constexpr int kPkThreads = 1024, kPkWaves = kPkThreads / 64, kPkRows = kPkR / kPkWaves;      // 4 ranges per thread
constexpr int kPkEntries = 8 * kPkWaves;                                                       // (slot, wave) counts

// The refinement is stated operation by operation in the header: nothing here is contracted into a fused multiply-add except the
// one the rule names (the power, as cfar.hip forms it).
#pragma clang fp contract(off)
__device__ __forceinline__ float pk_power(const float* __restrict__ x, int f, int cell) {
    const float vr = x[(2 * f) * kPkCells + cell], vi = x[(2 * f + 1) * kPkCells + cell];
    return fmaf(vr, vr, vi * vi);
}
__device__ __forceinline__ float pk_amp(float p) { return p == p ? sqrtf(p) : 0.f; }      // a NaN neighbour counts as 0

// Row `row` of a frame's points: (range, azimuth, Doppler, power, snr, cell) of the peak at `key` = (f * 64 + r) * 64 + a with power p.
__device__ __forceinline__ void pk_write_point(const float* __restrict__ x, const float* __restrict__ snr, int key, float p,
                                               float* __restrict__ row) {
    const int f = key / kPkCells, cell = key % kPkCells, r = cell / kPkA, a = cell % kPkA;
    const float a0 = sqrtf(p);
    const float am = r > 0 ? pk_amp(pk_power(x, f, cell - kPkA)) : 0.f;
    const float ap = r < kPkR - 1 ? pk_amp(pk_power(x, f, cell + kPkA)) : 0.f;
    const float rng = ap >= am ? (float)r + ap / (a0 + ap) : (float)r - am / (a0 + am);
    float delta = 0.f;
    if (a > 0 && a < kPkA - 1) {
        const float pm = pk_power(x, f, cell - 1), pp = pk_power(x, f, cell + 1);
        if (pm > 0.f && pp > 0.f) {
            // evaluated in fp64 and rounded: the fp32 logarithm to half a unit in the last place, the same on every libm
            const float lm = (float)log((double)pm), l0 = (float)log((double)p), lp = (float)log((double)pp);
            const float den = (lm - 2.f * l0) + lp;
            if (den < 0.f) delta = fminf(fmaxf(0.5f * ((lm - lp) / den), -0.5f), 0.5f);
        }
    }
    row[0] = rng;
    row[1] = (float)a + delta;
    row[2] = (float)(f - 4);
    row[3] = p;
    row[4] = snr ? snr[(long)f * kPkCells + cell] : 0.f;
    row[5] = (float)key;
}

__global__ __launch_bounds__(kPkThreads) void hupr_k_radar_peaks(const float* __restrict__ planes, const unsigned char* __restrict__ mask,
                                                                  const float* __restrict__ snr_or_null, int max_points, int sr, int sa,
                                                                  float* __restrict__ points, int* __restrict__ counts) {
    __shared__ float smem[3 * kPkCells];      // the ring of three power planes; afterwards the staged (power, cell) lists
    __shared__ int s_cnt[kPkEntries], s_base[kPkEntries], s_tot[2];
    const long frame = blockIdx.x;
    const float* x = planes + frame * 16 * kPkCells;
    const unsigned char* m = mask + frame * 8 * kPkCells;
    const float* snr = snr_or_null ? snr_or_null + frame * 8 * kPkCells : nullptr;
    const int tid = threadIdx.x, a = tid & 63, wave = tid >> 6, r0 = wave * kPkRows;

    unsigned flags = 0;      // bit 4 f + k: cell (f, r0 + k, a) is a peak
#pragma unroll
    for (int k = 0; k < kPkRows; ++k) smem[(r0 + k) * kPkA + a] = pk_power(x, 0, (r0 + k) * kPkA + a);
#pragma unroll 1
    for (int f = 0; f < 8; ++f) {
        const int nf = f + 1;
        if (nf < 8 && nf != 4) {      // slot f - 2 has been read for the last time before the barrier that ended the last round
            float* dst = smem + (nf % 3) * kPkCells;
#pragma unroll
            for (int k = 0; k < kPkRows; ++k) dst[(r0 + k) * kPkA + a] = pk_power(x, nf, (r0 + k) * kPkA + a);
        }
        __syncthreads();
        int wcount = 0;
        if (f != 4) {
            const float* own = smem + (f % 3) * kPkCells;
#pragma unroll 1
            for (int k = 0; k < kPkRows; ++k) {
                const int r = r0 + k, cell = r * kPkA + a;
                bool pk = false;
                if (m[f * kPkCells + cell] == 1) {
                    const float p = own[cell];
                    pk = p == p;
                    const int r_lo = max(r - sr, 0), r_hi = min(r + sr, kPkR - 1), a_lo = max(a - sa, 0), a_hi = min(a + sa, kPkA - 1);
                    for (int df = -1; df <= 1 && pk; ++df) {
                        const int f2 = f + df;
                        if (f2 < 0 || f2 > 7 || f2 == 4) continue;
                        const float* pl = smem + (f2 % 3) * kPkCells;
                        for (int r2 = r_lo; r2 <= r_hi && pk; ++r2) {
                            for (int a2 = a_lo; a2 <= a_hi; ++a2) {
                                const int rel = df != 0 ? df : (r2 != r ? r2 - r : a2 - a);      // < 0: below c in (f, r, a) order
                                if (rel == 0) continue;
                                const float q = pl[r2 * kPkA + a2];
                                if (!(rel < 0 ? p > q : p >= q)) { pk = false; break; }
                            }
                        }
                    }
                }
                wcount += __popcll(__ballot(pk));
                if (pk) flags |= 1u << (4 * f + k);
            }
        }
        if (a == 0) s_cnt[f * kPkWaves + wave] = wcount;
        __syncthreads();      // the next round overwrites slot f - 1's plane
    }

    // exclusive scan of the 128 (slot, wave) counts, which are in (f, r) order: two wave scans and the first wave's total
    int v = 0, incl = 0;
    if (tid < kPkEntries) {
        v = incl = s_cnt[tid];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (a >= o) incl += t;
        }
        if (a == 63) s_tot[wave] = incl;
    }
    __syncthreads();
    if (tid < kPkEntries) s_base[tid] = incl - v + (wave == 1 ? s_tot[0] : 0);
    __syncthreads();
    const int found = s_tot[0] + s_tot[1];
    const int staged = min(found, kPeaksStage), written = min(staged, max_points);

    float* st_p = smem;
    int* st_key = reinterpret_cast<int*>(smem + kPkCells);
#pragma unroll 1
    for (int f = 0; f < 8; ++f) {
        if (f == 4) continue;
        int pos = s_base[f * kPkWaves + wave];
#pragma unroll
        for (int k = 0; k < kPkRows; ++k) {
            const bool pk = (flags >> (4 * f + k)) & 1u;
            const unsigned long long b = __ballot(pk);
            const int mine = pos + __popcll(b & ((1ull << a) - 1ull));
            if (pk && mine < kPeaksStage) {
                const int cell = (r0 + k) * kPkA + a;
                st_p[mine] = pk_power(x, f, cell);
                st_key[mine] = f * kPkCells + cell;
            }
            pos += __popcll(b);
        }
    }
    __syncthreads();

    // rank by counting: descending power, ties to the lower cell; the keys differ, so the ranks 0 .. staged - 1 occur once each
    float* out = points + frame * max_points * 6;
    for (int i = tid; i < staged; i += kPkThreads) {
        const float pi = st_p[i];
        const int ki = st_key[i];
        int rank = 0;
#pragma unroll 4
        for (int j = 0; j < staged; ++j) {
            const float pj = st_p[j];
            rank += (pj > pi || (pj == pi && st_key[j] < ki)) ? 1 : 0;
        }
        if (rank < max_points) pk_write_point(x, snr, ki, pi, out + rank * 6);
    }
    for (int i = written + tid; i < max_points; i += kPkThreads) {
        float* row = out + i * 6;
        row[0] = 0.f; row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; row[4] = 0.f; row[5] = -1.f;
    }
    if (tid == 0) {
        counts[frame * 2] = written;
        counts[frame * 2 + 1] = found;
    }
}

// One wave per frame.  Rows: points (range, azimuth, Doppler, power, snr, cell), cloud (x, y, z, velocity, snr_h, snr_v, row_h, row_v).
__global__ __launch_bounds__(64) void hupr_k_radar_points_fuse(const float* __restrict__ points_h, const int* __restrict__ counts_h, int max_h,
                                                               const float* __restrict__ points_v, const int* __restrict__ counts_v, int max_v,
                                                               FuseGeometry g, double range_gate, int doppler_gate,
                                                               float* __restrict__ cloud, int* __restrict__ cloud_counts) {
    __shared__ float s_h[kPeaksMaxPoints * 6], s_v[kPeaksMaxPoints * 6];
    __shared__ int s_taken[kPeaksMaxPoints];
    const long frame = blockIdx.x;
    const int lane = threadIdx.x;
    const int nh = min(max(counts_h[frame * 2], 0), max_h), nv = min(max(counts_v[frame * 2], 0), max_v);      // inside the lists whatever they hold
    for (int i = lane; i < nh * 6; i += 64) s_h[i] = points_h[frame * max_h * 6 + i];
    for (int i = lane; i < nv * 6; i += 64) s_v[i] = points_v[frame * max_v * 6 + i];
    for (int i = lane; i < kPeaksMaxPoints; i += 64) s_taken[i] = 0;
    __syncthreads();
    float* out = cloud + frame * max_h * 8;
    int nout = 0;
#pragma unroll 1
    for (int i = 0; i < nh; ++i) {
        const float rh = s_h[i * 6], ah = s_h[i * 6 + 1], dh = s_h[i * 6 + 2];
        double best = INFINITY;
        int bj = 0x7fffffff;
        for (int j = lane; j < nv; j += 64) {
            if (s_taken[j]) continue;
            if (!(fabsf(dh - s_v[j * 6 + 2]) <= (float)doppler_gate)) continue;
            const double dr = fabs((double)rh - (double)s_v[j * 6]);
            if (!(dr <= range_gate)) continue;
            if (dr < best) { best = dr; bj = j; }      // j rises: a tie keeps the lower row
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
        }
        if (bj != 0x7fffffff) {      // the same in every lane
            if (lane == 0) s_taken[bj] = 1;
            const double Rh = (94.0 - (double)rh) * g.range_bin_m, uh = (31.0 - (double)ah) / 32.0;
            const double Rv = (94.0 - (double)s_v[bj * 6]) * g.range_bin_m, uv = (31.0 - (double)s_v[bj * 6 + 1]) / 32.0;
            const double c_h = g.oh_ah + Rh * uh, c_v = g.ov_av + Rv * uv;
            const double e_h = c_h - g.oh_ah, e_v = c_v - g.oh_av;
            const double rad = (Rh * Rh - e_h * e_h) - e_v * e_v;
            if (rad >= 0.0) {
                const double c_b = g.oh_b + sqrt(rad);
                if (lane == 0) {
                    float* row = out + nout * 8;
                    row[0] = (float)((c_h * g.a_h[0] + c_v * g.a_v[0]) + c_b * g.b[0]);
                    row[1] = (float)((c_h * g.a_h[1] + c_v * g.a_v[1]) + c_b * g.b[1]);
                    row[2] = (float)((c_h * g.a_h[2] + c_v * g.a_v[2]) + c_b * g.b[2]);
                    row[3] = (float)((double)dh * g.doppler_mps_per_bin);
                    row[4] = s_h[i * 6 + 4];
                    row[5] = s_v[bj * 6 + 4];
                    row[6] = (float)i;
                    row[7] = (float)bj;
                }
                ++nout;
            }
        }
        __syncthreads();      // the next point sees this one's partner as taken
    }
    for (int i = nout + lane; i < max_h; i += 64) {
        float* row = out + i * 8;
        row[0] = 0.f; row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; row[4] = 0.f; row[5] = 0.f; row[6] = -1.f; row[7] = -1.f;
    }
    if (lane == 0) cloud_counts[frame] = nout;
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_radar_peaks_f32(const float* planes, const unsigned char* mask, const float* snr_or_null, int n, int max_points,
                                    int sep_range, int sep_azimuth, float* points, int* counts, hupr_stream_t stream) {
    const char* bad = peaks_check(n, max_points, sep_range, sep_azimuth);
    HUPR_REQUIRE(!bad, "hupr_radar_peaks_f32: %s (n %d, max_points %d, sep_range %d, sep_azimuth %d)", bad, n, max_points, sep_range,
                 sep_azimuth);
    HUPR_REQUIRE(n <= (1 << 20), "hupr_radar_peaks_f32: more than 2^20 frames (%d)", n);
    if (n == 0) return HUPR_OK;
    HUPR_REQUIRE(planes && mask && points && counts, "hupr_radar_peaks_f32: null pointer");
    HUPR_LAUNCH(hupr_k_radar_peaks, dim3((unsigned)n), dim3(kPkThreads), 0, as_stream(stream), planes, mask, snr_or_null, max_points,
                sep_range, sep_azimuth, points, counts);
    HUPR_LAUNCH_OK("hupr_k_radar_peaks");
    return HUPR_OK;
}

extern "C" int hupr_radar_points_fuse_f32(const float* points_h, const int* counts_h, int max_h, const float* points_v, const int* counts_v,
                                          int max_v, int n, const double* geometry_host, double range_gate, int doppler_gate, float* cloud,
                                          int* cloud_counts, hupr_stream_t stream) {
    FuseGeometry g;
    const char* bad = fuse_check(n, max_h, max_v, geometry_host, range_gate, doppler_gate, &g);
    HUPR_REQUIRE(!bad, "hupr_radar_points_fuse_f32: %s (n %d, max_points %d and %d, range_gate %g, doppler_gate %d)", bad, n, max_h, max_v,
                 range_gate, doppler_gate);
    HUPR_REQUIRE(n <= (1 << 20), "hupr_radar_points_fuse_f32: more than 2^20 frames (%d)", n);
    if (n == 0) return HUPR_OK;
    HUPR_REQUIRE(points_h && counts_h && points_v && counts_v && cloud && cloud_counts, "hupr_radar_points_fuse_f32: null pointer");
    HUPR_LAUNCH(hupr_k_radar_points_fuse, dim3((unsigned)n), dim3(64), 0, as_stream(stream), points_h, counts_h, max_h, points_v, counts_v,
                max_v, g, range_gate, doppler_gate, cloud, cloud_counts);
    HUPR_LAUNCH_OK("hupr_k_radar_points_fuse");
    return HUPR_OK;
}
