// Interference blanking of the raw int16 ADC cube in front of the FFT chain (DATASET.interference, PoseStream(interference=...)): a
// second FMCW radar in the band leaves short high-amplitude bursts in single chirps; they are found on the clutter-removed residual
// of each (sensor-frame, rx, tx) group against the chirp's own median power, dilated by a guard and replaced by the group's clutter
// estimate (or by zero).  New, no reference counterpart.  The rule is stated in full in section (a15) of include/hupr.h: integer
// arithmetic throughout, no atomics, every output repeats bit for bit.
#include "hupr_common.h"

namespace hupr {

constexpr int kIfLoops = 64;        // chirp loops of a group
constexpr int kIfThreads = 512;     // 8 waves, 8 chirps each

// The eight int16 of a lane's 16 bytes: samples 4 lane + j, component c at index 2 j + c.
__device__ __forceinline__ void if_unpack(const uint4& v, int* x) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[2 * j] = (int)(short)(w[j] & 0xffffu);
        x[2 * j + 1] = (int)w[j] >> 16;
    }
}

// One step of the radix selection on bit `bit` of the words v[0..3]: the candidates (bit j of cand = sample 4 lane + j) with a 0
// there are counted over the wave; the k-th smallest (0-based) stays among them when k is below that count, among the others
// otherwise.  k and the return value (whether the bit of the selected value is 1) are wave-uniform.
__device__ __forceinline__ bool if_select_bit(const unsigned* v, int bit, unsigned& cand, int& k) {
    unsigned zeros = 0;
    int c0 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool z = ((cand >> j) & 1u) && !((v[j] >> bit) & 1u);
        c0 += __popcll(__ballot(z));
        zeros |= (z ? 1u : 0u) << j;
    }
    if (k < c0) {
        cand = zeros;
        return false;
    }
    k -= c0;
    cand &= ~zeros;
    return true;
}

// bit i of an 8-bit value -> bit 4 i
__device__ __forceinline__ unsigned if_spread4(unsigned b) {
    b = (b | (b << 12)) & 0x000F000Fu;
    b = (b | (b << 6)) & 0x03030303u;
    return (b | (b << 3)) & 0x11111111u;
}

__device__ __forceinline__ int if_floor_div(int a, int b) {      // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// One workgroup per group.  The 64 rows (1 KiB each, 3 KiB apart) land in LDS; every wave forms the column sums of the lane's four
// samples from there, then works through its eight chirps: residual power in 64 bits, the lower median by radix selection over bits
// 45..0 (four ballots per bit), the flags as four 64-bit ballots (bit l of word j = sample 4 l + j), the dilation as shifts of those
// words.  The dilated words go to LDS; behind a barrier every wave sums, per lane, the flagged loops' samples, forms the fill and
// writes its eight rows.  The whole group is in LDS before the first store, so out may be adc.
__global__ __launch_bounds__(kIfThreads) void hupr_k_adc_interference(const uint4* __restrict__ src, uint4* dst, int K, int guard, int fill_zero,
                                                                      unsigned* __restrict__ mask, int* __restrict__ counts) {
    __shared__ uint4 rows[kIfLoops][64];
    __shared__ unsigned long long flagw[kIfLoops][4];
    __shared__ int wave_counts[kIfThreads / 64][2];

    const int g = blockIdx.x, sf = g / 12, r12 = g - sf * 12, rx = r12 / 3, tx = r12 - rx * 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row0 = ((long)sf * 4 + rx) * 192 + tx;               // row of loop cc: row0 + 3 cc

    {
        uint4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = src[(row0 + 3 * (wave * 8 + i)) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 8; ++i) rows[wave * 8 + i][lane] = v[i];
    }
    __syncthreads();

    int S[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int cc = 0; cc < kIfLoops; ++cc) {
        int x[8];
        if_unpack(rows[cc][lane], x);
#pragma unroll
        for (int e = 0; e < 8; ++e) S[e] += x[e];
    }

    int n_samples = 0, n_chirps = 0;                                  // wave-uniform
    for (int i = 0; i < 8; ++i) {
        const int cc = wave * 8 + i;
        int x[8];
        if_unpack(rows[cc][lane], x);
        unsigned hi[4], lo[4];
        unsigned long long p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long ri = 64 * x[2 * j] - S[2 * j], rq = 64 * x[2 * j + 1] - S[2 * j + 1];
            p[j] = (unsigned long long)(ri * ri + rq * rq);
            hi[j] = (unsigned)(p[j] >> 32);
            lo[j] = (unsigned)p[j];
        }
        unsigned cand = 0xFu;
        int k = 127;
        unsigned med_hi = 0, med_lo = 0;
        for (int b = 13; b >= 0; --b)
            if (if_select_bit(hi, b, cand, k)) med_hi |= 1u << b;
        for (int b = 31; b >= 0; --b)
            if (if_select_bit(lo, b, cand, k)) med_lo |= 1u << b;
        unsigned long long med = ((unsigned long long)med_hi << 32) | med_lo;
        if (med == 0) med = 1;
        const unsigned long long thr = (unsigned long long)K * med;
        unsigned long long m[4], d[4], up[4], dn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = __ballot(p[j] > thr);
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = up[j] = dn[j] = m[j];
        for (int s = 0; s < guard; ++s) {
            // one sample up: (l, j) -> (l, j + 1), (l, 3) -> (l + 1, 0); one down the other way.  Bits leaving the word are
            // samples below 0 or above 255.
            const unsigned long long u3 = up[3] << 1, d0 = dn[0] >> 1;
            up[3] = up[2]; up[2] = up[1]; up[1] = up[0]; up[0] = u3;
            dn[0] = dn[1]; dn[1] = dn[2]; dn[2] = dn[3]; dn[3] = d0;
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] |= up[j] | dn[j];
        }
        const int c = __popcll(d[0]) + __popcll(d[1]) + __popcll(d[2]) + __popcll(d[3]);
        n_samples += c;
        n_chirps += c != 0 ? 1 : 0;
        if (lane < 4) flagw[cc][lane] = lane == 0 ? d[0] : lane == 1 ? d[1] : lane == 2 ? d[2] : d[3];
    }
    if (lane == 0) {
        wave_counts[wave][0] = n_samples;
        wave_counts[wave][1] = n_chirps;
    }
    __syncthreads();

    if (threadIdx.x < 2) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < kIfThreads / 64; ++w) t += wave_counts[w][threadIdx.x];
        counts[(long)g * 2 + threadIdx.x] = t;
    }
    if (mask) {                                                       // thread -> (loop, 32 samples = lanes 8 q .. 8 q + 7)
        const int cc = threadIdx.x >> 3, q = threadIdx.x & 7;
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= if_spread4((unsigned)(flagw[cc][j] >> (8 * q)) & 0xffu) << j;
        mask[(row0 + 3 * cc) * 8 + q] = w;
    }

    // the flagged loops' sums and counts at the lane's four samples
    int F[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nf[4] = {0, 0, 0, 0};
    for (int cc = 0; cc < kIfLoops; ++cc) {
        unsigned bits = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) bits |= ((unsigned)(flagw[cc][j] >> lane) & 1u) << j;
        if (bits) {
            int x[8];
            if_unpack(rows[cc][lane], x);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((bits >> j) & 1u) {
                    F[2 * j] += x[2 * j];
                    F[2 * j + 1] += x[2 * j + 1];
                    nf[j] += 1;
                }
            }
        }
    }
    unsigned fillw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = kIfLoops - nf[j];
        int fi = 0, fq = 0;
        if (!fill_zero && n > 0 && nf[j] > 0) {
            fi = if_floor_div(2 * (S[2 * j] - F[2 * j]) + n, 2 * n);
            fq = if_floor_div(2 * (S[2 * j + 1] - F[2 * j + 1]) + n, 2 * n);
        }
        fillw[j] = ((unsigned)fi & 0xffffu) | ((unsigned)fq << 16);
    }
    for (int i = 0; i < 8; ++i) {
        const int cc = wave * 8 + i;
        const uint4 v = rows[cc][lane];
        unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((flagw[cc][j] >> lane) & 1ull) w[j] = fillw[j];
        dst[(row0 + 3 * cc) * 64 + lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// stats[sf][k] = the sum of counts[sf][0..11][k], in group order
__global__ __launch_bounds__(256) void hupr_k_adc_interference_stats(const int* __restrict__ counts, int n, int* __restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int sf = i >> 1, k = i & 1;
    int t = 0;
#pragma unroll
    for (int r = 0; r < 12; ++r) t += counts[((long)sf * 12 + r) * 2 + k];
    stats[i] = t;
}

static bool if_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_adc_interference_i16(const void* adc, void* out, int n_sf, int K, int guard, int fill, unsigned char* mask_or_null,
                                         int* group_counts, hupr_stream_t stream) {
    HUPR_REQUIRE(n_sf >= 0 && n_sf <= (1 << 20), "hupr_adc_interference_i16: bad shape (n_sf %d must be in [0, 2^20])", n_sf);
    HUPR_REQUIRE(K >= 2 && K <= 1024, "hupr_adc_interference_i16: bad parameter (K %d must be in [2, 1024])", K);
    HUPR_REQUIRE(guard >= 0 && guard <= 8, "hupr_adc_interference_i16: bad parameter (guard %d must be in [0, 8])", guard);
    HUPR_REQUIRE(fill == HUPR_INTERFERENCE_FILL_CLUTTER || fill == HUPR_INTERFERENCE_FILL_ZERO,
                 "hupr_adc_interference_i16: bad parameter (fill %d must be 0 (clutter) or 1 (zero))", fill);
    if (n_sf == 0) return HUPR_OK;
    HUPR_REQUIRE(adc && out && group_counts, "hupr_adc_interference_i16: null pointer");
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(adc) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                 "hupr_adc_interference_i16: adc and out must be 16-byte aligned");
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(mask_or_null) | reinterpret_cast<uintptr_t>(group_counts)) & 3) == 0,
                 "hupr_adc_interference_i16: mask and group_counts must be 4-byte aligned");
    const size_t cube = (size_t)n_sf * 786432, mbytes = (size_t)n_sf * 4 * 192 * 32, cbytes = (size_t)n_sf * 12 * 2 * 4;
    HUPR_REQUIRE(adc == out || !if_overlap(adc, cube, out, cube),
                 "hupr_adc_interference_i16: adc and out overlap without being equal (in place means out == adc exactly)");
    HUPR_REQUIRE(!if_overlap(group_counts, cbytes, adc, cube) && !if_overlap(group_counts, cbytes, out, cube),
                 "hupr_adc_interference_i16: group_counts overlaps a cube");
    HUPR_REQUIRE(!mask_or_null || (!if_overlap(mask_or_null, mbytes, adc, cube) && !if_overlap(mask_or_null, mbytes, out, cube) &&
                                   !if_overlap(mask_or_null, mbytes, group_counts, cbytes)),
                 "hupr_adc_interference_i16: mask overlaps another buffer");
    HUPR_LAUNCH(hupr_k_adc_interference, dim3((unsigned)n_sf * 12u), dim3(kIfThreads), 0, as_stream(stream), static_cast<const uint4*>(adc),
                static_cast<uint4*>(out), K, guard, fill == HUPR_INTERFERENCE_FILL_ZERO ? 1 : 0, reinterpret_cast<unsigned*>(mask_or_null),
                group_counts);
    HUPR_LAUNCH_OK("hupr_k_adc_interference");
    return HUPR_OK;
}

extern "C" int hupr_adc_interference_stats(const int* group_counts, int n_sf, int* stats, hupr_stream_t stream) {
    HUPR_REQUIRE(n_sf >= 0 && n_sf <= (1 << 20), "hupr_adc_interference_stats: bad shape (n_sf %d must be in [0, 2^20])", n_sf);
    if (n_sf == 0) return HUPR_OK;
    HUPR_REQUIRE(group_counts && stats, "hupr_adc_interference_stats: null pointer");
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(group_counts) | reinterpret_cast<uintptr_t>(stats)) & 3) == 0,
                 "hupr_adc_interference_stats: misaligned pointer");
    HUPR_REQUIRE(!if_overlap(group_counts, (size_t)n_sf * 96, stats, (size_t)n_sf * 8), "hupr_adc_interference_stats: stats overlaps group_counts");
    HUPR_LAUNCH(hupr_k_adc_interference_stats, dim3((unsigned)((2 * n_sf + 255) / 256)), dim3(256), 0, as_stream(stream), group_counts, 2 * n_sf,
                stats);
    HUPR_LAUNCH_OK("hupr_k_adc_interference_stats");
    return HUPR_OK;
}
