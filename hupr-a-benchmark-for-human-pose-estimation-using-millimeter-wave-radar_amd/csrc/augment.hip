// Radar augmentation on the device (TRAINING.augMirror / augNoise / augMaskRange / augMaskAngle, TEST.flip): the step's plan drawn
// from a counter-based generator whose counter lives in device memory (so a replayed hipGraph draws a fresh plan), the left/right
// mirror as a permutation of the raw int16 ADC cube in front of the FFT chain, Gaussian noise and band masks on the normalised
// network input, the mirrored labels, and the merge of the flip test.  New, no reference counterpart: the reference augments
// nothing.  The rules are stated in full in section (a14) of include/hupr.h.  No atomics; every output repeats bit for bit.
#include "hupr_common.h"

namespace hupr {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): ten rounds, the key bumped by
// the Weyl constants between them.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

struct AugState {
    unsigned long long counter, mirrored, samples;
    double sum_sigma;
};

// floor(u n) for u = m 2^-24, exactly
__device__ __forceinline__ int scaled_floor(unsigned word, int n) { return (int)(((unsigned long long)(word >> 8) * (unsigned)n) >> 24); }

// One workgroup: thread t draws samples t, t + 256, ...; thread 0 then adds the statistics in sample order and bumps the counter.
// Every thread has read the counter before the barrier, thread 0 stores it behind the barrier.
__global__ __launch_bounds__(256) void hupr_k_augment_plan(int B, AugState* st, float p_mirror, float sigma_max, int max_range, int max_angle,
                                                           int R, int A, unsigned seed, unsigned key1, int* __restrict__ table,
                                                           unsigned char* __restrict__ flags) {
    const unsigned long long step = st->counter;
    const uint2 key = make_uint2(seed, key1);
    for (int b = threadIdx.x; b < B; b += 256) {
        const uint4 w0 = philox4x32_10(make_uint4((unsigned)step, (unsigned)(step >> 32), (unsigned)b, 0u), key);
        const uint4 w1 = philox4x32_10(make_uint4((unsigned)step, (unsigned)(step >> 32), (unsigned)b, 1u), key);
        const int mirror = (float)(w0.x >> 8) * 0x1p-24f < p_mirror ? 1 : 0;
        const float sigma = sigma_max * ((float)(w0.y >> 8) * 0x1p-24f);
        const int rl = scaled_floor(w0.z, max_range + 1), rs = scaled_floor(w0.w, R - rl + 1);
        const int hl = scaled_floor(w1.x, max_angle + 1), hs = scaled_floor(w1.y, A - hl + 1);
        const int vl = scaled_floor(w1.z, max_angle + 1), vs = scaled_floor(w1.w, A - vl + 1);
        int* row = table + (long)b * 8;
        row[0] = mirror;
        row[1] = __float_as_int(sigma);
        row[2] = rl; row[3] = rs; row[4] = hl; row[5] = hs; row[6] = vl; row[7] = vs;
        flags[b] = (unsigned char)mirror;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long mirrored = 0;
        double sum = 0.0;
        for (int b = 0; b < B; ++b) {
            mirrored += (unsigned long long)table[(long)b * 8];
            sum += (double)__int_as_float(table[(long)b * 8 + 1]);
        }
        st->counter = step + 1;
        st->mirrored += mirrored;
        st->samples += (unsigned long long)B;
        st->sum_sigma += sum;
    }
}

// The left/right mirror of flagged frames: row (rx, 3 cc + tx) of 256 complex int16 samples (1 KiB = 64 lanes x 16 B) is taken from
// row (3 - rx, 3 cc + 2 - tx).  A workgroup moves 16 rows of one frame (768 rows per frame), a wave four of them: four 16-byte
// loads in flight per lane, then four stores.
__global__ __launch_bounds__(256) void hupr_k_adc_mirror(const uint4* __restrict__ src, uint4* __restrict__ dst, int G,
                                                         const unsigned char* __restrict__ flags) {
    const long row0 = (long)blockIdx.x * 16 + (threadIdx.x >> 6) * 4;
    const int lane = threadIdx.x & 63;
    const long frame = row0 / 768;
    const int ri0 = (int)(row0 - frame * 768);
    const bool m = flags ? flags[frame / G] != 0 : true;
    uint4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ri = ri0 + i, rx = ri / 192, c = ri - rx * 192, tx = c % 3;
        const int sr = m ? (3 - rx) * 192 + c + 2 - 2 * tx : ri;
        v[i] = src[(frame * 768 + sr) * 64 + lane];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[(row0 + i) * 64 + lane] = v[i];
}

// -2 ln u1 for u1 = (m + 0.5) 2^-24, m < 2^24, from an argument that fp32 holds exactly: u1 itself in the lower half, 1 - u1 =
// (2^24 - 1 - m + 0.5) 2^-24 through log1pf in the upper half (m + 0.5 has 25 significant bits there).
__device__ __forceinline__ float neg2_log_u1(unsigned m) {
    if (m < (1u << 23)) return -2.f * logf(((float)m + 0.5f) * 0x1p-24f);
    return -2.f * log1pf(-(((float)(0xFFFFFFu - m) + 0.5f) * 0x1p-24f));
}

// Noise, then the band masks, on one sample per blockIdx.y; a thread owns the element quads q, q + stride, ... of the sample.
// VEC: 16-byte accesses (n % 4 == 0 and 16-byte aligned bases), otherwise 4-byte accesses of the same quads (the last one may be
// short).  sigma == 0 never touches the generator and leaves unmasked elements their bits.  y may be x: a quad is read and
// written by the same thread only.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_augment_apply(const float* x, float* y, long n, int R, int A, int E,
                                                            const int* __restrict__ table, int band_col,
                                                            const unsigned long long* __restrict__ counter, unsigned seed, unsigned key1) {
    const int b = blockIdx.y;
    const int* row = table + (long)b * 8;
    const float sigma = __int_as_float(row[1]);
    const int r_lo = row[3], r_hi = r_lo + row[2], a_lo = row[band_col + 1], a_hi = a_lo + row[band_col];
    const unsigned long long step = *counter - 1ull;        // the plan drawn last
    const uint2 key = make_uint2(seed, key1);
    const float* xs = x + (long)b * n;
    float* ys = y + (long)b * n;
    const long nq = (n + 3) >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const long e0 = q << 2;
        const int cnt = VEC ? 4 : (int)min(4L, n - e0);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            const float4 t = *reinterpret_cast<const float4*>(xs + e0);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            for (int i = 0; i < cnt; ++i) v[i] = xs[e0 + i];
        }
        if (sigma != 0.f) {
            const uint4 w = philox4x32_10(make_uint4((unsigned)step, (unsigned)(step >> 32), (unsigned)b, (unsigned)q), key);
            const float ra = sqrtf(neg2_log_u1(w.x >> 8)), rb = sqrtf(neg2_log_u1(w.z >> 8));
            const float ta = 2.f * ((float)(w.y >> 8) * 0x1p-24f), tb = 2.f * ((float)(w.w >> 8) * 0x1p-24f);
            v[0] = fmaf(sigma, ra * cospif(ta), v[0]);
            v[1] = fmaf(sigma, ra * sinpif(ta), v[1]);
            v[2] = fmaf(sigma, rb * cospif(tb), v[2]);
            v[3] = fmaf(sigma, rb * sinpif(tb), v[3]);
        }
        // element e = ((p R + r) A + a) E + el
        const long t0 = e0 / E;
        int el = (int)(e0 - t0 * E), a = (int)(t0 % A), r = (int)((t0 / A) % R);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if ((r >= r_lo && r < r_hi) || (a >= a_lo && a < a_hi)) v[i] = 0.f;
            if (++el == E) {
                el = 0;
                if (++a == A) {
                    a = 0;
                    if (++r == R) r = 0;
                }
            }
        }
        if (VEC) {
            *reinterpret_cast<float4*>(ys + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int i = 0; i < cnt; ++i) ys[e0 + i] = v[i];
        }
    }
}

struct PairTable {
    int K;
    int pair[64];
};

// One thread per joint: (x, y) of joint j of a flagged sample is (x_mirror - x, y) of joint pair[j]; other samples are copied.
template <typename T>
__global__ __launch_bounds__(256) void hupr_k_augment_joints(const T* __restrict__ in, T* __restrict__ out, long BK, PairTable pt, T x_mirror,
                                                             const unsigned char* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BK) return;
    const long b = i / pt.K;
    const int k = (int)(i - b * pt.K);
    if (flags ? flags[b] != 0 : true) {
        const T* s = in + (b * pt.K + pt.pair[k]) * 2;
        out[i * 2] = x_mirror - s[0];
        out[i * 2 + 1] = s[1];
    } else {
        out[i * 2] = in[i * 2];
        out[i * 2 + 1] = in[i * 2 + 1];
    }
}

// out[b][k][y][x] = 0.5f * (p[b][k][y][x] + pm[b][pair[k]][y][W - 1 - x]); VEC: four columns per thread, the mirrored four loaded as
// one 16-byte vector and reversed in registers.
template <bool VEC>
__global__ __launch_bounds__(256) void hupr_k_flip_merge(const float* __restrict__ p, const float* __restrict__ pm, float* __restrict__ out,
                                                         long n_units, PairTable pt, int H, int W) {
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_units) return;
    const int wq = VEC ? W >> 2 : W;
    const long rowi = u / wq;                         // (b K + k) H + y
    const int xq = (int)(u - rowi * wq);
    const long plane = rowi / H;
    const int yy = (int)(rowi - plane * H);
    const long b = plane / pt.K;
    const int k = (int)(plane - b * pt.K);
    const float* mrow = pm + (((b * pt.K + pt.pair[k]) * H) + yy) * (long)W;
    if (VEC) {
        const int x0 = xq << 2;
        const float4 a = *reinterpret_cast<const float4*>(p + rowi * W + x0);
        const float4 m = *reinterpret_cast<const float4*>(mrow + (W - 4 - x0));
        *reinterpret_cast<float4*>(out + rowi * W + x0) =
            make_float4(0.5f * (a.x + m.w), 0.5f * (a.y + m.z), 0.5f * (a.z + m.y), 0.5f * (a.w + m.x));
    } else {
        out[rowi * W + xq] = 0.5f * (p[rowi * W + xq] + mrow[W - 1 - xq]);
    }
}

static int fill_pairs(const char* who, PairTable& pt, int K, const int* pair_host) {
    HUPR_REQUIRE(pair_host, "%s: null pointer", who);
    HUPR_REQUIRE(K >= 1 && K <= 64, "%s: bad shape (K %d must be in [1, 64])", who, K);
    pt.K = K;
    for (int k = 0; k < K; ++k) {
        const int j = pair_host[k];
        HUPR_REQUIRE(j >= 0 && j < K && pair_host[j] == k, "%s: bad pair table (pair[%d] = %d; it must be an involution of [0, %d))", who, k, j, K);
        pt.pair[k] = j;
    }
    for (int k = K; k < 64; ++k) pt.pair[k] = 0;
    return HUPR_OK;
}

static bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

}  // namespace hupr

using namespace hupr;

extern "C" size_t hupr_augment_state_bytes(void) { return sizeof(AugState); }

extern "C" int hupr_augment_plan(int B, void* state, float p_mirror, float sigma_max, int max_range, int max_angle, int R, int A,
                                 unsigned seed, int rank, void* table, unsigned char* flags, hupr_stream_t stream) {
    HUPR_REQUIRE(state && table && flags, "hupr_augment_plan: null pointer");
    HUPR_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7) == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0,
                 "hupr_augment_plan: state must be 8-byte aligned, table 4-byte aligned");
    HUPR_REQUIRE(B >= 1 && B <= 65535, "hupr_augment_plan: bad shape (B %d must be in [1, 65535])", B);
    HUPR_REQUIRE(R >= 1 && R <= 65536 && A >= 1 && A <= 65536, "hupr_augment_plan: bad shape (R %d and A %d must be in [1, 65536])", R, A);
    HUPR_REQUIRE(p_mirror >= 0.f && p_mirror <= 1.f, "hupr_augment_plan: bad parameter (p_mirror %g must be in [0, 1])", p_mirror);
    HUPR_REQUIRE(sigma_max >= 0.f && sigma_max < INFINITY, "hupr_augment_plan: bad parameter (sigma_max %g must be finite and >= 0)", sigma_max);
    HUPR_REQUIRE(max_range >= 0 && max_range <= R / 2, "hupr_augment_plan: bad parameter (max_range %d must be in [0, R / 2 = %d])", max_range, R / 2);
    HUPR_REQUIRE(max_angle >= 0 && max_angle <= A / 2, "hupr_augment_plan: bad parameter (max_angle %d must be in [0, A / 2 = %d])", max_angle, A / 2);
    HUPR_REQUIRE(rank >= 0 && rank < (1 << 30), "hupr_augment_plan: bad rank %d", rank);
    HUPR_LAUNCH(hupr_k_augment_plan, dim3(1), dim3(256), 0, as_stream(stream), B, static_cast<AugState*>(state), p_mirror, sigma_max, max_range,
                max_angle, R, A, seed, 4u * (unsigned)rank, static_cast<int*>(table), flags);
    HUPR_LAUNCH_OK("hupr_k_augment_plan");
    return HUPR_OK;
}

extern "C" int hupr_adc_mirror_i16(const void* adc, void* out, int n_sf, int G, const unsigned char* flags_or_null, hupr_stream_t stream) {
    if (n_sf == 0) return HUPR_OK;
    HUPR_REQUIRE(adc && out, "hupr_adc_mirror_i16: null pointer");
    HUPR_REQUIRE(n_sf > 0 && n_sf <= (1 << 20), "hupr_adc_mirror_i16: bad shape (n_sf %d must be in [0, 2^20])", n_sf);
    HUPR_REQUIRE(G >= 1 && n_sf % G == 0, "hupr_adc_mirror_i16: bad shape (n_sf %d must be a multiple of G %d >= 1)", n_sf, G);
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(adc) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                 "hupr_adc_mirror_i16: adc and out must be 16-byte aligned");
    HUPR_REQUIRE(!overlap(adc, out, (size_t)n_sf * 786432), "hupr_adc_mirror_i16: adc and out overlap (the mirror is out of place)");
    HUPR_LAUNCH(hupr_k_adc_mirror, dim3((unsigned)n_sf * 48u), dim3(256), 0, as_stream(stream), static_cast<const uint4*>(adc),
                static_cast<uint4*>(out), G, flags_or_null);
    HUPR_LAUNCH_OK("hupr_k_adc_mirror");
    return HUPR_OK;
}

extern "C" int hupr_augment_apply_f32(const float* x, float* y, int B, int P, int R, int A, int E, const void* table, int sensor,
                                      const void* state, unsigned seed, int rank, hupr_stream_t stream) {
    HUPR_REQUIRE(x && y && table && state, "hupr_augment_apply_f32: null pointer");
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(table)) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(state) & 7) == 0, "hupr_augment_apply_f32: misaligned pointer");
    HUPR_REQUIRE(B >= 1 && B <= 65535, "hupr_augment_apply_f32: bad shape (B %d must be in [1, 65535])", B);
    HUPR_REQUIRE(P >= 1 && R >= 1 && A >= 1 && E >= 1 && R <= 65536 && A <= 65536 && E <= 65536,
                 "hupr_augment_apply_f32: bad shape (P %d, R %d, A %d, E %d)", P, R, A, E);
    HUPR_REQUIRE(sensor == 0 || sensor == 1, "hupr_augment_apply_f32: sensor %d must be 0 (horizontal) or 1 (vertical)", sensor);
    HUPR_REQUIRE(rank >= 0 && rank < (1 << 30), "hupr_augment_apply_f32: bad rank %d", rank);
    const long n = (long)P * R * A * E;                                   /* < 2^63: four factors, each <= 2^31 / 2^16 */
    HUPR_REQUIRE((long)P <= (1L << 33) / ((long)R * A * E), "hupr_augment_apply_f32: bad shape (a sample of %ld elements; at most 2^33)", n);
    const size_t bytes = (size_t)B * (size_t)n * 4;
    HUPR_REQUIRE(x == y || !overlap(x, y, bytes), "hupr_augment_apply_f32: x and y overlap without being equal");
    const long nq = (n + 3) >> 2;
    const dim3 grid((unsigned)min((nq + 255) / 256, 4096L), (unsigned)B);
    const unsigned key1 = 4u * (unsigned)rank + 1u + (unsigned)sensor;
    const unsigned long long* counter = static_cast<const unsigned long long*>(state);
    const int band_col = sensor == 0 ? 4 : 6;
    if (n % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0) {
        HUPR_LAUNCH(hupr_k_augment_apply<true>, grid, dim3(256), 0, as_stream(stream), x, y, n, R, A, E, static_cast<const int*>(table), band_col,
                    counter, seed, key1);
    } else {
        HUPR_LAUNCH(hupr_k_augment_apply<false>, grid, dim3(256), 0, as_stream(stream), x, y, n, R, A, E, static_cast<const int*>(table), band_col,
                    counter, seed, key1);
    }
    HUPR_LAUNCH_OK("hupr_k_augment_apply");
    return HUPR_OK;
}

extern "C" int hupr_augment_joints(const void* joints, void* out, long B, int K, int is_float, const unsigned char* flags_or_null,
                                   const int* pair_host, long x_mirror, hupr_stream_t stream) {
    PairTable pt;
    if (fill_pairs("hupr_augment_joints", pt, K, pair_host) != HUPR_OK) return HUPR_ERR_ARG;
    if (B == 0) return HUPR_OK;
    HUPR_REQUIRE(joints && out, "hupr_augment_joints: null pointer");
    HUPR_REQUIRE(B > 0 && B <= (1L << 32), "hupr_augment_joints: bad shape (B %ld)", B);
    HUPR_REQUIRE(is_float == 0 || is_float == 1, "hupr_augment_joints: is_float %d must be 0 (int64) or 1 (float32)", is_float);
    HUPR_REQUIRE(x_mirror >= 0 && x_mirror <= (1L << 24), "hupr_augment_joints: bad parameter (x_mirror %ld must be in [0, 2^24])", x_mirror);
    const size_t esz = is_float ? 4 : 8;
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(joints) | reinterpret_cast<uintptr_t>(out)) & (esz - 1)) == 0, "hupr_augment_joints: misaligned pointer");
    const long BK = B * K;
    HUPR_REQUIRE(!overlap(joints, out, (size_t)BK * 2 * esz), "hupr_augment_joints: joints and out overlap (the labels are written out of place)");
    const dim3 grid((unsigned)((BK + 255) / 256));
    if (is_float) {
        HUPR_LAUNCH(hupr_k_augment_joints<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const float*>(joints), static_cast<float*>(out), BK,
                    pt, (float)x_mirror, flags_or_null);
    } else {
        HUPR_LAUNCH(hupr_k_augment_joints<long long>, grid, dim3(256), 0, as_stream(stream), static_cast<const long long*>(joints),
                    static_cast<long long*>(out), BK, pt, (long long)x_mirror, flags_or_null);
    }
    HUPR_LAUNCH_OK("hupr_k_augment_joints");
    return HUPR_OK;
}

extern "C" int hupr_flip_merge_f32(const float* p, const float* pm, float* out, long B, int K, int H, int W, const int* pair_host,
                                   hupr_stream_t stream) {
    PairTable pt;
    if (fill_pairs("hupr_flip_merge_f32", pt, K, pair_host) != HUPR_OK) return HUPR_ERR_ARG;
    if (B == 0) return HUPR_OK;
    HUPR_REQUIRE(p && pm && out, "hupr_flip_merge_f32: null pointer");
    HUPR_REQUIRE(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "hupr_flip_merge_f32: bad shape (H %d and W %d must be in [1, 4096])", H, W);
    HUPR_REQUIRE(B > 0 && B <= (1L << 36) / ((long)K * H * W), "hupr_flip_merge_f32: bad shape (B %ld planes sets of %d x %d x %d)", B, K, H, W);
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(pm) | reinterpret_cast<uintptr_t>(out)) & 3) == 0,
                 "hupr_flip_merge_f32: misaligned pointer");
    const long n = B * K * H * W;
    HUPR_REQUIRE(!overlap(p, out, (size_t)n * 4) && !overlap(pm, out, (size_t)n * 4), "hupr_flip_merge_f32: out overlaps an input");
    if (W % 4 == 0 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(pm) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
        const long units = n / 4;
        HUPR_LAUNCH(hupr_k_flip_merge<true>, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, as_stream(stream), p, pm, out, units, pt, H, W);
    } else {
        HUPR_LAUNCH(hupr_k_flip_merge<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), p, pm, out, n, pt, H, W);
    }
    HUPR_LAUNCH_OK("hupr_k_flip_merge");
    return HUPR_OK;
}
