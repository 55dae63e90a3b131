// Radar scene simulator (hupr_amd.simulate, functional.radar_scene): S moving point scatterers seen by one IWR1843 (three
// transmitters fired in TDM order, four receivers) -> the raw ADC cube of a DCA1000 capture, int16 (frames, 4, 192, 256, 2), or its
// fp32 sums unrounded.  New, no reference counterpart.  The model and the arithmetic rule are stated in full in section (a16) of
// include/hupr.h: geometry and the two phase fractions in fp64, the phase of a sample on a 32-bit numerically controlled oscillator,
// sine and cosine and the sum over scatterers in fp32, in scatterer order.  One launch, no table in memory, no atomics; every output
// repeats bit for bit.
#include <math.h>

#include "hupr_common.h"

namespace hupr {

constexpr int kRsThreads = 256;     // one lane per ADC sample
constexpr int kRsChunk = 64;        // scatterers staged per pass: 64 scatterers x 4 receivers = one (phi0, dphi, amplitude) per lane
constexpr int kRsMaxS = 4096;

struct RsArray {                    // by value with the launch
    double tx[3][3];
    double rx[4][3];
};

struct RsTerm {                     // 16 B: one ds_read_b128, the same address in every lane (a broadcast)
    unsigned phi0, dphi;
    float amp;
    unsigned pad;
};

// The fp64 half of the rule is written so that numpy gives the same bits operation by operation: no contraction into fused
// multiply-adds here (sqrt and the divisions are correctly rounded on both sides).
#pragma clang fp contract(off)
__device__ __forceinline__ double rs_dist(double px, double py, double pz, const double* a) {
    const double dx = px - a[0], dy = py - a[1], dz = pz - a[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// a fraction of a turn in [0, 1) -> 32-bit fixed point, round to nearest even, 2^32 wrapping to 0
__device__ __forceinline__ unsigned rs_turn_u32(double turns) {
    const double f = turns - floor(turns);
    return (unsigned)(unsigned long long)rint(f * 4294967296.0);
}

__device__ __forceinline__ RsTerm rs_term(const double* __restrict__ pos, const double* __restrict__ vel, float a, const RsArray& arr, int tx,
                                          int rx, double t, double wavelength, double sample_den) {
    RsTerm o = {0u, 0u, 0.0f, 0u};
    const double px = pos[0] + vel[0] * t, py = pos[1] + vel[1] * t, pz = pos[2] + vel[2] * t;
    const double dt = rs_dist(px, py, pz, arr.tx[tx]), dr = rs_dist(px, py, pz, arr.rx[rx]);
    // a NaN or infinite position or velocity makes both distances non-finite; amplitudes that are 0, negative or not finite hide too
    if (!(a > 0.0f) || !isfinite(a) || !isfinite(dt) || !isfinite(dr) || dt == 0.0 || dr == 0.0) return o;
    const double path = dt + dr;
    o.phi0 = rs_turn_u32(path / wavelength);
    o.dphi = rs_turn_u32(path / sample_den);
    o.amp = (float)((double)a / (dt * dr));
    return o;
}
#pragma clang fp contract(fast)

template <bool kF32> struct RsOut;
template <> struct RsOut<false> {
    typedef unsigned T;             // I in the low half, Q in the high half
    static __device__ __forceinline__ T make(float re, float im) {
        const int i = (int)fminf(fmaxf(rintf(re), -32768.0f), 32767.0f), q = (int)fminf(fmaxf(rintf(im), -32768.0f), 32767.0f);
        return ((unsigned)i & 0xffffu) | ((unsigned)q << 16);
    }
};
template <> struct RsOut<true> {
    typedef float2 T;
    static __device__ __forceinline__ T make(float re, float im) { return make_float2(re, im); }
};

// One workgroup per (frame, chirp): the four receivers' rows of 256 samples, lane = sample.  Per chunk of 64 scatterers, lane
// 4 j + r works out scatterer j's term for receiver r in fp64 (the position at the chirp and the transmitter's distance are the same
// for its four lanes) and leaves it in LDS; behind a barrier every lane adds the chunk's terms to its four samples, reading each
// term as one broadcast.  A scatterer hidden from all four receivers is skipped: the branch is on an LDS value, the same in every lane.
template <bool kF32>
__global__ __launch_bounds__(kRsThreads) void hupr_k_radar_scene(const double* __restrict__ pos, const double* __restrict__ vel,
                                                                 const float* __restrict__ amp, RsArray arr, int S, double wavelength,
                                                                 double sample_den, double chirp_period, const float2* __restrict__ add,
                                                                 typename RsOut<kF32>::T* __restrict__ out) {
    __shared__ RsTerm terms[kRsChunk][4];
    __shared__ int live[kRsChunk];

    const int f = blockIdx.x / 192, c = blockIdx.x - f * 192, tx = c % 3;
    const int n = threadIdx.x, j = n >> 2, r = n & 3;
    const double t = (double)c * chirp_period;

    float re[4] = {0.0f, 0.0f, 0.0f, 0.0f}, im[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int base = 0; base < S; base += kRsChunk) {
        const int cnt = min(kRsChunk, S - base);
        if (j < cnt) {
            const long s = (long)f * S + base + j;
            const RsTerm tm = rs_term(pos + 3 * s, vel + 3 * s, amp[s], arr, tx, r, t, wavelength, sample_den);
            terms[j][r] = tm;
            // the four lanes of a scatterer sit in one wave
            const unsigned long long any = __ballot(tm.amp != 0.0f);
            if (r == 0) live[j] = (int)((any >> (n & 63)) & 0xfull) != 0;
        }
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            if (!live[k]) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const RsTerm tm = terms[k][q];
                const unsigned ph = tm.phi0 + (unsigned)n * tm.dphi;
                const float x = (float)(int)ph * 0x1p-32f;               // signed fraction of a turn, [-0.5, 0.5]
                float sn, cs;
                sincospif(2.0f * x, &sn, &cs);
                re[q] = fmaf(tm.amp, cs, re[q]);
                im[q] = fmaf(tm.amp, sn, im[q]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long i = (((long)f * 4 + q) * 192 + c) * 256 + n;
        float a = re[q], b = im[q];
        if (add) {
            const float2 e = add[i];
            a += e.x;
            b += e.y;
        }
        out[i] = RsOut<kF32>::make(a, b);
    }
}

static bool rs_pos(double v) { return isfinite(v) && v > 0.0; }

template <bool kF32>
static int rs_launch(const char* name, const double* pos, const double* vel, const float* amp, const double* tx_host, const double* rx_host,
                     int frames, int S, double wavelength, double range_bin_m, double chirp_period_s, const float* add_or_null, void* out,
                     hupr_stream_t stream) {
    HUPR_REQUIRE(frames >= 0 && frames <= (1 << 20), "%s: bad shape (frames %d must be in [0, 2^20])", name, frames);
    HUPR_REQUIRE(S >= 1 && S <= kRsMaxS, "%s: bad shape (S %d must be in [1, %d])", name, S, kRsMaxS);
    HUPR_REQUIRE(rs_pos(wavelength) && rs_pos(range_bin_m) && rs_pos(chirp_period_s),
                 "%s: bad parameter (wavelength %g, range_bin_m %g and chirp_period_s %g must be positive and finite)", name, wavelength,
                 range_bin_m, chirp_period_s);
    HUPR_REQUIRE(tx_host && rx_host, "%s: null pointer (tx, rx: host arrays)", name);
    RsArray arr;
    for (int i = 0; i < 9; ++i) arr.tx[i / 3][i % 3] = tx_host[i];
    for (int i = 0; i < 12; ++i) arr.rx[i / 3][i % 3] = rx_host[i];
    for (int i = 0; i < 9; ++i) HUPR_REQUIRE(isfinite(tx_host[i]), "%s: bad parameter (tx[%d][%d] is not finite)", name, i / 3, i % 3);
    for (int i = 0; i < 12; ++i) HUPR_REQUIRE(isfinite(rx_host[i]), "%s: bad parameter (rx[%d][%d] is not finite)", name, i / 3, i % 3);
    if (frames == 0) return HUPR_OK;
    HUPR_REQUIRE(pos && vel && amp && out, "%s: null pointer", name);
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(pos) | reinterpret_cast<uintptr_t>(vel) | reinterpret_cast<uintptr_t>(add_or_null)) & 7) == 0,
                 "%s: pos, vel and add must be 8-byte aligned", name);
    HUPR_REQUIRE((reinterpret_cast<uintptr_t>(amp) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (kF32 ? 7 : 3)) == 0,
                 "%s: amp or out misaligned", name);
    HUPR_LAUNCH(hupr_k_radar_scene<kF32>, dim3((unsigned)frames * 192u), dim3(kRsThreads), 0, as_stream(stream), pos, vel, amp, arr, S,
                wavelength, 512.0 * range_bin_m, chirp_period_s, reinterpret_cast<const float2*>(add_or_null),
                static_cast<typename RsOut<kF32>::T*>(out));
    HUPR_LAUNCH_OK(name);
    return HUPR_OK;
}

}  // namespace hupr

using namespace hupr;

extern "C" int hupr_radar_scene_i16(const double* pos, const double* vel, const float* amp, const double* tx_host, const double* rx_host,
                                    int frames, int S, double wavelength, double range_bin_m, double chirp_period_s, const float* add_or_null,
                                    void* out, hupr_stream_t stream) {
    return rs_launch<false>("hupr_radar_scene_i16", pos, vel, amp, tx_host, rx_host, frames, S, wavelength, range_bin_m, chirp_period_s,
                            add_or_null, out, stream);
}

extern "C" int hupr_radar_scene_f32(const double* pos, const double* vel, const float* amp, const double* tx_host, const double* rx_host,
                                    int frames, int S, double wavelength, double range_bin_m, double chirp_period_s, const float* add_or_null,
                                    float* out, hupr_stream_t stream) {
    return rs_launch<true>("hupr_radar_scene_f32", pos, vel, amp, tx_host, rx_host, frames, S, wavelength, range_bin_m, chirp_period_s,
                           add_or_null, out, stream);
}
