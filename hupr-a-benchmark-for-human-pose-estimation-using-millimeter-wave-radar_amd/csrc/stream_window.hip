// Live pose streaming: the per-frame operators of a sliding radar window (tools/stream.py, PoseStream).
//   * the MNet front end over the G-frame window around the frame that is due, fed from a device-resident ring of elevation-mean
//     planes — one new sensor-frame per sensor and lane comes in, G window positions go out
//     [models/networks.py:23-33 on the window datasets/dataset.py:120-139 gathers]
//   * the state advance that follows it (frame / pose counters live on the device, so no launch argument depends on the frame
//     number and one captured graph serves every frame), the reset, and the arg-max -> image-pixel keypoint decode
//     [misc/metrics.py:10-38 times imgSize / heatmapSize, tools/run.py:47-53]
#include "hupr_common.h"
#include "stream_state.h"      // StreamState: the device-resident session state

namespace hupr {

constexpr int kSNF = 32;      // MNet filters (spatial.hip kNF)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One thread = one (lane, window position, pixel) of one sensor (blockIdx.y): 16 coalesced plane reads, 32 channels out — the launch
// shape and, per pixel, the very arithmetic of hupr_k_mnet_fwd_means (same fma order, same max order), so the window is bit-identical
// to that kernel on the gathered planes.  The window position's source frame follows the window rule
// clamp(centre - G/2 + j, 0, newest); the new frame is read from the staging planes, every other one from its ring slot
// (frame mod G).  The threads of window position 0 also file the new planes in the ring: slot newest mod G, which no window
// position of this launch reads from the ring (the only source congruent to it within the last G frames is the new frame itself).
template <typename T>
__global__ __launch_bounds__(256) void hupr_k_mnet_stream(const float* __restrict__ staging, float* __restrict__ ring,
                                                          const StreamState* __restrict__ state, int lookahead, int flush,
                                                          const float* __restrict__ w_h, const float* __restrict__ b_h,
                                                          const float* __restrict__ w_v, const float* __restrict__ b_v,
                                                          T* __restrict__ out_h, T* __restrict__ out_v, int lanes, int G,
                                                          int pixels) {
    __shared__ float sw[kSNF * 4 + kSNF];
    const int sensor = blockIdx.y;
    const float* w = sensor ? w_v : w_h;
    const float* bias = sensor ? b_v : b_h;
    for (int i = threadIdx.x; i < kSNF * 4 + kSNF; i += 256) sw[i] = (i < kSNF * 4) ? w[i] : bias[i - kSNF * 4];
    __syncthreads();
    const int frames = state->frames;
    const int newest = flush ? frames - 1 : frames;
    const int centre = flush ? state->emitted : frames - lookahead;
    T* out = sensor ? out_v : out_h;
    const long total = (long)lanes * G * pixels;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long lg = idx / pixels;
        const int pix = (int)(idx - lg * pixels);
        const int lane = (int)(lg / G), j = (int)(lg - (long)lane * G);
        const int src = clampi(centre - G / 2 + j, 0, newest);
        const long sl = (long)sensor * lanes + lane;                                   // (sensor, lane) index of staging and ring
        const float* stg = staging + sl * 16 * (long)pixels + pix;
        const int slot = ((src % G) + G) % G;                                          // in range whatever the state holds
        const float* xb = (!flush && src == newest) ? stg : ring + (sl * G + slot) * 16 * (long)pixels + pix;
        float m[16];
#pragma unroll
        for (int p = 0; p < 16; ++p) m[p] = xb[(long)p * pixels];
        if (!flush && j == 0) {
            float* dst = ring + (sl * G + ((newest % G) + G) % G) * 16 * (long)pixels + pix;
#pragma unroll
            for (int p = 0; p < 16; ++p) dst[(long)p * pixels] = stg[(long)p * pixels];
        }
        T* o = out + idx * kSNF;
#pragma unroll
        for (int c4 = 0; c4 < kSNF / 4; ++c4) {
            float r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int co = c4 * 4 + k;
                const float w00 = sw[co * 4 + 0], w01 = sw[co * 4 + 1], w10 = sw[co * 4 + 2], w11 = sw[co * 4 + 3];
                float best = -INFINITY;
#pragma unroll
                for (int t2 = 0; t2 < 4; ++t2) {
                    float v = sw[kSNF * 4 + co];
                    v = fmaf(w00, m[2 * t2], v);
                    v = fmaf(w01, m[2 * t2 + 1], v);
                    v = fmaf(w10, m[8 + 2 * t2], v);
                    v = fmaf(w11, m[8 + 2 * t2 + 1], v);
                    best = fmaxf(best, v);
                }
                r[k] = best;
            }
            st_act4(o + c4 * 4, make_float4(r[0], r[1], r[2], r[3]));
        }
    }
}

// The counters move in a launch of their own, behind the window launch on the same stream: that one reads them, nothing hands
// values from workgroup to workgroup inside a launch.
__global__ void hupr_k_stream_advance(StreamState* __restrict__ state, int lookahead, int flush) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int frames = state->frames, emitted = state->emitted;
    if (flush) {
        state->emitted = emitted + 1;
    } else {
        state->frames = frames + 1;
        if (frames - lookahead >= 0) state->emitted = emitted + 1;
    }
}

__global__ void hupr_k_stream_reset(StreamState* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    state->frames = 0;
    state->emitted = 0;
    state->pad[0] = 0;
    state->pad[1] = 0;
}

__global__ __launch_bounds__(64) void hupr_k_stream_keypoints(const int* __restrict__ idx, const float* __restrict__ maxval,
                                                              float* __restrict__ kp, long rows, int W, float ratio) {
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    const int i = idx[r];
    const float keep = maxval[r] > 0.f ? 1.f : 0.f;       // a joint whose maximum is <= 0 decodes to (0, 0) (misc/metrics.py)
    *reinterpret_cast<float2*>(kp + r * 2) = make_float2((float)(i % W) * keep * ratio, (float)(i / W) * keep * ratio);
}

}  // namespace hupr

using namespace hupr;

extern "C" size_t hupr_stream_state_bytes(void) { return sizeof(StreamState); }

extern "C" int hupr_stream_reset(void* state, hupr_stream_t stream) {
    HUPR_REQUIRE(state, "hupr_stream_reset: null state");
    HUPR_LAUNCH(hupr_k_stream_reset, dim3(1), dim3(64), 0, as_stream(stream), static_cast<StreamState*>(state));
    HUPR_LAUNCH_OK("hupr_k_stream_reset");
    return HUPR_OK;
}

extern "C" int hupr_stream_advance(void* state, int lookahead, int flush, hupr_stream_t stream) {
    HUPR_REQUIRE(state, "hupr_stream_advance: null state");
    HUPR_REQUIRE(lookahead >= 0, "hupr_stream_advance: lookahead %d is negative", lookahead);
    HUPR_LAUNCH(hupr_k_stream_advance, dim3(1), dim3(64), 0, as_stream(stream), static_cast<StreamState*>(state), lookahead,
                flush ? 1 : 0);
    HUPR_LAUNCH_OK("hupr_k_stream_advance");
    return HUPR_OK;
}

template <typename T>
static int mnet_stream(const char* who, const float* staging, float* ring, const void* state, int lookahead, int flush,
                       const float* w_h, const float* b_h, const float* w_v, const float* b_v, T* out_h, T* out_v, int lanes,
                       int G, int pixels, hupr_stream_t stream) {
    if (lanes == 0) return HUPR_OK;
    HUPR_REQUIRE(lanes > 0 && pixels > 0, "%s: bad shape (lanes %d, pixels %d)", who, lanes, pixels);
    HUPR_REQUIRE(G >= 2 && G % 2 == 0 && G <= 64, "%s: the window must hold an even number of 2..64 frames, got %d", who, G);
    HUPR_REQUIRE(lookahead >= 0 && lookahead <= G / 2 - 1, "%s: lookahead %d outside 0..%d", who, lookahead, G / 2 - 1);
    HUPR_REQUIRE(ring && state && w_h && b_h && w_v && b_v && out_h && out_v, "%s: null pointer", who);
    HUPR_REQUIRE(flush || staging, "%s: null staging planes (only a flush takes none)", who);
    const long total = (long)lanes * G * pixels;
    const int grid = (int)min((long)4096, (total + 255) / 256);
    HUPR_LAUNCH(hupr_k_mnet_stream<T>, dim3(grid, 2), dim3(256), 0, as_stream(stream), staging, ring,
                static_cast<const StreamState*>(state), lookahead, flush ? 1 : 0, w_h, b_h, w_v, b_v, out_h, out_v, lanes, G,
                pixels);
    HUPR_LAUNCH_OK("hupr_k_mnet_stream");
    return HUPR_OK;
}

extern "C" int hupr_mnet_stream_f32(const float* staging_or_null, float* ring, const void* state, int lookahead, int flush,
                                    const float* w_hori, const float* bias_hori, const float* w_vert, const float* bias_vert,
                                    float* out_hori, float* out_vert, int lanes, int G, int pixels, hupr_stream_t stream) {
    return mnet_stream("hupr_mnet_stream_f32", staging_or_null, ring, state, lookahead, flush, w_hori, bias_hori, w_vert,
                       bias_vert, out_hori, out_vert, lanes, G, pixels, stream);
}
extern "C" int hupr_mnet_stream_bf16act(const float* staging_or_null, float* ring, const void* state, int lookahead, int flush,
                                        const float* w_hori, const float* bias_hori, const float* w_vert,
                                        const float* bias_vert, void* out_hori, void* out_vert, int lanes, int G, int pixels,
                                        hupr_stream_t stream) {
    return mnet_stream("hupr_mnet_stream_bf16act", staging_or_null, ring, state, lookahead, flush, w_hori, bias_hori, w_vert,
                       bias_vert, static_cast<__bf16*>(out_hori), static_cast<__bf16*>(out_vert), lanes, G, pixels, stream);
}

extern "C" int hupr_stream_keypoints_f32(const int* idx, const float* maxval, float* keypoints, long rows, int W, float ratio,
                                         hupr_stream_t stream) {
    if (rows == 0) return HUPR_OK;
    HUPR_REQUIRE(idx && maxval && keypoints && rows > 0 && W > 0, "hupr_stream_keypoints_f32: bad argument");
    HUPR_LAUNCH(hupr_k_stream_keypoints, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, as_stream(stream), idx, maxval,
                keypoints, rows, W, ratio);
    HUPR_LAUNCH_OK("hupr_k_stream_keypoints");
    return HUPR_OK;
}
