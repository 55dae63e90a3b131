// Exponential moving average of the weights, kept and swapped on the device (TRAINING.emaDecay).  The parameters live in flat
// buckets that the fused optimiser updates, possibly inside a replayed hipGraph, and a step skipped by the gradient guard must not
// move the average: so the update is stream-ordered launches behind the optimiser step, with a counter of their own in device
// memory and the guard's decision as an input.  New, no reference counterpart: the reference evaluates self.model as trained
// (tools/run.py:35-63).
//
//   hupr_ema_tick_f32    one thread: ema_state = {updates, weight} for this step (weight = 0 when the guard skipped the step)
//   hupr_ema_update_f32  one launch per bucket: ema += weight * (p - ema)
//   hupr_swap_f32        one launch per bucket: exchange the parameters and their average in place
//
// No atomics: every element belongs to one thread.  HBM-bound streaming: 8 B read + 4 B written (update), 8 B + 8 B (swap) per
// element.  float4 accesses where both arrays share their offset to a 16-byte boundary, a scalar launch otherwise; the update is
// one explicit fmaf on every path, so the bits do not depend on the path.
#include "hupr_common.h"

using namespace hupr;

namespace {
constexpr int kThreads = 256;
constexpr long kMaxBlocks = 2048;     // 8 workgroups per CU on 256 CUs; the rest of the array is walked grid-stride

// THE update, for every path: e + w (p - e) as one subtraction and one fused multiply-add
__device__ __forceinline__ float ema1(float e, float p, float w) { return __builtin_fmaf(w, p - e, e); }
__device__ __forceinline__ float4 ema4(float4 e, const float4 p, float w) {
    e.x = ema1(e.x, p.x, w);
    e.y = ema1(e.y, p.y, w);
    e.z = ema1(e.z, p.z, w);
    e.w = ema1(e.w, p.w, w);
    return e;
}

dim3 grid_for(long items) {
    long b = (items + kThreads - 1) / kThreads;
    return dim3((unsigned)(b < 1 ? 1 : b > kMaxBlocks ? kMaxBlocks : b));
}

// scalar elements in front of the first 16-byte boundary of q, at most n
long head_of(const float* q, long n) {
    const long head = (long)(((16 - (reinterpret_cast<uintptr_t>(q) & 15)) & 15) >> 2);
    return head > n ? n : head;
}
bool congruent16(const float* a, const float* b) {
    return ((reinterpret_cast<uintptr_t>(a) ^ reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}
}  // namespace

// state = {updates, weight}; guard = null or {coef, norm, skipped, finite} of hupr_k_grad_guard
__global__ void hupr_k_ema_tick(float* __restrict__ state, float decay, const float* __restrict__ guard) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (guard && guard[3] == 0.f) {                         // the step did not happen: the average and its count stay
        state[1] = 0.f;
        return;
    }
    const double k = (double)state[0];
    const double d = fmin((double)decay, (1.0 + k) / (10.0 + k));      // warm-up ramp: 0.1, 0.18, 0.25, ... up to decay
    state[1] = (float)(1.0 - d);
    state[0] = (float)(k + 1.0);
}

// ema[head ...] and p[head ...] are 16-byte aligned (head <= 3 scalar elements in front, < 4 behind the last whole float4)
__global__ __launch_bounds__(kThreads) void hupr_k_ema_update(float* __restrict__ ema, const float* __restrict__ p, long n, long head,
                                                              const float* __restrict__ state) {
    const float w = state[1];
    if (w == 0.f) return;                                   // skipped step: the same for every thread, nothing is stored
    const long tid = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
    const long n4 = (n - head) >> 2;
    float4* __restrict__ e4 = reinterpret_cast<float4*>(ema + head);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
    long i = tid;
    for (; i + 3 * stride < n4; i += 4 * stride) {          // eight loads in flight per thread
        const float4 ea = e4[i], eb = e4[i + stride], ec = e4[i + 2 * stride], ed = e4[i + 3 * stride];
        const float4 pa = p4[i], pb = p4[i + stride], pc = p4[i + 2 * stride], pd = p4[i + 3 * stride];
        e4[i] = ema4(ea, pa, w);
        e4[i + stride] = ema4(eb, pb, w);
        e4[i + 2 * stride] = ema4(ec, pc, w);
        e4[i + 3 * stride] = ema4(ed, pd, w);
    }
    for (; i < n4; i += stride) e4[i] = ema4(e4[i], p4[i], w);
    if (tid < head) ema[tid] = ema1(ema[tid], p[tid], w);
    for (long j = head + (n4 << 2) + tid; j < n; j += stride) ema[j] = ema1(ema[j], p[j], w);
}

// ema and p differ in their offset to a 16-byte boundary: 4-byte accesses
__global__ __launch_bounds__(kThreads) void hupr_k_ema_update_scalar(float* __restrict__ ema, const float* __restrict__ p, long n,
                                                                     const float* __restrict__ state) {
    const float w = state[1];
    if (w == 0.f) return;
    const long stride = (long)gridDim.x * kThreads;
    for (long j = (long)blockIdx.x * kThreads + threadIdx.x; j < n; j += stride) ema[j] = ema1(ema[j], p[j], w);
}

__global__ __launch_bounds__(kThreads) void hupr_k_swap(float* __restrict__ a, float* __restrict__ b, long n, long head) {
    const long tid = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
    const long n4 = (n - head) >> 2;
    float4* __restrict__ a4 = reinterpret_cast<float4*>(a + head);
    float4* __restrict__ b4 = reinterpret_cast<float4*>(b + head);
    long i = tid;
    for (; i + stride < n4; i += 2 * stride) {              // four loads in flight per thread
        const float4 x0 = a4[i], x1 = a4[i + stride], y0 = b4[i], y1 = b4[i + stride];
        a4[i] = y0;
        a4[i + stride] = y1;
        b4[i] = x0;
        b4[i + stride] = x1;
    }
    for (; i < n4; i += stride) {
        const float4 x = a4[i], y = b4[i];
        a4[i] = y;
        b4[i] = x;
    }
    if (tid < head) {
        const float x = a[tid];
        a[tid] = b[tid];
        b[tid] = x;
    }
    for (long j = head + (n4 << 2) + tid; j < n; j += stride) {
        const float x = a[j];
        a[j] = b[j];
        b[j] = x;
    }
}

__global__ __launch_bounds__(kThreads) void hupr_k_swap_scalar(float* __restrict__ a, float* __restrict__ b, long n) {
    const long stride = (long)gridDim.x * kThreads;
    for (long j = (long)blockIdx.x * kThreads + threadIdx.x; j < n; j += stride) {
        const float x = a[j];
        a[j] = b[j];
        b[j] = x;
    }
}

extern "C" int hupr_ema_tick_f32(float* ema_state, float decay, const float* guard, hupr_stream_t stream) {
    HUPR_REQUIRE(ema_state, "hupr_ema_tick_f32: bad argument (null ema_state)");
    HUPR_REQUIRE(decay > 0.f && decay < 1.f, "hupr_ema_tick_f32: decay must be inside (0, 1), got %g", (double)decay);
    HUPR_LAUNCH(hupr_k_ema_tick, dim3(1), dim3(1), 0, as_stream(stream), ema_state, decay, guard);
    HUPR_LAUNCH_OK("hupr_k_ema_tick");
    return HUPR_OK;
}

extern "C" int hupr_ema_update_f32(float* ema, const float* p, long n, const float* ema_state, hupr_stream_t stream) {
    HUPR_REQUIRE(ema && p && ema_state && n > 0, "hupr_ema_update_f32: bad argument (null pointer or n <= 0)");
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(p)) & 3) == 0,
                 "hupr_ema_update_f32: ema and p must be 4-byte aligned");
    if (congruent16(ema, p)) {
        const long head = head_of(ema, n);
        HUPR_LAUNCH(hupr_k_ema_update, grid_for(((n - head) >> 2) / 4), dim3(kThreads), 0, as_stream(stream), ema, p, n, head,
                    ema_state);
        HUPR_LAUNCH_OK("hupr_k_ema_update");
    } else {
        HUPR_LAUNCH(hupr_k_ema_update_scalar, grid_for(n), dim3(kThreads), 0, as_stream(stream), ema, p, n, ema_state);
        HUPR_LAUNCH_OK("hupr_k_ema_update_scalar");
    }
    return HUPR_OK;
}

extern "C" int hupr_swap_f32(float* a, float* b, long n, hupr_stream_t stream) {
    HUPR_REQUIRE(a && b && n > 0, "hupr_swap_f32: bad argument (null pointer or n <= 0)");
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) == 0,
                 "hupr_swap_f32: a and b must be 4-byte aligned");
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)n * 4;
    HUPR_REQUIRE(ua + bytes <= ub || ub + bytes <= ua, "hupr_swap_f32: the two ranges overlap");
    if (congruent16(a, b)) {
        const long head = head_of(a, n);
        HUPR_LAUNCH(hupr_k_swap, grid_for(((n - head) >> 2) / 2), dim3(kThreads), 0, as_stream(stream), a, b, n, head);
        HUPR_LAUNCH_OK("hupr_k_swap");
    } else {
        HUPR_LAUNCH(hupr_k_swap_scalar, grid_for(n), dim3(kThreads), 0, as_stream(stream), a, b, n);
        HUPR_LAUNCH_OK("hupr_k_swap_scalar");
    }
    return HUPR_OK;
}
