// Gradient guard: the global L2 norm of the flat gradient buckets, the clip_grad_norm_ coefficient and the finite / skip decision,
// all on the device, so that a step replayed from a hipGraph is protected as well (the host cannot look between backward and
// the optimiser there).  New, no reference counterpart: the reference steps on whatever backward left (tools/run.py:78-79).
//
//   hupr_grad_sumsq_f32    one launch per bucket: kPartials fp64 partial sums of g^2
//   hupr_grad_guard_f32    one workgroup: total -> {coef, norm, skipped, finite}, and the step count of dev_state
//   hupr_*_step_guard_f32  (head.hip) the optimiser steps that obey the decision
//
// No atomics anywhere: which thread adds which element, and every reduction order, are fixed by (n, alignment of g) alone, so
// the result is bit-identical from run to run.  HBM-bound: 4 B read per element, once per step.
#include "hupr_common.h"

using namespace hupr;

namespace {
constexpr int kPartials = 1024;       // workgroups per hupr_grad_sumsq_f32 launch = partials it writes (4 per CU on 256 CUs)
constexpr int kThreads = 256;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the workgroup's 256 threads, valid in thread 0: wave butterflies, then the four wave sums in wave order
__device__ __forceinline__ double block_sum_f64(double v) {
    __shared__ double wsum[kThreads / 64];
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) t += wsum[w];
    }
    return t;
}

__device__ __forceinline__ double sq4(double acc, const float4 v) {
    acc = fma((double)v.x, (double)v.x, acc);
    acc = fma((double)v.y, (double)v.y, acc);
    acc = fma((double)v.z, (double)v.z, acc);
    return fma((double)v.w, (double)v.w, acc);
}
}  // namespace

// g[head ...] is 16-byte aligned (head <= 3 scalar elements in front of it, < 4 behind the last whole float4).  Each thread sums in
// fp64: the square of any finite fp32 is finite there (3.4e38^2 = 1.2e77), and n of them cannot reach 1.8e308.
__global__ __launch_bounds__(kThreads) void hupr_k_grad_sumsq(const float* __restrict__ g, long n, long head,
                                                              double* __restrict__ partials) {
    const long tid = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
    const long n4 = (n - head) >> 2;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
    double acc = 0.0;
    long i = tid;
    for (; i + 3 * stride < n4; i += 4 * stride) {          // four loads in flight per thread
        const float4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
        acc = sq4(sq4(sq4(sq4(acc, a), b), c), d);
    }
    for (; i < n4; i += stride) acc = sq4(acc, g4[i]);
    if (tid < head) acc = fma((double)g[tid], (double)g[tid], acc);
    for (long j = head + (n4 << 2) + tid; j < n; j += stride) acc = fma((double)g[j], (double)g[j], acc);
    const double t = block_sum_f64(acc);                    // 0.0 from a workgroup that had no element
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// guard = {coef, norm, skipped, finite}; state = {lr, step}.  One workgroup; thread t sums partials t, t + 256, ... in order.
__global__ __launch_bounds__(kThreads) void hupr_k_grad_guard(const double* __restrict__ partials, int count, float gscale,
                                                              float max_norm, float* __restrict__ state,
                                                              float* __restrict__ guard) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += kThreads) acc += partials[i];
    const double total = block_sum_f64(acc);
    if (threadIdx.x != 0) return;
    if (!(total <= 1.7976931348623157e308)) {               // +inf or NaN (a sum of squares is never negative)
        guard[0] = 0.f;
        guard[1] = (float)((double)gscale * sqrt(total));
        guard[2] += 1.f;
        guard[3] = 0.f;
        return;                                             // the step count does not move: the step did not happen
    }
    const double norm = (double)gscale * sqrt(total);
    const double coef = fmin(1.0, (double)max_norm / (norm + 1e-6));      // torch.nn.utils.clip_grad_norm_; max_norm = +inf -> 1
    guard[0] = (float)coef;
    guard[1] = (float)norm;
    guard[3] = 1.f;
    state[1] += 1.f;
}

extern "C" int hupr_grad_sumsq_partials(void) { return kPartials; }

extern "C" int hupr_grad_sumsq_f32(const float* g, long n, double* partials, hupr_stream_t stream) {
    HUPR_REQUIRE(g && partials && n > 0, "hupr_grad_sumsq_f32: bad argument (null pointer or n <= 0)");
    HUPR_REQUIRE((reinterpret_cast<uintptr_t>(g) & 3) == 0 && (reinterpret_cast<uintptr_t>(partials) & 7) == 0,
                 "hupr_grad_sumsq_f32: g must be 4-byte and partials 8-byte aligned");
    long head = (long)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2);      // scalar elements before the first aligned float4
    if (head > n) head = n;
    HUPR_LAUNCH(hupr_k_grad_sumsq, dim3(kPartials), dim3(kThreads), 0, as_stream(stream), g, n, head, partials);
    HUPR_LAUNCH_OK("hupr_k_grad_sumsq");
    return HUPR_OK;
}

extern "C" int hupr_grad_guard_f32(const double* partials, int count, float gscale, float max_norm, float* dev_state, float* guard,
                                   hupr_stream_t stream) {
    HUPR_REQUIRE(partials && dev_state && guard && count > 0, "hupr_grad_guard_f32: bad argument (null pointer or count <= 0)");
    HUPR_REQUIRE(max_norm > 0.f, "hupr_grad_guard_f32: max_norm must be positive (+inf = no clipping), got %g", (double)max_norm);
    HUPR_LAUNCH(hupr_k_grad_guard, dim3(1), dim3(kThreads), 0, as_stream(stream), partials, count, gscale, max_norm, dev_state,
                guard);
    HUPR_LAUNCH_OK("hupr_k_grad_guard");
    return HUPR_OK;
}
