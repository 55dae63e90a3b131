// The optimiser family: the fused Adam, SGD-momentum and LAMB steps, the gradient guard in front of them and the weight average behind
// them.  All of it streams over the flat parameter / gradient buckets once per step and is HBM-bound.
//
// Adam and SGD (reference tools/base.py:44-47: SGD momentum 0.9 / Adam, coupled L2 decay), three forms each:
//   hupr_*_step_f32        learning rate and step count as launch arguments
//   hupr_*_step_dev_f32    {lr, step} read from device memory: usable inside a captured hipGraph, whose launch arguments are frozen
//   hupr_*_step_guard_f32  the _dev form that obeys the gradient guard's decision
//
// Gradient guard: the global L2 norm of the flat gradient buckets, the clip_grad_norm_ coefficient and the finite / skip decision,
// all on the device, so that a step replayed from a hipGraph is protected as well (the host cannot look between backward and
// the optimiser there).  New, no reference counterpart: the reference steps on whatever backward left (tools/run.py:78-79).
//   hupr_grad_sumsq_f32    one launch per bucket: kPartials fp64 partial sums of g^2
//   hupr_grad_guard_f32    one workgroup: total -> {coef, norm, skipped, finite}, and the step count of dev_state
// 4 B read per element, once per step.
//
// Exponential moving average of the weights, kept and swapped on the device (TRAINING.emaDecay).  The parameters live in flat
// buckets that the fused optimiser updates, possibly inside a replayed hipGraph, and a step skipped by the gradient guard must not
// move the average: so the update is stream-ordered launches behind the optimiser step, with a counter of their own in device
// memory and the guard's decision as an input.  New, no reference counterpart: the reference evaluates self.model as trained
// (tools/run.py:35-63).
//   hupr_ema_tick_f32      one thread: ema_state = {updates, weight} for this step (weight = 0 when the guard skipped the step)
//   hupr_ema_update_f32    one launch per bucket: ema += weight * (p - ema)
//   hupr_swap_f32          one launch per bucket: exchange the parameters and their average in place
// 8 B read + 4 B written (update), 8 B + 8 B (swap) per element.  float4 accesses where both arrays share their offset to a 16-byte
// boundary, 4-byte accesses otherwise; the update is one explicit fmaf on every path, so the bits do not depend on the path.
//
// LAMB (You et al. 2020, the update rule of apex's FusedLAMB): Adam's direction rescaled per parameter tensor by the trust ratio
// |p| / |u|.  New, no reference counterpart (the reference's choice is tools/base.py:44-47).  A parameter tensor is a segment of its
// flat bucket; the norms per tensor are a segmented reduction over a chunk table built on the host from the bucket layout: every
// segment is cut from its own start into chunks of kLambChunk elements, so a chunk never spans two tensors.
//   hupr_lamb_stage1_f32   one launch per bucket, one workgroup per chunk: new m and v, u, one fp64 pair {sum p^2, sum u^2} per chunk
//   hupr_lamb_ratio_f32    one launch per bucket, one workgroup per segment: the chunk pairs added in table order -> |p|, |u|, r
//   hupr_lamb_stage2_f32   one launch per bucket: u recomputed from p, m, v by stage 1's lamb_u, p <- p - lr r u
// 16 B read + 8 B written (stage 1), 12 B + 4 B (stage 2): 40 B per element, as much as a stored u would cost.  {lr, step} always
// come from device memory and the guard pointer is nullable.  Thread t of a chunk's workgroup takes elements 4t .. 4t + 3 of every
// 1024 of the chunk, as one float4 where the chunk starts on a 16-byte boundary in every array and 4 bytes at a time otherwise,
// through the same per-element function: which thread adds which element depends on the segment lengths alone.
//
// No atomics anywhere: every element belongs to one thread, and which thread adds which element of the square sum, and every
// reduction order, are fixed by (n, alignment of g) alone, so the result is bit-identical from run to run.
#include <type_traits>

#include "hupr_common.h"

using namespace hupr;

namespace {
constexpr int kThreads = 256;
constexpr int kPartials = 1024;       // workgroups per hupr_grad_sumsq_f32 launch = partials it writes (4 per CU on 256 CUs)
constexpr long kMaxBlocks = 2048;     // 8 workgroups per CU on 256 CUs; the rest of the array is walked grid-stride
constexpr long kAdamBlocks = 8192;
constexpr int kLambChunk = 2048;      // elements per chunk of the LAMB table = per workgroup of stages 1 and 2: two rounds of 256 float4

template <int U> using Unroll = std::integral_constant<int, U>;

// THE walk over a flat bucket a[0 .. n): `head` (<= 3) scalar elements in front of the first 16-byte boundary, n4 float4 from
// there, fewer than 4 scalar elements behind (n4 = 0: every element goes through the last loop, 4 bytes at a time).  Thread tid of
// the grid takes float4 tid, tid + stride, ..., U of them per round (vec(i, stride, Unroll<U>) issues its loads together) and one
// at a time (vec(i, stride, Unroll<1>)) once fewer than U are left; then scalar element tid of the head and its share of the tail.
template <int U, typename Vec, typename Elem>
__device__ __forceinline__ void walk_flat(long n, long head, long n4, Vec vec, Elem elem) {
    const long tid = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
    long i = tid;
    if constexpr (U > 1)
        for (; i + (U - 1) * stride < n4; i += U * stride) vec(i, stride, Unroll<U>());
    for (; i < n4; i += stride) vec(i, stride, Unroll<1>());
    if (tid < head) elem(tid);
    for (long j = head + (n4 << 2) + tid; j < n; j += stride) elem(j);
}

// ---- host side: how a launch walks its bucket ----
// scalar elements in front of the first 16-byte boundary of q, at most n
long head_of(const float* q, long n) {
    const long head = (long)(((16 - (reinterpret_cast<uintptr_t>(q) & 15)) & 15) >> 2);
    return head > n ? n : head;
}
// the arrays share their offset to a 16-byte boundary
bool congruent16(const float* a, const float* b, const float* c = nullptr) {
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b), uc = c ? reinterpret_cast<uintptr_t>(c) : ua;
    return (((ua ^ ub) | (ua ^ uc)) & 15) == 0;
}
// head and float4 count of the walk over n elements from a: float4 where vec (every array shares a's offset), else 4 bytes at a time
struct Span { long head, n4; };
Span span_of(const float* a, long n, bool vec) {
    const long head = vec ? head_of(a, n) : 0;
    return {head, vec ? (n - head) >> 2 : 0};
}
// ceil(items / per_block) workgroups, at least 1 and at most cap
dim3 grid_for(long items, long cap, long per_block = kThreads) {
    const long b = (items + per_block - 1) / per_block;
    return dim3((unsigned)(b < 1 ? 1 : b > cap ? cap : b));
}

__device__ __forceinline__ double sq4(double acc, const float4 v) {
    acc = fma((double)v.x, (double)v.x, acc);
    acc = fma((double)v.y, (double)v.y, acc);
    acc = fma((double)v.z, (double)v.z, acc);
    return fma((double)v.w, (double)v.w, acc);
}

// THE update of the average, for every path: e + w (p - e) as one subtraction and one fused multiply-add
__device__ __forceinline__ float ema1(float e, float p, float w) { return __builtin_fmaf(w, p - e, e); }
__device__ __forceinline__ float4 ema4(float4 e, const float4 p, float w) {
    e.x = ema1(e.x, p.x, w);
    e.y = ema1(e.y, p.y, w);
    e.z = ema1(e.z, p.z, w);
    e.w = ema1(e.w, p.w, w);
    return e;
}
}  // namespace

namespace hupr {

// ---- Adam with coupled L2 weight decay (torch.optim.Adam semantics), one flat launch --------------
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                          float bc1, float bc2_sqrt, float gscale) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float pv = p[i];
        const float gr = fmaf(wd, pv, g[i] * gscale);
        const float mv = fmaf(b1, m[i], (1.f - b1) * gr);
        const float vv = fmaf(b2, v[i], (1.f - b2) * gr * gr);
        m[i] = mv;
        v[i] = vv;
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        p[i] = pv - (lr / bc1) * (mv / denom);
    }
}

__global__ __launch_bounds__(256) void hupr_k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                   float wd, float bc1, float bc2_sqrt, float gscale) {
    adam_body(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
}

// the bias corrections of step `step` as hupr_adam_step_f32 forms them on the host
__device__ __forceinline__ void adam_bias_corrections(float b1, float b2, float step_f, float& bc1, float& bc2_sqrt) {
    const double step = (double)step_f;
    bc1 = (float)(1.0 - pow((double)b1, step));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, step));
}

// same update with the learning rate and the step count read from device memory (state = {lr, step}): the launch
// arguments of a captured hipGraph are frozen, the bias corrections must not be
__global__ __launch_bounds__(256) void hupr_k_adam_dev(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long n, const float* __restrict__ state, float b1,
                                                       float b2, float eps, float wd, float gscale) {
    float bc1, bc2_sqrt;
    adam_bias_corrections(b1, b2, state[1], bc1, bc2_sqrt);
    adam_body(p, g, m, v, n, state[0], b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
}

// hupr_k_adam_dev behind the gradient guard (guard = {coef, norm, skipped, finite}): nothing is written when the
// step's gradients were not finite, otherwise the gradient scale carries the clipping coefficient (one fp32 product; coef = 1
// leaves gscale's bits, so the unclipped step is hupr_k_adam_dev's)
__global__ __launch_bounds__(256) void hupr_k_adam_guard(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, long n, const float* __restrict__ state,
                                                         const float* __restrict__ guard, float b1, float b2, float eps, float wd,
                                                         float gscale) {
    if (guard[3] == 0.f) return;
    float bc1, bc2_sqrt;
    adam_bias_corrections(b1, b2, state[1], bc1, bc2_sqrt);
    adam_body(p, g, m, v, n, state[0], b1, b2, eps, wd, bc1, bc2_sqrt, gscale * guard[0]);
}

// ---- SGD with momentum and coupled L2 weight decay (torch.optim.SGD, dampening 0, no Nesterov), one flat launch -------------
// torch's single-tensor order of roundings: d = g + wd * p (one fma), buf = (buf * m) + d (two roundings: mul_ then add_, not
// fused), p = p - lr * buf (one fma).  The first step copies d into the buffer as torch's clone(d_p) does: buf * m + d over a
// zero buffer would turn a -0 of d into +0.  Measured bit-identical to torch.optim.SGD's foreach and single-tensor paths on
// the MI355X.  20 B per element, HBM-bound: float4 when p, g and buf are all 16-byte aligned.
__device__ __forceinline__ float sgd_elem(float& p, float g, float buf, float lr, float m, float wd, float gscale, bool first) {
#pragma clang fp contract(off)
    const float d = fmaf(wd, p, g * gscale);
    const float b = first ? d : buf * m + d;
    p = fmaf(-lr, b, p);
    return b;
}

// the walk without a head, one float4 per round: n4 = n / 4 when all three arrays are 16-byte aligned, 0 otherwise
__device__ __forceinline__ void sgd_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                         long n4, float lr, float m, float wd, float gscale, bool first) {
    walk_flat<1>(
        n, 0, n4,
        [&](long i, long, Unroll<1>) {
            float4 pv = reinterpret_cast<const float4*>(p)[i];
            const float4 gv = reinterpret_cast<const float4*>(g)[i];
            float4 bv = reinterpret_cast<const float4*>(buf)[i];
            bv.x = sgd_elem(pv.x, gv.x, bv.x, lr, m, wd, gscale, first);
            bv.y = sgd_elem(pv.y, gv.y, bv.y, lr, m, wd, gscale, first);
            bv.z = sgd_elem(pv.z, gv.z, bv.z, lr, m, wd, gscale, first);
            bv.w = sgd_elem(pv.w, gv.w, bv.w, lr, m, wd, gscale, first);
            reinterpret_cast<float4*>(p)[i] = pv;
            reinterpret_cast<float4*>(buf)[i] = bv;
        },
        [&](long i) {
            float pv = p[i];
            buf[i] = sgd_elem(pv, g[i], buf[i], lr, m, wd, gscale, first);
            p[i] = pv;
        });
}

__global__ __launch_bounds__(256) void hupr_k_sgd(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  long n, long n4, float lr, float m, float wd, float gscale, int first) {
    sgd_body(p, g, buf, n, n4, lr, m, wd, gscale, first != 0);
}

// same update with the learning rate and the step count read from device memory (state = {lr, step}, the layout of
// hupr_k_adam_dev): "first" is step == 1, so a captured hipGraph replays the right branch
__global__ __launch_bounds__(256) void hupr_k_sgd_dev(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                      long n, long n4, const float* __restrict__ state, float m, float wd,
                                                      float gscale) {
    sgd_body(p, g, buf, n, n4, state[0], m, wd, gscale, state[1] == 1.f);
}

// hupr_k_sgd_dev behind the gradient guard, as hupr_k_adam_guard
__global__ __launch_bounds__(256) void hupr_k_sgd_guard(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                        long n, long n4, const float* __restrict__ state,
                                                        const float* __restrict__ guard, float m, float wd, float gscale) {
    if (guard[3] == 0.f) return;
    sgd_body(p, g, buf, n, n4, state[0], m, wd, gscale * guard[0], state[1] == 1.f);
}

}  // namespace hupr

// ---- gradient guard ----
// g[head ...] is 16-byte aligned.  Each thread sums in fp64, four loads in flight: the square of any finite fp32 is finite there
// (3.4e38^2 = 1.2e77), and n of them cannot reach 1.8e308.
__global__ __launch_bounds__(kThreads) void hupr_k_grad_sumsq(const float* __restrict__ g, long n, long head, long n4,
                                                              double* __restrict__ partials) {
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
    double acc = 0.0;
    walk_flat<4>(
        n, head, n4,
        [&](long i, long stride, auto u) {
            constexpr int U = decltype(u)::value;
            float4 v[U];
#pragma unroll
            for (int k = 0; k < U; ++k) v[k] = g4[i + k * stride];
#pragma unroll
            for (int k = 0; k < U; ++k) acc = sq4(acc, v[k]);
        },
        [&](long j) { acc = fma((double)g[j], (double)g[j], acc); });
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

// ---- weight average ----
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

// ema[head ...] and p[head ...] are 16-byte aligned, eight loads in flight per thread; n4 = 0 when the two differ in their offset
// to a 16-byte boundary
__global__ __launch_bounds__(kThreads) void hupr_k_ema_update(float* __restrict__ ema, const float* __restrict__ p, long n, long head,
                                                              long n4, const float* __restrict__ state) {
    const float w = state[1];
    if (w == 0.f) return;                                   // skipped step: the same for every thread, nothing is stored
    float4* __restrict__ e4 = reinterpret_cast<float4*>(ema + head);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
    walk_flat<4>(
        n, head, n4,
        [&](long i, long stride, auto u) {
            constexpr int U = decltype(u)::value;
            float4 e[U], q[U];
#pragma unroll
            for (int k = 0; k < U; ++k) e[k] = e4[i + k * stride];
#pragma unroll
            for (int k = 0; k < U; ++k) q[k] = p4[i + k * stride];
#pragma unroll
            for (int k = 0; k < U; ++k) e4[i + k * stride] = ema4(e[k], q[k], w);
        },
        [&](long j) { ema[j] = ema1(ema[j], p[j], w); });
}

// as hupr_k_ema_update, four loads in flight per thread (native vectors: an array of float4 structs that is only copied ends up in LDS)
__global__ __launch_bounds__(kThreads) void hupr_k_swap(float* __restrict__ a, float* __restrict__ b, long n, long head, long n4) {
    hupr_f32x4* __restrict__ a4 = reinterpret_cast<hupr_f32x4*>(a + head);
    hupr_f32x4* __restrict__ b4 = reinterpret_cast<hupr_f32x4*>(b + head);
    walk_flat<2>(
        n, head, n4,
        [&](long i, long stride, auto u) {
            constexpr int U = decltype(u)::value;
            hupr_f32x4 x[U], y[U];
#pragma unroll
            for (int k = 0; k < U; ++k) x[k] = a4[i + k * stride];
#pragma unroll
            for (int k = 0; k < U; ++k) y[k] = b4[i + k * stride];
#pragma unroll
            for (int k = 0; k < U; ++k) a4[i + k * stride] = y[k];
#pragma unroll
            for (int k = 0; k < U; ++k) b4[i + k * stride] = x[k];
        },
        [&](long j) {
            const float x = a[j];
            a[j] = b[j];
            b[j] = x;
        });
}

// ---- entries ----
// step = 1-based step count after increment; gscale multiplies the gradient (e.g. 1/world_size)
extern "C" int hupr_adam_step_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int step, float gscale, hupr_stream_t stream) {
    HUPR_REQUIRE(p && g && exp_avg && exp_avg_sq && n > 0 && step >= 1, "hupr_adam_step_f32: bad argument");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    HUPR_LAUNCH(hupr_k_adam, grid_for(n, kAdamBlocks), dim3(256), 0, as_stream(stream), p, g, exp_avg, exp_avg_sq, n, lr,
                       beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), gscale);
    HUPR_LAUNCH_OK("hupr_k_adam");
    return HUPR_OK;
}

// Same as hupr_adam_step_f32 with {lr, step} in device memory (dev_state[0] = learning rate, dev_state[1] = step count,
// both float): usable inside a captured hipGraph whose launch arguments are frozen.
extern "C" int hupr_adam_step_dev_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n,
                                      const float* dev_state, float beta1, float beta2, float eps, float weight_decay,
                                      float gscale, hupr_stream_t stream) {
    HUPR_REQUIRE(p && g && exp_avg && exp_avg_sq && dev_state && n > 0, "hupr_adam_step_dev_f32: bad argument");
    HUPR_LAUNCH(hupr_k_adam_dev, grid_for(n, kAdamBlocks), dim3(256), 0, as_stream(stream), p, g, exp_avg, exp_avg_sq, n,
                       dev_state, beta1, beta2, eps, weight_decay, gscale);
    HUPR_LAUNCH_OK("hupr_k_adam_dev");
    return HUPR_OK;
}

// hupr_adam_step_dev_f32 behind the gradient guard: guard = the 4 floats hupr_grad_guard_f32 wrote on this stream before
extern "C" int hupr_adam_step_guard_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n,
                                        const float* dev_state, const float* guard, float beta1, float beta2, float eps,
                                        float weight_decay, float gscale, hupr_stream_t stream) {
    HUPR_REQUIRE(p && g && exp_avg && exp_avg_sq && dev_state && guard && n > 0,
                 "hupr_adam_step_guard_f32: bad argument (null pointer or n <= 0)");
    HUPR_LAUNCH(hupr_k_adam_guard, grid_for(n, kAdamBlocks), dim3(256), 0, as_stream(stream), p, g, exp_avg, exp_avg_sq, n,
                dev_state, guard, beta1, beta2, eps, weight_decay, gscale);
    HUPR_LAUNCH_OK("hupr_k_adam_guard");
    return HUPR_OK;
}

// float4 path only when all three streams are 16-byte aligned; grid = min(ceil(n / (256 * 4)), 2048) with a grid-stride loop
static inline long sgd_n4(const float* p, const float* g, const float* buf, long n) {
    return span_of(p, n, congruent16(p, g, buf) && head_of(p, n) == 0).n4;
}

// first != 0: the parameter's first step (the buffer's old contents are ignored); gscale multiplies the gradient (e.g. 1/world_size)
extern "C" int hupr_sgd_step_f32(float* p, const float* g, float* momentum_buf, long n, float lr, float momentum,
                                 float weight_decay, int first, float gscale, hupr_stream_t stream) {
    HUPR_REQUIRE(p && g && momentum_buf && n > 0, "hupr_sgd_step_f32: bad argument (null pointer or n <= 0)");
    HUPR_LAUNCH(hupr_k_sgd, grid_for(n, kMaxBlocks, 4 * kThreads), dim3(256), 0, as_stream(stream), p, g, momentum_buf, n,
                sgd_n4(p, g, momentum_buf, n), lr, momentum, weight_decay, gscale, first != 0);
    HUPR_LAUNCH_OK("hupr_k_sgd");
    return HUPR_OK;
}

// Same as hupr_sgd_step_f32 with {lr, step} in device memory (dev_state[0] = learning rate, dev_state[1] = step count after
// this step's increment, both float; step 1 is the first step): usable inside a captured hipGraph.
extern "C" int hupr_sgd_step_dev_f32(float* p, const float* g, float* momentum_buf, long n, const float* dev_state,
                                     float momentum, float weight_decay, float gscale, hupr_stream_t stream) {
    HUPR_REQUIRE(p && g && momentum_buf && dev_state && n > 0, "hupr_sgd_step_dev_f32: bad argument (null pointer or n <= 0)");
    HUPR_LAUNCH(hupr_k_sgd_dev, grid_for(n, kMaxBlocks, 4 * kThreads), dim3(256), 0, as_stream(stream), p, g, momentum_buf, n,
                sgd_n4(p, g, momentum_buf, n), dev_state, momentum, weight_decay, gscale);
    HUPR_LAUNCH_OK("hupr_k_sgd_dev");
    return HUPR_OK;
}

// hupr_sgd_step_dev_f32 behind the gradient guard (hupr_grad_guard_f32 advanced dev_state[1] on this stream before)
extern "C" int hupr_sgd_step_guard_f32(float* p, const float* g, float* momentum_buf, long n, const float* dev_state,
                                       const float* guard, float momentum, float weight_decay, float gscale, hupr_stream_t stream) {
    HUPR_REQUIRE(p && g && momentum_buf && dev_state && guard && n > 0,
                 "hupr_sgd_step_guard_f32: bad argument (null pointer or n <= 0)");
    HUPR_LAUNCH(hupr_k_sgd_guard, grid_for(n, kMaxBlocks, 4 * kThreads), dim3(256), 0, as_stream(stream), p, g, momentum_buf, n,
                sgd_n4(p, g, momentum_buf, n), dev_state, guard, momentum, weight_decay, gscale);
    HUPR_LAUNCH_OK("hupr_k_sgd_guard");
    return HUPR_OK;
}

extern "C" int hupr_grad_sumsq_partials(void) { return kPartials; }

extern "C" int hupr_grad_sumsq_f32(const float* g, long n, double* partials, hupr_stream_t stream) {
    HUPR_REQUIRE(g && partials && n > 0, "hupr_grad_sumsq_f32: bad argument (null pointer or n <= 0)");
    HUPR_REQUIRE((reinterpret_cast<uintptr_t>(g) & 3) == 0 && (reinterpret_cast<uintptr_t>(partials) & 7) == 0,
                 "hupr_grad_sumsq_f32: g must be 4-byte and partials 8-byte aligned");
    const Span w = span_of(g, n, true);
    HUPR_LAUNCH(hupr_k_grad_sumsq, dim3(kPartials), dim3(kThreads), 0, as_stream(stream), g, n, w.head, w.n4, partials);
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
    const bool vec = congruent16(ema, p);
    const Span w = span_of(ema, n, vec);
    HUPR_LAUNCH(hupr_k_ema_update, grid_for(vec ? w.n4 / 4 : n, kMaxBlocks), dim3(kThreads), 0, as_stream(stream), ema, p, n, w.head,
                w.n4, ema_state);
    HUPR_LAUNCH_OK("hupr_k_ema_update");
    return HUPR_OK;
}

extern "C" int hupr_swap_f32(float* a, float* b, long n, hupr_stream_t stream) {
    HUPR_REQUIRE(a && b && n > 0, "hupr_swap_f32: bad argument (null pointer or n <= 0)");
    HUPR_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) == 0,
                 "hupr_swap_f32: a and b must be 4-byte aligned");
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)n * 4;
    HUPR_REQUIRE(ua + bytes <= ub || ub + bytes <= ua, "hupr_swap_f32: the two ranges overlap");
    const bool vec = congruent16(a, b);
    const Span w = span_of(a, n, vec);
    HUPR_LAUNCH(hupr_k_swap, grid_for(vec ? w.n4 / 2 : n, kMaxBlocks), dim3(kThreads), 0, as_stream(stream), a, b, n, w.head, w.n4);
    HUPR_LAUNCH_OK("hupr_k_swap");
    return HUPR_OK;
}

// ---- LAMB ----
// The chunk table, int64 words (tools/optim.py lamb_chunk_table builds it, lamb_table_ok below checks the host copy in front of
// every launch, the kernels read the device copy):
//   [0] segments S   [1] chunks K   [2] chunk size   [3] n
//   S x {start, length, first chunk, chunk count, adapted}     segments tile [0, n) in order
//   K x {segment, start relative to the segment}                chunks of a segment are consecutive, relative starts 0, C, 2C, ...
namespace {
constexpr int kLambHead = 4, kLambSegWords = 5, kLambChunkWords = 2;

const char* lamb_table_error(const long* t, long words, long n) {
    if (words < kLambHead) return "shorter than its header";
    const long S = t[0], K = t[1];
    if (t[2] != kLambChunk) return "built for another chunk size than hupr_lamb_chunk()";
    if (t[3] != n) return "built for another n";
    if (S <= 0 || K <= 0 || S > n || K > n || K > 0x7fffffffL) return "segment or chunk count out of range";
    if (words != kLambHead + kLambSegWords * S + kLambChunkWords * K) return "length does not match its segment and chunk counts";
    const long* seg = t + kLambHead;
    const long* chunk = seg + kLambSegWords * S;
    long at = 0, first = 0;
    for (long s = 0; s < S; ++s, seg += kLambSegWords) {
        if (seg[0] < at) return "segments overlap";
        if (seg[0] > at) return "segments leave a gap";
        if (seg[1] <= 0 || seg[1] > n - at) return "a segment is empty or runs past n";
        const long count = (seg[1] + kLambChunk - 1) / kLambChunk;
        if (seg[2] != first || seg[3] != count || first + count > K) return "a segment's chunk range is not ceil(length / chunk) from the last one's end";
        if (seg[4] != 0 && seg[4] != 1) return "an adapted flag is neither 0 nor 1";
        for (long k = 0; k < count; ++k)
            if (chunk[kLambChunkWords * (first + k)] != s || chunk[kLambChunkWords * (first + k) + 1] != k * kLambChunk)
                return "a chunk does not sit at its place in its segment";
        at += seg[1];
        first += count;
    }
    if (at != n) return "segments do not reach n";
    if (first != K) return "chunks left over behind the last segment";
    return nullptr;
}

// The bias corrections of step `step` in the form of adam_bias_corrections.  The betas stay fp64 up to here and 1 - beta is rounded
// to fp32 once: 1.f - 0.999f is 1.3e-5 away from 0.001, which a norm ratio over a whole tensor does not average out
__device__ __forceinline__ void lamb_bias_corrections(double b1, double b2, float step_f, float& bc1, float& bc2_sqrt) {
    const double step = (double)step_f;
    bc1 = (float)(1.0 - pow(b1, step));
    bc2_sqrt = (float)sqrt(1.0 - pow(b2, step));
}

// Adam's direction plus the decoupled decay of an adapted tensor.  THE function of both stages: stage 2 sees stage 1's bits
__device__ __forceinline__ float lamb_u(float p, float m, float v, float bc1, float bc2_sqrt, float eps, float wd, bool adapted) {
#pragma clang fp contract(off)
    const float d = (m / bc1) / (sqrtf(v) / bc2_sqrt + eps);
    return adapted ? fmaf(wd, p, d) : d;
}

// new moments (Adam's, without its coupled decay) and u for one element; the squares go to the thread's fp64 sums
__device__ __forceinline__ void lamb_elem1(float p, float g, float& m, float& v, float gs, float b1, float b2, float omb1,
                                           float omb2, float bc1, float bc2_sqrt, float eps, float wd, bool adapted, double& sp,
                                           double& su) {
#pragma clang fp contract(off)
    const float gr = g * gs;
    m = fmaf(b1, m, omb1 * gr);
    v = fmaf(b2, v, omb2 * gr * gr);
    const float u = lamb_u(p, m, v, bc1, bc2_sqrt, eps, wd, adapted);
    sp = fma((double)p, (double)p, sp);
    su = fma((double)u, (double)u, su);
}

struct LambChunk { long base; int len; int seg; bool adapted; };
__device__ __forceinline__ LambChunk lamb_chunk_of(const long* __restrict__ table) {
    const long* seg = table + kLambHead;
    const long* chunk = seg + kLambSegWords * table[0] + kLambChunkWords * (long)blockIdx.x;
    seg += kLambSegWords * chunk[0];
    const long left = seg[1] - chunk[1];
    return {seg[0] + chunk[1], (int)(left < kLambChunk ? left : kLambChunk), (int)chunk[0], seg[4] != 0};
}

__device__ __forceinline__ bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
}  // namespace

__global__ __launch_bounds__(kThreads) void hupr_k_lamb_stage1(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, const long* __restrict__ table,
                                                               const float* __restrict__ state, const float* __restrict__ guard,
                                                               double beta1, double beta2, float eps, float wd, float gscale,
                                                               double* __restrict__ partials) {
    if (guard && guard[3] == 0.f) return;
    const float gs = guard ? gscale * guard[0] : gscale;
    const float b1 = (float)beta1, b2 = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
    float bc1, bc2_sqrt;
    lamb_bias_corrections(beta1, beta2, state[1], bc1, bc2_sqrt);
    const LambChunk c = lamb_chunk_of(table);
    p += c.base, g += c.base, m += c.base, v += c.base;
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
    double sp = 0.0, su = 0.0;
#pragma unroll
    for (int e = 4 * threadIdx.x; e < kLambChunk; e += 4 * kThreads) {
        if (vec && e + 4 <= c.len) {
            const float4 pv = *reinterpret_cast<const float4*>(p + e), gv = *reinterpret_cast<const float4*>(g + e);
            float4 mv = *reinterpret_cast<const float4*>(m + e), vv = *reinterpret_cast<const float4*>(v + e);
            lamb_elem1(pv.x, gv.x, mv.x, vv.x, gs, b1, b2, omb1, omb2, bc1, bc2_sqrt, eps, wd, c.adapted, sp, su);
            lamb_elem1(pv.y, gv.y, mv.y, vv.y, gs, b1, b2, omb1, omb2, bc1, bc2_sqrt, eps, wd, c.adapted, sp, su);
            lamb_elem1(pv.z, gv.z, mv.z, vv.z, gs, b1, b2, omb1, omb2, bc1, bc2_sqrt, eps, wd, c.adapted, sp, su);
            lamb_elem1(pv.w, gv.w, mv.w, vv.w, gs, b1, b2, omb1, omb2, bc1, bc2_sqrt, eps, wd, c.adapted, sp, su);
            *reinterpret_cast<float4*>(m + e) = mv;
            *reinterpret_cast<float4*>(v + e) = vv;
        } else {
            for (int k = e; k < e + 4 && k < c.len; ++k) {
                float mv = m[k], vv = v[k];
                lamb_elem1(p[k], g[k], mv, vv, gs, b1, b2, omb1, omb2, bc1, bc2_sqrt, eps, wd, c.adapted, sp, su);
                m[k] = mv;
                v[k] = vv;
            }
        }
    }
    const double tp = block_sum_f64(sp);
    __syncthreads();                                        // block_sum_f64's staging is reused
    const double tu = block_sum_f64(su);
    if (threadIdx.x == 0) {
        partials[2 * (long)blockIdx.x] = tp;
        partials[2 * (long)blockIdx.x + 1] = tu;
    }
}

// One workgroup per segment; thread t adds the pairs of the segment's chunks t, t + 256, ... in order.  stats = |p|, |u|, r, S each
__global__ __launch_bounds__(kThreads) void hupr_k_lamb_ratio(const double* __restrict__ partials, const long* __restrict__ table,
                                                              const float* __restrict__ guard, float* __restrict__ stats) {
    if (guard && guard[3] == 0.f) return;
    const long S = table[0];
    const long* seg = table + kLambHead + kLambSegWords * (long)blockIdx.x;
    const long first = seg[2], count = seg[3];
    double sp = 0.0, su = 0.0;
    for (long k = threadIdx.x; k < count; k += kThreads) {
        sp += partials[2 * (first + k)];
        su += partials[2 * (first + k) + 1];
    }
    const double tp = block_sum_f64(sp);
    __syncthreads();
    const double tu = block_sum_f64(su);
    if (threadIdx.x != 0) return;
    const double pn = sqrt(tp), un = sqrt(tu);
    stats[blockIdx.x] = (float)pn;
    stats[S + blockIdx.x] = (float)un;
    stats[2 * S + blockIdx.x] = seg[4] != 0 && pn > 0.0 && un > 0.0 ? (float)(pn / un) : 1.f;
}

__global__ __launch_bounds__(kThreads) void hupr_k_lamb_stage2(float* __restrict__ p, const float* __restrict__ m,
                                                               const float* __restrict__ v, const long* __restrict__ table,
                                                               const float* __restrict__ state, const float* __restrict__ guard,
                                                               double beta1, double beta2, float eps, float wd,
                                                               const float* __restrict__ stats) {
    if (guard && guard[3] == 0.f) return;
    float bc1, bc2_sqrt;
    lamb_bias_corrections(beta1, beta2, state[1], bc1, bc2_sqrt);
    const LambChunk c = lamb_chunk_of(table);
    const float step = state[0] * stats[2 * table[0] + c.seg];             // lr r: one fp32 product
    p += c.base, m += c.base, v += c.base;
    const bool vec = aligned16(p) && aligned16(m) && aligned16(v);
#pragma unroll
    for (int e = 4 * threadIdx.x; e < kLambChunk; e += 4 * kThreads) {
        if (vec && e + 4 <= c.len) {
            float4 pv = *reinterpret_cast<const float4*>(p + e);
            const float4 mv = *reinterpret_cast<const float4*>(m + e), vv = *reinterpret_cast<const float4*>(v + e);
            pv.x = fmaf(-step, lamb_u(pv.x, mv.x, vv.x, bc1, bc2_sqrt, eps, wd, c.adapted), pv.x);
            pv.y = fmaf(-step, lamb_u(pv.y, mv.y, vv.y, bc1, bc2_sqrt, eps, wd, c.adapted), pv.y);
            pv.z = fmaf(-step, lamb_u(pv.z, mv.z, vv.z, bc1, bc2_sqrt, eps, wd, c.adapted), pv.z);
            pv.w = fmaf(-step, lamb_u(pv.w, mv.w, vv.w, bc1, bc2_sqrt, eps, wd, c.adapted), pv.w);
            *reinterpret_cast<float4*>(p + e) = pv;
        } else {
            for (int k = e; k < e + 4 && k < c.len; ++k) p[k] = fmaf(-step, lamb_u(p[k], m[k], v[k], bc1, bc2_sqrt, eps, wd, c.adapted), p[k]);
        }
    }
}

extern "C" int hupr_lamb_chunk(void) { return kLambChunk; }

// host only, no launch: 0 when table_host[0 .. words) is a chunk table over [0, n) as documented above
extern "C" int hupr_lamb_table_check(const long* table_host, long words, long n) {
    HUPR_REQUIRE(table_host && n > 0, "hupr_lamb_table_check: bad argument (null table or n <= 0)");
    const char* why = lamb_table_error(table_host, words, n);
    HUPR_REQUIRE(!why, "hupr_lamb_table_check: bad chunk table: %s", why);
    return HUPR_OK;
}

#define HUPR_LAMB_TABLE(name)                                                                       \
    do {                                                                                            \
        const char* why__ = lamb_table_error(table_host, words, n);                                 \
        HUPR_REQUIRE(!why__, name ": bad chunk table: %s", why__);                                  \
    } while (0)

// table_host / table_dev: the same chunk table in host and in device memory (words int64 each); partials: 2 doubles per chunk
extern "C" int hupr_lamb_stage1_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, const long* table_host,
                                    long words, const long* table_dev, const float* dev_state, const float* guard, double beta1,
                                    double beta2, float eps, float weight_decay, float gscale, double* partials,
                                    hupr_stream_t stream) {
    HUPR_REQUIRE(p && g && exp_avg && exp_avg_sq && table_host && table_dev && dev_state && partials && n > 0,
                 "hupr_lamb_stage1_f32: bad argument (null pointer or n <= 0)");
    HUPR_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "hupr_lamb_stage1_f32: partials must be 8-byte aligned");
    HUPR_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "hupr_lamb_stage1_f32: betas must be inside [0, 1)");
    HUPR_LAMB_TABLE("hupr_lamb_stage1_f32");
    HUPR_LAUNCH(hupr_k_lamb_stage1, dim3((unsigned)table_host[1]), dim3(kThreads), 0, as_stream(stream), p, g, exp_avg, exp_avg_sq,
                table_dev, dev_state, guard, beta1, beta2, eps, weight_decay, gscale, partials);
    HUPR_LAUNCH_OK("hupr_k_lamb_stage1");
    return HUPR_OK;
}

// seg_stats: 3 floats per segment, |p| of every segment, then |u|, then r
extern "C" int hupr_lamb_ratio_f32(const double* partials, long n, const long* table_host, long words, const long* table_dev,
                                   const float* guard, float* seg_stats, hupr_stream_t stream) {
    HUPR_REQUIRE(partials && table_host && table_dev && seg_stats && n > 0, "hupr_lamb_ratio_f32: bad argument (null pointer or n <= 0)");
    HUPR_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "hupr_lamb_ratio_f32: partials must be 8-byte aligned");
    HUPR_LAMB_TABLE("hupr_lamb_ratio_f32");
    HUPR_LAUNCH(hupr_k_lamb_ratio, dim3((unsigned)table_host[0]), dim3(kThreads), 0, as_stream(stream), partials, table_dev, guard,
                seg_stats);
    HUPR_LAUNCH_OK("hupr_k_lamb_ratio");
    return HUPR_OK;
}

extern "C" int hupr_lamb_stage2_f32(float* p, const float* exp_avg, const float* exp_avg_sq, long n, const long* table_host,
                                    long words, const long* table_dev, const float* dev_state, const float* guard, double beta1,
                                    double beta2, float eps, float weight_decay, const float* seg_stats, hupr_stream_t stream) {
    HUPR_REQUIRE(p && exp_avg && exp_avg_sq && table_host && table_dev && dev_state && seg_stats && n > 0,
                 "hupr_lamb_stage2_f32: bad argument (null pointer or n <= 0)");
    HUPR_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "hupr_lamb_stage2_f32: betas must be inside [0, 1)");
    HUPR_LAMB_TABLE("hupr_lamb_stage2_f32");
    HUPR_LAUNCH(hupr_k_lamb_stage2, dim3((unsigned)table_host[1]), dim3(kThreads), 0, as_stream(stream), p, exp_avg, exp_avg_sq,
                table_dev, dev_state, guard, beta1, beta2, eps, weight_decay, seg_stats);
    HUPR_LAUNCH_OK("hupr_k_lamb_stage2");
    return HUPR_OK;
}
