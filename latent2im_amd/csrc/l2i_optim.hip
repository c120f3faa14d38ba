// l2i_optim.hip — the optimiser tail of the walk-training step on the fp16 path: finite check, guarded Adam, dynamic loss scale.
//
// The reference's step ends in `self.optimizers.step()` (transform_base.py:487-488: torch.optim.Adam, betas (0.5, 0.99)) on ONE tiny tensor,
// the walk [n_attr, n_latent, 512] (9 - 46 K floats).  Under autocast the reference would wrap that step in a torch GradScaler: skip the update
// when the scaled gradients hold an inf / NaN, halve the scale, grow it again after `interval` clean steps.  The fp16 path here (nets16.py) scales
// each loss branch by a static power of two times ONE dynamic factor that lives on the device; this file is the part of the GradScaler that must
// not cost a host synchronisation (torch's own reads `found_inf` back with .item() before every optimiser step):
//
//   l2i_nonfinite_flag_f32   state[FOUND] |= any(!isfinite(g))                    (multi-tensor walks: one call per gradient tensor first)
//   l2i_adam_guarded_f32     if !found: Adam update of (p, m, v, step) exactly as torch's single-tensor Adam computes it; found: nothing moves.
//                            `last`: then the scale state advances the way torch._amp_update_scale_ does and the flag is cleared.
//   l2i_sgd_guarded_f32      the same guard around torch.optim.SGD(lr, momentum)'s update of (p, buf, step): BP.py:140's optimiser for the inversion
//                            loop, whose "first step" (buf = g) is read from the device counter so that a captured graph replays it.
//
//   l2i_nonfinite_flag_multi_f32 / l2i_adam_guarded_multi_f32   the first two over a TABLE of up to L2I_ADAM_MAX_TENSORS tensors, many blocks.
//
// The single-tensor entries run one 1024-thread block per call: the tensors are tens of KB, and a single block can order "every lane has read the
// flag / the step counter" before "lane 0 rewrites them" with a barrier instead of a second launch.  The linear walk's whole tail is ONE launch
// (check_self = last = 1) where torch's foreach Adam issues ~12.  The MLP walk of the PGGAN graph has 2.1 M parameters in six tensors: there the
// table entries flag every gradient in one launch, update every tensor in a second (MB elements a block, nothing in it writes the flag or a step
// counter) and leave the counters and the scale state to a one-wave tail launch; the stream orders the three.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"

namespace {
constexpr int NT = 1024;

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ int block_any(int pred, int* sh) {
    // wave-wide OR by ballot, block-wide through one LDS word per wave
    const unsigned long long b = __ballot(pred);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = b != 0ull;
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) any |= sh[w];
    __syncthreads();
    return any;
}

// The guard's prologue, shared by both optimisers: the flag an earlier tensor of this step left, or (check_self) an inf / NaN in g itself.
// Every lane returns the same value; the caller's barrier orders these reads before lane 0's rewrite of the flag.
__device__ __forceinline__ int guard_found(const float* __restrict__ g, long n, int check_self, const int32_t* __restrict__ state, int* sh) {
    int found = state[L2I_LS_FOUND];
    if (check_self) {
        int bad = 0;
        for (long i = threadIdx.x; i < n; i += NT) bad |= nonfinite(g[i]);
        found |= block_any(bad, sh);
    }
    return found;
}

// The guard's tail, run by lane 0 alone after the update: the flag for the next tensor, and with `last` the scale state of the whole step.
__device__ __forceinline__ void scale_tail(int found, int check_self, int32_t* __restrict__ state, float* __restrict__ scale, float growth,
                                           float backoff, int interval, float max_scale, int last) {
    if (check_self && found) state[L2I_LS_FOUND] = 1;             // visible to the next tensor of a multi-tensor step
    if (last) {
        // torch._amp_update_scale_: found -> scale *= backoff, tracker = 0; clean -> ++tracker == interval -> scale *= growth (kept finite), tracker = 0
        if (found) {
            state[L2I_LS_TRACKER] = 0;
            state[L2I_LS_SKIPPED] += 1;
            if (scale) scale[0] *= backoff;
        } else {
            const int tr = state[L2I_LS_TRACKER] + 1;
            if (tr >= interval && interval > 0) {
                state[L2I_LS_TRACKER] = 0;
                if (scale) { const float s2 = scale[0] * growth; if (s2 <= max_scale) scale[0] = s2; }
            } else {
                state[L2I_LS_TRACKER] = tr;
            }
        }
        if (scale) scale[1] = 1.f / scale[0];
        state[L2I_LS_STEPS] += 1;
        state[L2I_LS_FOUND] = 0;
    }
}

// torch's _single_tensor_adam, stated once for the single-block and the multi-block kernel.  The prologue: bias corrections in double like the
// python floats of torch; one lane per block runs it.
__device__ __forceinline__ void adam_bias(float lr, float beta1, float beta2, float t, float* size, float* bc2s) {
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    *size = (float)((double)lr / bc1);
    *bc2s = (float)sqrt(bc2);
}

struct adam_coef { float size, bc2s, omb1, omb2, beta2, eps; };

// One element.  Every rounding is spelled out, so that no call site is free to contract it another way: the sequence is the one the single-block
// kernel has always compiled to (two fused multiply-adds for the moments, one for the parameter; IEEE sqrt and divisions).
__device__ __forceinline__ void adam_element(const adam_coef& c, float gi, float& p, float& m, float& v) {
    v = __fmaf_rn(gi, __fmul_rn(c.omb2, gi), __fmul_rn(c.beta2, v));    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    m = __fmaf_rn(c.omb1, __fsub_rn(gi, m), m);                         // exp_avg.lerp_(grad, 1 - beta1)
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), c.bc2s), c.eps);
    p = __fmaf_rn(-c.size, __fdiv_rn(m, denom), p);                     // param.addcdiv_(exp_avg, denom, value=-step_size)
}
}  // namespace

__global__ __launch_bounds__(NT) void nonfinite_flag_kernel(const float* __restrict__ g, long n, int32_t* __restrict__ state) {
    __shared__ int sh[NT / 64];
    int bad = 0;
    for (long i = threadIdx.x; i < n; i += NT) bad |= nonfinite(g[i]);
    bad = block_any(bad, sh);
    if (bad && threadIdx.x == 0) state[L2I_LS_FOUND] = 1;
}

__global__ __launch_bounds__(NT) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ step, long n, float lr, float beta1, float beta2,
                                                          float eps, int check_self, int32_t* __restrict__ state, float* __restrict__ scale,
                                                          float growth, float backoff, int interval, float max_scale, int last) {
    __shared__ int sh[NT / 64];
    __shared__ float s_size, s_bc2;
    const int found = guard_found(g, n, check_self, state, sh);
    const float t = step[0] + 1.f;
    if (threadIdx.x == 0) adam_bias(lr, beta1, beta2, t, &s_size, &s_bc2);
    __syncthreads();                                             // every lane holds `found` and `t`: the words may be rewritten below
    if (!found) {
        const adam_coef c = {s_size, s_bc2, 1.f - beta1, 1.f - beta2, beta2, eps};
        for (long i = threadIdx.x; i < n; i += NT) {
            float pi = p[i], mi = m[i], vi = v[i];
            adam_element(c, g[i], pi, mi, vi);
            m[i] = mi;
            v[i] = vi;
            p[i] = pi;
        }
        if (threadIdx.x == 0) step[0] = t;
    }
    if (threadIdx.x == 0) scale_tail(found, check_self, state, scale, growth, backoff, interval, max_scale, last);
}

namespace {
constexpr int MT = 256;                 // threads of a multi-tensor block
constexpr int MB = 4096;                // elements of one tensor a block covers: four 16-byte accesses a lane and operand

struct adam_table { l2i_adam_tensor t[L2I_ADAM_MAX_TENSORS]; int count; };

__host__ __device__ __forceinline__ long table_blocks(long n) { return (n + MB - 1) / MB; }

// Which tensor this block works on and where in it: the table is scanned in order, every tensor owning ceil(n / MB) consecutive blocks.
// Uniform over the block (blockIdx only).  false: a block past the last tensor (never launched; kept as the bound).
__device__ __forceinline__ bool table_find(const adam_table& tab, int* k, long* begin, long* len) {
    long b = blockIdx.x;
    for (int i = 0; i < tab.count; ++i) {
        const long nb = table_blocks(tab.t[i].n);
        if (b < nb) {
            *k = i;
            *begin = b * MB;
            *len = tab.t[i].n - *begin < MB ? tab.t[i].n - *begin : MB;
            return true;
        }
        b -= nb;
    }
    return false;
}

// Elements before the first 16-byte boundary of a float pointer (0..3).
__device__ __forceinline__ int head_of(const float* q) { return (int)((16u - ((uintptr_t)q & 15u)) & 15u) >> 2; }
}  // namespace

__global__ __launch_bounds__(MT) void nonfinite_flag_multi_kernel(const adam_table tab, int32_t* __restrict__ state) {
    int k;
    long begin, len;
    if (!table_find(tab, &k, &begin, &len)) return;
    const float* __restrict__ g = tab.t[k].g + begin;                 // begin is a multiple of 4 elements: g + begin is aligned as g is
    const int L = (int)len, h = head_of(g) < L ? head_of(g) : L, nv = (L - h) >> 2, tail = h + 4 * nv;
    int bad = 0;
    if ((int)threadIdx.x < h) bad |= nonfinite(g[threadIdx.x]);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + h);
    for (int i = threadIdx.x; i < nv; i += MT) {
        const float4 q = g4[i];
        bad |= (int)nonfinite(q.x) | (int)nonfinite(q.y) | (int)nonfinite(q.z) | (int)nonfinite(q.w);
    }
    if (tail + (int)threadIdx.x < L) bad |= nonfinite(g[tail + threadIdx.x]);
    if (bad) state[L2I_LS_FOUND] = 1;                                 // every writer writes the same word: no atomic, no reduction
}

__global__ __launch_bounds__(MT) void adam_guarded_multi_kernel(const adam_table tab, float lr, float beta1, float beta2, float eps,
                                                                const int32_t* __restrict__ state) {
    __shared__ float s_size, s_bc2;
    int k;
    long begin, len;
    if (!table_find(tab, &k, &begin, &len)) return;
    if (state[L2I_LS_FOUND]) return;                                  // uniform; neither the flag nor a step counter is written by this launch
    if (threadIdx.x == 0) adam_bias(lr, beta1, beta2, tab.t[k].step[0] + 1.f, &s_size, &s_bc2);
    __syncthreads();
    const adam_coef c = {s_size, s_bc2, 1.f - beta1, 1.f - beta2, beta2, eps};
    float* __restrict__ p = tab.t[k].p + begin;
    const float* __restrict__ g = tab.t[k].g + begin;
    float* __restrict__ m = tab.t[k].m + begin;
    float* __restrict__ v = tab.t[k].v + begin;
    const int L = (int)len;
    // 16-byte accesses when the four operands reach a 16-byte boundary after the same number of elements; element by element otherwise
    int h = head_of(p);
    if (head_of(g) != h || head_of(m) != h || head_of(v) != h || h > L) h = L;
    const int nv = (L - h) >> 2, tail = h + 4 * nv;
    for (int i = threadIdx.x; i < h; i += MT) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_element(c, g[i], pi, mi, vi);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p + h);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + h);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m + h);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v + h);
    for (int i = threadIdx.x; i < nv; i += MT) {
        float4 pq = p4[i], mq = m4[i], vq = v4[i];
        const float4 gq = g4[i];
        adam_element(c, gq.x, pq.x, mq.x, vq.x);
        adam_element(c, gq.y, pq.y, mq.y, vq.y);
        adam_element(c, gq.z, pq.z, mq.z, vq.z);
        adam_element(c, gq.w, pq.w, mq.w, vq.w);
        m4[i] = mq;
        v4[i] = vq;
        p4[i] = pq;
    }
    if (tail + (int)threadIdx.x < L) {                                // at most three elements
        const int i = tail + threadIdx.x;
        float pi = p[i], mi = m[i], vi = v[i];
        adam_element(c, g[i], pi, mi, vi);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
}

// One wave after the update launch: the step counters of the call's tensors, and with `last` the scale state of the whole step (scale_tail).
__global__ __launch_bounds__(64) void adam_multi_tail_kernel(const adam_table tab, int32_t* __restrict__ state, float* __restrict__ scale, float growth,
                                                             float backoff, int interval, float max_scale, int last) {
    const int found = state[L2I_LS_FOUND];
    __syncthreads();                                                  // every lane holds `found`: lane 0 may clear the word below
    if (!found && (int)threadIdx.x < tab.count) {
        float* step = tab.t[threadIdx.x].step;
        step[0] = step[0] + 1.f;
    }
    if (threadIdx.x == 0) scale_tail(found, 0, state, scale, growth, backoff, interval, max_scale, last);
}

// torch.optim.SGD(lr, momentum), dampening 0, no Nesterov, no weight decay (_single_tensor_sgd): first applied step buf = g, afterwards
// buf = momentum * buf + g; p = p - lr * buf.  Every product and sum is rounded on its own (no contraction): an exact float32 statement.
__global__ __launch_bounds__(NT) void sgd_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                         float* __restrict__ step, long n, float lr, float momentum, int check_self,
                                                         int32_t* __restrict__ state, float* __restrict__ scale, float growth, float backoff, int interval,
                                                         float max_scale, int last) {
    __shared__ int sh[NT / 64];
    const int found = guard_found(g, n, check_self, state, sh);
    const float t = step[0];
    __syncthreads();                                             // every lane holds `found` and `t`: the words may be rewritten below
    if (!found) {
#pragma clang fp contract(off)
        const bool first = t == 0.f;
        for (long i = threadIdx.x; i < n; i += NT) {
            const float gi = g[i];
            float bi = gi;
            if (!first) {
                const float mb = momentum * buf[i];
                bi = mb + gi;
            }
            buf[i] = bi;
            const float d = lr * bi;
            p[i] = p[i] - d;
        }
        if (threadIdx.x == 0) step[0] = t + 1.f;
    }
    if (threadIdx.x == 0) scale_tail(found, check_self, state, scale, growth, backoff, interval, max_scale, last);
}

extern "C" int l2i_nonfinite_flag_f32(const float* g, int64_t n, int32_t* state, void* stream) {
    if (!g || !state || n < 0) return l2i_set_error(L2I_E_ARG, "nonfinite_flag: null tensor");
    if (n == 0) return L2I_OK;
    hipLaunchKernelGGL(nonfinite_flag_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, g, (long)n, state);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_adam_guarded_f32(float* p, const float* g, float* m, float* v, float* step, int64_t n, float lr, float beta1, float beta2, float eps,
                                    int32_t check_self, int32_t* state, float* scale, float growth, float backoff, int32_t interval, float max_scale,
                                    int32_t last, void* stream) {
    if (!p || !g || !m || !v || !step || !state || n <= 0) return l2i_set_error(L2I_E_ARG, "adam_guarded: null tensor");
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) return l2i_set_error(L2I_E_ARG, "adam_guarded: betas in [0, 1), eps >= 0");
    if (scale && !(growth >= 1.f && backoff > 0.f && backoff <= 1.f)) return l2i_set_error(L2I_E_ARG, "adam_guarded: growth >= 1, 0 < backoff <= 1");
    hipLaunchKernelGGL(adam_guarded_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, step, (long)n, lr, beta1, beta2, eps, (int)check_self, state,
                       scale, growth, backoff, (int)interval, max_scale, (int)last);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

namespace {
// The table of a call, checked and copied into the kernel argument; blocks = the grid of the flag and the update launch.
int fill_table(const l2i_adam_tensor* tensors, int32_t count, bool update, adam_table* tab, long* blocks) {
    if (!tensors) return l2i_set_error(L2I_E_ARG, "adam table: null tensor table");
    if (count < 1 || count > L2I_ADAM_MAX_TENSORS) return l2i_set_error(L2I_E_ARG, "adam table: count outside 1..L2I_ADAM_MAX_TENSORS");
    *tab = adam_table{};
    tab->count = count;
    long total = 0;
    for (int i = 0; i < count; ++i) {
        const l2i_adam_tensor& t = tensors[i];
        if (!t.g || t.n <= 0 || (update && (!t.p || !t.m || !t.v || !t.step))) return l2i_set_error(L2I_E_ARG, "adam table: a tensor with a null pointer or n <= 0");
        tab->t[i] = t;
        total += table_blocks((long)t.n);
        if (total > 0x7fffffffL) return l2i_set_error(L2I_E_ARG, "adam table: more than 2^31 - 1 blocks");
    }
    *blocks = total;
    return L2I_OK;
}
}  // namespace

extern "C" int l2i_nonfinite_flag_multi_f32(const l2i_adam_tensor* tensors, int32_t count, int32_t* state, void* stream) {
    adam_table tab;
    long blocks;
    if (!state) return l2i_set_error(L2I_E_ARG, "nonfinite_flag_multi: null state");
    if (int rc = fill_table(tensors, count, false, &tab, &blocks)) return rc;
    hipLaunchKernelGGL(nonfinite_flag_multi_kernel, dim3((unsigned)blocks), dim3(MT), 0, (hipStream_t)stream, tab, state);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_adam_guarded_multi_f32(const l2i_adam_tensor* tensors, int32_t count, float lr, float beta1, float beta2, float eps, int32_t* state,
                                          float* scale, float growth, float backoff, int32_t interval, float max_scale, int32_t last, void* stream) {
    adam_table tab;
    long blocks;
    if (!state) return l2i_set_error(L2I_E_ARG, "adam_guarded_multi: null state");
    if (int rc = fill_table(tensors, count, true, &tab, &blocks)) return rc;
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) return l2i_set_error(L2I_E_ARG, "adam_guarded_multi: betas in [0, 1), eps >= 0");
    if (scale && !(growth >= 1.f && backoff > 0.f && backoff <= 1.f)) return l2i_set_error(L2I_E_ARG, "adam_guarded_multi: growth >= 1, 0 < backoff <= 1");
    hipLaunchKernelGGL(adam_guarded_multi_kernel, dim3((unsigned)blocks), dim3(MT), 0, (hipStream_t)stream, tab, lr, beta1, beta2, eps, (const int32_t*)state);
    L2I_CHECK_LAUNCH();
    hipLaunchKernelGGL(adam_multi_tail_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tab, state, scale, growth, backoff, (int)interval, max_scale, (int)last);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_sgd_guarded_f32(float* p, const float* g, float* buf, float* step, int64_t n, float lr, float momentum, int32_t check_self,
                                   int32_t* state, float* scale, float growth, float backoff, int32_t interval, float max_scale, int32_t last,
                                   void* stream) {
    if (!p || !g || !buf || !step || !state || n <= 0) return l2i_set_error(L2I_E_ARG, "sgd_guarded: null tensor");
    if (!(momentum >= 0.f && momentum < 1.f)) return l2i_set_error(L2I_E_ARG, "sgd_guarded: momentum in [0, 1)");
    if (!(lr >= 0.f && isfinite(lr))) return l2i_set_error(L2I_E_ARG, "sgd_guarded: lr finite and >= 0");
    if (scale && !(growth >= 1.f && backoff > 0.f && backoff <= 1.f)) return l2i_set_error(L2I_E_ARG, "sgd_guarded: growth >= 1, 0 < backoff <= 1");
    hipLaunchKernelGGL(sgd_guarded_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, p, g, buf, step, (long)n, lr, momentum, (int)check_self, state, scale,
                       growth, backoff, (int)interval, max_scale, (int)last);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
