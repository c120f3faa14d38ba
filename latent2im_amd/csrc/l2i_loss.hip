// l2i_loss.hip — [r6] the regressor head and its BCE term in ONE launch (gfx950).  Entry points l2i_reg_bce_f32 and l2i_reg_bce_keep_f32.
//
// Reference: transform_base.py:416-424 — `reg_preds = self.regressor(logit)` (torchvision ResNet-50: avg-pooled features -> fc), the attribute columns selected,
// `get_bce_loss(pred, y)` = -mean(y log(max(pred, eps)) + (1 - y) log(max(1 - pred, eps))) with y in float64 — and what autograd runs backwards through those
// ops.  As torch ops that is ~40 launches of a few microseconds each between the regressor's last conv and its first gradient conv, with nothing else on the
// stream (profiles/r06_timeline.txt: 0.2 - 0.3 ms without a large kernel running).  Here: block b finishes sample b — the K selected logits (2048-long dots
// with the fc rows, fp32), the predictions, d loss / d pred for an upstream gradient of 1 (fp32, the dtype autograd hands to the fp32 log nodes), and
// d loss / d feat = sum_k gpred[k] * fc_w[col_k][:]; block 0 also forms the loss itself over all samples in a fixed order (float64 sum of fp32 logs, like
// the torch expression): deterministic, no atomics.  The caller multiplies the stored gradient by the real upstream gradient (one launch).
//
// l2i_reg_bce_keep_f32 adds the attribute-preservation term w_keep * mean_bj |fc(feat1)[b, keep_j] - fc(feat0)[b, keep_j]| to the same launch: block b
// also forms the M kept outputs of both feature rows of sample b (keep_row: four columns x two rows a pass, every dot product summed in head_logit's
// order — thread t adds the features t, t + 256, .. ascending, the wave butterfly, (w0 + w1) + (w2 + w3), the bias — so bitwise equal rows give bitwise
// equal outputs and the difference is exactly 0), the sign of each difference, and adds sum_j w_keep sign_j / (B M) fc_w[keep_j][:] to the BCE part's
// d loss / d feat (one stored buffer, one upstream gradient, as before).  The loss reduction: block 0 recomputes the kept outputs of every sample with the
// same routine and adds |d| in float64, b ascending then j ascending — no ticket, no workspace, no float atomics; two launches give equal bits.  The BCE
// part is the arithmetic of l2i_reg_bce_f32 through the same device functions.
// Cost of that choice, by count (the launch has not been timed): block 0 runs B ceil(M / 4) passes of keep_row (eight dot products and three barriers a
// pass) where every other block runs ceil(M / 4) — 80 against 10 at B = 8, M = 39 — so the launch lasts as long as block 0.  tools/bench_attr_keep.py
// times it beside l2i_reg_bce_f32.  Per-sample float64 partials summed by the last block through an integer ticket would take the B-fold recompute
// off block 0 at the price of a zeroed counter that outlives the launch; that form is not built.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"

namespace {
__device__ __forceinline__ double bce_target(const void* target, int target_f64, size_t i) {
    return target_f64 ? reinterpret_cast<const double*>(target)[i] : (double)reinterpret_cast<const float*>(target)[i];
}
// one fc output: thread t adds x[i] w[i] over i = t, t + 256, .. ascending, block_sum, the bias
__device__ __forceinline__ float head_logit(const float* x, const float* w, float bias, int F, int tid, float* red) {
    float s = 0.f;
    for (int i = tid; i < F; i += 256) s += x[i] * w[i];
    return block_sum(s, red) + bias;
}
// d loss / d pred of one BCE entry for an upstream gradient of 1
__device__ __forceinline__ float bce_gpred(float p, double y, double inv_n, float eps) {
    const float a = (float)(-y * inv_n), c = (float)(-(1.0 - y) * inv_n);                          // d loss / d log(.) of the two terms, upstream gradient 1
    const float q = 1.f - p;
    float g = 0.f;
    if (p >= eps) g += a / fmaxf(p, eps);                                                           // clamp(min = eps) passes the gradient where p >= eps
    if (q >= eps) g -= c / fmaxf(q, eps);                                                           // d (1 - p) / d p = -1
    return g;
}
__device__ __forceinline__ double bce_logterm(float p, double y, float eps) {
    const float q = 1.f - p;
    // clamp(min = eps) as a select: torch.clamp keeps a NaN prediction and the loss is NaN; fmaxf would return eps for it
    return y * (double)logf(p < eps ? eps : p) + (1.0 - y) * (double)logf(q < eps ? eps : q);
}

__global__ __launch_bounds__(256) void reg_bce_kernel(double* loss, float* preds, float* g_feat, const float* feat, const float* fc_w, const float* fc_b,
                                                      const int64_t* cols, const void* target, int target_f64, int B, int F, int K, float eps) {
    __shared__ float red[4];
    __shared__ float gp_s[64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double inv_n = 1.0 / ((double)B * (double)K);
    for (int k = 0; k < K; ++k) {
        const float p = head_logit(feat + (size_t)b * F, fc_w + (size_t)cols[k] * F, fc_b[cols[k]], F, tid, red);
        if (tid == 0) {
            preds[(size_t)b * K + k] = p;
            gp_s[k] = bce_gpred(p, bce_target(target, target_f64, (size_t)b * K + k), inv_n, eps);
        }
    }
    __syncthreads();
    for (int i = tid; i < F; i += 256) {
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += gp_s[k] * fc_w[(size_t)cols[k] * F + i];
        g_feat[(size_t)b * F + i] = s;
    }
    if (b == 0) {                                           // the loss: every sample again, fixed order
        double acc = 0.0;
        for (int bb = 0; bb < B; ++bb)
            for (int k = 0; k < K; ++k) {
                const float p = head_logit(feat + (size_t)bb * F, fc_w + (size_t)cols[k] * F, fc_b[cols[k]], F, tid, red);
                if (tid == 0) acc += bce_logterm(p, bce_target(target, target_f64, (size_t)bb * K + k), eps);
            }
        if (tid == 0) loss[0] = -acc * inv_n;
    }
}

// The M kept fc outputs of the feature rows x1 and x0 into p1_s / p0_s: four columns a pass, each of the eight dot products in head_logit's order
// (one chain per thread over i = t, t + 256, .., the wave butterfly, (w0 + w1) + (w2 + w3), the bias).  Ends on a barrier: every thread may read them.
__device__ __forceinline__ void keep_row(float* p1_s, float* p0_s, float (*red8)[8], const float* x1, const float* x0, const float* fc_w, const float* fc_b,
                                         const int64_t* keep_cols, int F, int M, int tid) {
    for (int j0 = 0; j0 < M; j0 += 4) {
        const float* w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = fc_w + (size_t)keep_cols[min(j0 + c, M - 1)] * F;          // a pass past M repeats the last column; its result is dropped
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < F; i += 256) {
            const float a1 = x1[i], a0 = x0[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float wv = w[c][i];
                s[2 * c] += a1 * wv;
                s[2 * c + 1] += a0 * wv;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = wave_sum_all(s[e]);
        __syncthreads();
        if ((tid & 63) == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red8[tid >> 6][e] = s[e];
        }
        __syncthreads();
        if (tid < 8 && j0 + (tid >> 1) < M) {
            const int j = j0 + (tid >> 1);
            const float v = ((red8[0][tid] + red8[1][tid]) + (red8[2][tid] + red8[3][tid])) + fc_b[keep_cols[j]];
            if (tid & 1) p0_s[j] = v; else p1_s[j] = v;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void reg_bce_keep_kernel(double* loss, float* preds, float* pkeep, float* g_feat, const float* feat1, const float* feat0,
                                                           const float* fc_w, const float* fc_b, const int64_t* cols, const void* target, int target_f64,
                                                           const int64_t* keep_cols, int B, int F, int K, int M, float c_reg, float w_keep, float eps) {
    __shared__ float red[4];
    __shared__ float red8[4][8];
    __shared__ float gp_s[64], gk_s[64], p1_s[64], p0_s[64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double inv_n = K > 0 ? 1.0 / ((double)B * (double)K) : 0.0, inv_m = 1.0 / ((double)B * (double)M);
    const float inv_mf = (float)inv_m;
    // the BCE part on the edited image's features: l2i_reg_bce_f32's arithmetic, the gradient weighted by c_reg
    for (int k = 0; k < K; ++k) {
        const float p = head_logit(feat1 + (size_t)b * F, fc_w + (size_t)cols[k] * F, fc_b[cols[k]], F, tid, red);
        if (tid == 0) {
            preds[(size_t)b * K + k] = p;
            gp_s[k] = c_reg * bce_gpred(p, bce_target(target, target_f64, (size_t)b * K + k), inv_n, eps);
        }
    }
    // the kept outputs: block b its own sample; block 0 every sample, for the loss (fixed order: b ascending, j ascending)
    double acc = 0.0;
    const int lo = b == 0 ? 0 : b, hi = b == 0 ? B : b + 1;
    for (int bb = lo; bb < hi; ++bb) {
        keep_row(p1_s, p0_s, red8, feat1 + (size_t)bb * F, feat0 + (size_t)bb * F, fc_w, fc_b, keep_cols, F, M, tid);
        if (bb == b && tid < M) {
            const float p1 = p1_s[tid], p0 = p0_s[tid], d = p1 - p0;
            pkeep[((size_t)b * M + tid) * 2] = p1;
            pkeep[((size_t)b * M + tid) * 2 + 1] = p0;
            gk_s[tid] = w_keep * (d > 0.f ? inv_mf : (d < 0.f ? -inv_mf : 0.f));                    // torch.abs's subgradient; a NaN d: both comparisons false
        }
        if (b == 0 && tid == 0)
            for (int j = 0; j < M; ++j) acc += (double)fabsf(p1_s[j] - p0_s[j]);
    }
    __syncthreads();
    for (int i = tid; i < F; i += 256) {
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += gp_s[k] * fc_w[(size_t)cols[k] * F + i];
        for (int j = 0; j < M; ++j) s += gk_s[j] * fc_w[(size_t)keep_cols[j] * F + i];
        g_feat[(size_t)b * F + i] = s;
    }
    if (b == 0) {
        double bce = 0.0;
        for (int bb = 0; bb < B; ++bb)
            for (int k = 0; k < K; ++k) {
                const float p = head_logit(feat1 + (size_t)bb * F, fc_w + (size_t)cols[k] * F, fc_b[cols[k]], F, tid, red);
                if (tid == 0) bce += bce_logterm(p, bce_target(target, target_f64, (size_t)bb * K + k), eps);
            }
        if (tid == 0) {
            const double reg = K > 0 ? -bce * inv_n : 0.0, keep = acc * inv_m;
            loss[0] = reg;
            loss[1] = keep;
            loss[2] = K > 0 ? (double)c_reg * reg + (double)w_keep * keep : (double)w_keep * keep;
        }
    }
}
}  // namespace

extern "C" int l2i_reg_bce_f32(double* loss, float* preds, float* g_feat, const float* feat, const float* fc_w, const float* fc_b, const int64_t* cols,
                               const void* target, int target_f64, int B, int F, int K, float eps, void* stream) {
    if (!loss || !preds || !g_feat || !feat || !fc_w || !fc_b || !cols || !target) return l2i_set_error(L2I_E_ARG, "reg_bce: null tensor");
    if (B <= 0 || F <= 0 || K <= 0 || K > 64) return l2i_set_error(L2I_E_ARG, "reg_bce: 1 <= K <= 64 selected attributes");
    hipLaunchKernelGGL(reg_bce_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, loss, preds, g_feat, feat, fc_w, fc_b, cols, target, target_f64, B, F, K, eps);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_reg_bce_keep_f32(double* loss, float* preds, float* pkeep, float* g_feat, const float* feat1, const float* feat0, const float* fc_w,
                                    const float* fc_b, const int64_t* cols, const void* target, int target_f64, const int64_t* keep_cols, int B, int F, int K,
                                    int M, float c_reg, float w_keep, float eps, void* stream) {
    if (!loss || !pkeep || !g_feat || !feat1 || !feat0 || !fc_w || !fc_b || !keep_cols) return l2i_set_error(L2I_E_ARG, "reg_bce_keep: null tensor");
    if (B <= 0 || F <= 0 || M < 1 || M > 64 || K < 0 || K > 64)
        return l2i_set_error(L2I_E_ARG, "reg_bce_keep: 0 <= K <= 64 trained and 1 <= M <= 64 kept attributes");
    if (K > 0 && (!preds || !cols || !target)) return l2i_set_error(L2I_E_ARG, "reg_bce_keep: K > 0 needs preds, cols and target");
    hipLaunchKernelGGL(reg_bce_keep_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, loss, preds, pkeep, g_feat, feat1, feat0, fc_w, fc_b, cols, target,
                       target_f64, keep_cols, B, F, K, M, c_reg, w_keep, eps);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
