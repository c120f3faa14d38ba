// l2i_walk.hip — the linear layers of the PGGAN graph's MLP walk (WalkMlpZ3, graphs/pggan/transform_base.py:167-188):
//     z_new = z + alpha * L3(lrelu(L2(lrelu(L1(z)))))        L1: 512 -> 1024, L2: 1024 -> 1024, L3: 1024 -> 512, LeakyReLU(0.2)
// forward in three launches (bias, activation and the walk's tail ride in the epilogue) and backward in one pass per layer over its [N, K] index
// space: the activation mask, the weight gradient, the bias gradient and the input gradient from one read of W.
//
// These are skinny products — B <= 16 rows against 0.5-1 M weights — whose roof is the bytes of W (8.4 MB fp32 for the three layers), and the fp32
// MFMA rate of gfx950 equals the vector rate, so every loaded weight feeds B plain v_fma_f32.  W stays in nn.Linear's own [out, in] layout (no
// repacked copy of a trainable weight): a weight ROW is contiguous in k, so the lanes of a wave lie along k (float4 each: one wave reads 1 KB of
// a row per load) where l2i_modulation.hip's segmv_kernel, whose matrices are [k][row], puts them along the rows.
//   forward   a wave owns two rows n and all k; the B x K input slice is staged in LDS in chunks of 512 k (each lane reads back its own float4:
//             sequential, conflict-free, shared by the two rows), B accumulators per row and lane, then one butterfly sum per (row, sample).
//   backward  a block is ONE wave that owns 256 k (one float4 per lane) and a slice of rows: its x[b, k] sit in registers for the whole slice,
//             g'[b, n] (masked / alpha-scaled once per block) is broadcast from LDS.  Per row: gW[n, k] = sum_b g' x is complete in the lane and
//             stored at once; gx[b, k] accumulates over the slice's rows and goes to a workspace, which a second small kernel adds in slice
//             order.  No floating-point atomics anywhere: every sum has a fixed order (b ascending, n ascending inside a slice, slices
//             ascending), equal inputs give equal bits.
// Rows are taken in chunks of at most 16 samples (template NB = 4 / 8 / 16 by the batch, a ragged last chunk zero-filled); a batch beyond 16 adds
// the later chunks into gW / gb in index order (each element is owned by one lane: read-modify-write without a race).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"

namespace {
constexpr int KC = 512;        // k per LDS stage of the forward kernel
constexpr int FR = 2;          // rows per wave of the forward kernel
constexpr int KT = 256;        // k per block of the backward kernel: one float4 per lane

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float fma4(float4 a, float4 b, float c) {
    return __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, __builtin_fmaf(a.x, b.x, c))));
}
}

// y[b, n] = epi(sum_k x[b, k] W[n, k] + bias[n]); grid N / 8, block 256 (wave v: rows 8 blockIdx + 2 v, + 1)
template <int NB>
__global__ __launch_bounds__(256) void linear_rows_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ res, const float* __restrict__ a,
                                                          int B, int K, int N, int epi, float slope) {
    __shared__ __attribute__((aligned(16))) float xs[NB][KC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n0 = (blockIdx.x * 4 + wv) * FR;
    for (int b0 = 0; b0 < B; b0 += NB) {
        const int nb = (B - b0) < NB ? (B - b0) : NB;
        float acc[FR][NB];
#pragma unroll
        for (int r = 0; r < FR; ++r)
#pragma unroll
            for (int q = 0; q < NB; ++q) acc[r][q] = 0.f;
        for (int kc = 0; kc < K; kc += KC) {
            const int kk = (K - kc) < KC ? (K - kc) : KC, k4n = kk >> 2;
            __syncthreads();                                    // the previous stage's reads of xs are done
            for (int i = tid; i < NB * k4n; i += 256) {
                const int q = i / k4n, k4 = i - q * k4n;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);    // rows past the batch: zeros, their sums are never stored
                if (q < nb) v = ld4(x + (long)(b0 + q) * K + kc + 4 * k4);
                *reinterpret_cast<float4*>(&xs[q][4 * k4]) = v;
            }
            __syncthreads();
            for (int k = lane * 4; k < kk; k += 256) {
                float4 wr[FR];
#pragma unroll
                for (int r = 0; r < FR; ++r) wr[r] = ld4(w + (long)(n0 + r) * K + kc + k);
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    const float4 xv = *reinterpret_cast<const float4*>(&xs[q][k]);
#pragma unroll
                    for (int r = 0; r < FR; ++r) acc[r][q] = fma4(xv, wr[r], acc[r][q]);
                }
            }
        }
        float mine[FR];
#pragma unroll
        for (int r = 0; r < FR; ++r) {
            mine[r] = 0.f;
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const float v = wave_sum_all(acc[r][q]);
                if (lane == q) mine[r] = v;
            }
        }
        if (lane < nb) {                                        // lane q finishes sample b0 + q of both rows
            const int b = b0 + lane;
#pragma unroll
            for (int r = 0; r < FR; ++r) {
                const int n = n0 + r;
                float v = mine[r] + bias[n];
                if (epi == L2I_LINEAR_LRELU) v = v > 0.f ? v : v * slope;
                else if (epi == L2I_LINEAR_WALK) v = res[(long)b * N + n] + a[b] * v;
                y[(long)b * N + n] = v;
            }
        }
    }
}

// One pass over rows [rows * blockIdx.y, + rows) x columns [256 blockIdx.x, + 256) of a layer; block = one wave.
//   g'[b, n] = g[b, n] * (epi LRELU: y[b, n] > 0 ? 1 : slope;  WALK: a[b];  NONE: 1)
//   gw[n, k] (+)= sum_b g'[b, n] x[b, k]      gb[n] (+)= sum_b g'[b, n]  (column block 0)      part[slice][b, k] = sum_{n in slice} g'[b, n] W[n, k]
template <int NB>
__global__ __launch_bounds__(64) void linear_rows_bwd_kernel(float* __restrict__ gw, float* __restrict__ gb, float* __restrict__ part,
                                                             const float* __restrict__ add, const float* __restrict__ g, const float* __restrict__ y,
                                                             const float* __restrict__ a, const float* __restrict__ x, const float* __restrict__ w,
                                                             int B, int K, int N, int rows, int epi, float slope) {
    extern __shared__ __attribute__((aligned(16))) float gp[];     // [rows][NB]
    const int lane = threadIdx.x;
    const int k = blockIdx.x * KT + lane * 4;
    const bool kok = k < K;                                        // K % 64 == 0: a float4 is inside or outside as a whole
    const int n0 = blockIdx.y * rows;
    for (int b0 = 0; b0 < B; b0 += NB) {
        const int nb = (B - b0) < NB ? (B - b0) : NB;
        __syncthreads();                                            // the previous chunk's reads of gp are done
        for (int i = lane; i < rows * NB; i += 64) {
            const int r = i / NB, q = i - r * NB;
            float v = 0.f;
            if (q < nb) {
                const long gi = (long)(b0 + q) * N + n0 + r;
                v = g[gi];
                if (epi == L2I_LINEAR_LRELU) v = y[gi] > 0.f ? v : v * slope;
                else if (epi == L2I_LINEAR_WALK) v = a[b0 + q] * v;
            }
            gp[i] = v;
        }
        __syncthreads();
        if (gb && blockIdx.x == 0 && lane < rows) {                 // lane r: the bias gradient of row n0 + r, b in index order
            float s = b0 ? gb[n0 + lane] : 0.f;
            for (int q = 0; q < nb; ++q) s += gp[lane * NB + q];
            gb[n0 + lane] = s;
        }
        if (!kok) continue;                                         // (a one-wave block: the barrier above is passed by the wave as a whole)
        float4 xr[NB], gx[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            xr[q] = q < nb ? ld4(x + (long)(b0 + q) * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            gx[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll 4
        for (int r = 0; r < rows; ++r) {
            const long wi = (long)(n0 + r) * K + k;
            float4 wr = make_float4(0.f, 0.f, 0.f, 0.f), acc = wr;
            if (part) wr = ld4(w + wi);
            if (b0) acc = ld4(gw + wi);                             // a later chunk of a batch beyond 16 adds to the earlier ones, in index order
#pragma unroll
            for (int q4 = 0; q4 < NB; q4 += 4) {
                const float4 gv = *reinterpret_cast<const float4*>(&gp[r * NB + q4]);      // same address in every lane: LDS broadcast
                const float gs[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int q = q4 + j;
                    acc.x = __builtin_fmaf(gs[j], xr[q].x, acc.x); acc.y = __builtin_fmaf(gs[j], xr[q].y, acc.y);
                    acc.z = __builtin_fmaf(gs[j], xr[q].z, acc.z); acc.w = __builtin_fmaf(gs[j], xr[q].w, acc.w);
                    if (part) {
                        gx[q].x = __builtin_fmaf(gs[j], wr.x, gx[q].x); gx[q].y = __builtin_fmaf(gs[j], wr.y, gx[q].y);
                        gx[q].z = __builtin_fmaf(gs[j], wr.z, gx[q].z); gx[q].w = __builtin_fmaf(gs[j], wr.w, gx[q].w);
                    }
                }
            }
            *reinterpret_cast<float4*>(gw + wi) = acc;
        }
        if (part) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                if (q < nb) {
                    const long xi = (long)(b0 + q) * K + k;
                    float4 v = gx[q];
                    if (add) { const float4 t = ld4(add + xi); v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }     // (one slice: part is gx itself)
                    *reinterpret_cast<float4*>(part + (long)blockIdx.y * B * K + xi) = v;
                }
            }
        }
    }
}

// gx[i] = (part[0][i] + part[1][i] + ... in slice order) + add[i], i < B K (float4 per thread)
__global__ __launch_bounds__(256) void linear_rows_slice_sum_kernel(float* __restrict__ gx, const float* __restrict__ part, const float* __restrict__ add,
                                                                    long n, int slices) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    float4 s = ld4(part + i);
    int sl = 1;
    for (; sl + 8 <= slices; sl += 8) {                             // eight loads in flight, added in slice order
        float4 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = ld4(part + (long)(sl + j) * n + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) { s.x += t[j].x; s.y += t[j].y; s.z += t[j].z; s.w += t[j].w; }
    }
    for (; sl < slices; ++sl) { const float4 t = ld4(part + (long)sl * n + i); s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
    if (add) { const float4 t = ld4(add + i); s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
    *reinterpret_cast<float4*>(gx + i) = s;
}

static bool walk_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static const char* walk_shape_error(int B, int K, int N, int epi, float slope) {
    if (B <= 0 || K <= 0 || N <= 0) return "non-positive size";
    if (K % 64 || N % 64) return "K and N must be multiples of 64";
    if (epi != L2I_LINEAR_NONE && epi != L2I_LINEAR_LRELU && epi != L2I_LINEAR_WALK) return "unknown epilogue";
    if (!(slope == slope)) return "slope is NaN";
    return nullptr;
}

extern "C" int l2i_linear_rows_f32(float* y, const float* x, const float* w, const float* bias, const float* res, const float* a, int B, int K, int N,
                                   int epi, float slope, void* stream) {
    if (!y || !x || !w || !bias) return l2i_set_error(L2I_E_ARG, "linear_rows: null pointer");
    if (const char* e = walk_shape_error(B, K, N, epi, slope)) return l2i_set_error(L2I_E_ARG, e);
    if (epi == L2I_LINEAR_WALK && (!res || !a)) return l2i_set_error(L2I_E_ARG, "linear_rows: the walk epilogue needs the residual and alpha");
    if (!walk_aligned16(x) || !walk_aligned16(w)) return l2i_set_error(L2I_E_ARG, "linear_rows: x and w are read as float4 and must sit on 16-byte boundaries");
    const dim3 grid((unsigned)(N / (4 * FR)));
    hipStream_t st = (hipStream_t)stream;
    if (B <= 4) hipLaunchKernelGGL(linear_rows_kernel<4>, grid, dim3(256), 0, st, y, x, w, bias, res, a, B, K, N, epi, slope);
    else if (B <= 8) hipLaunchKernelGGL(linear_rows_kernel<8>, grid, dim3(256), 0, st, y, x, w, bias, res, a, B, K, N, epi, slope);
    else hipLaunchKernelGGL(linear_rows_kernel<16>, grid, dim3(256), 0, st, y, x, w, bias, res, a, B, K, N, epi, slope);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_linear_rows_bwd_f32(float* gw, float* gb, float* gx, float* ws, const float* gx_add, const float* g, const float* y, const float* a,
                                       const float* x, const float* w, int B, int K, int N, int epi, float slope, int slices, void* stream) {
    if (!gw || !g || !x) return l2i_set_error(L2I_E_ARG, "linear_rows_bwd: null pointer");
    if (const char* e = walk_shape_error(B, K, N, epi, slope)) return l2i_set_error(L2I_E_ARG, e);
    if (epi == L2I_LINEAR_LRELU && !y) return l2i_set_error(L2I_E_ARG, "linear_rows_bwd: the LeakyReLU mask needs the layer's output");
    if (epi == L2I_LINEAR_WALK && !a) return l2i_set_error(L2I_E_ARG, "linear_rows_bwd: the walk's tail needs alpha");
    if (slices < 1 || N % slices || N / slices > 64) return l2i_set_error(L2I_E_ARG, "linear_rows_bwd: slices must divide N into at most 64 rows each");
    if (slices > 65535) return l2i_set_error(L2I_E_ARG, "linear_rows_bwd: more than 65535 slices");
    if (gx && (!w || (slices > 1 && !ws))) return l2i_set_error(L2I_E_ARG, "linear_rows_bwd: gx needs w, and a workspace of slices * B * K floats when slices > 1");
    if (!gx && gx_add) return l2i_set_error(L2I_E_ARG, "linear_rows_bwd: gx_add without gx");
    if (!walk_aligned16(gw) || !walk_aligned16(x) || !walk_aligned16(w) || !walk_aligned16(gx) || !walk_aligned16(ws) || !walk_aligned16(gx_add))
        return l2i_set_error(L2I_E_ARG, "linear_rows_bwd: gw, x, w, gx, ws and gx_add are accessed as float4 and must sit on 16-byte boundaries");
    const int rows = N / slices;
    const dim3 grid((unsigned)((K + KT - 1) / KT), (unsigned)slices);
    hipStream_t st = (hipStream_t)stream;
    float* part = !gx ? nullptr : (slices == 1 ? gx : ws);
    const float* add1 = slices == 1 ? gx_add : nullptr;             // one slice: the pass writes gx itself, residual included
#define L2I_WALK_BWD(NB) hipLaunchKernelGGL(linear_rows_bwd_kernel<NB>, grid, dim3(64), (size_t)rows * NB * sizeof(float), st, gw, gb, part, add1, g, y, a, x, w, B, K, N, rows, epi, slope)
    if (B <= 4) L2I_WALK_BWD(4);
    else if (B <= 8) L2I_WALK_BWD(8);
    else L2I_WALK_BWD(16);
#undef L2I_WALK_BWD
    L2I_CHECK_LAUNCH();
    if (gx && slices > 1) {
        const long n = (long)B * K;
        hipLaunchKernelGGL(linear_rows_slice_sum_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, gx, ws, gx_add, n, slices);
        L2I_CHECK_LAUNCH();
    }
    return L2I_OK;
}
