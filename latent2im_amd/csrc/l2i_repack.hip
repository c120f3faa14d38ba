// l2i_repack.hip — what a net that is being TRAINED needs between two optimiser steps, in the memory it already occupies and without a host
// round trip, so that a captured hipGraph can hold it: the packed forms of a convolution weight rewritten from the weight itself, and a batch
// gathered from a dataset that lives on the device.
//
//   l2i_repack_taps_f32     every pack that is a permutation of w [Cout][Cin][K][K] (conv.pack_weight of the forward weight, of the flipped /
//                           role-swapped gradient weight, of a stride-2 gradient's parity sub-weights, FusedTransposed.w, SmallTransposed.w, w4):
//                           dst[r][t][c] = swap ? w[r][c][ky_t][kx_t] : w[c][r][ky_t][kx_t], zero for c >= the real column count.  One thread
//                           owns four consecutive c of one (r, t): one 16-byte store; the four loads are a 16-byte load too where the source is
//                           contiguous along c (swap, K = 1).  layout L2I_REPACK_OIHW writes the plain [rows][cols][taps] form (the w_src copies).
//   l2i_repack_wino_f32     U = G g G^T of a 3x3 weight for F(2x2) (4x4) or F(4x4) (6x6) in float64, in a FIXED order — T[i][l] = sum_k G[i][k] g[k][l]
//                           with k ascending, then U[i][j] = sum_l T[i][l] G[j][l] with l ascending, starting from the first product, zeros of G
//                           multiplied like every other entry, every product and sum rounded on its own (fp contract(off): no fused multiply-add) —
//                           rounded once to fp32 and written in the layout of conv.pack_weight_wino / pack_weight_wino4.  One thread per
//                           (input channel, padded output channel).
//   l2i_batch_from_u8_f32   out[b] = (fl(src[idx[b]] / 255) - 0.5) * 2 (CustomDataset's float32 expression; the division correctly rounded, the
//                           other two operations exact or a single rounding), labels gathered by the same index; an index outside [0, N) writes
//                           zeros and reads nothing.  16 bytes in, four 16-byte stores out per thread where the image size allows.
// All three are bandwidth trivial at ResNet-50 sizes (the whole net is 94 MB of weights): they are launch bound, which is the point of replaying them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_internal.h"

struct RepackTapsParams {
    float* dst; const float* w;
    int Cout, Cin, KK, K, rows, cols, colsP, ntaps, swap;
    l2i_repack_taps taps;
};

__global__ __launch_bounds__(256) void repack_taps_kernel(const RepackTapsParams p, long long nvec) {
    const int c4n = p.colsP >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
        const int c0 = (int)(i % c4n) * 4;
        const long long rt = i / c4n;
        const int t = (int)(rt % p.ntaps), r = (int)(rt / p.ntaps);
        const int tap = (int)p.taps.ky[t] * p.K + (int)p.taps.kx[t];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.swap) {                                              // w[r][c][tap]: consecutive c are KK floats apart
            const float* s = p.w + ((size_t)r * p.Cin + c0) * p.KK + tap;
            if (p.KK == 1 && c0 + 3 < p.cols && (((uintptr_t)s) & 15) == 0) {
                v = *reinterpret_cast<const float4*>(s);
            } else {
                if (c0 < p.cols) v.x = s[0];
                if (c0 + 1 < p.cols) v.y = s[p.KK];
                if (c0 + 2 < p.cols) v.z = s[2 * (size_t)p.KK];
                if (c0 + 3 < p.cols) v.w = s[3 * (size_t)p.KK];
            }
        } else {                                                   // w[c][r][tap]: consecutive c are Cin * KK floats apart
            const size_t cs = (size_t)p.Cin * p.KK;
            const float* s = p.w + ((size_t)c0 * p.Cin + r) * p.KK + tap;
            if (c0 < p.cols) v.x = s[0];
            if (c0 + 1 < p.cols) v.y = s[cs];
            if (c0 + 2 < p.cols) v.z = s[2 * cs];
            if (c0 + 3 < p.cols) v.w = s[3 * cs];
        }
        *reinterpret_cast<float4*>(p.dst + (size_t)rt * p.colsP + c0) = v;
    }
}

// the [rows][cols][taps] form (a Launch's w_src): one element per thread, stores consecutive along t
__global__ __launch_bounds__(256) void repack_oihw_kernel(const RepackTapsParams p, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int t = (int)(i % p.ntaps);
        const long long rc = i / p.ntaps;
        const int c = (int)(rc % p.cols), r = (int)(rc / p.cols);
        const int tap = (int)p.taps.ky[t] * p.K + (int)p.taps.kx[t];
        p.dst[i] = p.swap ? p.w[((size_t)r * p.Cin + c) * p.KK + tap] : p.w[((size_t)c * p.Cin + r) * p.KK + tap];
    }
}

extern "C" int l2i_repack_taps_f32(float* dst, const float* w, int Cout, int Cin, int K, const l2i_repack_taps* taps, int swap, int colsP, int layout,
                                   void* stream) {
    if (!dst || !w || !taps) return l2i_set_error(L2I_E_ARG, "repack_taps: null pointer");
    if (Cout <= 0 || Cin <= 0 || K <= 0 || K > 7) return l2i_set_error(L2I_E_ARG, "repack_taps: Cout, Cin >= 1 and 1 <= K <= 7");
    if (taps->count < 1 || taps->count > L2I_REPACK_MAX_TAPS) return l2i_set_error(L2I_E_ARG, "repack_taps: 1 .. 49 taps");
    for (int t = 0; t < taps->count; ++t)
        if (taps->ky[t] >= K || taps->kx[t] >= K) return l2i_set_error(L2I_E_ARG, "repack_taps: a tap outside the K x K weight");
    if (layout != L2I_REPACK_PACKED && layout != L2I_REPACK_OIHW) return l2i_set_error(L2I_E_ARG, "repack_taps: unknown layout");
    RepackTapsParams p;
    p.dst = dst; p.w = w; p.Cout = Cout; p.Cin = Cin; p.K = K; p.KK = K * K; p.swap = swap ? 1 : 0;
    p.rows = swap ? Cout : Cin; p.cols = swap ? Cin : Cout; p.colsP = colsP; p.ntaps = taps->count; p.taps = *taps;
    if (colsP < p.cols) return l2i_set_error(L2I_E_ARG, "repack_taps: colsP below the real column count");
    if (layout == L2I_REPACK_OIHW) {
        if (colsP != p.cols) return l2i_set_error(L2I_E_ARG, "repack_taps: the [rows][cols][taps] layout has no padding columns");
        const long long n = (long long)p.rows * p.cols * p.ntaps;
        hipLaunchKernelGGL(repack_oihw_kernel, dim3(l2i_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, p, n);
    } else {
        if (colsP % 4 || (((uintptr_t)dst) & 15)) return l2i_set_error(L2I_E_ARG, "repack_taps: colsP % 4 == 0 and a 16-byte aligned dst (16-byte stores)");
        const long long nvec = (long long)p.rows * p.ntaps * (colsP / 4);
        hipLaunchKernelGGL(repack_taps_kernel, dim3(l2i_grid_for(nvec, 256)), dim3(256), 0, (hipStream_t)stream, p, nvec);
    }
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Winograd weight transforms
// ---------------------------------------------------------------------------------------------------------------
__constant__ double WINO2_G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
__constant__ double WINO4_G[6][3] = {{1.0 / 4, 0.0, 0.0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                     {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0.0, 0.0, 1.0}};

template <int M>
__device__ __forceinline__ void wino_transform(float (&U)[M][M], const double (&g)[3][3], const double (*G)[3]) {
#pragma clang fp contract(off)                                   // every product and sum below is an instruction of its own
    double T[M][3];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const double a = G[i][0] * g[0][l], b = G[i][1] * g[1][l], c = G[i][2] * g[2][l];
            const double ab = a + b;
            T[i][l] = ab + c;
        }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const double a = T[i][0] * G[j][0], b = T[i][1] * G[j][1], c = T[i][2] * G[j][2];
            const double ab = a + b;
            U[i][j] = (float)(ab + c);
        }
}

// conv seen by the pack: co' < coutP, ci' < cin with (cout', cin') = swap ? (Cin, Cout) : (Cout, Cin); g[k][l] = w[..][flip ? 2 - k : k][flip ? 2 - l : l]
template <int M>
__global__ __launch_bounds__(256) void repack_wino_kernel(float* __restrict__ dst, const float* __restrict__ w, int Cout, int Cin, int swap, int flip,
                                                          int cout, int cin, int coutP) {
    const long long n = (long long)cin * coutP;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int co = (int)(i % coutP), ci = (int)(i / coutP);
        float U[M][M];
        if (co < cout) {
            const float* s = w + (swap ? ((size_t)ci * Cin + co) : ((size_t)co * Cin + ci)) * 9;
            double g[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int l = 0; l < 3; ++l) g[k][l] = (double)s[flip ? 8 - (k * 3 + l) : k * 3 + l];
            wino_transform<M>(U, g, M == 4 ? WINO2_G : WINO4_G);
        } else {
#pragma unroll
            for (int a = 0; a < M; ++a)
#pragma unroll
                for (int b = 0; b < M; ++b) U[a][b] = 0.f;
        }
        if constexpr (M == 4) {                                    // [cin][4 i][coutP][4 j]
#pragma unroll
            for (int a = 0; a < 4; ++a)
                *reinterpret_cast<float4*>(dst + (((size_t)ci * 4 + a) * coutP + co) * 4) = make_float4(U[a][0], U[a][1], U[a][2], U[a][3]);
        } else {                                                   // [cin / 4][coutP / 16][ [6 i][4 k][16 m][4 j] ++ [6 i][4 k][16 m][2 j] ]
            float* base = dst + ((size_t)(ci >> 2) * (coutP >> 4) + (co >> 4)) * 2304;
            const int k = ci & 3, m = co & 15;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const int slot = (a * 4 + k) * 16 + m;
                *reinterpret_cast<float4*>(base + slot * 4) = make_float4(U[a][0], U[a][1], U[a][2], U[a][3]);
                *reinterpret_cast<float2*>(base + 1536 + slot * 2) = make_float2(U[a][4], U[a][5]);
            }
        }
    }
}

extern "C" int l2i_repack_wino_f32(float* dst, const float* w, int Cout, int Cin, int kind, int swap, int flip, void* stream) {
    if (!dst || !w) return l2i_set_error(L2I_E_ARG, "repack_wino: null pointer");
    if (Cout <= 0 || Cin <= 0) return l2i_set_error(L2I_E_ARG, "repack_wino: non-positive dimension");
    if (kind != L2I_REPACK_WINO2 && kind != L2I_REPACK_WINO4) return l2i_set_error(L2I_E_ARG, "repack_wino: kind is L2I_REPACK_WINO2 or L2I_REPACK_WINO4");
    if (((uintptr_t)dst) & 15) return l2i_set_error(L2I_E_ARG, "repack_wino: dst off a 16-byte boundary");
    const int cout = swap ? Cin : Cout, cin = swap ? Cout : Cin, coutP = (cout + 31) / 32 * 32;
    if (kind == L2I_REPACK_WINO4 && cin % 4) return l2i_set_error(L2I_E_ARG, "repack_wino: the F(4x4) pack takes whole 4-channel chunks");
    const dim3 grid(l2i_grid_for((long long)cin * coutP, 256));
    if (kind == L2I_REPACK_WINO2)
        hipLaunchKernelGGL(repack_wino_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, dst, w, Cout, Cin, swap ? 1 : 0, flip ? 1 : 0, cout, cin, coutP);
    else
        hipLaunchKernelGGL(repack_wino_kernel<6>, grid, dim3(256), 0, (hipStream_t)stream, dst, w, Cout, Cin, swap ? 1 : 0, flip ? 1 : 0, cout, cin, coutP);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Device-resident dataset: a normalised batch by index
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float normalise_u8(unsigned v) {
#pragma clang fp contract(off)
    const float a = __fdiv_rn((float)v, 255.f);
    const float d = a - 0.5f;
    return d * 2.f;                                                // (a / 255 - 0.5) / 0.5: the division by 0.5 is an exact doubling
}

// grid.y = sample; VEC: 16 source bytes a thread
template <bool VEC>
__global__ __launch_bounds__(256) void batch_from_u8_kernel(float* __restrict__ out, float* __restrict__ label_out, const uint8_t* __restrict__ src,
                                                            const float* __restrict__ labels, const long long* __restrict__ idx, long long N,
                                                            long long elems, int L) {
    const int b = blockIdx.y;
    const long long j = idx[b];
    const bool ok = j >= 0 && j < N;
    float* o = out + (size_t)b * elems;
    const uint8_t* s = src + (ok ? (size_t)j * elems : 0);
    if (VEC) {
        const long long nv = elems >> 4;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (ok) q = reinterpret_cast<const uint4*>(s)[i];
            const unsigned wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) v = make_float4(normalise_u8(wd[k] & 255u), normalise_u8((wd[k] >> 8) & 255u), normalise_u8((wd[k] >> 16) & 255u),
                                        normalise_u8(wd[k] >> 24));
                reinterpret_cast<float4*>(o)[i * 4 + k] = v;
            }
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < elems; i += (long long)gridDim.x * 256)
            o[i] = ok ? normalise_u8(s[i]) : 0.f;
    }
    if (label_out && blockIdx.x == 0)
        for (int i = threadIdx.x; i < L; i += 256) label_out[(size_t)b * L + i] = ok ? labels[(size_t)j * L + i] : 0.f;
}

extern "C" int l2i_batch_from_u8_f32(float* out, float* label_out, const uint8_t* src, const float* labels, const int64_t* idx, int B, int64_t N,
                                     int64_t elems, int L, void* stream) {
    if (!out || !src || !idx) return l2i_set_error(L2I_E_ARG, "batch_from_u8: null pointer");
    if (B <= 0 || B > 65535 || N <= 0 || elems <= 0) return l2i_set_error(L2I_E_ARG, "batch_from_u8: 1 <= B <= 65535, N >= 1, elems >= 1");
    if (label_out && (!labels || L <= 0)) return l2i_set_error(L2I_E_ARG, "batch_from_u8: label_out needs labels and L >= 1");
    const bool vec = elems % 16 == 0 && (((uintptr_t)src) & 15) == 0 && (((uintptr_t)out) & 15) == 0;
    const dim3 grid(l2i_grid_for(vec ? elems / 16 : elems, 256, 256), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(batch_from_u8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out, label_out, src, labels, (const long long*)idx,
                           (long long)N, (long long)elems, L);
    else
        hipLaunchKernelGGL(batch_from_u8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out, label_out, src, labels, (const long long*)idx,
                           (long long)N, (long long)elems, L);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
