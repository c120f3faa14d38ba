// l2i_gram_common.h — the second and third pass of the Gram-matrix loss, shared by its fp32 (l2i_gram.hip) and h8 (l2i_gram_h8.hip) first
// passes: both leave one 32x32 fp32 partial tile per (sample, tile pair i <= j, HW slice) in ws, and from there on the element type of the
// tap no longer matters.  Internal linkage: every translation unit that includes this launches its own copy.
#ifndef L2I_GRAM_COMMON_H
#define L2I_GRAM_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i_device.h"

namespace gr {
constexpr int KC = 256;                    // pixels per staged chunk; slices are whole chunks
constexpr int TILE = 32 * 32;
}

// pair index -> (i, j), i <= j, row-major over the upper triangle of T x T tiles
__device__ __forceinline__ void gram_pair(int pair, int T, int& i, int& j) {
    int row = 0, left = pair;
    while (left >= T - row) { left -= T - row; ++row; }
    i = row; j = row + left;
}

// block (tile pair, sample): partial tiles added in slice order, / (C HW), G and its mirror written, D = G - Gt and the pair's sum of D^2
// (off-diagonal entries counted twice)
static __global__ __launch_bounds__(256) void gram_reduce_kernel(float* __restrict__ G, float* __restrict__ D, float* __restrict__ pair_loss, const float* __restrict__ ws,
                                                                 const float* __restrict__ Gt, int C, float norm, int nslices, int npairs) {
    __shared__ float red[4];
    const int tid = threadIdx.x, pair = blockIdx.x, b = blockIdx.y;
    int ti, tj;
    gram_pair(pair, C / 32, ti, tj);
    const float* part = ws + ((size_t)b * npairs + pair) * nslices * gr::TILE;
    const size_t base = (size_t)b * C * C;
    float sq = 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int e = tid + 256 * n, row = e >> 5, col = e & 31;
        if (ti == tj && row > col) continue;   // a diagonal tile writes its own lower triangle as the mirror of the upper one
        float s = 0.f;
        for (int k = 0; k < nslices; ++k) s += part[(size_t)k * gr::TILE + e];
        const float g = s / norm;
        const size_t up = base + (size_t)(ti * 32 + row) * C + tj * 32 + col, lo = base + (size_t)(tj * 32 + col) * C + ti * 32 + row;
        G[up] = g;
        G[lo] = g;
        if (Gt) {
            const float d = g - Gt[up];
            D[up] = d;
            D[lo] = d;
            sq += (up == lo ? 1.f : 2.f) * (d * d);
        }
    }
    if (Gt) {
        sq = block_sum(sq, red);
        if (tid == 0) pair_loss[(size_t)b * npairs + pair] = sq;
    }
}

// block (sample): the pair sums in pair order, loss[b] += C^2 * sum
static __global__ __launch_bounds__(256) void gram_finish_kernel(float* __restrict__ loss, const float* __restrict__ pair_loss, int npairs, float c2) {
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    float s = 0.f;
    for (int k = tid; k < npairs; k += 256) s += pair_loss[(size_t)b * npairs + k];
    s = block_sum(s, red);
    if (tid == 0) loss[b] += c2 * s;
}

#endif
