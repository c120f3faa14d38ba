// l2i_gram.hip — the VGG-16 Gram-matrix term of the inversion loss and its gradient (gfx950, fp32).  Entry points l2i_gram_loss_f32,
// l2i_gram_bwd_f32 (include/l2i.h).
//
// Reference: BP.py:68-73 (gram: G = f f^T / (ch h w) on a post-ReLU tap), :173-184 (perceptual_loss: per tap, sum (G_data - G_logit)^2 * C^2).
// Here the tap arrives as the PRE-ReLU conv output c (perceptual16.py carries the ReLU as masks, as perceptual.py does), so the ReLU is applied
// to the fragments after the LDS read and relu(c) is never materialised.
//
// Forward, three launches, all sums in a fixed order (no floating-point atomics: equal inputs give equal bits):
//   gram_partial_kernel   block (HW slice, tile pair i <= j, sample): rows of tile i (and of tile j when j != i) of a 256-pixel chunk go
//                         global -> LDS by DMA, ONE staged image feeds both MFMA operands (A[row][k] and B[k][col] are the same lane map on
//                         v_mfma_f32_32x32x2_f32: lane = row, half = k), the four waves take 64 pixels of the chunk each and their four
//                         32x32 accumulators are added in wave order into the slice's partial tile.
//   gram_reduce_kernel    (l2i_gram_common.h, shared with the h8 file, as is gram_finish_kernel) block (tile pair, sample): partial tiles added in slice order, / (C HW), G and its mirror written, D = G - Gt and the
//                         pair's sum of D^2 (off-diagonal entries counted twice).
//   gram_finish_kernel    block (sample): the pair sums in pair order, loss[b] += C^2 * sum.
// Backward: g[b] (+)= coef * scale[b * scale_stride] * (c[b] > 0) * (D[b] relu(c[b])), a [C, C] x [C, HW] product per sample with the K loop of l2i_gemm.hip
// (both operand tiles by DMA, double-buffered, ds_read + MFMA only) and D, being symmetric, as its own K-major form.  Its epilogue is two
// lines (mask and scale, optional add) straight from the accumulators: it is NOT the fused conv epilogue.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"
#include "l2i_gram_common.h"      // gram_pair, gram_reduce_kernel, gram_finish_kernel

namespace gr {
// (KC = 256 pixels per staged chunk, l2i_gram_common.h: one row of a chunk = 1 KiB = one wave DMA)
constexpr int RS = KC + 4;                 // LDS row stride in floats: 65 sixteen-byte units, odd, so the 16 lanes of a ds_read_b128 group (distinct rows) hit distinct banks
constexpr int CK = 16, CKh = 8, BN = 256;  // backward: channels per chunk, pixels per block
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void gram_partial_kernel(float* __restrict__ ws, const float* __restrict__ c, int C, int HW, int SL, int nslices, int npairs) {
    using namespace gr;
    extern __shared__ __attribute__((aligned(16))) float smem[];       // [64 or 32 rows][RS]; afterwards four 32x32 wave tiles
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
    const int slice = blockIdx.x, pair = blockIdx.y, b = blockIdx.z;
    int ti, tj;
    gram_pair(pair, C / 32, ti, tj);
    const bool diag = ti == tj;
    const int nrows = diag ? 32 : 64;
    const float* cb = c + (size_t)b * C * HW;
    const unsigned bytes = (unsigned)((size_t)C * HW * sizeof(float));
    const __amdgpu_buffer_rsrc_t rs = l2i_buffer_rsrc(cb, bytes);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int p_begin = slice * SL;
    const int p_end = min(HW, p_begin + SL);

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    for (int p0 = p_begin; p0 < p_end; p0 += KC) {
        if constexpr (VEC) {
            // row q of the stage <- channel (q < 32 ? 32 ti : 32 tj - 32) + q, pixels p0 + 4 lane .. + 3; a lane past the slice reads past the buffer: zeros
            const int px = p0 + lane * 4;
            for (int q = wave_u; q < nrows; q += 4) {
                const int ch = (q < 32 ? ti * 32 : tj * 32 - 32) + q;
                const unsigned voff = px < p_end ? (unsigned)(((size_t)ch * HW + px) * sizeof(float)) : bytes;
                l2i_lds_dma16(voff, rs, __builtin_amdgcn_readfirstlane(l2i_lds_addr(smem + q * RS)), 0u);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            const int px = p0 + tid;
            for (int q = 0; q < nrows; ++q) {
                const int ch = (q < 32 ? ti * 32 : tj * 32 - 32) + q;
                smem[q * RS + tid] = px < p_end ? cb[(size_t)ch * HW + px] : 0.f;
            }
        }
        __syncthreads();
        const float* ab = smem + r * RS + wave * 64 + half * 4;
        const float* bb = ab + (diag ? 0 : 32 * RS);
#pragma unroll
        for (int q = 0; q < 8; ++q) {          // 8 pixels per step: half h holds pixels 8 q + 4 h .. + 3, k-step t contracts pixels 8 q + t and 8 q + 4 + t
            f32x4 a = *reinterpret_cast<const f32x4*>(ab + q * 8);
            f32x4 bv = *reinterpret_cast<const f32x4*>(bb + q * 8);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float av = fmaxf(a[t], 0.f), bw = fmaxf(bv[t], 0.f);      // the ReLU, on load
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bw, acc, 0, 0, 0);
            }
        }
        __syncthreads();                       // the stage is free again
    }
    // the four waves' tiles, added in wave order
    float* wt = smem + wave * TILE;
#pragma unroll
    for (int e = 0; e < 16; ++e) wt[((e & 3) + 8 * (e >> 2) + 4 * half) * 32 + r] = acc[e];
    __syncthreads();
    float* out = ws + (((size_t)b * npairs + pair) * nslices + slice) * TILE;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int e = tid + 256 * n;
        out[e] = (smem[e] + smem[TILE + e]) + (smem[2 * TILE + e] + smem[3 * TILE + e]);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------------
template <int WM, bool VEC>
__global__ __launch_bounds__(256, 2) void gram_bwd_kernel(float* __restrict__ g, const float* __restrict__ c, const float* __restrict__ D, const float* __restrict__ scale,
                                                          float coef, int C, int HW, int accumulate, int scale_stride) {
    using namespace gr;
    constexpr int BM = WM * 32;
    constexpr int XS = CK * BN, WS = CK * BM, STAGE = XS + WS;         // floats per stage: relu-less c rows | D rows
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, j = lane & 31;
    const int mblk = blockIdx.x, tile = blockIdx.y, b = blockIdx.z;      // (grid indices, not divisions: the descriptors below must be built from scalar registers)
    const int m0 = mblk * BM, px0 = tile * BN;
    const float* cb = c + (size_t)b * C * HW;
    const float* Db = D + (size_t)b * C * C;
    const unsigned x_bytes = (unsigned)((size_t)C * HW * sizeof(float)), d_bytes = (unsigned)((size_t)C * C * sizeof(float));
    const __amdgpu_buffer_rsrc_t rs_x = l2i_buffer_rsrc(cb, x_bytes);
    const __amdgpu_buffer_rsrc_t rs_d = l2i_buffer_rsrc(Db, d_bytes);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    constexpr int WV = BM / 4, WPIECES = CK * WV / 64;                 // float4 per D row, wave pieces per chunk (4 for BM = 64, 2 for BM = 32)

    // stage <- channels c0 .. c0 + 15: c rows (row k * 4 + wave: 256 pixels = one wave DMA) and the D rows' BM columns from m0
    auto fill = [&](int c0, float* stage) {
        if constexpr (VEC) {
            const int px = px0 + lane * 4;
#pragma unroll
            for (int k = 0; k < CK / 4; ++k) {
                const int row = k * 4 + wave_u;
                const unsigned voff = px < HW ? (unsigned)(((size_t)(c0 + row) * HW + px) * sizeof(float)) : x_bytes;
                l2i_lds_dma16(voff, rs_x, __builtin_amdgcn_readfirstlane(l2i_lds_addr(stage + row * BN)), 0u);
            }
        } else {
            const int px = px0 + tid;
#pragma unroll
            for (int row = 0; row < CK; ++row) stage[row * BN + tid] = px < HW ? cb[(size_t)(c0 + row) * HW + px] : 0.f;
        }
        if (wave_u < WPIECES) {                // D rows are 16-byte aligned for every supported C (C % 32 == 0): always by DMA
            const int q = wave_u * 64 + lane;
            const unsigned voff = (unsigned)(((size_t)(c0 + q / WV) * C + m0 + (q % WV) * 4) * sizeof(float));
            l2i_lds_dma16(voff, rs_d, __builtin_amdgcn_readfirstlane(l2i_lds_addr(stage + XS + wave_u * 256)), 0u);
        }
    };

    f32x16 acc[WM][2];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

    const int nchunks = C / CK;
    fill(0, smem);
    for (int ch = 0; ch < nchunks; ++ch) {
        float* st = smem + (ch & 1) * STAGE;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this chunk's tiles have landed
        __syncthreads();                                   // ... for every wave; the other stage is free to refill
        if (ch + 1 < nchunks) fill((ch + 1) * CK, smem + ((ch + 1) & 1) * STAGE);
        const float* xb = st + half * CKh * BN + wave * 64 + j;
        const float* wb = st + XS + half * CKh * BM + j;
#pragma unroll
        for (int pp = 0; pp < CKh; ++pp) {
            float a[WM], bb[2];
#pragma unroll
            for (int m = 0; m < WM; ++m) a[m] = wb[pp * BM + m * 32];
#pragma unroll
            for (int n = 0; n < 2; ++n) bb[n] = fmaxf(xb[pp * BN + n * 32], 0.f);      // the ReLU, on load
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bb[n], acc[m][n], 0, 0, 0);
        }
    }
    // ---- epilogue: mask and scale, optional add.  Register e of lane (half, j) is row (e & 3) + 8 (e >> 2) + 4 half, pixel j of its 32 x 32 tile
    const float cs = coef * (scale ? scale[(size_t)b * scale_stride] : 1.f);
    float* gb = g + (size_t)b * C * HW;
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int px = px0 + wave * 64 + n * 32 + j;
            if (px >= HW) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const size_t idx = (size_t)(m0 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * half) * HW + px;
                const float v = cb[idx] > 0.f ? acc[m][n][e] * cs : 0.f;
                gb[idx] = accumulate ? gb[idx] + v : v;
            }
        }
}

static bool gram_shape_ok(int C) { return C > 0 && (C % 32) == 0 && C <= 512; }
static bool al16(const void* q) { return (((uintptr_t)q) % 16) == 0; }

extern "C" int l2i_gram_loss_f32(float* G, float* D, float* loss, const float* c, const float* Gt, float* ws, int B, int C, int HW, int nslices,
                                 void* stream) {
    if (!gram_shape_ok(C)) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_loss: built for C % 32 == 0, C <= 512");
    if (!G || !c || !ws || B <= 0 || HW <= 0 || nslices <= 0) return l2i_set_error(L2I_E_ARG, "gram_loss: null tensor or non-positive dimension");
    if (Gt && (!D || !loss)) return l2i_set_error(L2I_E_ARG, "gram_loss: a target needs D and loss");
    if ((size_t)C * HW * sizeof(float) >= 0xFFFFFFF0ull) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_loss: one sample's map must stay below 4 GiB");
    if (nslices > (HW + gr::KC - 1) / gr::KC) return l2i_set_error(L2I_E_ARG, "gram_loss: more slices than 256-pixel chunks");
    if (B > 65535) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_loss: B <= 65535");
    const int T = C / 32, npairs = T * (T + 1) / 2;
    const int per = (HW + nslices - 1) / nslices;
    const int SL = (per + gr::KC - 1) / gr::KC * gr::KC;               // whole chunks per slice; trailing slices may be empty (they write zeros)
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)64 * gr::RS * sizeof(float);
    const bool vec = (HW % 4) == 0 && al16(c);
    const dim3 grid((unsigned)nslices, (unsigned)npairs, (unsigned)B), t(256);
    if (vec) {
        L2I_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gram_partial_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(gram_partial_kernel<true>, grid, t, lds, st, ws, c, C, HW, SL, nslices, npairs);
    } else {
        L2I_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gram_partial_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(gram_partial_kernel<false>, grid, t, lds, st, ws, c, C, HW, SL, nslices, npairs);
    }
    L2I_CHECK_LAUNCH();
    float* pair_loss = ws + (size_t)B * npairs * nslices * gr::TILE;
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)npairs, (unsigned)B), t, 0, st, G, D, pair_loss, ws, Gt, C, (float)((double)C * (double)HW), nslices, npairs);
    L2I_CHECK_LAUNCH();
    if (Gt) {
        hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)B), t, 0, st, loss, pair_loss, npairs, (float)C * (float)C);
        L2I_CHECK_LAUNCH();
    }
    return L2I_OK;
}

extern "C" int l2i_gram_bwd_f32(float* g, const float* c, const float* D, const float* scale, float coef, int B, int C, int HW, int accumulate,
                                int scale_stride, void* stream) {
    if (!gram_shape_ok(C)) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_bwd: built for C % 32 == 0, C <= 512");
    if (!g || !c || !D || B <= 0 || HW <= 0) return l2i_set_error(L2I_E_ARG, "gram_bwd: null tensor or non-positive dimension");
    if (scale_stride != 0 && scale_stride != 1) return l2i_set_error(L2I_E_ARG, "gram_bwd: scale_stride is 0 (one scale) or 1 (one per sample)");
    if ((size_t)C * HW * sizeof(float) >= 0xFFFFFFF0ull) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_bwd: one sample's map must stay below 4 GiB");
    if (!al16(D)) return l2i_set_error(L2I_E_ARG, "gram_bwd: D must be 16-byte aligned");
    const int tiles = (HW + gr::BN - 1) / gr::BN;
    const bool wide = (C % 64) == 0;
    const int mblocks = C / (wide ? 64 : 32);
    if (tiles > 65535 || B > 65535) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_bwd: grid too large (HW <= 65535 * 256, B <= 65535)");
    const bool vec = (HW % 4) == 0 && al16(c);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)mblocks, (unsigned)tiles, (unsigned)B), t(256);
    if (wide) {
        if (vec) hipLaunchKernelGGL((gram_bwd_kernel<2, true>), grid, t, 0, st, g, c, D, scale, coef, C, HW, accumulate, scale_stride);
        else hipLaunchKernelGGL((gram_bwd_kernel<2, false>), grid, t, 0, st, g, c, D, scale, coef, C, HW, accumulate, scale_stride);
    } else {
        if (vec) hipLaunchKernelGGL((gram_bwd_kernel<1, true>), grid, t, 0, st, g, c, D, scale, coef, C, HW, accumulate, scale_stride);
        else hipLaunchKernelGGL((gram_bwd_kernel<1, false>), grid, t, 0, st, g, c, D, scale, coef, C, HW, accumulate, scale_stride);
    }
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
