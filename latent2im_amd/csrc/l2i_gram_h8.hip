// l2i_gram_h8.hip — the VGG-16 Gram-matrix term of the inversion loss and its gradient on 16-bit h8 taps [B][C/8][HW][8] (gfx950).  Entry points
// l2i_gram_loss_h8, l2i_gram_bwd_h8 and, compiled with -DL2I_H8_F16, their _f16 twins (include/l2i.h).  Same semantics as l2i_gram.hip: the tap is
// the PRE-ReLU conv output, the ReLU is applied to the fragments (packed integer max: a negative fp16 / bf16 is a negative int16).
//
// Forward.  G = F F^T / (C HW) contracts the PIXEL index, which h8 storage strides (one 16-byte slot of 8 channels per pixel), so both MFMA operands
// need a transpose; ds_read_b64_tr_b16 does it on the way out of LDS.  Block (HW slice, tile pair i <= j, sample), as in the fp32 file:
//   stage    the 4 channel-group planes of tile i (and of tile j when j != i) of a 256-pixel chunk go global -> LDS by DMA in the layout they have
//            in HBM, [plane][pixel][8 channels], planes PS = 4096 + 64 bytes apart.  A lane past the slice reads past the buffer: zeros.
//   read     v_mfma_f32_32x32x16: lane (half, r) holds channel r of the tile at 8 pixels 8 half .. + 7 of the K step, for A (tile i) and for B (tile j)
//            alike.  One transposed read hands each 16-lane group a block of 4 rows (pixels) x 16 columns (channels), lane n of the group
//            receiving column n: lane 4 q + p supplies the address of pixel q, channels 4 p .. + 3, i.e. plane 2 (group & 1) + (p >> 1), byte
//            8 (p & 1) of that pixel's slot.  Two reads (pixels + 0 .. 3, + 4 .. 7) make one fragment.  Every address is 8-byte aligned and all 64
//            lanes are active (256 threads, no divergence around the reads; the tail is zero-filled, not masked).
//   banks    a 32-lane half touches 4 planes x 64 contiguous bytes; PS = 64 (mod 256) puts them on four disjoint sets of 16 banks: conflict-free.
//   sum      the four waves take 64 pixels of the chunk each; their four accumulators are added in wave order into the slice's partial tile,
//            and l2i_gram_common.h's second and third pass (shared with the fp32 file) add the slices in slice order: no floating-point atomics.
// There is no second, scalar path: an h8 slot is 16 bytes whatever HW is, so the DMA path takes every accepted shape (the fp32 file needs one
// for HW % 4 != 0), and a tap off a 16-byte boundary is refused.
//
// Backward.  g (+)= cs * (c > 0) * (D relu(c)), cs = coef * scale[b], contracts the CHANNEL index: lane (half, j)'s B fragment of the 16-channel K
// step is the h8 slot of (group 2 k + half, pixel j) as stored, one 16-byte load, and its A fragment is 8 consecutive floats of a row of D.  D is
// scaled by cs in fp32 BEFORE it is rounded to the element type (|D| is ~1e-3 and would lose its low bits, or underflow in fp16, unscaled; cs
// carries the loss scale).  No LDS: D (<= 1 MiB) stays in L2, and a wave's 12 VALU instructions per A fragment hide under its 2 x 64-cycle MFMAs.
// The epilogue is the h8 one (h8_gather: accumulators -> one slot of 8 channels per lane), masks by the tap's own slot and, with `accumulate`,
// adds the incoming trunk gradient in fp32 before the single rounding of the store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"
#include "l2i_h8_common.h"
#include "l2i_gram_common.h"

namespace H8_NS {

namespace grh {
constexpr int PS = gr::KC * 16 + 64;       // bytes between staged planes
constexpr int BN = 256;                    // backward: pixels per block (4 waves x 2 x 32)
}

typedef short s16x4 __attribute__((ext_vector_type(4)));

// 4 pixels x this lane's channel, transposed out of LDS, ReLU applied: one half of a fragment (two dwords)
__device__ __forceinline__ u32x2 gram_tr_relu(const char* lds) {
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)lds);
    u32x2 u = __builtin_bit_cast(u32x2, v);
    asm("v_pk_max_i16 %0, %0, 0" : "+v"(u.x));
    asm("v_pk_max_i16 %0, %0, 0" : "+v"(u.y));
    return u;
}

__global__ __launch_bounds__(256, 2) void gram_partial_h8_kernel(float* __restrict__ ws, const void* __restrict__ c, int C, int HW, int SL, int nslices, int npairs) {
    using namespace gr;
    using namespace grh;
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [8 or 4 planes][PS]; afterwards four 32x32 fp32 wave tiles
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
    const int slice = blockIdx.x, pair = blockIdx.y, b = blockIdx.z;
    int ti, tj;
    gram_pair(pair, C / 32, ti, tj);
    const bool diag = ti == tj;
    const int npieces = diag ? 16 : 32;                                 // (plane, 64-pixel quarter): one wave DMA each
    const unsigned bytes = (unsigned)((size_t)C * HW * 2);
    const char* cb = reinterpret_cast<const char*>(c) + (size_t)b * bytes;
    const __amdgpu_buffer_rsrc_t rs = l2i_buffer_rsrc(cb, bytes);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int p_begin = slice * SL;
    const int p_end = min(HW, p_begin + SL);
    // this lane's address in a transposed read (header): group = lane / 16, q = pixel of the block, p = channel quad of the block
    const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int tr_off = ((grp & 1) * 2 + (p >> 1)) * PS + (wave * 64 + 8 * (grp >> 1) + q) * 16 + 8 * (p & 1);

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    for (int p0 = p_begin; p0 < p_end; p0 += KC) {
        for (int pc = wave_u; pc < npieces; pc += 4) {
            const int plane = pc >> 2, quarter = pc & 3;
            const int cg = (plane < 4 ? ti * 4 : tj * 4 - 4) + plane;
            const int px = p0 + quarter * 64 + lane;
            const unsigned voff = px < p_end ? (unsigned)(((size_t)cg * HW + px) * 16) : bytes;
            l2i_lds_dma16(voff, rs, __builtin_amdgcn_readfirstlane(l2i_lds_addr(smem + plane * PS + quarter * 1024)), 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* ab = smem + tr_off;
        const char* bb = ab + (diag ? 0 : 4 * PS);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {           // 16 pixels per K step
            const u32x2 a0 = gram_tr_relu(ab + ks * 256), a1 = gram_tr_relu(ab + ks * 256 + 64);
            const u32x2 b0 = gram_tr_relu(bb + ks * 256), b1 = gram_tr_relu(bb + ks * 256 + 64);
            const bf16x8 af = __builtin_bit_cast(bf16x8, (u32x4){a0.x, a0.y, a1.x, a1.y});
            const bf16x8 bf = __builtin_bit_cast(bf16x8, (u32x4){b0.x, b0.y, b1.x, b1.y});
            acc = H8_MFMA(af, bf, acc, 0, 0, 0);
        }
        __syncthreads();                           // the stage is free again
    }
    // the four waves' tiles, added in wave order
    float* tiles = reinterpret_cast<float*>(smem);
    float* wt = tiles + wave * TILE;
#pragma unroll
    for (int e = 0; e < 16; ++e) wt[((e & 3) + 8 * (e >> 2) + 4 * half) * 32 + r] = acc[e];
    __syncthreads();
    float* out = ws + (((size_t)b * npairs + pair) * nslices + slice) * TILE;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int e = tid + 256 * n;
        out[e] = (tiles[e] + tiles[TILE + e]) + (tiles[2 * TILE + e] + tiles[3 * TILE + e]);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------------
// block (M block of 32 WM output channels, 256-pixel tile, sample); wave: 32 WM channels x 64 pixels
template <int WM>
__global__ __launch_bounds__(256, 2) void gram_bwd_h8_kernel(void* __restrict__ g, const void* __restrict__ c, const float* __restrict__ D, const float* __restrict__ scale,
                                                             float coef, int C, int HW, int accumulate, int scale_stride) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, j = lane & 31;
    const int m0 = blockIdx.x * (32 * WM), px0 = blockIdx.y * grh::BN + wave * 64, b = blockIdx.z;
    const u32x4* cb = reinterpret_cast<const u32x4*>(c) + (size_t)b * (C / 8) * HW;      // slots [C/8][HW]
    u32x4* gb = reinterpret_cast<u32x4*>(g) + (size_t)b * (C / 8) * HW;
    const float* Db = D + (size_t)b * C * C;
    const float cs = coef * (scale ? scale[(size_t)b * scale_stride] : 1.f);
    int px[2];
    bool live[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) { px[n] = px0 + n * 32 + j; live[n] = px[n] < HW; }

    f32x16 acc[WM][2];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

    for (int k0 = 0; k0 < C; k0 += 16) {
        bf16x8 af[WM], bf[2];
#pragma unroll
        for (int m = 0; m < WM; ++m) {             // row m0 + 32 m + j of D, columns k0 + 8 half .. + 7: scaled in fp32, then rounded
            const float* dr = Db + (size_t)(m0 + m * 32 + j) * C + k0 + 8 * half;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(dr), hi = *reinterpret_cast<const f32x4*>(dr + 4);
            const u32x4 u = {h8_pk(lo[0] * cs, lo[1] * cs), h8_pk(lo[2] * cs, lo[3] * cs), h8_pk(hi[0] * cs, hi[1] * cs), h8_pk(hi[2] * cs, hi[3] * cs)};
            af[m] = __builtin_bit_cast(bf16x8, u);
        }
#pragma unroll
        for (int n = 0; n < 2; ++n) {              // the slot of (channel group k0 / 8 + half, pixel): a B fragment as stored; the ReLU, on load
            u32x4 raw = {0u, 0u, 0u, 0u};
            if (live[n]) raw = cb[(size_t)(k0 / 8 + half) * HW + px[n]];
            asm("v_pk_max_i16 %0, %0, 0" : "+v"(raw.x)); asm("v_pk_max_i16 %0, %0, 0" : "+v"(raw.y));
            asm("v_pk_max_i16 %0, %0, 0" : "+v"(raw.z)); asm("v_pk_max_i16 %0, %0, 0" : "+v"(raw.w));
            bf[n] = __builtin_bit_cast(bf16x8, raw);
        }
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = H8_MFMA(af[m], bf[n], acc[m][n], 0, 0, 0);
    }
    // ---- epilogue: lane (half, j) finishes the slot of channel group (m0 + 32 m) / 8 + 2 pr + half at pixel j of tile n.  The exchange crosses the
    // lane halves, so every lane runs it; only the loads and the store are guarded.
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                float v[8];
                h8_gather(acc[m][n], pr, half, v);
                if (!live[n]) continue;
                const size_t slot = (size_t)((m0 + m * 32) / 8 + 2 * pr + half) * HW + px[n];
                float cv[8];
                h8_unpack(cb[slot], cv);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = cv[e] > 0.f ? v[e] : 0.f;
                if (accumulate) {
                    float gv[8];
                    h8_unpack(gb[slot], gv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += gv[e];
                }
                gb[slot] = h8_pack(v);
            }
}

static bool gram_shape_ok(int C) { return C > 0 && (C % 32) == 0 && C <= 512; }
static bool al16(const void* q) { return (((uintptr_t)q) % 16) == 0; }

}  // namespace H8_NS

extern "C" int H8_NAME(l2i_gram_loss_h8)(float* G, float* D, float* loss, const void* c, const float* Gt, float* ws, int B, int C, int HW, int nslices,
                                         void* stream) {
    using namespace H8_NS;
    if (!gram_shape_ok(C)) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_loss_h8: built for C % 32 == 0, C <= 512");
    if (!G || !c || !ws || B <= 0 || HW <= 0 || nslices <= 0) return l2i_set_error(L2I_E_ARG, "gram_loss_h8: null tensor or non-positive dimension");
    if (Gt && (!D || !loss)) return l2i_set_error(L2I_E_ARG, "gram_loss_h8: a target needs D and loss");
    if (!al16(c)) return l2i_set_error(L2I_E_ARG, "gram_loss_h8: c must be 16-byte aligned");
    if ((size_t)C * HW * 2 >= 0xFFFFFFF0ull) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_loss_h8: one sample's map must stay below 4 GiB");
    if (nslices > (HW + gr::KC - 1) / gr::KC) return l2i_set_error(L2I_E_ARG, "gram_loss_h8: more slices than 256-pixel chunks");
    if (B > 65535) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_loss_h8: B <= 65535");
    const int T = C / 32, npairs = T * (T + 1) / 2;
    const int per = (HW + nslices - 1) / nslices;
    const int SL = (per + gr::KC - 1) / gr::KC * gr::KC;               // whole chunks per slice; trailing slices may be empty (they write zeros)
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)8 * grh::PS;
    const dim3 t(256);
    hipLaunchKernelGGL(gram_partial_h8_kernel, dim3((unsigned)nslices, (unsigned)npairs, (unsigned)B), t, lds, st, ws, c, C, HW, SL, nslices, npairs);
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

extern "C" int H8_NAME(l2i_gram_bwd_h8)(void* g, const void* c, const float* D, const float* scale, float coef, int B, int C, int HW, int accumulate,
                                        int scale_stride, void* stream) {
    using namespace H8_NS;
    if (!gram_shape_ok(C)) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_bwd_h8: built for C % 32 == 0, C <= 512");
    if (!g || !c || !D || B <= 0 || HW <= 0) return l2i_set_error(L2I_E_ARG, "gram_bwd_h8: null tensor or non-positive dimension");
    if (scale_stride != 0 && scale_stride != 1) return l2i_set_error(L2I_E_ARG, "gram_bwd_h8: scale_stride is 0 (one scale) or 1 (one per sample)");
    if (!al16(g) || !al16(c) || !al16(D)) return l2i_set_error(L2I_E_ARG, "gram_bwd_h8: g, c and D must be 16-byte aligned");
    if ((size_t)C * HW * 2 >= 0xFFFFFFF0ull) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_bwd_h8: one sample's map must stay below 4 GiB");
    const int tiles = (HW + grh::BN - 1) / grh::BN;
    const bool wide = (C % 64) == 0;
    if (tiles > 65535 || B > 65535) return l2i_set_error(L2I_E_UNSUPPORTED, "gram_bwd_h8: grid too large (HW <= 65535 * 256, B <= 65535)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(C / (wide ? 64 : 32)), (unsigned)tiles, (unsigned)B), t(256);
    if (wide) hipLaunchKernelGGL(gram_bwd_h8_kernel<2>, grid, t, 0, st, g, c, D, scale, coef, C, HW, accumulate, scale_stride);
    else hipLaunchKernelGGL(gram_bwd_h8_kernel<1>, grid, t, 0, st, g, c, D, scale, coef, C, HW, accumulate, scale_stride);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
