// l2i_train_h8.hip — what TRAINING a conv net needs on 16-bit h8 maps [B][C/8][H][W][8] (gfx950): the weight gradient of a convolution and
// training-mode BatchNorm.  Entry points l2i_conv2d_wgrad_h8, l2i_conv2d_wgrad_ws_h8, l2i_bn_stats_h8, l2i_bn_apply_h8, l2i_bn_bwd_reduce_h8,
// l2i_bn_bwd_apply_h8, l2i_bn_ws_h8, l2i_conv2d_wgrad_img_h8, l2i_conv2d_wgrad_img_ws_h8, l2i_repack_planes_h8 and, compiled with -DL2I_H8_F16, their _f16 twins (include/l2i.h).  The fp32 relatives are in l2i_train.hip;
// l2i_bn_finalize_f32 / l2i_bn_bwd_finalize_f32 of that file do the [C]-sized algebra for both.  No floating-point atomics anywhere: every sum has
// a fixed order, equal inputs give equal bits; nothing is allocated, the caller passes the workspaces (sizes: the two host-only *_ws_h8 queries).
//
// Weight gradient.  dw[co,ci,ky,kx] = out_scale * sum_{b,oy,ox} gy[b,co,oy,ox] * x[b,ci,oy*s+ky-p,ox*s+kx-p] is, per tap, a GEMM with M = Cout and
// N = Cin that contracts the PIXEL index, which h8 storage strides: l2i_gram_h8.hip's forward problem with two different maps.  As there:
//   stage    a chunk is 256 consecutive OUTPUT pixels q = (b * OH + oy) * OW + ox of the whole batch.  Wave w owns pixels 64 w .. + 63 of the chunk; its
//            lane computes (b, oy, ox) once per chunk (two integer divisions) and from them the byte offset of its gy slot and of the x slot the tap
//            pairs it with.  8 channel-group planes of gy (64 output channels) and 8 of x (64 input channels) go global -> LDS by DMA, one 16-byte
//            slot per lane, [plane][pixel][8 channels], planes PS = 4096 + 64 bytes apart.  A pixel past the slice, a tap that lands in the padding
//            and a plane past C / 8 (C % 64 == 32) get an offset past the buffer: the DMA writes zeros, so they contribute nothing.
//   read     ds_read_b64_tr_b16 transposes on the way out of LDS into v_mfma_f32_32x32x16 fragments exactly as the Gram kernel's reads do (same lane
//            -> address map, same conflict-free plane pitch).  A wave reads only the 64 pixels it staged: 4 K steps x (2 A + 2 B fragments) feed
//            4 x 4 MFMAs into a 64 x 64 (co, ci) accumulator tile.
//   sum      the four waves' tiles are added in wave order into the slice's partial tile in the workspace; wgrad_reduce_h8_kernel adds the slices in
//            slice order, multiplies by out_scale (a host float times an optional device float) and OVERWRITES dw in [Cout][Cin][K][K] order.
// Grid (slice, 64 x 64 tile, tap).  The slice count (wgrad_plan) aims at about 1024 blocks — two resident per CU on 256 CUs, twice over — whatever
// the shape: 256 slices of 2 chunks for layer1's 64 -> 256 1x1 (4 tiles, 131072 pixels at batch 32), 2 slices of 4 chunks for layer4's 3x3 (64 tiles
// x 9 taps).  Measured per shape: profiles/regressor_train16_bench.txt.
//
// BatchNorm.  A lane owns one 16-byte slot (8 channels of one pixel), a block one channel group; the grid's other dimensions are pixel blocks and,
// for the two apply kernels, the sample: no index is ever divided.  The two reductions sum in float64 per lane, then lanes, waves (fixed tree) and
// write one row of 16 partials per block; bn_finish_h8_kernel adds the rows in block order into the [C] sums l2i_bn_finalize_f32 reads.
//
// Stem weight gradient (l2i_conv2d_wgrad_img_h8, l2i_conv2d_wgrad_img_ws_h8).  conv1 of the regressor reads the fp32 IMAGE, so its gradient
// dw[co][ci][ky][kx] = sum_{b,oy,ox} gy[b,co,oy,ox] * x[b,ci,2 oy+ky-3,2 ox+kx-3] pairs an h8 map with fp32 NCHW: a 64 x 147 GEMM over the pixels with
// x taken as the fp32 value it is.  v_mfma_f32_32x32x2_f32 multiplies fp32 exactly and accumulates like an fmaf chain; gy is converted on load (exact).
//   slice    (sample, range of output rows, block of 128 output columns): one block.  It walks its rows in tiles of 4: the image strip a tile needs,
//            3 x 13 x 261 fp32 zero-padded, is staged once in LDS (40.7 KB) and every tap of every pixel reads it from there; gy goes through LDS one
//            output row at a time (8 channel-group planes of 128 slots, 16.6 KB, planes 32 bytes apart in bank so that the 2-byte reads do not collide).
//   product  a wave owns every fourth PAIR of pixels of the row; the lane halves are the two pixels (K = 2).  A = gy[co = 32 m + lane % 32], B = the
//            image at tap n = 32 t + lane % 32 (n = ci * 49 + ky * 7 + kx; n >= 147 and pixels past the row feed zeros): 2 x 5 MFMAs into ten 32 x 32
//            accumulators, 160 registers, 57.6 KB of LDS: two blocks per CU, no scratch.
//   sum      the four waves' tiles are added in wave order in LDS into the slice's [64][160] tile of the workspace; wgrad_img_reduce_kernel adds the
//            slices in slice order and OVERWRITES dw.  The slice count (wgrad_img_plan) aims at 512 blocks, two per CU.
//
// Weight planes (l2i_repack_planes_h8).  Every 16-bit plane set of a net that is being trained, rewritten IN PLACE from the fp32 master weights by
// one launch: a device table of segments (destination, weight, sizes, mode, contraction padding, first block), one lane per 16-byte slot, every slot
// of a destination written (padding = zeros), conversions = the packing convert of the path (round to nearest even, subnormals kept, overflow to inf).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"
#include "l2i_h8_common.h"

namespace H8_NS {

namespace wg {
constexpr int KC = 256;                    // output pixels per chunk (4 waves x 64)
constexpr int PS = KC * 16 + 64;           // bytes between staged planes
constexpr int TM = 64;                     // tile edge: 8 planes of gy x 8 planes of x
constexpr int TILE = TM * TM;
constexpr int TARGET_BLOCKS = 1024;
}

typedef short wg_s16x4 __attribute__((ext_vector_type(4)));

// 4 pixels x this lane's channel, transposed out of LDS: one half of a fragment (two dwords)
__device__ __forceinline__ u32x2 wg_tr(const char* lds) {
    const wg_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) wg_s16x4*)lds);
    return __builtin_bit_cast(u32x2, v);
}
__device__ __forceinline__ bf16x8 wg_frag(const char* lds) {
    const u32x2 a = wg_tr(lds), b = wg_tr(lds + 64);
    return __builtin_bit_cast(bf16x8, (u32x4){a.x, a.y, b.x, b.y});
}

struct WgradH8 {
    const void* x; const void* gy; float* ws;
    int Cin, H, W, Cout, OH, OW, K, stride, pad;
    int NP, ntn, nslices, chunks_per;
    unsigned xbytes, ybytes;
};

__global__ __launch_bounds__(256, 2) void wgrad_partial_h8_kernel(const WgradH8 p) {
    using namespace wg;
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [8 gy planes + 8 x planes][PS]; afterwards four 64x64 fp32 wave tiles
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
    const int slice = blockIdx.x, tile = blockIdx.y, tap = blockIdx.z;
    const int mt = tile / p.ntn, nt = tile - mt * p.ntn;
    const int ky = tap / p.K, kx = tap - ky * p.K;
    const __amdgpu_buffer_rsrc_t rs_y = l2i_buffer_rsrc(p.gy, p.ybytes), rs_x = l2i_buffer_rsrc(p.x, p.xbytes);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int p_begin = slice * p.chunks_per * KC;
    const int p_end = min(p.NP, p_begin + p.chunks_per * KC);
    const int OHW = p.OH * p.OW, cgo = p.Cout / 8, cgi = p.Cin / 8;
    // this lane's address in a transposed read (l2i_gram_h8.hip): group = lane / 16, q = pixel of the block, c = channel quad of the block
    const int grp = lane >> 4, tq = (lane >> 2) & 3, tc = lane & 3;
    const int tr_off = ((grp & 1) * 2 + (tc >> 1)) * PS + (wave * 64 + 8 * (grp >> 1) + tq) * 16 + 8 * (tc & 1);

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

    for (int p0 = p_begin; p0 < p_end; p0 += KC) {
        const int q = p0 + wave * 64 + lane;
        const bool live = q < p_end;
        const int b = q / OHW, rem = q - b * OHW;
        const int oy = rem / p.OW, ox = rem - oy * p.OW;
        const int iy = oy * p.stride + ky - p.pad, ix = ox * p.stride + kx - p.pad;
        const bool xin = live && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        const unsigned lds0 = l2i_lds_addr(smem + wave_u * 1024);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cg = mt * 8 + k;
            const unsigned voff = (live && cg < cgo) ? (unsigned)((((size_t)b * cgo + cg) * OHW + rem) * 16) : p.ybytes;
            l2i_lds_dma16(voff, rs_y, __builtin_amdgcn_readfirstlane(lds0 + k * PS), 0u);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cg = nt * 8 + k;
            const unsigned voff = (xin && cg < cgi) ? (unsigned)(((((size_t)b * cgi + cg) * p.H + iy) * p.W + ix) * 16) : p.xbytes;
            l2i_lds_dma16(voff, rs_x, __builtin_amdgcn_readfirstlane(lds0 + (8 + k) * PS), 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* ab = smem + tr_off;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {           // 16 pixels per K step
            bf16x8 af[2], bf[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) af[m] = wg_frag(ab + m * 4 * PS + ks * 256);
#pragma unroll
            for (int n = 0; n < 2; ++n) bf[n] = wg_frag(ab + (8 + n * 4) * PS + ks * 256);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = H8_MFMA(af[m], bf[n], acc[m][n], 0, 0, 0);
        }
        __syncthreads();                           // the stage is free again
    }
    // the four waves' tiles, added in wave order.  D[i][j]: lane column j = input channel, register e -> output channel (e & 3) + 8 (e >> 2) + 4 half
    float* tiles = reinterpret_cast<float*>(smem);
    float* wt = tiles + wave * TILE;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) wt[(m * 32 + (e & 3) + 8 * (e >> 2) + 4 * half) * TM + n * 32 + r] = acc[m][n][e];
    __syncthreads();
    float* out = p.ws + (((size_t)tile * gridDim.z + tap) * p.nslices + slice) * TILE;
#pragma unroll
    for (int n = 0; n < TILE / 256; ++n) {
        const int e = tid + 256 * n;
        out[e] = (tiles[e] + tiles[TILE + e]) + (tiles[2 * TILE + e] + tiles[3 * TILE + e]);
    }
}

// one thread per element of a partial tile: the slices in slice order, the scale, the [Cout][Cin][K][K] store
__global__ __launch_bounds__(256) void wgrad_reduce_h8_kernel(float* __restrict__ dw, const float* __restrict__ ws, float out_scale, const float* __restrict__ out_scale_dev,
                                                              int Cin, int Cout, int K, int ntn, int nslices, unsigned total) {
    using namespace wg;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int taps = K * K;
    const unsigned tt = idx / TILE, e = idx - tt * TILE;
    const int tile = tt / taps, tap = tt - tile * taps;
    const int mt = tile / ntn, nt = tile - mt * ntn;
    const int co = mt * TM + (int)(e / TM), ci = nt * TM + (int)(e % TM);
    if (co >= Cout || ci >= Cin) return;
    const float* src = ws + (size_t)tt * nslices * TILE + e;
    float s = 0.f;
    for (int sl = 0; sl < nslices; ++sl) s += src[(size_t)sl * TILE];
    const float sc = out_scale_dev ? out_scale * out_scale_dev[0] : out_scale;
    dw[((size_t)co * Cin + ci) * taps + tap] = s * sc;
}

struct WgradPlan { int tiles, ntn, taps, nchunks, nslices, chunks_per; int64_t ws_bytes; };

// shape checks shared by the entry and the workspace query; nullptr = accepted
static const char* wgrad_plan(WgradPlan& pl, int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return "non-positive dimension";
    if (K != 1 && K != 3) return "built for K = 1 and K = 3 (the 7x7 stem goes through l2i_conv2d_wgrad_f32)";
    if (stride != 1 && stride != 2) return "built for stride 1 and 2";
    if (pad != 0 && pad != 1) return "built for pad 0 and 1";
    if ((Cin % 32) != 0 || (Cout % 32) != 0) return "built for Cin % 32 == 0 and Cout % 32 == 0";
    if ((H + 2 * pad - K) / stride + 1 != OH || (W + 2 * pad - K) / stride + 1 != OW || H + 2 * pad < K || W + 2 * pad < K) return "OH / OW are not the conv's output size";
    if ((size_t)B * Cin * H * W * 2 >= 0xFFFFFFF0ull || (size_t)B * Cout * OH * OW * 2 >= 0xFFFFFFF0ull) return "x and gy must stay below 4 GiB each";
    const long np = (long)B * OH * OW;
    pl.ntn = (Cin + wg::TM - 1) / wg::TM;
    pl.tiles = (Cout + wg::TM - 1) / wg::TM * pl.ntn;
    pl.taps = K * K;
    if (pl.tiles > 65535) return "more than 65535 tiles";
    pl.nchunks = (int)((np + wg::KC - 1) / wg::KC);
    const int per_slice0 = pl.tiles * pl.taps;
    int want = (wg::TARGET_BLOCKS + per_slice0 - 1) / per_slice0;
    if (want > pl.nchunks) want = pl.nchunks;
    pl.chunks_per = (pl.nchunks + want - 1) / want;
    pl.nslices = (pl.nchunks + pl.chunks_per - 1) / pl.chunks_per;          // no empty slice
    pl.ws_bytes = (int64_t)pl.tiles * pl.taps * pl.nslices * wg::TILE * 4;
    if ((int64_t)pl.tiles * pl.taps * wg::TILE >= 0x7FFFFFFFll) return "dw too large";
    return nullptr;
}

// ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------------------
constexpr int BN_MAXBLK = 64;
static int bn_nblk(int B, int64_t HW) {
    int64_t per = (HW + 255) / 256, chunks = ((int64_t)B * HW + 256 * 8 - 1) / (256 * 8);
    int64_t n = chunks < per ? chunks : per;
    if (n > BN_MAXBLK) n = BN_MAXBLK;
    return n < 1 ? 1 : (int)n;
}

// 16 per-lane float64 sums -> one row of the workspace per block (lanes, then waves, in a fixed tree)
__device__ __forceinline__ void bn_block_row(double (&s)[16], double* __restrict__ row) {
    __shared__ double sh[4][16];
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = wave_sum(s[e]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sh[threadIdx.x >> 6][e] = s[e];
    }
    __syncthreads();
    if (threadIdx.x < 16) row[threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// grid (C / 8, nblk): block (group, pixel block) sums its pixels of every sample
__global__ __launch_bounds__(256) void bn_stats_h8_kernel(double* __restrict__ ws, const u32x4* __restrict__ x, int B, int CG, long long HW) {
    const int cg = blockIdx.x;
    double s[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.0;
    for (int b = 0; b < B; ++b) {
        const u32x4* xb = x + ((size_t)b * CG + cg) * HW;
        for (long long pix = (long long)blockIdx.y * 256 + threadIdx.x; pix < HW; pix += (long long)gridDim.y * 256) {
            float v[8];
            h8_unpack(xb[pix], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) { const double d = v[e]; s[e] += d; s[8 + e] += d * d; }
        }
    }
    bn_block_row(s, ws + ((size_t)cg * gridDim.y + blockIdx.y) * 16);
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_h8_kernel(double* __restrict__ ws, const u32x4* __restrict__ gy, const u32x4* __restrict__ out,
                                                               const u32x4* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               int B, int CG, long long HW) {
    const int cg = blockIdx.x;
    float mu[8], is[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = mean[cg * 8 + e]; is[e] = invstd[cg * 8 + e]; }
    double s[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.0;
    for (int b = 0; b < B; ++b) {
        const size_t base = ((size_t)b * CG + cg) * HW;
        for (long long pix = (long long)blockIdx.y * 256 + threadIdx.x; pix < HW; pix += (long long)gridDim.y * 256) {
            float dy[8], xv[8];
            h8_unpack(gy[base + pix], dy);
            h8_unpack(x[base + pix], xv);
            if (out) {
                float ov[8];
                h8_unpack(out[base + pix], ov);
#pragma unroll
                for (int e = 0; e < 8; ++e) dy[e] = ov[e] > 0.f ? dy[e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) { s[e] += (double)dy[e]; s[8 + e] += (double)dy[e] * (double)((xv[e] - mu[e]) * is[e]); }
        }
    }
    bn_block_row(s, ws + ((size_t)cg * gridDim.y + blockIdx.y) * 16);
}

// the rows of a channel group in block order -> the two [C] sums
__global__ __launch_bounds__(256) void bn_finish_h8_kernel(double* __restrict__ s0, double* __restrict__ s1, const double* __restrict__ ws, int C, int nblk) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double* row = ws + (size_t)(c >> 3) * nblk * 16 + (c & 7);
    double a = 0.0, q = 0.0;
    for (int k = 0; k < nblk; ++k) { a += row[(size_t)k * 16]; q += row[(size_t)k * 16 + 8]; }
    s0[c] = a; s1[c] = q;
}

// grid (pixel blocks, C / 8, B)
__global__ __launch_bounds__(256) void bn_apply_h8_kernel(u32x4* __restrict__ y, const u32x4* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const u32x4* __restrict__ residual, int relu, long long HW) {
    const int cg = blockIdx.y;
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = scale[cg * 8 + e]; sh[e] = shift[cg * 8 + e]; }
    const size_t base = ((size_t)blockIdx.z * gridDim.y + cg) * HW;
    for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < HW; pix += (long long)gridDim.x * 256) {
        float v[8];
        h8_unpack(x[base + pix], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] * sc[e] + sh[e];
        if (residual) {
            float rv[8];
            h8_unpack(residual[base + pix], rv);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += rv[e];
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        y[base + pix] = h8_pack(v);
    }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_h8_kernel(u32x4* __restrict__ dx, u32x4* __restrict__ dy_masked, const u32x4* __restrict__ gy,
                                                              const u32x4* __restrict__ out, const u32x4* __restrict__ x, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                              const float* __restrict__ m_dy, const float* __restrict__ m_dyxh, long long HW) {
    const int cg = blockIdx.y;
    float mu[8], is[8], gi[8], md[8], mx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = cg * 8 + e;
        mu[e] = mean[c]; is[e] = invstd[c]; gi[e] = gamma[c] * invstd[c]; md[e] = m_dy[c]; mx[e] = m_dyxh[c];
    }
    const size_t base = ((size_t)blockIdx.z * gridDim.y + cg) * HW;
    for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < HW; pix += (long long)gridDim.x * 256) {
        float dy[8], xv[8], v[8];
        h8_unpack(gy[base + pix], dy);
        h8_unpack(x[base + pix], xv);
        if (out) {
            float ov[8];
            h8_unpack(out[base + pix], ov);
#pragma unroll
            for (int e = 0; e < 8; ++e) dy[e] = ov[e] > 0.f ? dy[e] : 0.f;
        }
        if (dy_masked) dy_masked[base + pix] = h8_pack(dy);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xh = (xv[e] - mu[e]) * is[e];
            v[e] = gi[e] * (dy[e] - md[e] - xh * mx[e]);
        }
        dx[base + pix] = h8_pack(v);
    }
}

// ---- the stem's weight gradient: fp32 image x h8 gradient map ------------------------------------------------------------------------------------------
namespace wi {
constexpr int R = 4;                       // output rows per staged image tile
constexpr int CW = 128;                    // output columns per slice
constexpr int XH = 2 * R + 5;              // image rows of a tile
constexpr int XP = 2 * CW + 5;             // image columns of a tile = the row pitch in floats (odd: taps of neighbouring rows fall in different banks)
constexpr int NT = 147;                    // 3 x 7 x 7 taps
constexpr int NTP = 160;                   // ... in five MFMA tiles
constexpr int CO = 64;
constexpr int TILE = CO * NTP;             // floats of a slice's partial tile
constexpr int GP = CW * 16 + 32;           // bytes between the staged channel-group planes of gy
constexpr int G_OFF = TILE * 4;            // the image tile (3 * XH * XP * 4 = 40716 bytes), afterwards the partial tile, lie in front of gy
constexpr int LDS = G_OFF + 8 * GP;
constexpr int TARGET_BLOCKS = 512;
static_assert(3 * XH * XP * 4 <= G_OFF, "the image tile must fit in front of the gy planes");
}

struct WgradImg {
    const float* x; const void* gy; float* ws;
    int H, W, OH, OW, ncb, nrs, rows_per;
};

__global__ __launch_bounds__(256, 2) void wgrad_img_partial_kernel(const WgradImg p) {
    using namespace wi;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xs = reinterpret_cast<float*>(smem);
    char* gs = smem + G_OFF;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
    int s = blockIdx.x;
    const int cb = s % p.ncb;
    s /= p.ncb;
    const int rs = s % p.nrs, b = s / p.nrs;
    const int ox0 = cb * CW, cw = min(CW, p.OW - ox0);
    const int oy_begin = rs * p.rows_per, oy_end = min(p.OH, oy_begin + p.rows_per);
    int toff[5];
    bool tlive[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int n = 32 * t + r;
        tlive[t] = n < NT;
        const int ci = n / 49, rem = n - ci * 49, ky = rem / 7, kx = rem - ky * 7;
        toff[t] = tlive[t] ? (ci * XH + ky) * XP + kx : 0;
    }
    f32x16 acc[2][5];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][t][e] = 0.f;
    const u32x4* gyp = reinterpret_cast<const u32x4*>(p.gy);

    for (int ty = oy_begin; ty < oy_end; ty += R) {
        const int nr = min(R, oy_end - ty);
        const int iy0 = 2 * ty - 3, ix0 = 2 * ox0 - 3, nrow = 2 * nr + 5, ncol = 2 * cw + 5;
        __syncthreads();                           // the previous tile has been read
        for (int row = wave; row < 3 * nrow; row += 4) {
            const int c = row / nrow, rr = row - c * nrow, iy = iy0 + rr;
            const bool yin = iy >= 0 && iy < p.H;
            const float* src = p.x + (((size_t)b * 3 + c) * p.H + (yin ? iy : 0)) * p.W;
            float* dst = xs + (c * XH + rr) * XP;
            for (int cc = lane; cc < ncol; cc += 64) {
                const int ix = ix0 + cc;
                dst[cc] = (yin && ix >= 0 && ix < p.W) ? src[ix] : 0.f;
            }
        }
        for (int ry = 0; ry < nr; ++ry) {
            if (ry) __syncthreads();               // the previous row of gy has been read
            const size_t grow = (size_t)(ty + ry) * p.OW + ox0;
#pragma unroll
            for (int i = 0; i < 8 * CW / 256; ++i) {
                const int sl = tid + 256 * i, cg = sl / CW, ox = sl - cg * CW;
                if (ox < cw) *reinterpret_cast<u32x4*>(gs + cg * GP + ox * 16) = gyp[((size_t)b * 8 + cg) * p.OH * p.OW + grow + ox];
            }
            __syncthreads();
            const float* xrow = xs + 2 * ry * XP;
            for (int pp = wave; 2 * pp < cw; pp += 4) {
                const int px = 2 * pp + half;
                const bool live = px < cw;
                const int pxs = live ? px : 0;
                float a[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int co = 32 * m + r;
                    const unsigned h = *reinterpret_cast<const unsigned short*>(gs + (co >> 3) * GP + pxs * 16 + (co & 7) * 2);
                    a[m] = live ? h8_lo(h) : 0.f;
                }
                const float* xb = xrow + 2 * pxs;
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const float xv = xb[toff[t]];
                    const float bv = (live && tlive[t]) ? xv : 0.f;
#pragma unroll
                    for (int m = 0; m < 2; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bv, acc[m][t], 0, 0, 0);
                }
            }
        }
    }
    // the four waves' tiles in wave order.  D[i][j]: lane column j = tap, register e -> output channel (e & 3) + 8 (e >> 2) + 4 half
    __syncthreads();
    float* tile = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int t = 0; t < 5; ++t)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        float* q = tile + (32 * m + (e & 3) + 8 * (e >> 2) + 4 * half) * NTP + 32 * t + r;
                        *q = w ? *q + acc[m][t][e] : acc[m][t][e];
                    }
        }
        __syncthreads();
    }
    float* out = p.ws + (size_t)blockIdx.x * TILE;
    for (int i = tid; i < TILE; i += 256) out[i] = tile[i];
}

// one thread per element of dw: the slices in slice order
__global__ __launch_bounds__(256) void wgrad_img_reduce_kernel(float* __restrict__ dw, const float* __restrict__ ws, int nslices) {
    using namespace wi;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= CO * NT) return;
    const int co = idx / NT, n = idx - co * NT;
    const float* src = ws + co * NTP + n;
    float s = 0.f;
#pragma unroll 8
    for (int sl = 0; sl < nslices; ++sl) s += src[(size_t)sl * TILE];
    dw[idx] = s;
}

struct WgradImgPlan { int ncb, nrs, rows_per, nslices; int64_t ws_bytes; };

// shape checks shared by the entry and the workspace query; nullptr = accepted
static const char* wgrad_img_plan(WgradImgPlan& pl, int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return "non-positive dimension";
    if (Cin != 3 || Cout != 64) return "built for the stem: Cin == 3 and Cout == 64";
    if (K != 7 || stride != 2 || pad != 3) return "built for the stem: 7x7, stride 2, pad 3";
    if ((H - 1) / 2 + 1 != OH || (W - 1) / 2 + 1 != OW) return "OH / OW are not the conv's output size";
    if ((size_t)B * 3 * H * W * 4 >= 0xFFFFFFF0ull || (size_t)B * 64 * OH * OW * 2 >= 0xFFFFFFF0ull) return "x and gy must stay below 4 GiB each";
    pl.ncb = (OW + wi::CW - 1) / wi::CW;
    const int tiles = (OH + wi::R - 1) / wi::R;                            // row tiles of a sample
    const long per = (long)B * pl.ncb;
    long want = wi::TARGET_BLOCKS / per;                                  // row slices of a sample
    if (want < 1) want = 1;
    if (want > tiles) want = tiles;
    const int tiles_per = (int)((tiles + want - 1) / want);
    pl.rows_per = tiles_per * wi::R;
    pl.nrs = (OH + pl.rows_per - 1) / pl.rows_per;                        // no empty slice
    const long long ns = (long long)per * pl.nrs;
    if (ns > 0x7FFFFFFFll) return "more than 2^31 slices";
    pl.nslices = (int)ns;
    pl.ws_bytes = (int64_t)ns * wi::TILE * 4;
    return nullptr;
}

// ---- weight planes of a net in one launch --------------------------------------------------------------------------------------------------------
// a row of the device table: eight int64
struct PlaneSeg { long long dst, src, Cout, Cin, K, mode, qpad, first; };

__global__ __launch_bounds__(256) void repack_planes_kernel(const PlaneSeg* __restrict__ table, int nseg, int nblocks) {
    int sg = 0;
    while (sg + 1 < nseg && (long long)blockIdx.x >= table[sg + 1].first) ++sg;
    const PlaneSeg t = table[sg];
    const long long nb = (sg + 1 < nseg ? table[sg + 1].first : (long long)nblocks) - t.first;
    const int Cout = (int)t.Cout, Cin = (int)t.Cin, K = (int)t.K, mode = (int)t.mode, qpad = (int)t.qpad, KK = K * K;
    // rows = the slot index of a plane, contr = the contraction index (16 per group); mode 3: contr counts (channel, ky) rows of 8 elements
    const int rows = (mode == 0 || mode == 3) ? Cout : Cin;
    const int contr = mode == 0 ? Cin : mode == 3 ? Cin * K : Cout;
    const int groups = mode == 3 ? (contr + 1) / 2 : (contr + qpad - 1) / qpad * qpad / 16;
    const int taps = mode == 3 ? 1 : KK;
    const int rowsP = (rows + 31) / 32 * 32;
    const long long total = (long long)groups * taps * 2 * rowsP;
    const float* __restrict__ w = reinterpret_cast<const float*>(t.src);
    u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(t.dst);
    for (long long i = ((long long)blockIdx.x - t.first) * 256 + threadIdx.x; i < total; i += nb * 256) {
        const int row = (int)(i % rowsP);
        long long q = i / rowsP;
        const int half = (int)(q & 1);
        q >>= 1;
        const int tp = (int)(q % taps), g = (int)(q / taps);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        if (row < rows) {
            if (mode == 3) {
                const int j = 2 * g + half;
                if (j < contr) {
                    const float* src = w + ((size_t)row * Cin * K + j) * K;          // w[row][c][ky][.], (c, ky) = divmod(j, K)
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e < K) v[e] = src[e];
                }
            } else {
                const int tt = mode == 2 ? KK - 1 - tp : tp;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = 16 * g + 8 * half + e;
                    if (k < contr) v[e] = mode == 0 ? w[((size_t)row * Cin + k) * KK + tt] : w[((size_t)k * Cin + row) * KK + tt];
                }
            }
        }
        dst[i] = h8_pack(v);
    }
}

static bool al16(const void* q) { return (((uintptr_t)q) % 16) == 0; }
// nullptr = accepted
static const char* bn_shape(int B, int C, int64_t HW) {
    if (B <= 0 || C <= 0 || HW <= 0) return "non-positive dimension";
    if ((C % 8) != 0) return "C % 8 == 0 (an h8 slot holds 8 channels)";
    if (B > 65535 || C / 8 > 65535) return "B <= 65535 and C <= 8 * 65535";
    if (HW > (1ll << 31)) return "HW <= 2^31";
    return nullptr;
}
static unsigned bn_pixel_blocks(int64_t HW) {
    const int64_t n = (HW + 255) / 256;
    return (unsigned)(n > 4096 ? 4096 : n);
}

}  // namespace H8_NS

extern "C" int H8_NAME(l2i_conv2d_wgrad_ws_h8)(int64_t* bytes, int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad) {
    using namespace H8_NS;
    if (!bytes) return l2i_set_error(L2I_E_ARG, "conv2d_wgrad_ws_h8: null bytes");
    WgradPlan pl;
    if (const char* why = wgrad_plan(pl, B, Cin, H, W, Cout, OH, OW, K, stride, pad)) {
        *bytes = 0;
        return l2i_set_error(L2I_E_UNSUPPORTED, why);
    }
    *bytes = pl.ws_bytes;
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_conv2d_wgrad_h8)(float* dw, const void* x, const void* gy, float* ws, int64_t ws_bytes, float out_scale, const float* out_scale_dev,
                                            int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad, void* stream) {
    using namespace H8_NS;
    WgradPlan pl;
    if (const char* why = wgrad_plan(pl, B, Cin, H, W, Cout, OH, OW, K, stride, pad)) return l2i_set_error(L2I_E_UNSUPPORTED, why);
    if (!dw || !x || !gy) return l2i_set_error(L2I_E_ARG, "conv2d_wgrad_h8: null tensor");
    if (!ws) return l2i_set_error(L2I_E_UNSUPPORTED, "conv2d_wgrad_h8: null workspace (size: l2i_conv2d_wgrad_ws_h8)");
    if (ws_bytes < pl.ws_bytes) return l2i_set_error(L2I_E_UNSUPPORTED, "conv2d_wgrad_h8: workspace smaller than l2i_conv2d_wgrad_ws_h8 asks for");
    if (!al16(x) || !al16(gy) || !al16(ws)) return l2i_set_error(L2I_E_ARG, "conv2d_wgrad_h8: x, gy and ws must be 16-byte aligned");
    WgradH8 p;
    p.x = x; p.gy = gy; p.ws = ws; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.OH = OH; p.OW = OW; p.K = K; p.stride = stride; p.pad = pad;
    p.NP = B * OH * OW; p.ntn = pl.ntn; p.nslices = pl.nslices; p.chunks_per = pl.chunks_per;
    p.xbytes = (unsigned)((size_t)B * Cin * H * W * 2); p.ybytes = (unsigned)((size_t)B * Cout * OH * OW * 2);
    hipStream_t st = (hipStream_t)stream;
    const int lds = 16 * wg::PS;
    L2I_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_partial_h8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(wgrad_partial_h8_kernel, dim3((unsigned)pl.nslices, (unsigned)pl.tiles, (unsigned)pl.taps), dim3(256), (size_t)lds, st, p);
    L2I_CHECK_LAUNCH();
    const unsigned total = (unsigned)pl.tiles * pl.taps * wg::TILE;
    hipLaunchKernelGGL(wgrad_reduce_h8_kernel, dim3((total + 255) / 256), dim3(256), 0, st, dw, ws, out_scale, out_scale_dev, Cin, Cout, K, pl.ntn, pl.nslices, total);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_conv2d_wgrad_img_ws_h8)(int64_t* bytes, int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad) {
    using namespace H8_NS;
    if (!bytes) return l2i_set_error(L2I_E_ARG, "conv2d_wgrad_img_ws_h8: null bytes");
    WgradImgPlan pl;
    if (const char* why = wgrad_img_plan(pl, B, Cin, H, W, Cout, OH, OW, K, stride, pad)) {
        *bytes = 0;
        return l2i_set_error(L2I_E_UNSUPPORTED, why);
    }
    *bytes = pl.ws_bytes;
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_conv2d_wgrad_img_h8)(float* dw, const float* x, const void* gy, float* ws, int64_t ws_bytes, int B, int Cin, int H, int W, int Cout,
                                                int OH, int OW, int K, int stride, int pad, void* stream) {
    using namespace H8_NS;
    WgradImgPlan pl;
    if (const char* why = wgrad_img_plan(pl, B, Cin, H, W, Cout, OH, OW, K, stride, pad)) return l2i_set_error(L2I_E_UNSUPPORTED, why);
    if (!dw || !x || !gy) return l2i_set_error(L2I_E_ARG, "conv2d_wgrad_img_h8: null tensor");
    if (!ws) return l2i_set_error(L2I_E_UNSUPPORTED, "conv2d_wgrad_img_h8: null workspace (size: l2i_conv2d_wgrad_img_ws_h8)");
    if (ws_bytes < pl.ws_bytes) return l2i_set_error(L2I_E_UNSUPPORTED, "conv2d_wgrad_img_h8: workspace smaller than l2i_conv2d_wgrad_img_ws_h8 asks for");
    if (!al16(gy)) return l2i_set_error(L2I_E_ARG, "conv2d_wgrad_img_h8: gy must be 16-byte aligned");
    if ((((uintptr_t)dw) | ((uintptr_t)x) | ((uintptr_t)ws)) % 4) return l2i_set_error(L2I_E_ARG, "conv2d_wgrad_img_h8: dw, x and ws must be 4-byte aligned");
    WgradImg p;
    p.x = x; p.gy = gy; p.ws = ws; p.H = H; p.W = W; p.OH = OH; p.OW = OW; p.ncb = pl.ncb; p.nrs = pl.nrs; p.rows_per = pl.rows_per;
    hipStream_t st = (hipStream_t)stream;
    L2I_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_img_partial_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, wi::LDS));
    hipLaunchKernelGGL(wgrad_img_partial_kernel, dim3((unsigned)pl.nslices), dim3(256), (size_t)wi::LDS, st, p);
    L2I_CHECK_LAUNCH();
    hipLaunchKernelGGL(wgrad_img_reduce_kernel, dim3((wi::CO * wi::NT + 255) / 256), dim3(256), 0, st, dw, ws, pl.nslices);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_repack_planes_h8)(const void* table, int nseg, int nblocks, void* stream) {
    using namespace H8_NS;
    if (!table || (((uintptr_t)table) % 8) != 0) return l2i_set_error(L2I_E_ARG, "repack_planes_h8: the table must be a device pointer on an 8-byte boundary");
    if (nseg <= 0 || nblocks < nseg) return l2i_set_error(L2I_E_ARG, "repack_planes_h8: nseg >= 1 and at least one block per segment");
    hipLaunchKernelGGL(repack_planes_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const PlaneSeg*>(table), nseg, nblocks);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_bn_ws_h8)(int64_t* bytes, int B, int C, int64_t HW) {
    using namespace H8_NS;
    if (!bytes) return l2i_set_error(L2I_E_ARG, "bn_ws_h8: null bytes");
    if (const char* why = bn_shape(B, C, HW)) {
        *bytes = 0;
        return l2i_set_error(L2I_E_UNSUPPORTED, why);
    }
    *bytes = (int64_t)(C / 8) * bn_nblk(B, HW) * 16 * 8;
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_bn_stats_h8)(double* sum, double* sumsq, const void* x, double* ws, int64_t ws_bytes, int B, int C, int64_t HW, void* stream) {
    using namespace H8_NS;
    if (const char* why = bn_shape(B, C, HW)) return l2i_set_error(L2I_E_UNSUPPORTED, why);
    if (!sum || !sumsq || !x || !ws) return l2i_set_error(L2I_E_ARG, "bn_stats_h8: null pointer");
    if (!al16(x) || (((uintptr_t)ws) % 8) != 0) return l2i_set_error(L2I_E_ARG, "bn_stats_h8: x must be 16-byte, ws 8-byte aligned");
    const int nblk = bn_nblk(B, HW);
    if (ws_bytes < (int64_t)(C / 8) * nblk * 16 * 8) return l2i_set_error(L2I_E_ARG, "bn_stats_h8: workspace smaller than l2i_bn_ws_h8 asks for");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_stats_h8_kernel, dim3((unsigned)(C / 8), (unsigned)nblk), dim3(256), 0, st, ws, reinterpret_cast<const u32x4*>(x), B, C / 8, (long long)HW);
    L2I_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_finish_h8_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, sum, sumsq, ws, C, nblk);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_bn_apply_h8)(void* y, const void* x, const float* scale, const float* shift, const void* residual, int relu, int B, int C, int64_t HW,
                                        void* stream) {
    using namespace H8_NS;
    if (const char* why = bn_shape(B, C, HW)) return l2i_set_error(L2I_E_UNSUPPORTED, why);
    if (!y || !x || !scale || !shift) return l2i_set_error(L2I_E_ARG, "bn_apply_h8: null pointer");
    if (!al16(y) || !al16(x) || !al16(residual)) return l2i_set_error(L2I_E_ARG, "bn_apply_h8: maps must be 16-byte aligned");
    hipLaunchKernelGGL(bn_apply_h8_kernel, dim3(bn_pixel_blocks(HW), (unsigned)(C / 8), (unsigned)B), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<u32x4*>(y),
                       reinterpret_cast<const u32x4*>(x), scale, shift, reinterpret_cast<const u32x4*>(residual), relu, (long long)HW);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_bn_bwd_reduce_h8)(double* sum_dy, double* sum_dyxh, const void* gy, const void* out_mask, const void* x, const float* mean,
                                             const float* invstd, double* ws, int64_t ws_bytes, int B, int C, int64_t HW, void* stream) {
    using namespace H8_NS;
    if (const char* why = bn_shape(B, C, HW)) return l2i_set_error(L2I_E_UNSUPPORTED, why);
    if (!sum_dy || !sum_dyxh || !gy || !x || !mean || !invstd || !ws) return l2i_set_error(L2I_E_ARG, "bn_bwd_reduce_h8: null pointer");
    if (!al16(gy) || !al16(x) || !al16(out_mask) || (((uintptr_t)ws) % 8) != 0) return l2i_set_error(L2I_E_ARG, "bn_bwd_reduce_h8: maps must be 16-byte, ws 8-byte aligned");
    const int nblk = bn_nblk(B, HW);
    if (ws_bytes < (int64_t)(C / 8) * nblk * 16 * 8) return l2i_set_error(L2I_E_ARG, "bn_bwd_reduce_h8: workspace smaller than l2i_bn_ws_h8 asks for");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_bwd_reduce_h8_kernel, dim3((unsigned)(C / 8), (unsigned)nblk), dim3(256), 0, st, ws, reinterpret_cast<const u32x4*>(gy),
                       reinterpret_cast<const u32x4*>(out_mask), reinterpret_cast<const u32x4*>(x), mean, invstd, B, C / 8, (long long)HW);
    L2I_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_finish_h8_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, sum_dy, sum_dyxh, ws, C, nblk);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_bn_bwd_apply_h8)(void* dx, void* dy_masked, const void* gy, const void* out_mask, const void* x, const float* mean, const float* invstd,
                                            const float* gamma, const float* mean_dy, const float* mean_dyxh, int B, int C, int64_t HW, void* stream) {
    using namespace H8_NS;
    if (const char* why = bn_shape(B, C, HW)) return l2i_set_error(L2I_E_UNSUPPORTED, why);
    if (!dx || !gy || !x || !mean || !invstd || !gamma || !mean_dy || !mean_dyxh) return l2i_set_error(L2I_E_ARG, "bn_bwd_apply_h8: null pointer");
    if (!al16(dx) || !al16(dy_masked) || !al16(gy) || !al16(out_mask) || !al16(x)) return l2i_set_error(L2I_E_ARG, "bn_bwd_apply_h8: maps must be 16-byte aligned");
    hipLaunchKernelGGL(bn_bwd_apply_h8_kernel, dim3(bn_pixel_blocks(HW), (unsigned)(C / 8), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<u32x4*>(dx), reinterpret_cast<u32x4*>(dy_masked), reinterpret_cast<const u32x4*>(gy), reinterpret_cast<const u32x4*>(out_mask),
                       reinterpret_cast<const u32x4*>(x), mean, invstd, gamma, mean_dy, mean_dyxh, (long long)HW);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
