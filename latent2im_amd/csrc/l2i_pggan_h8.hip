// l2i_pggan_h8.hip — PixelNorm + LeakyReLU of the PGGAN-256 generator on 16-bit h8 maps [B][C/8][H][W][8] (gfx950), forward and backward, with the
// nearest 2x upsample that follows every block but the last fused into the forward's store and that upsample's adjoint (the 2x2 sum) fused into
// the backward's load.  Entry points l2i_pixelnorm_act_h8, l2i_pixelnorm_act_bwd_h8 and, compiled with -DL2I_H8_F16, their _f16 twins
// (include/l2i.h).  Same function as l2i_pggan.hip's fp32 pair: y = lrelu(x / sqrt(mean_c x^2 + eps)), dx = r g' - x r^3 sum_c(g' x) / C.
//
// A pixel's channel column is C/8 slots of 16 bytes, HW * 16 bytes apart: 1 KiB per pixel at C = 512, too much for one lane.  So:
//   split    (C >= 32) a block of four waves owns 64 consecutive pixels of the flattened [B][HW] index; lane l of every wave is pixel l, wave w
//            holds the slots w, w + 4, w + 8, ...  (at most NS = 16 of them: 64 VGPRs of packed x; the backward also keeps g' in fp32).  Every access
//            of a wave is then one slot of 64 consecutive pixels = a 1 KiB row.  The per-pixel partial sums (sum x^2; backward also sum g' x) meet
//            in LDS and are added in wave order ((w0 + w1) + w2) + w3, so every operand is read from HBM once and nothing is re-read from L2.
//   narrow   (C = 8, 16, 24: fewer slots than waves) every wave owns 64 pixels of its own and all their slots; no LDS.
// Inside a wave the slots are summed in ascending order and the eight channels of a slot in ascending order: a fixed order, no atomics, equal
// inputs give equal bits.  All arithmetic is fp32; the only rounding to the element type is the packing convert at the store.  With up = 2 the
// four copies of a result (and the optional 1x copy) are the same packed register.  With pool = 2 the window is summed (g00 + g01) + (g10 + g11)
// in fp32 before anything else, then the 1x addend is added: no pooled map is ever stored.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"
#include "l2i_h8_common.h"

namespace H8_NS {

namespace pgn {
constexpr int PX = 64;                     // pixels per wave (one per lane)

struct Pixel {                             // where lane's pixel sits: slot index of (b, slot 0, h, w) at 1x and at 2x, in 16-byte slots
    bool valid;
    long long at1, at2;
};

// SPLIT: the block's four waves share pixels [64 blk, 64 blk + 64); else wave w of the block owns pixels [64 (4 blk + w), .. + 64)
template <bool SPLIT>
__device__ __forceinline__ Pixel locate(long long NP, int G, int H, int W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long p = ((long long)blockIdx.x * (SPLIT ? 1 : 4) + (SPLIT ? 0 : wave)) * PX + lane;
    Pixel q;
    q.valid = p < NP;
    const long long HW = (long long)H * W;
    const long long b = q.valid ? p / HW : 0;
    const int hw = q.valid ? (int)(p - b * HW) : 0;
    const int h = hw / W, w = hw - h * W;
    q.at1 = b * G * HW + hw;
    q.at2 = b * G * HW * 4 + (long long)(2 * h) * (2 * W) + 2 * w;
    return q;
}

// sum of the four waves' partials of this lane's pixel, in wave order, in every wave
__device__ __forceinline__ float meet(float v, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    red[wave * PX + lane] = v;
    __syncthreads();
    return ((red[lane] + red[PX + lane]) + red[2 * PX + lane]) + red[3 * PX + lane];
}
}  // namespace pgn

// y (and y_low) = lrelu(x / sqrt(mean_c x^2 + eps), slope).  UP: y is the [.., 2H, 2W, 8] map and gets every result four times.
template <int NS, bool SPLIT, bool UP>
__global__ __launch_bounds__(256) void pixelnorm_act_h8_kernel(u32x4* __restrict__ y, u32x4* __restrict__ y_low, const u32x4* __restrict__ x, long long NP, int G,
                                                               int H, int W, float C, float eps, float slope) {
    __shared__ float red[SPLIT ? 4 * pgn::PX : 1];
    const pgn::Pixel q = pgn::locate<SPLIT>(NP, G, H, W);
    const int first = SPLIT ? (int)(threadIdx.x >> 6) : 0, step = SPLIT ? 4 : 1;
    const long long HW = (long long)H * W;
    u32x4 raw[NS];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = first + i * step;
        raw[i] = u32x4{0u, 0u, 0u, 0u};
        if (q.valid && s < G) raw[i] = x[q.at1 + s * HW];
        float v[8];
        h8_unpack(raw[i], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += v[e] * v[e];
    }
    if constexpr (SPLIT) ss = pgn::meet(ss, red);
    const float r = sqrtf(ss / C + eps);                                        // the reference DIVIDES by sqrt(mean + eps): so does this
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = first + i * step;
        if (!(q.valid && s < G)) continue;
        float v[8];
        h8_unpack(raw[i], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float t = v[e] / r;
            v[e] = t > 0.f ? t : t * slope;
        }
        const u32x4 o = h8_pack(v);
        if constexpr (UP) {
            u32x4* yp = y + q.at2 + s * HW * 4;
            yp[0] = o; yp[1] = o;
            yp[2 * W] = o; yp[2 * W + 1] = o;
            if (y_low) y_low[q.at1 + s * HW] = o;
        } else {
            y[q.at1 + s * HW] = o;
            if (y_low) y_low[q.at1 + s * HW] = o;
        }
    }
}

// dx = r g' - x r^3 sum_c(g' x) / C, r = 1 / sqrt(mean_c x^2 + eps), g' = g (x > 0 ? 1 : slope), g = gy (POOL: the sum of gy's 2x2 window) + addend
template <int NS, bool SPLIT, bool POOL>
__global__ __launch_bounds__(256) void pixelnorm_act_bwd_h8_kernel(u32x4* __restrict__ dx, const u32x4* __restrict__ gy, const u32x4* __restrict__ x,
                                                                   const u32x4* __restrict__ addend, long long NP, int G, int H, int W, float C, float eps,
                                                                   float slope) {
    __shared__ float red[SPLIT ? 8 * pgn::PX : 1];
    const pgn::Pixel q = pgn::locate<SPLIT>(NP, G, H, W);
    const int first = SPLIT ? (int)(threadIdx.x >> 6) : 0, step = SPLIT ? 4 : 1;
    const long long HW = (long long)H * W;
    u32x4 raw[NS];
    float gp[NS][8];
    float ss = 0.f, sg = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = first + i * step;
        const bool on = q.valid && s < G;
        raw[i] = u32x4{0u, 0u, 0u, 0u};
        if (on) raw[i] = x[q.at1 + s * HW];
        float v[8], g[8];
        h8_unpack(raw[i], v);
        if constexpr (POOL) {
            u32x4 a = u32x4{0u, 0u, 0u, 0u}, b = a, c = a, d = a;
            if (on) {
                const u32x4* p2 = gy + q.at2 + s * HW * 4;
                a = p2[0]; b = p2[1]; c = p2[2 * W]; d = p2[2 * W + 1];
            }
            float ga[8], gb[8], gc[8], gd[8];
            h8_unpack(a, ga); h8_unpack(b, gb); h8_unpack(c, gc); h8_unpack(d, gd);
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] = (ga[e] + gb[e]) + (gc[e] + gd[e]);
        } else {
            u32x4 a = u32x4{0u, 0u, 0u, 0u};
            if (on) a = gy[q.at1 + s * HW];
            h8_unpack(a, g);
        }
        if (addend) {                                                              // (kernel argument: uniform)
            u32x4 a = u32x4{0u, 0u, 0u, 0u};
            if (on) a = addend[q.at1 + s * HW];
            float ad[8];
            h8_unpack(a, ad);
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] += ad[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            gp[i][e] = v[e] > 0.f ? g[e] : g[e] * slope;
            ss += v[e] * v[e];
            sg += gp[i][e] * v[e];
        }
    }
    if constexpr (SPLIT) {
        ss = pgn::meet(ss, red);
        sg = pgn::meet(sg, red + 4 * pgn::PX);
    }
    const float r = 1.0f / sqrtf(ss / C + eps);
    const float k = r * r * r * sg / C;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = first + i * step;
        if (!(q.valid && s < G)) continue;
        float v[8];
        h8_unpack(raw[i], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = r * gp[i][e] - v[e] * k;
        dx[q.at1 + s * HW] = h8_pack(v);
    }
}

static bool al16(const void* q) { return (((uintptr_t)q) % 16) == 0; }

// slots a lane keeps: C / 8 for the narrow path (<= 3), a quarter of them, rounded up to a power of two, for the split path
static int slots_per_lane(int G) {
    if (G < 4) return 4;
    const int n = (G + 3) / 4;
    return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16;
}

template <bool UP>
static void launch_fwd(int ns, bool split, dim3 grid, hipStream_t st, u32x4* y, u32x4* y_low, const u32x4* x, long long NP, int G, int H, int W, float C, float eps,
                       float slope) {
#define L2I_PGN_FWD(NS_, SPLIT_) hipLaunchKernelGGL((pixelnorm_act_h8_kernel<NS_, SPLIT_, UP>), grid, dim3(256), 0, st, y, y_low, x, NP, G, H, W, C, eps, slope)
    if (!split) L2I_PGN_FWD(4, false);
    else if (ns == 1) L2I_PGN_FWD(1, true);
    else if (ns == 2) L2I_PGN_FWD(2, true);
    else if (ns == 4) L2I_PGN_FWD(4, true);
    else if (ns == 8) L2I_PGN_FWD(8, true);
    else L2I_PGN_FWD(16, true);
#undef L2I_PGN_FWD
}

template <bool POOL>
static void launch_bwd(int ns, bool split, dim3 grid, hipStream_t st, u32x4* dx, const u32x4* gy, const u32x4* x, const u32x4* addend, long long NP, int G, int H,
                       int W, float C, float eps, float slope) {
#define L2I_PGN_BWD(NS_, SPLIT_) \
    hipLaunchKernelGGL((pixelnorm_act_bwd_h8_kernel<NS_, SPLIT_, POOL>), grid, dim3(256), 0, st, dx, gy, x, addend, NP, G, H, W, C, eps, slope)
    if (!split) L2I_PGN_BWD(4, false);
    else if (ns == 1) L2I_PGN_BWD(1, true);
    else if (ns == 2) L2I_PGN_BWD(2, true);
    else if (ns == 4) L2I_PGN_BWD(4, true);
    else if (ns == 8) L2I_PGN_BWD(8, true);
    else L2I_PGN_BWD(16, true);
#undef L2I_PGN_BWD
}

// shared refusals; *blocks = the launch's grid
static int check_shape(const char* who, int B, int C, int H, int W, int factor, const char* factor_name, long long* blocks) {
    char msg[160];                                                                 // (l2i_set_error copies)
    if (C <= 0 || (C % 8) != 0 || C > 512) {
        snprintf(msg, sizeof msg, "%s: built for C %% 8 == 0, C <= 512", who);
        return l2i_set_error(L2I_E_UNSUPPORTED, msg);
    }
    if (factor != 1 && factor != 2) {
        snprintf(msg, sizeof msg, "%s: %s is 1 or 2", who, factor_name);
        return l2i_set_error(L2I_E_UNSUPPORTED, msg);
    }
    if (B <= 0 || H <= 0 || W <= 0) {
        snprintf(msg, sizeof msg, "%s: non-positive dimension", who);
        return l2i_set_error(L2I_E_ARG, msg);
    }
    const long long NP = (long long)B * H * W;
    const int per_block = C >= 32 ? pgn::PX : 4 * pgn::PX;
    *blocks = (NP + per_block - 1) / per_block;
    if (*blocks > 0x7fffffffLL || W > (1 << 28)) {
        snprintf(msg, sizeof msg, "%s: grid too large", who);
        return l2i_set_error(L2I_E_UNSUPPORTED, msg);
    }
    return L2I_OK;
}

}  // namespace H8_NS

extern "C" int H8_NAME(l2i_pixelnorm_act_h8)(void* y, void* y_low, const void* x, int B, int C, int H, int W, float eps, float slope, int up, void* stream) {
    using namespace H8_NS;
    long long blocks = 0;
    if (int rc = check_shape("pixelnorm_act_h8", B, C, H, W, up, "up", &blocks)) return rc;
    if (!y || !x) return l2i_set_error(L2I_E_ARG, "pixelnorm_act_h8: null tensor");
    if (!al16(y) || !al16(y_low) || !al16(x)) return l2i_set_error(L2I_E_ARG, "pixelnorm_act_h8: h8 maps must be 16-byte aligned");
    const int G = C / 8;
    const long long NP = (long long)B * H * W;
    const dim3 grid((unsigned)blocks);
    if (up == 2) launch_fwd<true>(slots_per_lane(G), G >= 4, grid, (hipStream_t)stream, (u32x4*)y, (u32x4*)y_low, (const u32x4*)x, NP, G, H, W, (float)C, eps, slope);
    else launch_fwd<false>(slots_per_lane(G), G >= 4, grid, (hipStream_t)stream, (u32x4*)y, (u32x4*)y_low, (const u32x4*)x, NP, G, H, W, (float)C, eps, slope);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int H8_NAME(l2i_pixelnorm_act_bwd_h8)(void* dx, const void* gy, const void* x, const void* addend, int B, int C, int H, int W, float eps, float slope,
                                                 int pool, void* stream) {
    using namespace H8_NS;
    long long blocks = 0;
    if (int rc = check_shape("pixelnorm_act_bwd_h8", B, C, H, W, pool, "pool", &blocks)) return rc;
    if (!dx || !gy || !x) return l2i_set_error(L2I_E_ARG, "pixelnorm_act_bwd_h8: null tensor");
    if (!al16(dx) || !al16(gy) || !al16(x) || !al16(addend)) return l2i_set_error(L2I_E_ARG, "pixelnorm_act_bwd_h8: h8 maps must be 16-byte aligned");
    const int G = C / 8;
    const long long NP = (long long)B * H * W;
    const dim3 grid((unsigned)blocks);
    if (pool == 2)
        launch_bwd<true>(slots_per_lane(G), G >= 4, grid, (hipStream_t)stream, (u32x4*)dx, (const u32x4*)gy, (const u32x4*)x, (const u32x4*)addend, NP, G, H, W, (float)C,
                         eps, slope);
    else
        launch_bwd<false>(slots_per_lane(G), G >= 4, grid, (hipStream_t)stream, (u32x4*)dx, (const u32x4*)gy, (const u32x4*)x, (const u32x4*)addend, NP, G, H, W, (float)C,
                          eps, slope);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
