// l2i_face.hip — the identity-preservation half of eval.py on the device (gfx950).  Entry points l2i_face_resize_f32, l2i_face_head_f32, and
// the differentiable twin of the pair for the identity loss of walk training: l2i_face_resize_lin_f32, l2i_face_resize_lin_bwd_f32,
// l2i_face_head_bwd_f32.
//
// Reference: eval.py:170-198 — every bucket entry's edited and original image is quantised (clip_ims: np.uint8(np.clip(((x + 1) / 2.0) * 255,
// 0, 255)) in float32), resized by PIL's Image.resize((160, 160)) (bicubic, antialiased), handed to facenet_pytorch's InceptionResnetV1 as
// raw 0..255 floats and compared by scipy's cosine distance.  Here the whole batch stays on the device:
//   * l2i_face_resize_f32: quantisation + PIL's two separable fixed-point passes (Resample.c: 22-bit coefficients, int32 accumulation from
//     2^21, >> 22 and clip to 0..255 after EACH pass, i.e. a uint8 intermediate).  The coefficient / bound tables are PIL's, computed by the
//     caller in double (latent2im_amd/facenet.py:resize_tables); the kernel does integer MACs only, so the result is PIL's bit for bit.  One
//     block makes FR_ROWS output rows of one plane: the horizontal pass of the input rows those rows read goes to LDS (uint8), then the
//     vertical pass reads LDS.
//   * l2i_face_head_f32: the network's head (avgpool_1a, last_linear with last_bn folded in by the caller, F.normalize) for the whole batch,
//     and optionally the cosine distance of every (edited, original) pair in float64.
//   * l2i_face_resize_lin_f32: the same taps without the byte intermediate, the rounding and the clips: u = clip(((x + 1) 0.5) 255, 0, 255) in
//     fp32, r = Ry u Rx^T with R = the table / 2^22, horizontal pass first.  The horizontal pass of the input rows a block's LIN_ROWS output rows
//     read goes to LDS as fp32, in chunks of as many rows as fit; every output keeps its sum in a register across the chunks, taps in
//     ascending order.  l2i_face_resize_lin_bwd_f32 is its adjoint as a gather over the inverse tables (per input pixel: first output, count,
//     coefficients): one block makes LINB_ROWS input rows of a plane, the vertical gather of their rows goes to LDS once, every lane then
//     gathers and writes its own pixels.  No atomics: every sum has a fixed order.
//   * l2i_face_head_bwd_f32: the gradient of 1 - cos(e, v) through the head, down to the trunk's output map; one block a sample.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdio.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"

namespace l2i_face {

constexpr int FR_ROWS = 16;            // output rows per block
constexpr int FR_LDS = 48 * 1024;      // bytes of uint8 intermediate rows per block
constexpr int FR_THREADS = 256;

// Resample.c clip8: the 22-bit fixed-point sum back to a byte
__device__ __forceinline__ int clip8(int acc) {
    if (acc >= (1 << 30)) return 255;
    if (acc <= 0) return 0;
    return acc >> 22;
}

__global__ __launch_bounds__(FR_THREADS) void face_resize_kernel(float* __restrict__ y, const float* __restrict__ x, int tiles, int H, int W, int OH,
                                                                 int OW, const int32_t* __restrict__ xb, const int32_t* __restrict__ xc, int xk,
                                                                 const int32_t* __restrict__ yb, const int32_t* __restrict__ yc, int yk) {
    __shared__ uint8_t mid[FR_LDS];
    const int64_t plane = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(plane * tiles);
    const int oy0 = tile * FR_ROWS, oy1 = min(oy0 + FR_ROWS, OH);
    const int r0 = yb[2 * oy0];
    const int r1 = yb[2 * (oy1 - 1)] + yb[2 * (oy1 - 1) + 1];            // bounds are non-decreasing in the output index
    const int nrows = min(r1 - r0, FR_LDS / OW);                         // (the host bounds the span; never write past the buffer)
    const float* xp = x + plane * (int64_t)H * W;
    for (int i = threadIdx.x; i < nrows * OW; i += FR_THREADS) {
        const int r = i / OW, ox = i - r * OW;
        const int iy = r0 + r;
        const int xmin = xb[2 * ox], n = min(xb[2 * ox + 1], xk);
        const int32_t* k = xc + (int64_t)ox * xk;
        int acc = 1 << 21;
        if (iy >= 0 && iy < H) {
            const float* row = xp + (int64_t)iy * W;
            for (int t = 0; t < n; ++t) {
                const int xi = xmin + t;
                if (xi >= 0 && xi < W) acc += quant8(row[xi]) * k[t];
            }
        }
        mid[i] = (uint8_t)clip8(acc);
    }
    __syncthreads();
    float* yp = y + plane * (int64_t)OH * OW;
    for (int i = threadIdx.x; i < (oy1 - oy0) * OW; i += FR_THREADS) {
        const int oy = oy0 + i / OW, ox = i - (i / OW) * OW;
        const int ymin = yb[2 * oy] - r0, n = min(yb[2 * oy + 1], yk);
        const int32_t* k = yc + (int64_t)oy * yk;
        int acc = 1 << 21;
        for (int t = 0; t < n; ++t) {
            const int r = ymin + t;
            if (r >= 0 && r < nrows) acc += (int)mid[r * OW + ox] * k[t];
        }
        yp[(int64_t)oy * OW + ox] = (float)clip8(acc);
    }
}

// ---- the differentiable resize ----------------------------------------------------------------------------------------------------------
constexpr int LIN_ROWS = 8;                       // output rows per block
constexpr int LIN_LDS = 12288;                    // fp32 intermediate values per block (48 KiB)
constexpr int LIN_ACC = LIN_ROWS * 256 / FR_THREADS;      // outputs per thread at the widest output (OW <= 256)
constexpr float LIN_COEF = 1.0f / 4194304.0f;     // 2^-22: the tables are 22-bit fixed point (exact in fp32: |coefficient| < 2^24)

// clip_ims without the truncating cast (NaN -> 0)
__device__ __forceinline__ float level255(float v) { return __fmul_rn(__fmul_rn(__fadd_rn(v, 1.0f), 0.5f), 255.0f); }
__device__ __forceinline__ float clip255(float v) { return fminf(fmaxf(level255(v), 0.0f), 255.0f); }

__global__ __launch_bounds__(FR_THREADS) void face_resize_lin_kernel(float* __restrict__ y, const float* __restrict__ x, int tiles, int H, int W, int OH,
                                                                     int OW, const int32_t* __restrict__ xb, const int32_t* __restrict__ xc, int xk,
                                                                     const int32_t* __restrict__ yb, const int32_t* __restrict__ yc, int yk) {
    __shared__ float mid[LIN_LDS];
    const int64_t plane = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(plane * tiles);
    const int oy0 = tile * LIN_ROWS, oy1 = min(oy0 + LIN_ROWS, OH);
    const int r0 = max(yb[2 * oy0], 0);                                                   // bounds are non-decreasing in the output index
    const int r1 = min(yb[2 * (oy1 - 1)] + min(yb[2 * (oy1 - 1) + 1], yk), H);
    const int cap = LIN_LDS / OW;                                                         // rows of the intermediate one chunk holds
    const int nout = (oy1 - oy0) * OW;
    const float* xp = x + plane * (int64_t)H * W;
    float acc[LIN_ACC];
#pragma unroll
    for (int j = 0; j < LIN_ACC; ++j) acc[j] = 0.f;
    for (int c0 = r0; c0 < r1; c0 += cap) {
        const int crows = min(cap, r1 - c0);
        __syncthreads();                                                                  // the previous chunk has been read
        for (int i = threadIdx.x; i < crows * OW; i += FR_THREADS) {
            const int r = i / OW, ox = i - r * OW;
            const int xmin = xb[2 * ox], n = min(xb[2 * ox + 1], xk);
            const int32_t* k = xc + (int64_t)ox * xk;
            const float* row = xp + (int64_t)(c0 + r) * W;
            float a = 0.f;
            for (int t = 0; t < n; ++t) {
                const int xi = xmin + t;
                if (xi >= 0 && xi < W) a = fmaf(__fmul_rn((float)k[t], LIN_COEF), clip255(row[xi]), a);
            }
            mid[i] = a;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LIN_ACC; ++j) {
            const int i = threadIdx.x + j * FR_THREADS;
            if (i < nout) {
                const int oy = oy0 + i / OW, ox = i - (i / OW) * OW;
                const int ymin = yb[2 * oy], n = min(yb[2 * oy + 1], yk);
                const int32_t* k = yc + (int64_t)oy * yk;
                const int t0 = max(c0 - ymin, 0), t1 = min(c0 + crows - ymin, n);
                float a = acc[j];
                for (int t = t0; t < t1; ++t) a = fmaf(__fmul_rn((float)k[t], LIN_COEF), mid[(ymin + t - c0) * OW + ox], a);
                acc[j] = a;
            }
        }
    }
    float* yp = y + plane * (int64_t)OH * OW + (int64_t)oy0 * OW;
#pragma unroll
    for (int j = 0; j < LIN_ACC; ++j) {
        const int i = threadIdx.x + j * FR_THREADS;
        if (i < nout) yp[i] = acc[j];
    }
}

constexpr int LINB_ROWS = 4;                      // input rows per block
constexpr int LINB_MAXOW = 256;

// gx[iy, ix] = 127.5 [0 < level(x) < 255] sum_ox cx[ix][.] (sum_oy cy[iy][.] gy[oy, ox]): ixb / iyb = (first output, count) per input pixel,
// ixc / iyc its coefficients (22-bit fixed point, the forward tables transposed)
__global__ __launch_bounds__(FR_THREADS) void face_resize_lin_bwd_kernel(float* __restrict__ gx, const float* __restrict__ gy, const float* __restrict__ x,
                                                                         int tiles, int H, int W, int OH, int OW, const int32_t* __restrict__ ixb,
                                                                         const int32_t* __restrict__ ixc, int ixk, const int32_t* __restrict__ iyb,
                                                                         const int32_t* __restrict__ iyc, int iyk) {
    __shared__ float v[LINB_ROWS * LINB_MAXOW];
    const int64_t plane = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(plane * tiles);
    const int iy0 = tile * LINB_ROWS, rows = min(LINB_ROWS, H - iy0);
    const float* gp = gy + plane * (int64_t)OH * OW;
    for (int i = threadIdx.x; i < rows * OW; i += FR_THREADS) {                            // Ry^T gy for the block's rows
        const int r = i / OW, ox = i - r * OW;
        const int iy = iy0 + r;
        const int omin = iyb[2 * iy], n = min(iyb[2 * iy + 1], iyk);
        const int32_t* k = iyc + (int64_t)iy * iyk;
        float a = 0.f;
        for (int t = 0; t < n; ++t) {
            const int oy = omin + t;
            if (oy >= 0 && oy < OH) a = fmaf(__fmul_rn((float)k[t], LIN_COEF), gp[(int64_t)oy * OW + ox], a);
        }
        v[r * LINB_MAXOW + ox] = a;
    }
    __syncthreads();
    for (int ix = threadIdx.x; ix < W; ix += FR_THREADS) {
        const int omin = ixb[2 * ix], n = min(ixb[2 * ix + 1], ixk);
        const int32_t* k = ixc + (int64_t)ix * ixk;
        const int t0 = max(-omin, 0), t1 = min(n, OW - omin);
        for (int r = 0; r < rows; ++r) {
            const int64_t idx = plane * (int64_t)H * W + (int64_t)(iy0 + r) * W + ix;
            float a = 0.f;
            for (int t = t0; t < t1; ++t) a = fmaf(__fmul_rn((float)k[t], LIN_COEF), v[r * LINB_MAXOW + omin + t], a);
            const float l = level255(x[idx]);
            gx[idx] = (l > 0.0f && l < 255.0f) ? __fmul_rn(127.5f, a) : 0.0f;            // (NaN: neither comparison holds)
        }
    }
}

constexpr int HEAD_THREADS = 256;
constexpr int HEAD_MAXC = 2048;
constexpr int HEAD_MAXE = 2 * HEAD_THREADS;

// Block j makes samples s[0], s[1]: (j, j + npairs) when pairs are asked for, else (2j, 2j + 1).
__global__ __launch_bounds__(HEAD_THREADS) void face_head_kernel(float* __restrict__ emb, double* __restrict__ dist, const float* __restrict__ feat,
                                                                 const float* __restrict__ w_t, const float* __restrict__ bias, int B, int C, int HW,
                                                                 int E, int npairs) {
    __shared__ float pooled[2][HEAD_MAXC];
    __shared__ float redf[4];
    __shared__ double redd[4];
    const int tid = threadIdx.x;
    int s[2];
    if (npairs > 0) {
        s[0] = blockIdx.x;
        s[1] = blockIdx.x + npairs;
    } else {
        s[0] = 2 * blockIdx.x;
        s[1] = 2 * blockIdx.x + 1 < B ? 2 * blockIdx.x + 1 : -1;
    }
    const float inv_hw = 1.0f / (float)HW;
    for (int j = 0; j < 2; ++j) {                                  // avgpool_1a
        if (s[j] < 0) {
            for (int c = tid; c < C; c += HEAD_THREADS) pooled[j][c] = 0.f;
            continue;
        }
        const float* f = feat + (int64_t)s[j] * C * HW;
        for (int c = tid; c < C; c += HEAD_THREADS) {
            float a = 0.f;
            for (int p = 0; p < HW; ++p) a += f[(int64_t)c * HW + p];
            pooled[j][c] = a * inv_hw;
        }
    }
    __syncthreads();
    float z[2][2] = {{0.f, 0.f}, {0.f, 0.f}};                      // [sample][output tid, tid + 256]
    const int e0 = tid, e1 = tid + HEAD_THREADS;
    for (int c = 0; c < C; ++c) {                                  // last_linear (+ folded last_bn scale): w_t is [C][E], coalesced in e
        const float w0 = e0 < E ? w_t[(int64_t)c * E + e0] : 0.f;
        const float w1 = e1 < E ? w_t[(int64_t)c * E + e1] : 0.f;
        const float p0 = pooled[0][c], p1 = pooled[1][c];
        z[0][0] += p0 * w0;
        z[0][1] += p0 * w1;
        z[1][0] += p1 * w0;
        z[1][1] += p1 * w1;
    }
    for (int j = 0; j < 2; ++j) {
        z[j][0] = e0 < E ? z[j][0] + bias[e0] : 0.f;
        z[j][1] = e1 < E ? z[j][1] + bias[e1] : 0.f;
    }
    for (int j = 0; j < 2; ++j) {                                  // F.normalize(p=2, eps=1e-12)
        const float ss = block_sum(z[j][0] * z[j][0] + z[j][1] * z[j][1], redf);
        const float nrm = fmaxf(sqrtf(ss), 1e-12f);
        z[j][0] = z[j][0] / nrm;
        z[j][1] = z[j][1] / nrm;
        if (s[j] >= 0) {
            if (e0 < E) emb[(int64_t)s[j] * E + e0] = z[j][0];
            if (e1 < E) emb[(int64_t)s[j] * E + e1] = z[j][1];
        }
    }
    if (npairs > 0) {                                              // scipy.spatial.distance.cosine on the float64 embeddings
        const double a0 = z[0][0], a1 = z[0][1], b0 = z[1][0], b1 = z[1][1];
        const double uv = block_sum(a0 * b0 + a1 * b1, redd);
        const double uu = block_sum(a0 * a0 + a1 * a1, redd);
        const double vv = block_sum(b0 * b0 + b1 * b1, redd);
        if (tid == 0) {
            double d = 1.0 - uv / sqrt(uu * vv);
            dist[blockIdx.x] = d < 0.0 ? 0.0 : (d > 2.0 ? 2.0 : d);
        }
    }
}

// One block a sample: the head again (the forward's own sums), then g_t = -g_dist (v^ - c e) / n, g_p = w_t g_t (one wave a channel, lanes over
// e, butterfly sum) and g_feat[c, :] = g_p[c] / HW.
__global__ __launch_bounds__(HEAD_THREADS) void face_head_bwd_kernel(float* __restrict__ g_feat, const float* __restrict__ feat, const float* __restrict__ w_t,
                                                                     const float* __restrict__ bias, const float* __restrict__ v,
                                                                     const float* __restrict__ g_dist, int C, int HW, int E) {
    __shared__ float pooled[HEAD_MAXC];
    __shared__ float gt[HEAD_MAXE];
    __shared__ float redf[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float inv_hw = 1.0f / (float)HW;
    const float* f = feat + (int64_t)b * C * HW;
    for (int c = tid; c < C; c += HEAD_THREADS) {                  // avgpool_1a
        float a = 0.f;
        for (int p = 0; p < HW; ++p) a += f[(int64_t)c * HW + p];
        pooled[c] = a * inv_hw;
    }
    __syncthreads();
    const int e0 = tid, e1 = tid + HEAD_THREADS;
    float z0 = 0.f, z1 = 0.f;
    for (int c = 0; c < C; ++c) {
        const float p = pooled[c];
        z0 += p * (e0 < E ? w_t[(int64_t)c * E + e0] : 0.f);
        z1 += p * (e1 < E ? w_t[(int64_t)c * E + e1] : 0.f);
    }
    z0 = e0 < E ? z0 + bias[e0] : 0.f;
    z1 = e1 < E ? z1 + bias[e1] : 0.f;
    const float nrm = fmaxf(sqrtf(block_sum(z0 * z0 + z1 * z1, redf)), 1e-12f);
    z0 = z0 / nrm;
    z1 = z1 / nrm;
    float v0 = e0 < E ? v[(int64_t)b * E + e0] : 0.f, v1 = e1 < E ? v[(int64_t)b * E + e1] : 0.f;
    const float vn = sqrtf(block_sum(v0 * v0 + v1 * v1, redf));
    v0 = v0 / vn;
    v1 = v1 / vn;
    const float c = block_sum(z0 * v0 + z1 * v1, redf);
    const float s = -g_dist[b] / nrm;
    if (e0 < E) gt[e0] = s * (v0 - c * z0);
    if (e1 < E) gt[e1] = s * (v1 - c * z1);
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    float* g = g_feat + (int64_t)b * C * HW;
    for (int ch = wave; ch < C; ch += HEAD_THREADS / 64) {
        float a = 0.f;
        for (int e = lane; e < E; e += 64) a += w_t[(int64_t)ch * E + e] * gt[e];
        a = wave_sum_all(a) / (float)HW;
        for (int p = lane; p < HW; p += 64) g[(int64_t)ch * HW + p] = a;
    }
}

}  // namespace l2i_face

// What both forward resizes take (l2i.h): 0, or the error already set.  The row bound is that of the byte kernel's LDS buffer for both, so that
// the two accept the same shapes.
static int face_resize_check(const char* name, const void* y, const void* x, int64_t planes, int H, int W, int OH, int OW, const void* xbounds,
                             const void* xcoef, int xk, const void* ybounds, const void* ycoef, int yk, int rows) {
    using namespace l2i_face;
    char msg[200];
    if (!y || !x || !xbounds || !xcoef || !ybounds || !ycoef || planes < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) {
        snprintf(msg, sizeof msg, "%s: null pointer or empty shape", name);
        return l2i_set_error(L2I_E_ARG, msg);
    }
    if (H > 4096 || W > 4096 || OH > 256 || OW > 256 || xk < 1 || yk < 1 || xk > 256 || yk > 256) {
        snprintf(msg, sizeof msg, "%s: built for inputs <= 4096 and outputs <= 256 pixels a side, <= 256 taps", name);
        return l2i_set_error(L2I_E_UNSUPPORTED, msg);
    }
    // input rows one block's FR_ROWS output rows read: at most (FR_ROWS - 1) * H / OH between their first taps, plus one support
    const int64_t span = ((int64_t)(FR_ROWS - 1) * H + OH - 1) / OH + yk + 1;
    if (span * OW > FR_LDS) {
        snprintf(msg, sizeof msg, "%s: the uint8 rows of one block's vertical support exceed its LDS buffer", name);
        return l2i_set_error(L2I_E_UNSUPPORTED, msg);
    }
    if (planes * ((OH + rows - 1) / rows) > 0x7FFFFFFF) {
        snprintf(msg, sizeof msg, "%s: too many planes", name);
        return l2i_set_error(L2I_E_UNSUPPORTED, msg);
    }
    return L2I_OK;
}

extern "C" int l2i_face_resize_f32(float* y, const float* x, int64_t planes, int H, int W, int OH, int OW, const int32_t* xbounds,
                                   const int32_t* xcoef, int xk, const int32_t* ybounds, const int32_t* ycoef, int yk, void* stream) {
    using namespace l2i_face;
    if (int rc = face_resize_check("l2i_face_resize_f32", y, x, planes, H, W, OH, OW, xbounds, xcoef, xk, ybounds, ycoef, yk, FR_ROWS)) return rc;
    const int tiles = (OH + FR_ROWS - 1) / FR_ROWS;
    hipLaunchKernelGGL(face_resize_kernel, dim3((unsigned)(planes * tiles)), dim3(FR_THREADS), 0, (hipStream_t)stream, y, x, tiles, H, W, OH, OW,
                       xbounds, xcoef, xk, ybounds, ycoef, yk);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_face_resize_lin_f32(float* y, const float* x, int64_t planes, int H, int W, int OH, int OW, const int32_t* xbounds,
                                       const int32_t* xcoef, int xk, const int32_t* ybounds, const int32_t* ycoef, int yk, void* stream) {
    using namespace l2i_face;
    if (int rc = face_resize_check("l2i_face_resize_lin_f32", y, x, planes, H, W, OH, OW, xbounds, xcoef, xk, ybounds, ycoef, yk, LIN_ROWS)) return rc;
    const int tiles = (OH + LIN_ROWS - 1) / LIN_ROWS;
    hipLaunchKernelGGL(face_resize_lin_kernel, dim3((unsigned)(planes * tiles)), dim3(FR_THREADS), 0, (hipStream_t)stream, y, x, tiles, H, W, OH, OW,
                       xbounds, xcoef, xk, ybounds, ycoef, yk);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_face_resize_lin_bwd_f32(float* gx, const float* gy, const float* x, int64_t planes, int H, int W, int OH, int OW,
                                           const int32_t* ixbounds, const int32_t* ixcoef, int ixk, const int32_t* iybounds, const int32_t* iycoef,
                                           int iyk, void* stream) {
    using namespace l2i_face;
    if (!gx || !gy || !x || !ixbounds || !ixcoef || !iybounds || !iycoef || planes < 1 || H < 1 || W < 1 || OH < 1 || OW < 1)
        return l2i_set_error(L2I_E_ARG, "l2i_face_resize_lin_bwd_f32: null pointer or empty shape");
    if (H > 4096 || W > 4096 || OH > LINB_MAXOW || OW > LINB_MAXOW || ixk < 1 || iyk < 1 || ixk > 256 || iyk > 256)
        return l2i_set_error(L2I_E_UNSUPPORTED, "l2i_face_resize_lin_bwd_f32: built for inputs <= 4096 and outputs <= 256 pixels a side, <= 256 taps");
    const int tiles = (H + LINB_ROWS - 1) / LINB_ROWS;
    if (planes * tiles > 0x7FFFFFFF) return l2i_set_error(L2I_E_UNSUPPORTED, "l2i_face_resize_lin_bwd_f32: too many planes");
    hipLaunchKernelGGL(face_resize_lin_bwd_kernel, dim3((unsigned)(planes * tiles)), dim3(FR_THREADS), 0, (hipStream_t)stream, gx, gy, x, tiles, H, W,
                       OH, OW, ixbounds, ixcoef, ixk, iybounds, iycoef, iyk);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_face_head_f32(float* emb, double* dist, const float* feat, const float* w_t, const float* bias, int B, int C, int HW, int E,
                                 int npairs, void* stream) {
    using namespace l2i_face;
    if (!emb || !feat || !w_t || !bias || B < 1 || C < 1 || HW < 1 || E < 1 || npairs < 0)
        return l2i_set_error(L2I_E_ARG, "l2i_face_head_f32: null pointer or empty shape");
    if (npairs > 0 && (B != 2 * npairs || !dist))
        return l2i_set_error(L2I_E_ARG, "l2i_face_head_f32: pairs need B == 2 * npairs and a dist buffer");
    if (C > HEAD_MAXC || E > HEAD_MAXE)
        return l2i_set_error(L2I_E_UNSUPPORTED, "l2i_face_head_f32: built for C <= 2048 pooled channels and E <= 512 embedding features");
    const int blocks = npairs > 0 ? npairs : (B + 1) / 2;
    hipLaunchKernelGGL(face_head_kernel, dim3(blocks), dim3(HEAD_THREADS), 0, (hipStream_t)stream, emb, dist, feat, w_t, bias, B, C, HW, E, npairs);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

extern "C" int l2i_face_head_bwd_f32(float* g_feat, const float* feat, const float* w_t, const float* bias, const float* v, const float* g_dist,
                                     int B, int C, int HW, int E, void* stream) {
    using namespace l2i_face;
    if (!g_feat || !feat || !w_t || !bias || !v || !g_dist || B < 1 || C < 1 || HW < 1 || E < 1)
        return l2i_set_error(L2I_E_ARG, "l2i_face_head_bwd_f32: null pointer or empty shape");
    if (C > HEAD_MAXC || E > HEAD_MAXE)
        return l2i_set_error(L2I_E_UNSUPPORTED, "l2i_face_head_bwd_f32: built for C <= 2048 pooled channels and E <= 512 embedding features");
    hipLaunchKernelGGL(face_head_bwd_kernel, dim3(B), dim3(HEAD_THREADS), 0, (hipStream_t)stream, g_feat, feat, w_t, bias, v, g_dist, C, HW, E);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
