// l2i_panels.hip — uint8 panel grids on the device (gfx950).  Entry point l2i_panels_u8.
//
// Reference: utils/image.py — clip_ims (np.uint8(np.clip(((x + 1) / 2.0) * 255, 0, 255)) in float32) and imgrid (every tile padded on its
// bottom and right with the fill value, tiles laid out row-major, the last gutter cropped).  The visualisation drivers made both on the host
// from fp32 copies of every panel (12 bytes a pixel through PCIe, four numpy passes); here one launch reads the fp32 images [N,C,H,W] where the
// generator left them and writes G finished channel-last grids [G][GH][GW][C] uint8, which then cross to the host at 1 byte a value.
//
// The launch owns `out`: the buffer is cut into its byte head up to the first 16-byte boundary, 16-byte vectors, and a byte tail.  One lane makes
// one vector — it walks the 16 output bytes through (grid, row, tile, pixel, channel), works out the source element of each (none in a gutter / an
// empty tile: `fill`), issues the 16 loads together and stores the four dwords at once — and one lane makes one head or tail byte.  So every
// byte is written exactly once, by one lane, without reading `out`: tiles that share a dword (pad 0 with W * C off a multiple of 4) need no
// read-modify-write.
// A gather and not a row staged in LDS: consecutive lanes of a vector row read consecutive runs of 16 / C floats in each of the C planes, which the
// vector cache already coalesces into whole lines (each line is fetched once per plane and used in full), and there is no reuse for LDS to serve.
// Traffic: 4 bytes read + 1 written per value, 15 bytes a pixel at C = 3.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"

namespace l2i_panels {

constexpr int PN_THREADS = 256;

struct geom {
    int rows, cols, C, H, W, pad, N, fill;
    int TH, TW;              // tile pitch: H + pad, W + pad
    int GH;                  // rows * TH - pad
    int64_t pitch;           // bytes of one grid row: (cols * TW - pad) * C
    int64_t plane;           // H * W
};

// Where one output byte lies: grid g, tile (trow, tcol), pixel (ty, tx) inside the tile pitch, channel ch.
struct cursor {
    int64_t g;
    int trow, ty, tcol, tx, ch;
};

__device__ __forceinline__ cursor locate(const geom& q, int64_t off) {
    cursor c;
    const int64_t row = off / q.pitch;
    const int xc = (int)(off - row * q.pitch);
    const int px = xc / q.C;
    c.ch = xc - px * q.C;
    c.tcol = px / q.TW;
    c.tx = px - c.tcol * q.TW;
    c.g = row / q.GH;
    const int y = (int)(row - c.g * q.GH);
    c.trow = y / q.TH;
    c.ty = y - c.trow * q.TH;
    return c;
}

// the next byte in memory order (the last tile of a row / column has no gutter: the byte after its last pixel starts the next row / grid);
// returns whether it lies in another tile than the byte before
__device__ __forceinline__ bool advance(const geom& q, cursor& c) {
    if (++c.ch < q.C) return false;
    c.ch = 0;
    ++c.tx;
    const bool last_col = c.tcol == q.cols - 1;
    if (c.tx < (last_col ? q.W : q.TW)) return false;
    c.tx = 0;
    if (!last_col) {
        ++c.tcol;
        return true;
    }
    c.tcol = 0;
    ++c.ty;
    const bool last_row = c.trow == q.rows - 1;
    if (c.ty < (last_row ? q.H : q.TH)) return true;
    c.ty = 0;
    if (!last_row) {
        ++c.trow;
        return true;
    }
    c.trow = 0;
    ++c.g;
    return true;
}

// the image of the cursor's tile, or -1 for an empty tile
__device__ __forceinline__ int tile_image(const geom& q, const cursor& c, const int32_t* __restrict__ tile_src) {
    const int s = tile_src[(c.g * q.rows + c.trow) * q.cols + c.tcol];
    return s < 0 || s >= q.N ? -1 : s;
}

// the element of x the cursor's byte is made from, or -1 where it is fill (a gutter, an empty tile)
__device__ __forceinline__ int64_t source_of(const geom& q, const cursor& c, int s) {
    if (s < 0 || c.tx >= q.W || c.ty >= q.H) return -1;
    return ((int64_t)s * q.C + c.ch) * q.plane + (int64_t)c.ty * q.W + c.tx;
}

// work items [0, nvec): the 16-byte vectors from byte `head` on; [nvec, nvec + nedge): the head bytes, then the tail bytes
__global__ __launch_bounds__(PN_THREADS) void panels_u8_kernel(uint8_t* __restrict__ out, const float* __restrict__ x, const int32_t* __restrict__ tile_src,
                                                               geom q, int64_t total, int head, int64_t nvec) {
    const int64_t tail0 = head + nvec * 16;
    const int64_t items = nvec + head + (total - tail0);
    for (int64_t i = (int64_t)blockIdx.x * PN_THREADS + threadIdx.x; i < items; i += (int64_t)gridDim.x * PN_THREADS) {
        if (i < nvec) {
            const int64_t off = head + i * 16;
            cursor c = locate(q, off);
            int s = tile_image(q, c, tile_src);
            // the 16 sources first, then 16 independent loads (a fill byte loads x[0] and drops it), then the quantiser: no load waits on another
            int64_t src[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                src[k] = source_of(q, c, s);
                if (advance(q, c) && k < 15) s = tile_image(q, c, tile_src);
            }
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = x[src[k] < 0 ? 0 : src[k]];
            u32x4 w;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                unsigned t = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int k = 4 * d + b;
                    t |= (unsigned)(src[k] < 0 ? q.fill : quant8(v[k])) << (8 * b);
                }
                w[d] = t;
            }
            *reinterpret_cast<u32x4*>(out + off) = w;
        } else {
            const int64_t e = i - nvec;
            const int64_t off = e < head ? e : tail0 + (e - head);
            const cursor c = locate(q, off);
            const int64_t src = source_of(q, c, tile_image(q, c, tile_src));
            out[off] = (uint8_t)(src < 0 ? q.fill : quant8(x[src]));
        }
    }
}

}  // namespace l2i_panels

extern "C" int l2i_panels_u8(uint8_t* out, const float* x, const int32_t* tile_src, int G, int rows, int cols, int C, int H, int W, int pad, int fill,
                             int N, void* stream) {
    using namespace l2i_panels;
    if (!out || !x || !tile_src) return l2i_set_error(L2I_E_ARG, "l2i_panels_u8: null pointer");
    if ((C != 1 && C != 3) || pad < 0 || fill < 0 || fill > 255 || G < 1 || rows < 1 || cols < 1 || H < 1 || W < 1 || N < 1)
        return l2i_set_error(L2I_E_UNSUPPORTED, "l2i_panels_u8: C is 1 or 3, pad >= 0, fill in 0..255, and G, rows, cols, H, W, N >= 1");
    if ((((uintptr_t)x) & 3) != 0) return l2i_set_error(L2I_E_UNSUPPORTED, "l2i_panels_u8: x off a 4-byte boundary");
    const int64_t TH = (int64_t)H + pad, TW = (int64_t)W + pad;
    const int64_t GH = rows * TH - pad, GW = cols * TW - pad;
    // 32-bit row coordinates inside the kernel; every byte offset is 64-bit
    if (GH > 0x3FFFFFFF || GW * C > 0x3FFFFFFF || (int64_t)G * rows * cols > 0x3FFFFFFF || (int64_t)H * W > 0x3FFFFFFF)
        return l2i_set_error(L2I_E_UNSUPPORTED, "l2i_panels_u8: a grid side, a plane or the tile table beyond 2^30");
    geom q;
    q.rows = rows, q.cols = cols, q.C = C, q.H = H, q.W = W, q.pad = pad, q.N = N, q.fill = fill;
    q.TH = (int)TH, q.TW = (int)TW, q.GH = (int)GH;
    q.pitch = GW * C;
    q.plane = (int64_t)H * W;
    const int64_t total = (int64_t)G * GH * q.pitch;
    int64_t head = (int64_t)((16 - (((uintptr_t)out) & 15)) & 15);
    if (head > total) head = total;
    const int64_t nvec = (total - head) / 16;
    const int64_t items = nvec + head + (total - head - nvec * 16);
    hipLaunchKernelGGL(panels_u8_kernel, dim3(l2i_grid_for(items, PN_THREADS, 256 * 32)), dim3(PN_THREADS), 0, (hipStream_t)stream, out, x, tile_src, q,
                       total, (int)head, nvec);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
