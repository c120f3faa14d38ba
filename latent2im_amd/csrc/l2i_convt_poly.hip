// l2i_convt_poly.hip — fp32 stride-2 TRANSPOSED 3x3 convolution on 25 of its 36 multiplies (gfx950, v_mfma_f32_16x16x4_f32).
//
//   y[b, co, 2*iy + ky - pad, 2*ix + kx - pad] += x[b, ci, iy, ix] * w[co, ci, ky, kx]                 (pad 0 or 1)
//
// In one dimension the outputs of one parity are a 2-tap filter over the input (taps w2, w0) and those of the other parity a 1-tap filter (w1).
// Two adjacent outputs of the 2-tap filter are Winograd F(2,2): with the raw values r0, r1, r2 = x[2W - 1 + pad + {0, 1, 2}] of WINDOW W
//   m0 = (r0 - r1) w2,  m1 = r1 (w0 + w2),  m2 = (r1 - r2) w0,    2-tap outputs  m0 + m1,  m1 - m2
//   m3 = s0 w1,  m4 = s1 w1        with (s0, s1) = (r1, r2) for pad 0, (r0, r1) for pad 1
// so a window yields the four outputs 4W .. 4W + 3 (pad 0: [m0 + m1, m3, m1 - m2, m4]; pad 1: [m3, m0 + m1, m4, m1 - m2]) from 5 products instead
// of 6, and in two dimensions a 3x3 raw patch yields a 4x4 output patch from 25 products instead of 36.  Only four transformed values per
// dimension are distinct (r0 - r1, r1, r1 - r2 and r2 / r0), and only four weight planes (w2, w0 + w2, w0, w1): the kernel keeps 16 B operands and
// 16 A operands per input channel and issues 25 MFMAs on them.  All coefficients are 0 or +-1.
//
// `w_lo` holds the fp32 pack [Cin][25][CoutP] of latent2im_amd/conv.py:pack_weight_convt_poly, plane 5 a + b = the product of the 1-D planes a and b
// above; planes with a == 4 or b == 4 repeat a == 3 / b == 3 and are not staged.
//
// Block = 256 threads = 4 waves, block tile = 16 output channels x 64 windows (WTH rows of WTW); a wave owns 16 windows: MFMA A = a weight plane
// (16 channels out x 4 channels in), B = a transformed value (4 channels in x 16 windows), 25 accumulators of 4 registers.  A lane ends with the 25
// products of ONE window for 4 output channels: the inverse transform (18 additions) is lane-local and gives a 4x4 output patch per channel, stored
// 16 bytes per row.  Both operands go global -> LDS by DMA (l2i_device.h) into the other of two stages while the current chunk of CK input channels
// multiplies, as in l2i_convt.hip's DMAIN path; a masked launch stages the mask tile the same way and applies it to the raw values as they are read.
// Fused: in_scale, in_mask (on the raw values, before the transform), out_scale, out_gain — what l2i_conv_transpose2d_f32 fuses.
//
// Occupancy decides here (profiles/convt_poly_ab.txt, the variants table): with 100 accumulator registers and ONE set of fragment registers a lane
// stays under 168 registers, so three blocks share a CU (<= 52 KiB of LDS each: 8 channels per stage unmasked, 4 masked) and the fragment reads of
// one wave hide behind the MFMAs of two others.  The same kernel at two blocks per CU with double-buffered fragments, and with the fragment reads
// carried across the chunk barrier, was 13 - 19 % slower on the step's forward shapes.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"

namespace {

constexpr int POLY_BM = 16;                       // output channels per block
constexpr int POLY_NW = 64;                       // windows per block (16 per wave)
constexpr int POLY_WP = 16 * POLY_BM + 16;        // LDS pitch of one input channel's 16 staged planes: + 16 puts the four channels of an A read on disjoint banks
constexpr int POLY_NSL = 6;                       // 64-element DMA slots per raw channel plane, at most
constexpr int POLY_LDS_MAX = 52 * 1024;           // three blocks per CU

struct PolyLaunch {
    int WTW, WTH;
    unsigned magic_tw, magic_iw;
    int tiles_x, tiles_y, mblocks, total;
    int IH, IW, nslots, plane, CK, stage_f;
};

template <int PAD, bool MASK>
__global__ __launch_bounds__(256, 3) void convt_poly_kernel(const l2i_conv_params p, const PolyLaunch L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // stage = [raw tile CK x plane | mask tile CK x plane (MASK) | weights CK x POLY_WP | input scales CK]
    const int in_f = L.CK * L.plane;
    const int w_off = in_f * (MASK ? 2 : 1), sc_off = w_off + L.CK * POLY_WP;

    const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, nl = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-aware block order (see l2i_conv.hip): the channel blocks of one window tile share an XCD and its L2
    int bid = (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3));
    if (bid >= L.total) return;
    const int mblk = bid % L.mblocks; bid /= L.mblocks;
    const int tx = bid % L.tiles_x; bid /= L.tiles_x;
    const int ty = bid % L.tiles_y;
    const int b = bid / L.tiles_y;
    const int m0 = mblk * POLY_BM;
    const int wy0 = ty * L.WTH, wx0 = tx * L.WTW;                 // tile origin in windows
    const int iy0 = 2 * wy0 - 1 + PAD, ix0 = 2 * wx0 - 1 + PAD;   // origin of the raw tile

    // this lane's window: B operand column and, after the loop, the owner of the output patch
    const int nwin = wave * 16 + nl;
    int wrow = (int)fast_div((unsigned)nwin, L.magic_tw), wcol = nwin - wrow * L.WTW;
    const bool used = wrow < L.WTH;                                // slots past WTH * WTW idle on window 0
    if (!used) { wrow = 0; wcol = 0; }
    const int pixoff = kq * L.plane + 2 * wrow * L.IW + 2 * wcol;
    const int wlane = kq * POLY_WP + nl;

    f32x4 acc[25];
#pragma unroll
    for (int q = 0; q < 25; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};

    const size_t plane_x = (size_t)p.H * p.W;
    const unsigned in_bytes = (unsigned)((size_t)p.Cin * plane_x * sizeof(float));                   // host: < 2^31
    const size_t smp_off = (size_t)b * p.Cin * plane_x;
    const __amdgpu_buffer_rsrc_t rs_x = l2i_buffer_rsrc(p.x + smp_off, in_bytes);
    const __amdgpu_buffer_rsrc_t rs_m = l2i_buffer_rsrc((MASK ? p.in_mask : p.x) + smp_off, in_bytes);
    const unsigned w_bytes = (unsigned)((size_t)p.Cin * 25 * p.CoutP * sizeof(float));
    const __amdgpu_buffer_rsrc_t rs_w = l2i_buffer_rsrc(p.w_lo, w_bytes);
    const __amdgpu_buffer_rsrc_t rs_s = l2i_buffer_rsrc((p.in_scale ? p.in_scale : p.x) + (size_t)b * p.Cin, p.in_scale ? (unsigned)(p.Cin * sizeof(float)) : 0u);

    // element e = 64 s + lane of a dense [IH][IW] channel plane -> byte offset inside the input plane, or out of range (reads zero)
    unsigned dvoff[POLY_NSL];
#pragma unroll
    for (int s = 0; s < POLY_NSL; ++s) {
        const unsigned e = (unsigned)(s * 64 + lane);
        const unsigned row = fast_div(e, L.magic_iw), ixu = e - row * L.IW;
        const int gy = iy0 + (int)row, gx = ix0 + (int)ixu;
        const bool ok = (s < L.nslots) & ((int)row < L.IH) & (gy >= 0) & (gy < p.H) & (gx >= 0) & (gx < p.W);
        dvoff[s] = ok ? (unsigned)(gy * p.W + gx) * 4u : 0x80000000u;
    }
    // weights: lane = (staged plane 4 a + b, four channels out) of one input channel; pack row 5 a + b
    const int wrow16 = lane >> 2;
    const unsigned wvoff = (unsigned)((((wrow16 >> 2) * 5 + (wrow16 & 3)) * p.CoutP + m0 + (lane & 3) * 4) * sizeof(float));
    const unsigned scoff = (tid < L.CK) ? (unsigned)(tid * sizeof(float)) : 0x80000000u;
    float rsc = 1.f;

    // a chunk's operands: wave w takes input channels w, w + 4, ...: one 1 KiB DMA of weights and nslots (x 2, MASK) DMAs of 256 bytes each
    auto dma = [&](int c0, int st) {
        const unsigned lds0 = l2i_lds_addr(smem + st * L.stage_f);
        for (int c = wave; c < L.CK; c += 4) {
            l2i_lds_dma16(wvoff, rs_w, __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((w_off + c * POLY_WP) * 4)),
                          (unsigned)((size_t)(c0 + c) * 25 * p.CoutP * sizeof(float)));
            const unsigned base = lds0 + (unsigned)(c * L.plane * 4);
            const unsigned so = (unsigned)((size_t)(c0 + c) * plane_x * sizeof(float));
#pragma unroll
            for (int s = 0; s < POLY_NSL; ++s) {
                if (s < L.nslots) {
                    l2i_lds_dma4(dvoff[s], rs_x, __builtin_amdgcn_readfirstlane(base + s * 256), so);
                    if constexpr (MASK) l2i_lds_dma4(dvoff[s], rs_m, __builtin_amdgcn_readfirstlane(base + (unsigned)(in_f * 4) + s * 256), so);
                }
            }
        }
        rsc = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_s, scoff, (unsigned)(c0 * sizeof(float)), 0));
    };
    auto store_sc = [&](int st) {
        if (tid < L.CK) smem[st * L.stage_f + sc_off + tid] = p.in_scale ? rsc : 1.f;
    };

    struct Frag { float a[16]; float r[9]; float m[MASK ? 9 : 1]; float sv; };
    auto load = [&](Frag& f, int st, int ks) {
        const float* lds_in = smem + st * L.stage_f;
        const float* wr = lds_in + w_off + ks * 4 * POLY_WP + wlane;
        const float* ir = lds_in + ks * 4 * L.plane + pixoff;
#pragma unroll
        for (int t = 0; t < 16; ++t) f.a[t] = wr[t * POLY_BM];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            f.r[t] = ir[(t / 3) * L.IW + (t % 3)];
            if constexpr (MASK) f.m[t] = ir[in_f + (t / 3) * L.IW + (t % 3)];
        }
        f.sv = lds_in[sc_off + ks * 4 + kq];
    };
    auto mfma = [&](const Frag& f) {
        float r[3][3];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            float v = f.r[t];
            if constexpr (MASK) v *= (f.m[t] > 0.f) ? p.mask_pos : p.mask_neg;
            r[t / 3][t % 3] = v * f.sv;
        }
        float R[4][3], T[4][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            R[0][c] = r[0][c] - r[1][c];
            R[1][c] = r[1][c];
            R[2][c] = r[1][c] - r[2][c];
            R[3][c] = PAD == 0 ? r[2][c] : r[0][c];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            T[a][0] = R[a][0] - R[a][1];
            T[a][1] = R[a][1];
            T[a][2] = R[a][1] - R[a][2];
            T[a][3] = PAD == 0 ? R[a][2] : R[a][0];
        }
        constexpr int bidx[5] = {0, 1, 2, PAD == 0 ? 1 : 3, PAD == 0 ? 3 : 1};
        constexpr int aidx[5] = {0, 1, 2, 3, 3};
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int c = 0; c < 5; ++c)
                acc[a * 5 + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[aidx[a] * 4 + aidx[c]], T[bidx[a]][bidx[c]], acc[a * 5 + c], 0, 0, 0);
    };

    // One set of fragment registers: each group of four channels is read from LDS and multiplied in turn (the reads hide behind the other blocks
    // of the CU, not behind this wave's own MFMAs).  The DMA of the next chunk goes into the other stage at the top of a chunk — every wave is
    // past the barrier that ended the chunk before, so nobody reads that stage — and is waited for (vmcnt(0)) after this chunk's MFMAs, before
    // the barrier that publishes it.  One barrier per chunk.
    const int nks = L.CK >> 2;
    dma(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    store_sc(0);
    __syncthreads();
    int st = 0;
    for (int c0 = 0; c0 < p.Cin; c0 += L.CK, st ^= 1) {
        const bool next = c0 + L.CK < p.Cin;
        if (next) dma(c0 + L.CK, st ^ 1);
        for (int ks = 0; ks < nks; ++ks) {
            Frag f;
            load(f, st, ks);
            mfma(f);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);
        if (next) store_sc(st ^ 1);
        __syncthreads();
    }

    // ---- epilogue: lane-local inverse transform, a 4x4 output patch per channel, 16 bytes per row ----
    if (!used) return;
    const int oy0 = 4 * (wy0 + wrow), ox0 = 4 * (wx0 + wcol);
    if (oy0 >= p.OHf || ox0 >= p.OWf) return;
    const size_t plane_o = (size_t)p.OHf * p.OWf;
    const float* osc = p.out_scale ? p.out_scale + (size_t)b * p.Cout : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = m0 + kq * 4 + r;
        if (co >= p.Cout) continue;
        float Yr[4][5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const float s01 = acc[0 * 5 + c][r] + acc[1 * 5 + c][r], d12 = acc[1 * 5 + c][r] - acc[2 * 5 + c][r];
            Yr[PAD == 0 ? 0 : 1][c] = s01;
            Yr[PAD == 0 ? 2 : 3][c] = d12;
            Yr[PAD == 0 ? 1 : 0][c] = acc[3 * 5 + c][r];
            Yr[PAD == 0 ? 3 : 2][c] = acc[4 * 5 + c][r];
        }
        float sc = p.out_gain;
        if (osc) sc *= osc[co];
        const bool scaled = osc || p.out_gain != 1.f;
        float* dst = p.y + ((size_t)b * p.Cout + co) * plane_o + (size_t)oy0 * p.OWf + ox0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float Y[4];
            Y[PAD == 0 ? 0 : 1] = Yr[i][0] + Yr[i][1];
            Y[PAD == 0 ? 2 : 3] = Yr[i][1] - Yr[i][2];
            Y[PAD == 0 ? 1 : 0] = Yr[i][3];
            Y[PAD == 0 ? 3 : 2] = Yr[i][4];
            if (scaled) { Y[0] *= sc; Y[1] *= sc; Y[2] *= sc; Y[3] *= sc; }
            if (oy0 + i < p.OHf) {
                float* d = dst + (size_t)i * p.OWf;
                if (ox0 + 3 < p.OWf) {
                    *reinterpret_cast<float4*>(d) = make_float4(Y[0], Y[1], Y[2], Y[3]);      // 4-byte aligned is enough on gfx950 (l2i_convt.hip)
                } else {
                    d[0] = Y[0];
                    if (ox0 + 1 < p.OWf) d[1] = Y[1];
                    if (ox0 + 2 < p.OWf) d[2] = Y[2];
                }
            }
        }
    }
}

unsigned magic_of(unsigned d) { return d == 1 ? 0u : (unsigned)((0x100000000ULL + d - 1) / d); }

// Shapes on which the per-launch A/B (profiles/convt_poly_ab.txt) shows convt_poly_kernel faster than convt_mfma_kernel beyond that A/B's own
// run-to-run spread: {pad, masked, Cin, Cout, H (= W)}.  tile_hint 0 takes the new kernel on these and the direct kernel everywhere else.
struct PolyRule { int pad, masked, cin, cout, h; };
constexpr PolyRule kPolyRules[] = {
    // the generator's up layers (forward form)
    {0, 0, 512, 512, 32}, {0, 0, 512, 256, 64}, {0, 0, 256, 128, 128}, {0, 0, 128, 64, 256}, {0, 0, 64, 32, 512},
    // The input gradients of the discriminator's stride-2 convs arrive UNMASKED on maps >= 32 wide (the FIR that produces the gradient writes it through
    // the leaky-ReLU mask as a second output, l2i_upfirdn2d_dual_f32) and have exactly the five shapes above, outputs three larger included: no row of
    // their own.  ResNet-50's three stride-2 bottlenecks arrive unmasked too (out_mask on c3's gradient GEMM), pad 1, natural size
    // (profiles/premask_stride2_ab.txt section 1: 0.74 - 0.78 of the direct kernel's time, both repetitions).  512 -> 512 @32 pad 1 wins there as well
    // (0.74) and is NOT listed: tests/test_convt_poly_cpu.py pins that struct to the direct kernel under tile_hint 0.
    {1, 0, 128, 128, 128}, {1, 0, 256, 256, 64},
    // No masked row: what still carries in_mask in the fp32 step (the deepest discriminator block, fed by the tail, and maps under 32 wide) is either too
    // narrow for this kernel or a single launch of a few microseconds.  tile_hint 10 runs a masked struct here.
};

}  // namespace

// The struct's launch plan (host only).  plan->eligible = 0 and the reason in l2i_last_error when the kernel does not take the struct.
extern "C" int l2i_convt_poly_plan_for(const l2i_conv_params* pp, l2i_convt_poly_plan* plan) {
    if (!pp || !plan) return l2i_set_error(L2I_E_ARG, "convt_poly_plan: null argument");
    const l2i_conv_params& p = *pp;
    memset(plan, 0, sizeof(*plan));
    const char* why = nullptr;
    if (p.KH != 3 || p.KW != 3 || p.pad_y != p.pad_x || (p.pad_y != 0 && p.pad_y != 1)) why = "convt_poly: 3x3, pad 0 or 1 only";
    else if (p.B <= 0 || p.Cin <= 0 || p.Cout <= 0 || p.H <= 0 || p.W <= 0) why = "convt_poly: non-positive dimension";
    else if (p.in_h8) why = "convt_poly: fp32 maps only";
    else if (p.ksplit > 1 && p.ws) why = "convt_poly: no split-K";
    else if (p.W < 32) why = "convt_poly: maps at least 32 positions wide";
    else if ((p.Cin % 4) != 0) why = "convt_poly: Cin must be a multiple of 4";
    else if (p.CoutP < p.Cout || (p.CoutP % 32) != 0) why = "convt_poly: CoutP must be Cout rounded up to 32";
    else if ((size_t)p.Cin * p.H * p.W * sizeof(float) >= 0x7FFF0000ull) why = "convt_poly: sample >= 2 GiB";
    else if ((size_t)p.Cin * 25 * p.CoutP * sizeof(float) >= 0xFFFFFFF0ull) why = "convt_poly: weight pack >= 4 GiB";
    else {
        const int full_h = (p.H - 1) * 2 - 2 * p.pad_y + 3, full_w = (p.W - 1) * 2 - 2 * p.pad_x + 3;
        if (p.OHf < full_h || p.OWf < full_w || p.OHf > full_h + 8 || p.OWf > full_w + 8) why = "convt_poly: output must be the natural size or up to 8 larger";
    }
    if (why) { l2i_set_error(L2I_E_UNSUPPORTED, why); return L2I_OK; }
    plan->masked = p.in_mask ? 1 : 0;
    plan->nwx = (p.OWf + 3) / 4;
    plan->nwy = (p.OHf + 3) / 4;
    // window tile: the WTW x WTH (<= 64 windows, raw tile <= 6 DMA slots) that covers the map with the fewest tiles, then the smallest raw tile
    long best = -1;
    for (int tw = 63; tw >= 4; --tw) {
        const int th = POLY_NW / tw;
        const int raw = (2 * th + 1) * (2 * tw + 1);
        if (raw > POLY_NSL * 64) continue;
        const long tiles = (long)((plan->nwx + tw - 1) / tw) * ((plan->nwy + th - 1) / th);
        const long cost = tiles * 4096 + raw;
        if (best < 0 || cost < best) { best = cost; plan->WTW = tw; plan->WTH = th; }
    }
    plan->tiles_x = (plan->nwx + plan->WTW - 1) / plan->WTW;
    plan->tiles_y = (plan->nwy + plan->WTH - 1) / plan->WTH;
    plan->mblocks = (p.Cout + POLY_BM - 1) / POLY_BM;             // (a block of nothing but channel padding is not launched)
    plan->IH = 2 * plan->WTH + 1;
    plan->IW = 2 * plan->WTW + 1;
    plan->org = p.pad_y - 1;
    plan->nslots = (plan->IH * plan->IW + 63) / 64;
    plan->plane = plan->nslots * 64 + 1;                          // odd pitch: the four channels of a B read start on different banks
    plan->wpitch = POLY_WP;
    const int per_c = plan->plane * (plan->masked ? 2 : 1) + POLY_WP + 1;
    int ck = (POLY_LDS_MAX / 2 / (int)sizeof(float) - 4) / per_c;
    // chunks must tile Cin exactly: the per-chunk channel offset travels in the scalar offset of the DMAs, which the hardware does not range-check
    ck &= ~3;
    if (ck > 16) ck = 16;
    if (ck > p.Cin) ck = p.Cin;
    while (ck > 4 && (p.Cin % ck) != 0) ck -= 4;
    if (ck < 4) { l2i_set_error(L2I_E_UNSUPPORTED, "convt_poly: tile cannot be staged"); return L2I_OK; }
    plan->CK = ck;
    plan->stage_floats = (ck * per_c + 3) & ~3;
    plan->lds_bytes = 2 * plan->stage_floats * (int)sizeof(float);
    const long total = (long)p.B * plan->tiles_y * plan->tiles_x * plan->mblocks;
    if (total <= 0 || total > 0x7ffffff0L) { l2i_set_error(L2I_E_UNSUPPORTED, "convt_poly: grid too large"); return L2I_OK; }
    plan->total = (int)total;
    plan->grid = (int)((total + 7) & ~7L);
    plan->eligible = 1;
    return L2I_OK;
}

bool l2i_convt_poly_eligible(const l2i_conv_params& p) {
    l2i_convt_poly_plan plan;
    return l2i_convt_poly_plan_for(&p, &plan) == L2I_OK && plan.eligible;
}

// tile_hint 0: the shapes of kPolyRules
bool l2i_convt_poly_preferred(const l2i_conv_params& p) {
    if (p.H != p.W) return false;
    for (const PolyRule& r : kPolyRules)
        if (r.pad == p.pad_y && r.masked == (p.in_mask ? 1 : 0) && r.cin == p.Cin && r.cout == p.Cout && r.h == p.H) return l2i_convt_poly_eligible(p);
    return false;
}

template <int PAD, bool MASK>
static int launch_poly(const l2i_conv_params& p, const l2i_convt_poly_plan& plan, hipStream_t st) {
    PolyLaunch L;
    L.WTW = plan.WTW; L.WTH = plan.WTH;
    L.magic_tw = magic_of((unsigned)plan.WTW);
    L.magic_iw = magic_of((unsigned)plan.IW);
    L.tiles_x = plan.tiles_x; L.tiles_y = plan.tiles_y; L.mblocks = plan.mblocks; L.total = plan.total;
    L.IH = plan.IH; L.IW = plan.IW; L.nslots = plan.nslots; L.plane = plan.plane; L.CK = plan.CK; L.stage_f = plan.stage_floats;
    L2I_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&convt_poly_kernel<PAD, MASK>), hipFuncAttributeMaxDynamicSharedMemorySize, POLY_LDS_MAX));
    hipLaunchKernelGGL((convt_poly_kernel<PAD, MASK>), dim3((unsigned)plan.grid), dim3(256), (size_t)plan.lds_bytes, st, p, L);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}

int l2i_launch_convt_poly(const l2i_conv_params& p, hipStream_t st) {
    l2i_convt_poly_plan plan;
    if (l2i_convt_poly_plan_for(&p, &plan) != L2I_OK || !plan.eligible) return L2I_E_UNSUPPORTED;      // (the reason is already recorded)
    if (!p.w_lo || (((uintptr_t)p.w_lo) % 16) != 0) return l2i_set_error(L2I_E_ARG, "convt_poly: w_lo must be the 16-byte aligned [Cin][25][CoutP] pack");
    if (plan.lds_bytes > POLY_LDS_MAX) return l2i_set_error(L2I_E_UNSUPPORTED, "convt_poly: tile cannot be staged");
    if (p.pad_y == 0) return p.in_mask ? launch_poly<0, true>(p, plan, st) : launch_poly<0, false>(p, plan, st);
    return p.in_mask ? launch_poly<1, true>(p, plan, st) : launch_poly<1, false>(p, plan, st);
}
