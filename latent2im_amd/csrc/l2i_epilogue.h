// l2i_epilogue.h — the one statement of the fp32 conv epilogue (include/l2i.h):
//   epi(a) = act( a*out_scale[b,co] * (out_mask > 0) + noise*noise_w + bias[co] + R * (res_mask > 0) ) * out_gain (+ y if accumulate)
//   R = residual, or res_coef * res_coef_dev[0] * (residual - res_sub) when res_sub is given; sq_out += sum (y - sq_ref)^2.
// It holds one small piece per term (epi_*), the two chains composed from them in the contract's order (l2i_epilogue_chain4 on four pixels of a
// channel, l2i_epilogue_chain1 on one value) and l2i_epilogue_32x32, the epilogue of the 32x32-accumulator kernels.  The chains are called by
// l2i_epilogue_32x32 (bf16-split kernels, stride-2 and small transposed kernels), by conv_mfma_kernel's epilogues A and B (l2i_conv.hip) and
// by gemm1x1_kernel, whose operand vectors are fetched ahead (l2i_epilogue_chain4_ops).  splitk_epilogue_kernel, l2i_wino.hip, both bodies
// of l2i_wino4.hip and l2i_cin3.hip compose the pieces themselves, each in its own grouping and instruction form (what
// differs and why).  The pieces take and return the running vector BY VALUE: by reference the compiler keeps it in memory form and the kernels change.
// Operand vectors that a caller loads under a test (l2i_epilogue_chain4_ops) come by const reference: by value the compiler splits each 16-byte
// load into four dword loads under the tests of its uses.
// Every kernel's composition of these terms is a route of tests/test_epilogue_contract_gpu.py: a new composition must be added there, where
// it is checked term by term against the float64 model of the contract.
// Against the inline copies (profiles/epilogue_share_asm.txt): registers, scratch, LDS and occupancy of every kernel are unchanged.
// Two sites keep their inline text for that.  (1) The scalar noise load `nz = noise[b*plane + pixel] * noise_w` of l2i_epilogue_32x32's scalar
// path and of conv_mfma_kernel's epilogue B: through a piece (four forms tried) the uniform base `noise + b*plane` is formed once per pixel
// row instead of once per tile, the WM = 1 callers then take 100 scalar registers for 98 and the WM = 2 callers spill two more scalars into
// vector lanes.  (2) The noise row of conv_mfma_kernel's epilogue A: through epi_noise4, conv_mfma_kernel<2,4,false,false> spills 57 scalars
// for 55 (every other caller of epi_noise4 is unchanged by it).
// Kept inline, not composed from these pieces: the lean classes of conv_wino4s_kernel (their stage order and fp-contract region are the
// specialisation), the scale-folded forms of l2i_conv16.hip / l2i_convt.hip, l2i_pair_f32.hip and the h8 epilogues (another contract).
#ifndef L2I_EPILOGUE_H
#define L2I_EPILOGUE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_device.h"

// ---- host: may the epilogue use 16-byte accesses? ----
static inline bool l2i_epilogue_operands_al16(const l2i_conv_params& p) {
    auto al16 = [](const void* q) { return (((uintptr_t)q) % 16) == 0; };
    return al16(p.y) && al16(p.residual) && al16(p.res_mask) && al16(p.res_sub) && al16(p.out_mask) && al16(p.noise);
}
static inline bool l2i_epilogue_vec_ok(const l2i_conv_params& p) {
    return p.ox_step == 1 && p.oy_step == 1 && (p.OWf % 4) == 0 && (p.OW % 4) == 0 && (p.ox_off % 4) == 0 && l2i_epilogue_operands_al16(p);
}

// ---- the terms, on four consecutive pixels of one channel (float4) or on one value (float) ----
__device__ __forceinline__ float4 epi_ld4(const float* q) { return *reinterpret_cast<const float4*>(q); }
__device__ __forceinline__ float4 epi_mul(float4 v, float s) { v.x *= s; v.y *= s; v.z *= s; v.w *= s; return v; }   // out_scale, noise_w, out_gain
__device__ __forceinline__ float4 epi_add(float4 v, float s) { v.x += s; v.y += s; v.z += s; v.w += s; return v; }   // bias
__device__ __forceinline__ float4 epi_add(float4 v, float4 a) { v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w; return v; }
// out_mask / res_mask: the value where the mask is positive, else 0
__device__ __forceinline__ float epi_keep(float v, float mk) { return mk > 0.f ? v : 0.f; }
__device__ __forceinline__ float4 epi_keep(float4 v, float4 mk) { return make_float4(epi_keep(v.x, mk.x), epi_keep(v.y, mk.y), epi_keep(v.z, mk.z), epi_keep(v.w, mk.w)); }
// noise * noise_w at element idx of the noise planes.  One value: the caller tests p.noise.  Four pixels: 0 without noise or where `on` is false
__device__ __forceinline__ float epi_noise(const l2i_conv_params& p, size_t idx) { return p.noise[idx] * p.noise_w; }
__device__ __forceinline__ float4 epi_noise4(const l2i_conv_params& p, bool on, size_t idx) {
    float4 nz = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on && p.noise) {                                       // (field by field: a vector assigned from a call under a branch stays an aggregate in the IR)
        nz = epi_ld4(p.noise + idx);
        nz.x *= p.noise_w; nz.y *= p.noise_w; nz.z *= p.noise_w; nz.w *= p.noise_w;
    }
    return nz;
}
// residual term R * (res_mask > 0); rc = epi_rc(p) is only read with res_sub, so a caller may hoist it (and pass anything without res_sub).
// The form that reads rc itself is the chains': hoisted out of them it costs the 32x32 kernels a register and ~45 instructions
__device__ __forceinline__ float epi_rc(const l2i_conv_params& p) { return p.res_coef * (p.res_coef_dev ? p.res_coef_dev[0] : 1.f); }
__device__ __forceinline__ float4 epi_res_sub(float4 rv, float4 sb, float rc) {
    return make_float4(rc * (rv.x - sb.x), rc * (rv.y - sb.y), rc * (rv.z - sb.z), rc * (rv.w - sb.w));
}
__device__ __forceinline__ float4 epi_residual(const l2i_conv_params& p, float4 rv, const float4& sb, const float4& rm, float rc) {   // operands already loaded
    if (p.res_sub) rv = epi_res_sub(rv, sb, rc);
    if (p.res_mask) rv = epi_keep(rv, rm);
    return rv;
}
__device__ __forceinline__ float4 epi_residual(const l2i_conv_params& p, size_t oidx, float rc) {   // rc hoisted by the caller
    float4 rv = epi_ld4(p.residual + oidx);
    if (p.res_sub) rv = epi_res_sub(rv, epi_ld4(p.res_sub + oidx), rc);
    if (p.res_mask) rv = epi_keep(rv, epi_ld4(p.res_mask + oidx));
    return rv;
}
__device__ __forceinline__ float4 epi_residual(const l2i_conv_params& p, size_t oidx) {             // rc read here, under res_sub
    float4 rv = epi_ld4(p.residual + oidx);
    if (p.res_sub) rv = epi_res_sub(rv, epi_ld4(p.res_sub + oidx), epi_rc(p));
    if (p.res_mask) rv = epi_keep(rv, epi_ld4(p.res_mask + oidx));
    return rv;
}
__device__ __forceinline__ float epi_residual1(const l2i_conv_params& p, size_t oidx) {
    float rv = p.residual[oidx];
    if (p.res_sub) rv = epi_rc(p) * (rv - p.res_sub[oidx]);
    if (p.res_mask) rv = epi_keep(rv, p.res_mask[oidx]);
    return rv;
}
// activation.  Select form: v > 0 ? v : slope v.  fmaxf form: max(v, slope v), the same value for 0 <= slope <= 1 and finite v; the two differ for NaN
// and in the sign of a zero, so a kernel keeps the form it has.
__device__ __forceinline__ float epi_lrelu_select(float v, float slope, float gain) { return (v > 0.f ? v : v * slope) * gain; }
__device__ __forceinline__ float epi_relu_select(float v) { return v > 0.f ? v : 0.f; }
__device__ __forceinline__ float epi_lrelu_fmax(float v, float slope, float gain) { return __builtin_fmaxf(v, v * slope) * gain; }
__device__ __forceinline__ float epi_relu_fmax(float v) { return __builtin_fmaxf(v, 0.f); }
__device__ __forceinline__ float4 epi_lrelu_select(float4 v, float s, float g) { return make_float4(epi_lrelu_select(v.x, s, g), epi_lrelu_select(v.y, s, g), epi_lrelu_select(v.z, s, g), epi_lrelu_select(v.w, s, g)); }
__device__ __forceinline__ float4 epi_relu_select(float4 v) { return make_float4(epi_relu_select(v.x), epi_relu_select(v.y), epi_relu_select(v.z), epi_relu_select(v.w)); }
__device__ __forceinline__ float4 epi_lrelu_fmax(float4 v, float s, float g) { return make_float4(epi_lrelu_fmax(v.x, s, g), epi_lrelu_fmax(v.y, s, g), epi_lrelu_fmax(v.z, s, g), epi_lrelu_fmax(v.w, s, g)); }
__device__ __forceinline__ float4 epi_relu_fmax(float4 v) { return make_float4(epi_relu_fmax(v.x), epi_relu_fmax(v.y), epi_relu_fmax(v.z), epi_relu_fmax(v.w)); }
template <typename T>
__device__ __forceinline__ T epi_act_select(const l2i_conv_params& p, T v, bool relu_by_fmax = false) {   // (relu_by_fmax: l2i_cin3.hip's mix of the forms)
    if (p.act == L2I_ACT_LRELU) return epi_lrelu_select(v, p.act_slope, p.act_gain);
    if (p.act == L2I_ACT_RELU) return relu_by_fmax ? epi_relu_fmax(v) : epi_relu_select(v);
    return v;
}
__device__ __forceinline__ float4 epi_act_fmax(const l2i_conv_params& p, float4 v) {
    if (p.act == L2I_ACT_LRELU) return epi_lrelu_fmax(v, p.act_slope, p.act_gain);
    if (p.act == L2I_ACT_RELU) return epi_relu_fmax(v);
    return v;
}
__device__ __forceinline__ float4 epi_gain(const l2i_conv_params& p, float4 v) { return p.out_gain != 1.f ? epi_mul(v, p.out_gain) : v; }
__device__ __forceinline__ float4 epi_accumulate(const l2i_conv_params& p, float4 v, size_t oidx) { return p.accumulate ? epi_add(v, epi_ld4(p.y + oidx)) : v; }
// sq_ref: ContentLoss value of a VGG tap, sum (y - reference)^2 while y is in registers.  epi_sq: one vector's term; epi_sq_commit: the block's sum
// (all 256 threads call it, under the uniform test of p.sq_ref) -> one atomic per block into L2I_SQ_SLOTS slots, through four LDS words at `lds`
// that the block is done with.
__device__ __forceinline__ float epi_sq(const l2i_conv_params& p, float4 v, size_t oidx) {
    const float4 rf = epi_ld4(p.sq_ref + oidx);
    const float d0 = v.x - rf.x, d1 = v.y - rf.y, d2 = v.z - rf.z, d3 = v.w - rf.w;
    return (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
}
__device__ __forceinline__ void epi_sq_commit(const l2i_conv_params& p, float sq, float* lds) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
    __syncthreads();                                           // every wave is done with what `lds` held
    if (lane == 0) lds[wave] = sq;
    __syncthreads();
    if (tid == 0) atomicAdd(p.sq_out + (blockIdx.x & (L2I_SQ_SLOTS - 1)), (lds[0] + lds[1]) + (lds[2] + lds[3]));
}
// one 32x32 accumulator (register r = channel (r & 3) + 8 (r >> 2) + 4 half, lane & 31 = pixel j) -> pixel columns q*32 .. q*32+31 of a wave's
// [32 channels][64 pixels] transpose strip
__device__ __forceinline__ void epi_strip_store(float* reg, int half, int j, int q, f32x16 a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) reg[((r & 3) + 8 * (r >> 2) + 4 * half) * 64 + q * 32 + j] = a[r];
}

// ---- the chains: the terms in the contract's order.  osc = out_scale row of the sample (or null), nz = epi_noise4 / epi_noise of the pixels ----
// on operand values: om / rv / sb / rm / yo = out_mask, residual, res_sub, res_mask, old y at oidx (each only read when the operand exists)
__device__ __forceinline__ float4 l2i_epilogue_chain4_ops(const l2i_conv_params& p, float4 v, const float* osc, float4 nz, int co, const float4& om, float4 rv,
                                                          const float4& sb, const float4& rm, const float4& yo, float rc) {
    if (osc) v = epi_mul(v, osc[co]);
    if (p.out_mask) v = epi_keep(v, om);
    if (p.noise) v = epi_add(v, nz);
    if (p.bias) v = epi_add(v, p.bias[co]);
    if (p.residual) v = epi_add(v, epi_residual(p, rv, sb, rm, rc));
    v = epi_gain(p, epi_act_select(p, v));
    if (p.accumulate) v = epi_add(v, yo);
    return v;
}
__device__ __forceinline__ float4 l2i_epilogue_chain4(const l2i_conv_params& p, float4 v, const float* osc, float4 nz, int co, size_t oidx) {
    if (osc) v = epi_mul(v, osc[co]);
    if (p.out_mask) v = epi_keep(v, epi_ld4(p.out_mask + oidx));
    if (p.noise) v = epi_add(v, nz);
    if (p.bias) v = epi_add(v, p.bias[co]);
    if (p.residual) v = epi_add(v, epi_residual(p, oidx));
    return epi_accumulate(p, epi_gain(p, epi_act_select(p, v)), oidx);
}
// one value; nz is added unconditionally (0 without noise), out_gain multiplied unconditionally
__device__ __forceinline__ float l2i_epilogue_chain1(const l2i_conv_params& p, float v, const float* osc, float nz, int co, size_t oidx) {
    if (osc) v *= osc[co];
    if (p.out_mask) v = epi_keep(v, p.out_mask[oidx]);
    v += nz;
    if (p.bias) v += p.bias[co];
    if (p.residual) v += epi_residual1(p, oidx);
    v = epi_act_select(p, v) * p.out_gain;
    if (p.accumulate) v += p.y[oidx];
    return v;
}

// ---- the epilogue of the 32x32-accumulator kernels.  Accumulator layout: wave w of the block owns output rows oy0 + w*WN + n (n < WN), 32 columns
// from ox0; acc[m][n][r] = channel m0 + 32 m + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), pixel lane & 31.  vec = true: per-wave LDS transpose (8 KiB
// strip per wave at `smemf`) -> 16-byte global accesses ----
template <int WM, int WN>
__device__ __forceinline__ void l2i_epilogue_32x32(const l2i_conv_params& p, f32x16 (&acc)[WM][WN], float* smemf, int b, int m0, int oy0, int ox0, bool vec) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, j = lane & 31;
    const size_t plane_o = (size_t)p.OHf * p.OWf;
    if (vec) {
        float sq = 0.f;
        float* reg = smemf + wave * (32 * 64);
        const int ch_l = lane >> 4;
        const int px = (lane & 15) * 4;
#pragma unroll
        for (int n0 = 0; n0 < WN; n0 += 2) {
            const int nn = px >> 5;
            const int oy = oy0 + wave * WN + n0 + nn;
            const int ox = ox0 + (px & 31);
            const bool pok = (n0 + nn < WN) && (oy < p.OH) && (ox < p.OW);
            const size_t poff = (size_t)(oy + p.oy_off) * p.OWf + ox + p.ox_off;
            const float4 nz = epi_noise4(p, pok, (size_t)b * plane_o + poff);
            const float* osc = (pok && p.out_scale) ? p.out_scale + (size_t)b * p.Cout : nullptr;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    if (n0 + q < WN) epi_strip_store(reg, half, j, q, acc[m][(n0 + q) < WN ? (n0 + q) : 0]);
#pragma unroll 2
                for (int i = 0; i < 8; ++i) {
                    const int ch = i * 4 + ch_l;
                    const int co = m0 + m * 32 + ch;
                    const float4 t = *reinterpret_cast<const float4*>(&reg[ch * 64 + px]);
                    if (pok && co < p.Cout) {
                        const size_t oidx = ((size_t)b * p.Cout + co) * plane_o + poff;
                        const float4 v = l2i_epilogue_chain4(p, t, osc, nz, co, oidx);
                        *reinterpret_cast<float4*>(p.y + oidx) = v;
                        if (p.sq_ref) sq += epi_sq(p, v, oidx);
                    }
                }
            }
        }
        if (p.sq_ref) epi_sq_commit(p, sq, smemf);             // (after its first barrier every wave is done with its transpose strip)
        return;
    }
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int oy = oy0 + wave * WN + n, ox = ox0 + j;
        const bool pok = (oy < p.OH) && (ox < p.OW);
        const size_t poff = (size_t)(oy * p.oy_step + p.oy_off) * p.OWf + ox * p.ox_step + p.ox_off;
        float nz = 0.f;
        if (pok && p.noise) nz = p.noise[(size_t)b * plane_o + poff] * p.noise_w;     // (inline: see the head of this file)
        const int co_lane = m0 + 4 * half;
        const size_t lane_base = ((size_t)b * p.Cout + co_lane) * plane_o + poff;
        const float* osc = p.out_scale ? p.out_scale + (size_t)b * p.Cout : nullptr;
#pragma unroll
        for (int m = 0; m < WM; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cofs = m * 32 + (r & 3) + 8 * (r >> 2);
                const int co = co_lane + cofs;
                if (pok && co < p.Cout) {
                    const size_t oidx = lane_base + (size_t)cofs * plane_o;
                    p.y[oidx] = l2i_epilogue_chain1(p, acc[m][n][r], osc, nz, co, oidx);
                }
            }
        }
    }
}
#endif
