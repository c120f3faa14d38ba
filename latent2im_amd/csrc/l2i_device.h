// l2i_device.h — the device primitives every kernel file shares (gfx950): vector types, buffer descriptors and LDS addresses, the LDS-DMA
// statements, the 16-bit element converts of the h8 layout, packed fp32 VALU, wave / block sums and the magic-number division.  Device code
// only: l2i_internal.h is the host-side launch header.  The hardware rules these helpers obey (M0 around a DMA, the s_nop after s_mov m0, no
// half selection on src1 of a packed fp32 instruction, the wait states between a VALU result and the MFMA that reads it) are stated here once.
#ifndef L2I_DEVICE_H
#define L2I_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- vector types ---------------------------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// Eight 16-bit elements, one MFMA fragment.  The h8 files are compiled twice (csrc/Makefile): as is = bf16 elements, and with -DL2I_H8_F16 =
// IEEE fp16 elements; everything else is built for bf16 only.
#ifdef L2I_H8_F16
constexpr bool L2I_H8_ELEM_F16 = true;
typedef _Float16 bf16x8 __attribute__((ext_vector_type(8)));          // (the fragment type keeps its name: "bf16x8" = eight 16-bit elements)
#else
constexpr bool L2I_H8_ELEM_F16 = false;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#endif

// ---- buffer descriptor, LDS byte address ----------------------------------------------------------------------------------------------
// Raw buffer of `bytes` bytes at `base` (stride 0: offsets are byte offsets, an offset >= bytes reads zeros and writes nothing).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t l2i_buffer_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ unsigned l2i_lds_addr(const void* lds_ptr) {
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds_ptr;
}

// ---- LDS-DMA: global -> LDS without registers -----------------------------------------------------------------------------------------
// buffer_load_dwordx4 ... lds: lane l of the wave lands at M0 base + 16 l (buffer_load_dword: + 4 l); `lds_addr` and `soff` are wave-uniform
// (callers pass readfirstlane of the address).  Inline asm on purpose: through the builtin, hipcc cannot tell the DMA's LDS target from the
// stage being read and drains vmcnt before the next ds_read; the waits (s_waitcnt vmcnt before the publishing barrier) are the caller's.  M0 is
// saved and restored around the instruction, and the s_nop covers the hazard between s_mov m0 and the instruction that reads it.
// FENCE: the statement carries a "memory" clobber.  l2i_gemm.hip and l2i_wino.hip were written without one (FENCE = false) and order their DMAs
// against the LDS reads by hand; each kernel keeps the form it was measured with until both are shown to assemble alike.
template <bool FENCE = true>
__device__ __forceinline__ void l2i_lds_dma16(unsigned voff, __amdgpu_buffer_rsrc_t rsrc, unsigned lds_addr, unsigned soff) {
    unsigned keep;
#define L2I_LDS_DMA16_TEXT "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
    if constexpr (FENCE) asm volatile(L2I_LDS_DMA16_TEXT : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff) : "memory");
    else asm volatile(L2I_LDS_DMA16_TEXT : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff));
#undef L2I_LDS_DMA16_TEXT
}
// one dword per lane (l2i_wino.hip's raw halo tile), no "memory" clobber
__device__ __forceinline__ void l2i_lds_dma4(unsigned voff, __amdgpu_buffer_rsrc_t rsrc, unsigned lds_addr, unsigned soff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff));
}

// ---- 16-bit elements of the h8 layout -------------------------------------------------------------------------------------------------
// The packing convert (v_cvt_pk_{bf16,f16}_f32: one instruction per pair, round to nearest even, both) and the two unpack converts.  F16 defaults
// to the translation unit's element type (l2i_h8_common.h).  [r5] The forms with a run-time flag: 16-bit elements of the h8 layout inside fp32
// translation units (`f16`: IEEE fp16, else bf16): l2i_convt_small.hip (in_h8), l2i_img_h8.hip.
template <bool F16 = L2I_H8_ELEM_F16>
__device__ __forceinline__ unsigned h8_pk(float lo, float hi) {
    unsigned r;
    if constexpr (F16) asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    else asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
template <bool F16 = L2I_H8_ELEM_F16>
__device__ __forceinline__ float h8_lo(unsigned u) {
    float r;
    if constexpr (F16) asm("v_cvt_f32_f16 %0, %1" : "=v"(r) : "v"(u));
    else r = __uint_as_float(u << 16);
    return r;
}
template <bool F16 = L2I_H8_ELEM_F16>
__device__ __forceinline__ float h8_hi(unsigned u) {
    float r;
    if constexpr (F16) asm("v_cvt_f32_f16_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(r) : "v"(u));
    else r = __uint_as_float(u & 0xffff0000u);
    return r;
}
__device__ __forceinline__ unsigned h8_pk(float lo, float hi, bool f16) { return f16 ? h8_pk<true>(lo, hi) : h8_pk<false>(lo, hi); }
__device__ __forceinline__ float h8_lo(unsigned u, bool f16) { return f16 ? h8_lo<true>(u) : h8_lo<false>(u); }
__device__ __forceinline__ float h8_hi(unsigned u, bool f16) { return f16 ? h8_hi<true>(u) : h8_hi<false>(u); }
// one 16-byte pixel slot <-> its eight channels
__device__ __forceinline__ void h8_unpack(const u32x4& u, float (&v)[8]) {
    v[0] = h8_lo(u.x); v[1] = h8_hi(u.x); v[2] = h8_lo(u.y); v[3] = h8_hi(u.y);
    v[4] = h8_lo(u.z); v[5] = h8_hi(u.z); v[6] = h8_lo(u.w); v[7] = h8_hi(u.w);
}
__device__ __forceinline__ u32x4 h8_pack(const float (&v)[8]) { return u32x4{h8_pk(v[0], v[1]), h8_pk(v[2], v[3]), h8_pk(v[4], v[5]), h8_pk(v[6], v[7])}; }

// ---- packed fp32 VALU -----------------------------------------------------------------------------------------------------------------
// Packed fp32 VALU (two independent lanes of work per issue slot).  Inline asm because hipcc scalarises most f32x2
// arithmetic (and cannot see hazards inside asm: see pk_mul_op).  [r3] A/B against the same arithmetic as two single-lane
// v_add / v_sub / v_mul per packed instruction (one asm statement each, so that the SLP vectoriser cannot re-pack them), interleaved in one
// process on fifteen launch shapes of the step: the single-lane build is 1.2 - 6.4 % SLOWER on every shape.  Packed stays.
// Half selections sit on SRC0 (or in op_sel_hi), never on src1: packed fp32 with op_sel set on
// src1 (what hipcc's SLP vectorizer emits) returns sporadically wrong results while a bf16-MFMA kernel is resident
// on the same CUs; op_sel on src0, op_sel_hi and plain operands do not (tools/probes/pk_beside_conv_h8.py).  Every
// half-selecting form a kernel file adds (l2i_wino.hip: pk_lo_pm_hi, l2i_wino4.hip: w4_fmak_lo / _hi, w4_lo_pm_lo_op) is bound by this.
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) { f32x2 r; asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) { f32x2 r; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ f32x2 pk_mul(f32x2 a, f32x2 b) { f32x2 r; asm("v_pk_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// pk_mul_op: the product feeds an MFMA next, the 2 wait states of "VALU write -> MFMA read" ride in the same asm statement
__device__ __forceinline__ f32x2 pk_mul_op(f32x2 a, f32x2 b) { f32x2 r; asm("v_pk_mul_f32 %0, %1, %2\n\ts_nop 1" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ f32x2 pk_sub_op(f32x2 a, f32x2 b) {
    f32x2 r; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]\n\ts_nop 1" : "=v"(r) : "v"(a), "v"(b)); return r;
}

// ---- reductions, integer helpers ------------------------------------------------------------------------------------------------------
// wave64 sum: wave_sum leaves the total in lane 0 (shuffle down), wave_sum_all in every lane (butterfly)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// sum over a 256-thread block through four words of LDS at `red`, in every thread
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {             // fixed order: deterministic
    v = wave_sum_all(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// wave64 / 256-thread block maximum in every thread, the same way (l2i_range.hip: the largest magnitude of a map, as an unsigned bit pattern)
template <typename T>
__device__ __forceinline__ T wave_max_all(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T block_max(T v, T* red) {
    v = wave_max_all(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const T a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}
__device__ __forceinline__ unsigned fast_div(unsigned n, unsigned magic) { return magic ? __umulhi(n, magic) : n; }   // magic 0 encodes d == 1; else ceil(2^32 / d)

// ---- image quantisation ---------------------------------------------------------------------------------------------------------------
// clip_ims in float32 with numpy's operation order (x + 1, / 2, * 255; / 2 is exact), np.clip, then the truncating uint8 cast (l2i_face.hip: the
// face resize reads its pixels through it; l2i_panels.hip: the panel grids)
__device__ __forceinline__ int quant8(float v) {
    float t = __fmul_rn(__fmul_rn(__fadd_rn(v, 1.0f), 0.5f), 255.0f);
    t = fminf(fmaxf(t, 0.0f), 255.0f);          // (NaN -> 0)
    return (int)t;
}

#endif
