/*
 * l2i.h — C ABI of libl2i_hip.so: the hand-written gfx950 (MI355X / CDNA4) kernels behind the Latent2im
 * walk-training hot path.
 *
 * Drop-in boundary.  The reference's only native code is two pybind/CUDA extensions that are JIT-built at
 * import (graphs/stylegan_v2_real/op/fused_act.py:10-16, op/upfirdn2d.py:9-15).  The entry points below are
 * what an FFI for this path binds instead:
 *
 *   l2i_fused_bias_act_f32   replaces  fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)
 *                                      op/fused_bias_act.cpp:11-21, op/fused_bias_act_kernel.cu:18-98
 *   l2i_upfirdn2d_f32        replaces  upfirdn2d_op.upfirdn2d(input, kernel, up_x, up_y, down_x, down_y,
 *                                      pad_x0, pad_x1, pad_y0, pad_y1)
 *                                      op/upfirdn2d.cpp:12-23, op/upfirdn2d_kernel.cu:140-272
 *   l2i_conv2d_f32           replaces  the F.conv2d(groups=batch) / F.conv_transpose2d(groups=batch) /
 *                                      weight-materialisation sequence of ModulatedConv2d.forward
 *                                      (networks.py:231-272), EqualConv2d.forward (networks.py:111-120) and the
 *                                      torchvision ResNet-50 / VGG-19 conv(+BN eval)+ReLU blocks called at
 *                                      transform_base.py:396-403,416-454, and their input-gradients
 *   l2i_torgb_* / l2i_sg2_act_bwd_f32 / l2i_dot_reduce_f32 / l2i_maxpool2d_* / l2i_sqdiff_f32
 *                            the streaming (HBM-bound) companions of the above on the same path:
 *                            ToRGB (networks.py:339-358), lrelu backward + style-gradient reductions,
 *                            MaxPool2d of ResNet/VGG, ContentLoss (transform_base.py:57-63).
 *
 * Conventions: every pointer is a DEVICE pointer to contiguous float32 (NCHW for maps); the caller owns all
 * buffers (nothing is allocated here); `stream` is a hipStream_t passed as void*; kernels are enqueued
 * asynchronously; return value 0 = enqueued, negative = L2I_E_* (nothing enqueued).  Thread-safe for distinct
 * streams.  No torch types anywhere in this ABI.
 */
#ifndef L2I_H
#define L2I_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L2I_OK 0
#define L2I_E_ARG (-1)      /* invalid argument combination */
#define L2I_E_LAUNCH (-2)   /* hipLaunch failed (see l2i_last_error) */
#define L2I_E_UNSUPPORTED (-3)

#define L2I_ACT_NONE 0
#define L2I_ACT_LRELU 1     /* y = (v > 0 ? v : v*slope) * gain */
#define L2I_ACT_RELU 2

/* Generic 2-D correlation as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).
 *   y[b,co,oy*oy_step+oy_off,ox*ox_step+ox_off] = epi( sum_{ci,ky,kx} pro(x)[b,ci,oy*stride-pad_y+ky,ox*stride-pad_x+kx]
 *                                                       * w[ci][ky*KW+kx][co] )     for oy<OH, ox<OW
 *   pro(x) = x * in_scale[b,ci] * (in_mask ? (in_mask[same idx] > 0 ? mask_pos : mask_neg) : 1)
 *   epi(a) = act( a*out_scale[b,co] * (out_mask ? (out_mask[idx] > 0 ? 1 : 0) : 1) + noise[b,oyf,oxf]*noise_w + bias[co]
 *                 + R * (res_mask ? (res_mask[idx] > 0 ? 1 : 0) : 1) ) * out_gain  (+ y[idx] if accumulate)
 *   R = res_sub ? res_coef * res_coef_dev[0] * (residual[idx] - res_sub[idx]) : residual[idx]
 * Out-of-range input coordinates read as zero (that is the padding).  Transposed (stride-2) convolutions are issued
 * as one call per output phase with (oy_step, ox_step) = 2 and a per-phase packed sub-kernel. */
typedef struct l2i_conv_params {
    const float* x;         /* [B, Cin, H, W] */
    const float* w;         /* packed [Cin][KH*KW][CoutP], CoutP = Cout rounded up to 32, zero padded */
    float* y;               /* [B, Cout, OHf, OWf] */
    int32_t B, Cin, H, W, Cout, CoutP;
    int32_t KH, KW, stride, pad_y, pad_x;
    int32_t OH, OW, OHf, OWf;
    int32_t oy_step, ox_step, oy_off, ox_off;
    const float* in_scale;  /* [B, Cin] or NULL */
    const float* in_mask;   /* like x, or NULL */
    float mask_pos, mask_neg;
    const float* out_scale; /* [B, Cout] or NULL */
    const float* noise;     /* [B, 1, OHf, OWf] or NULL */
    float noise_w;
    const float* bias;      /* [Cout] or NULL */
    const float* residual;  /* like y, or NULL */
    const float* res_mask;  /* like y, or NULL */
    const float* out_mask;  /* like y, or NULL */
    int32_t act;
    float act_slope, act_gain, out_gain;
    int32_t accumulate;
    int32_t tile_hint;      /* 0 = auto, else 1..N selects a tile configuration (tuning / tests) */
    const void* w_hi;       /* l2i_conv2d_bf16x3_f32 only: bf16 planes [Cin/16][KH*KW][CoutP][2][8], hi = bf16(w), */
    const void* w_lo;       /*                              lo = bf16(w - hi); NULL for the fp32 entry points, except l2i_conv_transpose2d_f32 with K = 3: */
                            /*                              fp32 [Cin][25][CoutP], the 25-plane pack of its 25-product kernel (see there), or NULL      */
    float* ws;              /* l2i_conv2d_f32 split-K workspace: ksplit * B*Cout*OHf*OWf floats, or NULL */
    int32_t ksplit;         /* > 1: the input channels are cut into ksplit ranges computed by separate blocks (raw partial sums in ws),
                               then one reduction pass applies the epilogue: for 4x4..16x16 maps, whose whole K = Cin*KH*KW would
                               otherwise be walked serially by a dozen blocks.  0 / 1: off. */
    const float* res_sub;   /* like y, or NULL.  Not NULL: the residual term becomes res_coef * res_coef_dev[0] * (residual - res_sub) — the */
    float res_coef;         /* ContentLoss gradient 2/N * g * (feat - feat_org) of a VGG tap (transform_base.py:57-63) formed inside the     */
    const float* res_coef_dev;  /* gradient conv that consumes it, instead of a separate pass.  res_coef_dev: 1 float on the device or NULL */
    const float* sq_ref;    /* like y, or NULL.  Not NULL (l2i_conv2d_wino_f32, l2i_conv2d_bf16x3_f32 with dense 16-byte output rows, and launches */
                            /* of l2i_conv2d_f32 that take the <= 3-input-channel kernel, L2I_FAMILY_CIN3; everything else refuses it): the launch */
                            /* also adds                                                                                                          */
    float* sq_out;          /* sum (y - sq_ref)^2 over its outputs into sq_out[0 .. L2I_SQ_SLOTS-1] (fp32 atomics, one slot per block id mod   */
                            /* L2I_SQ_SLOTS; the caller zeroes the slots and sums them): the ContentLoss value of a VGG tap                  */
                            /* (transform_base.py:57-63, mse = the sum / N) without re-reading the feature map in a separate pass             */
    int64_t w_bstride;      /* l2i_conv2d_h8 / l2i_conv_transpose2d_h8: bytes between the weight planes of consecutive samples (the generator's */
                            /* modulated convs: style and demodulation folded into one plane set per sample), 0 = one set for every sample    */
    int32_t out_f32;        /* l2i_conv2d_h8: 1 = the output (and residual / res_mask / out_mask / res_sub) is fp32 NCHW instead of bf16 h8      */
    /* ---- ABI version 5: fp32 <-> 16-bit boundaries of the 16-bit path without a cast pass (see also l2i_conv_img_h8) ------------------------- */
    int32_t in_h8;          /* l2i_conv_transpose2d_f32, 7x7 / pad 3 onto <= 3 channels (the ResNet stem's input gradient): 1 / 2 = x and in_mask are      */
                            /* bf16 / fp16 h8 tensors [B, Cin/8, H, W, 8] (Cin % 8 == 0)                                                                  */
    const float* rgb_w;     /* l2i_conv2d_h8 with the h8 output and every output channel in one block (Cout = 32 or 64): not NULL = the launch also writes the   */
    const float* rgb_bias;  /* ToRGB image of its output, rgb_out[b, o, oy, ox] = rgb_bias[o] + sum_c rgb_w[b, o, c] * epi(.)[b, c, oy, ox] (o < 3; fp32     */
    float* rgb_out;         /* NCHW [B, 3, OHf, OWf]; networks.py:349-358 on the 512^2 / 1024^2 StyledConv outputs), instead of a pass that re-reads y        */
    float* pool_out;        /* l2i_conv2d_wino4_f32 (position-split kernel, dense output with even OHf, OWf % 4 == 0, zero output offsets): not NULL = the launch    */
    uint8_t* pool_idx;      /* also writes MaxPool2d(2, 2) of its output y, pool_out [B, Cout, OHf/2, OWf/2] fp32 and the window-local arg-max pool_idx (same     */
                            /* shape, bytes; taps in (ky, kx) order, first maximum, NaN propagates: l2i_maxpool2d_fwd_f32's rule) — VGG-19's pool after conv1_2   */
                            /* (transform_base.py:426-454) from the 4x4 output tile a lane holds anyway, instead of a pass that reads the 2 GB map again          */
    /* ---- ABI version 6: one-bit activation masks on the 16-bit path (l2i_conv2d_h8 / l2i_conv_transpose2d_h8) ------------------------------------------- */
    uint8_t* mask_out;      /* h8 output: not NULL = the launch also writes the SIGN PLANE of its output, one byte per 16-byte pixel slot:                              */
                            /* mask_out[((b * Cout/8 + g) * OHf + oy) * OWf + ox] bit e = (the stored 16-bit y[b, 8 g + e, oy, ox] > 0).  The input-gradient launches of   */
                            /* a frozen ReLU network need exactly this bit of every saved activation (torchvision's bottleneck relu(bn(conv)) called at                   */
                            /* transform_base.py:396-403,416-424), and read it at 1/16 of the map's bytes                                                                 */
    int32_t mask_bits;      /* 1 = out_mask / res_mask point to such sign planes ([B, Cout/8, OHf, OWf] bytes) instead of h8 maps shaped like y                           */
} l2i_conv_params;
#define L2I_SQ_SLOTS 1024

int l2i_conv2d_f32(const l2i_conv_params* p, void* stream);

/* Which kernel family l2i_conv2d_f32 runs `p` on (no launch; pure function of the parameters): the measurement code uses it to
 * price every launch against the roofline of the kernel that actually ran. */
#define L2I_FAMILY_IMPLICIT_GEMM 0  /* conv_mfma_kernel: LDS-staged halo tile, v_mfma_f32_32x32x2_f32 */
#define L2I_FAMILY_GEMM1X1 1        /* gemm1x1_kernel: DMA-fed plain GEMM of unscaled 1x1 stride-1 layers */
#define L2I_FAMILY_CIN3 2           /* conv_cin3_kernel: 3x3 convs of <= 3-channel images */
#define L2I_FAMILY_DIRECT_SMALL 3   /* conv_direct_small_kernel: <= 4 output channels, VALU */
int l2i_conv2d_family(const l2i_conv_params* p);

/* Stride-2 TRANSPOSED convolution, all four output parities in one launch:
 *   y[b,co,2*iy+ky-pad,2*ix+kx-pad] += x[b,ci,iy,ix] * w[co,ci,ky,kx]          (F.conv_transpose2d(stride=2) of the up
 *   layers, networks.py:246-255, and the input-gradient of every stride-2 conv of the path).
 * Same struct as l2i_conv2d_f32 with KH = KW = K, pad_y = pad_x = pad, y = [B,Cout,OHf,OWf] of the natural size
 * (H-1)*2-2*pad+K (or up to 8 more: rows / columns no input reaches are written as zeros); `w` is the FUSED pack [Cin][K*K][CoutP] whose tap order is the kernel's walk order
 * (latent2im_amd/conv.py:fused_transposed_taps).  Fused: in_scale, in_mask, out_scale, out_gain; everything else must
 * be unset.  Built for (K,pad) in {(3,0),(3,1),(7,3)}; other shapes return L2I_E_UNSUPPORTED (use the per-parity
 * l2i_conv2d_f32 calls). */
int l2i_conv_transpose2d_f32(const l2i_conv_params* p, void* stream);
/* K = 3, pad 0 / 1, fp32 maps at least 32 positions wide, Cin % 4 == 0, no split-K: the entry can run the 25-PRODUCT form instead
 * (convt_poly_kernel, csrc/l2i_convt_poly.hip).  Per dimension the outputs of one parity are a 2-tap filter of the input, those of the other a 1-tap
 * filter; two adjacent 2-tap outputs are Winograd F(2,2) (3 products for 4), so a 3x3 raw patch x[2W - 1 + pad + {0,1,2}] of window W gives the
 * 4x4 output patch 4W .. 4W + 3 from 25 products instead of 36, with coefficients 0 / +-1 only.  It reads `w_lo` = fp32 [Cin][25][CoutP] (latent2im_amd/conv.py:pack_weight_convt_poly), plane
 * 5 a + b = sum_{ky,kx} g[a][ky] g[b][kx] w[co,ci,ky,kx] with the 1-D planes g = (w2, w0 + w2, w0, w1, w1), float64 sums rounded once; `w` stays
 * the fused pack.  Same fusions, same output sizes, results within fp32 rounding of the direct kernel (not bit-identical).
 * tile_hint: 0 = per shape: the new kernel where w_lo is set and the shape is in the launcher's measured table (l2i_convt_poly.hip:
 *                kPolyRules), else the direct kernel with its automatic tile;
 *            1 / 2 = the direct kernel's 128- / 256-position tile;   9 = the direct kernel, automatic tile (the A/B comparator; so does every
 *            other value: callers that walk l2i_conv2d_f32's tile numbers 1 .. 8 over both entries keep what they had);
 *            10 = the new kernel; L2I_E_UNSUPPORTED where it does not take the struct, L2I_E_ARG without w_lo.
 * Additive (a struct without w_lo runs as before): the ABI version did not move. */
#define L2I_CONVT_HINT_DIRECT 9
#define L2I_CONVT_HINT_POLY 10
/* Host only, no launch: the kernel family l2i_conv_transpose2d_f32 runs `p` on, ASSUMING the pack in w_lo is supplied (callers build that pack on the
 * first launch that reports L2I_TFAMILY_POLY); -1 for a null struct. */
#define L2I_TFAMILY_DIRECT 0        /* convt_mfma_kernel */
#define L2I_TFAMILY_POLY 1          /* convt_poly_kernel: 25 / 36 of the MFMA work */
#define L2I_TFAMILY_SMALL 2         /* convt_small_kernel: <= 3 output channels, VALU */
int l2i_conv_transpose2d_family(const l2i_conv_params* p);
/* Host only: the launch plan convt_poly_kernel would run `p` with (tests check its tiles, windows, halo and DMA slot ranges without a GPU).
 * eligible = 0 (and the reason in l2i_last_error) where the kernel does not take the struct; returns L2I_E_ARG for a null argument only.
 * Block tile = 16 output channels x WTH x WTW windows (<= 64); window (wy, wx) reads the raw rows 2 wy + org .. + 2 (columns alike) and owns the
 * outputs 4 wy .. 4 wy + 3; the raw tile of a block is IH x IW = (2 WTH + 1) x (2 WTW + 1) values per input channel, staged as nslots DMA slots of
 * 64 values at an LDS pitch of `plane` floats; CK input channels per stage (CK divides Cin), two stages of stage_floats floats. */
typedef struct l2i_convt_poly_plan {
    int32_t eligible, masked;
    int32_t nwx, nwy;           /* windows across / down the output: ceil(OWf / 4), ceil(OHf / 4) */
    int32_t WTW, WTH, tiles_x, tiles_y, mblocks;
    int32_t total, grid;        /* blocks with work = B * tiles_y * tiles_x * mblocks; the launch's grid (rounded up to 8) */
    int32_t IH, IW, org, nslots, plane, wpitch;
    int32_t CK, stage_floats, lds_bytes;
} l2i_convt_poly_plan;
int l2i_convt_poly_plan_for(const l2i_conv_params* p, l2i_convt_poly_plan* plan);

/* Split-precision variant of l2i_conv2d_f32 (BASELINE config 5's "16-bit MFMA" path; latent2im_amd.conv.PRECISION = 'bf16x3' selects
 * it): operands are split x = bf16(x) + bf16(x - bf16(x)) and a*b is evaluated as ah*bh + ah*bl + al*bh on v_mfma_f32_32x32x16_bf16
 * with fp32 accumulation (relative product error <= ~2^-17: fp32-class results).  fp32 tensors in and out, same prologue / epilogue
 * fusions; `w` is ignored, `w_hi` / `w_lo` are the host-split weight planes [Cin/16][KH*KW][2][CoutP][8] (hi = bf16(w), lo = bf16(w - hi)).
 * Layers: 1x1 (pad 0, Cin % 32 == 0) and 3x3 (pad 1; stride 2 also pad 0; Cin % 16 == 0), stride 1 or 2, dense output window, OW >= 32,
 * W % 4 == 0, 16-byte aligned x / in_mask.  Anything else returns L2I_E_UNSUPPORTED (callers use l2i_conv2d_f32). */
int l2i_conv2d_bf16x3_f32(const l2i_conv_params* p, void* stream);

/* l2i_conv_transpose2d_f32 on the split-precision bf16 matrix path (same arithmetic as l2i_conv2d_bf16x3_f32): 3x3 stride-2 transposed
 * conv, pad 0 (the generator's up layers, networks.py:246-255) or pad 1 (input-gradient of a 3x3 stride-2 pad-1 conv), all four output
 * parities per launch.  `w_hi` / `w_lo`: the bf16 planes of the [Cout, Cin, 3, 3] correlation-form weight in the layout of
 * l2i_conv2d_bf16x3_f32 ([Cin/16][9][2][CoutP][8]); `w` is ignored.  Fused: in_scale, in_mask, out_scale, out_gain.  Needs Cin % 16 == 0,
 * W % 4 == 0, W >= 32 and the natural output size; other shapes return L2I_E_UNSUPPORTED (use l2i_conv_transpose2d_f32). */
int l2i_conv_transpose2d_bf16x3_f32(const l2i_conv_params* p, void* stream);

/* 3x3 stride-1 layers (KH = KW = 3, stride 1, dense output window, Cin % 8 == 0, output rows 16-byte aligned multiples of
 * 4 pixels) as Winograd F(2x2,3x3) on the fp32 matrix cores: exact-fp32 products and accumulation like l2i_conv2d_f32,
 * 2.25x fewer of them (the algorithm vendor libraries select for the reference's F.conv2d 3x3 calls too).  Same struct,
 * same prologue / epilogue fusions; `w` is the TRANSFORMED pack U = G g G^T laid out [Cin][4][CoutP][4]
 * (latent2im_amd/conv.py:pack_weight_wino).  tile_hint must be 0.
 * Shapes outside the constraints return L2I_E_UNSUPPORTED (callers use l2i_conv2d_f32). */
int l2i_conv2d_wino_f32(const l2i_conv_params* p, void* stream);

/* The same layers as Winograd F(4x4,3x3): 36 multiplies per 4x4 output tile and (cin, cout) — 1.78x fewer than F(2x2,3x3), 4x fewer than the
 * direct form; fp32 products and accumulation, error ~1e-6..1e-5 of max|y| against the exact correlation (F(2x2): 3e-7).  Unmasked launches
 * only: `in_mask` must be NULL or the input itself with ReLU slopes (1, 0) (ReLU-on-load); Cin % 4 == 0.  `w` is the transformed pack
 * U = G g G^T (6x6 per (cin, cout)) in the kernel's LDS image order [Cin/4][CoutP/16][ [6 i][4 cin][16 cout][4 j=0..3] ++ [6][4][16][2 j=4,5] ]
 * (latent2im_amd/conv.py:pack_weight_wino4); CoutP = Cout rounded up to 32.  Same epilogue fusions as l2i_conv2d_wino_f32 (incl. sq_ref).
 * tile_hint 0: the position-split kernel (round 5: a block owns 32 output channels, two waves share the 36 Winograd positions of a tile row;
 * needs pad_x == 1 and W % 4 == 0); tile_hint 1: the round-4 kernel (16 channels per block), same arithmetic, bit-identical results;
 * tile_hint 2: the position-split kernel on 64 x 16-pixel tiles / eight waves where the map has >= 64 columns and >= 16 rows (an A/B form: slower). */
int l2i_conv2d_wino4_f32(const l2i_conv_params* p, void* stream);
/* Host only, no launch: the epilogue class the position-split kernel (tile_hint 0 / 2) takes for this struct.  A lean class is compiled for one exact
 * operand set (in_scale / ReLU-on-load, out_scale, noise, bias, out_mask, residual, res_sub, res_mask, act, out_gain != 1, accumulate, pool_out,
 * sq_ref) of the training step: 0 .. L2I_WINO4S_LEAN_CLASSES - 1; every other set takes the generic body = L2I_WINO4S_LEAN_CLASSES.  Same results
 * bit for bit either way.  -1: p is NULL.  (The struct's shape is not validated here: l2i_conv2d_wino4_f32 does that.) */
#define L2I_WINO4S_LEAN_CLASSES 8
int l2i_wino4s_epilogue_class(const l2i_conv_params* p);

/* ---- the 16-bit path (BASELINE config 5: "fp16 MFMA"; bf16 here: fp32's exponent range, so gradients of 1e-9 need no loss scaling) ----
 * Tensors in the channel-blocked "h8" layout [B][C/8][H][W][8] bf16 (the 8 channels of a pixel = 16 contiguous bytes = one MFMA fragment);
 * one v_mfma_f32_32x32x16_bf16 product per MAC, fp32 accumulation; fp32 only for bias, noise, per-sample scales and the loss sums.
 * l2i_conv2d_h8: 1x1 (pad 0) / 3x3 (pad 0 or 1) correlation, stride 1 or 2, Cin % 32 == 0.  Same struct as l2i_conv2d_f32 with
 *   x, y, residual, res_mask, out_mask, res_sub, sq_ref -> bf16 h8 tensors (fp32 NCHW for y and the epilogue operands when out_f32 = 1);
 *   w_hi -> bf16 weight planes [Cin/16][KH*KW][2][CoutP][8] (latent2im_amd/conv.py:pack_weight_bf16x3, hi plane), per sample when w_bstride != 0;
 *   noise [B,1,OHf,OWf], bias [Cout], out_scale [B,Cout] fp32; `w`, `w_lo` ignored; no prologue fusions (scales live in the weights, masks in
 *   the producing epilogue): in_scale must be NULL, in_mask NULL or == x with mask (1, 0) (ReLU-on-load, 3x3 stride-1 layers); with the h8
 *   output the output mask is leaky: * (out_mask > 0 ? mask_pos : mask_neg) (res_mask stays binary).  With out_f32 = 1 the epilogue is the fp32
 *   kernels' own, whose masks are binary: an out_mask with (mask_pos, mask_neg) != (1, 0) returns L2I_E_UNSUPPORTED.  h8 output needs Cout % 8 == 0.
 * l2i_conv_transpose2d_h8: stride-2 transposed 3x3 conv (pad 0 / 1), all four output parities per launch, h8 in and out. */
int l2i_conv2d_h8(const l2i_conv_params* p, void* stream);
int l2i_conv_transpose2d_h8(const l2i_conv_params* p, void* stream);
/* Host only, no launch: the plan l2i_conv2d_h8 (transposed = 0) / l2i_conv_transpose2d_h8 (transposed != 0) and their _f16 twins run `p` with — the
 * entry points take it from the same function.  eligible = 0 (every other field 0, the reason in l2i_last_error) where the entry refuses the struct;
 * returns L2I_E_ARG for a null argument only.  The instantiation of conv_h8_kernel: a block of 32 WM output channels x 4 WN rows x 32 columns (per
 * input position and four outputs each when TR != 0), K x K taps at stride S, KS 16-channel MFMA steps per chunk, relu_in = ReLU-on-load, out32 =
 * fp32 NCHW output, extra = the instantiation that carries the lean epilogue's optional outputs (rgb_w, sq_ref).  epilogue: which of the four the
 * launch takes.  total = B * tiles_y * tiles_x * mblocks blocks with work, grid = total rounded up to 8.  Additive: the ABI version did not move. */
#define L2I_H8_EPI_LEAN 0           /* h8 output, per-channel vectors and noise only, max(v gpos, v gneg): needs 0 <= gneg <= gpos */
#define L2I_H8_EPI_GENERAL 1        /* h8 output, every operand (H8Out::finish) */
#define L2I_H8_EPI_F32_VEC 2        /* fp32 output, the shared fp32 epilogue with 16-byte accesses */
#define L2I_H8_EPI_F32_SCALAR 3     /* fp32 output, the shared fp32 epilogue element by element */
typedef struct l2i_conv_h8_plan {
    int32_t eligible;
    int32_t WM, WN, KS, K, S, TR;   /* TR: 0 = correlation, 1 / 2 = transposed with pad 0 / 1 */
    int32_t out32, relu_in, extra, rgb;
    int32_t epilogue;               /* L2I_H8_EPI_* */
    int32_t nchunks, tiles_x, tiles_y, mblocks, total, grid, lds_bytes;
} l2i_conv_h8_plan;
int l2i_conv_h8_plan_for(const l2i_conv_params* p, int transposed, l2i_conv_h8_plan* plan);

/* [ABI 7] Two chained 1x1 stride-1 convolutions on h8 maps in one launch (csrc/l2i_pair_h8.hip): `first` (Cin1 -> Cout1, with its bias / residual /
 * ReLU / sign-plane masks / sign-plane output, y = the wide map, written) feeds `second` (Cout1 -> Cout2 <= 256, bias / ReLU / sign-plane mask / sign-plane
 * output) from registers: the wide map is not read back.  ResNet-50's trunk (torchvision Bottleneck as called at transform_base.py:396-403, 416-424):
 * forward = conv3 + identity + ReLU of a block, then conv1 + ReLU of the next; backward = conv1's input gradient + trunk gradient, masked, then conv3's
 * input gradient of the block below.  Each struct is filled exactly as for l2i_conv2d_h8 (second->x may be NULL or first->y); results are bit-identical
 * to the two l2i_conv2d_h8 launches.  Refused (L2I_E_UNSUPPORTED) unless: both 1x1 / stride 1 / pad 0 / h8 output, first->residual set, masks given as sign
 * planes (mask_bits), H * W a multiple of 128, (Cin1, Cout2) one of (64, 64), (128, 128), (256, 256), (64, 128), (128, 256) — the caller then launches the two convs separately.
 * variant: 0 = 256-pixel tiles, 1 = 128-pixel tiles (more blocks on small maps). */
int l2i_conv1x1_pair_h8(const l2i_conv_params* first, const l2i_conv_params* second, int variant, void* stream);
/* The same launch with the 3x3 stride-1 pad-1 conv in FRONT of the pair: head3x3 (C -> C, C <= 128 here: bias / ReLU / sign-plane mask / sign-plane output; its
 * map is written only if head3x3->y is set) -> first -> second: one launch per ResNet-50 bottleneck (conv2, conv3 + identity, the next block's conv1; backwards:
 * conv2's input gradient, conv1's + trunk gradient, conv3's of the block below).  The 3x3 runs exactly as l2i_conv2d_h8 would (16-channel chunks), so the
 * three results equal the three launches' bit for bit.  Needs W % 32 == 0, H % 4 == 0 and (C, Cout2) one of (64, 64), (128, 128), (64, 128). */
int l2i_conv_chain3_h8(const l2i_conv_params* head3x3, const l2i_conv_params* first, const l2i_conv_params* second, int variant, void* stream);

/* [ABI 7] The fp32 twin of l2i_conv1x1_pair_h8 (csrc/l2i_pair_f32.hip): `first` = a 1x1 stride-1 conv of l2i_conv2d_f32 with bias / residual / ReLU (its y, the wide
 * map, is written), `second` = the 1x1 conv that reads it (bias / ReLU), one launch, the wide map not read back.  Both structs filled as for l2i_conv2d_f32
 * (w = the [Cin][1][CoutP] pack).  The second conv adds its channel pairs in another order than l2i_conv2d_f32: equal to fp32 rounding, not bit for bit.
 * Refused (L2I_E_UNSUPPORTED; the caller launches the two convs) unless H * W % 256 == 0 and (Cin1, Cout2) is (64, 64), (64, 128) or (128, 128). */
int l2i_conv1x1_pair_f32(const l2i_conv_params* first, const l2i_conv_params* second, void* stream);

/* [r5] The image-side convolutions of the 16-bit path (csrc/l2i_img_h8.hip): x = fp32 NCHW image [B, Cin <= 4, H, W], y = 16-bit h8
 * [B, Cout/8, OHf, OWf, 8], 16-bit MFMA with fp32 accumulation on operands rounded to the element type inside the kernel — VGG-19 conv1_1
 * (3x3 / stride 1; transform_base.py:426-454), the discriminator's from-RGB 1x1 (networks.py:568-575), ResNet-50's 7x7 / stride 2 stem
 * (transform_base.py:396-403) without a zero-padded 16-bit copy of the image, an fp32 stem map or a cast pass.  Built for (KH, stride) in
 * {(1, 1), (3, 1), (7, 2)}, any symmetric padding.  `w_hi`: 16-bit planes [ceil(Cin KH / 2)][2][CoutP][8] whose element (s, half, co, e) is
 * w[co, c, ky, kx = e] for (c, ky) = divmod(2 s + half, KH), zero for e >= KW or 2 s + half >= Cin KH (latent2im_amd/conv.py:
 * pack_weight_img_h8).  Fused: bias, act, out_gain (> 0), sq_ref / sq_out (sq_ref h8 like y).  Everything else must be unset. */
int l2i_conv_img_h8(const l2i_conv_params* p, void* stream);

/* Streaming companions on h8 maps (csrc/l2i_stream_h8.hip; same functions as the fp32 entry points below, arithmetic in fp32 registers):
 * layout casts fp32 NCHW <-> bf16 h8 (Cpad = channel count of the h8 tensor, a multiple of 8, zero filled above C);
 * the reference's upfirdn2d on h8 planes (kernels up to 4x4, up / down in {1, 2}) with the generator's fused epilogue, in this order:
 *   v = act(fir(x) + noise[b,oy,ox] * noise_w + bias[c]) * act_gain   (act_gain under EVERY act, L2I_ACT_NONE included),
 *   v *= (mask > 0 ? mask_pos : mask_neg),   y = v + addend           (the addend is NOT inside the activation: the fp32 entry differs);
 * ToRGB (x h8 -> rgb fp32 [B,3,HW]); the fused activation backward of a styled conv (dz h8; gin h8; grgb fp32; reductions fp32, zeroed by the caller);
 * out[b,c] += sum_p a * b; MaxPool2d forward (idx: [planes][OH][OW][8] bytes; relu = 1: y = max(pool, 0)) and backward (optionally + coef *
 *   coef_dev[0] * (b - a): the ContentLoss term of the pooled tap); the ContentLoss difference; y[2oy, 2ox] += c[oy, ox]; and the per-sample
 *   weight planes of a modulated conv: planes[b] = bf16(w32 * s[b, input channel]) with w32 = the fp32 weights in plane order.
 * Operand sets: the same as the fp32 twins (l2i_torgb_fwd_f32, l2i_sg2_act_bwd_f32 below: which operands may be NULL, which pairs go together,
 * what is refused with L2I_E_ARG).  What the layout forces on top: C % 8 == 0 (and C <= 4096 for ToRGB, whose weights sit in LDS), any HW >= 1
 * (a pixel slot is one 16-byte access: no HW % 4 rule), h8 maps on 16-byte boundaries (every slot of a tensor the allocator returned is); the
 * fp32 operands (grgb, noise, bias, wmod, the sums) are read as scalars and need only their natural 4-byte alignment. */
int l2i_cast_f32_to_h8(void* y, const float* x, int B, int C, int Cpad, int64_t HW, void* stream);
int l2i_cast_h8_to_f32(float* y, const void* x, int B, int C, int Cpad, int64_t HW, void* stream);
int l2i_upfirdn2d_h8(void* y, const void* x, const float* k, int64_t planes, int channels, int in_h, int in_w, int kh, int kw, int up, int down,
                     int pad_x0, int pad_x1, int pad_y0, int pad_y1, const float* noise, float noise_w, const float* bias, int act, float act_slope,
                     float act_gain, const void* mask, float mask_pos, float mask_neg, const void* addend, const float* k1y, const float* k1x, int mask_bits,
                     void* stream);
                     /* ... then * (mask > 0 ? mask_pos : mask_neg) (h8, like y: a gradient through a (leaky) ReLU) and + addend (h8, like y).
                        k1y / k1x: HOST pointers to four floats each, or NULL: the caller states that k = outer(k1y, k1x) (4x4, up = down = 1: the
                        register-streaming separable kernel).  [ABI 6] mask_bits = 1: `mask` is the SIGN PLANE of that map (one byte per pixel slot,
                        l2i_conv_params::mask_out) — separable 4x4 blur without resampling only */
int l2i_torgb_fwd_h8(float* rgb, const void* x, const float* wmod, const float* bias, int B, int C, int64_t HW, void* stream);
int l2i_sg2_act_bwd_h8(void* dz, const void* gin, const float* gin_scale, const float* grgb, const float* wmod_rgb, const void* y, const float* bias,
                       const float* noise, float noise_w, float slope, float gain, float* red_dz_z, float* red_x_grgb, float* red_gin_y, int B, int C, int64_t HW, void* stream);
int l2i_dot_reduce_h8(float* out, const void* a, const void* b, int B, int C, int64_t HW, void* stream);
int l2i_maxpool2d_fwd_h8(void* y, void* idx, const void* x, int64_t planes, int H, int W, int k, int s, int pad, int OH, int OW, int relu, void* stream);
int l2i_maxpool2d_bwd_h8(void* gx, const void* gy, const void* idx, const void* a, const void* b, float coef, const float* coef_dev, int64_t planes, int H, int W,
                         int k, int s, int pad, int OH, int OW, void* stream);
int l2i_sqdiff_h8(float* sum_out, void* grad, const void* a, const void* b, int64_t slots, float coef, const float* coef_dev, void* stream);
int l2i_add_zero_insert_h8(void* y, const void* c, const void* mask, int64_t planes, int H, int W, int OH, int OW, void* stream);   /* mask (h8 like y, or NULL): c * (mask[2oy,2ox] > 0) */
int l2i_mask_mul_h8(void* y, const void* g, const void* ref, float pos, float neg, int64_t slots, void* stream);                     /* y = g * (ref > 0 ? pos : neg) */
int l2i_mask_mul_bits_h8(void* y, const void* g, const void* bits, float pos, float neg, int64_t slots, void* stream);               /* [ABI 6] the same with ref's sign plane (one byte per slot) */
int l2i_modulate_planes_h8(void* planes, const float* w32, const float* s, int B, int Cs, int CinP, int KK, int CoutP, void* stream);
/* CinP % 16 == 0, Cs == CinP, planes and w32 on 16-byte boundaries (16-byte accesses); anything else: L2I_E_ARG. */
/* [r5] l2i_modulate_planes_h8 for every modulated conv of a generator pass in one launch.  `table` (device): nseg rows of eight int64 — w32 offset
 * (floats from `w32`), scale offset (floats from `s`: the layer's [B, Cs] block), output offset (16-byte slots from `planes`: the layer's
 * [B][slots per sample] block), slots per sample (= CinP/16 * KK * 2 * CoutP), KK, CoutP, Cs (= CinP), first block of the segment (ascending,
 * row 0 = 0); `nblocks` = grid size (blocks of a segment = next row's first block - its own).  networks.py:234-235 per layer. */
int l2i_modulate_planes_multi_h8(void* planes, const float* w32, const float* s, const void* table, int nseg, int B, int nblocks, void* stream);

/* [r5] The same sixteen entry points with IEEE fp16 (binary16) elements instead of bf16 — BASELINE configs[4] names "fp16 MFMA"; what the reference
 * would run under autocast on networks.py:231-272.  Identical signatures, layouts and fusions; the contraction is v_mfma_f32_32x32x16_f16 (same rate
 * as the bf16 instruction), conversions round to nearest even.  fp16 has 3 more mantissa bits than bf16 and 3 fewer exponent bits: the caller keeps
 * gradients inside its range with power-of-two loss scales (latent2im_amd/nets16.py: one per loss branch, undone on the fp32 side: exact). */
int l2i_conv2d_h8_f16(const l2i_conv_params* p, void* stream);
int l2i_conv_transpose2d_h8_f16(const l2i_conv_params* p, void* stream);
int l2i_conv1x1_pair_h8_f16(const l2i_conv_params* first, const l2i_conv_params* second, int variant, void* stream);
int l2i_conv_chain3_h8_f16(const l2i_conv_params* head3x3, const l2i_conv_params* first, const l2i_conv_params* second, int variant, void* stream);
int l2i_conv_img_h8_f16(const l2i_conv_params* p, void* stream);
int l2i_cast_f32_to_h8_f16(void* y, const float* x, int B, int C, int Cpad, int64_t HW, void* stream);
int l2i_cast_h8_to_f32_f16(float* y, const void* x, int B, int C, int Cpad, int64_t HW, void* stream);
int l2i_upfirdn2d_h8_f16(void* y, const void* x, const float* k, int64_t planes, int channels, int in_h, int in_w, int kh, int kw, int up, int down,
                         int pad_x0, int pad_x1, int pad_y0, int pad_y1, const float* noise, float noise_w, const float* bias, int act, float act_slope,
                         float act_gain, const void* mask, float mask_pos, float mask_neg, const void* addend, const float* k1y, const float* k1x, int mask_bits,
                         void* stream);
int l2i_torgb_fwd_h8_f16(float* rgb, const void* x, const float* wmod, const float* bias, int B, int C, int64_t HW, void* stream);
int l2i_sg2_act_bwd_h8_f16(void* dz, const void* gin, const float* gin_scale, const float* grgb, const float* wmod_rgb, const void* y, const float* bias,
                           const float* noise, float noise_w, float slope, float gain, float* red_dz_z, float* red_x_grgb, float* red_gin_y, int B, int C, int64_t HW, void* stream);
int l2i_dot_reduce_h8_f16(float* out, const void* a, const void* b, int B, int C, int64_t HW, void* stream);
int l2i_maxpool2d_fwd_h8_f16(void* y, void* idx, const void* x, int64_t planes, int H, int W, int k, int s, int pad, int OH, int OW, int relu, void* stream);
int l2i_maxpool2d_bwd_h8_f16(void* gx, const void* gy, const void* idx, const void* a, const void* b, float coef, const float* coef_dev, int64_t planes, int H, int W,
                             int k, int s, int pad, int OH, int OW, void* stream);
int l2i_sqdiff_h8_f16(float* sum_out, void* grad, const void* a, const void* b, int64_t slots, float coef, const float* coef_dev, void* stream);
int l2i_add_zero_insert_h8_f16(void* y, const void* c, const void* mask, int64_t planes, int H, int W, int OH, int OW, void* stream);
int l2i_mask_mul_h8_f16(void* y, const void* g, const void* ref, float pos, float neg, int64_t slots, void* stream);
int l2i_mask_mul_bits_h8_f16(void* y, const void* g, const void* bits, float pos, float neg, int64_t slots, void* stream);
int l2i_modulate_planes_h8_f16(void* planes, const float* w32, const float* s, int B, int Cs, int CinP, int KK, int CoutP, void* stream);
int l2i_modulate_planes_multi_h8_f16(void* planes, const float* w32, const float* s, const void* table, int nseg, int B, int nblocks, void* stream);

/* out[i] = act_grad_table(x[i] + b[(i / step_b) % size_b], ref[i]) * scale   — the reference op, all six
 * act*10+grad cases (fused_bias_act_kernel.cu:36-47).  b / ref may be NULL (= the reference's empty tensors). */
int l2i_fused_bias_act_f32(float* y, const float* x, const float* b, const float* ref, int64_t n,
                           int64_t step_b, int64_t size_b, int act, int grad, float alpha, float scale, void* stream);

/* The same op for half tensors: the reference dispatches AT_DISPATCH_FLOATING_TYPES_AND_HALF (fused_bias_act_kernel.cu:79).  y / x / b / ref
 * point to IEEE binary16; arithmetic follows the reference's scalar_t = Half instantiation operation by operation (each binary op is
 * the float op rounded to half; alpha and scale are rounded to half first), so results are bit-identical to it. */
int l2i_fused_bias_act_f16(void* y, const void* x, const void* b, const void* ref, int64_t n, int64_t step_b, int64_t size_b,
                           int act, int grad, float alpha, float scale, void* stream);

/* The reference op on [major, in_h, in_w] maps (minor_dim == 1, the only layout the path uses:
 * op/upfirdn2d.py:98) with an optional fused epilogue (all NULL/0 = the plain reference op):
 *   v = fir(x) + noise[b,oy,ox]*noise_w + bias[c] + addend[idx],   major = b*channels + c   (the addend is INSIDE the activation),
 *   L2I_ACT_LRELU: y = (v > 0 ? v : v*act_slope) * act_gain;  L2I_ACT_RELU: y = max(v, 0);  L2I_ACT_NONE: y = v
 *   (act_gain is applied under L2I_ACT_LRELU ONLY; the h8 entry applies it under every act), then the mask of l2i_upfirdn2d_masked_f32, last.
 * kh * kw <= 64, up / down >= 1; pads may be negative (a crop).  major need not be a multiple of channels: b = major / channels, c = major %
 * channels, so the last sample is partial and noise holds ceil(major / channels) maps; channels <= 0 reads as 1. */
int l2i_upfirdn2d_f32(float* y, const float* x, const float* k, int64_t major, int in_h, int in_w, int kh, int kw,
                      int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                      int channels, const float* noise, float noise_w, const float* bias, const float* addend,
                      int act, float act_slope, float act_gain, void* stream);

/* [r5] The same op with one more fused term, y *= (mask[idx] > 0 ? mask_pos : mask_neg) after the activation: a gradient that passes a (leaky) ReLU on its
 * way out of the FIR (the discriminator's backward, networks.py:530-536 / 574-583: the 3x3 gradient conv that follows then needs no mask operand and
 * takes the Winograd F(4x4) kernel).  mask is shaped like y.  NULL mask = l2i_upfirdn2d_f32. */
int l2i_upfirdn2d_masked_f32(float* y, const float* x, const float* k, int64_t major, int in_h, int in_w, int kh, int kw,
                             int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                             int channels, const float* noise, float noise_w, const float* bias, const float* addend,
                             int act, float act_slope, float act_gain, const float* mask, float mask_pos, float mask_neg, void* stream);

/* The same launch with a second output: y is exactly what l2i_upfirdn2d_masked_f32 writes, and y2[idx] = y[idx] * (mask2[idx] > 0 ? pos2 : neg2), one fp32
 * multiply on the value held in registers.  The discriminator's backward: the FIR that produces a block's gradient g also writes g through the leaky ReLU
 * of the next block's stride-2 conv, so that conv's input gradient is an unmasked transposed launch (the DMA-fed kernels) while the skip path keeps reading
 * g.  y2 and mask2 are shaped like y and are given together or not at all: one without the other returns L2I_E_ARG and nothing is written; both NULL =
 * l2i_upfirdn2d_masked_f32.  Every fp32 FIR kernel has the second output; the vector paths want y2 and mask2 16-byte aligned like y (else the launch falls
 * through to the next kernel, as for y).  Additive: the ABI version is unchanged. */
int l2i_upfirdn2d_dual_f32(float* y, float* y2, const float* mask2, float pos2, float neg2, const float* x, const float* k, int64_t major,
                           int in_h, int in_w, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                           int channels, const float* noise, float noise_w, const float* bias, const float* addend,
                           int act, float act_slope, float act_gain, const float* mask, float mask_pos, float mask_neg, void* stream);

/* upfirdn2d for half tensors (upfirdn2d_kernel.cu:225 dispatches half too): plain reference op, no fused epilogue.  y / x / k point to IEEE
 * binary16; like the reference kernel the taps and products are float and the accumulator is rounded to half after every tap, taps in
 * ascending input row / column order (upfirdn2d_kernel.cu:118-123): bit-identical results. */
int l2i_upfirdn2d_f16(void* y, const void* x, const void* k, int64_t major, int in_h, int in_w, int kh, int kw, int up_x, int up_y,
                      int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* ToRGB 1x1 modulated conv without demodulation (networks.py:346-351):
 *   rgb[b,o,p] = sum_c x[b,c,p] * wmod[b,o,c] + bias[o],  wmod = scale*W[o,c]*s[b,c] prepared by the caller [B,3,C]
 * bias may be NULL (= zeros), in the h8 twin too.  HW % 4 == 0, and rgb / x on 16-byte boundaries (they are accessed as float4): anything else
 * returns L2I_E_ARG before a launch. */
int l2i_torgb_fwd_f32(float* rgb, const float* x, const float* wmod, const float* bias, int B, int C, int64_t HW,
                      void* stream);

/* Fused elementwise backward of one StyledConv output (FusedLeakyReLU + NoiseInjection + demod bookkeeping) with the
 * ToRGB branch folded in:
 *   g      = gin[idx]*gin_scale[b,c] + sum_o wmod_rgb[b,o,c]*grgb[b,o,p]          (either part optional)
 *   dz     = g * (y > 0 ? gain : gain*slope)                                        -> dz[idx]
 *   zpre   = (y > 0 ? y/gain : y/(gain*slope)) - bias[c] - noise[b,p]*noise_w
 *   red_dz_z[b,c] += sum_p dz*zpre            (-> d demod)        red_x_grgb[b,c,o] += sum_p y*grgb[b,o,p]  (-> d s_rgb)
 *   [r5] red_gin_y[b,c] += sum_p gin*y  (NULL: not formed) — y is the INPUT of the next layer and gin the gradient w.r.t. that layer's modulated input,
 *   so this is the next layer's style gradient d s (networks.py:234-235: x * s), formed while both maps pass through registers instead of by a
 *   l2i_dot_reduce pass that reads them again.
 * Reduction buffers must be zeroed by the caller (the kernel adds to them).
 * Operand sets, the same for this entry and l2i_sg2_act_bwd_h8:
 *   gin and / or grgb must be given; gin_scale NULL = 1; grgb and wmod_rgb go together (either without the other is refused, not ignored);
 *   bias / noise NULL = zeros; red_dz_z, red_x_grgb, red_gin_y may each be NULL (that sum is not formed); red_x_grgb without grgb and red_gin_y
 *   without gin are not touched; gain and slope must be non-zero (zpre divides by them).
 * Here HW % 4 == 0 and dz, y, gin, grgb, noise on 16-byte boundaries (accessed as float4; a view that starts one float into a buffer is refused).
 * Every violation returns L2I_E_ARG before a launch. */
int l2i_sg2_act_bwd_f32(float* dz, const float* gin, const float* gin_scale, const float* grgb, const float* wmod_rgb,
                        const float* y, const float* bias, const float* noise, float noise_w, float slope, float gain,
                        float* red_dz_z, float* red_x_grgb, float* red_gin_y, int B, int C, int64_t HW, void* stream);

/* out[r] (+)= sum_p a[r,p] * (b ? b[r,p] : 1), r < rows (rows = B*C).  `out` must be zeroed by the caller.  No alignment rule: a row whose
 * base is not on a 16-byte boundary, or cols % 4 != 0, is read with scalar loads. */
int l2i_dot_reduce_f32(float* out, const float* a, const float* b, int64_t rows, int64_t cols, void* stream);

/* MaxPool2d(k, s, pad) on [N, H, W] planes; idx holds the window-local argmax (first maximum in row-major order, like
 * ATen; a NaN in the window is the result and its position the index) so that the backward is exact under ties.  k <= 15.  No alignment
 * or shape rule: the 16-byte kernels of (k, s, pad) = (2, 2, 0) and (3, 2, 1) are taken where W == 2 OW, OW % 4 == 0 (forward) / W % 4 == 0
 * (backward) and the pointers allow, odd H included for (3, 2, 1); every other call takes the scalar kernels. */
int l2i_maxpool2d_fwd_f32(float* y, uint8_t* idx, const float* x, int64_t planes, int H, int W, int k, int s, int pad,
                          int OH, int OW, void* stream);
int l2i_maxpool2d_bwd_f32(float* gx, const float* gy, const uint8_t* idx, int64_t planes, int H, int W, int k, int s,
                          int pad, int OH, int OW, void* stream);
/* MaxPool2d(2, 2) backward fused with the ContentLoss gradient of the pooled layer's input (VGG conv1_2 tap,
 * transform_base.py:57-63,440-452): gx = maxpool_bwd(gy) + coef * (coef_dev ? coef_dev[0] : 1) * (b - a), a / b / gx [planes, 2*OH, 2*OW].
 * One pass over a and b instead of sqdiff-gradient + pool backward + add. */
int l2i_maxpool2x2_bwd_add_diff_f32(float* gx, const float* gy, const uint8_t* idx, const float* a, const float* b, float coef,
                                    const float* coef_dev, int64_t planes, int OH, int OW, void* stream);

/* ContentLoss (transform_base.py:57-63): sum_out[0] += sum (a-b)^2 ; grad[i] = coef*(coef_dev ? coef_dev[0] : 1)*(b[i]-a[i])
 * (= d/d b of the scaled loss; coef_dev is a device scalar so that the upstream gradient needs no host sync).
 * sum_out / grad / coef_dev may each be NULL. */
int l2i_sqdiff_f32(float* sum_out, float* grad, const float* a, const float* b, int64_t n, float coef,
                   const float* coef_dev, void* stream);

/* y[i] = a[i]*sa[(i/step) % ...] ... small utilities */
int l2i_axpby_f32(float* y, const float* a, const float* b, float alpha, float beta, int64_t n, void* stream);

/* relu-masked copy: y = g * (ref > 0 ? 1 : 0) */
int l2i_relu_mask_f32(float* y, const float* g, const float* ref, int64_t n, void* stream);

/* ---- training a conv net (scene_regressor_256.py:118-171 trains the ResNet-50 regressor; the walk path never needs these) ----
 * Weight gradient of a correlation: dw[co,ci,ky,kx] += sum_{b,oy,ox} gy[b,co,oy,ox] * x[b,ci,oy*stride+ky-pad_y,ox*stride+kx-pad_x]
 * (out-of-range x reads as zero).  dw [Cout,Cin,KH,KW] must be zeroed (or hold the value to accumulate into) by the caller; partial sums
 * meet by fp32 atomics, so the summation order is not fixed.  Built for KW in {1,3,7}. */
int l2i_conv2d_wgrad_f32(float* dw, const float* x, const float* gy, int B, int Cin, int H, int W, int Cout, int OH, int OW,
                         int KH, int KW, int stride, int pad_y, int pad_x, void* stream);
/* BatchNorm2d in training mode on [B,C,HW] maps.  stats: sum[c] += sum x, sumsq[c] += sum x^2 in float64 (caller zeroes them).
 * apply: y = relu?(x*scale[c] + shift[c] (+ residual)).  bwd_reduce: with dy = gy * (out_mask > 0 if given), xhat = (x-mean[c])*invstd[c]:
 * sum_dy[c] += sum dy, sum_dyxh[c] += sum dy*xhat (float64, caller zeroes).  bwd_apply: dx = gamma[c]*invstd[c] * (dy - mean_dy[c] -
 * xhat*mean_dyxh[c]) with mean_* = the sums / (B*HW); dy_masked (optional) receives dy (the gradient a residual branch takes). */
int l2i_bn_stats_f32(double* sum, double* sumsq, const float* x, int B, int C, int64_t HW, void* stream);
int l2i_bn_apply_f32(float* y, const float* x, const float* scale, const float* shift, const float* residual, int relu, int B, int C,
                     int64_t HW, void* stream);
int l2i_bn_bwd_reduce_f32(double* sum_dy, double* sum_dyxh, const float* gy, const float* out_mask, const float* x, const float* mean,
                          const float* invstd, int B, int C, int64_t HW, void* stream);
int l2i_bn_bwd_apply_f32(float* dx, float* dy_masked, const float* gy, const float* out_mask, const float* x, const float* mean,
                         const float* invstd, const float* gamma, const float* mean_dy, const float* mean_dyxh, int B, int C, int64_t HW,
                         void* stream);
/* [ABI 12, additive] The [C]-sized algebra between a reduction above and its apply pass, one launch over C each (csrc/l2i_train.hip), so that a
 * captured graph holds a whole BatchNorm.  n = B * HW of the reduction.  finalize, per channel, float64 until stated otherwise:
 *   m = sum / n;  var = max(sumsq / n - m * m, 0);  mean = fp32(m);  invstd = fp32(1 / sqrt(var + eps));  then in fp32 scale = weight * invstd,
 *   shift = bias - mean * scale, running_mean = running_mean * fp32(1 - momentum) + fp32(momentum) * mean, running_var likewise with
 *   fp32(var * (n / max(n - 1, 1))) (the unbiased variance); num_batches_tracked[0] += 1 (a device int64).  Every product, quotient and sum is
 *   rounded on its own, no contraction; the float64 square root and quotients are correctly rounded.  running_mean, running_var and
 *   num_batches_tracked may each be NULL (not updated).
 * bwd_finalize: d_bias = fp32(sum_dy), d_weight = fp32(sum_dyxh), mean_dy = fp32(sum_dy / n), mean_dyxh = fp32(sum_dyxh / n): exact conversions
 *   of the float64 sums and quotients.
 * Refused with L2I_E_ARG before a launch: a null pointer other than the three named, n <= 0, C <= 0, eps < 0, momentum outside [0, 1]. */
int l2i_bn_finalize_f32(float* mean, float* invstd, float* scale, float* shift, float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, const double* sum, const double* sumsq, const float* weight, const float* bias, int64_t n, int C,
                        double eps, double momentum, void* stream);
int l2i_bn_bwd_finalize_f32(float* d_bias, float* d_weight, float* mean_dy, float* mean_dyxh, const double* sum_dy, const double* sum_dyxh, int64_t n,
                            int C, void* stream);

/* ---- [ABI 12, additive] Repacking a trained convolution's weight in place, and batches from a device-resident dataset (csrc/l2i_repack.hip) ----------
 * l2i_repack_taps_f32: w is the weight itself, [Cout][Cin][K][K].  rows = swap ? Cout : Cin, cols = swap ? Cin : Cout.  layout L2I_REPACK_PACKED:
 *   dst [rows][count][colsP] with dst[r][t][c] = swap ? w[r][c][ky[t]][kx[t]] : w[c][r][ky[t]][kx[t]] for c < cols and 0 for cols <= c < colsP:
 *   every pack of latent2im_amd/conv.py that is a permutation of the weight (swap = 0 with the K * K taps in row order is pack_weight; swap = 1 with
 *   the taps reversed is the stride-1 gradient pack; the parity sub-packs, the fused transposed order and the 7x7 stem's [Cin][49][4] are other
 *   tables).  16-byte stores: colsP % 4 == 0, dst on a 16-byte boundary.  layout L2I_REPACK_OIHW: dst [rows][cols][count], colsP == cols (the plain
 *   weight a gradient launch keeps).  The table is passed to the kernel by value: a captured graph bakes it in.
 *   Refused with L2I_E_ARG before a launch: a null pointer, a non-positive size, K > 7, count outside 1..L2I_REPACK_MAX_TAPS, a tap outside the weight,
 *   colsP < cols, an unknown layout, or what the layout asks of colsP and dst above.
 * l2i_repack_wino_f32: the Winograd weight transform U = G g G^T of a 3x3 weight w [Cout][Cin][3][3] as seen by a conv of cout' = swap ? Cin : Cout
 *   output and cin' = swap ? Cout : Cin input channels, g[k][l] = w[..][flip ? 2 - k : k][flip ? 2 - l : l] (swap = flip = 1: the stride-1 gradient).
 *   kind L2I_REPACK_WINO2: F(2x2,3x3), dst [cin'][4][CoutP][4] (conv.pack_weight_wino); L2I_REPACK_WINO4: F(4x4,3x3), the LDS image order of
 *   csrc/l2i_wino4.hip (conv.pack_weight_wino4; cin' % 4 == 0); CoutP = cout' rounded up to 32, the padding written as zeros.
 *   Arithmetic, float64: rows first, T[i][l] = (G[i][0] g[0][l] + G[i][1] g[1][l]) + G[i][2] g[2][l] (k ascending), then columns,
 *   U[i][j] = (T[i][0] G[j][0] + T[i][1] G[j][1]) + T[i][2] G[j][2] (l ascending); zeros of G are multiplied like any entry, every product and sum
 *   is rounded on its own with no contraction, and U is rounded once to fp32.  tests/regtrain_ref.py states the same order in numpy.
 *   Refused with L2I_E_ARG before a launch: a null pointer, a non-positive size, an unknown kind, cin' % 4 != 0 for F(4x4), dst off a 16-byte boundary.
 * l2i_batch_from_u8_f32: out [B][elems] fp32 = (fp32(src[idx[b]][e]) / 255 - 0.5) * 2 of the uint8 images src [N][elems] (the division correctly
 *   rounded: CustomDataset's float32 expression bit for bit), idx [B] int64 on the device; label_out [B][L] = labels[idx[b]] when label_out is given.
 *   An index outside [0, N) writes zeros to both and reads neither.  Refused with L2I_E_ARG: a null out, src or idx, B outside 1..65535, N or elems
 *   <= 0, label_out without labels or L <= 0. */
#define L2I_REPACK_MAX_TAPS 49
#define L2I_REPACK_PACKED 0
#define L2I_REPACK_OIHW 1
#define L2I_REPACK_WINO2 2
#define L2I_REPACK_WINO4 4
typedef struct l2i_repack_taps { int32_t count; uint8_t ky[L2I_REPACK_MAX_TAPS]; uint8_t kx[L2I_REPACK_MAX_TAPS]; } l2i_repack_taps;
int l2i_repack_taps_f32(float* dst, const float* w, int Cout, int Cin, int K, const l2i_repack_taps* taps, int swap, int colsP, int layout,
                        void* stream);
int l2i_repack_wino_f32(float* dst, const float* w, int Cout, int Cin, int kind, int swap, int flip, void* stream);
int l2i_batch_from_u8_f32(float* out, float* label_out, const uint8_t* src, const float* labels, const int64_t* idx, int B, int64_t N, int64_t elems,
                          int L, void* stream);

/* ---- PGGAN-256 generator (BASELINE config 1; reference graphs/pggan/model_256.py) ----
 * PixelNorm fused with the LeakyReLU that follows it (model_256.py:78-84, 128-150) on [B,C,HW] maps:
 *   y = lrelu(x / sqrt(mean_c x^2 + eps), slope)      (slope = 1: the plain PixelNorm of the latent code, model_256.py:230)
 * and its backward given gy = dL/dy and the forward INPUT x. */
int l2i_pixelnorm_act_f32(float* y, const float* x, int B, int C, int64_t HW, float eps, float slope, void* stream);
int l2i_pixelnorm_act_bwd_f32(float* dx, const float* gy, const float* x, int B, int C, int64_t HW, float eps, float slope, void* stream);
/* F.upsample(scale_factor=2) (nearest, model_256.py:240) on [planes,H,W] -> [planes,2H,2W], times `scale` (scale 0.25 = the adjoint of the
 * 2x2 mean below); and y[i,j] = scale * sum of the 2x2 window of x [planes,2*OH,2*OW] (scale 0.25 = F.upsample(size=half, bilinear) of
 * graphs/pggan/transform_base.py:320; scale 1 = the adjoint of the nearest upsample).  Even widths only. */
int l2i_upsample2x_nearest_f32(float* y, const float* x, int64_t planes, int H, int W, float scale, void* stream);
int l2i_pool2x2_f32(float* y, const float* x, int64_t planes, int OH, int OW, float scale, void* stream);

/* ---- style-dependent vectors of a generator pass (networks.py:148-156 EqualLinear modulation, :231-239 demodulation, and their gradients) ----
 * Segmented mat-vec:  out[b, r] = epi( sum over the segment's parts of  sum_k pre(in)[b, k] * w[w_off + k * w_pitch + r] ),  r < rows, b < B.
 * One launch evaluates every layer of a kind (all modulations s = w A^T + bias and the ToRGB weights; all demodulation factors; all
 * d s; the whole latent gradient).  `segs` / `block_seg` are DEVICE arrays built once per network (latent2im_amd/generator.py): block i works
 * on rows block_seg[2i+1]*64 .. +63 of segment block_seg[2i].  Offsets that scale with the batch are (constant, per-sample) pairs:
 * offset = off_c + B * off_b.
 *   pre: 0  x = in[idx]                       idx = in_off + b * in_bstride + k
 *        1  x = in[idx]^2                                                              (demodulation: sum s^2 T)
 *        2  x = in[idx] * in2[idx]^2                                                   (d demod * demod^3 = red / demod * demod^3)
 *        3  x = sum_o in2[in_off + (b * K + k) * 3 + o] * wrgb[aux_off + o * K + k]    (ToRGB: d s_rgb from the [B, C, 3] reduction, read from in2)
 *   epi: 0  out = acc + bias[bias_off + r]; if rgb_off_b >= 0 also wmod[B * rgb_off_b + (b * 3 + o) * rows + r] = wrgb[rgb_w_off + o * rows + r] * out
 *        1  out = rsqrt(acc + 1e-8)
 *        2  out = e1[e] - e2[e] * acc          e = e_off + b * e_bstride + r            (d s = q - s * (d demod demod^3) T)
 *        3  out = acc
 * K <= 512 and K % 4 == 0 for every part. */
typedef struct l2i_segmv_part {
    int32_t K, in_off_c, in_off_b, in_bstride, w_pitch, pre, aux_off, pad_;
    int64_t w_off;
} l2i_segmv_part;
typedef struct l2i_segmv_seg {
    int32_t rows, nparts, out_off_c, out_off_b, out_bstride, epi, bias_off, e_off_c, e_off_b, e_bstride, rgb_off_b, rgb_w_off;
    l2i_segmv_part part[2];
} l2i_segmv_seg;
int l2i_segmented_matvec_f32(float* out, const float* in, const float* in2, const float* w, const float* bias, const float* e1, const float* e2,
                             float* wmod, const float* wrgb, const l2i_segmv_seg* segs, const int32_t* block_seg, int nblocks, int B, void* stream);

/* ---- ABI version 6: the optimiser tail of the walk step on the fp16 path (l2i_optim.hip) ------------------------------------------------------
 * The reference ends a step with torch.optim.Adam on the walk tensor (transform_base.py:329-331, 487-488); under autocast it would do so through
 * a GradScaler.  These two entry points are that pair without a host synchronisation: all state lives on the device.
 *   state  int32[4]:  [L2I_LS_FOUND] 1 = a gradient of this step held an inf / NaN, [L2I_LS_TRACKER] clean steps since the last scale change,
 *                     [L2I_LS_SKIPPED] updates skipped so far, [L2I_LS_STEPS] steps seen so far
 *   scale  float[2]:  [0] the dynamic loss-scale factor (a power of two; multiplies every loss branch's incoming gradient), [1] its inverse */
#define L2I_LS_FOUND 0
#define L2I_LS_TRACKER 1
#define L2I_LS_SKIPPED 2
#define L2I_LS_STEPS 3
/* state[L2I_LS_FOUND] |= any(!isfinite(g[0..n))).  For walks with several parameter tensors: one call per gradient before the first update. */
int l2i_nonfinite_flag_f32(const float* g, int64_t n, int32_t* state, void* stream);
/* One Adam update of p (moments m, v; step = float step counter on the device) with torch.optim.Adam's arithmetic (no weight decay, no amsgrad),
 * SKIPPED — p, m, v, step untouched — when state[L2I_LS_FOUND] is set or (check_self) g itself holds an inf / NaN.  last != 0: afterwards the
 * scale state advances as torch._amp_update_scale_ does (found: scale[0] *= backoff, tracker = 0, skipped += 1; clean: ++tracker == interval ->
 * scale[0] = min(scale[0] * growth, max_scale) and tracker = 0), scale[1] = 1 / scale[0], steps += 1, and the flag is cleared.  scale may be NULL. */
int l2i_adam_guarded_f32(float* p, const float* g, float* m, float* v, float* step, int64_t n, float lr, float beta1, float beta2, float eps,
                         int32_t check_self, int32_t* state, float* scale, float growth, float backoff, int32_t interval, float max_scale,
                         int32_t last, void* stream);
/* The same pair over a TABLE of tensors, many blocks a launch (the PGGAN graph's MLP walk: 2.1 M parameters in six tensors).  The table is passed
 * to the kernels by value, so a captured graph bakes it in and no device-side descriptor exists.  Added under ABI 12: nothing existing changed. */
#define L2I_ADAM_MAX_TENSORS 16
typedef struct l2i_adam_tensor { float* p; const float* g; float* m; float* v; float* step; int64_t n; } l2i_adam_tensor;
/* state[L2I_LS_FOUND] = 1 if any g of tensors[0..count) holds an inf / NaN: ONE launch, ceil(n / 4096) blocks a tensor; only g and n are read.
 * Refused with L2I_E_ARG: a null table or state, count outside 1..L2I_ADAM_MAX_TENSORS, a null g, n <= 0. */
int l2i_nonfinite_flag_multi_f32(const l2i_adam_tensor* tensors, int32_t count, int32_t* state, void* stream);
/* The guarded Adam update of tensors[0..count), bit for bit what l2i_adam_guarded_f32(check_self = 0) computes tensor by tensor (same device
 * function), each tensor with its own step counter: one multi-block update launch that reads state[L2I_LS_FOUND] and the counters and writes
 * neither, then a one-wave launch that adds 1 to every counter when the flag is clear and, with last != 0, advances the scale state and clears
 * the flag exactly as above.  16-byte accesses where p, g, m and v of a tensor share their offset to a 16-byte boundary, element by element
 * otherwise; 4-byte alignment is enough.  Call l2i_nonfinite_flag_multi_f32 on every tensor of the step first.  Refused with L2I_E_ARG: as
 * above, plus a null p, m, v or step, betas outside [0, 1), eps < 0, a scale with growth < 1 or backoff outside (0, 1]. */
int l2i_adam_guarded_multi_f32(const l2i_adam_tensor* tensors, int32_t count, float lr, float beta1, float beta2, float eps, int32_t* state,
                               float* scale, float growth, float backoff, int32_t interval, float max_scale, int32_t last, void* stream);
/* [ABI 12] The momentum-SGD twin (BP.py:140: torch.optim.SGD(lr, momentum), dampening 0, no Nesterov, no weight decay), same single 1024-thread block.
 * With t = step[0] (a float counter on the device): t == 0: buf = g; otherwise buf = fl(fl(momentum * buf) + g); then p = fl(p - fl(lr * buf)) and
 * step[0] = t + 1 — every product and sum rounded to float32 on its own, no contraction.  "First step" is read from the device, so a captured graph
 * replays the call; a skipped first step leaves the counter at 0 and the next applied one initialises buf.  The guard is l2i_adam_guarded_f32's,
 * word for word: SKIPPED — p, buf, step untouched — when state[L2I_LS_FOUND] is set or (check_self) g itself holds an inf / NaN (which then sets
 * the flag for the next tensor); last != 0 advances the scale state as above and clears the flag; scale may be NULL.  Refused with L2I_E_ARG
 * before any launch: a null p, g, buf, step or state, n <= 0, momentum outside [0, 1), lr negative or non-finite, a scale with growth < 1 or
 * backoff outside (0, 1]. */
int l2i_sgd_guarded_f32(float* p, const float* g, float* buf, float* step, int64_t n, float lr, float momentum, int32_t check_self, int32_t* state,
                        float* scale, float growth, float backoff, int32_t interval, float max_scale, int32_t last, void* stream);

/* [ABI 7] The regressor head and its BCE term in one launch (csrc/l2i_loss.hip) — transform_base.py:416-424: pred = fc(feat)[:, cols]; loss =
 * -mean(y log(max(pred, eps)) + (1 - y) log(max(1 - pred, eps))) (fp32 logs, float64 sum, like the torch expression on an fp32 pred and a float64 y).
 * feat [B, F], fc_w [A, F], fc_b [A] fp32; cols [K] int64 (K <= 64); target [B, K] float64 (target_f64 = 1) or fp32.  Writes loss[0] (float64), preds [B, K] and
 * g_feat [B, F] = d loss / d feat for an upstream gradient of 1 (clamp passes the gradient where its argument >= eps, as torch.clamp does).
 * A NaN prediction (a non-finite feature) is kept by the clamp, as torch.clamp keeps it: preds holds the NaN, loss[0] is NaN, and that
 * prediction contributes 0 to g_feat (neither comparison with eps holds).  Held to tests/regbce_ref.py. */
int l2i_reg_bce_f32(double* loss, float* preds, float* g_feat, const float* feat, const float* fc_w, const float* fc_b, const int64_t* cols,
                    const void* target, int target_f64, int B, int F, int K, float eps, void* stream);

/* [ABI 12, additive] l2i_reg_bce_f32 with the attribute-preservation term of walk training in the same launch (csrc/l2i_loss.hip; --attr_keep):
 * feat1 / feat0 [B, F] fp32 are the pooled features of the edited and of the original image, keep_cols [M] int64 (1 <= M <= 64) the regressor
 * outputs to hold still.  p1[b, j] / p0[b, j] = fc(feat1[b]) / fc(feat0[b]) at keep_cols[j], both by one dot-product routine in one summation order
 * (bitwise equal rows give bitwise equal outputs); d = fl32(p1 - p0); keep = sum_bj |d| / (B M), a float64 sum of fp32 values in a fixed order (b then j
 * ascending; no float atomics: two launches give equal bits); d keep / d p1 = sign(d) / (B M) in fp32, 0 where d == 0 (torch.abs's subgradient) and
 * where d is NaN (keep is then NaN).  The BCE part is l2i_reg_bce_f32's arithmetic on feat1, cols [K], target [B, K]; K = 0: no BCE part, preds, cols
 * and target may be NULL.  Writes loss[3] (float64) = {reg, keep, c_reg reg + w_keep keep} ({0, keep, w_keep keep} for K = 0), preds [B, K], pkeep
 * [B, M, 2] = (p1, p0), and g_feat [B, F] = sum_k c_reg g_bce_pred[b, k] fc_w[cols[k]] + sum_j w_keep g_keep_pred[b, j] fc_w[keep_cols[j]] =
 * d loss[2] / d feat1 for an upstream gradient of 1.  Refused with L2I_E_ARG before any launch, nothing written: a null loss, pkeep, g_feat, feat1,
 * feat0, fc_w, fc_b or keep_cols; B or F <= 0; M < 1, M > 64, K < 0, K > 64; K > 0 with a null preds, cols or target.  Every entry of cols and
 * keep_cols is a row of fc_w: the caller checks that.  Held to tests/regkeep_ref.py. */
int l2i_reg_bce_keep_f32(double* loss, float* preds, float* pkeep, float* g_feat, const float* feat1, const float* feat0, const float* fc_w,
                         const float* fc_b, const int64_t* cols, const void* target, int target_f64, const int64_t* keep_cols, int B, int F, int K,
                         int M, float c_reg, float w_keep, float eps, void* stream);

/* [ABI 8] The identity-preservation half of eval.py (csrc/l2i_face.hip; eval.py:170-209, latent2im_amd/facenet.py).
 * l2i_face_resize_f32: the generator's image -> the face network's input, bit-identical to the reference's clip_ims followed by PIL's
 *   Image.resize((OW, OH)) (bicubic a = -0.5, antialiased): x [planes, H, W] fp32 in [-1, 1] is quantised with clip_ims' float32 arithmetic
 *   (np.uint8(np.clip(((x + 1) / 2.0) * 255, 0, 255))), resized horizontally to a uint8 intermediate, then vertically; y [planes, OH, OW] fp32
 *   holds the resulting 0..255 bytes.  Each pass is PIL's fixed-point form: acc = 2^21 + sum_t q[first + t] * coef[o * k + t] (int32),
 *   clip(acc >> 22, 0, 255).  xbounds [OW, 2] / ybounds [OH, 2] = (first input pixel, tap count) and xcoef [OW, xk] / ycoef [OH, yk] int32 are
 *   PIL's tables of the axis (22-bit coefficients normalised in double; latent2im_amd/facenet.py:resize_tables), device pointers.  Equal sizes
 *   give identity tables: the image is a copy.  Built for inputs <= 4096 and outputs <= 256 pixels a side with <= 256 taps, where the input
 *   rows 16 output rows read fit 48 KiB of LDS as bytes (square inputs up to ~2048 onto 160); other shapes return L2I_E_UNSUPPORTED.
 * l2i_face_head_f32: InceptionResnetV1's head for the whole batch: emb[b, :] = F.normalize(w_t^T mean_hw(feat[b]) + bias) (eps 1e-12), feat
 *   [B, C, HW], w_t [C][E] = last_linear.weight^T with last_bn's eval-mode scale folded into its columns, bias [E] = last_bn's folded shift;
 *   emb [B, E] fp32.  npairs > 0: B == 2 * npairs, rows p and p + npairs are an (edited, original) pair and dist[p] (float64) =
 *   scipy.spatial.distance.cosine of the two embeddings taken as float64 vectors (1 - uv / sqrt(uu vv), float64 sums, clipped to [0, 2]);
 *   npairs = 0: dist is not touched (may be NULL).  Built for C <= 2048 and E <= 512; other shapes return L2I_E_UNSUPPORTED. */
int l2i_face_resize_f32(float* y, const float* x, int64_t planes, int H, int W, int OH, int OW, const int32_t* xbounds, const int32_t* xcoef,
                        int xk, const int32_t* ybounds, const int32_t* ycoef, int yk, void* stream);
int l2i_face_head_f32(float* emb, double* dist, const float* feat, const float* w_t, const float* bias, int B, int C, int HW, int E, int npairs,
                      void* stream);

/* The differentiable twin of the pair above: the face branch of walk training's identity loss (--id_loss; latent2im_amd/facenet.py:FaceIdFn).
 * Additive: the ABI version did not move.  No floating-point atomics; every sum has a fixed order, so two launches give equal bits.
 * l2i_face_resize_lin_f32: the arguments, tables and shape range of l2i_face_resize_f32 (it refuses the same shapes, nothing written).
 *   u = min(max(((x + 1) * 0.5) * 255, 0), 255) in fp32 (NaN -> 0: clip_ims without the truncating cast), y = Ry u Rx^T per plane with
 *   R = the table / 2^22, horizontal pass first, taps in ascending order: the same taps without the uint8 intermediate, the rounding and the clips.
 *   Both columns of ybounds (first input row, first + count) must be non-decreasing in the output index, as PIL's are: a block takes the input rows of
 *   its output rows from the first row's start and the last row's end, and taps of a table that breaks the rule outside that range are not read (not
 *   checked: the tables live on the device).
 * l2i_face_resize_lin_bwd_f32: its adjoint as a gather, gx = 127.5 * [0 < ((x + 1) * 0.5) * 255 < 255] * Rx^T (Ry^T gy); gx, x [planes, H, W], gy
 *   [planes, OH, OW].  ixbounds [W, 2] / iybounds [H, 2] = (first output, count) of the outputs whose support holds the input pixel, ixcoef
 *   [W, ixk] / iycoef [H, iyk] int32 their coefficients (the forward tables transposed: latent2im_amd/facenet.py:inverse_tables).  Every gx
 *   element is written once, by one lane.  Inputs <= 4096 and outputs <= 256 pixels a side, <= 256 taps; else L2I_E_UNSUPPORTED.
 * l2i_face_head_bwd_f32: the gradient of dist[b] = 1 - cos(e[b], v[b]) down to the trunk's output.  With p = mean_hw feat, t = w_t^T p + bias,
 *   n = max(|t|, 1e-12), e = t / n (l2i_face_head_f32's embedding, recomputed), v^ = v / |v| (v [B, E]: the other half's embedding, a constant)
 *   and c = e . v^:  g_t = -g_dist[b] (v^ - c e) / n,  g_p = w_t g_t,  g_feat[b, c, :] = g_p[c] / HW;  g_feat [B, C, HW], g_dist [B].  The limits
 *   of l2i_face_head_f32 (C <= 2048, E <= 512). */
int l2i_face_resize_lin_f32(float* y, const float* x, int64_t planes, int H, int W, int OH, int OW, const int32_t* xbounds, const int32_t* xcoef,
                            int xk, const int32_t* ybounds, const int32_t* ycoef, int yk, void* stream);
int l2i_face_resize_lin_bwd_f32(float* gx, const float* gy, const float* x, int64_t planes, int H, int W, int OH, int OW, const int32_t* ixbounds,
                                const int32_t* ixcoef, int ixk, const int32_t* iybounds, const int32_t* iycoef, int iyk, void* stream);
int l2i_face_head_bwd_f32(float* g_feat, const float* feat, const float* w_t, const float* bias, const float* v, const float* g_dist, int B, int C,
                          int HW, int E, void* stream);

/* [ABI 10] The Gram-matrix term of BP.py's inversion loss and its gradient (csrc/l2i_gram.hip; BP.py:68-73, :173-184).
 * l2i_gram_loss_f32: c [B, C, HW] is a tap's PRE-ReLU conv output.  G[b] = relu(c[b]) relu(c[b])^T / (C HW) -> G [B, C, C] (the ReLU is applied on
 *   load; only tile pairs i <= j are contracted, on v_mfma_f32_32x32x2_f32, and the lower triangle is the mirror of the upper one, so G is
 *   symmetric to the bit).  Gt [B, C, C] given: also D[b] = G[b] - Gt[b] -> D [B, C, C] and loss[b] += C^2 * sum(D[b]^2) (loss [B] is
 *   accumulated into: one call per tap).  Gt NULL: only G is written (D, loss may be NULL): the target image's Grams, once per image.
 *   HW is cut into `nslices` slices of whole 256-pixel chunks (1 <= nslices <= ceil(HW / 256)), one block per (slice, tile pair, sample); the
 *   partial tiles go to ws and are added in slice order by a second pass that also forms D and the loss: no floating-point atomics, equal inputs
 *   and equal nslices give equal bits.  ws: B * P * (1024 * nslices + 1) floats of scratch, P = (C / 32)(C / 32 + 1) / 2.
 * l2i_gram_bwd_f32: g[b] (+)= coef * scale[b * scale_stride] * (c[b] > 0) * (D[b] relu(c[b])), g [B, C, HW]; D [B, C, C] must be symmetric (it is read as its own
 *   K-major form).  For the loss above coef = 4 C / HW.  scale: optional device tensor (the upstream gradient: no host synchronisation), one
 *   element for every sample (scale_stride 0) or one per sample (scale_stride 1: a [B] loss takes its whole batch in one launch);
 *   accumulate != 0 adds into g (the trunk gradient arriving from the deeper taps), else g is overwritten.
 * Both: C % 32 == 0, C <= 512, any HW >= 1 with C * HW * 4 bytes < 4 GiB, any B; other shapes return L2I_E_UNSUPPORTED.  HW % 4 == 0 with a
 * 16-byte aligned c takes the LDS-DMA path, anything else a scalar-load path of the same arithmetic. */
int l2i_gram_loss_f32(float* G, float* D, float* loss, const float* c, const float* Gt, float* ws, int B, int C, int HW, int nslices, void* stream);
int l2i_gram_bwd_f32(float* g, const float* c, const float* D, const float* scale, float coef, int B, int C, int HW, int accumulate, int scale_stride,
                     void* stream);

/* [ABI 11] The same two on 16-bit h8 taps (csrc/l2i_gram_h8.hip; bf16 elements, and IEEE fp16 with the suffix _f16).  c, g: [B][C/8][HW][8];
 * G, D, Gt [B, C, C], loss [B], scale, ws (same size) stay fp32.
 * l2i_gram_loss_h8: the semantics, the slicing, the fixed summation order and the bit-symmetric G of l2i_gram_loss_f32.  The products run on
 *   v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulation (a product of two 16-bit elements is exact in fp32); the contraction index is the pixel,
 *   which h8 strides, so both operands are staged [pixel][channels] in LDS and read transposed (ds_read_b64_tr_b16).
 * l2i_gram_bwd_h8: g (+)= coef * scale[b * scale_stride] * (c > 0) * (D relu(c)) with g in h8.  D is multiplied by coef * scale[b] in fp32 and THEN
 *   rounded to the element type (the gradient scale protects it from fp16 underflow); the sum is fp32; accumulate != 0 adds the h8 gradient
 *   already in g in fp32, so the store is the only rounding of the sum.  D need not be symmetric here.
 * Both: C % 32 == 0, C <= 512, any HW >= 1 with C * HW * 2 bytes < 4 GiB, any B; other shapes return L2I_E_UNSUPPORTED.  c or g off a 16-byte
 * boundary returns L2I_E_ARG (an h8 slot is 16 bytes: there is no unaligned path). */
int l2i_gram_loss_h8(float* G, float* D, float* loss, const void* c, const float* Gt, float* ws, int B, int C, int HW, int nslices, void* stream);
int l2i_gram_loss_h8_f16(float* G, float* D, float* loss, const void* c, const float* Gt, float* ws, int B, int C, int HW, int nslices, void* stream);
int l2i_gram_bwd_h8(void* g, const void* c, const float* D, const float* scale, float coef, int B, int C, int HW, int accumulate, int scale_stride,
                    void* stream);
int l2i_gram_bwd_h8_f16(void* g, const void* c, const float* D, const float* scale, float coef, int B, int C, int HW, int accumulate, int scale_stride,
                        void* stream);

/* PixelNorm + LeakyReLU of the PGGAN-256 generator on 16-bit h8 maps (csrc/l2i_pggan_h8.hip; bf16 elements, and IEEE fp16 with the suffix _f16;
 * additive to ABI 12).  x [B][C/8][H][W][8]; the function, eps and slope of l2i_pixelnorm_act_f32 / _bwd_f32; the mean divides by C.
 * l2i_pixelnorm_act_h8: up = 1: y is shaped like x.  up = 2: y is [B][C/8][2H][2W][8] and every result is written to its four positions (the
 *   nearest 2x upsample that follows every block but the last).  y_low (may be NULL): the 1x map as well, bit-identical to y where they coincide.
 * l2i_pixelnorm_act_bwd_h8: dx = r g' - x r^3 sum_c(g' x) / C with r = 1 / sqrt(mean_c x^2 + eps), g' = g (x > 0 ? 1 : slope); pool = 1: g = gy
 *   (shaped like x); pool = 2: gy is [B][C/8][2H][2W][8] and g is the fp32 sum of its 2x2 window (the upsample's adjoint; no pooled map is
 *   stored).  addend (may be NULL; h8, shaped like x) is added to g in fp32.
 * Both: fp32 arithmetic, one rounding at the store, fixed summation order (no atomics: equal inputs give equal bits).  An all-zero column gives
 * y = 0 and dx = g' / sqrt(eps).  C % 8 != 0, C > 512 or up / pool outside {1, 2} return L2I_E_UNSUPPORTED; a NULL y, x, dx or gy, a
 * non-positive dimension or a map off a 16-byte boundary returns L2I_E_ARG; nothing is launched then. */
int l2i_pixelnorm_act_h8(void* y, void* y_low, const void* x, int B, int C, int H, int W, float eps, float slope, int up, void* stream);
int l2i_pixelnorm_act_h8_f16(void* y, void* y_low, const void* x, int B, int C, int H, int W, float eps, float slope, int up, void* stream);
int l2i_pixelnorm_act_bwd_h8(void* dx, const void* gy, const void* x, const void* addend, int B, int C, int H, int W, float eps, float slope, int pool,
                             void* stream);
int l2i_pixelnorm_act_bwd_h8_f16(void* dx, const void* gy, const void* x, const void* addend, int B, int C, int H, int W, float eps, float slope, int pool,
                                 void* stream);

/* ---- [ABI 12, additive] Training on 16-bit h8 maps: the weight gradient of a convolution and training-mode BatchNorm (csrc/l2i_train_h8.hip; bf16
 * elements, and IEEE fp16 with the suffix _f16).  Maps are h8 [B][C/8][H][W][8] on 16-byte boundaries.  No floating-point atomics: every sum has
 * a fixed order, so two calls on the same inputs give the same bits.  Nothing is allocated: the caller passes the workspaces.
 * l2i_conv2d_wgrad_h8: dw[co,ci,ky,kx] = out_scale * sum_{b,oy,ox} gy[b,co,oy,ox] * x[b,ci,oy*stride+ky-pad,ox*stride+kx-pad], products on
 *   v_mfma_f32_32x32x16 (exact in fp32), fp32 accumulation: per 64-pixel wave strip, the four waves of a block, then the pixel slices in slice order.
 *   dw fp32 [Cout][Cin][K][K] is OVERWRITTEN (no zeroed buffer needed).  out_scale = the host float, times *out_scale_dev when that pointer is not
 *   NULL (read on the device at run time: the inverse of a dynamic loss scale).  ws: ws_bytes >= what l2i_conv2d_wgrad_ws_h8 returns for the shape.
 *   Built for K in {1, 3}, stride in {1, 2}, pad in {0, 1}, Cin % 32 == 0, Cout % 32 == 0, OH / OW the conv's output size, x and gy below 4 GiB
 *   each: everything else, a NULL ws and a ws too small return L2I_E_UNSUPPORTED with a message and launch nothing.
 * l2i_conv2d_wgrad_ws_h8 (host only): *bytes = the workspace of that shape (0 and L2I_E_UNSUPPORTED for a refused shape).
 * l2i_bn_stats_h8: sum[c], sumsq[c] (float64, OVERWRITTEN) of the stored elements of x over (b, pixel): what l2i_bn_finalize_f32 reads.
 * l2i_bn_apply_h8: y = relu?(x * scale[c] + shift[c] (+ residual)), fp32 arithmetic, one rounding at the store; residual (h8) may be NULL.
 * l2i_bn_bwd_reduce_h8: sum_dy[c] = sum dy, sum_dyxh[c] = sum dy * xhat (float64, OVERWRITTEN) with dy = gy * (out_mask > 0) when out_mask (h8, may be
 *   NULL) is given, xhat = (x - mean[c]) * invstd[c] in fp32: what l2i_bn_bwd_finalize_f32 reads.
 * l2i_bn_bwd_apply_h8: dx = gamma[c] * invstd[c] * (dy - mean_dy[c] - xhat * mean_dyxh[c]) stored h8; dy_masked (h8, may be NULL) receives dy.
 * l2i_bn_ws_h8 (host only): *bytes = the float64 workspace of the two reductions (one row of 16 sums per block, added in block order).
 * All BatchNorm entries: C % 8 == 0, B <= 65535, any HW >= 1; other shapes return L2I_E_UNSUPPORTED, a NULL or misaligned pointer or a workspace
 * too small L2I_E_ARG; nothing is launched then. */
int l2i_conv2d_wgrad_h8(float* dw, const void* x, const void* gy, float* ws, int64_t ws_bytes, float out_scale, const float* out_scale_dev, int B, int Cin,
                        int H, int W, int Cout, int OH, int OW, int K, int stride, int pad, void* stream);
int l2i_conv2d_wgrad_h8_f16(float* dw, const void* x, const void* gy, float* ws, int64_t ws_bytes, float out_scale, const float* out_scale_dev, int B, int Cin,
                            int H, int W, int Cout, int OH, int OW, int K, int stride, int pad, void* stream);
int l2i_conv2d_wgrad_ws_h8(int64_t* bytes, int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad);
int l2i_conv2d_wgrad_ws_h8_f16(int64_t* bytes, int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad);
int l2i_bn_ws_h8(int64_t* bytes, int B, int C, int64_t HW);
int l2i_bn_ws_h8_f16(int64_t* bytes, int B, int C, int64_t HW);
int l2i_bn_stats_h8(double* sum, double* sumsq, const void* x, double* ws, int64_t ws_bytes, int B, int C, int64_t HW, void* stream);
int l2i_bn_stats_h8_f16(double* sum, double* sumsq, const void* x, double* ws, int64_t ws_bytes, int B, int C, int64_t HW, void* stream);
int l2i_bn_apply_h8(void* y, const void* x, const float* scale, const float* shift, const void* residual, int relu, int B, int C, int64_t HW, void* stream);
int l2i_bn_apply_h8_f16(void* y, const void* x, const float* scale, const float* shift, const void* residual, int relu, int B, int C, int64_t HW, void* stream);
int l2i_bn_bwd_reduce_h8(double* sum_dy, double* sum_dyxh, const void* gy, const void* out_mask, const void* x, const float* mean, const float* invstd,
                         double* ws, int64_t ws_bytes, int B, int C, int64_t HW, void* stream);
int l2i_bn_bwd_reduce_h8_f16(double* sum_dy, double* sum_dyxh, const void* gy, const void* out_mask, const void* x, const float* mean, const float* invstd,
                             double* ws, int64_t ws_bytes, int B, int C, int64_t HW, void* stream);
int l2i_bn_bwd_apply_h8(void* dx, void* dy_masked, const void* gy, const void* out_mask, const void* x, const float* mean, const float* invstd,
                        const float* gamma, const float* mean_dy, const float* mean_dyxh, int B, int C, int64_t HW, void* stream);
int l2i_bn_bwd_apply_h8_f16(void* dx, void* dy_masked, const void* gy, const void* out_mask, const void* x, const float* mean, const float* invstd,
                            const float* gamma, const float* mean_dy, const float* mean_dyxh, int B, int C, int64_t HW, void* stream);

/* ---- [ABI 12, additive] The 16-bit trainer's stem gradient and its weight planes (csrc/l2i_train_h8.hip; bf16 elements, IEEE fp16 with _f16) --------
 * l2i_conv2d_wgrad_img_h8: dw[co,ci,ky,kx] = sum_{b,oy,ox} gy[b,co,oy,ox] * x[b,ci,2 oy+ky-3,2 ox+kx-3] for the 7x7 / stride 2 / pad 3 stem.  x is
 *   the fp32 NCHW image [B][3][H][W] and enters the products as the fp32 value it is (reads in the padding give 0); gy is an h8 map
 *   [B][8][OH][OW][8] on a 16-byte boundary, OH = (H-1)/2+1, OW = (W-1)/2+1; dw fp32 [64][3][7][7] is OVERWRITTEN, in the units of gy (no scale).
 *   v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation in a fixed order (pixel pairs of a wave, the four waves of a block, then the
 *   pixel slices in slice order through ws): no atomics, equal inputs give equal bits.  Built for Cin == 3, Cout == 64, K == 7, stride == 2,
 *   pad == 3, any H, W >= 1, x and gy below 4 GiB each: everything else, a NULL ws and a ws smaller than the query's answer return
 *   L2I_E_UNSUPPORTED, a NULL tensor or a misaligned pointer L2I_E_ARG, with a message; nothing is launched then.
 * l2i_conv2d_wgrad_img_ws_h8 (host only): *bytes = the workspace of the shape = slices * L2I_WGRAD_IMG_SLICE_BYTES (0 and L2I_E_UNSUPPORTED for a
 *   refused shape).
 * l2i_repack_planes_h8: every 16-bit weight plane set of a net, rewritten in place from fp32 weights by ONE launch on `stream`.  `table` (device,
 *   8-byte aligned): nseg rows of eight int64 — destination (device address, 16-byte aligned), weight (device address of fp32
 *   [Cout][Cin][K][K]), Cout, Cin, K, mode, contraction padding qpad, first block of the segment (ascending, row 0 = 0); `nblocks` = grid size
 *   (blocks of a segment = the next row's first block - its own, each at least 1; they walk the segment grid-stride).
 *     mode L2I_PLANES_FWD   dst [ceil(Cin/qpad)*qpad/16][K*K][2][ceil32(Cout)][8], qpad in {16, 32}:
 *                           element (g, t, half, co, e) = rnd(w[co][16g+8half+e][t/K][t%K])
 *     mode L2I_PLANES_SWAP  the same with co and ci exchanged (dst [ceil32(Cout)/16][K*K][2][ceil32(Cin)][8]; qpad 32): the input-gradient planes of
 *                           stride-2 and transposed layers
 *     mode L2I_PLANES_FLIP  exchanged and the taps reversed (t -> K*K-1-t; qpad 32): the input-gradient planes of stride-1 layers
 *     mode L2I_PLANES_IMG   l2i_conv_img_h8's planes for Cin <= 4, K <= 8: dst [ceil(Cin*K/2)][1][2][ceil32(Cout)][8],
 *                           element (s, half, co, e) = rnd(w[co][c][ky][e]) with (c, ky) = divmod(2s+half, K)
 *   Every slot of dst is written; padding rows, padding channels and e >= K are zeros.  rnd = round to nearest even to the element type
 *   (subnormals kept, overflow to inf).  One lane writes one 16-byte slot; nothing is allocated.  The table lives on the device and is not read by
 *   the host: its rows are the caller's responsibility (conv.PlaneTable builds and checks them).  A NULL or misaligned table, nseg < 1 or
 *   nblocks < nseg return L2I_E_ARG and launch nothing. */
#define L2I_WGRAD_IMG_SLICE_BYTES (64 * 160 * 4)
#define L2I_PLANES_FWD 0
#define L2I_PLANES_SWAP 1
#define L2I_PLANES_FLIP 2
#define L2I_PLANES_IMG 3
int l2i_conv2d_wgrad_img_h8(float* dw, const float* x, const void* gy, float* ws, int64_t ws_bytes, int B, int Cin, int H, int W, int Cout, int OH, int OW,
                            int K, int stride, int pad, void* stream);
int l2i_conv2d_wgrad_img_h8_f16(float* dw, const float* x, const void* gy, float* ws, int64_t ws_bytes, int B, int Cin, int H, int W, int Cout, int OH,
                                int OW, int K, int stride, int pad, void* stream);
int l2i_conv2d_wgrad_img_ws_h8(int64_t* bytes, int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad);
int l2i_conv2d_wgrad_img_ws_h8_f16(int64_t* bytes, int B, int Cin, int H, int W, int Cout, int OH, int OW, int K, int stride, int pad);
int l2i_repack_planes_h8(const void* table, int nseg, int nblocks, void* stream);
int l2i_repack_planes_h8_f16(const void* table, int nseg, int nblocks, void* stream);

/* ---- [ABI 12, additive] the linear layers of the PGGAN graph's MLP walk (csrc/l2i_walk.hip; WalkMlpZ3, graphs/pggan/transform_base.py:167-188) ------
 * Skinny products on plain fp32 VALU: B rows (any B >= 1, taken in chunks of at most 16) against W in nn.Linear's own [N = out, K = in] layout.
 * l2i_linear_rows_f32:      y[B, N] = epi(x[B, K] W^T + bias[N]).  epi = L2I_LINEAR_NONE; L2I_LINEAR_LRELU: v > 0 ? v : v * slope; L2I_LINEAR_WALK: the
 *   walk's tail y = res[b, n] + a[b] * v (res [B, N] the residual z, a [B] the per-row alpha; both NULL otherwise).
 * l2i_linear_rows_bwd_f32:  one pass over the layer's [N, K] index space.  g [B, N] = the gradient at the layer's output; g' = g * (y > 0 ? 1 : slope)
 *   for L2I_LINEAR_LRELU (y [B, N] = the layer's activated output: the mask of an in-place LeakyReLU, y == 0 takes the slope), g' = a[b] * g for
 *   L2I_LINEAR_WALK (the residual's own gradient is not formed here), g' = g for L2I_LINEAR_NONE.  Writes gw[n, k] = sum_b g'[b, n] x[b, k], gb[n] =
 *   sum_b g'[b, n] (gb may be NULL) and, when gx is not NULL, gx[b, k] = sum_n g'[b, n] W[n, k] + gx_add[b, k] (gx_add [B, K] may be NULL: the
 *   residual path of the first layer).  N is cut into `slices` equal slices (N % slices == 0, at most 64 rows each); with slices > 1 the slices'
 *   shares of gx go to ws (slices * B * K floats) and a second kernel of the same call adds them in slice order.  Without gx, w and ws are not read.
 * Both: no floating-point atomics — b ascending, n ascending within a slice, slices ascending: equal inputs and equal `slices` give equal bits; no
 * host synchronisation, nothing allocated.  K % 64 != 0 or N % 64 != 0, a non-positive size, an unknown epi, a missing operand, or x / w / gw / gx /
 * ws / gx_add off a 16-byte boundary (they are accessed as float4) return L2I_E_ARG before a launch. */
#define L2I_LINEAR_NONE 0
#define L2I_LINEAR_LRELU 1
#define L2I_LINEAR_WALK 2
int l2i_linear_rows_f32(float* y, const float* x, const float* w, const float* bias, const float* res, const float* a, int B, int K, int N, int epi,
                        float slope, void* stream);
int l2i_linear_rows_bwd_f32(float* gw, float* gb, float* gx, float* ws, const float* gx_add, const float* g, const float* y, const float* a,
                            const float* x, const float* w, int B, int K, int N, int epi, float slope, int slices, void* stream);

/* ---- Range histogram of a stored map (csrc/l2i_range.hip): the device-side statistic behind nets16.RangeMonitor --------------------------------------
 * x = n consecutive elements of `kind` (an h8 map: every stored element, channel padding included — zeros, which move neither the maximum nor
 * the non-zero statistics).  row = L2I_RANGE_WORDS 64-bit words on the device; the call ADDS to it and never clears it (the host clears it):
 *   row[0..255]          elements whose value, converted exactly to fp32, has biased exponent field e: field 0 = zeros and fp32 subnormals, field
 *                        255 = inf / NaN; fp16 subnormals land in fields 103..112, fp16's smallest normal in 113
 *   row[L2I_RANGE_ZEROS] elements that are exactly +-0 (a subset of field 0)
 *   row[L2I_RANGE_MAX]   the largest |x| over the FINITE elements as its fp32 bit pattern (an unsigned maximum)
 *   row[L2I_RANGE_CALLS] calls that added to the row;  row[L2I_RANGE_N]  elements added (n summed)
 * Integer adds and maxima only: the row is bit-reproducible whatever the order in which blocks, streams or hipGraph replays arrive.  16-byte loads
 * over the aligned body, single elements in front of and behind it: x needs the alignment of its element type only.  n <= 0, a null pointer, an
 * unknown kind or a misaligned x / row returns L2I_E_ARG; more than 2^40 elements L2I_E_UNSUPPORTED.  Additive: the ABI version did not move. */
#define L2I_RANGE_F16 0      /* IEEE fp16 elements (h8 maps of the f16 path) */
#define L2I_RANGE_BF16 1
#define L2I_RANGE_F32 2
#define L2I_RANGE_WORDS 260
#define L2I_RANGE_ZEROS 256
#define L2I_RANGE_MAX 257
#define L2I_RANGE_CALLS 258
#define L2I_RANGE_N 259
int l2i_range_stats(uint64_t* row, const void* x, int64_t n, int kind, void* stream);

/* Panel grids as uint8 on the device (csrc/l2i_panels.hip; the reference's utils/image.py: clip_ims and imgrid).
 * out [G][GH][GW][C] uint8, channel-last, GH = rows * (H + pad) - pad, GW = cols * (W + pad) - pad: G grids of rows x cols tiles, every tile
 * padded by `pad` pixels on its bottom and right, the last gutter cropped.  x [N][C][H][W] fp32, C in {1, 3}.  tile_src [G * rows * cols] int32 on
 * the device, row-major over (grid, tile row, tile column), names the image of each tile; an image may be named by several tiles; any value
 * outside [0, N) is an empty tile (defined output, nothing read).  A tile pixel is clip_ims in float32 with numpy's operation order,
 *   t = ((x + 1) * 0.5) * 255 (each operation rounded), clamp to [0, 255], truncate; NaN -> 0,
 * gutters and empty tiles are `fill` (0..255).  The launch owns out: every byte of it is written exactly once, from its sources alone (out is
 * never read, so neighbouring tiles may share a dword), and nothing outside it is touched.  out may have any byte alignment (16-byte stores
 * between its first and last 16-byte boundary, byte stores in front of and behind them), x any 4-byte alignment; every offset is 64-bit.
 * L2I_E_UNSUPPORTED: another C, pad < 0, fill outside 0..255, a dimension (G, rows, cols, H, W, N) < 1, x off a 4-byte boundary, or a grid side
 * in bytes, a plane or the tile table beyond 2^30.  L2I_E_ARG: a null pointer.  Nothing is launched then.  Additive: the ABI version did not move. */
int l2i_panels_u8(uint8_t* out, const float* x, const int32_t* tile_src, int G, int rows, int cols, int C, int H, int W, int pad, int fill, int N,
                  void* stream);

const char* l2i_last_error(void);
/* Bumped whenever a struct of this header grows or an entry point changes meaning (1: round 1-2; 2: round 3, l2i_conv_params gained w_bstride /
 * out_f32; 3: round 4: l2i_conv2d_wino4_f32, l2i_sizeof_conv_params; 4: round 5: the l2i_*_h8_f16 entry points, wino4 tile_hint / CoutP % 32; 5: round 5: in_h8 / rgb_* fields, l2i_conv_img_h8; 6: round 6: l2i_nonfinite_flag_f32 / l2i_adam_guarded_f32, mask_out / mask_bits fields, l2i_mask_mul_bits_h8, the mask_bits argument of l2i_upfirdn2d_h8; 7: round 6: l2i_conv1x1_pair_h8, l2i_conv_chain3_h8, l2i_conv1x1_pair_f32, l2i_reg_bce_f32; 8: l2i_face_resize_f32, l2i_face_head_f32; 9: l2i_wino4s_epilogue_class; 10: l2i_gram_loss_f32, l2i_gram_bwd_f32; 11: l2i_gram_loss_h8, l2i_gram_bwd_h8 and their _f16 twins; 12: l2i_sgd_guarded_f32).  The ctypes binding (latent2im_amd/_lib.py) refuses a library whose version or struct size differs from its own mirror. */
#define L2I_ABI_VERSION 12
int l2i_abi_version(void);
int l2i_sizeof_conv_params(void);       /* sizeof(struct l2i_conv_params) of THIS build */

#ifdef __cplusplus
}
#endif
#endif /* L2I_H */
