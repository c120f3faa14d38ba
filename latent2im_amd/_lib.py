"""ctypes binding of libl2i_hip.so (the C ABI declared in include/l2i.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is no CPU fallback: every
op in this package raises if the library is missing or a kernel call is made without a GPU tensor.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('L2I_LIB') or os.path.join(_HERE, 'libl2i_hip.so')      # L2I_LIB: another build of the library (A/B probes)

ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
LINEAR_NONE, LINEAR_LRELU, LINEAR_WALK = 0, 1, 2      # L2I_LINEAR_*: the epilogues of l2i_linear_rows_f32 / _bwd_f32

c_f = ctypes.c_float
c_i = ctypes.c_int32
c_p = ctypes.c_void_p
c_l = ctypes.c_int64
c_d = ctypes.c_double


class ConvParams(ctypes.Structure):
    """Mirror of ``struct l2i_conv_params`` (include/l2i.h) — field order and types must match."""
    _fields_ = [
        ('x', c_p), ('w', c_p), ('y', c_p),
        ('B', c_i), ('Cin', c_i), ('H', c_i), ('W', c_i), ('Cout', c_i), ('CoutP', c_i),
        ('KH', c_i), ('KW', c_i), ('stride', c_i), ('pad_y', c_i), ('pad_x', c_i),
        ('OH', c_i), ('OW', c_i), ('OHf', c_i), ('OWf', c_i),
        ('oy_step', c_i), ('ox_step', c_i), ('oy_off', c_i), ('ox_off', c_i),
        ('in_scale', c_p), ('in_mask', c_p), ('mask_pos', c_f), ('mask_neg', c_f),
        ('out_scale', c_p), ('noise', c_p), ('noise_w', c_f), ('bias', c_p),
        ('residual', c_p), ('res_mask', c_p), ('out_mask', c_p),
        ('act', c_i), ('act_slope', c_f), ('act_gain', c_f), ('out_gain', c_f),
        ('accumulate', c_i), ('tile_hint', c_i),
        ('w_hi', c_p), ('w_lo', c_p),
        ('ws', c_p), ('ksplit', c_i), ('res_sub', c_p), ('res_coef', c_f), ('res_coef_dev', c_p),
        ('sq_ref', c_p), ('sq_out', c_p),
        ('w_bstride', c_l), ('out_f32', c_i),
        ('in_h8', c_i), ('rgb_w', c_p), ('rgb_bias', c_p), ('rgb_out', c_p), ('pool_out', c_p), ('pool_idx', c_p),
        ('mask_out', c_p), ('mask_bits', c_i),
    ]


SQ_SLOTS = 1024          # L2I_SQ_SLOTS
WINO4S_LEAN_CLASSES = 8   # L2I_WINO4S_LEAN_CLASSES: l2i_wino4s_epilogue_class returns this for the generic body


class SegmvPart(ctypes.Structure):
    """Mirror of ``struct l2i_segmv_part`` (include/l2i.h)."""
    _fields_ = [('K', c_i), ('in_off_c', c_i), ('in_off_b', c_i), ('in_bstride', c_i), ('w_pitch', c_i), ('pre', c_i), ('aux_off', c_i), ('pad_', c_i),
                ('w_off', c_l)]


class SegmvSeg(ctypes.Structure):
    """Mirror of ``struct l2i_segmv_seg`` (include/l2i.h)."""
    _fields_ = [('rows', c_i), ('nparts', c_i), ('out_off_c', c_i), ('out_off_b', c_i), ('out_bstride', c_i), ('epi', c_i), ('bias_off', c_i),
                ('e_off_c', c_i), ('e_off_b', c_i), ('e_bstride', c_i), ('rgb_off_b', c_i), ('rgb_w_off', c_i), ('part', SegmvPart * 2)]


# l2i_conv_transpose2d_f32, K = 3 (include/l2i.h): tile_hint 0 = per shape (the 25-product kernel convt_poly_kernel on the shapes of its measured table
# where ConvParams.w_lo carries its fp32 pack [Cin][25][CoutP] = conv.pack_weight_convt_poly, else the direct kernel); 1 / 2 = the direct kernel's two
# tiles; CONVT_HINT_DIRECT = the direct kernel's automatic tile (as every other value); CONVT_HINT_POLY = the new kernel, L2I_E_UNSUPPORTED where it
# does not take the struct.  l2i_conv_transpose2d_family (host only) says which of TFAMILY_* a struct runs on, assuming the pack is supplied;
# l2i_convt_poly_plan_for (host only) fills ConvtPolyPlan, the new kernel's launch plan.
CONVT_HINT_DIRECT, CONVT_HINT_POLY = 9, 10     # L2I_CONVT_HINT_*
TFAMILY_DIRECT, TFAMILY_POLY, TFAMILY_SMALL = 0, 1, 2      # L2I_TFAMILY_*: l2i_conv_transpose2d_family


class ConvtPolyPlan(ctypes.Structure):
    """Mirror of ``struct l2i_convt_poly_plan`` (include/l2i.h): the launch plan of convt_poly_kernel, a host-side function of the struct."""
    _fields_ = [(n, c_i) for n in ('eligible', 'masked', 'nwx', 'nwy', 'WTW', 'WTH', 'tiles_x', 'tiles_y', 'mblocks', 'total', 'grid',
                                   'IH', 'IW', 'org', 'nslots', 'plane', 'wpitch', 'CK', 'stage_floats', 'lds_bytes')]


H8_EPI_LEAN, H8_EPI_GENERAL, H8_EPI_F32_VEC, H8_EPI_F32_SCALAR = 0, 1, 2, 3      # L2I_H8_EPI_*: l2i_conv_h8_plan.epilogue


class ConvH8Plan(ctypes.Structure):
    """Mirror of ``struct l2i_conv_h8_plan`` (include/l2i.h): the instantiation, epilogue and grid l2i_conv2d_h8 / l2i_conv_transpose2d_h8 run a
    struct with, a host-side function of the struct (l2i_conv_h8_plan_for)."""
    _fields_ = [(n, c_i) for n in ('eligible', 'WM', 'WN', 'KS', 'K', 'S', 'TR', 'out32', 'relu_in', 'extra', 'rgb', 'epilogue', 'nchunks', 'tiles_x',
                                   'tiles_y', 'mblocks', 'total', 'grid', 'lds_bytes')]


def conv_h8_plan(p, transposed=False):
    """The ConvH8Plan of ConvParams ``p`` (no launch, no GPU); plan.eligible == 0 where the entry refuses the struct."""
    plan = ConvH8Plan()
    check(load().l2i_conv_h8_plan_for(ctypes.byref(p), int(bool(transposed)), ctypes.byref(plan)), 'l2i_conv_h8_plan_for')
    return plan


ADAM_MAX_TENSORS = 16     # L2I_ADAM_MAX_TENSORS


class AdamTensor(ctypes.Structure):
    """Mirror of ``struct l2i_adam_tensor`` (include/l2i.h): one row of the table the multi-tensor guarded Adam takes."""
    _fields_ = [('p', c_p), ('g', c_p), ('m', c_p), ('v', c_p), ('step', c_p), ('n', c_l)]


REPACK_MAX_TAPS = 49      # L2I_REPACK_MAX_TAPS
REPACK_PACKED, REPACK_OIHW = 0, 1      # L2I_REPACK_*: the layouts of l2i_repack_taps_f32
REPACK_WINO2, REPACK_WINO4 = 2, 4      # the kinds of l2i_repack_wino_f32


class RepackTaps(ctypes.Structure):
    """Mirror of ``struct l2i_repack_taps`` (include/l2i.h): the by-value (ky, kx) table of l2i_repack_taps_f32."""
    _fields_ = [('count', c_i), ('ky', ctypes.c_uint8 * REPACK_MAX_TAPS), ('kx', ctypes.c_uint8 * REPACK_MAX_TAPS)]


def repack_taps(taps):
    """RepackTaps of [(ky, kx)] (at most REPACK_MAX_TAPS: the entry point refuses more, the mirror has no room for them)."""
    t = RepackTaps()
    t.count = len(taps)
    for i, (ky, kx) in enumerate(taps[:REPACK_MAX_TAPS]):
        t.ky[i], t.kx[i] = ky, kx
    return t


_SIGNATURES = {
    'l2i_conv2d_f32': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv2d_family': (c_i, [ctypes.POINTER(ConvParams)]),
    'l2i_conv_transpose2d_f32': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv_transpose2d_family': (c_i, [ctypes.POINTER(ConvParams)]),
    'l2i_convt_poly_plan_for': (c_i, [ctypes.POINTER(ConvParams), ctypes.POINTER(ConvtPolyPlan)]),
    'l2i_conv2d_bf16x3_f32': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv_transpose2d_bf16x3_f32': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv2d_wino_f32': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv2d_wino4_f32': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_wino4s_epilogue_class': (c_i, [ctypes.POINTER(ConvParams)]),
    'l2i_conv1x1_pair_f32': (c_i, [ctypes.POINTER(ConvParams), ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv2d_h8': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv_transpose2d_h8': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv_h8_plan_for': (c_i, [ctypes.POINTER(ConvParams), c_i, ctypes.POINTER(ConvH8Plan)]),
    'l2i_conv_img_h8': (c_i, [ctypes.POINTER(ConvParams), c_p]),
    'l2i_conv1x1_pair_h8': (c_i, [ctypes.POINTER(ConvParams), ctypes.POINTER(ConvParams), c_i, c_p]),
    'l2i_conv_chain3_h8': (c_i, [ctypes.POINTER(ConvParams), ctypes.POINTER(ConvParams), ctypes.POINTER(ConvParams), c_i, c_p]),
    'l2i_fused_bias_act_f32': (c_i, [c_p, c_p, c_p, c_p, c_l, c_l, c_l, c_i, c_i, c_f, c_f, c_p]),
    'l2i_fused_bias_act_f16': (c_i, [c_p, c_p, c_p, c_p, c_l, c_l, c_l, c_i, c_i, c_f, c_f, c_p]),
    'l2i_upfirdn2d_f16': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_upfirdn2d_f32': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i,
                                c_i, c_p, c_f, c_p, c_p, c_i, c_f, c_f, c_p]),
    'l2i_upfirdn2d_masked_f32': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i,
                                       c_i, c_p, c_f, c_p, c_p, c_i, c_f, c_f, c_p, c_f, c_f, c_p]),
    'l2i_upfirdn2d_dual_f32': (c_i, [c_p, c_p, c_p, c_f, c_f, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i,
                                     c_i, c_p, c_f, c_p, c_p, c_i, c_f, c_f, c_p, c_f, c_f, c_p]),
    'l2i_torgb_fwd_f32': (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_sg2_act_bwd_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_dot_reduce_f32': (c_i, [c_p, c_p, c_p, c_l, c_l, c_p]),
    'l2i_maxpool2d_fwd_f32': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_maxpool2d_bwd_f32': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_maxpool2x2_bwd_add_diff_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_l, c_i, c_i, c_p]),
    'l2i_sqdiff_f32': (c_i, [c_p, c_p, c_p, c_p, c_l, c_f, c_p, c_p]),
    'l2i_axpby_f32': (c_i, [c_p, c_p, c_p, c_f, c_f, c_l, c_p]),
    'l2i_relu_mask_f32': (c_i, [c_p, c_p, c_p, c_l, c_p]),
    'l2i_conv2d_wgrad_f32': (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_bn_stats_f32': (c_i, [c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_bn_apply_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_l, c_p]),
    'l2i_bn_bwd_reduce_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_bn_bwd_apply_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_bn_finalize_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_l, c_i, c_d, c_d, c_p]),
    'l2i_bn_bwd_finalize_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_l, c_i, c_p]),
    'l2i_repack_taps_f32': (c_i, [c_p, c_p, c_i, c_i, c_i, ctypes.POINTER(RepackTaps), c_i, c_i, c_i, c_p]),
    'l2i_repack_wino_f32': (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_batch_from_u8_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_l, c_l, c_i, c_p]),
    'l2i_pixelnorm_act_f32': (c_i, [c_p, c_p, c_i, c_i, c_l, c_f, c_f, c_p]),
    'l2i_pixelnorm_act_bwd_f32': (c_i, [c_p, c_p, c_p, c_i, c_i, c_l, c_f, c_f, c_p]),
    'l2i_upsample2x_nearest_f32': (c_i, [c_p, c_p, c_l, c_i, c_i, c_f, c_p]),
    'l2i_pool2x2_f32': (c_i, [c_p, c_p, c_l, c_i, c_i, c_f, c_p]),
    'l2i_cast_f32_to_h8': (c_i, [c_p, c_p, c_i, c_i, c_i, c_l, c_p]),
    'l2i_cast_h8_to_f32': (c_i, [c_p, c_p, c_i, c_i, c_i, c_l, c_p]),
    'l2i_upfirdn2d_h8': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_f, c_p, c_i, c_f, c_f, c_p, c_f, c_f, c_p, c_p, c_p, c_i, c_p]),
    'l2i_torgb_fwd_h8': (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_sg2_act_bwd_h8': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_dot_reduce_h8': (c_i, [c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_maxpool2d_fwd_h8': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_maxpool2d_bwd_h8': (c_i, [c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_sqdiff_h8': (c_i, [c_p, c_p, c_p, c_p, c_l, c_f, c_p, c_p]),
    'l2i_add_zero_insert_h8': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_p]),
    'l2i_mask_mul_h8': (c_i, [c_p, c_p, c_p, c_f, c_f, c_l, c_p]),
    'l2i_mask_mul_bits_h8': (c_i, [c_p, c_p, c_p, c_f, c_f, c_l, c_p]),
    'l2i_modulate_planes_h8': (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_modulate_planes_multi_h8': (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    'l2i_segmented_matvec_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p]),
    'l2i_reg_bce_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    'l2i_reg_bce_keep_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_p]),
    'l2i_face_resize_f32': (c_i, [c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_p]),
    'l2i_face_head_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_face_resize_lin_f32': (c_i, [c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_p]),
    'l2i_face_resize_lin_bwd_f32': (c_i, [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_p]),
    'l2i_face_head_bwd_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    'l2i_nonfinite_flag_f32': (c_i, [c_p, c_l, c_p, c_p]),
    'l2i_adam_guarded_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_l, c_f, c_f, c_f, c_f, c_i, c_p, c_p, c_f, c_f, c_i, c_f, c_i, c_p]),
    'l2i_sgd_guarded_f32': (c_i, [c_p, c_p, c_p, c_p, c_l, c_f, c_f, c_i, c_p, c_p, c_f, c_f, c_i, c_f, c_i, c_p]),
    'l2i_nonfinite_flag_multi_f32': (c_i, [ctypes.POINTER(AdamTensor), c_i, c_p, c_p]),
    'l2i_adam_guarded_multi_f32': (c_i, [ctypes.POINTER(AdamTensor), c_i, c_f, c_f, c_f, c_f, c_p, c_p, c_f, c_f, c_i, c_f, c_i, c_p]),
    'l2i_gram_loss_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    'l2i_gram_bwd_f32': (c_i, [c_p, c_p, c_p, c_p, c_f, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_gram_loss_h8': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    'l2i_gram_bwd_h8': (c_i, [c_p, c_p, c_p, c_p, c_f, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_pixelnorm_act_h8': (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_f, c_i, c_p]),
    'l2i_pixelnorm_act_bwd_h8': (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_f, c_i, c_p]),
    'l2i_linear_rows_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    'l2i_linear_rows_bwd_f32': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_p]),
    'l2i_range_stats': (c_i, [c_p, c_p, c_l, c_i, c_p]),
    'l2i_conv2d_wgrad_h8': (c_i, [c_p, c_p, c_p, c_p, c_l, c_f, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_conv2d_wgrad_ws_h8': (c_i, [ctypes.POINTER(c_l), c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i]),
    'l2i_bn_ws_h8': (c_i, [ctypes.POINTER(c_l), c_i, c_i, c_l]),
    'l2i_bn_stats_h8': (c_i, [c_p, c_p, c_p, c_p, c_l, c_i, c_i, c_l, c_p]),
    'l2i_bn_apply_h8': (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_l, c_p]),
    'l2i_bn_bwd_reduce_h8': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_l, c_i, c_i, c_l, c_p]),
    'l2i_bn_bwd_apply_h8': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_l, c_p]),
    'l2i_conv2d_wgrad_img_h8': (c_i, [c_p, c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_conv2d_wgrad_img_ws_h8': (c_i, [ctypes.POINTER(c_l), c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i]),
    'l2i_repack_planes_h8': (c_i, [c_p, c_i, c_i, c_p]),
    'l2i_panels_u8': (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    'l2i_last_error': (ctypes.c_char_p, []),
    'l2i_abi_version': (c_i, []),
    'l2i_sizeof_conv_params': (c_i, []),
}

# [r5] every h8 entry point exists twice: bf16 elements (the name as is) and IEEE fp16 elements (suffix _f16), same signatures
_F16_TWINS = frozenset(k for k in _SIGNATURES if k.endswith('_h8') or k in ('l2i_cast_f32_to_h8', 'l2i_cast_h8_to_f32'))
for _n in [k for k in _SIGNATURES if k in _F16_TWINS]:
    _SIGNATURES[_n + '_f16'] = _SIGNATURES[_n]

ABI_VERSION = 12         # L2I_ABI_VERSION of include/l2i.h this binding mirrors
# csrc/l2i_train_h8.hip: the weight gradient and the training-mode BatchNorm on h8 maps, and their two host-only workspace queries
TRAIN_H8 = ('l2i_conv2d_wgrad_h8', 'l2i_conv2d_wgrad_ws_h8', 'l2i_bn_ws_h8', 'l2i_bn_stats_h8', 'l2i_bn_apply_h8', 'l2i_bn_bwd_reduce_h8', 'l2i_bn_bwd_apply_h8')
# the same file's later additions: the stem's weight gradient from the fp32 image (fixed summation order) with its host-only workspace query, and the
# in-place repack of every 16-bit weight plane of a net in one launch.  Without them (a library built before them) the 16-bit trainer keeps the
# fp32 atomics kernel for conv1 and the torch repack.
TRAIN_H8_STEM = ('l2i_conv2d_wgrad_img_h8', 'l2i_conv2d_wgrad_img_ws_h8', 'l2i_repack_planes_h8')
# Entry points added without an ABI bump: a library of the same ABI version built before them (L2I_LIB = a parent build, for A/B runs) still loads;
# has(name) tells, and the callers then stay on what that library knows (conv.run_fused_transposed: the direct transposed kernel).
ADDITIVE = frozenset(('l2i_conv_transpose2d_family', 'l2i_convt_poly_plan_for', 'l2i_conv_h8_plan_for', 'l2i_bn_finalize_f32', 'l2i_bn_bwd_finalize_f32',
                      'l2i_repack_taps_f32', 'l2i_repack_wino_f32', 'l2i_batch_from_u8_f32', 'l2i_upfirdn2d_dual_f32', 'l2i_panels_u8',
                      'l2i_face_resize_lin_f32', 'l2i_face_resize_lin_bwd_f32', 'l2i_face_head_bwd_f32', 'l2i_reg_bce_keep_f32')
                     + tuple(n + t for n in TRAIN_H8 + TRAIN_H8_STEM for t in ('', '_f16')))

EXPORTS = tuple(_SIGNATURES)

_lib = None


BUILD_HASHES = os.path.join(_HERE, 'csrc', 'BUILD_HASHES.json')      # tools/update_build_hash.py: library sha256 of the committed sources


def committed_build():
    """What tools/update_build_hash.py recorded for the committed kernel sources, and whether the library that would be loaded IS that build:
    dict(kernel_sources_sha256_16, library_sha256, hipcc, sources_match, library_match).  The build is reproducible (csrc/Makefile), so
    library_match = False with sources_match = True means a different compiler or a hand-built library."""
    import hashlib
    import json
    try:
        with open(BUILD_HASHES) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        return None
    rec['sources_match'] = rec.get('kernel_sources_sha256_16') == source_hash()
    try:
        with open(LIB_PATH, 'rb') as f:
            rec['library_match'] = hashlib.sha256(f.read()).hexdigest() == rec.get('library_sha256')
    except OSError:
        rec['library_match'] = False
    return rec


def source_hash():
    """sha256[:16] over the kernel SOURCES (csrc/*.hip, *.h, Makefile, include/l2i.h; names + contents, sorted).  The PMC traffic summaries
    under profiles/ are keyed to this and not to the .so file: a rebuild of the same sources in another directory hashes the binary
    differently, and the figure must survive the driver's own build()."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, 'csrc')
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.hip', '.h')) or f == 'Makefile')      # (not BUILD_HASHES.json)
    files.append(os.path.join(os.path.dirname(_HERE), 'include', 'l2i.h'))
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


class L2IError(RuntimeError):
    pass


def load():
    """Load the shared library once; raises (loudly) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise L2IError('%s is missing: run `python __graft_entry__.py build` (hipcc --offload-arch=gfx950); '
                           'there is no CPU fallback for the hot path' % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            if name in ADDITIVE and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)           # AttributeError if the export is absent
            fn.restype = res
            fn.argtypes = args
        # L2I_LIB may point at a foreign build: a library with another struct layout must not be called through this mirror
        if lib.l2i_abi_version() != ABI_VERSION or lib.l2i_sizeof_conv_params() != ctypes.sizeof(ConvParams):
            raise L2IError('%s has ABI version %d / sizeof(l2i_conv_params) %d, this binding mirrors version %d / %d bytes: rebuild it '
                           '(`python __graft_entry__.py build`)' % (LIB_PATH, lib.l2i_abi_version(), lib.l2i_sizeof_conv_params(), ABI_VERSION,
                                                                    ctypes.sizeof(ConvParams)))
        _lib = lib
    return _lib


def has(name):
    """Whether the loaded library exports ``name`` (one of ADDITIVE; everything else is always there)."""
    return hasattr(load(), name)


def check(rc, what):
    if rc != 0:
        raise L2IError('%s failed (%d): %s' % (what, rc, load().l2i_last_error().decode()))


def call(name, *args, dtype=None, stream=None):
    """Enqueue entry point ``name`` with ``args`` on the current stream, or on ``stream``: for h8 maps of ``dtype`` float16 its IEEE fp16 twin.
    Returns the name of the entry it called; raises L2IError naming it when it fails."""
    if dtype is torch.float16 and name in _F16_TWINS:
        name += '_f16'
    rc = getattr(_lib or load(), name)(*args, stream_ptr() if stream is None else stream)
    if rc:
        check(rc, name)
    return name


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a contiguous float32/uint8 CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise L2IError('l2i kernels take GPU tensors only (got a %s tensor): no CPU fallback' % t.device)
    if not t.is_contiguous():
        raise L2IError('l2i kernels take contiguous tensors')
    return ctypes.c_void_p(t.data_ptr())


def fptr(t):
    if t is not None and t.dtype != torch.float32:
        raise L2IError('expected float32, got %s' % t.dtype)
    return ptr(t)
