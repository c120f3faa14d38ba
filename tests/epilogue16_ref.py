"""The fused epilogue contract of the 16-bit (h8) conv entry points of include/l2i.h — l2i_conv2d_h8, l2i_conv_transpose2d_h8, l2i_conv_img_h8
and their _f16 twins (csrc/l2i_conv_h8.hip, csrc/l2i_img_h8.hip) — written once in float64, with derived bounds, and the route and case tables
that drive tests/test_epilogue16_contract_gpu.py (checked on the CPU by tests/test_epilogue16_ref_cpu.py).

Model.  The operands are what the kernel reads: x, the weight planes, residual, res_sub, the masks, the old y and sq_ref rounded to the element
type (bf16 or IEEE fp16, round to nearest even); fp32 NCHW for the output-shaped operands of an out_f32 launch; l2i_conv_img_h8 takes an fp32
image and fp32 weights and rounds both itself.  Then, in float64:

    a = corr(x', w')                      (or the stride-2 transposed form, rows / columns no input reaches = 0; x' = max(x, 0) under ReLU-on-load)
    v = a * out_scale[b,co] * (out_mask ? (out_mask > 0 ? mask_pos : mask_neg) : 1) + bias[co] + noise[b,oy,ox] * noise_w
        + R * (res_mask ? (res_mask > 0 ? 1 : 0) : 1)
    R = res_sub ? res_coef * res_coef_dev[0] * (residual - res_sub) : residual
    y = act(v) * out_gain  (+ old y if accumulate)          act_gain under L2I_ACT_LRELU only

followed by ONE rounding to the element type (none for out_f32, whose output mask is binary: the entry refuses other slopes).
Side outputs: mask_out bit e = (the STORED element > 0); sq_out summed = sum (stored y - sq_ref)^2; rgb_out = rgb_bias + sum_c rgb_w * (the value
before the 16-bit store).

Bounds (nothing here is measured on a kernel).  Per element
    bound = half_ulp(want, elem) + 2^-23 (K + k) M      (+ 2^-24 absolute for fp16, as stream_ref.bound16; no half-ulp term for out_f32)
K = Cin KH KW: the fp32 accumulation of exact 16-bit products in any order — 2^-23 per step (stream_ref.U23), twice the unit roundoff, because the
matrix pipe's internal adds are not promised to round to nearest.  k = the rounded fp32 operations of the case's epilogue terms (K_OPS below).
M = the same formula on magnitudes: |x'| * |w'| (correlated), |out_scale|, max(|mask_pos|, |mask_neg|), |bias|, |noise noise_w|, |R| with
|res_coef res_coef_dev| (|residual| + |res_sub|), the activation's max(1, |slope|) |act_gain|, |out_gain|, + |old y|.  Every rounding of the chain is
relative to a partial result no larger than M, so the sum of K + k roundings is below 2^-23 (K + k) M to first order, with a factor two to spare.
rgb_out: the same form with K + k + Cout operations and M_rgb = sum_c |rgb_w| M + |rgb_bias|.
sq: against the float64 sum over the RETURNED output, stream_ref.bound_red with the terms one lane adds in sequence: 8 elements x the slots a lane
finishes (2 WM WN per block of conv_h8_kernel, 16 per tile of conv_img_h8_kernel) + the blocks that share one of the L2I_SQ_SLOTS atomic slots.
mask_out (= sign plane of the returned output) and everything outside the launch window: bit-exact.

A plain module: no fixtures, no kernel code; the model runs on whatever device its operands live on."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import epilogue_ref as er
from tests.stream_ref import U23, ELEM_DTYPES, bound_red, f32, from_h8, half_ulp, rnd_for, sign_plane, to_h8, worst      # noqa: F401 (shared, re-exported)

ACT_NONE, ACT_LRELU, ACT_RELU = er.ACT_NONE, er.ACT_LRELU, er.ACT_RELU
SQRT2 = er.SQRT2
SENTINEL = -7680.0            # -15 * 2^9: exactly representable in fp32, bf16 and fp16; far from every result
SENTINEL_U8 = 0xA5            # what a sign plane holds before the launch
ELEMS = ('bf16', 'f16')
EPI_LEAN, EPI_GENERAL, EPI_F32_VEC, EPI_F32_SCALAR = 0, 1, 2, 3          # include/l2i.h: L2I_H8_EPI_*

MISTAKES = ('mask_ge', 'out_mask_after_add', 'one_mask_for_both', 'res_mask_gates_conv', 'coef_dropped', 'coef_squared', 'coef_null_is_zero',
            'accumulate_times_out_gain', 'accumulate_times_act_gain', 'accumulate_before_act', 'act_before_residual',
            # the h8 ones
            'leaky_mask_neg_dropped',        # mask_neg read as 0
            'res_mask_leaky',                # res_mask given the slopes
            'gain_under_every_act',          # act_gain applied under NONE / RELU, as the h8 FIR entry does
            'lean_max_with_bad_gains',       # max(v gpos, v gneg) evaluated where gneg > gpos or a gain is negative
            'sign_from_unrounded',           # mask_out taken from the fp32 value
            'sq_on_unrounded', 'rgb_from_rounded',
            'accumulate_rounded_twice')      # the sum rounded to 16 bits before the old y is added

# k: rounded fp32 operations per epilogue term
K_OPS = {'out_scale': 1, 'out_mask': 1, 'noise': 2, 'bias': 1, 'residual': 1, 'res_sub': 3, 'lrelu': 4, 'out_gain': 1, 'accumulate': 1}


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def _d(t, rnd=None):
    if t is None:
        return None
    t = torch.as_tensor(t).detach().float()
    return (t if rnd is None else rnd(t)).double()


def corr16(x, w, stride, pad, transposed, out_hw, elem, relu_in=False):
    """(a, Ma): the float64 correlation of the rounded operands on the out_hw = (OH, OW) pixels the launch writes, and the same on magnitudes.
    x [B, Cin, H, W]; w [Cout, Cin, K, K] in correlation form, or [B, Cout, Cin, K, K] (one plane set per sample: w_bstride)."""
    rnd = rnd_for(elem)
    xx = _d(x, rnd)
    if relu_in:
        xx = torch.relu(xx)
    ww = _d(w, rnd)

    def one(xs, ws):
        if transposed:
            a = F.conv_transpose2d(xs, ws.transpose(0, 1), stride=2)[:, :, pad:, pad:]
            a = F.pad(a, (0, max(0, out_hw[1] - a.shape[3]), 0, max(0, out_hw[0] - a.shape[2])))
        else:
            a = F.conv2d(xs, ws, stride=stride, padding=pad)
        assert a.shape[2] >= out_hw[0] and a.shape[3] >= out_hw[1], (a.shape, out_hw)
        return a[:, :, :out_hw[0], :out_hw[1]]
    if ww.dim() == 5:
        a = torch.cat([one(xx[b:b + 1], ww[b]) for b in range(xx.shape[0])])
        Ma = torch.cat([one(xx[b:b + 1].abs(), ww[b].abs()) for b in range(xx.shape[0])])
    else:
        a, Ma = one(xx, ww), one(xx.abs(), ww.abs())
    return a.contiguous(), Ma.contiguous()


def epi16(a, Ma, K, elem, *, out_f32=False, y_prev=None, out_scale=None, noise=None, noise_w=0.0, bias=None, residual=None, res_mask=None, out_mask=None,
          mask=(1.0, 0.0), act=ACT_NONE, slope=0.2, gain=1.0, out_gain=1.0, accumulate=False, res_sub=None, res_coef=1.0, res_coef_dev=None,
          rgb=None, _mistake=None):
    """The epilogue on the window: ``a`` / ``Ma`` from corr16; every output-shaped operand (noise [B,1,..], residual, masks, res_sub, y_prev) already cut
    to the window, float32, NOT yet rounded.  Returns dict(want, bound, M, k[, rgb = (want, bound)]): ``want`` float64 before the one rounding of the
    store, ``bound`` per element for the stored value."""
    assert _mistake is None or _mistake in MISTAKES, _mistake
    rnd = None if out_f32 else rnd_for(elem)
    dev = a.device
    T = lambda t, r=None: None if t is None else _d(t, r).to(dev)
    pos = (lambda m: m >= 0) if _mistake == 'mask_ge' else (lambda m: m > 0)
    one = torch.ones((), dtype=torch.float64, device=dev)
    mp, mn = f32(mask[0]), (0.0 if _mistake == 'leaky_mask_neg_dropped' else f32(mask[1]))
    leak = lambda m: torch.where(pos(T(m, rnd)), mp * one, mn * one)
    v, M, k = a, Ma, 0
    if out_scale is not None:
        s = T(out_scale)[:, :, None, None]
        v, M, k = v * s, M * s.abs(), k + K_OPS['out_scale']
    if res_mask is not None and _mistake == 'res_mask_gates_conv':
        v = v * pos(T(res_mask, rnd))
    if out_mask is not None:
        M, k = M * max(abs(f32(mask[0])), abs(f32(mask[1]))), k + K_OPS['out_mask']
        if _mistake != 'out_mask_after_add':
            v = v * leak(out_mask)
    if bias is not None:
        bb = T(bias)[None, :, None, None]
        v, M, k = v + bb, M + bb.abs(), k + K_OPS['bias']
    if noise is not None:
        nz = T(noise) * f32(noise_w)
        v, M, k = v + nz, M + nz.abs(), k + K_OPS['noise']
    if out_mask is not None and _mistake == 'out_mask_after_add':
        v = v * leak(out_mask)
    r = None
    if residual is not None:
        r = T(residual, rnd)
        Mr, k = r.abs(), k + K_OPS['residual']
        if res_sub is not None:
            devc = (0.0 if _mistake == 'coef_null_is_zero' else 1.0) if res_coef_dev is None else float(_d(res_coef_dev).reshape(-1)[0])
            coef = 1.0 if _mistake == 'coef_dropped' else f32(res_coef) * devc
            coef = coef * coef if _mistake == 'coef_squared' else coef
            sub = T(res_sub, rnd)
            r, Mr, k = coef * (r - sub), abs(f32(res_coef) * (1.0 if res_coef_dev is None else float(_d(res_coef_dev).reshape(-1)[0]))) * (Mr + sub.abs()), k + K_OPS['res_sub']
        rm = out_mask if (_mistake == 'one_mask_for_both' and out_mask is not None) else res_mask
        if rm is not None:
            r = r * (leak(rm) if _mistake == 'res_mask_leaky' else pos(T(rm, rnd)))
        M = M + Mr
    else:
        assert res_sub is None and res_mask is None
    prev = T(y_prev, rnd) if accumulate else None
    if r is not None and _mistake != 'act_before_residual':
        v = v + r
    if accumulate and _mistake == 'accumulate_before_act':
        v = v + prev
    sl, gn, og = f32(slope), f32(gain), f32(out_gain)
    if _mistake == 'lean_max_with_bad_gains':
        gpos = (gn if act == ACT_LRELU else 1.0) * og
        gneg = sl * gn * og if act == ACT_LRELU else (0.0 if act == ACT_RELU else og)
        v = torch.maximum(v * gpos, v * gneg) / og          # (out_gain is applied below)
    elif act == ACT_LRELU:
        v = torch.where(v > 0, v, v * sl) * gn
    elif act == ACT_RELU:
        v = torch.relu(v)
    if act == ACT_LRELU:
        M, k = M * max(1.0, abs(sl)) * abs(gn), k + K_OPS['lrelu']
    elif _mistake == 'gain_under_every_act':
        v = v * gn
    if r is not None and _mistake == 'act_before_residual':
        v = v + r
    if accumulate and _mistake == 'accumulate_times_out_gain':
        v = v + prev
    if og != 1.0:
        v, M, k = v * og, M * abs(og), k + K_OPS['out_gain']
    pre, Mpre, kpre = v, M, k                               # the value before the store (and before the old y, which rgb launches never have)
    if accumulate:
        k = k + K_OPS['accumulate']
        M = M + prev.abs()
        if _mistake == 'accumulate_times_act_gain':
            v = v + prev * gn
        elif _mistake == 'accumulate_rounded_twice':
            v = rnd(v.float()).double() + prev if rnd is not None else v + prev
        elif _mistake not in ('accumulate_before_act', 'accumulate_times_out_gain'):
            v = v + prev
    bound = U23 * (K + k) * M
    if not out_f32:
        bound = bound + half_ulp(v, elem).to(dev) + (2.0 ** -24 if elem == 'f16' else 0.0)
    out = dict(want=v, bound=bound, M=M, k=k)
    if rgb is not None:                                     # (rgb_w [B, 3, Cout], rgb_bias [3])
        w3, b3 = T(rgb[0]), T(rgb[1])
        src = rnd(pre.float()).double() if _mistake == 'rgb_from_rounded' else pre
        want = torch.einsum('bchw,boc->bohw', src, w3) + b3[None, :, None, None]
        Mrgb = torch.einsum('bchw,boc->bohw', Mpre, w3.abs()) + b3.abs()[None, :, None, None]
        out['rgb'] = (want, U23 * (K + kpre + a.shape[1]) * Mrgb)
    return out


def stored(want, elem, out_f32=False):
    """What the launch stores of ``want`` (the one rounding), as float64."""
    return want.float().double() if out_f32 else rnd_for(elem)(want.float()).double()


def mask_out_ref(y_stored_nchw, want=None, _mistake=None):
    """Sign plane [B, C/8, H, W] (uint8) of the STORED output (NCHW, C % 8 == 0); the mistake takes it from the unrounded value."""
    src = want if _mistake == 'sign_from_unrounded' else y_stored_nchw
    B, C, H, W = src.shape
    g = src.reshape(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2)
    return sign_plane(g.cpu())


def sq_ref_sum(y_stored, sq_ref, elem, want=None, _mistake=None):
    """(float64 sum (stored y - sq_ref')^2, its magnitude sum) with sq_ref rounded to the element type."""
    src = want if _mistake == 'sq_on_unrounded' else y_stored
    d = src.double() - _d(sq_ref, rnd_for(elem)).to(src.device)
    s = float((d * d).sum())
    return s, s


def sq_n_lane(plan=None, img_k=None, grid=0):
    """Terms one lane adds in sequence: 8 elements x its slots, + the blocks that share an atomic slot."""
    per_lane = 8 * 2 * plan['WM'] * plan['WN'] if img_k is None else 8 * 16 * (1 if img_k == 3 else 4)
    return per_lane + (grid + 1023) // 1024


# ---- routes -------------------------------------------------------------------------------------------------------------------------------------
# kind: 'conv' = H8Conv.forward of a correlation, 'tfwd' = forward of a stride-2 transposed H8Conv, 'dgrad' = H8Conv.dgrad of a stride-2 conv (the
# transposed launch), 'struct' = conv._conv_params by hand (the window offsets no product call uses), 'img' = ImgConvH8.forward.
# shape = (cin, cout, k, stride, pad, h, w, batch) of the launch's INPUT; extra = (rows, columns) y has beyond the conv's own size; off = (oy_off,
# ox_off); inst = (WM, WN, K, S, TR, KS) of conv_h8_kernel the dispatch must choose (l2i_conv_h8_plan_for).
Route = namedtuple('Route', 'name kind shape inst out_f32 cin_pad extra off', defaults=(False, 32, (0, 0), (0, 0)))
ROUTES = [
    Route('c3s1_ks1', 'conv', (32, 40, 3, 1, 1, 19, 45, 2), (1, 2, 3, 1, 0, 1)),                      # ragged Cout (CoutP 64, second block half empty), odd map
    Route('c3s1_cin16', 'conv', (16, 32, 3, 1, 1, 9, 70, 1), (1, 2, 3, 1, 0, 1), cin_pad=16),          # Cin % 32 != 0, one chunk; rgb on 32 channels
    Route('c3s1_rgb64', 'conv', (16, 64, 3, 1, 1, 12, 40, 1), (1, 2, 3, 1, 0, 1), cin_pad=16),         # rgb on 64 channels (then WM = 2: every channel in one block)
    Route('c3s1_ks2', 'conv', (512, 32, 3, 1, 1, 8, 8, 2), (1, 2, 3, 1, 0, 2)),                        # the 32-channel-chunk form (Cin > 256, OW <= 32)
    Route('c3s1_wide', 'conv', (16, 128, 3, 1, 1, 128, 128, 2), (2, 2, 3, 1, 0, 1), cin_pad=16),       # 256 blocks of 64 channels: WM = 2
    Route('c3s1_pad0', 'conv', (32, 32, 3, 1, 0, 18, 67, 1), (1, 2, 3, 1, 0, 1)),
    Route('c3s1_big_y', 'conv', (32, 40, 3, 1, 1, 19, 45, 2), (1, 2, 3, 1, 0, 1), extra=(3, 5)),       # OH < OHf: the rest untouched
    Route('c3s1_offset', 'struct', (32, 40, 3, 1, 1, 19, 45, 2), (1, 2, 3, 1, 0, 1), extra=(3, 5), off=(2, 3)),
    Route('c1s1', 'conv', (128, 96, 1, 1, 0, 33, 40, 2), (1, 2, 1, 1, 0, 2)),                          # 1x1, three narrow blocks
    Route('c1s1_wide', 'conv', (32, 128, 1, 1, 0, 128, 128, 2), (2, 2, 1, 1, 0, 2)),
    Route('c3s2_p1', 'conv', (64, 128, 3, 2, 1, 33, 31, 2), (1, 1, 3, 2, 0, 1)),                       # split-column stride-2 tile, WN = 1
    Route('c3s2_p0', 'conv', (32, 64, 3, 2, 0, 68, 68, 1), (1, 1, 3, 2, 0, 1)),
    Route('c3s2_wide', 'conv', (32, 128, 3, 2, 1, 128, 128, 4), (2, 1, 3, 2, 0, 1)),                   # 256 blocks at 4-row tiles
    Route('c1s2', 'conv', (64, 64, 1, 2, 0, 40, 36, 2), (1, 2, 1, 2, 0, 2)),                           # the gather form
    Route('f32_c3s1_vec', 'conv', (64, 3, 3, 1, 1, 24, 40, 2), (1, 2, 3, 1, 0, 2), out_f32=True),
    Route('f32_c3s1_scalar', 'conv', (64, 3, 3, 1, 1, 24, 45, 2), (1, 2, 3, 1, 0, 2), out_f32=True),
    Route('f32_c3s1_wide', 'conv', (32, 40, 3, 1, 1, 24, 40, 1), (2, 2, 3, 1, 0, 2), out_f32=True),
    Route('f32_c1s1', 'conv', (32, 3, 1, 1, 0, 17, 36, 2), (1, 2, 1, 1, 0, 2), out_f32=True),          # the ToRGB launches' form
    Route('t_p0_narrow', 'tfwd', (64, 32, 3, 2, 0, 17, 40, 1), (1, 2, 3, 1, 1, 2)),                    # transposed, four accumulators per pixel
    Route('t_p0_wide', 'tfwd', (32, 64, 3, 2, 0, 32, 32, 2), (2, 1, 3, 1, 1, 2)),
    Route('t_p1_ragged', 'dgrad', (64, 72, 3, 2, 1, 20, 33, 1), (1, 2, 3, 1, 2, 2)),                   # pad 1; CoutP 96
    Route('t_p1_wide', 'dgrad', (64, 64, 3, 2, 1, 20, 33, 1), (2, 1, 3, 1, 2, 2)),
    Route('t_p0_plus', 'tfwd', (64, 32, 3, 2, 0, 17, 40, 1), (1, 2, 3, 1, 1, 2), extra=(3, 8)),        # the zero-conv rows still take the epilogue
    Route('img_1x1', 'img', (3, 40, 1, 1, 0, 33, 37, 1), None),
    Route('img_3x3', 'img', (4, 96, 3, 1, 0, 18, 67, 1), None),
    Route('img_7x7s2', 'img', (3, 64, 7, 2, 3, 31, 45, 1), None),
]
BY_NAME = {r.name: r for r in ROUTES}


def transposed(route):
    return route.kind in ('tfwd', 'dgrad')


def geometry(route):
    """dict(x_shape, y_shape (NCHW, full), win = (oy0, ox0, OH, OW), K, CoutP) of a route."""
    cin, cout, k, stride, pad, h, w, b = route.shape
    if transposed(route):
        oh, ow = (h - 1) * 2 - 2 * pad + 3 + route.extra[0], (w - 1) * 2 - 2 * pad + 3 + route.extra[1]
        ohf, owf, win = oh, ow, (0, 0, oh, ow)
    else:
        oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        ohf, owf = oh + route.extra[0], ow + route.extra[1]
        win = (route.off[0], route.off[1], oh, ow)
    return dict(x_shape=(b, cin, h, w), y_shape=(b, cout, ohf, owf), win=win, K=cin * k * k, CoutP=(cout + 31) // 32 * 32)


def cut(t, win):
    oy, ox, oh, ow = win
    return None if t is None else t[:, :, oy:oy + oh, ox:ox + ow]


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------
# A case = the fields it sets (+ modifiers) and EVERY seeded mistake that changes its result (tests/test_epilogue16_ref_cpu.py proves both
# directions).  Fields: out_scale, out_mask (binary slopes (1, 0) unless `leaky`: (sqrt 2, 0.2 sqrt 2)), noise (noise_w 0.3), bias, residual, res_mask,
# res_sub (res_coef 0.25, res_coef_dev [2.0]), lrelu (slope 0.2, gain sqrt 2), relu, out_gain (0.5), accumulate, sq, rgb, mask_out, relu_in, w_bstride.
# Modifiers: leaky, mask_bits (the masks go in as sign planes), same_mask (res_mask IS out_mask), coef_null, big_prev, neg_residual, gain_only
# (act_gain sqrt 2 without LRELU), neg_out_gain (-0.5), slope_gt_1 (1.5), neg_act_gain (-sqrt 2), tiny (out_gain 2^-26), big_bias (bias x 64: the
# rounding of the store then outweighs the fp32 budget of the ToRGB sum, so that rgb_from_rounded shows for fp16 as well).
FIELDS = ('out_scale', 'out_mask', 'noise', 'bias', 'residual', 'res_mask', 'res_sub', 'lrelu', 'relu', 'out_gain', 'accumulate', 'sq', 'rgb', 'mask_out',
          'relu_in', 'w_bstride')
MODIFIERS = ('leaky', 'mask_bits', 'same_mask', 'coef_null', 'big_prev', 'neg_residual', 'gain_only', 'neg_out_gain', 'slope_gt_1', 'neg_act_gain', 'tiny',
             'big_bias')
BAD_GAINS = ('neg_out_gain', 'slope_gt_1', 'neg_act_gain')
_TWO = ('one_mask_for_both', 'res_mask_gates_conv', 'mask_ge')
_LEAKY2 = _TWO + ('res_mask_leaky', 'leaky_mask_neg_dropped')
CASES = {
    # each term alone on a bare conv (the single fields of epilogue_ref.CASES minus the prologue, which the h8 entries refuse)
    'bare': ((), ()),
    'out_scale': (('out_scale',), ()),
    'out_mask': (('out_mask',), ('mask_ge',)),
    'noise': (('noise',), ()),
    'bias': (('bias',), ()),
    'residual': (('residual',), ()),
    'lrelu': (('lrelu',), ()),
    'relu': (('relu',), ()),
    'out_gain': (('out_gain',), ()),
    'accumulate': (('accumulate',), ('accumulate_rounded_twice',)),
    # the order-discriminating combinations of epilogue_ref.COMBO_CASES
    'mask_noise_bias': (('out_mask', 'noise', 'bias'), ('out_mask_after_add', 'mask_ge')),
    'two_masks': (('out_scale', 'out_mask', 'residual', 'res_mask'), _TWO),
    'res_sub_coef': (('residual', 'res_sub', 'res_mask'), ('coef_dropped', 'coef_squared', 'res_mask_gates_conv', 'mask_ge')),
    'res_sub_coef_null': (('residual', 'res_sub', 'res_mask', 'coef_null'), ('coef_null_is_zero', 'coef_dropped', 'coef_squared', 'res_mask_gates_conv', 'mask_ge')),
    'gain_acc': (('out_gain', 'accumulate', 'big_prev'), ('accumulate_times_out_gain', 'accumulate_before_act', 'accumulate_rounded_twice')),
    'lrelu_gain_acc': (('lrelu', 'out_gain', 'accumulate', 'big_prev'), ('accumulate_times_out_gain', 'accumulate_times_act_gain', 'accumulate_before_act', 'accumulate_rounded_twice')),
    'relu_neg_residual': (('relu', 'residual', 'neg_residual'), ('act_before_residual',)),
    # the h8 contract
    'out_mask_leaky': (('out_mask', 'leaky'), ('leaky_mask_neg_dropped', 'mask_ge')),
    'mask_noise_bias_leaky': (('out_mask', 'leaky', 'noise', 'bias'), ('out_mask_after_add', 'leaky_mask_neg_dropped', 'mask_ge')),
    'two_masks_leaky': (('out_scale', 'out_mask', 'leaky', 'residual', 'res_mask'), _LEAKY2),
    'masks_as_planes': (('out_scale', 'out_mask', 'leaky', 'residual', 'res_mask', 'mask_bits'), _LEAKY2),
    'pair_planes': (('bias', 'out_mask', 'residual', 'res_mask', 'same_mask', 'mask_bits', 'mask_out'), ('out_mask_after_add', 'mask_ge')),      # l2i_conv1x1_pair_h8's backward set
    'relu_in': (('relu_in',), ()),
    'per_sample_planes': (('w_bstride',), ()),
    'gain_none': (('gain_only',), ('gain_under_every_act',)),
    'gain_relu': (('gain_only', 'relu'), ('gain_under_every_act',)),
    'neg_out_gain': (('relu', 'neg_out_gain'), ('lean_max_with_bad_gains',)),
    'slope_gt_1': (('lrelu', 'slope_gt_1'), ('lean_max_with_bad_gains',)),
    'neg_act_gain': (('lrelu', 'neg_act_gain'), ('lean_max_with_bad_gains',)),
    'mask_out_lean': (('bias', 'relu', 'mask_out'), ()),
    'mask_out_general': (('bias', 'residual', 'relu', 'mask_out'), ('act_before_residual',)),                           # l2i_conv1x1_pair_h8's forward set
    'tiny_out': (('bias', 'tiny', 'mask_out'), ('sign_from_unrounded',)),                                                # fp16 only
    'sq_lean': (('bias', 'relu', 'sq'), ('sq_on_unrounded',)),
    'sq_general': (('bias', 'residual', 'sq'), ('sq_on_unrounded',)),
    'rgb': (('bias', 'big_bias', 'lrelu', 'rgb'), ('rgb_from_rounded',)),
}
CASE_NAMES = list(CASES) + ['everything']
F16_ONLY = ('tiny_out',)

_EPI = frozenset(('out_scale', 'out_mask', 'noise', 'bias', 'residual', 'res_mask', 'res_sub', 'lrelu', 'relu', 'out_gain', 'accumulate'))


def accepts(route):
    """The fields and modifiers a route's entry implements (l2i.h).  Everything else is refused by the entry: the product's own calls cannot even
    express most of it (conv.run_h8 asserts, ImgConvH8.forward has no keyword), so those pairs are rows of REFUSALS in the GPU file, driven with the
    launch struct itself; tests/test_epilogue16_ref_cpu.py checks that every such pair has its row."""
    k, stride, cout = route.shape[2], route.shape[3], route.shape[1]
    if route.kind == 'img':
        return frozenset(('bias', 'lrelu', 'relu', 'out_gain', 'sq', 'gain_only', 'big_bias'))
    common = _EPI | {'w_bstride', 'coef_null', 'big_prev', 'neg_residual', 'gain_only', 'big_bias'} | set(BAD_GAINS)
    if route.out_f32:
        return frozenset(common)
    acc = common | {'leaky', 'mask_bits', 'same_mask', 'mask_out', 'tiny'}
    if not transposed(route):
        acc |= {'sq'}
        if k == 3 and stride == 1:
            acc |= {'relu_in'}
            if cout in (32, 64):
                acc |= {'rgb'}
    return frozenset(acc)


def everything(route):
    """Every field the route accepts at once: one activation, leaky masks as planes where the entry has them; sq and mask_out exclude each other
    (and rgb excludes the per-pixel operands), so `everything` keeps the per-pixel operands, sq and drops rgb / mask_out."""
    acc = accepts(route)
    f = [k for k in FIELDS if k in acc and k not in ('rgb', 'mask_out', 'relu', 'relu_in')]
    if route.kind == 'img':
        return tuple(f)
    return tuple(f + [m for m in ('leaky', 'mask_bits') if m in acc])


def case_fields(name, route=None):
    return everything(route) if name == 'everything' else CASES[name][0]


def runs_on(fields, route):
    acc = accepts(route)
    return all(k in acc for k in fields)


def pairs(elem=None):
    """(route, case) pairs of the matrix: every case a route accepts."""
    for r in ROUTES:
        for c in CASE_NAMES:
            if c in F16_ONLY and elem == 'bf16':
                continue
            if runs_on(case_fields(c, r), r):
                yield r, c


def expected_epilogue(route, fields, y_shape):
    """L2I_H8_EPI_* the launch must report (restated from launch_h8)."""
    if route.out_f32:
        ow, owf = geometry(route)['win'][3], y_shape[3]
        return EPI_F32_VEC if (owf % 4 == 0 and ow % 4 == 0 and route.off[1] % 4 == 0) else EPI_F32_SCALAR
    lean = not (set(fields) & {'out_mask', 'residual', 'accumulate'}) and not (set(fields) & set(BAD_GAINS))
    k, stride = route.shape[2], route.shape[3]
    if 'sq' in fields and not (k == 3 and stride == 1 and not transposed(route)):
        lean = False
    return EPI_LEAN if lean else EPI_GENERAL


def expected_plan(route, fields):
    """The l2i_conv_h8_plan fields a (route, fields) launch must report."""
    g = geometry(route)
    wm, wn, k, s, tr, ks = route.inst
    if 'rgb' in fields and g['CoutP'] % 64 == 0:
        wm = 2                                             # (a ToRGB launch keeps 64-channel blocks whatever the block count)
    oh, ow = g['win'][2:]
    if tr:
        oh, ow = (oh + 1) // 2, (ow + 1) // 2
    b = route.shape[7]
    tiles_x, tiles_y, mblocks = (ow + 31) // 32, (oh + 4 * wn - 1) // (4 * wn), (g['CoutP'] + 32 * wm - 1) // (32 * wm)
    total = b * tiles_x * tiles_y * mblocks
    epi = expected_epilogue(route, fields, g['y_shape'])
    extra = int(epi == EPI_LEAN and bool(set(fields) & {'rgb', 'sq'}))
    return dict(eligible=1, WM=wm, WN=wn, K=k, S=s, TR=tr, KS=ks, out32=int(route.out_f32), relu_in=int('relu_in' in fields), extra=extra, epilogue=epi,
                tiles_x=tiles_x, tiles_y=tiles_y, mblocks=mblocks, total=total, grid=(total + 7) // 8 * 8)


# ---- data ---------------------------------------------------------------------------------------------------------------------------------------
def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def route_data(route, variant='plain'):
    """(x, w) of a route: float32 CPU tensors, the same for every case (the raw correlation is computed once per route and element type).
    variant 'per_sample': w is [B, Cout, Cin, K, K]."""
    cin, cout, k, stride, pad, h, w, b = route.shape
    rs = np.random.RandomState(1000 + ROUTES.index(route))
    x = T(rs.randn(b, cin, h, w))
    wt = T(rs.randn(cout, cin, k, k) / np.sqrt(cin * k * k))
    if variant == 'per_sample':
        wt = wt[None] * T(rs.rand(b, 1, cin, 1, 1) + 0.5)
    return x, wt


def make_inputs(route, case, elem):
    """The epilogue operands of a (route, case) as float32 CPU tensors / Python scalars keyed by epi16's keyword names, full y-shaped where they are
    maps, plus 'y_prev' (what the output holds before the launch: the sentinel, or the old y inside the window of an accumulating case)."""
    fields = case_fields(case, route)
    g = geometry(route)
    y_shape, cout = g['y_shape'], route.shape[1]
    B = y_shape[0]
    rs = np.random.RandomState(ROUTES.index(route) * 1000 + CASE_NAMES.index(case) * 2 + ELEMS.index(elem))
    like_y = lambda: T(rs.randn(*y_shape))
    kw = {}
    if 'out_scale' in fields:
        kw['out_scale'] = T(rs.rand(B, cout) + 0.5)
    if 'out_mask' in fields:
        kw['out_mask'] = er.masks_like(rs, y_shape)
        kw['mask'] = (SQRT2, 0.2 * SQRT2) if 'leaky' in fields else (1.0, 0.0)
    if 'noise' in fields:
        kw['noise'], kw['noise_w'] = T(rs.randn(B, 1, *y_shape[2:])), 0.3
    if 'bias' in fields:
        kw['bias'] = T(rs.randn(cout)) * (64.0 if 'big_bias' in fields else 1.0)
    if 'residual' in fields:
        kw['residual'] = like_y() - 2.0 if 'neg_residual' in fields else like_y()
    if 'res_mask' in fields:
        kw['res_mask'] = kw['out_mask'] if 'same_mask' in fields else er.masks_like(rs, y_shape)
    if 'res_sub' in fields:
        kw['res_sub'], kw['res_coef'] = like_y(), 0.25
        kw['res_coef_dev'] = None if 'coef_null' in fields else torch.full((1,), 2.0)
    if 'lrelu' in fields:
        kw['act'], kw['slope'], kw['gain'] = ACT_LRELU, (1.5 if 'slope_gt_1' in fields else 0.2), (-SQRT2 if 'neg_act_gain' in fields else SQRT2)
    if 'relu' in fields:
        kw['act'] = ACT_RELU
    if 'gain_only' in fields:
        kw['gain'] = SQRT2
    if 'out_gain' in fields:
        kw['out_gain'] = 0.5
    if 'neg_out_gain' in fields:
        kw['out_gain'] = -0.5
    if 'tiny' in fields:
        kw['out_gain'] = 2.0 ** -26
    y_prev = torch.full(y_shape, SENTINEL)
    if 'accumulate' in fields:
        kw['accumulate'] = True
        oy, ox, oh, ow = g['win']
        y_prev[:, :, oy:oy + oh, ox:ox + ow] = T(rs.randn(B, cout, oh, ow)) * (100.0 if 'big_prev' in fields else 1.0)
    if 'rgb' in fields:
        kw['rgb'] = (T(rs.randn(B, 3, cout)), T(rs.randn(3)))
    return fields, kw, y_prev, rs


def sq_ref_for(want, elem, rs):
    """sq_ref of an sq case: the model's own stored output + N(0, 0.01), so that the sum is made of the store's rounding and a little noise (a
    kernel that sums the unrounded value shows) — float32, full window."""
    base = stored(want.cpu(), elem)
    return (base + 0.01 * torch.from_numpy(rs.randn(*base.shape))).float()


def model(route, case, elem, a, Ma, kw, y_prev, _mistake=None):
    """epi16 of a (route, case) on its window.  a, Ma: corr16 of the route (any device)."""
    g = geometry(route)
    c = lambda t: cut(t, g['win'])
    args = {k: (c(v) if torch.is_tensor(v) and v.dim() == 4 else v) for k, v in kw.items()}
    return epi16(a, Ma, g['K'], elem, out_f32=route.out_f32, y_prev=c(y_prev), _mistake=_mistake, **args)
