"""The contract of the FIR, bias-activation and weight-plane entry points of include/l2i.h (l2i_upfirdn2d_f32, l2i_upfirdn2d_masked_f32,
l2i_upfirdn2d_h8, l2i_fused_bias_act_f32, l2i_modulate_planes_h8, l2i_modulate_planes_multi_h8), written once, and the case table that drives
tests/test_fir_contract_gpu.py (checked on the CPU by tests/test_fir_ref_cpu.py).  Conventions, helpers and bounds are those of
tests/stream_ref.py: a model returns {output: (want, M)} with M the sum of the absolute values of the terms an output adds, carried through the
activation, gain and mask factors by their absolute values (an activation by the larger of its two slopes: it is Lipschitz with that constant).
Where M = 0 (an output no tap reaches and no operand feeds: a crop past the far edge, a 1x1 FIR between inserted zeros) the bound is 0: exactly 0.

The two FIR families apply their epilogues in different orders, and include/l2i.h says so:
  f32:  v = fir + noise noise_w + bias + addend;  LRELU: v = lrelu(v) gain, RELU: v = max(v, 0), NONE: v (gain under LRELU only);  v *= mask factor
  h8:   v = act(fir + noise noise_w + bias) gain (under every act);  v *= mask factor;  v += addend

A plain module: no fixtures, no GPU, no kernel code."""
import numpy as np
import torch

from tests.stream_ref import (ELEM_DTYPES, GUARD, SENTINEL, SQRT2, U23, Row, T, bound16, bound_elem, f32, from_h8, plant_signs,      # noqa: F401
                              rnd_for, sign_plane, to_h8, worst)

ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
MISTAKES = ('taps_not_flipped', 'taps_transposed', 'pad_xy_swapped', 'up_phase_shifted', 'down_phase_shifted', 'noise_per_channel', 'bias_by_batch',
            'addend_after_act', 'addend_before_mask', 'gain_without_lrelu', 'mask_zero_is_positive', 'mask_before_act', 'relu_is_lrelu',
            'fba_ref_ignored', 'fba_bias_index_no_modulo', 'planes_half_swapped', 'planes_scale_by_cout')

# ---- test kernels: none symmetric under a flip or a transpose; dyadic, so outer products and float32 copies are exact --------------------------------
K1Y = (0.125, 0.375, 1.0, -0.25)                 # [1, 3, 8, -2] / 8: the largest entry is 1, so kernels16.separable returns these very vectors
K1X = (0.1875, -0.0625, 0.25, 0.4375)            # [3, -1, 4, 7] / 16
SYM1 = (0.125, 0.375, 0.375, 0.125)              # the FIR every earlier test used: blind to a flip and to a transpose


def _k(a):
    return torch.tensor(a, dtype=torch.float64)


KERNELS = {
    'K44': torch.outer(_k(K1Y), _k(K1X)),
    'K44N': torch.outer(_k(K1Y), _k(K1X)) + _k([[0, 0, 0, 0], [0, 0, 0.25, 0], [0, 0, 0, 0], [-0.125, 0, 0, 0]]),          # not separable
    'SYM44': torch.outer(_k(SYM1), _k(SYM1)),
    'K11': _k([[0.75]]),
    'K23': _k([[1, -2, 3], [4, 5, -6]]) / 8,
    'K35': _k([[((i * 5 + j) * 3 % 7) - 2 for j in range(5)] for i in range(3)]) / 8,
    'K88': _k([[((i * 8 + j) * 5 % 17) - 6 for j in range(8)] for i in range(8)]) / 16,
}
TAPS = {'K44': (K1Y, K1X), 'SYM44': (SYM1, SYM1)}


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def _c(t, dt, rnd=None):
    if t is None:
        return None
    t = torch.as_tensor(t).detach().cpu().float()
    if rnd is not None:
        t = rnd(t)
    return t.to(dt)


def out_size(n, up, down, p0, p1, k):
    return (n * up + p0 + p1 - k) // down + 1


def _fma(a, b, c, dt):
    """round(a b + c) once, as v_fma_f32 does (dt float32: through float64, whose product of two float32 is exact)."""
    if dt == torch.float64:
        return a * b + c
    return (a.double() * b.double() + c.double()).to(dt)


def upfirdn2d(x, k=None, up=(1, 1), down=(1, 1), pad=(0, 0, 0, 0), noise=None, noise_w=0.0, bias=None, addend=None, act=ACT_NONE, slope=0.2,
              gain=1.0, mask=None, mask_vals=(1.0, 0.0), family='f32', rnd=None, taps=None, dt=torch.float64, order='kykx', _mistake=None):
    """The reference op from its definition — zero insertion by ``up`` = (ux, uy), pad or crop by ``pad`` = (x0, x1, y0, y1), correlation with the
    flipped kernel, every ``down``-th sample — and the fused epilogue of ``family``.  ``taps`` = (k1y, k1x): k = outer(k1y, k1x) in float64 (what
    the caller of the separable kernels vouches for).  ``order`` (the float32 evaluations of the CPU test): 'kykx' = taps row by row, multiply and
    add rounded separately; 'fma' = horizontal sums first, then vertical (``taps``), or column by column (no ``taps``), fused multiply-add."""
    assert _mistake is None or _mistake in MISTAKES
    assert family in ('f32', 'h8')
    x, mask, addend = _c(x, dt, rnd), _c(mask, dt, rnd), _c(addend, dt, rnd)
    noise, bias = _c(noise, dt), _c(bias, dt)
    if taps is not None:
        k1y, k1x = (torch.tensor(t, dtype=torch.float64) for t in taps)
        k = torch.outer(k1y, k1x)
    k = torch.as_tensor(k).double()
    if _mistake == 'taps_transposed' and k.shape[0] == k.shape[1]:
        k = k.t()
        taps = None if taps is None else (taps[1], taps[0])
    kh, kw = k.shape
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    B, C, H, W = x.shape
    oh, ow = out_size(H, uy, dy, py0, py1, kh), out_size(W, ux, dx, px0, px1, kw)
    assert oh > 0 and ow > 0
    if _mistake == 'pad_xy_swapped':                       # the near pads exchanged, the sums kept (so the output keeps its shape)
        px0, px1, py0, py1 = py0, px0 + px1 - py0, px0, py0 + py1 - px0
    # zero insertion: u[i up] = x[i]
    z = torch.zeros(B, C, H * uy, W * ux, dtype=dt)
    if _mistake == 'up_phase_shifted':
        z[:, :, uy - 1::uy, ux - 1::ux] = x
    else:
        z[:, :, ::uy, ::ux] = x
    # pad (positive) or crop (negative): P[r, c] = u[r - py0, c - px0], zero outside u
    PH, PW = H * uy + py0 + py1, W * ux + px0 + px1
    P = torch.zeros(B, C, PH, PW, dtype=dt)
    r0, r1, c0, c1 = max(py0, 0), min(PH, py0 + H * uy), max(px0, 0), min(PW, px0 + W * ux)
    if r1 > r0 and c1 > c0:
        P[:, :, r0:r1, c0:c1] = z[:, :, r0 - py0:r1 - py0, c0 - px0:c1 - px0]
    # correlation with the flipped kernel at every position, then every down-th sample
    kf = k if _mistake == 'taps_not_flipped' else torch.flip(k, [0, 1])
    fh, fw = PH - kh + 1, PW - kw + 1
    win = lambda ky, kx: P[:, :, ky:ky + fh, kx:kx + fw]
    full, M = torch.zeros(B, C, fh, fw, dtype=dt), torch.zeros(B, C, fh, fw, dtype=torch.float64)
    for ky in range(kh):
        for kx in range(kw):
            M += win(ky, kx).double().abs() * abs(float(kf[ky, kx]))
    if order == 'kykx':
        for ky in range(kh):
            for kx in range(kw):
                full = full + win(ky, kx) * kf[ky, kx].to(dt)
    elif taps is not None:
        ty, tx = (torch.flip(torch.tensor(t, dtype=torch.float64), [0]).to(dt) for t in taps)
        if _mistake == 'taps_not_flipped':
            ty, tx = torch.flip(ty, [0]), torch.flip(tx, [0])
        hs = []
        for ky in range(kh):
            h = torch.zeros(B, C, fh, fw, dtype=dt)
            for kx in range(kw):
                h = _fma(win(ky, kx), tx[kx], h, dt)
            hs.append(h)
        for ky in range(kh):
            full = _fma(hs[ky], ty[ky], full, dt)
    else:
        for kx in range(kw):
            for ky in range(kh):
                full = _fma(win(ky, kx), kf[ky, kx].to(dt), full, dt)
    if _mistake == 'down_phase_shifted':
        sub = lambda t: torch.nn.functional.pad(t[:, :, dy - 1::dy, dx - 1::dx], [0, ow, 0, oh])[:, :, :oh, :ow]
    else:
        sub = lambda t: t[:, :, ::dy, ::dx]
    v, M = sub(full), sub(M)
    assert v.shape[2:] == (oh, ow), (v.shape, oh, ow)
    # ---- epilogue
    one = torch.ones((), dtype=dt)
    slope, gain, nw = f32(slope), f32(gain), f32(noise_w)
    if noise is not None:
        nz = noise.expand(B, 1, oh, ow)
        if _mistake == 'noise_per_channel':                # indexed by the map (b C + c) and not by the sample
            nz = torch.stack([noise[(b * C + c) % noise.shape[0], 0] for b in range(B) for c in range(C)]).reshape(B, C, oh, ow)
        v, M = v + nz * nw, M + (nz * nw).abs().double()
    if bias is not None:
        bv = bias[None, :, None, None]
        if _mistake == 'bias_by_batch':
            bv = torch.stack([bias[b % C] for b in range(B)])[:, None, None, None]
        v, M = v + bv, M + bv.abs().double()
    inside = family == 'f32'                               # the addend: inside the activation (f32) or after the mask (h8)
    if addend is not None and inside and _mistake != 'addend_after_act':
        v, M = v + addend, M + addend.abs().double()
    mfac = None
    if mask is not None:
        pos = (mask >= 0) if _mistake == 'mask_zero_is_positive' else (mask > 0)
        mfac = torch.where(pos, f32(mask_vals[0]) * one, f32(mask_vals[1]) * one)
    if mfac is not None and _mistake == 'mask_before_act':
        v, M = v * mfac, M * mfac.abs().double()
    a = ACT_LRELU if (act == ACT_RELU and _mistake == 'relu_is_lrelu') else act
    if a == ACT_LRELU:
        v, M = torch.where(v > 0, v, v * slope), M * max(1.0, abs(slope))
    elif a == ACT_RELU:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    gain_always = (family == 'h8') != (_mistake == 'gain_without_lrelu')
    if a == ACT_LRELU or gain_always:
        v, M = v * gain, M * abs(gain)
    if addend is not None and ((inside and _mistake == 'addend_after_act') or (not inside and _mistake == 'addend_before_mask')):
        v, M = v + addend, M + addend.abs().double()
    if mfac is not None and _mistake != 'mask_before_act':
        v, M = v * mfac, M * mfac.abs().double()
    if addend is not None and not inside and _mistake != 'addend_before_mask':
        v, M = v + addend, M + addend.abs().double()
    return {'y': (v, M)}


def fused_bias_act(x, b=None, ref=None, step_b=1, size_b=1, act=3, grad=0, alpha=0.2, scale=1.0, _mistake=None):
    """out[i] = table(x[i] + b[(i / step_b) % size_b], ref[i]) * scale over the flat tensor, in float32 operation by operation (add, select,
    multiply by alpha, multiply by scale): the contract is exact equality.  Codes act * 10 + grad: 10 / 11 identity, 12 / 32 zero, 30 leaky by
    the sign of the sum, 31 leaky by the sign of ref; any other code: identity."""
    assert _mistake is None or _mistake in MISTAKES
    x = torch.as_tensor(x).float().reshape(-1)
    n = x.numel()
    v = x.clone()
    if b is not None:
        idx = torch.arange(n) // step_b
        idx = idx.clamp(max=size_b - 1) if _mistake == 'fba_bias_index_no_modulo' else idx % size_b
        v = v + torch.as_tensor(b).float()[idx]
    r = torch.zeros(n) if ref is None else torch.as_tensor(ref).float().reshape(-1)
    al, sc = torch.tensor(np.float32(alpha)), torch.tensor(np.float32(scale))
    code = act * 10 + grad
    if code in (12, 32):
        y = torch.zeros(n)
    elif code == 30 or (code == 31 and _mistake == 'fba_ref_ignored'):
        y = torch.where(v > 0, v, v * al)
    elif code == 31:
        y = torch.where(r > 0, v, v * al)
    else:
        y = v
    return {'y': (y * sc, None)}


def modulate_planes(w32, s, elem, _mistake=None):
    """planes[b, c16, t, half, co, e] = round_to_elem(float32(w32[c16, t, half, co, e]) * float32(s[b, 16 c16 + 8 half + e])): the channel of an
    element of the plane order [Cin/16][KK][2][CoutP][8].  Returned in the element type (compare bit patterns)."""
    assert _mistake is None or _mistake in MISTAKES
    w32, s = torch.as_tensor(w32).float(), torch.as_tensor(s).float()
    C16, KK, two, CoutP, eight = w32.shape
    assert two == 2 and eight == 8 and s.shape[1] == 16 * C16
    c16 = torch.arange(C16).view(C16, 1, 1, 1, 1)
    half = torch.arange(2).view(1, 1, 2, 1, 1)
    co = torch.arange(CoutP).view(1, 1, 1, CoutP, 1)
    e = torch.arange(8).view(1, 1, 1, 1, 8)
    if _mistake == 'planes_half_swapped':
        half = 1 - half
    ch = (16 * c16 + 8 * half + e + 0 * co).expand(C16, KK, 2, CoutP, 8)
    if _mistake == 'planes_scale_by_cout':
        ch = ((co + 0 * (c16 + half + e)) % (16 * C16)).expand(C16, KK, 2, CoutP, 8)
    prod = w32[None] * s[:, ch]                                        # float32 product, rounded once
    return {'planes': (prod.to(ELEM_DTYPES[elem]), None)}


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------------
K_CONST = 1                   # the module's constant (stream_ref: k_torgb = C + 1, K_OPS['dz'] ends in + 1)
K_TERMS = {'noise': 2, 'bias': 1, 'bias0': 1, 'addend': 1, 'lrelu': 2, 'relu': 0, 'gain': 1, 'mask': 1, 'mask1': 1}          # rounded operations a term adds


def k_fir(kh, kw, up, ops, family):
    """Live taps of an output (every up-th of the kernel's rows and columns meets a sample) + the epilogue's rounded operations + the constant."""
    live = -(-kh // up[1]) * -(-kw // up[0])
    terms = sum(K_TERMS[o] for o in ops)
    if family == 'h8' and 'relu' in ops:
        terms += 1                                          # h8 multiplies by the gain under every activation
    return live + terms + K_CONST


# ---- launch paths, restated from the two launchers ---------------------------------------------------------------------------------------------------
def path_f32(ih, iw, kh, kw, up, down, pad, ops=(), off=None):
    """The kernel l2i_upfirdn2d(_masked)_f32 takes.  ``off``: {tensor: floats its view starts past a 16-byte boundary}."""
    off = off or {}
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    oh, ow = out_size(ih, uy, dy, py0, py1, kh), out_size(iw, ux, dx, px0, px1, kw)
    has = lambda *names: any(o in ops for o in names)
    mis = lambda name, by: (4 * off.get(name, 0)) % by != 0
    noise, bias, addend, mask = has('noise'), has('bias', 'bias0'), has('addend'), has('mask', 'mask1')
    act = has('lrelu', 'relu')
    k4, unit = (kh, kw) == (4, 4), (ux, uy, dx, dy) == (1, 1, 1, 1)
    if unit and k4 and px0 in (1, 2) and ow >= 192 and iw % 4 == 0 and ow % 4 == 0 and not (
            mis('x', 16) or mis('y', 16) or (noise and mis('noise', 16)) or (addend and mis('addend', 16)) or (mask and mis('mask', 16))):
        return 'upfirdn2d_k4_stream_kernel<%d>' % px0
    if unit and k4:
        return 'upfirdn2d_k4_kernel'
    if (ux, uy, dx, dy) == (1, 1, 2, 2) and k4 and px0 == 1 and py0 == 1 and ow >= 96 and iw % 4 == 0 and ow % 2 == 0 and not (
            noise or bias or addend or mask or act) and not mis('x', 16) and not mis('y', 8):
        return 'upfirdn2d_k4_down2_stream_kernel'
    if (ux, uy, dx, dy) == (2, 2, 1, 1) and k4 and px0 == 2 and py0 == 2 and oh == 2 * ih and ow == 2 * iw and ow % 4 == 0 and not mask and not (
            mis('y', 16) or (addend and mis('addend', 16))):
        return 'upfirdn2d_up2k4_kernel'
    return 'upfirdn2d_kernel'


def path_h8(ih, iw, kh, kw, up, down, pad, ops=(), sep=True, mask_bits=False):
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    assert ux == uy and dx == dy
    oh, ow = out_size(ih, uy, dy, py0, py1, kh), out_size(iw, ux, dx, px0, px1, kw)
    has = lambda *names: any(o in ops for o in names)
    k4 = sep and (kh, kw) == (4, 4)
    if k4 and ux == 1 and dx == 1:
        return 'upfirdn2d_h8_sep4_kernel<MBITS>' if mask_bits else 'upfirdn2d_h8_sep4_kernel'
    plain = not has('noise', 'bias', 'bias0', 'lrelu', 'relu', 'gain', 'mask', 'mask1')
    if k4 and plain and ux == 1 and dx == 2 and not has('addend') and px0 == 1 and py0 == 1:
        return 'upfirdn2d_h8_sep4_down2_kernel'
    if k4 and plain and ux == 2 and dx == 1 and px0 == 2 and py0 == 2 and oh == 2 * ih and ow == 2 * iw:
        return 'upfirdn2d_h8_sep4_up2_kernel'
    return 'upfirdn2d_h8_kernel'


def path_fba(n, step_b, has_b, off=None):
    off = off or {}
    vec = n % 4 == 0 and (not has_b or step_b % 4 == 0) and not any(off.get(t, 0) % 4 for t in ('y', 'x', 'ref'))
    return 'fba_kernel<true>' if vec else 'fba_kernel<false>'


# ---- the dispatch predicates, each false alone in one twin row (tests/test_fir_ref_cpu.py counts them against the rows) -----------------------------------
PREDICATES = {
    'upfirdn2d_k4_stream_kernel': ('out_w_ge_192', 'in_w_mod4', 'out_w_mod4', 'pad_x0_is_0', 'pad_x0_is_3', 'x_off', 'y_off', 'noise_off', 'addend_off', 'mask_off'),
    'upfirdn2d_k4_down2_stream_kernel': ('out_w_ge_96', 'in_w_mod4', 'out_w_even', 'pad_x0_is_2', 'pad_y0_is_2', 'epilogue_operand', 'x_off', 'y_off'),
    'upfirdn2d_up2k4_kernel': ('out_w_mod4', 'natural_size', 'mask_present', 'y_off', 'addend_off'),
    'upfirdn2d_h8_sep4_kernel': ('no_k1',),
    'upfirdn2d_h8_sep4_down2_kernel': ('pad_x0_is_2', 'pad_y0_is_2', 'addend', 'epilogue_operand', 'no_k1'),
    'upfirdn2d_h8_sep4_up2_kernel': ('natural_size', 'no_k1'),
    'fba_kernel<true>': ('n_mod4', 'step_b_mod4', 'y_off', 'x_off', 'ref_off'),
}

# every l2i_set_error line of the five launchers (keyed by a piece of its message) and the mask_bits rule: the argument combinations that reach it
REFUSALS = {
    'fused_bias_act: null tensor': ('y_null', 'x_null', 'n_negative'),
    'fused_bias_act: bias needs': ('step_b_zero', 'size_b_zero'),
    'upfirdn2d: null tensor': ('y_null', 'x_null', 'k_null'),
    'upfirdn2d: empty input': ('major_zero', 'in_h_zero', 'in_w_zero'),
    'upfirdn2d: FIR must have': ('kh_zero', 'kw_zero', 'taps_65'),
    'upfirdn2d: up/down must be positive': ('up_x_zero', 'up_y_zero', 'down_x_zero', 'down_y_zero'),
    'upfirdn2d: empty output': ('out_h_zero', 'out_w_zero'),
    'upfirdn2d_h8: null tensor': ('y_null', 'x_null', 'k_null'),
    'upfirdn2d_h8: a sign-plane mask': ('bits_up2', 'bits_down2', 'bits_no_k1', 'bits_k3', 'bits_mask_null'),
    'upfirdn2d_h8: kernels up to 4x4': ('planes_zero', 'channels_zero', 'channels_12', 'in_h_zero', 'in_w_zero', 'kh_zero', 'kw_5', 'up_3', 'down_0'),
    'upfirdn2d_h8: empty output': ('out_h_zero', 'out_w_zero'),
    'modulate_planes_h8: bad arguments': ('planes_null', 'w32_null', 's_null', 'B_zero', 'CinP_zero', 'CinP_24', 'Cs_above', 'KK_zero', 'CoutP_zero'),
    'modulate_planes_h8: the scale vector': ('Cs_below',),
    'modulate_planes_h8: planes and w32 must be': ('w32_off', 'planes_off'),
    'modulate_planes_multi_h8: bad arguments': ('planes_null', 'w32_null', 's_null', 'table_null', 'nseg_zero', 'B_zero', 'nblocks_below_nseg'),
}
REFUSAL_CODE = {m: (-3 if 'sign-plane' in m else -1) for m in REFUSALS}
LAUNCHERS = {'l2i_stream.hip': ('l2i_fused_bias_act_f32', 'upfirdn2d_launch'),
             'l2i_stream_h8.hip': ('H8_NAME(l2i_upfirdn2d_h8)', 'H8_NAME(l2i_modulate_planes_h8)', 'H8_NAME(l2i_modulate_planes_multi_h8)')}

# __global__ kernels of the two files that a row of this module claims (the rest: stream_ref.CLAIMED_KERNELS)
CLAIMED_KERNELS = ('fba_kernel', 'upfirdn2d_kernel', 'upfirdn2d_k4_kernel', 'upfirdn2d_k4_down2_stream_kernel', 'upfirdn2d_up2k4_kernel',
                   'upfirdn2d_k4_stream_kernel', 'upfirdn2d_h8_kernel', 'upfirdn2d_h8_sep4_kernel', 'upfirdn2d_h8_sep4_down2_kernel',
                   'upfirdn2d_h8_sep4_up2_kernel', 'modulate_planes_kernel', 'modulate_planes_multi_kernel')

OPERANDS_F32 = (('noise',), ('bias',), ('addend',), ('lrelu',), ('relu',), ('gain',), ('mask',))
ALL_F32 = ('noise', 'bias', 'addend', 'lrelu', 'mask')
OPERANDS_H8 = OPERANDS_F32
ALL_H8 = ALL_F32
FBA_CODES = ((1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2), (2, 0))          # the six codes of the table and one outside it (20: the default branch)
# (CinP, KK, CoutP, B)
PLANE_GEOMS = [(16, 1, 32, 1), (48, 9, 96, 3), (16, 9, 96, 3), (48, 1, 32, 1)]
PLANE_MULTI = [(16, 9, 32), (48, 1, 96), (32, 9, 40)]                           # three unequal layers of one table: (CinP, KK, CoutP)


def _in(out, p0, p1, k=4):
    """Input extent that gives ``out`` at up = down = 1."""
    return out - p0 - p1 + k - 1


def _name(ops):
    return '+'.join(ops) if ops else 'plain'


def all_rows():
    rows = []

    def fir(kind, case, geom, B, C, ih, iw, path, k='K44', up=(1, 1), down=(1, 1), pad=(1, 2, 2, 1), ops=(), **extra):
        rows.append(Row('fir', kind, case, geom, (B, C, ih, iw), path, k=k, up=up, down=down, pad=pad, ops=tuple(ops), **extra))
        return rows[-1].id

    def k4(case, ow, oh, pad, path, ops=(), B=2, C=2, iw=None, **extra):
        return fir('f32', case, 'w%d_h%d_p%s' % (ow, oh, '_'.join(map(str, pad)).replace('-', 'm')), B, C, _in(oh, pad[2], pad[3]),
                   _in(ow, pad[0], pad[1]) if iw is None else iw, path, pad=pad, ops=ops, **extra)

    S1, S2, K4 = 'upfirdn2d_k4_stream_kernel<1>', 'upfirdn2d_k4_stream_kernel<2>', 'upfirdn2d_k4_kernel'
    # ---- upfirdn2d_k4_stream_kernel: strips of 256 columns (192 = smallest admitted, 260 = a second strip with one live lane), waves of 16 rows, bands of 64
    for ow, oh, pad in ((192, 15, (1, 2, 2, 1)), (256, 17, (2, 1, 1, 2)), (260, 65, (1, -2, 2, -2)), (260, 17, (2, 5, 1, 4)), (192, 65, (2, 1, 1, 2)),
                        (256, 15, (1, -2, 2, -2))):
        k4('plain', ow, oh, pad, S1 if pad[0] == 1 else S2)
    for ops in OPERANDS_F32 + (ALL_F32,):
        k4(_name(ops), 260, 17, (1, 2, 2, 1), S1, ops)
    k4(_name(ALL_F32), 260, 17, (2, 1, 1, 2), S2, ALL_F32)
    base = k4(_name(ALL_F32), 192, 15, (1, 2, 2, 1), S1, ALL_F32)
    # each predicate false alone: the launch falls to upfirdn2d_k4_kernel, whose result on the same data is the same bits (the code's claim)
    tw = dict(twin=base, ops=ALL_F32)
    k4('twin', 188, 15, (1, 2, 2, 1), K4, pred='out_w_ge_192', **tw)
    k4('twin', 192, 15, (1, 4, 2, 1), K4, pred='in_w_mod4', **tw)                       # in_w = 190
    k4('twin', 191, 15, (1, 1, 2, 1), K4, pred='out_w_mod4', **tw)                      # in_w = 192
    k4('twin', 192, 15, (0, 3, 2, 1), K4, pred='pad_x0_is_0', **tw)                     # x moved one column right
    k4('twin', 192, 15, (3, 0, 2, 1), K4, pred='pad_x0_is_3', **tw)                     # x moved two columns left
    for t in ('x', 'y', 'noise', 'addend', 'mask'):
        k4('twin_%s_off' % t, 192, 15, (1, 2, 2, 1), K4, pred=t + '_off', off={t: 1}, **tw)
    # ---- upfirdn2d_k4_kernel: tiles of 32 x 64 outputs, ragged both ways; the scalar store branch; pad_x0 over {-1 .. 5} with another pad_y0
    for oh, ow in ((31, 63), (33, 65), (32, 64)):
        k4('plain', ow, oh, (2, 1, 1, 2), K4)
    for px0, py0 in ((-1, 2), (0, 1), (1, 3), (2, 0), (3, 1), (5, -1)):
        k4('plain', 37, 9, (px0, 3 - px0, py0, 2), K4)
    k4('plain_y_off', 64, 9, (2, 1, 1, 2), K4, off={'y': 1})
    for ops in OPERANDS_F32 + (ALL_F32,):
        k4(_name(ops), 66, 33, (2, 1, 1, 2), K4, ops)
    k4('bias+noise_partial_sample', 37, 9, (1, 2, 2, 1), K4, ('noise', 'bias'), B=2, C=3, major=5)          # major = 5, channels = 3: not refused (l2i.h)
    # ---- upfirdn2d_k4_down2_stream_kernel: strips of 128 output columns, waves of 8 rows, bands of 32
    D2, G = 'upfirdn2d_k4_down2_stream_kernel', 'upfirdn2d_kernel'

    def d2(case, ow, oh, path, pad=None, iw=None, ih=None, **extra):
        pad = pad or (1, 1, 1, 1)
        iw, ih = iw or 2 * ow, ih or 2 * oh
        assert out_size(iw, 1, 2, pad[0], pad[1], 4) == ow and out_size(ih, 1, 2, pad[2], pad[3], 4) == oh, (case, ow, oh)
        return fir('f32', case, 'down2_w%d_h%d' % (ow, oh), 2, 2, ih, iw, path, down=(2, 2), pad=pad, **extra)

    for ow, oh in ((96, 8), (128, 9), (130, 33)):
        d2('plain', ow, oh, D2)
    base = d2('plain', 130, 9, D2)
    d2('twin_out_w_ge_96', 94, 9, G, twin=base, pred='out_w_ge_96')
    d2('twin_in_w_mod4', 130, 9, G, pad=(1, 3, 1, 1), iw=258, twin=base, pred='in_w_mod4')
    d2('twin_out_w_even', 129, 9, G, pad=(1, -1, 1, 1), iw=260, twin=base, pred='out_w_even')
    d2('twin_pad_x0_is_2', 130, 9, G, pad=(2, 0, 1, 1), twin=base, pred='pad_x0_is_2')
    d2('twin_pad_y0_is_2', 130, 9, G, pad=(1, 1, 2, 0), twin=base, pred='pad_y0_is_2')
    d2('twin_bias0', 130, 9, G, ops=('bias0',), twin=base, pred='epilogue_operand')
    d2('twin_x_off', 130, 9, G, off={'x': 1}, twin=base, pred='x_off')
    d2('twin_y_off', 130, 9, G, off={'y': 1}, twin=base, pred='y_off')
    # ---- upfirdn2d_up2k4_kernel: a thread owns 2 x 4 outputs
    U2 = 'upfirdn2d_up2k4_kernel'

    def u2(case, ih, iw, path, pad=(2, 1, 2, 1), ops=(), C=3, **extra):
        return fir('f32', case, 'up2_%dx%d%s' % (ih, iw, '' if C == 3 else '_c%d' % C), 2, C, ih, iw, path, up=(2, 2), pad=pad, ops=ops, **extra)

    for ih, iw in ((1, 2), (5, 6), (9, 34)):
        u2('plain', ih, iw, U2)
    for ops in (('noise',), ('bias',), ('addend',), ('lrelu',), ('relu',), ('noise', 'bias', 'addend', 'lrelu')):
        u2(_name(ops), 5, 6, U2, ops=ops)
    base, base_a = u2('plain', 9, 34, U2, C=2), u2('addend', 9, 34, U2, ops=('addend',), C=2)
    u2('twin_out_w_mod4', 9, 33, G, twin=base, pred='out_w_mod4', C=2)
    u2('twin_natural_size', 9, 34, G, pad=(2, 1, 2, 2), twin=base, pred='natural_size', C=2)          # out_h = 2 in_h + 1, out_w % 4 == 0 still
    u2('pad_2_2_2_1', 9, 34, G, pad=(2, 2, 2, 1), twin=base, C=2)                                     # out_w = 2 in_w + 1 (no multiple of 4 either)
    u2('twin_mask1', 9, 34, G, ops=('mask1',), twin=base, pred='mask_present', C=2)
    u2('twin_y_off', 9, 34, G, off={'y': 1}, twin=base, pred='y_off', C=2)
    u2('twin_addend_off', 9, 34, G, ops=('addend',), off={'addend': 1}, twin=base_a, pred='addend_off', C=2)
    # ---- upfirdn2d_kernel: tiles of 16 x 64; rectangular and non-separable FIRs, unequal up / down in x and y; output 17 x 65 where up = down = 1
    for kname in ('K11', 'K23', 'K35', 'K88', 'K44N'):
        kh, kw = KERNELS[kname].shape
        pad = (kw // 2, kw - 1 - kw // 2 + 1, kh - 1 - kh // 2, kh // 2 + 1)
        path = K4 if kname == 'K44N' else G
        fir('f32', 'plain', 'generic_%s' % kname, 2, 2, _in(17, pad[2], pad[3], kh), _in(65, pad[0], pad[1], kw), path, k=kname, pad=pad)
    for up, down in (((2, 1), (1, 1)), ((1, 3), (1, 1)), ((3, 2), (1, 1)), ((1, 1), (1, 2)), ((1, 1), (2, 1)), ((1, 1), (3, 3)), ((3, 2), (2, 3))):
        fir('f32', 'plain', 'generic_K35_up%d%d_down%d%d' % (up + down), 2, 2, 11, 23, G, k='K35', up=up, down=down, pad=(2, 3, 1, 0))
    for ops in OPERANDS_F32 + (ALL_F32,):
        fir('f32', _name(ops), 'generic_K44N_up12_down21', 2, 3, 10, 35, G, k='K44N', up=(1, 2), down=(2, 1), pad=(1, 2, 2, 1), ops=ops)
    fir('f32', 'bias+noise_partial_sample', 'generic_K23', 2, 3, 9, 20, G, k='K23', pad=(1, 1, 0, 1), ops=('noise', 'bias'), major=5)
    # ---- h8: the separable register-streaming kernels (chunks of 61 columns, bands of 16 rows) and the generic one
    P, PB, HG = 'upfirdn2d_h8_sep4_kernel', 'upfirdn2d_h8_sep4_kernel<MBITS>', 'upfirdn2d_h8_kernel'

    def h4(case, ow, oh, pad, path, ops=(), C=8, **extra):
        return fir('h8', case, 'w%d_h%d_p%s' % (ow, oh, '_'.join(map(str, pad)).replace('-', 'm')), 2, C, _in(oh, pad[2], pad[3]), _in(ow, pad[0], pad[1]),
                   path, pad=pad, ops=ops, **extra)

    for ow, oh, pad in ((60, 16, (1, 1, 2, 2)), (61, 17, (2, 2, 1, 1)), (62, 33, (0, 3, 3, 0)), (123, 17, (1, -2, 2, 5)), (62, 16, (1, 1, 2, 2)),
                        (123, 33, (2, 2, 1, 1))):
        h4('plain', ow, oh, pad, P, C=16 if ow == 61 else 8)
    for ops in OPERANDS_H8 + (ALL_H8,):
        h4(_name(ops), 62, 17, (1, 2, 2, 1), P, ops)
    h4('mask_bits', 62, 17, (1, 2, 2, 1), PB, ('mask',), mask_bits=True)
    h4(_name(ALL_H8) + '_bits', 123, 17, (2, 1, 1, 2), PB, ALL_H8, mask_bits=True, C=16)
    h4('twin_no_k1', 62, 17, (1, 2, 2, 1), HG, sep=False, pred='no_k1', pred_of=P)

    def hd(case, ow, oh, path, pad=(1, 1, 1, 1), ops=(), **extra):
        ih, iw = 2 * oh + 2 - pad[2] - pad[3], 2 * ow + 2 - pad[0] - pad[1]
        assert out_size(iw, 1, 2, pad[0], pad[1], 4) == ow and out_size(ih, 1, 2, pad[2], pad[3], 4) == oh
        return fir('h8', case, 'down2_w%d_h%d' % (ow, oh), 2, 8, ih, iw, path, down=(2, 2), pad=pad, ops=ops, **extra)

    HD, HU = 'upfirdn2d_h8_sep4_down2_kernel', 'upfirdn2d_h8_sep4_up2_kernel'
    for ow, oh in ((61, 8), (62, 9), (63, 9)):
        hd('plain', ow, oh, HD)
    hd('twin_pad_x0_is_2', 63, 9, HG, pad=(2, 0, 1, 1), pred='pad_x0_is_2', pred_of=HD)
    hd('twin_pad_y0_is_2', 63, 9, HG, pad=(1, 1, 2, 0), pred='pad_y0_is_2', pred_of=HD)
    hd('twin_addend', 63, 9, HG, ops=('addend',), pred='addend', pred_of=HD)
    hd('twin_bias', 63, 9, HG, ops=('bias',), pred='epilogue_operand', pred_of=HD)
    hd('twin_no_k1', 63, 9, HG, sep=False, pred='no_k1', pred_of=HD)
    for ih, iw in ((8, 61), (9, 62), (9, 63)):
        for ops in ((), ('addend',)):
            fir('h8', _name(ops), 'up2_%dx%d' % (ih, iw), 2, 8, ih, iw, HU, up=(2, 2), pad=(2, 1, 2, 1), ops=ops)
    fir('h8', 'twin_natural_size', 'up2_9x63', 2, 8, 9, 63, HG, up=(2, 2), pad=(2, 2, 2, 2), pred='natural_size', pred_of=HU)
    fir('h8', 'twin_no_k1', 'up2_9x63', 2, 8, 9, 63, HG, up=(2, 2), pad=(2, 1, 2, 1), sep=False, pred='no_k1', pred_of=HU)
    for kname in ('K11', 'K23', 'K44N'):
        kh, kw = KERNELS[kname].shape
        for up in (1, 2):
            for down in (1, 2):
                fir('h8', 'plain', 'generic_%s_up%d_down%d' % (kname, up, down), 2, 8, 7, 13, HG, k=kname, up=(up, up), down=(down, down),
                    pad=(kw // 2, kw // 2 + 1, kh - 1 - kh // 2, kh // 2), sep=False)
    for ops in OPERANDS_H8 + (ALL_H8,):
        fir('h8', _name(ops), 'generic_K23_up2_down1', 2, 16, 7, 13, HG, k='K23', up=(2, 2), pad=(1, 2, 1, 0), ops=ops, sep=False)
    # ---- fused_bias_act: six codes and the default, the vector path (step_b = 12: one channel per float4) and the scalar one (7); size_b = 5, three wraps
    V, Sc = 'fba_kernel<true>', 'fba_kernel<false>'

    def fba(case, geom, n, step_b, path, act=3, grad=0, **extra):
        rows.append(Row('fba', 'f32', case, geom, (1, 1, 1, n), path, step_b=step_b, size_b=5, act=act, grad=grad, **extra))

    for act, grad in FBA_CODES:
        fba('code%d%d' % (act, grad), 'step12', 180, 12, V, act, grad)
        fba('code%d%d' % (act, grad), 'step7', 105, 7, Sc, act, grad)
    fba('code30_no_bias', 'step12', 180, 12, V, has_b=False)
    fba('code30_no_bias', 'n105', 105, 7, Sc, has_b=False)
    fba('code31', 'two_blocks', 4 * 300, 12, V, 3, 1)
    fba('twin_n_mod4', 'step12', 182, 12, Sc, 3, 1, pred='n_mod4')
    fba('twin_step_b_mod4', 'step7', 140, 7, Sc, 3, 1, pred='step_b_mod4')
    for t in ('y', 'x', 'ref'):
        fba('twin_%s_off' % t, 'step12', 180, 12, Sc, 3, 1, off={t: 1}, pred=t + '_off')
    # ---- weight planes
    for CinP, KK, CoutP, B in PLANE_GEOMS:
        rows.append(Row('planes', 'h8', 'single', 'cin%d_kk%d_cout%d_b%d' % (CinP, KK, CoutP, B), (B, CinP, KK, CoutP), 'modulate_planes_kernel'))
    for B in (1, 3):
        for spread in (False, True):
            rows.append(Row('planes_multi', 'h8', 'blocks_%s' % ('above_minimum' if spread else 'minimum'), 'three_layers_b%d' % B, (B, 0, 0, 0),
                            'modulate_planes_multi_kernel', spread=spread))
    assert len({r.id for r in rows}) == len(rows), [r.id for r in rows if [q.id for q in rows].count(r.id) > 1]
    return rows


_ROWS = None


def row_by_id(rid):
    global _ROWS
    if _ROWS is None:
        _ROWS = {r.id: r for r in all_rows()}
    return _ROWS[rid]


def geom(row):
    """Sizes of a FIR row: dict(kh, kw, oh, ow, family)."""
    B, C, ih, iw = row.shape
    e = row.extra
    kh, kw = KERNELS[e['k']].shape
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = e['up'], e['down'], e['pad']
    return dict(kh=kh, kw=kw, oh=out_size(ih, uy, dy, py0, py1, kh), ow=out_size(iw, ux, dx, px0, px1, kw))


def row_path(row):
    """The kernel the launcher takes for a row, from the restated predicates."""
    e = row.extra
    if row.op == 'fir':
        B, C, ih, iw = row.shape
        kh, kw = KERNELS[e['k']].shape
        if row.kind == 'f32':
            return path_f32(ih, iw, kh, kw, e['up'], e['down'], e['pad'], e['ops'], e.get('off'))
        return path_h8(ih, iw, kh, kw, e['up'], e['down'], e['pad'], e['ops'], e.get('sep', True), e.get('mask_bits', False))
    if row.op == 'fba':
        return path_fba(row.shape[3], e['step_b'], e.get('has_b', True), e.get('off'))
    return row.path


def _edge_signs(m):
    """Both zeros, the smallest normals and values a 16-bit type rounds to zero where a wave's chunk or strip and a band end (columns 59 .. 62, rows 15, 16)."""
    v = [-0.0, 0.0, 2.0 ** -126, -2.0 ** -126, 1e-42, -1e-42]
    H, W = m.shape[2:]
    for i, (r, c) in enumerate((r, c) for r in (15, 16) for c in (59, 60, 61, 62)):
        if r < H and c < W:
            m[:, :, r, c] = v[i % len(v)]
    return m


def twin_shift(row, base):
    """(sx, sy): the twin's x is the base's moved so that both read the same samples, xt[r, c] = xb[r + sy, c + sx]."""
    return row.extra['pad'][0] - base.extra['pad'][0], row.extra['pad'][2] - base.extra['pad'][2]


def twin_valid(row, base):
    """[oh, ow] of the twin: outputs whose taps read the same samples in both launches (elsewhere one of them reads across an edge the other
    does not have) and that both have."""
    g, gb = geom(row), geom(base)
    sx, sy = twin_shift(row, base)

    def axis(n_t, n_b, o_t, o_b, k, u, d, p_t, s):
        ok = np.zeros(o_t, dtype=bool)
        for o in range(min(o_t, o_b)):
            good = True
            for t in range(k):
                ut = o * d + t - p_t
                if ut % u:
                    continue
                it = ut // u
                ib = it + s
                if not (0 <= it < n_t) and (0 <= ib < n_b):
                    good = False
            ok[o] = good
        return ok

    e = row.extra
    vx = axis(row.shape[3], base.shape[3], g['ow'], gb['ow'], g['kw'], e['up'][0], e['down'][0], e['pad'][0], sx)
    vy = axis(row.shape[2], base.shape[2], g['oh'], gb['oh'], g['kh'], e['up'][1], e['down'][1], e['pad'][2], sy)
    return torch.from_numpy(vy[:, None] & vx[None, :])


def _fit(t_own, t_base):
    """``t_own`` with the overlap (from the top left corner) replaced by ``t_base``."""
    h, w = min(t_own.shape[2], t_base.shape[2]), min(t_own.shape[3], t_base.shape[3])
    t_own = t_own.clone()
    t_own[:, :, :h, :w] = t_base[:, :, :h, :w]
    return t_own


def make_inputs(row, elem='f32'):
    """The operands of a row as float32 CPU tensors / Python scalars keyed by the model's keyword names ('_' keys: for the runner only)."""
    rs = np.random.RandomState(row.seed)
    e = row.extra
    if row.op == 'fir':
        B, C, ih, iw = row.shape
        g = geom(row)
        oh, ow = g['oh'], g['ow']
        ops, h8 = e['ops'], row.kind == 'h8'
        kw = {'x': T(rs.randn(B, C, ih, iw)), 'k': KERNELS[e['k']].float(), 'up': e['up'], 'down': e['down'], 'pad': e['pad'], 'act': ACT_NONE, 'slope': 0.2, 'gain': 1.0}
        if e.get('sep', True) and e['k'] in TAPS and h8:
            kw['taps'] = TAPS[e['k']]
        if 'noise' in ops:
            kw['noise'], kw['noise_w'] = T(rs.randn(B, 1, oh, ow)), 0.3
        if 'bias' in ops:
            kw['bias'] = T(rs.randn(C))
        if 'bias0' in ops:
            kw['bias'] = torch.zeros(C)
        if 'addend' in ops:
            kw['addend'] = T(rs.randn(B, C, oh, ow))
        if 'lrelu' in ops:
            kw['act'], kw['gain'] = ACT_LRELU, SQRT2
        if 'relu' in ops:
            kw['act'], kw['gain'] = ACT_RELU, 1.5
        if 'gain' in ops:
            kw['gain'] = 1.5
        if 'mask' in ops:
            kw['mask'], kw['mask_vals'] = _edge_signs(plant_signs(T(rs.randn(B, C, oh, ow)), h8)), (SQRT2, -0.2 * SQRT2)          # a negative factor: a positive one commutes with the activation, and mask_before_act would not show
        if 'mask1' in ops:
            kw['mask'], kw['mask_vals'] = torch.ones(B, C, oh, ow), (1.0, 0.0)
        if e.get('major'):                                  # a partial last sample: the maps past ``major`` do not exist
            kw['_major'] = e['major']
        if e.get('twin'):
            base = row_by_id(e['twin'])
            kb = make_inputs(base, elem)
            sx, sy = twin_shift(row, base)
            xb, xt = kb['x'], torch.zeros(B, C, ih, iw)
            for r in range(ih):
                if 0 <= r + sy < xb.shape[2]:
                    lo, hi = max(0, -sx), min(iw, xb.shape[3] - sx)
                    xt[:, :, r, lo:hi] = xb[:, :, r + sy, lo + sx:hi + sx]
            kw['x'] = xt
            for name in ('noise', 'addend', 'mask'):
                if name in kw and name in kb:
                    kw[name] = _fit(kw[name], kb[name])
            if 'bias' in kw and 'bias' in kb:
                kw['bias'] = kb['bias'].clone()
        return kw
    if row.op == 'fba':
        n = row.shape[3]
        kw = {'x': T(rs.randn(n)), 'step_b': e['step_b'], 'size_b': e['size_b'], 'act': e['act'], 'grad': e['grad'], 'alpha': 0.2, 'scale': SQRT2}
        if e.get('has_b', True):
            kw['b'] = T(rs.randn(e['size_b']))
        if e['grad'] == 1 or e['act'] == 2:
            kw['ref'] = plant_signs(T(rs.randn(n)))
        return kw
    if row.op == 'planes':
        B, CinP, KK, CoutP = row.shape
        return {'w32': T(rs.randn(CinP // 16, KK, 2, CoutP, 8)), 's': T(rs.rand(B, CinP) + 0.5)}
    if row.op == 'planes_multi':
        B = row.shape[0]
        return {'layers': [{'w32': T(rs.randn(CinP // 16, KK, 2, CoutP, 8)), 's': T(rs.rand(B, CinP) + 0.5)} for CinP, KK, CoutP in PLANE_MULTI]}
    raise KeyError(row.op)


def multi_table(layers, B, spread):
    """The device table of l2i_modulate_planes_multi_h8 for ``layers``: (rows of eight int64, nblocks).  One block per segment is the least the
    entry takes; ``spread``: 2, 1 and 4 blocks."""
    rows, w_off, s_off, out_off, first = [], 0, 0, 0, 0
    for i, L in enumerate(layers):
        C16, KK, _, CoutP, _ = L['w32'].shape
        sps = C16 * KK * 2 * CoutP
        rows.append([w_off, s_off, out_off, sps, KK, CoutP, 16 * C16, first])
        w_off, s_off, out_off = w_off + L['w32'].numel(), s_off + B * 16 * C16, out_off + sps * B
        first += (2, 1, 4)[i % 3] if spread else 1
    return rows, first


def expected(row, kw, elem, dt=torch.float64, order='kykx', _mistake=None):
    """{output: (want, bound)}: bound None = exact."""
    mk = {} if _mistake is None else {'_mistake': _mistake}
    arg = {k: v for k, v in kw.items() if not k.startswith('_')}
    if row.op == 'fir':
        family = row.kind
        g = geom(row)
        want, M = upfirdn2d(family=family, rnd=rnd_for(elem) if family == 'h8' else None, dt=dt, order=order, **arg, **mk)['y']
        k = k_fir(g['kh'], g['kw'], row.extra['up'], row.extra['ops'], family)
        if kw.get('_major'):
            n = kw['_major']
            want, M = want.reshape((-1,) + want.shape[2:])[:n], M.reshape((-1,) + M.shape[2:])[:n]
        return {'y': (want, bound16(want, M, k, elem) if family == 'h8' else bound_elem(M, k))}
    if row.op == 'fba':
        return fused_bias_act(**arg, **mk)
    if row.op == 'planes':
        return modulate_planes(kw['w32'], kw['s'], elem, **mk)
    if row.op == 'planes_multi':
        return {'planes%d' % i: modulate_planes(L['w32'], L['s'], elem, **mk)['planes'] for i, L in enumerate(kw['layers'])}
    raise KeyError(row.op)
