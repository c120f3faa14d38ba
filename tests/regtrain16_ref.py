"""The contract of the training kernels on 16-bit h8 maps (csrc/l2i_train_h8.hip; include/l2i.h: l2i_conv2d_wgrad_h8, l2i_bn_stats_h8,
l2i_bn_apply_h8, l2i_bn_bwd_reduce_h8, l2i_bn_bwd_apply_h8 and their _f16 twins), written once in float64 with derived bounds, and the case tables
that drive tests/test_regtrain16_kernels_gpu.py (checked on the CPU by tests/test_regtrain16_ref_cpu.py).

Model.  The operands are what the kernels read: the maps rounded to the element type (bf16 or IEEE fp16, round to nearest even), the [C] vectors
and scalars as float32.  Then, in float64:

    wgrad       dw[co,ci,ky,kx] = out_scale * sum_{b,oy,ox} gy[b,co,oy,ox] * x[b,ci,oy*s+ky-p,ox*s+kx-p]      (pixels in the padding contribute 0)
    stats       sum[c] = sum x, sumsq[c] = sum x^2 over (b, pixel)
    apply       y = relu?(x * scale[c] + shift[c] (+ residual)), ONE rounding to the element type
    bwd_reduce  sum_dy[c] = sum dy, sum_dyxh[c] = sum dy * xhat, dy = gy * (out > 0) when an output map is given, xhat = (x - mean[c]) * invstd[c]
    bwd_apply   dx = gamma[c] * invstd[c] * (dy - m_dy[c] - xhat * m_dyxh[c]), ONE rounding; the masked dy is stored exactly (a select)
    forward     stats -> finalize (mean, biased variance, invstd = 1 / sqrt(var + eps), scale = gamma invstd, shift = beta - mean scale) -> apply:
                what a BatchNorm layer of the 16-bit trainer computes; l2i_bn_finalize_f32 has its own test, here it ties the pieces together.

Bounds (nothing here is measured on a kernel).
    wgrad       a product of two fp16 or two bf16 values is exact in fp32, so only the accumulation rounds: N = B OH OW fp32 additions in some order,
                2^-23 each (twice the unit roundoff: the matrix pipe's internal adds are not promised to round to nearest), + 2 for the two
                multiplies of out_scale, relative to M = |out_scale| sum |gy| |x|:  bound = 2^-23 (N + 2) M.
    stats       float64 sums of exact values (the square of a 16-bit value is exact in float64): 2^-52 N M, M = sum |x| resp. sum x^2.
    apply       half an ulp of the store + 2^-23 k M (stream_ref.bound16), k = 3 (multiply, add, residual add), M = |x| |scale| + |shift| + |residual|.
    bwd_reduce  xhat costs two fp32 roundings relative to (|x| + |mean|) |invstd|; the products and sums are float64:
                bound = (2 * 2^-23 + 2^-52 N) M, M = sum |dy| (|x| + |mean|) |invstd|; sum_dy: 2^-52 N sum |dy|.
    bwd_apply   half an ulp + 2^-23 k M with k = 7 (gamma invstd; x - mean, * invstd; * m_dyxh; two subtractions; the final product),
                M = |gamma invstd| (|dy| + |m_dy| + (|x| + |mean|) |invstd| |m_dyxh|).
    forward     as apply, on the float64 statistics; scale and shift carry the few float32 roundings of finalize: k = 8, and M takes
                (|x| + |mean|) |scale| + |beta| in place of |x| |scale| + |shift| (the shift's own roundings are relative to its two terms).

MISTAKES are seeded errors; CASES name the ones each case must expose (tests/test_regtrain16_ref_cpu.py proves that each breaks the bound there
and that a correct float32 evaluation stays inside it).  A plain module: no fixtures, no kernel code."""
from collections import namedtuple

import numpy as np
import torch

from tests.stream_ref import U23, ELEM_DTYPES, bound16, bound_elem, from_h8, rnd_for, to_h8, worst      # noqa: F401 (shared, re-exported)

ELEMS = ('bf16', 'f16')
SENTINEL = -7680.0            # exactly representable in fp32, bf16 and fp16
U52 = 2.0 ** -52
BN_EPS = 1e-5

MISTAKES = ('dropped_tap', 'tap_shifted', 'padding_as_data', 'slice_tail_dropped', 'co_ci_swapped', 'stride_ignored', 'out_scale_forgotten',
            'mask_wrong_operand', 'unbiased_variance', 'residual_after_relu')

WgradCase = namedtuple('WgradCase', 'name k stride pad cin cout b h w host_scale dev_scale mistakes')
# (the cases of the issue; `slices`: enough pixels for several slices of 256-pixel chunks, so that the second pass does the adding)
WGRAD_CASES = (
    WgradCase('one_pixel', 1, 1, 0, 32, 32, 1, 1, 1, 1.0, None, ('co_ci_swapped',)),
    WgradCase('ragged_1x1', 1, 1, 0, 64, 96, 3, 5, 7, 0.25, None, ('slice_tail_dropped', 'out_scale_forgotten')),
    WgradCase('border_3x3', 3, 1, 1, 32, 64, 2, 5, 7, 1.0, None, ('dropped_tap', 'tap_shifted', 'padding_as_data')),
    WgradCase('odd_3x3_s2', 3, 2, 1, 64, 32, 2, 9, 7, 1.0, None, ('stride_ignored', 'padding_as_data', 'tap_shifted')),
    WgradCase('s2_1x1', 1, 2, 0, 32, 64, 2, 6, 10, 0.5, 0.125, ('stride_ignored', 'out_scale_forgotten')),
    WgradCase('slices_1x1', 1, 1, 0, 32, 32, 2, 24, 20, 1.0, None, ('slice_tail_dropped', 'co_ci_swapped')),
    WgradCase('slices_3x3', 3, 1, 1, 32, 32, 2, 24, 20, 2.0, 0.0625, ('dropped_tap', 'out_scale_forgotten', 'co_ci_swapped')),
)
# (argument, value): each must return L2I_E_UNSUPPORTED and leave every sentinel intact
WGRAD_REFUSALS = (('k', 7), ('stride', 3), ('cin', 24), ('pad', 2), ('ws', None), ('ws_bytes', 'short'))

BnCase = namedtuple('BnCase', 'name c hw b residual relu out_mask want_masked')
BN_CASES = (
    BnCase('c8_hw1', 8, (1, 1), 3, False, False, False, False),
    BnCase('c8_hw35', 8, (5, 7), 1, True, True, True, True),
    BnCase('c72_hw35', 72, (5, 7), 3, True, True, True, False),
    BnCase('c72_hw1', 72, (1, 1), 1, True, False, False, True),
    BnCase('c8_big', 8, (96, 96), 3, False, True, True, True),
    BnCase('c72_big', 72, (96, 96), 1, True, True, True, True),
)


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _d(t, rnd=None):
    t = torch.as_tensor(t).detach().cpu().float()
    return (t if rnd is None else rnd(t)).double()


def _f(v):
    return float(np.float32(v))


def bound_store(want, M, k, elem):
    """The bound of a stored element formed by k rounded fp32 operations: with the half ulp of a 16-bit store, or ('f32': the value is
    stored as computed) without it."""
    return bound_elem(M.double(), k) if elem == 'f32' else bound16(want, M, k, elem)


# ---- data -----------------------------------------------------------------------------------------------------------------------------------------
def wgrad_data(case, seed=0):
    """(x [B,Cin,H,W], gy [B,Cout,OH,OW]) float32, seeded by the case's name."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.name)))
    oh, ow = out_size(case.h, case.k, case.stride, case.pad), out_size(case.w, case.k, case.stride, case.pad)
    x = torch.randn(case.b, case.cin, case.h, case.w, generator=g)
    gy = torch.randn(case.b, case.cout, oh, ow, generator=g) * 0.5
    return x, gy


def bn_data(case, seed=0):
    """dict of float32 operands of a BatchNorm case: x, residual, gy, out (the mask: about half positive), gamma, beta."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.name)))
    shp = (case.b, case.c) + case.hw
    ch = torch.arange(case.c, dtype=torch.float32).view(1, -1, 1, 1)
    return dict(x=torch.randn(shp, generator=g) * (0.5 + 0.05 * ch) + 0.1 * ch - 1.0, residual=torch.randn(shp, generator=g),
                gy=torch.randn(shp, generator=g) * 0.25, out=torch.randn(shp, generator=g),
                gamma=torch.rand(case.c, generator=g) + 0.5, beta=torch.randn(case.c, generator=g) * 0.3)


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------------------
def _tap_view(xp, ky, kx, stride, oh, ow):
    return xp[:, :, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride]


def wgrad(x, gy, k, stride, pad, out_scale, elem, dt=torch.float64, _mistake=None, kw=None, pad_x=None, dw0=None):
    """(want, bound): dw [Cout, Cin, K, K] in ``dt`` (float64: the model; float32: the emulation the CPU test holds against the bound) and the
    bound per element.  ``out_scale`` = the product of the host and the device factor, as float32 values.

    What only the fp32 entry point allows (tests/regtrain32_ref.py): ``kw``: the kernel's width where it is not ``k`` (``k`` is then its height);
    ``pad_x``: the padding along x where it is not ``pad`` (then that along y); ``dw0`` [Cout, Cin, K, KW]: what dw holds before the call, which the
    result is added to (its magnitude joins M in the bound: the add into it is one of the roundings)."""
    assert _mistake is None or _mistake in MISTAKES, _mistake
    rnd = rnd_for(elem)
    xx, gg = _d(x, rnd).to(dt), _d(gy, rnd).to(dt)
    b, cin, h, w = xx.shape
    _, cout, oh, ow = gg.shape
    kh, kw = k, (k if kw is None else kw)
    pad_y, pad_x = pad, (pad if pad_x is None else pad_x)
    s = 1 if _mistake == 'stride_ignored' else stride
    margin = 1 + (stride * max(oh, ow) if _mistake == 'stride_ignored' else 0)          # room for the shifted / unstrided reads of the mistakes
    # (and for a gy that reaches past the padded map, as the fp32 entry point takes OH and OW as given: those pixels are padding, zeros)
    margin = max(margin, kh + stride * (oh - 1) + 1 - (h + 2 * pad_y), kw + stride * (ow - 1) + 1 - (w + 2 * pad_x))
    mode = 'replicate' if _mistake == 'padding_as_data' else 'constant'

    def padded(t):
        if mode == 'replicate' and (pad_y > 0 or pad_x > 0):
            t = torch.nn.functional.pad(t, (pad_x, pad_x, pad_y, pad_y), mode='replicate')
            return torch.nn.functional.pad(t, (0, margin, 0, margin))
        return torch.nn.functional.pad(t, (pad_x, pad_x + margin, pad_y, pad_y + margin))
    xp, xa = padded(xx), padded(xx.abs())
    if _mistake == 'slice_tail_dropped':                  # the pixels of the last, partial 256-pixel chunk contribute nothing
        keep = torch.ones(b * oh * ow, dtype=dt)
        keep[(b * oh * ow) // 256 * 256:] = 0
        gg = gg * keep.view(b, 1, oh, ow)
    sc = 1.0 if _mistake == 'out_scale_forgotten' else float(out_scale)
    want, M = torch.zeros(cout, cin, kh, kw, dtype=dt), torch.zeros(cout, cin, kh, kw, dtype=torch.float64)
    for ky in range(kh):
        for kx in range(kw):
            if _mistake == 'dropped_tap' and (ky, kx) == (kh - 1, kw - 1):
                continue
            sx = kx + 1 if (_mistake == 'tap_shifted' and (ky, kx) == (0, 0)) else kx
            want[:, :, ky, kx] = torch.einsum('bohw,bihw->oi', gg, _tap_view(xp, ky, sx, s, oh, ow))
            M[:, :, ky, kx] = torch.einsum('bohw,bihw->oi', gg.abs().double(), _tap_view(xa, ky, kx, s, oh, ow).double())
    if _mistake == 'co_ci_swapped':
        assert cin == cout
        want = want.transpose(0, 1).contiguous()
    want = want * sc
    bound = U23 * (b * oh * ow + 2) * M * abs(float(out_scale))
    if dw0 is not None:
        want = want + _d(dw0).to(dt)
        bound = U23 * (b * oh * ow + 2) * (M * abs(float(out_scale)) + _d(dw0).abs())
    return want, bound


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------------------------
def _cv(v):
    return _d(v).view(1, -1, 1, 1)


def bn_stats(x, elem):
    """((sum, sumsq), (bound, bound)) float64 [C]."""
    xx = _d(x, rnd_for(elem))
    n = xx.numel() // xx.shape[1]
    s, q = xx.sum((0, 2, 3)), (xx * xx).sum((0, 2, 3))
    k = n + 1 if elem == 'f32' else n                     # (the fp32 contract counts one more: see tests/regtrain32_ref.py)
    return (s, q), (U52 * k * xx.abs().sum((0, 2, 3)), U52 * k * q)


def bn_finalize(s, q, n, gamma, beta, eps=BN_EPS, _mistake=None):
    """(mean, invstd, scale, shift) float64 [C] from the sums: the biased variance normalises."""
    mean = s / n
    var = (q / n - mean * mean).clamp(min=0.0)
    if _mistake == 'unbiased_variance':
        var = var * (n / max(n - 1, 1))
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = _d(gamma) * invstd
    return mean, invstd, scale, _d(beta) - mean * scale


def bn_apply(x, scale, shift, residual, relu, elem, dt=torch.float64, k=3, _mistake=None):
    """(want before the one rounding of the store, bound per element); scale / shift [C] float32 (or float64 from bn_finalize)."""
    rnd = rnd_for(elem)
    xx = _d(x, rnd).to(dt)
    sc, sh = torch.as_tensor(scale).double().view(1, -1, 1, 1).to(dt), torch.as_tensor(shift).double().view(1, -1, 1, 1).to(dt)
    v = xx * sc + sh
    M = (xx.abs() * sc.abs() + sh.abs()).double()
    rr = None if residual is None else _d(residual, rnd).to(dt)
    if rr is not None:
        M = M + rr.abs().double()
        if _mistake != 'residual_after_relu':
            v = v + rr
    if relu:
        v = torch.relu(v)
    if rr is not None and _mistake == 'residual_after_relu':
        v = v + rr
    return v, bound_store(v.double(), M, k, elem)


def bn_forward(x, gamma, beta, residual, relu, elem, _mistake=None):
    """stats -> finalize -> apply in float64: (want, bound) of the stored BatchNorm output."""
    (s, q), _ = bn_stats(x, elem)
    n = x.numel() // x.shape[1]
    _, _, scale, shift = bn_finalize(s, q, n, gamma, beta, _mistake=_mistake)
    mean0, _, scale0, shift0 = bn_finalize(s, q, n, gamma, beta)
    want, _ = bn_apply(x, scale, shift, residual, relu, elem, _mistake=_mistake)
    want0, _ = bn_apply(x, scale0, shift0, residual, relu, elem)
    rnd = rnd_for(elem)
    c = lambda v: v.view(1, -1, 1, 1)
    M = (_d(x, rnd).abs() + c(mean0).abs()) * c(scale0).abs() + c(_d(beta)).abs() + (0 if residual is None else _d(residual, rnd).abs())
    return want, bound_store(want0, M, 8, elem)


def _masked(gy, out, x, rnd, dt, _mistake=None):
    gg, xx = _d(gy, rnd).to(dt), _d(x, rnd).to(dt)
    if out is None:
        return gg, xx, None
    keep = (_d(out, rnd) > 0).to(dt)
    if _mistake == 'mask_wrong_operand':                  # the mask lands on x (and through it on xhat) instead of dy
        return gg, xx * keep, keep
    return gg * keep, xx, keep


def bn_bwd_reduce(gy, out, x, mean, invstd, elem, dt=torch.float64, _mistake=None):
    """((sum_dy, sum_dyxh), (bound, bound)) [C]; mean / invstd [C] float32."""
    rnd = rnd_for(elem)
    dy, xx, _ = _masked(gy, out, x, rnd, dt, _mistake)
    mu, isd = _cv(mean).to(dt), _cv(invstd).to(dt)
    xh = (xx - mu) * isd
    n = xx.numel() // xx.shape[1]
    s, q = dy.double().sum((0, 2, 3)), (dy.double() * xh.double()).sum((0, 2, 3))
    Ms = dy.abs().double().sum((0, 2, 3))
    Mq = (dy.abs() * (xx.abs() + mu.abs()) * isd.abs()).double().sum((0, 2, 3))
    return (s, q), (U52 * n * Ms, (2 * U23 + U52 * n) * Mq)


def bn_bwd_apply(gy, out, x, mean, invstd, gamma, m_dy, m_dyxh, elem, dt=torch.float64, _mistake=None):
    """(dx before the store, bound, masked dy exactly as stored)."""
    rnd = rnd_for(elem)
    dy, xx, _ = _masked(gy, out, x, rnd, dt, _mistake)
    mu, isd, ga, md, mx = (_cv(v).to(dt) for v in (mean, invstd, gamma, m_dy, m_dyxh))
    xh = (xx - mu) * isd
    gi = ga * isd
    v = gi * (dy - md - xh * mx)
    M = (gi.abs() * (dy.abs() + md.abs() + (xx.abs() + mu.abs()) * isd.abs() * mx.abs())).double()
    return v, bound_store(v.double(), M, 7, elem), dy
