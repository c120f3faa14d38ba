"""The contract of the fp32 training kernels (csrc/l2i_train.hip; include/l2i.h: l2i_conv2d_wgrad_f32, l2i_bn_stats_f32, l2i_bn_apply_f32,
l2i_bn_bwd_reduce_f32, l2i_bn_bwd_apply_f32): the float64 models of tests/regtrain16_ref.py evaluated with elem = 'f32' (the operands are
the float32 values as they are, nothing is rounded on the way in and the stores keep what was computed), with bounds derived for fp32, and the
case tables that drive tests/test_regtrain32_kernels_gpu.py (checked on the CPU by tests/test_regtrain32_ref_cpu.py).

Model.  As in tests/regtrain16_ref.py, plus what only the fp32 entry points allow:

    wgrad       dw[co,ci,ky,kx] = dw0[co,ci,ky,kx] + sum_{b,oy,ox} gy[b,co,oy,ox] * x[b,ci,oy*s+ky-pad_y,ox*s+kx-pad_x]; KH and KW are separate,
                and so are pad_y and pad_x; dw0 is what dw held before the call ("must be zeroed (or hold the value to accumulate into)").
    stats       sum[c] = sum0[c] + sum x, sumsq[c] = sumsq0[c] + sum x^2     ("caller zeroes": the kernels add into what they find)
    bwd_reduce  sum_dy[c] = s0[c] + sum dy, sum_dyxh[c] = q0[c] + sum dy xhat
    apply, bwd_apply, forward: unchanged.

Bounds, u = 2^-23 (twice the unit roundoff of fp32: the matrix pipe's additions are not promised to round to nearest).  Nothing here is
measured on a kernel.
    wgrad       unlike a product of two 16-bit values, a product of two fp32 values is not exact in fp32: each of the N = B OH OW terms carries
                one rounding of its product (or none, where the pipe fuses it into the sum), relative to that term.  The terms are then added in
                some order (lanes, the two K steps of an MFMA, waves, row groups, the atomics) and at last into dw0: N additions, each relative
                to a partial sum that is at most M + |dw0|, M = sum |gy| |x|.  To first order that is u M for all the products together
                + N u (M + |dw0|) for the additions: bound = u (N + 2) (M + |dw0|), the + 2 = the products' share and one for the second order.
    stats       the kernel widens every fp32 value to float64 (exact) and squares it in float64.  A 24-bit significand squared has at most 48
                bits, which float64 (53) holds: the square is exact, like that of a 16-bit value; it does not round at all.  What rounds are the
                float64 additions: N - 1 among the N terms of a channel in whatever order (thread, wave, block, atomics) and 1 into the value
                the sum held before: N roundings, each at most 2^-53 of a partial sum <= M.  The contract states 2^-52 (N + 1) M
                (M = sum |x| + |sum0|, resp. sum x^2 + |sumsq0|): the count arrived at is N, the bound keeps one in hand and a factor two per
                rounding.
    apply       bound_elem(M, 3): multiply, add, residual add; M = |x| |scale| + |shift| + |residual|.  (ReLU is a select.)
    bwd_reduce  as the 16-bit model: xhat costs two fp32 roundings relative to (|x| + |mean|) |invstd|, products of two fp32 values are exact
                in float64, sums are float64: (2 u + 2^-52 N) M for sum_dyxh, 2^-52 N sum |dy| for sum_dy; a sum that starts from a non-zero
                value takes that value's magnitude into its M.
    bwd_apply   bound_elem(M, 7) with the 16-bit model's M; the masked dy is a select: exact.
    forward     (through regressor_train._BN.forward, whose finalize is a handful of torch expressions) bound_elem(M, 8), as the 16-bit model.
    backward    (through _BN.backward) the wrapper forms m_dy and m_dyxh from the KERNEL's sums, which may differ from the model's in their
                last float64 bits and so, rarely, in the last bit of their float32 values: one ulp = u of |m_dy| resp. |m_dyxh|, each of
                which M already holds: k = 7 + 2 = 9.

MISTAKES are seeded errors; the case tables name the ones each case must expose.  The mistakes of the 16-bit table that apply are passed
through to its model; the ones below are made here, on the operands (a mask on gy is a set of terms that were never added).
The *_geom functions restate the host side of the launches, so that the CPU test can prove that a case reaches the path it is named for.
A plain module: no fixtures, no kernel code."""
from collections import namedtuple

import torch

from tests import regtrain16_ref as rr
from tests.regtrain16_ref import SENTINEL, U52, _d, out_size      # noqa: F401 (re-exported)
from tests.stream_ref import U23, cdiv, plant_signs, worst       # noqa: F401 (re-exported)

ELEM = 'f32'
WGRAD_MISTAKES = ('dropped_tap', 'tap_shifted', 'padding_as_data', 'co_ci_swapped', 'stride_ignored',          # the 16-bit table's, as they are
                  'second_trip_dropped', 'odd_ow_tail_dropped', 'kernel_row_dropped', 'overwrites_dw', 'pad_xy_swapped')
BN_MISTAKES = ('mask_wrong_operand', 'unbiased_variance', 'residual_after_relu', 'chunk_tail_dropped', 'mask_ge_zero', 'sums_overwritten')
_RR_WGRAD = WGRAD_MISTAKES[:5]

WgradCase = namedtuple('WgradCase', 'name kh kw stride pad_y pad_x cin cout b h w dw0 mistakes')


def _sq(c, name=None, dw0=False, mistakes=None):
    """A square case of the 16-bit table, under the fp32 table's fields."""
    return WgradCase(name or c.name, c.k, c.k, c.stride, c.pad, c.pad, c.cin, c.cout, c.b, c.h, c.w, dw0, mistakes)


_R16 = {c.name: c for c in rr.WGRAD_CASES}
WGRAD_CASES = (
    WgradCase('one_pixel', 1, 1, 1, 0, 0, 32, 32, 1, 1, 1, False, ('co_ci_swapped',)),                               # three idle waves
    # odd OW (in the last MFMA step the upper lane half sits at ox == OW), both channel tails, one row per wave and no more
    WgradCase('ragged_3x3', 3, 3, 1, 1, 1, 40, 72, 1, 4, 5, False, ('odd_ow_tail_dropped', 'dropped_tap', 'tap_shifted')),
    WgradCase('ragged_3rows', 3, 3, 1, 1, 1, 40, 72, 1, 3, 5, False, ('odd_ow_tail_dropped', 'padding_as_data')),     # the same with an idle wave
    _sq(_R16['border_3x3'], mistakes=('dropped_tap', 'tap_shifted', 'padding_as_data', 'kernel_row_dropped')),
    _sq(_R16['odd_3x3_s2'], mistakes=('stride_ignored', 'padding_as_data', 'tap_shifted')),
    _sq(_R16['s2_1x1'], mistakes=('stride_ignored',)),
    WgradCase('stem', 7, 7, 2, 3, 3, 3, 40, 2, 13, 11, False, ('stride_ignored', 'kernel_row_dropped', 'padding_as_data', 'dropped_tap')),
    # 64 tiles, 64 row groups, 260 rows: 256 in the first trip of the row loop, 4 in the second (waves with and without a second row)
    WgradCase('row_loop', 1, 1, 1, 0, 0, 256, 256, 1, 260, 2, False, ('second_trip_dropped', 'co_ci_swapped')),
    _sq(_R16['slices_3x3'], name='row_groups_meet', mistakes=('dropped_tap', 'co_ci_swapped')),                      # 12 groups add into one dw
    _sq(_R16['border_3x3'], name='accumulate', dw0=True, mistakes=('overwrites_dw', 'kernel_row_dropped')),
    WgradCase('rect_1x3', 1, 3, 1, 0, 1, 32, 64, 2, 5, 7, False, ('pad_xy_swapped', 'tap_shifted')),
    WgradCase('rect_3x1', 3, 1, 1, 1, 0, 32, 64, 2, 5, 7, False, ('pad_xy_swapped', 'kernel_row_dropped')),
)

BnCase = namedtuple('BnCase', 'name c hw b residual relu out_mask want_masked preload mistakes')
_BN_MISTAKES_OF = {
    'c8_hw1': (),
    'c8_hw35': ('mask_wrong_operand', 'mask_ge_zero', 'residual_after_relu'),
    'c72_hw35': ('mask_wrong_operand', 'unbiased_variance', 'residual_after_relu', 'mask_ge_zero'),
    'c72_hw1': (),
    'c8_big': ('chunk_tail_dropped', 'mask_ge_zero'),
    'c72_big': ('chunk_tail_dropped', 'mask_wrong_operand'),
}
BN_CASES = tuple(BnCase(*c, False, _BN_MISTAKES_OF[c.name]) for c in rr.BN_CASES) + (
    # 294912 values per channel: 72 chunks of 4096, capped at 64 blocks, 18 whole trips each; 884736 elements: the second grid-stride trip.
    # residual / relu / out_mask / masked dy as bn1 and bn2 of a block and the stem have them
    BnCase('cap', 3, (384, 384), 2, False, True, True, False, False, ('mask_ge_zero',)),
    # 270400 values per channel: the cap again, and 16 whole trips + one that only the first 8256 threads of the 16384 take
    BnCase('cap_tail', 2, (520, 520), 1, False, True, True, False, False, ('chunk_tail_dropped',)),
    BnCase('preloaded', 24, (9, 7), 4, True, True, True, True, True, ('sums_overwritten', 'mask_wrong_operand')),
)
# (residual, relu) of the forward and (out_mask, masked dy) of the backward as regressor_train.TrainableResNet50 calls them: bn1 / bn2 / the
# stem, a downsample BatchNorm, bn3; and relu = 0 with a residual, which the entry point takes and no layer uses
TRAINER_COMBOS = ((False, True, True, False), (False, False, False, False), (True, True, True, True))
EXTRA_COMBOS = ((True, False),)          # (residual, relu)


# ---- launch geometry, restated from the entry points ----------------------------------------------------------------------------------------------
def wgrad_geom(case):
    """l2i_conv2d_wgrad_f32: a block is 4 waves; wave w of row group g walks the rows r = g * 4 + w + k * 4 * row_groups."""
    oh = out_size(case.h, case.kh, case.stride, case.pad_y)
    rows = case.b * oh
    tiles = cdiv(case.cout, 32) * cdiv(case.cin, 32)
    groups = max(min(cdiv(4096, tiles), cdiv(rows, 4), 65535), 1)
    per_trip = 4 * groups
    return dict(rows=rows, tiles=tiles, row_groups=groups, per_trip=per_trip, trips=cdiv(rows, per_trip), last_trip_rows=rows - (cdiv(rows, per_trip) - 1) * per_trip,
                idle_waves=max(per_trip - rows, 0), launches=case.kh)


def bn_reduce_geom(n):
    """l2i_bn_stats_f32 / l2i_bn_bwd_reduce_f32 on n = B * HW values per channel: grid (C, chunks), 256 threads, stride chunks * 256."""
    free = cdiv(n, 4096)
    chunks = min(free, 64)
    return dict(chunks=chunks, capped=free > 64, trips=cdiv(n, chunks * 256), tail=n % (chunks * 256))


def bn_elem_geom(n):
    """l2i_bn_apply_f32 / l2i_bn_bwd_apply_f32 on n = B * C * HW elements: l2i_grid_for(n, 256), at most 2048 blocks of 256."""
    grid = max(min(cdiv(n, 256), 2048), 1)
    return dict(grid=grid, trips=cdiv(n, grid * 256))


# ---- data -----------------------------------------------------------------------------------------------------------------------------------------
def wgrad_data(case, seed=0):
    """(x [B,Cin,H,W], gy [B,Cout,OH,OW], dw0 [Cout,Cin,KH,KW] or None) float32, seeded by the case's name."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.name)))
    oh, ow = out_size(case.h, case.kh, case.stride, case.pad_y), out_size(case.w, case.kw, case.stride, case.pad_x)
    x = torch.randn(case.b, case.cin, case.h, case.w, generator=g)
    gy = torch.randn(case.b, case.cout, oh, ow, generator=g) * 0.5
    dw0 = torch.randn(case.cout, case.cin, case.kh, case.kw, generator=g) * 3.0 if case.dw0 else None
    return x, gy, dw0


def bn_data(case, seed=0):
    """rr.bn_data with the mask operand a ReLU leaves: relu(randn), about half of it exact zeros, and a few -0.0 / +-tiny planted at both
    ends; for a preloaded case also the four sums' starting values s0, q0 (forward) and sd0, sq0 (backward), float64 [C]."""
    d = rr.bn_data(case, seed)
    d['out'] = plant_signs(torch.relu(d['out']))
    if case.preload:
        g = torch.Generator().manual_seed(seed + 1 + sum(map(ord, case.name)))
        for name, mag in (('s0', 50.0), ('q0', 200.0), ('sd0', 5.0), ('sq0', 5.0)):
            d[name] = torch.randn(case.c, generator=g, dtype=torch.float64) * mag
    return d


# ---- the model --------------------------------------------------------------------------------------------------------------------------------------
def wgrad(case, x, gy, dw0=None, dt=torch.float64, _mistake=None):
    """(want, bound) of a weight-gradient case: rr.wgrad with elem = 'f32' and out_scale 1."""
    assert _mistake is None or _mistake in WGRAD_MISTAKES, _mistake
    kh, kw, pad_y, pad_x = case.kh, case.kw, case.pad_y, case.pad_x
    gy = torch.as_tensor(gy).detach().cpu().float()
    oh, ow = gy.shape[2:]
    if _mistake == 'second_trip_dropped':                  # rows beyond the first 4 * row_groups contribute nothing
        keep = (torch.arange(case.b * oh) < wgrad_geom(case)['per_trip']).float().view(case.b, 1, oh, 1)
        gy = gy * keep
    if _mistake == 'odd_ow_tail_dropped' and ow % 2:       # the last pixel of an odd row is lost
        gy = gy.clone()
        gy[..., ow - 1] = 0
    if _mistake == 'pad_xy_swapped':
        pad_y, pad_x = pad_x, pad_y
    if _mistake == 'overwrites_dw':                        # a store instead of an add
        dw0 = None
    want, bound = rr.wgrad(x, gy, kh, case.stride, pad_y, 1.0, ELEM, dt=dt, _mistake=_mistake if _mistake in _RR_WGRAD else None, kw=kw, pad_x=pad_x,
                           dw0=dw0)
    if _mistake == 'kernel_row_dropped':                   # the launch of the last kernel row is missing: dw keeps what it held there
        want[:, :, kh - 1] = 0 if dw0 is None else _d(dw0).to(dt)[:, :, kh - 1]
    return want, bound


def _chunk_keep(t):
    """1 on the values of each channel that lie in a whole 4096-chunk of its (sample, pixel) index, 0 on the ones beyond the last."""
    b, c, h, w = t.shape
    n = b * h * w
    keep = (torch.arange(n) < n // 4096 * 4096).float().view(b, 1, h, w)
    return keep.expand(b, c, h, w)


def bn_stats(x, s0=None, q0=None, _mistake=None):
    """((sum, sumsq), (bound, bound)) float64 [C], added to what the sums held (s0, q0; None = zeros)."""
    assert _mistake in (None, 'chunk_tail_dropped', 'sums_overwritten')
    xx = torch.as_tensor(x).detach().cpu().float()
    if _mistake == 'chunk_tail_dropped':
        xx = xx * _chunk_keep(xx)
    (s, q), (bs, bq) = rr.bn_stats(xx, ELEM)
    n = xx.numel() // xx.shape[1]
    if s0 is not None:
        bs, bq = bs + U52 * (n + 1) * s0.abs(), bq + U52 * (n + 1) * q0.abs()
        if _mistake != 'sums_overwritten':
            s, q = s + s0, q + q0
    return (s, q), (bs, bq)


def _out_for(out, _mistake):
    if out is not None and _mistake == 'mask_ge_zero':     # `out >= 0` keeps the zeros of either sign
        o = torch.as_tensor(out).detach().cpu().float()
        return torch.where(o >= 0, torch.ones_like(o), -torch.ones_like(o))
    return out


def _rr_mistake(_mistake):
    return _mistake if _mistake in rr.MISTAKES else None


def bn_apply(x, scale, shift, residual, relu, dt=torch.float64, _mistake=None):
    return rr.bn_apply(x, scale, shift, residual, relu, ELEM, dt=dt, _mistake=_rr_mistake(_mistake))


def bn_forward(x, gamma, beta, residual, relu, _mistake=None):
    return rr.bn_forward(x, gamma, beta, residual, relu, ELEM, _mistake=_rr_mistake(_mistake))


def bn_bwd_reduce(gy, out, x, mean, invstd, sd0=None, sq0=None, dt=torch.float64, _mistake=None):
    """((sum_dy, sum_dyxh), (bound, bound)) float64 [C], added to what the sums held (sd0, sq0; None = zeros)."""
    gg = torch.as_tensor(gy).detach().cpu().float()
    if _mistake == 'chunk_tail_dropped':
        gg = gg * _chunk_keep(gg)
    (s, q), (bs, bq) = rr.bn_bwd_reduce(gg, _out_for(out, _mistake), x, mean, invstd, ELEM, dt=dt, _mistake=_rr_mistake(_mistake))
    n = gg.numel() // gg.shape[1]
    if sd0 is not None:
        bs, bq = bs + U52 * n * sd0.abs(), bq + (2 * U23 + U52 * n) * sq0.abs()
        if _mistake != 'sums_overwritten':
            s, q = s + sd0, q + sq0
    return (s, q), (bs, bq)


def bn_bwd_apply(gy, out, x, mean, invstd, gamma, m_dy, m_dyxh, dt=torch.float64, _mistake=None):
    """(dx, bound, masked dy exactly as stored)."""
    return rr.bn_bwd_apply(gy, _out_for(out, _mistake), x, mean, invstd, gamma, m_dy, m_dyxh, ELEM, dt=dt, _mistake=_rr_mistake(_mistake))


def masked_dy(gy, out):
    """The masked dy bit for bit, float32: gy where out > 0, +0.0 elsewhere (a product with a 0 / 1 mask, as the model above forms it, has the
    same VALUES and the sign of gy on its zeros); gy itself where there is no mask."""
    gy = torch.as_tensor(gy).detach().cpu().float()
    return gy.clone() if out is None else torch.where(torch.as_tensor(out).detach().cpu().float() > 0, gy, torch.zeros_like(gy))


K_BWD_APPLY, K_BWD_WRAPPER = 7, 9         # see "backward" above: the wrapper pass is held to bound * K_BWD_WRAPPER / K_BWD_APPLY


def bn_model(case):
    """Everything a BatchNorm case is held to, computed once: the data, the float32 [C] vectors the kernels are given (from the float64
    statistics) and (want, bound) per kernel."""
    d = bn_data(case)
    n = case.b * case.hw[0] * case.hw[1]
    (s, q), _ = rr.bn_stats(d['x'], ELEM)                                              # the statistics of x alone: what finalize is fed
    mean, invstd, scale, shift = (t.float() for t in rr.bn_finalize(s, q, n, d['gamma'], d['beta']))
    res = d['residual'] if case.residual else None
    out = d['out'] if case.out_mask else None
    (sd, sq), _ = rr.bn_bwd_reduce(d['gy'], out, d['x'], mean, invstd, ELEM)
    m_dy, m_dyxh = (sd / n).float(), (sq / n).float()
    return dict(d=d, n=n, small=(mean, invstd, scale, shift), res=res, out=out, means=(m_dy, m_dyxh),
                stats=bn_stats(d['x'], d.get('s0'), d.get('q0')), apply=bn_apply(d['x'], scale, shift, res, case.relu),
                forward=bn_forward(d['x'], d['gamma'], d['beta'], res, case.relu),
                reduce=bn_bwd_reduce(d['gy'], out, d['x'], mean, invstd, d.get('sd0'), d.get('sq0')),
                bwd=bn_bwd_apply(d['gy'], out, d['x'], mean, invstd, d['gamma'], m_dy, m_dyxh))
