"""The fused prologue / epilogue contract of include/l2i.h (struct l2i_conv_params), written once in float64, and the case table that drives
tests/test_epilogue_contract_gpu.py (checked on the CPU by tests/test_epilogue_ref_cpu.py).

    pro(x) = x * in_scale[b,ci] * (in_mask ? (in_mask > 0 ? mask_pos : mask_neg) : 1)
    epi(a) = act( a*out_scale[b,co] * (out_mask > 0) + noise*noise_w + bias[co] + R * (res_mask > 0) ) * out_gain  (+ y if accumulate)
    R      = res_sub ? res_coef * res_coef_dev[0] * (residual - res_sub) : residual

A plain module: no fixtures, no GPU, no kernel code."""
import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2          # include/l2i.h: L2I_ACT_*
SQRT2 = 2 ** 0.5
SENTINEL = -7777.25          # what y holds before a launch that does not accumulate: exactly representable, far from every result

# term-order mistakes `conv_epi_ref(_mistake=...)` can make on purpose (the CPU test proves that the case aimed at each one sees it)
MISTAKES = ('mask_ge', 'out_mask_after_add', 'one_mask_for_both', 'res_mask_gates_conv', 'coef_dropped', 'coef_squared', 'coef_null_is_zero',
            'accumulate_times_out_gain', 'accumulate_times_act_gain', 'accumulate_before_act', 'act_before_residual')


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def window(y_shape, step=1, off=(0, 0)):
    """Boolean map [OHf, OWf] of the pixels a launch with (oy_step, ox_step) = step and (oy_off, ox_off) = off writes."""
    m = torch.zeros(y_shape[-2], y_shape[-1], dtype=torch.bool)
    m[off[0]::step, off[1]::step] = True
    return m


def conv_epi_ref(x, w_oihw, stride, pad, *, transposed=False, step=1, off=(0, 0), y_prev=None, in_scale=None, in_mask=None, mask=(1.0, 0.0),
                 out_scale=None, noise=None, noise_w=0.0, bias=None, residual=None, res_mask=None, out_mask=None, res_sub=None, res_coef=1.0,
                 res_coef_dev=None, act=ACT_NONE, slope=0.2, gain=1.0, out_gain=1.0, accumulate=False, _mistake=None):
    """float64 result [B, Cout, OHf, OWf] of one conv launch.  ``w_oihw`` [Cout, Cin, KH, KW] is in correlation form; ``pad`` an int or
    (pad_y, pad_x); ``transposed``: y[co, 2i+k-pad] += x[ci, i] w[co, ci, k] (stride 2, every output index inside ``y_prev``: F.conv_transpose2d's
    size or up to 8 more, i.e. output_padding; rows / columns no input reaches carry a zero conv term).  The launch writes every
    ``step``-th pixel of ``y_prev``'s shape from ``off``; every other pixel is returned equal to ``y_prev``.  Without ``y_prev`` the output has the correlation's own size (dense launches only).  Maps shaped like
    the output (noise, residual, masks, res_sub) are full-size and read at the written pixels."""
    assert _mistake is None or _mistake in MISTAKES, _mistake
    pos = (lambda m: m >= 0) if _mistake == 'mask_ge' else (lambda m: m > 0)
    xx = _d(x)
    if in_scale is not None:
        xx = xx * _d(in_scale)[:, :, None, None]
    if in_mask is not None:
        xx = xx * torch.where(pos(_d(in_mask)), torch.tensor(float(mask[0]), dtype=torch.float64), torch.tensor(float(mask[1]), dtype=torch.float64))
    pad = (pad, pad) if isinstance(pad, int) else tuple(pad)
    if transposed:                                       # every in-range y[2i+k-pad]: the unpadded form, cut at pad (F.conv_transpose2d's own padding
        a = F.conv_transpose2d(xx, _d(w_oihw).transpose(0, 1), stride=2)[:, :, pad[0]:, pad[1]:]      # also drops the last `pad` rows an input reaches)
    else:
        a = F.conv2d(xx, _d(w_oihw), stride=stride, padding=pad)
    B, cout = a.shape[:2]
    if y_prev is None:
        assert step == 1 and tuple(off) == (0, 0) and not accumulate
        y_prev = torch.zeros_like(a)
    out = _d(y_prev).clone()
    assert out.shape[:2] == (B, cout), (out.shape, a.shape)
    win = lambda t: _d(t)[:, :, off[0]::step, off[1]::step]
    OH, OW = win(out).shape[2:]
    if transposed:                                       # F.conv_transpose2d's size, or up to 8 rows / columns more: zeros where no input reaches
        assert 0 <= OH - (a.shape[2] - pad[0]) <= 8 and 0 <= OW - (a.shape[3] - pad[1]) <= 8 and step == 1
        a = F.pad(a, (0, max(0, OW - a.shape[3]), 0, max(0, OH - a.shape[2])))
    assert a.shape[2] >= OH and a.shape[3] >= OW, (a.shape, OH, OW)
    v = a[:, :, :OH, :OW]
    if out_scale is not None:
        v = v * _d(out_scale)[:, :, None, None]
    if res_mask is not None and _mistake == 'res_mask_gates_conv':
        v = v * pos(win(res_mask))
    if out_mask is not None and _mistake != 'out_mask_after_add':
        v = v * pos(win(out_mask))
    if noise is not None:
        v = v + win(noise) * noise_w
    if bias is not None:
        v = v + _d(bias)[None, :, None, None]
    if out_mask is not None and _mistake == 'out_mask_after_add':
        v = v * pos(win(out_mask))
    r = None
    if residual is not None:
        r = win(residual)
        if res_sub is not None:
            dev = (0.0 if _mistake == 'coef_null_is_zero' else 1.0) if res_coef_dev is None else float(_d(res_coef_dev).reshape(-1)[0])
            coef = 1.0 if _mistake == 'coef_dropped' else res_coef * dev
            r = (coef * coef if _mistake == 'coef_squared' else coef) * (r - win(res_sub))
        rm = out_mask if (_mistake == 'one_mask_for_both' and out_mask is not None) else res_mask
        if rm is not None:
            r = r * pos(win(rm))
    else:
        assert res_sub is None and res_mask is None
    prev = win(out)
    if r is not None and _mistake != 'act_before_residual':
        v = v + r
    if accumulate and _mistake == 'accumulate_before_act':
        v = v + prev
    if act == ACT_LRELU:
        v = torch.where(v > 0, v, v * slope) * gain
    elif act == ACT_RELU:
        v = torch.relu(v)
    if r is not None and _mistake == 'act_before_residual':
        v = v + r
    if accumulate and _mistake == 'accumulate_times_out_gain':
        v = v + prev
    v = v * out_gain
    if accumulate and _mistake == 'accumulate_times_act_gain':
        v = v + prev * gain
    elif accumulate and _mistake not in ('accumulate_before_act', 'accumulate_times_out_gain'):
        v = v + prev
    out[:, :, off[0]::step, off[1]::step] = v
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------
# A case = the set of contract fields it sets (+ modifiers) and the mistakes it exists to catch.  Fields: in_scale, in_mask (leaky slopes
# (sqrt 2, 0.2 sqrt 2)), relu_in (in_mask IS x, slopes (1, 0)), out_scale, out_mask, noise (noise_w 0.3), bias, residual, res_mask, res_sub
# (res_coef 0.25, res_coef_dev [2.0]), lrelu (slope 0.2, gain sqrt 2), relu, out_gain (0.5), accumulate, sq (sq_ref / sq_out).
# Modifiers: coef_null (res_coef_dev = NULL), big_prev (y_prev ~ 100), neg_residual (residual ~ N(-2, 1)).
# (out_gain applied BEFORE a (leaky) ReLU is the same function for a positive gain — both are positively homogeneous — so no case aims at it.)
FIELDS = ('in_scale', 'in_mask', 'relu_in', 'out_scale', 'out_mask', 'noise', 'bias', 'residual', 'res_mask', 'res_sub', 'lrelu', 'relu', 'out_gain',
          'accumulate', 'sq')
MODIFIERS = ('coef_null', 'big_prev', 'neg_residual')
SINGLE_CASES = {          # each term alone on a bare conv
    'bare': ((), ()),
    'in_scale': (('in_scale',), ()),
    'in_mask': (('in_mask',), ('mask_ge',)),
    'relu_in': (('relu_in',), ()),
    'out_scale': (('out_scale',), ()),
    'out_mask': (('out_mask',), ('mask_ge',)),
    'noise': (('noise',), ()),
    'bias': (('bias',), ()),
    'residual': (('residual',), ()),
    'lrelu': (('lrelu',), ()),
    'relu': (('relu',), ()),
    'out_gain': (('out_gain',), ()),
    'accumulate': (('accumulate',), ()),
}
COMBO_CASES = {           # order-discriminating combinations: fields, the mistakes each must be able to see
    'mask_noise_bias': (('out_mask', 'noise', 'bias'), ('out_mask_after_add', 'mask_ge')),
    'two_masks': (('out_scale', 'out_mask', 'residual', 'res_mask'), ('one_mask_for_both', 'res_mask_gates_conv', 'mask_ge')),
    'res_sub_coef': (('residual', 'res_sub', 'res_mask'), ('coef_dropped', 'coef_squared', 'mask_ge')),
    'res_sub_coef_null': (('residual', 'res_sub', 'res_mask', 'coef_null'), ('coef_null_is_zero', 'coef_squared', 'mask_ge')),
    'gain_acc': (('out_gain', 'accumulate', 'big_prev'), ('accumulate_times_out_gain',)),          # (the kernels without an activation too)
    'lrelu_gain_acc': (('lrelu', 'out_gain', 'accumulate', 'big_prev'), ('accumulate_times_out_gain', 'accumulate_times_act_gain', 'accumulate_before_act')),
    'relu_neg_residual': (('relu', 'residual', 'neg_residual'), ('act_before_residual',)),
}
CASES = dict(SINGLE_CASES, **COMBO_CASES)


def everything(accepts):
    """The 'everything the route accepts at once' case: every accepted field, one prologue mask and one activation."""
    f = [k for k in FIELDS if k in accepts]
    if 'in_mask' in f and 'relu_in' in f:
        f.remove('relu_in')
    if 'lrelu' in f and 'relu' in f:
        f.remove('relu')
    if 'residual' not in f:
        f = [k for k in f if k not in ('res_mask', 'res_sub')]
    return tuple(f)


def case_fields(name, accepts=None):
    return everything(accepts) if name == 'everything' else CASES[name][0]


def runs_on(fields, accepts):
    return all(k in accepts or k in MODIFIERS for k in fields)


def masks_like(rs, shape):
    """Mask values from {-1, -0.0, +0.0, +1}: a third exact zeros of either sign (the contract is > 0: both zeros take the negative branch)."""
    return torch.from_numpy(rs.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32), size=shape, p=[1 / 3, 1 / 6, 1 / 6, 1 / 3]))


def make_inputs(seed, fields, x_shape, cout, y_shape):
    """The operands of a case as float32 CPU tensors / Python scalars, keyed by conv_epi_ref's (and run_launch's) keyword names, plus
    'y_prev' (what the output holds before the launch: the sentinel unless the case accumulates) and 'sq_ref' for the sq field."""
    rs = np.random.RandomState(seed)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    B, cin = x_shape[:2]
    kw = {}
    x = T(rs.randn(*x_shape))
    like_y = lambda: T(rs.randn(*y_shape))
    if 'in_scale' in fields:
        kw['in_scale'] = T(rs.rand(B, cin) + 0.5)
    if 'in_mask' in fields:
        kw['in_mask'], kw['mask'] = masks_like(rs, x_shape), (SQRT2, 0.2 * SQRT2)
    if 'relu_in' in fields:
        kw['in_mask'], kw['mask'] = x, (1.0, 0.0)
    if 'out_scale' in fields:
        kw['out_scale'] = T(rs.rand(B, cout) + 0.5)
    if 'out_mask' in fields:
        kw['out_mask'] = masks_like(rs, y_shape)
    if 'noise' in fields:
        kw['noise'], kw['noise_w'] = T(rs.randn(B, 1, *y_shape[2:])), 0.3
    if 'bias' in fields:
        kw['bias'] = T(rs.randn(cout))
    if 'residual' in fields:
        kw['residual'] = like_y() - 2.0 if 'neg_residual' in fields else like_y()
    if 'res_mask' in fields:
        kw['res_mask'] = masks_like(rs, y_shape)
    if 'res_sub' in fields:
        kw['res_sub'], kw['res_coef'] = like_y(), 0.25
        kw['res_coef_dev'] = None if 'coef_null' in fields else torch.full((1,), 2.0)
    if 'lrelu' in fields:
        kw['act'], kw['slope'], kw['gain'] = ACT_LRELU, 0.2, SQRT2
    if 'relu' in fields:
        kw['act'] = ACT_RELU
    if 'out_gain' in fields:
        kw['out_gain'] = 0.5
    if 'accumulate' in fields:
        kw['accumulate'] = True
        y_prev = like_y() * (100.0 if 'big_prev' in fields else 1.0)
    else:
        y_prev = torch.full(y_shape, SENTINEL)
    sq_ref = like_y() if 'sq' in fields else None
    return x, kw, y_prev, sq_ref



def rel_err(got, ref):
    """max|got - ref| / max|ref|: the measure every conv kernel test of the suite bounds."""
    return float((_d(got) - ref).abs().max() / ref.abs().max())
