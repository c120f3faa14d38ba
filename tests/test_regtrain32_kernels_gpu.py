"""The fp32 training kernels (csrc/l2i_train.hip: l2i_conv2d_wgrad_f32, l2i_bn_stats_f32, l2i_bn_apply_f32, l2i_bn_bwd_reduce_f32,
l2i_bn_bwd_apply_f32) against the float64 models and derived bounds of tests/regtrain32_ref.py.  The kernels are called through the raw
entry points (the only way to a rectangular kernel, a dw and sums that start non-zero), every output carved out of a sentinel-filled buffer
whose guards must survive; the square cases run once more through regressor_train.conv_wgrad, _BN.forward and _BN.backward, which holds the
wrappers' argument order.  The elementwise kernels are launched twice with bit-equal results; the three kernels whose partial sums meet in
atomics promise no order and are held to their bounds only.  Every test prints `rt32 <kernel> <case> error bound ratio`."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from latent2im_amd import regressor_train as RT
from tests import regtrain32_ref as r32

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                  # sentinel elements on either side of a carved tensor
WGRAD = {c.name: c for c in r32.WGRAD_CASES}
BN = {c.name: c for c in r32.BN_CASES}
_BN_MODEL = {}                # case -> the float64 model of the case, once
E_ARG, E_UNSUPPORTED = -1, -3


def carve(shape, dtype=torch.float32, init=None):
    """(buffer, view): ``view`` of ``shape`` inside a sentinel-filled buffer, itself holding the sentinel or ``init``."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), r32.SENTINEL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 16 == 0
    if isinstance(init, float):
        view.fill_(init)
    elif init is not None:
        view.copy_(init.to(dtype))
    return buf, view


def guards_intact(buf, what):
    fill = torch.full((GUARD,), r32.SENTINEL, dtype=buf.dtype, device=DEV)
    assert torch.equal(buf[:GUARD], fill) and torch.equal(buf[-GUARD:], fill), 'the launch wrote outside ' + what


def bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def bn_model(name):
    if name not in _BN_MODEL:
        _BN_MODEL[name] = r32.bn_model(BN[name])
    return _BN_MODEL[name]


def report(kernel, case, got, want, bound):
    err, b, ratio = r32.worst(got, want, bound)
    print('rt32 %s %s error %.3g bound %.3g ratio %.3g' % (kernel, case, err, b, ratio))
    return ratio


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(WGRAD))
def test_wgrad(name):
    case = WGRAD[name]
    x, gy, dw0 = r32.wgrad_data(case)
    want, bound = r32.wgrad(case, x, gy, dw0)
    xg, gg = x.to(DEV), gy.to(DEV)
    oh, ow = gy.shape[2:]
    obuf, dw = carve((case.cout, case.cin, case.kh, case.kw), init=0.0 if dw0 is None else dw0)
    _lib.call('l2i_conv2d_wgrad_f32', _lib.fptr(dw), _lib.fptr(xg), _lib.fptr(gg), case.b, case.cin, case.h, case.w, case.cout, oh, ow, case.kh, case.kw,
              case.stride, case.pad_y, case.pad_x)
    torch.cuda.synchronize()
    guards_intact(obuf, 'dw')
    assert report('wgrad', name, dw, want, bound) <= 1.0
    if case.kh == case.kw and case.pad_y == case.pad_x and dw0 is None:          # the wrapper: a square kernel into a zeroed dw of its own
        got = RT.conv_wgrad(xg, gg, case.kh, case.stride, case.pad_y)
        assert tuple(got.shape) == tuple(want.shape)
        assert report('wgrad(wrapper)', name, got, want, bound) <= 1.0


def _wgrad_refusal(expect, part, **change):
    a = dict(b=1, cin=32, h=5, w=7, cout=32, oh=5, ow=7, kh=3, kw=3, stride=1, pad_y=1, pad_x=1)
    null = change.pop('null', None)
    a.update(change)
    xg, gg = torch.ones(1, 32, 5, 7, device=DEV), torch.ones(1, 32, 5, 7, device=DEV)
    obuf, dw = carve((32, 32, 3, 5))                        # (room for the widest kernel asked for; it holds the sentinel)
    before = obuf.clone()
    lib = _lib.load()
    ptrs = {'dw': _lib.fptr(dw), 'x': _lib.fptr(xg), 'gy': _lib.fptr(gg)}
    if null:
        ptrs[null] = None
    rc = lib.l2i_conv2d_wgrad_f32(ptrs['dw'], ptrs['x'], ptrs['gy'], a['b'], a['cin'], a['h'], a['w'], a['cout'], a['oh'], a['ow'], a['kh'], a['kw'], a['stride'],
                                  a['pad_y'], a['pad_x'], _lib.stream_ptr())
    torch.cuda.synchronize()
    msg = lib.l2i_last_error().decode()
    print('rt32 wgrad refusal %s null=%s -> %d: %s' % (change, null, rc, msg))
    assert rc == expect and msg and part in msg
    assert torch.equal(bits(obuf), bits(before)), 'a refused call wrote something'
    assert bool((xg == 1).all()) and bool((gg == 1).all())


def test_wgrad_refuses_other_kernel_widths():
    _wgrad_refusal(E_UNSUPPORTED, 'conv2d_wgrad', kw=5)
    _wgrad_refusal(E_UNSUPPORTED, 'conv2d_wgrad', kh=1, kw=2)


@pytest.mark.parametrize('which', ['dw', 'x', 'gy'])
def test_wgrad_refuses_null(which):
    _wgrad_refusal(E_ARG, 'conv2d_wgrad', null=which)


@pytest.mark.parametrize('arg', ['b', 'cin', 'h', 'w', 'cout', 'oh', 'ow', 'kh', 'kw', 'stride'])
def test_wgrad_refuses_non_positive(arg):
    for value in (0, -1):
        _wgrad_refusal(E_ARG, 'conv2d_wgrad', **{arg: value})


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------------------------
def _stats(sum_, sumsq, x, case):
    _lib.call('l2i_bn_stats_f32', _lib.ptr(sum_), _lib.ptr(sumsq), _lib.fptr(x), case.b, case.c, case.hw[0] * case.hw[1])


def _apply(y, x, scale, shift, res, case):
    _lib.call('l2i_bn_apply_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(scale), _lib.fptr(shift), _lib.fptr(res), int(case.relu), case.b, case.c,
              case.hw[0] * case.hw[1])


@pytest.mark.parametrize('name', list(BN))
def test_bn_forward_kernels(name):
    case, m = BN[name], bn_model(name)
    d = m['d']
    xg = d['x'].to(DEV)
    resg = None if m['res'] is None else m['res'].to(DEV)
    mean, invstd, scale, shift = (t.to(DEV) for t in m['small'])
    s_buf, s = carve((case.c,), torch.float64, init=d['s0'] if case.preload else 0.0)
    q_buf, q = carve((case.c,), torch.float64, init=d['q0'] if case.preload else 0.0)
    _stats(s, q, xg, case)
    ys = []
    for _ in range(2):
        y_buf, y = carve(tuple(xg.shape))
        _apply(y, xg, scale, shift, resg, case)
        torch.cuda.synchronize()
        guards_intact(y_buf, 'y')
        ys.append(y)
    for buf, what in ((s_buf, 'sum'), (q_buf, 'sumsq')):
        guards_intact(buf, what)
    (ws, wq), (bs, bq) = m['stats']
    r_s, r_q = report('bn_stats.sum', name, s, ws, bs), report('bn_stats.sumsq', name, q, wq, bq)
    r_y = report('bn_apply', name, ys[0], *m['apply'])
    assert max(r_s, r_q, r_y) <= 1.0
    assert torch.equal(bits(ys[0]), bits(ys[1])), 'bn_apply is elementwise: two launches on the same inputs differ'
    assert torch.equal(bits(xg), bits(d['x'].to(DEV))) and (resg is None or torch.equal(bits(resg), bits(m['res'].to(DEV)))), 'an input changed'


@pytest.mark.parametrize('name', list(BN))
def test_bn_backward_kernels(name):
    case, m = BN[name], bn_model(name)
    d = m['d']
    xg, gg = d['x'].to(DEV), d['gy'].to(DEV)
    og = None if m['out'] is None else m['out'].to(DEV)
    mean, invstd = m['small'][0].to(DEV), m['small'][1].to(DEV)
    gamma, m_dy, m_dyxh = d['gamma'].to(DEV), m['means'][0].to(DEV), m['means'][1].to(DEV)
    hw = case.hw[0] * case.hw[1]
    s_buf, s = carve((case.c,), torch.float64, init=d['sd0'] if case.preload else 0.0)
    q_buf, q = carve((case.c,), torch.float64, init=d['sq0'] if case.preload else 0.0)
    _lib.call('l2i_bn_bwd_reduce_f32', _lib.ptr(s), _lib.ptr(q), _lib.fptr(gg), _lib.fptr(og), _lib.fptr(xg), _lib.fptr(mean), _lib.fptr(invstd), case.b, case.c, hw)
    got = []
    for _ in range(2):
        d_buf, dx = carve(tuple(xg.shape))
        m_buf, dym = carve(tuple(xg.shape))
        _lib.call('l2i_bn_bwd_apply_f32', _lib.fptr(dx), _lib.fptr(dym) if case.want_masked else None, _lib.fptr(gg), _lib.fptr(og), _lib.fptr(xg), _lib.fptr(mean),
                  _lib.fptr(invstd), _lib.fptr(gamma), _lib.fptr(m_dy), _lib.fptr(m_dyxh), case.b, case.c, hw)
        torch.cuda.synchronize()
        guards_intact(d_buf, 'dx')
        guards_intact(m_buf, 'the masked dy')
        got.append((dx, dym))
    for buf, what in ((s_buf, 'sum_dy'), (q_buf, 'sum_dyxh')):
        guards_intact(buf, what)
    (wd, wq), (bd, bq) = m['reduce']
    r_d, r_q = report('bn_bwd_reduce.sum_dy', name, s, wd, bd), report('bn_bwd_reduce.sum_dyxh', name, q, wq, bq)
    want, bound, dy_want = m['bwd']
    r_x = report('bn_bwd_apply', name, got[0][0], want, bound)
    assert max(r_d, r_q, r_x) <= 1.0
    if case.want_masked:                                   # a select: exact, and what it masks is +0.0
        assert torch.equal(got[0][1].cpu().double(), dy_want), 'the masked dy is a select: exact'
        assert torch.equal(bits(got[0][1].cpu()), bits(r32.masked_dy(d['gy'], m['out']))), 'the masked dy is a select: exact'
    else:
        assert torch.equal(got[0][1], torch.full_like(got[0][1], r32.SENTINEL)), 'no masked dy was asked for, yet its buffer changed'
    for a, b in zip(got[0], got[1]):
        assert torch.equal(bits(a), bits(b)), 'bn_bwd_apply is elementwise: two launches on the same inputs differ'


@pytest.mark.parametrize('name', [c.name for c in r32.BN_CASES if not c.preload])
def test_bn_wrappers(name):
    """regressor_train._BN.forward / .backward on the same cases: the argument order of the four calls and the algebra between them."""
    case, m = BN[name], bn_model(name)
    d, n = m['d'], m['n']
    P = {'bn.weight': d['gamma'].numpy(), 'bn.bias': d['beta'].numpy(), 'bn.running_mean': np.zeros(case.c, np.float32), 'bn.running_var': np.ones(case.c, np.float32)}
    bn = RT._BN(P, 'bn', DEV)
    xg, gg = d['x'].to(DEV), d['gy'].to(DEV)
    resg = None if m['res'] is None else m['res'].to(DEV)
    og = None if m['out'] is None else m['out'].to(DEV)
    y, saved = bn.forward(xg, residual=resg, relu=case.relu)
    r_y = report('bn_forward(wrapper)', name, y, *m['forward'])
    assert saved[0] is xg
    # the backward from the model's own mean / invstd, so that its bound (stated for those operands) applies
    mean, invstd = m['small'][0].to(DEV), m['small'][1].to(DEV)
    dx, d_weight, d_bias, gm = bn.backward(gg, (xg, mean, invstd), out_mask=og, want_masked=case.want_masked)
    torch.cuda.synchronize()
    want, bound, dy_want = m['bwd']
    r_x = report('bn_backward(wrapper)', name, dx, want, bound * (r32.K_BWD_WRAPPER / r32.K_BWD_APPLY))
    (wd, wq), (bd, bq) = m['reduce']
    half_ulp = lambda w: 2.0 ** -24 * w.abs()              # the sums leave as float32
    r_b, r_w = report('d_bias(wrapper)', name, d_bias, wd, bd + half_ulp(wd)), report('d_weight(wrapper)', name, d_weight, wq, bq + half_ulp(wq))
    assert max(r_y, r_x, r_b, r_w) <= 1.0
    assert (gm is not None) == case.want_masked
    if case.want_masked:
        assert torch.equal(bits(gm.cpu()), bits(r32.masked_dy(d['gy'], m['out'])))


def _bn_refusals(entry, part, ptr_names, required, call):
    """Each required pointer NULL and each of B, C, HW zero and negative: L2I_E_ARG, a message that names the entry, nothing written."""
    lib = _lib.load()
    c, b, hw = 4, 2, 6
    bufs = {}
    for name in ptr_names:
        dtype = torch.float64 if name.startswith('sum') else torch.float32
        shape = (c,) if (name.startswith('sum') or name in ('scale', 'shift', 'mean', 'invstd', 'gamma', 'm_dy', 'm_dyxh')) else (b, c, hw)
        bufs[name] = carve(shape, dtype)
    before = {k: v[0].clone() for k, v in bufs.items()}
    cases = [({name: None}, {}) for name in required] + [({}, {dim: v}) for dim in ('b', 'c', 'hw') for v in (0, -1)]
    for nulls, dims in cases:
        p = {k: (None if k in nulls else _lib.ptr(v[1])) for k, v in bufs.items()}
        g = dict(b=b, c=c, hw=hw)
        g.update(dims)
        rc = call(getattr(lib, entry), p, g)
        torch.cuda.synchronize()
        msg = lib.l2i_last_error().decode()
        print('rt32 %s refusal %s %s -> %d: %s' % (entry, sorted(nulls), dims, rc, msg))
        assert rc == E_ARG and msg and part in msg
        for k, v in bufs.items():
            assert torch.equal(bits(v[0]), bits(before[k])), 'a refused call wrote to ' + k


def test_bn_stats_refusals():
    _bn_refusals('l2i_bn_stats_f32', 'bn_stats', ('sum', 'sumsq', 'x'), ('sum', 'sumsq', 'x'),
                 lambda f, p, g: f(p['sum'], p['sumsq'], p['x'], g['b'], g['c'], g['hw'], _lib.stream_ptr()))


def test_bn_apply_refusals():
    _bn_refusals('l2i_bn_apply_f32', 'bn_apply', ('y', 'x', 'scale', 'shift', 'residual'), ('y', 'x', 'scale', 'shift'),
                 lambda f, p, g: f(p['y'], p['x'], p['scale'], p['shift'], p['residual'], 1, g['b'], g['c'], g['hw'], _lib.stream_ptr()))


def test_bn_bwd_reduce_refusals():
    _bn_refusals('l2i_bn_bwd_reduce_f32', 'bn_bwd_reduce', ('sum_dy', 'sum_dyxh', 'gy', 'out', 'x', 'mean', 'invstd'), ('sum_dy', 'sum_dyxh', 'gy', 'x', 'mean', 'invstd'),
                 lambda f, p, g: f(p['sum_dy'], p['sum_dyxh'], p['gy'], p['out'], p['x'], p['mean'], p['invstd'], g['b'], g['c'], g['hw'], _lib.stream_ptr()))


def test_bn_bwd_apply_refusals():
    names = ('dx', 'dy_masked', 'gy', 'out', 'x', 'mean', 'invstd', 'gamma', 'm_dy', 'm_dyxh')
    _bn_refusals('l2i_bn_bwd_apply_f32', 'bn_bwd_apply', names, tuple(k for k in names if k not in ('dy_masked', 'out')),
                 lambda f, p, g: f(*[p[k] for k in names], g['b'], g['c'], g['hw'], _lib.stream_ptr()))
