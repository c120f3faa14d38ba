"""The training kernels on h8 maps (csrc/l2i_train_h8.hip) against the float64 models and derived bounds of tests/regtrain16_ref.py: every kernel
x {bf16, fp16}, outputs and workspaces carved out of sentinel-filled buffers (nothing outside them may change), every case launched twice with
bit-equal results (no atomics, fixed summation order).  Every test prints `rt16 <kernel> <case> <elem> <error / bound>`."""
import ctypes

import pytest
import torch

from latent2im_amd import _lib, conv
from latent2im_amd import kernels16 as K16
from tests import regtrain16_ref as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                  # sentinel elements on either side of a carved tensor
WGRAD = {c.name: c for c in rr.WGRAD_CASES}
BN = {c.name: c for c in rr.BN_CASES}
_BN_MODEL = {}                # (case, elem) -> the float64 model of the case, once


def carve(shape, dtype, fill=rr.SENTINEL):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, what):
    fill = torch.full((GUARD,), rr.SENTINEL, dtype=buf.dtype, device=DEV)
    assert torch.equal(buf[:GUARD], fill) and torch.equal(buf[-GUARD:], fill), 'the launch wrote outside ' + what


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def h8(t, dtype):
    return conv.to_h8(t.to(DEV), 8, dtype)


def scale_of(case):
    return rr._f(rr._f(case.host_scale) * (1.0 if case.dev_scale is None else rr._f(case.dev_scale)))


@pytest.mark.parametrize('elem', rr.ELEMS)
@pytest.mark.parametrize('name', list(WGRAD))
def test_wgrad(name, elem):
    case, dtype = WGRAD[name], rr.ELEM_DTYPES[elem]
    x, gy = rr.wgrad_data(case)
    want, bound = rr.wgrad(x, gy, case.k, case.stride, case.pad, scale_of(case), elem)
    xg, gg = h8(x, dtype), h8(gy, dtype)
    oh, ow = gy.shape[2:]
    nbytes = K16.wgrad_ws_bytes(case.b, case.cin, case.h, case.w, case.cout, oh, ow, case.k, case.stride, case.pad, dtype)
    assert nbytes > 0 and nbytes % 4 == 0
    dev = None if case.dev_scale is None else torch.tensor([case.dev_scale], device=DEV)
    outs = []
    for _ in range(2):
        wbuf, ws = carve((nbytes // 4,), torch.float32)
        obuf, dw = carve((case.cout, case.cin, case.k, case.k), torch.float32)
        K16.conv_wgrad(xg, gg, case.k, case.stride, case.pad, out=dw, ws=ws, out_scale=case.host_scale, out_scale_dev=dev)
        torch.cuda.synchronize()
        guards_intact(wbuf, 'the workspace')
        guards_intact(obuf, 'dw')
        outs.append(dw.clone())
    err, b, ratio = rr.worst(outs[0], want, bound)
    print('rt16 wgrad %s %s error %.3g bound %.3g ratio %.3g' % (name, elem, err, b, ratio))
    assert ratio <= 1.0
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'two launches on the same inputs differ'


@pytest.mark.parametrize('elem', rr.ELEMS)
@pytest.mark.parametrize('arg,value', rr.WGRAD_REFUSALS)
def test_wgrad_refusals(arg, value, elem):
    dtype = rr.ELEM_DTYPES[elem]
    s = dict(k=3, stride=1, pad=1, cin=32, cout=32, b=1, h=5, w=7)
    good = K16.wgrad_ws_bytes(s['b'], s['cin'], s['h'], s['w'], s['cout'], 5, 7, 3, 1, 1, dtype)
    if arg in s:
        s[arg] = value
    oh, ow = max(1, rr.out_size(s['h'], s['k'], s['stride'], s['pad'])), max(1, rr.out_size(s['w'], s['k'], s['stride'], s['pad']))
    cg = (s['cin'] + 7) // 8
    xg = torch.zeros(s['b'], cg, s['h'], s['w'], 8, device=DEV, dtype=dtype)
    gg = torch.zeros(s['b'], s['cout'] // 8, oh, ow, 8, device=DEV, dtype=dtype)
    wbuf, ws = carve((good // 4,), torch.float32)
    obuf, dw = carve((s['cout'], s['cin'], s['k'], s['k']), torch.float32)
    before_w, before_o = wbuf.clone(), obuf.clone()
    lib = _lib.load()
    fn = getattr(lib, 'l2i_conv2d_wgrad_h8' + ('_f16' if elem == 'f16' else ''))
    ws_ptr = None if arg == 'ws' else _lib.fptr(ws)
    ws_bytes = good - 4 if arg == 'ws_bytes' else good
    rc = fn(_lib.fptr(dw), _lib.ptr(xg), _lib.ptr(gg), ws_ptr, ws_bytes, 1.0, None, s['b'], s['cin'], s['h'], s['w'], s['cout'], oh, ow, s['k'], s['stride'], s['pad'],
            _lib.stream_ptr())
    torch.cuda.synchronize()
    msg = lib.l2i_last_error().decode()
    print('rt16 wgrad refusal %s=%s %s -> %d: %s' % (arg, value, elem, rc, msg))
    assert rc == -3 and msg                                  # L2I_E_UNSUPPORTED, with a message
    assert torch.equal(bits(wbuf), bits(before_w)) and torch.equal(bits(obuf), bits(before_o)), 'a refused call wrote something'
    if arg in ('k', 'stride', 'cin', 'pad'):                 # the host-only query refuses the same shapes
        n = ctypes.c_int64(-1)
        q = getattr(lib, 'l2i_conv2d_wgrad_ws_h8' + ('_f16' if elem == 'f16' else ''))
        assert q(ctypes.byref(n), s['b'], s['cin'], s['h'], s['w'], s['cout'], oh, ow, s['k'], s['stride'], s['pad']) == -3 and n.value == 0


def bn_model(case, elem):
    key = (case.name, elem)
    if key not in _BN_MODEL:
        d = rr.bn_data(case)
        n = case.b * case.hw[0] * case.hw[1]
        (s, q), sb = rr.bn_stats(d['x'], elem)
        mean, invstd, scale, shift = (t.float() for t in rr.bn_finalize(s, q, n, d['gamma'], d['beta']))
        res = d['residual'] if case.residual else None
        out = d['out'] if case.out_mask else None
        (sd, sq), rb = rr.bn_bwd_reduce(d['gy'], out, d['x'], mean, invstd, elem)
        m_dy, m_dyxh = (sd / n).float(), (sq / n).float()
        _BN_MODEL[key] = dict(d=d, n=n, stats=((s, q), sb), small=(mean, invstd, scale, shift), res=res, out=out,
                              apply=rr.bn_apply(d['x'], scale, shift, res, case.relu, elem), reduce=((sd, sq), rb), means=(m_dy, m_dyxh),
                              bwd=rr.bn_bwd_apply(d['gy'], out, d['x'], mean, invstd, d['gamma'], m_dy, m_dyxh, elem))
    return _BN_MODEL[key]


def _ws(case, dtype):
    nbytes = K16.bn_ws_bytes(case.b, case.c, case.hw[0] * case.hw[1], dtype)
    assert nbytes > 0 and nbytes % 8 == 0
    return carve((nbytes // 8,), torch.float64)


@pytest.mark.parametrize('elem', rr.ELEMS)
@pytest.mark.parametrize('name', list(BN))
def test_bn_forward_kernels(name, elem):
    case, dtype = BN[name], rr.ELEM_DTYPES[elem]
    m = bn_model(case, elem)
    xg = h8(m['d']['x'], dtype)
    mean, invstd, scale, shift = (t.to(DEV) for t in m['small'])
    resg = None if m['res'] is None else h8(m['res'], dtype)
    got = []
    for _ in range(2):
        wbuf, ws = _ws(case, dtype)
        sbuf, sums = carve((2, case.c), torch.float64)
        ybuf, y = carve(tuple(xg.shape), dtype)
        K16.bn_stats(xg, sums, ws=ws)
        K16.bn_apply(xg, scale, shift, residual=resg, relu=case.relu, out=y)
        torch.cuda.synchronize()
        for buf, what in ((wbuf, 'the workspace'), (sbuf, 'the sums'), (ybuf, 'y')):
            guards_intact(buf, what)
        got.append((sums.clone(), y.clone()))
    (s, q), (bs, bq) = m['stats']
    r_s, r_q = rr.worst(got[0][0][0], s, bs)[2], rr.worst(got[0][0][1], q, bq)[2]
    want, bound = m['apply']
    r_y = rr.worst(conv.from_h8(got[0][1]), want, bound)[2]
    print('rt16 bn_stats / bn_apply %s %s ratios: sum %.3g sumsq %.3g y %.3g' % (name, elem, r_s, r_q, r_y))
    assert max(r_s, r_q, r_y) <= 1.0
    assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(bits(got[0][1]), bits(got[1][1])), 'two launches on the same inputs differ'


@pytest.mark.parametrize('elem', rr.ELEMS)
@pytest.mark.parametrize('name', list(BN))
def test_bn_backward_kernels(name, elem):
    case, dtype = BN[name], rr.ELEM_DTYPES[elem]
    m = bn_model(case, elem)
    d = m['d']
    xg, gg = h8(d['x'], dtype), h8(d['gy'], dtype)
    og = None if m['out'] is None else h8(m['out'], dtype)
    mean, invstd = m['small'][0].to(DEV), m['small'][1].to(DEV)
    gamma, m_dy, m_dyxh = d['gamma'].to(DEV), m['means'][0].to(DEV), m['means'][1].to(DEV)
    got = []
    for _ in range(2):
        wbuf, ws = _ws(case, dtype)
        sbuf, sums = carve((2, case.c), torch.float64)
        dbuf, dx = carve(tuple(xg.shape), dtype)
        mbuf, dym = carve(tuple(xg.shape), dtype)
        K16.bn_bwd_reduce(gg, og, xg, mean, invstd, sums, ws=ws)
        K16.bn_bwd_apply(gg, og, xg, mean, invstd, gamma, m_dy, m_dyxh, out=dx, masked=dym if case.want_masked else None)
        torch.cuda.synchronize()
        for buf, what in ((wbuf, 'the workspace'), (sbuf, 'the sums'), (dbuf, 'dx'), (mbuf, 'the masked dy')):
            guards_intact(buf, what)
        got.append((sums.clone(), dx.clone(), dym.clone()))
    (sd, sq), (bd, bq) = m['reduce']
    r_d, r_q = rr.worst(got[0][0][0], sd, bd)[2], rr.worst(got[0][0][1], sq, bq)[2]
    want, bound, dy_want = m['bwd']
    r_x = rr.worst(conv.from_h8(got[0][1]), want, bound)[2]
    print('rt16 bn_bwd_reduce / bn_bwd_apply %s %s ratios: sum_dy %.3g sum_dyxh %.3g dx %.3g' % (name, elem, r_d, r_q, r_x))
    assert max(r_d, r_q, r_x) <= 1.0
    if case.want_masked:
        assert torch.equal(conv.from_h8(got[0][2]).double().cpu(), dy_want), 'the masked dy is a select: exact'
    else:
        assert torch.equal(got[0][2], torch.full_like(got[0][2], rr.SENTINEL)), 'no masked dy was asked for, yet its buffer changed'
    for a, b in zip(got[0], got[1]):
        assert torch.equal(bits(a), bits(b)), 'two launches on the same inputs differ'
