"""Every streaming kernel of csrc/l2i_stream.hip and csrc/l2i_stream_h8.hip, operand by operand and launch path by launch path, against the
float64 model of tests/stream_ref.py with that module's derived bounds (2^-23 k M elementwise, 2^-23 (n_lane + 16) M reduced, half an ulp
more for a 16-bit output; exact where the contract is exact).  Every output lies between sentinel guards, an absent operand is NULL, the
reduction buffers are zeroed here (one row per reducer adds into a pre-filled buffer), and every argument combination an entry refuses is
checked for its error code and an untouched output.  L2I_STREAM_CONTRACT_ERRORS=<file>: every observed error beside its bound."""
import os
import re

import pytest
import torch

from latent2im_amd import _lib, conv, kernels, kernels16 as K16
from tests import stream_ref as sr
from tests.contract_gpu import DEV, compare as _compare, dev, guarded, keep, refused, release, untouched

pytestmark = pytest.mark.gpu
ROWS = sr.all_rows()
PARAMS = [(r, e) for r in ROWS for e in (('f32',) if r.kind == 'f32' else ('bf16', 'f16'))]
PREFILL = 3.5
_LOG = []


@pytest.fixture(scope='module', autouse=True)
def _error_log():
    yield
    path = os.environ.get('L2I_STREAM_CONTRACT_ERRORS')
    if path:
        with open(path, 'w') as f:
            f.write('# row element output: largest |got - want| over the bound at that element (tests/test_stream_contract_gpu.py)\n' + '\n'.join(_LOG) + '\n')


@pytest.fixture
def precision():
    old = conv.PRECISION
    yield lambda elem: setattr(conv, 'PRECISION', elem)
    conv.PRECISION = old


@pytest.fixture(autouse=True)
def _operands_outlive_the_launch():
    yield
    release()


def compare(row, elem, got, exp, add_m=None):
    _compare(row, elem, got, exp, _LOG)


def h8in(row, elem):
    dtype = sr.ELEM_DTYPES.get(elem)
    C = row.shape[1]
    return dtype, (lambda t: None if t is None else keep(sr.to_h8(t, C, dtype).to(DEV)))


def reducer(shape, prefill):
    buf, view = guarded(shape)
    view.fill_(PREFILL if prefill else 0.0)
    return buf, view


def shift_sum(exp, name, prefill):
    """A row that adds into a pre-filled buffer: the contract is +=, one more rounded addition of |PREFILL| + |sum|."""
    if prefill and name in exp:
        want, bound = exp[name]
        exp[name] = (want + PREFILL, bound + sr.U23 * (PREFILL + want.abs()))


# ---- one runner per operation: operands -> {output: CPU tensor in the model's layout} ---------------------------------------------------------------
def run_torgb(row, kw, elem):
    B, C, H, W = row.shape
    buf, rgb = guarded((B, 3, H, W))
    if row.kind == 'h8':
        dtype, H8 = h8in(row, elem)
        _lib.call('l2i_torgb_fwd_h8', _lib.fptr(rgb), _lib.ptr(H8(kw['x'])), _lib.fptr(dev(kw['wmod'])), _lib.fptr(dev(kw.get('bias'))), B, C, H * W, dtype=dtype)
    else:
        _lib.call('l2i_torgb_fwd_f32', _lib.fptr(rgb), _lib.fptr(dev(kw['x'])), _lib.fptr(dev(kw['wmod'])), _lib.fptr(dev(kw.get('bias'))), B, C, H * W)
    torch.cuda.synchronize()
    assert untouched(buf, rgb)
    return {'rgb': rgb.cpu()}


def run_sg2(row, kw, elem):
    B, C, H, W = row.shape
    h8 = row.kind == 'h8'
    dtype, H8 = h8in(row, elem)
    put = H8 if h8 else dev
    y, gin = put(kw['y']), put(kw.get('gin'))
    dbuf, dz = guarded(tuple(y.shape), y.dtype)
    prefill = row.extra.get('prefill', False)
    reds = {n: reducer(s, prefill) for n, s in (('red_dz_z', (B, C)), ('red_x_grgb', (B, C, 3)), ('red_gin_y', (B, C))) if n in kw['_reds']}
    for n, operand in (('red_x_grgb', 'grgb'), ('red_gin_y', 'gin')):
        if n in reds and operand not in kw:                # the sum's operand is absent: the buffer must keep what it holds
            reds[n][1].fill_(sr.SENTINEL)
    rp = lambda n: _lib.fptr(reds[n][1]) if n in reds else None
    _lib.call('l2i_sg2_act_bwd_h8' if h8 else 'l2i_sg2_act_bwd_f32', _lib.ptr(dz), _lib.ptr(gin), _lib.fptr(dev(kw.get('gin_scale'))), _lib.fptr(dev(kw.get('grgb'))),
              _lib.fptr(dev(kw.get('wmod_rgb'))), _lib.ptr(y), _lib.fptr(dev(kw.get('bias'))), _lib.fptr(dev(kw.get('noise'))), float(kw.get('noise_w', 0.0)),
              float(kw['slope']), float(kw['gain']), rp('red_dz_z'), rp('red_x_grgb'), rp('red_gin_y'), B, C, H * W, dtype=dtype)
    torch.cuda.synchronize()
    assert untouched(dbuf, dz) and all(untouched(b, v) for b, v in reds.values())
    out = {'dz': sr.from_h8(dz.cpu(), C) if h8 else dz.cpu()}
    out.update({n: v.cpu() for n, (_, v) in reds.items()})
    return out


def run_dot(row, kw, elem):
    B, C, H, W = row.shape
    buf, out = reducer((B * C,), row.extra.get('prefill', False))
    if row.kind == 'h8':
        dtype, H8 = h8in(row, elem)
        K16.dot_reduce(H8(kw['a']), H8(kw.get('b')), out=out)
    else:
        kernels.dot_reduce(dev(kw['a']), dev(kw.get('b')), out=out)
    torch.cuda.synchronize()
    assert untouched(buf, out)
    return {'out': out.cpu().view(B, C)}


def run_sqdiff(row, kw, elem):
    h8 = row.kind == 'h8'
    dtype, H8 = h8in(row, elem)
    put = H8 if h8 else dev
    a, b = put(kw['a']), put(kw['b'])
    sb, s = reducer((1,), row.extra.get('prefill', False)) if kw['_sum'] else (None, None)
    gb, g = guarded(tuple(b.shape), b.dtype) if kw['_grad'] else (None, None)
    _lib.call('l2i_sqdiff_h8' if h8 else 'l2i_sqdiff_f32', _lib.fptr(s), _lib.ptr(g), _lib.ptr(a), _lib.ptr(b), a.numel() // (8 if h8 else 1), float(kw['coef']),
              _lib.fptr(dev(kw.get('coef_dev'))), dtype=dtype)
    torch.cuda.synchronize()
    out = {}
    if s is not None:
        assert untouched(sb, s)
        out['sum'] = s.cpu()
    if g is not None:
        assert untouched(gb, g)
        out['grad'] = sr.from_h8(g.cpu(), row.shape[1]) if h8 else g.cpu()
    return out


def run_axpby(row, kw, elem):
    buf, y = guarded(row.shape)
    kernels.axpby(dev(kw['a']), dev(kw.get('b')), kw['alpha'], kw['beta'], out=y)
    torch.cuda.synchronize()
    assert untouched(buf, y)
    return {'y': y.cpu()}


def run_relu_mask(row, kw, elem):
    buf, y = guarded(row.shape)
    _lib.call('l2i_relu_mask_f32', _lib.fptr(y), _lib.fptr(dev(kw['g'])), _lib.fptr(dev(kw['ref'])), y.numel())
    torch.cuda.synchronize()
    assert untouched(buf, y)
    return {'y': y.cpu()}


def run_mask_mul(row, kw, elem):
    dtype, H8 = h8in(row, elem)
    g, ref = H8(kw['g']), H8(kw['ref'])
    bits = sr.sign_plane(ref.cpu()).to(DEV)
    (b1, y1), (b2, y2) = guarded(tuple(g.shape), dtype), guarded(tuple(g.shape), dtype)
    _lib.call('l2i_mask_mul_h8', _lib.ptr(y1), _lib.ptr(g), _lib.ptr(ref), float(kw['pos']), float(kw['neg']), g.numel() // 8, dtype=dtype)
    _lib.call('l2i_mask_mul_bits_h8', _lib.ptr(y2), _lib.ptr(g), _lib.ptr(bits), float(kw['pos']), float(kw['neg']), g.numel() // 8, dtype=dtype)
    torch.cuda.synchronize()
    assert untouched(b1, y1) and untouched(b2, y2)
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)), 'the sign-plane form differs from the map form'
    return {'y': sr.from_h8(y1.cpu(), row.shape[1])}


def run_zero_insert(row, kw, elem):
    dtype, H8 = h8in(row, elem)
    y0 = H8(kw['y'])
    buf, y = guarded(tuple(y0.shape), dtype)
    y.copy_(y0)
    K16.add_zero_insert(y, H8(kw['c']), H8(kw.get('mask')))
    torch.cuda.synchronize()
    assert untouched(buf, y)
    return {'y': sr.from_h8(y.cpu(), row.shape[1])}


def run_pool(row, kw, elem):
    B, C, H, W = row.shape
    k, s, pad = kw['k'], kw['s'], kw['pad']
    OH, OW = sr.pool_out(H, k, s, pad), sr.pool_out(W, k, s, pad)
    if row.kind == 'f32':
        off = sr.pool_offsets(row.extra['aligned'])          # views that start off a 16-byte boundary: the kernels that need it must not be taken
        (xb, x), (yb, y), (gb, gx) = guarded(row.shape, off=off.get('x', 0)), guarded((B, C, OH, OW), off=off.get('y', 0)), guarded(row.shape, off=off.get('gx', 0))
        (ib, idx), (_, gy) = guarded((B, C, OH, OW), torch.uint8, off=off.get('idx', 0)), guarded((B, C, OH, OW), off=off.get('gy', 0))
        x.copy_(kw['x'])
        gy.copy_(kw['gy'])
        for name, t in (('x', x), ('y', y), ('gx', gx), ('idx', idx), ('gy', gy)):
            assert t.data_ptr() % 64 == off.get(name, 0) * t.element_size(), name
        _lib.call('l2i_maxpool2d_fwd_f32', _lib.fptr(y), _lib.ptr(idx), _lib.fptr(x), B * C, H, W, k, s, pad, OH, OW)
        _lib.call('l2i_maxpool2d_bwd_f32', _lib.fptr(gx), _lib.fptr(gy), _lib.ptr(idx), B * C, H, W, k, s, pad, OH, OW)
        torch.cuda.synchronize()
        assert untouched(yb, y) and untouched(ib, idx) and untouched(gb, gx)
        return {'y': y.cpu(), 'idx': idx.cpu(), 'gx': gx.cpu()}
    dtype, H8 = h8in(row, elem)
    G8 = C // 8
    (yb, y), (ib, idx), (gb, gx) = guarded((B, G8, OH, OW, 8), dtype), guarded((B, G8, OH, OW, 8), torch.uint8), guarded((B, G8, H, W, 8), dtype)
    _lib.call('l2i_maxpool2d_fwd_h8', _lib.ptr(y), _lib.ptr(idx), _lib.ptr(H8(kw['x'])), B * G8, H, W, k, s, pad, OH, OW, int(kw['relu']), dtype=dtype)
    _lib.call('l2i_maxpool2d_bwd_h8', _lib.ptr(gx), _lib.ptr(H8(kw['gy'])), _lib.ptr(idx), _lib.ptr(H8(kw.get('a'))), _lib.ptr(H8(kw.get('b'))), float(kw.get('coef', 0.0)),
              _lib.fptr(dev(kw.get('coef_dev'))), B * G8, H, W, k, s, pad, OH, OW, dtype=dtype)
    torch.cuda.synchronize()
    assert untouched(yb, y) and untouched(ib, idx) and untouched(gb, gx)
    return {'y': sr.from_h8(y.cpu(), C), 'idx': idx.cpu().permute(0, 1, 4, 2, 3).reshape(B, C, OH, OW), 'gx': sr.from_h8(gx.cpu(), C)}


def run_add_diff(row, kw, elem):
    B, C, H, W = row.shape
    _, idx = kernels.maxpool2d_fwd(dev(kw['x']), 2, 2, 0)
    buf, gx = guarded(row.shape)
    _lib.call('l2i_maxpool2x2_bwd_add_diff_f32', _lib.fptr(gx), _lib.fptr(dev(kw['gy'])), _lib.ptr(idx), _lib.fptr(dev(kw['a'])), _lib.fptr(dev(kw['b'])), float(kw['coef']),
              _lib.fptr(dev(kw.get('coef_dev'))), B * C, H // 2, W // 2)
    torch.cuda.synchronize()
    assert untouched(buf, gx)
    return {'gx': gx.cpu()}


def run_cast(row, kw, elem):
    B, C, H, W = row.shape
    dtype, cpad = sr.ELEM_DTYPES[elem], row.extra['cpad']
    (tb, t), (fb, back) = guarded((B, cpad // 8, H, W, 8), dtype), guarded(row.shape)
    _lib.call('l2i_cast_f32_to_h8', _lib.ptr(t), _lib.fptr(dev(kw['x'])), B, C, cpad, H * W, dtype=dtype)
    _lib.call('l2i_cast_h8_to_f32', _lib.fptr(back), _lib.ptr(t), B, C, cpad, H * W, dtype=dtype)
    torch.cuda.synchronize()
    assert untouched(tb, t) and untouched(fb, back)
    assert torch.equal(t.cpu().view(torch.int16), sr.to_h8(kw['x'], cpad, dtype).view(torch.int16)), 'bit pattern (pad lanes: +0)'
    return {'h8': t.cpu(), 'back': back.cpu()}


RUN = {'torgb': run_torgb, 'sg2': run_sg2, 'dot': run_dot, 'sqdiff': run_sqdiff, 'axpby': run_axpby, 'relu_mask': run_relu_mask, 'mask_mul': run_mask_mul,
       'zero_insert': run_zero_insert, 'pool': run_pool, 'add_diff': run_add_diff, 'cast': run_cast}


@pytest.mark.parametrize('row,elem', PARAMS, ids=['%s-%s' % (r.id, e) for r, e in PARAMS])
def test_streaming_kernel_against_the_model(row, elem, precision):
    if row.kind == 'h8':
        precision(elem)
        # the library takes one strip everywhere when this is set: the strip rows would pass on the one-strip path
        assert not os.environ.get('L2I_H8_DET'), 'unset L2I_H8_DET: the h8 reducer rows name the strip count of the default launch'
    kw = sr.make_inputs(row, elem)
    exp = sr.expected(row, kw, elem)
    for name in ('red_dz_z', 'red_x_grgb', 'red_gin_y', 'out', 'sum'):
        shift_sum(exp, name, row.extra.get('prefill', False))
    got = RUN[row.op](row, kw, elem)
    assert set(got) >= set(exp), (sorted(got), sorted(exp))
    compare(row, elem, got, exp)


# ---- refusals: the error code, and outputs that still hold the sentinel ---------------------------------------------------------------------------------
def _f32_maps(B, C, HW, off=0):
    """A [B, C, HW] float map of ones that starts ``off`` floats into its (16-byte aligned) buffer."""
    buf = torch.ones(B * C * HW + 8, device=DEV)
    return buf[off:off + B * C * HW].view(B, C, HW)


@pytest.mark.parametrize('what', ['hw_mod4', 'x_off_one_float', 'rgb_off_one_float'])
def test_torgb_f32_refusals(what):
    B, C, HW = 1, 2, 6 if what == 'hw_mod4' else 8
    buf, rgb = guarded((B, 3, HW), off=1 if what == 'rgb_off_one_float' else 0)
    x = _f32_maps(B, C, HW, 1 if what == 'x_off_one_float' else 0)
    assert (x.data_ptr() % 16 != 0) == (what == 'x_off_one_float') and (rgb.data_ptr() % 16 != 0) == (what == 'rgb_off_one_float')
    refused(-1, 'l2i_torgb_fwd_f32', _lib.fptr(rgb), _lib.fptr(x), _lib.fptr(keep(torch.ones(B, 3, C, device=DEV))), None, B, C, HW, outs=[buf])


SG2_REFUSALS = ['hw_mod4', 'grgb_without_wmod', 'wmod_without_grgb', 'neither_gin_nor_grgb', 'zero_gain', 'zero_slope', 'dz_off', 'y_off', 'gin_off', 'grgb_off', 'noise_off']


@pytest.mark.parametrize('what', SG2_REFUSALS)
def test_sg2_act_bwd_f32_refusals(what):
    B, C, HW = 1, 2, 6 if what == 'hw_mod4' else 8
    off = lambda n: 1 if what == n + '_off' else 0
    dbuf, dz = guarded((B, C, HW), off=off('dz'))
    rbuf, red = guarded((B, C))
    y, gin, grgb, noise = _f32_maps(B, C, HW, off('y')), _f32_maps(B, C, HW, off('gin')), _f32_maps(B, 3, HW, off('grgb')), _f32_maps(B, 1, HW, off('noise'))
    wm = torch.ones(B, 3, C, device=DEV)
    if what == 'grgb_without_wmod':
        wm = None
    if what in ('wmod_without_grgb', 'neither_gin_nor_grgb'):
        grgb = None
    if what == 'neither_gin_nor_grgb':
        gin, wm = None, None
    refused(-1, 'l2i_sg2_act_bwd_f32', _lib.fptr(dz), _lib.fptr(gin), None, _lib.fptr(grgb), _lib.fptr(wm), _lib.fptr(y), None, _lib.fptr(noise), 0.3,
            0.0 if what == 'zero_slope' else 0.2, 0.0 if what == 'zero_gain' else 2.0, _lib.fptr(red), None, None, B, C, HW, outs=[dbuf, rbuf])


@pytest.mark.parametrize('elem', ['bf16', 'f16'])
@pytest.mark.parametrize('what', ['c_mod8', 'grgb_without_wmod', 'wmod_without_grgb', 'neither_gin_nor_grgb', 'zero_gain', 'zero_slope'])
def test_sg2_act_bwd_h8_refusals(what, elem):
    dtype = sr.ELEM_DTYPES[elem]
    B, C, HW = 1, 12 if what == 'c_mod8' else 8, 8
    dbuf, dz = guarded((B, 2, HW, 1, 8), dtype)
    rbuf, red = guarded((B, 16))
    y, gin = torch.ones(B, 2, HW, 1, 8, device=DEV, dtype=dtype), torch.ones(B, 2, HW, 1, 8, device=DEV, dtype=dtype)
    grgb, wm = torch.ones(B, 3, HW, device=DEV), torch.ones(B, 3, 16, device=DEV)
    if what == 'grgb_without_wmod':
        wm = None
    if what in ('wmod_without_grgb', 'neither_gin_nor_grgb'):
        grgb = None
    if what == 'neither_gin_nor_grgb':
        gin, wm = None, None
    refused(-1, 'l2i_sg2_act_bwd_h8', _lib.ptr(dz), _lib.ptr(gin), None, _lib.fptr(grgb), _lib.fptr(wm), _lib.ptr(y), None, None, 0.0,
            0.0 if what == 'zero_slope' else 0.2, 0.0 if what == 'zero_gain' else 2.0, _lib.fptr(red), None, None, B, C, HW, outs=[dbuf, rbuf], dtype=dtype)


@pytest.mark.parametrize('elem', ['bf16', 'f16'])
def test_h8_channel_count_refusals(elem):
    dtype = sr.ELEM_DTYPES[elem]
    x = torch.ones(1, 2, 8, 1, 8, device=DEV, dtype=dtype)
    buf, rgb = guarded((1, 3, 8))
    refused(-1, 'l2i_torgb_fwd_h8', _lib.fptr(rgb), _lib.ptr(x), _lib.fptr(keep(torch.ones(1, 3, 16, device=DEV))), None, 1, 12, 8, outs=[buf], dtype=dtype)
    buf, out = guarded((16,))
    refused(-1, 'l2i_dot_reduce_h8', _lib.fptr(out), _lib.ptr(x), None, 1, 12, 8, outs=[buf], dtype=dtype)


def test_maxpool_refusals():
    """k > 15 (the index is one byte per window); the fused 2x2 backward: odd OW, tensors off the 16-byte grid; h8: a without b and the reverse."""
    (yb, y), (ib, idx), (gb, gx) = guarded((1, 1, 2, 2)), guarded((1, 1, 2, 2), torch.uint8), guarded((1, 1, 17, 17))
    x = torch.ones(1, 1, 17, 17, device=DEV)
    refused(-1, 'l2i_maxpool2d_fwd_f32', _lib.fptr(y), _lib.ptr(idx), _lib.fptr(x), 1, 17, 17, 16, 1, 0, 2, 2, outs=[yb, ib])
    refused(-1, 'l2i_maxpool2d_bwd_f32', _lib.fptr(gx), _lib.fptr(keep(torch.ones(1, 1, 2, 2, device=DEV))), _lib.ptr(keep(torch.zeros(1, 1, 2, 2, device=DEV, dtype=torch.uint8))),
            1, 17, 17, 16, 1, 0, 2, 2, outs=[gb])
    a, gy, i8 = torch.ones(1, 1, 4, 8, device=DEV), torch.ones(1, 1, 2, 4, device=DEV), torch.zeros(1, 1, 2, 4, device=DEV, dtype=torch.uint8)
    gb, gx = guarded((1, 1, 4, 6))
    refused(-1, 'l2i_maxpool2x2_bwd_add_diff_f32', _lib.fptr(gx), _lib.fptr(gy), _lib.ptr(i8), _lib.fptr(a), _lib.fptr(a), 0.5, None, 1, 2, 3, outs=[gb])
    gb, gx = guarded((1, 1, 4, 8), off=1)
    refused(-1, 'l2i_maxpool2x2_bwd_add_diff_f32', _lib.fptr(gx), _lib.fptr(gy), _lib.ptr(i8), _lib.fptr(a), _lib.fptr(a), 0.5, None, 1, 2, 4, outs=[gb])
    for elem, dtype in sr.ELEM_DTYPES.items():
        t = torch.ones(1, 1, 4, 4, 8, device=DEV, dtype=dtype)
        g2, i2 = torch.ones(1, 1, 2, 2, 8, device=DEV, dtype=dtype), torch.zeros(1, 1, 2, 2, 8, device=DEV, dtype=torch.uint8)
        gb, gx = guarded((1, 1, 4, 4, 8), dtype)
        for a_, b_ in ((t, None), (None, t)):
            refused(-1, 'l2i_maxpool2d_bwd_h8', _lib.ptr(gx), _lib.ptr(g2), _lib.ptr(i2), _lib.ptr(a_), _lib.ptr(b_), 0.5, None, 1, 4, 4, 2, 2, 0, 2, 2, outs=[gb], dtype=dtype)
        big = torch.ones(1, 1, 17, 17, 8, device=DEV, dtype=dtype)
        (yb, y), (ib, idx) = guarded((1, 1, 2, 2, 8), dtype), guarded((1, 1, 2, 2, 8), torch.uint8)
        refused(-1, 'l2i_maxpool2d_fwd_h8', _lib.ptr(y), _lib.ptr(idx), _lib.ptr(big), 1, 17, 17, 16, 1, 0, 2, 2, 0, outs=[yb, ib], dtype=dtype)
        gb, gx = guarded((1, 1, 17, 17, 8), dtype)
        refused(-1, 'l2i_maxpool2d_bwd_h8', _lib.ptr(gx), _lib.ptr(g2), _lib.ptr(i2), None, None, 0.0, None, 1, 17, 17, 16, 1, 0, 2, 2, outs=[gb], dtype=dtype)


@pytest.mark.parametrize('elem', ['bf16', 'f16'])
def test_sign_plane_mask_on_a_resampling_fir_is_refused(elem):
    import ctypes
    dtype = sr.ELEM_DTYPES[elem]
    x = torch.ones(1, 1, 4, 4, 8, device=DEV, dtype=dtype)
    buf, y = guarded((1, 1, 8, 8, 8), dtype)
    k = torch.ones(4, 4, device=DEV)
    k1 = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    bits = torch.zeros(1, 1, 8, 8, device=DEV, dtype=torch.uint8)
    refused(-3, 'l2i_upfirdn2d_h8', _lib.ptr(y), _lib.ptr(x), _lib.fptr(k), 1, 8, 4, 4, 4, 4, 2, 1, 2, 1, 2, 1, None, 0.0, None, 0, 0.2, 1.0, _lib.ptr(bits), 1.0, 0.0, None,
            k1, k1, 1, outs=[buf], dtype=dtype)


def test_rows_cover_what_the_header_promises():
    """The decisions recorded in include/l2i.h each have a row: NULL bias in both ToRGB forms, NULL red_dz_z in both backward forms."""
    ids = {r.id for r in ROWS}
    assert {'torgb_f32-no_bias-operands', 'torgb_h8-no_bias-operands', 'sg2_f32-no_red_dz_z-base', 'sg2_h8-no_red_dz_z-base'} <= ids
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'l2i.h')) as f:
        text = f.read()
    assert re.search(r'grgb and wmod_rgb go together', text) and re.search(r'16-byte boundaries', text)
