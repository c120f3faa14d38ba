"""Every FIR, bias-activation and weight-plane kernel of csrc/l2i_stream.hip and csrc/l2i_stream_h8.hip, operand by operand and launch path by
launch path, against the model of tests/fir_ref.py with that module's derived bounds (2^-23 k M, half an ulp more for a 16-bit output; exact
where the contract is exact).  Every output lies between sentinel guards, an absent operand is NULL, the entry points are called directly, a
twin row (one dispatch predicate false alone) is also compared bit for bit with the launch it is the twin of where the code claims identity,
and every argument combination an entry refuses is checked for its code, its message and an untouched output.
L2I_FIR_CONTRACT_ERRORS=<file>: every observed error beside its bound."""
import ctypes
import os
import re

import pytest
import torch

from latent2im_amd import _lib
from tests import fir_ref as fr
from tests import stream_ref as sr
from tests.contract_gpu import DEV, compare, dev, guarded, keep, release, untouched

pytestmark = pytest.mark.gpu
ROWS = fr.all_rows()
PARAMS = [(r, e) for r in ROWS for e in (('f32',) if r.kind == 'f32' else ('bf16', 'f16'))]
_LOG = []
_RESULTS = {}          # (row id, element type) -> the output of a row other rows are twins of


@pytest.fixture(scope='module', autouse=True)
def _error_log():
    yield
    _RESULTS.clear()
    path = os.environ.get('L2I_FIR_CONTRACT_ERRORS')
    if path:
        with open(path, 'w') as f:
            f.write('# row element output: largest |got - want| over the bound at that element (tests/test_fir_contract_gpu.py)\n' + '\n'.join(_LOG) + '\n')


@pytest.fixture(autouse=True)
def _operands_outlive_the_launch():
    yield
    release()


def put(t, off=0):
    """``t`` on the device inside a guarded buffer, ``off`` elements past a 16-byte boundary (None stays None)."""
    if t is None:
        return None
    buf, view = guarded(tuple(t.shape), t.dtype, off=off)
    view.copy_(t)
    keep(buf)
    assert view.data_ptr() % 16 == (off * t.element_size()) % 16
    return view


def run_fir_f32(row, kw):
    B, C, ih, iw = row.shape
    g = fr.geom(row)
    oh, ow = g['oh'], g['ow']
    major = kw.get('_major', B * C)
    off = row.extra.get('off') or {}
    maps = lambda t, h, w: None if t is None else t.reshape(-1, h, w)[:major].contiguous()
    x = put(maps(kw['x'], ih, iw), off.get('x', 0))
    ybuf, y = guarded((major, oh, ow), off=off.get('y', 0))
    noise, addend, mask = put(kw.get('noise'), off.get('noise', 0)), put(maps(kw.get('addend'), oh, ow), off.get('addend', 0)), put(maps(kw.get('mask'), oh, ow), off.get('mask', 0))
    k = dev(kw['k'].contiguous())
    (ux, uy), (dx, dy), pad = kw['up'], kw['down'], kw['pad']
    args = [_lib.fptr(y), _lib.fptr(x), _lib.fptr(k), major, ih, iw, g['kh'], g['kw'], ux, uy, dx, dy, pad[0], pad[1], pad[2], pad[3], C,
            _lib.fptr(noise), float(kw.get('noise_w', 0.0)), _lib.fptr(dev(kw.get('bias'))), _lib.fptr(addend), int(kw['act']), float(kw['slope']), float(kw['gain'])]
    if mask is not None:
        _lib.call('l2i_upfirdn2d_masked_f32', *args, _lib.fptr(mask), float(kw['mask_vals'][0]), float(kw['mask_vals'][1]))
    else:
        _lib.call('l2i_upfirdn2d_f32', *args)
    torch.cuda.synchronize()
    assert untouched(ybuf, y)
    out = y.cpu()
    return {'y': out if '_major' in kw else out.view(B, C, oh, ow)}


def run_fir_h8(row, kw, elem):
    B, C, ih, iw = row.shape
    g = fr.geom(row)
    oh, ow = g['oh'], g['ow']
    dtype = sr.ELEM_DTYPES[elem]
    H8 = lambda t: None if t is None else keep(sr.to_h8(t, C, dtype).to(DEV))
    x, addend, mask = H8(kw['x']), H8(kw.get('addend')), H8(kw.get('mask'))
    bits = row.extra.get('mask_bits', False)
    if bits:
        mask = keep(sr.sign_plane(mask.cpu()).to(DEV))
    ybuf, y = guarded((B, C // 8, oh, ow, 8), dtype)
    k1y = k1x = None
    if 'taps' in kw:
        k1y, k1x = (ctypes.c_float * 4)(*kw['taps'][0]), (ctypes.c_float * 4)(*kw['taps'][1])
    up, down, pad = kw['up'][0], kw['down'][0], kw['pad']
    _lib.call('l2i_upfirdn2d_h8', _lib.ptr(y), _lib.ptr(x), _lib.fptr(dev(kw['k'].contiguous())), B * C // 8, C, ih, iw, g['kh'], g['kw'], up, down,
              pad[0], pad[1], pad[2], pad[3], _lib.fptr(dev(kw.get('noise'))), float(kw.get('noise_w', 0.0)), _lib.fptr(dev(kw.get('bias'))), int(kw['act']),
              float(kw['slope']), float(kw['gain']), _lib.ptr(mask), float(kw.get('mask_vals', (1.0, 0.0))[0]), float(kw.get('mask_vals', (1.0, 0.0))[1]),
              _lib.ptr(addend), k1y, k1x, int(bits), dtype=dtype)
    torch.cuda.synchronize()
    assert untouched(ybuf, y)
    return {'y': sr.from_h8(y.cpu(), C)}


def run_fba(row, kw):
    n = row.shape[3]
    off = row.extra.get('off') or {}
    x, ref = put(kw['x'], off.get('x', 0)), put(kw.get('ref'), off.get('ref', 0))
    ybuf, y = guarded((n,), off=off.get('y', 0))
    _lib.call('l2i_fused_bias_act_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(dev(kw.get('b'))), _lib.fptr(ref), n, kw['step_b'], kw['size_b'], kw['act'], kw['grad'],
              float(kw['alpha']), float(kw['scale']))
    torch.cuda.synchronize()
    assert untouched(ybuf, y)
    return {'y': y.cpu()}


def run_planes(row, kw, elem):
    dtype = sr.ELEM_DTYPES[elem]
    B, CinP, KK, CoutP = row.shape
    pbuf, planes = guarded((B,) + tuple(kw['w32'].shape), dtype)
    _lib.call('l2i_modulate_planes_h8', _lib.ptr(planes), _lib.fptr(dev(kw['w32'])), _lib.fptr(dev(kw['s'])), B, CinP, CinP, KK, CoutP, dtype=dtype)
    torch.cuda.synchronize()
    assert untouched(pbuf, planes)
    return {'planes': planes.cpu()}


def run_planes_multi(row, kw, elem):
    dtype = sr.ELEM_DTYPES[elem]
    B, layers = row.shape[0], kw['layers']
    table, nblocks = fr.multi_table(layers, B, row.extra['spread'])
    w32 = dev(torch.cat([L['w32'].reshape(-1) for L in layers]))
    s = dev(torch.cat([L['s'].reshape(-1) for L in layers]))
    total = sum(L['w32'].numel() * B for L in layers)
    pbuf, planes = guarded((total,), dtype)
    _lib.call('l2i_modulate_planes_multi_h8', _lib.ptr(planes), _lib.fptr(w32), _lib.fptr(s), _lib.ptr(dev(torch.tensor(table, dtype=torch.int64))), len(layers), B, nblocks,
              dtype=dtype)
    torch.cuda.synchronize()
    assert untouched(pbuf, planes)
    out, flat = {}, planes.cpu()
    for i, (L, t) in enumerate(zip(layers, table)):
        out['planes%d' % i] = flat[t[2] * 8:t[2] * 8 + L['w32'].numel() * B].view((B,) + tuple(L['w32'].shape))
    return out


def run(row, kw, elem):
    if row.op == 'fir':
        return run_fir_f32(row, kw) if row.kind == 'f32' else run_fir_h8(row, kw, elem)
    return {'fba': lambda: run_fba(row, kw), 'planes': lambda: run_planes(row, kw, elem), 'planes_multi': lambda: run_planes_multi(row, kw, elem)}[row.op]()


@pytest.mark.parametrize('row,elem', PARAMS, ids=['%s-%s' % (r.id, e) for r, e in PARAMS])
def test_kernel_against_the_model(row, elem):
    assert fr.row_path(row) == row.path
    kw = fr.make_inputs(row, elem)
    exp = fr.expected(row, kw, elem)
    got = run(row, kw, elem)
    assert set(got) >= set(exp), (sorted(got), sorted(exp))
    for name, (want, bound) in exp.items():
        if bound is None and want.dtype in sr.ELEM_DTYPES.values():          # an exact 16-bit output: the same bits, the sign of a zero included
            ok = torch.equal(got[name].view(torch.int16), want.view(torch.int16))
            _LOG.append('%s %s %s bits %s' % (row.id, elem, name, 'equal' if ok else 'DIFFERENT'))
            assert ok, _LOG[-1]
    compare(row, elem, got, exp, _LOG)
    twin = row.extra.get('twin')
    if twin:                                               # the code claims the two kernels give the same bits on the same data
        base = fr.row_by_id(twin)
        if (twin, elem) not in _RESULTS:
            _RESULTS[(twin, elem)] = run(base, fr.make_inputs(base, elem), elem)['y']
        ok = fr.twin_valid(row, base)
        assert int(ok.sum()) * 2 > ok.numel(), 'a twin shares most of its outputs with the launch it is the twin of'
        a, b = got['y'], _RESULTS[(twin, elem)]
        h, w = min(a.shape[-2], b.shape[-2]), min(a.shape[-1], b.shape[-1])
        okc = ok[:h, :w]
        same = torch.equal(a[..., :h, :w][..., okc], b[..., :h, :w][..., okc])
        _LOG.append('%s %s y twin_of %s %s' % (row.id, elem, twin, 'same bits' if same else 'DIFFERENT BITS'))
        assert same, _LOG[-1]


def test_fused_bias_act_of_nothing_is_ok_and_touches_nothing():
    ybuf, y = guarded((8,))
    x = dev(torch.ones(8))
    assert _lib.call('l2i_fused_bias_act_f32', _lib.fptr(y), _lib.fptr(x), None, None, 0, 1, 1, 3, 0, 0.2, 1.0) == 'l2i_fused_bias_act_f32'
    assert _lib.call('l2i_fused_bias_act_f32', None, None, None, None, 0, 0, 0, 3, 0, 0.2, 1.0)          # n = 0 is decided before anything else
    torch.cuda.synchronize()
    assert untouched(ybuf)


# ---- refusals: the code, the message of the very line, and outputs that still hold the sentinel -----------------------------------------------------------
def refused(message, name, args, outs, dtype=None):
    with pytest.raises(_lib.L2IError, match=r'failed \(%d\): .*%s' % (fr.REFUSAL_CODE[message], re.escape(message))):
        _lib.call(name, *args, dtype=dtype)
    torch.cuda.synchronize()
    assert all(untouched(b) for b in outs), (name, message)


def _cases(prefix):
    return [(m, c) for m, cs in fr.REFUSALS.items() if m.startswith(prefix) for c in cs]


@pytest.mark.parametrize('message,case', _cases('fused_bias_act:'))
def test_fused_bias_act_refusals(message, case):
    ybuf, y = guarded((8,))
    a = dict(y=_lib.fptr(y), x=_lib.fptr(dev(torch.ones(8))), b=_lib.fptr(dev(torch.ones(2))), n=8, step_b=4, size_b=2)
    a.update({'y_null': dict(y=None), 'x_null': dict(x=None), 'n_negative': dict(n=-4), 'step_b_zero': dict(step_b=0), 'size_b_zero': dict(size_b=0)}[case])
    refused(message, 'l2i_fused_bias_act_f32', [a['y'], a['x'], a['b'], None, a['n'], a['step_b'], a['size_b'], 3, 0, 0.2, 1.0], [ybuf])


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('message,case', _cases('upfirdn2d:'))
def test_upfirdn2d_f32_refusals(message, case, masked):
    ybuf, y = guarded((2, 16, 16))
    a = dict(y=_lib.fptr(y), x=_lib.fptr(dev(torch.ones(2, 6, 6))), k=_lib.fptr(dev(torch.ones(80))), major=2, in_h=6, in_w=6, kh=4, kw=4, up_x=1, up_y=1, down_x=1,
             down_y=1, px0=1, px1=2, py0=1, py1=2)
    a.update({'y_null': dict(y=None), 'x_null': dict(x=None), 'k_null': dict(k=None), 'major_zero': dict(major=0), 'in_h_zero': dict(in_h=0), 'in_w_zero': dict(in_w=0),
              'kh_zero': dict(kh=0), 'kw_zero': dict(kw=0), 'taps_65': dict(kh=5, kw=13), 'up_x_zero': dict(up_x=0), 'up_y_zero': dict(up_y=0),
              'down_x_zero': dict(down_x=0), 'down_y_zero': dict(down_y=0), 'out_h_zero': dict(py0=-4, py1=-4), 'out_w_zero': dict(px0=-4, px1=-4)}[case])
    args = [a['y'], a['x'], a['k'], a['major'], a['in_h'], a['in_w'], a['kh'], a['kw'], a['up_x'], a['up_y'], a['down_x'], a['down_y'], a['px0'], a['px1'], a['py0'],
            a['py1'], 1, None, 0.0, None, None, 0, 0.2, 1.0]
    if masked:
        refused(message, 'l2i_upfirdn2d_masked_f32', args + [_lib.fptr(dev(torch.ones(2, 16, 16))), 1.0, 0.0], [ybuf])
    else:
        refused(message, 'l2i_upfirdn2d_f32', args, [ybuf])


@pytest.mark.parametrize('elem', ['bf16', 'f16'])
@pytest.mark.parametrize('message,case', _cases('upfirdn2d_h8:'))
def test_upfirdn2d_h8_refusals(message, case, elem):
    dtype = sr.ELEM_DTYPES[elem]
    ybuf, y = guarded((1, 1, 8, 8, 8), dtype)
    k1 = (ctypes.c_float * 4)(1.0, 0.5, 0.25, 0.125)
    bits = case.startswith('bits_')
    a = dict(y=_lib.ptr(y), x=_lib.ptr(dev(torch.ones(1, 1, 4, 4, 8, dtype=dtype))), k=_lib.fptr(dev(torch.ones(4, 4))), planes=1, channels=8, in_h=4, in_w=4, kh=4, kw=4,
             up=1, down=1, px0=1, px1=2, py0=1, py1=2, mask=_lib.ptr(dev(torch.zeros(1, 1, 8, 8, dtype=torch.uint8))) if bits else None, k1y=k1, k1x=k1)
    a.update({'y_null': dict(y=None), 'x_null': dict(x=None), 'k_null': dict(k=None), 'bits_up2': dict(up=2), 'bits_down2': dict(down=2), 'bits_no_k1': dict(k1y=None),
              'bits_k3': dict(kh=3), 'bits_mask_null': dict(mask=None), 'planes_zero': dict(planes=0), 'channels_zero': dict(channels=0), 'channels_12': dict(channels=12),
              'in_h_zero': dict(in_h=0), 'in_w_zero': dict(in_w=0), 'kh_zero': dict(kh=0), 'kw_5': dict(kw=5), 'up_3': dict(up=3), 'down_0': dict(down=0),
              'out_h_zero': dict(py0=-3, py1=-3), 'out_w_zero': dict(px0=-3, px1=-3)}[case])
    refused(message, 'l2i_upfirdn2d_h8', [a['y'], a['x'], a['k'], a['planes'], a['channels'], a['in_h'], a['in_w'], a['kh'], a['kw'], a['up'], a['down'], a['px0'], a['px1'],
                                          a['py0'], a['py1'], None, 0.0, None, 0, 0.2, 1.0, a['mask'], 1.0, 0.0, None, a['k1y'], a['k1x'], int(bits)], [ybuf], dtype=dtype)


@pytest.mark.parametrize('elem', ['bf16', 'f16'])
@pytest.mark.parametrize('message,case', _cases('modulate_planes_h8:'))
def test_modulate_planes_refusals(message, case, elem):
    dtype = sr.ELEM_DTYPES[elem]
    pbuf, planes = guarded((2, 2, 1, 2, 8, 8), dtype, off=2 if case == 'planes_off' else 0)
    wbuf = dev(torch.ones(2 * 2 * 8 * 8 + 4))
    w32 = wbuf[1:] if case == 'w32_off' else wbuf
    a = dict(planes=_lib.ptr(planes), w32=ctypes.c_void_p(w32.data_ptr()), s=_lib.fptr(dev(torch.ones(2, 32))), B=1, Cs=16, CinP=16, KK=1, CoutP=8)
    a.update({'planes_null': dict(planes=None), 'w32_null': dict(w32=None), 's_null': dict(s=None), 'B_zero': dict(B=0), 'CinP_zero': dict(CinP=0, Cs=0),
              'CinP_24': dict(CinP=24, Cs=24), 'Cs_above': dict(Cs=32), 'KK_zero': dict(KK=0), 'CoutP_zero': dict(CoutP=0), 'Cs_below': dict(Cs=8), 'w32_off': {},
              'planes_off': {}}[case])
    refused(message, 'l2i_modulate_planes_h8', [a['planes'], a['w32'], a['s'], a['B'], a['Cs'], a['CinP'], a['KK'], a['CoutP']], [pbuf], dtype=dtype)


@pytest.mark.parametrize('elem', ['bf16', 'f16'])
@pytest.mark.parametrize('message,case', _cases('modulate_planes_multi_h8:'))
def test_modulate_planes_multi_refusals(message, case, elem):
    dtype = sr.ELEM_DTYPES[elem]
    pbuf, planes = guarded((2, 1, 1, 2, 8, 8), dtype)
    table = dev(torch.tensor([[0, 0, 0, 16, 1, 8, 16, 0], [0, 0, 16, 16, 1, 8, 16, 1]], dtype=torch.int64))
    a = dict(planes=_lib.ptr(planes), w32=_lib.fptr(dev(torch.ones(1, 1, 2, 8, 8))), s=_lib.fptr(dev(torch.ones(1, 16))), table=_lib.ptr(table), nseg=2, B=1, nblocks=2)
    a.update({'planes_null': dict(planes=None), 'w32_null': dict(w32=None), 's_null': dict(s=None), 'table_null': dict(table=None), 'nseg_zero': dict(nseg=0),
              'B_zero': dict(B=0), 'nblocks_below_nseg': dict(nblocks=1)}[case])
    refused(message, 'l2i_modulate_planes_multi_h8', [a['planes'], a['w32'], a['s'], a['table'], a['nseg'], a['B'], a['nblocks']], [pbuf], dtype=dtype)
