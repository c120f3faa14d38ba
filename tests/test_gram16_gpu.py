"""l2i_gram_loss_h8 / l2i_gram_bwd_h8 (bf16 and fp16 elements) against the float64 model of tests/gram16_ref.py at gram_ref's five shapes: with and
without a target; write and accumulate; unit, scalar and per-sample scale; the fp16 row with D * 2^-18 under a scale of 2^18.  Bounds are the
derived ones of gram16_ref; observed error / bound per row goes to profiles/gram16_contract_errors.txt."""
import os

import numpy as np
import pytest
import torch

from tests import gram16_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cases = {}
_report = {}


def _case(shape, dt):
    """Inputs and forward model of one (shape, element type), computed once and shared (read-only) by the tests."""
    if (shape, dt) not in _cases:
        case = R.make_case(shape, dt)
        case['fwd'] = R.gram_loss(case['c'], case['gt'])
        _cases[(shape, dt)] = case
    return _cases[(shape, dt)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _h8(a, shape, dt):
    """[B, C, HW] float32 holding element-type values -> the h8 device tensor [B, C/8, H, W, 8] (exact conversion)."""
    b, ch, h, w = shape
    t = torch.from_numpy(R.pack_h8(a)).to(R.TORCH[dt]).reshape(b, ch // 8, h, w, 8).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _from_h8(t):
    b, g8, h, w, _ = t.shape
    return R.unpack_h8(t.float().cpu().numpy().reshape(b, g8, h * w, 8)).astype(np.float64)


def _worst(err, bound):
    ratio = np.where(err > 0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny), 0.0)
    return float(ratio.max())


def _note(key, err, bound):
    _report[key] = (float(np.max(err)), float(np.max(bound)), _worst(err, bound))


@pytest.fixture(scope='module', autouse=True)
def _write_report():
    yield
    if not _report:
        return
    lines = ['# l2i_gram_loss_h8 / l2i_gram_bwd_h8 (and _f16) against tests/gram16_ref.py (float64 on rounded inputs): largest |error|, largest bound,',
             '# largest error / bound.  Written by tests/test_gram16_gpu.py; every ratio must be <= 1.  The G / D / loss bounds are gram_ref\'s fp32',
             '# any-order summation bounds with unit 2^-24, unchanged: the 16-bit MFMA\'s fp32 accumulation is held to the same unit as the fp32 MFMA\'s.']
    for key in sorted(_report):
        e, b, r = _report[key]
        lines.append('%-66s max_err %.3e  max_bound %.3e  worst_ratio %.4f' % (key, e, b, r))
    with open(os.path.join(ROOT, 'profiles', 'gram16_contract_errors.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


@pytest.mark.parametrize('with_target', [False, True], ids=['grams_only', 'target'])
@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_gram_loss(shape, dt, with_target):
    from latent2im_amd import kernels16 as K
    b, ch, h, w = shape
    case = _case(shape, dt)
    ref = case['fwd']
    c = _h8(case['c'], shape, dt)
    if not with_target:
        G = K.gram_loss(c)
    else:
        G, D, loss = K.gram_loss(c, _dev(case['gt']))
    G = G.cpu().numpy().astype(np.float64)
    assert np.array_equal(G, G.transpose(0, 2, 1)), 'G is not symmetric to the bit'
    err, bound = np.abs(G - ref['G']), R.gram_bound(ref, h * w)
    _note('%-4s G    %s %s' % (dt, shape, 'target' if with_target else 'grams_only'), err, bound)
    print('G', dt, shape, err.max(), bound.max(), _worst(err, bound))
    assert (err <= bound).all(), _worst(err, bound)
    if with_target:
        D = D.cpu().numpy().astype(np.float64)
        loss = loss.cpu().numpy().astype(np.float64)
        assert np.array_equal(D, D.transpose(0, 2, 1)), 'D is not symmetric to the bit'
        derr = np.abs(D - ref['D'])
        dbound = bound + 2.0 ** -24 * (np.abs(ref['D']) + bound)
        _note('%-4s D    %s' % (dt, shape), derr, dbound)
        assert (derr <= dbound).all(), _worst(derr, dbound)
        lerr, lbound = np.abs(loss - ref['loss']), R.loss_bound(ref, ch, h * w, case['gt'])
        _note('%-4s loss %s' % (dt, shape), lerr, lbound)
        print('loss', dt, shape, loss, ref['loss'], lerr, lbound)
        assert (lerr <= lbound).all(), (lerr, lbound)


def _run_bwd(shape, dt, case, sc, accumulate):
    from latent2im_amd import kernels16 as K
    b, ch, h, w = shape
    c = _h8(case['c'], shape, dt)
    if accumulate:
        out = _h8(case['g0'], shape, dt)
    else:
        out = torch.full((b, ch // 8, h, w, 8), float('nan'), device='cuda', dtype=R.TORCH[dt])      # an overwriting launch must write every element
    got = K.gram_bwd(c, _dev(case['d']), scale=None if sc is None else _dev(sc), out=out, accumulate=accumulate)
    assert got.dtype == R.TORCH[dt] and got.shape == c.shape
    return _from_h8(got)


@pytest.mark.parametrize('scale', [None, 'scale', 'scale_b'], ids=['unit', 'scale', 'scale_per_sample'])
@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_gram_bwd(shape, dt, accumulate, scale):
    b, ch, h, w = shape
    case = _case(shape, dt)
    sc = case[scale] if scale else None
    g0 = case['g0'] if accumulate else None
    ref = R.gram_bwd(case['c'], case['d'], dt, scale=sc, g0=g0)
    got = _run_bwd(shape, dt, case, sc, accumulate)
    err, bound = np.abs(got - ref['g']), R.bwd_bound(ref, ch, dt, g0)
    _note('%-4s g    %s %s %s' % (dt, shape, 'accumulate' if accumulate else 'write', scale or 'unit'), err, bound)
    print('g', dt, shape, err.max(), bound.max(), _worst(err, bound))
    assert np.isfinite(got).all()
    assert (err <= bound).all(), _worst(err, bound)


@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_gram_bwd_f16_small_d_under_a_large_scale(shape):
    """D * 2^-18 is subnormal in fp16; coef * 2^18 * D is not: the scaling comes first, in fp32."""
    b, ch, h, w = shape
    case = R.small_d_case(_case(shape, 'f16'))
    ref = R.gram_bwd(case['c'], case['d'], 'f16', scale=case['scale'])
    got = _run_bwd(shape, 'f16', case, case['scale'], False)
    err, bound = np.abs(got - ref['g']), R.bwd_bound(ref, ch, 'f16')
    _note('f16  g    %s write small_d_scale_2^18' % (shape,), err, bound)
    assert (err <= bound).all(), _worst(err, bound)


@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_two_runs_identical_bits(shape, dt):
    from latent2im_amd import kernels16 as K
    case = _case(shape, dt)
    c, gt, sc = _h8(case['c'], shape, dt), _dev(case['gt']), _dev(case['scale_b'])
    runs = []
    for _ in range(2):
        G, D, loss = K.gram_loss(c, gt)
        g = K.gram_bwd(c, D, scale=sc, out=_h8(case['g0'], shape, dt), accumulate=True)
        runs.append([t.cpu().numpy().view(np.uint32) for t in (G, D, loss)] + [g.view(torch.int16).cpu().numpy()])
    for a, b_ in zip(*runs):
        assert np.array_equal(a, b_)


@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('ch', [48, 544])
def test_shape_refusals(ch, dt):
    """C % 32 != 0 and C > 512 return L2I_E_UNSUPPORTED (-3) before any launch: nothing is written."""
    from latent2im_amd import _lib
    from latent2im_amd import kernels16 as K
    tw = '_f16' if dt == 'f16' else ''
    c = torch.zeros(1, ch // 8, 4, 4, 8, device='cuda', dtype=R.TORCH[dt])
    out = torch.full_like(c, 7.0)
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_bwd_h8%s failed \(-3\)' % tw):
        K.gram_bwd(c, torch.zeros(1, ch, ch, device='cuda'), out=out)
    assert bool((out == 7.0).all())
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_loss_h8%s failed \(-3\)' % tw):
        K.gram_loss(c)
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_loss_h8%s failed \(-3\)' % tw):
        K.gram_loss(c, torch.zeros(1, ch, ch, device='cuda'))


@pytest.mark.parametrize('dt', R.DTYPES)
def test_misaligned_pointer_is_refused(dt):
    """A tap or a gradient 2 bytes off a 16-byte boundary returns L2I_E_ARG (-1) before any launch: nothing is written."""
    from latent2im_amd import _lib
    tw = '_f16' if dt == 'f16' else ''
    b, ch, hw, T = 1, 32, 16, R.TORCH[dt]
    buf = torch.zeros(b * ch * hw + 8, device='cuda', dtype=T)
    out = torch.full((b * ch * hw + 8,), 7.0, device='cuda', dtype=T)
    off, ok, gout = buf[1:1 + b * ch * hw], buf[:b * ch * hw], out[1:1 + b * ch * hw]
    assert off.data_ptr() % 16 == 2 and ok.data_ptr() % 16 == 0
    G, ws, d = torch.full((b, ch, ch), 7.0, device='cuda'), torch.zeros(2048, device='cuda'), torch.zeros(b, ch, ch, device='cuda')
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_loss_h8%s failed \(-1\)' % tw):
        _lib.call('l2i_gram_loss_h8', _lib.ptr(G), None, None, _lib.ptr(off), None, _lib.ptr(ws), b, ch, hw, 1, dtype=T)
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_bwd_h8%s failed \(-1\)' % tw):
        _lib.call('l2i_gram_bwd_h8', _lib.ptr(gout), _lib.ptr(ok), _lib.ptr(d), None, 1.0, b, ch, hw, 0, 0, dtype=T)
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_bwd_h8%s failed \(-1\)' % tw):
        _lib.call('l2i_gram_bwd_h8', _lib.ptr(out[:b * ch * hw]), _lib.ptr(off), _lib.ptr(d), None, 1.0, b, ch, hw, 0, 0, dtype=T)
    assert bool((G == 7.0).all()) and bool((out == 7.0).all())
