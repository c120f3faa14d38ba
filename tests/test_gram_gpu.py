"""l2i_gram_loss_f32 / l2i_gram_bwd_f32 against the float64 model of tests/gram_ref.py, at the model's shapes, with and without a target,
with and without accumulate and scale.  Bounds (gram_ref.gram_bound / loss_bound / bwd_bound) are any-order summation bounds, so they do
not depend on how the kernels slice or tile; the observed errors are written beside them to profiles/gram_contract_errors.txt."""
import os

import numpy as np
import pytest
import torch

from tests import gram_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cases = {}
_report = {}


def _case(shape):
    """Inputs and model outputs of one shape, computed once and shared (read-only) by the tests."""
    if shape not in _cases:
        case = R.make_case(shape)
        case['fwd'] = R.gram_loss(case['c'], case['gt'])
        _cases[shape] = case
    return _cases[shape]


def _dev(a, shape=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if shape is None else t.reshape(shape)


def _worst(err, bound):
    """max err / bound over the entries (0 / 0 = 0: an entry with a zero bound must be exact)."""
    ratio = np.where(err > 0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny), 0.0)
    return float(ratio.max())


def _note(key, err, bound):
    _report[key] = (float(np.max(err)), float(np.max(bound)), _worst(err, bound))


@pytest.fixture(scope='module', autouse=True)
def _write_report():
    yield
    if not _report:
        return
    lines = ['# l2i_gram_loss_f32 / l2i_gram_bwd_f32 against tests/gram_ref.py (float64): largest |error|, largest bound, largest error / bound',
             '# written by tests/test_gram_gpu.py; every ratio must be <= 1']
    for key in sorted(_report):
        e, b, r = _report[key]
        lines.append('%-58s max_err %.3e  max_bound %.3e  worst_ratio %.4f' % (key, e, b, r))
    with open(os.path.join(ROOT, 'profiles', 'gram_contract_errors.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


@pytest.mark.parametrize('with_target', [False, True], ids=['grams_only', 'target'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_gram_loss(shape, with_target):
    from latent2im_amd import kernels as K
    b, ch, h, w = shape
    case = _case(shape)
    ref = case['fwd']
    c = _dev(case['c'], (b, ch, h, w))
    if not with_target:
        G = K.gram_loss(c)
    else:
        G, D, loss = K.gram_loss(c, _dev(case['gt']))
    G = G.cpu().numpy().astype(np.float64)
    assert np.array_equal(G, G.transpose(0, 2, 1)), 'G is not symmetric to the bit'
    err, bound = np.abs(G - ref['G']), R.gram_bound(ref, h * w)
    _note('G    %s %s' % (shape, 'target' if with_target else 'grams_only'), err, bound)
    print('G', shape, err.max(), bound.max(), _worst(err, bound))
    assert (err <= bound).all(), _worst(err, bound)
    if with_target:
        D = D.cpu().numpy().astype(np.float64)
        loss = loss.cpu().numpy().astype(np.float64)
        assert np.array_equal(D, D.transpose(0, 2, 1))
        derr = np.abs(D - ref['D'])
        dbound = bound + R.U * (np.abs(ref['D']) + bound)
        _note('D    %s' % (shape,), derr, dbound)
        assert (derr <= dbound).all(), _worst(derr, dbound)
        lerr, lbound = np.abs(loss - ref['loss']), R.loss_bound(ref, ch, h * w, case['gt'])
        _note('loss %s' % (shape,), lerr, lbound)
        print('loss', shape, loss, ref['loss'], lerr, lbound)
        assert (lerr <= lbound).all(), (lerr, lbound)


@pytest.mark.parametrize('scale', [None, 'scale', 'scale_b'], ids=['unit', 'scale', 'scale_per_sample'])
@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_gram_bwd(shape, accumulate, scale):
    from latent2im_amd import kernels as K
    b, ch, h, w = shape
    case = _case(shape)
    sc = case[scale] if scale else None
    g0 = case['g0'] if accumulate else None
    ref = R.gram_bwd(case['c'], case['d'], scale=sc, g0=g0)
    c = _dev(case['c'], (b, ch, h, w))
    if accumulate:
        out = _dev(case['g0'], (b, ch, h, w)).clone()
    else:
        out = torch.full((b, ch, h, w), float('nan'), device='cuda')        # an overwriting launch must write every element
    got = K.gram_bwd(c, _dev(case['d']), scale=None if sc is None else _dev(sc), out=out, accumulate=accumulate)
    got = got.cpu().numpy().astype(np.float64).reshape(b, ch, h * w)
    err, bound = np.abs(got - ref['g']), R.bwd_bound(ref, ch, g0)
    _note('g    %s %s %s' % (shape, 'accumulate' if accumulate else 'write', scale or 'unit'), err, bound)
    print('g', shape, err.max(), bound.max(), _worst(err, bound))
    assert np.isfinite(got).all()
    assert (err <= bound).all(), _worst(err, bound)


@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_two_runs_identical_bits(shape):
    from latent2im_amd import kernels as K
    b, ch, h, w = shape
    case = _case(shape)
    c, gt, g0, sc = _dev(case['c'], (b, ch, h, w)), _dev(case['gt']), _dev(case['g0'], (b, ch, h, w)), _dev(case['scale_b'])
    runs = []
    for _ in range(2):
        G, D, loss = K.gram_loss(c, gt)
        g = K.gram_bwd(c, D, scale=sc, out=g0.clone(), accumulate=True)
        runs.append([t.cpu().numpy().view(np.uint32) for t in (G, D, loss, g)])
    for a, b_ in zip(*runs):
        assert np.array_equal(a, b_)


@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_target_equal_to_input_is_a_fixed_point(shape):
    """D = 0, a loss of exactly 0 and a zero gradient when the target's Grams are the input's own."""
    from latent2im_amd import kernels as K
    b, ch, h, w = shape
    c = _dev(_case(shape)['c'], (b, ch, h, w))
    gt = K.gram_loss(c)
    G, D, loss = K.gram_loss(c, gt)
    assert torch.equal(G, gt)
    assert not D.any() and not loss.any()
    g = K.gram_bwd(c, D, out=torch.full_like(c, float('nan')))
    assert not g.any()


@pytest.mark.parametrize('ch', [48, 544, 16])
def test_refusals(ch):
    """C % 32 != 0 and C > 512 are refused with L2I_E_UNSUPPORTED (-3) before a launch: nothing is written."""
    from latent2im_amd import _lib
    from latent2im_amd import kernels as K
    c = torch.randn(1, ch, 4, 4, device='cuda')
    out = torch.full_like(c, 7.0)
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_bwd_f32 failed \(-3\)'):
        K.gram_bwd(c, torch.zeros(1, ch, ch, device='cuda'), out=out)
    assert bool((out == 7.0).all())
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_loss_f32 failed \(-3\)'):
        K.gram_loss(c)
    with pytest.raises(_lib.L2IError, match=r'l2i_gram_loss_f32 failed \(-3\)'):
        K.gram_loss(c, torch.zeros(1, ch, ch, device='cuda'))
