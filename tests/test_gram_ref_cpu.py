"""tests/gram_ref.py (the float64 model of l2i_gram_loss_f32 / l2i_gram_bwd_f32) against BP.py's own expressions — gram (BP.py:68-73) and the
Gram term of perceptual_loss (BP.py:180-183) restated with torch.bmm in float64, autograd for the backward — and the mistake table: every
planted fault must break the comparison, by far more than the GPU contract's bound, at every shape where the fault can act."""
import numpy as np
import pytest
import torch

from tests import gram_ref as R


def _bp(c, gt):
    """BP.py's expressions on the post-ReLU tap, float64: (G, per-sample loss, d sum(scale * loss) / d c for scale = 1)."""
    c = torch.tensor(np.asarray(c, dtype=np.float64), requires_grad=True)
    x = torch.relu(c)
    bs, ch, hw = x.shape
    G = x.bmm(x.transpose(1, 2)) / (ch * hw)
    diff = torch.tensor(np.asarray(gt, dtype=np.float64)) - G
    loss = torch.sum(diff.pow(2), [1, 2]) * (ch * ch)
    (g,) = torch.autograd.grad(loss.sum(), c)
    return G.detach().numpy(), loss.detach().numpy(), g.numpy()


def _model(case, mistake=None):
    fwd = R.gram_loss(case['c'], case['gt'], mistake=mistake)
    good_d = R.gram_loss(case['c'], case['gt'])['D']        # the backward is judged on its own: it gets the right D
    plain = R.gram_bwd(case['c'], good_d, mistake=mistake)
    acc = R.gram_bwd(case['c'], good_d, scale=case['scale_b'], g0=case['g0'], mistake=mistake)
    return fwd, plain, acc


@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_model_is_bp(shape):
    case = R.make_case(shape)
    G, loss, g = _bp(case['c'], case['gt'])
    fwd, plain, acc = _model(case)
    np.testing.assert_allclose(fwd['G'], G, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(fwd['G'], fwd['G'].transpose(0, 2, 1), rtol=0, atol=0)
    np.testing.assert_allclose(fwd['loss'], loss, rtol=1e-11)
    np.testing.assert_allclose(plain['g'], g, rtol=1e-10, atol=1e-13 * np.abs(g).max())
    s = case['scale_b'].astype(np.float64).reshape(-1, 1, 1)               # one upstream gradient per sample
    np.testing.assert_allclose(acc['g'], case['g0'].astype(np.float64) + s * g, rtol=1e-10, atol=1e-12 * np.abs(g).max())


def _visible(shape, mistake):
    b, ch, h, w = shape
    if mistake == 'no_mirror':
        return ch > 32                       # one tile has no lower triangle of tiles
    if mistake == 'scale_of_sample_0':
        return b > 1                         # one sample has one scale
    return True


@pytest.mark.parametrize('shape,mistake', [(s, m) for s in R.SHAPES for m in R.MISTAKES if _visible(s, m)], ids=str)
def test_planted_mistake_breaks_the_contract(shape, mistake):
    """The deviation a planted fault causes, in units of the GPU contract's own bound, is >= 100 somewhere in the outputs it touches."""
    b, ch, h, w = shape
    case = R.make_case(shape)
    fwd, plain, acc = _model(case)
    bad_fwd, bad_plain, bad_acc = _model(case, mistake)
    worst = 0.0
    tiny = np.finfo(np.float64).tiny
    worst = max(worst, (np.abs(bad_fwd['G'] - fwd['G']) / (R.gram_bound(fwd, h * w) + tiny)).max())
    worst = max(worst, (np.abs(bad_fwd['loss'] - fwd['loss']) / (R.loss_bound(fwd, ch, h * w, case['gt']) + tiny)).max())
    worst = max(worst, (np.abs(bad_plain['g'] - plain['g']) / (R.bwd_bound(plain, ch) + tiny)).max())
    worst = max(worst, (np.abs(bad_acc['g'] - acc['g']) / (R.bwd_bound(acc, ch, case['g0']) + tiny)).max())
    assert worst >= 100.0, (mistake, shape, worst)


def test_every_mistake_acts_somewhere():
    for m in R.MISTAKES:
        assert any(_visible(s, m) for s in R.SHAPES), m
