"""perceptual16.Vgg16Gram16 and invert.Inverter on the 16-bit networks (bf16 and fp16 elements) against the storage-rounding model of
tests/inversion16_ref.py, and the host side of `BP.py --precision`.

Tolerances are measured against the reference alone (inversion16_ref.measure): the model run three times with a 1e-7 relative perturbation before
every rounding and with rounded gradient maps, against its unperturbed self; the GPU may deviate by max(2 x that spread, the deviation rounded
gradient maps cause alone) — the factor 2 is the project's own rule (tests/test_inversion_gpu.py: own_rule) — and a loss by at least 1e-3.  The
spread itself must pass 1 - cos <= 5e-3 (image gradient) and 1e-3 (loss), else the inputs are ill-conditioned.  Spreads, GPU deviations and the
distance of the rounding model to the exact float64 model (the price of the format) go to profiles/invert16_parity.txt.
"""
import os

import numpy as np
import pytest
import torch

from tests import inversion16_ref as R16
from tests import inversion_ref as IR
from tests.test_inversion_gpu import _images, _setup, _vgg_states

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ('f16', 'bf16')


def _log2(dt, size, batch):
    """The committed static exponents the fp16 path rounds its gradient maps under (bf16 is unscaled)."""
    from latent2im_amd import nets16
    return nets16.invert_scale_for(size, batch) if dt == 'f16' else None
_memo = {}
_report = []


@pytest.fixture
def precision(monkeypatch):
    """Sets conv.PRECISION for the networks a test builds (restored afterwards)."""
    from latent2im_amd import conv

    def use(dt):
        monkeypatch.setattr(conv, 'PRECISION', dt)
        return R16.TORCH[dt]
    monkeypatch.setattr(conv, 'PRECISION', conv.PRECISION)
    return use


@pytest.fixture(scope='module', autouse=True)
def _write_report():
    yield
    if not _report:
        return
    head = ['# 16-bit inversion path against tests/inversion16_ref.py (float64 with the storage rounding restated); written by tests/test_inversion16_gpu.py',
            '# per quantity and figure: spread = the model perturbed (1e-7 before each rounding, rounded gradient maps; 3 draws) against itself, gradq = rounded',
            '# gradient maps alone, allowed = max(2 x spread, gradq[, 1e-3 for a loss]), gpu = the GPU against the unperturbed model, exact = the rounding',
            '# model against the exact float64 model of tests/inversion_ref.py (the price of the format)']
    with open(os.path.join(ROOT, 'profiles', 'invert16_parity.txt'), 'w') as f:
        f.write('\n'.join(head + sorted(_report)) + '\n')


def _check(what, m, got, cap=False):
    """Every figure of every quantity in ``got`` (name -> GPU tensor) against the measured model ``m``; prints and records before it asserts.
    ``cap``: the model's own spread must pass SPREAD_CAP (the VGG-16 loss and image gradient, where the condition is stated)."""
    bad, devs = [], {}
    for name, t in got.items():
        is_loss = name.startswith('loss')
        dev = devs[name] = R16.deviation(t, m['base'][name], is_loss)
        for fig, v in dev.items():
            a = R16.allowed(m, name, fig)
            line = '%-34s %-8s %-13s spread %.3e  gradq %.3e  allowed %.3e  gpu %.3e  exact %.3e' % (
                what, name, fig, m['spread'][name][fig], m['gradq'][name][fig], a, v, m['exact'][name][fig])
            print(line)
            _report.append(line)
            if cap and fig in R16.SPREAD_CAP:
                assert m['spread'][name][fig] <= R16.SPREAD_CAP[fig], ('the model\'s own spread is too wide: wrong inputs', line)
            if not v <= a:
                bad.append(line)
    assert not bad, bad
    return devs


def _vgg_model(size, batch, dt):
    """Target 0.35 x uniform (D = G - Gt is then no small difference of equals), image uniform: the measured model, once per (shape, type)."""
    key = ('vgg', size, batch, dt)
    if key not in _memo:
        PV = _vgg_states()[1]
        target, img = _images(size, batch, 11 + size)
        target = 0.35 * target
        coef = torch.linspace(0.5, 1.5, batch, dtype=torch.float64)

        def run(R):
            x = img.clone().requires_grad_()
            loss = R16.perceptual_loss(PV, target, x, R)
            (g,) = torch.autograd.grad((loss * coef).sum(), x)
            return dict(loss=loss.detach(), g_img=g)
        _memo[key] = (target, img, coef, R16.measure(run, dt, _log2(dt, size, batch)))
    return _memo[key]


def _vgg16(dt, size, batch):
    from latent2im_amd import nets16, optim
    from latent2im_amd.perceptual16 import Vgg16Gram16
    net = Vgg16Gram16(_vgg_states()[0], device=DEV)
    if dt == 'f16':
        nets16.attach_scaler((net,), optim.LossScaler(nets16.invert_scale_for(size, batch), DEV))
    return net


@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('size,batch', [(32, 2), (64, 1)])
def test_vgg16_gram_loss_and_image_gradient(size, batch, dt, precision):
    T = precision(dt)
    target, img, coef, m = _vgg_model(size, batch, dt)
    net = _vgg16(dt, size, batch)
    assert net.dtype == T
    grams = net.target_grams(target.float().to(DEV))
    assert all(g.dtype == torch.float32 for g in grams)
    x = img.float().to(DEV).requires_grad_()
    loss = net.loss(x, grams)
    assert loss.shape == (batch,) and loss.dtype == torch.float32
    (loss * coef.float().to(DEV)).sum().backward()
    assert x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all())
    dev = _check('vgg16 %s %d^2 x %d' % (dt, size, batch), m, dict(loss=loss, g_img=x.grad), cap=True)
    assert dev['g_img']['one_minus_cos'] < 1e-2           # (whatever the allowance: a wrong halo or a lost tap is far beyond this)


def _inverter(s, size, dt, lr=0.01, optim='Adam', batch=1):
    from latent2im_amd import nets16
    from latent2im_amd.invert import Inverter
    from latent2im_amd.perceptual16 import Vgg16Gram16
    gen = nets16.Generator(s['stG'], size, device=DEV)
    return Inverter(gen, Vgg16Gram16(_vgg_states()[0], device=DEV), lr=lr, optim=optim, n_mean_latent=64, batch=batch)


def _step_model(size, batch, dt):
    """One iteration from _setup's start latent towards the 0.35 x uniform target of the VGG test: (target, measured model)."""
    key = ('step', size, batch, dt)
    if key not in _memo:
        s = _setup(size, batch)
        PV = _vgg_states()[1]
        target = 0.35 * _images(size, batch, 11 + size)[0]

        def run(R):
            w = s['w0'].clone().requires_grad_()
            loss, out = R16.total_loss(s['P64'], PV, w, target, s['noise'], R)
            (g,) = torch.autograd.grad(loss, w)
            return dict(loss=loss.detach().reshape(1), g_w=g, image=out.detach())
        m = R16.measure(run, dt, _log2(dt, size, batch))
        image = m['base'].pop('image')                    # the generator's image: recorded beside the rest, not held to the rule
        _memo[key] = (target, m, image)
    return _memo[key]


@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('size,batch', [(32, 2), (64, 1)])
def test_one_inversion_step(size, batch, dt, precision):
    precision(dt)
    s = _setup(size, batch)
    target, m, image = _step_model(size, batch, dt)
    inv = _inverter(s, size, dt, batch=batch)
    assert (inv.scaler is not None) == (dt == 'f16')
    tgt = target.float().to(DEV)
    w = s['w0'].float().to(DEV).requires_grad_()
    loss, out = inv.loss(w, tgt, inv.vgg.target_grams(tgt), [n.float().to(DEV) for n in s['noise']])
    loss.backward()
    assert w.grad.dtype == torch.float32 and bool(torch.isfinite(w.grad).all())
    print('step  %s %d^2 x %d: image max |GPU - model| %.3e of max |image| %.3e' % (dt, size, batch, float((out.detach().cpu().double() - image).abs().max()),
                                                                                   float(image.abs().max())))
    dev = _check('step  %s %d^2 x %d' % (dt, size, batch), m, dict(loss=loss.reshape(1), g_w=w.grad))
    # the 16-bit contract the walk gradient already has (tests/test_h8_gpu.py), here against the rounding model
    assert 1.0 - dev['g_w']['one_minus_cos'] > 0.998 and dev['g_w']['rel_l2'] < 0.06, dev


@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
def test_three_guarded_adam_steps(dt, precision):
    precision(dt)
    size, n = 32, 3
    s = _setup(size)
    key = ('adam', dt)
    if key not in _memo:
        PV = _vgg_states()[1]
        _memo[key] = R16.measure(lambda R: dict(loss_curve=R16.adam_run(s['P64'], PV, s['w0'], s['target'], s['noise'], n, 0.01, R)), dt, _log2(dt, size, 1))
    m = _memo[key]
    inv = _inverter(s, size, dt, lr=0.01)
    w, curve = inv.invert(s['target'].float().to(DEV), n, noise=[t.float().to(DEV) for t in s['noise']], w=s['w0'].float().to(DEV))
    assert w.shape == s['w0'].shape and w.dtype == torch.float32 and curve.shape == (n,)
    print('model curve', m['base']['loss_curve'].tolist(), 'GPU', curve.tolist())
    _check('adam3 %s %d^2' % (dt, size), m, dict(loss_curve=torch.from_numpy(curve)))
    assert curve[-1] < curve[0]
    if dt == 'f16':
        st = inv.scaler.stats()
        assert st['skipped'] == 0 and st['steps'] == n, st


@pytest.mark.gpu
def test_f16_overflow_skips_the_iteration(precision, monkeypatch):
    """Exponents 20 octaves too high: the gradient maps overflow, the iteration is skipped, W+ keeps its bits, the dynamic scale halves."""
    from latent2im_amd import nets16
    precision('f16')
    real = nets16.invert_scale_for
    monkeypatch.setattr(nets16, 'invert_scale_for', lambda r, b: {k: v + 20 for k, v in real(r, b).items()})
    s = _setup(32)
    inv = _inverter(s, 32, 'f16')
    assert inv.scaler.log2 == {k: v + 20 for k, v in real(32, 1).items()}
    w0 = s['w0'].float().to(DEV)
    w, curve = inv.invert(s['target'].float().to(DEV), 1, noise=[t.float().to(DEV) for t in s['noise']], w=w0)
    st = inv.scaler.stats()
    assert st['skipped'] == 1 and st['scale'] == 0.5, st
    assert torch.equal(w, w0) and bool(torch.isfinite(w).all())


@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
def test_no_conv2d_or_bmm_on_the_path(dt, precision, monkeypatch):
    import torch.nn.functional as F
    precision(dt)
    s = _setup(32)
    inv = _inverter(s, 32, dt)

    def refuse(*a, **k):
        raise AssertionError('F.conv2d / torch.bmm on the inversion path')
    monkeypatch.setattr(F, 'conv2d', refuse)
    monkeypatch.setattr(torch, 'bmm', refuse)
    monkeypatch.setattr(torch.Tensor, 'bmm', refuse)
    w, curve = inv.invert(s['target'].float().to(DEV), 1)           # noise drawn
    assert np.isfinite(curve).all() and w.shape == (1, inv.gen.n_latent, 512)


@pytest.mark.gpu
def test_f16_with_gd_is_refused(precision):
    precision('f16')
    with pytest.raises(NotImplementedError, match='guarded SGD'):
        _inverter(_setup(32), 32, 'f16', optim='GD')


@pytest.mark.gpu
def test_bf16_takes_gd(precision):
    precision('bf16')
    s = _setup(32)
    inv = _inverter(s, 32, 'bf16', lr=1e-7, optim='GD')
    w, curve = inv.invert(s['target'].float().to(DEV), 2, w=s['w0'].float().to(DEV))
    assert inv.scaler is None and np.isfinite(curve).all() and bool(torch.isfinite(w).all())


@pytest.mark.gpu
def test_bp_main_precision_f16_writes_the_fp32_files(tmp_path, precision, monkeypatch):
    from PIL import Image
    from latent2im_amd import bp, constants
    precision('f16')                                               # (bp.main sets conv.PRECISION itself: this only restores it afterwards)
    monkeypatch.setattr(constants, 'ALLOW_SYNTHETIC_WEIGHTS', constants.ALLOW_SYNTHETIC_WEIGHTS)
    r = np.random.RandomState(3)
    os.makedirs(tmp_path / 'data' / 'a')
    for i in range(2):
        Image.fromarray(r.randint(0, 255, (40, 36, 3)).astype(np.uint8)).save(tmp_path / 'data' / 'a' / ('%d.png' % i))
    listing = {}
    for prec in ('f32', 'f16'):
        out = tmp_path / prec
        curve = bp.main(['--path', str(tmp_path / 'data'), '--save_path', str(out), '--resolution', '32', '--batch_size', '2', '--n_loops', '2',
                         '--synthetic_weights', '--precision', prec])
        assert curve.shape == (2,) and np.isfinite(curve).all()
        listing[prec] = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert listing['f16'] == listing['f32'] and 'latent/0_w.npy' in listing['f16']
    w = np.load(tmp_path / 'f16' / 'latent' / '0_w.npy')
    assert w.dtype == np.float32 and w.shape == (2, 8, 512) and np.isfinite(w).all()
    with pytest.raises(SystemExit):
        bp.main(['--path', str(tmp_path / 'data'), '--precision', 'f64'])
