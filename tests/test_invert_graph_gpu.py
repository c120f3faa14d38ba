"""invert.Inverter(capture=True): the inversion iteration replayed from a hipGraph — forward, backward, guarded optimiser update and loss record in
one graph.replay() — against the same CPU models and under the same rules as the eager loop (tests/test_inversion_gpu.py: the fp32 CPU model's own
deviation from float64; tests/test_inversion16_gpu.py: the storage-rounding model's measured spread), and `BP.py --hipgraph`.

Bit equality with the eager loop is not asked for: the generator's style-gradient reductions add across blocks in arrival order, so two eager runs
need not agree either."""
import os

import numpy as np
import pytest
import torch

from tests import inversion16_ref as R16
from tests import inversion_ref as IR
from tests.test_inversion16_gpu import _log2, _memo as _memo16
from tests.test_inversion_gpu import _setup, _vgg_states, own_rule

DEV = 'cuda'
pytestmark = pytest.mark.gpu
_memo = {}
SIZE = 32


@pytest.fixture
def precision(monkeypatch):
    """Sets conv.PRECISION for the networks a test builds (restored afterwards)."""
    from latent2im_amd import conv

    def use(dt):
        monkeypatch.setattr(conv, 'PRECISION', dt)
    monkeypatch.setattr(conv, 'PRECISION', conv.PRECISION)
    return use


def _inverter(dt='f32', lr=0.01, optim='Adam', batch=1, capture=True):
    """Both networks of one precision on _setup's synthetic weights (conv.PRECISION is the caller's: the ``precision`` fixture)."""
    from latent2im_amd.invert import Inverter
    s = _setup(SIZE, batch)
    if dt == 'f32':
        from latent2im_amd.generator import Generator
        from latent2im_amd.perceptual16 import Vgg16Gram
    else:
        from latent2im_amd.nets16 import Generator
        from latent2im_amd.perceptual16 import Vgg16Gram16 as Vgg16Gram
    return Inverter(Generator(s['stG'], SIZE, device=DEV), Vgg16Gram(_vgg_states()[0], device=DEV), lr=lr, optim=optim, n_mean_latent=64, batch=batch,
                    capture=capture)


def _gpu(s, target=None):
    return dict(batch=(s['target'] if target is None else target).float().to(DEV), noise=[t.float().to(DEV) for t in s['noise']], w=s['w0'].float().to(DEV))


def _sgd_run(total_loss, w0, n, lr):
    """BP.py:137-158 with torch.optim.SGD(lr, momentum=0.9) (BP.py:140) over ``total_loss(w)`` -> (curve [n], final W+)."""
    w = w0.detach().clone().requires_grad_()
    opt = torch.optim.SGD([w], lr=lr, momentum=0.9)
    curve = []
    for _ in range(n):
        loss, _ = total_loss(w)
        opt.zero_grad()
        loss.backward()
        opt.step()
        curve.append(loss.detach().reshape(1))
    return torch.cat(curve), w.detach()


def _ref32(kind, n, lr):
    """float64 and float32 CPU runs of ``n`` iterations from _setup's start latent, once per case: dict(c64, c32 [n], d64, d32 = W+ - start)."""
    key = (kind, n, lr)
    if key not in _memo:
        s = _setup(SIZE)
        _, V64, V32 = _vgg_states()
        out = {}
        for tag, dt, PG, PV in (('64', torch.float64, s['P64'], V64), ('32', torch.float32, s['P32'], V32)):
            tg = s['target'].to(dt)
            nz = [t.to(dt) for t in s['noise']]
            w0 = s['w0'].to(dt)
            if kind == 'adam':
                c, w = IR.adam_run(PG, PV, w0, tg, nz, n, lr)
                c = np.array(c)
            else:
                c, w = _sgd_run(lambda w_: IR.total_loss(PG, PV, w_, tg, nz), w0, n, lr)
                c = c.double().numpy()
            out['c' + tag], out['d' + tag] = c, w - w0
        _memo[key] = out
    return _memo[key]


def _hold32(what, ref, w, curve, w0):
    """test_ten_adam_steps's rule for the curve, own_rule for the displacement; prints before it asserts."""
    cpu_dev = np.abs(ref['c32'] - ref['c64']) / np.abs(ref['c64'])
    gpu_dev = np.abs(curve - ref['c64']) / np.abs(ref['c64'])
    print(what, 'float64 curve', ref['c64'].tolist())
    print(what, 'fp32 CPU per-step deviation', cpu_dev.tolist())
    print(what, 'GPU per-step deviation', gpu_dev.tolist())
    assert (gpu_dev <= np.maximum(2.0 * cpu_dev, 1e-3)).all(), (gpu_dev, cpu_dev)
    own_rule(w.detach().cpu().double() - w0.float().double(), ref['d64'], ref['d32'], what + ' displacement')


def test_f32_adam_ten_replays():
    n = 10
    s = _setup(SIZE)
    ref = _ref32('adam', n, 0.01)
    inv = _inverter(lr=0.01)
    w, curve = inv.invert(n_loops=n, **_gpu(s))
    assert w.shape == s['w0'].shape and w.dtype == torch.float32 and curve.shape == (n,) and curve.dtype == np.float64
    _hold32('adam f32 replayed', ref, w, curve, s['w0'])
    assert curve[-1] < curve[0]
    assert inv.last_image.shape == (1, 3, SIZE, SIZE) and bool(torch.isfinite(inv.last_image).all())
    from latent2im_amd.optim import GuardedAdam
    r = inv.graphs[1]
    assert isinstance(r.opt, GuardedAdam) and r.opt.scaler is None and r.capacity == 1024


def test_f32_gd_six_replays():
    n, lr = 6, 1e-9
    s = _setup(SIZE)
    ref = _ref32('gd', n, lr)
    assert (np.diff(ref['c64']) < 0).all(), ref['c64']                # at this lr the float64 curve falls monotonically
    inv = _inverter(lr=lr, optim='GD')
    w, curve = inv.invert(n_loops=n, **_gpu(s))
    _hold32('GD f32 replayed', ref, w, curve, s['w0'])
    assert curve[-1] < curve[0]
    from latent2im_amd.optim import GuardedSGD
    r = inv.graphs[1]
    assert isinstance(r.opt, GuardedSGD) and r.opt.param_groups[0]['momentum'] == 0.9 and float(r.opt.state[r.w]['step']) == n


def _check16(what, m, curve):
    dev = R16.deviation(torch.from_numpy(curve), m['base']['loss_curve'], True)['loss_rel']
    a = R16.allowed(m, 'loss_curve', 'loss_rel')
    print('%s: model curve %s GPU %s' % (what, m['base']['loss_curve'].tolist(), curve.tolist()))
    print('%s: spread %.3e  gradq %.3e  allowed %.3e  gpu %.3e' % (what, m['spread']['loss_curve']['loss_rel'], m['gradq']['loss_curve']['loss_rel'], a, dev))
    assert dev <= a, (what, dev, a)


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_16_bit_adam_three_replays(dt, precision):
    precision(dt)
    n = 3
    s = _setup(SIZE)
    key = ('adam', dt)                                                 # test_three_guarded_adam_steps's model, computed once for both files
    if key not in _memo16:
        PV = _vgg_states()[1]
        _memo16[key] = R16.measure(lambda R: dict(loss_curve=R16.adam_run(s['P64'], PV, s['w0'], s['target'], s['noise'], n, 0.01, R)), dt, _log2(dt, SIZE, 1))
    inv = _inverter(dt, lr=0.01)
    w, curve = inv.invert(n_loops=n, **_gpu(s))
    assert w.shape == s['w0'].shape and w.dtype == torch.float32 and curve.shape == (n,)
    _check16('adam3 %s replayed' % dt, _memo16[key], curve)
    assert curve[-1] < curve[0]
    assert (inv.scaler is not None) == (dt == 'f16')
    if dt == 'f16':
        st = inv.scaler.stats()
        assert st['skipped'] == 0 and st['steps'] == n, st
        assert inv.graphs[1].opt.scaler is inv.scaler


def test_f16_takes_gd_when_captured(precision):
    precision('f16')
    n, lr = 3, 1e-9
    s = _setup(SIZE)
    key = ('gd16', n, lr)
    if key not in _memo:
        PV = _vgg_states()[1]
        _memo[key] = R16.measure(lambda R: dict(loss_curve=_sgd_run(lambda w_: R16.total_loss(s['P64'], PV, w_, s['target'], s['noise'], R), s['w0'], n, lr)[0]),
                                 'f16', _log2('f16', SIZE, 1))
    inv = _inverter('f16', lr=lr, optim='GD')                          # the eager constructor refuses this pair (test_f16_with_gd_is_refused)
    w, curve = inv.invert(n_loops=n, **_gpu(s))
    _check16('GD3 f16 replayed', _memo[key], curve)
    from latent2im_amd.optim import GuardedSGD
    st = inv.scaler.stats()
    assert isinstance(inv.graphs[1].opt, GuardedSGD) and st['skipped'] == 0 and st['steps'] == n, st
    assert bool(torch.isfinite(w).all()) and not torch.equal(w, s['w0'].float().to(DEV))
    with pytest.raises(NotImplementedError, match='guarded SGD'):
        _inverter('f16', lr=lr, optim='GD', capture=False)


def test_f16_overflow_inside_the_graph_skips_the_iterations(precision, monkeypatch):
    """Exponents 20 octaves too high (floating-point overflow of the gradient maps, as in test_f16_overflow_skips_the_iteration): both replays are
    skipped on the device, W+ keeps its bits, the dynamic scale halves twice."""
    from latent2im_amd import nets16
    precision('f16')
    real = nets16.invert_scale_for
    monkeypatch.setattr(nets16, 'invert_scale_for', lambda r, b: {k: v + 20 for k, v in real(r, b).items()})
    s = _setup(SIZE)
    inv = _inverter('f16')
    assert inv.scaler.log2 == {k: v + 20 for k, v in real(SIZE, 1).items()}
    a = _gpu(s)
    w, curve = inv.invert(n_loops=2, **a)
    st = inv.scaler.stats()
    assert st['skipped'] == 2 and st['scale'] == 0.25 and st['steps'] == 2, st
    assert torch.equal(w, a['w']) and bool(torch.isfinite(w).all())
    assert curve.shape == (2,)
    assert float(inv.graphs[1].opt.state[inv.graphs[1].w]['step']) == 0.0


def test_one_graph_serves_two_images(monkeypatch):
    """Another image first (the target mirrored, 5 iterations), then test_f32_adam_ten_replays's case on the same Inverter: the second use of the
    graph is held to the float64 run by the rules, and on the inputs, a fresh run is held to.  (The mirrored target itself is not held to
    own_rule: Adam's normalised update turns the gradient's error into displacement where the gradient is small, and on that target the eager
    loop deviates by 6.8e-3 of the largest displacement, the replayed one by 6.5e-3, its fp32 CPU model fifteen times more than on this one.)"""
    nb, n = 5, 10
    s = _setup(SIZE)
    ref = _ref32('adam', n, 0.01)
    inv = _inverter(lr=0.01)
    wb, cb = inv.invert(n_loops=nb, **_gpu(s, s['target'].flip(3).contiguous()))
    r = inv.graphs[1]
    assert cb.shape == (nb,) and cb[-1] < cb[0] and float(r.opt.state[r.w]['step']) == nb
    captures = []
    real = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', lambda *a, **k: captures.append(1) or real(*a, **k))
    w, curve = inv.invert(n_loops=n, **_gpu(s))
    assert not captures and list(inv.graphs) == [1] and inv.graphs[1] is r
    assert curve.shape == (n,)
    _hold32('adam f32, second image of one graph', ref, w, curve, s['w0'])
    assert curve[-1] < curve[0] and not torch.equal(w, wb)
    assert float(r.opt.state[r.w]['step']) == n                       # n, not nb + n: the optimiser starts over with the image


def test_batch_2_after_batch_1_takes_its_own_graph():
    s1, s2 = _setup(SIZE), _setup(SIZE, 2)
    inv = _inverter(lr=0.01)
    w1, c1 = inv.invert(n_loops=2, **_gpu(s1))
    w2, c2 = inv.invert(n_loops=2, **_gpu(s2))
    assert sorted(inv.graphs) == [1, 2] and inv.graphs[1].graph is not inv.graphs[2].graph
    assert w1.shape == (1, 8, 512) and w2.shape == (2, 8, 512) and c1.shape == c2.shape == (2,)
    assert np.isfinite(c1).all() and np.isfinite(c2).all() and bool(torch.isfinite(w1).all()) and bool(torch.isfinite(w2).all())
    assert inv.last_image.shape == (2, 3, SIZE, SIZE)
    w1b, c1b = inv.invert(n_loops=2, **_gpu(s1))                       # and back: the first graph is still there
    assert sorted(inv.graphs) == [1, 2] and w1b.shape == (1, 8, 512) and np.allclose(c1b, c1, rtol=1e-3)


def test_replays_issue_no_library_calls(monkeypatch):
    from latent2im_amd import _lib, conv
    s = _setup(SIZE)
    inv = _inverter(lr=0.01)
    a = _gpu(s)
    inv.invert(n_loops=1, **a)
    n = [0]
    real_call, real_launch = _lib.call, conv._launch

    def call(*args, **kw):
        n[0] += 1
        return real_call(*args, **kw)

    def launch(*args, **kw):
        n[0] += 1
        return real_launch(*args, **kw)
    monkeypatch.setattr(_lib, 'call', call)
    monkeypatch.setattr(conv, '_launch', launch)
    curve = inv.graphs[1].run(5)
    assert n[0] == 0 and curve.shape == (5,) and np.isfinite(curve).all()
    loss, _ = inv.loss(a['w'].clone().requires_grad_(), a['batch'], inv.vgg.target_grams(a['batch']), a['noise'])
    loss.backward()
    assert n[0] > 50, n[0]                                             # the counter does see the eager iteration's calls


def test_noise_is_drawn_afresh_by_every_replay():
    s = _setup(SIZE)
    inv = _inverter(lr=0.0)
    a = _gpu(s)
    w, _ = inv.invert(a['batch'], 1, w=a['w'])                         # noise=None
    first = inv.last_image
    r = inv.graphs[1]
    assert not r.fixed_noise and r.noise is None
    r.run(1)
    second = r.out.detach().clone()
    assert bool(torch.isfinite(first).all()) and bool(torch.isfinite(second).all())
    assert not torch.equal(first, second)
    assert torch.equal(w, a['w']) and torch.equal(r.w.detach(), a['w'])


@pytest.mark.parametrize('dt', ['f32', 'f16'])
def test_no_conv2d_or_bmm_in_capture_or_replay(dt, precision, monkeypatch):
    import torch.nn.functional as F
    if dt != 'f32':
        precision(dt)
    s = _setup(SIZE)
    inv = _inverter(dt)

    def refuse(*a, **k):
        raise AssertionError('F.conv2d / torch.bmm on the inversion path')
    monkeypatch.setattr(F, 'conv2d', refuse)
    monkeypatch.setattr(torch, 'bmm', refuse)
    monkeypatch.setattr(torch.Tensor, 'bmm', refuse)
    w, curve = inv.invert(s['target'].float().to(DEV), 2)             # noise drawn
    assert np.isfinite(curve).all() and curve.shape == (2,) and w.shape == (1, inv.gen.n_latent, 512)


def _png_folder(tmp_path, n):
    from PIL import Image
    r = np.random.RandomState(3)
    os.makedirs(tmp_path / 'data' / 'a')
    for i in range(n):
        Image.fromarray(r.randint(0, 255, (40, 36, 3)).astype(np.uint8)).save(tmp_path / 'data' / 'a' / ('%d.png' % i))
    return str(tmp_path / 'data')


@pytest.mark.parametrize('prec', ['f32', 'f16'])
def test_bp_main_hipgraph_writes_what_the_eager_run_writes(prec, tmp_path, precision, monkeypatch):
    from latent2im_amd import bp, constants
    precision(prec)                                                    # (bp.main sets conv.PRECISION itself: this only restores it afterwards)
    monkeypatch.setattr(constants, 'ALLOW_SYNTHETIC_WEIGHTS', constants.ALLOW_SYNTHETIC_WEIGHTS)
    data = _png_folder(tmp_path, 3)                                    # batches of 2 and 1: the partial last batch takes its own graph
    listing = {}
    for flag in ((), ('--hipgraph',)):
        out = tmp_path / ('graph' if flag else 'eager')
        curve = bp.main(['--path', data, '--save_path', str(out), '--resolution', '32', '--batch_size', '2', '--n_loops', '2', '--synthetic_weights',
                         '--precision', prec, *flag])
        assert curve.shape == (2,) and np.isfinite(curve).all()
        listing[bool(flag)] = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert listing[True] == listing[False] and 'latent/1_w.npy' in listing[True] and '1_final.png' in listing[True]
    for i, b in ((0, 2), (1, 1)):
        w = np.load(tmp_path / 'graph' / 'latent' / ('%d_w.npy' % i))
        assert w.dtype == np.float32 and w.shape == (b, 8, 512) and np.isfinite(w).all()


def test_bp_main_f16_gd_needs_hipgraph(tmp_path, precision, monkeypatch):
    from latent2im_amd import bp, constants
    precision('f16')
    monkeypatch.setattr(constants, 'ALLOW_SYNTHETIC_WEIGHTS', constants.ALLOW_SYNTHETIC_WEIGHTS)
    data = _png_folder(tmp_path, 1)
    argv = ['--path', data, '--save_path', str(tmp_path / 'out'), '--resolution', '32', '--n_loops', '2', '--synthetic_weights', '--precision', 'f16',
            '--optimizer', 'GD', '--lr', '1e-9']
    curve = bp.main(argv + ['--hipgraph'])
    assert curve.shape == (2,) and np.isfinite(curve).all()
    w = np.load(tmp_path / 'out' / 'latent' / '0_w.npy')
    assert w.dtype == np.float32 and w.shape == (1, 8, 512) and np.isfinite(w).all()
    with pytest.raises(NotImplementedError, match='guarded SGD'):
        bp.main(argv)
