"""BASELINE config 1 on the 16-bit path: (A) nets16.PGGenerator against its rounding model (tests/pggan16_ref.generator_forward: the float64 oracle
with the storage rounding restated through tests/inversion16_ref.Rounding) with inversion16_ref.measure / allowed unchanged; (B) the whole step at
the graph's own size (256^2, batch 2) against the exact float64 step of tests/golden/pggan16_step.npz, with bars taken from the whole-step rounding
model on the CPU (tests/golden/make_pggan16_step.py); and the plumbing of pggan.load_networks / pggan.TransformGraph under conv.PRECISION 'f16' /
'bf16'.  Measured figures go to profiles/pggan16_parity.txt."""
import os

import numpy as np
import pytest
import torch

from latent2im_amd import constants, conv, synth
from latent2im_amd import pggan as pg
from tests import inversion16_ref as I16
from tests import pggan16_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_report = {}
_shared = {}


@pytest.fixture
def precision(monkeypatch):
    """Sets conv.PRECISION for the networks a test builds (restored afterwards)."""
    def set_(dt):
        monkeypatch.setattr(conv, 'PRECISION', dt)
    monkeypatch.setattr(conv, 'PRECISION', conv.PRECISION)
    return set_


@pytest.fixture(scope='module', autouse=True)
def _write_report():
    yield
    if not _report:
        return
    lines = ['# nets16.PGGenerator against tests/pggan16_ref.generator_forward (float64 oracle + storage rounding), synth.pggan_generator_state(seed=11),',
             '# z_sample(2, seed=3), probe seed 5: measured GPU figure / allowed (max(2 x the model\'s spread, gradq-only)) / the model\'s distance to the exact',
             '# float64 oracle.  "step 256^2 batch 2" rows: the whole config-1 step (strong walk, content on) against the EXACT float64 step of',
             '# tests/golden/pggan16_step.npz: gpu-to-exact / bar = model-to-exact + allowed (angles in radians; content: absolute).  Written by',
             '# tests/test_pggan16_gpu.py.']
    lines += ['%-34s %s' % (k, _report[k]) for k in sorted(_report)]
    with open(os.path.join(ROOT, 'profiles', 'pggan16_parity.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


def _f(a):
    """A one-element fixture array as a float."""
    return float(np.asarray(a).reshape(-1)[0])


def _inputs():
    """The generator state, z and (per setting and element type) the model's measurement: computed once, shared read-only."""
    if 'P' not in _shared:
        _shared['P'], _shared['z'] = R.generator_inputs()
        _shared['state'] = synth.pggan_generator_state(seed=11)
    return _shared


def _measure(step, alpha, dt):
    key = (step, alpha, dt)
    if key not in _shared:
        s = _inputs()
        _shared[key] = R.measure_generator(s['P'], s['z'], step, alpha, dt)
    return _shared[key]


@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('step,alpha', R.GEN_SETTINGS, ids=str)
def test_generator_matches_its_rounding_model(precision, step, alpha, dt):
    """The z gradient of sum(img * probe) (rel-L2 and 1 - cos) and the image (max |delta| over the largest pixel) within max(2 x the model's own
    spread, gradq-only) of the model.  sum(img * probe) itself is not held: it cancels (its own spread reaches 1e-2)."""
    from latent2im_amd import nets16, optim
    precision(dt)
    s = _inputs()
    m = _measure(step, alpha, dt)
    # condition, not measurement: beyond the cap the inputs are ill-conditioned and the setting needs another seed
    assert m['spread']['grad_z']['one_minus_cos'] <= I16.SPREAD_CAP['one_minus_cos'], m['spread']
    G = nets16.PGGenerator(s['state'], device=DEV)
    if dt == 'f16':                                      # the measured exponent of this setting (pggan16_ref.GEN_LOG2), no dynamic factor moving
        nets16.attach_scaler((G,), optim.LossScaler(dict(R=0, V=0, D=0, G=R.GEN_LOG2[(step, alpha)]), DEV))
    z = s['z'].float().to(DEV).requires_grad_(True)
    img = G(z, step=step, alpha=alpha)
    assert img.dtype == torch.float32 and tuple(img.shape) == (2, 3, 4 * 2 ** step, 4 * 2 ** step)
    (img * R.generator_probe(img.shape).float().to(DEV)).sum().backward()
    assert bool(torch.isfinite(z.grad).all())
    dev = I16.deviation(z.grad, m['base']['grad_z'], False)
    base_img = m['image']['base']
    img_dev = float((img.detach().double().cpu() - base_img).abs().max() / base_img.abs().max())
    tag = 'step %d alpha %-4g %-4s' % (step, alpha, dt)
    for fig in ('rel_l2', 'one_minus_cos'):
        _report['%s grad %s' % (tag, fig)] = 'gpu %.3e allowed %.3e model-to-exact %.3e' % (dev[fig], I16.allowed(m, 'grad_z', fig), m['exact']['grad_z'][fig])
    _report['%s image' % tag] = 'gpu %.3e allowed %.3e model-to-exact %.3e' % (img_dev, 2.0 * m['image']['spread'], m['image']['exact'])
    print(tag, dev, img_dev, m['spread'], m['gradq'], m['image']['spread'])
    for fig in ('rel_l2', 'one_minus_cos'):
        assert dev[fig] <= I16.allowed(m, 'grad_z', fig), (fig, dev[fig], I16.allowed(m, 'grad_z', fig))
    assert img_dev <= 2.0 * m['image']['spread'], (img_dev, m['image']['spread'])


@pytest.mark.parametrize('dt', R.DTYPES)
def test_step_at_the_graphs_size_against_the_float64_fixture(monkeypatch, golden, dt):
    """The strong-walk case of tests/test_pggan_gpu.py (seed-11 generator, walk_w0 x 50, regressor seed 300, VGG seed 400, no_gan_loss, content on)
    at 256^2, batch 2, against the exact float64 step.  The GPU may be as far from exact as the whole-step rounding model is, plus the model's own
    allowance (inversion16_ref.allowed, restated relative to the exact gradient): rel-L2 and the angle of the walk gradient (angles add on the
    sphere, 1 - cos does not), the same sum for the regressor loss.  The content term, a mean squared difference of two rounded maps, is held
    by its absolute size only (make_pggan16_step.py derives the bar)."""
    from latent2im_amd import nets16, optim
    from tests.golden import make_pggan16_step as tool
    fx = golden('pggan16_step')
    assert int(fx['fingerprint']) == tool.fingerprint(), 'tests/golden/pggan16_step.npz was made for other seeds or states: run tests/golden/make_pggan16_step.py'
    # condition, not measurement: the model's own spread within the cap
    assert _f(fx['%s.spread.grad_w.one_minus_cos' % dt]) <= I16.SPREAD_CAP['one_minus_cos']
    assert _f(fx['%s.spread.loss_reg.loss_rel' % dt]) <= I16.SPREAD_CAP['loss_rel']
    S = R.STEP
    monkeypatch.setattr(conv, 'PRECISION', dt)
    monkeypatch.setattr(constants, 'BATCH_SIZE', S['batch'])
    nets = (nets16.PGGenerator(synth.pggan_generator_state(seed=S['g_seed']), device=DEV), nets16.ResNet50(synth.resnet50_state(seed=S['r_seed']), device=DEV),
            nets16.VGG19Prefix(synth.vgg19_prefix_state(seed=S['v_seed']), device=DEV), {'G': 'synthetic'})
    if dt == 'f16':
        nets16.attach_scaler(nets[:3], optim.LossScaler(tool.scales(), DEV))
    state = np.random.get_state()
    graph = pg.faceGraph(lr=1e-3, walk_type='linear', loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': S['attr']}, layers=None,
                         pgan_opts=None, nets=nets)
    np.random.set_state(state)
    with torch.no_grad():
        graph.walk.w.copy_(torch.from_numpy(np.asarray(golden('pggan')['walk_w0'])).float() * S['walk_gain'])
    z = torch.from_numpy(np.asarray(synth.z_sample(S['batch'], seed=S['z_seed']))).float().to(DEV)
    x0 = graph.get_logits({'z': z})
    target, eps = graph.get_alphas(graph.get_reg_preds(x0), torch.full((S['batch'], 1), S['alpha_delta'], device=DEV))
    x1 = graph.get_logits({'z': graph.get_z_new_tensor(z, eps)})
    loss = graph.get_w_loss({'org': x0, 'logit': x1, 'alpha': target}, no_content_loss=False, no_gan_loss=True)
    loss.backward()
    grad = graph.walk.w.grad
    assert bool(torch.isfinite(grad).all())
    dev = I16.deviation(grad, torch.from_numpy(fx['grad_w']), False)
    ratio = _f(fx['%s.norm_ratio' % dt])
    got = dict(rel_l2=dev['rel_l2'], angle=R.angle(dev['one_minus_cos']),
               reg=abs(float(graph.last_terms['reg']) - _f(fx['loss_reg'])) / abs(_f(fx['loss_reg'])),
               cont=abs(float(graph.last_terms['cont']) - _f(fx['loss_cont'])))
    bar = dict(rel_l2=_f(fx['%s.model.grad_w.rel_l2' % dt]) + _f(fx['%s.allowed.grad_w.rel_l2' % dt]) * ratio,
               angle=R.angle(_f(fx['%s.model.grad_w.one_minus_cos' % dt])) + R.angle(_f(fx['%s.allowed.grad_w.one_minus_cos' % dt])),
               reg=_f(fx['%s.model.loss_reg.loss_rel' % dt]) + _f(fx['%s.allowed.loss_reg.loss_rel' % dt]) * abs(_f(fx['%s.loss_reg' % dt]) / _f(fx['loss_reg'])),
               cont=_f(fx['%s.cont_abs_allowed' % dt]))
    model = dict(rel_l2=_f(fx['%s.model.grad_w.rel_l2' % dt]), angle=R.angle(_f(fx['%s.model.grad_w.one_minus_cos' % dt])),
                 reg=_f(fx['%s.model.loss_reg.loss_rel' % dt]), cont=abs(_f(fx['%s.loss_cont' % dt]) - _f(fx['loss_cont'])))
    for k, label in (('rel_l2', 'walk grad rel_l2'), ('angle', 'walk grad angle'), ('reg', 'regressor loss rel'), ('cont', 'content term abs')):
        _report['step 256^2 batch 2 %-4s %s' % (dt, label)] = 'gpu-to-exact %.3e bar %.3e model-to-exact %.3e' % (got[k], bar[k], model[k])
    print(dt, got, bar, model, 'content exact %.4e gpu %.4e' % (_f(fx['loss_cont']), float(graph.last_terms['cont'])))
    for k in ('rel_l2', 'angle', 'reg', 'cont'):
        assert got[k] <= bar[k], (k, got[k], bar[k])


def test_narrow_steps_are_refused_before_any_launch(precision):
    from latent2im_amd import nets16
    precision('bf16')
    G = nets16.PGGenerator(_inputs()['state'], device=DEV)
    z = torch.zeros(1, 511, device=DEV)
    with pytest.raises(NotImplementedError):
        G(z, step=8, alpha=0)
    with pytest.raises(IndexError):
        G(z, step=9, alpha=0)
    with pytest.raises(RuntimeError):
        G(torch.zeros(1, 512, device=DEV))
    assert tuple(G(z, step=7, alpha=-1).shape) == (1, 3, 512, 512)           # block 7, 64 -> 32 -> 32 channels: the narrowest maps the convs read


def _graph(monkeypatch, dt, batch=2):
    monkeypatch.setattr(conv, 'PRECISION', dt)
    monkeypatch.setattr(constants, 'ALLOW_SYNTHETIC_WEIGHTS', True)
    monkeypatch.setattr(constants, 'BATCH_SIZE', batch)
    state = np.random.get_state()
    np.random.seed(0)
    graph = pg.faceGraph(lr=1e-3, walk_type='linear', loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': 31}, layers=None, pgan_opts=None)
    np.random.set_state(state)
    return graph


@pytest.mark.parametrize('dt', R.DTYPES)
def test_graph_builds_the_16_bit_networks_and_trains(monkeypatch, tmp_path, dt):
    """load_networks follows conv.PRECISION (the fp32 classes under 'f16' were the silent fallback this replaces); one optimizeParametersAll returns a
    finite float64 loss and moves the walk; apply_alpha and the vis path run; no torch conv anywhere."""
    import torch.nn.functional as F
    from latent2im_amd import nets16, optim

    def refuse(*a, **k):
        raise AssertionError('F.conv2d on the 16-bit config-1 path')
    graph = _graph(monkeypatch, dt)
    monkeypatch.setattr(F, 'conv2d', refuse)
    assert type(graph.module.netG) is nets16.PGGenerator and type(graph.regressor) is nets16.ResNet50 and type(graph.vgg19) is nets16.VGG19Prefix
    assert graph.weight_sources['precision'] == dt
    if dt == 'f16':
        assert isinstance(graph.optimizer, optim.GuardedAdam) and graph.loss_scaler is graph.module.netG.scaler is graph.regressor.scaler is graph.vgg19.scaler
        assert graph.loss_scaler.log2 == nets16.pggan_scale_for(256, 2) == graph.weight_sources['loss_scale_log2']
        half = nets16.loss_scale_for(128, 2)
        assert graph.loss_scaler.log2['R'] == half['R'] and graph.loss_scaler.log2['V'] == half['V']
    else:
        assert graph.loss_scaler is None and type(graph.optimizer) is torch.optim.Adam
    w0 = graph.walk.w.detach().clone()
    loss, x0, x1, a_org, a_tgt = pg.walk_training_step(graph, synth.z_sample(2, seed=0), np.full((2, 1), 0.3), no_content_loss=False)
    assert loss.dtype == torch.float64 and np.isfinite(float(loss.detach()))
    assert tuple(x0.shape) == (2, 3, 128, 128) and x0.dtype == torch.float32
    assert bool(torch.isfinite(graph.walk.w.grad).all()) and float(graph.walk.w.grad.abs().max()) > 0
    assert not torch.equal(graph.walk.w.detach(), w0)
    if dt == 'f16':
        st = graph.loss_scaler.stats()
        assert st['skipped'] == 0 and st['steps'] == 1 and st['scale'] == 1.0
    out, aorg = graph.apply_alpha({'z': synth.z_sample(2, seed=0)}, np.full((2, 1), 0.8))
    assert list(out.shape) == [2, 3, 128, 128] and list(aorg.shape) == [2, 1] and bool(torch.isfinite(out).all())
    written = graph.vis_multi_image_batch_alphas({'z': synth.z_sample(2, seed=0)}, str(tmp_path / 'vis'), [np.full((2, 1), a) for a in (0.2, 0.8)], None, 0)
    assert len(written) == 2 and all(os.path.getsize(p) > 0 for p in written)


def test_f16_oversized_scales_skip_the_step_on_the_device(monkeypatch):
    """With the static exponents 13 octaves too high the scaled gradient maps leave fp16: the walk gradient is non-finite, the update is skipped
    (walk unchanged) and the dynamic factor is halved — all on the device."""
    from latent2im_amd import nets16
    base = nets16.pggan_scale_for(256, 2)
    monkeypatch.setenv('L2I_F16_SCALES', ','.join(str(base[k] + 13) for k in 'RVDG'))
    graph = _graph(monkeypatch, 'f16')
    monkeypatch.delenv('L2I_F16_SCALES')
    assert graph.loss_scaler.log2 == {k: v + 13 for k, v in base.items()}
    w0 = graph.walk.w.detach().clone()
    pg.walk_training_step(graph, synth.z_sample(2, seed=0), np.full((2, 1), 0.3), no_content_loss=False)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(graph.walk.w.grad).all())
    assert torch.equal(graph.walk.w.detach(), w0)
    st = graph.loss_scaler.stats()
    assert st['skipped'] == 1 and st['scale'] == 0.5, st


@pytest.mark.parametrize('dt', ['f32', 'bf16x3'])
def test_other_precisions_build_the_fp32_classes(monkeypatch, dt):
    from latent2im_amd.perceptual import VGG19Prefix
    from latent2im_amd.regressor import ResNet50
    graph = _graph(monkeypatch, dt)
    assert type(graph.module.netG) is pg.Generator and type(graph.regressor) is ResNet50 and type(graph.vgg19) is VGG19Prefix
    assert graph.loss_scaler is None and type(graph.optimizer) is torch.optim.Adam and graph.weight_sources['precision'] == dt
