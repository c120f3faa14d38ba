"""capture.CapturedZStep: the config-1 step (PGGAN-256, walk in z) replayed from one hipGraph against pggan.walk_training_step launched eagerly.
256^2, batch 2, synthetic weights, one attribute; the frozen networks are built once per precision and shared by the eager and the captured
graph through ``nets=``; every graph has its own walk from the same seed.

Bars, from the project's capture tests: fp32 — tests/test_networks_gpu.py::test_hipgraph_captured_step_matches_eager (images rtol 1e-4 / atol 1e-5,
loss 1e-5 / 1e-6, gradient and walk under 1e-3 of the largest entry), replaced by bit equality when the eager side itself is bit-reproducible run to
run; 16-bit — tests/test_h8_gpu.py::test_fp16_hipgraph_captured_steps_follow_eager_steps (x1 within 2^-8 of its largest value, loss within 1e-4
relative, gradient cosine over 0.9995 per parameter tensor)."""
import os

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, capture, constants, conv, synth
from latent2im_amd import pggan as pg
from tests import emu

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BATCH = 2
WALK_SEED = 81
ALPHAS = (0.3, -0.2, 0.5, 0.7, -0.6, 0.1)
_NETS = {}


def _setup(monkeypatch, dt):
    monkeypatch.setattr(conv, 'PRECISION', dt)
    monkeypatch.setattr(constants, 'ALLOW_SYNTHETIC_WEIGHTS', True)
    monkeypatch.setattr(constants, 'BATCH_SIZE', BATCH)
    if dt not in _NETS:
        _NETS[dt] = pg.load_networks(torch.device(DEV, torch.cuda.current_device()))
    return _NETS[dt]


def _graph(monkeypatch, dt, walk_type='NNz'):
    nets = _setup(monkeypatch, dt)
    rng = np.random.get_state()
    np.random.seed(WALK_SEED)                                               # the linear walk draws from the global numpy RNG
    try:
        graph = pg.faceGraph(lr=1e-3, walk_type=walk_type, loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': 31}, layers=None,
                             pgan_opts=None, nets=nets)
    finally:
        np.random.set_state(rng)
    if walk_type != 'linear':
        emu.seeded_state(graph.walk, WALK_SEED)
    sc = graph.loss_scaler
    if sc is not None:                                                      # the scaler travels with the shared networks: every graph starts it over
        sc.state.zero_()
        sc.scale.fill_(1.0)
    return graph


def _inputs(n, seed=40):
    return [synth.z_sample(BATCH, seed=seed + i) for i in range(n)], [np.full((BATCH, 1), ALPHAS[i % len(ALPHAS)]) for i in range(n)]


def _walk(graph):
    return [p.detach().clone() for p in graph.walk.parameters()]


def _eager(graph, zs, al):
    out = []
    for z, a in zip(zs, al):
        loss, x0, x1, a0, target = pg.walk_training_step(graph, z, a, no_content_loss=False)
        torch.cuda.synchronize()
        out.append(dict(loss=loss.detach().clone(), x0=x0.detach().clone(), x1=x1.detach().clone(), a0=a0.detach().clone(), target=target.detach().clone(),
                        grads=[p.grad.detach().clone() for p in graph.walk.parameters()]))
    return out


def _counting(monkeypatch):
    seen = []
    real_call, real_launch = _lib.call, conv._launch

    def call(name, *a, **k):
        seen.append(name)
        return real_call(name, *a, **k)

    def launch(*a, **k):
        seen.append('conv launch')
        return real_launch(*a, **k)
    monkeypatch.setattr(_lib, 'call', call)
    monkeypatch.setattr(conv, '_launch', launch)
    return seen


def close(a, b, rtol, atol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and bool(((a - b).abs() <= atol + rtol * b.abs()).all()), float((a - b).abs().max())


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('walk_type', ['NNz', 'linear'])
def test_f32_replayed_steps_match_eager_steps(monkeypatch, walk_type):
    zs, al = _inputs(3)
    ge = _graph(monkeypatch, 'f32', walk_type)
    w0 = _walk(ge)
    eager = _eager(ge, zs, al)
    g2 = _graph(monkeypatch, 'f32', walk_type)
    assert all(torch.equal(a, b) for a, b in zip(w0, _walk(g2)))           # same seed, same walk
    again = _eager(g2, zs, al)
    exact = all(torch.equal(a[k], b[k]) for a, b in zip(eager, again) for k in ('loss', 'x1')) \
        and all(torch.equal(x, y) for a, b in zip(eager, again) for x, y in zip(a['grads'], b['grads'])) \
        and all(torch.equal(x, y) for x, y in zip(_walk(ge), _walk(g2)))
    print('eager fp32 step bit-reproducible run to run:', exact)
    gc_ = _graph(monkeypatch, 'f32', walk_type)
    step = capture.CapturedZStep(gc_, BATCH, 1)
    assert all(torch.equal(a, b) for a, b in zip(w0, _walk(gc_)))          # warm-up and capture ran no update
    assert type(gc_.optimizer) is torch.optim.Adam and not gc_.optimizer.state
    for i in range(3):
        r = step(zs[i], al[i])
        torch.cuda.synchronize()
        e = eager[i]
        assert len(r['grads']) == len(e['grads']) == (6 if walk_type == 'NNz' else 1)
        if exact:
            assert torch.equal(r['loss'], e['loss']) and torch.equal(r['x1'], e['x1']) and torch.equal(r['x0'], e['x0'])
            assert all(torch.equal(g, h) for g, h in zip(r['grads'], e['grads']))
        else:
            close(r['x1'], e['x1'], 1e-4, 1e-5)
            close(r['x0'], e['x0'], 1e-4, 1e-5)
            close(r['loss'], e['loss'], 1e-5, 1e-6)
            assert max(relmax(g, h) for g, h in zip(r['grads'], e['grads'])) < 1e-3
        assert torch.equal(r['a0'], e['a0']) or relmax(r['a0'], e['a0']) < 1e-4
        assert torch.equal(r['target'], (r['a0'] + torch.as_tensor(al[i], dtype=torch.float32, device=DEV)).clamp(0, 1))
        assert r['terms']['reg'] is not None and r['terms']['cont'] is not None and r['terms']['gan'] is None
    if exact:
        assert all(torch.equal(a, b) for a, b in zip(_walk(gc_), _walk(ge)))
    else:
        assert max(relmax(a, b) for a, b in zip(_walk(gc_), _walk(ge))) < 1e-3
    assert all(not torch.equal(a, b) for a, b in zip(_walk(gc_), w0))        # the walk moved
    # a replay plus its tail issues no library call on fp32: the optimiser is torch's Adam
    seen = _counting(monkeypatch)
    step(zs[0], al[0])
    torch.cuda.synchronize()
    assert seen == [], seen


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_16_bit_replayed_steps_follow_eager_steps(monkeypatch, dt):
    from latent2im_amd import optim
    zs, al = _inputs(3)
    ge = _graph(monkeypatch, dt)
    w0 = _walk(ge)
    eager = _eager(ge, zs, al)
    if dt == 'f16':
        st = ge.loss_scaler.stats()
        assert st['steps'] == 3 and st['skipped'] == 0 and st['scale'] == 1.0, st
    gc_ = _graph(monkeypatch, dt)
    assert isinstance(gc_.optimizer, optim.GuardedAdam) == (dt == 'f16')
    step = capture.CapturedZStep(gc_, BATCH, 1)
    assert all(torch.equal(a, b) for a, b in zip(w0, _walk(gc_)))
    if dt == 'f16':
        st = gc_.loss_scaler.stats()
        assert st['steps'] == 0 and st['scale'] == 1.0, st                  # warm-up and capture never ran the update
    for i in range(3):
        r = step(zs[i], al[i])
        torch.cuda.synchronize()
        e = eager[i]
        assert float((r['x1'].float() - e['x1'].float()).abs().max()) <= 2.0 ** -8 * float(e['x1'].float().abs().max())
        assert abs(float(r['loss']) - float(e['loss'])) <= 1e-4 * abs(float(e['loss']))
        for g, h in zip(r['grads'], e['grads']):
            g, h = g.double(), h.double()
            cos = float((g * h).sum() / (g.norm() * h.norm()))
            assert cos > 0.9995, (i, cos)
    assert all(not torch.equal(a, b) for a, b in zip(_walk(gc_), w0))
    assert all(bool(torch.isfinite(a).all()) for a in _walk(gc_))
    if dt == 'f16':
        st = gc_.loss_scaler.stats()
        assert st['steps'] == 3 and st['skipped'] == 0 and st['scale'] == 1.0, st
    seen = _counting(monkeypatch)
    step(zs[0], al[0])
    torch.cuda.synchronize()
    if dt == 'f16':
        assert len(seen) <= 2 and seen == ['l2i_nonfinite_flag_multi_f32', 'l2i_adam_guarded_multi_f32'], seen
    else:
        assert seen == [], seen


def test_f16_overflow_inside_the_replay_skips_and_backs_off(monkeypatch):
    """The dynamic factor 20 octaves up (the static exponents leave eleven under fp16's largest number): the gradient maps overflow inside the
    replayed graph, the guard leaves every walk tensor bit-unchanged and halves the scale; replays go on backing off until the gradient is finite
    again, and that replay updates."""
    zs, al = _inputs(1)
    g = _graph(monkeypatch, 'f16')
    sc = g.loss_scaler
    step = capture.CapturedZStep(g, BATCH, 1)
    w0 = _walk(g)
    sc.scale.copy_(torch.tensor([2.0 ** 20, 2.0 ** -20], device=DEV))
    step(zs[0], al[0])
    torch.cuda.synchronize()
    st = sc.stats()
    assert st['skipped'] == 1 and st['steps'] == 1 and st['scale'] == 2.0 ** 19 and st['tracker'] == 0, st
    assert float(sc.inv_dyn) == 2.0 ** -19 and int(sc.state[0]) == 0
    assert all(torch.equal(a, b) for a, b in zip(_walk(g), w0))
    assert all(float(g.optimizer.state[p]['step']) == 0.0 for p in g.walk.parameters())
    for k in range(2, 32):                                                  # at most 20 more halvings bring the factor back to 1
        step(zs[0], al[0])
        st = sc.stats()
        if st['skipped'] < k:
            break
    assert st['steps'] == k and st['skipped'] == k - 1 and st['scale'] == 2.0 ** (20 - (k - 1)) and st['scale'] >= 1.0, st
    assert all(not torch.equal(a, b) for a, b in zip(_walk(g), w0))
    assert all(bool(torch.isfinite(a).all()) for a in _walk(g))
    assert all(float(g.optimizer.state[p]['step']) == 1.0 for p in g.walk.parameters())


def test_replays_back_to_back_without_host_sync(monkeypatch):
    """tests/test_networks_gpu.py::test_hipgraph_replays_back_to_back_without_host_sync on this step: six replays queued with no synchronisation
    in between (more than the staging ring holds) against the same six steps launched eagerly with a sync after each."""
    n = 6
    zs, al = _inputs(n, seed=60)
    ge = _graph(monkeypatch, 'f32')
    w0 = torch.cat([a.reshape(-1) for a in _walk(ge)]).cpu()
    _eager(ge, zs, al)
    gc_ = _graph(monkeypatch, 'f32')
    step = capture.CapturedZStep(gc_, BATCH, 1)
    torch.cuda.synchronize()
    for i in range(n):                                                      # no synchronisation: the host runs ahead
        step(zs[i], al[i])
    torch.cuda.synchronize()
    we = torch.cat([a.reshape(-1) for a in _walk(ge)]).cpu()
    wc = torch.cat([a.reshape(-1) for a in _walk(gc_)]).cpu()
    moved = float((we - w0).abs().max())
    assert moved > 3e-3                                                     # six Adam steps of ~lr each
    d = (wc - we).abs()
    assert float(d.median()) < 1e-5 and float((d > 0.2 * moved).double().mean()) < 0.02, (float(d.median()), float(d.max()), moved)


def test_train_step_routes_full_batches_to_the_replay_and_ragged_ones_to_eager(monkeypatch):
    from latent2im_amd import trainer
    g = _graph(monkeypatch, 'f32', 'linear')
    opt = type('O', (), dict(hip_graph=True, no_content_loss=False, no_gan_loss=True))()
    replays = []
    real = capture.CapturedZStep.__call__
    monkeypatch.setattr(capture.CapturedZStep, '__call__', lambda self, *a, **k: replays.append(1) or real(self, *a, **k))
    rng = np.random.get_state()
    try:
        loss, at, x0, x1 = trainer.train_step(g, synth.z_sample(4, seed=1), ['Smiling'], opt=opt)
        assert replays == [1] and isinstance(g._captured_step, capture.CapturedZStep) and g._captured_step.z.shape[0] == 4
        assert x1.shape == (4, 3, 128, 128) and np.isfinite(float(loss))
        w1 = _walk(g)
        loss, at, x0, x1 = trainer.train_step(g, synth.z_sample(BATCH, seed=2), ['Smiling'], opt=opt)  # a ragged batch: eager, and it trains
        assert replays == [1] and x1.shape == (BATCH, 3, 128, 128) and np.isfinite(float(loss))
        assert not torch.equal(_walk(g)[0], w1[0])
        trainer.train_step(g, synth.z_sample(4, seed=3), ['Smiling'], opt=opt)
        assert replays == [1, 1]
        opt.no_gan_loss = False
        with pytest.raises(TypeError, match='no_gan_loss'):                 # the GAN term still raises, as on the eager route
            trainer.train_step(g, synth.z_sample(4, seed=4), ['Smiling'], opt=opt)
    finally:
        np.random.set_state(rng)


@pytest.mark.parametrize('precision,hip_graph', [('f32', True), ('f16', True), ('f32', False)])
def test_driver_trains_config_1_with_hip_graph(monkeypatch, tmp_path, precision, hip_graph):
    """train.py's command line: six samples at batch 4 are one iteration (the loop floors, as it does for the StyleGAN2 route), replayed."""
    from latent2im_amd import trainer
    for name in ('ALLOW_SYNTHETIC_WEIGHTS', 'BATCH_SIZE'):
        monkeypatch.setattr(constants, name, getattr(constants, name))
    monkeypatch.setattr(conv, 'PRECISION', conv.PRECISION)
    replays = []
    real = capture.CapturedZStep.__call__
    monkeypatch.setattr(capture.CapturedZStep, '__call__', lambda self, *a, **k: replays.append(1) or real(self, *a, **k))
    models = str(tmp_path / 'models')
    argv = ['--model', 'pggan', '--transform', 'face', '--no_gan_loss', '--synthetic_weights', '--num_samples', '6', '--batch_size', '4', '--n_epoch', '1',
            '--learning_rate', '1e-3', '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt', '--models_dir', models, '--overwrite_config',
            '--seed', '3', '--model_save_freq', '1000', '--precision', precision] + (['--hip_graph'] if hip_graph else [])
    state = np.random.get_state()
    try:
        trainer.main(multi_attr=False, argv=argv)
    finally:
        np.random.set_state(state)
    assert len(replays) == (1 if hip_graph else 0)
    out = os.path.join(models, 'pggan_face_NNz_lr0.001_l2')
    ckpt = os.path.join(out, 'model_w_1_final_walk_module.ckpt')
    assert os.path.isfile(ckpt), os.listdir(out)
    walk = torch.load(ckpt, map_location='cpu', weights_only=False)
    assert type(walk) is pg.WalkMlpZ3
    assert all(bool(torch.isfinite(p).all()) for p in walk.parameters())
    log = open(os.path.join(out, 'log.txt')).read()
    assert log.count('T, epc, bst, lss, alpha') == 1
