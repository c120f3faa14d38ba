"""The PGGAN graph's MLP walk on the GPU: (A) l2i_linear_rows_f32 / l2i_linear_rows_bwd_f32 (csrc/l2i_walk.hip) against the float64 model and its
per-element bounds (tests/walk_mlp_ref.py), outputs inside sentinel guards, every case launched twice and compared bit for bit; (B) pggan.WalkMlpZ3
against the fixture made from the reference's own module and against the model's bounds composed over the three layers, its launch budget, shapes
and the no-grad path; (C) the graph: the default walk type builds it, one training step at 256^2 against the float64 oracle (fp32) and against
the model fed with the z gradient that arrived (f16 / bf16), the optimiser step, the checkpoint; (D) the command-line driver.
L2I_WALK_CONTRACT_ERRORS=<path> writes the largest observed share of each bound."""
import os

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, constants, conv, synth
from latent2im_amd import kernels as K
from latent2im_amd import pggan as pg
from tests import emu
from tests import walk_mlp_ref as M
from tests.contract_gpu import guarded, untouched
from tests.golden import make_walk_mlp as tool
from tests.test_walk_mlp_ref_cpu import KEYS, case

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
_SHARES = {}


@pytest.fixture(scope='module', autouse=True)
def _write_shares():
    yield
    path = os.environ.get('L2I_WALK_CONTRACT_ERRORS')
    if path and _SHARES:
        with open(path, 'w') as f:
            f.write('# output: largest |got - want| / bound over every case of tests/test_walk_mlp_gpu.py (bounds: tests/walk_mlp_ref.py)\n')
            f.write('\n'.join('%-44s %.4f' % (k, _SHARES[k]) for k in sorted(_SHARES)) + '\n')


def _note(name, got, want, bound):
    s = M.share(got.detach().cpu().numpy(), want, bound)
    _SHARES[name] = max(_SHARES.get(name, 0.0), s)
    return s


# ---- (A) the kernel contract -------------------------------------------------------------------------------------------------------------------
def _fwd(x, w, b, epi, res, a, B, Kd, N):
    buf, y = guarded((B, N))
    _lib.call('l2i_linear_rows_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(w), _lib.fptr(b), _lib.fptr(res), _lib.fptr(a), B, Kd, N, epi, 0.2)
    return buf, y


def _bwd(g, x, w, epi, y, a, add, want_gx, B, Kd, N, slices):
    bufs = {'gw': guarded((N, Kd)), 'gb': guarded((N,))}
    if want_gx:
        bufs['gx'] = guarded((B, Kd))
        if slices > 1:
            bufs['ws'] = guarded((slices, B, Kd))
    view = lambda k: bufs[k][1] if k in bufs else None
    _lib.call('l2i_linear_rows_bwd_f32', _lib.fptr(view('gw')), _lib.fptr(view('gb')), _lib.fptr(view('gx')), _lib.fptr(view('ws')), _lib.fptr(add),
              _lib.fptr(g), _lib.fptr(y), _lib.fptr(a), _lib.fptr(x), _lib.fptr(w), B, Kd, N, epi, 0.2, slices)
    return bufs


@pytest.mark.parametrize('Kd,N', [(64, 128), (128, 64), (512, 1024), (1024, 1024), (1024, 512)])
@pytest.mark.parametrize('B', [1, 3, 16, 17, 33])
def test_kernels_against_the_model(B, Kd, N):
    rs = np.random.RandomState(1000 * B + Kd + N)
    x = rs.standard_normal((B, Kd)).astype(np.float32)
    w = (rs.standard_normal((N, Kd)) / np.sqrt(Kd)).astype(np.float32)
    b = (rs.standard_normal(N) * 0.1).astype(np.float32)
    a = rs.uniform(-1, 1, B).astype(np.float32)
    res = rs.standard_normal((B, N)).astype(np.float32)
    g = rs.standard_normal((B, N)).astype(np.float32)
    add = rs.standard_normal((B, Kd)).astype(np.float32)
    yact = M.linear_fwd(x, w, b, M.LRELU)[0].astype(np.float32)
    yact[B - 1, ::7] = 0.0                                                  # exact zeros: they take the slope
    d = {k: T(v).to(DEV) for k, v in dict(x=x, w=w, b=b, a=a, res=res, g=g, add=add, yact=yact).items()}
    tag = 'B%d K%d N%d' % (B, Kd, N)
    for epi, name in ((M.NONE, 'none'), (M.LRELU, 'lrelu'), (M.WALK, 'walk')):
        walk = epi == M.WALK
        want, bound = M.linear_fwd(x, w, b, epi, res=res if walk else None, a=a if walk else None)
        runs = [_fwd(d['x'], d['w'], d['b'], epi, d['res'] if walk else None, d['a'] if walk else None, B, Kd, N) for _ in range(2)]
        torch.cuda.synchronize()
        assert all(untouched(buf, y) for buf, y in runs), (tag, name)
        assert torch.equal(runs[0][1], runs[1][1]), (tag, name, 'two launches differ')
        s = _note('fwd %s' % name, runs[0][1], want, bound)
        assert s <= 1.0, (tag, name, s)
        for want_gx in (True, False):
            for slices, gx_add in ((K.linear_rows_slices(N), want_gx and epi == M.LRELU), (1 if N == 64 else 2 * K.linear_rows_slices(N), False)):
                if not want_gx and slices != K.linear_rows_slices(N):
                    continue
                want = M.linear_bwd(g, x, w, epi, y=yact, a=a, want_gx=want_gx, gx_add=add if gx_add else None)
                runs = [_bwd(d['g'], d['x'], d['w'], epi, d['yact'] if epi == M.LRELU else None, d['a'] if walk else None, d['add'] if gx_add else None,
                             want_gx, B, Kd, N, slices) for _ in range(2)]
                torch.cuda.synchronize()
                for k in want:
                    assert all(untouched(*r[k]) for r in runs), (tag, name, k)
                    assert torch.equal(runs[0][k][1], runs[1][k][1]), (tag, name, k, 'two launches differ')
                    s = _note('bwd %s %s' % (name, k), runs[0][k][1], *want[k])
                    assert s <= 1.0, (tag, name, k, slices, s)
                if 'ws' in runs[0]:
                    assert untouched(*runs[0]['ws'])
                if not want_gx:
                    assert 'gx' not in runs[0]


def test_kernels_refuse_what_they_are_not_built_for():
    x, w, b = torch.zeros(2, 96, device=DEV), torch.zeros(64, 96, device=DEV), torch.zeros(64, device=DEV)
    with pytest.raises(_lib.L2IError, match='multiples of 64'):
        K.linear_rows(x, w, b)                                              # K = 96
    with pytest.raises(_lib.L2IError, match='multiples of 64'):
        K.linear_rows_bwd(torch.zeros(2, 64, device=DEV), x, w)
    with pytest.raises(_lib.L2IError, match='multiples of 64'):
        K.linear_rows(torch.zeros(2, 64, device=DEV), torch.zeros(96, 64, device=DEV), torch.zeros(96, device=DEV))      # N = 96
    x, w = torch.zeros(2, 64, device=DEV), torch.zeros(128, 64, device=DEV)
    with pytest.raises(_lib.L2IError):
        K.linear_rows_bwd(torch.zeros(2, 128, device=DEV), x, w, slices=3)  # does not divide N
    with pytest.raises(_lib.L2IError):
        K.linear_rows_bwd(torch.zeros(2, 128, device=DEV), x, w, slices=1)  # 128 rows a slice
    with pytest.raises(_lib.L2IError):
        K.linear_rows_bwd(torch.zeros(2, 128, device=DEV), x, w, K.LINEAR_LRELU)          # the mask's y is missing
    with pytest.raises(_lib.L2IError):
        K.linear_rows(x[:, :0].reshape(0, 64), w, torch.zeros(128, device=DEV))           # B = 0
    buf = torch.zeros(2 * 64 + 1, device=DEV)
    with pytest.raises(_lib.L2IError, match='16-byte'):
        K.linear_rows(buf[1:].view(2, 64), w, torch.zeros(128, device=DEV))               # x one float into a buffer
    torch.cuda.synchronize()


# ---- (B) the module --------------------------------------------------------------------------------------------------------------------------------
def _module(tag):
    state, z, alpha, r = case(tag)
    walk = pg.WalkMlpZ3(tool.CASES[tag]['dim_z'], 6, 1, ['Smiling'])
    walk.load_state_dict({k: T(v) for k, v in state.items()})
    return walk.to(DEV), state, z, alpha, r


@pytest.fixture
def calls(monkeypatch):
    """Counts library calls by entry-point name."""
    seen = []
    real = _lib.call

    def counting(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(_lib, 'call', counting)
    return seen


@pytest.mark.parametrize('tag', ['s', 'l'])
def test_module_reproduces_the_fixture_inside_the_models_bounds_within_the_launch_budget(golden, calls, tag):
    g = golden('walk_mlp')
    walk, state, z, alpha, r = _module(tag)
    zt = T(z).to(DEV).requires_grad_(True)
    z_new = walk(zt, T(alpha).to(DEV))
    torch.cuda.synchronize()
    assert calls == ['l2i_linear_rows_f32'] * 3, calls                     # forward: at most 3 library calls
    del calls[:]
    (z_new * T(r).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert [c for c in calls if c.startswith('l2i_linear')] == ['l2i_linear_rows_bwd_f32'] * 3 and len(calls) <= 6, calls     # backward: at most 6
    tol = dict(rtol=1e-3, atol=1e-4)
    grads = {k: p.grad.cpu().numpy() for k, p in walk.named_parameters()}
    np.testing.assert_allclose(z_new.detach().cpu().numpy(), g[tag + '.z_new'], **tol)
    np.testing.assert_allclose(zt.grad.cpu().numpy(), g[tag + '.grad.z'], **tol)
    for k in KEYS:
        if tag == 's' or k.endswith('bias'):
            np.testing.assert_allclose(grads[k], g['%s.grad.%s' % (tag, k)], err_msg=k, **tol)
        else:
            np.testing.assert_allclose(grads[k].astype(np.float64).sum(1), g['%s.grad.%s.rowsum' % (tag, k)], err_msg=k, **tol)
            np.testing.assert_allclose(grads[k].astype(np.float64).sum(0), g['%s.grad.%s.colsum' % (tag, k)], err_msg=k, **tol)
    f, b = M.walk_forward(z, alpha, state), M.walk_backward(z, alpha, state, r)
    shares = {'z_new': _note('module z_new', z_new, *f['z_new']), 'z': _note('module grad z', zt.grad, *b['z'])}
    shares.update({k: _note('module grad ' + k, walk.state_dict(keep_vars=True)[k].grad, *b[k]) for k in KEYS})
    print(tag, shares)
    assert max(shares.values()) <= 1.0, shares


def test_module_shapes_no_grad_and_frozen_z(monkeypatch):
    walk, state, z, alpha, r = _module('s')
    zd, ad = T(z).to(DEV), T(alpha).to(DEV)
    # a 1-D z is one sample: [1, dim_z], as torch's broadcasting gives
    one = walk(zd[0], ad[:1])
    assert tuple(one.shape) == (1, 64)
    assert M.share(one.detach().cpu().numpy(), *M.walk_forward(z[:1], alpha[:1], state)['z_new']) <= 1.0
    # alpha is one value per row
    with pytest.raises(RuntimeError, match=r'\(3, 2\).*\(3, 64\)'):
        walk(zd, torch.zeros(3, 2, device=DEV))
    # no_grad (apply_alpha): nothing is kept
    with torch.no_grad():
        out = walk(zd, ad)
    assert out.grad_fn is None and not out.requires_grad
    probe = pg._WalkMlpFn
    kept = []
    real = probe.forward

    class Spy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *a):
            y = real(ctx, *a)
            kept.append((len(ctx.to_save) if getattr(ctx, 'to_save', None) else 0, hasattr(ctx, 'weights')))
            return y
        backward = probe.backward
    monkeypatch.setattr(pg, '_WalkMlpFn', Spy)
    with torch.no_grad():
        walk(zd, ad)
    walk(zd, ad)
    monkeypatch.undo()
    assert kept == [(0, False), (3, True)], kept                            # z, h1, h2 and nothing else; nothing under no_grad
    # z frozen: the first layer's input gradient is not asked for, the parameters still get theirs
    z_new = walk(zd, ad)
    (z_new * T(r).to(DEV)).sum().backward()
    b = M.walk_backward(z, alpha, state, r, want_gz=False)
    assert all(M.share(p.grad.cpu().numpy(), *b[k]) <= 1.0 for k, p in walk.named_parameters())


# ---- (C) the graph ---------------------------------------------------------------------------------------------------------------------------------
WALK_SEED = 81


def _nets32(g_state):
    from latent2im_amd.perceptual import VGG19Prefix
    from latent2im_amd.regressor import ResNet50
    return (pg.Generator(g_state, device=DEV), ResNet50(synth.resnet50_state(seed=300), device=DEV), VGG19Prefix(synth.vgg19_prefix_state(seed=400), device=DEV),
            {'G': 'synthetic'})


def _graph(monkeypatch, nets=None, dt='f32', batch=2, walk_type='NNz'):
    monkeypatch.setattr(conv, 'PRECISION', dt)
    monkeypatch.setattr(constants, 'ALLOW_SYNTHETIC_WEIGHTS', True)
    monkeypatch.setattr(constants, 'BATCH_SIZE', batch)
    graph = pg.faceGraph(lr=1e-3, walk_type=walk_type, loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': 31}, layers=None, pgan_opts=None,
                         nets=nets)
    state = emu.seeded_state(graph.walk, WALK_SEED) if walk_type != 'linear' else None
    return graph, state


def test_default_walk_type_builds_the_mlp_walk_and_checkpoints_round_trip(monkeypatch, tmp_path):
    from tests.test_pggan_gpu import fixture_state
    graph, _ = _graph(monkeypatch, _nets32(fixture_state()))
    assert type(graph.walk) is pg.WalkMlpZ3 and graph.walk_type == 'NNz' and type(graph.optimizer) is torch.optim.Adam
    assert list(graph.walk.state_dict()) == KEYS and all(p.is_cuda for p in graph.walk.parameters())
    assert tuple(graph.walk.linear[0].weight.shape) == (1024, 512) and tuple(graph.walk.linear[4].weight.shape) == (512, 1024)
    graph.save_multi_models(str(tmp_path / 'model_w_0'), str(tmp_path / 'gan'))
    blob = open(str(tmp_path / 'model_w_0_walk_module.ckpt'), 'rb').read()
    assert b'graphs.pggan.transform_base' in blob and b'WalkMlpZ3' in blob
    before = {k: v.detach().clone() for k, v in graph.walk.state_dict().items()}
    with torch.no_grad():
        for p in graph.walk.parameters():
            p.zero_()
    graph.load_multi_models(str(tmp_path / 'model_w_0_walk_module.ckpt'), None)
    assert type(graph.walk) is pg.WalkMlpZ3 and type(graph.walk).__module__ == 'graphs.pggan.transform_base'
    assert all(torch.equal(graph.walk.state_dict()[k], before[k]) for k in KEYS)
    out, aorg = graph.apply_alpha({'z': synth.z_sample(2, seed=0)}, np.full((2, 1), 0.8))
    assert list(out.shape) == [2, 3, 128, 128] and list(aorg.shape) == [2, 1] and bool(torch.isfinite(out).all())


def _adam_reference(before, grads, lr=1e-3):
    """One torch.optim.Adam step (CPU, fp32, the graph's betas) on the downloaded gradients."""
    ps = [torch.nn.Parameter(before[k].clone()) for k in KEYS]
    for p, k in zip(ps, KEYS):
        p.grad = grads[k].clone()
    torch.optim.Adam(ps, lr=lr, betas=(0.5, 0.99)).step()
    return {k: p.detach() for k, p in zip(KEYS, ps)}


def test_training_step_gradients_vs_float64_oracle_and_adam(monkeypatch):
    """One walk_training_step at 256^2, batch 2, content on, fp32: every parameter gradient against the float64 composition of oracle/pggan.py's
    generator (with the regressor and VGG oracles) and the model, held per parameter tensor to what
    tests/test_pggan_gpu.py::test_pggan_graph_gradient_strong_walk_vs_float64_oracle accepts for the linear walk (max error under 5e-3 of the
    largest element); then the six tensors after the optimiser step against torch.optim.Adam on the downloaded gradients."""
    from oracle import nets as onets
    from oracle import pggan as opg
    from oracle import step as ostep
    st = synth.pggan_generator_state(seed=11)
    graph, wstate = _graph(monkeypatch, _nets32(st))
    before = {k: v.detach().cpu().clone() for k, v in graph.walk.state_dict().items()}
    z = T(synth.z_sample(2, seed=0)).float()
    loss, x0, x1, a_org, a_tgt = pg.walk_training_step(graph, z.to(DEV), np.full((2, 1), 0.3), no_content_loss=False)
    grads = {k: p.grad.detach().cpu().clone() for k, p in graph.walk.named_parameters()}
    after = {k: v.detach().cpu().clone() for k, v in graph.walk.state_dict().items()}
    dt = torch.float64
    P = {k: T(v).to(dt) for k, v in st.items()}
    PR, PV = ostep.to_torch(synth.resnet50_state(seed=300), dt), ostep.to_torch(synth.vgg19_prefix_state(seed=400), dt)
    with torch.no_grad():
        ox0 = opg.get_logits(P, z.to(dt))
        otarget, oeps = ostep.get_alphas_clamp(onets.resnet50_forward(PR, ox0)[:, [31]], torch.full((2, 1), 0.3, dtype=dt))
    zn = T(M.walk_forward(z.numpy(), oeps.numpy(), wstate)['z_new'][0]).requires_grad_(True)
    ox1 = opg.get_logits(P, zn)
    oreg = opg.reg_loss_quirk(onets.resnet50_forward(PR, ox1)[:, [31]], otarget)
    ocont, _ = ostep.content_loss(PV, ox0, ox1)
    oloss = opg.total_loss(oreg, ocont, None, no_content_loss=False, no_gan_loss=True)
    gz, = torch.autograd.grad(oloss, zn)
    want = M.walk_backward(z.numpy(), oeps.numpy(), wstate, gz.numpy(), want_gz=False)
    np.testing.assert_allclose(float(loss.detach()), float(oloss.detach()), rtol=1e-4)
    errs = {k: float(np.abs(grads[k].double().numpy() - want[k][0]).max() / np.abs(want[k][0]).max()) for k in KEYS}
    print(errs)
    assert max(errs.values()) < 5e-3, errs
    ref = _adam_reference(before, grads)
    step = {k: float((after[k] - ref[k]).abs().max()) for k in KEYS}
    assert max(step.values()) < 1e-6, step                                  # the multi-tensor tolerance of tests/test_h8_gpu.py's guarded-Adam test
    assert all(not torch.equal(after[k], before[k]) for k in KEYS)


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_training_step_on_the_16_bit_path(monkeypatch, dt):
    """The same step with the 16-bit networks: the z gradient that arrives at the walk (a hook on z_new) pushed through the float64 model bounds
    the parameter gradients, so the generator's rounding stays out of this test; finite loss, no skipped step, the scaler advanced once; the
    optimiser step against torch.optim.Adam."""
    from latent2im_amd import optim
    graph, wstate = _graph(monkeypatch, None, dt)
    assert type(graph.walk) is pg.WalkMlpZ3 and all(p.dtype == torch.float32 for p in graph.walk.parameters())
    assert isinstance(graph.optimizer, optim.GuardedAdam) == (dt == 'f16')
    before = {k: v.detach().cpu().clone() for k, v in graph.walk.state_dict().items()}
    seen = {}
    real = graph.get_z_new_tensor

    def spying(zz, alpha, **kw):
        out = real(zz, alpha, **kw)
        seen['z'], seen['alpha'] = zz.detach().cpu().numpy(), alpha.detach().cpu().numpy()
        out.register_hook(lambda gr: seen.__setitem__('g', gr.detach().cpu().numpy()))
        return out
    monkeypatch.setattr(graph, 'get_z_new_tensor', spying)
    loss, *_ = pg.walk_training_step(graph, synth.z_sample(2, seed=0), np.full((2, 1), 0.3), no_content_loss=False)
    torch.cuda.synchronize()
    assert loss.dtype == torch.float64 and np.isfinite(float(loss.detach()))
    assert np.isfinite(seen['g']).all() and np.abs(seen['g']).max() > 0
    grads = {k: p.grad.detach().cpu().clone() for k, p in graph.walk.named_parameters()}
    want = M.walk_backward(seen['z'], seen['alpha'], wstate, seen['g'], want_gz=False)
    shares = {k: _note('step %s grad %s' % (dt, k), grads[k], *want[k]) for k in KEYS}
    print(dt, shares)
    assert max(shares.values()) <= 1.0, shares
    if dt == 'f16':
        stats = graph.loss_scaler.stats()
        assert stats['skipped'] == 0 and stats['steps'] == 1 and stats['scale'] == 1.0, stats
    after = {k: v.detach().cpu().clone() for k, v in graph.walk.state_dict().items()}
    ref = _adam_reference(before, grads)
    step = {k: float((after[k] - ref[k]).abs().max()) for k in KEYS}
    assert max(step.values()) < 1e-6, step
    assert all(not torch.equal(after[k], before[k]) for k in KEYS)


# ---- (D) the driver --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('walk_type', [None, 'linear'])
def test_driver_trains_config_1_from_the_command_line(monkeypatch, tmp_path, walk_type):
    from latent2im_amd import trainer
    for name in ('ALLOW_SYNTHETIC_WEIGHTS', 'BATCH_SIZE'):
        monkeypatch.setattr(constants, name, getattr(constants, name))
    monkeypatch.setattr(conv, 'PRECISION', conv.PRECISION)
    models = str(tmp_path / 'models')
    argv = ['--model', 'pggan', '--transform', 'face', '--no_gan_loss', '--synthetic_weights', '--num_samples', '4', '--batch_size', '2', '--n_epoch', '1',
            '--learning_rate', '1e-3', '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt', '--models_dir', models, '--overwrite_config',
            '--seed', '3', '--model_save_freq', '1000'] + (['--walk_type', walk_type] if walk_type else [])
    state = np.random.get_state()
    try:
        trainer.main(multi_attr=False, argv=argv)
    finally:
        np.random.set_state(state)
    out = os.path.join(models, 'pggan_face_%s_lr0.001_l2' % (walk_type or 'NNz'))
    ckpt = os.path.join(out, 'model_w_1_final_walk_module.ckpt')
    assert os.path.isfile(ckpt), os.listdir(out)
    walk = torch.load(ckpt, map_location='cpu', weights_only=False)
    assert type(walk) is (pg.WalkLinearZ_free if walk_type else pg.WalkMlpZ3)
    assert all(bool(torch.isfinite(p).all()) for p in walk.parameters())
    log = open(os.path.join(out, 'log.txt')).read()
    assert log.count('T, epc, bst, lss, alpha') == 2                        # two iterations at batch 2


def test_driver_refuses_hip_graph_on_the_pggan_graph():
    from latent2im_amd import trainer

    class _Z:                                                               # a graph without get_w: refused before anything of it is used
        pass
    opt = type('O', (), dict(hip_graph=True, no_content_loss=False, no_gan_loss=True))()
    with pytest.raises(NotImplementedError, match='hip_graph'):
        trainer.train_step(_Z(), np.zeros((2, 512)), ['Smiling'], opt=opt)
