"""The identity-preservation loss of walk training (--id_loss) on the MI355X: the differentiable face branch (facenet.FaceIdFn) against the
float64 fixture (tests/golden/faceid.npz, tests/faceid_ref.py), the term inside one training step of the StyleGAN2 graph, the refusals, and
the drivers.  The measured figures go to profiles/faceid_contract_errors.txt."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from latent2im_amd import capture, constants, conv, face_specs, facenet, graph, selfcheck, synth
from tests import faceid_ref as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_report = {}


@pytest.fixture(scope='module', autouse=True)
def _write_report():
    yield
    if not _report:
        return
    lines = ['# the identity loss on the device (facenet.FaceIdFn) against the float64 model (tests/golden/faceid.npz): written by tests/test_faceid_gpu.py',
             '# loss: |gpu - float64| beside faceid_ref.loss_bound; gradient: max |gpu - float64| / max |float64| of d loss / d x1 beside',
             '# max(2 x the float32 restatement\'s own deviation, 1e-4); share_1e-3: the share of entries off by more than 1e-3 of the largest']
    lines += ['%-10s %s' % (k, _report[k]) for k in sorted(_report)]
    try:
        with open(os.path.join(ROOT, 'profiles', 'faceid_contract_errors.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
    except OSError:
        pass


@pytest.fixture(scope='module')
def net():
    return facenet.InceptionResnetV1(face_specs.facenet_state(seed=constants.SYNTH_SEED_F), device=DEV)


@pytest.fixture(scope='module')
def golden_faceid():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'faceid.npz'))


@pytest.mark.parametrize('name,res,seed', M.CASES, ids=[c[0] for c in M.CASES])
def test_loss_and_image_gradient_vs_float64(net, golden_faceid, monkeypatch, name, res, seed):
    """Both fixture cases: loss_id inside the model's bound, d loss_id / d x1 within max(2 x the stored float32-restatement deviation, 1e-4) of
    float64, relative to the largest entry (the rule of tests/test_facenet_gpu.py::test_embeddings_vs_float64).  No F.conv2d on the path.

    Measured on the MI355X (profiles/faceid_contract_errors.txt): up64 loss error 8.8e-8, gradient 5.6e-6 of the largest entry (bound 5.1e-4);
    down256 loss error 7.5e-9, gradient 3.2e-4 (bound 4.8e-2: the float32 restatement itself is 2.4e-2 off there, ReLU masks that flip)."""
    fx = golden_faceid
    x0, x1 = M.case_images(res, seed)
    if name + '.g_x1' in fx:
        want = fx[name + '.g_x1']
    else:                                               # the stored d loss / d r through the float64 adjoint of the resize (make_faceid.py)
        want, _ = M.resize_lin_bwd(fx[name + '.g_r'].astype(np.float64), x1)
    from tests.golden import make_faceid
    probe = make_faceid.probe_index(want.size, seed)
    assert np.abs(want.reshape(-1)[probe] - fx[name + '.g_x1_probe']).max() <= 1e-6 * np.abs(want).max()

    def refuse(*a, **k):
        raise AssertionError('torch.nn.functional.conv2d on the identity branch')
    monkeypatch.setattr(F, 'conv2d', refuse)
    monkeypatch.setattr(torch, 'conv2d', refuse)
    xg = torch.from_numpy(x1).to(DEV).requires_grad_(True)
    loss = net.id_distances(xg, torch.from_numpy(x0).to(DEV)).mean()
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    loss = loss.detach()
    got = xg.grad.double().cpu().numpy()
    err_l, bound_l = abs(float(loss) - float(fx[name + '.loss'])), M.loss_bound(float(fx[name + '.loss_dev32']))
    scale = np.abs(want).max()
    err_g, bound_g = np.abs(got - want).max() / scale, M.gradient_rule(float(fx[name + '.g_dev32']))
    share = float((np.abs(got - want) > 1e-3 * scale).mean())
    _report[name] = ('loss %.8f (float64 %.8f) err %.3e bound %.3e | gradient err %.3e bound %.3e (float32 restatement %.3e) share_1e-3 %.2e'
                     % (float(loss), float(fx[name + '.loss']), err_l, bound_l, err_g, bound_g, float(fx[name + '.g_dev32']), share))
    print(name, _report[name])
    assert got.shape == x1.shape and np.isfinite(got).all()
    assert err_l <= bound_l
    assert err_g <= bound_g


def test_two_passes_give_equal_bits(net):
    x0, x1 = M.case_images(64, 21)
    grads = []
    for _ in range(2):
        xg = torch.from_numpy(x1).to(DEV).requires_grad_(True)
        d = net.id_distances(xg, torch.from_numpy(x0).to(DEV))
        d.sum().backward()
        grads.append((d.detach().clone(), xg.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    xg = torch.from_numpy(x1).to(DEV).requires_grad_(True)                 # a second backward over a retained graph gives the first one's gradient
    d = net.id_distances(xg, torch.from_numpy(x0).to(DEV)).sum()
    a, = torch.autograd.grad(d, xg, retain_graph=True)
    b, = torch.autograd.grad(d, xg)
    assert torch.equal(a, b) and torch.equal(a, grads[0][1])
    with torch.no_grad():                                                  # and no tape is kept where no gradient is asked for
        assert torch.equal(net.id_distances(xg.detach(), torch.from_numpy(x0).to(DEV)), grads[0][0])


def grad_ok(a, b, frac_tol=5e-3, elem=2e-3, worst=0.1):
    """tests/test_networks_gpu.py:34-46, restated: at most 0.5 % of the entries may deviate by more than 2e-3 * max|g|, none by more than 10 %."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    m = float(b.abs().max())
    e = (a - b).abs()
    frac = float((e > elem * m).double().mean())
    assert frac <= frac_tol and float(e.max()) <= worst * m, (frac, float(e.max()) / m)


def _step_grad(g, zs, alpha, weight):
    torch.manual_seed(5)                                # fixed generator noise
    g.id_weight = weight
    r = capture.forward_backward(g, torch.Tensor(zs).to(g.device), torch.tensor(alpha).float().to(g.device), no_content_loss=True, no_gan_loss=True)
    return g.walk.w.grad.detach().clone(), r


def test_term_inside_one_graph_step():
    """Batch 2 at 32^2, no content / GAN loss, fixed noise: (walk gradient with W = 0.5) - (walk gradient with W = 0) = 0.5 J_G^T g_id, g_id the
    face branch's image gradient pushed through the generator's backward alone."""
    try:
        g = selfcheck.build_graph(32, ['Smiling'], 2)
        zs, alpha = synth.z_sample(2, seed=3), np.ones((2, 1)) * 0.3
        g0, r0 = _step_grad(g, zs, alpha, 0.0)
        assert g._face_net is None and r0['terms']['id'] is None          # W = 0: no face network is constructed
        g1, r1 = _step_grad(g, zs, alpha, 0.5)
        assert g._face_net is not None and g.weight_sources['F'].startswith('synthetic')
        assert torch.equal(r0['x1'], r1['x1'])
        lid = r1['terms']['id']
        assert torch.isfinite(lid) and 0.0 <= float(lid) <= 2.0
        torch.testing.assert_close(r1['loss'], r0['loss'] + 0.5 * lid, rtol=1e-5, atol=1e-6)
        # the expected difference
        torch.manual_seed(5)
        feed, r = capture.forward(g, torch.Tensor(zs).to(g.device), torch.tensor(alpha).float().to(g.device))
        assert torch.equal(r['x1'], r1['x1'])
        g_img, = torch.autograd.grad(g.get_id_loss(feed['org'], feed['logit']), feed['logit'], retain_graph=True)
        g.optimizers.zero_grad()
        feed['logit'].backward(0.5 * g_img)
        want = g.walk.w.grad.detach().clone()
        assert float(want.abs().max()) > 0
        grad_ok(g1 - g0, want)
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


@pytest.mark.parametrize('precision', ('bf16x3', 'bf16'))
def test_term_beside_the_other_precisions(net, precision):
    """--precision bf16x3 / bf16: the walk's networks change their matrix path, the face branch stays fp32 — its term is the fp32 net's on the
    step's own images, and the step's gradient is finite."""
    saved = conv.PRECISION
    try:
        conv.PRECISION = precision
        g = selfcheck.build_graph(64, ['Smiling'], 2)
        g.id_weight = 0.5
        zs, alpha = synth.z_sample(2, seed=3), np.ones((2, 1)) * 0.3
        r = capture.forward_backward(g, torch.Tensor(zs).to(g.device), torch.tensor(alpha).float().to(g.device), no_content_loss=True, no_gan_loss=True)
        assert conv.PRECISION == precision and torch.isfinite(g.walk.w.grad).all() and float(g.walk.w.grad.abs().max()) > 0
        conv.PRECISION = 'f32'
        want = net.id_distances(r['x1'].detach().float(), r['x0'].detach().float()).mean()
        assert torch.equal(r['terms']['id'], want)
    finally:
        conv.PRECISION = saved
        constants.resolution, constants.BATCH_SIZE = 256, 4


def _face_graph(**kw):
    with open(os.path.join(ROOT, 'dataset', 'attributes_celeba.txt')) as f:
        names = [l.strip() for l in f if l.strip()]
    return dict(lr=1e-3, walk_type='linear', loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={n: i for i, n in enumerate(names)}, layers=None, **kw)


def test_refusals(tmp_path):
    from latent2im_amd import pggan
    saved = conv.PRECISION, constants.ALLOW_SYNTHETIC_WEIGHTS, constants.facenet_path
    try:
        with pytest.raises(NotImplementedError, match='id_loss'):
            pggan.faceGraph(**_face_graph(pgan_opts=types.SimpleNamespace(dset='celebahq'), id_weight=0.5))
        constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS = 64, 2, True
        conv.PRECISION = 'f16'                                                 # refused where the term is trained with, not where a graph is built:
        g16 = graph.faceGraph(**_face_graph(stylegan_opts=types.SimpleNamespace(latent='w'), id_weight=0.5))      # eval.py / vis_w.py rebuild a run's graph
        for call in (lambda: g16.get_w_loss({'logit': None}), lambda: g16.captured_step(2, 1), g16.check_id_loss):
            with pytest.raises(NotImplementedError, match='id_loss.*fifth static gradient-scale exponent'):
                call()
        assert g16._face_net is None
        del g16
        conv.PRECISION = 'f32'
        g = graph.faceGraph(**_face_graph(stylegan_opts=types.SimpleNamespace(latent='w'), id_weight=0.5, facenet_ckpt=str(tmp_path / 'absent.pt')))
        assert g.captured_step(2, 1) is None                                   # --hip_graph: the step is not recorded with the term on
        constants.ALLOW_SYNTHETIC_WEIGHTS = False
        with pytest.raises(FileNotFoundError, match='face network'):         # a missing checkpoint without --synthetic_weights is an error
            g.face_net()
    finally:
        conv.PRECISION, constants.ALLOW_SYNTHETIC_WEIGHTS, constants.facenet_path = saved
        constants.resolution, constants.BATCH_SIZE = 256, 4


def _train_argv(models, *extra):
    return ['--model', 'stylegan_v2_real', '--transform', 'face', '--num_samples', '4', '--learning_rate', '1e-3', '--latent', 'w', '--walk_type', 'linear',
            '--loss', 'l2', '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt', '--models_dir', models, '--overwrite_config',
            '--resolution', '32', '--batch_size', '2', '--n_epoch', '1', '--seed', '3', '--synthetic_weights', '--max_iters', '2', '--no_gc_freeze',
            '--id_loss', '0.5'] + list(extra)


@pytest.mark.parametrize('hip_graph', (False, True), ids=('eager', 'hip_graph'))
def test_train_cli_with_id_loss(tmp_path, hip_graph):
    """train.py --id_loss 0.5 --synthetic_weights --max_iters 2: finite losses, the flag and the face network's source in opt.yml, and the
    round trip through opt.yml; with --hip_graph the step runs eagerly."""
    import yaml
    from latent2im_amd import trainer
    from latent2im_amd.options import TrainOptions
    models = str(tmp_path / 'models')
    cwd, saved = os.getcwd(), constants.ALLOW_SYNTHETIC_WEIGHTS
    os.chdir(ROOT)
    try:
        trainer.main(multi_attr=False, argv=_train_argv(models, *(['--hip_graph'] if hip_graph else [])))
        out = os.path.join(models, 'stylegan_v2_real_face_linear_lr0.001_l2_w')
        log = open(os.path.join(out, 'log.txt')).read()
        losses = [float(l.split(', ')[-2]) for l in log.splitlines() if 'T, epc, bst, lss, alpha:' in l]
        assert len(losses) == 2 and all(np.isfinite(losses))
        assert ('the identity branch is not recorded' in log) == hip_graph
        with open(os.path.join(out, 'opt.yml')) as f:
            dump = yaml.load(f, Loader=yaml.FullLoader)
        assert dump['id_loss'] == 0.5 and dump['weight_sources']['F'].startswith('synthetic')
        dump.pop('weight_sources')
        cfg = tmp_path / 'again.yml'
        cfg.write_text(yaml.dump(dump))
        again = TrainOptions().parse(print_opt=False, argv=['--config_file', str(cfg), '--models_dir', str(tmp_path / 'again')])
        assert again.id_loss == 0.5 and bool(getattr(again, 'hip_graph', False)) == hip_graph
    finally:
        os.chdir(cwd)
        constants.ALLOW_SYNTHETIC_WEIGHTS = saved
        constants.resolution, constants.BATCH_SIZE = 256, 4
