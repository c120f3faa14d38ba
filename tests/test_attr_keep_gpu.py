"""The attribute-preservation loss of walk training (--attr_keep) on the MI355X: the term inside one training step of the StyleGAN2 graph against the
float64 head on the step's own regressor features (tests/regkeep_ref.py) and against torch's composite pushed through the same backward, the other
precisions, the choice of the kept columns and the constructor's refusals, the replayed step of both graphs, and the drivers."""
import os
import types

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, capture, constants, conv, graph, selfcheck, synth
from tests import regkeep_ref as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMILING = 31


def grad_ok(a, b, frac_tol=5e-3, elem=2e-3, worst=0.1):
    """tests/test_networks_gpu.py:34-46, restated: at most 0.5 % of the entries may deviate by more than 2e-3 * max|g|, none by more than 10 %."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    m = float(b.abs().max())
    e = (a - b).abs()
    frac = float((e > elem * m).double().mean())
    assert frac <= frac_tol and float(e.max()) <= worst * m, (frac, float(e.max()) / m)


def close(a, b, rtol, atol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and bool(((a - b).abs() <= atol + rtol * b.abs()).all()), float((a - b).abs().max())


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _recording_features(monkeypatch, g):
    """The pooled features the step's regressor passes produce, in call order."""
    seen, real = [], g.regressor.features

    def features(img):
        out = real(img)
        seen.append(out)
        return out
    monkeypatch.setattr(g.regressor, 'features', features)
    return seen


def _recording_calls(monkeypatch):
    seen, real = [], _lib.call

    def call(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(_lib, 'call', call)
    return seen


def _step(g, zs, alpha, weight, **flags):
    torch.manual_seed(5)                                # fixed generator noise
    g._init_attr_keep(weight, None)
    r = capture.forward_backward(g, torch.Tensor(zs).to(g.device), torch.tensor(alpha).float().to(g.device), **flags)
    torch.cuda.synchronize()
    return g.walk.w.grad.detach().clone(), r


def _head_model(g, feat1, feat0, target, c_reg):
    """tests/regkeep_ref.py's float64 model of the step's head on the step's own features."""
    c = dict(feat1=feat1.detach().float().cpu().numpy(), feat0=feat0.detach().float().cpu().numpy(), fc_w=g.regressor.fc_w.cpu().numpy(),
             fc_b=g.regressor.fc_b.cpu().numpy(), cols=np.array(g.attrIdx, dtype=np.int64), keep=np.array(g.keepIdx, dtype=np.int64),
             target=target.detach().float().cpu().numpy(), nan_row=None, equal_rows=(), c_reg=float(c_reg), w_keep=float(g.attr_keep))
    return M.model(c)


def test_weight_zero_is_the_step_as_it_was(monkeypatch):
    """The default: the new entry is never called, nothing is stashed, last_terms['keep'] is None."""
    try:
        g = selfcheck.build_graph(32, ['Smiling'], 2)
        assert g.attr_keep == 0.0 and g.keepIdx is None
        seen = _recording_calls(monkeypatch)
        zs, alpha = synth.z_sample(2, seed=3), np.ones((2, 1)) * 0.3
        r = capture.forward_backward(g, torch.Tensor(zs).to(g.device), torch.tensor(alpha).float().to(g.device))
        torch.cuda.synchronize()
        assert 'l2i_reg_bce_keep_f32' not in seen and seen.count('l2i_reg_bce_f32') == 1
        assert r['terms']['keep'] is None and g.last_terms['keep'] is None and g._org_feat is None and g.last_keep_preds is None
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_term_inside_one_graph_step(monkeypatch):
    """Batch 2 at 32^2, fp32, no content / GAN loss, fixed noise: loss = reg + 0.5 keep to float64 rounding; keep is the float64 head on the step's
    own features inside the kernel's bound; (walk gradient with W = 0.5) - (walk gradient with W = 0) is the gradient of torch's float64 composite
    0.5 * mean|fc(feat1) - fc(feat0)| pushed through the same regressor and generator backward."""
    try:
        g = selfcheck.build_graph(32, ['Smiling'], 2)
        zs, alpha = synth.z_sample(2, seed=3), np.ones((2, 1)) * 0.3
        flags = dict(no_content_loss=True, no_gan_loss=True)
        g0, r0 = _step(g, zs, alpha, 0.0, **flags)
        assert r0['terms']['keep'] is None
        feats = _recording_features(monkeypatch, g)
        seen = _recording_calls(monkeypatch)
        g1, r1 = _step(g, zs, alpha, 0.5, **flags)
        assert g.keepIdx == [i for i in range(40) if i != SMILING]
        assert seen.count('l2i_reg_bce_keep_f32') == 1 and 'l2i_reg_bce_f32' not in seen and len(feats) == 2          # one regressor pass an image, one head launch
        assert torch.equal(r0['x1'], r1['x1']) and torch.equal(r0['terms']['reg'], r1['terms']['reg'])
        reg, keep, loss = (float(r1['terms']['reg']), float(r1['terms']['keep']), float(r1['loss']))
        assert r1['loss'].dtype == torch.float64 and np.isfinite(keep) and keep > 0
        assert abs(loss - (reg + 0.5 * keep)) <= 2.0 ** -51 * (abs(reg) + abs(0.5 * keep))
        # the float64 head on the step's own features
        f0, f1 = feats
        ref = _head_model(g, f1, f0, torch.tensor(alpha), 1.0)
        w64, b64 = g.regressor.fc_w.double(), g.regressor.fc_b.double()
        keep_idx = torch.tensor(g.keepIdx, device=DEV)
        want = float(((f1.detach().double() @ w64.t() + b64) - (f0.detach().double() @ w64.t() + b64))[:, keep_idx].abs().mean())
        assert abs(want - ref['loss'][1]) <= 1e-12
        print('attr_keep f32 keep %.9g float64 %.9g err %.3e bound %.3e' % (keep, want, abs(keep - want), ref['loss_bound'][1]))
        assert abs(keep - want) <= ref['loss_bound'][1]
        pk = g.last_keep_preds
        assert pk is not None and tuple(pk.shape) == (2, 39, 2) and M.ratio(pk.cpu().numpy(), ref['pkeep'], ref['pkeep_bound']) <= 1.0
        monkeypatch.undo()
        # the expected gradient difference
        g._init_attr_keep(0.0, None)
        torch.manual_seed(5)
        feed, r = capture.forward(g, torch.Tensor(zs).to(g.device), torch.tensor(alpha).float().to(g.device))
        assert torch.equal(r['x1'], r1['x1'])
        e1 = g.regressor.features(feed['logit'])
        with torch.no_grad():
            e0 = g.regressor.features(feed['org'])
        comp = 0.5 * ((e1.double() @ w64.t() + b64) - (e0.double() @ w64.t() + b64))[:, keep_idx].abs().mean()
        g.optimizers.zero_grad()
        comp.backward()
        want_g = g.walk.w.grad.detach().clone()
        assert float(want_g.abs().max()) > 0
        grad_ok(g1 - g0, want_g)
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


@pytest.mark.parametrize('precision', ('bf16x3', 'bf16', 'f16'))
def test_term_beside_the_other_precisions(monkeypatch, precision):
    """--precision bf16x3 / bf16 / f16 at 64^2: the networks change their matrix path, the head stays fp32 — the term is the float64 head on the step's
    own features inside the kernel's bound, and the step's gradient is finite and not zero."""
    saved = conv.PRECISION
    try:
        conv.PRECISION = precision
        g = selfcheck.build_graph(64, ['Smiling'], 2, attr_keep=0.5)
        feats = _recording_features(monkeypatch, g)
        zs, alpha = synth.z_sample(2, seed=3), np.ones((2, 1)) * 0.3
        r = capture.forward_backward(g, torch.Tensor(zs).to(g.device), torch.tensor(alpha).float().to(g.device), no_content_loss=True, no_gan_loss=True)
        torch.cuda.synchronize()
        assert conv.PRECISION == precision and torch.isfinite(g.walk.w.grad).all() and float(g.walk.w.grad.abs().max()) > 0
        f0, f1 = feats
        assert f0.dtype == f1.dtype == torch.float32
        ref = _head_model(g, f1, f0, torch.tensor(alpha), 1.0)
        keep = float(r['terms']['keep'])
        print('attr_keep %s keep %.9g float64 %.9g err %.3e bound %.3e' % (precision, keep, ref['loss'][1], abs(keep - ref['loss'][1]), ref['loss_bound'][1]))
        assert np.isfinite(keep) and keep > 0 and abs(keep - ref['loss'][1]) <= ref['loss_bound'][1]
    finally:
        conv.PRECISION = saved
        constants.resolution, constants.BATCH_SIZE = 256, 4


def _face_graph(names, **kw):
    return dict(lr=1e-3, walk_type='linear', loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={n: i for i, n in enumerate(names)}, layers=None,
                stylegan_opts=types.SimpleNamespace(latent='w'), **kw)


def test_kept_columns_and_constructor_refusals():
    try:
        g = selfcheck.build_graph(32, ['Smiling'], 2, attr_keep=0.5)
        nets = (g.module.netG, g.module.netD, g.regressor, g.vgg19, g.weight_sources)
        with open(os.path.join(ROOT, 'dataset', 'attributes_celeba.txt')) as f:
            names = [l.strip() for l in f if l.strip()]
        table = {n: i for i, n in enumerate(names)}
        assert g.attr_keep == 0.5 and g.keepIdx == [i for i in range(40) if i != table['Smiling']] and len(g.keepIdx) == 39
        assert g._keep_columns().tolist() == g.keepIdx and g._keep_columns().dtype == torch.long
        g2 = graph.faceGraph(**_face_graph(names, nets=nets, attr_keep=0.25, attr_keep_attrs=['Young', 'Eyeglasses']))
        assert g2.keepIdx == [table['Young'], table['Eyeglasses']] and g2.attr_keep == 0.25
        g3 = graph.faceGraph(**dict(_face_graph(names, nets=nets, attr_keep=1.0), attrList=['Smiling', 'Young']))
        assert g3.keepIdx == [i for i in range(40) if i not in (table['Smiling'], table['Young'])] and len(g3.keepIdx) == 38
        off = graph.faceGraph(**_face_graph(names, nets=nets))
        assert off.attr_keep == 0.0 and off.keepIdx is None
        # a graph rebuilt with the option (eval.py / vis_w.py from a run's opt.yml) never runs or prepares the term: inference stashes nothing
        zs = synth.z_sample(2, seed=3)
        want = off.apply_alpha({'z': zs}, np.ones((2, 1)) * 0.3)
        got = g.apply_alpha({'z': zs}, np.ones((2, 1)) * 0.3)
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])          # (alpha_org, original image): the two graphs' walks differ
        g.sweep({'z': zs}, [np.ones((2, 1)) * a for a in (0.2, 0.7)])
        g.get_reg_preds(got[0])
        assert g._org_feat is None and g.last_keep_preds is None and g.last_terms is None
        for kw, why in ((dict(attr_keep=0.5, attr_keep_attrs=['Smiling_']), 'not in the attribute table'),
                        (dict(attr_keep=0.5, attr_keep_attrs=['Young', 'Smiling']), 'trained by this walk'),
                        (dict(attr_keep=0.5, attr_keep_attrs=[]), 'no regressor output is left'),
                        (dict(attr_keep=0.5, attrList=list(names)), 'no regressor output is left'),
                        (dict(attr_keep=0.5, attr_keep_attrs=['Young'] * 65), 'at most 64'),
                        (dict(attr_keep=-0.5), '>= 0'),
                        (dict(attr_keep_attrs=['Young']), 'needs attr_keep'),
                        (dict(attr_keep=0.0, attr_keep_attrs=['Young']), 'needs attr_keep')):
            with pytest.raises(ValueError, match=why):
                graph.faceGraph(**dict(_face_graph(names, nets=nets), **kw))
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_replayed_step_matches_the_eager_step():
    """The StyleGAN2 graph's captured_step with the term on against eager steps: the comparison of
    tests/test_networks_gpu.py::test_hipgraph_captured_step_matches_eager (images rtol 1e-4 / atol 1e-5, loss 1e-5 / 1e-6, gradient and walk under 1e-3 of
    the largest entry), two optimiser steps at 64^2, batch 2, full loss.  The term is held by the loss's relative 1e-5 alone, with no absolute allowance
    (measured on the MI355X: the replayed term is the eager one bit for bit)."""
    try:
        size, batch = 64, 2
        zs = [synth.z_sample(batch, seed=40 + i) for i in range(2)]
        al = [np.ones((batch, 1)) * a for a in (0.3, 0.8)]
        ge = selfcheck.build_graph(size, ['Smiling'], batch, lr=1e-3, attr_keep=0.5)
        eager = []
        for i in range(2):
            eager.append(selfcheck.run_step(ge, zs[i], al[i]))
            eager[-1]['pkeep'] = ge.last_keep_preds.detach().clone()
            assert ge._org_feat is None                           # the stash is consumed by the step
        gc_ = selfcheck.build_graph(size, ['Smiling'], batch, lr=1e-3, attr_keep=0.5)
        step = gc_.captured_step(batch, 1)
        assert isinstance(step, capture.CapturedStep)
        for i in range(2):
            r = step(zs[i], al[i])
            torch.cuda.synchronize()
            e = eager[i]
            close(r['x1'], e['x1'], 1e-4, 1e-5)
            close(r['x0'], e['x0'], 1e-4, 1e-5)
            close(r['eps'], e['eps'], 1e-4, 1e-6)
            close(r['loss'], e['loss'], 1e-5, 1e-6)
            keep, keep_e = float(r['terms']['keep']), float(e['terms']['keep'])
            print('attr_keep replay step %d keep %.9g eager %.9g diff %.3e' % (i, keep, keep_e, abs(keep - keep_e)))
            assert keep > 0 and abs(keep - keep_e) <= 1e-5 * abs(keep_e)
            assert relmax(r['grad'], e['grad']) < 1e-3
        assert relmax(gc_.walk.w, ge.walk.w) < 1e-3 and not torch.equal(gc_.walk.w.detach().cpu(), torch.from_numpy(synth.walk_init(1, 10, seed=7)).float())
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_pggan_replayed_step_matches_the_eager_step(monkeypatch):
    """The PGGAN graph (no_gan_loss=True; the term through the entry's K = 0 mode beside the graph's own BCE) replayed against eager steps: the
    comparison of tests/test_pggan_graph_gpu.py::test_f32_replayed_steps_match_eager_steps — equal bits where the eager step is bit-reproducible run to
    run, else images 1e-4 / 1e-5, loss 1e-5 / 1e-6, gradients under 1e-3 of the largest entry."""
    from latent2im_amd import pggan as pg
    from tests import emu
    monkeypatch.setattr(conv, 'PRECISION', 'f32')
    monkeypatch.setattr(constants, 'ALLOW_SYNTHETIC_WEIGHTS', True)
    monkeypatch.setattr(constants, 'BATCH_SIZE', 2)
    nets = pg.load_networks(torch.device(DEV, torch.cuda.current_device()), need_vgg=False)

    def make():
        gr = pg.faceGraph(lr=1e-3, walk_type='NNz', loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': SMILING}, layers=None, pgan_opts=None,
                          nets=nets, attr_keep=0.5)
        emu.seeded_state(gr.walk, 81)
        return gr

    def eager_steps(gr):
        out = []
        for z, a in zip(zs, al):
            loss, x0, x1, a0, target = pg.walk_training_step(gr, z, a, no_content_loss=True, no_gan_loss=True)
            torch.cuda.synchronize()
            assert gr._org_feat is None                               # the stash is consumed by the step
            out.append(dict(loss=loss.detach().clone(), x0=x0.detach().clone(), x1=x1.detach().clone(), a0=a0.detach().clone(), target=target.detach().clone(),
                            keep=gr.last_terms['keep'].clone(), reg=gr.last_terms['reg'].clone(), pkeep=gr.last_keep_preds.detach().clone(),
                            grads=[p.grad.detach().clone() for p in gr.walk.parameters()]))
        return out

    def walk_of(gr):
        return [p.detach().clone() for p in gr.walk.parameters()]
    zs = [synth.z_sample(2, seed=40 + i) for i in range(2)]
    al = [np.full((2, 1), a) for a in (0.3, -0.2)]
    ge = make()
    n_out = int(ge.regressor.fc_w.shape[0])
    assert ge.keepIdx == [i for i in range(n_out) if i != SMILING]
    w0 = walk_of(ge)
    eager = eager_steps(ge)
    g2 = make()
    again = eager_steps(g2)
    exact = all(torch.equal(a[k], b[k]) for a, b in zip(eager, again) for k in ('loss', 'x1', 'keep')) \
        and all(torch.equal(x, y) for a, b in zip(eager, again) for x, y in zip(a['grads'], b['grads'])) \
        and all(torch.equal(x, y) for x, y in zip(walk_of(ge), walk_of(g2)))
    print('eager fp32 step with the term bit-reproducible run to run:', exact)
    for e in eager:
        reg, keep = float(e['reg']), float(e['keep'])
        assert keep > 0 and abs(float(e['loss']) - (reg + 0.5 * keep)) <= 2.0 ** -50 * (abs(reg) + abs(0.5 * keep))
    gc_ = make()
    step = gc_.captured_step(2, 1, no_content_loss=True, no_gan_loss=True)
    assert isinstance(step, capture.CapturedZStep)
    assert all(torch.equal(a, b) for a, b in zip(w0, walk_of(gc_)))            # warm-up and capture ran no update
    for i in range(2):
        r = step(zs[i], al[i])
        torch.cuda.synchronize()
        e = eager[i]
        if exact:
            assert torch.equal(r['loss'], e['loss']) and torch.equal(r['x1'], e['x1']) and torch.equal(r['x0'], e['x0'])
            assert torch.equal(r['terms']['keep'], e['keep'])
            assert all(torch.equal(a, b) for a, b in zip(r['grads'], e['grads']))
        else:
            close(r['x1'], e['x1'], 1e-4, 1e-5)
            close(r['x0'], e['x0'], 1e-4, 1e-5)
            close(r['loss'], e['loss'], 1e-5, 1e-6)
            assert abs(float(r['terms']['keep']) - float(e['keep'])) <= 1e-5 * abs(float(e['keep']))          # the loss's relative 1e-5, no absolute allowance
            assert max(relmax(a, b) for a, b in zip(r['grads'], e['grads'])) < 1e-3
        assert torch.equal(r['a0'], e['a0']) or relmax(r['a0'], e['a0']) < 1e-4
        assert torch.equal(r['target'], (r['a0'] + torch.as_tensor(al[i], dtype=torch.float32, device=DEV)).clamp(0, 1))
        assert r['terms']['gan'] is None and r['terms']['cont'] is None
    if exact:
        assert all(torch.equal(a, b) for a, b in zip(walk_of(gc_), walk_of(ge)))
    else:
        assert max(relmax(a, b) for a, b in zip(walk_of(gc_), walk_of(ge))) < 1e-3
    assert all(not torch.equal(a, b) for a, b in zip(walk_of(gc_), w0))        # the walk moved


def _train_argv(models, *extra):
    return ['--model', 'stylegan_v2_real', '--transform', 'face', '--num_samples', '4', '--learning_rate', '1e-3', '--latent', 'w', '--walk_type', 'linear',
            '--loss', 'l2', '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt', '--models_dir', models, '--overwrite_config',
            '--resolution', '32', '--batch_size', '2', '--n_epoch', '1', '--seed', '3', '--synthetic_weights', '--max_iters', '2', '--no_gc_freeze'] + list(extra)


@pytest.mark.parametrize('mode', ('eager', 'hip_graph', 'no_flag'))
def test_train_cli(tmp_path, mode):
    """train.py --attr_keep 0.5 --synthetic_weights --max_iters 2, eager and --hip_graph: two finite losses, the flag in opt.yml and its round trip
    through --config_file, and the step is not sent to the eager route; a run without the flag writes an opt.yml without the key."""
    import yaml
    from latent2im_amd import trainer
    from latent2im_amd.options import TrainOptions
    models = str(tmp_path / 'models')
    cwd, saved = os.getcwd(), constants.ALLOW_SYNTHETIC_WEIGHTS
    os.chdir(ROOT)
    try:
        extra = [] if mode == 'no_flag' else ['--attr_keep', '0.5'] + (['--hip_graph'] if mode == 'hip_graph' else [])
        trainer.main(multi_attr=False, argv=_train_argv(models, *extra))
        out = os.path.join(models, 'stylegan_v2_real_face_linear_lr0.001_l2_w')
        log = open(os.path.join(out, 'log.txt')).read()
        losses = [float(l.split(', ')[-2]) for l in log.splitlines() if 'T, epc, bst, lss, alpha:' in l]
        assert len(losses) == 2 and all(np.isfinite(losses))
        assert 'runs eagerly' not in log
        with open(os.path.join(out, 'opt.yml')) as f:
            dump = yaml.load(f, Loader=yaml.FullLoader)
        if mode == 'no_flag':
            assert 'attr_keep' not in dump and 'attr_keep_attrs' not in dump
            return
        assert dump['attr_keep'] == 0.5 and 'attr_keep_attrs' not in dump
        dump.pop('weight_sources')
        cfg = tmp_path / 'again.yml'
        cfg.write_text(yaml.dump(dump))
        again = TrainOptions().parse(print_opt=False, argv=['--config_file', str(cfg), '--models_dir', str(tmp_path / 'again')])
        assert again.attr_keep == 0.5 and bool(getattr(again, 'hip_graph', False)) == (mode == 'hip_graph')
    finally:
        os.chdir(cwd)
        constants.ALLOW_SYNTHETIC_WEIGHTS = saved
        constants.resolution, constants.BATCH_SIZE = 256, 4
