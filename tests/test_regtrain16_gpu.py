"""The 16-bit regressor trainer (regressor_train.TrainableResNet50H8: h8 maps, l2i_conv2d_wgrad_h8, BatchNorm on csrc/l2i_train_h8.hip) — the whole
step at test_regressor_graph_gpu's shape, seeds and float64 oracle, for both element types.

The bars are not "close to fp32": 16-bit storage of a random-init net with batch statistics moves the gradient by 7 % (fp16) / 18 % (bf16) in
aggregate whatever the kernels do.  tests/golden/regtrain16_emulation.npz records what storage ALONE does (a float64 CPU emulation with a rounding
at every point where the GPU path stores a map, tests/golden/make_regtrain16.py) and the GPU step is held to that:
    each parameter's relative L2 deviation from the float64 gradient <= 1.5 x the emulation's for that parameter, the aggregate <= 1.25 x (two
    emulations that differ only in arithmetic differ by 0.85 - 1.15 x per parameter and 1.006 x in aggregate: single ReLU decisions flip);
    the losses of steps 1 - 3 within 4 x the emulation's deviation from float64 at that step, and strictly decreasing.
Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

from latent2im_amd import synth
from latent2im_amd import regressor_train as RT
from oracle import nets as onets
from oracle import step as ostep

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'regtrain16_emulation.npz')
STATS = ('bn1.running_mean', 'bn1.running_var', 'layer2.0.downsample.1.running_var', 'layer4.2.bn3.running_mean')
UNIT = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}
MIN_COS = {'f16': 0.99, 'bf16': 0.98}
ELEMS = ('f16', 'bf16')


@pytest.fixture(scope='module')
def ref():
    """test_regressor_graph_gpu's inputs and float64 oracle: the gradient of step 1 and the state (running statistics) it leaves."""
    rs = np.random.RandomState(5)
    st = synth.resnet50_state(seed=300)
    data = T(rs.randn(8, 3, 128, 128).astype(np.float32) * 0.5)
    label = T(rs.rand(8, 40).astype(np.float32))
    P64 = {k: v.clone() for k, v in ostep.to_torch(st, torch.float64).items()}
    lo, g64 = onets.resnet50_train_step(P64, data.double(), label.double(), lr=1e-4, steps=1)
    return dict(st=st, data=data, label=label, g64=g64, P1=P64, loss1=float(lo[0]), golden=dict(np.load(GOLDEN)))


def _fit(ref, elem):
    g = ref['golden']
    if not float(g[elem + '_agg_cos']) >= MIN_COS[elem]:
        raise RuntimeError('the recorded emulation of %s has aggregate cosine %.4f < %.2f: these inputs do not test a 16-bit trainer' % (elem, float(g[elem + '_agg_cos']), MIN_COS[elem]))
    assert abs(float(g['loss_f64'][0]) - ref['loss1']) <= 1e-9, 'the golden file was made from other inputs'
    return g


def _model(ref, elem):
    model = RT.TrainableResNet50H8(ref['st'], device=DEV, precision=elem, image_size=128, batch=8)
    return model, RT.make_optimizer(model, lr=1e-4, guarded=True)


@pytest.mark.parametrize('elem', ELEMS)
def test_step_vs_float64_oracle(ref, elem):
    g = _fit(ref, elem)
    model, opt = _model(ref, elem)
    assert model.loss_scale_log2 == (15 if elem == 'f16' else 0) and opt.scaler is model.scaler
    data, label = ref['data'].to(DEV), ref['label'].to(DEV)
    l1 = float(RT.train_step_resident(model, opt, data, label))
    grads = {k: t.detach().double().cpu() for k, t in model.grads.items()}
    arena = model.grad_arena.clone()
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    l2 = float(RT.train_step_resident(model, opt, data, label))
    l3 = float(RT.train_step_resident(model, opt, data, label))
    # ---- gradients
    names = [str(n) for n in g['names']]
    assert names == list(ref['g64']) and set(names) == set(grads)
    emu = dict(zip(names, g[elem + '_rel_l2'].astype(np.float64)))
    rel = {k: float((grads[k].reshape(-1) - ref['g64'][k].reshape(-1)).norm() / (ref['g64'][k].norm() + 1e-300)) for k in names}
    a = torch.cat([grads[k].reshape(-1) for k in names])
    b = torch.cat([ref['g64'][k].reshape(-1) for k in names])
    agg, cos = float((a - b).norm() / b.norm()), float(torch.dot(a, b) / (a.norm() * b.norm()))
    ratios = sorted(((rel[k] / emu[k], k) for k in names), reverse=True)
    print('rt16 step %s: aggregate relative L2 %.4f (emulation %.4f, ratio %.3f), cosine %.4f (emulation %.4f)'
          % (elem, agg, float(g[elem + '_agg_l2']), agg / float(g[elem + '_agg_l2']), cos, float(g[elem + '_agg_cos'])))
    print('rt16 step %s: per-parameter ratio to the emulation: max %.3f at %s (%.4f against %.4f), median %.3f, min %.3f'
          % (elem, ratios[0][0], ratios[0][1], rel[ratios[0][1]], emu[ratios[0][1]], ratios[len(ratios) // 2][0], ratios[-1][0]))
    # ---- losses
    want, emul = g['loss_f64'], g[elem + '_losses']
    got = (l1, l2, l3)
    lr = [abs(got[i] - float(want[i])) / abs(float(emul[i]) - float(want[i])) for i in range(3)]
    print('rt16 step %s: losses %.6f %.6f %.6f, emulation %.6f %.6f %.6f, float64 %.6f %.6f %.6f, deviation ratios %.2f %.2f %.2f'
          % ((elem,) + got + tuple(float(v) for v in emul) + tuple(float(v) for v in want) + tuple(lr)))
    # ---- running statistics
    u = UNIT[elem]
    sr = []
    for k in STATS:
        d = (sd[k].double() - ref['P1'][k].double()).abs()
        sr.append(float((d / (1e-5 + u + (1e-3 + u) * ref['P1'][k].double().abs())).max()))
    print('rt16 step %s: running statistics, worst deviation / bar %s' % (elem, ' '.join('%.3f' % v for v in sr)))
    assert all(np.isfinite(v) for v in got)
    for k in names:
        assert rel[k] <= 1.5 * emu[k], (k, rel[k], emu[k])
    assert agg <= 1.25 * float(g[elem + '_agg_l2'])
    assert all(r <= 4.0 for r in lr), lr
    assert l1 > l2 > l3
    assert max(sr) <= 1.0 and int(sd['bn1.num_batches_tracked']) == 1
    assert all(int(bn.num_batches_tracked) == 3 for bn in model._bns())
    assert opt.scaler.stats()['skipped'] == 0
    # ---- reproducible: a second model stepped on the same batch, bit for bit (conv1.weight alone still sums by atomics)
    other, oopt = _model(ref, elem)
    RT.train_step_resident(other, oopt, data, label)
    o = model.grad_offsets['conv1.weight']
    keep = torch.ones_like(arena, dtype=torch.bool)
    keep[o:o + model.stem.weight.numel()] = False
    assert torch.equal(arena.view(torch.int32)[keep], other.grad_arena.view(torch.int32)[keep])
    # ---- the checkpoint is the fp32 trainer's
    plain = RT.TrainableResNet50(ref['st'], device=DEV)
    plain.load_state_dict(model.state_dict())
    sd3, sdp = model.state_dict(), plain.state_dict()
    assert set(sd3) == set(sdp) and all(torch.equal(sd3[k], sdp[k]) for k in sd3)


def test_non_finite_gradient_skips_the_update_and_halves_the_scale(ref):
    model, opt = _model(ref, 'f16')
    rs = np.random.RandomState(2)
    data, label = T(rs.randn(4, 3, 64, 64).astype(np.float32) * 0.5).to(DEV), T(rs.rand(4, 40).astype(np.float32)).to(DEV)
    assert np.isfinite(float(RT.train_step_resident(model, opt, data, label)))
    params = [p.clone() for p in model.parameters()]
    planes = model.blocks[0]['c1'].h8.fwd_planes.clone()
    assert opt.scaler.stats()['scale'] == 1.0
    bad = label.clone()
    bad[1, 7] = float('inf')                                  # the forward is clean; the loss and every gradient behind it are not
    assert not np.isfinite(float(RT.train_step_resident(model, opt, data, bad)))
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))
    assert torch.equal(model.blocks[0]['c1'].h8.fwd_planes, planes)
    st = opt.scaler.stats()
    assert st['scale'] == 0.5 and st['skipped'] == 1 and all(float(opt.state[p]['step']) == 1 for p in model.parameters())
    assert np.isfinite(float(RT.train_step_resident(model, opt, data, label)))
    assert all(float(opt.state[p]['step']) == 2 for p in model.parameters())
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), params))
    assert not torch.equal(model.blocks[0]['c1'].h8.fwd_planes, planes), 'replan() did not rebuild the 16-bit planes from the updated master weight'


def test_driver_runs_f16_on_device_data(tmp_path):
    from tests.test_regressor_graph_gpu import _png_set
    import scene_regressor_256 as drv
    images, tsv, splits = _png_set(str(tmp_path))
    np.random.seed(3)
    out = str(tmp_path / 'ckpt')
    args = drv.parse_args(['--precision', 'f16', '--device_data', '--n_epoch', '1', '--batch_size', '4', '--image_size', '64', '--out_dir', out])
    assert args['precision'] == 'f16' and args['device_data'] is True
    model = RT.main(images, tsv, splits, state=synth.resnet50_state(seed=300), **args)
    assert isinstance(model, RT.TrainableResNet50H8) and model.precision == 'f16' and model.loss_scale_log2 == RT.regtrain_scale_for(64, 4)
    assert all(int(bn.num_batches_tracked) == 4 for bn in model._bns())               # 13 images = 3 x 4 + 1
    path = os.path.join(out, '001_dict.model')
    ck = torch.load(path, map_location='cpu')
    assert set(ck) == {'model', 'optm'} and all(float(s['step']) == 4 for s in ck['optm']['state'].values())
    plain = RT.TrainableResNet50(synth.resnet50_state(seed=300), device=DEV)
    plain, _ = RT.load_ckpt(path, plain, RT.make_optimizer(plain))
    sd, sd2 = model.state_dict(), plain.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert drv.parse_args(['--precision', 'bf16', '--loss_scale_log2', '0'])['loss_scale_log2'] == 0


def test_hip_graph_with_a_16_bit_precision_raises(tmp_path):
    with pytest.raises(NotImplementedError, match='follow-up'):
        RT.main(str(tmp_path), str(tmp_path / 'none.tsv'), str(tmp_path), precision='f16', hip_graph=True)
