"""The resident regressor trainer — eager (regressor_train.train_step_resident) and replayed from one hipGraph (capture.CapturedRegressorStep) —
held to the bars of test_networks_gpu.test_regressor_training_step_vs_oracle at that test's shape, seeds and oracle (8 x 3 x 128 x 128,
oracle.nets.resnet50_train_step), and the driver's opt-in flags on a 13-image PNG set.

No bit equality with the non-resident path is asked: l2i_conv2d_wgrad_f32 sums by atomics and the in-place F(4x4) pack may differ from
torch's einsum by 1 ulp (tests/test_regtrain_ref_cpu.py)."""
import os

import numpy as np
import pytest
import torch

from latent2im_amd import capture, synth
from latent2im_amd import conv as C
from latent2im_amd import regressor_train as RT
from latent2im_amd.regressor import ResNet50
from oracle import nets as onets
from oracle import step as ostep
from tests import regtrain_ref as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
MOVED = ('conv1.weight', 'layer1.0.conv2.weight', 'layer3.5.conv3.weight', 'layer4.0.downsample.0.weight', 'fc.weight', 'layer2.1.bn2.weight')
STATS = ('bn1.running_mean', 'bn1.running_var', 'layer2.0.downsample.1.running_var', 'layer4.2.bn3.running_mean')


def close(a, b, rtol=1e-3, atol=1e-4):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


@pytest.fixture(scope='module')
def ref():
    """The oracle, once for both tests: the float64 gradient of step 1, the float32 state after step 1, and the float32 losses of three
    consecutive steps (one Adam state, as the trainer's)."""
    rs = np.random.RandomState(5)
    st = synth.resnet50_state(seed=300)
    data = T(rs.randn(8, 3, 128, 128).astype(np.float32) * 0.5)
    label = T(rs.rand(8, 40).astype(np.float32))
    P64 = {k: v.clone() for k, v in ostep.to_torch(st, torch.float64).items()}
    _, g64 = onets.resnet50_train_step(P64, data.double(), label.double(), lr=1e-4, steps=1)
    P1 = {k: v.clone() for k, v in ostep.to_torch(st).items()}
    lo1, g1 = onets.resnet50_train_step(P1, data, label, lr=1e-4, steps=1)
    P3 = {k: v.clone() for k, v in ostep.to_torch(st).items()}
    lo, _ = onets.resnet50_train_step(P3, data, label, lr=1e-4, steps=3)
    assert float(lo[0]) == float(lo1[0])
    return dict(st=st, data=data, label=label, g64=g64, g1=g1, P1=P1, losses=[float(x) for x in lo])


def _bars_after_step_one(ref, model, loss1):
    """test_regressor_training_step_vs_oracle's bars on the state a first step leaves behind (the gradients are still in the arena)."""
    close(loss1, ref['losses'][0], 1e-4, 1e-6)
    worst = (1.0, 0.0, '')
    for k, want in ref['g64'].items():
        got = model.grads[k].detach().double().cpu().reshape(-1)
        w_ = want.reshape(-1)
        cos = float(torch.dot(got, w_) / (got.norm() * w_.norm() + 1e-300))
        l2 = float((got - w_).norm() / (w_.norm() + 1e-300))
        worst = min(worst, (cos, l2, k))
        assert cos >= 0.999 and l2 <= 5e-2, (k, cos, l2)
    print('lowest cosine similarity with the float64 oracle gradient %.6f (relative L2 error %.2e) at %s' % worst)
    sd = model.state_dict()
    for k in STATS:
        close(sd[k], ref['P1'][k], 1e-3, 1e-5)
    assert int(sd['bn1.num_batches_tracked']) == 1
    for k in MOVED:
        w0 = T(np.asarray(ref['st'][k])).double()
        moved_ref, moved = ref['P1'][k].detach().double() - w0, sd[k].cpu().double() - w0
        gk = ref['g1'][k].double()
        clear = gk.abs() > 0.05 * gk.abs().max()
        assert float((moved - moved_ref)[clear].abs().max()) < 0.05e-4 and float(moved_ref[clear].abs().min()) > 0.5e-4, k


def _pointers(model, opt):
    p = {'arena': model.grad_arena.data_ptr()}
    for k, t in model.named_parameters():
        st = opt.state[t]
        p.update({k: t.data_ptr(), k + '.grad': t.grad.data_ptr(), k + '.m': st['exp_avg'].data_ptr(), k + '.v': st['exp_avg_sq'].data_ptr(),
                  k + '.step': st['step'].data_ptr()})
    for cv in model._convs():
        p.update({cv.name + '/' + n: t.data_ptr() for n, t in rr.derived_tensors(cv.fc).items()})
    return p


def _packs_are_current(model):
    """Every gather pack equals, bit for bit, the one a fresh FrozenConv2d builds from the weight as it is now (a stale repack fails here at once)."""
    for cv in model._convs():
        fresh = rr.derived_tensors(C.FrozenConv2d(cv.weight.clone(), stride=cv.stride, padding=cv.padding, device=DEV))
        for n, t in rr.derived_tensors(cv.fc).items():
            if 'wino' not in n:
                assert torch.equal(t, fresh[n].reshape(t.shape)), (cv.name, n)


def test_resident_eager_step_vs_oracle(ref):
    model = RT.TrainableResNet50(ref['st'], device=DEV, resident=True)
    opt = RT.make_optimizer(model, lr=1e-4, guarded=True)
    data, label = ref['data'].to(DEV), ref['label'].to(DEV)
    before = _pointers(model, opt)
    l1 = RT.train_step_resident(model, opt, data, label)
    _bars_after_step_one(ref, model, l1)
    l2 = RT.train_step_resident(model, opt, data, label)
    l3 = RT.train_step_resident(model, opt, data, label)
    print('losses %.6f %.6f %.6f, oracle %.6f %.6f %.6f' % ((float(l1), float(l2), float(l3)) + tuple(ref['losses'])))
    close(l2, ref['losses'][1], 2e-3, 1e-6)
    close(l3, ref['losses'][2], 2e-3, 1e-6)
    after = _pointers(model, opt)
    assert all(after[k] == v for k, v in before.items())
    assert all('wino' in k for k in set(after) - set(before))                # built on first use, by the first forward / backward; then in place too
    _packs_are_current(model)


def test_replayed_step_vs_oracle(ref, tmp_path):
    model = RT.TrainableResNet50(ref['st'], device=DEV, resident=True)
    opt = RT.make_optimizer(model, lr=1e-4, guarded=True)
    w0 = {k: t.clone() for k, t in model.state_dict().items()}
    step = capture.CapturedRegressorStep(model, opt, 8, 128)
    torch.cuda.synchronize()
    for k, t in model.state_dict().items():                                  # the warm-up and the capture itself change nothing
        assert torch.equal(t, w0[k]), k
    assert all(float(opt.state[p]['step']) == 0 for p in model.parameters())
    before = _pointers(model, opt)
    l1 = float(step(ref['data'], ref['label']))
    _bars_after_step_one(ref, model, torch.tensor(l1))
    l2 = float(step(ref['data'], ref['label']))
    l3 = float(step(ref['data'], ref['label']))
    print('losses %.6f %.6f %.6f, oracle %.6f %.6f %.6f' % ((l1, l2, l3) + tuple(ref['losses'])))
    close(l2, ref['losses'][1], 2e-3, 1e-6)                                   # computed on the updated, REPACKED weights and statistics
    close(l3, ref['losses'][2], 2e-3, 1e-6)
    assert all(int(bn.num_batches_tracked) == 3 for bn in model._bns())
    assert all(float(opt.state[p]['step']) == 3 for p in model.parameters())
    assert _pointers(model, opt) == before
    _packs_are_current(model)
    # checkpoint in the reference's format -> a NON-resident model and torch's own Adam; eval-mode forward of both states agree
    path = str(tmp_path / '003_dict.model')
    RT.save_ckpt(path, model, opt)
    plain = RT.TrainableResNet50(ref['st'], device=DEV)
    plain, popt = RT.load_ckpt(path, plain, RT.make_optimizer(plain))
    sd, sd2 = model.state_dict(), plain.state_dict()
    assert set(sd) == set(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert all(float(popt.state[p]['step']) == 3 for p in plain.parameters())
    x = ref['data'].to(DEV)
    f1 = ResNet50({k: v.cpu().numpy() for k, v in sd.items()}, device=DEV)(x)
    f2 = ResNet50({k: v.cpu().numpy() for k, v in sd2.items()}, device=DEV)(x)
    assert torch.equal(f1, f2)
    # and the reverse: a checkpoint written with torch's Adam loads into the guarded one
    RT.save_ckpt(path, plain, popt)
    back = RT.TrainableResNet50(ref['st'], device=DEV, resident=True)
    back, bopt = RT.load_ckpt(path, back, RT.make_optimizer(back, guarded=True))
    RT.train_step_resident(back, bopt, x, ref['label'].to(DEV))
    assert all(float(bopt.state[p]['step']) == 4 and bopt.state[p]['step'].is_cuda for p in back.parameters())


def _png_set(root, n=13, n_test=3):
    from PIL import Image
    rs = np.random.RandomState(9)
    os.makedirs(os.path.join(root, 'images', 'a'))
    os.makedirs(os.path.join(root, 'splits'))
    names = []
    with open(os.path.join(root, 'annotations.tsv'), 'w') as f:
        for i in range(n + n_test):
            name = 'a/%02d.png' % i
            h, w = 70 + 3 * (i % 4), 96 - 5 * (i % 3)
            Image.fromarray(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(root, 'images', name))
            f.write(name + '\t' + '\t'.join('%.4f,1.0' % v for v in rs.rand(40)) + '\n')
            names.append(name)
    with open(os.path.join(root, 'splits', 'training.txt'), 'w') as f:
        f.write('\n'.join(names[:n]) + '\n')
    with open(os.path.join(root, 'splits', 'test.txt'), 'w') as f:
        f.write('\n'.join(names[n:]) + '\n')
    return os.path.join(root, 'images'), os.path.join(root, 'annotations.tsv'), os.path.join(root, 'splits') + '/'


def test_driver_replays_full_batches_from_device_data(tmp_path, monkeypatch):
    images, tsv, splits = _png_set(str(tmp_path))
    train = RT.CustomDataset(images, RT.load_labelfile(tsv), splits + 'training.txt', image_size=64)
    assert len(train) == 13
    dd = RT.DeviceDataset(train)
    sel = [12, 0, 5, 5, 3]
    data, label = dd.batch(sel)
    want = [train[j] for j in sel]
    assert torch.equal(data.cpu(), torch.stack([b[0] for b in want])) and torch.equal(label.cpu(), torch.stack([b[1] for b in want]))
    with pytest.raises(IndexError):
        dd.indices([0, 13])
    replayed, eager = [], []
    call, step = capture.CapturedRegressorStep.__call__, RT.train_step_resident
    monkeypatch.setattr(capture.CapturedRegressorStep, '__call__', lambda self, *a, **k: replayed.append(float(call(self, *a, **k))) or self.loss)

    def counted(model, optimizer, data, label, update=True):
        loss = step(model, optimizer, data, label, update=update)
        if update and not torch.cuda.is_current_stream_capturing():
            eager.append((tuple(data.shape), float(loss)))
        return loss
    monkeypatch.setattr(RT, 'train_step_resident', counted)
    np.random.seed(3)
    out = str(tmp_path / 'ckpt')
    model = RT.main(images, tsv, splits, n_epoch=2, batch_size=4, out_dir=out, state=synth.resnet50_state(seed=300), image_size=64, hip_graph=True, device_data=True)
    assert len(replayed) == 6 and [s for s, _ in eager] == [(1, 3, 64, 64)] * 2          # 13 = 3 x 4 replayed + 1 ragged, eagerly, per epoch
    assert np.isfinite(replayed).all() and np.isfinite([l for _, l in eager]).all()
    assert model.resident and all(int(bn.num_batches_tracked) == 8 + 1 for bn in model._bns())      # 8 training batches + the test batch of epoch 2
    for e in (1, 2):
        ck = torch.load(os.path.join(out, '%03d_dict.model' % e), map_location='cpu')
        assert set(ck) == {'model', 'optm'} and ck['model']['fc.weight'].shape == (40, 2048)
        assert all(float(s['step']) == 4 * e for s in ck['optm']['state'].values())


def test_non_finite_gradient_skips_the_replayed_update():
    model = RT.TrainableResNet50(synth.resnet50_state(seed=300), device=DEV, resident=True)
    opt = RT.make_optimizer(model, guarded=True)
    step = capture.CapturedRegressorStep(model, opt, 4, 64)
    rs = np.random.RandomState(2)
    data, label = T(rs.randn(4, 3, 64, 64).astype(np.float32) * 0.5), T(rs.rand(4, 40).astype(np.float32))
    assert np.isfinite(float(step(data, label)))
    params = [p.clone() for p in model.parameters()]
    moments = [opt.state[p]['exp_avg'].clone() for p in model.parameters()]
    bad = label.clone()
    bad[1, 7] = float('inf')                                                  # the loss and every gradient behind it are non-finite; the forward is clean
    assert not np.isfinite(float(step(data, bad)))
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))
    assert all(torch.equal(opt.state[p]['exp_avg'], m) for p, m in zip(model.parameters(), moments))
    assert all(float(opt.state[p]['step']) == 1 for p in model.parameters())
    assert np.isfinite(float(step(data, label)))                              # and the next clean step updates again
    assert all(float(opt.state[p]['step']) == 2 for p in model.parameters())
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), params))
