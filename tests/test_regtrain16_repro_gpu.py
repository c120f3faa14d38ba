"""The 16-bit regressor step with the fixed-order stem gradient and the one-launch in-place repack (regressor_train.TrainableResNet50H8 on
l2i_conv2d_wgrad_img_h8 / l2i_repack_planes_h8), at 4 x 3 x 64 x 64, seed 300, both element types:
    (a) two fresh models stepped three times on the same batches agree bit for bit in every parameter, Adam moment, plane, running statistic and loss;
    (b) after a step the planes are H8Conv.repack / pack_weight_img_h8 of the master weights bit for bit, and no pointer has moved;
    (c) conv1.weight's gradient of a step is within the bound of tests/stemgrad16_ref.py of the float64 model evaluated on the step's own stored g_z0;
    (d) capture.CapturedRegressorStep records this model: three replays equal three eager steps from the same state bit for bit (everything of (a),
        the batch counters and the scaler's state), a replay with an inf label skips the update, halves the scale and leaves parameters and planes
        alone, the next replay steps again, and the ``dataset=`` form replays a batch equal to the staged form."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib, capture, conv, synth
from latent2im_amd import regressor_train as RT
from tests import stemgrad16_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ELEMS = ('f16', 'bf16')
B, S = 4, 64
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope='module')
def inputs():
    rs = np.random.RandomState(2)
    batches = [(T(rs.randn(B, 3, S, S).astype(np.float32) * 0.5), T(rs.rand(B, 40).astype(np.float32))) for _ in range(3)]
    return dict(st=synth.resnet50_state(seed=300), batches=batches)


def make(inputs, elem):
    model = RT.TrainableResNet50H8(inputs['st'], device=DEV, precision=elem, image_size=S, batch=B)
    assert model.stem_kernel and model.planes_kernel and model.planes is not None
    return model, RT.make_optimizer(model, lr=1e-4, guarded=True)


def plane_tensors(model):
    out = {'conv1/planes': model.stem.img.planes}
    for cv in model._convs()[1:]:
        out[cv.name + '/fwd'], out[cv.name + '/bwd'] = cv.h8.fwd_planes, cv.h8.bwd_planes
    return out


def state_tensors(model, opt, counters=False):
    out = dict(plane_tensors(model))
    for k, t in model.named_parameters():
        st = opt.state[t]
        out.update({k: t, k + '.m': st['exp_avg'], k + '.v': st['exp_avg_sq'], k + '.step': st['step']})
    for bn in model._bns():
        out[bn.name + '.running_mean'], out[bn.name + '.running_var'] = bn.running_mean, bn.running_var
        if counters:
            out[bn.name + '.num_batches_tracked'] = bn.num_batches_tracked
    if counters:
        out['scaler.scale'], out['scaler.state'] = opt.scaler.scale, opt.scaler.state
    return out


def bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same(a, b, what):
    assert set(a) == set(b)
    diff = [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]
    assert not diff, '%s: %d of %d tensors differ, first %s' % (what, len(diff), len(a), diff[:4])


def snapshot(tensors):
    return {k: t.detach().clone() for k, t in tensors.items()}


class _KeepStemMaps:
    """A stand-in for the range monitor: keeps what the step stores under T.g.stem (g_a0, g_z0)."""

    def __init__(self):
        self.maps = []

    def add(self, tag, t):
        if tag == 'T.g.stem':
            self.maps.append(t.detach().clone())


@pytest.mark.parametrize('elem', ELEMS)
def test_step_is_reproducible_in_place_and_inside_the_stem_bound(inputs, elem):
    runs = []
    for r in range(2):
        model, opt = make(inputs, elem)
        ptrs = {k: t.data_ptr() for k, t in plane_tensors(model).items()}
        losses = []
        for i, (data, label) in enumerate(inputs['batches']):
            if r == 0 and i == 0:
                model.monitor = keep = _KeepStemMaps()
            losses.append(RT.train_step_resident(model, opt, data.to(DEV), label.to(DEV)).clone())
            if r == 0 and i == 0:
                model.monitor = None
                # ---- (c) conv1.weight's gradient of this step against the float64 model on the stored g_z0
                g_z0 = keep.maps[1]
                assert tuple(g_z0.shape) == (B, 8, S // 2, S // 2, 8) and g_z0.dtype == sr.ELEM_DTYPES[elem]
                want, bound = sr.stem_wgrad(data, conv.from_h8(g_z0).cpu(), elem)
                unit = float(model.static) * float(opt.scaler.stats()['scale'])            # p.grad is the true gradient: back to the units of g_z0
                got = model.grads['conv1.weight'].detach().double().cpu() * unit
                err, b, ratio = sr.worst(got, want, bound)
                print('rt16 stem_wgrad in the step %s: error %.3g bound %.3g ratio %.3g (largest |dw| %.3g)' % (elem, err, b, ratio, float(want.abs().max())))
                assert ratio <= 1.0 and float(want.abs().max()) > 0
                # ---- (b) the planes are the torch packs of the masters, where they were
                for cv in model._convs()[1:]:
                    ref = conv.H8Conv(cv.weight.detach().cpu(), stride=cv.stride, padding=cv.padding, device='cpu', dtype=model.dtype)
                    assert torch.equal(bits(cv.h8.fwd_planes).cpu(), bits(ref.fwd_planes)) and torch.equal(bits(cv.h8.bwd_planes).cpu(), bits(ref.bwd_planes)), cv.name
                assert torch.equal(bits(model.stem.img.planes).cpu(), bits(conv.pack_weight_img_h8(model.stem.weight.detach().cpu(), dtype=model.dtype)))
        assert {k: t.data_ptr() for k, t in plane_tensors(model).items()} == ptrs, 'a plane set moved'
        assert all(np.isfinite(float(l)) for l in losses) and opt.scaler.stats()['skipped'] == 0
        runs.append((snapshot(state_tensors(model, opt)), losses))
    assert_same(runs[0][0], runs[1][0], 'two fresh models after three steps')
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(runs[0][1], runs[1][1])), 'the losses differ'
    print('rt16 repro %s: %d tensors and 3 losses bit-equal between two runs; losses %s' % (elem, len(runs[0][0]), ' '.join('%.6f' % float(l) for l in runs[0][1])))


@pytest.mark.parametrize('elem', ELEMS)
def test_replay_equals_eager(inputs, elem):
    eager, eopt = make(inputs, elem)
    model, opt = make(inputs, elem)
    before = snapshot(state_tensors(model, opt, counters=True))
    ptrs = {k: t.data_ptr() for k, t in plane_tensors(model).items()}
    step = capture.CapturedRegressorStep(model, opt, B, S)
    torch.cuda.synchronize()
    assert_same(before, state_tensors(model, opt, counters=True), 'the warm-up and the capture changed the state')
    for i, (data, label) in enumerate(inputs['batches']):
        want = RT.train_step_resident(eager, eopt, data.to(DEV), label.to(DEV))
        got = step(data, label)
        assert torch.equal(bits(got), bits(want)), 'loss of step %d: replay %r eager %r' % (i + 1, float(got), float(want))
    assert_same(state_tensors(eager, eopt, counters=True), state_tensors(model, opt, counters=True), 'three replays against three eager steps')
    assert opt.scaler.stats() == eopt.scaler.stats() and opt.scaler.stats()['steps'] == 3
    assert {k: t.data_ptr() for k, t in plane_tensors(model).items()} == ptrs
    # ---- a non-finite gradient: the replayed update is skipped, the scale halves, parameters and planes stay
    data, label = inputs['batches'][0]
    kept = snapshot({k: t for k, t in state_tensors(model, opt).items() if 'running' not in k})
    bad = label.clone()
    bad[1, 7] = float('inf')
    assert not np.isfinite(float(step(data, bad)))
    assert_same(kept, {k: t for k, t in state_tensors(model, opt).items() if 'running' not in k}, 'a skipped replay')
    st = opt.scaler.stats()
    assert st['scale'] == 0.5 and st['skipped'] == 1
    assert np.isfinite(float(step(data, label)))
    after = state_tensors(model, opt)
    assert not torch.equal(after['fc.weight'], kept['fc.weight']) and not torch.equal(after['layer1.0.conv1/fwd'], kept['layer1.0.conv1/fwd'])
    assert all(float(opt.state[p]['step']) == 4 for p in model.parameters())
    print('rt16 replay %s: 3 replays bit-equal to 3 eager steps; skipped replay left %d tensors alone' % (elem, len(kept)))


def test_dataset_form_replays_a_batch_equal_to_the_staged_form(inputs, tmp_path):
    from tests.test_regressor_graph_gpu import _png_set
    images, tsv, splits = _png_set(str(tmp_path))
    dd = RT.DeviceDataset(RT.CustomDataset(images, RT.load_labelfile(tsv), splits + 'training.txt', image_size=S))
    sel = [12, 0, 5, 3]
    data, label = dd.batch(sel)
    staged, sopt = make(inputs, 'f16')
    gathered, gopt = make(inputs, 'f16')
    s_step = capture.CapturedRegressorStep(staged, sopt, B, S)
    g_step = capture.CapturedRegressorStep(gathered, gopt, B, S, dataset=dd)
    a, b = s_step(data.cpu(), label.cpu()), g_step(idx=dd.indices(sel))
    assert torch.equal(bits(a), bits(b)) and np.isfinite(float(a))
    assert_same(state_tensors(staged, sopt, counters=True), state_tensors(gathered, gopt, counters=True), 'dataset= against the staged form')
