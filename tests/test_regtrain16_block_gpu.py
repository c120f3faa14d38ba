"""The 16-bit regressor trainer block by block: TrainableResNet50H8 runs TrainableResNet50's one schedule, so ``model.block_backward`` can be held
to float64 autograd of the same block on h8 maps the way test_networks_gpu.test_regressor_training_step_vs_oracle holds the fp32 flavour.

For both element types, at 4 x 3 x 64 x 64 (the shape of test_regtrain16_gpu's skip-update test) and loss_scale_log2 = 0: blocks 0 (downsample,
stride 1), 3 (downsample, stride 2) and 4 (no downsample) are back-propagated on the GPU from their saved h8 input and a random incoming gradient.
  reference   float64 autograd of the block on cast_from_h8 of the saved input with the 16-bit-rounded conv weights, nothing else rounded;
  bar         16-bit storage alone moves these gradients, so the bar is not invented: tests/golden/make_regtrain16.py's emulation (block16: a
              rounding at every stored map, forward and backward) is evaluated on the same block, input and gradient, here, on the CPU, and per
              tensor (the input gradient and the block's 9 or 12 parameter gradients) the GPU's relative L2 deviation from float64 may be
              1.5 x the emulation's (test_regtrain16_gpu's per-parameter factor; its docstring has the reason) + 2^-23.  The additive term is
              for bn3.bias and downsample.1.bias, whose gradient is a plain sum of the incoming 16-bit gradient: the emulation is exact there
              and the GPU rounds its float64 sum once to fp32 (2^-24; the sum itself: 2^-52 per addition).
  ReLU flips  as in the fp32 test the incoming gradient is zeroed where the block output's ReLU pattern differs from float64's (here: the GPU's
              or the emulation's), and every such entry must be within 1 ulp of the element type (2^-10 / 2^-7) of zero relative to the map's
              largest pre-activation — checked for the emulation alone, on the CPU, and for the GPU.  The fp32 test's COUNT cap (at most 4 per
              block) cannot be kept for either element type, whatever the seed: a stored map is off by up to half an ulp relative to its
              own size, the pre-activations are dense around zero, and the emulation alone flips 12 - 47 (fp16) and 87 - 332 (bf16) entries of
              the 131072 - 262144 per block (data seeds 2, 3, 4; every one below 0.28 / 0.46 ulp).  The count is a matter of density, not of
              seed, so the cap used is the emulation's own count n for that block: the GPU may flip n + 3 sqrt(2 n) + 4 — two counts of
              independent rare events with one mean differ by sqrt(2 n) (Poisson; in fact the two round nearly the same values and mostly
              flip the same entries), and 4 is the fp32 test's allowance, which is what remains where n = 0.
Every figure is printed before it is asserted."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from latent2im_amd import conv, synth
from latent2im_amd import kernels16 as K16
from latent2im_amd import regressor_train as RT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = {'f16': 2.0 ** -10, 'bf16': 2.0 ** -7}
BLOCKS = (0, 3, 4)          # downsample stride 1, downsample stride 2, no downsample (block 15 adds nothing beyond 4 and its map is 2 x 2)


@pytest.fixture(scope='module')
def mk():
    spec = importlib.util.spec_from_file_location('make_regtrain16', os.path.join(ROOT, 'tests', 'golden', 'make_regtrain16.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope='module')
def inputs():
    rs = np.random.RandomState(2)
    return synth.resnet50_state(seed=300), torch.from_numpy(rs.randn(4, 3, 64, 64).astype(np.float32) * 0.5)


def _block64(P, x, p, s, down):
    """(pre-activation of the block output, block output) in plain float64."""
    bn = lambda t, b: F.batch_norm(t, None, None, P[p + b + '.weight'], P[p + b + '.bias'], training=True, eps=1e-5)
    o = F.relu(bn(F.conv2d(x, P[p + '.conv1.weight']), '.bn1'))
    o = F.relu(bn(F.conv2d(o, P[p + '.conv2.weight'], stride=s, padding=1), '.bn2'))
    pre = bn(F.conv2d(o, P[p + '.conv3.weight']), '.bn3')
    pre = pre + (bn(F.conv2d(x, P[p + '.downsample.0.weight'], stride=s), '.downsample.1') if down else x)
    return pre, F.relu(pre)


@pytest.mark.parametrize('elem', ('f16', 'bf16'))
def test_block_backward_vs_float64_autograd(inputs, mk, elem):
    st, data = inputs
    dt = RT.H8_DTYPES[elem]
    model = RT.TrainableResNet50H8(st, device=DEV, precision=elem, loss_scale_log2=0)
    model(data.to(DEV))
    sv = model._saved
    D = lambda t: t.detach().double().cpu()
    rounders = mk._rounders(dt)
    fails = []
    for bi in BLOCKS:
        blk, saved = model.blocks[bi], sv['blocks'][bi]
        cur, out = saved[0], saved[7]
        p, s, down = blk['c1'].name[:-len('.conv1')], blk['c2'].stride, blk['cd'] is not None

        def leaves():
            prm = {}
            for c_, b_ in (('c1', 'b1'), ('c2', 'b2'), ('c3', 'b3'), ('cd', 'bd')):
                if blk[c_] is not None:
                    prm[blk[c_].name + '.weight'] = blk[c_].weight.detach().to(dt).double().cpu().requires_grad_(True)      # what the planes hold
                    prm[blk[b_].name + '.weight'], prm[blk[b_].name + '.bias'] = D(blk[b_].weight).requires_grad_(True), D(blk[b_].bias).requires_grad_(True)
            return D(K16.cast_from_h8(cur)).requires_grad_(True), prm
        x64, p64 = leaves()
        pre, o64 = _block64(p64, x64, p, s, down)
        xe, pe = leaves()
        oe = mk.block16(pe, rounders[0](xe), p, s, down, rounders, running=False)          # (the store on the input rounds the summed input gradient, as the block before does)
        top = float(pre.detach().abs().max())
        flips = {}
        for who, o in (('emulation', oe.detach()), ('gpu', D(K16.cast_from_h8(out)))):
            f = (o > 0).ne(pre.detach() > 0)
            flips[who] = (f, int(f.sum()), float(pre.detach()[f].abs().max()) / top if int(f.sum()) else 0.0)
        n_emu, n_gpu = flips['emulation'][1], flips['gpu'][1]
        cap = n_emu + 3.0 * math.sqrt(2.0 * n_emu) + 4
        print('rt16 block %s %d (%s): flipped ReLUs of %d: emulation %d (worst %.3f ulp), gpu %d (worst %.3f ulp), cap %.1f'
              % (elem, bi, p, out.numel(), n_emu, flips['emulation'][2] / ULP[elem], n_gpu, flips['gpu'][2] / ULP[elem], cap))
        if not (flips['emulation'][2] < ULP[elem] and flips['gpu'][2] < ULP[elem] and n_gpu <= cap):
            fails.append((bi, 'flips', n_emu, flips['emulation'][2], n_gpu, flips['gpu'][2], cap))
        keep = ~(flips['emulation'][0] | flips['gpu'][0])
        gin = torch.randn(out.shape[0], out.shape[1] * 8, out.shape[2], out.shape[3], generator=torch.Generator().manual_seed(bi)).to(dt).float() * keep
        names = ['input'] + list(p64)
        ref = dict(zip(names, torch.autograd.grad(o64, [x64] + list(p64.values()), gin.double())))
        emu = dict(zip(names, torch.autograd.grad(oe, [xe] + list(pe.values()), gin.double())))
        grads = {}
        gx = model.block_backward(blk, saved, conv.to_h8(gin.to(DEV), dtype=dt), grads)
        assert set(grads) == set(p64) and gx.dtype == dt and gx.shape == cur.shape
        got = dict(grads, input=K16.cast_from_h8(gx))
        rel = lambda a, k: float((D(a) - ref[k]).norm() / ref[k].norm())
        for k in names:
            r_gpu, r_emu = rel(got[k], k), rel(emu[k], k)
            print('rt16 block %s %d: %-32s relative L2 from float64: gpu %.3e, emulation %.3e, ratio %.3f' % (elem, bi, k, r_gpu, r_emu, r_gpu / r_emu if r_emu > 0 else float('inf')))
            if not r_gpu <= 1.5 * r_emu + 2.0 ** -23:
                fails.append((bi, k, r_gpu, r_emu))
    assert not fails, fails
