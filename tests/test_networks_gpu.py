"""GPU parity of the frozen networks and of the whole training step (through the C ABI) against the CPU oracle and
the fixtures captured from the reference.  Tolerances: fp32 rtol 1e-3 / atol 1e-4 on images, predictions and losses
(BASELINE.json north_star); walk/latent gradients relative to their largest entry (see tests/test_oracle_golden.py)."""
import numpy as np
import pytest
import torch

from latent2im_amd import selfcheck, synth
from latent2im_amd.discriminator import Discriminator
from latent2im_amd.generator import Generator
from latent2im_amd.perceptual import VGG19Prefix
from latent2im_amd.regressor import ResNet50
from oracle import nets as onets
from oracle import sg2
from oracle import step as ostep

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def close(a, b, rtol=1e-3, atol=1e-4):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def relmax(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


def grad_ok(a, b, frac_tol=5e-3, elem=2e-3, worst=0.1):
    """Gradients of a piecewise-linear network: float32 rounding flips a few (leaky-)ReLU / max-pool masks, which moves
    a small set of gradient entries by O(1e-2 * max) — the CPU oracle itself differs by 4e-3*max between float32 and
    float64 on the 64^2 discriminator.  A wrong kernel is wrong everywhere, so: at most 0.5 % of the entries may deviate
    by more than 2e-3 * max|g|, and none by more than 10 %."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    m = float(b.abs().max())
    e = (a - b).abs()
    frac = float((e > elem * m).double().mean())
    assert frac <= frac_tol and float(e.max()) <= worst * m, (frac, float(e.max()) / m)


@pytest.mark.parametrize('size,batch', [(32, 4), (64, 4), (256, 2)])
def test_generator_forward_golden(golden, size, batch):
    g = golden('generator')
    G = Generator(synth.generator_state(size, seed=100, noise_strength=0.5), size, device=DEV)
    z = T(synth.z_sample(batch, seed=0)).float().to(DEV)
    w = G.style(z)
    close(w, g['w_%d' % size], 1e-4, 1e-5)
    lat = torch.stack([w * (1.0 + 0.05 * i) for i in range(G.n_latent)], 1).contiguous()
    noise = [T(n).to(DEV) for n in synth.noise_maps(size, batch)]
    img = G.synthesis(lat, noise)
    torch.cuda.synchronize()
    if size <= 64:
        close(img, g['img_%d' % size])
        G0 = Generator(synth.generator_state(size, seed=100, noise_strength=0.5), size, device=DEV)
        img0 = G0.synthesis(torch.stack([w] * G.n_latent, 1).contiguous(), [0 * n for n in noise])
        close(img0, g['img0_%d' % size])
    else:
        a = img.cpu().numpy()
        close(a[:, :, 96:128, 112:144], g['img_256_crop'])
        idx = g['img_256_probe_idx']
        close(a[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], g['img_256_probe'])
        close(a.sum(3), g['img_256_rowsum'], 1e-3, 2e-3)


@pytest.mark.parametrize('size,noise_strength', [(32, 0.5), (64, 0.0)])
def test_generator_latent_gradient_vs_oracle(size, noise_strength):
    st = synth.generator_state(size, seed=100, noise_strength=noise_strength)
    G = Generator(st, size, device=DEV)
    P = ostep.to_torch(st, torch.float64)
    rs = np.random.RandomState(size)
    lat = rs.randn(2, G.n_latent, 512)
    gy = rs.randn(2, 3, size, size)
    noise = synth.noise_maps(size, 2) if noise_strength else None
    lg = T(lat).float().to(DEV).requires_grad_(True)
    img = G.synthesis(lg, [T(n).to(DEV) for n in noise] if noise else None)
    img.backward(T(gy).float().to(DEV))
    lo = T(lat).requires_grad_(True)
    img_o = sg2.generator_synthesis(P, lo, [T(n).double() for n in noise] if noise else None)
    go, = torch.autograd.grad(img_o, lo, T(gy))
    close(img, img_o)
    grad_ok(lg.grad, go)
    assert relmax(lg.grad, go) < 5e-3


@pytest.mark.parametrize('res,batch', [(64, 2), (96, 1)])
def test_resnet50_forward_and_image_gradient(res, batch):
    st = synth.resnet50_state(seed=300)
    net = ResNet50(st, device=DEV)
    P = ostep.to_torch(st, torch.float64)
    rs = np.random.RandomState(res)
    x = rs.randn(batch, 3, res, res)
    gy = rs.randn(batch, 40)
    xg = T(x).float().to(DEV).requires_grad_(True)
    y = net(xg)
    y.backward(T(gy).float().to(DEV))
    xo = T(x).requires_grad_(True)
    yo = onets.resnet50_forward(P, xo)
    go, = torch.autograd.grad(yo, xo, T(gy))
    close(y, yo)
    grad_ok(xg.grad, go)
    # attribute column selection is integer work: bit-exact against indexing the same output on the host
    idx = [31, 39, 20, 15, 5]
    assert torch.equal(y[:, idx].cpu(), y.cpu()[:, idx])


def test_vgg_content_loss_and_gradient():
    st = synth.vgg19_prefix_state(seed=400)
    net = VGG19Prefix(st, device=DEV)
    P = ostep.to_torch(st, torch.float64)
    rs = np.random.RandomState(9)
    x0, x1 = rs.randn(2, 3, 48, 48), rs.randn(2, 3, 48, 48)
    xg = T(x1).float().to(DEV).requires_grad_(True)
    losses = net.content_losses(T(x0).float().to(DEV), xg)
    wts = T(np.asarray([0.3, 0.2, 0.4, 0.1])).float().to(DEV)
    (losses * wts).sum().backward()
    xo = T(x1).requires_grad_(True)
    _, lo = ostep.content_loss(P, T(x0), xo)
    go, = torch.autograd.grad(sum(l * float(w) for l, w in zip(lo, wts.cpu())), xo)
    close(losses, torch.stack(lo))
    assert relmax(xg.grad, go) < 2e-3


@pytest.mark.parametrize('size', [32, 64])
def test_discriminator_forward_golden_and_gradient(golden, size):
    st = synth.discriminator_state(size, seed=200)
    D = Discriminator(st, size, device=DEV)
    g = golden('generator')
    close(D(T(g['img_%d' % size]).to(DEV)), g['d_%d' % size])
    P = ostep.to_torch(st, torch.float64)
    x = np.random.RandomState(size).randn(4, 3, size, size)
    xg = T(x).float().to(DEV).requires_grad_(True)
    d = D(xg)
    d.sum().backward()
    xo = T(x).requires_grad_(True)
    do = sg2.discriminator_forward(P, xo)
    go, = torch.autograd.grad(do.sum(), xo)
    close(d, do)
    grad_ok(xg.grad, go)


@pytest.fixture(params=['f32', 'bf16x3'])
def precision(request):
    """Every step-level parity test runs on the default exact-fp32 matrix path and on the opt-in 3-term bf16 split."""
    from latent2im_amd import conv
    old, conv.PRECISION = conv.PRECISION, request.param
    yield request.param
    conv.PRECISION = old


def test_training_step_golden_and_float64_oracle(golden, precision):
    """The reference's own optimizeParametersAll step (fixture 'single'): every loss term, alpha_org, the walk gradient
    (against the reference's float64 evaluation) and the walk after Adam."""
    g = golden('step')
    gr = selfcheck.build_graph(64, ['Smiling'], 4, lr=1e-3)
    zs = synth.z_sample(12, seed=0)
    r = selfcheck.run_step(gr, zs[0:4], g['single.alphas'][0])
    torch.cuda.synchronize()
    assert r['loss'].dtype == torch.float64                         # get_reg_loss promotes (transform_base.py:418)
    close(r['a0'], g['single64.a0'])
    close(r['loss'], g['single64.loss'], 1e-3, 1e-4)
    close(r['terms']['reg'], g['single64.reg'], 1e-3, 1e-5)          # <= 1e-3 per-attr regressor-loss delta
    close(r['terms']['cont'], g['single64.cont'].mean(), 1e-3, 1e-6)
    close(r['terms']['gan'], g['single64.gan'], 1e-3, 1e-5)
    err = relmax(r['grad'], T(g['single64.grad']))
    ref32 = float(np.abs(g['single.0.grad'] - g['single64.grad']).max() / np.abs(g['single64.grad']).max())
    assert err < max(2 * ref32, 5e-3), (err, ref32)                  # no worse than the reference's own fp32 rounding
    close(r['x1'].sum(3), g['single.0.x1_rowsum'], 1e-3, 2e-3)
    # Adam(lr, betas=(0.5,0.99)) moved the walk exactly like the reference for every entry with a settled sign
    moved = gr.walk.w.detach().cpu().numpy()
    assert np.mean(np.abs(moved - g['single64.walk']) > 2e-4) < 0.02


def test_three_consecutive_training_steps_vs_reference_sequence(golden):
    """[r5] The reference's own three-step optimizeParametersAll sequence (transform_base.py:456-490 + Adam, fixture 'single.{0,1,2}': its walk carried
    from step to step, its z batches 0-3 / 4-7 / 8-11, its alpha draws) replayed on the HIP path from the product's OWN state: Adam's moments and
    bias correction are carried by the product's optimizer, nothing is reset between steps.  Per step: alpha_org, every loss term and the walk
    gradient against the reference's numbers (bounds of tests/test_oracle_golden.py::test_training_steps_single_attr); the walk after each step
    (a) against the Adam restatement fed with the product's own gradient sequence (exact: pins m, v, bias correction, lr, betas), (b) against the
    reference's walk (entries whose gradient sign is settled move identically; Adam's first steps are lr * sign(g), so an entry whose float32
    gradient is rounding noise may step the other way: at most 2 % more of the entries per step may be further than 0.2 lr per step from it)."""
    g = golden('step')
    gr = selfcheck.build_graph(64, ['Smiling'], 4, lr=1e-3)
    zs = synth.z_sample(12, seed=0)
    own = ostep.Adam(T(synth.walk_init(1, 10, seed=7)).float(), lr=1e-3)
    for i in range(3):
        r = selfcheck.run_step(gr, zs[4 * i:4 * i + 4], g['single.alphas'][i])
        torch.cuda.synchronize()
        assert r['loss'].dtype == torch.float64
        close(r['a0'], g['single.%d.a0' % i], 1e-3, 1e-4)
        close(r['terms']['reg'], g['single.%d.reg' % i], 1e-3, 1e-5)
        close(r['terms']['cont'], g['single.%d.cont' % i].mean(), 2e-3, 1e-6)
        close(r['terms']['gan'], g['single.%d.gan' % i], 1e-3, 1e-5)
        close(r['loss'], g['single.%d.loss' % i], 1e-3, 1e-4)
        close(r['x1'].sum(3), g['single.%d.x1_rowsum' % i], 1e-3, 3e-3)
        gerr = relmax(r['grad'], T(g['single.%d.grad' % i]))
        assert gerr < 1e-2 * (i + 1), (i, gerr)                       # (steps 1, 2 start from walks that already differ in their noise entries)
        own.step(r['grad'].detach().cpu().float())
        moved = gr.walk.w.detach().cpu()
        assert float((moved - own.p).abs().max()) < 2e-6, (i, float((moved - own.p).abs().max()))      # Adam state carried exactly
        frac = float(np.mean(np.abs(moved.numpy() - g['single.%d.walk' % i]) > 2e-4 * (i + 1)))
        assert frac < 0.02 * (i + 1), (i, frac)


def test_training_step_multi_attr_clamp_and_regonly(golden, precision):
    g = golden('step')
    zs = synth.z_sample(12, seed=0)
    gr = selfcheck.build_graph(64, ['Smiling', 'Young', 'Male', 'Eyeglasses', 'Bangs'], 4, lr=1e-3)
    assert gr.attrIdx == [31, 39, 20, 15, 5]
    r = selfcheck.run_step(gr, zs[0:4], g['multi.delta'], clamp=True)
    close(r['a0'], g['multi64.a0'])
    close(r['eps'], g['multi64.eps'])
    close(r['loss'], g['multi64.loss'], 1e-3, 1e-4)
    assert relmax(r['grad'], T(g['multi64.grad'])) < 1e-2
    gr = selfcheck.build_graph(64, ['Smiling'], 4, lr=1e-3)
    r = selfcheck.run_step(gr, zs[0:4], g['single.alphas'][0], no_content_loss=True, no_gan_loss=True, layers=[0, 1, 2, 3, 4, 5])
    close(r['loss'], g['regonly.loss'], 1e-3, 1e-4)
    assert relmax(r['grad'], T(g['regonly.grad'])) < 1e-2
    assert float(r['grad'][:, 6:].abs().max()) == 0.0


def test_full_size_1024_forward_parity_and_consistency(precision):
    """BASELINE configs 2-4 run at 1024^2: one sample through every network at full resolution against the CPU oracle
    (seconds of CPU work), plus size-independent consistency properties of the kernels at the full bench shape."""
    from latent2im_amd import conv
    size = 1024
    stG = synth.generator_state(size, seed=100)
    G = Generator(stG, size, device=DEV)
    PG = ostep.to_torch(stG)
    z = T(synth.z_sample(1, seed=3)).float()
    w = G.style(z.to(DEV))
    lat = torch.stack([w * (1.0 + 0.02 * i) for i in range(G.n_latent)], 1).contiguous()
    img = G.synthesis(lat)
    wo = sg2.style_mlp(PG, z)
    img_o = sg2.generator_synthesis(PG, torch.stack([wo * (1.0 + 0.02 * i) for i in range(G.n_latent)], 1), None)
    close(img, img_o)
    stR = synth.resnet50_state(seed=300)
    close(ResNet50(stR, device=DEV)(img), onets.resnet50_forward(ostep.to_torch(stR), img_o))
    stD = synth.discriminator_state(size, seed=200)
    close(Discriminator(stD, size, device=DEV)(img), sg2.discriminator_forward(ostep.to_torch(stD), img_o))
    stV = synth.vgg19_prefix_state(seed=400)
    other = torch.roll(img_o, 7, 3)
    V = VGG19Prefix(stV, device=DEV)
    _, lo = ostep.content_loss(ostep.to_torch(stV), other, img_o)
    close(V.content_losses(other.to(DEV), img), torch.stack(lo))
    if precision != 'f32':
        return
    # consistency at the bench batch: fused transposed conv == per-parity launches; linearity of the conv in its input
    x = torch.randn(8, 64, 512, 512, device=DEV)
    up = G.layers[-2].conv                                             # 64 -> 32 up layer at 512 -> 1025
    y1 = up.forward(x)
    conv.USE_FUSED_TRANSPOSED = False
    try:
        y0 = up.forward(x)
    finally:
        conv.USE_FUSED_TRANSPOSED = True
    assert float((y1 - y0).abs().max()) <= 1e-4 * float(y0.abs().max())
    c = G.layers[-3].conv                                              # 64 -> 64 3x3 at 512
    a, b = torch.randn_like(x), torch.randn_like(x)
    lhs = c.forward(2.0 * a - 3.0 * b)
    rhs = 2.0 * c.forward(a) - 3.0 * c.forward(b)
    assert float((lhs - rhs).abs().max()) <= 1e-4 * float(rhs.abs().max())
    # every tile configuration computes the same convolution
    ref = c.forward(a)
    for hint in (1, 2, 3, 4, 8):
        # (ref runs on the Winograd kernel the dispatch picks, the forced tiles on the direct kernel: 1e-5 for F(2x2,3x3), 3e-5 for F(4x4,3x3))
        assert float((c.forward(a, tile_hint=hint) - ref).abs().max()) <= (1e-5 if conv.WINO4 == 'off' else 3e-5) * float(ref.abs().max())


@pytest.mark.parametrize('size,batch,attrs,clamp', [(256, 16, ['Smiling'], False),
                                                    (1024, 1, ['Smiling', 'Young', 'Male', 'Eyeglasses', 'Bangs'], True)])
def test_full_size_training_step_vs_oracle(size, batch, attrs, clamp):
    """BASELINE configs 2 (256^2, batch 16, one attribute, train.py flow) and 3/4 (1024^2, five attributes, train_multi_attr.py
    clamp flow; one sample, which is what the CPU oracle finishes in under a minute): a whole training step — both generator
    passes, regressor, VGG content, discriminator, backward into the walk — against the float32 CPU oracle on the same z/seed.
    Images, alpha_org and every loss term within rtol 1e-3 / atol 1e-4 (the per-attribute regressor loss included); the walk
    gradient like tests/test_oracle_golden.py: relative to its largest entry.  [r5] The batch-16 oracle evaluation (56 s on the GPU box) is read
    from tests/golden/oracle_1024.npz (case 'c2'; tests/oracle_cache.py); the one-sample 1024^2 case stays a live evaluation."""
    from latent2im_amd import constants
    from tests import oracle_cache
    from tests.conftest import GOLDEN
    try:
        gr = selfcheck.build_graph(size, attrs, batch, lr=1e-3)
        zs = synth.z_sample(batch, seed=5)
        rs = np.random.RandomState(8)
        alpha = np.ones((batch, len(attrs))) * (rs.uniform(-1, 1, len(attrs)) if clamp else rs.uniform(0, 1, len(attrs)))
        r = selfcheck.run_step(gr, zs, alpha, clamp=clamp, optimize=False)
        torch.cuda.synchronize()
        idx = gr.attrIdx
        if size == 256:
            case = oracle_cache.CASES['c2']
            assert (case['batch'], case['attrs'], case['z_seed'], case['clamp']) == (batch, attrs, 5, clamp) and np.array_equal(case['alpha'](), alpha)
            o = oracle_cache.load(GOLDEN, 'c2')
            o.check_image(r['x0'], 'x0')
            o.check_image(r['x1'], 'x1')
            po = o['po'].double()
        else:
            nets = dict(G=ostep.to_torch(synth.generator_state(size, seed=100)), D=ostep.to_torch(synth.discriminator_state(size, seed=200)),
                        R=ostep.to_torch(synth.resnet50_state(seed=300)), V=ostep.to_torch(synth.vgg19_prefix_state(seed=400)))
            o = ostep.train_step(nets, T(synth.walk_init(len(attrs), gr.module.netG.n_latent, seed=7)), T(zs).float(), T(alpha).float(), idx,
                                 clamp_variant=clamp)
            close(r['x0'], o['x0'])
            close(r['x1'], o['x1'])
            po = onets.resnet50_forward(nets['R'], o['x1'])[:, idx].double()
        close(r['a0'], o['alpha_org'])
        close(r['eps'], o['eps'])
        close(r['terms']['reg'], o['reg'], 1e-3, 1e-5)
        close(r['terms']['cont'], o['cont'], 1e-3, 1e-6)
        close(r['terms']['gan'], o['gan'], 1e-3, 1e-5)
        close(r['loss'], o['loss'], 1e-3, 1e-4)
        # per-attribute regressor loss (the "<= 1e-3 per-attr regressor-loss delta" of the north star)
        pg = gr.regressor(r['x1'])[:, idx].double().cpu()
        tgt = o['target'].double()
        per_attr = lambda p: -(tgt * p.clamp(min=1e-12).log() + (1 - tgt) * (1 - p).clamp(min=1e-12).log()).mean(0)
        close(per_attr(pg), per_attr(po), 1e-3, 1e-5)
        # both sides are float32 here (the float32 oracle itself sits ~1e-2 * max from its float64 evaluation: a few flipped
        # (leaky-)ReLU / max-pool masks move individual entries), so: few entries off by more than 1 % of the largest, none by 10 %
        # both sides are float32 here and the float32 oracle itself sits ~1e-2 * max from its float64 evaluation at this depth
        # (see test_walk_gradient_256_vs_float64_oracle for the gradient against float64): only a coarse bound here
        assert relmax(r['grad'], o['grad']) < 5e-2
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def _oracle_nets(size, dt=torch.float32):
    return dict(G=ostep.to_torch(synth.generator_state(size, seed=100), dt), D=ostep.to_torch(synth.discriminator_state(size, seed=200), dt),
                R=ostep.to_torch(synth.resnet50_state(seed=300), dt), V=ostep.to_torch(synth.vgg19_prefix_state(seed=400), dt))


def test_config3_whole_step_1024_batch8_vs_oracle():
    """BASELINE config 3 at its own batch: one whole training step at 1024^2, batch 8, one attribute, full loss (both generator
    passes, regressor, VGG content, discriminator WITH its group-of-4 minibatch stddev over {0,2,4,6} / {1,3,5,7}, backward into the
    walk) against the float32 CPU oracle on the same z / seed.  [r5] The oracle's answer for these fixed seeds is a constant: it is read from
    tests/golden/oracle_1024.npz (written by tests/golden/make_oracle_cache.py with oracle.step.train_step_bounded — the bounded-memory evaluation
    pinned to the plain train_step in tests/test_oracle_golden.py; tests/test_oracle_cache_cpu.py re-derives the 256^2 entry live) instead of
    128 s of CPU work on the GPU box.  Images (4096 probe pixels per image and channel elementwise, row and column sums), alpha, every loss
    term: rtol 1e-3 / atol 1e-4."""
    from latent2im_amd import constants
    from tests import oracle_cache
    from tests.conftest import GOLDEN
    try:
        case = oracle_cache.CASES['c3']
        size, batch, attrs = case['size'], case['batch'], case['attrs']
        gr = selfcheck.build_graph(size, attrs, batch, lr=1e-3)
        zs = synth.z_sample(batch, seed=case['z_seed'])
        alpha = case['alpha']()
        r = selfcheck.run_step(gr, zs, alpha, optimize=False)
        torch.cuda.synchronize()
        o = oracle_cache.load(GOLDEN, 'c3')
        o.check_image(r['x0'], 'x0')
        close(r['a0'], o['alpha_org'])
        close(r['eps'], o['eps'])
        o.check_image(r['x1'], 'x1')
        close(r['terms']['reg'], o['reg'], 1e-3, 1e-5)
        close(r['terms']['cont'], o['cont'], 1e-3, 1e-6)
        close(r['terms']['gan'], o['gan'], 1e-3, 1e-5)
        close(r['loss'], o['loss'], 1e-3, 1e-4)
        assert r['loss'].dtype == torch.float64
        pg = gr.regressor(r['x1'])[:, gr.attrIdx].double().cpu()
        po = o['po'].double()
        tgt = o['target'].double()
        per_attr = lambda p: -(tgt * p.clamp(min=1e-12).log() + (1 - tgt) * (1 - p).clamp(min=1e-12).log()).mean(0)
        close(per_attr(pg), per_attr(po), 1e-3, 1e-5)
        # float32 against float32 through ~60 piecewise-linear layers: coarse here, the float64 bound is the next test
        e = relmax(r['grad'], o['grad'])
        print('1024^2 batch-8 walk gradient, HIP vs float32 oracle, relative to the largest entry: %.3e' % e)
        grad_ok(r['grad'], o['grad'])                       # <= 0.5 % of the entries off by more than 2e-3 * max|g|, none by 10 %
        assert e < 1e-2, e
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_config4_whole_step_1024_batch8_five_attrs_vs_oracle():
    """BASELINE config 4 at its per-GPU shape: train_multi_attr.py flow (train_multi_attr.py:71-154: five CelebA attributes, clamped
    targets, transform_base.py:456-490 full loss) at 1024^2, batch 8, against the float32 CPU oracle (bounded-memory evaluation).
    Images, alpha_org, the clamp pair (target, epsilon), every loss term and the per-attribute regressor loss within rtol 1e-3 / atol 1e-4;
    the walk gradient [5, 18, 512] under the distribution bound of grad_ok and 1e-2 of its largest entry.  Then the same step at batch 8 on
    the 16-bit path against the same oracle evaluation, under the bf16 contract.  [r5] The oracle evaluation is read from
    tests/golden/oracle_1024.npz (see test_config3_whole_step_1024_batch8_vs_oracle)."""
    from latent2im_amd import constants
    from tests import oracle_cache
    from tests.conftest import GOLDEN
    try:
        case = oracle_cache.CASES['c4']
        size, batch, attrs = case['size'], case['batch'], case['attrs']
        gr = selfcheck.build_graph(size, attrs, batch, lr=1e-3)
        assert gr.attrIdx == [31, 39, 20, 15, 5]
        zs = synth.z_sample(batch, seed=case['z_seed'])
        alpha = case['alpha']()
        r = selfcheck.run_step(gr, zs, alpha, clamp=True, optimize=False)
        torch.cuda.synchronize()
        o = oracle_cache.load(GOLDEN, 'c4')
        o.check_image(r['x0'], 'x0')
        close(r['a0'], o['alpha_org'])
        close(r['eps'], o['eps'])
        o.check_image(r['x1'], 'x1')
        close(r['terms']['reg'], o['reg'], 1e-3, 1e-5)
        close(r['terms']['cont'], o['cont'], 1e-3, 1e-6)
        close(r['terms']['gan'], o['gan'], 1e-3, 1e-5)
        close(r['loss'], o['loss'], 1e-3, 1e-4)
        pg = gr.regressor(r['x1'])[:, gr.attrIdx].double().cpu()
        po = o['po'].double()
        tgt = o['target'].double()
        per_attr = lambda p: -(tgt * p.clamp(min=1e-12).log() + (1 - tgt) * (1 - p).clamp(min=1e-12).log()).mean(0)
        close(per_attr(pg), per_attr(po), 1e-3, 1e-5)
        e = relmax(r['grad'], o['grad'])
        print('config 4 (1024^2, batch 8, 5 attrs, clamp) walk gradient, HIP vs float32 oracle, relative to the largest entry: %.3e' % e)
        grad_ok(r['grad'], o['grad'])
        assert e < 1e-2, e
        # [r4] The SAME batch-8 step on the 16-bit path against the SAME oracle evaluation (the multi-attribute clamp flow is config 5's; the float32
        # oracle's own distance from float64 — 3e-3 of the largest gradient entry — is far inside the bf16 contract of tests/test_h8_gpu.py): the
        # batch-8 bf16 gradient had only ever been compared with itself (replay == eager)
        import gc
        from latent2im_amd import conv
        del gr, r
        gc.collect()
        torch.cuda.empty_cache()
        old = conv.PRECISION
        try:
            conv.PRECISION = 'bf16'
            g16 = selfcheck.build_graph(size, attrs, batch, lr=1e-3)
            assert type(g16.module.netG).__module__.endswith('nets16')
            h = selfcheck.run_step(g16, zs, alpha, clamp=True, optimize=False)
            torch.cuda.synchronize()
            rel = lambda a, b: float((a.detach().double().cpu() - b.double()).abs().max() / b.double().abs().max())
            assert o.image_rel_to_max(h['x0'], 'x0') < 4e-2 and o.image_rel_to_max(h['x1'], 'x1') < 4e-2
            assert float((h['a0'].double().cpu() - o['alpha_org'].double()).abs().max()) < 2e-3
            assert float((h['eps'].double().cpu() - o['eps'].double()).abs().max()) < 2e-3
            assert abs(float(h['loss']) - float(o['loss'])) < 5e-3 * abs(float(o['loss']))
            assert abs(float(h['terms']['reg']) - float(o['reg'])) < 5e-3 * abs(float(o['reg']))
            assert abs(float(h['terms']['gan']) - float(o['gan'])) < 2e-2 * abs(float(o['gan']))
            p16 = g16.regressor(h['x1'])[:, g16.attrIdx].double().cpu()
            assert float((per_attr(p16) - per_attr(po)).abs().max()) < 1e-3
            ga, gb = h['grad'].detach().double().cpu().reshape(-1), o['grad'].double().reshape(-1)
            cos, l2 = float(torch.dot(ga, gb) / (ga.norm() * gb.norm())), float((ga - gb).norm() / gb.norm())
            print('config 4 shape on the 16-bit path, batch 8: walk-gradient cosine %.4f, relative L2 %.3f vs the float32 oracle' % (cos, l2))
            assert cos > 0.97 and l2 < 0.27, (cos, l2)
            del g16, h
        finally:
            conv.PRECISION = old
            gc.collect()
            torch.cuda.empty_cache()
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_config5_step_1024_bf16x3_hipgraph_vs_oracle():
    """BASELINE config 5 at its own shape: SceneGraph on the transient-scene table, five attributes, train_multi_attr.py clamp flow
    (train_multi_attr.py:71-154), every eligible contraction on the split-precision bf16 matrix path (conv.PRECISION = 'bf16x3'), forward +
    backward REPLAYED from one hipGraph (capture.CapturedStep) at 1024^2 — one sample against the oracle in FLOAT64 (bounded-memory
    evaluation, cached): images, epsilon and every loss term within rtol 1e-3 / atol 1e-4, the walk gradient no further from the exact value than
    twice the oracle's own float32 run (or 5e-3 of the largest entry) — the bar of test_walk_gradient_1024_vs_float64_oracle.  Then the
    per-GPU batch of the config: one replay at batch 8 equals the same step launched eagerly."""
    from latent2im_amd import capture, constants, conv
    old = conv.PRECISION
    try:
        conv.PRECISION = 'bf16x3'
        attrs = ['dirty', 'daylight', 'night', 'sunrisesunset', 'dawndusk']
        size = 1024
        gr = selfcheck.build_graph(size, attrs, 1, lr=1e-3, transform='scene')
        assert type(gr).__name__ == 'SceneGraph' and gr.attrIdx == [0, 1, 2, 3, 4]
        zs = synth.z_sample(1, seed=15)
        alpha = np.ones((1, 5)) * np.random.RandomState(16).uniform(-1, 1, 5)           # SceneTransform.get_train_alpha
        step = capture.CapturedStep(gr, 1, 5, clamp=True)
        r = step(zs, alpha, optimize=False)
        torch.cuda.synchronize()
        # [r5] the float64 oracle evaluation of this sample and the float32 run's gradient: tests/golden/oracle_1024.npz, case 'c5'
        from tests import oracle_cache
        from tests.conftest import GOLDEN
        case = oracle_cache.CASES['c5']
        assert case['z_seed'] == 15 and np.array_equal(case['alpha'](), alpha) and case['attrs'] == attrs
        o64 = oracle_cache.load(GOLDEN, 'c5')
        errs = dict(hip=relmax(r['grad'], o64['grad']), oracle32=relmax(o64['grad32'], o64['grad']))
        o64.check_image(r['x0'], 'x0')
        o64.check_image(r['x1'], 'x1')
        close(r['a0'], o64['alpha_org'])
        close(r['eps'], o64['eps'])
        close(r['loss'], o64['loss'], 1e-3, 1e-4)
        close(r['terms']['reg'], o64['reg'], 1e-3, 1e-5)
        close(r['terms']['cont'], o64['cont'], 1e-3, 1e-6)
        close(r['terms']['gan'], o64['gan'], 1e-3, 1e-5)
        print('config 5 (1024^2, bf16x3, hipGraph replay) walk gradient vs float64 oracle, relative to the largest entry:', errs)
        assert errs['hip'] < max(2 * errs['oracle32'], 5e-3), errs
        del step, gr
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        # the config's per-GPU batch: a replayed step == the same step launched eagerly
        batch = 8
        zs = synth.z_sample(batch, seed=17)
        alpha = np.ones((batch, 5)) * np.random.RandomState(18).uniform(-1, 1, 5)
        ge = selfcheck.build_graph(size, attrs, batch, lr=1e-3, transform='scene')
        e = selfcheck.run_step(ge, zs, alpha, clamp=True, optimize=False)
        e = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in e.items()}
        del ge
        gc.collect()
        torch.cuda.empty_cache()
        gc_ = selfcheck.build_graph(size, attrs, batch, lr=1e-3, transform='scene')
        step = capture.CapturedStep(gc_, batch, 5, clamp=True)
        r = step(zs, alpha, optimize=False)
        torch.cuda.synchronize()
        close(r['x1'], e['x1'], 1e-4, 1e-5)
        close(r['eps'], e['eps'], 1e-4, 1e-6)
        close(r['loss'], e['loss'], 1e-5, 1e-6)
        grad_ok(r['grad'], e['grad'])                        # same kernels, same inputs; atomics in the reductions reorder sums
        assert relmax(r['grad'], e['grad']) < 2e-3
    finally:
        conv.PRECISION = old
        constants.resolution, constants.BATCH_SIZE = 256, 4


@pytest.mark.parametrize('name', ['g1024', 'g1024b', 'g1024c'])
def test_walk_gradient_1024_vs_float64_oracle(name):
    """The walk gradient of a full-loss step at 1024^2 (one sample) against the oracle evaluated in FLOAT64 — the same bar as
    test_walk_gradient_256_vs_float64_oracle at the bench resolution: no further from the exact value than twice the oracle's own
    float32 run, or 5e-3 of the largest entry.  [r5] Oracle values from tests/golden/oracle_1024.npz; [r6] three samples (latents and walk
    amplitudes 0.41 / 0.77 / 0.15) instead of one."""
    from latent2im_amd import constants
    from tests import oracle_cache
    from tests.conftest import GOLDEN
    try:
        case = oracle_cache.CASES[name]
        size, batch = case['size'], case['batch']
        gr = selfcheck.build_graph(size, case['attrs'], batch, lr=1e-3)
        zs = synth.z_sample(batch, seed=case['z_seed'])
        r = selfcheck.run_step(gr, zs, case['alpha'](), optimize=False)
        torch.cuda.synchronize()
        o64 = oracle_cache.load(GOLDEN, name)
        errs = dict(hip=relmax(r['grad'], o64['grad']), oracle32=relmax(o64['grad32'], o64['grad']))
        o64.check_image(r['x1'], 'x1')
        close(r['loss'], o64['loss'], 1e-3, 1e-4)
        close(r['terms']['reg'], o64['reg'], 1e-3, 1e-5)
        close(r['terms']['cont'], o64['cont'], 1e-3, 1e-6)
        close(r['terms']['gan'], o64['gan'], 1e-3, 1e-5)
        print('1024^2 walk gradient vs float64 oracle (%s), relative to the largest entry:' % name, errs)
        assert errs['hip'] < max(2 * errs['oracle32'], 5e-3), errs
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_walk_gradient_256_vs_float64_oracle():
    """Walk gradient of a full-loss step at 256^2 (batch 4) against the oracle evaluated in float64 — the value the arithmetic
    has without rounding.  The HIP path must be no further from it than twice the oracle's own float32 run (or 5e-3 of the
    largest entry, whichever is larger): the same bar as the 64^2 fixture test, at a BASELINE resolution.  [r5] Both oracle evaluations are
    constants of the seeds: read from tests/golden/oracle_1024.npz (case 'g256': the float64 result and the float32 run's gradient)."""
    from latent2im_amd import constants
    from tests import oracle_cache
    from tests.conftest import GOLDEN
    try:
        case = oracle_cache.CASES['g256']
        size, batch, attrs = case['size'], case['batch'], case['attrs']
        gr = selfcheck.build_graph(size, attrs, batch, lr=1e-3)
        zs = synth.z_sample(batch, seed=case['z_seed'])
        r = selfcheck.run_step(gr, zs, case['alpha'](), optimize=False)
        torch.cuda.synchronize()
        o64 = oracle_cache.load(GOLDEN, 'g256')
        errs = dict(hip=relmax(r['grad'], o64['grad']), oracle32=relmax(o64['grad32'], o64['grad']))
        close(r['loss'], o64['loss'], 1e-3, 1e-4)
        close(r['terms']['reg'], o64['reg'], 1e-3, 1e-5)
        print('walk gradient vs float64 oracle, relative to the largest entry:', errs)
        assert errs['hip'] < max(2 * errs['oracle32'], 5e-3), errs
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_train_cli_then_vis_cli_roundtrip(tmp_path):
    """The two drop-in drivers end to end on the GPU: train.py (2 iterations at 32^2) writes opt.yml, log.txt, sample grids
    and the pickled walk; vis_w.py loads them and writes one strip per sample.  apply_alpha == the oracle's two passes."""
    import pickle
    from latent2im_amd import trainer, vis, constants
    models = str(tmp_path / 'models')
    argv = ['--model', 'stylegan_v2_real', '--transform', 'face', '--num_samples', '8', '--learning_rate', '1e-3', '--latent', 'w',
            '--walk_type', 'linear', '--loss', 'l2', '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt',
            '--models_dir', models, '--overwrite_config', '--resolution', '32', '--batch_size', '4', '--n_epoch', '1', '--seed', '3',
            '--model_save_freq', '1', '--synthetic_weights']
    import os
    os.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        trainer.main(multi_attr=False, argv=argv)
        out = os.path.join(models, 'stylegan_v2_real_face_linear_lr0.001_l2_w')
        ck = os.path.join(out, 'model_w_1_final_walk_module.ckpt')
        for f in ('opt.yml', 'opt.txt', 'log.txt', 'model_w_0_walk_module.ckpt'):
            assert os.path.isfile(os.path.join(out, f)), f
        assert len([f for f in os.listdir(os.path.join(out, 'results')) if f.endswith('.png')]) == 4
        assert 'T, epc, bst, lss, alpha:' in open(os.path.join(out, 'log.txt')).read()
        walk = torch.load(ck, map_location='cpu', weights_only=False)
        assert type(walk).__module__ == 'graphs.stylegan_v2_real.transform_base' and tuple(walk.w.shape) == (1, 8, 512)
        # opt.yml needs the additive flags for the visualiser to rebuild the same graph
        written = vis.main([os.path.join(out, 'opt.yml'), '--save_path_w', ck, '--num_samples', '4', '--num_panels', '3', '--noise_seed', '1'])
        assert len(written) == 4 and all(os.path.isfile(w) for w in written)
        # apply_alpha against the oracle
        gr = selfcheck.build_graph(32, ['Smiling'], 4)
        with torch.no_grad():
            gr.walk.w.copy_(walk.w.to(gr.device))
        zs = synth.z_sample(4, seed=1)
        alpha = np.full((4, 1), 0.8)
        img1, a0, img0 = gr.apply_alpha({'z': zs}, alpha)
        nets_ = dict(G=ostep.to_torch(synth.generator_state(32, seed=100)), R=ostep.to_torch(synth.resnet50_state(seed=300)))
        ws = ostep.get_w(nets_['G'], T(zs).float(), 8)
        x0 = ostep.get_logits(nets_['G'], ws)
        p0 = ostep.get_reg_preds(nets_['R'], x0, [31])
        x1 = ostep.get_logits(nets_['G'], ostep.walk_linear_multi_w(ws, T(alpha).float() - p0, walk.w.detach()))
        close(img0, x0)
        close(a0, p0)
        close(img1, x1)
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_smoke_entry():
    selfcheck.smoke()


# ---- the rows next to the training step -------------------------------------------------------------------
def _inference_graph(size, attrs, walk_seed, fc_scale=1.0, walk_scale=1.0):
    import types
    from latent2im_amd import constants, graph
    constants.resolution, constants.BATCH_SIZE = size, 4
    r_state = synth.resnet50_state(seed=300)
    r_state['fc.weight'] = r_state['fc.weight'] * fc_scale
    nets = (Generator(synth.generator_state(size, seed=100), size, device=DEV), None, ResNet50(r_state, device=DEV), None, {})
    with open('dataset/attributes_celeba.txt') as f:
        names = [l.strip() for l in f if l.strip()]
    g = graph.faceGraph(lr=1e-3, walk_type='linear', loss='l2', trainEmbed=False, attrList=list(attrs),
                        attrTable={n: i for i, n in enumerate(names)}, layers=None, stylegan_opts=types.SimpleNamespace(latent='w'), nets=nets)
    with torch.no_grad():
        g.walk.w.copy_(T(synth.walk_init(len(attrs), g.module.netG.n_latent, seed=walk_seed)) * walk_scale)
    return g


def test_eval_attribute_buckets_match_reference(golden):
    """eval.py's attribute-preservation pass (vis_multi_image_batch_alphas_compute_multi_attr) on the GPU against the buckets
    the reference's own method produced on the same seeds: identical membership (integer selection), regressor outputs within
    the fp32 tolerance, and the same metric."""
    import os
    from latent2im_amd import constants, evaluate
    os.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    g = golden('next')
    try:
        gr = _inference_graph(64, ['Smiling', 'Young'], 9, float(g['fc_scale']), float(g['walk_scale']))
        zs = synth.z_sample(4, seed=11)
        idx = int(g['index_'])
        x1, a0, x0 = gr.apply_alpha({'z': zs}, g['alphas'][3], index_=idx)
        close(a0, g['apply.a0'])
        close(x0.sum(3), g['apply.x0_rowsum'], 1e-3, 2e-3)
        close(x1.sum(3), g['apply.x1_rowsum'], 1e-3, 2e-3)
        ma, ao, im, og = gr.vis_multi_image_batch_alphas_compute_multi_attr({'z': zs}, '/tmp/unused', list(g['alphas']),
                                                                           list(np.linspace(-0.5, 1.5, 5)), 0, index_=idx)
        assert [len(m) for m in ma] == [6, 5, 6]
        for k in range(3):
            close(np.asarray(ma[k]), g['bucket%d.multi_attr' % k], 1e-3, 2e-3)
            close(np.asarray(ao[k]), g['bucket%d.attri_org' % k], 1e-3, 2e-3)
            assert all(i.dtype == np.uint8 and i.shape == (3, 64, 64) for i in im[k] + og[k])
            s = np.asarray([int(i.astype(np.int64).sum()) for i in im[k]])
            assert np.all(np.abs(s - g['bucket%d.img_sum' % k]) <= 64)
        _, got = evaluate.attribute_preservation(ma, ao, idx)
        _, want = evaluate.attribute_preservation([list(g['bucket%d.multi_attr' % k]) for k in range(3)],
                                                  [list(g['bucket%d.attri_org' % k]) for k in range(3)], idx)
        close(got, want, 1e-3, 1e-4)
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_checkpoint_formats_round_trip(tmp_path):
    """networks load from files in the reference's formats — StyleGAN2 ``{'g_ema': state_dict}``
    (transform_base.py:544-547), regressor ``{'model': state_dict, 'optm': ...}`` (scene_regressor_256.py:167-170), torchvision
    VGG ``features.N.*`` — and give the same outputs as the same weights handed over directly."""
    from latent2im_amd import constants, graph
    saved = (constants.g_path, constants.reg_path, constants.vgg_path, constants.resolution, constants.BATCH_SIZE)
    try:
        gs, rs_, vs = synth.generator_state(32, seed=5), synth.resnet50_state(seed=6), synth.vgg19_prefix_state(seed=7)
        torch.save({'g_ema': {k: T(np.asarray(v)) for k, v in gs.items()}, 'g': {}, 'd': {}}, tmp_path / 'g.pt')
        torch.save({'model': {k: T(np.asarray(v)) for k, v in rs_.items()}, 'optm': {}}, tmp_path / 'r.model')
        torch.save({'features.' + k: T(np.asarray(v)) for k, v in vs.items()}, tmp_path / 'vgg.pth')
        constants.g_path, constants.reg_path, constants.vgg_path = str(tmp_path / 'g.pt'), str(tmp_path / 'r.model'), str(tmp_path / 'vgg.pth')
        constants.resolution, constants.BATCH_SIZE = 32, 4
        netG, netD, reg, vgg, src = graph.load_networks(32, torch.device(DEV))
        assert src['G'].endswith('g.pt') and src['R'].endswith('r.model') and src['V'].endswith('vgg.pth')
        z = T(synth.z_sample(4, seed=2)).float().to(DEV)
        w = netG.style(z).unsqueeze(1).repeat(1, netG.n_latent, 1)
        x, _ = netG(w, input_is_latent=True)
        G2 = Generator(gs, 32, device=DEV)
        x2, _ = G2(G2.style(z).unsqueeze(1).repeat(1, G2.n_latent, 1), input_is_latent=True)
        assert torch.equal(x, x2)
        assert torch.equal(reg(x), ResNet50(rs_, device=DEV)(x))
        l1 = vgg.content_losses(x, x * 0.9)
        l2 = VGG19Prefix(vs, device=DEV).content_losses(x, x * 0.9)
        close(l1, l2, 1e-5, 0)                                          # atomics in the squared-difference reduction
        # a configured checkpoint that is missing is an error (the reference crashes in torch.load) ...
        constants.g_path = str(tmp_path / 'absent.pt')
        constants.ALLOW_SYNTHETIC_WEIGHTS = False
        with pytest.raises(FileNotFoundError, match='absent.pt'):
            graph.load_networks(32, torch.device(DEV), need_vgg=False, need_d=False)
        # ... unless seeded synthetic weights were asked for, and then the choice is reported
        constants.ALLOW_SYNTHETIC_WEIGHTS = True
        assert graph.load_networks(32, torch.device(DEV), need_vgg=False, need_d=False)[4]['G'].startswith('synthetic')
    finally:
        constants.g_path, constants.reg_path, constants.vgg_path, constants.resolution, constants.BATCH_SIZE = saved
        constants.ALLOW_SYNTHETIC_WEIGHTS = True


def test_eval_cli_after_training(tmp_path):
    """train.py (2 iterations at 32^2) then eval.py on its output: the metric dict comes back, bucket sizes add up to at most
    samples x panels, and the printed line has the reference's wording."""
    import os
    from latent2im_amd import constants, evaluate, trainer
    os.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    models = str(tmp_path / 'models')
    argv = ['--model', 'stylegan_v2_real', '--transform', 'face', '--num_samples', '8', '--learning_rate', '1e-3', '--latent', 'w',
            '--walk_type', 'linear', '--loss', 'l2', '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt',
            '--models_dir', models, '--overwrite_config', '--resolution', '32', '--batch_size', '4', '--n_epoch', '1', '--seed', '3',
            '--model_save_freq', '1', '--synthetic_weights']
    try:
        trainer.main(multi_attr=False, argv=argv)
        out = os.path.join(models, 'stylegan_v2_real_face_linear_lr0.001_l2_w')
        ck = os.path.join(out, 'model_w_1_final_walk_module.ckpt')
        r = evaluate.main([os.path.join(out, 'opt.yml'), '--save_path_w', ck, '--num_samples', '8', '--num_panels', '3',
                           '--attrPath', './dataset/attributes_celeba.txt', '--target_attrList', 'Smiling'], all_batches=True)
        assert r['index_'] == 31 and sum(r['bucket_sizes']) <= 8 * 3 and sum(r['bucket_sizes']) > 0
        assert len(r['results_avg']) == sum(1 for b in r['bucket_sizes'] if b)
        last = evaluate.main([os.path.join(out, 'opt.yml'), '--save_path_w', ck, '--num_samples', '8', '--num_panels', '3',
                              '--attrPath', './dataset/attributes_celeba.txt', '--target_attrList', 'Smiling'])
        assert sum(last['bucket_sizes']) <= 4 * 3                       # reference quirk: only the last batch is scored
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_train_multi_attr_cli(tmp_path):
    """train_multi_attr.py (BASELINE config 4 flow: five CelebA attributes, clamped targets, full loss) end to end at 32^2: the
    walk tensor has one direction per attribute and moves; log and checkpoints are written under the reference's names."""
    import os
    from latent2im_amd import constants, trainer
    os.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    models = str(tmp_path / 'models')
    argv = ['--model', 'stylegan_v2_real', '--transform', 'face', '--num_samples', '8', '--learning_rate', '1e-3', '--latent', 'w',
            '--walk_type', 'linear', '--loss', 'l2', '--attrList', 'Smiling,Young,Male,Eyeglasses,Bangs',
            '--attrPath', './dataset/attributes_celeba.txt', '--models_dir', models, '--overwrite_config', '--resolution', '32',
            '--batch_size', '4', '--n_epoch', '1', '--seed', '3', '--model_save_freq', '1', '--synthetic_weights']
    try:
        trainer.main(multi_attr=True, argv=argv)
        out = os.path.join(models, 'stylegan_v2_real_face_linear_lr0.001_l2_w')
        first = torch.load(os.path.join(out, 'model_w_0_walk_module.ckpt'), map_location='cpu', weights_only=False)
        last = torch.load(os.path.join(out, 'model_w_1_final_walk_module.ckpt'), map_location='cpu', weights_only=False)
        assert tuple(last.w.shape) == (5, 8, 512) and torch.isfinite(last.w).all()
        assert torch.equal(last.w.detach(), first.w.detach())                     # one epoch: the epoch-0 and the final checkpoint are the same state
        assert float(last.w.detach().std()) > 0.01                               # N(0, 0.02) init, moved by two Adam steps
        assert 'T, epc, bst, lss, alpha:' in open(os.path.join(out, 'log.txt')).read()
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_nonlinear_walks_on_device_match_reference(golden):
    """WalkMlpMultiW / WalkNonLinearW (transform_base.py:168-243) built on the GPU like the graph builds them
    (.to(device)), against the outputs of the reference's own modules (tests/golden/next.npz), and a training step of the product
    graph with the MLP walk switched on (constants.WALK_IS_MLP: the reference's hand-edited ``is_mlp``): the gradient reaches every
    MLP parameter and one Adam step changes them."""
    from latent2im_amd import constants, graph
    from tests import emu
    g = golden('next')
    ws = [T(synth.z_sample(4, seed=21 + i)).float().to(DEV) for i in range(3)]
    al = T(np.asarray([[0.3], [-0.7], [1.2], [0.0]], dtype=np.float32)).to(DEV)
    mlp = graph.WalkMlpMultiW(512, 6, 1, ['Smiling'])
    emu.seeded_state(mlp, 31)
    mlp = mlp.to(DEV)
    close(torch.stack(mlp(ws, al)), g['mlp.out'], 1e-4, 1e-5)
    with pytest.raises(TypeError):
        mlp(ws, al, layers=[0])
    nl = graph.WalkNonLinearW(512, 6, 1, ['Smiling'])
    emu.seeded_state(nl, 32)
    nl = nl.to(DEV)
    close(torch.stack(nl(ws, None, al, None)), g['nonlinear.out'], 1e-4, 1e-5)
    close(torch.stack(nl(ws, None, al, None, layers=[1])), g['nonlinear.out_layers1'], 1e-4, 1e-5)
    with pytest.raises(TypeError):
        nl(ws, alpha=al, layers=None)
    # the product graph with the MLP walk: one real step (regressor-only loss at 32^2)
    try:
        constants.WALK_IS_MLP = True
        gr = selfcheck.build_graph(32, ['Smiling'], 4, lr=1e-3)
        assert type(gr.walk).__name__ == 'WalkMlpMultiW' and next(gr.walk.parameters()).is_cuda
        before = [p.detach().clone() for p in gr.walk.parameters()]
        zs = synth.z_sample(4, seed=2)
        z = T(zs).float().to(DEV)
        w = gr.get_w(z)
        x0 = gr.get_logits({'w': w})
        a0 = gr.get_reg_preds(x0)
        ag = torch.full((4, 1), 0.8, device=DEV)
        w1 = gr.get_w_new_tensor(w, gr.get_alphas(a0, ag))
        x1 = gr.get_logits({'w': w1})
        loss = gr.optimizeParametersAll({'w': w1, 'org': x0, 'logit': x1, 'alpha': ag}, False, False, no_content_loss=True, no_gan_loss=True)
        assert torch.isfinite(loss)
        for p, b in zip(gr.walk.parameters(), before):
            assert p.grad is not None and float(p.grad.abs().max()) > 0
            assert not torch.equal(p.detach(), b)
    finally:
        constants.WALK_IS_MLP = False
        constants.resolution, constants.BATCH_SIZE = 256, 4


@pytest.mark.parametrize('no_gan', [True, False])
def test_data_parallel_product_graph_matches_single_process(tmp_path, no_gan):
    """SURVEY 8(e) on the product graph: two fresh rank processes (sharing this box's one GPU, process group over gloo —
    L2I_DIST_BACKEND=gloo; on a multi-GPU node the same code runs one rank per GPU over RCCL) run the real faceGraph for two
    optimizeParametersAll steps on their strided shards of a global batch of 8, with the single all-reduce of the walk gradient
    inside the step; a single process runs the same steps on the global batch.  The all-reduced gradient, every (mean) loss term and
    the walk after two Adam steps must agree — with the GAN term too: the strided shards keep the discriminator's minibatch-stddev
    subgroups {0,2,4,6} / {1,3,5,7} intact (dist.shard)."""
    import os
    import subprocess
    import sys
    from latent2im_amd import dist
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dp_worker.py')
    args = ['64', '8', '2', '1' if no_gan else '0']
    env = dict(os.environ, L2I_DIST_BACKEND='gloo')
    env.pop('WORLD_SIZE', None)
    single, multi = str(tmp_path / 'single.npz'), str(tmp_path / 'dp2.npz')
    # (one after the other: three processes time-slicing the box's one GPU at once were measured 2x SLOWER than the two runs in sequence)
    r = subprocess.run([sys.executable, worker, single] + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    codes, _ = dist.spawn_local(2, [sys.executable, worker, multi] + args, env=env, timeout=600)
    assert codes == [0, 0], codes
    a, b = np.load(single), np.load(multi)
    assert int(a['world']) == 1 and int(b['world']) == 2
    close(b['losses'][0], a['losses'][0], 1e-4, 1e-6)                 # total, reg, content (, gan): mean of shard means == global mean
    # the second step starts from the walk Adam produced: ~ lr * sign(g) per entry, so entries whose gradient is within rounding of
    # zero may have stepped the other way (see below) and the small content term sees it at the 1e-4 level
    close(b['losses'][1], a['losses'][1], 1e-3, 1e-6)
    for s in range(2):
        # same samples, different launch shapes: at 64^2 most maps are <= 16 x 16, where a batch-4 and a batch-8 launch pack different samples
        # into a tile and sum in a different order, so ReLU / max-pool masks within rounding of zero flip between the two runs (they do not
        # between either run and the oracle's bar at the bench shapes): 2.5 % of the entries may be off by more than 2e-3 of the largest, none by 10 %
        # ([r6] measured 1.9 % / largest deviation 0.5 % of max with the pre-masked ResNet trunk, 0.9 % with the round-5 plumbing — two forms that agree to
        #  2e-5 on equal launch shapes, test_resnet_backward_premasked_trunk_equals_round5_plumbing: which masks flip between a batch-4 and a batch-8
        #  launch is chaotic in the summation order, the size of what a flip moves is what the second bound holds)
        grad_ok(T(b['grads'][s]), T(a['grads'][s]), frac_tol=2.5e-2)
        assert relmax(T(b['grads'][s]), T(a['grads'][s])) < 2e-2
    step = np.abs(a['walk'] - synth.walk_init(2, 10, seed=7).reshape(-1)).max()
    assert step > 1e-4                                                # Adam moved the walk ...
    # ... and both runs moved it the same way.  Adam's first updates are ~ lr * sign(g): entries whose gradient is within rounding
    # of zero may legitimately step the other way, so the comparison is made where the gradient is well away from zero
    clear = np.abs(a['grads']).min(0) > 0.02 * np.abs(a['grads']).max()
    assert clear.mean() > 0.1
    assert np.abs(b['walk'] - a['walk'])[clear].max() < 0.05 * step
    assert np.median(np.abs(b['walk'] - a['walk'])) < 0.01 * step


def test_data_parallel_mlp_walk_broadcast_and_step(tmp_path):
    """Data parallelism with a walk that has no ``.w`` (WalkMlpMultiW, transform_base.py:168-204, six parameter tensors): every rank
    builds its own random init (different torch seeds), dist.broadcast_parameters makes rank 0's the common start (trainer.main /
    bench.py), the all-reduce covers every parameter gradient.  Two ranks on strided shards == one process on the global batch."""
    import os
    import subprocess
    import sys
    from latent2im_amd import dist
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dp_worker.py')
    args = ['32', '8', '2', '1', 'mlp']
    env = dict(os.environ, L2I_DIST_BACKEND='gloo')
    env.pop('WORLD_SIZE', None)
    single, multi = str(tmp_path / 'single.npz'), str(tmp_path / 'dp2.npz')
    # (one after the other: three processes time-slicing the box's one GPU at once were measured 2x SLOWER than the two runs in sequence)
    r = subprocess.run([sys.executable, worker, single] + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    codes, _ = dist.spawn_local(2, [sys.executable, worker, multi] + args, env=env, timeout=600)
    assert codes == [0, 0], codes
    a, b = np.load(single), np.load(multi)
    assert int(b['world']) == 2 and a['walk'].shape == b['walk'].shape and a['walk'].size > 512 * 1024
    close(b['losses'][0], a['losses'][0], 1e-4, 1e-6)
    grad_ok(T(b['grads'][0]), T(a['grads'][0]))
    assert relmax(T(b['grads'][0]), T(a['grads'][0])) < 2e-2
    assert np.median(np.abs(b['walk'] - a['walk'])) < 1e-5            # same start (the broadcast) and the same two Adam steps


@pytest.mark.parametrize('size,batch', [(32, 8), (64, 16), (128, 8)])
def test_networks_small_maps_large_batch_vs_oracle(size, batch):
    """Every frozen network where a kernel tile packs many samples (<= 4x4 maps at batch >= 8: ResNet-50's tail at small inputs, the
    first generator / last discriminator blocks) against the CPU oracle.  Regression test of a round-2 finding (the scale table of
    the implicit-GEMM kernel was only filled for the first 256 (sample, channel) pairs of a tile)."""
    stG, stR, stV, stD = (synth.generator_state(size, seed=100), synth.resnet50_state(seed=300), synth.vgg19_prefix_state(seed=400),
                          synth.discriminator_state(size, seed=200))
    G = Generator(stG, size, device=DEV)
    z = T(synth.z_sample(batch, seed=3)).float()
    w = G.style(z.to(DEV))
    img = G.synthesis(torch.stack([w] * G.n_latent, 1).contiguous())
    PG = ostep.to_torch(stG)
    img_o = sg2.generator_synthesis(PG, torch.stack([sg2.style_mlp(PG, z)] * G.n_latent, 1), None)
    close(img, img_o)
    close(ResNet50(stR, device=DEV)(img_o.to(DEV)), onets.resnet50_forward(ostep.to_torch(stR), img_o))
    close(Discriminator(stD, size, device=DEV)(img_o.to(DEV)), sg2.discriminator_forward(ostep.to_torch(stD), img_o))
    other = torch.roll(img_o, 3, 3)
    _, lo = ostep.content_loss(ostep.to_torch(stV), other, img_o)
    close(VGG19Prefix(stV, device=DEV).content_losses(other.to(DEV), img_o.to(DEV)), torch.stack(lo), 1e-3, 1e-6)


def test_hipgraph_captured_step_matches_eager(precision):
    """BASELINE config 5's step shape at test size: SceneGraph on the transient-scene attribute table, five attributes, the
    train_multi_attr.py clamp flow, forward+backward replayed from ONE hipGraph (latent2im_amd.capture.CapturedStep: static device
    inputs, device-side epsilon, the three loss-branch streams captured as forks) — against the same steps launched eagerly and
    against the CPU oracle.  Three optimiser steps: the replayed graph must follow the walk as Adam moves it."""
    from latent2im_amd import capture, constants
    try:
        attrs = ['dirty', 'daylight', 'night', 'sunrisesunset', 'dawndusk']
        size, batch = 64, 4
        rs = np.random.RandomState(3)
        zs = [synth.z_sample(batch, seed=40 + i) for i in range(3)]
        al = [np.ones((batch, 5)) * rs.uniform(-1, 1, 5) for _ in range(3)]          # SceneTransform.get_train_alpha
        ge = selfcheck.build_graph(size, attrs, batch, lr=1e-3, transform='scene')
        assert type(ge).__name__ == 'SceneGraph' and ge.attrIdx == [0, 1, 2, 3, 4]
        eager = [selfcheck.run_step(ge, zs[i], al[i], clamp=True) for i in range(3)]
        gc = selfcheck.build_graph(size, attrs, batch, lr=1e-3, transform='scene')
        step = capture.CapturedStep(gc, batch, 5, clamp=True)
        for i in range(3):
            r = step(zs[i], al[i])
            torch.cuda.synchronize()
            close(r['x1'], eager[i]['x1'], 1e-4, 1e-5)
            close(r['eps'], eager[i]['eps'], 1e-4, 1e-6)
            close(r['loss'], eager[i]['loss'], 1e-5, 1e-6)
            assert relmax(r['grad'], eager[i]['grad']) < 1e-3
        assert relmax(gc.walk.w, ge.walk.w) < 1e-3 and not torch.equal(gc.walk.w.detach().cpu(), T(synth.walk_init(5, 10, seed=7)))
        # the first step against the oracle (scene attribute indices 0..4, clamp flow)
        o = ostep.train_step(_oracle_nets(size), T(synth.walk_init(5, 10, seed=7)), T(zs[0]).float(), T(al[0]).float(), [0, 1, 2, 3, 4], clamp_variant=True)
        close(eager[0]['x1'], o['x1'])
        close(eager[0]['eps'], o['eps'])
        close(eager[0]['loss'], o['loss'], 1e-3, 1e-4)
        assert relmax(eager[0]['grad'], o['grad']) < 2e-2
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4


def test_regressor_training_step_vs_oracle(tmp_path):
    """SURVEY 8(f-4), scene_regressor_256.py:118-171: optimiser steps of the ResNet-50 regressor (BatchNorm in training mode, MSE loss,
    Adam over every parameter) on the HIP kernels — weight gradients by l2i_conv2d_wgrad_f32, BatchNorm by l2i_bn_* — against the CPU
    oracle (torch autograd on the restated network).

    Gradients are checked at two levels.  (1) EXACTLY, block by block: the stem and three bottleneck blocks (with / without downsample,
    stride 1 / 2) are back-propagated on the GPU from their saved inputs and a random incoming gradient, and compared with float64 autograd
    of the same block on the same inputs: every parameter gradient and the input gradient to 1e-4 of its largest entry.  (2) END TO END
    against the float64 oracle.  With batch statistics over 128 values per channel in the last layer a single ReLU flipped by float32
    rounding moves that channel's gradients by ~1 % (the float32 CPU oracle itself is up to 7 % away from float64 on some tensors), so the
    whole-network comparison is in norms: cosine similarity >= 0.999 and relative L2 error <= 5 % per parameter tensor."""
    import torch.nn.functional as F
    from latent2im_amd import regressor_train as RT
    rs = np.random.RandomState(5)
    st = synth.resnet50_state(seed=300)
    data = T(rs.randn(8, 3, 128, 128).astype(np.float32) * 0.5)
    label = T(rs.rand(8, 40).astype(np.float32))
    model = RT.TrainableResNet50(st, device=DEV)
    P64 = {k: v.clone() for k, v in ostep.to_torch(st, torch.float64).items()}
    _, g64 = onets.resnet50_train_step(P64, data.double(), label.double(), lr=1e-4, steps=1)
    P = {k: v.clone() for k, v in ostep.to_torch(st).items()}
    lo1, g1 = onets.resnet50_train_step(P, data, label, lr=1e-4, steps=1)
    preds = model(data.to(DEV))
    sv = model._saved
    loss, g = RT.mse_loss_and_grad(preds, label.to(DEV))
    close(loss, lo1[0], 1e-4, 1e-6)
    D = lambda t: t.detach().double().cpu()
    rel = lambda a, b: float((D(a) - b.detach()).abs().max() / b.detach().abs().max())
    # (1) block-level exactness
    for bi in (0, 3, 4, 15):
        blk, saved = model.blocks[bi], sv['blocks'][bi]
        cur, y1, s1, y2, s2, s3, sd, out = saved
        gin = torch.randn(out.shape, generator=torch.Generator().manual_seed(bi)).to(DEV)
        x = D(cur).requires_grad_(True)
        prm = {}
        for c_, b_ in (('c1', 'b1'), ('c2', 'b2'), ('c3', 'b3'), ('cd', 'bd')):
            if blk[c_] is not None:
                prm[blk[c_].name + '.weight'] = D(blk[c_].weight).requires_grad_(True)
                prm[blk[b_].name + '.weight'], prm[blk[b_].name + '.bias'] = D(blk[b_].weight).requires_grad_(True), D(blk[b_].bias).requires_grad_(True)
        bn = lambda t, b_: F.batch_norm(t, None, None, prm[blk[b_].name + '.weight'], prm[blk[b_].name + '.bias'], training=True, eps=1e-5)
        cv = lambda t, c_: F.conv2d(t, prm[blk[c_].name + '.weight'], stride=blk[c_].stride, padding=blk[c_].padding)
        pre = bn(cv(F.relu(bn(cv(F.relu(bn(cv(x, 'c1'), 'b1')), 'c2'), 'b2')), 'c3'), 'b3')
        pre = pre + (bn(cv(x, 'cd'), 'bd') if blk['cd'] is not None else x)
        o = F.relu(pre)
        # same ReLU pattern (the comparison below is then exact arithmetic) — except where the float64 pre-activation is a rounding error away
        # from zero (the 3x3 of blocks on maps >= 32 wide runs on F(4x4): ~1e-5 of the largest value): at most a handful of entries, and the
        # incoming gradient is zeroed there on both sides so the mask's value at them does not matter
        flip = (D(out) > 0).ne(o > 0)
        assert int(flip.sum()) <= 4 and (int(flip.sum()) == 0 or float(pre.detach()[flip].abs().max()) < 1e-5 * float(pre.detach().abs().max())), \
            (bi, int(flip.sum()), float(pre.detach()[flip].abs().max()) / float(pre.detach().abs().max()))
        gin = gin * (~flip).to(DEV)
        grads = {}
        gx = model.block_backward(blk, saved, gin, grads)
        ref = torch.autograd.grad(o, [x] + list(prm.values()), D(gin))
        assert rel(gx, ref[0]) < 1e-4, (bi, 'input', rel(gx, ref[0]))
        for k, r in zip(prm, ref[1:]):
            assert rel(grads[k], r) < 1e-4, (bi, k, rel(grads[k], r))
    gpool = torch.randn(sv['blocks'][0][0].shape, generator=torch.Generator().manual_seed(99)).to(DEV)
    grads = {}
    model.stem_backward(sv, gpool, grads)
    w0, gam, bet = D(model.stem.weight).requires_grad_(True), D(model.stem_bn.weight).requires_grad_(True), D(model.stem_bn.bias).requires_grad_(True)
    o = F.max_pool2d(F.relu(F.batch_norm(F.conv2d(D(data), w0, stride=2, padding=3), None, None, gam, bet, training=True, eps=1e-5)), 3, 2, 1)
    for k, r in zip(('conv1.weight', 'bn1.weight', 'bn1.bias'), torch.autograd.grad(o, (w0, gam, bet), D(gpool))):
        assert rel(grads[k], r) < 1e-4, (k, rel(grads[k], r))
    # (2) end to end against the float64 oracle, in norms
    grads = model.backward(g)
    worst = (1.0, 0.0, '')
    for k, want in g64.items():
        got = D(grads[k]).reshape(-1)
        w_ = want.reshape(-1)
        cos = float(torch.dot(got, w_) / (got.norm() * w_.norm() + 1e-300))
        l2 = float((got - w_).norm() / (w_.norm() + 1e-300))
        worst = min(worst, (cos, l2, k))
        assert cos >= 0.999 and l2 <= 5e-2, (k, cos, l2)
    print('regressor training: lowest cosine similarity with the float64 oracle gradient %.6f (relative L2 error %.2e) at %s' % worst)
    # the whole step through train_step (a fresh model: the statistics above were already updated once)
    model = RT.TrainableResNet50(st, device=DEV)
    opt = RT.make_optimizer(model, lr=1e-4)
    l1 = RT.train_step(model, opt, data.to(DEV), label.to(DEV))
    close(l1, lo1[0], 1e-4, 1e-6)
    sd = model.state_dict()
    for k in ('bn1.running_mean', 'bn1.running_var', 'layer2.0.downsample.1.running_var', 'layer4.2.bn3.running_mean'):
        close(sd[k], P[k], 1e-3, 1e-5)
    assert int(sd['bn1.num_batches_tracked']) == 1
    # Adam's first step moves every entry by ~lr * sign(g): compare where the gradient is clearly non-zero
    for k in ('conv1.weight', 'layer1.0.conv2.weight', 'layer3.5.conv3.weight', 'layer4.0.downsample.0.weight', 'fc.weight', 'layer2.1.bn2.weight'):
        w0 = T(np.asarray(st[k])).double()
        moved_ref, moved = P[k].detach().double() - w0, sd[k].cpu().double() - w0
        gk = g1[k].double()
        clear = gk.abs() > 0.05 * gk.abs().max()
        assert float((moved - moved_ref)[clear].abs().max()) < 0.05e-4 and float(moved_ref[clear].abs().min()) > 0.5e-4, k
    # a second step: the loss must have been computed on the updated parameters and statistics (compared with the oracle's own second
    # forward; its Adam state restarts, which does not enter the loss)
    lo2, _ = onets.resnet50_train_step(P, data, label, lr=1e-4, steps=1)
    l2 = RT.train_step(model, opt, data.to(DEV), label.to(DEV))
    close(l2, lo2[0], 2e-3, 1e-6)
    assert int(model.state_dict()['bn1.num_batches_tracked']) == 2
    # checkpoint in the reference's format -> the frozen regressor of the walk path
    path = str(tmp_path / '001_dict.model')
    RT.save_ckpt(path, model, opt)
    ck = torch.load(path, map_location='cpu')
    assert set(ck) == {'model', 'optm'} and 'layer4.2.bn3.running_var' in ck['model'] and ck['model']['fc.weight'].shape == (40, 2048)
    frozen = ResNet50({k: v.numpy() for k, v in ck['model'].items()}, device=DEV)
    close(frozen(data.to(DEV)), onets.resnet50_forward({k: v.float() for k, v in ck['model'].items()}, data))      # eval-mode use by the walk path
    fresh = RT.TrainableResNet50(st, device=DEV)
    m2, _ = RT.load_ckpt(path, fresh, RT.make_optimizer(fresh))
    assert torch.equal(m2.state_dict()['layer1.0.conv1.weight'].cpu(), ck['model']['layer1.0.conv1.weight'])


def test_rccl_one_rank_group_through_optimize_parameters(tmp_path):
    """The `nccl` backend path of latent2im_amd.dist (RCCL; dist.py:init_from_env) on the one GPU of this box: L2I_FORCE_PG=1 builds a
    ONE-rank RCCL process group, and the product graph's optimizeParametersAll then runs its all-reduce of the walk gradient over it
    (dist.average_gradients no longer short-cuts a one-rank group).  Same losses, gradient and walk as the run without a group."""
    import os
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dp_worker.py')
    args = ['32', '4', '2', '0']
    base = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'L2I_DIST_BACKEND', 'L2I_FORCE_PG')}
    plain, forced = str(tmp_path / 'plain.npz'), str(tmp_path / 'rccl1.npz')
    r = subprocess.run([sys.executable, worker, plain] + args, env=base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(base, L2I_FORCE_PG='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29517', HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, worker, forced] + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = np.load(plain), np.load(forced)
    assert str(a['backend']) == 'none' and str(b['backend']) == 'nccl' and int(b['world']) == 1
    close(b['losses'], a['losses'], 1e-5, 1e-7)
    assert relmax(T(b['grads']), T(a['grads'])) < 1e-3               # same kernels; atomics in the reductions reorder a few sums
    assert np.median(np.abs(b['walk'] - a['walk'])) < 1e-6


def test_hipgraph_replays_back_to_back_without_host_sync():
    """CapturedStep refills the graph's static inputs from a ring of pinned staging buffers (one event per slot): the host may queue
    several replays ahead of the GPU (bench.py c5, trainer --hip_graph --no_log_sync) without a later step's z / alpha overwriting a
    staging buffer whose copy has not run yet.  Six steps queued with no synchronisation in between (more than the ring holds) against
    the same six steps launched eagerly with a sync after each."""
    from latent2im_amd import capture, constants
    try:
        attrs = ['dirty', 'daylight', 'night']
        size, batch, n = 32, 4, 6
        rs = np.random.RandomState(5)
        zs = [synth.z_sample(batch, seed=60 + i) for i in range(n)]
        al = [np.ones((batch, 3)) * rs.uniform(-1, 1, 3) for _ in range(n)]
        ge = selfcheck.build_graph(size, attrs, batch, lr=1e-3, transform='scene')
        for i in range(n):
            selfcheck.run_step(ge, zs[i], al[i], clamp=True)
            torch.cuda.synchronize()
        gc_ = selfcheck.build_graph(size, attrs, batch, lr=1e-3, transform='scene')
        step = capture.CapturedStep(gc_, batch, 3, clamp=True)
        torch.cuda.synchronize()
        for i in range(n):                                            # no synchronisation: the host runs ahead
            step(zs[i], al[i])
        torch.cuda.synchronize()
        w0 = T(synth.walk_init(3, 8, seed=7))
        moved = float((ge.walk.w.detach().cpu() - w0).abs().max())
        assert moved > 3e-3                                           # six Adam steps of ~lr each
        d = (gc_.walk.w.detach().cpu() - ge.walk.w.detach().cpu()).abs()
        # a step fed with the wrong z / alpha moves most entries the other way at least once: the median stays at rounding level only
        # when every replay saw its own inputs
        assert float(d.median()) < 1e-5 and float((d > 0.2 * moved).double().mean()) < 0.02, (float(d.median()), float(d.max()), moved)
    finally:
        constants.resolution, constants.BATCH_SIZE = 256, 4



# ---- [r6] the reference's ModulatedConv2d / StyledConv / ToRGB layer fixtures (tests/golden/modconv.npz, networks.py:176-358) on the HIP kernels ------
# The generator tests above pin whole images; these pin ONE layer each, with the call sequence generator._SynthesisFn uses for it (style-scaled input,
# demodulation as the conv's out_scale, blur + noise + bias + leaky ReLU in the FIR epilogue, the input gradient with the demodulation as in_scale, the
# style gradient from the pixel reductions), so a kernel regression is localised to a layer instead of showing up as a wrong 1024^2 image.
def _modconv_case(g, name):
    import math
    from latent2im_amd.generator import _Mod
    P = {'m.' + k[len(name) + 3:]: g[k] for k in g.files if k.startswith(name + '.P.')}
    W = T(P['m.weight'])[0]
    cout, cin, k, _ = W.shape
    ws = W * (1.0 / math.sqrt(cin * k * k))
    mod = _Mod(P, 'm', DEV)
    x, w, gy = (T(g['%s.%s' % (name, n)]).float().to(DEV) for n in ('x', 'w', 'gy'))
    return P, ws, mod, x, w, gy


@pytest.mark.parametrize('name,up', [('same', False), ('up', True), ('same512', False), ('up512', True)])
def test_modulated_conv_layer_fixture(golden, precision, name, up):
    """ModulatedConv2d with demodulation (networks.py:231-272), plain and upsampling: y, d y / d x and d y / d style against the reference's own
    autograd on its own module, through FrozenConv2d.forward(in_scale, out_scale) / the blur FIR / FrozenConv2d.dgrad(in_scale) / dot_reduce."""
    from latent2im_amd import conv as C, kernels as K
    g = golden('modconv')
    P, ws, mod, x, w, gy = _modconv_case(g, name)
    s = mod(w)                                                                          # [B, Cin]
    Tm = (ws * ws).sum((2, 3)).to(DEV)                                                  # [Cout, Cin]
    demod = torch.rsqrt((s * s) @ Tm.t() + 1e-8)
    cv = C.FrozenConv2d(ws, stride=2 if up else 1, padding=0 if up else 1, transposed=up, device=DEV)
    t = cv.forward(x, in_scale=s.contiguous(), out_scale=demod.contiguous())
    if up:
        bk = T(P['m.blur.kernel']).to(DEV)
        y = K.upfirdn2d(t, bk, pad=(1, 1, 1, 1))
    else:
        y = t
    close(y, g[name + '.y'], 2e-4, 2e-5)
    # backward, in the order generator._SynthesisFn.backward runs it
    dt = K.upfirdn2d(gy, torch.flip(bk, [0, 1]).contiguous(), pad=(2, 2, 2, 2)) if up else gy
    dxmod = cv.dgrad(dt.contiguous(), (x.shape[2], x.shape[3]), in_scale=demod.contiguous())        # gradient w.r.t. x * s
    close(dxmod * s[:, :, None, None], g[name + '.gx'], 2e-4, 2e-5)
    q = K.dot_reduce(dxmod, x)                                                          # sum_p dxmod * x: the style gradient through the modulated input
    red = K.dot_reduce(gy, y)                                                           # sum_p gy * y = demod * d demod
    ds = q - s * ((red * demod * demod) @ Tm)                                           # (+ through demod = rsqrt(s^2 T + eps))
    close(ds @ mod.A, g[name + '.gw'], 2e-4, 2e-4)


def test_to_rgb_and_styled_conv_layer_fixtures(golden, precision):
    """ToRGB (1x1 modulated conv without demodulation + bias + up-sampled skip, networks.py:339-358) forward and backward, the bare 1x1 modulated conv
    fixture ('rgb'), and StyledConv (networks.py:302-336: up-sampling modulated conv, blur, explicit noise with weight 0.7, bias, fused leaky ReLU) forward,
    through l2i_torgb_fwd / the up-2 FIR with the addend / l2i_sg2_act_bwd's ToRGB branch and the FIR epilogue."""
    import math
    from latent2im_amd import conv as C, kernels as K
    from latent2im_amd.generator import _Mod, _StyledLayer, _ToRGB
    g = golden('modconv')
    # (1) bare 1x1 modulated conv, demodulate=False
    P, ws, mod, x, w, gy = _modconv_case(g, 'rgb')
    s = mod(w)
    # (a 9 x 9 map: l2i_torgb_fwd / l2i_sg2_act_bwd take whole 4-pixel groups — every map of the generator is a power of two — so this fixture runs
    # on the generic conv kernels: 1x1, style as in_scale, three output channels)
    cv = C.FrozenConv2d(ws, stride=1, padding=0, device=DEV)
    close(cv.forward(x, in_scale=s.contiguous()), g['rgb.y'], 2e-4, 2e-5)
    dxmod = cv.dgrad(gy.contiguous(), (x.shape[2], x.shape[3]))
    close(dxmod * s[:, :, None, None], g['rgb.gx'], 2e-4, 2e-5)
    close(K.dot_reduce(dxmod, x) @ mod.A, g['rgb.gw'], 2e-4, 2e-4)
    SQ2 = math.sqrt(2.0)
    # (2) ToRGB with skip
    Pt = {'t.' + k[len('torgb.P.'):]: g[k] for k in g.files if k.startswith('torgb.P.')}
    R = _ToRGB(Pt, 't', 8, True, DEV)
    x, w, skip, gy = (T(g['torgb.' + n]).float().to(DEV) for n in ('x', 'w', 'skip', 'gy'))
    s = R.mod(w)
    wmod = (R.W[None] * s[:, None, :]).contiguous()
    rgb = K.torgb_fwd(x, wmod, R.bias)
    y = K.upfirdn2d(skip, R.up_k, up=(2, 2), pad=(2, 1, 2, 1), addend=rgb)
    close(y, g['torgb.y'], 2e-4, 2e-5)
    close(K.upfirdn2d(gy, R.up_k_flip, up=(1, 1), down=(2, 2), pad=(1, 1, 1, 1)), g['torgb.gskip'], 2e-4, 2e-5)
    dz, _, red = K.sg2_act_bwd(x, None, None, gy, wmod, torch.zeros(8, device=DEV), None, 0.0, 0.2, SQ2)
    close(dz / torch.where(x > 0, SQ2, 0.2 * SQ2), g['torgb.gx'], 2e-4, 2e-5)
    close(((red * R.W.t()[None]).sum(2)) @ R.mod.A, g['torgb.gw'], 2e-4, 2e-4)
    # (3) StyledConv, upsample=True, explicit noise
    Ps = {'s.' + k[len('styled.P.'):]: g[k] for k in g.files if k.startswith('styled.P.')}
    L = _StyledLayer(Ps, 's', 8, 6, True, DEV)
    x, w, nz = (T(g['styled.' + n]).float().to(DEV) for n in ('x', 'w', 'noise'))
    s = L.mod(w)
    demod = torch.rsqrt((s * s) @ L.T.t() + 1e-8)
    t = L.conv.forward(x, in_scale=s.contiguous(), out_scale=demod.contiguous())
    y = K.upfirdn2d(t, L.blur_k, pad=(1, 1, 1, 1), noise=nz.contiguous(), noise_w=L.noise_w, bias=L.bias, act=K.ACT_LRELU, slope=0.2, gain=SQ2)
    assert abs(L.noise_w - 0.7) < 1e-6
    close(y, g['styled.y'], 2e-4, 2e-5)


@pytest.mark.parametrize('size,batch', [(64, 8), (64, 4), (256, 2)])
def test_resnet_backward_premasked_trunk_equals_round5_plumbing(size, batch):
    """[r6] regressor._ResNetFeatFn.backward carries the gradient w.r.t. each block's PRE-ReLU sum (the block-input mask applied once, in the epilogue of
    the launch that produces it) where round 5 carried the gradient w.r.t. the ReLU output and masked it in both consumers.  Same masks (the stored
    activations), same products, another order of the two fp32 additions per element: the image gradients of the two forms must agree to fp32
    rounding — far below the mask-flip bar the gradient tests need against the oracle."""
    from latent2im_amd import regressor as R
    net = ResNet50(synth.resnet50_state(seed=300), device=DEV)
    rs = np.random.RandomState(size + batch)
    x = T(rs.randn(batch, 3, size, size) * 0.5).float().to(DEV)
    gy = T(rs.randn(batch, 40)).float().to(DEV)
    grads = []
    old = R.PREMASK
    try:
        for flag in (True, False):
            R.PREMASK = flag
            xg = x.clone().requires_grad_(True)
            net(xg).backward(gy)
            grads.append(xg.grad.detach().double().cpu())
    finally:
        R.PREMASK = old
    err = float((grads[0] - grads[1]).abs().max() / grads[1].abs().max())
    assert err < 2e-5, err


@pytest.mark.parametrize('c1,c2,c3,h,w,batch', [(64, 256, 64, 16, 32, 2), (64, 256, 128, 16, 16, 3), (128, 512, 128, 32, 32, 1)])
def test_conv1x1_pair_f32_matches_two_launches(c1, c2, c3, h, w, batch):
    """[r6] l2i_conv1x1_pair_f32 (csrc/l2i_pair_f32.hip): ResNet-50's conv3 + identity + ReLU and the next block's conv1 + ReLU in one fp32 launch, the wide map
    handed over in the MFMA's registers.  Against the two l2i_conv2d_f32 launches: the wide map bit for bit (same K order), the second conv's output to fp32
    rounding (its channel pairs are summed in another order: 1e-5 of the map's magnitude), and both against float64 torch."""
    from latent2im_amd import conv
    rs = np.random.RandomState(c1 + h)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    wa, wb = T(rs.randn(c2, c1, 1, 1) / np.sqrt(c1)), T(rs.randn(c3, c2, 1, 1) / np.sqrt(c2))
    A, Bc = conv.FrozenConv2d(wa, 1, 0, device=DEV), conv.FrozenConv2d(wb, 1, 0, device=DEV)
    x, res = T(rs.randn(batch, c1, h, w)).to(DEV), T(rs.randn(batch, c2, h, w)).to(DEV)
    ba, bb = T(rs.randn(c2)).to(DEV), T(rs.randn(c3) * 0.3).to(DEV)
    assert conv.pair_f32_shapes_ok(c1, c2, c3, h * w)
    mid0 = A.forward(x, bias=ba, residual=res, act=conv.ACT_RELU)
    out0 = Bc.forward(mid0, bias=bb, act=conv.ACT_RELU)
    d = []
    mid1 = A.forward(x, bias=ba, residual=res, act=conv.ACT_RELU, _defer=d)
    out1 = Bc.forward(mid1, bias=bb, act=conv.ACT_RELU, _defer=d)
    conv.launch_pair_f32(d)
    torch.cuda.synchronize()
    ref_mid = torch.relu(torch.nn.functional.conv2d(x.double(), wa.double().to(DEV)) + ba.double().view(1, -1, 1, 1) + res.double())
    ref_out = torch.relu(torch.nn.functional.conv2d(ref_mid, wb.double().to(DEV)) + bb.double().view(1, -1, 1, 1))
    scale_m, scale_o = float(ref_mid.abs().max()), float(ref_out.abs().max())
    assert float((mid1.double() - ref_mid).abs().max()) < 2e-6 * scale_m and float((out1.double() - ref_out).abs().max()) < 4e-6 * scale_o
    assert float((mid1 - mid0).abs().max()) < 1e-6 * scale_m and float((out1 - out0).abs().max()) < 1e-5 * scale_o
    assert 0.1 < float((out1 > 0).float().mean()) < 0.9


def test_fused_regressor_bce_matches_torch_ops():
    """[r6] l2i_reg_bce_f32 (csrc/l2i_loss.hip): fc + attribute-column select + the float64 BCE of transform_base.py:416-424 and their autograd backward in one
    launch each way, against the torch expression it replaces (graph.get_bce_loss on fc(feat)[:, cols]) — loss (float64) and d loss / d feat, for float64 and fp32
    targets, with predictions on both sides of the clamp (pred < eps and 1 - pred < eps: the clamp stops the gradient there), K = 1, 5, 40."""
    from latent2im_amd import graph as G
    rs = np.random.RandomState(7)
    F, A = 2048, 40
    fc_w = torch.from_numpy((rs.randn(A, F) / np.sqrt(F)).astype(np.float32)).to(DEV)
    fc_b = torch.from_numpy((rs.randn(A) * 0.3 + 0.5).astype(np.float32)).to(DEV)
    bce = G.TransformGraph.get_bce_loss
    for B, cols, dt in ((8, [3, 7, 11, 20, 39], torch.float64), (8, [31], torch.float32), (3, list(range(40)), torch.float64)):
        K = len(cols)
        feat0 = torch.from_numpy(rs.randn(B, F).astype(np.float32) * 0.8).to(DEV)
        target = torch.from_numpy(rs.uniform(0, 1, size=(B, K))).to(DEV).to(dt)
        ci = torch.tensor(cols, dtype=torch.long, device=DEV)
        fa = feat0.clone().requires_grad_(True)
        la = bce(None, torch.addmm(fc_b, fa, fc_w.t()).index_select(1, ci), target.to(torch.double)).mean()
        (la * 10).backward()
        fb = feat0.clone().requires_grad_(True)
        lb = G._RegBceFn.apply(fb, fc_w, fc_b, ci, target)
        (lb * 10).backward()
        torch.cuda.synchronize()
        assert lb.dtype == torch.float64 and lb.dim() == 0
        assert abs(float(la) - float(lb)) < 1e-6 * max(1.0, abs(float(la))), (float(la), float(lb))
        scale = float(fa.grad.abs().max())
        # (1 / pred amplifies the last-bit difference of two summation orders of the 2048-long fc dot where pred is small: 1.5e-4 measured with predictions at 1e-3)
        assert scale > 0 and float((fa.grad - fb.grad).abs().max()) < 5e-4 * scale, (float((fa.grad - fb.grad).abs().max()), scale)
        p = torch.addmm(fc_b, feat0, fc_w.t()).index_select(1, ci)
        assert bool((p < 1e-12).any()) and bool((p > 1).any())          # both clamp branches are exercised
