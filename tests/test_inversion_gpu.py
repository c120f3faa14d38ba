"""latent2im_amd.perceptual16 / latent2im_amd.invert against the plain-torch CPU model of tests/inversion_ref.py (BP.py's loss on the oracle's
generator), and the host-side pieces of the inversion path."""
import numpy as np
import pytest
import torch

from latent2im_amd import synth
from latent2im_amd import vgg16_specs as V
from oracle import step as ostep
from tests import inversion_ref as IR

DEV = 'cuda'
_memo = {}


def grad_ok(a, b, frac_tol=5e-3, elem=2e-3, worst=0.1):
    """tests/test_networks_gpu.py's rule for gradients of a piecewise-linear network, restated: at most 0.5 % of the entries may deviate by
    more than 2e-3 * max|g|, and none by more than 10 %."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    m = float(b.abs().max())
    e = (a - b).abs()
    frac = float((e > elem * m).double().mean())
    assert frac <= frac_tol and float(e.max()) <= worst * m, (frac, float(e.max()) / m)


def own_rule(got, ref64, ref32, what):
    """The project's rule: within max(2 x the fp32 CPU model's own deviation from float64, 5e-3) * max|g|."""
    m = float(ref64.abs().max())
    cpu_dev = float((ref32.double() - ref64).abs().max()) / m
    gpu_dev = float((got.detach().cpu().double() - ref64).abs().max()) / m
    print('%s: fp32 CPU model deviates %.3e, GPU %.3e (of max|g|)' % (what, cpu_dev, gpu_dev))
    assert gpu_dev <= max(2.0 * cpu_dev, 5e-3), (what, gpu_dev, cpu_dev)


def _vgg_states():
    if 'vgg' not in _memo:
        st = V.vgg16_state()
        _memo['vgg'] = (st, IR.vgg_state(st, torch.float64), IR.vgg_state(st, torch.float32))
    return _memo['vgg']


def _images(size, batch, seed):
    r = np.random.RandomState(seed)
    return (torch.from_numpy(r.uniform(-1, 1, (batch, 3, size, size))), torch.from_numpy(r.uniform(-1, 1, (batch, 3, size, size))))


def _vgg_ref(size, batch):
    """Loss [B] and image gradient of sum(coef * loss) in float64 and float32 on the CPU, once per shape."""
    key = ('vggref', size, batch)
    if key not in _memo:
        _, P64, P32 = _vgg_states()
        target, img = _images(size, batch, 11 + size)
        coef = torch.linspace(0.5, 1.5, batch, dtype=torch.float64)
        out = {}
        for dt, P in ((torch.float64, P64), (torch.float32, P32)):
            x = img.to(dt).clone().requires_grad_()          # a copy: .to() of the same dtype returns img itself
            loss = IR.perceptual_loss(P, target.to(dt), x)
            (g,) = torch.autograd.grad((loss * coef.to(dt)).sum(), x)
            out[dt] = (loss.detach(), g)
        _memo[key] = (target, img, coef, out)
    return _memo[key]


@pytest.mark.gpu
@pytest.mark.parametrize('size,batch', [(32, 2), (64, 1)])
def test_vgg16_gram_loss_and_image_gradient(size, batch):
    from latent2im_amd.perceptual16 import Vgg16Gram
    target, img, coef, ref = _vgg_ref(size, batch)
    net = Vgg16Gram(_vgg_states()[0], device=DEV)
    grams = net.target_grams(target.float().to(DEV))
    x = img.float().to(DEV).requires_grad_()
    loss = net.loss(x, grams)
    assert loss.shape == (batch,)
    (loss * coef.float().to(DEV)).sum().backward()
    l64, g64 = ref[torch.float64]
    print('loss', loss.tolist(), l64.tolist())
    np.testing.assert_allclose(loss.detach().cpu().double().numpy(), l64.numpy(), rtol=1e-3)
    own_rule(x.grad, g64, ref[torch.float32][1], 'VGG-16 Gram image gradient %d^2 x %d' % (size, batch))
    grad_ok(x.grad, g64)


def _setup(size, batch=1):
    """Synthetic generator of ``size``, fixed noise maps, the target G(w*) of a seeded w*, a start latent: CPU float64 / float32 and GPU forms."""
    key = ('setup', size, batch)
    if key not in _memo:
        stG = synth.generator_state(size, seed=100, noise_strength=0.5)
        r = np.random.RandomState(21 + size)
        nl = 2 * int(np.log2(size)) - 2
        noise = [torch.from_numpy(r.randn(batch, 1, 4 << ((li + 1) // 2), 4 << ((li + 1) // 2))) for li in range(nl - 1)]
        w_star = torch.from_numpy(r.randn(batch, 1, 512)).repeat(1, nl, 1) * 0.7
        w0 = torch.from_numpy(0.3 * r.randn(batch, nl, 512))
        P64 = ostep.to_torch(stG, torch.float64)
        with torch.no_grad():
            target = IR.sg2.generator_synthesis(P64, w_star, noise)
        _memo[key] = dict(stG=stG, noise=noise, w0=w0, target=target, P64=P64, P32=ostep.to_torch(stG, torch.float32))
    return _memo[key]


def _gpu_inverter(s, size, lr=0.01):
    from latent2im_amd.generator import Generator
    from latent2im_amd.invert import Inverter
    from latent2im_amd.perceptual16 import Vgg16Gram
    gen = Generator(s['stG'], size, device=DEV)
    return Inverter(gen, Vgg16Gram(_vgg_states()[0], device=DEV), lr=lr, optim='Adam', n_mean_latent=64)


@pytest.mark.gpu
@pytest.mark.parametrize('size', [32, 64])
def test_one_inversion_step(size):
    s = _setup(size)
    _, V64, V32 = _vgg_states()
    ref = {}
    for dt, PG, PV in ((torch.float64, s['P64'], V64), (torch.float32, s['P32'], V32)):
        w = s['w0'].to(dt).clone().requires_grad_()  # a copy: the memoised w0 stays a plain tensor
        loss, _ = IR.total_loss(PG, PV, w, s['target'].to(dt), [n.to(dt) for n in s['noise']])
        (g,) = torch.autograd.grad(loss, w)
        ref[dt] = (float(loss.detach()), g)
    inv = _gpu_inverter(s, size)
    batch = s['target'].float().to(DEV)
    w = s['w0'].float().to(DEV).requires_grad_()
    loss, _ = inv.loss(w, batch, inv.vgg.target_grams(batch), [n.float().to(DEV) for n in s['noise']])
    loss.backward()
    print('total loss', float(loss), ref[torch.float64][0])
    np.testing.assert_allclose(float(loss), ref[torch.float64][0], rtol=1e-3)
    own_rule(w.grad, ref[torch.float64][1], ref[torch.float32][1], 'dL/dW+ at %d^2' % size)
    grad_ok(w.grad, ref[torch.float64][1])


@pytest.mark.gpu
def test_ten_adam_steps():
    size, n = 32, 10
    s = _setup(size)
    _, V64, V32 = _vgg_states()
    c64, _ = IR.adam_run(s['P64'], V64, s['w0'], s['target'], s['noise'], n, 0.01)
    c32, _ = IR.adam_run(s['P32'], V32, s['w0'].float(), s['target'].float(), [t.float() for t in s['noise']], n, 0.01)
    inv = _gpu_inverter(s, size, lr=0.01)
    w, curve = inv.invert(s['target'].float().to(DEV), n, noise=[t.float().to(DEV) for t in s['noise']], w=s['w0'].float().to(DEV))
    assert w.shape == s['w0'].shape and curve.shape == (n,)
    c64, c32 = np.array(c64), np.array(c32)
    cpu_dev = np.abs(c32 - c64) / np.abs(c64)
    gpu_dev = np.abs(curve - c64) / np.abs(c64)
    print('float64 curve', c64.tolist())
    print('fp32 CPU per-step deviation', cpu_dev.tolist())
    print('GPU per-step deviation', gpu_dev.tolist())
    assert (gpu_dev <= np.maximum(2.0 * cpu_dev, 1e-3)).all(), (gpu_dev, cpu_dev)
    assert curve[-1] < curve[0]


@pytest.mark.gpu
def test_no_conv2d_or_bmm_on_the_path(monkeypatch):
    import torch.nn.functional as F
    s = _setup(32)
    inv = _gpu_inverter(s, 32)

    def refuse(*a, **k):
        raise AssertionError('F.conv2d / torch.bmm on the inversion path')
    monkeypatch.setattr(F, 'conv2d', refuse)
    monkeypatch.setattr(torch, 'bmm', refuse)
    monkeypatch.setattr(torch.Tensor, 'bmm', refuse)
    w, curve = inv.invert(s['target'].float().to(DEV), 1)           # noise drawn
    assert np.isfinite(curve).all() and w.shape == (1, inv.gen.n_latent, 512)


@pytest.mark.gpu
def test_mean_latent():
    from latent2im_amd.generator import Generator
    gen = Generator(synth.generator_state(32, seed=100), 32, device=DEV)
    torch.manual_seed(5)
    m = gen.mean_latent(256)
    torch.manual_seed(5)
    z = torch.randn(256, 512, device=DEV)
    assert m.shape == (1, 512)
    assert torch.equal(m, gen.style(z).mean(0, keepdim=True))


def test_vgg16_state_dict_key_check():
    st = V.vgg16_state()
    tv = {'features.' + k: torch.from_numpy(v) for k, v in st.items()}
    for i in (24, 26, 28):
        tv['features.%d.weight' % i] = torch.zeros(512, 512, 3, 3)
        tv['features.%d.bias' % i] = torch.zeros(512)
    tv['classifier.0.weight'] = torch.zeros(8, 8)
    got = V.load_vgg16_state(tv)
    assert list(got) == list(V.vgg16_spec()) and all(np.array_equal(got[k], st[k]) for k in st)
    assert list(V.load_vgg16_state(st)) == list(st)                 # a features-only dict
    missing = dict(tv)
    del missing['features.21.bias']
    with pytest.raises(KeyError, match='missing'):
        V.load_vgg16_state(missing)
    vgg19 = dict(tv)
    vgg19['features.16.weight'] = torch.zeros(256, 256, 3, 3)      # VGG-19 has a conv where VGG-16 has its third pool
    with pytest.raises(KeyError, match='unexpected'):
        V.load_vgg16_state(vgg19)
    bad = dict(tv)
    bad['features.0.weight'] = torch.zeros(64, 3, 5, 5)
    with pytest.raises(ValueError, match='shape'):
        V.load_vgg16_state(bad)
    assert [c[0] for c in V.VGG16_CONVS] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21]
    assert sum(l[0] == 'pool' for l in V.VGG16_LAYERS) == 3 and sum(l[0] == 'tap' for l in V.VGG16_LAYERS) == 4
