"""tests/inversion_ref.py with the STORAGE ROUNDING of the 16-bit inversion path restated in float64, the way oracle/nets16.py restates it for
ResNet-50 (``q``): every sum stays float64, the values are rounded to the element type where the GPU stores them, and the rounding is a
straight-through estimator for autograd, so the gradient is the exact gradient of the piecewise-linear network whose ReLU / max-pool masks come from
the ROUNDED maps.  tests/test_inversion16_gpu.py holds perceptual16.Vgg16Gram16 and invert.Inverter (16-bit networks) to it.

What is rounded (latent2im_amd/perceptual16.py, nets16.py):
  VGG-16     the image where conv1_1 reads it, the ten conv weights, every conv output after its bias (the pre-ReLU map the GPU stores; the pooled
             maps are maxima of stored values and need no rounding of their own).  Biases, Grams, D and the loss are fp32 on the GPU: not rounded.
  generator  the constant input, the per-sample modulated weights (weight * style; the demodulation factor is an fp32 output scale, formed from the
             unrounded weights), the transposed conv's output in front of the blur, every styled conv's output after noise, bias and leaky ReLU.
             The ToRGB convs and the skip image are fp32.
``Rounding(dt, perturb, gradq, seed)``: ``perturb`` = relative Gaussian noise on a value before it is rounded (1e-7: an fp32 summation-order
difference), ``gradq`` = the gradient with respect to every stored map is rounded to the element type too (the GPU's gradient maps are h8).
``log2``: the static exponents under which fp16 gradient maps are rounded (nets16.invert_scale_for; unscaled they leave fp16's range).
``dt=None`` rounds nothing: the exact model of tests/inversion_ref.py.

``measure(run, dt)``: the model's own spread — three runs with perturb = 1e-7 and gradq against the unperturbed, unrounded-gradient run, the largest
deviation per quantity — beside the gradq-only deviation and the distance to the exact float64 model.  The GPU is allowed max(2 x spread, gradq-only).
"""
import math

import torch
import torch.nn.functional as F

from oracle import sg2
from tests import inversion_ref as IR

TORCH = {'f16': torch.float16, 'bf16': torch.bfloat16}
PERTURB = 1e-7
SPREAD_RUNS = 3
SPREAD_CAP = dict(one_minus_cos=5e-3, loss_rel=1e-3)      # what the model's own spread has to pass: beyond it the inputs are ill-conditioned


class _GradQ(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, T, scale):
        ctx.T, ctx.scale = T, scale
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (g * ctx.scale).float().to(ctx.T).to(g.dtype) / ctx.scale, None, None


class Rounding:
    def __init__(self, dt=None, perturb=0.0, gradq=False, seed=0, log2=None):
        self.T = TORCH[dt] if dt else None
        self.perturb, self.gradq = perturb, gradq
        self.log2 = dict(log2 or {})          # fp16: the static gradient scales of the branches ('P', 'G'), under which the GPU rounds its gradient maps
        self.gen = torch.Generator().manual_seed(1000 + seed)

    def _round(self, v):
        return v.float().to(self.T).to(v.dtype)

    def w(self, t):
        """A weight or an input: rounded, straight-through, never perturbed (the GPU rounds it from an exact fp32 value)."""
        if self.T is None:
            return t
        return t + (self._round(t.detach()) - t.detach())

    def q(self, t, branch):
        """A stored map of branch 'P' (VGG-16) or 'G' (generator): the GPU rounds its fp32 accumulator, whose low bits depend on the summation order."""
        if self.T is None:
            return t
        v = t.detach()
        if self.perturb:
            v = v * (1.0 + self.perturb * torch.randn(v.shape, generator=self.gen, dtype=v.dtype))
        out = t + (self._round(v) - t.detach())
        return _GradQ.apply(out, self.T, 2.0 ** self.log2.get(branch, 0)) if self.gradq else out


def vgg16_taps(PV, img, R):
    x, taps = R.w(img), []
    for i in range(23):
        if i in IR.FEATURES_CONV:
            x = R.q(F.conv2d(x, R.w(PV['%d.weight' % i]), PV['%d.bias' % i], padding=1), 'P')
        elif i in IR.FEATURES_POOL:
            x = F.max_pool2d(x, 2, 2)
        else:
            x = torch.relu(x)
        if i in IR.FEATURES_TAP:
            taps.append(x)
    return taps


def perceptual_loss(PV, batch, logit, R):
    """inversion_ref.perceptual_loss on the rounded taps -> [B]."""
    p = torch.zeros(batch.shape[0], dtype=batch.dtype)
    with torch.no_grad():
        gds = [IR.gram(t) for t in vgg16_taps(PV, batch, _plain(R))]
    for gd, gl in zip(gds, [IR.gram(t) for t in vgg16_taps(PV, logit, R)]):
        p = p + torch.sum((gd - gl).pow(2), [1, 2]) * (gd.shape[1] * gd.shape[2])
    return p


def _plain(R):
    """The same element type without perturbation: the target's Grams are computed once and are the same numbers in every run."""
    out = Rounding(None)
    out.T = R.T
    return out


def styled_conv(P, prefix, x, w, noise, upsample, R):
    """sg2.styled_conv with the 16-bit path's roundings (module docstring)."""
    weight = P[prefix + '.conv.weight'][0]
    cout, cin, k, _ = weight.shape
    s = sg2.equal_linear(w, P[prefix + '.conv.modulation.weight'], P[prefix + '.conv.modulation.bias'])
    ws = weight * (1.0 / math.sqrt(cin * k * k))
    outs = []
    for b in range(x.shape[0]):
        wb = ws * s[b].reshape(1, cin, 1, 1)
        d = torch.rsqrt((wb * wb).sum([1, 2, 3]) + 1e-8)
        wq = R.w(wb)
        o = F.conv_transpose2d(x[b:b + 1], wq.transpose(0, 1), stride=2, padding=0) if upsample else F.conv2d(x[b:b + 1], wq, padding=k // 2)
        outs.append(o * d.reshape(1, cout, 1, 1))
    out = torch.cat(outs, 0)
    if upsample:
        out = sg2.upfirdn2d(R.q(out, 'G'), P[prefix + '.conv.blur.kernel'], pad=(1, 1))
    if noise is not None:
        out = out + P[prefix + '.noise.weight'] * noise
    return R.q(sg2.fused_leaky_relu(out, P[prefix + '.activate.bias']), 'G')


def generator_synthesis(P, latent, noise, R):
    """sg2.generator_synthesis with the styled convs above; ToRGB and the skip image as the oracle has them (fp32 on the GPU)."""
    b, n_latent = latent.shape[0], latent.shape[1]
    log_size = (n_latent + 2) // 2
    nz = (lambda i: None) if noise is None else (lambda i: noise[i])
    out = R.w(P['input.input']).repeat(b, 1, 1, 1)
    out = styled_conv(P, 'conv1', out, latent[:, 0], nz(0), False, R)
    skip = sg2.to_rgb(P, 'to_rgb1', out, latent[:, 1])
    i = 1
    for j in range(log_size - 2):
        out = styled_conv(P, 'convs.%d' % (2 * j), out, latent[:, i], nz(2 * j + 1), True, R)
        out = styled_conv(P, 'convs.%d' % (2 * j + 1), out, latent[:, i + 1], nz(2 * j + 2), False, R)
        skip = sg2.to_rgb(P, 'to_rgbs.%d' % j, out, latent[:, i + 2], skip)
        i += 2
    return skip


def total_loss(PG, PV, w, batch, noise, R):
    """inversion_ref.total_loss on the rounding model."""
    out = generator_synthesis(PG, w, noise, R)
    n = batch.shape[2] * batch.shape[3] * 3
    nll = torch.sum((out - batch).pow(2), [1, 2, 3]) / n
    return (nll + perceptual_loss(PV, batch, out, R).mean()).sum(), out


def adam_run(PG, PV, w0, batch, noise, n_loops, lr, R):
    w = w0.detach().clone().requires_grad_()
    opt = torch.optim.Adam([w], lr=lr, betas=(0.5, 0.9))
    curve = []
    for _ in range(n_loops):
        loss, _ = total_loss(PG, PV, w, batch, noise, R)
        opt.zero_grad()
        loss.backward()
        opt.step()
        curve.append(loss.detach().reshape(1))
    return torch.cat(curve)


def deviation(got, ref, is_loss):
    """A loss (any shape): the largest relative deviation.  A gradient: relative L2 distance and 1 - cosine."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    if is_loss:
        return dict(loss_rel=float(((got - ref).abs() / ref.abs()).max()))
    cos = float((got * ref).sum() / (got.norm() * ref.norm()))
    return dict(rel_l2=float((got - ref).norm() / ref.norm()), one_minus_cos=1.0 - cos)


def measure(run, dt, log2=None):
    """``run(R)`` -> dict name -> tensor (names starting with 'loss' are losses, the others gradients).  Returns dict(base, spread, gradq, exact):
    the unperturbed model's outputs, and per quantity and figure the spread, the gradq-only deviation and the distance to the exact float64 model."""
    base = run(Rounding(dt))
    exact = run(Rounding(None))
    gq = run(Rounding(dt, gradq=True, log2=log2))
    pert = [run(Rounding(dt, PERTURB, True, seed=k, log2=log2)) for k in range(SPREAD_RUNS)]
    out = dict(base=base, spread={}, gradq={}, exact={})
    for name, ref in base.items():
        if name == 'image':
            continue
        is_loss = name.startswith('loss')
        devs = [deviation(p[name], ref, is_loss) for p in pert]
        out['spread'][name] = {k: max(d[k] for d in devs) for k in devs[0]}
        out['gradq'][name] = deviation(gq[name], ref, is_loss)
        out['exact'][name] = deviation(ref, exact[name], is_loss)
    return out


def allowed(m, name, figure):
    """The GPU's allowance for one figure of one quantity: max(2 x spread, gradq-only), and for a loss at least 1e-3."""
    a = max(2.0 * m['spread'][name][figure], m['gradq'][name][figure])
    return max(a, 1e-3) if figure == 'loss_rel' else a
