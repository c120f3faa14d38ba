"""Inversion of real images into W+ (reference BP.py:99-193, Trainer): optimise a W+ latent so that the generator's image matches a given
one under a per-pixel squared error plus the VGG-16 Gram term (perceptual16.Vgg16Gram).

What differs from the reference, and why: W+ has ``gen.n_latent`` rows (BP.py:132 hard-codes 14, i.e. 256^2); the target image's Gram
matrices are computed once per image, not once per iteration (BP.py:174, 176); the loss curve stays on the device until the loop ends (BP.py:157
synchronises every iteration).  The loss is the reference's ``(nllloss + p_loss.mean()).sum()`` (BP.py:147-152) with nllloss = sum((out -
batch)^2, [1, 2, 3]) / (3 H W) per sample: for a batch of B that is sum_b nll_b + sum_b p_b, which is how it is formed here (the pixel kernel
returns the batch's sum).

The 16-bit path: ``Inverter`` takes nets16.Generator with perceptual16.Vgg16Gram16 as it takes the fp32 pair.  With fp16 elements it owns an
optim.LossScaler built from nets16.invert_scale_for and attached to both networks: the Gram branch multiplies the gradient it receives by its static
exponent times the dynamic factor and hands the image gradient on divided by the static one, the fp32 pixel term's gradient is multiplied by the
dynamic factor here, and the generator divides it out of the latent gradient.  The optimiser is then optim.GuardedAdam: an iteration whose
gradient overflowed is skipped and the dynamic factor halves.  There is no guarded SGD, so fp16 with 'GD' is refused; bf16 needs no scale and
takes both torch optimisers.
"""
import numpy as np
import torch

from . import kernels as K


class _PixelFn(torch.autograd.Function):
    """sum((out - batch)^2) / n over the whole batch as a 1-element tensor (kernels.sqdiff); the gradient is formed by the same kernel with the
    upstream gradient as its device coefficient."""

    @staticmethod
    def forward(ctx, out, batch, n, dyn=None):
        out = out.detach().contiguous()
        s, _ = K.sqdiff(batch, out)
        ctx.save_for_backward(out, batch)
        ctx.n, ctx.dyn = n, dyn
        return s / float(n)

    @staticmethod
    def backward(ctx, g):
        out, batch = ctx.saved_tensors
        if ctx.dyn is not None:                  # fp16 elements: the image gradient carries the scaler's dynamic factor (a device tensor) into the generator
            g = g * ctx.dyn
        _, grad = K.sqdiff(batch, out, coef=2.0 / float(ctx.n), coef_dev=g.contiguous(), want_grad=True, want_sum=False)
        return grad, None, None, None


class Inverter:
    """``Inverter(gen, vgg, lr, optim).invert(batch, n_loops, noise=None)`` -> (W+ [B, n_latent, 512], loss curve [n_loops])."""

    def __init__(self, gen, vgg, lr=0.01, optim='Adam', n_mean_latent=4096, batch=1):
        assert optim in ('Adam', 'GD'), optim
        self.gen, self.vgg, self.lr, self.optim = gen, vgg, lr, optim
        self.dtype = getattr(gen, 'dtype', torch.float32)                      # element type of the feature maps: both networks on the same path
        if getattr(vgg, 'dtype', torch.float32) != self.dtype:
            raise ValueError('generator maps are %s, VGG-16 maps %s: build both networks for one precision' % (self.dtype, getattr(vgg, 'dtype', torch.float32)))
        self.scaler = None
        if self.dtype == torch.float16:
            if optim == 'GD':
                raise NotImplementedError('fp16 inversion needs an optimiser that skips an overflowed iteration; only Adam has one '
                                          '(optim.GuardedAdam): there is no guarded SGD.  Use --optimizer Adam, or --precision bf16 / f32 with GD')
            from . import nets16
            from .optim import LossScaler
            self.scaler = nets16.attach_scaler((gen, vgg), LossScaler(nets16.invert_scale_for(gen.size, batch), gen.device))
        with torch.no_grad():
            self.mean_latent = gen.mean_latent(n_mean_latent)                  # [1, 512]  (BP.py:111-112)

    def start_latent(self, b):
        """The mean latent in every row of W+, per sample (BP.py:129-136)."""
        return self.mean_latent.reshape(1, 1, -1).repeat(b, self.gen.n_latent, 1).contiguous()

    def loss(self, w, batch, grams, noise=None):
        """The reference's total loss of one iteration as a 1-element tensor, and the generator's image."""
        out = self.gen.synthesis(w, noise)
        nll = _PixelFn.apply(out, batch, 3 * batch.shape[2] * batch.shape[3], None if self.scaler is None else self.scaler.dyn)     # sum_b nll_b
        p = self.vgg.loss(out, grams)                                             # [B]
        return nll + p.mean() * float(batch.shape[0]), out

    def invert(self, batch, n_loops, noise=None, w=None):
        """``noise``: a fixed list of per-layer noise maps (reproducible runs); None: fresh noise in every iteration, as the reference's
        generator call draws it (BP.py:144).  ``w``: another starting point than the mean latent."""
        batch = batch.detach().contiguous().float()
        grams = self.vgg.target_grams(batch)
        w = (self.start_latent(batch.shape[0]) if w is None else w.detach().clone().contiguous()).requires_grad_()
        if self.scaler is not None:
            from .optim import GuardedAdam
            opt = GuardedAdam([w], lr=self.lr, betas=(0.5, 0.9), scaler=self.scaler)
        elif self.optim == 'Adam':
            opt = torch.optim.Adam([w], lr=self.lr, betas=(0.5, 0.9))             # BP.py:138
        else:
            opt = torch.optim.SGD([w], lr=self.lr, momentum=0.9)                  # BP.py:140
        curve, out = [], None
        for _ in range(n_loops):
            loss, out = self.loss(w, batch, grams, noise)
            opt.zero_grad()
            loss.backward()
            opt.step()
            curve.append(loss.detach())
        self.last_image = None if out is None else out.detach()                   # the image of the last iteration's W+ BEFORE its update, as BP.py:168 saves it
        curve = torch.cat(curve).cpu().numpy().astype(np.float64) if curve else np.zeros(0)
        return w.detach(), curve
