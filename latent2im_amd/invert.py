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
gradient overflowed is skipped and the dynamic factor halves.  The eager loop has no guarded SGD, so there fp16 with 'GD' is refused; bf16 needs no
scale and takes both torch optimisers.

``capture=True`` replays the iteration from a hipGraph: forward, backward, the optimiser's update and the loss record are ONE ``graph.replay()``
with no host read (the eager iteration is 157-160 library calls from Python and bound by them).  What makes the update replayable is that the
guarded optimisers (optim.GuardedAdam, optim.GuardedSGD) keep their step counter on the device, so every precision takes them there, and fp16
takes 'GD' as well.  One graph per batch size, recorded on the first ``invert`` of that size and refilled per image (``_Replay``).
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

    def __init__(self, gen, vgg, lr=0.01, optim='Adam', n_mean_latent=4096, batch=1, capture=False):
        assert optim in ('Adam', 'GD'), optim
        self.gen, self.vgg, self.lr, self.optim = gen, vgg, lr, optim
        self.capture = bool(capture)
        self.graphs = {}                                                       # batch size -> _Replay (capture=True)
        self.dtype = getattr(gen, 'dtype', torch.float32)                      # element type of the feature maps: both networks on the same path
        if getattr(vgg, 'dtype', torch.float32) != self.dtype:
            raise ValueError('generator maps are %s, VGG-16 maps %s: build both networks for one precision' % (self.dtype, getattr(vgg, 'dtype', torch.float32)))
        self.scaler = None
        if self.dtype == torch.float16:
            if optim == 'GD' and not self.capture:
                raise NotImplementedError('fp16 inversion needs an optimiser that skips an overflowed iteration; only Adam has one '
                                          '(optim.GuardedAdam): there is no guarded SGD on the eager loop.  Use --optimizer Adam, --hipgraph (capture=True), '
                                          'or --precision bf16 / f32 with GD')
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
        if self.capture:
            return self._invert_replayed(batch, grams, n_loops, noise, w)
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

    def _invert_replayed(self, batch, grams, n_loops, noise, w):
        b = batch.shape[0]
        start = self.start_latent(b) if w is None else w.detach()
        r = self.graphs.get(b)
        if r is not None and r.fixed_noise != (noise is not None):           # drawn or given noise is part of the recording
            r = None
        if r is None:
            r = self.graphs[b] = _Replay(self, batch, grams, start, noise, n_loops)
        else:
            r.load(batch, grams, start, noise)
        curve = r.run(n_loops)
        self.last_image = r.out.detach().clone() if n_loops > 0 else None      # the image of the last iteration's W+ BEFORE its update, as eager
        return r.w.detach().clone(), curve


class _Replay:
    """One inversion iteration of one batch size as a hipGraph, after capture.CapturedStep: synthesis, pixel term + VGG-16 Gram loss, backward, the
    guarded optimiser's update, ``curve[idx] = loss`` and ``idx += 1`` on ONE stream.  Static inputs, refilled per image outside the graph: the
    batch, its four target Grams, W+, the optimiser's buffers and step counter, the curve index and (when given) the noise maps; without a noise
    list the maps are drawn inside the graph from torch's graph-safe Philox stream, fresh on every replay.  The fp16 scaler is the Inverter's and
    carries over from image to image, as on the eager loop.  Recorded by capture.record."""

    MIN_CAPACITY = 1024

    def __init__(self, inv, batch, grams, start, noise, n_loops, warmup=2):
        from .capture import record
        from .optim import GuardedAdam, GuardedSGD
        self.fixed_noise = noise is not None
        self.batch = batch.clone()
        self.grams = [g.clone() for g in grams]
        self.noise = None if noise is None else [None if t is None else t.detach().float().contiguous().clone() for t in noise]
        self.w = start.clone().contiguous().requires_grad_()
        if inv.optim == 'Adam':
            self.opt = GuardedAdam([self.w], lr=inv.lr, betas=(0.5, 0.9), scaler=inv.scaler)      # BP.py:138
        else:
            self.opt = GuardedSGD([self.w], lr=inv.lr, momentum=0.9, scaler=inv.scaler)           # BP.py:140
        self.opt.init_state()                                                  # state and guard words outside the graph's pool
        self.capacity = max(int(n_loops), self.MIN_CAPACITY)
        self.curve = torch.zeros(self.capacity, dtype=torch.float32, device=batch.device)
        self.idx = torch.zeros(1, dtype=torch.int64, device=batch.device)
        self.graph, self.out, self._ws_keep = record(batch.device, lambda: self._step(inv), warmup, lambda: self.opt.zero_grad(set_to_none=True))

    def _step(self, inv):
        """Loss and backward of one iteration -> the image, detached (capture.record's rules); while recording, also the update, the curve write
        and the index increment."""
        loss, out = inv.loss(self.w, self.batch, self.grams, self.noise)
        self.w.grad = None
        loss.backward()
        if torch.cuda.is_current_stream_capturing():
            self.opt.step()
            self.curve.index_copy_(0, self.idx, loss.detach().reshape(1))
            self.idx += 1
        return out.detach()

    @torch.no_grad()
    def load(self, batch, grams, start, noise):
        """Another image into the recorded graph: every static input refilled, the optimiser back at its first step."""
        self.batch.copy_(batch)
        for dst, src in zip(self.grams, grams):
            dst.copy_(src)
        self.w.copy_(start)
        for st in self.opt.state.values():
            for t in st.values():
                t.zero_()
        if self.noise is not None:
            assert len(noise) == len(self.noise), (len(noise), len(self.noise))
            for dst, src in zip(self.noise, noise):
                if dst is not None:
                    dst.copy_(src)

    def run(self, n_loops):
        """``n_loops`` replays -> the loss curve (float64 numpy).  The curve buffer is drained every ``capacity`` replays: the only host read."""
        self.idx.zero_()
        parts, filled = [], 0
        for _ in range(n_loops):
            if filled == self.capacity:
                parts.append(self.curve.cpu())
                self.idx.zero_()
                filled = 0
            self.graph.replay()
            filled += 1
        parts.append(self.curve[:filled].cpu())
        return torch.cat(parts).numpy().astype(np.float64) if n_loops > 0 else np.zeros(0)
