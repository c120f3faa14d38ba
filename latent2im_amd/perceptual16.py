"""VGG-16 Gram-matrix loss of BP.py on the l2i HIP kernels.

Reference: perceptual_vgg/vgg.py:5-37 (Vgg16: torchvision ``vgg16().features[0:23]`` with taps relu1_2, relu2_2, relu3_3, relu4_3), BP.py:68-73
(gram), BP.py:173-184 (perceptual_loss: per tap sum((G_data - G_logit)^2, [1, 2]) * C^2, added over the four taps).  As in BP.py:174-175 the
network takes the generator's [-1, 1] image as it stands: no mean / std normalisation.

The ten convolutions run on ``conv.FrozenConv2d`` and the three pools on the pool kernels, with the ReLU carried as an input mask of the next
conv and an output mask of the gradient convs, exactly as perceptual.py does; the taps therefore exist only as PRE-ReLU conv outputs, and
``kernels.gram_loss`` / ``kernels.gram_bwd`` (csrc/l2i_gram.hip) apply the ReLU on load.  The reference evaluates the target image's Grams in
every iteration; here ``target_grams`` runs once per image.  The backward walks the network once: every tap's Gram gradient is ADDED by
l2i_gram_bwd_f32 into the gradient that arrives from the deeper taps.

``Vgg16Gram16`` is the same network on the 16-bit path (conv.PRECISION 'bf16' / 'f16'): every map is an h8 tensor [B, C/8, H, W, 8], conv1_1 reads the
fp32 image (conv.ImgConvH8), the other nine convs are conv.H8Conv with the ReLU on load (``relu_in``) and as the output mask of the gradient convs, the
pools are kernels16.maxpool2d_* and the Gram term is kernels16.gram_loss / gram_bwd (csrc/l2i_gram_h8.hip).  Grams, D and the loss stay fp32.  With fp16
elements the gradient that enters the backward is multiplied by the scaler's static exponent of branch 'P' (nets16.invert_scale_for) times its dynamic
factor; the fp32 image gradient leaves divided by the static one (the generator divides the dynamic one out of the latent gradient).
"""
import numpy as np
import torch

from . import conv as C
from . import kernels as K
from . import kernels16 as K16
from . import nets16
from . import vgg16_specs as V


class Vgg16Gram:
    def __init__(self, state, device='cuda'):
        self.device = device
        self.stages = []                # per tap: the convs that lead to it, each (FrozenConv2d, bias); a 2x2 max-pool sits between two stages
        stage = []
        for layer in V.VGG16_LAYERS:
            if layer[0] == 'conv':
                idx = layer[1]
                w = torch.as_tensor(np.asarray(state['%d.weight' % idx]), dtype=torch.float32)
                b = torch.as_tensor(np.asarray(state['%d.bias' % idx]), dtype=torch.float32).contiguous().to(device)
                stage.append((C.FrozenConv2d(w, 1, 1, device=device), b))
            elif layer[0] == 'tap':
                self.stages.append(stage)
                stage = []

    def _forward(self, img):
        """[B, 3, H, W] -> per stage (input map, pool indices or None, [pre-ReLU conv outputs]); the last conv output of a stage is its tap."""
        acts = []
        x, masked = img.contiguous(), False
        for si, stage in enumerate(self.stages):
            idx = None
            if si:
                x, idx = K.maxpool2d_fwd(x, 2, 2, 0)             # relu(maxpool(.)) == maxpool(relu(.)): the ReLU stays a mask
            xin, cs = x, []
            for cv, bias in stage:
                x = cv.forward(x, in_mask=x, mask=(1.0, 0.0), bias=bias) if masked else cv.forward(x, bias=bias)
                masked = True
                cs.append(x)
            acts.append((xin, idx, cs))
        return acts

    def target_grams(self, img):
        """The four Gram matrices [B, C_k, C_k] of a target image: once per image."""
        with torch.no_grad():
            return tuple(K.gram_loss(cs[-1]) for _, _, cs in self._forward(img.detach()))

    def loss(self, img, grams):
        """[B]: sum over the four taps of C^2 * sum((G_k(img) - grams[k])^2), differentiable w.r.t. ``img``."""
        return _GramLossFn.apply(img, self, tuple(grams))


class _GramLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, net, grams):
        acts = net._forward(img.detach())
        loss = torch.zeros(img.shape[0], device=img.device, dtype=torch.float32)
        diffs = []
        for (_, _, cs), gt in zip(acts, grams):
            diffs.append(K.gram_loss(cs[-1], gt, loss)[1])
        if img.requires_grad:
            ctx.net, ctx.acts, ctx.diffs, ctx.in_hw = net, acts, diffs, (img.shape[2], img.shape[3])
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        net, acts, diffs = ctx.net, ctx.acts, ctx.diffs
        g_loss = g_loss.contiguous()

        g = None                                                  # gradient w.r.t. the current stage's tap (pre-ReLU)
        for si in range(len(net.stages) - 1, -1, -1):
            xin, idx, cs = acts[si]
            if g is None:
                g = torch.empty_like(cs[-1])
                K.gram_bwd(cs[-1], diffs[si], scale=g_loss, out=g)                    # the per-sample upstream gradient stays on the device
            else:
                K.gram_bwd(cs[-1], diffs[si], scale=g_loss, out=g, accumulate=True)
            for li in range(len(cs) - 1, -1, -1):
                cv = net.stages[si][li][0]
                below = cs[li - 1] if li else xin
                if si == 0 and li == 0:
                    g = cv.dgrad(g, ctx.in_hw)                    # the image itself: no ReLU in front of the first conv
                else:
                    g = cv.dgrad(g, (below.shape[2], below.shape[3]), out_mask=below)
            if si:
                prev = acts[si - 1][2][-1]
                g = K.maxpool2d_bwd(g, idx, (prev.shape[2], prev.shape[3]), 2, 2, 0)
        ctx.acts = ctx.diffs = None
        return g, None, None


class Vgg16Gram16:
    def __init__(self, state, device='cuda'):
        self.device = device
        self.dtype = K16.h8_dtype()
        self.scaler = None              # nets16.attach_scaler: an optim.LossScaler with a 'P' exponent (fp16 elements); None = unscaled
        self.stages = []                # per tap: the convs that lead to it, each (H8Conv, bias); weights are packed here, once
        stage = []
        for layer in V.VGG16_LAYERS:
            if layer[0] == 'conv':
                idx = layer[1]
                w = torch.as_tensor(np.asarray(state['%d.weight' % idx]), dtype=torch.float32)
                b = torch.as_tensor(np.asarray(state['%d.bias' % idx]), dtype=torch.float32).contiguous().to(device)
                first = not self.stages and not stage
                if first:
                    self.conv0_img = C.ImgConvH8(w, 1, 1, device=device)       # conv1_1 forward on the fp32 image; its gradient: stages[0][0].dgrad
                stage.append((C.H8Conv(w, 1, 1, device=device, cin_pad=16 if first else 32), b))
            elif layer[0] == 'tap':
                self.stages.append(stage)
                stage = []

    def _forward(self, img):
        """[B, 3, H, W] fp32 -> per stage (input map, pool indices or None, [pre-ReLU conv outputs, h8]); the last conv output of a stage is its tap.
        A stage's input map is the image (stage 0) or the RECTIFIED pooled tap of the stage below."""
        acts = []
        x = img.contiguous()
        for si, stage in enumerate(self.stages):
            idx = None
            if si:
                x, idx = K16.maxpool2d_fwd(x, 2, 2, 0, relu=True)       # relu(maxpool(.)) == maxpool(relu(.)); the stored map is already rectified
            xin, cs = x, []
            for li, (cv, bias) in enumerate(stage):
                if si == 0 and li == 0:
                    x = self.conv0_img.forward(x, bias=bias)
                else:
                    x = cv.forward(x, relu_in=li > 0, bias=bias)
                cs.append(x)
            acts.append((xin, idx, cs))
            nets16._probe('P.fwd.tap%d' % si, x)
        return acts

    def target_grams(self, img):
        """The four Gram matrices [B, C_k, C_k] (fp32) of a target image: once per image."""
        with torch.no_grad():
            return tuple(K16.gram_loss(cs[-1]) for _, _, cs in self._forward(img.detach().float()))

    def loss(self, img, grams):
        """[B]: sum over the four taps of C^2 * sum((G_k(img) - grams[k])^2), differentiable w.r.t. the fp32 ``img``."""
        return _GramLoss16Fn.apply(img, self, tuple(grams))


class _GramLoss16Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, net, grams):
        acts = net._forward(img.detach())
        loss = torch.zeros(img.shape[0], device=img.device, dtype=torch.float32)
        diffs = []
        for (_, _, cs), gt in zip(acts, grams):
            diffs.append(K16.gram_loss(cs[-1], gt, loss)[1])
        if img.requires_grad:
            ctx.net, ctx.acts, ctx.diffs, ctx.in_hw = net, acts, diffs, (img.shape[2], img.shape[3])
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        net, acts, diffs = ctx.net, ctx.acts, ctx.diffs
        S, dyn = nets16._gs(net, 'P'), nets16._dyn(net)
        gs = (g_loss if dyn is None else g_loss * (dyn * S)).contiguous()     # static * dynamic scale (fp16 elements; exact: powers of two), per sample, on the device
        hw = lambda t: (t.shape[2], t.shape[3])
        g = None                                                  # gradient w.r.t. the current stage's tap (pre-ReLU), h8
        for si in range(len(net.stages) - 1, -1, -1):
            xin, idx, cs = acts[si]
            g = K16.gram_bwd(cs[-1], diffs[si], scale=gs, out=g, accumulate=g is not None)       # added into the gradient from the deeper taps
            nets16._probe('P.g.tap%d' % si, g)
            for li in range(len(cs) - 1, -1, -1):
                cv = net.stages[si][li][0]
                if si == 0 and li == 0:
                    g = cv.dgrad(g, ctx.in_hw, out_f32=True, out_gain=1.0 / S)      # the fp32 image: no ReLU in front of the first conv
                else:
                    below = cs[li - 1] if li else xin
                    g = cv.dgrad(g, hw(below), out_mask=below)
            if si:
                g = K16.maxpool2d_bwd(g, idx, hw(acts[si - 1][2][-1]), 2, 2, 0)
                nets16._probe('P.g.pool%d' % si, g)
        ctx.acts = ctx.diffs = None
        return g, None, None
