"""VGG-16 Gram-matrix loss of BP.py on the l2i HIP kernels.

Reference: perceptual_vgg/vgg.py:5-37 (Vgg16: torchvision ``vgg16().features[0:23]`` with taps relu1_2, relu2_2, relu3_3, relu4_3), BP.py:68-73
(gram), BP.py:173-184 (perceptual_loss: per tap sum((G_data - G_logit)^2, [1, 2]) * C^2, added over the four taps).  As in BP.py:174-175 the
network takes the generator's [-1, 1] image as it stands: no mean / std normalisation.

The ten convolutions run on ``conv.FrozenConv2d`` and the three pools on the pool kernels, with the ReLU carried as an input mask of the next
conv and an output mask of the gradient convs, exactly as perceptual.py does; the taps therefore exist only as PRE-ReLU conv outputs, and
``kernels.gram_loss`` / ``kernels.gram_bwd`` (csrc/l2i_gram.hip) apply the ReLU on load.  The reference evaluates the target image's Grams in
every iteration; here ``target_grams`` runs once per image.  The backward walks the network once: every tap's Gram gradient is ADDED by
l2i_gram_bwd_f32 into the gradient that arrives from the deeper taps.
"""
import numpy as np
import torch

from . import conv as C
from . import kernels as K
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
