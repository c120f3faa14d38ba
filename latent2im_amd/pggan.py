"""BASELINE config 1 on the product side: the in-repo PGGAN-256 generator and the PGGAN graph's z-space walk training step on the l2i HIP
kernels.  Same class / method names, argument meaning and error behaviour as the reference:

    graphs/pggan/model_256.py:53-150,188-259     EqualConv2d / PixelNorm / ConvBlock / Generator(code_dim=511, n_label=1)
    graphs/pggan/pggan_256.py:11-51              PGGAN holder (netG / netD)
    graphs/pggan/transform_base.py:86-102        WalkLinearZ_free
    graphs/pggan/transform_base.py:167-188       WalkMlpZ3 (the default walk: every --walk_type but 'linear')
    graphs/pggan/transform_base.py:211-510       TransformGraph (get_logits with the bilinear halving, get_z_new_tensor, get_reg_preds,
                                                 the clamp pair get_alphas, the [B,1,C] x [B,C] broadcast of get_reg_loss, the `or`
                                                 loss-weight rule of optimizeParametersAll), :596-640 apply_alpha
    graphs/transform_graph_scene.py:5-125        SceneGraph / faceGraph built over this base

What the shipped reference does differently, and what is kept: its constructor loads the generator from torch.hub
(``facebookresearch/pytorch_GAN_zoo``, :554-566 — un-vendored, needs the network) and leaves the in-repo ``pggan_256.PGGAN`` commented out
(:219-220); config 1 names the in-repo generator, so that is what is built here.  ``model_256.Generator`` takes a 511-d code plus a 1-d label
embedding while ``constants.DIM_Z`` is 512: like the oracle and the fixture generator (tests/golden/make_golden.py::gen_pggan), ``netG`` uses
the first 511 columns of z.  ``model_256.Discriminator.forward`` returns a tuple, on which the reference's ``BCE_loss_logits`` raises: the GAN
term therefore raises here too and config 1 runs with ``--no_gan_loss``.

Arithmetic restructured for the hardware, same function: the 4x4 "conv" of a 1x1 map is one GEMM; every 3x3 conv is a frozen-weight
FrozenConv2d (Winograd / implicit-GEMM MFMA kernels) with the bias in its epilogue; PixelNorm + LeakyReLU is one fused pass
(l2i_pixelnorm_act_f32); with the graph's ``alpha = 0`` the last progression block is multiplied by zero (model_256.py:249-251) and is not
evaluated; ``to_rgb`` (1x1) is applied BEFORE the nearest upsample it commutes with (bit-identical values, a quarter of the work).  The
backward produces d(image)/dz only — every weight is frozen.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import constants, synth
from . import conv as C
from . import kernels as K
from .graph import ContentLoss  # noqa: F401  (graphs/pggan/transform_base.py re-exports it from here)
from .graph import (FaceTransform, SceneTransform, WalkGraph, _attach_loss_scaler, _checkpoint_or_synthetic, _make_graph, _regressor_state,
                    _to_numpy_state, _vgg19_state)
from .perceptual import VGG19Prefix
from .regressor import ResNet50

PG_CHANNELS = ((512, 512), (512, 512), (512, 512), (512, 512), (512, 256), (256, 128), (128, 64), (64, 32), (32, 16))   # model_256.py:208-216


def _t(a, device):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).contiguous().to(device)


class _EqualConv:
    """EqualConv2d (model_256.py:53-68,96-104): weight_orig * sqrt(2 / fan_in), plain bias; frozen."""

    def __init__(self, P, name, padding, device):
        w = torch.as_tensor(np.asarray(P[name + '.conv.weight_orig']), dtype=torch.float32)
        fan_in = w.shape[1] * w.shape[2] * w.shape[3]
        self.conv = C.FrozenConv2d(w * math.sqrt(2.0 / fan_in), stride=1, padding=padding, device=device)
        self.bias = _t(P[name + '.conv.bias'], device)


class Generator:
    """Frozen ``model_256.Generator(511, 1)``.  ``netG(z511, step=6, alpha=0)`` -> [B, 3, 4 * 2**step, 4 * 2**step]."""

    def __init__(self, state, device='cuda'):
        P = state
        self.device = device
        self.label = _t(P['label_embed.weight'], device)[0:1]                     # label 0 for every sample (model_256.py:232-234)
        self.code_dim = 512 - self.label.shape[1]
        w0 = torch.as_tensor(np.asarray(P['progression.0.conv.0.conv.weight_orig']), dtype=torch.float32)       # [512, 512, 4, 4]
        w0 = w0 * math.sqrt(2.0 / (w0.shape[1] * 16))
        # 4x4 kernel, padding 3, on a 1x1 map: out[b, co, y, x] = sum_ci in[b, ci] * w[co, ci, 3 - y, 3 - x] -> one [512] x [512, 512*16] GEMM
        self.w0 = torch.flip(w0, [2, 3]).permute(1, 0, 2, 3).reshape(w0.shape[1], -1).contiguous().to(device)
        self.b0 = _t(P['progression.0.conv.0.conv.bias'], device)
        self.n_blocks = len(PG_CHANNELS)
        self.convs = []
        for i in range(self.n_blocks):
            first = None if i == 0 else _EqualConv(P, 'progression.%d.conv.0' % i, 1, device)
            self.convs.append((first, _EqualConv(P, 'progression.%d.conv.3' % i, 1, device)))
        self.rgb = [(C.FrozenConv2d(np.asarray(P['to_rgb.%d.weight' % i]), 1, 0, device=device), _t(P['to_rgb.%d.bias' % i], device))
                    for i in range(self.n_blocks)]

    def __call__(self, input, label=None, step=6, alpha=0):
        if not 0 <= step < self.n_blocks:
            raise IndexError('step %r outside the %d progression blocks' % (step, self.n_blocks))
        if input.shape[1] != self.code_dim:
            raise RuntimeError('model_256.Generator(%d, %d) takes a %d-d code, got %d' % (self.code_dim, self.label.shape[1], self.code_dim, input.shape[1]))
        return _PGFn.apply(input, self, int(step), float(alpha))

    def eval(self):
        return self


class _PGFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gen, step, alpha):
        keep = z.requires_grad
        zc = z.detach().contiguous()
        B = zc.shape[0]
        code = K.pixelnorm_act(zc, slope=1.0)                                       # code_norm (model_256.py:230)
        x = torch.cat([code, gen.label.expand(B, -1)], 1)
        saved = []
        blend = step > 0 and 0 <= alpha < 1                                        # (1 - alpha) * to_rgb[step-1](upsampled) + alpha * to_rgb[step](block)
        last = step - 1 if (blend and alpha == 0) else step                       # alpha = 0: the last block is multiplied by zero
        out = None
        for i in range(last + 1):
            if i == 0:
                a1 = torch.addmm(gen.b0.repeat_interleave(16), x, gen.w0).reshape(B, -1, 4, 4)
            else:
                a1 = gen.convs[i][0].conv.forward(K.upsample2x_nearest(out), bias=gen.convs[i][0].bias)
            h1 = K.pixelnorm_act(a1, slope=0.2)
            a2 = gen.convs[i][1].conv.forward(h1, bias=gen.convs[i][1].bias)
            prev, out = out, K.pixelnorm_act(a2, slope=0.2)
            saved.append((a1 if keep else None, a2 if keep else None))
        if not blend:
            img = gen.rgb[step][0].forward(out, bias=gen.rgb[step][1])
        elif alpha == 0:
            img = K.upsample2x_nearest(gen.rgb[step - 1][0].forward(out, bias=gen.rgb[step - 1][1]))     # to_rgb commutes with the nearest upsample
        else:
            skip = K.upsample2x_nearest(gen.rgb[step - 1][0].forward(prev, bias=gen.rgb[step - 1][1]))
            img = gen.rgb[step][0].forward(out, bias=gen.rgb[step][1])
            img = K.axpby(skip, img, 1.0 - alpha, alpha)
        ctx.gen, ctx.step, ctx.alpha, ctx.blend, ctx.last = gen, step, alpha, blend, last
        ctx.saved = saved if keep else None
        ctx.zc = zc if keep else None
        return img

    @staticmethod
    def backward(ctx, g_img):
        gen, step, alpha, saved = ctx.gen, ctx.step, ctx.alpha, ctx.saved
        if saved is None:
            raise RuntimeError('the generator was run without a differentiable latent')
        g_img = g_img.contiguous()
        B = g_img.shape[0]
        g_prev = None                                                               # gradient reaching block `last - 1`'s output through the skip branch
        if not ctx.blend:
            g = gen.rgb[step][0].dgrad(g_img, saved[-1][1].shape[2:])
        elif alpha == 0:
            g = gen.rgb[step - 1][0].dgrad(K.pool2x2(g_img, 1.0), saved[-1][1].shape[2:])
        else:
            g = gen.rgb[step][0].dgrad(K.axpby(g_img, None, alpha, 0.0), saved[-1][1].shape[2:])
            g_prev = gen.rgb[step - 1][0].dgrad(K.pool2x2(g_img, 1.0 - alpha), saved[-2][1].shape[2:])
        for i in range(ctx.last, -1, -1):
            a1, a2 = saved[i]
            g = K.pixelnorm_act_bwd(g, a2, slope=0.2)
            g = gen.convs[i][1].conv.dgrad(g, a1.shape[2:])
            g = K.pixelnorm_act_bwd(g, a1, slope=0.2)
            if i == 0:
                g_x = torch.mm(g.reshape(B, -1), gen.w0.t())                        # [B, 512]: code (511) | label embedding (frozen)
                break
            g_up = gen.convs[i][0].conv.dgrad(g, (a1.shape[2], a1.shape[3]))
            g = K.pool2x2(g_up, 1.0)                                                # adjoint of the nearest upsample
            if g_prev is not None and i == ctx.last:
                g = K.axpby(g, g_prev, 1.0, 1.0)
        g_z = K.pixelnorm_act_bwd(g_x[:, :gen.code_dim].contiguous(), ctx.zc, slope=1.0)
        ctx.saved = ctx.zc = None
        return g_z, None, None, None


class PGGAN:
    """Attribute contract of pggan_256.PGGAN (pggan_256.py:11-30): ``netG`` / ``netD``.  ``netD`` is None: the graph's GAN term cannot be
    evaluated on the in-repo discriminator (see the module docstring)."""

    def __init__(self, netG, netD=None):
        self.netG, self.netD = netG, netD


class WalkLinearZ_free(nn.Module):
    """Input-dependent linear walk in z (transform_base.py:86-102): z + alpha * z * w, w [n_attr, dim_z] ~ N(0, 0.02) from the global numpy RNG."""

    def __init__(self, dim_z, step, Nsliders, attrList):
        super().__init__()
        self.dim_z = dim_z
        self.step = step
        self.Nsliders = Nsliders
        self.w = nn.Parameter(torch.Tensor(np.random.normal(0.0, 0.02, [len(attrList), self.dim_z])))

    def forward(self, input, alpha, layers=None, name=None, index_=None):
        al = alpha.to(self.w.device)
        direction = al * input * self.w
        return input + direction


WalkLinearZ_free.__module__ = 'graphs.pggan.transform_base'            # pickles resolve in the reference's vis_w.py


class _WalkMlpFn(torch.autograd.Function):
    """z + alpha * L3(lrelu(L2(lrelu(L1(z))))) on l2i_linear_rows_f32 / _bwd_f32 (csrc/l2i_walk.hip): three launches forward, one pass per layer
    backward.  Kept for the backward: z, h1, h2 (and a reference to alpha, an input); nothing when no input requires a gradient."""

    @staticmethod
    def forward(ctx, keep, z, alpha, w1, b1, w2, b2, w3, b3):
        zc, a = z.detach().contiguous(), alpha.detach().reshape(-1).contiguous()
        P = [t.detach().contiguous() for t in (w1, b1, w2, b2, w3, b3)]
        h1 = K.linear_rows(zc, P[0], P[1], K.LINEAR_LRELU, 0.2)
        h2 = K.linear_rows(h1, P[2], P[3], K.LINEAR_LRELU, 0.2)
        z_new = K.linear_rows(h2, P[4], P[5], K.LINEAR_WALK, res=zc, a=a)
        if keep and any(ctx.needs_input_grad):                  # keep = the caller's grad mode (needs_input_grad is set under no_grad too)
            ctx.save_for_backward(zc, h1, h2)
            ctx.alpha, ctx.weights = a, (P[0], P[2], P[4])
        return z_new

    @staticmethod
    def backward(ctx, g):
        z, h1, h2 = ctx.saved_tensors
        w1, w2, w3 = ctx.weights
        g = g.contiguous()
        gw3, gb3, g2 = K.linear_rows_bwd(g, h2, w3, K.LINEAR_WALK, a=ctx.alpha)
        gw2, gb2, g1 = K.linear_rows_bwd(g2, h1, w2, K.LINEAR_LRELU, 0.2, y=h2)
        want_z = ctx.needs_input_grad[1]
        gw1, gb1, gz = K.linear_rows_bwd(g1, z, w1, K.LINEAR_LRELU, 0.2, y=h1, want_gx=want_z, gx_add=g if want_z else None)
        return None, gz, None, gw1, gb1, gw2, gb2, gw3, gb3


class WalkMlpZ3(nn.Module):
    """The PGGAN graph's MLP walk (transform_base.py:167-188): z + alpha * MLP(z), MLP = dim_z -> 2 dim_z -> 2 dim_z -> dim_z with LeakyReLU(0.2).
    ``self.linear`` is the reference's nn.Sequential, so default init, parameter order and state_dict keys (linear.0.weight ... linear.4.bias)
    are the reference's; its modules are never called — forward runs one autograd.Function over the six parameters on the HIP kernels, in fp32
    on every --precision.  ``alpha`` [B, 1] gets no gradient (it never requires one on this path: the Function returns None for it)."""

    def __init__(self, dim_z, step, Nsliders, attrList):
        super().__init__()
        self.dim_z = dim_z
        self.step = step
        self.Nsliders = Nsliders
        self.linear = nn.Sequential(*[nn.Linear(self.dim_z, self.dim_z * 2), nn.LeakyReLU(0.2, True), nn.Linear(self.dim_z * 2, self.dim_z * 2),
                                      nn.LeakyReLU(0.2, True), nn.Linear(self.dim_z * 2, self.dim_z)])

    def forward(self, input, alpha, layers=None, name=None, index_=None):
        z = input.unsqueeze(0) if input.dim() == 1 else input              # a 1-D z is one sample: [1, dim_z] comes back, as broadcasting gives
        dev = self.linear[0].weight.device
        al = alpha.to(device=dev, dtype=torch.float32)
        if al.dim() == 1:
            al = al.unsqueeze(0)
        if al.dim() != 2 or al.shape[1] != 1 or al.shape[0] not in (1, z.shape[0]):
            # the reference's `al * out2` broadcasts [B, C] against [B, dim_z] and raises for every C but 1 (and dim_z, which no driver builds:
            # the kernels take one alpha per row)
            raise RuntimeError('WalkMlpZ3: alpha of shape %s against the walk direction of shape %s: alpha is one value per row, [B, 1]'
                               % (tuple(alpha.shape), tuple(z.shape)))
        if al.shape[0] != z.shape[0]:
            al = al.expand(z.shape[0], 1)
        lin = self.linear
        return _WalkMlpFn.apply(torch.is_grad_enabled(), z.to(torch.float32), al, lin[0].weight, lin[0].bias, lin[2].weight, lin[2].bias, lin[4].weight, lin[4].bias)


WalkMlpZ3.__module__ = 'graphs.pggan.transform_base'


def load_networks(device, need_vgg=True):
    """Frozen nets of the PGGAN graph.  The reference hard-codes private checkpoint paths (transform_base.py:536-538, 578-582): a configured
    path that does not exist is an error unless synthetic weights were requested explicitly (graph._checkpoint_or_synthetic)."""
    src = {}
    if _checkpoint_or_synthetic('PGGAN generator (pg_path)', constants.pg_path):
        ckpt = torch.load(constants.pg_path, map_location='cpu')['G']
        g_state = _to_numpy_state({k[7:] if k.startswith('module.') else k: v for k, v in ckpt.items()})           # transform_base.py:586-590
        src['G'] = constants.pg_path
    else:
        g_state = synth.pggan_generator_state(seed=constants.SYNTH_SEED_G)
        src['G'] = 'synthetic(seed=%d)' % constants.SYNTH_SEED_G
    r_state = _regressor_state(src)
    v_state = _vgg19_state(src) if need_vgg else None
    if C.PRECISION in C.H8_PRECISIONS:                                  # the 16-bit path: h8 feature maps, 16-bit MFMA with fp32 accumulation (nets16.py)
        from . import nets16
        GenCls, RegCls, VggCls = nets16.PGGenerator, nets16.ResNet50, nets16.VGG19Prefix
    else:
        GenCls, RegCls, VggCls = Generator, ResNet50, VGG19Prefix
    src['precision'] = C.PRECISION
    vgg = VggCls(v_state, device=device) if need_vgg else None
    nets = GenCls(g_state, device=device), RegCls(r_state, device=device), vgg
    if C.PRECISION == 'f16':
        _attach_loss_scaler(nets, nets16.pggan_scale_for, constants.PG_RESOLUTION, device, src)
    return nets + (src,)


class TransformGraph(WalkGraph):
    def __init__(self, lr, walk_type, nsliders, loss_type, eps, N_f, trainEmbed, attrList, attrTable, layers, pgan_opts=None, nets=None,
                 id_weight=0.0, facenet_ckpt=None, attr_keep=0.0, attr_keep_attrs=None):
        if id_weight:
            raise NotImplementedError('id_loss: the identity term is built for the StyleGAN2 graph (graph.TransformGraph); the PGGAN graph has none')
        WalkGraph.__init__(self, lr, nsliders, loss_type, trainEmbed)
        if nets is None:
            nets = load_networks(self.device)
        netG, self.regressor, self.vgg19, self.weight_sources = nets
        self.module = PGGAN(netG, None)
        self.img_size = constants.PG_RESOLUTION
        self.step = 6                                           # PGAN 256 (transform_base.py:244-246)
        self.alpha = 0
        if not attrTable:                                        # transform_base.py:248-256
            from .hostutil import SCENE_DEFAULT_TABLE
            from collections import OrderedDict
            self.attrTable = OrderedDict(SCENE_DEFAULT_TABLE)
        else:
            self.attrTable = attrTable
        self.attrList = attrList
        self.attrIdx = self.get_attr_idx()
        self._init_attr_keep(attr_keep, attr_keep_attrs)
        if walk_type == 'linear':
            self.walk = WalkLinearZ_free(self.dim_z, self.step, nsliders, self.attrList).to(self.device)
        else:                                                    # "MLP" (transform_base.py:270-275): every other walk type
            self.walk = WalkMlpZ3(self.dim_z, self.step, nsliders, self.attrList).to(self.device)
        self._make_optimizer(netG)
        self.walk_type = walk_type
        self.N_f = N_f
        self.eps = eps

    def get_logits(self, inputs_dict, reshape=True):
        """netG(z) then F.upsample(size=half, mode='bilinear') (:308-321) = the mean of every 2x2 window."""
        z = inputs_dict['z']
        outputs_orig = self.module.netG(z[:, :self.module.netG.code_dim], step=self.step, alpha=self.alpha)
        return _Half.apply(outputs_orig)

    def get_z_new_tensor(self, z, alpha, name=None, trainEmbed=False, index_=None, layers=None):
        return self.walk(z.squeeze(), alpha, name=name, index_=index_)

    def get_alphas(self, alpha_org, alpha_delta):
        """(clamped target, new delta) (:358-364) — the pair train_multi_attr.py:113 unpacks."""
        alpha_target = torch.clamp(alpha_org + alpha_delta, min=0, max=1)
        return alpha_target, alpha_target - alpha_org

    def get_reg_loss(self, feed_dict):
        """:366-380 — preds[:, attrIdx].unsqueeze(1) is [B,1,C] against alpha [B,C]: the BCE broadcasts to [B,B,C] before the mean (kept)."""
        logit = feed_dict['logit']
        alpha_gt = feed_dict['alpha'].to(torch.double)
        preds = self.regressor(logit).index_select(1, self._attr_columns())
        preds = preds.unsqueeze(1).to(torch.double)
        return self.get_bce_loss(preds, alpha_gt).mean()

    def get_reg_keep_loss(self, feed_dict):
        """--attr_keep: (reg, attr_keep * keep, keep).  The edited image's pooled features are computed once: ``get_reg_loss``'s expression on the
        regressor's own addmm of them, and the kept outputs through l2i_reg_bce_keep_f32 without its BCE part (one launch)."""
        reg = self.regressor
        alpha_gt = feed_dict['alpha'].to(torch.double)
        feat1 = reg.features(feed_dict['logit'])
        preds = torch.addmm(reg.fc_b, feat1, reg.fc_w.t()).index_select(1, self._attr_columns())
        preds = preds.unsqueeze(1).to(torch.double)
        keep_total, _, keep_loss = self.get_keep_loss(feed_dict['org'], feat1)
        return self.get_bce_loss(preds, alpha_gt).mean(), keep_total, keep_loss

    def get_content_loss(self, org_img, shifted_img):
        losses = self.vgg19.content_losses(org_img, shifted_img)
        return [losses[i] for i in range(4)]

    def get_w_loss(self, feed_dict, no_content_loss=False, no_gan_loss=False):
        """Total loss of optimizeParametersAll (:473-504) without the optimiser step; note the `or` in the weight rule (:496-499)."""
        if not no_gan_loss:
            raise TypeError("the PGGAN graph's GAN term needs the torch.hub discriminator (transform_base.py:476): model_256.Discriminator "
                            'returns a tuple, on which BCEWithLogitsLoss raises in the reference too — run config 1 with --no_gan_loss')
        content_losses = None
        if not no_content_loss:
            content_loss_list = self.get_content_loss(feed_dict['org'], feed_dict['logit'])
            content_losses = sum(content_loss_list) / len(content_loss_list)
        keep_loss = None
        if self.attr_keep:
            reg_loss, keep_total, keep_loss = self.get_reg_keep_loss(feed_dict)
        else:
            reg_loss = self.get_reg_loss(feed_dict)
        loss = reg_loss if (no_content_loss or no_gan_loss) else 10 * reg_loss
        if not no_content_loss:
            loss = loss + 0.05 * content_losses
        if keep_loss is not None:
            loss = loss + keep_total
        self.last_terms = dict(reg=reg_loss.detach(), cont=None if content_losses is None else content_losses.detach(), gan=None,
                               keep=None if keep_loss is None else keep_loss.detach())
        return loss

    def _probe_step(self, z, alpha, no_content_loss=False, **ignored):
        """calibrate_scales' probe: walk_forward_backward.  The GAN term cannot be evaluated here, so the D exponent, which has no tags, keeps its
        start; ``clamp`` / ``layers`` are the StyleGAN2 graph's and are ignored."""
        walk_forward_backward(self, z, alpha, no_content_loss=no_content_loss, no_gan_loss=True)

    def eager_step(self, zs_batch, alpha_delta, *, clamp=True, layers=None, no_content_loss=False, no_gan_loss=True, trainEmbed=False, updateGAN=False):
        """walk_training_step -> (loss, original images, edited images).  The walk in z always clamps and has no ``layers``."""
        loss, out_zs, transformed_output, _, _ = walk_training_step(self, torch.Tensor(zs_batch).to(self.device), alpha_delta,
                                                                    no_content_loss=no_content_loss, no_gan_loss=no_gan_loss)
        return loss, out_zs, transformed_output

    def captured_step(self, batch, n_attr, *, clamp=True, layers=None, no_content_loss=False, no_gan_loss=True):
        """The step as a hipGraph for ``batch`` samples a replay (capture.CapturedZStep): what trainer.train_step asks for under --hip_graph.
        None with the GAN term on: that step raises (get_w_loss), and it does so on the eager route."""
        from . import capture
        return capture.CapturedZStep(self, batch, n_attr, no_content_loss=no_content_loss) if no_gan_loss else None

    def clip_ims(self, ims):
        return np.uint8(np.clip(((ims + 1) / 2.0) * 256, 0, 255))              # 256, not 255: transform_base.py:595

    def apply_alpha(self, graph_inputs, alpha_to_graph, layers=None, name=None, trainEmbed=False, index_=None, given_w=None):
        """:600-640: (edited image, alpha_org); alpha_delta = alpha_to_graph - alpha_org."""
        with torch.no_grad():
            zs_batch = graph_inputs['z']
            if not torch.is_tensor(zs_batch):
                zs_batch = torch.Tensor(zs_batch).to(self.device)
            out_zs = self.get_logits({'z': zs_batch})
            alpha_to_graph = torch.tensor(np.asarray(alpha_to_graph)).float().to(self.device)
            alpha_org = self.get_reg_preds(out_zs)
            alpha_delta = alpha_to_graph - alpha_org
            z_new = self.get_z_new_tensor(zs_batch, alpha_delta, name, trainEmbed=trainEmbed, index_=index_)
            best_im_out = self.get_logits({'z': z_new})
        return best_im_out, alpha_org

    def vis_multi_image_batch_alphas(self, graph_inputs, filename, alphas_to_graph, alphas_to_target, batch_start, layers=None, name=None,
                                     wgt=False, wmask=False, trainEmbed=False, computeL2=False, given_w=None, index_=None):
        """:714-760: one PNG strip per sample, one panel per requested alpha (``np.uint8(clip((x + 1) / 2 * 255))`` like the reference's
        loop, which does not use clip_ims here); file name ``<filename>_sample<i>[_wgt][_wmask].png``.  Returns the written paths."""
        from PIL import Image
        zs_batch = np.asarray(graph_inputs['z'])
        ims_transformed = []
        for ag in alphas_to_graph:
            best_im_out, alpha_org = self.apply_alpha({'z': torch.Tensor(zs_batch).to(self.device)}, ag, name=name, layers=layers,
                                                      trainEmbed=trainEmbed, given_w=given_w, index_=0)
            x = best_im_out.detach().cpu().numpy()
            ims_transformed.append(np.uint8(np.clip(((x + 1) / 2.0) * 255, 0, 255)))
        written = []
        for ii in range(zs_batch.shape[0]):
            strip = np.concatenate([x[ii].transpose(1, 2, 0) for x in ims_transformed], axis=1)
            path = filename + '_sample{}'.format(ii + batch_start) + ('_wgt' if wgt else '') + ('_wmask' if wmask else '') + '.png'
            Image.fromarray(strip).save(path)
            written.append(path)
        return written


def walk_forward_backward(graph, z, alpha_delta, no_content_loss=False, no_gan_loss=True):
    """The z-walk step up to the walk gradient, on DEVICE inputs and without a host synchronisation (capture.CapturedZStep records exactly this
    call): the no-grad first pass, the clamp pair, the walk, the second generator pass, zero_grad, loss and backward.  Leaves d loss / d walk
    in the walk's ``.grad``.  Returns (loss, x0, x1, alpha_org, alpha_target)."""
    with torch.no_grad():
        out_zs = graph.get_logits({'z': z})
        alpha_org = graph.get_reg_preds(out_zs, keep_feats=True)
    alpha_target, alpha_delta_new = graph.get_alphas(alpha_org, alpha_delta)
    z_new = graph.get_z_new_tensor(z, alpha_delta_new)
    transformed_output = graph.get_logits({'z': z_new})
    feed_dict = {'z': z_new, 'org': out_zs, 'logit': transformed_output, 'alpha': alpha_target}
    graph.optimizer.zero_grad()
    loss = graph.get_w_loss(feed_dict, no_content_loss, no_gan_loss)
    loss.backward()
    return loss, out_zs, transformed_output, alpha_org, alpha_target


def walk_update(graph):
    """The tail of the step: WalkGraph.walk_update (all-reduce of the walk gradient, optimiser step)."""
    graph.walk_update()


def walk_training_step(graph, zs_batch, alpha_delta, no_content_loss=False, no_gan_loss=True):
    """One z-walk training step in the order of train_multi_attr.py:93-140 on the PGGAN graph's own methods.  (The shipped drivers call
    ``get_w`` / ``get_w_new_tensor``, which only the StyleGAN2 graph has; the PGGAN graph is driven method by method — this is that
    sequence, the graph's ``eager_step``.)  walk_forward_backward + walk_update: the two parts the captured step (capture.CapturedZStep)
    replays and runs.  Returns (loss, x0, x1, alpha_org, alpha_target)."""
    z = zs_batch if torch.is_tensor(zs_batch) else torch.Tensor(zs_batch).to(graph.device)
    ad = alpha_delta if torch.is_tensor(alpha_delta) else torch.tensor(np.asarray(alpha_delta)).float().to(graph.device)
    r = walk_forward_backward(graph, z, ad, no_content_loss=no_content_loss, no_gan_loss=no_gan_loss)
    graph.walk_update()
    return r


class _Half(torch.autograd.Function):
    """F.upsample(x, size=(H // 2, W // 2), mode='bilinear') for even H, W (align_corners=False): the 2x2 mean; backward = 0.25 * nearest."""

    @staticmethod
    def forward(ctx, x):
        return K.pool2x2(x.detach(), 0.25)

    @staticmethod
    def backward(ctx, g):
        return K.upsample2x_nearest(g.contiguous(), 0.25)


class PixelTransform(TransformGraph):
    """transform_base.py: the graph the plugin classes are built over."""


SceneGraph = _make_graph('SceneGraph', SceneTransform, PixelTransform, 'PG_RESOLUTION')
faceGraph = _make_graph('faceGraph', FaceTransform, PixelTransform, 'PG_RESOLUTION')
