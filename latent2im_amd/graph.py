"""Host-side mirror of the reference Graph API for the StyleGAN2 walk-training path.

Same class / method names, argument meaning and error behaviour as the reference so that ``train.py`` reads the same:

    graphs/__init__.py:3-22                      find_model_using_name
    graphs/transform_graph_scene.py:5-125        get_transform_graphs -> [SceneGraph, faceGraph]
    graphs/stylegan_v2_real/transform_base.py    TransformGraph (:246-549), PixelTransform (:901-903),
                                                 WalkLinearMultiW (:140-165), ContentLoss/Normalization (:44-63)
    utils/transforms.py:634-735                  FaceTransform / SceneTransform alpha samplers

Underneath, every network is the frozen HIP implementation of this package (generator.py, regressor.py, perceptual.py,
discriminator.py); nothing here runs on the CPU and nothing imports the oracle.  Differences from the reference,
all output-equivalent: frozen networks carry no autograd state (the reference keeps requires_grad=True everywhere and
back-propagates weight gradients it never uses); the first generator/regressor pass therefore builds
no graph (A.4); the VGG prefix is evaluated once per image instead of once per tap.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import constants, dist, synth
from .discriminator import Discriminator
from .generator import Generator
from .perceptual import VGG19Prefix
from .regressor import ResNet50


# ----------------------------------------------------------------------------------------------------------------
# walk modules
# ----------------------------------------------------------------------------------------------------------------
class WalkLinearMultiW(nn.Module):
    """Input-independent linear walk in W+ (transform_base.py:140-165): w_i + alpha @ W[:, i, :].
    ``self.w`` [n_attr, 2*(step+1), dim_z] ~ N(0, 0.02) from the global numpy RNG, exactly like the reference."""

    def __init__(self, dim_z, step, Nsliders, attrList):
        super().__init__()
        self.dim_z = dim_z
        self.step = step
        self.w = nn.Parameter(torch.Tensor(np.random.normal(0.0, 0.02, [len(attrList), (self.step + 1) * 2, self.dim_z])))

    def forward(self, input, alpha, layers=None, name=None, index_=None):
        al = alpha.to(self.w.device)
        dirs = torch.matmul(al, self.w.permute(1, 0, 2))                 # [n_latent, B, dim_z] in one batched GEMM
        if layers is None and len(input) == dirs.shape[0] and all(t is input[0] for t in input):
            # get_w hands the SAME tensor n_latent times (transform_base.py:372-378): one broadcast add instead of n_latent, the list entries are
            # views of its result (same values, same list-of-[B,512] contract)
            return list((input[0].unsqueeze(0) + dirs).unbind(0))
        w_transformed = []
        for i in range(len(input)):
            if layers is None or i in layers:
                w_transformed.append(input[i] + dirs[i])
            else:
                w_transformed.append(input[i])
        return w_transformed


# pickles written by save_multi_models must resolve in the reference's vis_w.py (transform_base.py:499-509)
WalkLinearMultiW.__module__ = 'graphs.stylegan_v2_real.transform_base'


class WalkMlpMultiW(nn.Module):
    """Input-dependent MLP walk in W+ (transform_base.py:168-204; "an unused setting in the paper", built only when
    ``is_mlp`` is switched on by hand): w_i + alpha[:, :1] * MLP(w_i), MLP = 512 -> 1024 -> 1024 -> 512 with LeakyReLU(0.2).
    With ``layers`` given the reference calls ``self.linear(input[i], 1)``, which raises TypeError: kept."""

    def __init__(self, dim_z, step, Nsliders, attrList):
        super().__init__()
        self.dim_z = dim_z
        self.step = step
        self.Nsliders = Nsliders
        self.linear = nn.Sequential(nn.Linear(dim_z, 2 * dim_z), nn.LeakyReLU(0.2, True),
                                    nn.Linear(2 * dim_z, 2 * dim_z), nn.LeakyReLU(0.2, True),
                                    nn.Linear(2 * dim_z, dim_z))

    def forward(self, input, alpha, layers=None, name=None, index_=None):
        al = torch.unsqueeze(alpha[:, 0], 1).to(self.linear[0].weight.device)
        if layers is None:
            same = all(t is input[0] for t in input)               # get_w hands the SAME tensor n_latent times: one MLP pass
            step0 = self.linear(input[0]) if same else None
            return [input[i] + al * (step0 if same else self.linear(input[i])) for i in range(len(input))]
        out = []
        for i in range(len(input)):
            out.append(input[i] + al * self.linear(input[i], 1) if i in layers else input[i])
        return out


class WalkNonLinearW(nn.Module):
    """MLP walk conditioned on an embedding of alpha (transform_base.py:207-243), chosen by ``--walk_type NN*``:
    e = Linear(10, 256)(alpha[:, :1] repeated 10x); d = MLP([e, w_i]); w_i + d / ||d|| (no normalisation when ``layers``
    is given).  NOTE the argument order (input, name, alpha, index_, layers): the reference's get_w_new_tensor calls every
    walk as ``walk(multi_ws, alpha=..., layers=...)`` (transform_base.py:380-386), so with this walk it raises TypeError
    (missing ``name`` / ``index_``) — the same happens here; call the module directly to use it."""

    def __init__(self, dim_z, step, Nsliders, attrList):
        super().__init__()
        self.dim_z = dim_z
        self.step = step
        self.Nsliders = Nsliders
        self.embed = nn.Linear(10, dim_z // 2)
        self.linear = nn.Sequential(nn.Linear(dim_z // 2 + dim_z, 2 * dim_z), nn.LeakyReLU(0.2, True),
                                    nn.Linear(2 * dim_z, dim_z))

    def forward(self, input, name, alpha, index_, layers=None):
        al = torch.unsqueeze(alpha[:, 0], 1).to(self.embed.weight.device)
        out = self.embed(al.repeat(1, 10))
        w_transformed = []
        for i in range(len(input)):
            if layers is None:
                out2 = self.linear(torch.cat([out, input[i]], 1))
                w_transformed.append(input[i] + out2 / torch.norm(out2, dim=1, keepdim=True))
            elif i in layers:
                w_transformed.append(input[i] + self.linear(torch.cat([out, input[i]], 1)))
            else:
                w_transformed.append(input[i])
        return w_transformed


WalkMlpMultiW.__module__ = WalkNonLinearW.__module__ = 'graphs.stylegan_v2_real.transform_base'


class ContentLoss(nn.Module):
    """transform_base.py:57-63."""

    def forward(self, org, shifted):
        self.loss = torch.nn.functional.mse_loss(org.detach(), shifted)
        return self.loss


# ----------------------------------------------------------------------------------------------------------------
# network holders
# ----------------------------------------------------------------------------------------------------------------
class StyleGAN:
    """Attribute contract of stylegan2.StyleGAN (stylegan2.py:19-31): ``netG`` / ``netD``.  The reference also builds
    ``g_running`` and two Adam optimisers that the walk path never touches (updateGAN raises, train.py:40-41)."""

    def __init__(self, netG, netD):
        self.netG, self.netD = netG, netD


def _to_numpy_state(sd):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in sd.items()}


def _checkpoint_or_synthetic(what, path):
    """True: load ``path``.  False: synthetic weights were requested explicitly.  Otherwise raise: a mistyped checkpoint path must
    not train a walk against random frozen networks without anyone noticing."""
    if path and os.path.isfile(path):
        return True
    if constants.ALLOW_SYNTHETIC_WEIGHTS:
        return False
    raise FileNotFoundError('%s checkpoint %r does not exist (graphs.stylegan_v2_real.constants); pass --synthetic_weights / set '
                            'L2I_SYNTHETIC_WEIGHTS=1 to run on seeded random-init weights of the same architecture instead' % (what, path))


def _regressor_state(src):
    """The attribute regressor's weights (both graphs' load_networks); the source goes to ``src['R']``."""
    if _checkpoint_or_synthetic('regressor (reg_path)', constants.reg_path):
        src['R'] = constants.reg_path
        return _to_numpy_state(torch.load(constants.reg_path, map_location='cpu')['model'])
    src['R'] = 'synthetic(seed=%d)' % constants.SYNTH_SEED_R
    return synth.resnet50_state(seed=constants.SYNTH_SEED_R)


def _vgg19_state(src):
    """The VGG-19 prefix's weights, torchvision's ``features.`` prefix stripped; the source goes to ``src['V']``."""
    if _checkpoint_or_synthetic('VGG-19 (vgg_path; the reference downloads torchvision weights)', constants.vgg_path):
        src['V'] = constants.vgg_path
        return {k.replace('features.', ''): v for k, v in _to_numpy_state(torch.load(constants.vgg_path, map_location='cpu')).items()}
    src['V'] = 'synthetic(seed=%d)' % constants.SYNTH_SEED_V
    return synth.vgg19_prefix_state(seed=constants.SYNTH_SEED_V)


def _attach_loss_scaler(nets, scale_for, resolution, device, src):
    """Gradient scales of the fp16 path: the static exponents ``scale_for(resolution, per-rank batch)`` (nets16.loss_scale_for /
    pggan_scale_for) — every rank's losses are means over its own shard — times one dynamic factor on the device; one scaler per graph, carried
    by its networks.  The exponents go to ``src['loss_scale_log2']``."""
    from . import nets16, optim
    per_rank = max(constants.BATCH_SIZE // dist.world_size(), 1)
    scaler = optim.LossScaler(scale_for(resolution, per_rank), device, growth_interval=constants.LOSS_SCALE_GROWTH_INTERVAL)
    nets16.attach_scaler(nets, scaler)
    src['loss_scale_log2'] = dict(scaler.log2)


def load_networks(resolution, device, need_vgg=True, need_d=True):
    """Frozen nets from the checkpoint paths of ``constants`` (reference transform_base.py:522-549).  Deterministic synthetic
    weights of the same architecture (latent2im_amd.synth) are used only on explicit request (constants.ALLOW_SYNTHETIC_WEIGHTS);
    the choice per network is returned as the last element and logged by the drivers."""
    src = {}
    if _checkpoint_or_synthetic('generator (g_path)', constants.g_path):
        g_state = _to_numpy_state(torch.load(constants.g_path, map_location='cpu')['g_ema'])
        src['G'] = constants.g_path
    else:
        g_state = synth.generator_state(resolution, seed=constants.SYNTH_SEED_G, noise_strength=constants.SYNTH_NOISE_STRENGTH)
        src['G'] = 'synthetic(seed=%d%s)' % (constants.SYNTH_SEED_G, ', noise_strength=%g' % constants.SYNTH_NOISE_STRENGTH if constants.SYNTH_NOISE_STRENGTH else '')
    r_state = _regressor_state(src)
    from . import conv
    if conv.PRECISION in conv.H8_PRECISIONS:                           # the 16-bit path (BASELINE config 5): bf16 h8 feature maps, one bf16 MFMA per MAC (nets16.py)
        from . import nets16
        GenCls, RegCls, VggCls, DCls = nets16.Generator, nets16.ResNet50, nets16.VGG19Prefix, nets16.Discriminator
    else:
        GenCls, RegCls, VggCls, DCls = Generator, ResNet50, VGG19Prefix, Discriminator
    src['precision'] = conv.PRECISION
    netG = GenCls(g_state, resolution, device=device)
    reg = RegCls(r_state, device=device)
    vgg = netD = None
    if need_vgg:
        vgg = VggCls(_vgg19_state(src), device=device)
    if need_d:
        # the reference's netD is ALWAYS freshly initialised (never loaded): seeded here for reproducibility
        netD = DCls(synth.discriminator_state(resolution, seed=constants.SYNTH_SEED_D), resolution, device=device)
        src['D'] = 'random-init(seed=%d)' % constants.SYNTH_SEED_D
    if conv.PRECISION == 'f16':
        _attach_loss_scaler((netG, netD, reg, vgg), nets16.loss_scale_for, resolution, device, src)
    return netG, netD, reg, vgg, src


def attribute_change_bucket(pred, org):
    """Bucket index per sample (transform_base.py:722-738): 0 if |pred - org| <= 0.3, 1 if <= 0.6, 2 if <= 1, else 3
    (dropped).  The comparison is made on the float32 difference against the float32 thresholds, which is what numpy does
    for ``np.abs(float32 - float32) <= 0.3`` under NumPy >= 2 (a python float is a weak scalar; NumPy 1.x promoted the
    scalar comparison to float64, which differs only for a difference that rounds exactly onto a threshold)."""
    d = np.abs(np.asarray(pred, dtype=np.float32) - np.asarray(org, dtype=np.float32))
    return np.where(d <= np.float32(0.3), 0, np.where(d <= np.float32(0.6), 1, np.where(d <= np.float32(1), 2, 3))).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------
# TransformGraph
# ----------------------------------------------------------------------------------------------------------------
class _RegBceFn(torch.autograd.Function):
    """loss = get_bce_loss(fc(feat)[:, cols], target.double()).mean() (transform_base.py:416-424), forward and d loss / d feat, one launch (l2i_reg_bce_f32)."""

    @staticmethod
    def forward(ctx, feat, fc_w, fc_b, cols, target):
        from . import _lib
        feat = feat.detach().contiguous()
        assert feat.dtype == torch.float32 and feat.is_cuda and fc_w.shape[1] == feat.shape[1] and target.dtype in (torch.float32, torch.float64)
        B, F = feat.shape
        K = int(cols.numel())
        target = target.detach().contiguous()
        assert tuple(target.shape) == (B, K), (target.shape, B, K)
        loss = torch.empty(1, dtype=torch.float64, device=feat.device)
        preds = torch.empty(B, K, dtype=torch.float32, device=feat.device)
        g = torch.empty_like(feat)
        _lib.call('l2i_reg_bce_f32', _lib.ptr(loss), _lib.fptr(preds), _lib.fptr(g), _lib.fptr(feat), _lib.fptr(fc_w), _lib.fptr(fc_b), _lib.ptr(cols),
                  _lib.ptr(target), int(target.dtype == torch.float64), B, F, K, 1e-12)
        ctx.save_for_backward(g)
        ctx.preds = preds
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        (g,) = ctx.saved_tensors
        return torch.mul(g, g_loss), None, None, None, None          # (fp32 tensor x 0-dim float64 tensor -> fp32: one launch)


class _RegBceKeepFn(torch.autograd.Function):
    """c_reg * _RegBceFn's loss on ``feat1`` + w_keep * mean_bj |fc(feat1) - fc(feat0)| over the columns ``keep_cols`` (--attr_keep), forward and
    d total / d feat1 in one launch (l2i_reg_bce_keep_f32).  ``cols`` / ``target`` None: no BCE part (the PGGAN graph, whose BCE keeps its own
    broadcast).  Returns (total, reg, keep, pkeep): three float64 scalars and the launch's read-out pkeep [B, M, 2] = (fc(feat1), fc(feat0)) at the
    kept columns; only ``total`` carries a gradient."""

    @staticmethod
    def forward(ctx, feat1, feat0, fc_w, fc_b, cols, target, keep_cols, c_reg, w_keep):
        from . import _lib
        feat1, feat0 = feat1.detach().contiguous(), feat0.detach().contiguous()
        assert feat1.dtype == feat0.dtype == torch.float32 and feat1.is_cuda and feat0.shape == feat1.shape and fc_w.shape[1] == feat1.shape[1]
        B, F = feat1.shape
        K, M = (0 if cols is None else int(cols.numel())), int(keep_cols.numel())
        preds = None
        if K:
            target = target.detach().contiguous()
            assert target.dtype in (torch.float32, torch.float64) and tuple(target.shape) == (B, K), (target.shape, B, K)
            preds = torch.empty(B, K, dtype=torch.float32, device=feat1.device)
        loss = torch.empty(3, dtype=torch.float64, device=feat1.device)
        pkeep = torch.empty(B, M, 2, dtype=torch.float32, device=feat1.device)
        g = torch.empty_like(feat1)
        _lib.call('l2i_reg_bce_keep_f32', _lib.ptr(loss), _lib.fptr(preds), _lib.fptr(pkeep), _lib.fptr(g), _lib.fptr(feat1), _lib.fptr(feat0),
                  _lib.fptr(fc_w), _lib.fptr(fc_b), _lib.ptr(cols) if K else None, _lib.ptr(target) if K else None,
                  int(K > 0 and target.dtype == torch.float64), _lib.ptr(keep_cols), B, F, K, M, float(c_reg), float(w_keep), 1e-12)
        ctx.save_for_backward(g)
        total, reg, keep = loss[2], loss[0], loss[1]
        ctx.mark_non_differentiable(reg, keep, pkeep)
        return total, reg, keep, pkeep

    @staticmethod
    def backward(ctx, g_total, g_reg, g_keep, g_pkeep):
        (g,) = ctx.saved_tensors
        return torch.mul(g, g_total), None, None, None, None, None, None, None, None          # one launch, as _RegBceFn


class WalkGraph:
    """What the StyleGAN2 graph (TransformGraph below) and the PGGAN graph (pggan.TransformGraph) share: bookkeeping, the walk's optimiser, the
    regressor read-out, the tail of the step, the fp16 calibration and the checkpoints.  A subclass builds its networks and its walk and supplies
    ``get_logits``, ``get_alphas``, ``get_reg_loss``, ``get_content_loss``, ``get_w_loss``, ``_probe_step``, ``eager_step`` and
    ``captured_step``: there the reference's two graphs differ."""

    def __init__(self, lr, nsliders, loss_type, trainEmbed):
        assert (loss_type in ['l2', 'lpips']), 'unimplemented loss'
        if not torch.cuda.is_available():
            raise RuntimeError('latent2im_amd runs on an MI355X (ROCm) device only: no GPU is visible and there is no CPU path')
        self.lr = lr
        self.useGPU = constants.useGPU
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.reg_optmizer = None
        self.dim_z = constants.DIM_Z
        self.Nsliders = nsliders
        self.num_channels = constants.NUM_CHANNELS
        self.BATCH_SIZE = constants.BATCH_SIZE
        self.BCE_loss_logits = nn.BCEWithLogitsLoss()
        self.ContentLoss = ContentLoss()
        self.trainEmbed = trainEmbed
        self.last_terms = None
        self.attr_keep, self.attr_keep_attrs, self.keepIdx = 0.0, None, None          # the attribute-preservation term: off until _init_attr_keep

    def _make_optimizer(self, netG):
        """fp16 elements (the networks carry a scaler, load_networks): Adam with GradScaler semantics on the device — a step whose gradient holds an
        inf / NaN is skipped and the dynamic loss scale halves (optim.py); every other precision: torch's own, as in the reference
        (transform_base.py:329-331)."""
        self.loss_scaler = getattr(netG, 'scaler', None)
        if self.loss_scaler is not None:
            from . import optim
            self.optimizer = optim.GuardedAdam(self.walk.parameters(), lr=self.lr, betas=(0.5, 0.99), scaler=self.loss_scaler)
        else:
            self.optimizer = torch.optim.Adam(self.walk.parameters(), lr=self.lr, betas=(0.5, 0.99))

    def get_attr_idx(self):
        return [self.attrTable[i] for i in self.attrList]

    def _attr_columns(self):
        """attrIdx as a device index tensor, built once: indexing with the python list would copy it host -> device on every call
        (a synchronous copy, and not permitted while the step is being captured into a hipGraph)."""
        t = getattr(self, '_attr_index', None)
        if t is None or t.numel() != len(self.attrIdx) or t.device != self.device:
            t = self._attr_index = torch.tensor(list(self.attrIdx), dtype=torch.long, device=self.device)
        return t

    def _init_attr_keep(self, attr_keep, attr_keep_attrs):
        """--attr_keep W [--attr_keep_attrs A,B,...]: the term W * mean_bj |regressor(edited)[b, j] - regressor(original)[b, j]| over the regressor
        outputs j the walk is NOT trained on — eval.py's attribute-preservation metric as a training term.  The kept columns: the table indices of
        ``attr_keep_attrs``, by default every regressor output that is not in attrIdx, ascending.  0 (the default): nothing is built, stashed or
        launched.  Called by the subclasses once regressor, attrTable and attrIdx exist."""
        self.attr_keep = float(attr_keep or 0.0)
        self.attr_keep_attrs = None if attr_keep_attrs is None else list(attr_keep_attrs)
        self.keepIdx, self._org_feat, self.last_keep_preds = None, None, None
        if self.attr_keep < 0 or self.attr_keep != self.attr_keep:
            raise ValueError('attr_keep takes a weight >= 0 (got %r)' % (attr_keep,))
        if self.attr_keep_attrs is not None and not self.attr_keep:
            raise ValueError('attr_keep_attrs names the attributes of the attribute-preservation term: it needs attr_keep W with W > 0')
        if not self.attr_keep:
            return
        n_out = int(self.regressor.fc_w.shape[0])
        if self.attr_keep_attrs is None:
            trained = set(self.attrIdx)
            idx = [i for i in range(n_out) if i not in trained]
        else:
            idx = []
            for name in self.attr_keep_attrs:
                if name not in self.attrTable:
                    raise ValueError('attr_keep_attrs: %r is not in the attribute table' % (name,))
                if name in self.attrList:
                    raise ValueError('attr_keep_attrs: %r is trained by this walk (attrList); it cannot be held still as well' % (name,))
                idx.append(int(self.attrTable[name]))
        if not idx:
            raise ValueError('attr_keep: no regressor output is left to hold still (all %d are in attrList)' % n_out)
        if len(idx) > 64 or len(self.attrIdx) > 64:
            raise ValueError('attr_keep: l2i_reg_bce_keep_f32 takes at most 64 kept and 64 trained attributes (got %d and %d)' % (len(idx), len(self.attrIdx)))
        if min(idx) < 0 or max(idx) >= n_out:
            raise ValueError('attr_keep: attribute index %d outside the regressor\'s %d outputs' % (max(idx) if max(idx) >= n_out else min(idx), n_out))
        if not hasattr(self.regressor, 'features'):
            raise ValueError('attr_keep: the regressor has no pooled-feature read-out (features) for the fused head')
        self.keepIdx = idx

    def _keep_columns(self):
        """keepIdx as a device index tensor, built once (as _attr_columns)."""
        t = getattr(self, '_keep_index', None)
        if t is None or t.numel() != len(self.keepIdx) or t.device != self.device:
            t = self._keep_index = torch.tensor(list(self.keepIdx), dtype=torch.long, device=self.device)
        return t

    def _regressor_outputs(self, logit, keep_feats=False):
        """All regressor outputs of ``logit``.  ``keep_feats`` (the training step's pass over the original image) with the attribute-preservation
        term on: the pooled features are computed once and remembered with the image (as prefetch_content_taps remembers ``_org_taps``);
        ``get_keep_feats`` picks them up.  The values are the regressor's own addmm.  Inference (apply_alpha, sweep, eval.py, vis_w.py) never asks:
        nothing is stashed there."""
        reg = self.regressor
        if not (keep_feats and getattr(self, 'attr_keep', 0.0)):
            return reg(logit)
        feat = reg.features(logit)
        self._org_feat = (logit, feat.detach())
        return torch.addmm(reg.fc_b, feat, reg.fc_w.t())

    def get_keep_feats(self, org):
        """The regressor's pooled features of the original image, a constant of the step: what get_reg_preds left when it was handed the same
        tensor, otherwise recomputed without a gradient."""
        pre, self._org_feat = self._org_feat, None
        if pre is not None and pre[0] is org:
            return pre[1]
        with torch.no_grad():
            return self.regressor.features(org.detach())

    def get_keep_loss(self, org, feat1, cols=None, target=None, c_reg=0.0):
        """(total, reg, keep) of _RegBceKeepFn on ``feat1`` = regressor.features(edited image) and the original's features (get_keep_feats):
        total = c_reg * reg + attr_keep * keep; ``cols`` None: no BCE part, total = attr_keep * keep.  ``last_keep_preds`` [B, M, 2]: the kept
        outputs of the edited and the original image as the launch formed them."""
        reg = self.regressor
        total, reg_loss, keep, self.last_keep_preds = _RegBceKeepFn.apply(feat1, self.get_keep_feats(org), reg.fc_w, reg.fc_b, cols, target,
                                                                          self._keep_columns(), float(c_reg), self.attr_keep)
        return total, reg_loss, keep

    def get_reg_preds(self, logit, keep_feats=False):
        """The regressor outputs of ``logit`` at attrIdx.  ``keep_feats``: the training step's call on the original image (_regressor_outputs)."""
        preds = self._regressor_outputs(logit, keep_feats).index_select(1, self._attr_columns())        # integer column select: bit-exact
        if len(preds.size()) == 1:
            preds = preds.unsqueeze(1)
        return preds

    def get_bce_loss(self, pred, y, eps=1e-12):
        return -(y * pred.clamp(min=eps).log() + (1 - y) * (1 - pred).clamp(min=eps).log()).mean()

    def walk_update(self):
        """The tail of every step, eager or replayed: the data-parallel all-reduce of the walk gradient (one RCCL call of <= 184 KB for the linear
        W+ walk), then the optimiser step."""
        dist.average_gradients(self.walk.parameters())
        self.optimizer.step()

    def optimizeParametersAll(self, feed_dict, trainEmbed, updateGAN, no_content_loss=False, no_gan_loss=False):
        self.optimizer.zero_grad()
        loss = self.get_w_loss(feed_dict, no_content_loss, no_gan_loss)
        loss.backward()
        self.walk_update()
        return loss

    optimize_parameters = optimizeParametersAll              # BASELINE.json spelling

    def calibrate_scales(self, n_steps, clamp=False, layers=None, no_content_loss=False, no_gan_loss=False):
        """--f16_calibrate: measure the fp16 path's static gradient exponents on THIS graph's weights (nets16.calibrate: ``n_steps`` probe steps a
        round — forward, loss and backward as the graph's ``_probe_step`` runs them for these loss flags, fresh z and alpha draws, no optimiser
        step — with a nets16.RangeMonitor behind the probe points).  The chosen exponents land in ``loss_scaler.log2`` and
        ``weight_sources['loss_scale_log2']``; the walk, its gradients, the optimiser state, the scaler's dynamic factor and counters and the RNG
        streams are left as they were.  Before the first capture only.  Returns nets16.calibrate's record."""
        from . import hostutil, nets16
        if self.loss_scaler is None:
            raise RuntimeError('calibrate_scales: only the fp16 path (--precision f16) has gradient scales')
        if getattr(self, '_captured_step', None) is not None:
            raise RuntimeError('calibrate_scales after the step was captured: the recorded graph has the static scales baked in')
        params = list(self.walk.parameters())
        grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
        terms = self.last_terms
        sl = dist.shard(self.BATCH_SIZE)

        def probe(k):
            zs = hostutil.z_sample(self.BATCH_SIZE, seed=nets16.CALIBRATE_SEED + k, dim_z=self.dim_z)[sl]
            alpha, _, _ = self.get_train_alpha(zs, N_attr=len(self.attrList), trainEmbed=False)
            self._probe_step(torch.Tensor(zs).to(self.device), torch.tensor(np.asarray(alpha)).float().to(self.device), clamp=clamp, layers=layers,
                             no_content_loss=no_content_loss, no_gan_loss=no_gan_loss)
        try:
            rec = nets16.calibrate(self.loss_scaler, probe, int(n_steps), self.device)
        finally:
            torch.cuda.synchronize()
            for p, g in zip(params, grads):
                p.grad = g
            self.last_terms = terms
        self.weight_sources['loss_scale_log2'] = dict(self.loss_scaler.log2)
        self.f16_calibration = rec
        return rec

    def save_multi_models(self, save_path_w, save_path_gan, trainEmbed=False, updateGAN=False, single_transform_name=None):
        print('Save W and GAN in %s and %s' % (save_path_w, save_path_gan))
        if updateGAN:
            raise NotImplementedError('jointly training the GAN is not implemented in the reference either (train.py:40-41)')
        if dist.rank() == 0:
            torch.save(self.walk, save_path_w + '_walk_module.ckpt')

    def load_multi_models(self, save_path_w, save_path_gan, trainEmbed=False, updateGAN=False, single_transform_name=None):
        print('Load w in %s' % save_path_w)
        self.walk = torch.load(save_path_w, map_location=self.device, weights_only=False)

    def vis_image_batch(self, graph_inputs, filename, batch_start, wgt=False, wmask=False, num_panels=7):
        raise NotImplementedError('Subclass should implement vis_image_batch')


class TransformGraph(WalkGraph):
    def __init__(self, lr, walk_type, nsliders, loss_type, eps, N_f, trainEmbed, attrList, attrTable, layers, stylegan_opts,
                 nets=None, id_weight=0.0, facenet_ckpt=None, attr_keep=0.0, attr_keep_attrs=None):
        WalkGraph.__init__(self, lr, nsliders, loss_type, trainEmbed)
        self.img_size = constants.resolution
        # --id_loss W: a fourth loss term W * mean_b (1 - cos(face(edited), face(original))) on the face network of eval.py's identity metric
        # (facenet.FaceIdFn).  0 (the default): nothing is built, launched or changed.
        self.id_weight, self.facenet_ckpt, self._face_net = float(id_weight or 0.0), facenet_ckpt, None
        if nets is None:
            nets = load_networks(self.img_size, self.device)
        netG, netD, self.regressor, self.vgg19, self.weight_sources = nets
        self.module = StyleGAN(netG, netD)

        self.attrTable = attrTable
        self.attrList = attrList
        self.attrIdx = self.get_attr_idx()
        self._init_attr_keep(attr_keep, attr_keep_attrs)

        # the reference hard-codes step = 6 (256^2, transform_base.py:285); generalised: n_latent = 2*(step+1)
        self.step = int(math.log2(self.img_size)) - 2
        self.stylegan_opts = stylegan_opts
        self.layers = layers
        self.is_mlp = constants.WALK_IS_MLP

        if walk_type == 'linear':
            if self.trainEmbed:
                raise NotImplementedError('WalkEmbed is unused in the paper (transform_base.py:298-303) and out of scope')
            if stylegan_opts.latent == 'z':
                raise NotImplementedError('Not implemented setting of linear transformation for z')
            elif stylegan_opts.latent == 'w':
                cls = WalkMlpMultiW if constants.WALK_IS_MLP else WalkLinearMultiW    # reference: is_mlp hard-coded False (:290)
                self.walk = cls(self.dim_z, self.step, nsliders, self.attrList).to(self.device)
            else:
                raise NotImplementedError('Not implemented latent walk type:' '{}'.format(stylegan_opts.latent))
        elif 'NN' in walk_type:
            self.walk = WalkNonLinearW(self.dim_z, self.step, nsliders, self.attrList).to(self.device)
        else:
            raise NotImplementedError('unknown walk_type %r' % (walk_type,))

        self._make_optimizer(netG)
        self.walk_type = walk_type

    # the reference's StyleGAN2 graph spells its optimiser ``optimizers`` (transform_base.py:329): the same slot
    optimizers = property(lambda self: self.optimizer, lambda self, opt: setattr(self, 'optimizer', opt))

    # -- reference helpers ---------------------------------------------------------------------------------------
    def get_logits(self, inputs_dict, reshape=True):
        if self.stylegan_opts.latent == 'z':
            raise NameError("latent: the reference's Generator.forward fails for input_is_latent=False (networks.py:471-494)")
        w = inputs_dict['w']
        if isinstance(w, (list, tuple)):
            w = torch.stack(list(w)).transpose(0, 1)
        else:
            w = w.transpose(0, 1)
        outputs_orig, _ = self.module.netG(w.contiguous(), input_is_latent=True)
        return outputs_orig

    def get_w(self, z, is_single=False):
        w = self.module.netG.style(z)
        if is_single:
            return [w]
        return [w] * (self.step + 1) * 2

    def get_w_new_tensor(self, multi_ws, alpha, layers=None, name=None, trainEmbed=False, index_=None):
        if layers is not None:
            layers = [int(l) for l in layers]                 # the reference passes strings through
        return self.walk(multi_ws, alpha=alpha, layers=layers)

    def get_alphas(self, alpha_org, alpha_target):
        """train.py flow (transform_base.py:405-408): epsilon = target - org."""
        return alpha_target - alpha_org

    def get_alphas_clamped(self, alpha_org, alpha_delta):
        """train_multi_attr.py:113 flow (graphs/pggan/transform_base.py:358-364): (clamped target, new delta)."""
        alpha_target = torch.clamp(alpha_org + alpha_delta, min=0, max=1)
        return alpha_target, alpha_target - alpha_org

    def get_reg_loss(self, feed_dict):
        logit = feed_dict['logit']
        reg = self.regressor
        if hasattr(reg, 'features') and len(self.attrIdx) <= 64:
            # [r6] fc + column select + the float64 BCE and everything autograd would run backwards through them as ONE launch each way (csrc/l2i_loss.hip):
            # ~40 launches of a few microseconds between the regressor's last conv and its first gradient conv otherwise
            return _RegBceFn.apply(reg.features(logit), reg.fc_w, reg.fc_b, self._attr_columns(), feed_dict['alpha'])
        alpha_gt = feed_dict['alpha'].to(torch.double)
        preds = reg(logit).index_select(1, self._attr_columns())
        return self.get_bce_loss(preds, alpha_gt).mean()

    def prefetch_content_taps(self, org_img):
        """[r6] Start the VGG-19 prefix of the ORIGINAL image (transform_base.py:444-454: ``target = model(org).detach()``, no gradient) on the content
        branch's stream as soon as that image exists, i.e. while the regressor reads it and the second generator pass runs: 6 ms (fp32) of large
        matrix-bound launches that fill the chip where the regressor's tail and the generator's 4^2 .. 64^2 layers do not.  ``get_content_loss`` picks
        the taps up when it is handed the same tensor; the values are the same launches' outputs, issued earlier.  The drivers call this (capture.forward,
        trainer.train_step) when the content loss is on; without the call nothing changes."""
        # Measured in round 6 (alternating runs on one box): the 16-bit path gains 0.8 % (c5 35.43 / 35.24 -> 35.08 / 34.99 ms per step: its
        # launches are short and the chip has holes to fill); the fp32 path LOSES 0.4 % (c3 99.27 / 99.54 -> 99.82 / 99.94: its launches saturate the chip
        # and the early taps only lengthen the critical chain) — so: on for the 16-bit path, off for fp32.
        from . import conv
        if self.vgg19 is None or not constants.CONCURRENT_LOSS_BRANCHES or conv.PRECISION not in conv.H8_PRECISIONS:
            return
        cur = torch.cuda.current_stream()
        side = self._side_streams()[1]
        side.wait_stream(cur)
        with torch.cuda.stream(side), torch.no_grad():
            self._org_taps = (org_img, self.vgg19.org_taps(org_img.detach()))

    def get_content_loss(self, org_img, shifted_img):
        """List of four scalars (transform_base.py:426-454)."""
        pre = getattr(self, '_org_taps', None)
        self._org_taps = None
        taps = pre[1] if (pre is not None and pre[0] is org_img) else None
        losses = self.vgg19.content_losses(org_img, shifted_img, org_taps=taps)
        return [losses[i] for i in range(4)]

    def face_net(self):
        """The face network of the identity term, loaded on first use from ``facenet_ckpt`` / constants.facenet_path (synthetic weights under
        the rule of the other networks; a missing checkpoint without them is an error)."""
        if self._face_net is None:
            from . import facenet
            self._face_net, src = facenet.load(self.facenet_ckpt, device=self.device)
            self.weight_sources['F'] = src
        return self._face_net

    def check_id_loss(self):
        """The refusals of the identity term, raised where the term is trained with (get_w_loss, captured_step, trainer.main), not where a graph
        is built: eval.py / vis_w.py rebuild the graph from a run's opt.yml, id_loss included, at whatever --precision they are asked for."""
        from . import conv
        if self.id_weight and conv.PRECISION == 'f16':
            raise NotImplementedError('id_loss with --precision f16: the face branch would need a fifth static gradient-scale exponent '
                                      '(nets16.loss_scale_for has R, V, D, G), which is not calibrated; use f32, bf16x3 or bf16')

    def get_id_loss(self, org, logit):
        """mean_b (1 - cos(e(logit[b]), e(org[b]))): the embedding of the original is a constant, the edit's is differentiable."""
        return self.face_net().id_distances(logit, org.detach()).mean()

    # -- loss / optimiser ----------------------------------------------------------------------------------------
    def _side_streams(self):
        if getattr(self, '_streams', None) is None:
            self._streams = (torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device))
        return self._streams

    def get_w_loss(self, feed_dict, no_content_loss=False, no_gan_loss=False):
        """Total walk loss of optimizeParametersAll (transform_base.py:459-486) without the optimiser step."""
        logit = feed_dict['logit']
        self.check_id_loss()
        gan_loss = content_losses = None
        # The three loss branches (discriminator, VGG content, regressor) are independent forward+backward chains over
        # the same image: each runs on its own HIP stream (autograd replays every node's backward on its forward
        # stream), so the tail of one network's launches overlaps the next one's instead of leaving CUs idle.
        cur = torch.cuda.current_stream()
        side = self._side_streams() if constants.CONCURRENT_LOSS_BRANCHES else (cur, cur)
        if not no_gan_loss:
            side[0].wait_stream(cur)
            with torch.cuda.stream(side[0]):
                D_fake_result = self.module.netD(logit)
                gan_loss = self.BCE_loss_logits(D_fake_result, torch.ones_like(D_fake_result))
        if not no_content_loss:
            side[1].wait_stream(cur)
            with torch.cuda.stream(side[1]):
                content_loss_list = self.get_content_loss(feed_dict['org'], feed_dict['logit'])
                content_losses = sum(content_loss_list) / len(content_loss_list)
        keep_loss = None
        if self.attr_keep:
            # --attr_keep: the regressor branch through the one launch that also holds the other attributes still (l2i_reg_bce_keep_f32); its total
            # already carries the 10 / 1 of the weight rule below and the option's weight
            head, reg_loss, keep_loss = self.get_keep_loss(feed_dict['org'], self.regressor.features(logit), self._attr_columns(), feed_dict['alpha'],
                                                           c_reg=1.0 if (no_content_loss and no_gan_loss) else 10.0)
        else:
            reg_loss = self.get_reg_loss(feed_dict)
        id_loss = self.get_id_loss(feed_dict['org'], logit) if self.id_weight else None
        if side[0] is not cur:
            cur.wait_stream(side[0])
            cur.wait_stream(side[1])
        if keep_loss is not None:
            loss = head
        else:
            loss = reg_loss if (no_content_loss and no_gan_loss) else 10 * reg_loss
        if not no_content_loss:
            loss = loss + 0.05 * content_losses
        if not no_gan_loss:
            loss = loss + 0.05 * gan_loss
        if id_loss is not None:
            loss = loss + self.id_weight * id_loss
        self.last_terms = dict(reg=reg_loss.detach(), cont=None if content_losses is None else content_losses.detach(),
                               gan=None if gan_loss is None else gan_loss.detach(), id=None if id_loss is None else id_loss.detach(),
                               keep=None if keep_loss is None else keep_loss.detach())
        return loss

    # -- the step as the drivers run it ----------------------------------------------------------------------------
    def _probe_step(self, z, alpha, **flags):
        from . import capture
        capture.forward_backward(self, z, alpha, **flags)

    def eager_step(self, zs_batch, alpha_for_graph, *, clamp=False, layers=None, no_content_loss=False, no_gan_loss=False, trainEmbed=False,
                   updateGAN=False):
        """One training step launched call by call, in the reference's order (train.py:56-101; ``clamp``: train_multi_attr.py:113,133) ->
        (loss, original images, edited images)."""
        z_global = torch.Tensor(zs_batch).to(self.device)                        # train.py:56
        w_global = self.get_w(z_global)                                          # :62
        out_zs = self.get_logits({'z': z_global, 'w': w_global})                 # :66
        if not no_content_loss:
            self.prefetch_content_taps(out_zs)                                   # the VGG taps of the original start beside the regressor / second generator pass
        alpha_org = self.get_reg_preds(out_zs, keep_feats=True)                  # :69
        ag = torch.tensor(alpha_for_graph).float().to(self.device)               # :84-85
        if clamp:
            alpha_target, epsilon = self.get_alphas_clamped(alpha_org, ag)
        else:                                                                    # train.py:86
            alpha_target, epsilon = ag, self.get_alphas(alpha_org, ag)
        w_new = self.get_w_new_tensor(w_global, epsilon, layers=layers)          # :89
        transformed_output = self.get_logits({'z': z_global, 'w': w_new})        # :94
        feed_dict = {'w': w_new, 'org': out_zs, 'logit': transformed_output, 'alpha': alpha_target}
        loss = self.optimizeParametersAll(feed_dict, trainEmbed=trainEmbed, updateGAN=updateGAN, no_content_loss=no_content_loss, no_gan_loss=no_gan_loss)
        return loss, out_zs, transformed_output

    def captured_step(self, batch, n_attr, *, clamp=False, layers=None, no_content_loss=False, no_gan_loss=False):
        """The same step as a hipGraph for ``batch`` samples a replay (capture.CapturedStep): what trainer.train_step asks for under --hip_graph."""
        from . import capture
        self.check_id_loss()
        if self.id_weight:                   # the face branch is not recorded: trainer.train_step takes its eager route
            if not getattr(self, '_id_eager_logged', False):
                import logging
                logging.info('--hip_graph with --id_loss: the identity branch is not recorded into the hipGraph; the step runs eagerly')
                self._id_eager_logged = True
            return None
        return capture.CapturedStep(self, batch, n_attr, clamp=clamp, layers=layers, no_content_loss=no_content_loss, no_gan_loss=no_gan_loss)

    # -- checkpoints ---------------------------------------------------------------------------------------------
    def load_multi_models_from_single(self, save_path_ws, save_path_gan, trainEmbed=False, updateGAN=False,
                                      single_transform_name=None, index=None):
        for i in range(len(save_path_ws)):
            walk_ckpt = torch.load(save_path_ws[i], map_location=self.device, weights_only=False)
            with torch.no_grad():
                self.walk.w[index[i]] = walk_ckpt.w[0]

    # -- inference ("next" row f-1: vis_w.py) --------------------------------------------------------------------
    def clip_ims(self, ims):
        return np.uint8(np.clip(((ims + 1) / 2.0) * 255, 0, 255))

    def apply_alpha(self, graph_inputs, alpha_to_graph, layers=None, name=None, trainEmbed=False, index_=None, given_w=None):
        """transform_base.py:554-603 (w branch): returns (edited image, alpha_org, original image)."""
        with torch.no_grad():
            zs_batch = graph_inputs['z']
            if not torch.is_tensor(zs_batch):
                zs_batch = torch.Tensor(zs_batch).to(self.device)
            latent_w = given_w if given_w is not None else self.get_w(zs_batch)
            out_zs = self.get_logits({'w': latent_w})
            alpha_org = self.get_reg_preds(out_zs)
            alpha_delta = self.get_alphas(alpha_org, torch.Tensor(np.asarray(alpha_to_graph)).to(self.device))
            if index_ is not None:
                if len(self.attrIdx) == len(self.attrTable):
                    alpha_delta[:, index_] = torch.Tensor(np.asarray(alpha_to_graph)).to(self.device) - alpha_org[:, index_]
                else:
                    i = self.attrIdx.index(index_)
                    alpha_delta[:, i] = torch.Tensor(np.asarray(alpha_to_graph)[:, 0]).to(self.device) - alpha_org[:, i]
            latent_w_new = self.get_w_new_tensor(latent_w, alpha_delta, layers=layers, name=name, trainEmbed=trainEmbed,
                                                 index_=index_)
            best_im_out = self.get_logits({'w': latent_w_new})
        return best_im_out, alpha_org, out_zs

    def vis_multi_image_batch_alphas(self, graph_inputs, filename, alphas_to_graph, alphas_to_target, batch_start,
                                     layers=None, name=None, wgt=False, wmask=False, trainEmbed=False, computeL2=False,
                                     given_w=None, index_=None):
        """transform_base.py:606-659: one PNG strip per sample, one panel per requested alpha; file name
        ``<filename>_sample<i>[_wgt]_<alpha_org>.png``.  Returns the list of written paths."""
        from PIL import Image
        zs_batch = graph_inputs['z']
        ims_transformed = []
        for ag in alphas_to_graph:
            best_im_out, alpha_org, out_zs = self.apply_alpha({'z': torch.Tensor(zs_batch).to(self.device)}, ag, name=name,
                                                              layers=layers, trainEmbed=trainEmbed, given_w=given_w, index_=index_)
            ims_transformed.append(self.clip_ims(best_im_out.detach().cpu().numpy()))
        written = []
        for ii in range(zs_batch.shape[0]):
            a = alpha_org[ii, index_].item() if (index_ is not None and len(self.attrList) > 1) else alpha_org[ii].reshape(-1)[0].item()
            strip = np.concatenate([x[ii].transpose(1, 2, 0) for x in ims_transformed], axis=1)      # panels side by side
            path = filename + '_sample{}'.format(ii + batch_start) + ('_wgt' if wgt else '') + '_%.2f.png' % a
            print('Save in ', path)
            Image.fromarray(strip).save(path)
            written.append(path)
        return written

    # -- inference: several attributes at once, whole sweeps, uint8 grids made on the device ------------------------
    def _walk_column(self, index):
        """The walk column of attribute-table index ``index`` (apply_alpha's mapping: the index itself with the full table)."""
        return index if len(self.attrIdx) == len(self.attrTable) else self.attrIdx.index(index)

    def _combine_delta(self, alpha_org, alpha_to_graph, index_):
        """transform_base.py:784-790: zero except column k of each index_[k], alpha_to_graph[k][:, 0] - alpha_org[:, col]."""
        alpha_delta = torch.zeros_like(alpha_org)
        for k, i in enumerate(index_):
            col = self._walk_column(i)
            alpha_delta[:, col] = torch.Tensor(np.asarray(alpha_to_graph[k])[:, 0]).to(self.device) - alpha_org[:, col]
        return alpha_delta

    def _sweep_delta(self, alpha_org, alpha_to_graph, index_):
        """alpha_delta of one panel: apply_alpha's for ``index_`` None or an int, apply_alpha_combine's for a list."""
        if isinstance(index_, (list, tuple)):
            return self._combine_delta(alpha_org, alpha_to_graph, index_)
        target = torch.Tensor(np.asarray(alpha_to_graph)).to(self.device)
        alpha_delta = self.get_alphas(alpha_org, target)
        if index_ is not None:
            if len(self.attrIdx) == len(self.attrTable):
                alpha_delta[:, index_] = target - alpha_org[:, index_]
            else:
                i = self.attrIdx.index(index_)
                alpha_delta[:, i] = torch.Tensor(np.asarray(alpha_to_graph)[:, 0]).to(self.device) - alpha_org[:, i]
        return alpha_delta

    def apply_alpha_combine(self, graph_inputs, alpha_to_graph, layers=None, name=None, trainEmbed=False, index_=None, given_w=None):
        """transform_base.py:769-811 (w branch): edit several attributes at once.  ``index_``: attribute-table indices (mapped to walk columns as
        in apply_alpha), ``alpha_to_graph[k]`` [B, >= 1]: the target of index_[k]; every other attribute keeps a zero delta.  Returns (edited
        image, alpha_org, original image)."""
        with torch.no_grad():
            zs_batch = graph_inputs['z']
            if not torch.is_tensor(zs_batch):
                zs_batch = torch.Tensor(zs_batch).to(self.device)
            latent_w = given_w if given_w is not None else self.get_w(zs_batch)
            out_zs = self.get_logits({'w': latent_w})
            alpha_org = self.get_reg_preds(out_zs)
            alpha_delta = self._combine_delta(alpha_org, alpha_to_graph, index_)
            latent_w_new = self.get_w_new_tensor(latent_w, alpha_delta, layers=layers, name=name, trainEmbed=trainEmbed, index_=index_)
            best_im_out = self.get_logits({'w': latent_w_new})
        return best_im_out, alpha_org, out_zs

    def _sweep(self, graph_inputs, alphas_to_graph, layers=None, given_w=None, index_=None, chunk=None):
        """sweep's work: (buf [P + 1, B, 3, R, R] fp32 on the device — the P panels, then the original —, alpha_org).  One buffer, so that a
        panel grid which also shows the original reads all its tiles from one tensor."""
        with torch.no_grad():
            zs_batch = graph_inputs['z']
            if not torch.is_tensor(zs_batch):
                zs_batch = torch.Tensor(zs_batch).to(self.device)
            latent_w = given_w if given_w is not None else self.get_w(zs_batch)
            out_zs = self.get_logits({'w': latent_w})
            alpha_org = self.get_reg_preds(out_zs)
            P, B = len(alphas_to_graph), out_zs.shape[0]
            buf = torch.empty((P + 1,) + tuple(out_zs.shape), device=self.device, dtype=torch.float32)
            buf[P].copy_(out_zs)
            chunk = B if chunk is None else int(chunk)
            if chunk < 1:
                raise ValueError('sweep: chunk must be >= 1 (got %d)' % chunk)
            new_ws = (self.get_w_new_tensor(latent_w, self._sweep_delta(alpha_org, ag, index_), layers=layers, index_=index_) for ag in alphas_to_graph)
            if chunk == B:                                     # one panel per generator call: apply_alpha's launches
                for p, w_new in enumerate(new_ws):
                    buf[p].copy_(self.get_logits({'w': w_new}))
            else:
                ws = torch.cat([torch.stack(list(w_new)) for w_new in new_ws], 1)          # [n_latent, P * B, dim_z], panel-major
                flat = buf[:P].view((P * B,) + tuple(out_zs.shape[1:]))
                for s in range(0, P * B, chunk):
                    flat[s:s + chunk].copy_(self.get_logits({'w': ws[:, s:s + chunk]}))
        return buf, alpha_org

    def sweep(self, graph_inputs, alphas_to_graph, layers=None, given_w=None, index_=None, chunk=None):
        """Every panel of an alpha sweep from one pass over the original: returns (panels [P, B, 3, R, R] fp32 on the device, alpha_org, out_zs).
        panels[p] is what ``apply_alpha(graph_inputs, alphas_to_graph[p], index_=index_)`` returns (``index_`` None or an int), or
        ``apply_alpha_combine(graph_inputs, alphas_to_graph[p], index_=index_)`` (``index_`` a list, every alphas_to_graph[p] a list with one
        target per index); get_w, the original image and its regressor pass run once instead of once per panel (P + 1 generator passes for
        2P).  The generator runs ``chunk`` images a call; the default, B, is one panel a call: the launches of apply_alpha, bit for bit."""
        buf, alpha_org = self._sweep(graph_inputs, alphas_to_graph, layers=layers, given_w=given_w, index_=index_, chunk=chunk)
        return buf[:-1], alpha_org, buf[-1]

    @staticmethod
    def _save_png(arr, path):
        from PIL import Image
        print('Save in ', path)
        Image.fromarray(arr).save(path)
        return path

    def vis_sweep_strips(self, graph_inputs, filename, alphas_to_graph, alphas_to_target, batch_start, layers=None, name=None, wgt=False,
                         given_w=None, index_=None, pad=0, chunk=None):
        """vis_multi_image_batch_alphas from one ``sweep`` and one l2i_panels_u8 launch: the same file names, one strip of P panels per sample
        (``pad`` > 0: imgrid's white gutters between them), quantised and laid out on the device and copied to the host once, as uint8.
        ``index_`` None or an int: apply_alpha's panels (an int still moves every attribute of the walk, as in the reference); a list: only the
        listed attributes move, every other one keeps a zero delta (apply_alpha_combine with the panel's alpha for each of them)."""
        from . import kernels
        only = isinstance(index_, (list, tuple))                # move these attributes alone, all of them to the panel's alpha
        if only:
            alphas_to_graph = [[ag] * len(index_) for ag in alphas_to_graph]
        buf, alpha_org = self._sweep(graph_inputs, alphas_to_graph, layers=layers, given_w=given_w, index_=index_, chunk=chunk)
        P, B = buf.shape[0] - 1, buf.shape[1]
        shown = index_[0] if only else index_                   # the attribute whose original value names the file
        tiles = [p * B + ii for ii in range(B) for p in range(P)]
        strips = kernels.panels_u8(buf.view((-1,) + tuple(buf.shape[2:])), tiles, B, 1, P, pad=pad, fill=255).cpu().numpy()
        written = []
        for ii in range(B):
            a = alpha_org[ii, self._walk_column(shown)].item() if (shown is not None and len(self.attrList) > 1) else alpha_org[ii].reshape(-1)[0].item()
            path = filename + '_sample{}'.format(ii + batch_start) + ('_wgt' if wgt else '') + '_%.2f.png' % a
            written.append(self._save_png(strips[ii], path))
        return written

    def vis_multi_image_batch_alphas_combine(self, graph_inputs, filename, alphas_to_graph, alphas_to_target, batch_start, layers=None,
                                             name=None, given_w=None, index_=None, pad=1):
        """transform_base.py:814-869, the paper's two-attribute figure: one PNG per sample, a P x P grid whose row follows index_[0]'s alpha and
        whose column follows index_[1]'s, with imgrid's white gutters of ``pad`` pixels; file ``<filename>_idx{a}_idx{b}_sample{i}.png``, and
        ``org_img/<same>_org.png`` for the unedited image.  One ``sweep`` of the P * P panels and one l2i_panels_u8 launch per batch (the
        originals ride in a spare tile column that is cut off on the host), then one device-to-host copy of uint8.  Returns the written paths.
        Two differences from the reference: it writes the grid as P separate strips (one file per row, the row's alpha in the name), here the
        grid is one file; and it saves the original as a JPEG through torchvision, here it is a PNG of the same clip_ims bytes."""
        from . import kernels
        if index_ is None or len(index_) != 2:
            raise ValueError('vis_multi_image_batch_alphas_combine: index_ names two attributes (got %r)' % (index_,))
        P = len(alphas_to_graph)
        pairs = [[ag1, ag2] for ag1 in alphas_to_graph for ag2 in alphas_to_graph]
        buf, _ = self._sweep(graph_inputs, pairs, layers=layers, given_w=given_w, index_=list(index_))
        B, R = buf.shape[1], buf.shape[-1]
        tiles = []
        for ii in range(B):
            for r in range(P):
                tiles += [(r * P + c) * B + ii for c in range(P)] + [P * P * B + ii if r == 0 else -1]
        grids = kernels.panels_u8(buf.view((-1,) + tuple(buf.shape[2:])), tiles, B, P, P + 1, pad=pad, fill=255).cpu().numpy()
        side = P * (R + pad) - pad
        org_dir = os.path.join(os.path.dirname(filename), 'org_img')
        os.makedirs(org_dir, exist_ok=True)
        written = []
        for ii in range(B):
            stem = filename + '_idx{}_idx{}_sample{}'.format(index_[0], index_[1], ii + batch_start)
            written.append(self._save_png(np.ascontiguousarray(grids[ii, :, :side]), stem + '.png'))
            written.append(self._save_png(np.ascontiguousarray(grids[ii, :R, side + pad:side + pad + R]),
                                          os.path.join(org_dir, os.path.basename(stem) + '_org.png')))
        return written

    def vis_multi_image_batch_alphas_compute_multi_attr(self, graph_inputs, filename, alphas_to_graph, alphas_to_target,
                                                        batch_start, layers=None, name=None, wgt=False, wmask=False,
                                                        trainEmbed=False, computeL2=False, given_w=None, index_=None):
        """Attribute-preservation half of eval.py (transform_base.py:675-767): for every requested alpha edit the batch,
        read all 40 regressor outputs of the edited and the original image, and sort every sample into one of three
        buckets by how far the TARGET attribute moved: |d| <= 0.3, <= 0.6, <= 1 (samples that moved further are dropped).
        Returns (multi_attr, attri_org, imgs, orgs): four lists of three lists (edited attrs [40], original attrs [40],
        uint8 edited image [3,R,R], uint8 original image)."""
        return self._compute_multi_attr(graph_inputs, alphas_to_graph, alphas_to_target, layers, name, trainEmbed, given_w, index_)[:4]

    def vis_multi_image_batch_alphas_compute_multi_attr_identity(self, graph_inputs, filename, alphas_to_graph, alphas_to_target,
                                                                 batch_start, face_net, layers=None, name=None, wgt=False, wmask=False,
                                                                 trainEmbed=False, computeL2=False, given_w=None, index_=None):
        """Both halves of eval.py from one generator pass per alpha: what vis_multi_image_batch_alphas_compute_multi_attr returns, plus
        ``dists`` (three lists, one per bucket, in the order of the other lists): the float64 cosine distance between the face embeddings of
        each bucket entry's edited and original image (eval.py:170-189).  ``face_net`` (facenet.InceptionResnetV1) embeds the whole batch
        on the device, from the generator's output: resize, network and distance never see a host copy of the images."""
        return self._compute_multi_attr(graph_inputs, alphas_to_graph, alphas_to_target, layers, name, trainEmbed, given_w, index_,
                                        face_net=face_net)

    def _compute_multi_attr(self, graph_inputs, alphas_to_graph, alphas_to_target, layers, name, trainEmbed, given_w, index_, face_net=None):
        zs_batch = graph_inputs['z']
        multi_attr, attri_org, imgs, orgs, dists = [[], [], []], [[], [], []], [[], [], []], [[], [], []], [[], [], []]
        index_list = [index_] if type(index_) == int else index_
        with torch.no_grad():
            for ag1, at1 in zip(alphas_to_graph, alphas_to_target):
                best_im_out, alpha_org, out_zs = self.apply_alpha({'z': torch.Tensor(zs_batch).to(self.device)}, ag1, name=name,
                                                                  layers=layers, trainEmbed=trainEmbed, given_w=given_w,
                                                                  index_=index_)
                pred_attr = self.regressor(best_im_out).detach().cpu().numpy()       # [N, 40]
                org = self.regressor(out_zs).detach().cpu().numpy()
                face_d = face_net.pair_distances(best_im_out, out_zs)[0].cpu().numpy() if face_net is not None else None
                best_im_out = self.clip_ims(best_im_out.detach().cpu().numpy())
                out_zs = self.clip_ims(out_zs.cpu().numpy())
                bucket = attribute_change_bucket(pred_attr[:, index_list[0]], org[:, index_list[0]])
                for i in range(pred_attr.shape[0]):
                    k = int(bucket[i])
                    if k < 3:
                        multi_attr[k].append(pred_attr[i])
                        attri_org[k].append(org[i])
                        imgs[k].append(best_im_out[i])
                        orgs[k].append(out_zs[i])
                        if face_d is not None:
                            dists[k].append(float(face_d[i]))
        return multi_attr, attri_org, imgs, orgs, dists


class PixelTransform(TransformGraph):
    """transform_base.py:901-903."""


# ----------------------------------------------------------------------------------------------------------------
# alpha samplers (utils/transforms.py:634-735 and the overrides in stylegan_v2_real/transform_op.py:65-77)
# ----------------------------------------------------------------------------------------------------------------
class FaceTransform:
    def __init__(self, atrr_name='Black_Hair'):
        self.atrr_name = atrr_name
        self.alpha_original = 1
        self.num_panel = 6
        self.embed_alpha_max = 1
        self.embedding_alpha = np.linspace(0.0, 1.0, self.num_panel)
        self.alpha_max = 1

    def get_train_alpha(self, zs_batch, N_attr=40, trainEmbed=False):
        """One target alpha ~ U(0,1)^N_attr per step, shared by the whole batch (global numpy RNG)."""
        batch_size = zs_batch.shape[0]
        if trainEmbed:
            index_ = np.random.choice(self.num_panel)
            alpha_val = self.embedding_alpha[index_]
            return np.ones((batch_size, self.Nsliders)) * (alpha_val / self.embed_alpha_max), alpha_val, index_
        alpha_val = np.random.uniform(0, 1, N_attr)
        return np.ones((batch_size, self.Nsliders)) * alpha_val, alpha_val, None

    def scale_test_alpha_for_graph(self, alpha, zs_batch, **kwargs):
        return alpha * np.ones((zs_batch.shape[0], self.Nsliders))

    def test_alphas(self):
        return np.linspace(0, 1, 9)

    def vis_alphas(self, num_panels):
        return np.linspace(0, 1, num_panels)


class SceneTransform:
    def __init__(self):
        self.alpha_max = 1
        self.num_panel = 6
        self.embed_alpha_max = 1
        self.embedding_alpha = np.linspace(0.0, 1.0, self.num_panel)

    def get_train_alpha(self, zs_batch, N_attr=40, trainEmbed=False):
        """One delta ~ U(-1,1)^N_attr per step, shared by the whole batch."""
        batch_size = zs_batch.shape[0]
        if trainEmbed:
            index_ = np.random.choice(self.num_panel)
            alpha_val = self.embedding_alpha[index_]
            return np.ones((batch_size, self.Nsliders)) * alpha_val, alpha_val, index_
        alpha_val = np.random.uniform(-1, 1, N_attr)
        return np.ones((batch_size, N_attr)) * alpha_val, alpha_val, None

    def scale_test_alpha_for_graph(self, alpha, zs_batch, **kwargs):
        return alpha * np.ones((zs_batch.shape[0], self.Nsliders))

    def test_alphas(self):
        return np.linspace(0, 1, 10)

    def vis_alphas(self, num_panels):
        return np.linspace(0, 1, num_panels)


# ----------------------------------------------------------------------------------------------------------------
# plugin lookup
# ----------------------------------------------------------------------------------------------------------------
def _make_graph(name, op_cls, pixel_cls=PixelTransform, size_constant='resolution'):
    """transform_graph_scene.py:5-125: ``pixel_cls`` (a graph's PixelTransform) with ``op_cls``'s alpha sampler; the image size is read from
    ``constants`` when a graph is built."""
    def __init__(self, lr=0.001, walk_type='NNz', loss='l2', eps=1.41, N_f=4, **kwargs):
        nsliders = 1
        self.walk_type = walk_type
        self.num_channels = constants.NUM_CHANNELS
        self.Nsliders = nsliders
        self.img_size = getattr(constants, size_constant)
        pixel_cls.__init__(self, lr, walk_type, nsliders, loss, eps, N_f, **kwargs)
        op_cls.__init__(self)

    def vis_image_batch(self, graph_inputs, filename, batch_start, wgt=False, wmask=False, num_panels=7, max_alpha=None,
                        min_alpha=None, N_attr=40):
        zs_batch = graph_inputs['z']
        if max_alpha is not None and min_alpha is not None:
            alphas = np.linspace(min_alpha, max_alpha, num_panels)
        else:
            alphas = np.linspace(0, 1, num_panels)
        return [self.scale_test_alpha_for_graph(a, zs_batch) for a in alphas], list(alphas)

    return type(name, (pixel_cls, op_cls), {'__init__': __init__, 'vis_image_batch': vis_image_batch, '__module__': pixel_cls.__module__})


SceneGraph = _make_graph('SceneGraph', SceneTransform)
faceGraph = _make_graph('faceGraph', FaceTransform)


def get_transform_graphs(model):
    if model == 'pggan':                                   # BASELINE config 1: z-space walk on the in-repo PGGAN-256 generator
        from . import pggan
        return [pggan.SceneGraph, pggan.faceGraph]
    if model != 'stylegan_v2_real':
        raise ImportError("No module named 'graphs.%s' in this build (stylegan_v2_real and pggan are MI355X-native)" % model)
    return [SceneGraph, faceGraph]


def find_model_using_name(model, transform):
    """graphs/__init__.py:3-22: class whose lower-cased name equals transform.replace('_','') + 'graph'."""
    target = transform.replace('_', '') + 'graph'
    for g in get_transform_graphs(model):
        if g.__name__.lower() == target.lower():
            print('Find NAME: ', target.lower())
            return g
    print("In graphs.transform_graph_scene, there should be a Class with class name that matches %s in lowercase." % target)
    raise SystemExit(0)
