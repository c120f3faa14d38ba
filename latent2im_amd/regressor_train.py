"""Training the attribute regressor (reference scene_regressor_256.py:86-171): torchvision ResNet-50 v1.5 with
``fc = Linear(2048, 40)``, BatchNorm in TRAINING mode (the reference never calls ``model.eval()``: batch statistics, running
statistics updated with momentum 0.1 — in its test loop too), ``MSELoss(preds, label).mean()``, ``Adam(model.parameters(), lr=1e-4)``,
checkpoints ``{'model': state_dict, 'optm': optimizer.state_dict()}`` that ``constants.reg_path`` then loads for the walk training.

Everything heavy runs on libl2i_hip.so: the forward / input-gradient convolutions are the walk path's kernels (weights repacked on the
GPU after every optimiser step), the weight gradients ``l2i_conv2d_wgrad_f32`` and the training-mode BatchNorm passes ``l2i_bn_*``
(csrc/l2i_train.hip).  torch supplies tensors, the [C]-sized statistics algebra, the 2048x40 fc GEMMs and ``torch.optim.Adam`` (the
reference uses it too).  No autograd graph is built: the backward is scheduled by hand like the frozen networks' input-gradients.

ONE schedule, three layer families.  ``TrainableResNet50.forward`` / ``backward`` / ``block_backward`` / ``stem_backward`` are the only walk over
the network; what a step launches is decided by the layer objects ``_layer_types()`` selects — all with one interface (conv: ``plan``, ``forward``,
``dgrad(gy, in_hw, residual=None)``, ``wgrad(x, gy)``; BatchNorm: ``forward``, ``backward``) — by the module the pool and the average come from
(``maps``: kernels or kernels16) and by four small hooks (``_input``, ``_head_grad``, ``_end_backward``, ``_probe``):
  _Conv / _BN                   the default eager fp32 step (``train_step``): 53 FrozenConv2d rebuilt per step, the [C]-sized algebra in torch;
  _ResidentConv / _ResidentBN   opt-in (``TrainableResNet50(resident=True)``, ``make_optimizer(guarded=True)``, ``DeviceDataset``, ``main(resident /
                                hip_graph / device_data)``): nothing packed, allocated or counted on the host between two batches — packs rewritten in
                                place (csrc/l2i_repack.hip), the [C]-sized algebra as kernels, one gradient arena, optim.GuardedAdam, batches gathered
                                from uint8 crops on the device — which capture.CapturedRegressorStep records into one hipGraph;
  _H8StemConv / _H8Conv / _H8BN ``TrainableResNet50H8`` (``main(precision='f16' / 'bf16')``): the resident step on 16-bit h8
                                maps — conv.ImgConvH8 / H8Conv forward and input gradients (every plane rewritten in place by one launch of
                                ``l2i_repack_planes_h8``), ``l2i_conv2d_wgrad_h8``, ``l2i_conv2d_wgrad_img_h8`` for conv1 and the h8 BatchNorm kernels
                                of csrc/l2i_train_h8.hip (every sum in a fixed order: a bit-reproducible step), fp32 master weights, a static x
                                dynamic loss scale (optim.LossScaler) — with the fp32 model's interface and checkpoints; capture.CapturedRegressorStep
                                records it too (the driver's ``hip_graph`` flag does not reach it yet).
"""
import csv
import os

import numpy as np
import torch

from . import _lib
from . import conv as C
from . import kernels as K
from . import kernels16 as K16
from .specs import RESNET50_LAYERS

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def conv_wgrad(x, gy, k, stride, pad):
    """dW [Cout,Cin,k,k] of a correlation y = conv(x, W, stride, pad) given gy = dL/dy."""
    b, cin, h, w = x.shape
    _, cout, oh, ow = gy.shape
    dw = torch.zeros(cout, cin, k, k, device=x.device, dtype=torch.float32)
    _lib.call('l2i_conv2d_wgrad_f32', _lib.fptr(dw), _lib.fptr(x), _lib.fptr(gy), b, cin, h, w, cout, oh, ow, k, k, stride, pad, pad)
    return dw


class _BN:
    """BatchNorm2d parameters + the training-mode forward / backward on the l2i_bn_* kernels."""

    def __init__(self, P, name, device):
        t = lambda k: torch.as_tensor(np.asarray(P[name + '.' + k]), dtype=torch.float32).clone().to(device)
        self.weight, self.bias = t('weight'), t('bias')
        self.running_mean, self.running_var = t('running_mean'), t('running_var')
        self.num_batches_tracked = torch.as_tensor(np.asarray(P.get(name + '.num_batches_tracked', 0))).to(torch.long).to(device)
        self.name = name

    def forward(self, x, residual=None, relu=True):
        b, c, h, w = x.shape
        n = b * h * w
        s = torch.zeros(2, c, device=x.device, dtype=torch.float64)
        _lib.call('l2i_bn_stats_f32', _lib.ptr(s[0]), _lib.ptr(s[1]), _lib.fptr(x), b, c, h * w)
        mean64 = s[0] / n
        var64 = (s[1] / n - mean64 * mean64).clamp_(min=0.0)                    # biased variance normalises (BatchNorm2d.forward)
        mean, invstd = mean64.float(), torch.rsqrt(var64 + BN_EPS).float()
        with torch.no_grad():                                                  # running statistics: momentum 0.1, UNBIASED variance
            self.running_mean.mul_(1 - BN_MOMENTUM).add_(mean, alpha=BN_MOMENTUM)
            self.running_var.mul_(1 - BN_MOMENTUM).add_((var64 * (n / max(n - 1, 1))).float(), alpha=BN_MOMENTUM)
            self.num_batches_tracked += 1
        scale = (self.weight * invstd).contiguous()
        shift = (self.bias - mean * scale).contiguous()
        y = torch.empty_like(x)
        _lib.call('l2i_bn_apply_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(scale), _lib.fptr(shift), _lib.fptr(residual), int(relu), b, c, h * w)
        return y, (x, mean.contiguous(), invstd.contiguous())

    def backward(self, gy, saved, out_mask=None, want_masked=False):
        """gy = dL/d(output of relu(bn(x) [+ residual])); out_mask = that output when a ReLU followed.  Returns (dx, d weight, d bias,
        masked gy or None)."""
        x, mean, invstd = saved
        b, c, h, w = x.shape
        n = b * h * w
        s = torch.zeros(2, c, device=x.device, dtype=torch.float64)
        _lib.call('l2i_bn_bwd_reduce_f32', _lib.ptr(s[0]), _lib.ptr(s[1]), _lib.fptr(gy), _lib.fptr(out_mask), _lib.fptr(x), _lib.fptr(mean),
                  _lib.fptr(invstd), b, c, h * w)
        d_bias, d_weight = s[0].float(), s[1].float()
        m_dy, m_dyxh = (s[0] / n).float().contiguous(), (s[1] / n).float().contiguous()
        dx = torch.empty_like(x)
        gm = torch.empty_like(x) if want_masked else None
        _lib.call('l2i_bn_bwd_apply_f32', _lib.fptr(dx), _lib.fptr(gm), _lib.fptr(gy), _lib.fptr(out_mask), _lib.fptr(x), _lib.fptr(mean),
                  _lib.fptr(invstd), _lib.fptr(self.weight), _lib.fptr(m_dy), _lib.fptr(m_dyxh), b, c, h * w)
        return dx, d_weight, d_bias, gm

    def tensors(self):
        return [('weight', self.weight), ('bias', self.bias)]


class _Conv:
    """A trainable bias-free convolution: the weight lives on the GPU; ``plan()`` (re)builds the packed forward / input-gradient
    launches of the frozen-conv machinery from the current weight (called once per step, after the optimiser)."""

    def __init__(self, P, name, stride, padding, device):
        self.weight = torch.as_tensor(np.asarray(P[name + '.weight']), dtype=torch.float32).clone().to(device)
        self.stride, self.padding, self.k = stride, padding, self.weight.shape[2]
        self.name, self.fc = name, None

    def plan(self):
        self.fc = C.FrozenConv2d(self.weight.detach(), stride=self.stride, padding=self.padding, device=self.weight.device)

    def forward(self, x):
        return self.fc.forward(x)

    def dgrad(self, gy, in_hw, residual=None):
        """dL/dx (+ ``residual``).  The sum is one axpby with alpha = beta = 1: a + b and b + a are the same bits, so the operand order is not
        special-cased (a downsample block hands conv1's gradient in as the residual of the downsample conv's)."""
        g = self.fc.dgrad(gy, in_hw)
        return g if residual is None else K.axpby(g, residual)

    def wgrad(self, x, gy):
        return conv_wgrad(x, gy, self.k, self.stride, self.padding)


class _ResidentBN(_BN):
    """_BN of a resident model: the sums of both passes are slices of the model's two float64 arenas (zeroed by one memset per pass), the
    [C]-sized algebra is l2i_bn_finalize_f32 / l2i_bn_bwd_finalize_f32 into buffers that live as long as the model, and the parameter gradients
    land in the model's gradient arena.  ``owner.track_stats`` False (the warm-up of a recording): the running statistics and the batch
    counter stay as they are."""

    def attach(self, owner, fwd_sums, bwd_sums, small, g_weight, g_bias):
        self.owner, self.fs, self.bs = owner, fwd_sums, bwd_sums
        self.mean, self.invstd, self.scale, self.shift, self.m_dy, self.m_dyxh = small
        self.g_weight, self.g_bias = g_weight, g_bias

    def _finalize(self, n, c):
        """The forward sums of ``n`` values per channel -> mean, invstd, scale, shift (and the running statistics)."""
        track = self.owner.track_stats
        _lib.call('l2i_bn_finalize_f32', _lib.fptr(self.mean), _lib.fptr(self.invstd), _lib.fptr(self.scale), _lib.fptr(self.shift),
                  _lib.fptr(self.running_mean) if track else None, _lib.fptr(self.running_var) if track else None,
                  _lib.ptr(self.num_batches_tracked) if track else None, _lib.ptr(self.fs[0]), _lib.ptr(self.fs[1]), _lib.fptr(self.weight),
                  _lib.fptr(self.bias), n, c, BN_EPS, BN_MOMENTUM)

    def _bwd_finalize(self, n, c):
        """The backward sums -> the parameter gradients (in the arena) and the two means the apply pass subtracts."""
        _lib.call('l2i_bn_bwd_finalize_f32', _lib.fptr(self.g_bias), _lib.fptr(self.g_weight), _lib.fptr(self.m_dy), _lib.fptr(self.m_dyxh),
                  _lib.ptr(self.bs[0]), _lib.ptr(self.bs[1]), n, c)

    def forward(self, x, residual=None, relu=True):
        b, c, h, w = x.shape
        _lib.call('l2i_bn_stats_f32', _lib.ptr(self.fs[0]), _lib.ptr(self.fs[1]), _lib.fptr(x), b, c, h * w)
        self._finalize(b * h * w, c)
        y = torch.empty_like(x)
        _lib.call('l2i_bn_apply_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(self.scale), _lib.fptr(self.shift), _lib.fptr(residual), int(relu), b, c, h * w)
        return y, (x, self.mean, self.invstd)

    def backward(self, gy, saved, out_mask=None, want_masked=False):
        x, mean, invstd = saved
        b, c, h, w = x.shape
        _lib.call('l2i_bn_bwd_reduce_f32', _lib.ptr(self.bs[0]), _lib.ptr(self.bs[1]), _lib.fptr(gy), _lib.fptr(out_mask), _lib.fptr(x), _lib.fptr(mean),
                  _lib.fptr(invstd), b, c, h * w)
        self._bwd_finalize(b * h * w, c)
        dx = torch.empty_like(x)
        gm = torch.empty_like(x) if want_masked else None
        _lib.call('l2i_bn_bwd_apply_f32', _lib.fptr(dx), _lib.fptr(gm), _lib.fptr(gy), _lib.fptr(out_mask), _lib.fptr(x), _lib.fptr(mean),
                  _lib.fptr(invstd), _lib.fptr(self.weight), _lib.fptr(self.m_dy), _lib.fptr(self.m_dyxh), b, c, h * w)
        return dx, self.g_weight, self.g_bias, gm


class _ResidentConv(_Conv):
    """_Conv of a resident model: packed once, then rewritten in place from the weight (FrozenConv2d.repack_); the weight gradient accumulates
    straight into its view of the model's gradient arena (zeroed once per step)."""

    def attach(self, owner, g_weight):
        self.owner, self.g_weight = owner, g_weight

    def plan(self):
        if self.fc is None:
            super().plan()
        else:
            self.fc.repack_(self.weight)

    def wgrad(self, x, gy):
        b, cin, h, w = x.shape
        _, cout, oh, ow = gy.shape
        _lib.call('l2i_conv2d_wgrad_f32', _lib.fptr(self.g_weight), _lib.fptr(x), _lib.fptr(gy), b, cin, h, w, cout, oh, ow, self.k, self.k, self.stride,
                  self.padding, self.padding)
        return self.g_weight


class TrainableResNet50:
    """torchvision ResNet-50 v1.5 (stride on the 3x3, downsample on the first block of a layer, adaptive average pool), every parameter
    trainable, BatchNorm in training mode.  ``state_dict()`` / ``load_state_dict()`` use torchvision's key names, so the checkpoints are
    the ones ``graph.load_networks`` (and the reference) read.

    ``resident=True``: nothing the step touches between two batches is allocated or packed by the host — every parameter gradient is a view
    of ONE flat buffer (``grad_arena``, zeroed once per step; ``p.grad`` points into it for good, so an optimiser's table of pointers never
    changes), the BatchNorm sums of a pass are one float64 arena zeroed by one memset, ``replan()`` is 53 ``FrozenConv2d.repack_`` calls.
    The step is then ``train_step_resident``; it can be recorded into a hipGraph (capture.CapturedRegressorStep)."""

    def __init__(self, state, device='cuda', num_classes=40, resident=False):
        P = state
        self.device = device
        self.resident, self.track_stats = bool(resident), True
        Stem, Conv, BN = self._layer_types()
        self.stem, self.stem_bn = Stem(P, 'conv1', 2, 3, device), BN(P, 'bn1', device)
        self.blocks = []
        for li, (planes, blocks, stride) in enumerate(RESNET50_LAYERS):
            for b in range(blocks):
                p = 'layer%d.%d' % (li + 1, b)
                s = stride if b == 0 else 1
                self.blocks.append(dict(
                    c1=Conv(P, p + '.conv1', 1, 0, device), b1=BN(P, p + '.bn1', device),
                    c2=Conv(P, p + '.conv2', s, 1, device), b2=BN(P, p + '.bn2', device),
                    c3=Conv(P, p + '.conv3', 1, 0, device), b3=BN(P, p + '.bn3', device),
                    cd=Conv(P, p + '.downsample.0', s, 0, device) if b == 0 else None,
                    bd=BN(P, p + '.downsample.1', device) if b == 0 else None))
        self.fc_w = torch.as_tensor(np.asarray(P['fc.weight']), dtype=torch.float32).clone().to(device)
        self.fc_b = torch.as_tensor(np.asarray(P['fc.bias']), dtype=torch.float32).clone().to(device)
        assert self.fc_w.shape[0] == num_classes
        if resident:
            self._make_resident()
        self.replan()

    def _layer_types(self):
        """(stem conv, conv, BatchNorm) classes of this model."""
        conv, bn = (_ResidentConv, _ResidentBN) if self.resident else (_Conv, _BN)
        return conv, conv, bn

    def _arena_order(self, named):
        """The order in which the parameters' gradients lie in the gradient arena (every view is found by name: any order serves)."""
        return named

    def _convs(self):
        return [self.stem] + [blk[c] for blk in self.blocks for c in ('c1', 'c2', 'c3', 'cd') if blk[c] is not None]

    def _make_resident(self):
        """The arenas of a resident model, and every object's views into them."""
        named = self.named_parameters()
        offs, total = {}, 0
        for k, t in self._arena_order(named):
            offs[k] = total
            total += (t.numel() + 3) // 4 * 4                       # every view on a 16-byte boundary (the optimiser's 16-byte accesses)
        self.grad_offsets, self.grad_arena = offs, torch.zeros(total, device=self.device, dtype=torch.float32)
        self.grads = {k: self.grad_arena[offs[k]:offs[k] + t.numel()].view(t.shape) for k, t in named}
        for k, t in named:
            t.grad = self.grads[k]
        bns = self._bns()
        csum = sum(bn.weight.numel() for bn in bns)
        self.fwd_sums = torch.zeros(2 * csum, device=self.device, dtype=torch.float64)
        self.bwd_sums = torch.zeros(2 * csum, device=self.device, dtype=torch.float64)
        small = torch.zeros(6 * csum, device=self.device, dtype=torch.float32)
        o = 0
        for bn in bns:
            c = bn.weight.numel()
            bn.attach(self, self.fwd_sums[2 * o:2 * (o + c)].view(2, c), self.bwd_sums[2 * o:2 * (o + c)].view(2, c),
                      [small[6 * o + i * c:6 * o + (i + 1) * c] for i in range(6)], self.grads[bn.name + '.weight'], self.grads[bn.name + '.bias'])
            o += c
        for cv in self._convs():
            cv.attach(self, self.grads[cv.name + '.weight'])

    def zero_grad(self):
        """Resident: one memset over every parameter gradient."""
        self.grad_arena.zero_()

    # -- parameters (torchvision order: conv1, bn1, layer*.*, fc) ------------------------------------------------------------
    def named_parameters(self):
        out = [('conv1.weight', self.stem.weight)] + [('bn1.' + k, t) for k, t in self.stem_bn.tensors()]
        for blk in self.blocks:
            for c, b in (('c1', 'b1'), ('c2', 'b2'), ('c3', 'b3'), ('cd', 'bd')):
                if blk[c] is not None:
                    out.append((blk[c].name + '.weight', blk[c].weight))
                    out += [(blk[b].name + '.' + k, t) for k, t in blk[b].tensors()]
        return out + [('fc.weight', self.fc_w), ('fc.bias', self.fc_b)]

    def parameters(self):
        return [t for _, t in self.named_parameters()]

    def _bns(self):
        return [self.stem_bn] + [blk[b] for blk in self.blocks for b in ('b1', 'b2', 'b3', 'bd') if blk[b] is not None]

    def state_dict(self):
        sd = {k: t.detach().clone() for k, t in self.named_parameters()}
        for bn in self._bns():
            sd[bn.name + '.running_mean'], sd[bn.name + '.running_var'] = bn.running_mean.clone(), bn.running_var.clone()
            sd[bn.name + '.num_batches_tracked'] = bn.num_batches_tracked.clone()
        return sd

    def load_state_dict(self, sd):
        with torch.no_grad():
            for k, t in self.named_parameters():
                t.copy_(torch.as_tensor(sd[k]).to(t.device))
            for bn in self._bns():
                bn.running_mean.copy_(torch.as_tensor(sd[bn.name + '.running_mean']).to(self.device))
                bn.running_var.copy_(torch.as_tensor(sd[bn.name + '.running_var']).to(self.device))
                if bn.name + '.num_batches_tracked' in sd:
                    bn.num_batches_tracked.copy_(torch.as_tensor(sd[bn.name + '.num_batches_tracked']).to(bn.num_batches_tracked.device))
        self.replan()

    def replan(self):
        """Repack every convolution from its current weight (after an optimiser step)."""
        self.stem.plan()
        for blk in self.blocks:
            for c in ('c1', 'c2', 'c3', 'cd'):
                if blk[c] is not None:
                    blk[c].plan()

    # -- forward / backward: the one schedule of every flavour ------------------------------------------------------------------
    maps = K                 # the module of the pool and the average: the maps are fp32 NCHW here
    monitor = None           # (TrainableResNet50H8 can hold a range monitor; nothing listens here)

    def _input(self, img):
        return img.detach().contiguous()

    def _head_grad(self, g_preds, last):
        """dL/d preds [B,40] -> dL/d(last block's output) through the fc and the average pool."""
        b, c, h, w = last
        return (torch.mm(g_preds, self.fc_w) * (1.0 / (h * w))).reshape(b, c, 1, 1).expand(b, c, h, w).contiguous()

    def _end_backward(self):
        pass

    def _probe(self, tag, *maps):
        pass

    def forward(self, img, keep=True):
        """[B,3,H,W] -> [B,40] in training mode; ``keep``: save what ``backward`` needs."""
        x = self._input(img)
        if self.resident:
            self.fwd_sums.zero_()                                   # every BatchNorm's sums of this pass: one memset
        z0 = self.stem.forward(x)
        a0, s0 = self.stem_bn.forward(z0)
        p0, idx0 = self.maps.maxpool2d_fwd(a0, 3, 2, 1)
        self._probe('T.fwd.stem', z0, a0)
        saved = dict(img=x, s0=s0, a0=a0, idx0=idx0, blocks=[])
        cur = p0
        for blk in self.blocks:
            y1, s1 = blk['b1'].forward(blk['c1'].forward(cur))
            y2, s2 = blk['b2'].forward(blk['c2'].forward(y1))
            z3 = blk['c3'].forward(y2)
            if blk['cd'] is not None:
                idt, sd = blk['bd'].forward(blk['cd'].forward(cur), relu=False)
            else:
                idt, sd = cur, None
            out, s3 = blk['b3'].forward(z3, residual=idt, relu=True)
            self._probe('T.fwd.' + blk['c1'].name.split('.')[0], s1[0], y1, s2[0], y2, z3, out)
            if keep:
                saved['blocks'].append((cur, y1, s1, y2, s2, s3, sd, out))
            cur = out
        feat = self.maps.dot_reduce(cur) * (1.0 / (cur.shape[2] * cur.shape[3]))
        self._saved = dict(saved, feat=feat, last=tuple(cur.shape[:4])) if keep else None
        return torch.addmm(self.fc_b, feat, self.fc_w.t())

    __call__ = forward

    def backward(self, g_preds):
        """dL/d preds [B,40] -> {parameter name: gradient} (resident: the views of the arena, which the caller zeroed — the fp32 weight
        gradients accumulate) and nothing else: the image gets no gradient here."""
        sv = self._saved
        if self.resident:
            self.bwd_sums.zero_()
            grads = self.grads
            torch.mm(g_preds.t(), sv['feat'], out=grads['fc.weight'])
            torch.sum(g_preds, 0, out=grads['fc.bias'])
        else:
            grads = {'fc.weight': torch.mm(g_preds.t(), sv['feat']), 'fc.bias': g_preds.sum(0)}
        g = self._head_grad(g_preds, sv['last'])
        self._probe('T.g.head', g)
        for blk, saved in zip(reversed(self.blocks), reversed(sv['blocks'])):
            g = self.block_backward(blk, saved, g, grads)
        self.stem_backward(sv, g, grads)
        self._end_backward()
        self._saved = None
        return grads

    def block_backward(self, blk, saved, g, grads):
        """One bottleneck block: g = dL/d(block output) -> dL/d(block input); parameter gradients are added to ``grads`` by name."""
        cur, y1, s1, y2, s2, s3, sd, out = saved
        hw = lambda t: (t.shape[2], t.shape[3])
        # out = relu(bn3(z3) + idt): the masked gradient gm feeds bn3 and the identity branch
        g_z3, dw, db, gm = blk['b3'].backward(g, s3, out_mask=out, want_masked=True)
        grads[blk['b3'].name + '.weight'], grads[blk['b3'].name + '.bias'] = dw, db
        grads[blk['c3'].name + '.weight'] = blk['c3'].wgrad(y2, g_z3)
        g_z2, dw, db, _ = blk['b2'].backward(blk['c3'].dgrad(g_z3, hw(y2)), s2, out_mask=y2)
        grads[blk['b2'].name + '.weight'], grads[blk['b2'].name + '.bias'] = dw, db
        grads[blk['c2'].name + '.weight'] = blk['c2'].wgrad(y1, g_z2)
        g_z1, dw, db, _ = blk['b1'].backward(blk['c2'].dgrad(g_z2, hw(y1)), s1, out_mask=y1)
        grads[blk['b1'].name + '.weight'], grads[blk['b1'].name + '.bias'] = dw, db
        grads[blk['c1'].name + '.weight'] = blk['c1'].wgrad(cur, g_z1)
        self._probe('T.g.' + blk['c1'].name.split('.')[0], g_z3, g_z2, g_z1)
        if blk['cd'] is None:
            return blk['c1'].dgrad(g_z1, hw(cur), residual=gm)      # the identity gradient rides on the conv's residual operand
        g_zd, dw, db, _ = blk['bd'].backward(gm, sd)
        grads[blk['bd'].name + '.weight'], grads[blk['bd'].name + '.bias'] = dw, db
        grads[blk['cd'].name + '.weight'] = blk['cd'].wgrad(cur, g_zd)
        return blk['cd'].dgrad(g_zd, hw(cur), residual=blk['c1'].dgrad(g_z1, hw(cur)))

    def stem_backward(self, sv, g, grads):
        """maxpool <- relu <- bn1 <- conv1: g = dL/d(pooled map); the image itself gets no gradient."""
        a0 = sv['a0']
        g_a0 = self.maps.maxpool2d_bwd(g, sv['idx0'], (a0.shape[2], a0.shape[3]), 3, 2, 1)
        g_z0, dw, db, _ = self.stem_bn.backward(g_a0, sv['s0'], out_mask=a0)
        self._probe('T.g.stem', g_a0, g_z0)
        grads['bn1.weight'], grads['bn1.bias'] = dw, db
        grads['conv1.weight'] = self.stem.wgrad(sv['img'], g_z0)


# ------------------------------------------------------------------------------------------------------------------------------------
# The 16-bit trainer: h8 maps, 16-bit MFMA, fp32 master weights
# ------------------------------------------------------------------------------------------------------------------------------------
PRECISIONS = ('f32', 'f16', 'bf16')
H8_DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16}


def regtrain_scale_for(image_size, batch):
    """log2 of the STATIC gradient scale of fp16 regressor training at ``image_size``^2 and ``batch``: the project's rule (nets16.loss_scale_for) —
    the largest stored gradient map lands near 2^5.  The MSE loss is a mean over B x 40 and reaches the maps through an average pool, so the
    gradients fall one octave per doubling of the batch and two per doubling of the side: 15 at 8 x 128^2, 19 at 32 x 256^2 (DESIGN.md section
    5.3 holds the measured maps).  bf16 has fp32's exponent range and takes 0 (TrainableResNet50H8 does that itself)."""
    import math
    return 15 + (int(round(math.log2(max(batch, 1)))) - 3) + 2 * (int(round(math.log2(image_size))) - 7)


def _in_scaled_tail(name, t):
    """Is the gradient of this parameter written in SCALED units (conv1.weight and the BatchNorm parameters of the 16-bit trainer)?"""
    return name == 'conv1.weight' or t.dim() == 1 and not name.startswith('fc.')


class _H8BN(_ResidentBN):
    """_ResidentBN on h8 maps: the two reductions and the two apply passes are csrc/l2i_train_h8.hip's, the [C]-sized algebra between them is the
    fp32 model's (_finalize / _bwd_finalize).  The parameter gradients land in the arena in SCALED units (the gradient maps carry the loss
    scale); the owner unscales them with one multiply after the backward."""

    def forward(self, x, residual=None, relu=True):
        b, g8, h, w, _ = x.shape
        K16.bn_stats(x, self.fs, ws=self.owner.bn_ws(x))
        self._finalize(b * h * w, g8 * 8)
        return K16.bn_apply(x, self.scale, self.shift, residual=residual, relu=relu), (x, self.mean, self.invstd)

    def backward(self, gy, saved, out_mask=None, want_masked=False):
        x, mean, invstd = saved
        b, g8, h, w, _ = x.shape
        K16.bn_bwd_reduce(gy, out_mask, x, mean, invstd, self.bs, ws=self.owner.bn_ws(x))
        self._bwd_finalize(b * h * w, g8 * 8)
        dx, gm = K16.bn_bwd_apply(gy, out_mask, x, mean, invstd, self.weight, self.m_dy, self.m_dyxh, want_masked=want_masked)
        return dx, self.g_weight, self.g_bias, gm


class _H8Conv(_ResidentConv):
    """A trainable bias-free convolution of the 16-bit trainer: fp32 master weight; ``plan()`` builds a conv.H8Conv of the element type once; after
    that the owner rewrites the planes of every convolution in place with one launch (TrainableResNet50H8.replan: conv.PlaneTable) and ``plan()``
    is only the path of a library without that kernel (H8Conv.repack: torch ops that allocate); the weight gradient is l2i_conv2d_wgrad_h8
    straight into the gradient arena, overwritten and already unscaled."""

    def __init__(self, P, name, stride, padding, device, elem='f16'):
        super().__init__(P, name, stride, padding, device)
        self.dtype, self.h8 = H8_DTYPES[elem], None

    def plan(self):
        w = self.weight.detach()
        if self.h8 is None:
            self.h8 = C.H8Conv(w, stride=self.stride, padding=self.padding, device=w.device, dtype=self.dtype)
        else:
            self.h8.repack(w)

    def forward(self, x):
        return self.h8.forward(x)

    def dgrad(self, gy, in_hw, residual=None):
        if residual is not None and self.stride == 2:              # the strided 1x1 downsample: compact conv + zero insertion onto the residual
            return K16.add_zero_insert(residual, self.h8.dgrad_compact(gy))
        return self.h8.dgrad(gy, in_hw, residual=residual)          # stride 1: the residual rides on the conv's own operand

    def wgrad(self, x, gy):
        o = self.owner
        return K16.conv_wgrad(x, gy, self.k, self.stride, self.padding, out=self.g_weight, ws=o.wgrad_ws(x, gy, self), out_scale=o.inv_static,
                              out_scale_dev=o.scaler.inv_dyn)


class _H8StemConv(_ResidentConv):
    """conv1 of the 16-bit trainer: conv.ImgConvH8 (7x7 stride 2, fp32 image in, h8 out), its 16-bit planes rewritten with every other
    convolution's by the owner's one launch; the weight gradient is l2i_conv2d_wgrad_img_h8 on the h8 gradient map as it lies and the fp32 image
    (fixed summation order, OVERWRITES its view of the arena, in scaled units).  A library without those entry points: ImgConvH8.repack (a host
    pack of 9408 weights) and the fp32 atomics kernel on the gradient map cast to fp32 (_ResidentConv.wgrad)."""

    def __init__(self, P, name, stride, padding, device, elem='f16'):
        super().__init__(P, name, stride, padding, device)
        self.dtype, self.img = H8_DTYPES[elem], None

    def plan(self):
        if self.img is None:
            self.img = C.ImgConvH8(self.weight.detach(), self.stride, self.padding, device=self.weight.device, dtype=self.dtype)
        else:
            self.img.repack(self.weight.detach())

    def forward(self, x):
        return self.img.forward(x)

    def wgrad(self, x, gy):
        if not self.owner.stem_kernel:
            return super().wgrad(x, K16.cast_from_h8(gy))
        return K16.conv_wgrad_img(x, gy, out=self.g_weight, ws=self.owner.stem_ws(x, gy))


class TrainableResNet50H8(TrainableResNet50):
    """TrainableResNet50 on the 16-bit path: every feature map and gradient map is an h8 tensor of ``precision`` ('f16', recommended, or 'bf16'),
    the convolutions run on the 16-bit MFMA (conv.H8Conv / conv.ImgConvH8, l2i_conv2d_wgrad_h8), BatchNorm on csrc/l2i_train_h8.hip; master
    weights, gradients, BatchNorm statistics, the fc and the loss stay fp32 / float64.  Resident from the start (one gradient arena, the two
    float64 BatchNorm arenas, optim.GuardedAdam with ``self.scaler``): ``train_step_resident`` drives it, checkpoints are TrainableResNet50's.
    The schedule is TrainableResNet50's: only the layer objects, ``maps`` and the hooks below differ.

    Loss scale: the gradient entering the maps is multiplied by 2^``loss_scale_log2`` (default regtrain_scale_for for fp16, 0 for bf16) times the
    scaler's dynamic factor; the weight gradients are unscaled by the kernel that writes them, conv1's and the BatchNorm parameters' by one
    multiply over their stretch of the arena, so ``p.grad`` is the true gradient — or non-finite after an overflow, which GuardedAdam skips."""
    maps = K16

    def __init__(self, state, device='cuda', num_classes=40, precision='f16', loss_scale_log2=None, image_size=256, batch=32):
        from . import optim
        assert precision in H8_DTYPES, precision
        self.precision, self.dtype = precision, H8_DTYPES[precision]
        if loss_scale_log2 is None:
            loss_scale_log2 = regtrain_scale_for(image_size, batch) if precision == 'f16' else 0
        self.loss_scale_log2 = int(loss_scale_log2)
        self.static, self.inv_static = float(2.0 ** self.loss_scale_log2), float(2.0 ** -self.loss_scale_log2)
        self.scaler = optim.LossScaler(dict(T=self.loss_scale_log2), device)
        self._bn_ws = self._wg_ws = self.planes = None
        # the stem's fixed-order weight gradient and the one-launch repack, where the library has them (an older build through L2I_LIB: today's path)
        self.stem_kernel, self.planes_kernel = _lib.has('l2i_conv2d_wgrad_img_h8'), _lib.has('l2i_repack_planes_h8')
        self.monitor = None                                       # a nets16.RangeMonitor: every stored map of a step is added to it by stage (tools/bench_regressor_train.py --ranges)
        super().__init__(state, device=device, num_classes=num_classes, resident=True)

    def _probe(self, tag, *maps):
        if self.monitor is not None:
            for t in maps:
                self.monitor.add(tag, t)

    def _layer_types(self):
        from functools import partial
        return partial(_H8StemConv, elem=self.precision), partial(_H8Conv, elem=self.precision), _H8BN

    def _arena_order(self, named):
        """conv1.weight and the BatchNorm parameters at the end, in one stretch: their gradients are written in scaled units."""
        return [kt for kt in named if not _in_scaled_tail(*kt)] + [kt for kt in named if _in_scaled_tail(*kt)]

    def _make_resident(self):
        super()._make_resident()
        first = next(k for k, t in self.named_parameters() if _in_scaled_tail(k, t))      # (the tail keeps the parameters' order)
        self.scaled_grads = self.grad_arena[self.grad_offsets[first]:]

    def bn_ws(self, x):
        b, g8, h, w, _ = x.shape
        n = K16.bn_ws_bytes(b, g8 * 8, h * w, x.dtype) // 8
        if self._bn_ws is None or self._bn_ws.numel() < n:
            self._bn_ws = torch.empty(n, device=x.device, dtype=torch.float64)
        return self._bn_ws

    def _wg_room(self, n, device):
        """The one float32 workspace of every weight gradient of the step, grown to ``n`` elements (the first step of a shape grows it to the
        largest need; nothing grows after that, so a recording's warm-up leaves it final)."""
        if self._wg_ws is None or self._wg_ws.numel() < n:
            self._wg_ws = torch.empty(n, device=device, dtype=torch.float32)
        return self._wg_ws

    def wgrad_ws(self, x, gy, cv):
        return self._wg_room(K16.wgrad_ws_bytes(x.shape[0], x.shape[1] * 8, x.shape[2], x.shape[3], gy.shape[1] * 8, gy.shape[2], gy.shape[3], cv.k, cv.stride,
                                                cv.padding, x.dtype) // 4, x.device)

    def stem_ws(self, x, gy):
        return self._wg_room(K16.wgrad_img_ws_bytes(x.shape[0], x.shape[2], x.shape[3], gy.dtype) // 4, x.device)

    def replan(self):
        """The first call builds every convolution's planes (packed on the host) and, once, the table of all 53 convolutions plus the stem; every
        later call is ONE launch that rewrites them in place from the master weights (conv.PlaneTable: the optimiser updates the masters in
        place and the planes never move, so the table stays valid)."""
        if self.planes is not None:
            return self.planes.run()
        super().replan()
        if self.planes_kernel:
            convs = self._convs()
            self.planes = C.PlaneTable(convs[0].img.segments(convs[0].weight) + [sg for cv in convs[1:] for sg in cv.h8.segments(cv.weight)], self.dtype)

    def _input(self, img):
        return img.detach().float().contiguous()

    def _head_grad(self, g_preds, last):
        """The head gradient in h8, times the static and the dynamic loss scale."""
        b, g8, h, w = last
        g_feat = torch.mm(g_preds, self.fc_w) * (self.static / (h * w)) * self.scaler.dyn
        return g_feat.reshape(b, g8, 1, 1, 8).expand(b, g8, h, w, 8).contiguous().to(self.dtype)

    def _end_backward(self):
        self.scaled_grads.mul_(self.scaler.inv_dyn * self.inv_static)          # conv1.weight and the BatchNorm parameters: scaled -> true gradients


def make_model(state, precision='f32', device='cuda', resident=False, **kw):
    """The trainer of ``precision``: TrainableResNet50 ('f32') or TrainableResNet50H8 ('f16' / 'bf16'; always resident)."""
    if precision not in PRECISIONS:
        raise ValueError('precision is one of %s, got %r' % (', '.join(PRECISIONS), precision))
    if precision == 'f32':
        return TrainableResNet50(state, device=device, resident=resident)
    return TrainableResNet50H8(state, device=device, precision=precision, **kw)


def mse_loss_and_grad(preds, label):
    """nn.MSELoss()(preds, label).mean() (scene_regressor_256.py:136,150) and its gradient w.r.t. preds."""
    d = preds - label
    return (d * d).mean(), d * (2.0 / d.numel())


def train_step(model, optimizer, data, label):
    """scene_regressor_256.py:147-153: forward, zero_grad, loss, backward, optimiser step.  Returns the loss (device scalar)."""
    preds = model(data)
    optimizer.zero_grad()
    loss, g = mse_loss_and_grad(preds, label.to(preds.device).float())
    grads = model.backward(g)
    for k, t in model.named_parameters():
        t.grad = grads[k]
    optimizer.step()
    model.replan()
    return loss


def train_step_resident(model, optimizer, data, label, update=True):
    """``train_step`` on a resident model: the gradients land in the model's arena (``p.grad`` already points there), the packs are rewritten
    in place.  Nothing here reads the device or depends on the step count, so a stream capture records it as it stands (``update`` False: the
    warm-up of a recording stops before the optimiser)."""
    assert model.resident
    preds = model(data)
    model.zero_grad()
    loss, g = mse_loss_and_grad(preds, label.to(preds.device).float())
    model.backward(g)
    if update:
        optimizer.step()
        model.replan()
    return loss


def make_optimizer(model, lr=1e-4, guarded=False):
    """scene_regressor_256.py:116: Adam(lr=1e-4), default betas.  ``guarded``: optim.GuardedAdam — the same arithmetic on the device (step
    counters included, so a hipGraph replays it; a step with a non-finite gradient is skipped as a whole), state allocated here and now."""
    if guarded:
        from . import optim
        opt = optim.GuardedAdam(model.parameters(), lr=lr, scaler=getattr(model, 'scaler', None))      # (the 16-bit model's dynamic loss scale)
        opt.init_state()
        return opt
    return torch.optim.Adam(model.parameters(), lr=lr)                          # scene_regressor_256.py:116


def save_ckpt(path, model, optimizer):
    """scene_regressor_256.py:166-170: {'model', 'optm'} — what constants.reg_path points at for the walk training."""
    torch.save({'model': {k: v.cpu() for k, v in model.state_dict().items()}, 'optm': optimizer.state_dict()}, path)


def load_ckpt(path, model, optimizer):
    ckpt = torch.load(path, map_location='cpu')
    model.load_state_dict(ckpt['model'])
    optimizer.load_state_dict(ckpt['optm'])
    return model, optimizer


def load_labelfile(path):
    """annotations.tsv: name <tab> 40 x 'value,confidence' (scene_regressor_256.py:67-74)."""
    labels = {}
    with open(path, 'r') as f:
        for line in csv.reader(f, delimiter='\t'):
            labels[line[0]] = np.array([float(i.split(',')[0]) for i in line[1:]])
    return labels


class CustomDataset:
    """The reference dataset (scene_regressor_256.py:27-64): images under folder/*/* listed in a split file; Resize(256) + CenterCrop(256)
    + ToTensor + Normalize(0.5, 0.5) with PIL and numpy (torchvision is not a dependency of this build)."""

    def __init__(self, folder_path, label_dict, split_file, image_size=256):
        import glob
        self.label_dict, self.image_size = label_dict, image_size
        with open(split_file, 'r') as f:
            split = set(i.strip() for i in f.readlines())
        self.image_list = [i for i in sorted(glob.glob(folder_path + '/*/*')) if '/'.join(i.split('/')[-2:]) in split]

    def __len__(self):
        return len(self.image_list)

    def __getitem__(self, index):
        crop, label = self.crop_u8(index)
        a = np.asarray(crop, dtype=np.float32) / 255.0
        x = torch.from_numpy((a.transpose(2, 0, 1) - 0.5) / 0.5)
        return x, torch.Tensor(label)

    def crop_u8(self, index):
        """(the resized, centre-cropped image as uint8 [S, S, 3], its label row): everything of ``__getitem__`` before ToTensor."""
        from PIL import Image
        path = self.image_list[index]
        im = Image.open(path).convert('RGB')
        w, h = im.size
        # torchvision Resize(int): the short side becomes image_size, the long side int(image_size * long / short) (truncated, not rounded)
        size = self.image_size
        new = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
        im = im.resize(new, Image.BILINEAR)
        w, h = im.size
        l, t = (w - self.image_size) // 2, (h - self.image_size) // 2
        return np.asarray(im.crop((l, t, l + self.image_size, t + self.image_size)), dtype=np.uint8), self.label_dict['/'.join(path.split('/')[-2:])]


class DeviceDataset:
    """A split kept on the GPU: ``dataset`` (a CustomDataset: deterministic Resize + CenterCrop, no augmentation) is decoded ONCE; the uint8
    crops [N, 3, S, S] and the labels [N, 40] stay on the device (the whole training split is under 2 GB) and a batch is one launch of
    l2i_batch_from_u8_f32 by an int64 index tensor — bit for bit what ``dataset[j]`` gives."""

    def __init__(self, dataset, device='cuda'):
        n, s = len(dataset), dataset.image_size
        crops, labels = np.empty((n, 3, s, s), dtype=np.uint8), None
        for j in range(n):
            crop, label = dataset.crop_u8(j)
            crops[j] = crop.transpose(2, 0, 1)
            if labels is None:
                labels = np.empty((n, len(label)), dtype=np.float32)
            labels[j] = np.asarray(label, dtype=np.float32)              # (what torch.Tensor(label) rounds to)
        self.n, self.size, self.device = n, s, device
        self.crops, self.labels = torch.from_numpy(crops).to(device), torch.from_numpy(labels).to(device)

    def __len__(self):
        return self.n

    def indices(self, sel):
        """A host selection -> int64 indices, checked here (on the device an index outside [0, N) gives a zero image, not an error)."""
        sel = np.asarray(sel, dtype=np.int64).reshape(-1)
        if sel.size == 0 or sel.min() < 0 or sel.max() >= self.n:
            raise IndexError('DeviceDataset: indices outside [0, %d)' % self.n)
        return torch.from_numpy(sel)

    def gather(self, idx, data=None, label=None):
        """data [B, 3, S, S], label [B, 40] <- the images / labels at the device indices ``idx`` (on the current stream)."""
        b = idx.numel()
        data = torch.empty(b, 3, self.size, self.size, device=self.device) if data is None else data
        label = torch.empty(b, self.labels.shape[1], device=self.device) if label is None else label
        assert idx.dtype == torch.long and data.shape[0] == b and label.shape == (b, self.labels.shape[1])
        _lib.call('l2i_batch_from_u8_f32', _lib.fptr(data), _lib.fptr(label), _lib.ptr(self.crops), _lib.fptr(self.labels), _lib.ptr(idx), b, self.n,
                  3 * self.size * self.size, self.labels.shape[1])
        return data, label

    def batch(self, sel):
        return self.gather(self.indices(sel).to(self.device))


def main(data_path='/transient_scene/imageAlignedLD/', label_path='/transient_scene/annotations/annotations.tsv',
         split_path='/transient_scene/training_test_splits/random_split/', n_epoch=500, batch_size=32, out_dir='./checkpoint_256', state=None,
         image_size=256, resident=False, hip_graph=False, device_data=False, precision='f32', loss_scale_log2=None):
    """The reference script's __main__ (scene_regressor_256.py:86-171) without tensorboard / tqdm: train, evaluate (in training mode, like the
    reference), save a checkpoint per epoch.  Opt-in: ``resident`` — the resident model and the guarded Adam (train_step_resident);
    ``hip_graph`` (implies resident) — full batches replay capture.CapturedRegressorStep, the ragged last batch and the test loop run the same
    model and optimiser eagerly; ``device_data`` — the training split lives on the GPU (DeviceDataset); ``precision`` 'f16' / 'bf16' — the 16-bit
    trainer (TrainableResNet50H8: always resident; it takes the same fp32 batches) with the static loss-scale exponent ``loss_scale_log2``
    (default regtrain_scale_for).  Its step is not captured yet: ``hip_graph`` with a 16-bit precision raises."""
    from . import synth
    if precision not in PRECISIONS:
        raise ValueError('precision is one of %s, got %r' % (', '.join(PRECISIONS), precision))
    if hip_graph and precision != 'f32':
        raise NotImplementedError('--hip_graph with --precision %s: the 16-bit regressor step is not recorded into a hipGraph yet (a follow-up: its '
                                  'weight planes are repacked by torch ops between two steps); drop --hip_graph or use --precision f32' % precision)
    os.makedirs(out_dir, exist_ok=True)
    labels = load_labelfile(label_path)
    train = CustomDataset(data_path, labels, split_path + 'training.txt', image_size=image_size)
    test = CustomDataset(data_path, labels, split_path + 'test.txt', image_size=image_size)
    resident = resident or hip_graph or precision != 'f32'
    # the reference starts from torchvision's ImageNet weights (a download); offline the caller passes a state dict, or seeded random init
    state = state if state is not None else synth.resnet50_state(seed=300)
    model = make_model(state, precision, device='cuda', resident=resident, loss_scale_log2=loss_scale_log2, image_size=image_size, batch=batch_size)
    optimizer = make_optimizer(model, guarded=resident)
    step = train_step_resident if resident else train_step
    on_device = DeviceDataset(train) if device_data else None
    captured = None
    for epoch in range(n_epoch):
        order = np.random.permutation(len(train))
        for i in range(0, len(order), batch_size):
            sel = order[i:i + batch_size]
            if on_device is None:
                batch = [train[j] for j in sel]
                data, label = torch.stack([b[0] for b in batch]), torch.stack([b[1] for b in batch])
            if hip_graph and len(sel) == batch_size:
                if captured is None:
                    from . import capture
                    captured = capture.CapturedRegressorStep(model, optimizer, batch_size, image_size, dataset=on_device)
                loss = captured(idx=on_device.indices(sel)) if on_device is not None else captured(data, label)
                continue
            if on_device is not None:
                data, label = on_device.batch(sel)
            loss = step(model, optimizer, data.cuda(), label.cuda())
        if epoch != 0:
            tl = []
            for i in range(0, len(test), batch_size):
                batch = [test[j] for j in range(i, min(len(test), i + batch_size))]
                preds = model(torch.stack([b[0] for b in batch]).cuda(), keep=False)
                tl.append(float(mse_loss_and_grad(preds, torch.stack([b[1] for b in batch]).cuda())[0]))
            print('Test epoch %d; Loss: %.5f' % (epoch, float(np.mean(tl))))
        save_ckpt(os.path.join(out_dir, '%s_dict.model' % str(epoch + 1).zfill(3)), model, optimizer)
    return model
