"""The face network of the identity-preservation metric (reference eval.py:29-32,170-209) on the l2i HIP kernels.

facenet_pytorch's ``InceptionResnetV1`` (vggface2 weights) is not on this path's dependency list, so it is restated here from the public
architecture (layer table and synthetic weights: face_specs.py), the way oracle/nets.py restates torchvision's ResNet-50 / VGG-19: it loads a facenet_pytorch
state dict by its key names (constants.facenet_path / ``--facenet_ckpt``) or runs on seeded synthetic weights (face_specs.facenet_state) under
the ALLOW_SYNTHETIC_WEIGHTS rule of the other networks.  Parity with facenet_pytorch itself is unpinned (no copy of it exists to compare
against); the restatement is pinned to a plain-torch float64 one (tests/facenet_ref.py).

Device path of one call, all fp32 whatever --precision the walk ran with:
  * ``l2i_face_resize_f32``: the generator's [-1, 1] image -> clip_ims -> PIL's ``resize((160, 160))``, bit for bit, one launch for the batch
    (host tables: ``resize_tables``).  No image leaves the device.
  * 132 convolutions through ``conv.run_launch`` (l2i_conv2d_f32 and its Winograd siblings): eval-mode BatchNorm folded into the weights and
    the epilogue bias in float64 at load time, ReLU in the epilogue; the residual blocks' ``relu(scale * (W cat + b) + x)`` is one launch
    with the scale folded into W and b and x as the epilogue residual.  Branch outputs are joined by ``torch.cat``.
  * max pools: ``l2i_maxpool2d_fwd_f32``.
  * ``l2i_face_head_f32``: avgpool + last_linear + folded last_bn + F.normalize, and the float64 cosine distance of every (edited, original)
    pair, one launch.

The identity loss of walk training (``--id_loss``, graph.TransformGraph.get_id_loss) runs the same network differentiably (``FaceIdFn``,
``InceptionResnetV1.id_distances``): ``l2i_face_resize_lin_f32`` (the same taps without the byte intermediate and the rounding, which have no
gradient), the same 132 launches keeping the post-ReLU maps and the pool indices, and a backward scheduled by hand on the conv kernels
(``_ConvBwd``, ``_features_bwd``) between ``l2i_face_head_bwd_f32`` and ``l2i_face_resize_lin_bwd_f32``.  The gradient launches are packed on
the first differentiable call: eval.py never builds them.
"""
import contextlib
import math
import os

import numpy as np
import torch

from . import constants, face_specs
from . import conv as C
from . import kernels as K

FACE_SIZE = 160


# ------------------------------------------------------------------------------------------------------------------------------------
# image -> network input
# ------------------------------------------------------------------------------------------------------------------------------------
def _bicubic(x):
    a = -0.5                                                  # PIL's bicubic_filter (Resample.c)
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_tables(in_size, out_size):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for one axis of ``Image.resize`` (box = the whole image, bicubic, support
    2 * max(in / out, 1)): bounds int32 [out, 2] = (first input pixel, tap count), coefficients int32 [out, ksize] (22-bit fixed point of
    the double taps normalised to sum 1, rounded half away from zero)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for o in range(out_size):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((t + xmin - center + 0.5) / filterscale) for t in range(n)]
        ww = sum(w)
        for t in range(n):
            k = w[t] / ww if ww != 0.0 else w[t]
            coef[o, t] = int(-0.5 + k * (1 << 22)) if k < 0 else int(0.5 + k * (1 << 22))
        bounds[o] = (xmin, n)
    return bounds, coef


_TABLES = {}        # (in, out, device) -> (bounds, coefficients) on the device


def _device_tables(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _TABLES:
        b, c = resize_tables(in_size, out_size)
        _TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device))
    return _TABLES[key]


def inverse_tables(in_size, out_size):
    """``resize_tables`` of one axis transposed, for the adjoint written as a gather: per INPUT pixel the outputs whose support holds it —
    bounds int32 [in, 2] = (first output, count), coefficients int32 [in, k] (the forward coefficient of that (output, input) pair).  The
    forward bounds are non-decreasing, so the outputs of one input pixel are consecutive."""
    b, c = resize_tables(in_size, out_size)
    lo = np.searchsorted(b[:, 0] + b[:, 1], np.arange(in_size), side='right')       # first output with first + count > i
    hi = np.searchsorted(b[:, 0], np.arange(in_size), side='right')                 # one past the last output with first <= i
    cnt = np.maximum(hi - lo, 0)
    ib = np.stack([np.where(cnt > 0, lo, 0), cnt], 1).astype(np.int32)
    ic = np.zeros((in_size, max(int(cnt.max()), 1)), np.int32)
    for i in range(in_size):
        for t in range(cnt[i]):
            o = lo[i] + t
            ic[i, t] = c[o, i - b[o, 0]]
    return ib, ic


_INV_TABLES = {}


def _device_inverse_tables(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _INV_TABLES:
        b, c = inverse_tables(in_size, out_size)
        _INV_TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device))
    return _INV_TABLES[key]


def face_input_lin(img, size=FACE_SIZE):
    """The differentiable ``face_input``: [B, C, H, W] -> Ry clip(((img + 1) 0.5) 255, 0, 255) Rx^T, fp32, the same taps / 2^22 without the
    byte intermediate, the rounding and the final clip (l2i_face_resize_lin_f32)."""
    img = img.float().contiguous()
    xb, xc = _device_tables(img.shape[3], size, img.device)
    yb, yc = _device_tables(img.shape[2], size, img.device)
    return K.face_resize_lin(img, xb, xc, yb, yc)


def face_input_lin_bwd(g, img):
    """The adjoint of ``face_input_lin`` at ``img``: g [B, C, size, size] -> the gradient w.r.t. img (l2i_face_resize_lin_bwd_f32)."""
    img = img.float().contiguous()
    ixb, ixc = _device_inverse_tables(img.shape[3], g.shape[3], img.device)
    iyb, iyc = _device_inverse_tables(img.shape[2], g.shape[2], img.device)
    return K.face_resize_lin_bwd(g, img, ixb, ixc, iyb, iyc)


def face_input(img, size=FACE_SIZE):
    """[B, C, H, W] generator image in [-1, 1] (on the GPU) -> [B, C, size, size] fp32 holding the bytes of
    ``Image.fromarray(clip_ims(img)[b].transpose(1, 2, 0)).resize((size, size))`` — eval.py:174-183 without the host round trip."""
    img = img.float().contiguous()
    xb, xc = _device_tables(img.shape[3], size, img.device)
    yb, yc = _device_tables(img.shape[2], size, img.device)
    return K.face_resize(img, xb, xc, yb, yc)


# ------------------------------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------------------------------
def _ignored(name):
    return name.startswith(face_specs.FACENET_IGNORED) or name.endswith('num_batches_tracked')


def check_state(sd):
    """A facenet_pytorch ``InceptionResnetV1`` state dict -> name -> float32 ndarray of face_specs.facenet_spec().  ``logits.*`` (the classifier)
    and ``num_batches_tracked`` are ignored; any other missing or extra key, or a shape that differs, is an error."""
    spec = face_specs.facenet_spec()
    need = [k for k in spec if not _ignored(k)]
    have = {k: v for k, v in sd.items() if not _ignored(k)}
    missing, extra = [k for k in need if k not in have], sorted(k for k in have if k not in spec)
    if missing or extra:
        raise KeyError('not an InceptionResnetV1 state dict: %d missing keys %s, %d unexpected keys %s'
                       % (len(missing), missing[:4], len(extra), extra[:4]))
    out = {}
    for k in need:
        v = have[k]
        v = v.detach().cpu().float().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float32)
        if tuple(v.shape) != tuple(spec[k]):
            raise ValueError('%s has shape %s, InceptionResnetV1 has %s' % (k, tuple(v.shape), tuple(spec[k])))
        out[k] = v
    return out


def load_state(path):
    """The vggface2 file of facenet_pytorch is a plain state_dict."""
    return check_state(torch.load(path, map_location='cpu'))


def load(path=None, device='cuda'):
    """The face network from ``path`` (default constants.facenet_path) or, on explicit request (constants.ALLOW_SYNTHETIC_WEIGHTS), from
    synthetic weights; (net, source)."""
    from .graph import _checkpoint_or_synthetic
    path = constants.facenet_path if path is None else path
    if _checkpoint_or_synthetic('face network (facenet_path / --facenet_ckpt; the reference downloads facenet_pytorch vggface2 weights)', path):
        return InceptionResnetV1(load_state(path), device=device), path
    return InceptionResnetV1(face_specs.facenet_state(seed=constants.SYNTH_SEED_F), device=device), 'synthetic(seed=%d)' % constants.SYNTH_SEED_F


# ------------------------------------------------------------------------------------------------------------------------------------
# network
# ------------------------------------------------------------------------------------------------------------------------------------
def _f64(P, name):
    return torch.as_tensor(np.asarray(P[name]), dtype=torch.float64)


class _Conv:
    """One launch: conv (+ folded BN) * scale, epilogue bias, optional residual, ReLU / none."""

    def __init__(self, w, b, stride, pad, relu, device):
        self.L = C.Launch(w.float(), stride, pad[0], pad[1], device=device)
        self.bias = b.float().contiguous().to(device)
        self.stride, self.pad, self.relu = stride, pad, relu

    def weight(self):
        """The folded weight [Cout, Cin, kh, kw] on the host, read back from the forward pack ([Cin][kh*kw][CoutP], exact): what the gradient
        launches are packed from (_ConvBwd) on the first differentiable call, so that a network that only evaluates keeps no second copy."""
        L = self.L
        return L.w[:, :, :L.cout].permute(2, 0, 1).reshape(L.cout, L.cin, L.kh, L.kw).contiguous().cpu()

    def __call__(self, x, residual=None):
        kh, kw = self.L.kh, self.L.kw
        oh = (x.shape[2] + 2 * self.pad[0] - kh) // self.stride + 1
        ow = (x.shape[3] + 2 * self.pad[1] - kw) // self.stride + 1
        y = torch.empty(x.shape[0], self.L.cout, oh, ow, device=x.device, dtype=torch.float32)
        C.run_launch(self.L, x, y, bias=self.bias, residual=residual, act=C.ACT_RELU if self.relu else C.ACT_NONE)
        return y


class _ConvBwd:
    """The input gradient of one _Conv (or, ``cols``: of the input channels [lo, hi) of it, the up-conv seen from one branch of the cat):
    stride 1, whatever the window, one launch of the flipped, channel-transposed weight with pads (kh - 1 - pad_y, kw - 1 - pad_x); the 3x3
    stride-2 pad-0 layers the transposed forms of conv.py (one fused launch, or the four parity launches where the gradient lands on the
    image's 3 channels).  ``mask``: the layer's own ReLU output; its mask rides on the launch's loads (in_mask)."""

    def __init__(self, cv, device, cols=None):
        w = cv.weight()
        if cols is not None:
            w = w[:, cols[0]:cols[1]]
        wt = w.transpose(0, 1).contiguous()                       # [Cin, Cout, kh, kw]: roles swapped for the gradient
        self.cin, self.stride = wt.shape[0], cv.stride
        kh, kw = wt.shape[2], wt.shape[3]
        self.L = self.plan = self.fused = None
        if cv.stride == 1:
            self.L = C.Launch(torch.flip(wt, [2, 3]), 1, kh - 1 - cv.pad[0], kw - 1 - cv.pad[1], device=device)
        else:
            assert cv.stride == 2 and (kh, kw) == (3, 3) and tuple(cv.pad) == (0, 0), (cv.stride, kh, kw, cv.pad)
            self.plan = [L.to(device) for L in C.transposed_plan(wt, 0)]
            if (3, 0) in C.FUSED_TRANSPOSED_SHAPES and wt.shape[0] > 4 and wt.shape[1] % 4 == 0:
                self.fused = C.FusedTransposed(wt, 0).to(device)

    def __call__(self, g, in_hw, mask=None, out=None, **kw):
        """g: the gradient w.r.t. the layer's output (after its ReLU where ``mask`` is given) -> w.r.t. its input [B, Cin, *in_hw]; ``kw``: the
        epilogue of conv.run_launch (residual, res_mask, accumulate)."""
        if out is None:
            out = torch.empty(g.shape[0], self.cin, in_hw[0], in_hw[1], device=g.device, dtype=torch.float32)
        m = dict(in_mask=mask, mask=(1.0, 0.0)) if mask is not None else {}
        if self.L is not None:
            C.run_launch(self.L, g, out, **m, **kw)
        elif self.fused is not None and C.USE_FUSED_TRANSPOSED and not kw:
            C.run_fused_transposed(self.fused, g, out, **m)
        else:
            C.run_plan(self.plan, g, out, **m, **kw)
        return out


def _basic(P, prefix, stride, pad, device):
    """BasicConv2d: conv (no bias) + BatchNorm2d(eps=1e-3) folded in float64 + ReLU."""
    w = _f64(P, prefix + '.conv.weight')
    k = _f64(P, prefix + '.bn.weight') / torch.sqrt(_f64(P, prefix + '.bn.running_var') + face_specs.FACENET_BN_EPS)
    b = _f64(P, prefix + '.bn.bias') - _f64(P, prefix + '.bn.running_mean') * k
    return _Conv(w * k.reshape(-1, 1, 1, 1), b, stride, pad, True, device)


@contextlib.contextmanager
def _fp32():
    """The identity half runs the exact-fp32 kernels whatever --precision the walk ran with (bf16x3 would send eligible layers to the
    split-precision kernel)."""
    saved = C.PRECISION
    C.PRECISION = 'f32'
    try:
        yield
    finally:
        C.PRECISION = saved


class InceptionResnetV1:
    """facenet_pytorch ``InceptionResnetV1(classify=False).eval()``: [B, 3, 160, 160] raw 0..255 -> unit embeddings [B, 512]."""

    def __init__(self, state, device='cuda'):
        P = check_state(state)
        self.device = device
        self.stem = [(_basic(P, name, stride, pad, device), name == 'conv2d_2b') for name, _, _, _, stride, pad in face_specs.FACENET_STEM]
        self.trunk = []
        for prefix, kind, scale, relu in face_specs.FACENET_TRUNK:
            branches = face_specs.FACENET_MIXED[prefix] if kind == 'mixed' else face_specs.FACENET_BLOCKS[kind][1]
            convs = [[_basic(P, prefix + '.' + sfx, stride, pad, device) for sfx, _, _, _, stride, pad in br] for br in branches]
            up = None
            if kind != 'mixed':               # relu(scale * (W cat + b) + x): scale folded into W and b, x is the epilogue residual
                up = _Conv(_f64(P, prefix + '.conv2d.weight') * scale, _f64(P, prefix + '.conv2d.bias') * scale, 1, (0, 0), relu, device)
            self.trunk.append((convs, up))
        w = _f64(P, 'last_linear.weight')                                                   # [512, 1792]
        k = _f64(P, 'last_bn.weight') / torch.sqrt(_f64(P, 'last_bn.running_var') + face_specs.FACENET_BN_EPS)
        self.head_w_t = (w * k.reshape(-1, 1)).t().float().contiguous().to(device)           # [1792, 512]
        self.head_b = (_f64(P, 'last_bn.bias') - _f64(P, 'last_bn.running_mean') * k).float().contiguous().to(device)

    def features(self, x):
        """[B, 3, 160, 160] -> the trunk's output [B, 1792, 3, 3] (what avgpool_1a reads)."""
        with torch.no_grad(), _fp32():
            x = x.float().contiguous()
            for cv, pool in self.stem:
                x = cv(x)
                if pool:                                                 # maxpool_3a after conv2d_2b
                    x = K.maxpool2d_fwd(x, 3, 2, 0)[0]
            for convs, up in self.trunk:
                outs = []
                for br in convs:
                    y = x
                    for cv in br:
                        y = cv(y)
                    outs.append(y)
                if up is None:                                           # mixed_6a / mixed_7a: MaxPool2d(3, 2) branch last
                    x = torch.cat(outs + [K.maxpool2d_fwd(x, 3, 2, 0)[0]], 1)
                else:
                    x = up(torch.cat(outs, 1), residual=x)
        return x

    def embed(self, x):
        """[B, 3, 160, 160] raw 0..255 -> unit embeddings [B, 512] (fp32)."""
        return K.face_head(self.features(x), self.head_w_t, self.head_b)[0]

    def __call__(self, x):
        return self.embed(x)

    # -- the differentiable branch (the identity loss of walk training) ---------------------------------------------------------------
    def _gradient_launches(self):
        """The _ConvBwd of every conv, built on the first differentiable call (eval.py never pays for them): (stem, trunk) in the layout of
        self.stem / self.trunk; a residual block's up-conv as one _ConvBwd per branch, on that branch's weight columns — the adjoint of
        ``torch.cat`` without a split copy."""
        if getattr(self, '_bwd', None) is None:
            dev = self.device
            stem = [_ConvBwd(cv, dev) for cv, _ in self.stem]
            trunk = []
            for convs, up in self.trunk:
                ups, lo = None, 0
                if up is not None:
                    ups = []
                    for br in convs:
                        ups.append(_ConvBwd(up, dev, cols=(lo, lo + br[-1].L.cout)))
                        lo += br[-1].L.cout
                trunk.append(([[_ConvBwd(cv, dev) for cv in br] for br in convs], ups))
            self._bwd = (stem, trunk)
        return self._bwd

    def _features_taped(self, x):
        """``features`` (the same 132 launches) keeping what the backward reads: every conv's post-ReLU output (they are the masks), the max
        pools' indices and the input sizes -> (trunk output, tape)."""
        x = x.float().contiguous()
        tape = dict(stem=[], trunk=[])
        for cv, pool in self.stem:
            hw = (x.shape[2], x.shape[3])
            y = cv(x)
            x, idx = y, None
            if pool:
                x, idx = K.maxpool2d_fwd(y, 3, 2, 0)
            tape['stem'].append((hw, y, idx))
        for convs, up in self.trunk:
            hw, outs, idx = (x.shape[2], x.shape[3]), [], None
            for br in convs:
                ys, y = [], x
                for cv in br:
                    y = cv(y)
                    ys.append(y)
                outs.append(ys)
            if up is None:
                p, idx = K.maxpool2d_fwd(x, 3, 2, 0)
                x = torch.cat([ys[-1] for ys in outs] + [p], 1)
            else:
                x = up(torch.cat([ys[-1] for ys in outs], 1), residual=x)
            tape['trunk'].append((hw, outs, idx, x))
        return x, tape

    def _features_bwd(self, tape, g):
        """g = the gradient w.r.t. the trunk's output -> w.r.t. the network's input.  Throughout, g is the gradient w.r.t. a map AFTER its
        ReLU; the mask is applied by the launches that read g (in_mask; on the identity path of a block res_mask).  Where a map has several
        readers their gradients meet in the epilogue of the 1x1 launches that land on it (residual / accumulate); only a reduction block's
        strided branch and its pool come as maps of their own."""
        stem_b, trunk_b = self._gradient_launches()
        for (convs, up), (bconvs, bups), (hw, outs, idx, x_out) in zip(reversed(self.trunk), reversed(trunk_b), reversed(tape['trunk'])):
            pending, first = [], {}
            if up is not None:                                   # x_out = relu?(up(cat) + x)
                m = x_out if up.relu else None
                heads = [bu(g, hw, mask=m) for bu in bups]
                first = dict(residual=g, res_mask=m)
            else:                                                # x_out = cat(branches, maxpool(x))
                heads, lo = [], 0
                for br in convs:
                    heads.append(g[:, lo:lo + br[-1].L.cout].contiguous())
                    lo += br[-1].L.cout
                pending.append(K.maxpool2d_bwd(g[:, lo:].contiguous(), idx, hw, 3, 2, 0))
            acc = None
            for br, bbr, ys, h in zip(convs, bconvs, outs, heads):
                for j in range(len(br) - 1, 0, -1):
                    h = bbr[j](h, (ys[j - 1].shape[2], ys[j - 1].shape[3]), mask=ys[j])
                if br[0].stride != 1:                            # mixed_6a.branch0: the strided conv reads x itself
                    pending.append(bbr[0](h, hw, mask=ys[0]))
                elif acc is None:
                    if not first and pending:
                        first = dict(residual=pending.pop())
                    acc = bbr[0](h, hw, mask=ys[0], **first)
                else:
                    bbr[0](h, hw, mask=ys[0], out=acc, accumulate=True)
            assert acc is not None
            for t in pending:
                K.axpby(acc, t, out=acc)
            g = acc
        for bcv, (hw, y, idx) in zip(reversed(stem_b), reversed(tape['stem'])):
            if idx is not None:
                g = K.maxpool2d_bwd(g, idx, (y.shape[2], y.shape[3]), 3, 2, 0)
            g = bcv(g, hw, mask=y)
        return g

    def embed_lin(self, img):
        """Generator images [B, 3, R, R] in [-1, 1] -> unit embeddings [B, 512] through the differentiable resize (no gradient kept)."""
        with torch.no_grad(), _fp32():
            return K.face_head(self.features(face_input_lin(img.detach())), self.head_w_t, self.head_b)[0]

    def id_distances(self, edited, original):
        """1 - cos(e(edited[b]), e(original[b])), [B] fp32, differentiable w.r.t. ``edited``; the original's embedding is a constant."""
        return FaceIdFn.apply(edited, self.embed_lin(original), self)

    def pair_distances(self, edited, original):
        """Generator images [N, 3, R, R] in [-1, 1], both on the GPU -> (float64 cosine distances [N] of each (edited, original) pair as
        eval.py:186-189 computes them, embeddings [2N, 512]): one resize launch, one network pass and one head launch for the 2N images."""
        n = edited.shape[0]
        assert original.shape == edited.shape
        x = face_input(torch.cat([edited.float(), original.float()], 0))
        emb, dist = K.face_head(self.features(x), self.head_w_t, self.head_b, npairs=n)
        return dist, emb


class FaceIdFn(torch.autograd.Function):
    """dist[b] = 1 - cos(e1[b], e0[b]) with e1 = head(trunk(resize_lin(x1))) and e0 [B, 512] a constant: the face branch of the identity loss,
    differentiable w.r.t. the edited images x1 [B, 3, R, R] (in the style of regressor._ResNetFeatFn).  Forward: the resize, the network's 132
    launches keeping the post-ReLU maps and the pool indices, the head.  Backward, by hand on the same kernels: l2i_face_head_bwd_f32, the
    gradient launches of InceptionResnetV1._features_bwd, l2i_face_resize_lin_bwd_f32.  fp32 whatever --precision the walk runs with."""

    @staticmethod
    def forward(ctx, x1, e0, net):
        x = x1.detach().float().contiguous()
        e0 = e0.detach().float().contiguous()
        with _fp32():
            feat, tape = net._features_taped(face_input_lin(x))
            e1 = K.face_head(feat, net.head_w_t, net.head_b)[0]
        ctx.net, ctx.in_dtype = net, x1.dtype
        ctx.tape = tape if ctx.needs_input_grad[0] else None
        ctx.save_for_backward(x, e0, feat)
        return 1.0 - torch.nn.functional.cosine_similarity(e1, e0, dim=1)

    @staticmethod
    def backward(ctx, g_dist):
        net, tape = ctx.net, ctx.tape
        if tape is None:
            raise RuntimeError('the face branch was run without a differentiable input')
        x, e0, feat = ctx.saved_tensors                  # (the tape stays with ctx: a second backward under retain_graph finds it)
        with _fp32():
            g = K.face_head_bwd(feat, net.head_w_t, net.head_b, e0, g_dist.float())
            g = net._features_bwd(tape, g)
            g = face_input_lin_bwd(g, x)
        return g.to(ctx.in_dtype), None, None


def identity_preservation(sim):
    """eval.py:200-209: per non-empty bucket, (sum of the cosine distances, 1 - their mean)."""
    results, results_avg = [], []
    for k in range(3):
        if len(sim[k]) == 0:
            continue
        results.append(np.sum(sim[k]))
        results_avg.append(1 - np.mean(sim[k]))
    return results, results_avg


def identity_mode(mode, path):
    """--identity {auto, on, off} -> whether the identity half runs.  auto: only when the face checkpoint ``path`` exists (one line on
    stderr otherwise, so the printed output is that of a run without the option); on: a checkpoint or, where the run allows them, synthetic
    weights, else FileNotFoundError; off: never."""
    import sys
    if mode == 'off':
        return False
    if mode == 'auto':
        if path and os.path.isfile(path):
            return True
        print('[identity] no face network checkpoint (%r; set constants.facenet_path or pass --facenet_ckpt): identity preservation skipped'
              % (path or ''), file=sys.stderr)
        return False
    if mode != 'on':
        raise ValueError('--identity must be auto, on or off, got %r' % (mode,))
    from .graph import _checkpoint_or_synthetic
    _checkpoint_or_synthetic('face network (facenet_path / --facenet_ckpt; the reference downloads facenet_pytorch vggface2 weights)', path)
    return True
