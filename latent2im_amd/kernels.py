"""Python call wrappers for the streaming kernels of libl2i_hip.so (include/l2i.h).  Tensors in, tensors out;
all GPU float32 contiguous; no autograd here (see op/ and the network modules for the differentiable forms)."""
import torch

from . import _lib
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU  # noqa: F401
from ._lib import LINEAR_LRELU, LINEAR_NONE, LINEAR_WALK  # noqa: F401

SQRT2 = 2 ** 0.5


def fused_bias_act(x, b, ref, act, grad, alpha, scale, out=None):
    """Reference signature fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)
    (op/fused_bias_act.cpp:11-21); empty tensors / None mean "absent"."""
    x = x.contiguous()
    b = None if (b is None or b.numel() == 0) else b.contiguous()
    ref = None if (ref is None or ref.numel() == 0) else ref.contiguous()
    y = torch.empty_like(x) if out is None else out
    step_b = 1
    for i in range(2, x.dim()):
        step_b *= x.shape[i]
    size_b = b.numel() if b is not None else 0
    if ref is not None:
        assert ref.shape == x.shape
    _lib.call('l2i_fused_bias_act_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(b), _lib.fptr(ref), x.numel(),
              step_b, size_b, int(act), int(grad), float(alpha), float(scale))
    return y


def upfirdn2d_out_hw(h, w, kh, kw, up, down, pad):
    px0, px1, py0, py1 = pad
    return (h * up[1] + py0 + py1 - kh) // down[1] + 1, (w * up[0] + px0 + px1 - kw) // down[0] + 1


def upfirdn2d(x, kernel, up=(1, 1), down=(1, 1), pad=(0, 0, 0, 0), noise=None, noise_w=0.0, bias=None, addend=None,
              act=ACT_NONE, slope=0.2, gain=1.0, out=None, mask=None, mask_vals=(1.0, 0.0), mask2=None, mask2_vals=(1.0, 0.0), out2=None):
    """x [N, C, H, W]; up/down = (x, y); pad = (x0, x1, y0, y1) as in op/upfirdn2d.cpp:12-23.  Optional fused
    epilogue: act(fir(x) + noise*noise_w + bias[c] + addend) * gain, then [r5] * (mask > 0 ? mask_vals[0] : mask_vals[1]) (mask shaped like the output).
    With ``mask2`` (shaped like the output) the launch writes a second map y2 = y * (mask2 > 0 ? mask2_vals[0] : mask2_vals[1]) and returns (y, y2)
    (l2i_upfirdn2d_dual_f32)."""
    x = x.contiguous()
    n, c, h, w = x.shape
    kh, kw = kernel.shape
    oh, ow = upfirdn2d_out_hw(h, w, kh, kw, up, down, pad)
    y = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32) if out is None else out
    assert y.shape == (n, c, oh, ow), (y.shape, (n, c, oh, ow))
    if addend is not None:
        assert addend.shape == y.shape
    if mask2 is not None:
        assert mask2.shape == y.shape and (mask is None or mask.shape == y.shape)
        y2 = torch.empty_like(y) if out2 is None else out2
        assert y2.shape == y.shape
        _lib.call('l2i_upfirdn2d_dual_f32', _lib.fptr(y), _lib.fptr(y2), _lib.fptr(mask2.contiguous()), float(mask2_vals[0]), float(mask2_vals[1]),
                  _lib.fptr(x), _lib.fptr(kernel.contiguous()), n * c, h, w, kh, kw,
                  up[0], up[1], down[0], down[1], pad[0], pad[1], pad[2], pad[3], c,
                  _lib.fptr(noise), float(noise_w), _lib.fptr(bias), _lib.fptr(addend),
                  int(act), float(slope), float(gain), _lib.fptr(None if mask is None else mask.contiguous()), float(mask_vals[0]), float(mask_vals[1]))
        return y, y2
    if mask is not None:
        assert mask.shape == y.shape
        _lib.call('l2i_upfirdn2d_masked_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(kernel.contiguous()), n * c, h, w, kh, kw,
                  up[0], up[1], down[0], down[1], pad[0], pad[1], pad[2], pad[3], c,
                  _lib.fptr(noise), float(noise_w), _lib.fptr(bias), _lib.fptr(addend),
                  int(act), float(slope), float(gain), _lib.fptr(mask.contiguous()), float(mask_vals[0]), float(mask_vals[1]))
        return y
    _lib.call('l2i_upfirdn2d_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(kernel.contiguous()), n * c, h, w, kh, kw,
              up[0], up[1], down[0], down[1], pad[0], pad[1], pad[2], pad[3], c,
              _lib.fptr(noise), float(noise_w), _lib.fptr(bias), _lib.fptr(addend),
              int(act), float(slope), float(gain))
    return y


def torgb_fwd(x, wmod, bias):
    """x [B,C,H,W], wmod [B,3,C], bias [3] -> rgb [B,3,H,W]."""
    b, c, h, w = x.shape
    rgb = torch.empty(b, 3, h, w, device=x.device, dtype=torch.float32)
    _lib.call('l2i_torgb_fwd_f32', _lib.fptr(rgb), _lib.fptr(x), _lib.fptr(wmod.contiguous()), _lib.fptr(bias), b, c,
              h * w)
    return rgb


def sg2_act_bwd(y, gin=None, gin_scale=None, grgb=None, wmod_rgb=None, bias=None, noise=None, noise_w=0.0,
                slope=0.2, gain=SQRT2, want_rgb_red=True, red=None, red_rgb=None, red_q=None):
    """Fused StyledConv elementwise backward (see l2i.h).  Returns (dz, red_dz_z [B,C], red_x_grgb [B,C,3] or None).  ``red`` / ``red_rgb`` /
    ``red_q`` ([r5] [B*C]: sum_p gin * y, the NEXT layer's style gradient): ZEROED destination buffers of the reductions (views of one buffer zeroed once per backward pass); allocated here when absent."""
    b, c, h, w = y.shape
    dz = torch.empty_like(y)
    if red is None:
        red = torch.zeros(b, c, device=y.device, dtype=torch.float32)
    if red_rgb is None and grgb is not None and want_rgb_red:
        red_rgb = torch.zeros(b, c, 3, device=y.device, dtype=torch.float32)
    if grgb is None or not want_rgb_red:
        red_rgb = None
    _lib.call('l2i_sg2_act_bwd_f32', _lib.fptr(dz), _lib.fptr(gin), _lib.fptr(gin_scale), _lib.fptr(grgb),
              _lib.fptr(wmod_rgb), _lib.fptr(y), _lib.fptr(bias), _lib.fptr(noise),
              float(noise_w), float(slope), float(gain), _lib.fptr(red), _lib.fptr(red_rgb), _lib.fptr(red_q),
              b, c, h * w)
    return dz, red, red_rgb


def dot_reduce(a, b=None, out=None):
    """a, b [..., P] viewed as [rows, cols] with cols = prod(last 2 dims) for 4-D maps: returns sum over pixels.  ``out``: a ZEROED
    contiguous destination of ``rows`` floats (a view of a buffer zeroed once per backward pass); allocated here when absent."""
    if a.dim() == 4:
        rows, cols = a.shape[0] * a.shape[1], a.shape[2] * a.shape[3]
        shape = a.shape[:2]
    else:
        rows, cols = a.shape[0], a.numel() // a.shape[0]
        shape = (rows,)
    if out is None:
        out = torch.zeros(rows, device=a.device, dtype=torch.float32)
    assert out.numel() == rows and out.is_contiguous()
    _lib.call('l2i_dot_reduce_f32', _lib.fptr(out), _lib.fptr(a), _lib.fptr(b), rows, cols)
    return out.reshape(shape)


def maxpool2d_fwd(x, k, s, pad):
    n, c, h, w = x.shape
    oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    y = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32)
    idx = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.uint8)
    _lib.call('l2i_maxpool2d_fwd_f32', _lib.fptr(y), _lib.ptr(idx), _lib.fptr(x), n * c, h, w, k, s, pad, oh, ow)
    return y, idx


def maxpool2d_bwd(gy, idx, in_hw, k, s, pad):
    n, c, oh, ow = gy.shape
    gx = torch.empty(n, c, in_hw[0], in_hw[1], device=gy.device, dtype=torch.float32)
    _lib.call('l2i_maxpool2d_bwd_f32', _lib.fptr(gx), _lib.fptr(gy), _lib.ptr(idx), n * c, in_hw[0], in_hw[1], k, s,
              pad, oh, ow)
    return gx


def maxpool2x2_bwd_add_diff(gy, idx, a, b, coef, coef_dev=None):
    """maxpool(2,2) backward of ``gy`` plus coef*coef_dev*(b - a) on the pool's input, in one pass (VGG conv1_2 tap)."""
    n, c, oh, ow = gy.shape
    assert a.shape == b.shape == (n, c, 2 * oh, 2 * ow)
    gx = torch.empty_like(b)
    _lib.call('l2i_maxpool2x2_bwd_add_diff_f32', _lib.fptr(gx), _lib.fptr(gy), _lib.ptr(idx), _lib.fptr(a), _lib.fptr(b), float(coef),
              _lib.fptr(coef_dev), n * c, oh, ow)
    return gx


def sqdiff(a, b, coef=0.0, want_grad=False, coef_dev=None, want_sum=True):
    """sum((b-a)^2) as a 1-element tensor, and optionally coef*coef_dev*(b-a) (coef_dev: 1-element device tensor)."""
    s = torch.zeros(1, device=a.device, dtype=torch.float32) if want_sum else None
    g = torch.empty_like(b) if want_grad else None
    _lib.call('l2i_sqdiff_f32', _lib.fptr(s), _lib.fptr(g), _lib.fptr(a), _lib.fptr(b), a.numel(), float(coef),
              _lib.fptr(coef_dev))
    return s, g


def gram_slices(B, C, HW):
    """How many HW slices l2i_gram_loss_f32 is launched with: whole 256-pixel chunks, two chunks a slice where the map has them, and no
    more slices than fill the chip about three times over with B * (tile pairs) blocks each.  A function of the shape alone: the Gram of a
    target and of an image of the same shape are summed in the same order."""
    t = C // 32
    chunks = -(-HW // 256)
    n = max(1, min(chunks, 768 // max(1, B * t * (t + 1) // 2), max(1, chunks // 2)))
    sl = -(-(-(-HW // n)) // 256) * 256
    return -(-HW // sl)


def gram_loss(c, target=None, loss=None):
    """l2i_gram_loss_f32: c [B, C, H, W] (or [B, C, HW]), a tap's pre-ReLU conv output -> G [B, C, C] = relu(c) relu(c)^T / (C HW).  With
    ``target`` [B, C, C] returns (G, D, loss): D = G - target and loss [B] += C^2 * sum(D^2) (``loss``: the accumulator of the taps, zeros when
    absent).  Without it returns G alone."""
    b, ch = c.shape[:2]
    hw = c[0, 0].numel()
    t = ch // 32
    ns = gram_slices(b, ch, hw)
    g = torch.empty(b, ch, ch, device=c.device, dtype=torch.float32)
    ws = torch.empty(max(1, b * (t * (t + 1) // 2) * (1024 * ns + 1)), device=c.device, dtype=torch.float32)
    d = None
    if target is not None:
        assert tuple(target.shape) == (b, ch, ch), (target.shape, (b, ch, ch))
        d = torch.empty_like(g)
        if loss is None:
            loss = torch.zeros(b, device=c.device, dtype=torch.float32)
        assert loss.numel() == b
    _lib.call('l2i_gram_loss_f32', _lib.fptr(g), _lib.fptr(d), _lib.fptr(loss if target is not None else None), _lib.fptr(c), _lib.fptr(target),
              _lib.fptr(ws), b, ch, hw, ns)
    return g if target is None else (g, d, loss)


def gram_bwd(c, d, scale=None, out=None, accumulate=False, coef=None):
    """l2i_gram_bwd_f32: out (+)= coef * scale * (c > 0) * (d relu(c)); d [B, C, C] symmetric, coef = 4 C / HW (the gradient of gram_loss's
    term) when absent, ``scale`` a device tensor of 1 element (every sample) or B elements (one per sample).  ``accumulate`` adds into ``out``
    (the trunk gradient from the deeper taps)."""
    b, ch = c.shape[:2]
    hw = c[0, 0].numel()
    assert tuple(d.shape) == (b, ch, ch)
    assert out is not None or not accumulate
    if out is None:
        out = torch.empty_like(c)
    assert out.shape == c.shape
    assert scale is None or scale.numel() in (1, b), (scale.shape, b)
    per_sample = scale is not None and scale.numel() == b and b > 1
    _lib.call('l2i_gram_bwd_f32', _lib.fptr(out), _lib.fptr(c), _lib.fptr(d), _lib.fptr(scale), float(4.0 * ch / hw if coef is None else coef),
              b, ch, hw, int(bool(accumulate)), int(per_sample))
    return out


def axpby(a, b=None, alpha=1.0, beta=1.0, out=None):
    y = torch.empty_like(a) if out is None else out
    _lib.call('l2i_axpby_f32', _lib.fptr(y), _lib.fptr(a), _lib.fptr(b), float(alpha), float(beta), a.numel())
    return y


def relu_mask(g, ref):
    y = torch.empty_like(g)
    _lib.call('l2i_relu_mask_f32', _lib.fptr(y), _lib.fptr(g), _lib.fptr(ref), g.numel())
    return y


def pixelnorm_act(x, slope=0.2, eps=1e-8):
    """lrelu(x / sqrt(mean_c x^2 + eps), slope) on [B,C,...] (model_256.py:78-84 + the LeakyReLU(0.2) that follows; slope 1: PixelNorm alone)."""
    x = x.contiguous()
    y = torch.empty_like(x)
    hw = x.numel() // (x.shape[0] * x.shape[1])
    _lib.call('l2i_pixelnorm_act_f32', _lib.fptr(y), _lib.fptr(x), x.shape[0], x.shape[1], hw, float(eps), float(slope))
    return y


def pixelnorm_act_bwd(gy, x, slope=0.2, eps=1e-8):
    gy, x = gy.contiguous(), x.contiguous()
    assert gy.shape == x.shape
    dx = torch.empty_like(x)
    hw = x.numel() // (x.shape[0] * x.shape[1])
    _lib.call('l2i_pixelnorm_act_bwd_f32', _lib.fptr(dx), _lib.fptr(gy), _lib.fptr(x), x.shape[0], x.shape[1], hw, float(eps), float(slope))
    return dx


def upsample2x_nearest(x, scale=1.0):
    x = x.contiguous()
    n, c, h, w = x.shape
    y = torch.empty(n, c, 2 * h, 2 * w, device=x.device, dtype=torch.float32)
    _lib.call('l2i_upsample2x_nearest_f32', _lib.fptr(y), _lib.fptr(x), n * c, h, w, float(scale))
    return y


def pool2x2(x, scale=0.25):
    """scale * (sum of every 2x2 window): 0.25 = bilinear halving (align_corners=False), 1 = adjoint of the nearest 2x upsample."""
    x = x.contiguous()
    n, c, h, w = x.shape
    assert h % 2 == 0 and w % 2 == 0
    y = torch.empty(n, c, h // 2, w // 2, device=x.device, dtype=torch.float32)
    _lib.call('l2i_pool2x2_f32', _lib.fptr(y), _lib.fptr(x), n * c, h // 2, w // 2, float(scale))
    return y


def segmented_matvec(out, inp, w, segs, block_seg, nblocks, B, in2=None, bias=None, e1=None, e2=None, wmod=None, wrgb=None):
    """l2i_segmented_matvec_f32 (include/l2i.h): every layer's style-dependent vectors of one kind in one launch.  ``segs`` / ``block_seg``
    are device tensors holding the segment tables (latent2im_amd/generator.py:_ModPlan)."""
    _lib.call('l2i_segmented_matvec_f32', _lib.fptr(out), _lib.fptr(inp), _lib.fptr(in2), _lib.fptr(w), _lib.fptr(bias), _lib.fptr(e1), _lib.fptr(e2),
              _lib.fptr(wmod), _lib.fptr(wrgb), _lib.ptr(segs), _lib.ptr(block_seg), int(nblocks), int(B))
    return out



def linear_rows(x, w, b, epi=LINEAR_NONE, slope=0.2, res=None, a=None, out=None):
    """l2i_linear_rows_f32: y [B, N] = epi(x [B, K] w^T + b), w [N, K] as nn.Linear holds it.  LINEAR_LRELU: LeakyReLU(slope); LINEAR_WALK: the
    walk's tail res + a[:, None] * (...) with res [B, N] and a [B]."""
    B, Kd = x.shape
    N = w.shape[0]
    assert tuple(w.shape) == (N, Kd) and b.numel() == N, (x.shape, w.shape, b.shape)
    if epi == LINEAR_WALK:
        assert tuple(res.shape) == (B, N) and a.numel() == B, (res.shape, a.shape)
    y = torch.empty(B, N, device=x.device, dtype=torch.float32) if out is None else out
    assert tuple(y.shape) == (B, N)
    _lib.call('l2i_linear_rows_f32', _lib.fptr(y), _lib.fptr(x), _lib.fptr(w), _lib.fptr(b), _lib.fptr(res), _lib.fptr(a), B, Kd, N, int(epi), float(slope))
    return y


def linear_rows_slices(N):
    """How many row slices l2i_linear_rows_bwd_f32 is launched with: 16 rows a slice (one wave each per 256 columns — 256 waves on a 1024 x 1024
    layer).  A function of the shape alone: equal inputs give equal bits."""
    return max(1, N // 16)


def linear_rows_bwd(g, x, w, epi=LINEAR_NONE, slope=0.2, y=None, a=None, want_gx=True, gx_add=None, gw=None, gb=None, gx=None, slices=None):
    """l2i_linear_rows_bwd_f32: one pass over a layer's [N, K] weights.  g [B, N] the gradient at the layer's output, g' = g * (y > 0 ? 1 : slope)
    (LINEAR_LRELU, y the activated output), a[:, None] * g (LINEAR_WALK) or g.  Returns (gw [N, K], gb [N], gx [B, K] or None); gx_add [B, K] is
    added to gx (the residual path).  gw / gb / gx: destinations, allocated when absent."""
    B, N = g.shape
    Kd = x.shape[1]
    assert x.shape[0] == B and tuple(w.shape) == (N, Kd), (g.shape, x.shape, w.shape)
    assert y is None or tuple(y.shape) == (B, N)
    assert a is None or a.numel() == B
    slices = linear_rows_slices(N) if slices is None else int(slices)
    gw = torch.empty(N, Kd, device=g.device, dtype=torch.float32) if gw is None else gw
    gb = torch.empty(N, device=g.device, dtype=torch.float32) if gb is None else gb
    ws = None
    if want_gx:
        gx = torch.empty(B, Kd, device=g.device, dtype=torch.float32) if gx is None else gx
        assert gx_add is None or tuple(gx_add.shape) == (B, Kd)
        ws = torch.empty(slices, B, Kd, device=g.device, dtype=torch.float32) if slices > 1 else None
    else:
        assert gx_add is None
        gx = None
    assert tuple(gw.shape) == (N, Kd) and gb.numel() == N
    _lib.call('l2i_linear_rows_bwd_f32', _lib.fptr(gw), _lib.fptr(gb), _lib.fptr(gx), _lib.fptr(ws), _lib.fptr(gx_add), _lib.fptr(g), _lib.fptr(y), _lib.fptr(a),
              _lib.fptr(x), _lib.fptr(w), B, Kd, N, int(epi), float(slope), slices)
    return gw, gb, gx


def face_resize(x, xbounds, xcoef, ybounds, ycoef):
    """l2i_face_resize_f32: x [B, C, H, W] fp32 in [-1, 1] -> clip_ims + PIL's resize to [B, C, OH, OW] (fp32 bytes 0..255).  The int32
    tables [O, 2] / [O, k] of each axis are PIL's (facenet.resize_tables), on the device."""
    x = x.contiguous()
    b, c, h, w = x.shape
    oh, ow = ybounds.shape[0], xbounds.shape[0]
    assert xcoef.shape[0] == ow and ycoef.shape[0] == oh and all(t.dtype == torch.int32 and t.is_contiguous() for t in (xbounds, xcoef, ybounds, ycoef))
    y = torch.empty(b, c, oh, ow, device=x.device, dtype=torch.float32)
    _lib.call('l2i_face_resize_f32', _lib.fptr(y), _lib.fptr(x), b * c, h, w, oh, ow, _lib.ptr(xbounds), _lib.ptr(xcoef), xcoef.shape[1],
              _lib.ptr(ybounds), _lib.ptr(ycoef), ycoef.shape[1])
    return y


def face_head(feat, w_t, bias, npairs=0):
    """l2i_face_head_f32: feat [B, C, h, w] -> (unit embeddings [B, E], float64 cosine distances [npairs] of rows (p, p + npairs), or None).
    w_t [C, E] / bias [E]: last_linear with last_bn folded in (facenet.InceptionResnetV1)."""
    feat = feat.contiguous()
    b, c = feat.shape[:2]
    e = w_t.shape[1]
    assert w_t.shape[0] == c and bias.numel() == e
    emb = torch.empty(b, e, device=feat.device, dtype=torch.float32)
    dist = torch.empty(npairs, device=feat.device, dtype=torch.float64) if npairs else None
    _lib.call('l2i_face_head_f32', _lib.fptr(emb), _lib.ptr(dist), _lib.fptr(feat), _lib.fptr(w_t), _lib.fptr(bias), b, c,
              feat[0, 0].numel(), e, int(npairs))
    return emb, dist


def _resize_tables_ok(n_b, n_c, *tables):
    xb, xc, yb, yc = tables
    assert xb.shape[0] == xc.shape[0] == n_b and yb.shape[0] == yc.shape[0] == n_c, ([tuple(t.shape) for t in tables], n_b, n_c)
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in tables)


def face_resize_lin(x, xbounds, xcoef, ybounds, ycoef):
    """l2i_face_resize_lin_f32: x [B, C, H, W] fp32 -> Ry clip(((x + 1) 0.5) 255, 0, 255) Rx^T, [B, C, OH, OW] fp32 (the taps of face_resize
    without the byte intermediate, the rounding and the clips); the tables of face_resize."""
    x = x.contiguous()
    b, c, h, w = x.shape
    oh, ow = ybounds.shape[0], xbounds.shape[0]
    _resize_tables_ok(ow, oh, xbounds, xcoef, ybounds, ycoef)
    y = torch.empty(b, c, oh, ow, device=x.device, dtype=torch.float32)
    _lib.call('l2i_face_resize_lin_f32', _lib.fptr(y), _lib.fptr(x), b * c, h, w, oh, ow, _lib.ptr(xbounds), _lib.ptr(xcoef), xcoef.shape[1],
              _lib.ptr(ybounds), _lib.ptr(ycoef), ycoef.shape[1])
    return y


def face_resize_lin_bwd(gy, x, ixbounds, ixcoef, iybounds, iycoef):
    """l2i_face_resize_lin_bwd_f32: the adjoint of face_resize_lin at x, gy [B, C, OH, OW] -> gx like x.  The inverse tables of each axis
    (facenet.inverse_tables): int32 [in, 2] = (first output, count) and [in, k] coefficients per input pixel, on the device."""
    x, gy = x.contiguous(), gy.contiguous()
    b, c, h, w = x.shape
    oh, ow = gy.shape[2], gy.shape[3]
    assert gy.shape[:2] == x.shape[:2]
    _resize_tables_ok(w, h, ixbounds, ixcoef, iybounds, iycoef)
    gx = torch.empty_like(x)
    _lib.call('l2i_face_resize_lin_bwd_f32', _lib.fptr(gx), _lib.fptr(gy), _lib.fptr(x), b * c, h, w, oh, ow, _lib.ptr(ixbounds), _lib.ptr(ixcoef),
              ixcoef.shape[1], _lib.ptr(iybounds), _lib.ptr(iycoef), iycoef.shape[1])
    return gx


def face_head_bwd(feat, w_t, bias, v, g_dist):
    """l2i_face_head_bwd_f32: d sum_b g_dist[b] (1 - cos(e[b], v[b])) / d feat, with e = face_head(feat)'s embedding and v [B, E] a constant."""
    feat = feat.contiguous()
    b, c = feat.shape[:2]
    e = w_t.shape[1]
    assert w_t.shape[0] == c and bias.numel() == e and tuple(v.shape) == (b, e) and g_dist.numel() == b
    g_feat = torch.empty_like(feat)
    _lib.call('l2i_face_head_bwd_f32', _lib.fptr(g_feat), _lib.fptr(feat), _lib.fptr(w_t), _lib.fptr(bias), _lib.fptr(v.contiguous()),
              _lib.fptr(g_dist.contiguous()), b, c, feat[0, 0].numel(), e)
    return g_feat


def panels_grid_hw(rows, cols, h, w, pad):
    """(GH, GW) of one l2i_panels_u8 grid: imgrid's size, every tile padded on its bottom and right and the last gutter cropped."""
    return rows * (h + pad) - pad, cols * (w + pad) - pad


def panels_u8(x, tile_src, G, rows, cols, pad=0, fill=0, out=None):
    """l2i_panels_u8: x [N, C, H, W] fp32 (C in {1, 3}) -> G channel-last uint8 grids [G, GH, GW, C] of rows x cols tiles on the device, one
    launch: clip_ims (the reference's float32 quantiser, bit for bit) and imgrid (``pad`` pixels of ``fill`` below and right of every tile, the
    last gutter cropped).  tile_src: int32 [G * rows * cols] on the device (or a sequence of ints), the image of each tile, row-major over
    (grid, tile row, tile column); an index outside [0, N) is an empty tile of ``fill``.  ``out``: a contiguous uint8 tensor of that size, at any
    byte alignment; every byte of it is written."""
    x = x.contiguous()
    n, c, h, w = x.shape
    if not torch.is_tensor(tile_src):
        tile_src = torch.tensor(list(tile_src), dtype=torch.int32, device=x.device)
    assert tile_src.dtype == torch.int32 and tile_src.numel() == G * rows * cols
    gh, gw = panels_grid_hw(rows, cols, h, w, pad)
    if out is None:
        out = torch.empty(G, gh, gw, c, device=x.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.numel() == G * gh * gw * c
    _lib.call('l2i_panels_u8', _lib.ptr(out), _lib.fptr(x), _lib.ptr(tile_src), int(G), int(rows), int(cols), c, h, w, int(pad), int(fill), n)
    return out
