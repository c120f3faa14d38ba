"""Python call wrappers for the streaming kernels of the 16-bit path (csrc/l2i_stream_h8.hip, l2i_gram_h8.hip, l2i_pggan_h8.hip, l2i_train_h8.hip; include/l2i.h): bf16 tensors in the
channel-blocked h8 layout [B, C/8, H, W, 8] in, out; fp32 for images, noise, bias, per-sample vectors and reductions.  No autograd here."""
import ctypes

import torch

from . import _lib
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU  # noqa: F401

BF = torch.bfloat16
H8_DTYPES = (torch.bfloat16, torch.float16)


def h8_dtype():
    """Element type of the 16-bit path's h8 maps: bf16 (conv.PRECISION 'bf16') or IEEE fp16 ('f16', [r5])."""
    from . import conv
    return conv.h8_dtype()


def separable(kernel):
    """(k1y, k1x) with kernel == outer(k1y, k1x) (to float32 rounding), or None: computed ONCE from a host copy of a constant FIR kernel (the
    networks do it at construction: [1,3,3,1] x [1,3,3,1] / 64 times the up-sampling gain) and handed to ``upfirdn2d(..., sep=...)``, which then
    takes the register-streaming separable kernel; nothing is read back from the device per call."""
    import numpy as np
    k = np.asarray(kernel.detach().float().cpu().numpy() if torch.is_tensor(kernel) else kernel, dtype=np.float64)
    if k.shape != (4, 4):
        return None
    i, j = divmod(int(np.abs(k).argmax()), 4)
    if k[i, j] == 0:
        return None
    ky, kx = k[:, j] / k[i, j], k[i, :].copy()
    if not np.allclose(np.outer(ky, kx), k, rtol=1e-6, atol=0):
        return None
    return [float(v) for v in ky], [float(v) for v in kx]


def _h8(t):
    assert t.dtype in H8_DTYPES and t.dim() == 5 and t.shape[4] == 8 and t.is_contiguous(), (t.dtype, t.shape)
    return _lib.ptr(t)


def cast_to_h8(x, cpad=None, dtype=None):
    """fp32 NCHW -> 16-bit h8 with ``cpad`` channels (zero filled above C)."""
    B, C, H, W = x.shape
    cpad = (C + 7) // 8 * 8 if cpad is None else cpad
    dtype = dtype or h8_dtype()
    y = torch.empty(B, cpad // 8, H, W, 8, device=x.device, dtype=dtype)
    _lib.call('l2i_cast_f32_to_h8', _lib.ptr(y), _lib.fptr(x.contiguous()), B, C, cpad, H * W, dtype=dtype)
    return y


def cast_from_h8(t, channels=None):
    B, G8, H, W, _ = t.shape
    C = G8 * 8 if channels is None else channels
    y = torch.empty(B, C, H, W, device=t.device, dtype=torch.float32)
    _lib.call('l2i_cast_h8_to_f32', _lib.fptr(y), _h8(t), B, C, G8 * 8, H * W, dtype=t.dtype)
    return y


def upfirdn2d(x, kernel, up=1, down=1, pad=(0, 0, 0, 0), noise=None, noise_w=0.0, bias=None, act=ACT_NONE, slope=0.2, gain=1.0, mask=None, mask_vals=(1.0, 0.0),
              addend=None, sep=None, mask_bits=False):
    """x h8; pad = (x0, x1, y0, y1) as in op/upfirdn2d.cpp:12-23; optional fused epilogue act(fir(x) + noise*noise_w + bias[c]) * gain, then
    * (mask > 0 ? mask_vals[0] : mask_vals[1]) and + addend (both h8, shaped like the output).  ``sep`` = separable(kernel) (4x4, no resampling): the
    register-streaming separable kernel."""
    B, G8, H, W, _ = x.shape
    kh, kw = kernel.shape
    oh = (H * up + pad[2] + pad[3] - kh) // down + 1
    ow = (W * up + pad[0] + pad[1] - kw) // down + 1
    y = torch.empty(B, G8, oh, ow, 8, device=x.device, dtype=x.dtype)
    assert (mask is None or tuple(mask.shape) == (tuple(y.shape[:4]) if mask_bits else tuple(y.shape))) and (addend is None or addend.shape == y.shape)
    use_sep = sep is not None and kh == 4 and kw == 4            # the library picks its separable register-streaming kernels (no resampling, down 2, up 2) where they apply
    k1y = (ctypes.c_float * 4)(*sep[0]) if use_sep else None
    k1x = (ctypes.c_float * 4)(*sep[1]) if use_sep else None
    _lib.call('l2i_upfirdn2d_h8', _lib.ptr(y), _h8(x), _lib.fptr(kernel.contiguous()), B * G8, G8 * 8, H, W, kh, kw, up, down, pad[0], pad[1], pad[2], pad[3],
              _lib.fptr(noise), float(noise_w), _lib.fptr(bias), int(act), float(slope), float(gain), None if mask is None else (_lib.ptr(mask) if mask_bits else _h8(mask)),
              float(mask_vals[0]), float(mask_vals[1]), None if addend is None else _h8(addend), k1y, k1x, int(bool(mask_bits)), dtype=x.dtype)
    return y


def torgb_fwd(x, wmod, bias):
    """x h8 [B,C/8,H,W,8], wmod [B,3,C] fp32, bias [3] -> rgb fp32 [B,3,H,W]."""
    B, G8, H, W, _ = x.shape
    rgb = torch.empty(B, 3, H, W, device=x.device, dtype=torch.float32)
    _lib.call('l2i_torgb_fwd_h8', _lib.fptr(rgb), _h8(x), _lib.fptr(wmod.contiguous()), _lib.fptr(bias), B, G8 * 8, H * W, dtype=x.dtype)
    return rgb


def sg2_act_bwd(y, gin, gin_scale, grgb, wmod_rgb, bias, noise, noise_w, slope, gain, red, red_rgb=None, red_q=None):
    """Fused StyledConv elementwise backward on h8 maps (l2i_sg2_act_bwd_h8): returns dz (h8); ``red`` [B,C] / ``red_rgb`` [B,C,3] / ``red_q`` ([r5] [B*C]: sum_p gin * y, the next layer's style gradient) are ZEROED fp32 buffers."""
    B, G8, H, W, _ = y.shape
    dz = torch.empty_like(y)
    _lib.call('l2i_sg2_act_bwd_h8', _lib.ptr(dz), None if gin is None else _h8(gin), _lib.fptr(gin_scale), _lib.fptr(grgb), _lib.fptr(wmod_rgb), _h8(y), _lib.fptr(bias),
              _lib.fptr(noise), float(noise_w), float(slope), float(gain), _lib.fptr(red), _lib.fptr(red_rgb), _lib.fptr(red_q), B, G8 * 8, H * W, dtype=y.dtype)
    return dz


def dot_reduce(a, b=None, out=None):
    """out[b,c] += sum_p a*b on h8 maps; ``out``: zeroed fp32 [B*C] (allocated when absent).  Returns [B, C]."""
    B, G8, H, W, _ = a.shape
    if out is None:
        out = torch.zeros(B * G8 * 8, device=a.device, dtype=torch.float32)
    _lib.call('l2i_dot_reduce_h8', _lib.fptr(out), _h8(a), None if b is None else _h8(b), B, G8 * 8, H * W, dtype=a.dtype)
    return out.view(B, G8 * 8)


def maxpool2d_fwd(x, k, s, pad, relu=False):
    B, G8, H, W, _ = x.shape
    oh, ow = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    y = torch.empty(B, G8, oh, ow, 8, device=x.device, dtype=x.dtype)
    idx = torch.empty(B, G8, oh, ow, 8, device=x.device, dtype=torch.uint8)
    _lib.call('l2i_maxpool2d_fwd_h8', _lib.ptr(y), _lib.ptr(idx), _h8(x), B * G8, H, W, k, s, pad, oh, ow, int(relu), dtype=x.dtype)
    return y, idx


def maxpool2d_bwd(gy, idx, in_hw, k, s, pad, a=None, b=None, coef=0.0, coef_dev=None):
    """Pool backward on h8 maps; a / b (h8, input-sized): + coef * coef_dev[0] * (b - a) in the same pass."""
    B, G8, oh, ow, _ = gy.shape
    gx = torch.empty(B, G8, in_hw[0], in_hw[1], 8, device=gy.device, dtype=gy.dtype)
    _lib.call('l2i_maxpool2d_bwd_h8', _lib.ptr(gx), _h8(gy), _lib.ptr(idx), None if a is None else _h8(a), None if b is None else _h8(b), float(coef), _lib.fptr(coef_dev),
              B * G8, in_hw[0], in_hw[1], k, s, pad, oh, ow, dtype=gy.dtype)
    return gx


def sqdiff(a, b, coef=0.0, want_grad=False, coef_dev=None, want_sum=True):
    s = torch.zeros(1, device=a.device, dtype=torch.float32) if want_sum else None
    g = torch.empty_like(b) if want_grad else None
    _lib.call('l2i_sqdiff_h8', _lib.fptr(s), None if g is None else _lib.ptr(g), _h8(a), _h8(b), a.numel() // 8, float(coef), _lib.fptr(coef_dev), dtype=a.dtype)
    return s, g


def gram_loss(c, target=None, loss=None):
    """l2i_gram_loss_h8: kernels.gram_loss on an h8 tap c [B, C/8, H, W, 8] (pre-ReLU).  G, ``target``, D [B, C, C] and ``loss`` [B] are fp32;
    the slicing is kernels.gram_slices, a function of the shape alone, so a target's Grams and an image's are summed in the same order."""
    from .kernels import gram_slices
    b, g8, h, w, _ = c.shape
    ch, hw = g8 * 8, h * w
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
    _lib.call('l2i_gram_loss_h8', _lib.fptr(g), _lib.fptr(d), _lib.fptr(loss if target is not None else None), _h8(c), _lib.fptr(target),
              _lib.fptr(ws), b, ch, hw, ns, dtype=c.dtype)
    return g if target is None else (g, d, loss)


def gram_bwd(c, d, scale=None, out=None, accumulate=False, coef=None):
    """l2i_gram_bwd_h8: kernels.gram_bwd with c and ``out`` in h8: out (+)= coef * scale * (c > 0) * (d relu(c)); d [B, C, C] fp32 is scaled by
    coef * scale in fp32 before it is rounded to the element type.  ``accumulate`` adds into ``out`` (the trunk gradient from the deeper taps)."""
    b, g8, h, w, _ = c.shape
    ch, hw = g8 * 8, h * w
    assert tuple(d.shape) == (b, ch, ch)
    assert out is not None or not accumulate
    if out is None:
        out = torch.empty_like(c)
    assert out.shape == c.shape and out.dtype == c.dtype
    assert scale is None or scale.numel() in (1, b), (scale.shape, b)
    per_sample = scale is not None and scale.numel() == b and b > 1
    _lib.call('l2i_gram_bwd_h8', _h8(out), _h8(c), _lib.fptr(d), _lib.fptr(scale), float(4.0 * ch / hw if coef is None else coef),
              b, ch, hw, int(bool(accumulate)), int(per_sample), dtype=c.dtype)
    return out


def pixelnorm_act(x, slope, up=1, low=False, eps=1e-8):
    """l2i_pixelnorm_act_h8: lrelu(x / sqrt(mean_c x^2 + eps), slope) on an h8 map (PGGAN's PixelNorm + LeakyReLU).  ``up`` = 2 writes every result
    to its four positions of the [B, C/8, 2H, 2W, 8] map (the nearest upsample that follows the block); ``low`` returns (y, the 1x map) from
    the same pass."""
    B, G8, H, W, _ = x.shape
    up = int(up)
    y = torch.empty(B, G8, max(up, 1) * H, max(up, 1) * W, 8, device=x.device, dtype=x.dtype)
    y_low = torch.empty_like(x) if low else None
    _lib.call('l2i_pixelnorm_act_h8', _lib.ptr(y), _lib.ptr(y_low), _h8(x), B, G8 * 8, H, W, float(eps), float(slope), up, dtype=x.dtype)
    return (y, y_low) if low else y


def pixelnorm_act_bwd(gy, x, slope, pool=1, addend=None, eps=1e-8):
    """l2i_pixelnorm_act_bwd_h8: dx of the above given the saved pre-norm map ``x``.  ``pool`` = 2: ``gy`` is the [B, C/8, 2H, 2W, 8] gradient of the
    upsampled map, its 2x2 windows are summed while it is read; ``addend`` (h8, shaped like x) is added to that sum."""
    B, G8, H, W, _ = x.shape
    pool = int(pool)
    assert tuple(gy.shape) == (B, G8, max(pool, 1) * H, max(pool, 1) * W, 8) and gy.dtype == x.dtype, (gy.shape, x.shape, pool)
    assert addend is None or (addend.shape == x.shape and addend.dtype == x.dtype)
    dx = torch.empty_like(x)
    _lib.call('l2i_pixelnorm_act_bwd_h8', _lib.ptr(dx), _h8(gy), _h8(x), None if addend is None else _h8(addend), B, G8 * 8, H, W, float(eps), float(slope), pool,
              dtype=x.dtype)
    return dx


def add_zero_insert(y, c, mask=None):
    """y[.., 2oy, 2ox, :] += c[.., oy, ox, :] * (mask[.., 2oy, 2ox, :] > 0 if a mask is given) in place (h8)."""
    B, G8, H, W, _ = y.shape
    _lib.call('l2i_add_zero_insert_h8', _h8(y), _h8(c), None if mask is None else _h8(mask), B * G8, H, W, c.shape[2], c.shape[3], dtype=y.dtype)
    return y


def mask_mul(g, ref, pos=1.0, neg=0.0):
    """g * (ref > 0 ? pos : neg) on h8 maps; ``ref`` may be the map or ([r6]) its sign plane (uint8 [B, C/8, H, W]: l2i_conv_params::mask_out)."""
    y = torch.empty_like(g)
    if ref.dtype == torch.uint8:
        assert tuple(ref.shape) == tuple(g.shape[:4]) and ref.is_contiguous()
        _lib.call('l2i_mask_mul_bits_h8', _lib.ptr(y), _h8(g), _lib.ptr(ref), float(pos), float(neg), g.numel() // 8, dtype=g.dtype)
        return y
    _lib.call('l2i_mask_mul_h8', _lib.ptr(y), _h8(g), _h8(ref), float(pos), float(neg), g.numel() // 8, dtype=g.dtype)
    return y


RANGE_WORDS, RANGE_ZEROS, RANGE_MAX, RANGE_CALLS, RANGE_N = 260, 256, 257, 258, 259      # L2I_RANGE_* of include/l2i.h
RANGE_KINDS = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}


def range_stats(t, row):
    """l2i_range_stats: ADD the octave histogram, zero count, largest finite magnitude, call and element counts of every stored element of ``t``
    (contiguous fp16 / bf16 / fp32) to ``row``, RANGE_WORDS contiguous int64 words on the device, on the current stream.  No host read."""
    kind = RANGE_KINDS.get(t.dtype)
    if kind is None:
        raise _lib.L2IError('range_stats reads float16, bfloat16 or float32 tensors, got %s' % t.dtype)
    if row.dtype != torch.int64 or row.numel() != RANGE_WORDS:
        raise _lib.L2IError('range_stats adds to %d int64 words, got %s x %d' % (RANGE_WORDS, row.dtype, row.numel()))
    _lib.call('l2i_range_stats', _lib.ptr(row), _lib.ptr(t), t.numel(), kind)
    return row


def modulate_planes(w32, s, dtype=None):
    """w32: fp32 weights in plane order [Cin/16, KK, 2, CoutP, 8] (conv.pack_weight_h8_f32); s [B, Cin] fp32 -> 16-bit planes [B, Cin/16, KK, 2, CoutP, 8]
    (int16 view) in the element type of the path (or ``dtype``)."""
    dtype = dtype or h8_dtype()
    B = s.shape[0]
    c16, kk, _, coutp, _ = w32.shape
    assert s.shape[1] == c16 * 16 and s.is_contiguous()
    planes = torch.empty((B,) + tuple(w32.shape), device=w32.device, dtype=torch.int16)
    _lib.call('l2i_modulate_planes_h8', _lib.ptr(planes), _lib.fptr(w32), _lib.fptr(s), B, c16 * 16, c16 * 16, kk, coutp, dtype=dtype)
    return planes


class ModulatePlan:
    """[r5] The weight planes of EVERY modulated conv of a generator pass in one launch (l2i_modulate_planes_multi_h8): ``w32s`` = the layers' fp32
    weights in plane order (conv.pack_weight_h8_f32), ``s_offsets`` = rows before each layer's block in the per-layer-contiguous scale buffer
    ([layer][B][C], generator._ModPlan: s_all for the forward, demod_all for the backward).  ``run(scales, B)`` returns one int16 view
    [B, Cin/16, KK, 2, CoutP, 8] per layer of one buffer."""
    BLOCK_SLOTS = 256 * 8                      # slots a block handles at most per pass of its grid-stride loop

    def __init__(self, w32s, s_offsets, device, widths=None):
        self.shapes = [tuple(w.shape) for w in w32s]
        if widths is not None:                   # rows of the scale buffer per layer: the kernel reads c16 * 16 scales per sample, like modulate_planes asserts
            for w, n in zip(w32s, widths):
                assert n == w.shape[0] * 16, 'scale row of %d entries for a weight plane set of %d padded input channels' % (n, w.shape[0] * 16)
        self.w32 = torch.cat([w.reshape(-1) for w in w32s]).contiguous().to(device)
        self.w_off = [0]
        for w in w32s[:-1]:
            self.w_off.append(self.w_off[-1] + w.numel())
        self.s_off = list(s_offsets)
        self.sps = [w.numel() // 8 for w in w32s]
        self.device = device
        self._tables = {}

    def _table(self, B):
        if B not in self._tables:
            rows, out_off, first = [], 0, 0
            for (c16, kk, _, coutp, _), w_off, s_off, sps in zip(self.shapes, self.w_off, self.s_off, self.sps):
                rows.append([w_off, s_off * B, out_off, sps, kk, coutp, c16 * 16, first])
                out_off += sps * B
                first += max(1, min((sps * B + self.BLOCK_SLOTS - 1) // self.BLOCK_SLOTS, 1024))
            self._tables[B] = (torch.tensor(rows, dtype=torch.int64).to(self.device), out_off, first)
        return self._tables[B]

    def run(self, scales, B, dtype=None):
        dtype = dtype or h8_dtype()
        table, slots, nblocks = self._table(B)
        planes = torch.empty(slots * 8, device=self.w32.device, dtype=torch.int16)
        _lib.call('l2i_modulate_planes_multi_h8', _lib.ptr(planes), _lib.fptr(self.w32), _lib.fptr(scales), _lib.ptr(table), len(self.shapes), B, nblocks, dtype=dtype)
        views, off = [], 0
        for shp, sps in zip(self.shapes, self.sps):
            views.append(planes[off * 8:(off + sps * B) * 8].view((B,) + shp))
            off += sps * B
        return views


# ---- training on h8 maps (csrc/l2i_train_h8.hip): the weight gradient and training-mode BatchNorm ---------------------------------------------------
def _twin(name, dtype):
    return getattr(_lib.load(), name + ('_f16' if dtype is torch.float16 else ''))


def wgrad_ws_bytes(b, cin, h, w, cout, oh, ow, k, stride, pad, dtype=None):
    """l2i_conv2d_wgrad_ws_h8: bytes of workspace l2i_conv2d_wgrad_h8 needs for the shape (host only); raises for a shape it refuses."""
    n = ctypes.c_int64(0)
    _lib.check(_twin('l2i_conv2d_wgrad_ws_h8', dtype)(ctypes.byref(n), b, cin, h, w, cout, oh, ow, k, stride, pad), 'l2i_conv2d_wgrad_ws_h8')
    return n.value


def bn_ws_bytes(b, c, hw, dtype=None):
    """l2i_bn_ws_h8: bytes of the float64 workspace of bn_stats / bn_bwd_reduce for the shape (host only)."""
    n = ctypes.c_int64(0)
    _lib.check(_twin('l2i_bn_ws_h8', dtype)(ctypes.byref(n), b, c, hw), 'l2i_bn_ws_h8')
    return n.value


def conv_wgrad(x, gy, k, stride, pad, out=None, ws=None, out_scale=1.0, out_scale_dev=None):
    """l2i_conv2d_wgrad_h8: dw [Cout, Cin, k, k] fp32 = out_scale * out_scale_dev[0] * sum gy * x over (b, pixel) of h8 maps x, gy; ``out`` is
    OVERWRITTEN; ``ws`` a float32 workspace of at least wgrad_ws_bytes (allocated when absent)."""
    b, gi, h, w, _ = x.shape
    _, go, oh, ow, _ = gy.shape
    cin, cout = gi * 8, go * 8
    assert gy.dtype == x.dtype and gy.shape[0] == b
    if ws is None:
        ws = torch.empty(wgrad_ws_bytes(b, cin, h, w, cout, oh, ow, k, stride, pad, x.dtype) // 4, device=x.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(cout, cin, k, k, device=x.device, dtype=torch.float32)
    assert out.numel() == cout * cin * k * k
    _lib.call('l2i_conv2d_wgrad_h8', _lib.fptr(out), _h8(x), _h8(gy), _lib.fptr(ws), ws.numel() * 4, float(out_scale), _lib.fptr(out_scale_dev), b, cin, h, w,
              cout, oh, ow, k, stride, pad, dtype=x.dtype)
    return out


WGRAD_IMG_SLICE_BYTES = 64 * 160 * 4      # L2I_WGRAD_IMG_SLICE_BYTES: the workspace of l2i_conv2d_wgrad_img_h8 per pixel slice


def wgrad_img_ws_bytes(b, h, w, dtype=None, cin=3, cout=64, k=7, stride=2, pad=3):
    """l2i_conv2d_wgrad_img_ws_h8: bytes of workspace the stem's weight gradient needs for a [b, 3, h, w] image (host only; = slices *
    WGRAD_IMG_SLICE_BYTES); raises for a shape it refuses."""
    n = ctypes.c_int64(0)
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    _lib.check(_twin('l2i_conv2d_wgrad_img_ws_h8', dtype)(ctypes.byref(n), b, cin, h, w, cout, oh, ow, k, stride, pad), 'l2i_conv2d_wgrad_img_ws_h8')
    return n.value


def conv_wgrad_img(x, gy, out=None, ws=None):
    """l2i_conv2d_wgrad_img_h8: dw [64, 3, 7, 7] fp32 = sum gy * x over (b, pixel) for the 7x7 / stride 2 / pad 3 stem: x the fp32 NCHW image (taken
    as the fp32 value it is), gy the h8 gradient of the conv's output; ``out`` is OVERWRITTEN, in the units of gy; fixed summation order; ``ws`` a
    float32 workspace of at least wgrad_img_ws_bytes (allocated when absent)."""
    b, cin, h, w = x.shape
    _, go, oh, ow, _ = gy.shape
    assert gy.shape[0] == b and x.dtype == torch.float32
    if ws is None:
        ws = torch.empty(wgrad_img_ws_bytes(b, h, w, gy.dtype) // 4, device=x.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(go * 8, cin, 7, 7, device=x.device, dtype=torch.float32)
    assert out.numel() == go * 8 * cin * 49
    _lib.call('l2i_conv2d_wgrad_img_h8', _lib.fptr(out), _lib.fptr(x), _h8(gy), _lib.fptr(ws), ws.numel() * 4, b, cin, h, w, go * 8, oh, ow, 7, 2, 3,
              dtype=gy.dtype)
    return out


def _bn_ws(x, ws):
    b, g8, h, w, _ = x.shape
    if ws is None:
        ws = torch.empty(bn_ws_bytes(b, g8 * 8, h * w, x.dtype) // 8, device=x.device, dtype=torch.float64)
    assert ws.dtype == torch.float64
    return ws


def bn_stats(x, sums, ws=None):
    """l2i_bn_stats_h8: sums [2, C] float64 (OVERWRITTEN) <- per-channel sum and sum of squares of the stored h8 map x."""
    b, g8, h, w, _ = x.shape
    ws = _bn_ws(x, ws)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (2, g8 * 8)
    _lib.call('l2i_bn_stats_h8', _lib.ptr(sums[0]), _lib.ptr(sums[1]), _h8(x), _lib.ptr(ws), ws.numel() * 8, b, g8 * 8, h * w, dtype=x.dtype)
    return sums


def bn_apply(x, scale, shift, residual=None, relu=True, out=None):
    """l2i_bn_apply_h8: relu?(x * scale[c] + shift[c] (+ residual)) on h8 maps."""
    b, g8, h, w, _ = x.shape
    out = torch.empty_like(x) if out is None else out
    assert residual is None or (residual.shape == x.shape and residual.dtype == x.dtype)
    _lib.call('l2i_bn_apply_h8', _h8(out), _h8(x), _lib.fptr(scale), _lib.fptr(shift), None if residual is None else _h8(residual), int(bool(relu)), b, g8 * 8,
              h * w, dtype=x.dtype)
    return out


def bn_bwd_reduce(gy, out_mask, x, mean, invstd, sums, ws=None):
    """l2i_bn_bwd_reduce_h8: sums [2, C] float64 (OVERWRITTEN) <- sum dy, sum dy * xhat with dy = gy * (out_mask > 0) when a mask map is given."""
    b, g8, h, w, _ = x.shape
    ws = _bn_ws(x, ws)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (2, g8 * 8) and gy.shape == x.shape and gy.dtype == x.dtype
    _lib.call('l2i_bn_bwd_reduce_h8', _lib.ptr(sums[0]), _lib.ptr(sums[1]), _h8(gy), None if out_mask is None else _h8(out_mask), _h8(x), _lib.fptr(mean),
              _lib.fptr(invstd), _lib.ptr(ws), ws.numel() * 8, b, g8 * 8, h * w, dtype=x.dtype)
    return sums


def bn_bwd_apply(gy, out_mask, x, mean, invstd, gamma, m_dy, m_dyxh, want_masked=False, out=None, masked=None):
    """l2i_bn_bwd_apply_h8: (dx, masked dy or None) on h8 maps."""
    b, g8, h, w, _ = x.shape
    out = torch.empty_like(x) if out is None else out
    if want_masked and masked is None:
        masked = torch.empty_like(x)
    _lib.call('l2i_bn_bwd_apply_h8', _h8(out), None if masked is None else _h8(masked), _h8(gy), None if out_mask is None else _h8(out_mask), _h8(x),
              _lib.fptr(mean), _lib.fptr(invstd), _lib.fptr(gamma), _lib.fptr(m_dy), _lib.fptr(m_dyxh), b, g8 * 8, h * w, dtype=x.dtype)
    return out, masked
