"""The contract of the streaming entry points of include/l2i.h (csrc/l2i_stream.hip, csrc/l2i_stream_h8.hip), written once in float64, and the
case table that drives tests/test_stream_contract_gpu.py (checked on the CPU by tests/test_stream_ref_cpu.py).

Every model function takes NCHW tensors and returns {output name: (want, M)}: ``want`` in ``dt`` (float64 unless the CPU test asks for the
same formula in float32) and ``M``, the sum of the absolute values of the terms that output adds up — every bound is stated against M.
``rnd``: what a 16-bit h8 map holds of an operand (None: the fp32 entry points); it is applied to the operands that ARE h8 maps and to
nothing else.  Float arguments of the C ABI (gain, slope, coef, ...) are rounded to float32 first, as the call does.

A plain module: no fixtures, no GPU, no kernel code."""
import numpy as np
import torch

SQRT2 = 2 ** 0.5
U23 = 2.0 ** -23
SENTINEL = -7776.0            # exactly representable in fp32, bf16 and fp16; far from every result
SENTINEL_U8 = 0xA5
GUARD = 64                    # guard elements on either side of an output (a multiple of 16 bytes for every element type)
ELEM_DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}

MISTAKES = ('noise_after_bias', 'gin_scale_on_rgb', 'zpre_pos_inverse', 'red_gin_y_scaled', 'red_x_grgb_boc', 'coef_dev_ignored', 'sqdiff_sign',
            'relu_before_argmax')


def f32(v):
    return float(np.float32(v))


def rnd_for(elem):
    """The rounding an h8 map of element type ``elem`` applies ('f32': none)."""
    if elem == 'f32':
        return None
    dtype = ELEM_DTYPES[elem]
    return lambda t: t.to(dtype).to(torch.float32)


def _c(t, dt, rnd=None):
    if t is None:
        return None
    t = torch.as_tensor(t).detach().cpu().float()
    if rnd is not None:
        t = rnd(t)
    return t.to(dt)


def _psum(t, chunked=False):
    """Sum over the pixel axes (2, 3) of [B, C, H, W]; ``chunked``: per 256-element block first, then across blocks (another order)."""
    t = t.flatten(2)
    if not chunked:
        return t.sum(-1)
    n = t.shape[-1]
    pad = (-n) % 256
    if pad:
        t = torch.cat([t, t.new_zeros(t.shape[:-1] + (pad,))], -1)
    return t.reshape(t.shape[:-1] + (-1, 256)).sum(-1).sum(-1)


# ---- layout -------------------------------------------------------------------------------------------------------------------------------------
def to_h8(x, cpad, dtype):
    """fp32 NCHW -> h8 [B, cpad/8, H, W, 8] of ``dtype`` (round to nearest even), zeros in the channels >= C."""
    B, C, H, W = x.shape
    full = torch.zeros(B, cpad, H, W, dtype=torch.float32)
    full[:, :C] = x
    return full.reshape(B, cpad // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().to(dtype)


def from_h8(t, C=None):
    B, G8, H, W, _ = t.shape
    x = t.float().permute(0, 1, 4, 2, 3).reshape(B, G8 * 8, H, W)
    return x if C is None else x[:, :C].contiguous()


def sign_plane(ref_h8):
    """One byte per pixel slot, bit e = element e > 0 (l2i_conv_params::mask_out)."""
    bits = (ref_h8.float() > 0).to(torch.int32) << torch.arange(8, dtype=torch.int32)
    return bits.sum(-1).to(torch.uint8)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def torgb_fwd(x, wmod, bias=None, rnd=None, dt=torch.float64):
    """rgb[b,o,p] = sum_c x[b,c,p] wmod[b,o,c] + bias[o]"""
    x, wmod, bias = _c(x, dt, rnd), _c(wmod, dt), _c(bias, dt)
    want = torch.einsum('bchw,boc->bohw', x, wmod)
    M = torch.einsum('bchw,boc->bohw', x.abs(), wmod.abs())
    if bias is not None:
        want, M = want + bias[None, :, None, None], M + bias.abs()[None, :, None, None]
    return {'rgb': (want, M)}


def sg2_act_bwd(y, gin=None, gin_scale=None, grgb=None, wmod_rgb=None, bias=None, noise=None, noise_w=0.0, slope=0.2, gain=SQRT2,
                rnd=None, dt=torch.float64, chunked=False, _mistake=None):
    """g = gin gin_scale + sum_o wmod_rgb grgb;  dz = g (y > 0 ? gain : gain slope);  zpre = y / (that factor) - bias - noise noise_w;
    red_dz_z = sum_p dz zpre;  red_x_grgb[b,c,o] = sum_p y grgb[b,o];  red_gin_y = sum_p gin y.  Sums that need an absent operand are None."""
    assert _mistake is None or _mistake in MISTAKES
    assert (gin is not None or grgb is not None) and (grgb is None) == (wmod_rgb is None)
    y, gin = _c(y, dt, rnd), _c(gin, dt, rnd)
    gin_scale, grgb, wmod_rgb, bias, noise = (_c(t, dt) for t in (gin_scale, grgb, wmod_rgb, bias, noise))
    gp, gn, nw = f32(gain), f32(gain) * f32(slope), f32(noise_w)
    pos = y > 0                                            # both zeros take the negative side
    one = torch.ones((), dtype=dt)
    fac = torch.where(pos, gp * one, gn * one)
    gs = one if gin_scale is None else gin_scale[:, :, None, None]
    g, Mg = torch.zeros_like(y), torch.zeros_like(y)
    if gin is not None:
        g, Mg = gin * gs, (gin * gs).abs()
    if grgb is not None:
        part = torch.einsum('bohw,boc->bchw', grgb, wmod_rgb)
        g = (gin + part) * gs if (_mistake == 'gin_scale_on_rgb' and gin is not None) else g + part
        Mg = Mg + torch.einsum('bohw,boc->bchw', grgb.abs(), wmod_rgb.abs())
    dz, Mdz = g * fac, Mg * fac.abs()
    inv = torch.where(pos, one / gp, one / (gp if _mistake == 'zpre_pos_inverse' else gn))
    zp, Mz = y * inv, (y * inv).abs()
    if _mistake == 'noise_after_bias' and bias is not None and noise is not None:
        zp = zp - (bias[None, :, None, None] + noise) * nw
    else:
        if bias is not None:
            zp, Mz = zp - bias[None, :, None, None], Mz + bias.abs()[None, :, None, None]
        if noise is not None:
            zp, Mz = zp - noise * nw, Mz + (noise * nw).abs()
    out = {'dz': (dz, Mdz), 'red_dz_z': (_psum(dz * zp, chunked), _psum(Mdz * Mz)), 'red_x_grgb': None, 'red_gin_y': None}
    if grgb is not None:
        B, C = y.shape[:2]
        r = torch.stack([_psum(y * grgb[:, o:o + 1], chunked) for o in range(3)], -1)          # [B, C, 3]
        if _mistake == 'red_x_grgb_boc':
            r = r.permute(0, 2, 1).reshape(B, C, 3)
        out['red_x_grgb'] = (r, torch.stack([_psum((y * grgb[:, o:o + 1]).abs()) for o in range(3)], -1))
    if gin is not None:
        q = gin * gs * y if _mistake == 'red_gin_y_scaled' else gin * y
        out['red_gin_y'] = (_psum(q, chunked), _psum((gin * y).abs()))
    return out


def dot_reduce(a, b=None, rnd=None, dt=torch.float64, chunked=False):
    """out[b,c] = sum_p a (b ? b : 1)"""
    a, b = _c(a, dt, rnd), _c(b, dt, rnd)
    t = a if b is None else a * b
    return {'out': (_psum(t, chunked), _psum(t.abs()))}


def sqdiff(a, b, coef=0.0, coef_dev=None, rnd=None, dt=torch.float64, chunked=False, _mistake=None):
    """sum = sum (a - b)^2;  grad = coef coef_dev[0] (b - a)   (coef_dev NULL = 1)"""
    a, b = _c(a, dt, rnd), _c(b, dt, rnd)
    cf = f32(coef) * (1.0 if (coef_dev is None or _mistake == 'coef_dev_ignored') else float(_c(coef_dev, dt).reshape(-1)[0]))
    d = (a - b) if _mistake == 'sqdiff_sign' else (b - a)
    s = d.reshape(1, 1, 1, -1) ** 2
    return {'sum': (_psum(s, chunked).reshape(1), _psum(s).reshape(1)), 'grad': (cf * d, abs(cf) * d.abs())}


def axpby(a, b=None, alpha=1.0, beta=1.0, dt=torch.float64):
    a, b = _c(a, dt), _c(b, dt)
    want, M = f32(alpha) * a, abs(f32(alpha)) * a.abs()
    if b is not None:
        want, M = want + f32(beta) * b, M + abs(f32(beta)) * b.abs()
    return {'y': (want, M)}


def relu_mask(g, ref, dt=torch.float64):
    g, ref = _c(g, dt), _c(ref, dt)
    return {'y': (torch.where(ref > 0, g, torch.zeros_like(g)), g.abs())}


def mask_mul(g, ref, pos=1.0, neg=0.0, rnd=None, dt=torch.float64):
    """y = g (ref > 0 ? pos : neg); the sign plane of ``ref`` is the same statement about ``ref``."""
    g, ref = _c(g, dt, rnd), _c(ref, dt, rnd)
    one = torch.ones((), dtype=dt)
    want = g * torch.where(ref > 0, f32(pos) * one, f32(neg) * one)
    return {'y': (want, want.abs())}


def add_zero_insert(y, c, mask=None, rnd=None, dt=torch.float64):
    """y[2 oy, 2 ox] += c[oy, ox] (mask ? mask[2 oy, 2 ox] > 0 : 1); c covers ceil(H / 2) x ceil(W / 2)"""
    y, c, mask = _c(y, dt, rnd), _c(c, dt, rnd), _c(mask, dt, rnd)
    assert c.shape[2] == (y.shape[2] + 1) // 2 and c.shape[3] == (y.shape[3] + 1) // 2
    add = c if mask is None else torch.where(mask[:, :, ::2, ::2] > 0, c, torch.zeros_like(c))
    want, M = y.clone(), y.abs()
    want[:, :, ::2, ::2] += add
    M[:, :, ::2, ::2] += add.abs()
    return {'y': (want, M)}


def pool_out(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def maxpool_fwd(x, k, s, pad, relu=False, rnd=None, dt=torch.float64, _mistake=None):
    """MaxPool2d(k, s, pad): the value and the window-local index ky k + kx of the FIRST maximum in row-major order over the taps inside the map;
    a NaN in the window is the result (the last one met gives the index, as in ATen).  relu: y = max(pool, 0), the index unchanged."""
    x = _c(x, dt, rnd)
    if _mistake == 'relu_before_argmax':
        x = torch.where(x > 0, x, torch.where(torch.isnan(x), x, torch.zeros_like(x)))
    B, C, H, W = x.shape
    OH, OW = pool_out(H, k, s, pad), pool_out(W, k, s, pad)
    ext_h, ext_w = (OH - 1) * s + k, (OW - 1) * s + k
    xp = torch.zeros(B, C, max(ext_h, H + pad), max(ext_w, W + pad), dtype=dt)
    ok = torch.zeros(xp.shape[2:], dtype=torch.bool)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    ok[pad:pad + H, pad:pad + W] = True
    best = torch.full((B, C, OH, OW), float('-inf'), dtype=dt)
    bi = torch.zeros(B, C, OH, OW, dtype=torch.uint8)
    found = torch.zeros(OH, OW, dtype=torch.bool)
    for ky in range(k):
        for kx in range(k):
            v = xp[:, :, ky:ky + (OH - 1) * s + 1:s, kx:kx + (OW - 1) * s + 1:s]
            inside = ok[ky:ky + (OH - 1) * s + 1:s, kx:kx + (OW - 1) * s + 1:s]
            upd = inside & (~found | (v > best) | torch.isnan(v))
            best = torch.where(upd, v, best)
            bi = torch.where(upd, torch.tensor(ky * k + kx, dtype=torch.uint8), bi)
            found = found | inside
    assert bool(found.all())
    if relu:
        best = torch.where(best > 0, best, torch.where(torch.isnan(best), best, torch.zeros_like(best)))
    return {'y': (best, best.abs()), 'idx': (bi, None)}


def maxpool_bwd(gy, idx, in_hw, k, s, pad, a=None, b=None, coef=0.0, coef_dev=None, rnd=None, dt=torch.float64, _mistake=None):
    """gx[iy, ix] = sum of gy over the windows whose arg-max (iy, ix) is  (+ coef coef_dev[0] (b - a) when a / b are given; coef_dev NULL = 1)"""
    gy, a, b = _c(gy, dt, rnd), _c(a, dt, rnd), _c(b, dt, rnd)
    B, C, OH, OW = gy.shape
    H, W = in_hw
    ext_h, ext_w = max((OH - 1) * s + k, H + pad), max((OW - 1) * s + k, W + pad)
    gx, M = torch.zeros(B, C, ext_h, ext_w, dtype=dt), torch.zeros(B, C, ext_h, ext_w, dtype=dt)
    for ky in range(k):
        for kx in range(k):
            hit = torch.where(idx == ky * k + kx, gy, torch.zeros_like(gy))
            gx[:, :, ky:ky + (OH - 1) * s + 1:s, kx:kx + (OW - 1) * s + 1:s] += hit
            M[:, :, ky:ky + (OH - 1) * s + 1:s, kx:kx + (OW - 1) * s + 1:s] += hit.abs()
    gx, M = gx[:, :, pad:pad + H, pad:pad + W].clone(), M[:, :, pad:pad + H, pad:pad + W].clone()
    if a is not None:
        cf = f32(coef) * (1.0 if (coef_dev is None or _mistake == 'coef_dev_ignored') else float(_c(coef_dev, dt).reshape(-1)[0]))
        gx, M = gx + cf * (b - a), M + abs(cf) * (b - a).abs()
    return {'gx': (gx, M)}


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------------
# k = rounded fp32 operations that form one element of an elementwise output (products, sums, the factor gain * slope, the product coef * coef_dev)
K_OPS = {'dz': 10,                 # gin gs (1) + three products and three sums of the ToRGB part (6) + gain slope (1) + the factor (1) + 1
         'sqdiff_grad': 3,         # b - a, coef coef_dev, their product
         'axpby': 3, 'mask_mul': 1, 'add_zero_insert': 1}


def k_torgb(C):
    return C + 1


def k_pool_bwd(k, s):
    return 3 + ((k + s - 1) // s) ** 2          # b - a, coef coef_dev, product + one sum per window that can hold the pixel


def bound_elem(M, k):
    return U23 * k * M


def bound_red(M, n_lane):
    """n_lane terms added by one lane in sequence; 16 for the wave (6), block (2) and atomic stages and the few roundings inside a term."""
    return U23 * (n_lane + 16) * M


def half_ulp(want, elem):
    mant, emin = (7, -126) if elem == 'bf16' else (10, -14)
    e = torch.frexp(want.abs().double())[1].double() - 1.0           # floor(log2 |want|)
    e = torch.where(want == 0, torch.full_like(e, emin), torch.clamp(e, min=emin))
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def bound16(want, M, k, elem):
    return half_ulp(want, elem) + U23 * k * M.double() + (2.0 ** -24 if elem == 'f16' else 0.0)


def worst(got, want, bound):
    """(largest error, its bound, largest error / bound) over the elements; an element with bound 0 must match exactly."""
    err = (torch.as_tensor(got).detach().cpu().double() - want.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)
    i = int(ratio.reshape(-1).argmax()) if ratio.numel() else 0
    return float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]), float(ratio.reshape(-1)[i])


# ---- launch geometry, restated from the entry points (the path a row names is derived here, and n_lane for the reduced bounds) ----------------------
def grid_for(work, per_block, cap=256 * 8):
    return int(min(max((work + per_block - 1) // per_block, 1), cap))


def cdiv(a, b):
    return (a + b - 1) // b


def rows_geom_f32(rows, cols, vec=True):
    """l2i_sg2_act_bwd_f32 / l2i_dot_reduce_f32: chunks per row, whether the cap cut them, terms per lane."""
    free = max(cdiv(cols // 4, 1024), 1)
    cap = cdiv(256 * 16, rows)
    chunks = max(min(free, cap), 1)
    n_lane = 4 * cdiv(cols // 4, chunks * 256) if vec else cdiv(cols, chunks * 256)
    return dict(chunks=chunks, capped=chunks < free, n_lane=n_lane)


def torgb_geom_f32(B, HW):
    free = cdiv(HW // 4, 256)
    cap = cdiv(256 * 8, B)
    bpb = max(min(free, cap), 1)
    return dict(bpb=bpb, capped=bpb < free, passes=cdiv(HW // 4, bpb * 256))


def h8_strips(groups, HW):
    return int(max(min(cdiv(4096, groups), cdiv(HW, 2048), 256), 1))


def h8_red_geom(groups, HW):
    st = h8_strips(groups, HW)
    return dict(strips=st, n_lane=cdiv(HW, st * 256), forced_one=st == 1 and cdiv(HW, 2048) > 1)


def torgb_geom_h8(HW):
    bps = min(cdiv(HW, 256), 512)
    return dict(bps=bps, passes=cdiv(HW, bps * 256))


def pool_offsets(aligned):
    """{tensor: elements its view starts past a 64-byte boundary}.  True: none; False: x, y and gx one float; or a dict naming one tensor."""
    return aligned if isinstance(aligned, dict) else ({} if aligned else {'x': 1, 'y': 1, 'gx': 1})


def pool_fwd_kernel_f32(H, W, k, s, pad, aligned=True):
    OH, OW = pool_out(H, k, s, pad), pool_out(W, k, s, pad)
    off = pool_offsets(aligned)
    ptr_ok = (4 * off.get('x', 0)) % 16 == 0 and (4 * off.get('y', 0)) % 16 == 0 and off.get('idx', 0) % 4 == 0
    vec_ok = s == 2 and W == 2 * OW and OW % 4 == 0 and ptr_ok
    if vec_ok and k == 2 and pad == 0 and H == 2 * OH:
        return 'maxpool_fwd_vec_kernel<2>'
    if vec_ok and k == 3 and pad == 1 and (H + 1) // 2 == OH:
        return 'maxpool_fwd_vec_kernel<3>'
    return 'maxpool_fwd_kernel'


def pool_bwd_kernel_f32(H, W, k, s, pad, aligned=True):
    OH, OW = pool_out(H, k, s, pad), pool_out(W, k, s, pad)
    off = pool_offsets(aligned)
    gx_b, gy_b, idx_b = 4 * off.get('gx', 0), 4 * off.get('gy', 0), off.get('idx', 0)
    if k == 2 and s == 2 and pad == 0 and H == 2 * OH and W == 2 * OW and gx_b % 8 == 0:
        return 'maxpool_bwd_k2s2_kernel'
    if k == 3 and s == 2 and pad == 1 and W == 2 * OW and (H + 1) // 2 == OH and W % 4 == 0 and gx_b % 16 == 0 and gy_b % 8 == 0 and idx_b % 2 == 0:
        return 'maxpool_bwd_k3s2p1_vec_kernel'
    return 'maxpool_bwd_kernel<3,2,1>' if (k, s, pad) == (3, 2, 1) else 'maxpool_bwd_kernel<0,0,0>'


# ---- data ---------------------------------------------------------------------------------------------------------------------------------------
TINY = 2.0 ** -126            # smallest normal fp32 (= smallest normal bf16; rounds to zero in fp16)
DENORM = 1e-42                # an fp32 subnormal: rounds to a zero of its sign in bf16 and fp16


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def plant_signs(t, h8=False):
    """-0.0, +0.0 and +-(smallest normal) at fixed positions (first and last elements); h8 forms also get values that round to a zero."""
    v = [-0.0, 0.0, TINY, -TINY] + ([DENORM, -DENORM] if h8 else [])
    f = t.reshape(-1)
    n = min(len(v), f.numel() // 2)
    f[:n] = torch.tensor(v[:n])
    if n:
        f[-n:] = torch.tensor(v[:n])
    return t


def pool_input(rs, shape, k, s, pad, nan=True):
    """Coarse values (ties inside windows), one all-equal window, one NaN, and on a map whose last window row hangs over the edge the
    plane's largest value in the last real row (the window's maximum sits beside the padding row)."""
    x = T(np.round(rs.randn(*shape) * 2) / 2)
    H, W = shape[2:]
    x[0, 0, :min(k, H), :min(k, W)] = 0.5
    x[-1, -1, H - 1, W // 2] = 9.0
    if nan:
        x[0, -1, H // 2, W // 2] = float('nan')
    return x


# ---- the case table -------------------------------------------------------------------------------------------------------------------------------
# operand cases: name -> (operands present, mistakes the case exists to catch)
SG2_ALL = ('gin', 'gin_scale', 'rgb', 'bias', 'noise', 'red_dz_z', 'red_x_grgb', 'red_gin_y')          # rgb = grgb + wmod_rgb (they go together)
SG2_CASES = {
    'everything': (SG2_ALL, ()),
    # each optional operand absent, alone
    'no_gin': (tuple(f for f in SG2_ALL if f not in ('gin', 'gin_scale', 'red_gin_y')), ()),
    'no_gin_scale': (tuple(f for f in SG2_ALL if f != 'gin_scale'), ()),
    'no_rgb': (tuple(f for f in SG2_ALL if f not in ('rgb', 'red_x_grgb')), ()),
    'no_bias': (tuple(f for f in SG2_ALL if f != 'bias'), ()),
    'no_noise': (tuple(f for f in SG2_ALL if f != 'noise'), ()),
    'no_red_dz_z': (tuple(f for f in SG2_ALL if f != 'red_dz_z'), ()),
    'no_red_x_grgb': (tuple(f for f in SG2_ALL if f != 'red_x_grgb'), ()),
    'no_red_gin_y': (tuple(f for f in SG2_ALL if f != 'red_gin_y'), ()),
    # each optional operand present, alone on the bare op (gin -> dz); bias and noise show in red_dz_z only
    'bare': (('gin',), ()),
    'gin_scale': (('gin', 'gin_scale'), ()),
    'rgb_alone': (('rgb',), ()),
    'rgb': (('gin', 'rgb'), ()),
    'bias': (('gin', 'bias', 'red_dz_z'), ()),
    'noise': (('gin', 'noise', 'red_dz_z'), ()),
    'red_dz_z': (('gin', 'red_dz_z'), ('zpre_pos_inverse',)),
    'red_x_grgb': (('rgb', 'red_x_grgb'), ('red_x_grgb_boc',)),
    'red_gin_y': (('gin', 'red_gin_y'), ()),
    # a sum buffer whose operand is absent is not touched (the header's promise): the buffer is passed holding the sentinel and must keep it
    'red_x_grgb_without_rgb': (('gin', 'red_x_grgb'), ()),
    'red_gin_y_without_gin': (('rgb', 'red_gin_y'), ()),
    # combinations, each for the mistake it names
    'noise_bias': (('gin', 'bias', 'noise', 'red_dz_z'), ('noise_after_bias',)),
    'scale_rgb': (('gin', 'gin_scale', 'rgb'), ('gin_scale_on_rgb',)),
    'scaled_gin_y': (('gin', 'gin_scale', 'red_gin_y'), ('red_gin_y_scaled',)),
}
SQDIFF_CASES = {'both_dev': (('sum', 'grad', 'coef_dev'), ('coef_dev_ignored', 'sqdiff_sign')), 'both_null': (('sum', 'grad'), ('sqdiff_sign',)),
                'sum_only': (('sum',), ()), 'grad_only': (('grad', 'coef_dev'), ())}


def sg2_inputs(seed, fields, B, C, H, W, h8=False):
    """Operands of an sg2_act_bwd case as float32 CPU tensors keyed by the model's keyword names (absent operands are absent keys)."""
    rs = np.random.RandomState(seed)
    kw = {'y': plant_signs(T(rs.randn(B, C, H, W)), h8), 'slope': 0.2, 'gain': SQRT2}
    if 'gin' in fields:
        kw['gin'] = T(rs.randn(B, C, H, W))
    if 'gin_scale' in fields:
        kw['gin_scale'] = T(rs.rand(B, C) + 0.5)
    if 'rgb' in fields:
        kw['grgb'], kw['wmod_rgb'] = T(rs.randn(B, 3, H, W)), T(rs.randn(B, 3, C))
    if 'bias' in fields:
        kw['bias'] = T(rs.randn(C))
    if 'noise' in fields:
        kw['noise'], kw['noise_w'] = T(rs.randn(B, 1, H, W)), 0.3
    return kw


# geometry rows: (id, kernel the row is meant to reach, shape).  Every predicate is restated by the *_geom functions above and asserted by
# tests/test_stream_ref_cpu.py::test_geometry_rows_enter_the_paths_they_name.
TORGB_F32_GEOMS = [          # (id, B, C, H, W): C covers no unrolled pass (1, 5), the tail only after passes (13), passes only (8, 24)
    ('c1_hw4_15', 2, 1, 6, 10), ('c5_hw4_15', 2, 5, 6, 10), ('c8_hw4_300', 1, 8, 30, 40), ('c13_hw4_300', 2, 13, 30, 40), ('c24_hw4_15', 1, 24, 6, 10),
    ('capped_second_pass', 2048, 1, 4, 257),          # cap = 1 block per sample, hw4 = 257: the grid-stride loop runs twice
]
SG2_F32_GEOMS = [            # (id, B, C, H, W)
    ('hw16_one_wave', 2, 3, 4, 4), ('hw5184_two_chunks_ragged', 1, 2, 72, 72), ('capped_chunks', 1, 4096, 50, 82),
]
DOT_F32_GEOMS = SG2_F32_GEOMS + [('scalar_odd_cols', 2, 3, 5, 7)]          # cols = 35: cols % 4 != 0 and rows off the 16-byte grid
H8_RED_GEOMS = [             # (id, B, C, H, W)
    ('hw400_one_strip', 2, 8, 20, 20), ('hw2304_two_strips', 1, 40, 48, 48), ('hw4100_three_strips', 1, 8, 50, 82),
]
H8_DOT_FORCED = ('strips_forced_to_one', 1, 8 * 4096, 1, 2052)          # 4096 groups: strips = 1 on a map that would take 2 (dot_reduce, a only)
# The fused backward has no such row: strips falls back to 1 on HW > 2048 only from 4096 groups on, 67 M elements per map at the least, and its
# float64 model with three maps and their temporaries takes far more than the few seconds a row may.  h8_strips() is one host function shared by
# both reducers (the dot_reduce row holds the fall-back), and the kernel's loop of several two-slot iterations inside one strip, with `two` false
# on the last, runs in hw2304_two_strips (step 512: pixels p, p + 1024, p + 2048) and hw4100_three_strips.
TORGB_H8_GEOMS = [           # (id, B, C, H, W): G8 = 1, 3, 4, 5, 9; HW = 300 is no multiple of 256
    ('g1', 2, 8, 15, 20), ('g3', 1, 24, 15, 20), ('g4', 2, 32, 15, 20), ('g5', 1, 40, 15, 20), ('g9', 1, 72, 15, 20),
    ('bps_capped_second_pass', 1, 8, 362, 363),        # HW = 131406 > 512 * 256
]
ELEMWISE_N = {               # sizes: 1, 255, the first with two blocks, one past the grid cap (l2i_grid_for(n, per_block, cap): per_block * cap + 1)
    'sqdiff_f32': (1, 255, 2049, 2048 * 2048 + 1), 'axpby_f32': (1, 255, 1025, 1024 * 2048 + 1), 'relu_mask_f32': (1, 255, 1025, 1024 * 2048 + 1),
    'sqdiff_h8': (1, 255, 257, 2049, 256 * 2048 + 1), 'mask_mul_h8': (1, 255, 257, 2049, 256 * 4096 + 1), 'mask_mul_bits_h8': (1, 255, 257, 2049, 256 * 4096 + 1),
}
POOL_F32_GEOMS = [           # (id, k, s, pad, H, W, aligned, forward kernel, backward kernel); 3 planes; non-square throughout
    ('k2_vec', 2, 2, 0, 6, 16, True, 'maxpool_fwd_vec_kernel<2>', 'maxpool_bwd_k2s2_kernel'),
    ('k2_ow_mod4', 2, 2, 0, 6, 12, True, 'maxpool_fwd_kernel', 'maxpool_bwd_k2s2_kernel'),
    ('k2_odd', 2, 2, 0, 7, 17, True, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<0,0,0>'),
    ('k2_unaligned', 2, 2, 0, 6, 16, False, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<0,0,0>'),
    ('k3_vec', 3, 2, 1, 8, 16, True, 'maxpool_fwd_vec_kernel<3>', 'maxpool_bwd_k3s2p1_vec_kernel'),
    ('k3_vec_odd_h', 3, 2, 1, 7, 16, True, 'maxpool_fwd_vec_kernel<3>', 'maxpool_bwd_k3s2p1_vec_kernel'),
    ('k3_ow_mod4', 3, 2, 1, 8, 12, True, 'maxpool_fwd_kernel', 'maxpool_bwd_k3s2p1_vec_kernel'),
    ('k3_w_mod4', 3, 2, 1, 9, 10, True, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<3,2,1>'),
    ('k3_odd_w', 3, 2, 1, 9, 15, True, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<3,2,1>'),
    ('k3_unaligned', 3, 2, 1, 7, 16, False, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<3,2,1>'),
    # each pointer clause of the predicates false alone (x, y: 16 bytes; idx: 4 forward, 2 backward; gx: 8 for k2s2, 16 for k3; gy: 8)
    ('k2_x_off', 2, 2, 0, 6, 16, {'x': 1}, 'maxpool_fwd_kernel', 'maxpool_bwd_k2s2_kernel'),
    ('k2_y_off', 2, 2, 0, 6, 16, {'y': 1}, 'maxpool_fwd_kernel', 'maxpool_bwd_k2s2_kernel'),
    ('k2_idx_off2', 2, 2, 0, 6, 16, {'idx': 2}, 'maxpool_fwd_kernel', 'maxpool_bwd_k2s2_kernel'),
    ('k2_gx_off2', 2, 2, 0, 6, 16, {'gx': 2}, 'maxpool_fwd_vec_kernel<2>', 'maxpool_bwd_k2s2_kernel'),
    ('k2_gx_off1', 2, 2, 0, 6, 16, {'gx': 1}, 'maxpool_fwd_vec_kernel<2>', 'maxpool_bwd_kernel<0,0,0>'),
    ('k3_gx_off2', 3, 2, 1, 7, 16, {'gx': 2}, 'maxpool_fwd_vec_kernel<3>', 'maxpool_bwd_kernel<3,2,1>'),
    ('k3_gy_off1', 3, 2, 1, 7, 16, {'gy': 1}, 'maxpool_fwd_vec_kernel<3>', 'maxpool_bwd_kernel<3,2,1>'),
    ('k3_idx_off1', 3, 2, 1, 7, 16, {'idx': 1}, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<3,2,1>'),
    ('k3_idx_off2', 3, 2, 1, 7, 16, {'idx': 2}, 'maxpool_fwd_kernel', 'maxpool_bwd_k3s2p1_vec_kernel'),
    ('k3s1p1', 3, 1, 1, 7, 10, True, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<0,0,0>'),
    ('k2s1p0', 2, 1, 0, 7, 10, True, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<0,0,0>'),
    ('k3s3p0', 3, 3, 0, 7, 10, True, 'maxpool_fwd_kernel', 'maxpool_bwd_kernel<0,0,0>'),
]
POOL_H8_KSP = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (2, 1, 0), (3, 3, 0)]          # on a 7 x 9 map
ADD_DIFF_GEOMS = [('oh3_ow4', 3, 4), ('oh5_ow6', 5, 6)]
CAST_GEOMS = [('c3_pad16', 2, 3, 16, 5, 7), ('hw1', 1, 8, 8, 1, 1), ('c13_pad16_hw1', 1, 13, 16, 1, 1)]          # (id, B, C, Cpad, H, W)

# __global__ kernels of the two files: the ones a row above claims (tests/fir_ref.py claims the others), and the ones out of scope by name (a new kernel has to be placed)
CLAIMED_KERNELS = {
    'torgb_fwd_kernel': 'TORGB_F32_GEOMS', 'sg2_act_bwd_kernel': 'SG2_F32_GEOMS', 'dot_reduce_kernel': 'DOT_F32_GEOMS',
    'maxpool_fwd_kernel': 'POOL_F32_GEOMS', 'maxpool_fwd_vec_kernel': 'POOL_F32_GEOMS', 'maxpool_bwd_kernel': 'POOL_F32_GEOMS',
    'maxpool_bwd_k2s2_kernel': 'POOL_F32_GEOMS', 'maxpool_bwd_k3s2p1_vec_kernel': 'POOL_F32_GEOMS', 'maxpool2x2_bwd_add_diff_kernel': 'ADD_DIFF_GEOMS',
    'sqdiff_kernel': 'ELEMWISE_N', 'axpby_kernel': 'ELEMWISE_N', 'relu_mask_kernel': 'ELEMWISE_N',
    'cast_f32_to_h8_kernel': 'CAST_GEOMS', 'cast_h8_to_f32_kernel': 'CAST_GEOMS', 'torgb_fwd_h8_kernel': 'TORGB_H8_GEOMS',
    'sg2_act_bwd_h8_kernel': 'H8_RED_GEOMS', 'dot_reduce_h8_kernel': 'H8_RED_GEOMS', 'maxpool_fwd_h8_kernel': 'POOL_H8_KSP',
    'maxpool_bwd_h8_kernel': 'POOL_H8_KSP', 'sqdiff_h8_kernel': 'ELEMWISE_N', 'add_zero_insert_h8_kernel': 'ZERO_INSERT_GEOMS',
    'mask_mul_h8_kernel': 'ELEMWISE_N', 'mask_mul_bits_h8_kernel': 'ELEMWISE_N',
}
ZERO_INSERT_GEOMS = [('odd_9x13', 2, 16, 9, 13), ('even_4x6', 1, 8, 4, 6)]          # (id, B, C, H, W): OH = ceil(H / 2), OW = ceil(W / 2)
OUT_OF_SCOPE_KERNELS = ()          # the FIR, bias-activation and weight-plane kernels are claimed by the rows of tests/fir_ref.py


# ---- rows: operation x operand case x geometry ------------------------------------------------------------------------------------------------------
class Row:
    """One test row.  ``kind``: 'f32' (l2i_stream.hip) or 'h8' (l2i_stream_h8.hip, run once per element type); ``path``: the kernel(s) it is meant
    to reach; ``big``: above a few megabytes (a row past a grid cap)."""

    def __init__(self, op, kind, case, geom, shape, path, big=False, **extra):
        self.op, self.kind, self.case, self.geom, self.shape, self.path, self.big, self.extra = op, kind, case, geom, tuple(shape), path, big, extra
        self.id = '%s_%s-%s-%s' % (op, kind, case, geom)

    def __repr__(self):
        return self.id

    @property
    def seed(self):
        import zlib
        return zlib.crc32(self.id.encode()) % (2 ** 31)


def all_rows():
    rows = []
    add = lambda *a, **k: rows.append(Row(*a, **k))
    base = (2, 16, 12, 20)                               # operand cases run here: HW = 240, two channel groups
    # ToRGB
    for case in ('bias', 'no_bias'):
        add('torgb', 'f32', case, 'operands', (2, 13, 30, 40), 'torgb_fwd_kernel')
        add('torgb', 'h8', case, 'operands', (1, 40, 15, 20), 'torgb_fwd_h8_kernel')
    for gid, B, C, H, W in TORGB_F32_GEOMS:
        add('torgb', 'f32', 'bias', gid, (B, C, H, W), 'torgb_fwd_kernel', big=B > 64)
    for gid, B, C, H, W in TORGB_H8_GEOMS:
        add('torgb', 'h8', 'bias', gid, (B, C, H, W), 'torgb_fwd_h8_kernel')
    # fused activation backward
    for case in SG2_CASES:
        add('sg2', 'f32', case, 'base', base, 'sg2_act_bwd_kernel')
        add('sg2', 'h8', case, 'base', base, 'sg2_act_bwd_h8_kernel')
    for gid, B, C, H, W in SG2_F32_GEOMS:
        add('sg2', 'f32', 'red_gin_y' if C > 64 else 'everything', gid, (B, C, H, W), 'sg2_act_bwd_kernel', big=C > 64)
    for gid, B, C, H, W in H8_RED_GEOMS:
        add('sg2', 'h8', 'everything', gid, (B, C, H, W), 'sg2_act_bwd_h8_kernel')
    add('sg2', 'f32', 'everything', 'accumulates', base, 'sg2_act_bwd_kernel', prefill=True)
    add('sg2', 'h8', 'everything', 'accumulates', base, 'sg2_act_bwd_h8_kernel', prefill=True)
    # row reductions
    for case in ('ab', 'a_only'):
        add('dot', 'f32', case, 'base', base, 'dot_reduce_kernel')
        add('dot', 'h8', case, 'base', base, 'dot_reduce_h8_kernel')
    for gid, B, C, H, W in DOT_F32_GEOMS:
        add('dot', 'f32', 'a_only' if C > 64 else 'ab', gid, (B, C, H, W), 'dot_reduce_kernel', big=C > 64)
    for gid, B, C, H, W in H8_RED_GEOMS:
        add('dot', 'h8', 'ab', gid, (B, C, H, W), 'dot_reduce_h8_kernel')
    add('dot', 'h8', 'a_only', H8_DOT_FORCED[0], H8_DOT_FORCED[1:], 'dot_reduce_h8_kernel', big=True)
    add('dot', 'f32', 'ab', 'accumulates', base, 'dot_reduce_kernel', prefill=True)
    add('dot', 'h8', 'ab', 'accumulates', base, 'dot_reduce_h8_kernel', prefill=True)
    # ContentLoss difference and the small elementwise kernels, by n (h8: n = pixel slots of an 8-channel map)
    for case in SQDIFF_CASES:
        add('sqdiff', 'f32', case, 'operands', (1, 1, 1, 2049), 'sqdiff_kernel')
        add('sqdiff', 'h8', case, 'operands', (1, 8, 1, 257), 'sqdiff_h8_kernel')
    add('sqdiff', 'f32', 'both_dev', 'accumulates', (1, 1, 1, 2049), 'sqdiff_kernel', prefill=True)
    add('sqdiff', 'h8', 'both_dev', 'accumulates', (1, 8, 1, 257), 'sqdiff_h8_kernel', prefill=True)
    for n in ELEMWISE_N['sqdiff_f32']:
        add('sqdiff', 'f32', 'both_dev', 'n%d' % n, (1, 1, 1, n), 'sqdiff_kernel', big=n > 10 ** 6)
    for n in ELEMWISE_N['sqdiff_h8']:
        add('sqdiff', 'h8', 'both_dev', 'n%d' % n, (1, 8, 1, n), 'sqdiff_h8_kernel', big=n > 10 ** 5)
    for n in ELEMWISE_N['axpby_f32']:
        for case in ('ab', 'a_only'):
            add('axpby', 'f32', case, 'n%d' % n, (1, 1, 1, n), 'axpby_kernel', big=n > 10 ** 6)
        add('relu_mask', 'f32', 'plain', 'n%d' % n, (1, 1, 1, n), 'relu_mask_kernel', big=n > 10 ** 6)
    for n in ELEMWISE_N['mask_mul_h8']:
        add('mask_mul', 'h8', 'map_and_bits', 'n%d' % n, (1, 8, 1, n), 'mask_mul_h8_kernel mask_mul_bits_h8_kernel', big=n > 10 ** 5)
    # zero insertion
    for gid, B, C, H, W in ZERO_INSERT_GEOMS:
        for case in ('mask', 'no_mask'):
            add('zero_insert', 'h8', case, gid, (B, C, H, W), 'add_zero_insert_h8_kernel')
    # max-pool: forward + backward of one geometry in one row
    for gid, k, s, pad, H, W, aligned, fk, bk in POOL_F32_GEOMS:
        add('pool', 'f32', 'plain', gid, (1, 3, H, W), fk + ' ' + bk, ksp=(k, s, pad), aligned=aligned)
    for k, s, pad in POOL_H8_KSP:
        for case in ('plain', 'relu', 'diff_null', 'diff_dev'):
            add('pool', 'h8', case, 'k%ds%dp%d_7x9' % (k, s, pad), (2, 16, 7, 9), 'maxpool_fwd_h8_kernel maxpool_bwd_h8_kernel', ksp=(k, s, pad), aligned=True)
    for gid, OH, OW in ADD_DIFF_GEOMS:
        for case in ('diff_null', 'diff_dev'):
            add('add_diff', 'f32', case, gid, (1, 3, 2 * OH, 2 * OW), 'maxpool2x2_bwd_add_diff_kernel')
    for gid, B, C, cpad, H, W in CAST_GEOMS:
        add('cast', 'h8', 'round_trip', gid, (B, C, H, W), 'cast_f32_to_h8_kernel cast_h8_to_f32_kernel', cpad=cpad)
    assert len({r.id for r in rows}) == len(rows)
    return rows


POOL_MISTAKE_ROWS = {'relu_before_argmax': 'relu', 'coef_dev_ignored': 'diff_dev'}


def make_inputs(row, elem):
    """The operands of a row as float32 CPU tensors / Python scalars, keyed by the model's keyword names."""
    rs = np.random.RandomState(row.seed)
    B, C, H, W = row.shape
    h8 = row.kind == 'h8'
    gen = torch.Generator().manual_seed(row.seed)          # one stream per row: successive operands of a big row are successive draws from it
    big = lambda *s: T(rs.standard_normal(size=s).astype(np.float32)) if not row.big else torch.randn(*s, generator=gen)
    if row.op == 'torgb':
        kw = {'x': big(B, C, H, W), 'wmod': T(rs.randn(B, 3, C))}
        if row.case == 'bias':
            kw['bias'] = T(rs.randn(3))
        return kw
    if row.op == 'sg2':
        fields = SG2_CASES[row.case][0]
        if row.big:
            kw = {'y': plant_signs(big(B, C, H, W), h8), 'gin': big(B, C, H, W), 'slope': 0.2, 'gain': SQRT2}
        else:
            kw = sg2_inputs(row.seed, fields, B, C, H, W, h8)
        kw['_reds'] = tuple(f for f in ('red_dz_z', 'red_x_grgb', 'red_gin_y') if f in fields)
        return kw
    if row.op == 'dot':
        kw = {'a': big(B, C, H, W)}
        if row.case == 'ab':
            kw['b'] = big(B, C, H, W)
        return kw
    if row.op == 'sqdiff':
        fields = SQDIFF_CASES[row.case][0]
        kw = {'a': big(B, C, H, W), 'b': big(B, C, H, W), 'coef': 0.25, '_sum': 'sum' in fields, '_grad': 'grad' in fields}
        if 'coef_dev' in fields:
            kw['coef_dev'] = torch.full((1,), 1.75)
        return kw
    if row.op == 'axpby':
        kw = {'a': big(B, C, H, W), 'alpha': 0.5, 'beta': -2.25}
        if row.case == 'ab':
            kw['b'] = big(B, C, H, W)
        return kw
    if row.op == 'relu_mask':
        return {'g': big(B, C, H, W), 'ref': plant_signs(big(B, C, H, W))}
    if row.op == 'mask_mul':
        return {'g': big(B, C, H, W), 'ref': plant_signs(big(B, C, H, W), True), 'pos': SQRT2, 'neg': 0.2 * SQRT2}
    if row.op == 'zero_insert':
        kw = {'y': T(rs.randn(B, C, H, W)), 'c': T(rs.randn(B, C, (H + 1) // 2, (W + 1) // 2))}
        if row.case == 'mask':
            kw['mask'] = plant_signs(T(rs.randn(B, C, H, W)), True)
        return kw
    if row.op == 'pool':
        k, s, pad = row.extra['ksp']
        kw = {'x': pool_input(rs, row.shape, k, s, pad), 'k': k, 's': s, 'pad': pad, 'relu': row.case == 'relu',
              'gy': T(rs.randn(B, C, pool_out(H, k, s, pad), pool_out(W, k, s, pad)))}
        if row.case.startswith('diff'):
            kw.update(a=T(rs.randn(B, C, H, W)), b=T(rs.randn(B, C, H, W)), coef=0.3)
            if row.case == 'diff_dev':
                kw['coef_dev'] = torch.full((1,), 1.75)
        return kw
    if row.op == 'add_diff':
        kw = {'x': pool_input(rs, row.shape, 2, 2, 0, nan=False), 'k': 2, 's': 2, 'pad': 0, 'relu': False, 'gy': T(rs.randn(B, C, H // 2, W // 2)),
              'a': T(rs.randn(B, C, H, W)), 'b': T(rs.randn(B, C, H, W)), 'coef': 0.3}
        if row.case == 'diff_dev':
            kw['coef_dev'] = torch.full((1,), 1.75)
        return kw
    if row.op == 'cast':
        return {'x': plant_signs(T(rs.randn(B, C, H, W)), True) if H * W * C >= 12 else T(rs.randn(B, C, H, W))}
    raise KeyError(row.op)


def expected(row, kw, elem, dt=torch.float64, chunked=False, _mistake=None):
    """{output: (want, bound)} of a row for element type ``elem`` ('f32' rows: 'f32'): bound None = exact (torch.equal); outputs the row does
    not ask for are absent."""
    rnd = rnd_for(elem) if row.kind == 'h8' else None
    B, C, H, W = row.shape
    HW = H * W
    arg = {k: v for k, v in kw.items() if not k.startswith('_')}
    mk = {} if _mistake is None else {'_mistake': _mistake}
    b16 = lambda wm, k: (wm[0], bound16(wm[0], wm[1], k, elem))
    if row.op == 'torgb':
        want, M = torgb_fwd(rnd=rnd, dt=dt, **arg)['rgb']
        return {'rgb': (want, bound_elem(M, k_torgb(C)))}
    if row.op in ('sg2', 'dot'):
        n_lane = h8_red_geom(B * C // 8, HW)['n_lane'] if row.kind == 'h8' else rows_geom_f32(B * C, HW, vec=HW % 4 == 0)['n_lane']
        if row.op == 'dot':
            want, M = dot_reduce(rnd=rnd, dt=dt, chunked=chunked, **arg)['out']
            return {'out': (want, bound_red(M, n_lane))}
        m = sg2_act_bwd(rnd=rnd, dt=dt, chunked=chunked, **arg, **mk)
        out = {'dz': b16(m['dz'], K_OPS['dz']) if row.kind == 'h8' else (m['dz'][0], bound_elem(m['dz'][1], K_OPS['dz']))}
        for name in kw['_reds']:
            if m[name] is not None:
                out[name] = (m[name][0], bound_red(m[name][1], n_lane))
            else:                                          # its operand is absent: the buffer keeps what it held (the test passes it sentinel-filled)
                out[name] = (torch.full((B, C, 3) if name == 'red_x_grgb' else (B, C), SENTINEL, dtype=dt), None)
        return out
    if row.op == 'sqdiff':
        m = sqdiff(rnd=rnd, dt=dt, chunked=chunked, **arg, **mk)
        n = B * C * HW
        n_lane = 8 * cdiv(n // 8, grid_for(n // 8, 256, 256 * 8) * 256) if row.kind == 'h8' else cdiv(n, grid_for(n, 256 * 8) * 256)
        out = {}
        if kw['_sum']:
            out['sum'] = (m['sum'][0], bound_red(m['sum'][1], n_lane))
        if kw['_grad']:
            out['grad'] = b16(m['grad'], K_OPS['sqdiff_grad']) if row.kind == 'h8' else (m['grad'][0], bound_elem(m['grad'][1], K_OPS['sqdiff_grad']))
        return out
    if row.op == 'axpby':
        want, M = axpby(dt=dt, **arg)['y']
        return {'y': (want, bound_elem(M, K_OPS['axpby']))}
    if row.op == 'relu_mask':
        return {'y': (relu_mask(dt=dt, **arg)['y'][0], None)}
    if row.op == 'mask_mul':
        return {'y': b16(mask_mul(rnd=rnd, dt=dt, **arg)['y'], K_OPS['mask_mul'])}
    if row.op == 'zero_insert':
        return {'y': b16(add_zero_insert(rnd=rnd, dt=dt, **arg)['y'], K_OPS['add_zero_insert'])}
    if row.op in ('pool', 'add_diff'):
        k, s, pad = kw['k'], kw['s'], kw['pad']
        f = maxpool_fwd(kw['x'], k, s, pad, relu=kw['relu'], rnd=rnd, dt=dt, **({'_mistake': _mistake} if _mistake == 'relu_before_argmax' else {}))
        g = maxpool_bwd(kw['gy'], f['idx'][0], (H, W), k, s, pad, a=kw.get('a'), b=kw.get('b'), coef=kw.get('coef', 0.0), coef_dev=kw.get('coef_dev'),
                        rnd=rnd, dt=dt, **({'_mistake': _mistake} if _mistake == 'coef_dev_ignored' else {}))['gx']
        gx = b16(g, k_pool_bwd(k, s)) if row.kind == 'h8' else (g[0], bound_elem(g[1], k_pool_bwd(k, s)))
        return {'gx': gx} if row.op == 'add_diff' else {'y': (f['y'][0], None), 'idx': (f['idx'][0], None), 'gx': gx}
    if row.op == 'cast':
        t = to_h8(kw['x'], row.extra['cpad'], ELEM_DTYPES[elem])
        return {'h8': (t, None), 'back': (from_h8(t, C), None)}
    raise KeyError(row.op)
