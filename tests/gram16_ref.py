"""Float64 model of l2i_gram_loss_h8 / l2i_gram_bwd_h8 (include/l2i.h): the model of tests/gram_ref.py, imported and not copied, evaluated on
inputs rounded to the 16-bit element type, with a numpy restatement of the h8 layout [B][C/8][HW][8].  tests/test_gram16_ref_cpu.py pins the
bounds and the mistake table, tests/test_gram16_gpu.py holds the kernels to them.

The bounds are derived, not measured.  u_h is the unit roundoff of the element type.
  G, D, loss   gram_ref.gram_bound / loss_bound unchanged: a product of two 16-bit elements is exact in fp32 (22 or 16 significand bits), so only the
               fp32 summation (any order) remains.
  backward     gram_ref.bwd_bound (the fp32 sums, and the fp32 add when accumulating)
               + u_h * coef |s| (|D| @ |F|)          the operand coef * s * D, rounded to the element type after the fp32 scaling
               + u_h * (|g| + the terms above)       the h8 store
               + 2^-25 for fp16                      the store of a subnormal
               + u_h * |g| when accumulating.
"""
import numpy as np
import torch

from tests import gram_ref as R

SHAPES = R.SHAPES
DTYPES = ('f16', 'bf16')
TORCH = {'f16': torch.float16, 'bf16': torch.bfloat16}
UH = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}
MISTAKES = R.MISTAKES + ('chunk_as_plane', 'd_rounded_before_scaling', 'g0_ignored_in_h8')


def round16(a, dt):
    """Round a float array to the element type (through float32, nearest even) -> float32."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(TORCH[dt]).float().numpy()


def pack_h8(a):
    """[B, C, HW] -> [B, C/8, HW, 8]: channel 8 g + e of pixel p at [g][p][e]."""
    b, ch, hw = a.shape
    assert ch % 8 == 0
    return np.ascontiguousarray(a.reshape(b, ch // 8, 8, hw).transpose(0, 1, 3, 2))


def unpack_h8(a):
    """[B, C/8, HW, 8] -> [B, C, HW]."""
    b, g8, hw, _ = a.shape
    return np.ascontiguousarray(a.transpose(0, 1, 3, 2).reshape(b, g8 * 8, hw))


def make_case(shape, dt, seed=0):
    """gram_ref.make_case with the tap c and the incoming gradient g0 rounded to the element type (what an h8 map can hold); the Gram target, D
    and the scales stay fp32, as the kernels take them."""
    case = R.make_case(shape, seed)
    case['c'] = round16(case['c'], dt)
    case['g0'] = round16(case['g0'], dt)
    return case


def small_d_case(case):
    """The row of 'd_rounded_before_scaling': D * 2^-18 (fp16 subnormals: |D| ~ 3e-7) under an upstream scale of 2^18."""
    out = dict(case)
    out['d'] = (case['d'].astype(np.float64) * 2.0 ** -18).astype(np.float32)
    out['scale'] = np.array([2.0 ** 18], dtype=np.float32)
    return out


def _as_plane(c):
    """h8 memory read as if it were [C][HW] planes."""
    return pack_h8(c).reshape(c.shape)


def gram_loss(c, gt=None, mistake=None):
    assert mistake in (None,) + MISTAKES
    if mistake == 'chunk_as_plane':
        return R.gram_loss(_as_plane(np.asarray(c)), gt)
    return R.gram_loss(c, gt, mistake=mistake if mistake in R.MISTAKES else None)


def gram_bwd(c, d, dt, scale=None, g0=None, mistake=None):
    """-> dict(g, absg) of the exact float64 result on these inputs, as [B, C, HW]."""
    assert mistake in (None,) + MISTAKES
    if mistake == 'chunk_as_plane':              # tap, incoming gradient and result all misread the same way
        ref = R.gram_bwd(_as_plane(np.asarray(c)), d, scale=scale, g0=None if g0 is None else _as_plane(np.asarray(g0)))
        b, ch, hw = ref['g'].shape
        return dict(g=unpack_h8(ref['g'].reshape(b, ch // 8, hw, 8)), absg=unpack_h8(ref['absg'].reshape(b, ch // 8, hw, 8)))
    if mistake == 'd_rounded_before_scaling':
        d = round16(d, dt)
    if mistake == 'g0_ignored_in_h8':
        g0 = None
    return R.gram_bwd(c, d, scale=scale, g0=g0, mistake=mistake if mistake in R.MISTAKES else None)


gram_bound = R.gram_bound
loss_bound = R.loss_bound


def bwd_bound(ref, ch, dt, g0=None):
    """|g - model| allowed per entry (module docstring)."""
    uh = UH[dt]
    bound = R.bwd_bound(ref, ch, g0)
    bound = bound + uh * ref['absg']
    bound = bound + uh * (np.abs(ref['g']) + bound)
    if dt == 'f16':
        bound = bound + 2.0 ** -25
    if g0 is not None:
        bound = bound + uh * np.abs(ref['g'])
    return bound


def bwd_float32(c, d, dt, scale=None, g0=None, reverse=False):
    """The kernel's arithmetic in float32, for the CPU test: coef * s * D rounded to the element type, fp32 sums over the channels in ascending
    or (``reverse``) descending order, mask, fp32 add of g0, one rounding to the element type."""
    c = np.asarray(c, dtype=np.float32)
    b, ch, hw = c.shape
    s = np.ones(1, np.float32) if scale is None else np.asarray(scale, dtype=np.float32).reshape(-1)
    s = np.broadcast_to(s, (b,))
    f = np.maximum(c, np.float32(0))
    out = np.zeros_like(c)
    order = range(ch - 1, -1, -1) if reverse else range(ch)
    for i in range(b):
        a = round16(np.asarray(d[i], dtype=np.float32) * (np.float32(4.0 * ch / hw) * s[i]), dt)
        acc = np.zeros((ch, hw), np.float32)
        for k in order:
            acc += a[:, k:k + 1] * f[i, k:k + 1, :]
        acc = np.where(c[i] > 0, acc, np.float32(0))
        if g0 is not None:
            acc = acc + np.asarray(g0[i], dtype=np.float32)
        out[i] = round16(acc, dt)
    return out
