"""The contract of the 16-bit trainer's stem gradient and of its weight-plane repack (csrc/l2i_train_h8.hip; include/l2i.h: l2i_conv2d_wgrad_img_h8,
l2i_conv2d_wgrad_img_ws_h8, l2i_repack_planes_h8 and their _f16 twins), written once with derived bounds, and the case tables that drive
tests/test_stemgrad16_gpu.py, tests/test_planes16_gpu.py and tests/test_regtrain16_repro_gpu.py (checked on the CPU by
tests/test_stemgrad16_ref_cpu.py).

Stem gradient.  The operands are what the kernel reads: gy rounded to the element type (bf16 or IEEE fp16, round to nearest even), x as the
float32 image it is — NOT rounded to 16 bits.  Then, in float64:

    dw[co,ci,ky,kx] = sum_{b,oy,ox} gy[b,co,oy,ox] * x[b,ci,2*oy+ky-3,2*ox+kx-3]          (reads in the padding give 0; OH = (H-1)/2+1, OW alike)

Bound (nothing here is measured on a kernel).  A 16-bit value times a float32 value has up to 35 significant bits: the product rounds once, and the
N = B OH OW additions round once each, 2^-23 per pixel for the two together (twice the unit roundoff of one fused multiply-add: the matrix
pipe's internal adds are not promised to round to nearest), + 2 for the tree that joins the partial sums, relative to M = sum |gy| |x|:
bound = 2^-23 (N + 2) M.  A tap that only ever reads padding has M = 0 and must be exactly 0.

Planes.  l2i_repack_planes_h8 is a pure data movement with one rounding per element, so its contract is bit equality: ``planes_np`` states the
element formula of include/l2i.h in numpy, independently of conv.pack_weight_h8 / pack_weight_img_h8 (which the library's host side uses), with
the roundings done by numpy (fp16) or on the bit pattern (bf16).

MISTAKES are seeded errors; CASES name the ones each case must expose (tests/test_stemgrad16_ref_cpu.py proves that each breaks the bound there
and that a float32 evaluation stays inside it).  A plain module: no fixtures, no kernel code."""
from collections import namedtuple

import numpy as np
import torch

from tests.stream_ref import U23, ELEM_DTYPES, rnd_for, worst      # noqa: F401 (shared, re-exported)

ELEMS = ('bf16', 'f16')
SENTINEL = -7680.0            # exactly representable in fp32, bf16 and fp16
K, STRIDE, PAD, CIN, COUT = 7, 2, 3, 3, 64
SLICE_BYTES = 64 * 160 * 4    # L2I_WGRAD_IMG_SLICE_BYTES: the workspace of one pixel slice

MISTAKES = ('dropped_tap', 'tap_shifted', 'ky_kx_swapped', 'padding_as_data', 'stride_ignored', 'ci_swapped', 'slice_tail_dropped', 'x_rounded_to_elem')

StemCase = namedtuple('StemCase', 'name b h w mistakes')
# (the cases of the issue.  one_pixel: only the centre tap is data; even: the last tap row and column fall in the bottom and right padding;
#  slices: at least three pixel slices and more than one per sample — the GPU test asserts that through the workspace query)
CASES = (
    StemCase('one_pixel', 1, 1, 1, ('padding_as_data', 'x_rounded_to_elem')),
    StemCase('two', 1, 2, 2, ('ky_kx_swapped', 'ci_swapped')),
    StemCase('odd', 3, 9, 13, ('dropped_tap', 'tap_shifted', 'stride_ignored', 'slice_tail_dropped', 'x_rounded_to_elem')),
    StemCase('even', 2, 10, 6, ('padding_as_data', 'x_rounded_to_elem')),
    StemCase('square', 2, 12, 12, ('ky_kx_swapped', 'dropped_tap', 'stride_ignored')),
    StemCase('slices', 2, 96, 80, ('tap_shifted', 'ci_swapped', 'slice_tail_dropped')),
)
# (what changes, value): each must be refused with a message and leave every sentinel intact
REFUSALS = (('cin', 4), ('cout', 32), ('ws', None), ('ws_bytes', 'short'), ('gy', 'misaligned'))


def out_size(n):
    return (n - 1) // 2 + 1


def pixels(case):
    return case.b * out_size(case.h) * out_size(case.w)


def _d(t, rnd=None):
    t = torch.as_tensor(t).detach().cpu().float()
    return (t if rnd is None else rnd(t)).double()


def data(case, seed=0):
    """(x [B,3,H,W], gy [B,64,OH,OW]) float32, seeded by the case's name."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.name)))
    x = torch.randn(case.b, CIN, case.h, case.w, generator=g)
    gy = torch.randn(case.b, COUT, out_size(case.h), out_size(case.w), generator=g) * 0.5
    return x, gy


def _tap_view(xp, ky, kx, stride, oh, ow):
    return xp[:, :, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride]


def stem_wgrad(x, gy, elem, dt=torch.float64, _mistake=None):
    """(want, bound): dw [64, 3, 7, 7] in ``dt`` (float64: the model; float32: the emulation the CPU test holds against the bound) and the bound
    per element."""
    assert _mistake is None or _mistake in MISTAKES, _mistake
    rnd = rnd_for(elem)
    gg = _d(gy, rnd).to(dt)
    xx = _d(x, rnd if _mistake == 'x_rounded_to_elem' else None).to(dt)
    b, cin, h, w = xx.shape
    _, cout, oh, ow = gg.shape
    assert (oh, ow) == (out_size(h), out_size(w))
    s = 1 if _mistake == 'stride_ignored' else STRIDE
    margin = 1 + STRIDE * max(oh, ow)                       # room for the shifted read of tap_shifted and for every legitimate read of an even side
    mode = 'replicate' if _mistake == 'padding_as_data' else 'constant'

    def padded(t):
        if mode == 'replicate':
            t = torch.nn.functional.pad(t, (PAD, PAD, PAD, PAD), mode='replicate')
            return torch.nn.functional.pad(t, (0, margin, 0, margin))
        return torch.nn.functional.pad(t, (PAD, PAD + margin, PAD, PAD + margin))
    xp, xa = padded(xx), padded(xx.abs())
    if _mistake == 'slice_tail_dropped':                  # the last output row of every sample (the tail of its last row slice) contributes nothing
        gg = gg.clone()
        gg[:, :, oh - 1] = 0
    want, M = torch.zeros(cout, cin, K, K, dtype=dt), torch.zeros(cout, cin, K, K, dtype=torch.float64)
    ga = _d(gy, rnd).abs()
    for ky in range(K):
        for kx in range(K):
            M[:, :, ky, kx] = torch.einsum('bohw,bihw->oi', ga, _tap_view(xa, ky, kx, STRIDE, oh, ow).double())
            if _mistake == 'dropped_tap' and (ky, kx) == (K - 1, K - 1):
                continue
            sx = kx + 1 if (_mistake == 'tap_shifted' and (ky, kx) == (0, 0)) else kx
            want[:, :, ky, kx] = torch.einsum('bohw,bihw->oi', gg, _tap_view(xp, ky, sx, s, oh, ow))
    if _mistake == 'ky_kx_swapped':
        want = want.transpose(2, 3).contiguous()
    if _mistake == 'ci_swapped':
        want = want[:, [1, 0, 2]].contiguous()
    bound = U23 * (b * oh * ow + 2) * M
    return want, bound


# ---- weight planes ----------------------------------------------------------------------------------------------------------------------------------
FWD, SWAP, FLIP, IMG = 0, 1, 2, 3          # L2I_PLANES_*
PLANTED = (70000.0, 1e-6, -3e-8, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -8, -0.0)      # fp16 overflow, subnormal, half the smallest subnormal, an fp16 tie, a bf16 tie, -0

PlaneCase = namedtuple('PlaneCase', 'name cout cin k stride pad qpad transposed')
PLANE_CASES = (
    PlaneCase('c40x24_1x1', 40, 24, 1, 1, 0, 32, False),
    PlaneCase('c64x16_3x3_q16', 64, 16, 3, 1, 1, 16, False),
    PlaneCase('c32x72_3x3_s2', 32, 72, 3, 2, 1, 32, False),
    PlaneCase('c96x64_1x1_s2', 96, 64, 1, 2, 0, 32, False),
    PlaneCase('c48x40_3x3_tr', 48, 40, 3, 2, 1, 32, True),
    PlaneCase('stem', 64, 3, 7, 2, 3, 16, False),
)


def plane_weight(case, seed=0):
    """[Cout, Cin, K, K] float32 randn, seeded by the case's name, with PLANTED in its first elements."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.name)))
    w = torch.randn(case.cout, case.cin, case.k, case.k, generator=g)
    w.view(-1)[:len(PLANTED)] = torch.tensor(PLANTED, dtype=torch.float32)
    return w


def plane_modes(case):
    """[(attribute of the conv object, mode, qpad)] of a case: the stem has one plane set, every other convolution two."""
    if case.name == 'stem':
        return [('planes', IMG, 16)]
    return [('fwd_planes', FWD, case.qpad), ('bwd_planes', SWAP if case.transposed or case.stride == 2 else FLIP, 32)]


def round_bits(a, elem):
    """float32 array -> the uint16 bit patterns of its elements rounded to nearest even to ``elem``."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if elem == 'f16':
        with np.errstate(over='ignore'):
            return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)                  # (no NaN among the weights)


def planes_np(w, mode, qpad, elem):
    """The plane set of include/l2i.h's element formula as uint16 bit patterns [groups][taps][2][ceil32(rows)][8]."""
    w = np.asarray(w, dtype=np.float32)
    cout, cin, k, _ = w.shape
    if mode == IMG:
        rows, contr, groups, taps = cout, cin * k, (cin * k + 1) // 2, 1
    else:
        rows, contr = (cout, cin) if mode == FWD else (cin, cout)
        groups, taps = (contr + qpad - 1) // qpad * qpad // 16, k * k
    out = np.zeros((groups, taps, 2, (rows + 31) // 32 * 32, 8), dtype=np.float32)
    for g in range(groups):
        for half in range(2):
            if mode == IMG:
                j = 2 * g + half
                if j < contr:
                    c, ky = divmod(j, k)
                    out[g, 0, half, :rows, :k] = w[:, c, ky, :]
                continue
            for t in range(taps):
                tt = taps - 1 - t if mode == FLIP else t
                for e in range(8):
                    q = 16 * g + 8 * half + e
                    if q < contr:
                        out[g, t, half, :rows, e] = w[:, q, tt // k, tt % k] if mode == FWD else w[q, :, tt // k, tt % k]
    return round_bits(out, elem)
