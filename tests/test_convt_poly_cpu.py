"""The 25-product form of the stride-2 transposed 3x3 conv (csrc/l2i_convt_poly.hip), without a GPU.

1. A numpy float64 emulation of what the kernel computes — the 25-plane pack (conv.pack_weight_convt_poly, the function the product uses, asked for
   float64), the input transform of a 3x3 raw patch per window, the 25 products and the inverse transform into a 4x4 output patch — equals
   F.conv_transpose2d(stride=2) in float64 to 1e-12: pad 0 and 1, odd and even H and W (including one more than a multiple of 2), natural and
   padded output sizes.
2. The kernel's launch plan (l2i_convt_poly_plan_for, a host function of the struct) is checked for bounds: tiles cover the windows, every window's
   raw patch lies inside the staged tile, the DMA slots of a channel plane stay inside its LDS pitch, the stages fit the LDS budget, the block
   order is a permutation — and the LDS image the plan describes, filled as the DMA fills it, hands every window the raw values the emulation uses."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from latent2im_amd import _lib, conv

BIDX = {0: (0, 1, 2, 1, 3), 1: (0, 1, 2, 3, 1)}     # product -> which of the four distinct transformed values (r0 - r1, r1, r1 - r2, r2 | r0) it multiplies
OUT = {0: ((0, 1, +1), (3, 3, 0), (1, 2, -1), (4, 4, 0)),       # output 4W + i = m[a] + sign * m[b]  (sign 0: m[a] alone)
       1: ((3, 3, 0), (0, 1, +1), (4, 4, 0), (1, 2, -1))}


def reference(x, w, pad, ohf, owf):
    """conv_transpose2d(stride 2) of correlation-form w [Cout, Cin, 3, 3], its natural extension to ohf x owf (rows no input reaches: zeros)."""
    full = F.conv_transpose2d(x, w.transpose(0, 1), stride=2)                      # pad 0: 2H + 1 rows
    out = torch.zeros(x.shape[0], w.shape[0], ohf, owf, dtype=x.dtype)
    crop = full[:, :, pad:pad + ohf, pad:pad + owf]
    out[:, :, :crop.shape[2], :crop.shape[3]] = crop
    return out


def raw_patches(x, pad, nwy, nwx):
    """[3][3] arrays [B, Cin, nwy, nwx]: raw value (dy, dx) of window (wy, wx) = x[2 wy - 1 + pad + dy, 2 wx - 1 + pad + dx], zero outside."""
    B, C, H, W = x.shape
    xp = np.zeros((B, C, 2 * nwy + 3, 2 * nwx + 3))
    o = 1 - pad
    h, w = min(H, xp.shape[2] - o), min(W, xp.shape[3] - o)
    xp[:, :, o:o + h, o:o + w] = x[:, :, :h, :w]
    return [[xp[:, :, dy:dy + 2 * nwy:2, dx:dx + 2 * nwx:2] for dx in range(3)] for dy in range(3)]


def transform_1d(r, pad):
    return [r[0] - r[1], r[1], r[1] - r[2], r[2] if pad == 0 else r[0]]


def emulate(x, w, pad, ohf, owf):
    x = np.asarray(x, dtype=np.float64)
    cout = w.shape[0]
    U = conv.pack_weight_convt_poly(w, dtype=torch.float64).numpy()[:, :, :cout]     # [Cin, 25, Cout]
    nwy, nwx = (ohf + 3) // 4, (owf + 3) // 4
    r = raw_patches(x, pad, nwy, nwx)
    R = [transform_1d([r[0][c], r[1][c], r[2][c]], pad) for c in range(3)]           # R[c][a]: rows transformed, column c
    T = [transform_1d([R[0][a], R[1][a], R[2][a]], pad) for a in range(4)]           # T[a][b]
    M = [[np.einsum('bcyx,co->boyx', T[BIDX[pad][a]][BIDX[pad][b]], U[:, 5 * a + b, :]) for b in range(5)] for a in range(5)]
    y = np.zeros((x.shape[0], cout, 4 * nwy, 4 * nwx))
    for i, (a0, a1, sa) in enumerate(OUT[pad]):
        row = [M[a0][b] + sa * M[a1][b] if sa else M[a0][b] for b in range(5)]
        for j, (b0, b1, sb) in enumerate(OUT[pad]):
            y[:, :, i::4, j::4] = row[b0] + sb * row[b1] if sb else row[b0]
    return y[:, :, :ohf, :owf]


SHAPES = [(5, 6), (6, 5), (7, 9), (8, 8), (1, 3), (2, 2), (33, 32)]


@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('hw', SHAPES)
def test_emulation_equals_conv_transpose2d(pad, hw):
    h, w_ = hw
    rs = np.random.RandomState(h * 100 + w_ + pad)
    x = torch.tensor(rs.randn(2, 4, h, w_))
    w = torch.tensor(rs.randn(3, 4, 3, 3))
    nat_h, nat_w = 2 * h + 1 - 2 * pad, 2 * w_ + 1 - 2 * pad
    for eh, ew in ((0, 0), (3, 4), (4, 3), (8, 8), (1, 0)):
        ref = reference(x, w, pad, nat_h + eh, nat_w + ew).numpy()
        got = emulate(x.numpy(), w, pad, nat_h + eh, nat_w + ew)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12, (pad, hw, eh, ew, np.abs(got - ref).max())
    if pad == 1 and h > 1 and w_ > 1:      # one row / column past the natural size is torch's own output_padding
        ref1 = F.conv_transpose2d(x, w.transpose(0, 1), stride=2, padding=1, output_padding=1).numpy()
        assert np.abs(emulate(x.numpy(), w, 1, nat_h + 1, nat_w + 1) - ref1).max() <= 1e-12


def test_pack_planes_are_sums_of_at_most_four_taps_rounded_once():
    rs = np.random.RandomState(3)
    w = torch.tensor(rs.randn(40, 8, 3, 3), dtype=torch.float32)
    pk = conv.pack_weight_convt_poly(w)
    assert tuple(pk.shape) == (8, 25, 64) and pk.dtype == torch.float32 and float(pk[:, :, 40:].abs().max()) == 0.0
    g = [[2], [0, 2], [0], [1], [1]]
    wd = w.double()
    for a in range(5):
        for b in range(5):
            want = sum(wd[:, :, ky, kx] for ky in g[a] for kx in g[b])
            assert len(g[a]) * len(g[b]) <= 4
            assert torch.equal(pk[:, 5 * a + b, :40], want.float().t())
    assert torch.equal(pk[:, 20:25], pk[:, 15:20]) and torch.equal(pk[:, 4::5], pk[:, 3::5])      # the repeated planes the kernel does not stage


def _params(B, cin, cout, h, w, pad, eh=0, ew=0, masked=False, **kw):
    p = _lib.ConvParams()
    p.B, p.Cin, p.H, p.W, p.Cout, p.CoutP = B, cin, h, w, cout, (cout + 31) // 32 * 32
    p.KH = p.KW = 3
    p.stride, p.pad_y, p.pad_x = 2, pad, pad
    p.OHf, p.OWf = 2 * h + 1 - 2 * pad + eh, 2 * w + 1 - 2 * pad + ew
    p.OH, p.OW = (p.OHf + 1) // 2, (p.OWf + 1) // 2
    p.oy_step = p.ox_step = 2
    p.out_gain = 1.0
    if masked:
        p.in_mask = ctypes.c_void_p(16)         # (host-only queries never dereference it)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _plan(p):
    lib = _lib.load()
    plan = _lib.ConvtPolyPlan()
    assert lib.l2i_convt_poly_plan_for(ctypes.byref(p), ctypes.byref(plan)) == 0
    return plan


PLAN_CASES = [  # B, cin, cout, h, w, pad, eh, ew, masked
    (1, 8, 24, 5, 32, 0, 0, 0, False), (3, 20, 32, 33, 34, 1, 0, 0, True), (1, 136, 40, 5, 70, 0, 3, 4, False), (1, 256, 96, 32, 32, 0, 3, 3, False),
    (8, 64, 32, 512, 512, 0, 3, 3, False), (8, 128, 64, 256, 256, 0, 3, 3, False), (8, 512, 512, 32, 32, 0, 3, 3, False), (8, 512, 256, 64, 64, 0, 3, 3, False),
    (8, 128, 64, 257, 257, 0, 0, 0, False), (8, 64, 32, 513, 513, 0, 0, 0, True), (8, 512, 512, 33, 33, 0, 0, 0, True), (2, 128, 128, 56, 56, 1, 0, 0, True),
    (1, 4, 3, 33, 47, 1, 4, 3, True), (1, 12, 16, 40, 126, 0, 8, 8, False),
]


@pytest.mark.parametrize('case', PLAN_CASES)
def test_launch_plan_stays_in_bounds(case):
    B, cin, cout, h, w, pad, eh, ew, masked = case
    p = _params(B, cin, cout, h, w, pad, eh, ew, masked)
    pl = _plan(p)
    assert pl.eligible == 1 and pl.masked == int(masked)
    assert _lib.load().l2i_conv_transpose2d_family(ctypes.byref(_params(B, cin, cout, h, w, pad, eh, ew, masked, tile_hint=_lib.CONVT_HINT_POLY))) == _lib.TFAMILY_POLY
    # windows and tiles
    assert pl.nwx * 4 >= p.OWf > (pl.nwx - 1) * 4 and pl.nwy * 4 >= p.OHf > (pl.nwy - 1) * 4
    assert 1 <= pl.WTW and 1 <= pl.WTH and pl.WTW * pl.WTH <= 64
    assert pl.tiles_x * pl.WTW >= pl.nwx > (pl.tiles_x - 1) * pl.WTW and pl.tiles_y * pl.WTH >= pl.nwy > (pl.tiles_y - 1) * pl.WTH
    assert pl.mblocks * 16 >= cout > (pl.mblocks - 1) * 16 and pl.mblocks * 16 <= p.CoutP
    assert pl.total == B * pl.tiles_x * pl.tiles_y * pl.mblocks and pl.grid % 8 == 0 and pl.total <= pl.grid < pl.total + 8
    g8 = pl.grid >> 3
    if pl.grid <= 1 << 16:
        assert sorted((blk & 7) * g8 + (blk >> 3) for blk in range(pl.grid)) == list(range(pl.grid))      # the block order is a permutation
    # raw tile, halo, DMA slots
    assert pl.org == pad - 1 and pl.IH == 2 * pl.WTH + 1 and pl.IW == 2 * pl.WTW + 1
    assert pl.IH * pl.IW <= pl.nslots * 64 < pl.IH * pl.IW + 64 and 1 <= pl.nslots <= 6
    assert pl.plane >= pl.nslots * 64 and pl.plane % 2 == 1
    assert (2 * (pl.WTH - 1) + 2) * pl.IW + 2 * (pl.WTW - 1) + 2 < pl.IH * pl.IW                  # the last window's last raw value
    # stages
    assert pl.CK % 4 == 0 and pl.CK >= 4 and cin % pl.CK == 0 and pl.wpitch >= 256 and pl.wpitch % 4 == 0
    in_f = pl.CK * pl.plane
    assert (in_f * 4) % 16 == 0                                                                    # the weight image starts on a 16-byte boundary
    need = in_f * (2 if masked else 1) + pl.CK * pl.wpitch + pl.CK
    assert need <= pl.stage_floats and pl.stage_floats % 4 == 0 and pl.lds_bytes == 8 * pl.stage_floats <= 52 * 1024
    assert cin * h * w * 4 < 0x7FFF0000


def test_plan_image_hands_every_window_its_raw_patch():
    """Fill one channel's LDS plane as the DMA does (element e = 64 s + lane of the dense IH x IW tile <- x[iy0 + e // IW, ix0 + e % IW], zero outside the
    map) and read every window's 3x3 patch at 2 wrow * IW + 2 wcol + dy * IW + dx: it is the patch the emulation transforms."""
    for (h, w, pad, eh, ew) in ((5, 34, 0, 3, 4), (33, 32, 1, 0, 0), (6, 70, 0, 0, 0), (9, 33, 1, 4, 3)):
        p = _params(1, 4, 8, h, w, pad, eh, ew)
        pl = _plan(p)
        x = np.random.RandomState(h + w).randn(1, 1, h, w)
        r = raw_patches(x, pad, pl.nwy, pl.nwx)
        for ty in range(pl.tiles_y):
            for tx in range(pl.tiles_x):
                iy0, ix0 = 2 * ty * pl.WTH + pl.org, 2 * tx * pl.WTW + pl.org
                img = np.full(pl.plane, np.nan)
                for e in range(pl.nslots * 64):
                    gy, gx = iy0 + e // pl.IW, ix0 + e % pl.IW
                    ok = e // pl.IW < pl.IH and 0 <= gy < h and 0 <= gx < w
                    if ok:
                        assert (gy * w + gx) * 4 < h * w * 4
                    img[e] = x[0, 0, gy, gx] if ok else 0.0
                for n in range(64):
                    wrow, wcol = divmod(n, pl.WTW)
                    wy, wx = ty * pl.WTH + wrow, tx * pl.WTW + wcol
                    if wrow >= pl.WTH or wy >= pl.nwy or wx >= pl.nwx:
                        continue
                    for dy in range(3):
                        for dx in range(3):
                            assert img[(2 * wrow + dy) * pl.IW + 2 * wcol + dx] == r[dy][dx][0, 0, wy, wx]


def test_ineligible_structs_report_no_plan_and_the_direct_family():
    lib = _lib.load()
    bad = [_params(1, 8, 8, 16, 16, 0), _params(1, 6, 8, 32, 32, 0), _params(1, 8, 8, 32, 32, 1, eh=9), _params(1, 8, 8, 32, 32, 0, in_h8=1),
           _params(1, 8, 8, 32, 32, 0, ksplit=4, ws=ctypes.c_void_p(16)), _params(1, 8, 8, 32, 32, 0, KH=7, KW=7, pad_y=3, pad_x=3)]
    for p in bad:
        assert _plan(p).eligible == 0
        p.tile_hint = _lib.CONVT_HINT_POLY
        assert lib.l2i_conv_transpose2d_family(ctypes.byref(p)) == _lib.TFAMILY_DIRECT
    assert lib.l2i_conv_transpose2d_family(None) == -1
    # tile_hint 0 follows the launcher's table: the generator's five up-layer shapes (forward form, any batch, natural or padded output) and nothing else
    fam = lambda *a, **k: lib.l2i_conv_transpose2d_family(ctypes.byref(_params(*a, **k)))
    for cin, cout, h in ((512, 512, 32), (512, 256, 64), (256, 128, 128), (128, 64, 256), (64, 32, 512)):
        assert fam(8, cin, cout, h, h, 0, 3, 3) == _lib.TFAMILY_POLY and fam(2, cin, cout, h, h, 0) == _lib.TFAMILY_POLY
        assert fam(8, cin, cout, h, h, 0, 3, 3, masked=True) == _lib.TFAMILY_DIRECT          # masked launches stay on the direct kernel
        assert fam(8, cin, cout, h, h, 1) == _lib.TFAMILY_DIRECT and fam(8, cin, cout, h, h + 4, 0) == _lib.TFAMILY_DIRECT
        assert fam(8, cin, cout, h, h, 0, ksplit=4, ws=ctypes.c_void_p(16)) == _lib.TFAMILY_DIRECT
    for off in ((8, 512, 512, 64, 64, 0), (8, 128, 128, 64, 64, 1, 0, 0, True), (8, 256, 256, 32, 32, 1, 0, 0, True), (8, 64, 64, 512, 512, 0), (1, 8, 24, 5, 32, 0)):
        assert fam(*off) == _lib.TFAMILY_DIRECT
    assert lib.l2i_convt_poly_plan_for(None, None) == -1
    for hint in (1, 2, 3, 8, _lib.CONVT_HINT_DIRECT):                                     # the direct kernel's hints never report the new family
        assert lib.l2i_conv_transpose2d_family(ctypes.byref(_params(8, 64, 32, 512, 512, 0, 3, 3, tile_hint=hint))) == _lib.TFAMILY_DIRECT


def test_family_info_and_header():
    kern, ratio, peak = conv.FAMILY_INFO['transposed_poly_f32']
    assert kern == 'convt_poly_kernel' and ratio == 25.0 / 36.0 and peak == 157.3
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'l2i.h')).read()
    for name in ('l2i_conv_transpose2d_family', 'l2i_convt_poly_plan_for', 'L2I_CONVT_HINT_DIRECT 9', 'L2I_CONVT_HINT_POLY 10', 'L2I_TFAMILY_POLY 1'):
        assert name in hdr
    assert ctypes.sizeof(_lib.ConvtPolyPlan) == 80


def test_a_cuda_weight_keeps_no_poly_source():
    """A net that is being trained hands FusedTransposed a CUDA weight every step: no 25-plane repack, it stays on the direct kernel."""
    Fz = conv.FusedTransposed(torch.randn(8, 8, 3, 3), 0)
    assert Fz.poly_src is not None and Fz.poly is None
    assert conv.FusedTransposed(torch.randn(8, 8, 7, 7), 3).poly_src is None and conv.FusedTransposed(torch.randn(8, 6, 3, 3), 1).poly_src is None
