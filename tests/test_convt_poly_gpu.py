"""convt_poly_kernel (csrc/l2i_convt_poly.hip), forced through tile_hint 10 of l2i_conv_transpose2d_f32, against F.conv_transpose2d evaluated in float64.

Shapes are the smallest that take each way the kernel can go wrong: widths 32, 34 and 70 (one and several window tiles across, a partial last
window), odd and even heights, batch 1 and 3, Cin of one chunk, of a multiple of 4 that no chunk of 8 / 16 divides (20, 136) and of many ring turns
(256 at 32 x 32), Cout 24 / 32 / 40 / 96 (a partial and several 16-channel blocks), pad 0 and 1, the natural output size and + 3 / + 4.  Forward form
(in_scale, out_scale, out_gain), gradient form (in_mask with both mask value pairs), each operand alone.  Bound: the entry's own,
close(y, ref, 1e-4, 2e-5) of test_fused_transposed_conv_matches_per_parity_launches.

L2I_CONVT_POLY_ERRORS=<file>: the maximum error of the new kernel and of the direct kernel against float64 on the same inputs is appended there
(profiles/convt_poly_errors.txt is such a record)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from latent2im_amd import _lib, conv

pytestmark = pytest.mark.gpu
DEV = 'cuda'
POLY, DIRECT = _lib.CONVT_HINT_POLY, _lib.CONVT_HINT_DIRECT
_RECORD = os.environ.get('L2I_CONVT_POLY_ERRORS')


def close(a, ref, rtol, atol):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    err = (a - ref).abs().max().item()
    bound = atol + rtol * ref.abs().max().item()
    assert err <= bound, 'max err %.3e > %.3e' % (err, bound)


def reference(x, w, pad, ohf, owf):
    """float64 conv_transpose2d(stride 2) of correlation-form w, extended to ohf x owf the way the entry defines it."""
    full = F.conv_transpose2d(x.double(), w.double().transpose(0, 1), stride=2)
    out = torch.zeros(x.shape[0], w.shape[0], ohf, owf, dtype=torch.float64)
    crop = full[:, :, pad:pad + ohf, pad:pad + owf]
    out[:, :, :crop.shape[2], :crop.shape[3]] = crop
    return out


def record(tag, case, y_new, y_dir, ref):
    if _RECORD:
        m = ref.abs().max().item()
        with open(_RECORD, 'a') as f:
            f.write('%-8s %-44s max|ref| %.3e  poly max err %.3e  direct max err %.3e\n' % (
                tag, case, m, (y_new.double().cpu() - ref).abs().max().item(), (y_dir.double().cpu() - ref).abs().max().item()))


CASES = [  # cin, cout, pad, h, w, b, extra rows, extra columns
    (8, 24, 0, 5, 32, 1, 0, 0), (20, 32, 1, 33, 34, 3, 0, 0), (136, 40, 0, 5, 70, 1, 3, 4), (256, 96, 0, 32, 32, 1, 3, 3),
    (16, 32, 1, 5, 70, 3, 4, 3), (8, 40, 0, 33, 32, 1, 0, 0), (20, 24, 1, 34, 34, 1, 3, 3), (64, 96, 1, 33, 70, 1, 0, 0),
]


def _run(fc, x, shape, hint, **kw):
    y = torch.full(shape, float('nan'), device=DEV)
    guard = torch.full((64,), 7.0, device=DEV)          # (allocated right behind y more often than not: a write past y would show)
    fc.forward(x, out=y, tile_hint=hint, **kw)
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    return y


@pytest.mark.parametrize('case', CASES)
def test_forward_form(case):
    cin, cout, pad, h, w_, b, eh, ew = case
    rs = np.random.RandomState(cin + cout + h + w_)
    w = torch.tensor(rs.randn(cout, cin, 3, 3) / np.sqrt(cin * 9), dtype=torch.float32)
    fc = conv.FrozenConv2d(w, 2, pad, transposed=True, device=DEV)
    x = torch.tensor(rs.randn(b, cin, h, w_), dtype=torch.float32)
    s = torch.tensor(rs.rand(b, cin) + 0.5, dtype=torch.float32)
    d = torch.tensor(rs.rand(b, cout) + 0.5, dtype=torch.float32)
    oh, ow = fc.out_hw(h, w_)
    shape = (b, cout, oh + eh, ow + ew)
    g = lambda t: t.to(DEV)
    ref0 = reference(x, w, pad, *shape[2:])
    ref = reference(x * s[:, :, None, None], w, pad, *shape[2:]) * d[:, :, None, None].double() * 0.75
    y = _run(fc, g(x), shape, POLY, in_scale=g(s), out_scale=g(d), out_gain=0.75)
    assert fc.fwd_fused.poly is not None                                         # (the launch took the new kernel: its pack was built)
    close(y, ref, 1e-4, 2e-5)
    record('forward', case, y, _run(fc, g(x), shape, DIRECT, in_scale=g(s), out_scale=g(d), out_gain=0.75), ref)
    # each operand alone, and none
    close(_run(fc, g(x), shape, POLY), ref0, 1e-4, 2e-5)
    close(_run(fc, g(x), shape, POLY, in_scale=g(s)), reference(x * s[:, :, None, None], w, pad, *shape[2:]), 1e-4, 2e-5)
    close(_run(fc, g(x), shape, POLY, out_scale=g(d)), ref0 * d[:, :, None, None].double(), 1e-4, 2e-5)
    close(_run(fc, g(x), shape, POLY, out_gain=0.75), ref0 * 0.75, 1e-4, 2e-5)


@pytest.mark.parametrize('mask', [(1.0, 0.2), (2 ** 0.5, 0.2 * 2 ** 0.5)])
@pytest.mark.parametrize('case', CASES)
def test_gradient_form(case, mask):
    """Input-gradient of a stride-2 conv with a leaky-ReLU mask on the incoming gradient: the conv's Cout is the launch's Cin."""
    cin, cout, pad, h, w_, b, eh, ew = case
    rs = np.random.RandomState(cin + cout + h + w_ + 1)
    wc = torch.tensor(rs.randn(cin, cout, 3, 3) / np.sqrt(cin * 9), dtype=torch.float32)           # conv weight [its Cout = cin][its Cin = cout]
    fc = conv.FrozenConv2d(wc, 2, pad, device=DEV)
    assert fc.bwd_fused is not None
    gy = torch.tensor(rs.randn(b, cin, h, w_), dtype=torch.float32)
    act = torch.tensor(rs.randn(b, cin, h, w_), dtype=torch.float32)
    act[:, :, 0, :4] = 0.0                                                                          # exact zeros take the negative value
    oh, ow = 2 * h + 1 - 2 * pad + eh, 2 * w_ + 1 - 2 * pad + ew
    g = lambda t: t.to(DEV)
    gm = gy.double() * torch.where(act > 0, torch.tensor(mask[0]), torch.tensor(mask[1])).double()
    ref = reference(gm, wc.transpose(0, 1), pad, oh, ow) * 0.5
    run = lambda hint, **kw: _dgrad(fc, g(gy), (b, cout, oh, ow), hint, **kw)
    y = run(POLY, in_mask=g(act), mask=mask, out_gain=0.5)
    assert fc.bwd_fused.poly is not None
    close(y, ref, 1e-4, 2e-5)
    record('gradient', (case, round(mask[0], 3)), y, run(DIRECT, in_mask=g(act), mask=mask, out_gain=0.5), ref)
    close(run(POLY, in_mask=g(act), mask=mask), ref * 2.0, 1e-4, 2e-5)                              # the mask alone


def _dgrad(fc, gy, shape, hint, **kw):
    out = torch.full(shape, float('nan'), device=DEV)
    guard = torch.full((64,), 7.0, device=DEV)
    fc.dgrad(gy, shape[2:], out=out, tile_hint=hint, **kw)
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    return out


def test_ineligible_struct_under_the_force_hint_is_refused():
    lib = _lib.load()
    w = torch.randn(32, 8, 3, 3)
    fc = conv.FrozenConv2d(w, 2, 0, transposed=True, device=DEV)
    x = torch.randn(1, 8, 16, 16, device=DEV)                                                       # 16 positions wide: not the new kernel's
    y = torch.empty(1, 32, 33, 33, device=DEV)
    with pytest.raises(_lib.L2IError, match='-3'):
        fc.forward(x, out=y, tile_hint=POLY)
    p = conv._conv_params(x, fc.fwd_fused.w, y, 1, 8, 16, 16, 32, 3, 3, 2, 0, 0, 17, 17, 33, 33, 2)
    p.tile_hint = POLY
    assert lib.l2i_conv_transpose2d_f32(ctypes.byref(p), _lib.stream_ptr()) == -3                  # L2I_E_UNSUPPORTED
    x = torch.randn(1, 8, 32, 32, device=DEV)
    y = torch.empty(1, 32, 65, 65, device=DEV)
    p = conv._conv_params(x, fc.fwd_fused.w, y, 1, 8, 32, 32, 32, 3, 3, 2, 0, 0, 33, 33, 65, 65, 2)
    p.tile_hint = POLY
    assert lib.l2i_conv_transpose2d_f32(ctypes.byref(p), _lib.stream_ptr()) == -1                  # eligible, but no pack in w_lo: L2I_E_ARG
    fc7 = conv.FrozenConv2d(torch.randn(8, 8, 7, 7), 2, 3, device=DEV)
    with pytest.raises(_lib.L2IError, match='-3'):
        fc7.dgrad(torch.randn(1, 8, 32, 32, device=DEV), (64, 64), tile_hint=POLY)
    torch.cuda.synchronize()


def test_a_weight_on_the_device_stays_on_the_direct_kernel():
    """A net that is being trained builds its FrozenConv2d from a CUDA weight every step: no 25-plane repack; hint 0 launches never build one either
    on a shape outside the measured table."""
    fc = conv.FrozenConv2d(torch.randn(32, 8, 3, 3, device=DEV), 2, 0, transposed=True, device=DEV)
    assert fc.fwd_fused.poly_src is None
    fh = conv.FrozenConv2d(torch.randn(32, 8, 3, 3), 2, 0, transposed=True, device=DEV)
    fh.forward(torch.randn(1, 8, 5, 34, device=DEV))
    assert fh.fwd_fused.poly_src is not None and fh.fwd_fused.poly is None
