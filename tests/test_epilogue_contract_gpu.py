"""Every kernel's fused conv prologue / epilogue (include/l2i.h: pro / epi / R) against ONE float64 model (tests/epilogue_ref.py), term by
term: route x case.  A route is one kernel (one kernel's composition of the shared terms of csrc/l2i_epilogue.h, or an epilogue a kernel keeps
inline) reached through the dispatch the product uses; a new composition is a new route.  A route asserts the entry point
and kernel family that ran, so a dispatch change cannot empty a row silently.  A case sets one contract field alone, or a combination that exists
to expose one term-order mistake (tests/test_epilogue_ref_cpu.py proves that it can).  Masks hold exact +-0.0; every output is carved from a larger
buffer filled with a sentinel and everything outside the launch window must come back bit-identical.  A field a route does not implement must move
the launch to a kernel that does (the recorded family says which) or be refused with y untouched: never ignored.

Bounds are the ones the suite already asserts per family (max|got - ref| / max|ref|): 5e-6 exact-fp32 kernels and the fp32 pair, 3e-5 F(4x4), 2e-5
bf16x3 (test_bf16x3_split_precision_conv).

The 16-bit (h8) epilogues of l2i_conv_h8.hip / l2i_img_h8.hip have another contract (leaky output mask, sign-plane masks): their matrix is
tests/test_epilogue16_contract_gpu.py, against tests/epilogue16_ref.py; the pair / chain3 kernels of l2i_pair_h8.hip are held bit for bit to separate
l2i_conv2d_h8 launches by tests/test_h8_gpu.py, whose operand sets that matrix contains."""
from collections import namedtuple
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, conv
from tests import epilogue_ref as er

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SLACK = 64          # floats of sentinel on each side of y
BOUND = {'implicit_gemm_f32': 5e-6, 'gemm1x1_f32': 5e-6, 'cin3_f32': 5e-6, 'direct_small_valu': 5e-6, 'transposed_f32': 5e-6, 'winograd_f32': 5e-6,
         'winograd4_f32': 3e-5, 'implicit_gemm_bf16x3': 2e-5, 'transposed_bf16x3': 2e-5}          # (the last: test_bf16x3_transposed_conv's)
SWITCHES = ('WINO4', 'USE_WINOGRAD', 'PRECISION', 'SPLIT_K', 'WINO4_R4_MIN_W', 'USE_FUSED_TRANSPOSED')

ALLF = frozenset(er.FIELDS) - {'sq'}
GENERIC = ('l2i_conv2d_f32', 'implicit_gemm_f32')
F2 = ('l2i_conv2d_wino_f32', 'winograd_f32')

# kind: 'fwd' = FrozenConv2d.forward, 'tfwd' = forward of a stride-2 transposed conv, 'dgrad' = input gradient of a stride-2 conv (a transposed
# conv of the gradient), 'parity' = the four per-parity launches of a transposed conv one by one.  shape = (cin, cout, k, stride, pad, h, w, batch)
# of the launch's INPUT.  accepts = the fields the kernel fuses; moved(fields) = where a launch with other fields must land instead.
Route = namedtuple('Route', 'name kind shape ran accepts moved switches hint misalign proof', defaults=(None, {}, 0, None, None))
# proof: the name of a kernel that shares its entry point and family with another one; the test then checks the library's own conditions for it
# on the shape and the fields (KERNEL_TAKES), so that such a row cannot drift to the other kernel unseen.


def _small7_moved(fields):          # per-parity launches onto 3 channels: the direct VALU kernel unless an epilogue operand needs the generic one
    return GENERIC if set(fields) & {'out_scale', 'noise', 'bias', 'residual', 'out_mask', 'lrelu', 'relu'} else ('l2i_conv2d_f32', 'direct_small_valu')


_generic = lambda f: GENERIC
ROUTES = [
    # generic implicit GEMM, vector epilogue: maps under 32 wide stay off Winograd; automatic tile and the forced (4,2), (2,2), (2,1) tiles
    *[Route('generic_vec_hint%d' % h, 'fwd', (40, 48, 3, 1, 1, 20, 20, 2), GENERIC, ALLF, hint=h) for h in (0, 1, 2, 4)],
    Route('generic_scalar_odd_shape', 'fwd', (40, 48, 3, 1, 1, 19, 21, 2), GENERIC, ALLF),
    Route('generic_scalar_misaligned_out', 'fwd', (40, 48, 3, 1, 1, 20, 20, 2), GENERIC, ALLF, misalign='out'),
    Route('generic_scalar_misaligned_residual', 'fwd', (40, 48, 3, 1, 1, 20, 20, 2), GENERIC, ALLF, misalign='residual'),
    Route('generic_1x1_stride2_gather', 'fwd', (16, 24, 1, 2, 0, 16, 16, 1), GENERIC, ALLF),
    Route('generic_window_step_offset', 'parity', (12, 20, 3, 2, 0, 8, 8, 2), GENERIC, ALLF, switches={'USE_FUSED_TRANSPOSED': False}),
    # 3x3 stride-2 DMA kernel: same entry and family as the generic kernel, which takes its masked launches (l2i_conv3x3s2_eligible: no in_mask), so
    # the row proves the DMA kernel's conditions on every case it claims; the last: Cout % 32 != 0
    Route('s2_dma_p1', 'fwd', (16, 64, 3, 2, 1, 64, 64, 2), GENERIC, ALLF - {'in_mask', 'relu_in'}, _generic, proof='conv3x3s2_dma'),
    Route('s2_dma_p0_odd', 'fwd', (8, 64, 3, 2, 0, 67, 67, 1), GENERIC, ALLF - {'in_mask', 'relu_in'}, _generic, proof='conv3x3s2_dma'),
    Route('s2_dma_ragged_cout', 'fwd', (16, 40, 3, 2, 1, 64, 64, 1), GENERIC, ALLF - {'in_mask', 'relu_in'}, _generic, proof='conv3x3s2_dma'),
    # 1x1 DMA GEMM: no style scale (those launches take the generic kernel); 64 -> 256 is the CoutP % 128 == 0 shape of test_gemm_1x1_conv, but NO shape
    # here takes the 128-channel tile (l2i_launch_gemm1x1 wants B * tiles * CoutP / 128 >= 512 blocks and, unmasked, Cin * 4 > Cout: two samples of
    # 256x256 at the least, too large for this file): all three run gemm1x1_kernel<2, ..>, whose epilogue code the <4, ..> form shares; the last: Cout % 32 != 0
    Route('gemm1x1', 'fwd', (16, 64, 1, 1, 0, 64, 64, 1), ('l2i_conv2d_f32', 'gemm1x1_f32'), ALLF - {'in_scale'}, _generic),
    Route('gemm1x1_coutp128', 'fwd', (64, 256, 1, 1, 0, 32, 32, 2), ('l2i_conv2d_f32', 'gemm1x1_f32'), ALLF - {'in_scale'}, _generic),
    Route('gemm1x1_ragged_cout', 'fwd', (16, 40, 1, 1, 0, 64, 64, 1), ('l2i_conv2d_f32', 'gemm1x1_f32'), ALLF - {'in_scale'}, _generic),
    Route('split_k', 'fwd', (256, 96, 3, 1, 1, 8, 8, 2), GENERIC, ALLF, proof='split_k'),
    Route('split_k_ragged_cout', 'fwd', (256, 88, 3, 1, 1, 8, 8, 2), GENERIC, ALLF, proof='split_k'),
    Route('wino2', 'fwd', (16, 40, 3, 1, 1, 36, 36, 1), F2, ALLF | {'sq'}, switches={'WINO4': 'off'}),
    # F(4x4): unmasked launches only, a general in_mask goes to F(2x2)
    Route('wino4_all', 'fwd', (16, 40, 3, 1, 1, 18, 72, 1), ('l2i_conv2d_wino4_f32', 'winograd4_f32'), (ALLF | {'sq'}) - {'in_mask'}, lambda f: F2,
          {'WINO4': 'all'}),
    Route('wino4_r4', 'fwd', (16, 40, 3, 1, 1, 18, 72, 1), ('l2i_conv2d_wino4_f32', 'winograd4_f32'), (ALLF | {'sq'}) - {'in_mask'}, lambda f: F2,
          {'WINO4': 'r4', 'WINO4_R4_MIN_W': 32}),
    Route('wino4_tall', 'fwd', (16, 40, 3, 1, 1, 16, 64, 1), ('l2i_conv2d_wino4_f32', 'winograd4_f32'), (ALLF | {'sq'}) - {'in_mask'}, lambda f: F2,
          {'WINO4': 'tall'}),
    # bf16x3: vector branch of l2i_epilogue.h (fuses sq), scalar branch (OW = 33), and the smallest 1x1 _bf16x3_eligible takes (cin * cout >= 65536;
    # masked 1x1 launches stay on the fp32 kernels: the DMA GEMM, or the generic kernel where CoutP % 64 != 0)
    Route('bf16x3_3x3_vec', 'fwd', (16, 40, 3, 1, 1, 36, 36, 1), ('l2i_conv2d_bf16x3_f32', 'implicit_gemm_bf16x3'), ALLF | {'sq'}, switches={'PRECISION': 'bf16x3'}),
    Route('bf16x3_3x3_s2_scalar', 'fwd', (16, 40, 3, 2, 0, 9, 68, 1), ('l2i_conv2d_bf16x3_f32', 'implicit_gemm_bf16x3'), ALLF, switches={'PRECISION': 'bf16x3'}),
    Route('bf16x3_1x1', 'fwd', (256, 256, 1, 1, 0, 8, 32, 1), ('l2i_conv2d_bf16x3_f32', 'implicit_gemm_bf16x3'), (ALLF | {'sq'}) - {'in_mask', 'relu_in'},
          lambda f: ('l2i_conv2d_f32', 'gemm1x1_f32'), {'PRECISION': 'bf16x3'}),
    Route('bf16x3_1x1_ragged_cout', 'fwd', (256, 272, 1, 1, 0, 8, 32, 1), ('l2i_conv2d_bf16x3_f32', 'implicit_gemm_bf16x3'), (ALLF | {'sq'}) - {'in_mask', 'relu_in'},
          _generic, {'PRECISION': 'bf16x3'}),
    # <= 3 input channels: bias / activation / gain / sq only, everything else is the generic kernel's
    Route('cin3', 'fwd', (3, 64, 3, 1, 1, 20, 36, 1), ('l2i_conv2d_f32', 'cin3_f32'), frozenset({'bias', 'lrelu', 'relu', 'out_gain', 'sq'}), _generic),
    Route('cin3_ragged_cout', 'fwd', (3, 40, 3, 1, 1, 20, 36, 1), ('l2i_conv2d_f32', 'cin3_f32'), frozenset({'bias', 'lrelu', 'relu', 'out_gain', 'sq'}), _generic),
    # <= 4 output channels: the register-streaming kernel (>= 192 columns, 16-byte rows, NO style scale: launch_direct_small sends in_scale to the
    # LDS-tile kernel, same family) and the LDS-tile kernel
    Route('direct_small_stream', 'fwd', (24, 3, 3, 1, 1, 18, 260, 2), ('l2i_conv2d_f32', 'direct_small_valu'),
          frozenset({'in_mask', 'relu_in', 'out_gain', 'accumulate'}), lambda f: ('l2i_conv2d_f32', 'direct_small_valu') if set(f) == {'in_scale'} else GENERIC,
          proof='conv3x3_small_stream'),
    Route('direct_small_tile', 'fwd', (24, 3, 3, 1, 1, 9, 12, 1), ('l2i_conv2d_f32', 'direct_small_valu'),
          frozenset({'in_scale', 'in_mask', 'relu_in', 'out_gain', 'accumulate'}), _generic),
    # one-launch transposed convs: other fields go out as per-parity launches of l2i_conv2d_f32
    Route('fused_transposed_p0', 'tfwd', (24, 40, 3, 2, 0, 17, 17, 2), ('l2i_conv_transpose2d_f32', 'transposed_f32'),
          frozenset({'in_scale', 'in_mask', 'relu_in', 'out_scale', 'out_gain'}), _generic),
    Route('fused_transposed_p1_dgrad', 'dgrad', (24, 40, 3, 2, 1, 17, 15, 2), ('l2i_conv_transpose2d_f32', 'transposed_f32'),
          frozenset({'in_scale', 'in_mask', 'relu_in', 'out_scale', 'out_gain'}), _generic),
    # the same launch on the split-precision path (W >= 32, Cin % 16 == 0); other fields: per-parity launches, which stay on the fp32 generic kernel
    Route('bf16x3_transposed_p0', 'tfwd', (16, 40, 3, 2, 0, 8, 32, 1), ('l2i_conv_transpose2d_bf16x3_f32', 'transposed_bf16x3'),
          frozenset({'in_scale', 'in_mask', 'relu_in', 'out_scale', 'out_gain'}), _generic, {'PRECISION': 'bf16x3'}),
    Route('transposed_7x7_small', 'dgrad', (64, 3, 7, 2, 3, 32, 32, 1), ('l2i_conv_transpose2d_f32', 'direct_small_valu'),
          frozenset({'in_mask', 'relu_in', 'out_gain'}), _small7_moved),
]
BY_NAME = {r.name: r for r in ROUTES}
DGRAD_OUT = {'fused_transposed_p1_dgrad': (34, 30), 'transposed_7x7_small': (64, 64)}          # size of the gradient's target map
CASE_NAMES = list(er.CASES) + ['everything']


def _pairs():
    for r in ROUTES:
        for c in CASE_NAMES:
            if r.misalign == 'residual' and 'residual' not in er.case_fields(c, r.accepts):
                continue                                   # (a route about the residual pointer: only cases that have one)
            yield pytest.param(r, c, id='%s-%s' % (r.name, c))


@contextmanager
def switched(**kw):
    """Module switches of latent2im_amd.conv set for the launches inside, conv.PROFILE collecting them; everything restored on the way out."""
    saved = {k: getattr(conv, k) for k in SWITCHES}
    launched = []
    try:
        for k, v in kw.items():
            assert k in SWITCHES, k
            setattr(conv, k, v)
        conv.PROFILE = launched
        yield launched
    finally:
        conv.PROFILE = None
        for k, v in saved.items():
            setattr(conv, k, v)


def guarded(t, misalign=False):
    """``t`` copied into the middle of a sentinel-filled buffer: (buffer, view shaped like t, offset).  16-byte aligned unless ``misalign``."""
    lo = SLACK + (1 if misalign else 0)
    buf = torch.full((lo + t.numel() + SLACK + 3,), er.SENTINEL, device=DEV)
    view = buf[lo:lo + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) != misalign
    return buf, view, lo


def slack_untouched(buf, lo, n):
    return bool((buf[:lo] == er.SENTINEL).all()) and bool((buf[lo + n:] == er.SENTINEL).all())


def to_gpu(x, kw, misalign_residual=False):
    xg = x.to(DEV)
    out = {}
    for k, v in kw.items():
        if torch.is_tensor(v):
            out[k] = xg if v is x else v.to(DEV)
    if misalign_residual:
        out['residual'] = guarded(kw['residual'], True)[1]
    return xg, dict(kw, **out)


def weights(route, seed):
    cin, cout, k = route.shape[:3]
    rs = np.random.RandomState(77 + seed)
    return torch.from_numpy((rs.randn(cout, cin, k, k) / np.sqrt(cin * k * k)).astype(np.float32))


def problem(route, case):
    """(FrozenConv2d, call, model arguments, x, kw, y_prev, sq_ref) of a (route, case) pair."""
    cin, cout, k, stride, pad, h, w, b = route.shape
    seed = ROUTES.index(route) * 100 + CASE_NAMES.index(case)
    fields = er.case_fields(case, route.accepts)
    wt = weights(route, seed)                              # [cout, cin, k, k]: output channels of the LAUNCH first
    if route.kind == 'dgrad':                              # a stride-2 conv cout -> cin whose input gradient is the launch cin -> cout
        fc = conv.FrozenConv2d(wt.transpose(0, 1).contiguous(), 2, pad, device=DEV)
        out_hw = DGRAD_OUT[route.name]
        call = lambda xg, y, **kw: fc.dgrad(xg, out_hw, out=y, **kw)
        model = dict(stride=2, pad=pad, transposed=True)
    elif route.kind in ('tfwd', 'parity'):
        fc = conv.FrozenConv2d(wt, 2, pad, transposed=True, device=DEV)
        out_hw = fc.out_hw(h, w)
        call = lambda xg, y, **kw: fc.forward(xg, out=y, **kw)
        model = dict(stride=2, pad=pad, transposed=True)
    else:
        fc = conv.FrozenConv2d(wt, stride, pad, device=DEV)
        out_hw = fc.out_hw(h, w)
        call = lambda xg, y, **kw: fc.forward(xg, out=y, **kw)
        model = dict(stride=stride, pad=pad)
    x, kw, y_prev, sq_ref = er.make_inputs(seed, fields, (b, cin, h, w), cout, (b, cout) + tuple(out_hw))
    return fc, wt, call, model, fields, x, kw, y_prev, sq_ref


def _kernel_takes(route, fields, y_shape):
    """The library's own conditions (csrc) for the kernel a ``proof`` route names, on this shape and these fields."""
    cin, cout, k, stride, pad, h, w, b = route.shape
    coutp, (oh, ow) = (cout + 31) // 32 * 32, y_shape[2:]
    masked = 'in_mask' in fields or 'relu_in' in fields
    probe = _lib.ConvParams()
    conv._split_k(probe, b * oh * ow, cin, torch.empty(y_shape, device=DEV))
    if route.proof == 'split_k':                       # conv.run_launch hands the generic kernel a workspace and ksplit > 1
        return probe.ksplit > 1 and cin % probe.ksplit == 0 and (cin // probe.ksplit) % 2 == 0
    if route.proof == 'conv3x3s2_dma':                 # l2i_conv3x3s2_eligible (l2i_conv_s2.hip): CK = 2, BM = 64
        return (k == 3 and stride == 2 and not masked and probe.ksplit <= 1 and (pad == 0 or (pad == 1 and w % 4 == 0)) and cin % 2 == 0 and cin >= 8
                and (coutp % 64 == 0 or coutp >= 160) and ow >= 32 and 'sq' not in fields and (cin <= 1024 or 'in_scale' not in fields))
    if route.proof == 'conv3x3_small_stream':          # launch_direct_small (l2i_conv.hip); the guarded tensors of a route without `misalign` are 16-byte aligned
        return (k == 3 and stride == 1 and pad == 1 and cout <= 3 and 'in_scale' not in fields and (oh, ow) == (h, w) and ow >= 192 and w % 4 == 0
                and route.misalign is None)
    raise KeyError(route.proof)


@pytest.mark.parametrize('route,case', list(_pairs()))
def test_epilogue_matches_the_contract(route, case):
    fc, wt, call, model, fields, x, kw, y_prev, sq_ref = problem(route, case)
    expect = route.ran if er.runs_on(fields, route.accepts) else route.moved(fields)
    if route.proof and expect == route.ran and er.runs_on(fields, route.accepts):
        assert _kernel_takes(route, fields, y_prev.shape), (route.proof, fields)
    xg, gkw = to_gpu(x, kw, route.misalign == 'residual')
    buf, y, lo = guarded(y_prev, route.misalign == 'out')
    sq = None
    if sq_ref is not None:
        sq = (sq_ref.to(DEV), torch.zeros(_lib.SQ_SLOTS, device=DEV), [False])
        gkw['sq'] = sq
    if route.hint:
        gkw['tile_hint'] = route.hint
    with switched(**route.switches) as launched:
        if route.kind == 'parity':
            ref = run_parities(fc, wt, route, x, xg, kw, gkw, y, y_prev)
        else:
            call(xg, y, **gkw)
            ref = er.conv_epi_ref(x, wt, y_prev=y_prev, **model, **kw)
    torch.cuda.synchronize()
    ran = sorted(set((q[4], q[5]) for q in launched))
    assert ran == [expect], (ran, expect)
    assert slack_untouched(buf, lo, y.numel()), 'the launch wrote outside y'
    err = er.rel_err(y, ref)
    print('%s %s: %s err %.3g (bound %g)' % (route.name, case, expect[1], err, BOUND[expect[1]]))
    assert err < BOUND[expect[1]], (route.name, case, err)
    if sq is not None:
        assert sq[2][0], 'sq_ref was not fused'
        want = float(((y.double().cpu() - sq_ref.double()) ** 2).sum())
        got = float(sq[1].double().sum())
        print('   sq %.9g want %.9g' % (got, want))
        assert abs(got - want) <= 1e-5 * want


def run_parities(fc, wt, route, x, xg, kw, gkw, y, y_prev):
    """The four per-parity launches one by one: each must equal the model of ITS window (step 2, its offset, its sub-kernel and padding) and
    leave the other three parities bit-identical.  Returns the model after all four."""
    pad, K = route.shape[4], route.shape[2]
    ref = y_prev.double()
    assert len([L for L in fc.fwd if L is not None]) == 4
    for L in fc.fwd:
        ty, pad_y = conv._phase_axis(K, pad, L.off_y)
        tx, pad_x = conv._phase_axis(K, pad, L.off_x)
        assert (pad_y, pad_x, L.step) == (L.pad_y, L.pad_x, 2)
        sub = wt[:, :, ty, :][:, :, :, tx].contiguous()
        before = y.clone()
        conv.run_launch(L, xg, y, **gkw)
        win = er.window(y.shape, 2, (L.off_y, L.off_x)).to(DEV)
        assert torch.equal(y[:, :, ~win].view(torch.int32), before[:, :, ~win].view(torch.int32)), 'parity (%d, %d) wrote outside its window' % (L.off_y, L.off_x)
        ref = er.conv_epi_ref(x, sub, 1, (pad_y, pad_x), step=2, off=(L.off_y, L.off_x), y_prev=ref, **kw)
        w64 = win.cpu()
        e = float((y.double().cpu()[:, :, w64] - ref[:, :, w64]).abs().max() / ref[:, :, w64].abs().max())
        assert e < 5e-6, (L.off_y, L.off_x, e)
    return ref


# ---- l2i_conv1x1_pair_f32 ------------------------------------------------------------------------------------------------------------------------
def _pair_problem(cin=64, mid=256, cout=64, h=16, w=16, b=2, seed=3):
    rs = np.random.RandomState(seed)
    T = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    w1, w2 = T(mid, cin, 1, 1) / np.sqrt(cin), T(cout, mid, 1, 1) / np.sqrt(mid)
    x, b1, b2, res = T(b, cin, h, w), T(mid), T(cout), T(b, mid, h, w) - 1.0          # (the residual drives about half the sums negative)
    return w1, w2, x, b1, b2, res


def test_conv1x1_pair_f32_against_the_model():
    """64 -> 256 -> 64 on 16x16, batch 2, through launch_pair_f32: first conv bias + residual + ReLU (its wide map is written), second conv bias +
    ReLU; both outputs against the float64 model, to fp32 rounding (5e-6: l2i.h says 'equal to fp32 rounding, not bit for bit').  The entry is
    built for Cout % 32 == 0 only, so this is the one route without a ragged channel count."""
    w1, w2, x, b1, b2, res = _pair_problem()
    f1, f2 = conv.FrozenConv2d(w1, 1, 0, device=DEV), conv.FrozenConv2d(w2, 1, 0, device=DEV)
    g = lambda t: t.to(DEV)
    buf1, y1, lo1 = guarded(torch.full((2, 256, 16, 16), er.SENTINEL))
    buf2, y2, lo2 = guarded(torch.full((2, 64, 16, 16), er.SENTINEL))
    d = []
    xg, b1g, b2g, rg = g(x), g(b1), g(b2), g(res)
    with switched() as launched:
        conv.run_launch(f1.fwd[0], xg, y1, bias=b1g, residual=rg, act=conv.ACT_RELU, _defer=d)
        conv.run_launch(f2.fwd[0], y1, y2, bias=b2g, act=conv.ACT_RELU, _defer=d)
        assert conv.pair_f32_shapes_ok(64, 256, 64, 256) and not launched
        conv.launch_pair_f32(d)
    torch.cuda.synchronize()
    assert [(q[4], q[5]) for q in launched] == [('l2i_conv1x1_pair_f32', 'gemm1x1_f32')]
    ref1 = er.conv_epi_ref(x, w1, 1, 0, bias=b1, residual=res, act=er.ACT_RELU)
    ref2 = er.conv_epi_ref(ref1, w2, 1, 0, bias=b2, act=er.ACT_RELU)
    e1, e2 = er.rel_err(y1, ref1), er.rel_err(y2, ref2)
    print('pair_f32: err first %.3g second %.3g' % (e1, e2))
    assert e1 < 5e-6 and e2 < 5e-6
    assert float((ref1 == 0).double().mean()) > 0.2 and float((ref2 == 0).double().mean()) > 0.2          # both ReLUs do clip
    assert slack_untouched(buf1, lo1, y1.numel()) and slack_untouched(buf2, lo2, y2.numel())


# ---- applied or refused, never ignored: the entries with narrow contracts, driven with hand-filled structs -------------------------------------
def _refused(name, *structs, bufs):
    """The entry returns L2I_E_UNSUPPORTED / L2I_E_ARG (raised by _lib.call) and writes nothing."""
    before = [b.clone() for b in bufs]
    with pytest.raises(_lib.L2IError, match=r'failed \((-1|-3)\)'):
        _lib.call(name, *structs)
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b.view(torch.int32), b0.view(torch.int32)), '%s refused the launch but wrote to y' % name


def _operands(b, cin, h, w, cout, oh, ow, seed=11):
    rs = np.random.RandomState(seed)
    T = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(DEV)
    one = T(b, cout, oh, ow)
    return dict(noise=(T(b, 1, oh, ow), 0.3), bias=T(cout), residual=one, res_mask=one, out_mask=one, res_sub=one, in_scale=T(b, cin).abs() + 0.5,
                out_scale=T(b, cout).abs() + 0.5, in_mask=T(b, cin, h, w), sq=(one, torch.zeros(_lib.SQ_SLOTS, device=DEV), [False]))


FUSED_T_REFUSES = ('noise', 'bias', 'residual', 'res_mask', 'out_mask', 'res_sub', 'lrelu', 'relu', 'accumulate', 'sq')


@pytest.mark.parametrize('field', FUSED_T_REFUSES)
@pytest.mark.parametrize('entry', ['l2i_conv_transpose2d_f32', 'l2i_conv_transpose2d_bf16x3_f32'])
def test_fused_transposed_entries_refuse_what_they_do_not_fuse(entry, field):
    """l2i_conv_transpose2d_f32 and its split-precision twin fuse in_scale / in_mask / out_scale / out_gain: 'everything else must be unset' (l2i.h)."""
    route = BY_NAME['fused_transposed_p0' if entry == 'l2i_conv_transpose2d_f32' else 'bf16x3_transposed_p0']
    cin, cout, _, _, _, h, w, b = route.shape
    oh, ow = 2 * h + 1, 2 * w + 1
    F = conv.FusedTransposed(weights(route, 0), 0).to(DEV)
    planes = F.bf16x3_planes() if entry.endswith('bf16x3_f32') else None
    x = torch.randn(b, cin, h, w, device=DEV)
    buf, y, lo = guarded(torch.full((b, cout, oh, ow), er.SENTINEL))
    ops = _operands(b, cin, h, w, cout, oh, ow)

    def struct(**kw):
        p = conv._conv_params(x, F.w, y, b, cin, h, w, cout, 3, 3, 2, 0, 0, h + 1, w + 1, oh, ow, 2, **kw)
        if planes is not None:
            p.w_hi, p.w_lo = _lib.ptr(planes[0]), _lib.ptr(planes[1])
        return p
    _lib.call(entry, struct(out_gain=0.5))                # the struct itself is good
    torch.cuda.synchronize()
    assert slack_untouched(buf, lo, y.numel()) and not bool((y == er.SENTINEL).any())
    kw = {'lrelu': dict(act=conv.ACT_LRELU, slope=0.2, gain=2 ** 0.5), 'relu': dict(act=conv.ACT_RELU), 'accumulate': dict(accumulate=True),
          'noise': dict(noise=ops['noise'][0], noise_w=0.3), 'res_sub': dict(residual=ops['residual'], res_sub=ops['res_sub']),
          'res_mask': dict(res_mask=ops['res_mask'])}.get(field) or {field: ops[field]}
    p = struct(**kw)
    if field == 'res_sub':
        p.residual = None                                 # res_sub alone (with its residual the residual is what gets refused)
    _refused(entry, p, bufs=[buf])


def test_wino4_entry_refuses_a_general_input_mask():
    """l2i_conv2d_wino4_f32 takes unmasked launches and ReLU-on-load (in_mask == x, slopes (1, 0)) only."""
    cin, cout, h, w = 16, 40, 18, 72
    L = conv.FrozenConv2d(weights(BY_NAME['wino4_all'], 0), 1, 1, device=DEV).fwd[0]
    pk = L.wino4_pack()
    x, m = torch.randn(1, cin, h, w, device=DEV), torch.randn(1, cin, h, w, device=DEV)
    buf, y, lo = guarded(torch.full((1, cout, h, w), er.SENTINEL))

    def struct(**kw):
        p = conv._conv_params(x, L.w, y, 1, cin, h, w, cout, 3, 3, 1, 1, 1, h, w, h, w, **kw)
        p.w, p.CoutP = _lib.fptr(pk), pk.shape[1] * 16
        return p
    for tile in (0, 1, 2):
        for kw in (dict(in_mask=m, mask=(1.0, 0.0)), dict(in_mask=m, mask=(2 ** 0.5, 0.2 * 2 ** 0.5)), dict(in_mask=x, mask=(1.0, 0.2))):
            p = struct(**kw)
            p.tile_hint = tile
            _refused('l2i_conv2d_wino4_f32', p, bufs=[buf])
    _lib.call('l2i_conv2d_wino4_f32', struct(in_mask=x, mask=(1.0, 0.0)))
    torch.cuda.synchronize()
    assert slack_untouched(buf, lo, y.numel()) and not bool((y == er.SENTINEL).any())


def test_generic_and_winograd_entries_refuse_sq_or_res_sub_they_cannot_apply():
    """sq_ref / sq_out on a launch of l2i_conv2d_f32 that is not the <= 3-channel kernel's, and res_sub without a residual on every entry that
    takes res_sub: refused, not dropped."""
    cin, cout, h, w = 16, 40, 36, 36
    L = conv.FrozenConv2d(weights(BY_NAME['wino2'], 0), 1, 1, device=DEV).fwd[0]
    x = torch.randn(1, cin, h, w, device=DEV)
    buf, y, lo = guarded(torch.full((1, cout, h, w), er.SENTINEL))
    ops = _operands(1, cin, h, w, cout, h, w)
    struct = lambda **kw: conv._conv_params(x, L.w, y, 1, cin, h, w, cout, 3, 3, 1, 1, 1, h, w, h, w, **kw)
    _refused('l2i_conv2d_f32', struct(sq=ops['sq']), bufs=[buf])
    packs = {'l2i_conv2d_f32': (L.w, L.w.shape[-1]), 'l2i_conv2d_wino_f32': (L.wino_pack(), L.w.shape[-1]),
             'l2i_conv2d_wino4_f32': (L.wino4_pack(), L.wino4_pack().shape[1] * 16)}
    for name, (pk, coutp) in packs.items():
        p = struct(residual=ops['residual'], res_sub=ops['res_sub'])
        p.w, p.CoutP, p.residual = _lib.fptr(pk), coutp, None
        _refused(name, p, bufs=[buf])


PAIR_REFUSES = ('in_scale', 'in_mask', 'out_scale', 'noise', 'out_mask', 'res_mask', 'res_sub', 'lrelu', 'out_gain', 'accumulate', 'sq', 'second_residual',
                'no_first_residual', 'shape_96_96', 'pixels_not_256')


@pytest.mark.parametrize('what', PAIR_REFUSES)
def test_pair_f32_entry_refuses_fields_and_shapes_outside_its_contract(what):
    """l2i_conv1x1_pair_f32 fuses bias / residual (first conv) / ReLU on (Cin1, Cout2) in {(64, 64), (64, 128), (128, 128)} with H * W % 256 == 0."""
    cin, mid, cout, h, w, b = (96, 64, 96, 16, 16, 2) if what == 'shape_96_96' else (64, 256, 64, 16, 12 if what == 'pixels_not_256' else 16, 2)
    w1, w2, x, b1, b2, res = _pair_problem(cin, mid, cout, h, w, b)
    L1, L2 = conv.FrozenConv2d(w1, 1, 0, device=DEV).fwd[0], conv.FrozenConv2d(w2, 1, 0, device=DEV).fwd[0]
    buf1, y1, _ = guarded(torch.full((b, mid, h, w), er.SENTINEL))
    buf2, y2, _ = guarded(torch.full((b, cout, h, w), er.SENTINEL))
    xg, resg = x.to(DEV), res.to(DEV)
    ops = _operands(b, cin, h, w, mid, h, w)
    kw1 = dict(bias=b1.to(DEV), residual=resg, act=conv.ACT_RELU)
    kw2 = dict(bias=b2.to(DEV), act=conv.ACT_RELU)
    extra = {'lrelu': dict(act=conv.ACT_LRELU, slope=0.2, gain=2 ** 0.5), 'out_gain': dict(out_gain=0.5), 'accumulate': dict(accumulate=True),
             'noise': dict(noise=ops['noise'][0], noise_w=0.3), 'res_sub': dict(res_sub=ops['res_sub']), 'second_residual': {}, 'no_first_residual': {},
             'shape_96_96': {}, 'pixels_not_256': {}}.get(what)
    kw1.update({what: ops[what]} if extra is None else extra)
    if what == 'no_first_residual':
        del kw1['residual']
    if what == 'second_residual':
        kw2['residual'] = torch.randn(b, cout, h, w, device=DEV)
    p1 = conv._conv_params(xg, L1.w, y1, b, cin, h, w, mid, 1, 1, 1, 0, 0, h, w, h, w, **kw1)
    p2 = conv._conv_params(y1, L2.w, y2, b, mid, h, w, cout, 1, 1, 1, 0, 0, h, w, h, w, **kw2)
    _refused('l2i_conv1x1_pair_f32', p1, p2, bufs=[buf1, buf2])


def test_sq_is_left_to_the_caller_where_the_kernel_does_not_fuse_it():
    """run_launch sets the fused flag only where the chosen kernel sums (y - sq_ref)^2; elsewhere the flag stays clear, the launch carries no sq
    fields (the entry would refuse them) and the caller runs the sqdiff pass."""
    for route in (BY_NAME[n] for n in ('generic_vec_hint0', 's2_dma_p1', 'gemm1x1', 'bf16x3_3x3_s2_scalar')):
        fc, wt, call, model, fields, x, kw, y_prev, _ = problem(route, 'bias')
        xg, gkw = to_gpu(x, kw)
        buf, y, lo = guarded(y_prev)
        sq = (torch.randn(y.shape, device=DEV), torch.zeros(_lib.SQ_SLOTS, device=DEV), [False])
        with switched(**route.switches) as launched:
            call(xg, y, sq=sq, **gkw)
        torch.cuda.synchronize()
        assert not sq[2][0] and float(sq[1].abs().max()) == 0.0, route.name
        assert sorted(set((q[4], q[5]) for q in launched)) == [route.ran], route.name
        assert er.rel_err(y, er.conv_epi_ref(x, wt, y_prev=y_prev, **model, **kw)) < BOUND[route.ran[1]]
