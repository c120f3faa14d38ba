"""The epilogue classes of conv_wino4s_kernel (csrc/l2i_wino4.hip): a lean class is compiled for one exact operand set of the training step, every
other set takes the generic body.  Whatever class the dispatcher picks, the position-split kernel (tile_hint 0, and 2 = the eight-wave tile) must
stay BIT-IDENTICAL to the round-4 kernel (tile_hint 1), which has one generic epilogue and is not specialised: same inputs, torch.equal on y.
pool_out / pool_idx have no twin in the round-4 kernel: they are checked against torch.max_pool2d of the bit-identical y.  sq_out sums the same
(y - ref)^2 terms in another block order than the round-4 kernel (16- against 32-channel blocks), so it is held to the float64 sum of the
bit-identical y with the contract test's bound (1e-5 relative: ~1e5 non-negative fp32 terms summed in blocks).
Shapes: Cin 16, Cout 40 (ragged against the 32-channel block), batch 2; 18 x 72 (partial tile row, partial second tile column), 18 x 40 (under 64
wide: the 32 x 16 tile) and 16 x 64 (the tall tile takes it with tile_hint 2).  Masks hold exact +-0.0; y sits inside a sentinel-filled buffer."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib, conv
from tests import epilogue_ref as er

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CIN, COUT, B = 16, 40, 2
SHAPES = [(18, 72), (18, 40), (16, 64)]
GENERIC = _lib.WINO4S_LEAN_CLASSES
G_SET = ('in_scale', 'out_scale', 'noise', 'bias', 'lrelu')
# case -> (fields of tests/epilogue_ref.make_inputs, pool, sq, the class l2i_wino4s_epilogue_class must report for tile_hint 0).  Per lean class: its exact
# set, then the set plus one operand (generic).  The sets are the ones the c3 step launches (profiles/wino4s_epilogue_classes_ab.txt).
CASES = {
    'styled': (G_SET, False, False, 0), 'styled+out_gain': (G_SET + ('out_gain',), False, False, GENERIC),
    'vgg': (('relu_in', 'bias'), False, False, 1), 'vgg+relu': (('relu_in', 'bias', 'relu'), False, False, GENERIC),
    'vgg_pool': (('relu_in', 'bias'), True, False, 2), 'vgg_pool+out_gain': (('relu_in', 'bias', 'out_gain'), True, False, GENERIC),
    'vgg_sq': (('relu_in', 'bias'), False, True, 3), 'vgg_sq+noise': (('relu_in', 'bias', 'noise'), False, True, GENERIC),
    'vgg_pool_sq': (('relu_in', 'bias'), True, True, 4), 'vgg_pool_sq+lrelu': (('relu_in', 'bias', 'lrelu'), True, True, GENERIC),
    'dgrad': (('out_mask',), False, False, 5), 'dgrad+accumulate': (('out_mask', 'accumulate'), False, False, GENERIC),
    'dgrad_tap': (('out_mask', 'residual', 'res_sub'), False, False, 6), 'dgrad_tap+res_mask': (('out_mask', 'residual', 'res_sub', 'res_mask'), False, False, GENERIC),
    'resnet': (('bias', 'relu'), False, False, 7), 'resnet+residual': (('bias', 'relu', 'residual'), False, False, GENERIC),
    # sets outside the table
    'bare': ((), False, False, GENERIC), 'in_scale': (('in_scale',), False, False, GENERIC), 'bias_lrelu': (('bias', 'lrelu'), False, False, GENERIC),
    'everything': (('in_scale', 'out_scale', 'out_mask', 'noise', 'bias', 'residual', 'res_mask', 'res_sub', 'lrelu', 'out_gain', 'accumulate'), True, True, GENERIC),
}
_PACK = {}


def _layer():
    if 'L' not in _PACK:
        rs = np.random.RandomState(5)
        wt = torch.from_numpy((rs.randn(COUT, CIN, 3, 3) / np.sqrt(CIN * 9)).astype(np.float32))
        L = conv.FrozenConv2d(wt, 1, 1, device=DEV).fwd[0]
        _PACK['L'], _PACK['pk'] = L, L.wino4_pack()
    return _PACK['L'], _PACK['pk']


def _guarded(t):
    lo = 64
    buf = torch.full((lo + t.numel() + 64,), er.SENTINEL, device=DEV)
    view = buf[lo:lo + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view, lo


def _run(case, hw, tile_hint):
    """One launch of l2i_conv2d_wino4_f32 on the case's operands: (y, guard intact, pooled, pool index, sq_out, sq_ref, class reported)."""
    fields, pool, sq, _ = CASES[case]
    h, w = hw
    L, pk = _layer()
    x, kw, y_prev, _ = er.make_inputs(1000 + sorted(CASES).index(case), fields, (B, CIN, h, w), COUT, (B, COUT, h, w))
    xg = x.to(DEV)
    gkw = {k: (xg if v is x else v.to(DEV)) if torch.is_tensor(v) else v for k, v in kw.items()}
    buf, y, lo = _guarded(y_prev)
    sq_ref = torch.from_numpy(np.random.RandomState(7).randn(B, COUT, h, w).astype(np.float32)).to(DEV) if sq else None
    sq_t = (sq_ref, torch.zeros(_lib.SQ_SLOTS, device=DEV), [False]) if sq else None
    p = conv._conv_params(xg, L.w, y, B, CIN, h, w, COUT, 3, 3, 1, 1, 1, h, w, h, w, sq=sq_t, **gkw)
    p.w, p.CoutP, p.tile_hint = _lib.fptr(pk), pk.shape[1] * 16, tile_hint
    pooled = idx = None
    if pool and tile_hint != 1:                            # (the round-4 kernel refuses pool_out)
        pooled = torch.full((B, COUT, h // 2, w // 2), er.SENTINEL, device=DEV)
        idx = torch.full((B, COUT, h // 2, w // 2), 255, dtype=torch.uint8, device=DEV)
        p.pool_out, p.pool_idx = _lib.fptr(pooled), _lib.ptr(idx)
    cls = _lib.load().l2i_wino4s_epilogue_class(p)
    _lib.call('l2i_conv2d_wino4_f32', p)
    torch.cuda.synchronize()
    intact = bool((buf[:lo] == er.SENTINEL).all()) and bool((buf[lo + y.numel():] == er.SENTINEL).all())
    return y, intact, pooled, idx, (sq_t[1] if sq else None), sq_ref, cls


@pytest.mark.parametrize('hw', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('case', list(CASES))
def test_position_split_classes_equal_the_round4_kernel(case, hw):
    fields, pool, sq, want_cls = CASES[case]
    y1, ok1, _, _, sq1, sq_ref, _ = _run(case, hw, 1)
    assert ok1
    for hint in (0, 2):
        y, ok, pooled, idx, sq_out, _, cls = _run(case, hw, hint)
        tall = hint == 2 and hw[1] >= 64 and hw[0] >= 16
        assert cls == (GENERIC if tall else want_cls), (case, hint, cls)
        assert ok, 'tile_hint %d wrote outside y' % hint
        assert torch.equal(y.view(torch.int32), y1.view(torch.int32)), (case, hw, hint, float((y - y1).abs().max()))
        if pool:
            want, arg = torch.nn.functional.max_pool2d(y, 2, return_indices=True)
            assert torch.equal(pooled, want)
            py, px = torch.meshgrid(torch.arange(hw[0] // 2, device=DEV), torch.arange(hw[1] // 2, device=DEV), indexing='ij')
            flat = (2 * py + (idx.long() >> 1)) * hw[1] + 2 * px + (idx.long() & 1)
            assert torch.equal(torch.gather(y.flatten(2), 2, flat.flatten(2)).view_as(pooled), pooled)
        if sq:
            want = float(((y.double() - sq_ref.double()) ** 2).sum())
            for name, got in (('tile_hint %d' % hint, float(sq_out.double().sum())), ('tile_hint 1', float(sq1.double().sum()))):
                print('%s %s sq %.9g want %.9g' % (case, name, got, want))
                assert abs(got - want) <= 1e-5 * want, (case, name, got, want)


def test_class_query_on_the_steps_operand_sets():
    """The operand sets of the c3 step take a lean class, sets outside the table the generic one; the query launches nothing (NULL tensors)."""
    def cls(tile_hint=0, ow=64, **kw):
        p = _lib.ConvParams()
        p.OH, p.OW, p.out_gain, p.tile_hint = 64, ow, 1.0, tile_hint
        for k, v in kw.items():
            setattr(p, k, v)
        return _lib.load().l2i_wino4s_epilogue_class(p)
    G = dict(in_scale=1, out_scale=1, noise=1, bias=1, act=conv.ACT_LRELU)
    V = dict(in_mask=1, bias=1)
    assert cls(**G) == 0 and cls(**V) == 1 and cls(pool_out=1, **V) == 2 and cls(sq_ref=1, **V) == 3 and cls(pool_out=1, sq_ref=1, **V) == 4
    assert cls(out_mask=1) == 5 and cls(out_mask=1, residual=1, res_sub=1) == 6 and cls(bias=1, act=conv.ACT_RELU) == 7
    assert cls(ow=32, **G) == 0 and cls(tile_hint=2, ow=32, **G) == 0          # under 64 wide there is no tall tile
    for kw in (dict(), dict(in_scale=1), dict(bias=1, act=conv.ACT_LRELU), dict(out_gain=0.5, **G), dict(accumulate=1, out_mask=1), dict(in_scale=1, **V),
               dict(tile_hint=2, **G), dict(res_mask=1, out_mask=1, residual=1, res_sub=1)):
        assert cls(**kw) == GENERIC, kw
    assert _lib.load().l2i_wino4s_epilogue_class(None) == -1
