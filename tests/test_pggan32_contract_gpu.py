"""l2i_pixelnorm_act_f32, l2i_pixelnorm_act_bwd_f32, l2i_upsample2x_nearest_f32 and l2i_pool2x2_f32 (csrc/l2i_pggan.hip) through their raw entry
points against tests/pggan32_ref.py: every row twice on fresh sentinel-guarded outputs, the worst error as a share of its derived bound (bit
equality for the two exact maps), the guards, equal bits of the two launches, and refused calls that write nothing.  Every row prints
`pggan32 <row> <output> err bound ratio`."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from tests import contract_gpu as cg
from tests import pggan32_ref as P
from tests import stream_ref as sr

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -3
_models = {}


def _model(row):
    """Inputs and float64 models of a row, computed once and left unchanged."""
    if row.id not in _models:
        case = P.make_case(row)
        _models[row.id] = (case, P.forward(row, case), P.backward(row, case))
    return _models[row.id]


def _operand(a, off=0):
    """A device copy of ``a`` whose base pointer is ``off`` elements past a 16-byte boundary."""
    buf = cg.keep(torch.empty(a.size + 4, dtype=torch.float32, device=cg.DEV))
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
    assert view.data_ptr() % 16 == 4 * off
    return view


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _held(row, name, got, want, bound):
    same, g, w, b = P.split_nan(got.cpu().numpy(), want, bound)
    err, bnd, ratio = sr.worst(torch.from_numpy(g), torch.from_numpy(w), torch.from_numpy(b))
    print('pggan32 %s %s err %.3e bound %.3e ratio %.3f nan-pattern %s' % (row.id, name, err, bnd, ratio, 'equal' if same else 'DIFFERENT'))
    assert same, 'NaNs of %s are not where the model has them' % name
    assert ratio <= 1.0, (row.id, name, ratio)


@pytest.mark.parametrize('row', P.ROWS, ids=lambda r: r.id)
def test_pixelnorm_rows(row):
    case, (y, by), (dx, bd) = _model(row)
    if row.id in P.BIG:
        assert P.work_items(row) > P.CAP
    oy, ox, og = row.off
    x, gy = _operand(case['x'], ox), _operand(case['gy'], og)
    shape = (row.B, row.C, row.HW)
    runs = []
    for _ in range(2):
        ybuf, yv = cg.guarded(shape, off=oy)
        dbuf, dv = cg.guarded(shape, off=oy)
        assert yv.data_ptr() % 16 == 4 * oy and dv.data_ptr() % 16 == 4 * oy
        _lib.call('l2i_pixelnorm_act_f32', _lib.fptr(yv), _lib.fptr(x), row.B, row.C, row.HW, P.EPS, row.slope)
        _lib.call('l2i_pixelnorm_act_bwd_f32', _lib.fptr(dv), _lib.fptr(gy), _lib.fptr(x), row.B, row.C, row.HW, P.EPS, row.slope)
        torch.cuda.synchronize()
        assert cg.untouched(ybuf, yv) and cg.untouched(dbuf, dv), 'a launch wrote outside its output'
        runs.append((yv, dv))
    _held(row, 'y', runs[0][0], y, by)
    _held(row, 'dx', runs[0][1], dx, bd)
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), 'two launches differ'
    if row.nan:                                              # the NaN column is NaN, the three pixels of its float4 are not
        nb, _, npx = case['nan']
        gy_, gd_ = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
        assert np.isnan(gy_[nb, :, npx]).all() and np.isnan(gd_[nb, :, npx]).all()
        others = [p for p in range(npx // 4 * 4, npx // 4 * 4 + 4) if p != npx]
        assert np.isfinite(gy_[nb][:, others]).all() and np.isfinite(gd_[nb][:, others]).all()
    cg.release()


@pytest.mark.parametrize('m', P.MAPS, ids=lambda m: m.id)
def test_upsample_and_pool_are_exact(m):
    if m.id == P.BIG_MAP:
        assert P.map_work_items(m) > P.CAP
    xu, xp = P.map_input(m, pool=False), P.map_input(m, pool=True)
    du, dp = _operand(xu), _operand(xp)
    for scale in P.SCALES:
        want_u, want_p = torch.from_numpy(P.up_float32(xu, scale)), torch.from_numpy(P.pool_float32(xp, scale))
        runs = []
        for _ in range(2):
            ubuf, uv = cg.guarded((m.planes, 2 * m.H, 2 * m.W))
            pbuf, pv = cg.guarded((m.planes, m.H, m.W))
            _lib.call('l2i_upsample2x_nearest_f32', _lib.fptr(uv), _lib.fptr(du), m.planes, m.H, m.W, scale)
            _lib.call('l2i_pool2x2_f32', _lib.fptr(pv), _lib.fptr(dp), m.planes, m.H, m.W, scale)
            torch.cuda.synchronize()
            assert cg.untouched(ubuf, uv) and cg.untouched(pbuf, pv), 'a launch wrote outside its output'
            runs.append((uv, pv))
        up_ok, pool_ok = cg.same(runs[0][0], want_u), cg.same(runs[0][1], want_p)
        print('pggan32 %s scale %g upsample exact %s pool exact %s' % (m.id, scale, 'equal' if up_ok else 'DIFFERENT', 'equal' if pool_ok else 'DIFFERENT'))
        assert up_ok and pool_ok
        assert torch.equal(_bits(runs[0][0]), _bits(want_u)) and torch.equal(_bits(runs[0][1]), _bits(want_p))          # signed zeros too
        assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), 'two launches differ'
    cg.release()


def test_pixelnorm_refusals():
    """A null pointer or a non-positive size: L2I_E_ARG before any launch, nothing written."""
    b, c, hw = 2, 8, 16
    x = cg.keep(torch.ones(b * c * hw, device=cg.DEV))
    g = cg.keep(torch.ones(b * c * hw, device=cg.DEV))
    obuf, out = cg.guarded((b, c, hw))
    F = _lib.fptr
    fwd = lambda y, xx, bb, cc, hh: cg.refused(E_ARG, 'l2i_pixelnorm_act_f32', y, xx, bb, cc, hh, P.EPS, P.SLOPE, outs=(obuf,))
    bwd = lambda d, gg, xx, bb, cc, hh: cg.refused(E_ARG, 'l2i_pixelnorm_act_bwd_f32', d, gg, xx, bb, cc, hh, P.EPS, P.SLOPE, outs=(obuf,))
    fwd(None, F(x), b, c, hw)
    fwd(F(out), None, b, c, hw)
    bwd(None, F(g), F(x), b, c, hw)
    bwd(F(out), None, F(x), b, c, hw)
    bwd(F(out), F(g), None, b, c, hw)
    for sizes in ((0, c, hw), (-1, c, hw), (b, 0, hw), (b, -8, hw), (b, c, 0), (b, c, -16)):
        fwd(F(out), F(x), *sizes)
        bwd(F(out), F(g), F(x), *sizes)
    assert bool((x == 1).all()) and bool((g == 1).all())
    cg.release()


def test_upsample_and_pool_refusals():
    """An odd width, or y / x off their 16- and 8-byte boundaries: L2I_E_UNSUPPORTED; a null pointer or a non-positive size: L2I_E_ARG."""
    planes, h, w = 2, 4, 6
    big = cg.keep(torch.ones(planes * 4 * h * w + 8, device=cg.DEV))
    obuf, out = cg.guarded((planes * 4 * h * w + 8,))
    F = _lib.fptr
    assert out.data_ptr() % 16 == 0 and big.data_ptr() % 16 == 0
    up = lambda code, y, x, pl, hh, ww: cg.refused(code, 'l2i_upsample2x_nearest_f32', y, x, pl, hh, ww, 1.0, outs=(obuf,))
    pool = lambda code, y, x, pl, hh, ww: cg.refused(code, 'l2i_pool2x2_f32', y, x, pl, hh, ww, 1.0, outs=(obuf,))
    for fn in (up, pool):
        fn(E_UNSUPPORTED, F(out), F(big), planes, h, 5)
        fn(E_UNSUPPORTED, F(out), F(big), planes, h, 1)
        fn(E_ARG, None, F(big), planes, h, w)
        fn(E_ARG, F(out), None, planes, h, w)
        for sizes in ((0, h, w), (planes, 0, w), (planes, h, 0), (planes, -4, w)):
            fn(E_ARG, F(out), F(big), *sizes)
    # upsample: y on 16 bytes, x on 8; pool: x on 16 bytes, y on 8
    for off in (1, 2, 3):
        up(E_UNSUPPORTED, F(out[off:]), F(big), planes, h, w)
        pool(E_UNSUPPORTED, F(out), F(big[off:]), planes, h, w)
    for off in (1, 3):
        up(E_UNSUPPORTED, F(out), F(big[off:]), planes, h, w)
        pool(E_UNSUPPORTED, F(out[off:]), F(big), planes, h, w)
    assert bool((big == 1).all())
    cg.release()
