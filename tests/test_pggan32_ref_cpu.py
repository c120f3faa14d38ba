"""tests/pggan32_ref.py on the CPU: the rows reach every path and cross the grid cap, a float32 evaluation of the kernels' arithmetic in the
kernel's channel order and in the reversed one is inside the derived bounds on every row, each planted mistake leaves them on a named row, the
NaN stays in its column, and upsample and pool are adjoint."""
import numpy as np
import pytest

from tests import pggan32_ref as P

_cases = {}


def _case(row):
    if row.id not in _cases:
        _cases[row.id] = P.make_case(row)
    return _cases[row.id]


ROW = {r.id: r for r in P.ROWS}


def test_rows_reach_both_paths_and_cross_the_cap():
    assert P.CAP == 1048576
    paths = {r.id: P.path(r) for r in P.ROWS}
    assert paths['vec_2x512x16'] == 'vector' and paths['scalar_hw_1x8x15'] == 'scalar' and paths['scalar_hw_1x37x35'] == 'scalar'
    for rid in ('off_y_2x16x64', 'off_x_2x16x64', 'off_both_2x16x64'):
        assert paths[rid] == 'scalar' and ROW[rid].HW % 4 == 0          # the scalar path because of a base pointer alone
    assert paths[P.BIG[0]] == 'vector' and paths[P.BIG[1]] == 'scalar'
    for rid in P.BIG:
        assert P.work_items(ROW[rid]) > P.CAP
    assert all(P.work_items(r) <= P.CAP for r in P.ROWS if r.id not in P.BIG)
    big = {m.id: m for m in P.MAPS}[P.BIG_MAP]
    assert P.map_work_items(big) > P.CAP and all(P.map_work_items(m) <= P.CAP for m in P.MAPS if m.id != P.BIG_MAP)
    assert all(m.W % 2 == 0 for m in P.MAPS) and any((m.W // 2) % 2 == 1 for m in P.MAPS)
    assert sum(r.nan for r in P.ROWS) == 1 and ROW['latent_3x511x1'].slope == 1.0


@pytest.mark.parametrize('row', P.ROWS, ids=lambda r: r.id)
def test_inputs_hold_the_edges(row):
    case = _case(row)
    x, gy = case['x'], case['gy']
    zeros = x == 0
    assert 0.05 < zeros.mean() < 0.6 and (gy[zeros] != 0).all()
    b, p = case['zero']
    assert not x[b, :, p].any() and gy[b, :, p].any()
    b, p = case['small']
    col = np.abs(x[b, :, p])
    assert col.max() < 1e-4 and (col ** 2).mean() < 100 * P.EPS
    y, _ = P.forward(row, case)
    dx, _ = P.backward(row, case)
    zb, zp = case['zero']
    assert not y[zb, :, zp].any()
    fac = np.where(x[zb, :, zp] > 0, 1.0, row.slope)
    assert np.allclose(dx[zb, :, zp], gy[zb, :, zp].astype(np.float64) * fac / np.sqrt(P.EPS), rtol=1e-12)
    if row.nan:
        nb, nc, npx = case['nan']
        want = np.zeros(x.shape, bool)
        want[nb, :, npx] = True
        assert np.array_equal(np.isnan(y), want) and np.array_equal(np.isnan(dx), want)
        assert P.path(row) == 'vector' and npx % 4 != 0      # three other pixels share its float4, one of them before it
    else:
        assert np.isfinite(y).all() and np.isfinite(dx).all()


@pytest.mark.parametrize('order', ['kernel', 'reversed'])
@pytest.mark.parametrize('row', P.ROWS, ids=lambda r: r.id)
def test_float32_arithmetic_is_inside_the_bounds(row, order):
    case = _case(row)
    y, by = P.forward(row, case)
    dx, bd = P.backward(row, case)
    rf, rb = P.ratio(P.fwd_float32(row, case, order), y, by), P.ratio(P.bwd_float32(row, case, order), dx, bd)
    print('pggan32 f32 %s %s fwd ratio %.3f bwd ratio %.3f' % (row.id, order, rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (rf, rb)


# the row on which each planted mistake must leave the bounds
CAUGHT_ON = {'eps_dropped': 'vec_2x512x16', 'mask_from_gy_sign': 'scalar_hw_1x8x15', 'sum_term_dropped': 'off_x_2x16x64',
             'zero_takes_one': 'vec_1x37x36', 'mean_over_padded_c': 'latent_3x511x1'}


@pytest.mark.parametrize('mistake', P.MISTAKES)
def test_planted_mistake_exceeds_the_bounds(mistake):
    row = ROW[CAUGHT_ON[mistake]]
    case = _case(row)
    dx, bd = P.backward(row, case)
    worst = P.ratio(P.backward(row, case, mistake)[0], dx, bd)
    if mistake in P.FWD_MISTAKES:
        y, by = P.forward(row, case)
        assert P.ratio(P.forward(row, case, mistake)[0], y, by) > 1.0, (mistake, row.id)
    print('pggan32 mistake %s on %s: backward ratio %.3g' % (mistake, row.id, worst))
    assert worst > 1.0, (mistake, row.id, worst)


def test_every_mistake_is_in_the_table():
    assert set(CAUGHT_ON) == set(P.MISTAKES) and len(P.MISTAKES) == 5


def test_ratio_counts_a_stray_nan_as_out():
    want = np.array([1.0, np.nan, 2.0])
    bound = np.array([1e-6, 0.0, 1e-6])
    assert P.ratio(np.array([1.0, np.nan, 2.0]), want, bound) == 0.0
    assert P.ratio(np.array([np.nan, np.nan, 2.0]), want, bound) == float('inf')
    assert P.ratio(np.array([1.0, 3.0, 2.0]), want, bound) == float('inf')
    assert P.ratio(np.array([1.0, np.nan, 2.0 + 3e-6]), want, bound) > 2.9


@pytest.mark.parametrize('m', [m for m in P.MAPS if m.id != P.BIG_MAP], ids=lambda m: m.id)
def test_maps_are_exact_and_adjoint(m):
    x, g = P.map_input(m, pool=False), P.map_input(m, pool=True)
    for scale in P.SCALES:
        up, pool = P.up_float32(x, scale), P.pool_float32(g, scale)
        assert up.dtype == np.float32 and pool.dtype == np.float32
        assert up.shape == g.shape and pool.shape == x.shape
        assert np.array_equal(up[:, 1::2, 0::2], up[:, 0::2, 1::2]) and np.array_equal(up[:, 0::2, 0::2], x * np.float32(scale))
        lhs, rhs = (up.astype(np.float64) * g).sum(), (x.astype(np.float64) * pool).sum()
        assert abs(lhs - rhs) <= 8 * P.U * np.abs(up.astype(np.float64) * g).sum()
    s = np.float32(0.3)                                     # the window sum keeps its order: (a + b) + (c + d), one product after it
    w = np.array([[[1.0, 2.0 ** -24], [2.0 ** -24, -1.0]]], dtype=np.float32)
    assert P.pool_float32(w, 0.3)[0, 0, 0] == s * ((w[0, 0, 0] + w[0, 0, 1]) + (w[0, 1, 0] + w[0, 1, 1]))
