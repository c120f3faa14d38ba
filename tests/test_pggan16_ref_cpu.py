"""tests/pggan16_ref.py on the CPU: the h8 restatement round-trips, a float32 evaluation of the kernels' arithmetic in three summation orders is
inside the derived bounds, every planted mistake is outside them at the GPU test's own shapes, and the ctypes rows of the two entry points are
the declarations of include/l2i.h."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import pggan16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ('kernel', 'ascending', 'descending')


def _kinds(dt):
    return ('mixed', 'big') if dt == 'f16' else ('mixed',)


def test_h8_round_trip_and_resampling():
    a = np.arange(2 * 16 * 3 * 5, dtype=np.float32).reshape(2, 16, 3, 5)
    p = R.to_h8(a)
    assert p.shape == (2, 2, 3, 5, 8) and p[1, 1, 2, 4, 3] == a[1, 8 + 3, 2, 4]
    assert np.array_equal(R.from_h8(p), a)
    u = R.up2(a)
    assert u.shape == (2, 16, 6, 10) and u[1, 3, 5, 9] == a[1, 3, 2, 4] and u[0, 0, 2, 3] == a[0, 0, 1, 1]
    assert np.array_equal(R.pool2(u), 4 * a)
    g = np.random.RandomState(0).standard_normal(u.shape)
    assert abs((u * g).sum() - (a * R.pool2(g)).sum()) <= 1e-9 * np.abs(u * g).sum()          # pool2 is up2's adjoint


@pytest.mark.parametrize('dt', R.DTYPES)
def test_rounding_is_the_element_type(dt):
    x = np.array([1.0 + R.UH[dt], 1.0 + 3 * R.UH[dt], -0.3, 65000.0], dtype=np.float32)
    y = R.round16(x, dt)
    assert y[0] == 1.0 and y[1] == 1.0 + 4 * R.UH[dt]
    assert np.all(np.abs(y - x) <= R.UH[dt] * np.abs(x)) and np.array_equal(R.round16(y, dt), y)


def test_constants_are_linear_in_c():
    for k in (R.k_f, R.k_b):
        assert abs((k(512) - k(256)) - (k(256) - k(0))) < 1e-12 and k(8) > 0


@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_float32_arithmetic_is_inside_the_bounds(shape, dt):
    for kind in _kinds(dt):
        case = R.make_case(shape, dt, kind)
        y = R.pixelnorm_act(case['x'], dt)
        for order in ORDERS:
            got = R.fwd_float32(case['x'], dt, order=order)
            assert R.share(got, y, R.fwd_bound(y, dt)) < 1.0, (kind, order, R.share(got, y, R.fwd_bound(y, dt)))
        for pool in (1, 2):
            for addend in (None, case['addend']):
                gy = case['gy2'] if pool == 2 else case['gy1']
                ref = R.pixelnorm_act_bwd(gy, case['x'], dt, pool=pool, addend=addend)
                for order in ORDERS:
                    got = R.bwd_float32(gy, case['x'], dt, pool=pool, addend=addend, order=order)
                    s = R.share(got, ref['dx'], R.bwd_bound(ref, dt))
                    assert s < 1.0, (kind, pool, addend is not None, order, s)


def test_all_zero_column():
    """y = 0 and dx = g' / sqrt(eps) there."""
    for dt in R.DTYPES:
        case = R.make_case((2, 32, 3, 5), dt)
        b, h, w = case['zero']
        assert not case['x'][b, :, h, w].any()
        assert not R.pixelnorm_act(case['x'], dt)[b, :, h, w].any()
        ref = R.pixelnorm_act_bwd(case['gy1'], case['x'], dt)
        assert np.allclose(ref['dx'][b, :, h, w], case['gy1'][b, :, h, w].astype(np.float64) * R.SLOPE / np.sqrt(R.EPS), rtol=1e-12)


def _visible(shape, mistake):
    b, ch, h, w = shape
    if mistake == 'mean_over_padded_c':
        return ch % 32 != 0
    if mistake == 'eps_dropped':
        return b * h * w > 1                      # the all-zero column (make_case)
    return True


def _rows(shape, dt, mistake):
    """(model, faulty model, bound) for every output the GPU test checks."""
    rows = []
    for kind in _kinds(dt):
        case = R.make_case(shape, dt, kind)
        if mistake in R.FWD_MISTAKES:
            y = R.pixelnorm_act(case['x'], dt)
            rows.append((y, R.pixelnorm_act(case['x'], dt, mistake=mistake), R.fwd_bound(y, dt)))
        for pool in (1, 2):
            for addend in (None, case['addend']):
                gy = case['gy2'] if pool == 2 else case['gy1']
                ref = R.pixelnorm_act_bwd(gy, case['x'], dt, pool=pool, addend=addend)
                bad = R.pixelnorm_act_bwd(gy, case['x'], dt, pool=pool, addend=addend, mistake=mistake)
                rows.append((ref['dx'], bad['dx'], R.bwd_bound(ref, dt)))
    return rows


CASES = [(s, dt, m) for s in R.SHAPES for dt in R.DTYPES for m in R.MISTAKES if _visible(s, m)]


@pytest.mark.parametrize('shape,dt,mistake', CASES, ids=str)
def test_planted_mistake_exceeds_the_bounds(shape, dt, mistake):
    worst = max(R.share(bad, ref, bound) for ref, bad, bound in _rows(shape, dt, mistake))
    assert worst > 1.0, (mistake, shape, dt, worst)


def test_every_mistake_is_in_the_table():
    assert len(R.MISTAKES) == 6
    for m in R.MISTAKES:
        assert any(c[2] == m for c in CASES), m


def test_entries_are_declared_and_bound():
    from latent2im_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'l2i.h')).read()
    P, F, I = ctypes.c_void_p, ctypes.c_float, ctypes.c_int32
    want = {'l2i_pixelnorm_act_h8': (['y', 'y_low', 'x', 'B', 'C', 'H', 'W', 'eps', 'slope', 'up', 'stream'], [P, P, P, I, I, I, I, F, F, I, P]),
            'l2i_pixelnorm_act_bwd_h8': (['dx', 'gy', 'x', 'addend', 'B', 'C', 'H', 'W', 'eps', 'slope', 'pool', 'stream'], [P, P, P, P, I, I, I, I, F, F, I, P])}
    ctype_of = {'void*': P, 'float': F, 'int': I}
    for base, (names, args) in want.items():
        for name in (base, base + '_f16'):
            m = re.search(r'int %s\(([^)]*)\);' % name, hdr)
            assert m, '%s is not declared in include/l2i.h' % name
            decl = [a.split() for a in m.group(1).split(',')]
            assert [d[-1].lstrip('*') for d in decl] == names
            types = [ctype_of[''.join(t for t in d[:-1] if t != 'const') + ('*' if d[-1].startswith('*') else '')] for d in decl]
            assert name in _lib.EXPORTS and _lib._SIGNATURES[name] == (I, args) and types == args, name
    assert _lib.ABI_VERSION == 12 and '#define L2I_ABI_VERSION 12' in hdr              # additive: the version stays
