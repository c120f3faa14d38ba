"""tests/gram16_ref.py on the CPU: the h8 pack / unpack round trip, a float32 evaluation of the kernels' arithmetic in two summation orders inside
the derived bounds, and the mistake table: every planted fault exceeds 10x the GPU contract's bound at the GPU test's shapes."""
import numpy as np
import pytest

from tests import gram16_ref as R16
from tests import gram_ref as R


@pytest.mark.parametrize('shape', R16.SHAPES, ids=str)
def test_pack_unpack_round_trip(shape):
    b, ch, h, w = shape
    a = np.arange(b * ch * h * w, dtype=np.float32).reshape(b, ch, h * w)
    p = R16.pack_h8(a)
    assert p.shape == (b, ch // 8, h * w, 8)
    assert p[b - 1, 1, 2, 3] == a[b - 1, 8 + 3, 2]                       # channel 8 g + e of pixel p sits at [g][p][e]
    assert np.array_equal(R16.unpack_h8(p), a)
    assert not np.array_equal(p.reshape(a.shape), a)                     # (which is why 'chunk_as_plane' is a mistake)


@pytest.mark.parametrize('dt', R16.DTYPES)
def test_rounding_is_the_element_type(dt):
    x = np.array([1.0 + R16.UH[dt], 1.0 + 3 * R16.UH[dt], -0.3, 65000.0], dtype=np.float32)
    y = R16.round16(x, dt)
    assert y[0] == 1.0 and y[1] == 1.0 + 4 * R16.UH[dt]                  # ties to even, one ulp = 2 u_h
    assert np.all(np.abs(y - x) <= R16.UH[dt] * np.abs(x))
    assert np.array_equal(R16.round16(y, dt), y)


@pytest.mark.parametrize('dt', R16.DTYPES)
@pytest.mark.parametrize('shape', R16.SHAPES, ids=str)
def test_float32_in_two_orders_is_inside_the_bounds(shape, dt):
    b, ch, h, w = shape
    case = R16.make_case(shape, dt)
    # forward: float32 sums of exact products, pixels ascending and descending
    ref = R16.gram_loss(case['c'], case['gt'])
    f = np.maximum(case['c'], np.float32(0))
    for fl in (f, f[:, :, ::-1]):
        G = np.zeros((b, ch, ch), np.float32)
        for p in range(h * w):
            G += fl[:, :, p:p + 1] * fl[:, None, :, p]
        G = G / np.float32(ch * h * w)
        assert (np.abs(G.astype(np.float64) - ref['G']) <= R16.gram_bound(ref, h * w)).all()
    # backward, write and accumulate, both orders
    for g0, sc in ((None, None), (case['g0'], case['scale_b'])):
        bref = R16.gram_bwd(case['c'], case['d'], dt, scale=sc, g0=g0)
        bound = R16.bwd_bound(bref, ch, dt, g0)
        for rev in (False, True):
            got = R16.bwd_float32(case['c'], case['d'], dt, scale=sc, g0=g0, reverse=rev).astype(np.float64)
            assert (np.abs(got - bref['g']) <= bound).all(), (np.abs(got - bref['g']) / bound).max()
    if dt == 'f16':                                                      # the row of 'd_rounded_before_scaling': right code is inside its bound there too
        small = R16.small_d_case(case)
        bref = R16.gram_bwd(small['c'], small['d'], dt, scale=small['scale'])
        got = R16.bwd_float32(small['c'], small['d'], dt, scale=small['scale']).astype(np.float64)
        assert (np.abs(got - bref['g']) <= R16.bwd_bound(bref, ch, dt)).all()


def _visible(shape, mistake):
    b, ch, h, w = shape
    if mistake == 'no_mirror':
        return ch > 32
    if mistake == 'scale_of_sample_0':
        return b > 1
    return True


def _rows(shape, dt, mistake):
    """(model, faulty model, bound) for every output the GPU test checks."""
    b, ch, h, w = shape
    case = R16.make_case(shape, dt)
    rows = []
    fwd, bad = R16.gram_loss(case['c'], case['gt']), R16.gram_loss(case['c'], case['gt'], mistake)
    rows.append((fwd['G'], bad['G'], R16.gram_bound(fwd, h * w)))
    rows.append((fwd['loss'], bad['loss'], R16.loss_bound(fwd, ch, h * w, case['gt'])))
    runs = [(case['d'], None, None), (case['d'], case['scale_b'], case['g0'])]
    if dt == 'f16':
        small = R16.small_d_case(case)
        runs.append((small['d'], small['scale'], None))
    for d, sc, g0 in runs:
        ref = R16.gram_bwd(case['c'], d, dt, scale=sc, g0=g0)
        bad = R16.gram_bwd(case['c'], d, dt, scale=sc, g0=g0, mistake=mistake)
        rows.append((ref['g'], bad['g'], R16.bwd_bound(ref, ch, dt, g0)))
    return rows


CASES = [(s, dt, m) for s in R16.SHAPES for dt in R16.DTYPES for m in R16.MISTAKES
         if _visible(s, m) and (m != 'd_rounded_before_scaling' or dt == 'f16')]


@pytest.mark.parametrize('shape,dt,mistake', CASES, ids=str)
def test_planted_mistake_exceeds_ten_bounds(shape, dt, mistake):
    tiny = np.finfo(np.float64).tiny
    with np.errstate(over='ignore'):             # an entry with a zero bound (masked, bf16) that the fault moves: infinitely far out
        worst = max(float((np.abs(bad - ref) / (bound + tiny)).max()) for ref, bad, bound in _rows(shape, dt, mistake))
    assert worst >= 10.0, (mistake, shape, dt, worst)


def test_every_mistake_is_in_the_table():
    assert set(R.MISTAKES) < set(R16.MISTAKES) and len(R.MISTAKES) == 8
    for m in R16.MISTAKES:
        assert any(c[2] == m for c in CASES), m
