"""l2i_pixelnorm_act_h8 / l2i_pixelnorm_act_bwd_h8 (bf16 and fp16 elements) against the float64 model of tests/pggan16_ref.py at its seven shapes:
forward x up in {1, 2} x with / without the 1x output, backward x pool in {1, 2} x with / without the addend, on inputs with exact zeros and one
all-zero column and, for fp16, on |x| near 2^15.  The bounds are the derived ones of pggan16_ref; the worst error as a share of its bound goes to
profiles/pggan16_contract_errors.txt and must be below 1."""
import os

import numpy as np
import pytest
import torch

from tests import pggan16_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                       # 16-bit elements (128 bytes: a guarded view stays on a 16-byte boundary)
SENTINEL = 7.0
_cases = {}
_report = {}


def _kinds(dt):
    return ('mixed', 'big') if dt == 'f16' else ('mixed',)


def _case(shape, dt, kind):
    """Inputs and models of one (shape, element type, kind), computed once and shared (read-only) by the tests."""
    key = (shape, dt, kind)
    if key not in _cases:
        case = R.make_case(shape, dt, kind)
        case['y'] = R.pixelnorm_act(case['x'], dt)
        _cases[key] = case
    return _cases[key]


def _h8(a, dt):
    t = torch.from_numpy(R.to_h8(np.asarray(a, dtype=np.float32))).to(R.TORCH[dt]).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _from_h8(t):
    return R.from_h8(t.float().cpu().numpy()).astype(np.float64)


def _bits(t):
    return t.view(torch.int16).cpu().numpy()


def _guarded(shape, dt):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device='cuda', dtype=R.TORCH[dt])
    view = buf[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


@pytest.fixture(scope='module', autouse=True)
def _write_report():
    yield
    if not _report:
        return
    lines = ['# l2i_pixelnorm_act_h8 / l2i_pixelnorm_act_bwd_h8 (and _f16) against tests/pggan16_ref.py (float64 on rounded inputs): the worst |error| as a',
             '# share of its derived bound, per element type, kernel, shape (B, C, H, W), input kind and case.  Written by',
             '# tests/test_pggan16_kernels_gpu.py; every share must be below 1.',
             '# worst of all: %.4f' % max(_report.values())]
    for key in sorted(_report):
        lines.append('%-84s share %.4f' % (key, _report[key]))
    with open(os.path.join(ROOT, 'profiles', 'pggan16_contract_errors.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


@pytest.mark.parametrize('low', [False, True], ids=['y', 'y+low'])
@pytest.mark.parametrize('up', [1, 2])
@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_forward(shape, dt, up, low):
    from latent2im_amd import kernels16 as K
    b, ch, h, w = shape
    for kind in _kinds(dt):
        case = _case(shape, dt, kind)
        x = _h8(case['x'], dt)
        out = K.pixelnorm_act(x, R.SLOPE, up=up, low=low)
        y, y_low = out if low else (out, None)
        assert y.dtype == R.TORCH[dt] and tuple(y.shape) == (b, ch // 8, up * h, up * w, 8)
        got = _from_h8(y)
        ref = R.up2(case['y']) if up == 2 else case['y']
        share = R.share(got, ref, R.fwd_bound(ref, dt))
        _report['%-4s fwd %-18s %-5s up %d %s' % (dt, shape, kind, up, 'y+low' if low else 'y')] = share
        print('fwd', dt, shape, kind, up, low, share)
        assert share < 1.0, share
        if up == 2:                                          # the four copies of a result are the same bits
            yb = _bits(y)
            for dy in (0, 1):
                for dx in (0, 1):
                    assert np.array_equal(yb[:, :, dy::2, dx::2], yb[:, :, 0::2, 0::2])
        if low:                                              # the 1x and the 2x output are equal bit for bit where they coincide
            assert tuple(y_low.shape) == tuple(x.shape)
            assert np.array_equal(_bits(y_low), _bits(y)[:, :, 0::up, 0::up])
        if case['zero'] is not None:
            zb, zh, zw = case['zero']
            assert not got[zb, :, up * zh, up * zw].any()      # an all-zero column gives y = 0, not NaN


@pytest.mark.parametrize('with_addend', [False, True], ids=['gy', 'gy+addend'])
@pytest.mark.parametrize('pool', [1, 2])
@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_backward(shape, dt, pool, with_addend):
    from latent2im_amd import kernels16 as K
    for kind in _kinds(dt):
        case = _case(shape, dt, kind)
        gy = case['gy2'] if pool == 2 else case['gy1']
        addend = case['addend'] if with_addend else None
        ref = R.pixelnorm_act_bwd(gy, case['x'], dt, pool=pool, addend=addend)
        x = _h8(case['x'], dt)
        dx = K.pixelnorm_act_bwd(_h8(gy, dt), x, R.SLOPE, pool=pool, addend=None if addend is None else _h8(addend, dt))
        assert dx.dtype == R.TORCH[dt] and dx.shape == x.shape
        got = _from_h8(dx)
        share = R.share(got, ref['dx'], R.bwd_bound(ref, dt))
        _report['%-4s bwd %-18s %-5s pool %d %s' % (dt, shape, kind, pool, 'gy+addend' if with_addend else 'gy')] = share
        print('bwd', dt, shape, kind, pool, with_addend, share)
        assert np.isfinite(got).all()
        assert share < 1.0, share


@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_upsample_and_pool_are_adjoint(shape, dt):
    """<up(y), g> == <y, pool(g)> to fp32 rounding on the kernel's own two outputs, and the fused pool IS that adjoint: with a gradient whose window
    sums are exact in the element type (multiples of 1/8 up to 2), pool = 2 gives the bits of pool = 1 on the summed map."""
    from latent2im_amd import kernels16 as K
    case = _case(shape, dt, 'mixed')
    x = _h8(case['x'], dt)
    y2, y1 = K.pixelnorm_act(x, R.SLOPE, up=2, low=True)
    y2, y1 = _from_h8(y2), _from_h8(y1)
    g = case['gy2'].astype(np.float64)
    lhs, rhs = (y2 * g).sum(), (y1 * R.pool2(g)).sum()
    assert abs(lhs - rhs) <= 2.0 ** -24 * np.abs(y2 * g).sum()
    b, ch, h, w = shape
    g2 = np.random.RandomState(5).randint(-16, 17, size=(b, ch, 2 * h, 2 * w)).astype(np.float32) / 8
    g1 = R.pool2(g2)
    assert np.array_equal(R.round16(g1, dt), g1)
    fused = K.pixelnorm_act_bwd(_h8(g2, dt), x, R.SLOPE, pool=2)
    plain = K.pixelnorm_act_bwd(_h8(g1, dt), x, R.SLOPE, pool=1)
    assert np.array_equal(_bits(fused), _bits(plain))


@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_two_runs_identical_bits(shape, dt):
    from latent2im_amd import kernels16 as K
    case = _case(shape, dt, 'mixed')
    x, gy, add = _h8(case['x'], dt), _h8(case['gy2'], dt), _h8(case['addend'], dt)
    runs = []
    for _ in range(2):
        y2, y1 = K.pixelnorm_act(x, R.SLOPE, up=2, low=True)
        dx = K.pixelnorm_act_bwd(gy, x, R.SLOPE, pool=2, addend=add)
        runs.append([_bits(t) for t in (y2, y1, dx)])
    for a, b_ in zip(*runs):
        assert np.array_equal(a, b_)


@pytest.mark.parametrize('dt', R.DTYPES)
@pytest.mark.parametrize('shape', [(1, 256, 5, 13), (1, 32, 3, 5), (3, 24, 2, 2), (1, 8, 1, 1)], ids=str)
def test_nothing_is_written_outside_the_outputs(shape, dt):
    """Every output inside sentinel guards, pre-filled with NaN: each element is written, nothing around it is."""
    from latent2im_amd import _lib
    b, ch, h, w = shape
    T = R.TORCH[dt]
    case = _case(shape, dt, 'mixed')
    x, gy, add = _h8(case['x'], dt), _h8(case['gy2'], dt), _h8(case['addend'], dt)
    bufs = [_guarded((b, ch // 8, 2 * h, 2 * w, 8), dt), _guarded((b, ch // 8, h, w, 8), dt), _guarded((b, ch // 8, h, w, 8), dt)]
    for _, view in bufs:
        view.fill_(float('nan'))
    (b2, y2), (b1, y1), (bd, dx) = bufs
    _lib.call('l2i_pixelnorm_act_h8', _lib.ptr(y2), _lib.ptr(y1), _lib.ptr(x), b, ch, h, w, R.EPS, R.SLOPE, 2, dtype=T)
    _lib.call('l2i_pixelnorm_act_bwd_h8', _lib.ptr(dx), _lib.ptr(gy), _lib.ptr(x), _lib.ptr(add), b, ch, h, w, R.EPS, R.SLOPE, 2, dtype=T)
    torch.cuda.synchronize()
    for buf, view in bufs:
        assert _untouched(buf) and not bool(torch.isnan(view.float()).any())


@pytest.mark.parametrize('dt', R.DTYPES)
def test_refusals(dt):
    """C % 8 != 0, C > 512 and up / pool outside {1, 2} return L2I_E_UNSUPPORTED (-3), a NULL tensor or a map off a 16-byte boundary L2I_E_ARG (-1),
    before any launch: nothing is written."""
    from latent2im_amd import _lib
    T = R.TORCH[dt]
    tw = '_f16' if dt == 'f16' else ''
    b, h, w = 1, 2, 2
    n = 528 * 4 * h * w                                       # room for every shape named below, upsampled
    x = torch.zeros(n + 8, device='cuda', dtype=T)
    g = torch.zeros(n + 8, device='cuda', dtype=T)
    out = torch.full((n + 8,), SENTINEL, device='cuda', dtype=T)
    low = torch.full((n + 8,), SENTINEL, device='cuda', dtype=T)
    P = _lib.ptr

    def fwd(code, y, y_low, xx, ch, up):
        with pytest.raises(_lib.L2IError, match=r'l2i_pixelnorm_act_h8%s failed \(%d\)' % (tw, code)):
            _lib.call('l2i_pixelnorm_act_h8', y, y_low, xx, b, ch, h, w, R.EPS, R.SLOPE, up, dtype=T)

    def bwd(code, dx, gy, xx, add, ch, pool):
        with pytest.raises(_lib.L2IError, match=r'l2i_pixelnorm_act_bwd_h8%s failed \(%d\)' % (tw, code)):
            _lib.call('l2i_pixelnorm_act_bwd_h8', dx, gy, xx, add, b, ch, h, w, R.EPS, R.SLOPE, pool, dtype=T)

    for ch in (12, 520, 0):
        fwd(-3, P(out), P(low), P(x), ch, 1)
        bwd(-3, P(out), P(g), P(x), None, ch, 1)
    for factor in (0, 3, 4, -1):
        fwd(-3, P(out), None, P(x), 32, factor)
        bwd(-3, P(out), P(g), P(x), None, 32, factor)
    fwd(-1, None, P(low), P(x), 32, 1)
    fwd(-1, P(out), P(low), None, 32, 2)
    bwd(-1, None, P(g), P(x), None, 32, 1)
    bwd(-1, P(out), None, P(x), None, 32, 2)
    bwd(-1, P(out), P(g), None, P(g), 32, 1)
    assert x[1:].data_ptr() % 16 == 2
    fwd(-1, P(out[1:]), None, P(x), 32, 1)
    fwd(-1, P(out), P(low[1:]), P(x), 32, 1)
    fwd(-1, P(out), None, P(x[1:]), 32, 1)
    bwd(-1, P(out), P(g[1:]), P(x), None, 32, 1)
    bwd(-1, P(out), P(g), P(x), P(g[1:]), 32, 1)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((low == SENTINEL).all())
