"""tests/regbce_ref.py on the CPU: the model is torch's own expression (clamp, log, autograd) in float64, NaN row included; the exact rows cover
every clamp edge and the random rows stay clear of them; a float32 evaluation of the kernel's arithmetic in its own order and in the reversed
one is inside the derived bounds on every case; each planted mistake leaves them on a named case."""
import numpy as np
import pytest
import torch

from tests import regbce_ref as R

CASE = {c.id: c for c in R.CASES}
_cache = {}


def _case(cid):
    if cid not in _cache:
        data = R.make_case(CASE[cid])
        _cache[cid] = (data, R.model(data))
    return _cache[cid]


def test_cases_are_the_ones_the_issue_describes():
    assert [(s.B, s.F, s.A, s.K) for s in R.SHAPES] == [(1, 256, 4, 1), (3, 300, 40, 5), (8, 2048, 40, 40), (2, 2048, 70, 64)]
    last = R.SHAPES[3].cols
    assert len(set(last)) == len(last) - 1 and list(last) != sorted(last)
    assert all(len(s.cols) == s.K and max(s.cols) < s.A and s.K <= 64 for s in R.SHAPES)
    assert len(R.CASES) == 4 * 3 * 2
    eps = R.EPS
    assert eps == np.float32(1e-12) and R.EDGES.dtype == np.float32
    assert list(R.EDGES) == [eps, np.nextafter(eps, np.float32(0)), 0, -0.25, np.float32(1 - 2.0 ** -24), 1, 1.5, 0.5] and R.EDGES[4] < 1
    # every edge is a prediction of some exact case
    seen = set()
    for s in R.SHAPES:
        seen |= {c % 8 for c in s.cols}
    assert seen == set(range(8))


@pytest.mark.parametrize('cid', list(CASE))
def test_model_is_the_torch_expression(cid):
    """-mean(y log(clamp(p, eps)) + (1 - y) log(clamp(1 - p, eps))) and its autograd gradient, in float64 on the same operands."""
    data, ref = _case(cid)
    feat = torch.from_numpy(data['feat']).double().requires_grad_(True)
    w, b = torch.from_numpy(data['fc_w']).double(), torch.from_numpy(data['fc_b']).double()
    y = torch.from_numpy(np.asarray(data['target'], dtype=np.float64))
    p = (feat @ w.t() + b)[:, torch.from_numpy(data['cols'])]
    eps = float(R.EPS)
    loss = -(y * p.clamp(min=eps).log() + (1 - y) * (1 - p).clamp(min=eps).log()).mean()
    g, = torch.autograd.grad(loss, feat)
    g = g.numpy()
    if data['nan_row'] is None:
        assert abs(float(loss.detach()) - ref['loss']) <= 1e-12 * max(1.0, abs(ref['loss']))
        scale = np.abs(ref['g_feat']).max() + 1e-300
        assert np.abs(g - ref['g_feat']).max() <= 1e-9 * scale
    else:
        n = data['nan_row']
        assert np.isnan(float(loss.detach())) and np.isnan(ref['loss']) and np.isnan(ref['preds'][n]).all()
        assert not ref['g_feat'][n].any() and not ref['g_feat_bound'][n].any()
        # (autograd gives 0 at every feature of the row but the NaN one, whose own gradient is 0 * NaN; the kernel's contract is 0 throughout)
        keep = ~np.isnan(data['feat'][n])
        assert not g[n][keep].any()
        others = [b_ for b_ in range(g.shape[0]) if b_ != n]
        assert np.allclose(g[others], ref['g_feat'][others], rtol=1e-9, atol=1e-300)


def test_exact_rows_sit_on_the_edges_and_random_rows_clear_of_them():
    for c in R.CASES:
        data, ref = _case(c.id)
        p = ref['preds']
        if c.kind == 'exact':
            assert ref['preds_bound'] is None and np.array_equal(p.astype(np.float32), data['fc_b'][data['cols']][None, :].repeat(c.shape.B, 0))
        elif c.kind == 'random':
            assert ref['preds_bound'] is not None and p.min() >= 0.1 and p.max() <= 0.9 and np.isfinite(ref['loss'])          # no case needs excluding
            assert np.abs(p - 0.5).max() > 0.3
        y = np.asarray(data['target'], dtype=np.float64)
        assert (y == 0).any() and (y == 1).any() or y.size == 1
        assert data['target'].dtype == (np.float64 if c.tf64 else np.float32)
    # the clamp's branches, exactly: the gradient passes at eps and not just below it; at q = 2^-24 and not at q = 0
    data, ref = _case('8x2048x40x40_exact_f64')
    y = data['target']
    n = 8 * 40
    for b in range(8):
        for k in range(40):
            e = R.EDGE_NAMES[k % 8]
            pv = float(R.EDGES[k % 8])
            want = 0.0
            if e in ('eps', 'one_minus_u', 'one', 'above_one', 'half'):
                want += -y[b, k] / n / pv
            if e in ('eps', 'below_eps', 'zero', 'negative', 'one_minus_u', 'half'):
                want -= -(1 - y[b, k]) / n / (1 - pv)
            assert abs(ref['g_pred'][b, k] - want) <= 1e-12 * abs(want), (e, ref['g_pred'][b, k], want)


@pytest.mark.parametrize('order', ['kernel', 'reversed'])
@pytest.mark.parametrize('cid', list(CASE))
def test_float32_arithmetic_is_inside_the_bounds(cid, order):
    data, ref = _case(cid)
    got = R.float32(data, order)
    rp = R.ratio(got['preds'], ref['preds'], ref['preds_bound'])
    rg = R.ratio(got['g_feat'], ref['g_feat'], ref['g_feat_bound'])
    rl = R.ratio(got['loss'], ref['loss'], ref['loss_bound'])
    print('regbce f32 %s %s preds %.3f g_feat %.3f loss %.3f' % (cid, order, rp, rg, rl))
    assert rp <= 1.0 and rg <= 1.0 and rl <= 1.0, (rp, rg, rl)


# mistake -> (case, output) on which it must leave the bounds
CAUGHT_ON = {'clamp_grad_passes': ('3x300x40x5_exact_f64', 'g_feat'), 'boundary_excluded': ('1x256x4x1_exact_f32', 'g_feat'),
             'mean_over_b_only': ('3x300x40x5_random_f32', 'loss'), 'cols_ignored': ('2x2048x70x64_random_f64', 'preds'),
             'bias_dropped': ('8x2048x40x40_random_f64', 'preds'), 'nan_clamped': ('8x2048x40x40_nan_f32', 'loss')}


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_planted_mistake_exceeds_the_bounds(mistake):
    cid, name = CAUGHT_ON[mistake]
    data, ref = _case(cid)
    bad = R.model(data, mistake)
    r = R.ratio(bad[name], ref[name], ref[name + '_bound'])
    print('regbce mistake %s on %s %s: ratio %.3g' % (mistake, cid, name, r))
    assert r > 1.0, (mistake, cid, name, r)


def test_every_mistake_is_in_the_table():
    assert set(CAUGHT_ON) == set(R.MISTAKES) and len(R.MISTAKES) == 6 and all(c in CASE for c, _ in CAUGHT_ON.values())


def test_ratio_and_probe():
    assert R.ratio(np.array([1.0, np.nan]), np.array([1.0, np.nan]), np.array([0.0, 0.0])) == 0.0
    assert R.ratio(np.array([1.0, 2.0]), np.array([1.0, np.nan]), np.array([1.0, 1.0])) == float('inf')
    assert R.ratio(np.array([1.0 + 1e-7]), np.array([1.0]), np.array([0.0])) == float('inf')
    assert R.ratio(np.float32([0.1]), np.array([float(np.float32(0.1))]), None) == 0.0 and R.ratio(np.float32([0.1]), np.array([0.1 + 1e-8]), None) == float('inf')
    bias, want = R.log_probe()
    assert len(bias) == R.LOG_PROBE and bias.dtype == np.float32 and want[0] == np.log(float(R.EPS)) and want[6] == 0.0
    assert R.ulps(np.log(bias.astype(np.float64)).astype(np.float32), want).max() <= 0.5          # a correctly rounded logf
    assert R.LOGF_ULPS >= 2 and (R.LOGF_MEASURED is None or R.LOGF_ULPS == int(np.ceil(R.LOGF_MEASURED)) + 1)
