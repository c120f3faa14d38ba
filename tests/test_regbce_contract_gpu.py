"""l2i_reg_bce_f32 (csrc/l2i_loss.hip) through its raw entry point against tests/regbce_ref.py: every case (four shapes x exact / random / NaN rows x
float64 / fp32 targets) twice on fresh sentinel-guarded loss, preds and g_feat; the worst error as a share of its derived bound (preds bit for
bit on the exact rows, the loss NaN on the NaN row), the guards, equal bits of the two launches; the device logf measured on exact rows that
return it alone; refused calls that write nothing.  Every case prints `regbce <case> <output> err bound ratio`."""
import math

import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from tests import contract_gpu as cg
from tests import regbce_ref as R
from tests import stream_ref as sr

pytestmark = pytest.mark.gpu

E_ARG = -1
_models = {}


def _model(case):
    if case.id not in _models:
        data = R.make_case(case)
        _models[case.id] = (data, R.model(data))
    return _models[case.id]


def _launch(loss, preds, g_feat, d, B, F, K, tf64):
    P = _lib.ptr
    _lib.call('l2i_reg_bce_f32', P(loss), P(preds), P(g_feat), P(d['feat']), P(d['fc_w']), P(d['fc_b']), P(d['cols']), P(d['target']), int(tf64), B, F, K,
              float(R.EPS))


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def _held(case, name, got, want, bound):
    got = got.cpu().numpy()
    ratio = R.ratio(got, want, bound)
    if bound is None:
        print('regbce %s %s exact %s' % (case.id, name, 'equal' if ratio == 0.0 else 'DIFFERENT'))
    else:
        fin = ~np.isnan(np.asarray(want, dtype=np.float64))
        nanpat = np.array_equal(np.isnan(got), ~fin)
        if fin.any() and nanpat:
            err, bnd, _ = sr.worst(torch.from_numpy(np.atleast_1d(got)[np.atleast_1d(fin)]), torch.from_numpy(np.atleast_1d(want)[np.atleast_1d(fin)]),
                                   torch.from_numpy(np.atleast_1d(np.broadcast_to(bound, np.shape(want)))[np.atleast_1d(fin)]))
            print('regbce %s %s err %.3e bound %.3e ratio %.3f' % (case.id, name, err, bnd, ratio))
        else:
            print('regbce %s %s got %s want %s ratio %.3f' % (case.id, name, 'NaN' if np.isnan(got).all() else got.reshape(-1)[:4],
                                                              'NaN' if not fin.any() else 'finite', ratio))
    return ratio


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.id)
def test_cases(case):
    data, ref = _model(case)
    s = case.shape
    d = {k: cg.dev(torch.from_numpy(v)) for k, v in data.items() if isinstance(v, np.ndarray)}
    runs = []
    for _ in range(2):
        lbuf, loss = cg.guarded((1,), dtype=torch.float64)
        pbuf, preds = cg.guarded((s.B, s.K))
        gbuf, g_feat = cg.guarded((s.B, s.F))
        _launch(loss, preds, g_feat, d, s.B, s.F, s.K, case.tf64)
        torch.cuda.synchronize()
        assert cg.untouched(lbuf, loss) and cg.untouched(pbuf, preds) and cg.untouched(gbuf, g_feat), 'the launch wrote outside an output'
        runs.append((loss, preds, g_feat))
    loss, preds, g_feat = runs[0]
    ratios = dict(preds=_held(case, 'preds', preds, ref['preds'], ref['preds_bound']),
                  g_feat=_held(case, 'g_feat', g_feat, ref['g_feat'], ref['g_feat_bound']),
                  loss=_held(case, 'loss', loss, np.array([ref['loss']]), np.array([ref['loss_bound']])))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    if case.kind == 'nan':                                   # NaN in the row's predictions and in the loss, zeros in the row's gradient
        n = data['nan_row']
        assert bool(torch.isnan(preds[n]).all()) and bool(torch.isnan(loss).all()) and not bool(g_feat[n].any())
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), 'two launches differ'
    cg.release()


def test_logf_is_within_its_allowance():
    """The device logf in units of the last place against float64: B = K = 1, feat = 0 and y = 1 make loss = -logf(max(fc_b[col], eps)) alone."""
    bias, want = R.log_probe()
    n = len(bias)
    d = dict(feat=cg.dev(torch.zeros(1, 256)), fc_w=cg.dev(torch.ones(n, 256)), fc_b=cg.dev(torch.from_numpy(bias)),
             target=cg.dev(torch.ones(1, 1, dtype=torch.float64)))
    cols = cg.dev(torch.arange(n, dtype=torch.int64))
    lbuf, losses = cg.guarded((n,), dtype=torch.float64)
    pbuf, preds = cg.guarded((n,))
    gbuf, g_feat = cg.guarded((1, 256))
    P = _lib.ptr
    for i in range(n):
        _lib.call('l2i_reg_bce_f32', P(losses[i:]), P(preds[i:]), P(g_feat), P(d['feat']), P(d['fc_w']), P(d['fc_b']), P(cols[i:]), P(d['target']), 1, 1, 256, 1,
                  float(R.EPS))
    torch.cuda.synchronize()
    assert cg.untouched(lbuf, losses) and cg.untouched(pbuf, preds) and cg.untouched(gbuf, g_feat)
    assert torch.equal(_bits(preds), _bits(torch.from_numpy(bias))), 'an exact row: p is the bias bit for bit'
    got = -losses.cpu().numpy()
    ulps = R.ulps(got, want)
    i = int(ulps.argmax())
    print('regbce logf worst %.4f ulp at p = %.9g (got %.9g, float64 %.17g); mean %.4f ulp; allowance %d ulp'
          % (ulps[i], bias[i], got[i], want[i], ulps.mean(), R.LOGF_ULPS))
    assert np.isfinite(got).all()
    assert math.ceil(ulps.max()) + 1 <= R.LOGF_ULPS, ulps.max()
    cg.release()


def test_refusals():
    """Each null operand, K = 0, K = 65: L2I_E_ARG before any launch, nothing written."""
    case = R.CASES[6]                                        # 3 x 300 x 40 x 5, exact, float64 targets
    data, _ = _model(case)
    s = case.shape
    d = {k: cg.dev(torch.from_numpy(v)) for k, v in data.items() if isinstance(v, np.ndarray)}
    d['cols'] = cg.dev(torch.zeros(65, dtype=torch.int64))
    d['target'] = cg.dev(torch.ones(s.B, 65, dtype=torch.float64))
    lbuf, loss = cg.guarded((1,), dtype=torch.float64)
    pbuf, preds = cg.guarded((s.B, 65))
    gbuf, g_feat = cg.guarded((s.B, s.F))
    P = _lib.ptr
    full = dict(loss=P(loss), preds=P(preds), g_feat=P(g_feat), feat=P(d['feat']), fc_w=P(d['fc_w']), fc_b=P(d['fc_b']), cols=P(d['cols']),
                target=P(d['target']), K=5)

    def refuse(**change):
        a = dict(full, **change)
        cg.refused(E_ARG, 'l2i_reg_bce_f32', a['loss'], a['preds'], a['g_feat'], a['feat'], a['fc_w'], a['fc_b'], a['cols'], a['target'], 1, s.B, s.F, a['K'],
                   float(R.EPS), outs=(lbuf, pbuf, gbuf))
    for name in ('loss', 'preds', 'g_feat', 'feat', 'fc_w', 'fc_b', 'cols', 'target'):
        refuse(**{name: None})
    refuse(K=0)
    refuse(K=65)
    cg.release()
