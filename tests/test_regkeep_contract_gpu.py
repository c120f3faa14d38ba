"""l2i_reg_bce_keep_f32 (csrc/l2i_loss.hip) through its raw entry point against tests/regkeep_ref.py: every case (five shapes x exact / random /
equal rows / NaN row x float64 / fp32 targets) twice on fresh sentinel-guarded loss, preds, pkeep and g_feat; the worst error as a share of its derived
bound (predictions bit for bit on the exact rows and p1 == p0 bit for bit on bitwise equal rows), the guards, equal bits of the two launches, the BCE
outputs against a launch of l2i_reg_bce_f32 on the same operands; refused calls that write nothing.  Every case prints
`regkeep <case> <output> err bound ratio`."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from tests import contract_gpu as cg
from tests import regkeep_ref as M
from tests import stream_ref as sr

pytestmark = pytest.mark.gpu

E_ARG = -1
_models = {}


def _model(case):
    if case.id not in _models:
        data = M.make_case(case)
        _models[case.id] = (data, M.model(data))
    return _models[case.id]


def _launch(out, d, s, tf64, c_reg, w_keep):
    P = _lib.ptr
    _lib.call('l2i_reg_bce_keep_f32', P(out['loss']), P(out['preds']), P(out['pkeep']), P(out['g_feat']), P(d['feat1']), P(d['feat0']), P(d['fc_w']), P(d['fc_b']),
              P(d['cols']) if s.K else None, P(d['target']) if s.K else None, int(tf64), P(d['keep']), s.B, s.F, s.K, s.M, float(c_reg), float(w_keep), float(M.EPS))


def _outputs(s):
    bufs, out = {}, {}
    for name, shape, dt in (('loss', (3,), torch.float64), ('preds', (s.B, max(s.K, 1)), torch.float32), ('pkeep', (s.B, s.M, 2), torch.float32),
                            ('g_feat', (s.B, s.F), torch.float32)):
        bufs[name], out[name] = cg.guarded(shape, dtype=dt)
    return bufs, out


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def _held(case, name, got, want, bound):
    got = got.cpu().numpy()
    ratio = M.ratio(got, want, bound)
    if bound is None:
        print('regkeep %s %s exact %s' % (case.id, name, 'equal' if ratio == 0.0 else 'DIFFERENT'))
        return ratio
    want, bound = np.asarray(want, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(want))
    fin = ~np.isnan(want)
    if fin.any() and np.array_equal(np.isnan(got), ~fin):
        err, bnd, _ = sr.worst(torch.from_numpy(got[fin]), torch.from_numpy(want[fin]), torch.from_numpy(bound[fin]))
        print('regkeep %s %s err %.3e bound %.3e ratio %.3f' % (case.id, name, err, bnd, ratio))
    else:
        print('regkeep %s %s got %s want %s ratio %.3f' % (case.id, name, 'NaN' if np.isnan(got).all() else got.reshape(-1)[:4],
                                                           'NaN' if not fin.any() else 'finite', ratio))
    return ratio


@pytest.mark.parametrize('case', M.CASES, ids=lambda c: c.id)
def test_cases(case):
    data, ref = _model(case)
    s = case.shape
    d = {k: cg.dev(torch.from_numpy(v)) for k, v in data.items() if isinstance(v, np.ndarray) and v.size}
    runs = []
    for _ in range(2):
        bufs, out = _outputs(s)
        _launch(out, d, s, case.tf64, s.c_reg, s.w_keep)
        torch.cuda.synchronize()
        assert all(cg.untouched(bufs[k], out[k]) for k in out), 'the launch wrote outside an output'
        if s.K == 0:
            assert cg.untouched(bufs['preds']), 'K = 0 writes no prediction'
        runs.append(out)
    out = runs[0]
    ratios = dict(pkeep=_held(case, 'pkeep', out['pkeep'], ref['pkeep'], ref['pkeep_bound']),
                  g_feat=_held(case, 'g_feat', out['g_feat'], ref['g_feat'], ref['g_feat_bound']))
    for i, name in enumerate(('reg', 'keep', 'total')):
        ratios[name] = _held(case, name, out['loss'][i:i + 1], ref['loss'][i:i + 1], ref['loss_bound'][i:i + 1])
    if s.K:
        ratios['preds'] = _held(case, 'preds', out['preds'], ref['preds'], ref['preds_bound'])
    assert all(r <= 1.0 for r in ratios.values()), ratios
    pk = out['pkeep']
    if case.kind in ('exact', 'equal_rows'):                  # bitwise equal feature rows: bitwise equal outputs, a zero keep gradient
        eq = list(data['equal_rows']) if case.kind == 'equal_rows' else list(range(s.B))
        assert torch.equal(_bits(pk[eq][..., 0]), _bits(pk[eq][..., 1]))
    if case.kind == 'exact':
        assert float(out['loss'][1]) == 0.0
        if s.K == 0:
            assert not bool(out['g_feat'].any()) and float(out['loss'][0]) == 0.0 and float(out['loss'][2]) == 0.0
    if case.kind == 'nan':                                    # NaN in the row's p1 and in keep, zeros in the row's gradient
        n = data['nan_row']
        assert bool(torch.isnan(pk[n, :, 0]).all()) and not bool(torch.isnan(pk[n, :, 1]).any())
        assert bool(torch.isnan(out['loss'][1:]).all()) and not bool(out['g_feat'][n].any())
        assert bool(torch.isnan(out['loss'][0])) if s.K else float(out['loss'][0]) == 0.0
    for k in out:
        if k != 'preds' or s.K:
            assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), 'two launches differ in %s' % k
    # the BCE outputs against l2i_reg_bce_f32 on the same operands: preds and loss[0] always, g_feat too at c_reg = 1, w_keep = 0
    if s.K:
        P = _lib.ptr
        lbuf, loss = cg.guarded((1,), dtype=torch.float64)
        pbuf, preds = cg.guarded((s.B, s.K))
        gbuf, g_feat = cg.guarded((s.B, s.F))
        _lib.call('l2i_reg_bce_f32', P(loss), P(preds), P(g_feat), P(d['feat1']), P(d['fc_w']), P(d['fc_b']), P(d['cols']), P(d['target']), int(case.tf64),
                  s.B, s.F, s.K, float(M.EPS))
        bufs, plain = _outputs(s)
        _launch(plain, d, s, case.tf64, 1.0, 0.0)
        torch.cuda.synchronize()
        assert all(cg.untouched(bufs[k], plain[k]) for k in plain)
        assert torch.equal(_bits(out['preds']), _bits(preds)) and torch.equal(_bits(plain['preds']), _bits(preds)), 'preds differ from l2i_reg_bce_f32'
        assert torch.equal(_bits(out['loss'][:1]), _bits(loss)) and torch.equal(_bits(plain['loss'][:1]), _bits(loss)), 'loss[0] differs from l2i_reg_bce_f32'
        assert torch.equal(_bits(plain['g_feat']), _bits(g_feat)), 'g_feat at c_reg = 1, w_keep = 0 differs from l2i_reg_bce_f32'
        assert torch.equal(_bits(plain['pkeep']), _bits(out['pkeep']))
        print('regkeep %s bce outputs equal to l2i_reg_bce_f32 bit for bit' % case.id)
    cg.release()


def test_refusals():
    """Each required null operand, M = 0, M = 65, K = -1, K = 65, K > 0 with a null preds / cols / target: L2I_E_ARG before any launch, nothing written."""
    case = next(c for c in M.CASES if c.shape.K == 5 and c.kind == 'exact' and c.tf64)
    data, _ = _model(case)
    s = case.shape
    d = {k: cg.dev(torch.from_numpy(v)) for k, v in data.items() if isinstance(v, np.ndarray)}
    d['cols'] = cg.dev(torch.zeros(65, dtype=torch.int64))
    d['keep'] = cg.dev(torch.zeros(65, dtype=torch.int64))
    d['target'] = cg.dev(torch.ones(s.B, 65, dtype=torch.float64))
    lbuf, loss = cg.guarded((3,), dtype=torch.float64)
    pbuf, preds = cg.guarded((s.B, 65))
    kbuf, pkeep = cg.guarded((s.B, 65, 2))
    gbuf, g_feat = cg.guarded((s.B, s.F))
    P = _lib.ptr
    full = dict(loss=P(loss), preds=P(preds), pkeep=P(pkeep), g_feat=P(g_feat), feat1=P(d['feat1']), feat0=P(d['feat0']), fc_w=P(d['fc_w']), fc_b=P(d['fc_b']),
                cols=P(d['cols']), target=P(d['target']), keep=P(d['keep']), B=s.B, F=s.F, K=5, M=35)

    def refuse(**change):
        a = dict(full, **change)
        cg.refused(E_ARG, 'l2i_reg_bce_keep_f32', a['loss'], a['preds'], a['pkeep'], a['g_feat'], a['feat1'], a['feat0'], a['fc_w'], a['fc_b'], a['cols'],
                   a['target'], 1, a['keep'], a['B'], a['F'], a['K'], a['M'], 10.0, 0.5, float(M.EPS), outs=(lbuf, pbuf, kbuf, gbuf))
    for name in ('loss', 'pkeep', 'g_feat', 'feat1', 'feat0', 'fc_w', 'fc_b', 'keep'):
        refuse(**{name: None})
    for name in ('preds', 'cols', 'target'):                  # required when K > 0
        refuse(**{name: None})
    for change in (dict(M=0), dict(M=65), dict(M=-1), dict(K=-1), dict(K=65), dict(B=0), dict(F=0)):
        refuse(**change)
    cg.release()
