"""tests/regkeep_ref.py on the CPU: the model is torch's own expression (the BCE of regbce_ref plus w_keep * mean|fc(feat1) - fc(feat0)|, autograd) in
float64; the cases are the ones the issue lists and hold no undecided sign; a float32 evaluation of the kernel's arithmetic in its own order and in a
reversed one is inside the derived bounds on every case; each planted mistake leaves them on a named case; the header declares the entry point, the
ABI version did not move and the ctypes table binds it."""
import os
import re

import numpy as np
import pytest
import torch

from tests import regbce_ref as R
from tests import regkeep_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = {c.id: c for c in M.CASES}
_cache = {}


def _case(cid):
    if cid not in _cache:
        data = M.make_case(CASE[cid])
        _cache[cid] = (data, M.model(data))
    return _cache[cid]


def test_cases_are_the_ones_the_issue_describes():
    assert [(s.B, s.F, s.A, s.K, s.M) for s in M.SHAPES] == [(1, 256, 4, 1, 1), (3, 300, 40, 5, 35), (8, 2048, 40, 1, 39), (2, 2048, 70, 0, 64),
                                                             (2, 512, 130, 64, 64)]
    for s in M.SHAPES:
        assert len(s.cols) == s.K and len(s.keep) == s.M and max(s.cols + s.keep) < s.A and 0 <= s.K <= 64 and 1 <= s.M <= 64
        assert not set(s.cols) & set(s.keep)
    unsorted = M.SHAPES[3].keep
    assert len(set(unsorted)) == len(unsorted) - 1 and list(unsorted) != sorted(unsorted)
    assert M.KINDS == ('exact', 'random', 'equal_rows', 'nan') and len(M.CASES) == 5 * 4 * 2
    assert {c.tf64 for c in M.CASES} == {True, False}
    assert any(s.c_reg == 1.0 for s in M.SHAPES) and any(s.c_reg == 10.0 for s in M.SHAPES) and all(s.w_keep not in (0.0, 1.0) for s in M.SHAPES)


@pytest.mark.parametrize('cid', list(CASE))
def test_no_sign_is_undecided_and_the_kinds_are_what_they_say(cid):
    data, ref = _case(cid)
    c = CASE[cid]
    s = c.shape
    assert ref['undecided'] == 0 and ref['margin_ok']
    d, dd = ref['d'], ref['dd']
    fin = ~np.isnan(d)
    assert bool(((d[fin] == 0) | (np.abs(d[fin]) > 2 * dd[fin])).all())
    assert data['target'].dtype == (np.float64 if c.tf64 else np.float32) and data['cols'].dtype == data['keep'].dtype == np.int64
    if c.kind == 'exact':
        assert not data['feat1'].any() and not data['feat0'].any() and ref['pkeep_bound'] is None
        want = data['fc_b'][data['keep']]
        assert np.array_equal(ref['pkeep'][..., 0].astype(np.float32), want[None, :].repeat(s.B, 0))
        assert np.array_equal(ref['pkeep'][..., 0], ref['pkeep'][..., 1]) and ref['loss'][1] == 0.0 and not ref['g_keep'].any()
    elif c.kind == 'random':
        assert fin.all() and (d != 0).all() and ref['loss'][1] > 1e-3
        assert (ref['g_keep'] > 0).any() and (ref['g_keep'] < 0).any() or d.size == 1
    elif c.kind == 'equal_rows':
        eq = list(data['equal_rows'])
        assert eq and eq[0] == 0 and np.array_equal(data['feat1'][eq].view(np.int32), data['feat0'][eq].view(np.int32))
        assert not d[eq].any() and not dd[eq].any() and not ref['g_keep'][eq].any()
        others = [b for b in range(s.B) if b not in eq]
        assert (d[others] != 0).all()
    else:
        n = data['nan_row']
        assert n == s.B - 1 and np.isnan(d[n]).all() and np.isnan(ref['loss'][1]) and np.isnan(ref['loss'][2])
        assert not ref['g_keep'][n].any() and not ref['g_feat'][n].any() and not ref['g_feat_bound'][n].any()
        assert (ref['loss'][0] == 0.0) if s.K == 0 else np.isnan(ref['loss'][0])
    if s.K == 0:
        assert ref['preds'] is None and ref['loss'][0] == 0.0 and ref['loss_bound'][0] == 0.0


@pytest.mark.parametrize('cid', [c for c in CASE if CASE[c].kind != 'nan'])
def test_model_is_the_torch_expression(cid):
    """c_reg * regbce's loss + w_keep * mean|fc(feat1)[:, keep] - fc(feat0)[:, keep]| and its autograd gradient in float64 on the same operands.
    (The NaN rows, where autograd leaves 0 * NaN at the NaN feature, are pinned in test_no_sign_is_undecided_and_the_kinds_are_what_they_say.)"""
    data, ref = _case(cid)
    feat1 = torch.from_numpy(data['feat1']).double().requires_grad_(True)
    feat0 = torch.from_numpy(data['feat0']).double()
    w, b = torch.from_numpy(data['fc_w']).double(), torch.from_numpy(data['fc_b']).double()
    keep = torch.from_numpy(data['keep'])
    o1, o0 = feat1 @ w.t() + b, feat0 @ w.t() + b
    lk = (o1[:, keep] - o0[:, keep]).abs().mean()
    total = data['w_keep'] * lk
    if len(data['cols']):
        y = torch.from_numpy(np.asarray(data['target'], dtype=np.float64))
        p = o1[:, torch.from_numpy(data['cols'])]
        eps = float(M.EPS)
        lr = -(y * p.clamp(min=eps).log() + (1 - y) * (1 - p).clamp(min=eps).log()).mean()
        total = total + data['c_reg'] * lr
        assert abs(float(lr.detach()) - ref['loss'][0]) <= 1e-12 * max(1.0, abs(ref['loss'][0]))
    g, = torch.autograd.grad(total, feat1)
    assert abs(float(lk.detach()) - ref['loss'][1]) <= 1e-12 and abs(float(total.detach()) - ref['loss'][2]) <= 1e-12 * max(1.0, abs(ref['loss'][2]))
    assert np.abs(g.numpy() - ref['g_feat']).max() <= 1e-9 * (np.abs(ref['g_feat']).max() + 1e-300)


@pytest.mark.parametrize('order', ['kernel', 'reversed'])
@pytest.mark.parametrize('cid', list(CASE))
def test_float32_arithmetic_is_inside_the_bounds(cid, order):
    data, ref = _case(cid)
    got = M.float32(data, order)
    r = dict(pkeep=M.ratio(got['pkeep'], ref['pkeep'], ref['pkeep_bound']), g_feat=M.ratio(got['g_feat'], ref['g_feat'], ref['g_feat_bound']),
             loss=M.ratio(got['loss'], ref['loss'], ref['loss_bound']))
    if ref['preds'] is not None:
        r['preds'] = M.ratio(got['preds'], ref['preds'], ref['preds_bound'])
    print('regkeep f32 %s %s %s' % (cid, order, ' '.join('%s %.3f' % kv for kv in sorted(r.items()))))
    assert all(v <= 1.0 for v in r.values()), r
    if CASE[cid].kind in ('exact', 'equal_rows'):               # equal rows: equal bits of p1 and p0 in either order
        eq = list(data['equal_rows']) if CASE[cid].kind == 'equal_rows' else list(range(CASE[cid].shape.B))
        assert np.array_equal(got['pkeep'][eq][..., 0].view(np.int32), got['pkeep'][eq][..., 1].view(np.int32))


# mistake -> (case, output) on which it must leave the bounds
CAUGHT_ON = {'mean_over_b_only': ('3x300x40x5x35_random_f32', 'loss'), 'sign0_is_1': ('8x2048x40x1x39_equal_rows_f64', 'g_feat'),
             'keep_cols_ignored': ('2x2048x70x0x64_random_f64', 'pkeep'), 'p0_from_feat1': ('8x2048x40x1x39_random_f64', 'loss'),
             'w_keep_dropped': ('2x512x130x64x64_random_f32', 'g_feat'), 'c_reg_dropped': ('3x300x40x5x35_random_f64', 'g_feat'),
             'nan_clamped': ('2x2048x70x0x64_nan_f32', 'loss'), 'bias_one_side': ('1x256x4x1x1_random_f64', 'pkeep')}


@pytest.mark.parametrize('mistake', M.MISTAKES)
def test_planted_mistake_exceeds_the_bounds(mistake):
    cid, name = CAUGHT_ON[mistake]
    data, ref = _case(cid)
    bad = M.model(data, mistake)
    r = M.ratio(bad[name], ref[name], ref[name + '_bound'])
    print('regkeep mistake %s on %s %s: ratio %.3g' % (mistake, cid, name, r))
    assert r > 1.0, (mistake, cid, name, r)


def test_every_mistake_is_in_the_table():
    assert set(CAUGHT_ON) == set(M.MISTAKES) and len(M.MISTAKES) == 8 and all(c in CASE for c, _ in CAUGHT_ON.values())


def test_bce_model_is_reused_by_import():
    assert M.R is R and M.ratio is R.ratio and M.EPS is R.EPS


def test_header_declares_the_entry_and_the_binding_mirrors_it():
    from latent2im_amd import _lib
    with open(os.path.join(ROOT, 'include', 'l2i.h')) as f:
        hdr = f.read()
    m = re.search(r'int l2i_reg_bce_keep_f32\(([^;]*)\);', hdr)
    assert m and '#define L2I_ABI_VERSION 12' in hdr and _lib.ABI_VERSION == 12
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert [p.rsplit(' ', 1)[1].lstrip('*') for p in params] == ['loss', 'preds', 'pkeep', 'g_feat', 'feat1', 'feat0', 'fc_w', 'fc_b', 'cols', 'target',
                                                                 'target_f64', 'keep_cols', 'B', 'F', 'K', 'M', 'c_reg', 'w_keep', 'eps', 'stream']
    want = [_lib.c_p if '*' in p else (_lib.c_f if p.startswith('float') else _lib.c_i) for p in params]
    res, args = _lib._SIGNATURES['l2i_reg_bce_keep_f32']
    assert res is _lib.c_i and args == want
    assert 'l2i_reg_bce_keep_f32' in _lib.EXPORTS and 'l2i_reg_bce_keep_f32' in _lib.ADDITIVE
    # the old entry is as it was
    assert len(_lib._SIGNATURES['l2i_reg_bce_f32'][1]) == 14 and re.search(r'int l2i_reg_bce_f32\(double\* loss, float\* preds, float\* g_feat,', hdr)
    with open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'l2i_loss.hip')) as f:
        src = f.read()
    assert 'extern "C" int l2i_reg_bce_keep_f32(' in src and 'atomicAdd' not in src


def test_options_and_graph_kwargs(tmp_path, capsys):
    """--attr_keep / --attr_keep_attrs: checked after the YAML merge, absent from the namespace and opt.yml when unset, routed to the graph."""
    import yaml
    from latent2im_amd import hostutil
    from latent2im_amd.options import TrainOptions
    base = ['--model', 'stylegan_v2_real', '--transform', 'face', '--attrList', 'Smiling', '--attrPath', os.path.join(ROOT, 'dataset', 'attributes_celeba.txt'),
            '--walk_type', 'linear', '--overwrite_config']

    def parse(models, *extra, print_opt=False):
        return TrainOptions().parse(print_opt=print_opt, argv=base + ['--models_dir', str(models)] + list(extra))
    p = TrainOptions().initialize()
    assert p.get_default('attr_keep') == 0.0 and p.get_default('attr_keep_attrs') is None
    opt = parse(tmp_path / 'a', print_opt=True)
    assert not hasattr(opt, 'attr_keep') and not hasattr(opt, 'attr_keep_attrs')
    kw = hostutil.set_graph_kwargs(opt)
    assert 'attr_keep' not in kw and 'attr_keep_attrs' not in kw
    with open(os.path.join(opt.output_dir, 'opt.yml')) as f:
        assert 'attr_keep' not in f.read()
    opt = parse(tmp_path / 'b', '--attr_keep', '0.5', '--attr_keep_attrs', 'Eyeglasses,Young', print_opt=True)
    capsys.readouterr()
    kw = hostutil.set_graph_kwargs(opt)
    assert kw['attr_keep'] == 0.5 and kw['attr_keep_attrs'] == ['Eyeglasses', 'Young']
    with open(os.path.join(opt.output_dir, 'opt.yml')) as f:
        dump = yaml.load(f, Loader=yaml.FullLoader)
    assert dump['attr_keep'] == 0.5 and dump['attr_keep_attrs'] == 'Eyeglasses,Young'
    cfg = tmp_path / 'again.yml'
    cfg.write_text(yaml.dump(dump))
    again = TrainOptions().parse(print_opt=False, argv=['--config_file', str(cfg), '--models_dir', str(tmp_path / 'c')])
    assert again.attr_keep == 0.5 and again.attr_keep_attrs == 'Eyeglasses,Young'
    assert hostutil.set_graph_kwargs(parse(tmp_path / 'd', '--attr_keep', '0.25'))['attr_keep_attrs'] is None
    spaced = hostutil.set_graph_kwargs(parse(tmp_path / 'f', '--attr_keep', '0.25', '--attr_keep_attrs', ' Eyeglasses, Young ,'))
    assert spaced['attr_keep_attrs'] == ['Eyeglasses', 'Young']
    for bad, why in ((['--attr_keep', '-1'], '>= 0'), (['--attr_keep_attrs', 'Young'], 'needs --attr_keep')):
        with pytest.raises(SystemExit):
            parse(tmp_path / 'e', *bad)
        assert why in capsys.readouterr().err
