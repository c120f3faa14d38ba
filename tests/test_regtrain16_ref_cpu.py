"""tests/regtrain16_ref.py on the CPU: a float32 evaluation of every model stays inside its derived bound, every seeded mistake breaks the bound on
the cases that list it (so the bounds are not vacuous), and the build lists what the GPU tests call: both forms of every entry point in
include/l2i.h and in _lib.ADDITIVE, ABI 12, the new file and its _f16 object in csrc/Makefile."""
import os
import re

import pytest
import torch

from latent2im_amd import _lib
from tests import regtrain16_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('l2i_conv2d_wgrad_h8', 'l2i_conv2d_wgrad_ws_h8', 'l2i_bn_ws_h8', 'l2i_bn_stats_h8', 'l2i_bn_apply_h8', 'l2i_bn_bwd_reduce_h8', 'l2i_bn_bwd_apply_h8')
WGRAD = {c.name: c for c in rr.WGRAD_CASES}
BN = {c.name: c for c in rr.BN_CASES}
SMALL_BN = [c.name for c in rr.BN_CASES if c.hw[0] * c.hw[1] <= 64]


def scale_of(case):
    return rr._f(rr._f(case.host_scale) * (1.0 if case.dev_scale is None else rr._f(case.dev_scale)))


@pytest.mark.parametrize('elem', rr.ELEMS)
@pytest.mark.parametrize('name', list(WGRAD))
def test_wgrad_float32_inside_bound(name, elem):
    case = WGRAD[name]
    x, gy = rr.wgrad_data(case)
    want, bound = rr.wgrad(x, gy, case.k, case.stride, case.pad, scale_of(case), elem)
    got, _ = rr.wgrad(x, gy, case.k, case.stride, case.pad, scale_of(case), elem, dt=torch.float32)
    err, b, ratio = rr.worst(got, want, bound)
    print('rt16 wgrad %s %s float32 emulation: error %.3g bound %.3g ratio %.3g' % (name, elem, err, b, ratio))
    assert ratio <= 1.0
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize('elem', rr.ELEMS)
@pytest.mark.parametrize('name,mistake', [(c.name, m) for c in rr.WGRAD_CASES for m in c.mistakes])
def test_wgrad_mistake_breaks_bound(name, mistake, elem):
    case = WGRAD[name]
    x, gy = rr.wgrad_data(case)
    want, bound = rr.wgrad(x, gy, case.k, case.stride, case.pad, scale_of(case), elem)
    wrong, _ = rr.wgrad(x, gy, case.k, case.stride, case.pad, scale_of(case), elem, _mistake=mistake)
    _, _, ratio = rr.worst(wrong, want, bound)
    print('rt16 wgrad %s %s mistake %s: ratio %.3g' % (name, elem, mistake, ratio))
    assert ratio > 1.0


def test_every_wgrad_mistake_is_listed():
    listed = {m for c in rr.WGRAD_CASES for m in c.mistakes}
    assert listed == set(rr.MISTAKES[:7])


def _bn_inputs(case, elem):
    d = rr.bn_data(case)
    (s, q), _ = rr.bn_stats(d['x'], elem)
    n = d['x'].numel() // case.c
    mean, invstd, scale, shift = (t.float() for t in rr.bn_finalize(s, q, n, d['gamma'], d['beta']))
    return d, n, mean, invstd, scale, shift


@pytest.mark.parametrize('elem', rr.ELEMS)
@pytest.mark.parametrize('name', SMALL_BN)
def test_bn_float32_inside_bounds(name, elem):
    case = BN[name]
    d, n, mean, invstd, scale, shift = _bn_inputs(case, elem)
    res = d['residual'] if case.residual else None
    out = d['out'] if case.out_mask else None
    # stats: another summation order in float64 (the kernels sum in float64 too)
    (s, q), (bs, bq) = rr.bn_stats(d['x'], elem)
    xx = rr._d(d['x'], rr.rnd_for(elem))
    perm = torch.randperm(case.b * case.hw[0] * case.hw[1], generator=torch.Generator().manual_seed(1))
    flat = xx.permute(1, 0, 2, 3).reshape(case.c, -1)[:, perm]
    assert rr.worst(flat.cumsum(1)[:, -1], s, bs)[2] <= 1.0 and rr.worst((flat * flat).cumsum(1)[:, -1], q, bq)[2] <= 1.0
    # apply
    want, bound = rr.bn_apply(d['x'], scale, shift, res, case.relu, elem)
    got, _ = rr.bn_apply(d['x'], scale, shift, res, case.relu, elem, dt=torch.float32)
    r_apply = rr.worst(rr.rnd_for(elem)(got), want, bound)[2]
    # the whole forward on float32 scale / shift
    want_f, bound_f = rr.bn_forward(d['x'], d['gamma'], d['beta'], res, case.relu, elem)
    r_fwd = rr.worst(rr.rnd_for(elem)(got), want_f, bound_f)[2]
    # backward
    (sd, sq), (bd, bq2) = rr.bn_bwd_reduce(d['gy'], out, d['x'], mean, invstd, elem)
    (sd32, sq32), _ = rr.bn_bwd_reduce(d['gy'], out, d['x'], mean, invstd, elem, dt=torch.float32)
    r_red = max(rr.worst(sd32, sd, bd)[2], rr.worst(sq32, sq, bq2)[2])
    m_dy, m_dyxh = (sd / n).float(), (sq / n).float()
    want_b, bound_b, dym = rr.bn_bwd_apply(d['gy'], out, d['x'], mean, invstd, d['gamma'], m_dy, m_dyxh, elem)
    got_b, _, dym32 = rr.bn_bwd_apply(d['gy'], out, d['x'], mean, invstd, d['gamma'], m_dy, m_dyxh, elem, dt=torch.float32)
    r_bwd = rr.worst(rr.rnd_for(elem)(got_b), want_b, bound_b)[2]
    print('rt16 bn %s %s float32 emulation: apply %.3g forward %.3g bwd_reduce %.3g bwd_apply %.3g' % (name, elem, r_apply, r_fwd, r_red, r_bwd))
    assert max(r_apply, r_fwd, r_red, r_bwd) <= 1.0
    assert torch.equal(dym32.double(), dym)


@pytest.mark.parametrize('elem', rr.ELEMS)
def test_bn_mistakes_break_bounds(elem):
    case = BN['c72_hw35']
    d, n, mean, invstd, scale, shift = _bn_inputs(case, elem)
    want, bound = rr.bn_apply(d['x'], scale, shift, d['residual'], True, elem)
    wrong, _ = rr.bn_apply(d['x'], scale, shift, d['residual'], True, elem, _mistake='residual_after_relu')
    assert rr.worst(wrong, want, bound)[2] > 1.0
    want, bound = rr.bn_forward(d['x'], d['gamma'], d['beta'], d['residual'], True, elem)
    wrong, _ = rr.bn_forward(d['x'], d['gamma'], d['beta'], d['residual'], True, elem, _mistake='unbiased_variance')
    print('rt16 bn unbiased_variance %s: ratio %.3g' % (elem, rr.worst(wrong, want, bound)[2]))
    assert rr.worst(wrong, want, bound)[2] > 1.0
    (sd, sq), (bd, bq) = rr.bn_bwd_reduce(d['gy'], d['out'], d['x'], mean, invstd, elem)
    (wd, wq), _ = rr.bn_bwd_reduce(d['gy'], d['out'], d['x'], mean, invstd, elem, _mistake='mask_wrong_operand')
    assert rr.worst(wd, sd, bd)[2] > 1.0 and rr.worst(wq, sq, bq)[2] > 1.0
    m_dy, m_dyxh = (sd / n).float(), (sq / n).float()
    want, bound, _ = rr.bn_bwd_apply(d['gy'], d['out'], d['x'], mean, invstd, d['gamma'], m_dy, m_dyxh, elem)
    wrong, _, _ = rr.bn_bwd_apply(d['gy'], d['out'], d['x'], mean, invstd, d['gamma'], m_dy, m_dyxh, elem, _mistake='mask_wrong_operand')
    assert rr.worst(wrong, want, bound)[2] > 1.0


def test_case_tables_cover_the_issue():
    shapes = {(c.k, c.stride, c.cin, c.cout, c.b, c.h, c.w) for c in rr.WGRAD_CASES}
    for need in ((1, 1, 32, 32, 1, 1, 1), (1, 1, 64, 96, 3, 5, 7), (3, 1, 32, 64, 2, 5, 7), (3, 2, 64, 32, 2, 9, 7), (1, 2, 32, 64, 2, 6, 10)):
        assert need in shapes, need
    assert any(c.k == 1 and c.b * c.h * c.w > 512 for c in rr.WGRAD_CASES) and any(c.k == 3 and c.b * c.h * c.w > 512 for c in rr.WGRAD_CASES)
    assert any(c.dev_scale is None and c.host_scale != 1.0 for c in rr.WGRAD_CASES) and any(c.dev_scale is not None for c in rr.WGRAD_CASES)
    assert {a for a, _ in rr.WGRAD_REFUSALS} == {'k', 'stride', 'cin', 'pad', 'ws', 'ws_bytes'}
    assert {c.c for c in rr.BN_CASES} == {8, 72} and {c.b for c in rr.BN_CASES} == {1, 3}
    assert {c.hw[0] * c.hw[1] for c in rr.BN_CASES} == {1, 35, 96 * 96}
    for field in ('residual', 'relu', 'out_mask', 'want_masked'):
        assert {getattr(c, field) for c in rr.BN_CASES} == {False, True}, field


def test_golden_emulation_file_is_what_the_emulation_gives():
    """Step 1 of the fp16 emulation, re-run, against tests/golden/regtrain16_emulation.npz; the recorded figures of both element types are
    printed (properties of 16-bit storage on a random-init net with batch statistics, not of any kernel)."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location('make_regtrain16', os.path.join(ROOT, 'tests', 'golden', 'make_regtrain16.py'))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    g = dict(np.load(mk.PATH))
    assert os.path.getsize(mk.PATH) < 64 * 1024 and len(g['names']) == 161
    for elem in rr.ELEMS:
        rel = g[elem + '_rel_l2']
        print('rt16 emulation %s (2^%d): per-parameter relative L2 max / median %.3f / %.3f, aggregate L2 %.4f cosine %.4f, losses %s; float64 %s'
              % (elem, int(g[elem + '_log2_scale']), rel.max(), np.median(rel), float(g[elem + '_agg_l2']), float(g[elem + '_agg_cos']),
                 ' '.join('%.6f' % v for v in g[elem + '_losses']), ' '.join('%.6f' % v for v in g['loss_f64'])))
        assert float(g[elem + '_agg_cos']) >= {'f16': 0.99, 'bf16': 0.98}[elem]
        assert int(g[elem + '_log2_scale']) == mk.static_log2(elem)
    assert mk.static_log2('f16') == 15 and mk.static_log2('bf16') == 0
    state, data, label = mk.inputs()
    loss64, g64 = mk.oracle64(state, data, label, 1)
    losses, grads = mk.emulate(state, data, label, 'f16', mk.static_log2('f16'), steps=1)
    names, rel, agg, cos = mk.deviations(grads, g64)
    assert names == [str(n) for n in g['names']]
    assert abs(loss64[0] - float(g['loss_f64'][0])) <= 1e-12 and abs(losses[0] - float(g['f16_losses'][0])) <= 1e-9
    # (a conv summed by another number of threads may flip single fp16 roundings: the deviations themselves move in their third digit at most)
    np.testing.assert_allclose(rel, g['f16_rel_l2'], rtol=2e-2)
    assert abs(agg - float(g['f16_agg_l2'])) <= 1e-2 * agg and abs(cos - float(g['f16_agg_cos'])) <= 1e-4


def test_build_lists_the_entry_points():
    with open(os.path.join(ROOT, 'include', 'l2i.h')) as f:
        header = f.read()
    for name in ENTRIES:
        for n in (name, name + '_f16'):
            assert re.search(r'\bint %s\(' % n, header), n + ' is not declared in include/l2i.h'
            assert n in _lib.ADDITIVE and n in _lib.EXPORTS, n
    assert _lib.ABI_VERSION == 12 and re.search(r'#define L2I_ABI_VERSION 12\b', header)
    with open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'Makefile')) as f:
        mk = f.read()
    srcs = re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    objs = re.search(r'^OBJS := (.*)$', mk, re.M).group(1).split()
    assert 'l2i_train_h8.hip' in srcs and 'l2i_train_h8_f16.o' in objs
    assert '-fno-slp-vectorize' in mk
    src = open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'l2i_train_h8.hip')).read()
    assert 'atomic' not in src.split('#include', 1)[1].lower(), 'the new kernels sum in a fixed order: no atomics'
