"""The float64 model of the 16-bit conv epilogues (tests/epilogue16_ref.py) proved on the CPU: a float32 emulation of the kernels (operands rounded to
the element type, F.conv2d in float32, the epilogue in float32 in the kernels' term order, one rounding) stays inside the derived bound on every
(route, case, element type) of tests/test_epilogue16_contract_gpu.py; every seeded mistake exceeds the bound on exactly the cases that list it; the
inputs hold the edges the cases need; and l2i_conv_h8_plan_for (host only) gives every route the instantiation, epilogue and grid its row names."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from latent2im_amd import _lib
from tests import epilogue16_ref as e16
from tests import stream_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RAW = {}


def raw32(route, elem, variant):
    """(float32 correlation of the rounded operands, corr16's (a, Ma)) of a route, once."""
    key = (route.name, elem, variant)
    if key not in _RAW:
        cin, cout, k, stride, pad, h, w, b = route.shape
        x, wt = e16.route_data(route, 'per_sample' if variant == 'per_sample' else 'plain')
        g = e16.geometry(route)
        rnd = sr.rnd_for(elem)
        xx = rnd(x)
        if variant == 'relu_in':
            xx = torch.relu(xx)
        ww = rnd(wt)
        oh, ow = g['win'][2:]

        def one(xs, ws):
            if e16.transposed(route):
                a = F.conv_transpose2d(xs, ws.transpose(0, 1), stride=2)[:, :, pad:, pad:]
                a = F.pad(a, (0, max(0, ow - a.shape[3]), 0, max(0, oh - a.shape[2])))
            else:
                a = F.conv2d(xs, ws, stride=stride, padding=pad)
            return a[:, :, :oh, :ow]
        a32 = torch.cat([one(xx[i:i + 1], ww[i]) for i in range(b)]) if ww.dim() == 5 else one(xx, ww)
        _RAW[key] = (a32.contiguous(), e16.corr16(x, wt, stride, pad, e16.transposed(route), (oh, ow), elem, relu_in=variant == 'relu_in'))
    return _RAW[key]


def variant_of(fields):
    return 'relu_in' if 'relu_in' in fields else ('per_sample' if 'w_bstride' in fields else 'plain')


def emulate(route, fields, elem, a32, kw, y_prev, sq_ref=None):
    """The kernels' arithmetic in float32: H8Out::finish's term order (scale, mask, bias, noise, residual, activation by select, out_gain, old y), the
    lean epilogue's max(v gpos, v gneg) where the launch takes it; one rounding.  Returns dict(y = stored, rgb, sq, mask)."""
    g = e16.geometry(route)
    rnd = (lambda t: t) if route.out_f32 else sr.rnd_for(elem)
    c = lambda t: None if t is None else rnd(e16.cut(t, g['win']))
    f = np.float32
    v = a32.clone()
    if 'out_scale' in kw:
        v = v * kw['out_scale'][:, :, None, None]
    mp, mn = kw.get('mask', (1.0, 0.0))
    if 'out_mask' in kw:
        v = v * torch.where(c(kw['out_mask']) > 0, torch.tensor(f(mp)), torch.tensor(f(mn)))
    if 'bias' in kw:
        v = v + kw['bias'][None, :, None, None]
    if 'noise' in kw:
        v = v + e16.cut(kw['noise'], g['win']) * f(kw['noise_w'])
    if 'residual' in kw:
        r = c(kw['residual'])
        if 'res_sub' in kw:
            rc = f(kw['res_coef']) * (f(1.0) if kw['res_coef_dev'] is None else kw['res_coef_dev'][0])
            r = rc * (r - c(kw['res_sub']))
        if 'res_mask' in kw:
            r = torch.where(c(kw['res_mask']) > 0, r, torch.zeros_like(r))
        v = v + r
    act, sl, gn, og = kw.get('act', e16.ACT_NONE), f(kw.get('slope', 0.2)), f(kw.get('gain', 1.0)), f(kw.get('out_gain', 1.0))
    if e16.expected_epilogue(route, fields, g['y_shape']) == e16.EPI_LEAN or route.kind == 'img':
        gpos = (gn if act == e16.ACT_LRELU else f(1.0)) * og
        gneg = sl * gn * og if act == e16.ACT_LRELU else (f(0.0) if act == e16.ACT_RELU else og)
        v = torch.maximum(v * gpos, v * gneg)
    else:
        if act == e16.ACT_LRELU:
            v = torch.where(v > 0, v, v * sl) * gn
        elif act == e16.ACT_RELU:
            v = torch.relu(v)
        v = v * og
    pre = v
    if kw.get('accumulate'):
        v = v + c(y_prev)
    assert v.dtype == torch.float32
    out = dict(y=rnd(v).double())
    if 'rgb' in kw:
        out['rgb'] = (torch.einsum('bchw,boc->bohw', pre, kw['rgb'][0]) + kw['rgb'][1][None, :, None, None]).double()
    if sq_ref is not None:
        d = rnd(v) - sr.rnd_for(elem)(sq_ref)
        out['sq'] = float((d * d).sum(dtype=torch.float32))
    return out


def compare(route, case, elem, _mistake=None):
    """Emulation against the model (made with ``_mistake``): the largest error / bound over every output, inf where an exact output differs."""
    fields, kw, y_prev, rs = e16.make_inputs(route, case, elem)
    a32, (a, Ma) = raw32(route, elem, variant_of(fields))
    good = e16.model(route, case, elem, a, Ma, kw, y_prev)
    m = good if _mistake is None else e16.model(route, case, elem, a, Ma, kw, y_prev, _mistake=_mistake)
    sq_ref = e16.sq_ref_for(good['want'], elem, rs) if 'sq' in fields else None
    emu = emulate(route, fields, elem, a32, kw, y_prev, sq_ref)
    ratio = sr.worst(emu['y'], m['want'], m['bound'])[2]
    if 'rgb' in fields:
        ratio = max(ratio, sr.worst(emu['rgb'], *m['rgb'])[2])
    if 'mask_out' in fields:
        if not torch.equal(e16.mask_out_ref(emu['y']), e16.mask_out_ref(emu['y'], m['want'], _mistake)):
            ratio = float('inf')
    if 'sq' in fields:
        want, M = e16.sq_ref_sum(emu['y'], sq_ref, elem, m['want'], _mistake)
        n_lane = e16.sq_n_lane(dict(WM=2, WN=2), None, 1024) if route.kind != 'img' else e16.sq_n_lane(None, route.shape[2], 1024)
        ratio = max(ratio, abs(emu['sq'] - want) / float(sr.bound_red(torch.tensor(M), n_lane)))
    return ratio, fields, kw, good, emu


@pytest.mark.parametrize('elem', e16.ELEMS)
@pytest.mark.parametrize('route', e16.ROUTES, ids=lambda r: r.name)
def test_float32_emulation_stays_inside_the_bound(route, elem):
    """The inputs of every (route, case) are ones for which a correct float32 evaluation stays within the derived bound: no GPU involved."""
    n = 0
    for r, case in e16.pairs(elem):
        if r is not route:
            continue
        ratio, fields, kw, good, emu = compare(route, case, elem)
        assert ratio <= 1.0, (route.name, case, elem, ratio)
        a = raw32(route, elem, variant_of(fields))[1][0]          # the unmasked value takes both signs, and both reach the output's activation
        assert bool((a > 0).any()) and bool((a < 0).any()) and bool((good['want'] != 0).any()), (route.name, case)
        n += 1
    assert n >= 4, route.name
    _RAW.clear()


def mistake_route(case):
    return e16.BY_NAME['c3s1_cin16' if 'rgb' in e16.CASES[case][0] else 'c3s1_ks1']


@pytest.mark.parametrize('elem', e16.ELEMS)
@pytest.mark.parametrize('case', list(e16.CASES))
def test_each_mistake_is_seen_by_the_cases_that_list_it_and_by_no_other(case, elem):
    if case in e16.F16_ONLY and elem == 'bf16':
        return
    route = mistake_route(case)
    assert e16.runs_on(e16.CASES[case][0], route)
    seen = tuple(m for m in e16.MISTAKES if compare(route, case, elem, _mistake=m)[0] > 1.0)
    assert set(seen) == set(e16.CASES[case][1]), (case, elem, sorted(set(seen) ^ set(e16.CASES[case][1])))


DATA_MODIFIERS = ('same_mask', 'coef_null', 'big_prev', 'neg_residual', 'tiny', 'big_bias')          # they shape a field's data: no struct field of their own


def where_refused(route, f):
    """The REFUSALS row of tests/test_epilogue16_contract_gpu.py that shows what the route's entry does with a field it does not accept; None for a
    modifier that only shapes the data of a field (which has its own row)."""
    if f in DATA_MODIFIERS:
        return None
    if route.kind == 'img':
        return {'rgb': 'img_rgb_w', 'relu_in': 'img_in_mask', 'leaky': 'img_out_mask'}.get(f, 'img_' + f)
    if route.out_f32:
        return {'leaky': 'out_f32_leaky_mask', 'mask_bits': 'mask_bits_out_f32', 'mask_out': 'mask_out_out_f32', 'sq': 'out_f32_sq', 'relu_in': 'relu_in_f32_output',
                'rgb': 'rgb_out_f32'}[f]
    if e16.transposed(route):
        return {'sq': 'transposed_sq', 'relu_in': 'transposed_relu_in', 'rgb': 'rgb_transposed'}[f]
    k, stride = route.shape[2], route.shape[3]
    if k == 3 and stride == 1:
        return {'rgb': 'rgb_cout40'}[f]
    return {'relu_in': 'relu_in_1x1' if k == 1 else 'relu_in_stride2', 'rgb': 'rgb_1x1'}[f]


from tests.test_epilogue16_contract_gpu import REFUSALS          # noqa: E402 (the table only: nothing there runs without a GPU)
REFUSAL_IDS = {r[0] for r in REFUSALS}


def test_every_mistake_has_a_case_and_the_tables_are_well_formed():
    assert {m for _, ms in e16.CASES.values() for m in ms} == set(e16.MISTAKES)
    for name, (fields, _) in e16.CASES.items():
        assert all(f in e16.FIELDS or f in e16.MODIFIERS for f in fields), name
    assert len({r.name for r in e16.ROUTES}) == len(e16.ROUTES)
    for r in e16.ROUTES:
        ev = e16.everything(r)
        assert e16.runs_on(ev, r) and 'bias' in ev and not ('relu' in ev and 'lrelu' in ev)
        for f in set(e16.FIELDS + e16.MODIFIERS) - e16.accepts(r):          # not accepted: a refusal row of the GPU file says what the entry does with it
            row = where_refused(r, f)
            assert row is None or row in REFUSAL_IDS, (r.name, f, row)
    # the operand sets the pair / chain3 tests of test_h8_gpu.py lean on, on the 1x1 stride-1 routes
    for name in ('mask_out_general', 'pair_planes'):
        assert e16.runs_on(e16.CASES[name][0], e16.BY_NAME['c1s1']) and e16.runs_on(e16.CASES[name][0], e16.BY_NAME['c1s1_wide'])
    assert set(e16.CASES['mask_out_general'][0]) == {'bias', 'residual', 'relu', 'mask_out'}
    # the sentinels are exact in every element type
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert float(torch.tensor(e16.SENTINEL, dtype=dt)) == e16.SENTINEL
    assert float(torch.tensor(-7777.25, dtype=torch.bfloat16)) != -7777.25


def test_case_inputs_hold_the_edges():
    route = e16.BY_NAME['c3s1_ks1']
    for case, (fields, _) in e16.CASES.items():
        if not e16.runs_on(fields, route):
            continue
        _, kw, y_prev, _ = e16.make_inputs(route, case, 'f16')
        for name in ('out_mask', 'res_mask'):
            if name in kw:
                m = kw[name]
                z = m == 0
                assert 0.25 < float(z.float().mean()) < 0.42 and bool(torch.signbit(m[z]).any()) and not bool(torch.signbit(m[z]).all()), (case, name)
        assert ('accumulate' in fields) == bool((y_prev != e16.SENTINEL).any())
    # tiny_out: stored fp16 outputs that are subnormal, and ones that round to zero from a positive fp32 value
    ratio, fields, kw, good, emu = compare(route, 'tiny_out', 'f16')
    y, v = emu['y'], good['want']
    assert bool(((y > 0) & (y < 2.0 ** -14)).any()) and bool(((y == 0) & (v > 2.0 ** -60)).any())
    assert not torch.equal(e16.mask_out_ref(y), e16.mask_out_ref(y, v, 'sign_from_unrounded'))


def test_half_ulp_at_the_edges():
    h = lambda v, elem: float(sr.half_ulp(torch.tensor([v], dtype=torch.float64), elem))
    assert h(1.0, 'bf16') == 2.0 ** -8 and h(2.0 - 2.0 ** -20, 'bf16') == 2.0 ** -8 and h(2.0, 'bf16') == 2.0 ** -7 and h(-2.0, 'bf16') == 2.0 ** -7
    assert h(1.0, 'f16') == 2.0 ** -11 and h(0.999, 'f16') == 2.0 ** -12
    assert h(0.0, 'f16') == 2.0 ** -25 and h(0.0, 'bf16') == 2.0 ** -134                                   # the spacing of the subnormals
    assert h(2.0 ** -14, 'f16') == 2.0 ** -25 and h(2.0 ** -15, 'f16') == 2.0 ** -25 and h(2.0 ** -13, 'f16') == 2.0 ** -24
    assert e16.half_ulp is sr.half_ulp and e16.worst is sr.worst


# ---- l2i_conv_h8_plan_for ---------------------------------------------------------------------------------------------------------------------
def fake_params(route, fields):
    """The struct conv.run_h8 fills for a (route, fields) launch, with made-up 16-byte aligned addresses (the host-only query never dereferences them)."""
    g = e16.geometry(route)
    cin, cout, k, stride, pad, h, w, b = route.shape
    cin = (cin + route.cin_pad - 1) // route.cin_pad * route.cin_pad
    P = ctypes.c_void_p
    p = _lib.ConvParams()
    p.x, p.y, p.w_hi = P(4096), P(8192), P(12288)
    p.B, p.Cin, p.H, p.W, p.Cout, p.CoutP = b, cin, h, w, cout, g['CoutP']
    p.KH = p.KW = k
    p.stride, p.pad_y, p.pad_x = stride, pad, pad
    p.OHf, p.OWf = g['y_shape'][2:]
    oy, ox, oh, ow = g['win']
    tr = e16.transposed(route)
    p.OH, p.OW = ((oh + 1) // 2, (ow + 1) // 2) if tr else (oh, ow)
    p.oy_step = p.ox_step = 2 if tr else 1
    p.oy_off, p.ox_off = oy, ox
    p.mask_pos, p.mask_neg = (2 ** 0.5, 0.2 * 2 ** 0.5) if 'leaky' in fields else (1.0, 0.0)
    p.act = e16.ACT_LRELU if 'lrelu' in fields else (e16.ACT_RELU if 'relu' in fields else e16.ACT_NONE)
    p.act_slope, p.act_gain = (1.5 if 'slope_gt_1' in fields else 0.2), (-1.0 if 'neg_act_gain' in fields else 1.0)
    p.out_gain = -0.5 if 'neg_out_gain' in fields else 1.0
    for name in ('out_scale', 'out_mask', 'noise', 'bias', 'residual', 'res_mask', 'res_sub'):
        if name in fields:
            setattr(p, name, P(16384))
    p.accumulate = int('accumulate' in fields)
    if 'sq' in fields:
        p.sq_ref, p.sq_out = P(16384), P(16384)
    if 'rgb' in fields:
        p.rgb_w, p.rgb_bias, p.rgb_out = P(16384), P(16384), P(16384)
    if 'mask_out' in fields:
        p.mask_out = P(16384)
    p.mask_bits = int('mask_bits' in fields)
    if 'relu_in' in fields:
        p.in_mask, p.mask_pos, p.mask_neg = p.x, 1.0, 0.0
    p.out_f32 = int(route.out_f32)
    return p


def plan_dict(plan):
    return {n: getattr(plan, n) for n, _ in _lib.ConvH8Plan._fields_}


@pytest.mark.parametrize('route', [r for r in e16.ROUTES if r.kind != 'img'], ids=lambda r: r.name)
def test_plan_of_every_route_and_case(route):
    """Every row reaches the instantiation it names, with the epilogue its fields ask for: a tuning change that moves a row shows here, without a GPU."""
    for r, case in e16.pairs('f16'):
        if r is not route:
            continue
        fields = e16.case_fields(case, route)
        got = plan_dict(_lib.conv_h8_plan(fake_params(route, fields), e16.transposed(route)))
        want = e16.expected_plan(route, fields)
        assert {k: got[k] for k in want} == want, (route.name, case, _lib.load().l2i_last_error())
        assert got['rgb'] == int('rgb' in fields) and 0 < got['lds_bytes'] <= 160 * 1024 and got['nchunks'] * 16 * got['KS'] == fake_params(route, fields).Cin
        if set(fields) & set(e16.BAD_GAINS) and not route.out_f32:
            assert got['epilogue'] == e16.EPI_GENERAL
        g8 = got['grid'] >> 3
        assert sorted((blk & 7) * g8 + (blk >> 3) for blk in range(got['grid'])) == list(range(got['grid']))      # the block order is a permutation


def test_plan_refusals_and_header():
    lib = _lib.load()
    route = e16.BY_NAME['f32_c3s1_vec']
    p = fake_params(route, ('out_mask',))
    assert _lib.conv_h8_plan(p).eligible == 1
    p.mask_pos, p.mask_neg = 2 ** 0.5, 0.2 * 2 ** 0.5                                        # a leaky mask on the fp32 output: refused, not ignored
    refused = _lib.conv_h8_plan(p)
    assert refused.eligible == 0 and not any(v for k, v in plan_dict(refused).items()) and b'binary' in lib.l2i_last_error()
    p = fake_params(e16.BY_NAME['c3s1_ks1'], ())
    p.in_scale = ctypes.c_void_p(16384)
    assert _lib.conv_h8_plan(p).eligible == 0
    assert _lib.conv_h8_plan(fake_params(e16.BY_NAME['c3s1_ks1'], ()), transposed=True).eligible == 0          # a correlation struct on the transposed entry
    assert lib.l2i_conv_h8_plan_for(None, 0, None) == -1
    hdr = open(os.path.join(ROOT, 'include', 'l2i.h')).read()
    assert 'l2i_conv_h8_plan_for' in hdr and 'l2i_conv_h8_plan_for' in _lib.ADDITIVE and '#define L2I_ABI_VERSION 12' in hdr and _lib.ABI_VERSION == 12
    names = re.search(r'typedef struct l2i_conv_h8_plan \{(.*?)\} l2i_conv_h8_plan;', hdr, re.S).group(1)
    names = re.sub(r'/\*.*?\*/', '', names, flags=re.S)
    assert [n.strip() for part in re.findall(r'int32_t ([^;]+);', names) for n in part.split(',')] == [n for n, _ in _lib.ConvH8Plan._fields_]
    for i, name in enumerate(('LEAN', 'GENERAL', 'F32_VEC', 'F32_SCALAR')):
        assert '#define L2I_H8_EPI_%s %d' % (name, i) in hdr and getattr(_lib, 'H8_EPI_' + name) == i == getattr(e16, 'EPI_' + name)
    assert 'mask is leaky here' not in hdr
