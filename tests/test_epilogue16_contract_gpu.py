"""Every 16-bit (h8) conv kernel's fused epilogue against ONE float64 model (tests/epilogue16_ref.py): route x case x element type.  A route is one
instantiation of conv_h8_kernel (or conv_img_h8_kernel) reached through the calls the product uses — conv.H8Conv.forward / .dgrad -> conv.run_h8,
conv.ImgConvH8.forward, and for one route a struct of conv._conv_params — and asserts the plan l2i_conv_h8_plan_for reports for the launch's own
struct (instantiation, epilogue, grid), so a tuning change cannot empty a row unseen.  A case sets one contract field alone, or a combination that
exposes one mistake (tests/test_epilogue16_ref_cpu.py proves that it can, and that a correct float32 evaluation stays inside the bound).

The bound is derived, per element: half an ulp of the store + 2^-23 (K + k) M (epilogue16_ref's docstring); sign planes and everything outside the
launch window — the margins of the buffer the output is carved from, pixels of a y larger than the conv's own size, channel groups at and above
Cout, the whole buffer after a refusal — are bit-exact.  Every test prints `e16 <route> <case> <elem> <error / bound>`."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, conv
from tests import epilogue16_ref as e16
from tests import stream_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                  # sentinel elements on either side of a carved tensor (a multiple of 16 bytes for every element type)
_RAW = {}                     # (route, elem, variant) -> (a, Ma) float64 on the GPU: the raw correlation, once


@contextmanager
def precision(elem):
    old, conv.PRECISION = conv.PRECISION, elem
    try:
        yield sr.ELEM_DTYPES[elem]
    finally:
        conv.PRECISION = old


@contextmanager
def spied():
    """Every _lib.call made inside, as (entry name, struct, dtype): the launch's own struct is what l2i_conv_h8_plan_for is asked about."""
    calls, orig = [], _lib.call

    def spy(name, *args, **k):
        calls.append((name, args[0], k.get('dtype')))
        return orig(name, *args, **k)
    _lib.call = spy
    try:
        yield calls
    finally:
        _lib.call = orig


def variant_of(fields):
    return 'relu_in' if 'relu_in' in fields else ('per_sample' if 'w_bstride' in fields else 'plain')


def raw(route, elem, variant):
    key = (route.name, elem, variant)
    if key not in _RAW:
        cin, cout, k, stride, pad, h, w, b = route.shape
        x, wt = e16.route_data(route, 'per_sample' if variant == 'per_sample' else 'plain')
        a, Ma = e16.corr16(x, wt, stride, pad, e16.transposed(route), e16.geometry(route)['win'][2:], elem, relu_in=variant == 'relu_in')
        _RAW[key] = (a.to(DEV), Ma.to(DEV))
    return _RAW[key]


def carve(t, fill):
    """``t`` in the middle of a buffer filled with ``fill``: (buffer, view shaped like t), 16-byte aligned."""
    buf = torch.full((GUARD + t.numel() + GUARD,), fill, dtype=t.dtype, device=DEV)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def h8(t, dtype, pad_to=8):
    return conv.to_h8(t.to(DEV), pad_to, dtype)


def written_like(view, nchw_mask):
    """Boolean tensor shaped like ``view`` (h8 [B, C/8, H, W, 8] / plane [B, C/8, H, W] / NCHW): the elements of the launch window."""
    if view.dim() == 4 and view.shape[1] == nchw_mask.shape[1]:
        return nchw_mask
    B, C, H, W = nchw_mask.shape
    m = nchw_mask.reshape(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2)
    return m if view.dim() == 5 else m[..., 0]


def untouched_outside(buf, view, before, win_mask, what):
    assert torch.equal(bits(buf[:GUARD]), bits(before[:GUARD])) and torch.equal(bits(buf[-GUARD:]), bits(before[-GUARD:])), 'the launch wrote outside ' + what
    old = before[GUARD:GUARD + view.numel()].view(view.shape)
    out = ~written_like(view, win_mask).to(DEV)
    assert torch.equal(bits(view)[out], bits(old)[out]), 'the launch wrote outside its window of ' + what


def operands(route, fields, kw, dtype):
    """run_h8's keyword arguments of a case, on the GPU; the tensors created here are returned in a second dict (mask_out / rgb / sq buffers)."""
    g, out, side = e16.geometry(route), {}, {}
    B, cout = g['y_shape'][:2]
    m = (lambda t: t.to(DEV)) if route.out_f32 else (lambda t: h8(t, dtype))
    for name in ('out_scale', 'noise', 'bias', 'res_coef_dev'):
        if kw.get(name) is not None:
            out[name] = kw[name].to(DEV)
    for name in ('residual', 'res_sub'):
        if name in kw:
            out[name] = m(kw[name])
    if 'mask_bits' in fields:
        om = sr.sign_plane(sr.to_h8(kw['out_mask'], cout, dtype)).to(DEV)
        out['out_mask'], out['mask_bits'] = om, True
        out['res_mask'] = om if 'same_mask' in fields else sr.sign_plane(sr.to_h8(kw['res_mask'], cout, dtype)).to(DEV)
    else:
        for name in ('out_mask', 'res_mask'):
            if name in kw:
                out[name] = m(kw[name])
    for name in ('noise_w', 'mask', 'act', 'slope', 'gain', 'out_gain', 'accumulate', 'res_coef'):
        if name in kw:
            out[name] = kw[name]
    if 'relu_in' in fields:
        out['relu_in'] = True
    if 'mask_out' in fields:
        side['mask_out'] = carve(torch.full((B, cout // 8) + g['y_shape'][2:], e16.SENTINEL_U8, dtype=torch.uint8), e16.SENTINEL_U8)
        out['mask_out'] = side['mask_out'][1]
    if 'rgb' in fields:
        side['rgb'] = carve(torch.full((B, 3) + g['y_shape'][2:], e16.SENTINEL), e16.SENTINEL)
        out['rgb'] = (kw['rgb'][0].to(DEV), kw['rgb'][1].to(DEV), side['rgb'][1])
    return out, side


def launch(route, fields, dtype, xg, y, wt, gkw):
    """The launch through the product's call of the route's kind; returns (entry name, struct, plan or None)."""
    cin, cout, k, stride, pad, h, w, b = route.shape
    with spied() as calls:
        if route.kind == 'img':
            keep = {n: v for n, v in gkw.items() if n in ('bias', 'act', 'slope', 'gain', 'out_gain', 'sq')}
            assert len(keep) == len(gkw), sorted(set(gkw) - set(keep))
            conv.ImgConvH8(wt, stride, pad, device=DEV).forward(xg, out=y, **keep)
        else:
            if route.out_f32:
                gkw = dict(gkw, out_f32=True)
            if 'w_bstride' in fields:
                planes = torch.stack([conv.pack_weight_h8(wt[i], route.cin_pad) for i in range(b)]).to(DEV)
                gkw = dict(gkw, planes=planes, w_bstride=planes[0].numel() * planes.element_size())
                wt = wt[0]
            if route.kind == 'dgrad':                      # the input gradient of the stride-2 conv cout -> cin is the transposed launch cin -> cout
                conv.H8Conv(wt.transpose(0, 1).contiguous(), 2, pad, device=DEV).dgrad(xg, tuple(y.shape[2:4]), out=y, **gkw)
            elif route.kind == 'struct':                   # run_h8's struct (conv._conv_params) with the window offsets no product call sets
                d = []
                hc = conv.H8Conv(wt, stride, pad, device=DEV, cin_pad=route.cin_pad)
                hc.forward(xg, out=y, _defer=d, **gkw)
                p = d[0][0]
                p.oy_off, p.ox_off = route.off
                _lib.call('l2i_conv2d_h8', p, dtype=dtype)
            else:
                hc = conv.H8Conv(wt, 2 if route.kind == 'tfwd' else stride, pad, transposed=route.kind == 'tfwd', device=DEV, cin_pad=route.cin_pad)
                hc.forward(xg, out=y, **gkw)
    assert len(calls) == 1, calls
    name, p, dt = calls[0]
    assert dt == dtype and name == ('l2i_conv_img_h8' if route.kind == 'img' else 'l2i_conv_transpose2d_h8' if e16.transposed(route) else 'l2i_conv2d_h8')
    return name, p, (None if route.kind == 'img' else _lib.conv_h8_plan(p, e16.transposed(route)))


TRIPLES = [pytest.param(r, c, e, id='%s-%s-%s' % (r.name, c, e)) for e in e16.ELEMS for r, c in e16.pairs(e)]


@pytest.mark.parametrize('route,case,elem', TRIPLES)
def test_h8_epilogue_matches_the_contract(route, case, elem):
    fields, kw, y_prev, rs = e16.make_inputs(route, case, elem)
    g = e16.geometry(route)
    B, cout = g['y_shape'][:2]
    a, Ma = raw(route, elem, variant_of(fields))
    m = e16.model(route, case, elem, a, Ma, kw, y_prev)
    x, wt = e16.route_data(route, 'per_sample' if 'w_bstride' in fields else 'plain')
    oy, ox, oh, ow = g['win']
    win = torch.zeros(g['y_shape'], dtype=torch.bool)
    win[:, :, oy:oy + oh, ox:ox + ow] = True
    with precision(elem) as dtype:
        xg = x.to(DEV) if route.kind == 'img' else h8(x, dtype, route.cin_pad)
        buf, y = carve(y_prev if route.out_f32 else sr.to_h8(y_prev, cout, dtype), e16.SENTINEL)
        gkw, side = operands(route, fields, kw, dtype)
        sq = None
        if 'sq' in fields:
            sq_ref = e16.sq_ref_for(m['want'], elem, rs)
            full = torch.zeros(g['y_shape'])
            full[:, :, oy:oy + oh, ox:ox + ow] = sq_ref
            sq = gkw['sq'] = (h8(full, dtype), torch.zeros(_lib.SQ_SLOTS, device=DEV), [False])
        before = buf.clone()
        name, p, plan = launch(route, fields, dtype, xg, y, wt, gkw)
        torch.cuda.synchronize()
    # the plan of the launch's own struct: the instantiation the row names, the epilogue its fields ask for
    if plan is not None:
        want_plan = e16.expected_plan(route, fields)
        got_plan = {k: getattr(plan, k) for k in want_plan}
        assert got_plan == want_plan, (got_plan, want_plan)
        if set(fields) & set(e16.BAD_GAINS) and not route.out_f32:
            assert plan.epilogue == _lib.H8_EPI_GENERAL          # such gains leave the lean epilogue
    # outside the window: bit-identical
    untouched_outside(buf, y, before, win, 'y')
    got = (y if route.out_f32 else conv.from_h8(y, cout)).double()[:, :, oy:oy + oh, ox:ox + ow]
    err, bound, ratio = sr.worst(got, m['want'].cpu(), m['bound'].cpu())
    worst_of = {'y': ratio}
    if 'mask_out' in fields:
        mbuf, mview = side['mask_out']
        untouched_outside(mbuf, mview, torch.full_like(mbuf, e16.SENTINEL_U8), win, 'mask_out')
        assert torch.equal(mview.cpu()[:, :, oy:oy + oh, ox:ox + ow], e16.mask_out_ref(got)), 'mask_out is not the sign plane of the stored output'
    if 'rgb' in fields:
        rbuf, rview = side['rgb']
        untouched_outside(rbuf, rview, torch.full_like(rbuf, e16.SENTINEL), win[:, :3], 'rgb_out')
        worst_of['rgb'] = sr.worst(rview.double()[:, :, oy:oy + oh, ox:ox + ow], m['rgb'][0].cpu(), m['rgb'][1].cpu())[2]
    if sq is not None:
        assert sq[2][0], 'sq_ref was not fused'
        want_sq, M = e16.sq_ref_sum(got.cpu(), sq_ref, elem)
        n_lane = e16.sq_n_lane(None, route.shape[2], 1024) if plan is None else e16.sq_n_lane(dict(WM=plan.WM, WN=plan.WN), None, plan.grid)
        worst_of['sq'] = abs(float(sq[1].double().sum()) - want_sq) / float(sr.bound_red(torch.tensor(M), n_lane))
    print('e16 %s %s %s %.4f %s' % (route.name, case, elem, max(worst_of.values()), ' '.join('%s=%.4f' % kv for kv in worst_of.items())))
    assert max(worst_of.values()) <= 1.0, (route.name, case, elem, worst_of, err, bound)


# ---- refused, with every buffer untouched: never ignored --------------------------------------------------------------------------------------------
ARG, UNSUPPORTED = -1, -3          # include/l2i.h: L2I_E_ARG, L2I_E_UNSUPPORTED
LEAKY = (2 ** 0.5, 0.2 * 2 ** 0.5)


def _set(**fields):
    """A mutation of the base struct: pointer fields named with the value True get the scratch tensor Z."""
    def mutate(p, Z):
        for k, v in fields.items():
            if k == 'relu_in':
                p.in_mask, p.mask_pos, p.mask_neg = p.x, 1.0, 0.0
            elif k == 'mask':
                p.mask_pos, p.mask_neg = v
            else:
                setattr(p, k, _lib.ptr(Z) if v is True else v)
    return mutate


_SQ = dict(sq_ref=True, sq_out=True)
_RGB = dict(rgb_w=True, rgb_bias=True, rgb_out=True)
REFUSALS = [
    # (id, route, mutation, the code l2i.h names)
    ('in_scale', 'c3s1_ks1', _set(in_scale=True), UNSUPPORTED),
    ('in_scale_transposed', 't_p0_narrow', _set(in_scale=True), UNSUPPORTED),
    ('in_mask_not_x', 'c3s1_ks1', _set(in_mask=True, mask=(1.0, 0.0)), UNSUPPORTED),
    ('in_mask_x_leaky', 'c3s1_ks1', _set(relu_in=True, mask=LEAKY), UNSUPPORTED),
    ('relu_in_1x1', 'c1s1', _set(relu_in=True), UNSUPPORTED),
    ('relu_in_stride2', 'c3s2_p1', _set(relu_in=True), UNSUPPORTED),
    ('relu_in_with_out_mask', 'c3s1_ks1', _set(relu_in=True, out_mask=True), UNSUPPORTED),
    ('relu_in_f32_output', 'f32_c3s1_vec', _set(relu_in=True), UNSUPPORTED),
    ('transposed_sq', 't_p0_narrow', _set(**_SQ), UNSUPPORTED),
    ('transposed_relu_in', 't_p1_wide', _set(relu_in=True), UNSUPPORTED),
    ('transposed_out_f32', 't_p0_wide', _set(out_f32=1), UNSUPPORTED),
    ('out_f32_stride2', 'c3s2_p1', _set(out_f32=1), UNSUPPORTED),
    ('out_f32_sq', 'f32_c3s1_vec', _set(**_SQ), UNSUPPORTED),
    ('out_f32_leaky_mask', 'f32_c3s1_vec', _set(out_mask=True, mask=LEAKY), UNSUPPORTED),          # the fp32 epilogue's masks are binary: refused, not ignored
    ('out_f32_leaky_mask_1x1', 'f32_c1s1', _set(out_mask=True, mask=LEAKY), UNSUPPORTED),
    ('mask_out_out_f32', 'f32_c3s1_wide', _set(mask_out=True), UNSUPPORTED),
    ('mask_out_sq', 'c3s1_ks1', _set(mask_out=True, **_SQ), UNSUPPORTED),
    ('mask_out_rgb', 'c3s1_cin16', _set(mask_out=True, **_RGB), UNSUPPORTED),
    ('mask_bits_out_f32', 'f32_c3s1_vec', _set(mask_bits=1, out_mask=True), ARG),
    ('mask_bits_without_a_mask', 'c3s1_ks1', _set(mask_bits=1), ARG),
    ('rgb_with_residual', 'c3s1_cin16', _set(residual=True, **_RGB), UNSUPPORTED),
    ('rgb_with_out_mask', 'c3s1_rgb64', _set(out_mask=True, **_RGB), UNSUPPORTED),
    ('rgb_with_accumulate', 'c3s1_cin16', _set(accumulate=1, **_RGB), UNSUPPORTED),
    ('rgb_cout40', 'c3s1_ks1', _set(**_RGB), UNSUPPORTED),
    ('rgb_1x1', 'c1s2', _set(**_RGB), UNSUPPORTED),
    ('rgb_transposed', 't_p0_narrow', _set(**_RGB), UNSUPPORTED),
    ('rgb_out_f32', 'f32_c3s1_wide', _set(**_RGB), UNSUPPORTED),
    ('res_sub_without_residual', 'c3s1_ks1', _set(res_sub=True), ARG),
    ('sq_ref_without_sq_out', 'c3s1_ks1', _set(sq_ref=True), ARG),
] + [('img_' + k, 'img_3x3', _set(**{k: v}), UNSUPPORTED) for k, v in dict(
    in_scale=True, in_mask=True, out_scale=True, noise=True, residual=True, res_mask=True, out_mask=True, res_sub=True, accumulate=1, out_f32=1, rgb_w=True,
    mask_out=True, mask_bits=1, ksplit=2, w_bstride=16).items()] + [
    ('img_neg_out_gain', 'img_1x1', _set(out_gain=-0.5), UNSUPPORTED),
    ('img_slope_gt_1', 'img_7x7s2', _set(act=e16.ACT_LRELU, act_slope=1.5), UNSUPPORTED),
    ('img_neg_act_gain', 'img_3x3', _set(act=e16.ACT_LRELU, act_gain=-(2 ** 0.5)), UNSUPPORTED),
]


def base_struct(route, dtype):
    """(entry, struct, keep-alive, buffer, y) of the bare launch of a route, filled as the product fills it."""
    cin, cout, k, stride, pad, h, w, b = route.shape
    g = e16.geometry(route)
    x, wt = e16.route_data(route)
    y_prev = torch.full(g['y_shape'], e16.SENTINEL)
    buf, y = carve(y_prev if route.out_f32 else sr.to_h8(y_prev, cout, dtype), e16.SENTINEL)
    OHf, OWf = g['y_shape'][2:]
    if route.kind == 'img':
        xg, planes = x.to(DEV), conv.pack_weight_img_h8(wt, dtype).to(DEV)
        p = conv._conv_params(xg, planes, y, b, cin, h, w, cout, k, k, stride, pad, pad, OHf, OWf, OHf, OWf)
        return 'l2i_conv_img_h8', p, (xg, planes), buf, y
    xg = h8(x, dtype, route.cin_pad)
    cinp = xg.shape[1] * 8
    if e16.transposed(route):
        planes = conv.pack_weight_h8(wt, 32, dtype).to(DEV)
        p = conv._conv_params(xg, planes, y, b, cinp, h, w, cout, 3, 3, 2, pad, pad, (OHf + 1) // 2, (OWf + 1) // 2, OHf, OWf, 2, mask=(1.0, 0.0))
        return 'l2i_conv_transpose2d_h8', p, (xg, planes), buf, y
    d = []
    hc = conv.H8Conv(wt, stride, pad, device=DEV, cin_pad=route.cin_pad)
    hc.forward(xg, out=y, _defer=d, out_f32=route.out_f32)
    return 'l2i_conv2d_h8', d[0][0], (xg, hc, d), buf, y


@pytest.mark.parametrize('elem', e16.ELEMS)
@pytest.mark.parametrize('what,route,mutate,code', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_field_the_entry_does_not_implement_is_refused_with_the_buffer_untouched(what, route, mutate, code, elem):
    route = e16.BY_NAME[route]
    with precision(elem) as dtype:
        entry, p, keep, buf, y = base_struct(route, dtype)
        _lib.call(entry, p, dtype=dtype)                   # the struct itself is good: the bare launch runs and fills its window
        torch.cuda.synchronize()
        assert bool((y != e16.SENTINEL).any())
        buf.fill_(e16.SENTINEL)
        Z = torch.zeros(max(y.numel(), keep[0].numel()) + 4096, device=DEV)          # in bounds for every operand, should a launch read or write it after all
        mutate(p, Z)
        if route.kind != 'img':
            assert _lib.conv_h8_plan(p, e16.transposed(route)).eligible == 0
        with pytest.raises(_lib.L2IError, match=r'failed \(%d\)' % code):
            _lib.call(entry, p, dtype=dtype)
        torch.cuda.synchronize()
    assert bool((buf == e16.SENTINEL).all()) and float(Z.abs().max()) == 0.0, '%s refused the launch but wrote' % entry
