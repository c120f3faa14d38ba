"""The model of the FIR, bias-activation and weight-plane kernels (tests/fir_ref.py) against independently written compositions (oracle.sg2,
F.conv2d on a zero-inserted and padded input, plain torch epilogues) and the committed fixtures; the row table against the mistakes it claims to
catch, and the blind spot of a symmetric FIR; every row's bound against float32 evaluations of the same formula in two orders; the rows against
the launch predicates, the refusal lines and the kernels of the two source files."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from latent2im_amd import kernels16, synth
from oracle import sg2
from tests import fir_ref as fr
from tests import stream_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = fr.all_rows()
FIR_ROWS = [r for r in ROWS if r.op == 'fir']
ELEMS = lambda row: ('f32',) if row.kind == 'f32' else ('bf16', 'f16')
_LOG = []


@pytest.fixture(scope='module', autouse=True)
def _error_log():
    """L2I_FIR_CONTRACT_ERRORS=<file>: the error of the float32 evaluations of every row beside its bound (profiles/fir_contract_errors.txt)."""
    yield
    path = os.environ.get('L2I_FIR_CONTRACT_ERRORS')
    if path:
        with open(path, 'w') as f:
            f.write('# row element output order: largest |fp32 evaluation - float64 model| over the bound at that element (tests/test_fir_ref_cpu.py)\n' + '\n'.join(_LOG) + '\n')


def conv_composition(x, k, up, down, pad):
    """Zero insertion, F.pad (negative: a crop), F.conv2d with the flipped kernel, a strided slice: x and y treated apart."""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    B, C, H, W = x.shape
    z = x.new_zeros(B, C, H, uy, W, ux)
    z[:, :, :, 0, :, 0] = x
    z = F.pad(z.reshape(B * C, 1, H * uy, W * ux), [px0, px1, py0, py1])
    y = F.conv2d(z, torch.flip(k, [0, 1])[None, None].to(x.dtype))[:, :, ::dy, ::dx]
    return y.reshape(B, C, y.shape[2], y.shape[3])


def test_test_kernels_are_asymmetric_dyadic_and_separable_as_stated():
    for name, k in fr.KERNELS.items():
        if name in ('SYM44', 'K11'):
            continue
        assert not torch.equal(k, torch.flip(k, [0, 1])) and (k.shape[0] != k.shape[1] or not torch.equal(k, k.t())), name
        assert torch.equal(k.float().double(), k) and torch.equal(k * 1024, torch.round(k * 1024)) and bool((k < 0).any()), name
    assert len(set(fr.K1Y + fr.K1X)) == 8 and fr.K1Y != fr.K1X
    ky, kx = kernels16.separable(fr.KERNELS['K44'].float())
    assert tuple(ky) == fr.K1Y and tuple(kx) == fr.K1X
    assert kernels16.separable(fr.KERNELS['K44N'].float()) is None
    s = fr.KERNELS['SYM44']
    assert torch.equal(s, torch.flip(s, [0, 1])) and torch.equal(s, s.t())


@pytest.mark.parametrize('row', FIR_ROWS, ids=lambda r: r.id)
def test_fir_of_every_row_is_the_conv2d_composition_and_the_oracle(row):
    kw = fr.make_inputs(row, ELEMS(row)[0])
    x, k, up, down, pad = kw['x'].double(), kw['k'].double(), kw['up'], kw['down'], kw['pad']
    want = fr.upfirdn2d(x, k, up, down, pad)['y'][0]
    assert torch.allclose(want, conv_composition(x, k, up, down, pad), rtol=0, atol=1e-12)
    if up[0] == up[1] and down[0] == down[1] and pad[0] == pad[2] and pad[1] == pad[3]:
        assert torch.allclose(want, sg2.upfirdn2d(x, k, up[0], down[0], (pad[0], pad[1])), rtol=0, atol=1e-12)


@pytest.mark.parametrize('up,down,p0,p1', [(1, 1, 2, 1), (2, 1, 2, 1), (1, 2, 1, 1), (2, 2, 3, 2), (1, 1, -1, 2), (3, 2, 0, 4)])
@pytest.mark.parametrize('kname', ['K44', 'K44N', 'K23', 'K35', 'K88'])
def test_model_is_the_oracle_where_the_oracle_can_say_it(kname, up, down, p0, p1):
    x = torch.randn(2, 3, 9, 11, generator=torch.Generator().manual_seed(7)).double()
    k = fr.KERNELS[kname]
    assert torch.allclose(fr.upfirdn2d(x, k, (up, up), (down, down), (p0, p1, p0, p1))['y'][0], sg2.upfirdn2d(x, k, up, down, (p0, p1)), rtol=0, atol=1e-12)


def test_model_reproduces_the_committed_fixtures(golden):
    g = golden('upfirdn2d')
    for i, (n, c, h, w, up, down, p0, p1, gain) in enumerate(g['cases']):
        up, down, p0, p1 = int(up), int(down), int(p0), int(p1)
        x = np.random.RandomState(20 + i).randn(int(n), int(c), int(h), int(w)).astype(np.float32)
        y = fr.upfirdn2d(sr.T(x), sr.T(synth.fir_kernel(gain=gain)), (up, up), (down, down), (p0, p1, p0, p1))['y'][0]
        assert torch.allclose(y, sr.T(g['y_%d' % i]).double(), rtol=1e-5, atol=1e-6), i
    g = golden('fused_bias_act')
    x, b, ref = sr.T(g['x']), sr.T(g['b']), sr.T(g['ref'])
    step_b = x[0, 0].numel()
    for act in (1, 3):
        for grad in (0, 1, 2):
            y = fr.fused_bias_act(x, b if grad == 0 else None, ref if grad == 1 else None, step_b, b.numel(), act, grad, 0.2, 2 ** 0.5)['y'][0]
            assert torch.allclose(y.view(x.shape), sr.T(g['y_%d%d' % (act, grad)]), rtol=1e-6, atol=1e-7), (act, grad)


def test_the_two_epilogue_orders_are_the_plain_compositions():
    rs = torch.Generator().manual_seed(11)
    R = lambda *s: torch.randn(*s, generator=rs).double()
    x, k = R(2, 3, 6, 7), fr.KERNELS['K44']
    fir = conv_composition(x, k, (1, 1), (1, 1), (1, 2, 2, 1))
    noise, bias, addend, mask = R(2, 1, 6, 7), R(3), R(2, 3, 6, 7), R(2, 3, 6, 7)
    nw, slope, gain, mv = sr.f32(0.3), sr.f32(0.2), sr.f32(1.5), (sr.f32(2.0), sr.f32(0.25))
    mf = torch.where(mask > 0, mv[0], mv[1])
    pre = fir + noise * nw + bias[None, :, None, None]
    acts = {fr.ACT_NONE: lambda v: v, fr.ACT_LRELU: lambda v: F.leaky_relu(v, slope), fr.ACT_RELU: torch.relu}
    for act, fn in acts.items():
        kw = dict(pad=(1, 2, 2, 1), noise=noise, noise_w=0.3, bias=bias, addend=addend, act=act, slope=0.2, gain=1.5, mask=mask, mask_vals=(2.0, 0.25))
        f32 = fn(pre + addend) * (gain if act == fr.ACT_LRELU else 1.0) * mf
        h8 = fn(pre) * gain * mf + addend
        assert torch.allclose(fr.upfirdn2d(x, k, family='f32', **kw)['y'][0], f32, rtol=0, atol=1e-12), act
        assert torch.allclose(fr.upfirdn2d(x, k, family='h8', **kw)['y'][0], h8, rtol=0, atol=1e-12), act
    m = fr.upfirdn2d(x, k, family='h8', **kw)['y']
    assert bool((m[1] + 1e-12 >= m[0].abs()).all())
    # h8: x, mask and addend are what the 16-bit maps hold, nothing else is rounded
    r = sr.rnd_for('bf16')
    a = fr.upfirdn2d(x, k, family='h8', rnd=r, **kw)['y'][0]
    b = fr.upfirdn2d(r(x.float()), k, family='h8', **dict(kw, mask=r(mask.float()), addend=r(addend.float())))['y'][0]
    assert torch.equal(a, b) and not torch.equal(a, fr.upfirdn2d(x, k, family='h8', **kw)['y'][0])


def test_fused_bias_act_and_weight_plane_models_against_inline_torch():
    x, b, ref = torch.randn(3, 5, 4), torch.randn(5), torch.randn(3, 5, 4)
    v = x + b[None, :, None]
    al, sc = torch.tensor(np.float32(0.2)), torch.tensor(np.float32(2 ** 0.5))
    want = {(1, 0): v * sc, (1, 1): v * sc, (1, 2): torch.zeros_like(v), (3, 0): torch.where(v > 0, v, v * al) * sc, (3, 1): torch.where(ref > 0, v, v * al) * sc,
            (3, 2): torch.zeros_like(v), (2, 0): v * sc}
    assert set(want) == set(fr.FBA_CODES)
    for (act, grad), w in want.items():
        assert torch.equal(fr.fused_bias_act(x, b, ref, 4, 5, act, grad, 0.2, 2 ** 0.5)['y'][0].view(3, 5, 4), w), (act, grad)
    assert torch.equal(fr.fused_bias_act(x, None, None, 4, 5, 3, 0, 0.2, 1.0)['y'][0].view(3, 5, 4), torch.where(x > 0, x, x * al))
    w32, s = torch.randn(2, 3, 2, 4, 8), torch.rand(2, 32) + 0.5
    for elem, dtype in sr.ELEM_DTYPES.items():
        got = fr.modulate_planes(w32, s, elem)['planes'][0]
        assert got.dtype == dtype and got.shape == (2, 2, 3, 2, 4, 8)
        for b_, c16, t, half, co, e in ((0, 0, 0, 0, 0, 0), (1, 1, 2, 1, 3, 7), (1, 0, 1, 1, 2, 5)):
            assert float(got[b_, c16, t, half, co, e]) == float((w32[c16, t, half, co, e] * s[b_, 16 * c16 + 8 * half + e]).to(dtype))


# ---- the table against its mistakes ---------------------------------------------------------------------------------------------------------------
def _moved(row, mistake, elem):
    kw = fr.make_inputs(row, elem)
    good, bad = fr.expected(row, kw, elem), fr.expected(row, kw, elem, _mistake=mistake)
    moved = 0.0
    for name, (want, bound) in good.items():
        if bound is None:
            moved = max(moved, 0.0 if torch.equal(want, bad[name][0]) else float('inf'))
        else:
            moved = max(moved, sr.worst(bad[name][0], want, bound)[2])
    return moved


FAMILY_OF = {'addend_after_act': ('f32',), 'addend_before_mask': ('h8',)}


@pytest.mark.parametrize('mistake', fr.MISTAKES)
def test_every_named_mistake_moves_a_row_by_ten_bounds(mistake):
    """Made in the model, the mistake moves at least one row of each family it can be made in by more than 10x that row's bound (exact: at all)."""
    op = 'fba' if mistake.startswith('fba') else 'planes' if mistake.startswith('planes') else 'fir'
    kinds = FAMILY_OF.get(mistake, ('f32',) if op == 'fba' else ('h8',) if op == 'planes' else ('f32', 'h8'))
    for kind in kinds:
        hit = None
        for r in ROWS:
            if r.op.split('_')[0] != op or r.kind != kind or r.extra.get('twin'):
                continue
            if all(_moved(r, mistake, e) > 10 for e in ELEMS(r)):
                hit = r
                break
        assert hit is not None, (mistake, kind)


def test_a_symmetric_fir_cannot_show_unflipped_or_transposed_taps():
    """Why no row uses [1,3,3,1] x [1,3,3,1]: with it the two tap mistakes change nothing, so the whole earlier suite passed a kernel that made them."""
    x = torch.randn(2, 2, 9, 12, generator=torch.Generator().manual_seed(3))
    for taps, k in ((None, fr.KERNELS['SYM44']), (fr.TAPS['SYM44'], None)):
        for pad in ((1, 2, 2, 1), (2, 1, 1, 2)):
            good = fr.upfirdn2d(x, k, pad=pad, taps=taps)['y'][0]
            for m in ('taps_not_flipped', 'taps_transposed'):
                assert torch.equal(good, fr.upfirdn2d(x, k, pad=pad, taps=taps, _mistake=m)['y'][0]), m
    good = fr.upfirdn2d(x, fr.KERNELS['K44'], pad=(1, 2, 2, 1))['y'][0]
    for m in ('taps_not_flipped', 'taps_transposed'):
        assert float((good - fr.upfirdn2d(x, fr.KERNELS['K44'], pad=(1, 2, 2, 1), _mistake=m)['y'][0]).abs().max()) > 0.1, m


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ROWS, ids=lambda r: r.id)
def test_fp32_evaluations_stay_inside_every_bound_in_two_orders(row):
    """A correct kernel cannot fail the row: the same formula in float32 with the taps in (ky, kx) order, multiply and add rounded apart, and in
    the separable order (horizontal, then vertical; a FIR without 1-D taps: column by column) with fused multiply-add, is inside the bound
    (16-bit outputs: after rounding to the element type)."""
    for elem in ELEMS(row):
        kw = fr.make_inputs(row, elem)
        exp = fr.expected(row, kw, elem)
        if row.op != 'fir':
            assert all(bound is None for _, bound in exp.values())
            continue
        if row.kind == 'h8' and 'taps' not in kw and fr.KERNELS[row.extra['k']].shape == (4, 4) and row.extra['k'] in fr.TAPS:
            kw = dict(kw, taps=fr.TAPS[row.extra['k']])          # the separable order exists for this FIR: evaluate it even where the row withholds the taps
        for order in ('kykx', 'fma'):
            want, bound = exp['y']
            g = fr.expected(row, kw, elem, dt=torch.float32, order=order)['y'][0]
            if row.kind == 'h8':
                g = g.to(sr.ELEM_DTYPES[elem])
            err, bnd, ratio = sr.worst(g, want, bound)
            _LOG.append('%s %s y %s err %.3e bound %.3e ratio %.3f' % (row.id, elem, order, err, bnd, ratio))
            assert ratio <= 1.0, (row.id, elem, order, err, bnd)


@pytest.mark.parametrize('row', FIR_ROWS, ids=lambda r: r.id)
def test_no_row_checks_zeros_against_zero(row):
    """M is positive wherever a tap or an operand reaches; the outputs nothing reaches (a far pad wider than the FIR, a 1x1 FIR between inserted
    zeros) are few, and there the contract is an exact zero."""
    kw = fr.make_inputs(row, ELEMS(row)[0])
    ts = [(k, v) for k, v in kw.items() if torch.is_tensor(v) and v.numel() > 16 and k != 'k']
    for i, (ka, a) in enumerate(ts):
        for kb, b in ts[i + 1:]:
            assert a.shape != b.shape or not torch.equal(a, b), (row.id, ka, kb)
    want, M = fr.upfirdn2d(family=row.kind, **{k: v for k, v in kw.items() if not k.startswith('_')})['y']
    dead = M == 0
    unreachable = fr.upfirdn2d(torch.ones_like(kw['x']), torch.ones_like(kw['k']), kw['up'], kw['down'], kw['pad'])['y'][0] == 0
    assert float(want.abs().max()) > 0 and bool((want[dead] == 0).all())
    if not any(o in row.extra['ops'] for o in ('noise', 'bias', 'addend')):
        assert torch.equal(dead, unreachable), row.id
    limit = 0.8 if (row.extra['k'] == 'K11' and row.extra['up'] != (1, 1)) else 0.25
    assert float(dead.float().mean()) < limit, (row.id, float(dead.float().mean()))


# ---- the rows against the launch code and the sources -----------------------------------------------------------------------------------------------
def test_rows_enter_the_paths_they_name_and_every_path_has_rows():
    for r in ROWS:
        assert fr.row_path(r) == r.path, r.id
    paths = {r.path for r in ROWS}
    assert paths == {'upfirdn2d_k4_stream_kernel<1>', 'upfirdn2d_k4_stream_kernel<2>', 'upfirdn2d_k4_kernel', 'upfirdn2d_k4_down2_stream_kernel', 'upfirdn2d_up2k4_kernel',
                     'upfirdn2d_kernel', 'upfirdn2d_h8_sep4_kernel', 'upfirdn2d_h8_sep4_kernel<MBITS>', 'upfirdn2d_h8_sep4_down2_kernel', 'upfirdn2d_h8_sep4_up2_kernel',
                     'upfirdn2d_h8_kernel', 'fba_kernel<true>', 'fba_kernel<false>', 'modulate_planes_kernel', 'modulate_planes_multi_kernel'}
    ow = lambda p: sorted({fr.geom(r)['ow'] for r in FIR_ROWS if r.path.startswith(p)})
    oh = lambda p: sorted({fr.geom(r)['oh'] for r in FIR_ROWS if r.path.startswith(p)})
    # the smallest widths at which a second strip or chunk starts, and the heights at which a second wave and a second band start
    assert {192, 256, 260} <= set(ow('upfirdn2d_k4_stream')) and {15, 17, 65} <= set(oh('upfirdn2d_k4_stream'))
    assert {96, 128, 130} <= set(ow('upfirdn2d_k4_down2')) and {8, 9, 33} <= set(oh('upfirdn2d_k4_down2'))
    assert {60, 61, 62, 123} <= set(ow('upfirdn2d_h8_sep4_kernel')) and {16, 17, 33} <= set(oh('upfirdn2d_h8_sep4_kernel'))
    assert {61, 62, 63} <= set(ow('upfirdn2d_h8_sep4_down2')) and {8, 9} <= set(oh('upfirdn2d_h8_sep4_down2'))
    assert {61, 62, 63} <= {r.shape[3] for r in FIR_ROWS if r.path == 'upfirdn2d_h8_sep4_up2_kernel'}
    for r in FIR_ROWS:                                     # x and y are never padded alike: a kernel that reads one pad for the other shows
        if r.path.split('<')[0] in ('upfirdn2d_k4_stream_kernel', 'upfirdn2d_k4_kernel', 'upfirdn2d_h8_sep4_kernel'):
            assert r.extra['pad'][0] != r.extra['pad'][2], r.id


def test_every_dispatch_predicate_is_false_alone_in_one_twin_row():
    twins = {}
    for r in ROWS:
        if r.extra.get('pred'):
            of = r.extra.get('pred_of') or ('fba_kernel<true>' if r.op == 'fba' else fr.row_by_id(r.extra['twin']).path.split('<')[0])
            twins.setdefault(of, []).append(r.extra['pred'])
            assert r.path.split('<')[0] != of.split('<')[0] or r.op == 'fba', r.id          # it left the fast path
    assert set(twins) == set(fr.PREDICATES)
    for of, preds in fr.PREDICATES.items():
        assert sorted(twins[of]) == sorted(preds) and len(preds) == len(set(preds)), of
    assert sum(len(v) for v in twins.values()) == sum(len(v) for v in fr.PREDICATES.values())
    # false ALONE: restoring the one clause puts the launch back on the fast path (the alignment twins: drop the offset)
    for r in ROWS:
        if r.extra.get('pred', '').endswith('_off'):
            e = dict(r.extra, off=None)
            fast = fr.path_fba(r.shape[3], e['step_b'], True) if r.op == 'fba' else fr.path_f32(r.shape[2], r.shape[3], 4, 4, e['up'], e['down'], e['pad'], e['ops'])
            assert fast != r.path, r.id


def test_every_refusal_line_of_the_five_launchers_has_its_cases():
    found = set()
    for fname, funcs in fr.LAUNCHERS.items():
        with open(os.path.join(ROOT, 'latent2im_amd', 'csrc', fname)) as fh:
            text = fh.read()
        for fn in funcs:
            at = [m.start() for m in re.finditer(re.escape(fn) + r'\(', text)][-1]          # the definition (after a forward declaration)
            body = text[at:]
            body = body[:body.index('\n}\n')]
            msgs = re.findall(r'l2i_set_error\(\s*L2I_E_\w+,\s*"([^"]*)"', body)
            assert msgs, fn
            found |= set(msgs)
    for key, cases in fr.REFUSALS.items():
        assert sum(m.startswith(key) for m in found) == 1 and cases, key
    assert len(found) == len(fr.REFUSALS), sorted(found)


def test_every_streaming_kernel_is_claimed_by_exactly_one_table():
    found = set()
    for f in ('l2i_stream.hip', 'l2i_stream_h8.hip'):
        with open(os.path.join(ROOT, 'latent2im_amd', 'csrc', f)) as fh:
            found |= set(re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(', fh.read()))
    mine = {k.split('<')[0] for r in ROWS for k in r.path.split()}
    assert mine == set(fr.CLAIMED_KERNELS) and not sr.OUT_OF_SCOPE_KERNELS
    assert mine | set(sr.CLAIMED_KERNELS) == found and not (mine & set(sr.CLAIMED_KERNELS))


def test_the_header_states_both_epilogue_orders():
    with open(os.path.join(ROOT, 'include', 'l2i.h')) as f:
        text = f.read()
    assert 'act_gain is applied under L2I_ACT_LRELU ONLY' in text and 'addend is INSIDE the activation' in text
    assert 'act_gain under EVERY act' in text and 'addend is NOT inside the activation' in text and 'major need not be a multiple of channels' in text
