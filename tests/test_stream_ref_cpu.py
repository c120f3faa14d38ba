"""The float64 model of the streaming kernels (tests/stream_ref.py) against independently written torch compositions and autograd; the case
table against the mistakes it claims to catch; every row's bound against an fp32 evaluation of the same formula in two summation orders; and
the kernels of the two source files against the rows that claim them."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import stream_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = sr.all_rows()
ELEMS = lambda row: ('f32',) if row.kind == 'f32' else ('bf16', 'f16')
_LOG = []


@pytest.fixture(scope='module', autouse=True)
def _error_log():
    """L2I_STREAM_CONTRACT_ERRORS=<file>: the error of the fp32 evaluation of every row beside its bound (profiles/stream_contract_errors.txt)."""
    yield
    path = os.environ.get('L2I_STREAM_CONTRACT_ERRORS')
    if path:
        with open(path, 'w') as f:
            f.write('# row element output order: largest |fp32 evaluation - float64 model| over the bound at that element (tests/test_stream_ref_cpu.py)\n' + '\n'.join(_LOG) + '\n')


def test_activation_backward_and_its_three_sums_are_autograd_of_the_plain_composition():
    kw = sr.sg2_inputs(3, sr.SG2_ALL, 2, 5, 6, 7)
    D = lambda t: t.double()
    gain, slope, nw = sr.f32(kw['gain']), sr.f32(kw['slope']), sr.f32(kw['noise_w'])
    z0 = D(sr.T(torch.randn(2, 5, 6, 7, generator=torch.Generator().manual_seed(1)).numpy()))
    t = torch.ones(2, 5, dtype=torch.float64, requires_grad=True)                         # a unit scale on z: d L / d t = sum_p dz z
    s = D(kw['gin_scale']).clone().requires_grad_(True)                                   # the next layer's style: its input is y s
    wm = D(kw['wmod_rgb']).clone().requires_grad_(True)
    zact = (t[:, :, None, None] * z0 + D(kw['noise']) * nw + D(kw['bias'])[None, :, None, None]).requires_grad_(True)
    y = F.leaky_relu(zact, slope) * gain
    loss = (D(kw['gin']) * (y * s[:, :, None, None])).sum() + (D(kw['grgb']) * torch.einsum('bchw,boc->bohw', y, wm)).sum()
    g_z, g_s, g_wm = torch.autograd.grad(loss, (zact, s, wm))
    # the model sees y rounded to float32: z recovered from it carries 2^-24 of |y|
    yd = y.detach().float().double()
    m = sr.sg2_act_bwd(**dict(kw, y=yd))
    assert torch.allclose(m['dz'][0], g_z, rtol=0, atol=1e-12)
    assert torch.allclose(m['red_dz_z'][0], (g_z * z0).sum((2, 3)), rtol=0, atol=1e-5)      # z0 = zpre up to the float32 rounding of y
    assert torch.allclose(m['red_x_grgb'][0], g_wm.permute(0, 2, 1), rtol=0, atol=1e-5)
    assert torch.allclose(m['red_gin_y'][0], g_s, rtol=0, atol=1e-5)
    assert float(m['dz'][1].min()) >= 0 and bool((m['dz'][1] + 1e-12 >= m['dz'][0].abs()).all())


def test_both_zeros_and_values_that_round_to_zero_take_the_negative_side():
    y = torch.tensor([-0.0, 0.0, sr.TINY, -sr.TINY, sr.DENORM, -sr.DENORM, 1.0, -1.0]).reshape(1, 8, 1, 1)
    g = torch.ones(1, 8, 1, 1)
    for elem, pos in (('f32', [0, 0, 1, 0, 1, 0, 1, 0]), ('bf16', [0, 0, 1, 0, 0, 0, 1, 0]), ('f16', [0, 0, 0, 0, 0, 0, 1, 0])):
        dz = sr.sg2_act_bwd(y, gin=g, slope=0.25, gain=2.0, rnd=sr.rnd_for(elem))['dz'][0].reshape(-1)
        assert dz.tolist() == [2.0 if p else 0.5 for p in pos], elem
        mm = sr.mask_mul(g, y, 3.0, 5.0, rnd=sr.rnd_for(elem))['y'][0].reshape(-1)
        assert mm.tolist() == [3.0 if p else 5.0 for p in pos], elem
    t = sr.plant_signs(torch.ones(16), h8=True)
    assert torch.signbit(t[0]) and not torch.signbit(t[1]) and float(t[0]) == 0.0 and float(t[2]) == sr.TINY and float(t[-1]) == float(torch.tensor(-sr.DENORM))


def test_torgb_dot_sqdiff_axpby_against_inline_torch():
    rs = torch.Generator().manual_seed(5)
    R = lambda *s: torch.randn(*s, generator=rs)
    x, wm, bias, y2 = R(2, 5, 4, 6), R(2, 3, 5), R(3), R(2, 5, 4, 6)
    want = sum(x.double()[:, c:c + 1] * wm.double()[:, :, c, None, None] for c in range(5)) + bias.double()[None, :, None, None]
    assert torch.allclose(sr.torgb_fwd(x, wm, bias)['rgb'][0], want, rtol=0, atol=1e-12)
    assert torch.allclose(sr.torgb_fwd(x, wm)['rgb'][0], want - bias.double()[None, :, None, None], rtol=0, atol=1e-12)
    assert torch.allclose(sr.dot_reduce(x, y2)['out'][0], (x.double() * y2.double()).flatten(2).sum(-1), rtol=0, atol=1e-12)
    assert torch.allclose(sr.dot_reduce(x, chunked=True)['out'][0], x.double().sum((2, 3)), rtol=0, atol=1e-12)
    b = y2.double().clone().requires_grad_(True)
    cd = torch.full((1,), 1.75)
    g, = torch.autograd.grad(0.5 * sr.f32(0.3) * 1.75 * ((b - x.double()) ** 2).sum(), b)
    m = sr.sqdiff(x, y2, 0.3, cd)
    assert torch.allclose(m['grad'][0], g, rtol=0, atol=1e-12) and abs(float(m['sum'][0]) - float(((x.double() - y2.double()) ** 2).sum())) < 1e-9
    assert torch.allclose(sr.sqdiff(x, y2, 0.3)['grad'][0] * 1.75, g, rtol=0, atol=1e-12)          # NULL coef_dev reads as 1
    assert torch.allclose(sr.axpby(x, y2, 0.5, -2.25)['y'][0], 0.5 * x.double() - 2.25 * y2.double(), rtol=0, atol=1e-12)
    assert torch.equal(sr.axpby(x, None, 0.5)['y'][0], 0.5 * x.double())
    assert torch.equal(sr.relu_mask(x, y2)['y'][0], x.double() * (y2 > 0))


@pytest.mark.parametrize('k,s,pad,h,w', [(2, 2, 0, 6, 8), (3, 2, 1, 7, 9), (3, 2, 1, 8, 12), (3, 1, 1, 5, 6), (2, 1, 0, 5, 6), (3, 3, 0, 7, 10)])
def test_maxpool_model_is_aten(k, s, pad, h, w):
    import numpy as np
    x = sr.pool_input(np.random.RandomState(k * 100 + h), (2, 3, h, w), k, s, pad, nan=False)
    xr = x.double().requires_grad_(True)
    ref, flat = F.max_pool2d(xr, k, s, pad, return_indices=True)
    m = sr.maxpool_fwd(x, k, s, pad)
    assert torch.equal(m['y'][0], ref.detach())
    OH, OW = ref.shape[2:]
    oy, ox = torch.arange(OH)[:, None], torch.arange(OW)[None, :]
    local = (flat // w - (oy * s - pad)) * k + (flat % w - (ox * s - pad))
    assert torch.equal(m['idx'][0].long(), local)                                           # first maximum in row-major order, ties included
    gy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2))
    gref, = torch.autograd.grad(ref, xr, gy.double())
    assert torch.allclose(sr.maxpool_bwd(gy, m['idx'][0], (h, w), k, s, pad)['gx'][0], gref, rtol=0, atol=1e-12)
    a, b = torch.randn(2, 3, h, w), torch.randn(2, 3, h, w)
    got = sr.maxpool_bwd(gy, m['idx'][0], (h, w), k, s, pad, a=a, b=b, coef=0.5, coef_dev=torch.full((1,), 3.0))['gx'][0]
    assert torch.allclose(got, gref + 1.5 * (b.double() - a.double()), rtol=0, atol=1e-12)
    assert torch.equal(sr.maxpool_fwd(x, k, s, pad, relu=True)['y'][0], torch.relu(ref.detach()))
    # a NaN is the result of every window that holds it, and of no other
    xn = x.clone()
    xn[1, 2, h // 2, w // 2] = float('nan')
    yn = sr.maxpool_fwd(xn, k, s, pad, relu=True)['y'][0]
    refn = F.max_pool2d(xn.double(), k, s, pad)
    assert torch.equal(torch.isnan(yn), torch.isnan(refn)) and bool(torch.isnan(yn).any())


def test_layout_zero_insert_and_sign_plane():
    x = torch.randn(2, 3, 4, 5, generator=torch.Generator().manual_seed(3))
    for dtype in sr.ELEM_DTYPES.values():
        t = sr.to_h8(x, 16, dtype)
        assert t.shape == (2, 2, 4, 5, 8) and t.dtype == dtype and torch.equal(t[0, 0, 1, 2, :3].float(), x[0, :, 1, 2].to(dtype).float())
        assert float(t[:, 0, :, :, 3:].abs().max()) == 0 and float(t[:, 1].abs().max()) == 0
        assert torch.equal(sr.from_h8(t, 3), x.to(dtype).float())
    y, c, mk = torch.randn(1, 8, 5, 7), torch.randn(1, 8, 3, 4), torch.randn(1, 8, 5, 7)
    want = y.double().clone()
    for oy in range(3):
        for ox in range(4):
            want[0, :, 2 * oy, 2 * ox] += torch.where(mk[0, :, 2 * oy, 2 * ox] > 0, c[0, :, oy, ox].double(), torch.zeros(8, dtype=torch.float64))
    assert torch.equal(sr.add_zero_insert(y, c, mk)['y'][0], want)
    plane = sr.sign_plane(sr.to_h8(mk, 8, torch.bfloat16))
    assert plane.shape == (1, 1, 5, 7) and int(plane[0, 0, 2, 3]) == sum(1 << e for e in range(8) if float(mk[0, e, 2, 3]) > 0)


# ---- the table against its mistakes ---------------------------------------------------------------------------------------------------------------
def _mistake_rows():
    out = []
    for r in ROWS:
        if r.geom not in ('base', 'operands') and r.op != 'pool':
            continue
        ms = {'sg2': lambda: sr.SG2_CASES[r.case][1], 'sqdiff': lambda: sr.SQDIFF_CASES[r.case][1],
              'pool': lambda: tuple(m for m, c in sr.POOL_MISTAKE_ROWS.items() if c == r.case and r.kind == 'h8')}.get(r.op, lambda: ())()
        out += [(r, m, e) for m in ms for e in ELEMS(r)]
    return out


@pytest.mark.parametrize('row,mistake,elem', _mistake_rows(), ids=lambda v: str(v))
def test_each_case_sees_the_mistake_it_is_aimed_at(row, mistake, elem):
    """The mistake, made in the model, moves an output by more than 10x the row's own bound (an exact output: at all)."""
    kw = sr.make_inputs(row, elem)
    good, bad = sr.expected(row, kw, elem), sr.expected(row, kw, elem, _mistake=mistake)
    moved = 0.0
    for name, (want, bound) in good.items():
        if bound is None:
            moved = max(moved, float('inf') if not torch.equal(want, bad[name][0]) else 0.0)
        else:
            moved = max(moved, sr.worst(bad[name][0], want, bound)[2])
    assert moved > 10, (row.id, mistake, moved)


def test_every_mistake_has_a_case():
    assert {m for _, m, _ in _mistake_rows()} == set(sr.MISTAKES)
    for name, (fields, _) in sr.SG2_CASES.items():
        assert all(f in sr.SG2_ALL for f in fields) and ('gin' in fields or 'rgb' in fields), name
    for f in ('gin_scale', 'rgb', 'bias', 'noise', 'red_dz_z', 'red_x_grgb', 'red_gin_y', 'gin'):
        assert 'no_' + f in sr.SG2_CASES and f not in sr.SG2_CASES['no_' + f][0]


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ROWS, ids=lambda r: r.id)
def test_fp32_evaluation_stays_inside_every_bound_in_two_summation_orders(row):
    """A correct fp32 kernel cannot fail the row: the same formula in float32, summed flat and per 256-element block, is inside the bound
    (16-bit outputs: after rounding to the element type)."""
    for elem in ELEMS(row):
        kw = sr.make_inputs(row, elem)
        exp = sr.expected(row, kw, elem)
        for chunked in (False, True):
            got = sr.expected(row, kw, elem, dt=torch.float32, chunked=chunked)
            for name, (want, bound) in exp.items():
                g = got[name][0]
                if bound is None:
                    assert torch.equal(g.to(want.dtype), want) or (torch.equal(torch.isnan(g), torch.isnan(want)) and torch.equal(torch.nan_to_num(g.to(want.dtype)), torch.nan_to_num(want))), (row.id, name)
                    continue
                if row.kind == 'h8' and name in ('dz', 'grad', 'y', 'gx'):
                    g = g.to(sr.ELEM_DTYPES[elem])
                err, bnd, ratio = sr.worst(g, want, bound)
                _LOG.append('%s %s %s %s err %.3e bound %.3e ratio %.3f' % (row.id, elem, name, 'blocks_of_256' if chunked else 'flat', err, bnd, ratio))
                assert ratio <= 1.0, (row.id, elem, name, chunked, err, bnd)
            if row.op not in ('sg2', 'dot', 'sqdiff'):
                break


@pytest.mark.parametrize('row', ROWS, ids=lambda r: r.id)
def test_no_row_checks_zeros_against_zero(row):
    """The tensor operands of a row differ from one another, and no sum it checks has magnitude M = 0: a row whose operands coincide (a = b in
    sqdiff) would hold a kernel that drops elements to 0 <= 0."""
    kw = sr.make_inputs(row, ELEMS(row)[0])
    ts = [(k, v) for k, v in kw.items() if torch.is_tensor(v) and v.numel() > 1]
    for i, (ka, a) in enumerate(ts):
        for kb, b in ts[i + 1:]:
            assert a.shape != b.shape or not torch.equal(a, b), (row.id, ka, kb)
    for elem in ELEMS(row):
        for name, (want, bound) in sr.expected(row, kw, elem).items():
            if name in ('red_dz_z', 'red_x_grgb', 'red_gin_y', 'out', 'sum') and bound is not None:
                assert float(torch.as_tensor(bound).min()) > 0 and float(want.abs().max()) > 0, (row.id, elem, name)


# ---- the rows against the launch code and the sources -----------------------------------------------------------------------------------------------
def test_geometry_rows_enter_the_paths_they_name():
    g = {gid: sr.torgb_geom_f32(B, H * W) for gid, B, C, H, W in sr.TORGB_F32_GEOMS}
    assert g['capped_second_pass'] == dict(bpb=1, capped=True, passes=2) and not g['c8_hw4_300']['capped'] and g['c8_hw4_300']['bpb'] == 2
    assert sr.torgb_geom_f32(2047, 4 * 257)['passes'] == 1                                 # one sample fewer: not capped
    assert all(H * W // 4 < 64 or (H * W // 4) % 256 for _, _, _, H, W in sr.TORGB_F32_GEOMS) and {C for _, _, C, _, _ in sr.TORGB_F32_GEOMS} == {1, 5, 8, 13, 24}
    s = {gid: sr.rows_geom_f32(B * C, H * W) for gid, B, C, H, W in sr.SG2_F32_GEOMS}
    assert s['hw16_one_wave'] == dict(chunks=1, capped=False, n_lane=4) and s['hw5184_two_chunks_ragged'] == dict(chunks=2, capped=False, n_lane=12)
    assert 1296 % 512 != 0 and s['capped_chunks']['capped'] and s['capped_chunks']['chunks'] == 1
    assert not sr.rows_geom_f32(4095, 4100)['capped'] and not sr.rows_geom_f32(4096, 4096)['capped']          # the smallest capped (rows, HW)
    h = {gid: sr.h8_red_geom(B * C // 8, H * W) for gid, B, C, H, W in sr.H8_RED_GEOMS}
    assert [h[k]['strips'] for k in ('hw400_one_strip', 'hw2304_two_strips', 'hw4100_three_strips')] == [1, 2, 3]
    assert {C for _, _, C, _, _ in sr.H8_RED_GEOMS} == {8, 40}
    _, B, C, H, W = sr.H8_DOT_FORCED
    assert sr.h8_red_geom(B * C // 8, H * W)['forced_one'] and sr.h8_strips(4095, H * W) == 2
    t = {gid: sr.torgb_geom_h8(H * W) for gid, _, _, H, W in sr.TORGB_H8_GEOMS}
    assert t['bps_capped_second_pass'] == dict(bps=512, passes=2) and t['g4'] == dict(bps=2, passes=1)
    assert [C // 8 for _, _, C, _, _ in sr.TORGB_H8_GEOMS[:5]] == [1, 3, 4, 5, 9]
    for name, per_block, cap in (('sqdiff_f32', 2048, 2048), ('axpby_f32', 1024, 2048), ('relu_mask_f32', 1024, 2048), ('sqdiff_h8', 256, 2048),
                                 ('mask_mul_h8', 256, 4096), ('mask_mul_bits_h8', 256, 4096)):
        ns = sr.ELEMWISE_N[name]
        assert ns[0] == 1 and ns[1] == 255 and sr.grid_for(ns[-1], per_block, cap) == cap and sr.grid_for(ns[-1] - 1, per_block, cap) == cap
        assert ns[-1] - 1 == per_block * cap and any(sr.grid_for(n, per_block, cap) == 2 and sr.grid_for(n - 1, per_block, cap) == 1 for n in ns)
    for gid, k, s, pad, H, W, aligned, fk, bk in sr.POOL_F32_GEOMS:
        assert H != W and sr.pool_fwd_kernel_f32(H, W, k, s, pad, aligned) == fk and sr.pool_bwd_kernel_f32(H, W, k, s, pad, aligned) == bk, gid
    kernels = {k for row in sr.POOL_F32_GEOMS for k in row[7:9]}
    assert kernels == {'maxpool_fwd_kernel', 'maxpool_fwd_vec_kernel<2>', 'maxpool_fwd_vec_kernel<3>', 'maxpool_bwd_k2s2_kernel',
                       'maxpool_bwd_k3s2p1_vec_kernel', 'maxpool_bwd_kernel<3,2,1>', 'maxpool_bwd_kernel<0,0,0>'}
    assert {(k, s, p) for _, k, s, p, *_ in sr.POOL_F32_GEOMS if (k, s, p) not in ((2, 2, 0), (3, 2, 1))} == {(3, 1, 1), (2, 1, 0), (3, 3, 0)}
    assert any(H % 2 and W % 4 == 0 and fk.endswith('<3>') and 'vec' in bk for _, k, s, p, H, W, al, fk, bk in sr.POOL_F32_GEOMS)


def test_every_streaming_kernel_is_claimed_by_a_row_or_out_of_scope_by_name():
    found = set()
    for f in ('l2i_stream.hip', 'l2i_stream_h8.hip'):
        with open(os.path.join(ROOT, 'latent2im_amd', 'csrc', f)) as fh:
            found |= set(re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(', fh.read()))
    assert len(found) > 30
    from tests import fir_ref
    claimed = {k.split('<')[0] for r in ROWS for k in r.path.split()}
    others = set(fir_ref.CLAIMED_KERNELS) | set(sr.OUT_OF_SCOPE_KERNELS)          # the second claim table (tests/fir_ref.py) and the kernels out of scope by name
    assert not (found - claimed - others), 'kernels no row claims: %s' % sorted(found - claimed - others)
    assert not (claimed - found) and not (set(sr.OUT_OF_SCOPE_KERNELS) - found) and not (claimed & set(sr.OUT_OF_SCOPE_KERNELS))
    assert claimed == set(sr.CLAIMED_KERNELS) and all(hasattr(sr, t) for t in sr.CLAIMED_KERNELS.values())
    assert claimed | set(fir_ref.CLAIMED_KERNELS) == found and not (claimed & set(fir_ref.CLAIMED_KERNELS))
