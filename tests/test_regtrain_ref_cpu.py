"""The model of tests/regtrain_ref.py against the torch packing code it restates (latent2im_amd/conv.py) and CustomDataset's numpy expression —
no GPU.  The GPU tests then hold the kernels to the model."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from latent2im_amd import conv as C
from tests import regtrain_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weight(cout, cin, k, seed):
    return np.random.RandomState(seed).randn(cout, cin, k, k).astype(np.float32)


def _packs(w, k, stride, pad):
    """[(name, torch pack, taps, swap, pad_to)] of every gather pack FrozenConv2d derives from w, built with conv.py's own code on the host."""
    wt = torch.as_tensor(w).transpose(0, 1).contiguous()
    out = [('forward', C.pack_weight(torch.as_tensor(w)), rr.taps_forward(k), False, 32)]
    if stride == 1:
        out.append(('grad s1', C.correlation_plan(torch.flip(wt, [2, 3]), 1, k - 1 - pad)[0].w, rr.taps_grad_s1(k), True, 32))
        return out
    plan = C.transposed_plan(wt, pad)
    for L, (py, px) in zip(plan, ((0, 0), (0, 1), (1, 0), (1, 1))):
        taps = rr.taps_parity(k, pad, py, px)
        assert (L is None) == (taps is None)
        if L is not None:
            out.append(('parity %d%d' % (py, px), L.w, taps, True, 32))
            if L.w4 is not None:
                out.append(('parity %d%d w4' % (py, px), L.w4, taps, True, 4))
    if (k, pad) in C.FUSED_TRANSPOSED_SHAPES and w.shape[1] > 4 and w.shape[0] % 4 == 0:
        out.append(('fused', C.FusedTransposed(wt, pad).w, C.fused_transposed_taps(k, pad), True, 32))
    if (k, pad) == (7, 3) and w.shape[1] <= 3:
        out.append(('small', C.SmallTransposed(wt, pad).w, rr.taps_forward(k), True, 4))
    return out


@pytest.mark.parametrize('kind', rr.KINDS, ids=[k[0] for k in rr.KINDS])
def test_gather_reproduces_every_pack_bit_for_bit(kind):
    _, cout, cin, k, stride, pad = kind
    w = _weight(cout, cin, k, 11)
    packs = _packs(w, k, stride, pad)
    names = [p[0] for p in packs]
    assert 'forward' in names and (stride == 1) == ('grad s1' in names)
    if kind[0] == '3x3 s2 p1 16->32':
        assert 'fused' in names and sum(n.startswith('parity') for n in names) == 4
    if kind[0] == '7x7 s2 p3 3->64':
        assert 'small' in names and any(n.endswith('w4') for n in names)
    if kind[0] == '1x1 s2 16->64':
        assert [n for n in names if n.startswith('parity')] == ['parity 00']          # the other three parities receive nothing
    for name, pack, taps, swap, pad_to in packs:
        assert len(taps) <= rr.MAX_TAPS
        got = rr.gather(w, taps, swap, pad_to)
        want = pack.numpy().reshape(got.shape)
        assert got.tobytes() == want.tobytes(), (kind[0], name)


def test_gather_oihw_is_the_kept_plain_weight():
    """A gradient launch keeps its own [cout', cin', kh, kw] weight (Launch.w_src, FusedTransposed.w_src): same taps, rows = the pack's columns."""
    w = _weight(16, 16, 3, 12)
    wt = torch.as_tensor(w).transpose(0, 1).contiguous()
    L = C.correlation_plan(torch.flip(wt, [2, 3]), 1, 1)[0]
    assert rr.gather(w, rr.taps_grad_s1(3), False, oihw=True).tobytes() == L.w_src.contiguous().numpy().tobytes()
    w = _weight(32, 16, 3, 13)
    wt = torch.as_tensor(w).transpose(0, 1).contiguous()
    for L, (py, px) in zip(C.transposed_plan(wt, 1), ((0, 0), (0, 1), (1, 0), (1, 1))):
        assert rr.gather(w, rr.taps_parity(3, 1, py, px), False, oihw=True).tobytes() == L.w_src.contiguous().numpy().tobytes()
    assert rr.gather(w, rr.taps_forward(3), False, oihw=True).tobytes() == C.FusedTransposed(wt, 1).w_src.numpy().tobytes()


def test_mistake_table():
    """Each wrong gather is caught by the comparison above on at least the pack it concerns; the right one passes on all of them."""
    caught = {}
    for kind in rr.KINDS:
        _, cout, cin, k, stride, pad = kind
        w = _weight(cout, cin, k, 11)
        for name, pack, taps, swap, pad_to in _packs(w, k, stride, pad):
            for m in (None,) + rr.MISTAKES:
                try:
                    got = rr.gather(w, taps, swap, pad_to, mistake=m)
                    same = got.shape == tuple(pack.reshape(got.shape).shape) and got.tobytes() == pack.numpy().reshape(got.shape).tobytes()
                except (ValueError, RuntimeError):                    # a swapped role with Cout != Cin: not even the shape
                    same = False
                caught.setdefault(m, []).append(((kind[0], name), not same))
    assert not any(c for _, c in caught[None])
    hit = {m: {key for key, c in caught[m] if c} for m in rr.MISTAKES}
    assert ('3x3 s1 16->16', 'grad s1') in hit['swapped role'] and ('3x3 s1 16->16', 'forward') in hit['swapped role']      # square: only the values tell
    assert ('3x3 s1 16->16', 'grad s1') in hit['missed flip'] and ('7x7 s2 p3 3->64', 'small') in hit['missed flip']
    assert {('3x3 s2 p1 16->32', 'parity %d%d' % p) for p in ((0, 0), (0, 1), (1, 0), (1, 1))} <= hit['wrong parity tap']
    assert ('3x3 s2 p1 16->32', 'fused') in hit['wrong parity tap']
    assert ('1x1 16->40', 'forward') in hit['unfilled padding'] and ('7x7 s2 p3 3->64', 'small') in hit['unfilled padding']


def test_unfilled_padding_needs_padding_columns():
    """(why the 1x1 16 -> 40 kind exists) 40 columns pad to 64; a pack whose column count is a multiple of 32 has nothing to fill."""
    w = _weight(32, 32, 1, 3)
    assert rr.gather(w, rr.taps_forward(1), False, mistake='unfilled padding').tobytes() == rr.gather(w, rr.taps_forward(1), False).tobytes()
    w = _weight(40, 16, 1, 3)
    assert np.isnan(rr.gather(w, rr.taps_forward(1), False, mistake='unfilled padding')[:, :, 40:]).all()


@pytest.mark.parametrize('ch', (64, 512))
def test_winograd_model_within_one_ulp_of_the_torch_packs(ch):
    w = _weight(ch, ch, 3, 20 + ch) * np.float32(0.05)
    for swap, flip in ((False, False), (True, True)):
        view = torch.as_tensor(rr.conv_view(w, swap, flip))
        d2 = rr.ulp_distance(rr.wino2_pack(w, swap, flip), C.pack_weight_wino(view).numpy())
        assert d2.max() == 0, 'F(2x2): every sum is exact or a single rounding in any order'
        d4 = rr.ulp_distance(rr.wino4_pack(w, swap, flip).reshape(-1), C.pack_weight_wino4(view).numpy().reshape(-1))
        print('F(4x4) %dx%d swap=%d: %.3f %% of entries differ from the einsum pack, largest distance %d ulp' % (ch, ch, swap, 100.0 * (d4 > 0).mean(), d4.max()))
        assert d4.max() <= 1


def test_winograd_model_corners_and_another_float64_route():
    """The corners of U are exact scalings of single taps, and any other float64 route to U (numpy's einsum here) stays within 1 ulp of the
    model's fixed order — which is why the order is stated: bit equality holds against the model only."""
    w = _weight(64, 64, 3, 7)
    g = w.astype(np.float64)
    U = rr.wino_u(w, rr.G4)
    cols_first = np.einsum('ocil,jl->ocij', np.einsum('ik,ockl->ocil', rr.G4, g), rr.G4).astype(np.float32)      # any other float64 route
    assert rr.ulp_distance(U, cols_first).max() <= 1
    assert U.shape == (64, 64, 6, 6) and np.array_equal(U[:, :, 0, 0], (g[:, :, 0, 0] * 0.25 * 0.25).astype(np.float32))
    assert np.array_equal(U[:, :, 5, 5], w[:, :, 2, 2])


def test_normalise_model_equals_the_dataset_expression_on_every_byte():
    u = np.arange(256, dtype=np.uint8)
    a = np.asarray(u.reshape(16, 16, 1).repeat(3, 2), dtype=np.float32) / 255.0              # CustomDataset.__getitem__, word for word
    want = (a.transpose(2, 0, 1) - 0.5) / 0.5
    assert want.dtype == np.float32
    got = rr.normalise(u.reshape(16, 16, 1).repeat(3, 2).transpose(2, 0, 1))
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert got.min() == -1.0 and got.max() == 1.0


def test_bn_finalize_model_is_todays_torch_expression():
    """_BN.forward's [C]-sized algebra (float64 tensors on the host here) against the model, within the model's own bounds; the exact outputs bit-equal."""
    rs = np.random.RandomState(4)
    for c, n in ((1, 1), (64, 2048), (100, 37)):
        x = rs.randn(n, c) * 3 + rs.randn(c)
        x[:, 0] = 1.25                                                   # a constant channel: the variance clamps at (or rounds to) zero
        s, q = torch.as_tensor(x.sum(0)), torch.as_tensor((x * x).sum(0))
        weight, bias = torch.as_tensor(rs.randn(c).astype(np.float32)), torch.as_tensor(rs.randn(c).astype(np.float32))
        rm, rv = torch.as_tensor(rs.randn(c).astype(np.float32)), torch.as_tensor(rs.rand(c).astype(np.float32) + 0.5)
        ref = rr.bn_finalize(s.numpy(), q.numpy(), n, weight.numpy(), bias.numpy(), rm.numpy(), rv.numpy())
        bound = rr.bn_finalize_bounds(ref, rv.numpy())
        mean64 = s / n
        var64 = (q / n - mean64 * mean64).clamp_(min=0.0)
        mean, invstd = mean64.float(), torch.rsqrt(var64 + 1e-5).float()
        rm2 = rm.clone().mul_(1 - 0.1).add_(mean, alpha=0.1)
        rv2 = rv.clone().mul_(1 - 0.1).add_((var64 * (n / max(n - 1, 1))).float(), alpha=0.1)
        scale = weight * invstd
        shift = bias - mean * scale
        assert mean.numpy().tobytes() == ref['mean'].tobytes()
        assert rr.ulp_distance(invstd.numpy(), ref['invstd']).max() <= 1
        for k, t in (('scale', scale), ('shift', shift), ('running_mean', rm2), ('running_var', rv2)):
            err = np.abs(t.numpy().astype(np.float64) - ref[k].astype(np.float64))
            assert (err <= bound[k]).all(), (c, n, k, float((err / bound[k]).max()))
        b = rr.bn_bwd_finalize(s.numpy(), q.numpy(), n)
        assert b['d_bias'].tobytes() == s.float().numpy().tobytes() and b['m_dyxh'].tobytes() == (q / n).float().numpy().tobytes()


def test_header_and_binding_agree_on_the_new_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'l2i.h')).read()
    I, P, L, D = ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    want = {
        'l2i_repack_taps_f32': [P, P, I, I, I, ctypes.POINTER(_lib.RepackTaps), I, I, I, P],
        'l2i_repack_wino_f32': [P, P, I, I, I, I, I, P],
        'l2i_batch_from_u8_f32': [P, P, P, P, P, I, L, L, I, P],
        'l2i_bn_finalize_f32': [P] * 11 + [L, I, D, D, P],
        'l2i_bn_bwd_finalize_f32': [P] * 6 + [L, I, P],
    }
    for name, args in want.items():
        m = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert m, name
        assert len(m.group(1).split(',')) == len(args), name
        assert name in _lib.EXPORTS and name in _lib.ADDITIVE and _lib._SIGNATURES[name] == (I, args), name
    assert '#define L2I_ABI_VERSION 12' in hdr and _lib.ABI_VERSION == 12
    assert int(re.search(r'#define L2I_REPACK_MAX_TAPS (\d+)', hdr).group(1)) == _lib.REPACK_MAX_TAPS == rr.MAX_TAPS == 49
    assert ctypes.sizeof(_lib.RepackTaps) == 4 + 2 * 49 + 2                        # int32 + two byte arrays, padded to the int's alignment
    for macro, value in (('L2I_REPACK_PACKED', _lib.REPACK_PACKED), ('L2I_REPACK_OIHW', _lib.REPACK_OIHW), ('L2I_REPACK_WINO2', _lib.REPACK_WINO2),
                         ('L2I_REPACK_WINO4', _lib.REPACK_WINO4)):
        assert int(re.search(r'#define %s (\d+)' % macro, hdr).group(1)) == value
    t = _lib.repack_taps(rr.taps_grad_s1(7))
    assert t.count == 49 and (t.ky[0], t.kx[0], t.ky[48], t.kx[48]) == (6, 6, 0, 0)
