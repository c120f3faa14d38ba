"""FrozenConv2d.repack_ and the two kernels under it (csrc/l2i_repack.hip) against the model of tests/regtrain_ref.py and against a freshly
built FrozenConv2d: same memory, same bits."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from latent2im_amd import conv as C
from tests import regtrain_ref as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KINDS = rr.KINDS + (('3x3 s1 64->64 on a 32-wide map', 64, 64, 3, 1, 1),)


def _w(cout, cin, k, seed, scale=0.1):
    return torch.as_tensor(np.random.RandomState(seed).randn(cout, cin, k, k).astype(np.float32) * np.float32(scale)).to(DEV)


_tensors = rr.derived_tensors


def _run(fc, x, gy, hw):
    return fc.forward(x), fc.dgrad(gy, hw)


@pytest.mark.parametrize('kind', KINDS, ids=[k[0] for k in KINDS])
def test_repack_in_place_equals_a_fresh_object(kind):
    name, cout, cin, k, stride, pad = kind
    wino = 'wide map' in name
    h = 32 if wino else 12
    w1, w2 = _w(cout, cin, k, 1), _w(cout, cin, k, 2)
    w2_host = w2.cpu().numpy()
    rs = np.random.RandomState(3)
    x = torch.as_tensor(rs.randn(2, cin, h, h).astype(np.float32)).to(DEV)
    fc = C.FrozenConv2d(w1, stride=stride, padding=pad, device=DEV)
    oh, ow = fc.out_hw(h, h)
    gy = torch.as_tensor(rs.randn(2, cout, oh, ow).astype(np.float32)).to(DEV)
    _run(fc, x, gy, (h, h))
    if wino:                                                      # the map takes F(4x4); the F(2x2) packs are what WINO4 = 'off' would build
        fc.fwd[0].wino_pack(), fc.bwd[0].wino_pack()
        assert all(getattr(L, a) is not None for L in (fc.fwd[0], fc.bwd[0]) for a in ('wino', 'wino4'))
    before = {n: t.data_ptr() for n, t in _tensors(fc).items()}
    fc.repack_(w2)
    y, gx = _run(fc, x, gy, (h, h))
    fresh = C.FrozenConv2d(w2.clone(), stride=stride, padding=pad, device=DEV)
    y_f, gx_f = _run(fresh, x, gy, (h, h))
    if wino:
        fresh.fwd[0].wino_pack(), fresh.bwd[0].wino_pack()
    torch.cuda.synchronize()
    got, want = _tensors(fc), _tensors(fresh)
    assert set(got) == set(want) and {n: t.data_ptr() for n, t in got.items()} == before
    assert fc.fwd[0].w_src is None or fc.fwd[0].w_src.data_ptr() == w2.data_ptr()
    assert torch.equal(w2.cpu(), torch.as_tensor(w2_host))         # the source is only read
    for n in got:
        a, b = got[n].cpu().numpy(), want[n].cpu().numpy()
        assert a.shape == b.shape, n
        if 'wino' not in n:
            assert a.tobytes() == b.tobytes(), (name, n)
            continue
        swap = n.startswith('launch1')                             # the stride-1 gradient: roles swapped, taps reversed
        model = (rr.wino4_pack if n.endswith('wino4') else rr.wino2_pack)(w2_host, swap, swap)
        assert a.tobytes() == model.reshape(a.shape).tobytes(), (name, n)
        d = rr.ulp_distance(a.reshape(-1), b.reshape(-1))
        print('%s: %.3f %% of entries 1 ulp from the fresh pack' % (n, 100.0 * float((d > 0).mean())))
        assert d.max() <= 1, (name, n, int(d.max()))
    if wino:        # F(4x4) packs may differ by 1 ulp in a few entries: the outputs are then close, not equal (error of the route itself: ~1e-5 of max|y|)
        assert float((y - y_f).abs().max()) <= 1e-5 * float(y_f.abs().max()) and float((gx - gx_f).abs().max()) <= 1e-5 * float(gx_f.abs().max())
    else:
        assert torch.equal(y, y_f) and torch.equal(gx, gx_f), name


def _gpu_gather(w, taps, swap, pad_to=32, oihw=False):
    cout, cin, k, _ = w.shape
    rows, cols = (cout, cin) if swap else (cin, cout)
    shape = (rows, cols, len(taps)) if oihw else (rows, len(taps), rr.round_up(cols, pad_to))
    dst = torch.full(shape, float('nan'), device=DEV, dtype=torch.float32)
    C._repack_taps(dst, w, taps, swap, _lib.REPACK_OIHW if oihw else _lib.REPACK_PACKED)
    return dst.cpu().numpy()


@pytest.mark.parametrize('cout,cin,k', [(5, 7, 1), (5, 7, 3), (7, 5, 1), (36, 4, 1), (512, 512, 3)],
                         ids=['5x7 1x1', '5x7 3x3', '7x5 1x1', '36x4 1x1 (16-byte loads)', '512x512 3x3 (more vectors than threads in the grid)'])
def test_gather_kernel_equals_the_model(cout, cin, k):
    """Odd channel counts (partial last vector, unaligned source rows), the 16-byte load path of 1x1 role-swapped packs, and a pack larger
    than one pass of the grid-stride loop; every layout."""
    w = _w(cout, cin, k, 5)
    wh = w.cpu().numpy()
    for taps in (rr.taps_forward(k), rr.taps_grad_s1(k)):
        for swap in (False, True):
            for pad_to in (32, 4):
                assert _gpu_gather(w, taps, swap, pad_to).tobytes() == rr.gather(wh, taps, swap, pad_to).tobytes(), (swap, pad_to)
            assert _gpu_gather(w, taps, swap, oihw=True).tobytes() == rr.gather(wh, taps, swap, oihw=True).tobytes(), swap


@pytest.mark.parametrize('cout,cin', [(40, 8), (8, 40), (64, 64)])
def test_winograd_kernel_equals_the_model(cout, cin):
    w = _w(cout, cin, 3, 6)
    wh = w.cpu().numpy()
    for swap, flip in ((False, False), (True, True), (False, True)):
        for kind, model in ((_lib.REPACK_WINO2, rr.wino2_pack), (_lib.REPACK_WINO4, rr.wino4_pack)):
            want = model(wh, swap, flip)
            dst = torch.full((want.size,), float('nan'), device=DEV, dtype=torch.float32)
            _lib.call('l2i_repack_wino_f32', _lib.fptr(dst), _lib.fptr(w), cout, cin, kind, int(swap), int(flip))
            assert dst.cpu().numpy().tobytes() == want.tobytes(), (kind, swap, flip)


def test_refusals():
    lib = _lib.load()
    w = _w(8, 16, 3, 7)
    dst = torch.zeros(16 * 9 * 32, device=DEV)
    t9 = _lib.repack_taps(rr.taps_forward(3))
    ok = lambda *a: lib.l2i_repack_taps_f32(*a, _lib.stream_ptr())
    assert ok(_lib.fptr(dst), _lib.fptr(w), 8, 16, 3, t9, 0, 32, _lib.REPACK_PACKED) == 0
    E_ARG = -1
    assert ok(None, _lib.fptr(w), 8, 16, 3, t9, 0, 32, 0) == E_ARG and b'null' in lib.l2i_last_error()
    assert ok(_lib.fptr(dst), None, 8, 16, 3, t9, 0, 32, 0) == E_ARG
    assert ok(_lib.fptr(dst), _lib.fptr(w), 8, 16, 3, None, 0, 32, 0) == E_ARG
    t50 = _lib.RepackTaps()
    t50.count = 50
    assert ok(_lib.fptr(dst), _lib.fptr(w), 8, 16, 3, t50, 0, 32, 0) == E_ARG and b'49' in lib.l2i_last_error()
    assert ok(_lib.fptr(dst), _lib.fptr(w), 8, 16, 3, t9, 0, 4, 0) == E_ARG and b'colsP' in lib.l2i_last_error()      # 8 real columns
    assert ok(_lib.fptr(dst), _lib.fptr(w), 8, 16, 3, t9, 1, 8, 0) == E_ARG                                           # swapped: 16 real columns
    t_out = _lib.repack_taps([(0, 3)])
    assert ok(_lib.fptr(dst), _lib.fptr(w), 8, 16, 3, t_out, 0, 32, 0) == E_ARG
    assert ok(_lib.fptr(dst), _lib.fptr(w), 8, 16, 3, t9, 0, 32, 7) == E_ARG
    wino = lambda *a: lib.l2i_repack_wino_f32(*a, _lib.stream_ptr())
    assert wino(None, _lib.fptr(w), 8, 16, _lib.REPACK_WINO2, 0, 0) == E_ARG and wino(_lib.fptr(dst), None, 8, 16, _lib.REPACK_WINO2, 0, 0) == E_ARG
    assert wino(_lib.fptr(dst), _lib.fptr(w), 8, 16, 3, 0, 0) == E_ARG
    assert wino(_lib.fptr(dst), _lib.fptr(w), 6, 16, _lib.REPACK_WINO4, 1, 1) == E_ARG                                # cin' = 6 is no whole 4-channel chunk
    torch.cuda.synchronize()
    assert float(dst.abs().sum()) > 0                                                                                  # (the one good call wrote)
