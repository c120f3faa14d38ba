"""The three entry points of the differentiable face branch (csrc/l2i_face.hip: l2i_face_resize_lin_f32, l2i_face_resize_lin_bwd_f32,
l2i_face_head_bwd_f32) called raw on sentinel-carved buffers: inside the float64 model's any-order bounds (tests/faceid_ref.py), bit-equal from
one launch to the next, nothing written outside the output, and nothing written at all by a refused call."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib, facenet
from tests import contract_gpu as G
from tests import faceid_ref as M
from tests import stream_ref as sr

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = -1, -3
PLANES = 6
# H x W -> 160 x 160: upscale (every output clamps a border), identity tables, ratio 1.25, 256, an axis swap shows, 27 taps (the LDS chunks)
RESIZE_SHAPES = ((32, 32), (160, 160), (200, 200), (256, 256), (96, 64), (1024, 1024))


def _tables(n, fn):
    b, c = fn(n, M.FACE)
    return G.dev(torch.from_numpy(b)), G.dev(torch.from_numpy(c))


def _image(h, w, seed):
    x = (0.8 * np.random.RandomState(seed).randn(PLANES, h, w)).astype(np.float32)
    x[0, : max(h // 8, 1)] = 1.2                       # saturated rows, an exact edge and a NaN: the clamp's corner cases
    x[1, :, : max(w // 8, 1)] = -1.0
    x[2, h // 2, w // 2] = np.nan
    return x


def _twice(name, out_shape, args_of):
    outs = []
    for _ in range(2):
        buf, y = G.guarded(out_shape)
        _lib.call(name, *args_of(y))
        torch.cuda.synchronize()
        assert G.untouched(buf, y), name
        outs.append(y.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), '%s: two launches differ' % name
    return outs[0]


@pytest.mark.parametrize('h,w', RESIZE_SHAPES)
def test_resize_lin_forward_and_adjoint(h, w):
    x = _image(h, w, h + w)
    xd = G.dev(torch.from_numpy(x))
    xb, xc = _tables(w, facenet.resize_tables)
    yb, yc = _tables(h, facenet.resize_tables)
    got = _twice('l2i_face_resize_lin_f32', (PLANES, M.FACE, M.FACE),
                 lambda y: (_lib.fptr(y), _lib.fptr(xd), PLANES, h, w, M.FACE, M.FACE, _lib.ptr(xb), _lib.ptr(xc), xc.shape[1], _lib.ptr(yb), _lib.ptr(yc),
                            yc.shape[1]))
    want, bound = M.resize_lin(x)
    err, bnd, ratio = sr.worst(got, torch.from_numpy(want), bound)
    print('resize_lin %dx%d: err %.3e bound %.3e ratio %.3f' % (h, w, err, bnd, ratio))
    assert ratio <= 1.0

    gy = np.random.RandomState(h * 3 + w).randn(PLANES, M.FACE, M.FACE).astype(np.float32)
    gyd = G.dev(torch.from_numpy(gy))
    ixb, ixc = _tables(w, facenet.inverse_tables)
    iyb, iyc = _tables(h, facenet.inverse_tables)
    gx = _twice('l2i_face_resize_lin_bwd_f32', (PLANES, h, w),
                lambda o: (_lib.fptr(o), _lib.fptr(gyd), _lib.fptr(xd), PLANES, h, w, M.FACE, M.FACE, _lib.ptr(ixb), _lib.ptr(ixc), ixc.shape[1], _lib.ptr(iyb),
                           _lib.ptr(iyc), iyc.shape[1]))
    want, bound = M.resize_lin_bwd(gy, x)
    err, bnd, ratio = sr.worst(gx, torch.from_numpy(want), bound)
    print('resize_lin_bwd %dx%d: err %.3e bound %.3e ratio %.3f' % (h, w, err, bnd, ratio))
    assert ratio <= 1.0
    assert float(gx[2, h // 2, w // 2]) == 0.0 and float(gx[0, 0].abs().max()) == 0.0 and float(gx[1, :, 0].abs().max()) == 0.0
    G.release()


@pytest.mark.parametrize('B,C,HW,E', [(2, 1792, 9, 512), (3, 64, 4, 32)])
def test_head_bwd(B, C, HW, E):
    rs = np.random.RandomState(C + E)
    feat = np.maximum(rs.randn(B, C, HW), 0).astype(np.float32)
    w_t = (rs.randn(C, E) / np.sqrt(C)).astype(np.float32)
    bias = (0.05 * rs.randn(E)).astype(np.float32)
    v = rs.randn(B, E).astype(np.float32)
    v /= np.sqrt((v.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    gd = rs.uniform(0.1, 1.0, B).astype(np.float32)
    d = [G.dev(torch.from_numpy(a)) for a in (feat, w_t, bias, v, gd)]
    got = _twice('l2i_face_head_bwd_f32', (B, C, HW), lambda o: (_lib.fptr(o),) + tuple(_lib.fptr(t) for t in d) + (B, C, HW, E))
    want, bound = M.head_bwd(feat, w_t, bias, v, gd)
    err, bnd, ratio = sr.worst(got, torch.from_numpy(want), bound)
    print('head_bwd %s: err %.3e bound %.3e ratio %.3f' % ((B, C, HW, E), err, bnd, ratio))
    assert ratio <= 1.0
    G.release()


def test_refusals_leave_the_outputs_alone():
    buf, y = G.guarded((1 << 16,))
    x = G.dev(torch.zeros(1 << 16))
    t = G.dev(torch.zeros(1 << 12, dtype=torch.int32))
    p, q, o = _lib.fptr(x), _lib.ptr(t), _lib.fptr(y)
    fwd, bwd, head = 'l2i_face_resize_lin_f32', 'l2i_face_resize_lin_bwd_f32', 'l2i_face_head_bwd_f32'
    # the forward refuses what l2i_face_resize_f32 refuses (tests/test_facenet_gpu.py::test_refusals), the same way
    G.refused(E_UNSUPPORTED, fwd, o, p, 3, 1024, 1024, 320, 320, q, q, 27, q, q, 27, outs=(buf,))      # output > 256
    G.refused(E_UNSUPPORTED, fwd, o, p, 3, 4096, 4096, 160, 160, q, q, 103, q, q, 103, outs=(buf,))    # vertical support beyond the byte kernel's LDS
    G.refused(E_UNSUPPORTED, fwd, o, p, 3, 8192, 64, 160, 160, q, q, 5, q, q, 5, outs=(buf,))          # input > 4096
    G.refused(E_UNSUPPORTED, fwd, o, p, 3, 64, 64, 160, 160, q, q, 300, q, q, 5, outs=(buf,))          # taps > 256
    G.refused(E_ARG, fwd, o, p, 0, 64, 64, 160, 160, q, q, 5, q, q, 5, outs=(buf,))                    # no planes
    G.refused(E_ARG, fwd, o, p, 3, 64, 64, 160, 160, None, q, 5, q, q, 5, outs=(buf,))                 # a null table
    G.refused(E_UNSUPPORTED, bwd, o, p, p, 3, 1024, 1024, 320, 320, q, q, 4, q, q, 4, outs=(buf,))
    G.refused(E_UNSUPPORTED, bwd, o, p, p, 3, 8192, 64, 160, 160, q, q, 4, q, q, 4, outs=(buf,))
    G.refused(E_UNSUPPORTED, bwd, o, p, p, 3, 64, 64, 160, 160, q, q, 300, q, q, 4, outs=(buf,))
    G.refused(E_ARG, bwd, o, p, None, 3, 64, 64, 160, 160, q, q, 4, q, q, 4, outs=(buf,))
    G.refused(E_UNSUPPORTED, head, o, p, p, p, p, p, 2, 4096, 9, 512, outs=(buf,))                     # C > 2048
    G.refused(E_UNSUPPORTED, head, o, p, p, p, p, p, 2, 1792, 9, 1024, outs=(buf,))                    # E > 512
    G.refused(E_ARG, head, o, p, p, p, None, p, 2, 1792, 9, 512, outs=(buf,))                          # no embedding of the other half
    G.release()
