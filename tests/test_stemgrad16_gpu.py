"""l2i_conv2d_wgrad_img_h8 (csrc/l2i_train_h8.hip: the 16-bit trainer's stem gradient from the fp32 image and the h8 gradient map) against the float64
model and derived bound of tests/stemgrad16_ref.py: every case x {bf16, fp16}, dw and the workspace carved out of sentinel-filled buffers (nothing
outside them may change), every case launched twice with bit-equal results (no atomics, fixed summation order), and the refusals.  Every test
prints `rt16 stem_wgrad <case> <elem> <error / bound>`."""
import ctypes

import pytest
import torch

from latent2im_amd import _lib, conv
from latent2im_amd import kernels16 as K16
from tests import stemgrad16_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                  # sentinel elements on either side of a carved tensor
CASES = {c.name: c for c in sr.CASES}


def carve(shape, dtype, fill=sr.SENTINEL):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, what):
    fill = torch.full((GUARD,), sr.SENTINEL, dtype=buf.dtype, device=DEV)
    assert torch.equal(buf[:GUARD], fill) and torch.equal(buf[-GUARD:], fill), 'the launch wrote outside ' + what


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.mark.parametrize('elem', sr.ELEMS)
@pytest.mark.parametrize('name', list(CASES))
def test_stem_wgrad(name, elem):
    case, dtype = CASES[name], sr.ELEM_DTYPES[elem]
    x, gy = sr.data(case)
    want, bound = sr.stem_wgrad(x, gy, elem)
    xg, gg = x.to(DEV), conv.to_h8(gy.to(DEV), 8, dtype)
    nbytes = K16.wgrad_img_ws_bytes(case.b, case.h, case.w, dtype)
    assert nbytes > 0 and nbytes % sr.SLICE_BYTES == 0 and K16.WGRAD_IMG_SLICE_BYTES == sr.SLICE_BYTES
    slices = nbytes // sr.SLICE_BYTES
    if name == 'slices':                                     # the second pass must have something to add, within a sample too
        assert slices >= 3 and slices > case.b, slices
    outs = []
    for _ in range(2):
        wbuf, ws = carve((nbytes // 4,), torch.float32)
        obuf, dw = carve((sr.COUT, sr.CIN, sr.K, sr.K), torch.float32)
        K16.conv_wgrad_img(xg, gg, out=dw, ws=ws)
        torch.cuda.synchronize()
        guards_intact(wbuf, 'the workspace')
        guards_intact(obuf, 'dw')
        outs.append(dw.clone())
    err, b, ratio = sr.worst(outs[0], want, bound)
    print('rt16 stem_wgrad %s %s slices %d error %.3g bound %.3g ratio %.3g' % (name, elem, slices, err, b, ratio))
    assert ratio <= 1.0
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'two launches on the same inputs differ'


@pytest.mark.parametrize('elem', sr.ELEMS)
@pytest.mark.parametrize('arg,value', sr.REFUSALS)
def test_stem_wgrad_refusals(arg, value, elem):
    dtype = sr.ELEM_DTYPES[elem]
    s = dict(cin=3, cout=64, b=2, h=9, w=13)
    good = K16.wgrad_img_ws_bytes(s['b'], s['h'], s['w'], dtype)
    if arg in s:
        s[arg] = value
    oh, ow = sr.out_size(s['h']), sr.out_size(s['w'])
    xg = torch.zeros(s['b'], s['cin'], s['h'], s['w'], device=DEV)
    gbuf, gg = carve((s['b'], (s['cout'] + 7) // 8, oh, ow, 8), dtype, fill=0.0)
    wbuf, ws = carve((good // 4,), torch.float32)
    obuf, dw = carve((s['cout'], s['cin'], 7, 7), torch.float32)
    before_w, before_o = wbuf.clone(), obuf.clone()
    lib = _lib.load()
    fn = getattr(lib, 'l2i_conv2d_wgrad_img_h8' + ('_f16' if elem == 'f16' else ''))
    ws_ptr = None if arg == 'ws' else _lib.fptr(ws)
    ws_bytes = good - 4 if arg == 'ws_bytes' else good
    gy_ptr = ctypes.c_void_p(gg.data_ptr() + (2 if arg == 'gy' else 0))             # (inside gbuf's leading guard + map: still readable memory)
    rc = fn(_lib.fptr(dw), _lib.fptr(xg), gy_ptr, ws_ptr, ws_bytes, s['b'], s['cin'], s['h'], s['w'], s['cout'], oh, ow, 7, 2, 3, _lib.stream_ptr())
    torch.cuda.synchronize()
    msg = lib.l2i_last_error().decode()
    print('rt16 stem_wgrad refusal %s=%s %s -> %d: %s' % (arg, value, elem, rc, msg))
    assert rc in (-1, -3) and msg                            # L2I_E_ARG or L2I_E_UNSUPPORTED, with a message
    assert torch.equal(bits(wbuf), bits(before_w)) and torch.equal(bits(obuf), bits(before_o)), 'a refused call wrote something'
    if arg in ('cin', 'cout'):                               # the host-only query refuses the same shapes
        n = ctypes.c_int64(-1)
        q = getattr(lib, 'l2i_conv2d_wgrad_img_ws_h8' + ('_f16' if elem == 'f16' else ''))
        assert q(ctypes.byref(n), s['b'], s['cin'], s['h'], s['w'], s['cout'], oh, ow, 7, 2, 3) == -3 and n.value == 0
