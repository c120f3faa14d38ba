"""conv.H8Conv and conv.ImgConvH8 own their element type (``dtype=``) and their repack (``repack(weight)``): the weight planes of the four layer
kinds of the 16-bit regressor trainer, for both element types, without touching conv.PRECISION.  The packing is plain torch: no GPU."""
import pytest
import torch

from latent2im_amd import conv
from latent2im_amd.regressor_train import H8_DTYPES

# (name, kernel, cin, cout, stride, padding) — the trainer's layer kinds
LAYERS = (('1x1', 1, 64, 256, 1, 0), ('3x3_s2', 3, 64, 64, 2, 1), ('1x1_s2', 1, 256, 512, 2, 0), ('stem_7x7', 7, 3, 64, 2, 3))


def _build(w, k, stride, padding, **kw):
    if k == 7:
        return conv.ImgConvH8(w, stride, padding, device='cpu', **kw)
    return conv.H8Conv(w, stride=stride, padding=padding, device='cpu', **kw)


def _planes(obj):
    return [obj.planes] if isinstance(obj, conv.ImgConvH8) else [obj.fwd_planes, obj.bwd_planes]


def _same(a, b):
    return len(a) == len(b) and all(p.dtype == q.dtype == torch.int16 and p.shape == q.shape and torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('elem', sorted(H8_DTYPES))
@pytest.mark.parametrize('layer', LAYERS, ids=[l[0] for l in LAYERS])
def test_dtype_and_repack_give_the_planes_of_a_fresh_object(layer, elem, monkeypatch):
    _, k, cin, cout, stride, padding = layer
    g = torch.Generator().manual_seed(k * 1000 + cin + cout + stride)
    w1, w2 = torch.randn(cout, cin, k, k, generator=g) * 0.1, torch.randn(cout, cin, k, k, generator=g) * 0.1
    assert conv.PRECISION == 'f32'
    with monkeypatch.context() as m:                              # the old way: the element type read from the global while the object is built
        m.setattr(conv, 'PRECISION', elem)
        old1 = _build(w1, k, stride, padding)
    assert conv.PRECISION == 'f32'
    obj = _build(w1, k, stride, padding, dtype=H8_DTYPES[elem])
    assert obj.dtype == old1.dtype == H8_DTYPES[elem]
    before = [p.clone() for p in _planes(obj)]
    assert _same(before, _planes(old1))
    obj.repack(w2)
    fresh = _build(w2, k, stride, padding, dtype=H8_DTYPES[elem])
    assert _same(_planes(obj), _planes(fresh))
    assert all(not torch.equal(p, q) for p, q in zip(_planes(obj), before))
    assert all(torch.equal(p, q) for p, q in zip(_planes(old1), before))          # (not in place: the old tensors are as they were)
    assert conv.PRECISION == 'f32'
