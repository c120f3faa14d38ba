"""tests/stemgrad16_ref.py on the CPU: a float32 evaluation of the stem gradient stays inside the derived bound, every seeded mistake breaks the bound
on the cases that list it (so the bound is not vacuous), the numpy statement of the plane formula equals conv.pack_weight_h8 / pack_weight_img_h8
bit for bit (through H8Conv / ImgConvH8 on the host) on the plane cases, and the build lists what the GPU tests call: both forms of every new
entry point in include/l2i.h, in _lib.ADDITIVE and _lib.EXPORTS, with ABI 12."""
import os
import re

import pytest
import torch

from latent2im_amd import _lib, conv
from tests import stemgrad16_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('l2i_conv2d_wgrad_img_h8', 'l2i_conv2d_wgrad_img_ws_h8', 'l2i_repack_planes_h8')
CASES = {c.name: c for c in sr.CASES}
PLANES = {c.name: c for c in sr.PLANE_CASES}
_MODEL = {}


def model(name, elem):
    if (name, elem) not in _MODEL:
        x, gy = sr.data(CASES[name])
        _MODEL[name, elem] = (x, gy) + sr.stem_wgrad(x, gy, elem)
    return _MODEL[name, elem]


@pytest.mark.parametrize('elem', sr.ELEMS)
@pytest.mark.parametrize('name', list(CASES))
def test_float32_inside_bound(name, elem):
    x, gy, want, bound = model(name, elem)
    got, _ = sr.stem_wgrad(x, gy, elem, dt=torch.float32)
    err, b, ratio = sr.worst(got, want, bound)
    print('rt16 stem_wgrad %s %s float32 emulation: error %.3g bound %.3g ratio %.3g' % (name, elem, err, b, ratio))
    assert ratio <= 1.0
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize('elem', sr.ELEMS)
@pytest.mark.parametrize('name,mistake', [(c.name, m) for c in sr.CASES for m in c.mistakes])
def test_mistake_breaks_bound(name, mistake, elem):
    x, gy, want, bound = model(name, elem)
    wrong, _ = sr.stem_wgrad(x, gy, elem, _mistake=mistake)
    _, _, ratio = sr.worst(wrong, want, bound)
    print('rt16 stem_wgrad %s %s mistake %s: ratio %.3g' % (name, elem, mistake, ratio))
    assert ratio > 1.0


def test_case_table_covers_the_issue():
    assert {(c.name, c.b, c.h, c.w) for c in sr.CASES} == {('one_pixel', 1, 1, 1), ('two', 1, 2, 2), ('odd', 3, 9, 13), ('even', 2, 10, 6), ('square', 2, 12, 12),
                                                          ('slices', 2, 96, 80)}
    assert [sr.pixels(c) for c in sr.CASES] == [1, 1, 105, 30, 72, 3840]
    assert {m for c in sr.CASES for m in c.mistakes} == set(sr.MISTAKES) and len(sr.MISTAKES) == 8
    for name in ('one_pixel', 'odd', 'even'):
        assert 'x_rounded_to_elem' in CASES[name].mistakes
    for name in ('two', 'square'):
        assert 'ky_kx_swapped' in CASES[name].mistakes
    assert {a for a, _ in sr.REFUSALS} == {'cin', 'cout', 'ws', 'ws_bytes', 'gy'}
    # one_pixel: only the centre tap is data, so every other tap has bound 0 and must be exactly 0
    _, _, want, bound = model('one_pixel', 'f16')
    centre = torch.zeros(7, 7, dtype=torch.bool)
    centre[3, 3] = True
    assert bool((bound[:, :, ~centre] == 0).all()) and bool((want[:, :, ~centre] == 0).all()) and bool((bound[:, :, centre] > 0).all())


def test_plane_case_table_covers_the_issue():
    got = {(c.cout, c.cin, c.k, c.stride, c.qpad) for c in sr.PLANE_CASES if not c.transposed}
    assert {(40, 24, 1, 1, 32), (64, 16, 3, 1, 16), (32, 72, 3, 2, 32), (96, 64, 1, 2, 32), (64, 3, 7, 2, 16)} <= got
    assert any(c.transposed and c.k == 3 for c in sr.PLANE_CASES)
    assert {m for c in sr.PLANE_CASES for _, m, _ in sr.plane_modes(c)} == {sr.FWD, sr.SWAP, sr.FLIP, sr.IMG}
    assert (sr.FWD, sr.SWAP, sr.FLIP, sr.IMG) == (conv.PLANES_FWD, conv.PLANES_SWAP, conv.PLANES_FLIP, conv.PLANES_IMG)
    w = sr.plane_weight(PLANES['c40x24_1x1'])
    assert [float(v) for v in w.view(-1)[:6]] == [float(torch.tensor(v, dtype=torch.float32)) for v in sr.PLANTED]


def test_rounding_of_the_planted_values():
    """numpy's (fp16) and the bit-pattern (bf16) rounding against torch's casts on the planted values: overflow, subnormals, ties, -0."""
    v = torch.tensor(sr.PLANTED + (-70000.0, 65519.9, 65520.0, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 1.0 + 3 * 2.0 ** -11, 1.0 + 3 * 2.0 ** -8), dtype=torch.float32)
    for elem in sr.ELEMS:
        want = v.to(sr.ELEM_DTYPES[elem]).view(torch.int16).numpy().view('uint16')
        assert (sr.round_bits(v.numpy(), elem) == want).all(), elem


def host_conv(case, w, dtype):
    if case.name == 'stem':
        return conv.ImgConvH8(w, case.stride, case.pad, device='cpu', dtype=dtype)
    return conv.H8Conv(w, stride=case.stride, padding=case.pad, transposed=case.transposed, device='cpu', cin_pad=case.qpad, dtype=dtype)


@pytest.mark.parametrize('elem', sr.ELEMS)
@pytest.mark.parametrize('name', list(PLANES))
def test_plane_formula_equals_the_torch_pack(name, elem):
    case = PLANES[name]
    w = sr.plane_weight(case)
    hc = host_conv(case, w, sr.ELEM_DTYPES[elem])
    for attr, mode, qpad in sr.plane_modes(case):
        want = getattr(hc, attr)
        got = sr.planes_np(w.numpy(), mode, qpad, elem)
        assert tuple(want.shape) == got.shape == conv.plane_set_shape(case.cout, case.cin, case.k, mode, qpad), (attr, tuple(want.shape), got.shape)
        assert (want.contiguous().view(torch.int16).numpy().view('uint16') == got).all(), '%s %s %s: the formula and the torch pack differ' % (name, attr, elem)


def test_build_lists_the_entry_points():
    with open(os.path.join(ROOT, 'include', 'l2i.h')) as f:
        header = f.read()
    for name in ENTRIES:
        for n in (name, name + '_f16'):
            assert re.search(r'\bint %s\(' % n, header), n + ' is not declared in include/l2i.h'
            assert n in _lib.ADDITIVE and n in _lib.EXPORTS, n
            assert _lib._SIGNATURES[n] is _lib._SIGNATURES[name]
    assert _lib.ABI_VERSION == 12 and re.search(r'#define L2I_ABI_VERSION 12\b', header)
    assert re.search(r'#define L2I_WGRAD_IMG_SLICE_BYTES \(64 \* 160 \* 4\)', header) and sr.SLICE_BYTES == 64 * 160 * 4
    src = open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'l2i_train_h8.hip')).read()
    for name in ENTRIES:
        assert 'H8_NAME(%s)' % name in src, name
