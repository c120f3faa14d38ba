"""The numpy model of tests/panels_ref.py against the expressions it restates (clip_ims, imgrid's pad / reshape / crop), the power of the inputs
the GPU tests use to tell seeded mistakes apart, and the declarations of l2i_panels_u8 — no GPU.  tests/test_panels_gpu.py then holds the kernel
to the model."""
import os
import re

import numpy as np
import pytest

from latent2im_amd import _lib
from tests import panels_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quantiser_inputs_are_the_thresholds_and_their_neighbours():
    q = pr.quant_inputs()
    assert q.size == 778 and q.dtype == np.float32
    got = pr.clip_ims(q)
    assert set(np.unique(got)) == set(range(256))
    t = q[1:768:3]
    assert np.array_equal(t, (2.0 * np.arange(256) / 255.0 - 1.0).astype(np.float32))
    # around every threshold the byte moves by at most one level (float32 rounding decides on which side of float32(2k / 255 - 1) it steps)
    tri = got[:768].reshape(256, 3).astype(int)
    assert (np.diff(tri, axis=1) >= 0).all() and (tri[:, 2] - tri[:, 0] <= 1).all()
    assert (tri[1:, 2] - tri[1:, 0]).sum() >= 128 and (tri[:, 2] == np.arange(256)).all()
    assert got[768:].tolist() == [255, 0, 127, 127, 255, 0, 127, 127, 255, 0]


def test_the_model_is_the_numpy_expression_of_clip_ims():
    x = np.random.RandomState(3).uniform(-1.3, 1.3, size=(2, 3, 9, 5)).astype(np.float32)
    assert np.array_equal(pr.clip_ims(x), np.uint8(np.clip(((x + 1) / 2.0) * 255, 0, 255)))


@pytest.mark.parametrize('mistake', pr.QUANT_MISTAKES)
def test_every_seeded_quantiser_mistake_changes_at_least_100_of_the_778_bytes(mistake):
    """Measured with numpy: rint instead of truncation 274, evaluation in float64 112, the folded x * 127.5 + 127.5 206."""
    q = pr.quant_inputs()
    changed = int((pr.clip_ims(q, mistake) != pr.clip_ims(q)).sum())
    print(mistake, changed)
    assert changed >= 100
    assert changed == {'rint': 274, 'float64': 112, 'fused': 206}[mistake]


def _imgrid(imarray, cols, pad, fill):
    """imgrid's steps (np.pad on the bottom / right, reshape, transpose, crop) written out for one grid [N, H, W, C]."""
    n, h, w, c = imarray.shape
    rows = -(-n // cols)
    a = np.pad(imarray, [[0, rows * cols - n], [0, pad], [0, pad], [0, 0]], 'constant', constant_values=fill)
    g = a.reshape(rows, cols, h + pad, w + pad, c).transpose(0, 2, 1, 3, 4).reshape(rows * (h + pad), cols * (w + pad), c)
    return g[:-pad, :-pad] if pad else g


@pytest.mark.parametrize('case', pr.CASES)
def test_the_model_is_imgrid_of_clip_ims_per_grid(case):
    G, rows, cols, C, H, W, pad, N = case
    x, tile_src = pr.case_inputs(case)
    got = pr.panels(x, tile_src, G, rows, cols, pad, 255)
    assert got.shape == (G,) + pr.grid_hw(rows, cols, H, W, pad) + (C,) and got.dtype == np.uint8
    q = pr.clip_ims(x).transpose(0, 2, 3, 1)
    per = rows * cols
    for g in range(G):
        ims = q[g * per:min((g + 1) * per, N)]
        assert np.array_equal(got[g], _imgrid(ims, cols, pad, 255))


@pytest.mark.parametrize('case', [c for c in pr.CASES if c[6] > 0])
@pytest.mark.parametrize('mistake', pr.GRID_MISTAKES)
def test_every_seeded_imgrid_mistake_changes_bytes_on_the_padded_cases(case, mistake):
    G, rows, cols, C, H, W, pad, N = case
    x, tile_src = pr.case_inputs(case)
    for fill in (0, 255):
        assert pr.panels(x, tile_src, G, rows, cols, pad, fill, mistake).tobytes() != pr.panels(x, tile_src, G, rows, cols, pad, fill).tobytes()


def test_empty_and_repeated_tiles():
    x, _ = pr.case_inputs((1, 1, 4, 3, 3, 3, 1, 2))
    out = pr.panels(x, [1, -1, 1, 2], 1, 1, 4, 1, 9)
    q = pr.clip_ims(x).transpose(0, 2, 3, 1)
    assert np.array_equal(out[0, :, 0:3], q[1]) and np.array_equal(out[0, :, 8:11], q[1])
    assert (out[0, :, 4:7] == 9).all() and (out[0, :, 12:15] == 9).all() and (out[0, :, 3::4] == 9).all()


def test_entry_point_is_declared_bound_additive_and_built():
    with open(os.path.join(ROOT, 'include', 'l2i.h')) as f:
        header = f.read()
    m = re.search(r'int l2i_panels_u8\(([^)]*)\)', header)
    assert m, 'include/l2i.h does not declare l2i_panels_u8'
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    assert args == ['uint8_t* out', 'const float* x', 'const int32_t* tile_src', 'int G', 'int rows', 'int cols', 'int C', 'int H', 'int W',
                    'int pad', 'int fill', 'int N', 'void* stream']
    res, argtypes = _lib._SIGNATURES['l2i_panels_u8']
    assert res is _lib.c_i and argtypes == [_lib.c_p] * 3 + [_lib.c_i] * 9 + [_lib.c_p]
    assert 'l2i_panels_u8' in _lib.ADDITIVE and 'l2i_panels_u8' in _lib.EXPORTS
    assert _lib.ABI_VERSION == 12 and re.search(r'#define L2I_ABI_VERSION 12\b', header)
    with open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'Makefile')) as f:
        srcs = [l for l in f.read().splitlines() if l.startswith('SRCS')][0]
    assert 'l2i_panels.hip' in srcs.split()
    with open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'l2i_device.h')) as f:
        assert len(re.findall(r'int quant8\(float', f.read())) == 1
    with open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'l2i_face.hip')) as f:
        assert not re.search(r'int quant8\(float', f.read()), 'quant8 is stated once, in l2i_device.h'
