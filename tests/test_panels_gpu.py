"""l2i_panels_u8 against the exact model of tests/panels_ref.py (clip_ims + imgrid), bit for bit: every case with ``out`` at byte offsets 0..3 past
a 16-byte boundary inside a sentinel-filled buffer (the sentinel intact on both sides: the launch writes its buffer and nothing else), ``x`` at
element offsets 0 and 1, two launches compared, fill 0 and 255."""

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, kernels
from tests import panels_ref as pr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 0xA5
GUARD = 64          # sentinel bytes in front of and behind out


def _aligned_bytes(n):
    """A uint8 device buffer of n bytes that starts on a 16-byte boundary."""
    buf = torch.empty(n + 16, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 16
    return buf[off:off + n]


def _launch(x, tile_src, G, rows, cols, pad, fill, out_off=0, x_off=0):
    """One launch with out at byte offset out_off past a 16-byte boundary and x at element offset x_off; returns (out as numpy, guards intact)."""
    n, c, h, w = x.shape
    gh, gw = pr.grid_hw(rows, cols, h, w, pad)
    total = G * gh * gw * c
    buf = _aligned_bytes(GUARD + out_off + total + GUARD)
    buf.fill_(SENTINEL)
    out = buf[GUARD + out_off:GUARD + out_off + total]
    assert out.data_ptr() % 16 == out_off
    xbuf = torch.empty(x.size + 4 + x_off, dtype=torch.float32, device=DEV)
    xoff = ((-xbuf.data_ptr()) % 16) // 4 + x_off
    xd = xbuf[xoff:xoff + x.size].view(x.shape)
    xd.copy_(torch.as_tensor(x))
    assert xd.data_ptr() % 16 == 4 * x_off
    ts = torch.as_tensor(np.asarray(tile_src, dtype=np.int32)).to(DEV)
    got = kernels.panels_u8(xd, ts, G, rows, cols, pad=pad, fill=fill, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    intact = (host[:GUARD + out_off] == SENTINEL).all() and (host[GUARD + out_off + total:] == SENTINEL).all()
    return host[GUARD + out_off:GUARD + out_off + total].reshape(G, gh, gw, c).copy(), bool(intact)


@pytest.fixture(scope='module')
def references():
    """The model's output of every case, for fill 0 and 255: computed once, read by every alignment."""
    ref = {}
    for case in pr.CASES:
        G, rows, cols, C, H, W, pad, N = case
        x, tile_src = pr.case_inputs(case)
        ref[case] = (x, tile_src, {fill: pr.panels(x, tile_src, G, rows, cols, pad, fill) for fill in (0, 255)})
    return ref


@pytest.mark.parametrize('case', pr.CASES)
def test_cases_bit_equal_at_every_alignment(case, references):
    G, rows, cols, C, H, W, pad, N = case
    x, tile_src, want = references[case]
    for out_off in (0, 1, 2, 3):
        for x_off in (0, 1):
            fill = 255 if (out_off + x_off) % 2 else 0
            got, intact = _launch(x, tile_src, G, rows, cols, pad, fill, out_off, x_off)
            assert intact, 'bytes outside out were written (out offset %d, x offset %d)' % (out_off, x_off)
            assert got.tobytes() == want[fill].tobytes(), 'out offset %d, x offset %d, fill %d' % (out_off, x_off, fill)
    again, _ = _launch(x, tile_src, G, rows, cols, pad, 255, 3, 1)
    assert again.tobytes() == want[255].tobytes()                      # a second launch of the same inputs: the same bytes
    for fill in (0, 255):
        got, intact = _launch(x, tile_src, G, rows, cols, pad, fill)
        assert intact and got.tobytes() == want[fill].tobytes()


def test_one_image_in_several_tiles_and_bad_indices_become_fill():
    case = (2, 2, 3, 3, 6, 5, 1, 4)
    G, rows, cols, C, H, W, pad, N = case
    x, _ = pr.case_inputs(case)
    tile_src = [2, 2, -1, 0, N, 2, 2 ** 30, 3, 3, 1, -2 ** 31, 0]
    for fill in (0, 255, 77):
        got, intact = _launch(x, tile_src, G, rows, cols, pad, fill, out_off=1)
        assert intact and got.tobytes() == pr.panels(x, tile_src, G, rows, cols, pad, fill).tobytes()
        for t in (2, 4, 6, 10):                                        # the four bad indices: whole tiles of fill
            g, r, c = t // (rows * cols), (t // cols) % rows, t % cols
            assert (got[g, r * (H + pad):r * (H + pad) + H, c * (W + pad):c * (W + pad) + W] == fill).all()


def test_the_778_boundary_values_and_nan():
    q = pr.quant_inputs()
    vals = np.concatenate([q, np.array([np.nan, -np.nan], dtype=np.float32), q[:30]])          # 810 = 3 * 18 * 15
    x = vals.reshape(1, 3, 18, 15)
    got, intact = _launch(x, [0], 1, 1, 1, 0, 0, out_off=2, x_off=1)
    assert intact
    got = got[0].transpose(2, 0, 1).reshape(-1)                          # back to the order of vals
    finite = ~np.isnan(vals)
    assert np.array_equal(got[finite], pr.clip_ims(vals[finite]))
    assert (got[~finite] == 0).all() and (~finite).sum() == 2
    for m in pr.QUANT_MISTAKES:                                        # these inputs do tell the seeded mistakes from the kernel
        assert (got[finite] != pr.clip_ims(vals[finite], m)).sum() >= 100


def test_unsupported_arguments_are_refused_and_leave_out_untouched():
    lib = _lib.load()
    x = torch.zeros(2, 3, 4, 4, device=DEV)
    x1 = torch.zeros(2, 2, 4, 4, device=DEV)
    ts = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=DEV)

    def call(xx, G, rows, cols, C, H, W, pad, fill, N, o=out, t=ts):
        return lib.l2i_panels_u8(_lib.ptr(o), _lib.fptr(xx), _lib.ptr(t), G, rows, cols, C, H, W, pad, fill, N, _lib.stream_ptr())

    UNSUPPORTED = -3
    assert call(x1, 1, 1, 2, 2, 4, 4, 0, 0, 2) == UNSUPPORTED           # C = 2
    assert call(x1, 1, 1, 2, 4, 4, 4, 0, 0, 1) == UNSUPPORTED           # C = 4
    assert call(x, 1, 1, 2, 3, 4, 4, -1, 0, 2) == UNSUPPORTED           # pad < 0
    assert call(x, 1, 1, 2, 3, 4, 4, 0, 256, 2) == UNSUPPORTED          # fill outside 0..255
    assert call(x, 1, 1, 2, 3, 4, 4, 0, -1, 2) == UNSUPPORTED
    for empty in ((0, 1, 2, 3, 4, 4), (1, 0, 2, 3, 4, 4), (1, 1, 0, 3, 4, 4), (1, 1, 2, 3, 0, 4), (1, 1, 2, 3, 4, 0)):
        assert call(x, *empty, 0, 0, 2) == UNSUPPORTED                  # empty dimensions
    assert call(x, 1, 1, 2, 3, 4, 4, 0, 0, 0) == UNSUPPORTED            # no images
    assert b'l2i_panels_u8' in lib.l2i_last_error()
    assert lib.l2i_panels_u8(None, _lib.fptr(x), _lib.ptr(ts), 1, 1, 2, 3, 4, 4, 0, 0, 2, _lib.stream_ptr()) < 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert call(x, 1, 1, 2, 3, 4, 4, 0, 0, 2) == 0                      # and the same arguments, valid, do run
    assert (out[:96].cpu().numpy() == 127).all() and (out[96:].cpu().numpy() == SENTINEL).all()


def test_binding_allocates_and_takes_a_python_table():
    x, _ = pr.case_inputs((1, 1, 2, 1, 3, 3, 1, 2))
    got = kernels.panels_u8(torch.as_tensor(x).to(DEV), [1, 0], 1, 1, 2, pad=1, fill=255)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 3, 7, 1) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), pr.panels(x, [1, 0], 1, 1, 2, 1, 255))


def test_offsets_past_two_to_the_31_bytes():
    """720 grids of one 1024 x 1024 tile, every one naming the same image: 2.26e9 output bytes from a 12 MB source.  Grid 0 against the model, every
    other grid against grid 0 on the device."""
    x = np.random.RandomState(5).uniform(-1.1, 1.1, size=(1, 3, 1024, 1024)).astype(np.float32)
    G = 720
    out = kernels.panels_u8(torch.as_tensor(x).to(DEV), torch.zeros(G, dtype=torch.int32, device=DEV), G, 1, 1)
    assert out.numel() > 2 ** 31
    assert np.array_equal(out[0].cpu().numpy(), pr.panels(x, [0], 1, 1, 1)[0])
    assert bool((out == out[0]).all())
