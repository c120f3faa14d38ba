"""l2i_batch_from_u8_f32: a normalised batch gathered by index from uint8 images on the device, bit for bit the model of tests/regtrain_ref.py
(which is CustomDataset's float32 expression: tests/test_regtrain_ref_cpu.py)."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from tests import regtrain_ref as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _gather(src, labels, idx):
    n, elems = src.shape[0], int(np.prod(src.shape[1:]))
    d_src, d_lab = torch.as_tensor(src).to(DEV), torch.as_tensor(labels).to(DEV)
    d_idx = torch.as_tensor(np.asarray(idx, dtype=np.int64)).to(DEV)
    out = torch.full((len(idx),) + src.shape[1:], float('nan'), device=DEV)
    lab = torch.full((len(idx), labels.shape[1]), float('nan'), device=DEV)
    _lib.call('l2i_batch_from_u8_f32', _lib.fptr(out), _lib.fptr(lab), _lib.ptr(d_src), _lib.fptr(d_lab), _lib.ptr(d_idx), len(idx), n, elems, labels.shape[1])
    return out.cpu().numpy(), lab.cpu().numpy()


@pytest.mark.parametrize('s', (1, 7, 64))
def test_every_byte_value_repeated_descending_and_out_of_range_indices(s):
    """S = 1 and 7: 3 and 147 bytes an image (no whole 16-byte vector, images off any alignment): the byte path; S = 64: the 16-byte path, more than
    one block a sample."""
    rs = np.random.RandomState(s)
    n = 300 if s == 1 else 9
    src = rs.randint(0, 256, size=(n, 3, s, s)).astype(np.uint8)
    flat = src.reshape(-1)
    flat[:256] = np.arange(256, dtype=np.uint8)                       # every byte value is there, whatever the size
    flat[-256:] = np.arange(255, -1, -1).astype(np.uint8)
    labels = rs.rand(n, 40).astype(np.float32)
    idx = [n - 1, n - 2, 3, 3, 0, n - 1, 1, 0] + list(range(n - 1, -1, -1)) + [n, -1, 2 ** 40, 2]
    got, lab = _gather(src, labels, idx)
    want, want_lab = rr.batch_from_u8(src, labels, idx)
    assert set(np.unique(src[np.unique([i for i in idx if 0 <= i < n])])) == set(range(256))
    assert got.tobytes() == want.tobytes() and lab.tobytes() == want_lab.tobytes()
    for b in (-4, -3, -2):                                              # out of range: zeros, nothing read
        assert not got[b].any() and not lab[b].any()
    assert got.min() == -1.0 and got.max() == 1.0


def test_labels_are_optional_and_bad_arguments_are_refused():
    src = torch.arange(96, dtype=torch.uint8, device=DEV).reshape(2, 48)
    idx = torch.tensor([1, 0], device=DEV)
    out = torch.zeros(2, 48, device=DEV)
    _lib.call('l2i_batch_from_u8_f32', _lib.fptr(out), None, _lib.ptr(src), None, _lib.ptr(idx), 2, 2, 48, 0)
    assert out.cpu().numpy().tobytes() == rr.normalise(src.cpu().numpy()[[1, 0]]).tobytes()
    lib = _lib.load()
    st = _lib.stream_ptr
    assert lib.l2i_batch_from_u8_f32(None, None, _lib.ptr(src), None, _lib.ptr(idx), 2, 2, 48, 0, st()) == -1
    assert lib.l2i_batch_from_u8_f32(_lib.fptr(out), None, _lib.ptr(src), None, None, 2, 2, 48, 0, st()) == -1
    assert lib.l2i_batch_from_u8_f32(_lib.fptr(out), None, _lib.ptr(src), None, _lib.ptr(idx), 0, 2, 48, 0, st()) == -1
    assert lib.l2i_batch_from_u8_f32(_lib.fptr(out), _lib.fptr(out), _lib.ptr(src), None, _lib.ptr(idx), 2, 2, 48, 40, st()) == -1
