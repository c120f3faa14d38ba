"""What the GPU contract tests share (tests/test_stream_contract_gpu.py, tests/test_fir_contract_gpu.py): outputs inside sentinel guards, device
operands kept alive until the test ends, the comparison of a row's outputs with its bounds, and a refused call.  A plain module: no fixtures."""
import pytest
import torch

from latent2im_amd import _lib
from tests import stream_ref as sr

DEV = 'cuda'


def guarded(shape, dtype=torch.float32, off=0):
    """(buffer, view): ``view`` of ``shape`` inside a sentinel-filled buffer, GUARD (+ off) elements from its start."""
    n = 1
    for s in shape:
        n *= s
    fill = sr.SENTINEL_U8 if dtype == torch.uint8 else sr.SENTINEL
    buf = torch.full((n + 2 * sr.GUARD + 4,), fill, dtype=dtype, device=DEV)
    return buf, buf[sr.GUARD + off:sr.GUARD + off + n].view(shape)


def untouched(buf, view=None):
    """The guards of ``buf`` around ``view`` (the whole buffer when ``view`` is None) still hold the sentinel."""
    fill = sr.SENTINEL_U8 if buf.dtype == torch.uint8 else sr.SENTINEL
    if view is None:
        return bool((buf == fill).all())
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


KEEP = []          # the device operands of the running test: a pointer handed to _lib.call has to outlive the launch that reads it


def release():
    torch.cuda.synchronize()
    KEEP.clear()


def keep(t):
    if t is not None:
        KEEP.append(t)
    return t


def dev(t):
    return None if t is None else keep(t.to(DEV))


def same(got, want):
    got, want = got.cpu(), want.cpu()
    if got.dtype.is_floating_point:
        return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got.double()), torch.nan_to_num(want.double()))
    return torch.equal(got, want)


def compare(row, elem, got, exp, log):
    bad = []
    for name, (want, bound) in exp.items():
        if bound is None:
            ok = same(got[name], want)
            log.append('%s %s %s exact %s' % (row.id, elem, name, 'equal' if ok else 'DIFFERENT'))
        else:
            err, bnd, ratio = sr.worst(got[name], want, bound)
            ok = ratio <= 1.0
            log.append('%s %s %s err %.3e bound %.3e ratio %.3f' % (row.id, elem, name, err, bnd, ratio))
        if not ok:
            bad.append(log[-1])
    assert not bad, bad


def refused(code, name, *args, outs=(), dtype=None):
    with pytest.raises(_lib.L2IError, match=r'failed \(%d\)' % code):
        _lib.call(name, *args, dtype=dtype)
    torch.cuda.synchronize()
    assert all(untouched(b) for b in outs), name
