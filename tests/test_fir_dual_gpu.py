"""l2i_upfirdn2d_dual_f32 (csrc/l2i_stream.hip): one FIR pass, two outputs.  y must be what the single-output entry writes, bit for bit, and
y2 = y * (mask2 > 0 ? pos2 : neg2), one fp32 multiply: bit-equal to torch.where(mask2 > 0, y * pos2, y * neg2).

One case per kernel the launcher can pick, at the smallest shapes that still reach its branches: the zero-insertion kernel (natural 2x size, a
partial last sample, with and without the addend), the staged 4x4 kernel (an output width that is no multiple of 4: the scalar tail columns, with
the first mask too), the two streaming instantiations (192 and 196 columns: one strip, a partial wave), the generic kernel (up 2 on a width the
zero-insertion kernel refuses), and the staged kernel again from views 4 bytes past a 16-byte boundary (the scalar stores of both outputs).
mask2 holds +0, -0 and negative values: none of them is positive.  Both outputs lie inside sentinel-filled buffers."""
import pytest
import torch

from latent2im_amd import _lib
from tests import fir_ref as fr
from tests.contract_gpu import DEV, guarded, keep, refused, release, untouched

pytestmark = pytest.mark.gpu
VALS2 = (1.0, 0.2)

CASES = {  # id: (major, channels, ih, iw, up, pad, operands, offset of y2 / mask2 in floats, the kernel)
    'up2k4_8x8': (3, 2, 8, 8, 2, (2, 1, 2, 1), ('addend', 'bias'), 0, 'upfirdn2d_up2k4_kernel'),
    'up2k4_8x8_plain': (3, 2, 8, 8, 2, (2, 1, 2, 1), (), 0, 'upfirdn2d_up2k4_kernel'),
    'up2k4_6x10': (3, 2, 6, 10, 2, (2, 1, 2, 1), ('addend',), 0, 'upfirdn2d_up2k4_kernel'),
    'up2k4_6x10_plain': (3, 2, 6, 10, 2, (2, 1, 2, 1), ('bias',), 0, 'upfirdn2d_up2k4_kernel'),
    'k4_9x13': (3, 2, 9, 13, 1, (2, 1, 2, 1), ('addend', 'mask'), 0, 'upfirdn2d_k4_kernel'),
    'k4_40x72_off': (2, 2, 40, 72, 1, (2, 1, 2, 1), ('addend',), 1, 'upfirdn2d_k4_kernel'),
    'k4_stream_8x192': (2, 2, 8, 192, 1, (1, 2, 1, 2), ('addend',), 0, 'upfirdn2d_k4_stream_kernel<1>'),
    'k4_stream_8x196': (2, 2, 8, 196, 1, (2, 1, 2, 1), ('addend', 'mask'), 0, 'upfirdn2d_k4_stream_kernel<2>'),
    'k4_stream_off': (2, 2, 8, 192, 1, (1, 2, 1, 2), (), 1, 'upfirdn2d_k4_kernel'),          # y2 / mask2 unaligned: the launch leaves the vector kernel
    'generic_4x5': (3, 2, 4, 5, 2, (2, 1, 2, 1), ('addend', 'bias'), 0, 'upfirdn2d_kernel'),
}


@pytest.fixture(autouse=True)
def _operands_outlive_the_launch():
    yield
    release()


def _setup(case):
    major, ch, ih, iw, up, pad, ops, off2, path = CASES[case]
    g = torch.Generator().manual_seed(len(case) * 1000 + ih * iw)
    oh, ow = fr.out_size(ih, up, 1, pad[2], pad[3], 4), fr.out_size(iw, up, 1, pad[0], pad[1], 4)
    # the dispatch model of tests/fir_ref.py names the kernel this case is meant for (y2 / mask2 count like y)
    model_ops = tuple(o for o in ops if o != 'bias') + (('bias',) if 'bias' in ops else ())
    assert fr.path_f32(ih, iw, 4, 4, (up, up), (1, 1), pad, model_ops, off={'y': off2} if off2 else None) == path
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = keep(rnd(major, ih, iw).to(DEV))
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
    k = keep((torch.outer(k1, k1) / 64.0 * up * up).contiguous().to(DEV))
    addend = keep(rnd(major, oh, ow).to(DEV)) if 'addend' in ops else None
    bias = keep(rnd(ch).to(DEV)) if 'bias' in ops else None
    mask = keep(rnd(major, oh, ow).to(DEV)) if 'mask' in ops else None
    m2 = rnd(major, oh, ow)
    flat = m2.view(-1)
    flat[0::7] = 0.0
    flat[1::7] = -0.0
    flat[2::7] = -flat[2::7].abs() - 1e-30
    assert bool((flat[0::7] == 0).all()) and bool(torch.signbit(flat[1::7]).all()) and bool((flat[2::7] < 0).all()) and bool((flat > 0).any())
    m2buf, mask2 = guarded((major, oh, ow), off=off2)
    mask2.copy_(m2)
    keep(m2buf)
    tail = [_lib.fptr(x), _lib.fptr(k), major, ih, iw, 4, 4, up, up, 1, 1, pad[0], pad[1], pad[2], pad[3], ch,
            None, 0.0, _lib.fptr(bias), _lib.fptr(addend), 0, 0.2, 1.0, _lib.fptr(mask), 2.0 ** 0.5, 0.2 * 2.0 ** 0.5]
    return (major, oh, ow), off2, mask2, m2, tail


@pytest.mark.parametrize('case', list(CASES))
def test_dual_outputs(case):
    shape, off2, mask2, m2, tail = _setup(case)
    sbuf, ys = guarded(shape)
    _lib.call('l2i_upfirdn2d_masked_f32', _lib.fptr(ys), *tail)
    ybuf, y = guarded(shape)
    y2buf, y2 = guarded(shape, off=off2)
    _lib.call('l2i_upfirdn2d_dual_f32', _lib.fptr(y), _lib.fptr(y2), _lib.fptr(mask2), VALS2[0], VALS2[1], *tail)
    torch.cuda.synchronize()
    assert untouched(sbuf, ys) and untouched(ybuf, y) and untouched(y2buf, y2)
    yc, y2c = y.cpu(), y2.cpu()
    assert bool(torch.isfinite(yc).all()) and float(yc.abs().max()) > 0
    assert torch.equal(yc, ys.cpu())                                                   # y: bit-equal to the single-output launch
    pos, neg = torch.tensor(VALS2[0], dtype=torch.float32), torch.tensor(VALS2[1], dtype=torch.float32)
    want = torch.where(m2 > 0, yc * pos, yc * neg)
    assert torch.equal(y2c, want)                                                      # y2: one fp32 multiply of y
    # both NULL: the single-output entry
    nbuf, yn = guarded(shape)
    _lib.call('l2i_upfirdn2d_dual_f32', _lib.fptr(yn), None, None, VALS2[0], VALS2[1], *tail)
    torch.cuda.synchronize()
    assert untouched(nbuf, yn) and torch.equal(yn.cpu(), yc)


@pytest.mark.parametrize('case', ['up2k4_8x8', 'k4_9x13', 'k4_stream_8x192', 'generic_4x5'])
def test_half_given_pair_is_refused(case):
    shape, off2, mask2, m2, tail = _setup(case)
    ybuf, y = guarded(shape)
    y2buf, y2 = guarded(shape)
    refused(-1, 'l2i_upfirdn2d_dual_f32', _lib.fptr(y), _lib.fptr(y2), None, VALS2[0], VALS2[1], *tail, outs=(ybuf, y2buf))
    refused(-1, 'l2i_upfirdn2d_dual_f32', _lib.fptr(y), None, _lib.fptr(mask2), VALS2[0], VALS2[1], *tail, outs=(ybuf, y2buf))
    assert 'together or not at all' in _lib.load().l2i_last_error().decode()
