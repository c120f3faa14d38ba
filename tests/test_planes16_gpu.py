"""l2i_repack_planes_h8 (csrc/l2i_train_h8.hip: every 16-bit weight plane set of a net rewritten in place by one launch) against the torch packs of
conv.H8Conv / conv.ImgConvH8 and the numpy statement of tests/stemgrad16_ref.py, bit for bit: every plane case and mode x {bf16, fp16} into a
sentinel-filled destination, one launch over a table of every case's segments, ``repack_`` keeping its pointers, and the refusals."""
import pytest
import torch

from latent2im_amd import _lib, conv
from tests import stemgrad16_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096
PLANES = {c.name: c for c in sr.PLANE_CASES}
SENTINEL_BITS = 0x5A5A          # no weight of the cases rounds to this pattern in a whole slot


def carve(shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), SENTINEL_BITS, dtype=torch.int16, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf):
    fill = torch.full((GUARD,), SENTINEL_BITS, dtype=torch.int16, device=DEV)
    assert torch.equal(buf[:GUARD], fill) and torch.equal(buf[-GUARD:], fill), 'the launch wrote outside its destination'


def host_conv(case, w, dtype, device='cpu'):
    if case.name == 'stem':
        return conv.ImgConvH8(w, case.stride, case.pad, device=device, dtype=dtype)
    return conv.H8Conv(w, stride=case.stride, padding=case.pad, transposed=case.transposed, device=device, cin_pad=case.qpad, dtype=dtype)


def as_bits(t):
    return t.contiguous().view(torch.int16)


def segments_of(case, dtype):
    """(weight on the device, [(sentinel buffer, destination, torch pack, mode, qpad)]) of a case."""
    w = sr.plane_weight(case)
    hc = host_conv(case, w, dtype)
    out = []
    for attr, mode, qpad in sr.plane_modes(case):
        want = as_bits(getattr(hc, attr))
        buf, dst = carve(tuple(want.shape))
        out.append((buf, dst, want.to(DEV), mode, qpad))
    return w.to(DEV), out


@pytest.mark.parametrize('elem', sr.ELEMS)
@pytest.mark.parametrize('name', list(PLANES))
def test_every_mode_equals_the_torch_pack(name, elem):
    case, dtype = PLANES[name], sr.ELEM_DTYPES[elem]
    w, segs = segments_of(case, dtype)
    for buf, dst, want, mode, qpad in segs:
        for _ in range(2):
            dst.fill_(SENTINEL_BITS)
            conv.PlaneTable([(dst, w, mode, qpad)], dtype).run()
            torch.cuda.synchronize()
            guards_intact(buf)
            assert torch.equal(dst, want), '%s mode %d %s differs from the torch pack' % (name, mode, elem)
        got = dst.cpu().numpy().view('uint16')
        assert (got == sr.planes_np(w.cpu().numpy(), mode, qpad, elem)).all()
        print('rt16 repack_planes %s mode %d %s: %d slots bit-equal' % (name, mode, elem, dst.numel() // 8))


@pytest.mark.parametrize('elem', sr.ELEMS)
def test_one_launch_over_a_table_of_segments(elem):
    dtype = sr.ELEM_DTYPES[elem]
    rows, checks = [], []
    for case in sr.PLANE_CASES:
        w, segs = segments_of(case, dtype)
        for buf, dst, want, mode, qpad in segs:
            rows.append((dst, w, mode, qpad))
            checks.append((case.name, mode, buf, dst, want))
    table = conv.PlaneTable(rows, dtype)
    assert table.nseg == len(rows) >= 4 and len({tuple(r[0].shape) for r in rows}) >= 4 and table.nblocks >= table.nseg
    launches = []
    call = _lib.call
    try:
        _lib.call = lambda name, *a, **k: launches.append(name) or call(name, *a, **k)
        table.run()
    finally:
        _lib.call = call
    torch.cuda.synchronize()
    assert launches == ['l2i_repack_planes_h8'], launches
    for name, mode, buf, dst, want in checks:
        guards_intact(buf)
        assert torch.equal(dst, want), '%s mode %d %s differs from its separate pack' % (name, mode, elem)
    print('rt16 repack_planes table %s: %d segments, %d slots, %d blocks' % (elem, table.nseg, table.slots, table.nblocks))


@pytest.mark.parametrize('elem', sr.ELEMS)
def test_repack_in_place_keeps_the_pointers(elem):
    dtype = sr.ELEM_DTYPES[elem]
    for name in ('c64x16_3x3_q16', 'c32x72_3x3_s2', 'stem'):
        case = PLANES[name]
        w0 = sr.plane_weight(case)
        hc = host_conv(case, w0, dtype, device=DEV)
        attrs = [a for a, _, _ in sr.plane_modes(case)]
        ptrs = [getattr(hc, a).data_ptr() for a in attrs]
        w1 = (sr.plane_weight(case, seed=1) * 0.5).to(DEV)
        want = host_conv(case, w1.cpu(), dtype)
        assert hc.repack_(w1) is hc
        torch.cuda.synchronize()
        assert [getattr(hc, a).data_ptr() for a in attrs] == ptrs
        for a in attrs:
            assert torch.equal(as_bits(getattr(hc, a)).cpu(), as_bits(getattr(want, a))), (name, a, elem)
        w1.mul_(2.0)                                          # an optimiser updates the master in place: the table built by the first call serves
        table = hc._table
        hc.repack_(w1)
        assert hc._table is table
        want2 = host_conv(case, w1.cpu(), dtype)
        for a in attrs:
            assert torch.equal(as_bits(getattr(hc, a)).cpu(), as_bits(getattr(want2, a))), (name, a, elem)


def test_refusals_launch_nothing():
    case = PLANES['c40x24_1x1']
    w, segs = segments_of(case, torch.float16)
    buf, dst, want, mode, qpad = segs[0]
    lib = _lib.load()
    table = conv.PlaneTable([(dst, w, mode, qpad)], torch.float16)
    before = buf.clone()
    for args in ((None, 1, 1), (_lib.ptr(table.table), 0, 1), (_lib.ptr(table.table), 2, 1)):
        rc = lib.l2i_repack_planes_h8_f16(*args, _lib.stream_ptr())
        assert rc == -1 and lib.l2i_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    with pytest.raises(_lib.L2IError):                        # the host side checks the rows the library cannot see
        conv.PlaneTable([(dst[:, :, :, :8], w, mode, qpad)], torch.float16)
    with pytest.raises(_lib.L2IError):
        conv.PlaneTable([(dst, w, mode, 24)], torch.float16)
    with pytest.raises(_lib.L2IError):
        conv.PlaneTable([(dst, w.cpu(), mode, qpad)], torch.float16)
