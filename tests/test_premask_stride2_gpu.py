"""The leaky-ReLU / ReLU mask of a stride-2 conv's incoming gradient applied by the launch that PRODUCES the gradient (the discriminator's dual-output
FIR, l2i_upfirdn2d_dual_f32; ResNet-50's out_mask on c3's gradient GEMM) instead of the transposed conv's prologue (in_mask).

Launch level: the in_mask launch on g against the unmasked launch on g * m, both against F.conv_transpose2d in float64 with the bound
tests/test_convt_poly_gpu.py holds these kernels to (close(y, ref, 1e-4, 2e-5)), on the direct kernel (tile_hint 9) and the 25-product kernel
(tile_hint 10); whether the two direct launches are bit-equal is printed, not asserted.  Network level: image gradients of a size-256 discriminator
(batch 2: the staged-FIR dual launches and the rule rows 256->128 @128, 512->256 @64, 512->512 @32) and of ResNet-50 on 2x3x128x128 with the switch on
and off against the float64 oracle, at the bar of tests/test_networks_gpu.py (grad_ok).  A size-256 discriminator has no block behind a compact skip
path, so the zero-insertion FIR's second output is not reached there (tests/test_fir_dual_gpu.py holds it at launch level); one size-512 backward,
switch on against off at the same bar, runs it inside the network.  Schedule: the ordered entry points of one discriminator backward."""
import ctypes

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, conv, discriminator, regressor, synth
from latent2im_amd import kernels as K
from latent2im_amd.discriminator import Discriminator
from latent2im_amd.regressor import ResNet50
from oracle import nets as onets
from oracle import sg2
from oracle import step as ostep
from tests.test_convt_poly_gpu import close, reference
from tests.test_networks_gpu import grad_ok, relmax

pytestmark = pytest.mark.gpu
DEV = 'cuda'
POLY, DIRECT = _lib.CONVT_HINT_POLY, _lib.CONVT_HINT_DIRECT
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


# ---- launch level ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vals', [(1.0, 0.2), (1.0, 0.0)])
@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('shape', [(8, 32, 32, 32), (4, 20, 33, 40)])
def test_unmasked_launch_on_the_premasked_gradient(shape, pad, vals):
    cin, cout, h, w_ = shape                                            # of the launch: the conv's Cout and Cin
    rs = np.random.RandomState(cin + cout + h + pad)
    wc = torch.tensor(rs.randn(cin, cout, 3, 3) / np.sqrt(cin * 9), dtype=torch.float32)
    fc = conv.FrozenConv2d(wc, 2, pad, device=DEV)
    assert fc.bwd_fused is not None and fc.bwd_fused.poly_src is not None
    x = torch.tensor(rs.randn(1, cin, h, w_), dtype=torch.float32).to(DEV)
    act = torch.tensor(rs.randn(1, cin, h, w_), dtype=torch.float32)
    act[:, :, 0, :4] = 0.0                                              # exact zeros take the negative value
    act = act.to(DEV)
    kf = torch.tensor(synth.fir_kernel(), dtype=torch.float32).to(DEV)
    # g and g * m as the discriminator's backward produces them: one FIR launch, two outputs; the ReLU pair also through l2i_relu_mask_f32
    g, gm = K.upfirdn2d(x, kf, pad=(2, 1, 2, 1), mask2=act, mask2_vals=vals)
    m = torch.where(act > 0, torch.tensor(vals[0], device=DEV), torch.tensor(vals[1], device=DEV))
    assert torch.equal(gm, g * m)
    if vals == (1.0, 0.0):
        assert torch.equal(K.relu_mask(g, act), gm)
    extra = 3 if pad == 0 else 0
    oh, ow = 2 * h + 1 - 2 * pad + extra, 2 * w_ + 1 - 2 * pad + extra
    ref = reference(g.double().cpu() * m.double().cpu(), wc.transpose(0, 1), pad, oh, ow)

    def run(hint, gy, **kw):
        out = torch.full((1, cout, oh, ow), float('nan'), device=DEV)
        fc.dgrad(gy, (oh, ow), out=out, tile_hint=hint, **kw)
        torch.cuda.synchronize()
        return out
    for hint, name in ((DIRECT, 'direct'), (POLY, 'poly')):
        y_masked = run(hint, g, in_mask=act, mask=vals)
        y_plain = run(hint, gm)
        print('%s pad %d %s %s: in_mask launch and unmasked launch on g*m bit-equal: %s; max err against float64 %.3e / %.3e (max|ref| %.3e)' % (
            shape, pad, vals, name, torch.equal(y_masked, y_plain), (y_masked.double().cpu() - ref).abs().max().item(),
            (y_plain.double().cpu() - ref).abs().max().item(), ref.abs().max().item()))
        close(y_masked, ref, 1e-4, 2e-5)
        close(y_plain, ref, 1e-4, 2e-5)


# ---- network level -----------------------------------------------------------------------------------------------------------------------------------
def _d_grad(D, x, premask):
    old, discriminator.PREMASK = discriminator.PREMASK, premask
    try:
        xg = x.clone().requires_grad_(True)
        d = D(xg)
        d.sum().backward()
        torch.cuda.synchronize()
        return d.detach(), xg.grad
    finally:
        discriminator.PREMASK = old


@pytest.fixture(scope='module')
def disc256():
    st = synth.discriminator_state(256, seed=200)
    D = Discriminator(st, 256, device=DEV)
    x = np.random.RandomState(256).randn(2, 3, 256, 256)
    xo = T(x).requires_grad_(True)
    do = sg2.discriminator_forward(ostep.to_torch(st, torch.float64), xo)
    go, = torch.autograd.grad(do.sum(), xo)
    return D, T(x).float().to(DEV), do.detach(), go


def test_discriminator_gradient_with_the_switch_on_and_off(disc256):
    D, x, do, go = disc256
    assert discriminator.PREMASK is True
    for premask in (True, False):
        d, g = _d_grad(D, x, premask)
        m = float(go.abs().max())
        e = (g.cpu().double() - go).abs()
        print('discriminator 256 batch 2, PREMASK %s: image gradient against float64: largest deviation %.3e of max, %.4f %% of the entries beyond 2e-3 of max'
              % (premask, float(e.max()) / m, 100.0 * float((e > 2e-3 * m).double().mean())))
        np.testing.assert_allclose(d.cpu().double().numpy(), do.numpy(), rtol=1e-3, atol=1e-4)
        grad_ok(g, go)


def test_discriminator_512_backward_on_equals_off():
    """A size-512 backward: the block at 256 sits behind the compact skip path, so its gradient comes from the zero-insertion FIR's dual launch.  The masks
    are the saved activations in both forms, so the two differ by fp32 summation order alone; held to the oracle bar all the same."""
    D = Discriminator(synth.discriminator_state(512, seed=200), 512, device=DEV)
    x = T(np.random.RandomState(512).randn(1, 3, 512, 512)).float().to(DEV)
    on = []
    rec = _recorded(lambda: on.append(_d_grad(D, x, True)))
    assert ('l2i_upfirdn2d_dual_f32', 2) in rec and ('l2i_upfirdn2d_dual_f32', 1) in rec
    g_on = on[0][1]
    _, g_off = _d_grad(D, x, False)
    print('discriminator 512 batch 1: PREMASK on against off, largest deviation %.3e of max' % relmax(g_on, g_off))
    grad_ok(g_on, g_off)


def test_resnet50_gradient_with_the_stride2_switch_on_and_off():
    st = synth.resnet50_state(seed=300)
    net = ResNet50(st, device=DEV)
    rs = np.random.RandomState(128)
    x, gy = rs.randn(2, 3, 128, 128), rs.randn(2, 40)
    xo = T(x).requires_grad_(True)
    yo = onets.resnet50_forward(ostep.to_torch(st, torch.float64), xo)
    go, = torch.autograd.grad(yo, xo, T(gy))
    assert regressor.PREMASK_STRIDE2 is True
    old = regressor.PREMASK_STRIDE2
    try:
        for on in (True, False):
            regressor.PREMASK_STRIDE2 = on
            xg = T(x).float().to(DEV).requires_grad_(True)
            rec = _recorded(lambda: net(xg).backward(T(gy).float().to(DEV)))
            masked = [r for r in rec if r[0] == 'l2i_conv_transpose2d_f32' and r[1] == 3 and r[4]]
            assert (len(masked) == 0) if on else (len(masked) == 3), rec
            m = float(go.abs().max())
            e = (xg.grad.cpu().double() - go).abs()
            print('ResNet-50 2x3x128x128, stride-2 premask %s: image gradient against float64: largest deviation %.3e of max, %.4f %% of the entries beyond 2e-3 of max'
                  % (on, float(e.max()) / m, 100.0 * float((e > 2e-3 * m).double().mean())))
            grad_ok(xg.grad, go)
    finally:
        regressor.PREMASK_STRIDE2 = old


# ---- schedule ----------------------------------------------------------------------------------------------------------------------------------------
def _recorded(fn):
    """The entry points ``fn`` calls, in order: (name, up_x) of a FIR launch; (name, KH, W, family, has in_mask) of a transposed launch."""
    rec, call = [], _lib.call

    def spy(name, *args, **kw):
        if name == 'l2i_conv_transpose2d_f32':
            p = args[0]
            fam = _lib.load().l2i_conv_transpose2d_family(ctypes.byref(p)) if _lib.has('l2i_conv_transpose2d_family') else None
            rec.append((name, p.KH, p.W, fam, bool(p.in_mask)))
        elif name.startswith('l2i_upfirdn2d_dual'):
            rec.append((name, args[12]))
        else:
            rec.append((name,))
        return call(name, *args, **kw)
    _lib.call = spy
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.call = call
    return rec


def test_discriminator_backward_schedule(disc256):
    D, x, _, _ = disc256
    xg = x.clone().requires_grad_(True)
    d = D(xg)
    rec = _recorded(lambda: d.sum().backward())
    tr = [(i, r) for i, r in enumerate(rec) if r[0] == 'l2i_conv_transpose2d_f32' and r[1] == 3]
    # gradient maps of the six blocks of a size-256 body, deepest first; the deepest is fed by the tail, the next two are under 32 wide
    assert [r[2] for _, r in tr] == [4, 8, 16, 32, 64, 128]
    assert [r[4] for _, r in tr] == [True, True, True, False, False, False]
    assert all(r[3] == _lib.TFAMILY_POLY for _, r in tr[3:])                      # 512->512 @32, 512->256 @64, 256->128 @128: the rule rows
    for i, r in tr[3:]:                                                           # each is fed by a dual FIR launch that ran before it, after the previous conv
        prev = [j for j, q in enumerate(rec[:i]) if q[0] == 'l2i_conv_transpose2d_f32' and q[1] == 3][-1]
        assert any(q[0] == 'l2i_upfirdn2d_dual_f32' for q in rec[prev:i]), rec[prev:i]
    assert sum(q[0] == 'l2i_upfirdn2d_dual_f32' for q in rec) == 3
