"""The host side of the replayed inversion (`BP.py --hipgraph`, invert.Inverter(capture=True)) and of l2i_sgd_guarded_f32, and the float32 model
of the momentum-SGD sequence that tests/test_sgd_guarded_gpu.py holds the kernel to bit for bit, itself held to torch.optim.SGD here."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SGD_SIZES = (1, 1023, 1025, 4096 + 7)          # one lane, one short of / one past the block's 1024 threads, several rounds with a ragged tail
SGD_LRS = (1e-2, 1e-3)
SGD_STEPS = 6


def sgd_numpy(p, grads, lr, momentum, buf=None, step=0):
    """include/l2i.h's statement of l2i_sgd_guarded_f32 in numpy float32, every product and sum rounded on its own: step 0: buf = g; afterwards
    buf = fl(fl(momentum * buf) + g); p = fl(p - fl(lr * buf)).  Returns (p, buf, step)."""
    f = np.float32
    p = np.asarray(p, f).copy()
    buf = None if buf is None else np.asarray(buf, f).copy()
    lr, momentum = f(lr), f(momentum)
    for g in grads:
        g = np.asarray(g, f)
        if step == 0:
            buf = g.copy()
        else:
            mb = (momentum * buf).astype(f)
            buf = (mb + g).astype(f)
        d = (lr * buf).astype(f)
        p = (p - d).astype(f)
        step += 1
    return p, buf, step


def sgd_case(n, lr):
    """(start, six gradients) of one case: magnitudes from 1e-2 to 1e2, seeded by the case."""
    rs = np.random.RandomState(1000 + n + int(round(1.0 / lr)))
    p0 = rs.randn(n).astype(np.float32)
    mags = 10.0 ** np.linspace(-2.0, 2.0, SGD_STEPS)
    rs.shuffle(mags)
    return p0, [(rs.randn(n) * m).astype(np.float32) for m in mags]


def torch_sgd(p0, grads, lr, momentum=0.9):
    """torch.optim.SGD(lr, momentum) on the CPU -> (p, momentum_buffer) as numpy."""
    p = torch.nn.Parameter(torch.from_numpy(np.array(p0, np.float32)))
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum)
    for g in grads:
        p.grad = torch.from_numpy(np.array(g, np.float32))
        opt.step()
    return p.detach().numpy(), opt.state[p]['momentum_buffer'].numpy()


def sgd_bound(p):
    """Six steps, per step one rounding of the product and one of the sum where torch's fused multiply-add may differ: 6 * 2^-23 * max|p|."""
    return SGD_STEPS * 2.0 ** -23 * float(np.abs(p).max())


@pytest.mark.parametrize('lr', SGD_LRS)
@pytest.mark.parametrize('n', SGD_SIZES)
def test_sgd_model_against_torch_sgd(n, lr):
    p0, grads = sgd_case(n, lr)
    want, _ = torch_sgd(p0, grads, lr)
    got, buf, step = sgd_numpy(p0, grads, lr, 0.9)
    dev, bound = float(np.abs(got.astype(np.float64) - want).max()), sgd_bound(want)
    print('n %d lr %g: model against torch.optim.SGD %.3e, bound %.3e (%.2f of it)' % (n, lr, dev, bound, dev / bound))
    assert step == SGD_STEPS and buf.dtype == np.float32 and got.dtype == np.float32
    assert dev <= bound, (dev, bound)


def test_sgd_model_first_step_sets_the_buffer():
    g = np.array([3.0, -2.0], np.float32)
    p, buf, step = sgd_numpy(np.zeros(2, np.float32), [g], 0.5, 0.9, buf=np.full(2, 7.0, np.float32), step=0)
    assert np.array_equal(buf, g) and np.array_equal(p, -0.5 * g) and step == 1
    p, buf, step = sgd_numpy(p, [g], 0.5, 0.9, buf=buf, step=step)
    assert np.array_equal(buf, (np.float32(0.9) * g).astype(np.float32) + g) and step == 2


def test_parser_takes_hipgraph_and_defaults_it_off():
    from latent2im_amd import bp
    p = bp.build_parser()
    assert p.parse_args(['--path', 'x']).hipgraph is False
    assert p.parse_args(['--path', 'x', '--hipgraph']).hipgraph is True
    assert p.parse_args(['--hipgraph', '--precision', 'f16', '--optimizer', 'GD']).hipgraph is True
    help_text = p.format_help()
    assert '--hipgraph' in help_text and 'eager loop' in help_text


def test_inverter_signature_has_capture_false():
    from latent2im_amd.invert import Inverter
    par = inspect.signature(Inverter.__init__).parameters
    assert 'capture' in par and par['capture'].default is False
    assert list(par)[:7] == ['self', 'gen', 'vgg', 'lr', 'optim', 'n_mean_latent', 'batch']          # the eager call shape is unchanged


def test_sgd_entry_is_declared_and_bound():
    import ctypes
    from latent2im_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'l2i.h')).read()
    m = re.search(r'int l2i_sgd_guarded_f32\(([^)]*)\);', hdr)
    assert m, 'l2i_sgd_guarded_f32 is not declared in include/l2i.h'
    names = [a.split()[-1].lstrip('*') for a in m.group(1).split(',')]
    assert names == ['p', 'g', 'buf', 'step', 'n', 'lr', 'momentum', 'check_self', 'state', 'scale', 'growth', 'backoff', 'interval', 'max_scale',
                     'last', 'stream']
    assert 'l2i_sgd_guarded_f32' in _lib.EXPORTS
    res, args = _lib._SIGNATURES['l2i_sgd_guarded_f32']
    assert res is ctypes.c_int32 and len(args) == 16
    P, F, I, L = ctypes.c_void_p, ctypes.c_float, ctypes.c_int32, ctypes.c_int64
    assert args == [P, P, P, P, L, F, F, I, P, P, F, F, I, F, I, P]
    assert _lib.ABI_VERSION == 12 and '#define L2I_ABI_VERSION 12' in hdr
    adam = re.search(r'int l2i_adam_guarded_f32\(([^)]*)\);', hdr)                   # the existing signature is kept
    assert adam and len(adam.group(1).split(',')) == 19 and len(_lib._SIGNATURES['l2i_adam_guarded_f32'][1]) == 19


def test_guarded_sgd_refuses_what_the_kernel_does_not_do():
    """Raised before any GPU call: the checks run on CPU parameters too."""
    from latent2im_amd import optim
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    for kw in (dict(nesterov=True), dict(dampening=0.5), dict(weight_decay=0.1), dict(maximize=True)):
        opt = optim.GuardedSGD([p], lr=0.1, momentum=0.9)
        opt.param_groups[0].update(kw)
        with pytest.raises(NotImplementedError):
            opt.step()
    with pytest.raises(NotImplementedError):
        optim.GuardedSGD([p], lr=0.1, momentum=0.9).step(lambda: 0.0)
