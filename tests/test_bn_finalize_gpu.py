"""l2i_bn_finalize_f32 / l2i_bn_bwd_finalize_f32 against the model of tests/regtrain_ref.py and against the torch expressions of
regressor_train._BN they replace: exact conversions bit for bit, invstd within 1 ulp, the rest within the bounds the model derives from that."""
import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from latent2im_amd import regressor_train as RT
from tests import regtrain_ref as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = lambda a: torch.as_tensor(a).to(DEV)


def _case(c, n, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, c) * 3 + rs.randn(c)
    x[:, 0] = 1.25                                                       # a constant channel: the variance clamps at (or rounds to) zero
    x = x.astype(np.float32).astype(np.float64)
    return dict(s=x.sum(0), q=(x * x).sum(0), weight=rs.randn(c).astype(np.float32), bias=rs.randn(c).astype(np.float32),
                rm=rs.randn(c).astype(np.float32), rv=(rs.rand(c) + 0.5).astype(np.float32))


@pytest.mark.parametrize('c,n', [(1, 1), (64, 2048), (100, 37), (100, 1), (300, 5)])
def test_finalize_against_model_and_todays_expression(c, n):
    k = _case(c, n, 10 + c + n)
    ref = rr.bn_finalize(k['s'], k['q'], n, k['weight'], k['bias'], k['rm'], k['rv'])
    bound = rr.bn_finalize_bounds(ref, k['rv'])
    s, q, weight, bias = T(k['s']), T(k['q']), T(k['weight']), T(k['bias'])
    rm, rv, nbt = T(k['rm']).clone(), T(k['rv']).clone(), torch.full((), 6, dtype=torch.long, device=DEV)
    out = {name: torch.full((c,), float('nan'), device=DEV) for name in ('mean', 'invstd', 'scale', 'shift')}
    _lib.call('l2i_bn_finalize_f32', *[_lib.fptr(out[name]) for name in ('mean', 'invstd', 'scale', 'shift')], _lib.fptr(rm), _lib.fptr(rv), _lib.ptr(nbt),
              _lib.ptr(s), _lib.ptr(q), _lib.fptr(weight), _lib.fptr(bias), n, c, RT.BN_EPS, RT.BN_MOMENTUM)
    out.update(running_mean=rm, running_var=rv)
    # today's expression (regressor_train._BN.forward), on the device
    mean64 = s / n
    var64 = (q / n - mean64 * mean64).clamp_(min=0.0)
    today = dict(mean=mean64.float(), invstd=torch.rsqrt(var64 + RT.BN_EPS).float())
    today['running_mean'] = T(k['rm']).clone().mul_(1 - RT.BN_MOMENTUM).add_(today['mean'], alpha=RT.BN_MOMENTUM)
    today['running_var'] = T(k['rv']).clone().mul_(1 - RT.BN_MOMENTUM).add_((var64 * (n / max(n - 1, 1))).float(), alpha=RT.BN_MOMENTUM)
    today['scale'] = weight * today['invstd']
    today['shift'] = bias - today['mean'] * today['scale']
    assert int(nbt) == 7
    assert float(ref['invstd'][0]) > 300.0                              # the constant channel: invstd = 1 / sqrt(eps) (= 316.2) or close to it
    for side, vals in (('kernel', out), ('today', today)):
        v = {name: t.cpu().numpy() for name, t in vals.items()}
        assert v['mean'].tobytes() == ref['mean'].tobytes(), side
        d = rr.ulp_distance(v['invstd'], ref['invstd'])
        assert d.max() <= 1, (side, int(d.max()))
        for name in ('scale', 'shift', 'running_mean', 'running_var'):
            err = np.abs(v[name].astype(np.float64) - ref[name].astype(np.float64))
            print('%s %s: worst error / bound %.3f' % (side, name, float((err / bound[name]).max())))
            assert (err <= bound[name]).all(), (side, name, float((err / bound[name]).max()))
    # with the model's own invstd every float32 step is a single stated operation: the kernel equals the model wherever invstd does
    same = out['invstd'].cpu().numpy().view(np.int32) == ref['invstd'].view(np.int32)
    for name in ('scale', 'shift', 'running_mean', 'running_var'):
        assert (out[name].cpu().numpy().view(np.int32)[same] == ref[name].view(np.int32)[same]).all(), name


def test_optional_outputs_may_be_null_and_bad_arguments_are_refused():
    k = _case(8, 4, 1)
    s, q, weight, bias = T(k['s']), T(k['q']), T(k['weight']), T(k['bias'])
    o = [torch.zeros(8, device=DEV) for _ in range(4)]
    _lib.call('l2i_bn_finalize_f32', *[_lib.fptr(t) for t in o], None, None, None, _lib.ptr(s), _lib.ptr(q), _lib.fptr(weight), _lib.fptr(bias), 4, 8, 1e-5, 0.1)
    ref = rr.bn_finalize(k['s'], k['q'], 4, k['weight'], k['bias'], k['rm'], k['rv'])
    assert o[0].cpu().numpy().tobytes() == ref['mean'].tobytes()
    lib = _lib.load()
    args = [_lib.fptr(t) for t in o] + [None, None, None, _lib.ptr(s), _lib.ptr(q), _lib.fptr(weight), _lib.fptr(bias)]
    assert lib.l2i_bn_finalize_f32(*args, 0, 8, 1e-5, 0.1, _lib.stream_ptr()) == -1
    assert lib.l2i_bn_finalize_f32(*args, 4, 8, -1.0, 0.1, _lib.stream_ptr()) == -1
    assert lib.l2i_bn_finalize_f32(*([None] + args[1:]), 4, 8, 1e-5, 0.1, _lib.stream_ptr()) == -1
    assert lib.l2i_bn_bwd_finalize_f32(*[_lib.fptr(t) for t in o], _lib.ptr(s), None, 4, 8, _lib.stream_ptr()) == -1
    assert lib.l2i_bn_bwd_finalize_f32(*[_lib.fptr(t) for t in o], _lib.ptr(s), _lib.ptr(q), 4, 0, _lib.stream_ptr()) == -1


@pytest.mark.parametrize('c,n', [(1, 1), (64, 2048), (100, 37)])
def test_bwd_finalize_is_exact(c, n):
    rs = np.random.RandomState(c + n)
    s, q = rs.randn(c) * 10, rs.randn(c) * 1e-3
    s[0] = 0.0
    ref = rr.bn_bwd_finalize(s, q, n)
    out = [torch.full((c,), float('nan'), device=DEV) for _ in range(4)]
    sd, qd = T(s), T(q)
    _lib.call('l2i_bn_bwd_finalize_f32', *[_lib.fptr(t) for t in out], _lib.ptr(sd), _lib.ptr(qd), n, c)
    today = (sd.float(), qd.float(), (sd / n).float(), (qd / n).float())                     # regressor_train._BN.backward
    for name, got, was in zip(('d_bias', 'd_weight', 'm_dy', 'm_dyxh'), out, today):
        assert got.cpu().numpy().tobytes() == ref[name].tobytes() == was.cpu().numpy().tobytes(), name
