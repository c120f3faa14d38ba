"""l2i_sgd_guarded_f32 through the C ABI and optim.GuardedSGD on it: the arithmetic bit for bit against the float32 statement of
tests/test_invert_graph_cpu.py (sgd_numpy) and within 6 * 2^-23 * max|p| of torch.optim.SGD on the CPU; the guard, the scale rules and the refusals
as the header states them (the same words as l2i_adam_guarded_f32's)."""
import io

import numpy as np
import pytest
import torch

from tests.test_invert_graph_cpu import SGD_LRS, SGD_SIZES, SGD_STEPS, sgd_bound, sgd_case, sgd_numpy, torch_sgd

DEV = 'cuda'
pytestmark = pytest.mark.gpu
E_ARG = -1          # L2I_E_ARG


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _state():
    return torch.zeros(4, dtype=torch.int32, device=DEV)


def _scale():
    return torch.tensor([1.0, 1.0], device=DEV)


def sgd(p, g, buf, step, lr, momentum=0.9, check_self=1, state=None, scale=None, growth=2.0, backoff=0.5, interval=2000, max_scale=256.0, last=1, n=None,
        raw=False):
    """One call of the entry point.  ``raw``: the return code instead of an exception."""
    from latent2im_amd import _lib
    args = (_lib.fptr(p), _lib.fptr(g), _lib.fptr(buf), _lib.fptr(step), p.numel() if n is None else n, float(lr), float(momentum), int(check_self),
            _lib.ptr(state), _lib.ptr(scale), float(growth), float(backoff), int(interval), float(max_scale), int(last))
    if raw:
        return _lib.load().l2i_sgd_guarded_f32(*args, _lib.stream_ptr())
    return _lib.call('l2i_sgd_guarded_f32', *args)


@pytest.mark.parametrize('lr', SGD_LRS)
@pytest.mark.parametrize('n', SGD_SIZES)
def test_six_steps_are_the_float32_statement_bit_for_bit(n, lr):
    p0, grads = sgd_case(n, lr)
    want_p, want_buf, _ = sgd_numpy(p0, grads, lr, 0.9)
    ref_p, _ = torch_sgd(p0, grads, lr)
    p, buf, step, state = T(p0), T(np.full(n, 123.0)), torch.zeros((), device=DEV), _state()          # (the stale buffer must not leak into step 0)
    for g in grads:
        sgd(p, T(g), buf, step, lr, state=state)
    got_p, got_buf = p.cpu().numpy(), buf.cpu().numpy()
    dev, bound = float(np.abs(got_p.astype(np.float64) - ref_p).max()), sgd_bound(ref_p)
    print('n %d lr %g: differing words p %d buf %d; against torch.optim.SGD %.3e, bound %.3e' % (
        n, lr, int((got_p.view(np.uint32) != want_p.view(np.uint32)).sum()), int((got_buf.view(np.uint32) != want_buf.view(np.uint32)).sum()), dev, bound))
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    assert np.array_equal(got_buf.view(np.uint32), want_buf.view(np.uint32))
    assert float(step) == SGD_STEPS
    assert dev <= bound, (dev, bound)
    assert state.tolist() == [0, SGD_STEPS, 0, SGD_STEPS]          # six clean steps tracked and seen, none skipped, the flag down


@pytest.mark.parametrize('bad', [float('inf'), float('nan')], ids=['inf', 'nan'])
def test_a_nonfinite_gradient_skips_the_update_and_halves_the_scale(bad):
    n = 1025
    rs = np.random.RandomState(5)
    p0, buf0 = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    p, buf, step, state, scale = T(p0), T(buf0), torch.zeros((), device=DEV), _state(), _scale()
    state[1] = 5                                           # a tracker under way
    g = rs.randn(n).astype(np.float32)
    g[1024] = bad                                          # the ragged tail's only element
    sgd(p, T(g), buf, step, 1e-2, state=state, scale=scale)
    assert np.array_equal(p.cpu().numpy().view(np.uint32), p0.view(np.uint32))
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), buf0.view(np.uint32))
    assert float(step) == 0.0
    assert state.tolist() == [0, 0, 1, 1]                  # flag cleared by `last`, tracker back to 0, one skip, one step seen
    assert scale.tolist() == [0.5, 2.0]
    # a skipped FIRST iteration left the counter at 0: the next applied one initialises the buffer
    g2 = rs.randn(n).astype(np.float32)
    sgd(p, T(g2), buf, step, 1e-2, state=state, scale=scale)
    want_p, want_buf, _ = sgd_numpy(p0, [g2], 1e-2, 0.9)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), g2.view(np.uint32))
    assert np.array_equal(p.cpu().numpy().view(np.uint32), want_p.view(np.uint32))
    assert float(step) == 1.0 and state.tolist() == [0, 1, 1, 2] and scale.tolist() == [0.5, 2.0]


def test_scale_grows_after_interval_clean_steps_up_to_its_cap_and_may_be_absent():
    n = 64
    rs = np.random.RandomState(6)
    p, buf, step, state, scale = T(rs.randn(n)), T(np.zeros(n)), torch.zeros((), device=DEV), _state(), _scale()
    seen = []
    for _ in range(7):
        sgd(p, T(rs.randn(n)), buf, step, 1e-3, state=state, scale=scale, interval=3, max_scale=2.0)
        seen.append((scale.tolist(), state.tolist()[1]))
    # doubles after the third clean step; the cap 2.0 stops the second doubling (the tracker still restarts, as torch._amp_update_scale_'s does)
    assert [s[0][0] for s in seen] == [1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0], seen
    assert [s[1] for s in seen] == [1, 2, 0, 1, 2, 0, 1], seen
    assert seen[-1][0][1] == 0.5 and state.tolist() == [0, 1, 0, 7]
    # no scaler (bf16 / f32): scale == NULL runs, the words still count
    p0 = p.clone()
    st2 = _state()
    sgd(p, T(rs.randn(n)), buf, step, 1e-3, state=st2, scale=None, interval=0)
    assert st2.tolist() == [0, 1, 0, 1] and not torch.equal(p, p0) and float(step) == 8.0
    g = rs.randn(n).astype(np.float32)
    g[0] = np.inf
    p0 = p.clone()
    sgd(p, T(g), buf, step, 1e-3, state=st2, scale=None, interval=0)
    assert st2.tolist() == [0, 0, 1, 2] and torch.equal(p, p0) and float(step) == 8.0
    # last = 0 with check_self: the flag stays up for the next tensor, nothing is counted
    st3 = _state()
    sgd(p, T(g), buf, step, 1e-3, state=st3, scale=None, last=0)
    assert st3.tolist() == [1, 0, 0, 0] and torch.equal(p, p0)


def test_a_nonfinite_entry_in_the_second_tensor_stops_the_first_too():
    from latent2im_amd import _lib
    rs = np.random.RandomState(7)
    ns = (1500, 33)
    ps = [T(rs.randn(n)) for n in ns]
    bufs = [T(rs.randn(n)) for n in ns]
    steps = [torch.full((), 3.0, device=DEV) for _ in ns]
    keep = [t.clone() for t in ps + bufs + steps]
    gs = [rs.randn(n).astype(np.float32) for n in ns]
    gs[1][32] = np.nan
    gs = [T(g) for g in gs]
    state, scale = _state(), _scale()
    for g in gs:
        _lib.call('l2i_nonfinite_flag_f32', _lib.fptr(g), g.numel(), _lib.ptr(state))
    for i in range(2):
        sgd(ps[i], gs[i], bufs[i], steps[i], 1e-2, check_self=0, state=state, scale=scale, last=int(i == 1))
    assert all(torch.equal(a, b) for a, b in zip(ps + bufs + steps, keep))
    assert state.tolist() == [0, 0, 1, 1] and scale.tolist() == [0.5, 2.0]
    # the same two tensors with finite gradients move, from step 3: the momentum form
    gs = [T(rs.randn(n)) for n in ns]
    for g in gs:
        _lib.call('l2i_nonfinite_flag_f32', _lib.fptr(g), g.numel(), _lib.ptr(state))
    for i in range(2):
        sgd(ps[i], gs[i], bufs[i], steps[i], 1e-2, check_self=0, state=state, scale=scale, last=int(i == 1))
    for i in range(2):
        want_p, want_buf, _ = sgd_numpy(keep[i].cpu().numpy(), [gs[i].cpu().numpy()], 1e-2, 0.9, buf=keep[2 + i].cpu().numpy(), step=3)
        assert np.array_equal(ps[i].cpu().numpy().view(np.uint32), want_p.view(np.uint32))
        assert np.array_equal(bufs[i].cpu().numpy().view(np.uint32), want_buf.view(np.uint32))
        assert float(steps[i]) == 4.0
    assert state.tolist() == [0, 1, 1, 2]


def test_refusals_return_e_arg_and_write_nothing():
    n = 256
    sent = 77.25
    mk = lambda: torch.full((n,), sent, device=DEV)
    p, g, buf, scale = mk(), mk(), mk(), torch.full((2,), sent, device=DEV)
    step = torch.full((), sent, device=DEV)
    state = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    ok = dict(p=p, g=g, buf=buf, step=step, lr=1e-2, momentum=0.9, state=state, scale=scale)
    cases = [('null p', dict(p=None, n=n)), ('null g', dict(g=None)), ('null buf', dict(buf=None)), ('null step', dict(step=None)),
             ('null state', dict(state=None)), ('n = 0', dict(n=0)), ('n < 0', dict(n=-5)), ('momentum 1', dict(momentum=1.0)),
             ('momentum < 0', dict(momentum=-0.1)), ('momentum nan', dict(momentum=float('nan'))), ('lr < 0', dict(lr=-1e-3)),
             ('lr inf', dict(lr=float('inf'))), ('lr nan', dict(lr=float('nan'))), ('growth < 1', dict(growth=0.5)), ('backoff 0', dict(backoff=0.0)),
             ('backoff > 1', dict(backoff=1.5)), ('backoff nan', dict(backoff=float('nan')))]
    for what, kw in cases:
        a = dict(ok, **kw)
        a.setdefault('n', n)
        assert sgd(raw=True, **a) == E_ARG, what
    torch.cuda.synchronize()
    for t in (p, g, buf, scale, step):
        assert bool((t == sent).all())
    assert state.tolist() == [77] * 4
    # growth / backoff are read only with a scale: without one they are not refused
    state.zero_(), step.zero_()
    assert sgd(raw=True, **dict(ok, scale=None, growth=0.5, backoff=0.0)) == 0
    assert float(step) == 1.0


def _pair(shapes, rs, lr, **kw):
    from latent2im_amd import optim
    ps = [torch.nn.Parameter(T(rs.randn(*s))) for s in shapes]
    qs = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    return ps, qs, optim.GuardedSGD(ps, lr=lr, momentum=0.9, **kw), torch.optim.SGD(qs, lr=lr, momentum=0.9)


@pytest.mark.parametrize('shapes', [[(2, 8, 512)], [(64, 32), (32,)]], ids=['one', 'two'])
def test_guarded_sgd_class_against_torch_sgd(shapes):
    from latent2im_amd import optim
    rs = np.random.RandomState(8)
    sc = optim.LossScaler(dict(R=0, V=0, D=0, G=0), DEV, growth_interval=4, max_log2=1)
    ps, qs, opt, ref = _pair(shapes, rs, 1e-2, scaler=sc)
    for i in range(SGD_STEPS):
        for p, q in zip(ps, qs):
            g = (rs.randn(*p.shape) * 10.0 ** rs.uniform(-2, 2)).astype(np.float32)
            p.grad, q.grad = T(g), torch.from_numpy(g.copy())
        opt.step()
        ref.step()
    for p, q in zip(ps, qs):
        dev, bound = float((p.detach().cpu().double() - q.detach().double()).abs().max()), sgd_bound(q.detach().numpy())
        print('GuardedSGD %s against torch.optim.SGD: %.3e, bound %.3e' % (tuple(p.shape), dev, bound))
        assert dev <= bound
        st = opt.state[p]
        assert set(st) == {'momentum_buffer', 'step'} and st['step'].shape == () and st['step'].dtype == torch.float32 and st['step'].is_cuda
        assert float(st['step']) == SGD_STEPS
    assert sc.stats() == dict(scale=2.0, tracker=2, skipped=0, steps=SGD_STEPS)
    # an inf in the LAST tensor's gradient: nothing moves, the scale halves
    keep = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad = T(rs.randn(*p.shape))
    ps[-1].grad.view(-1)[-1] = float('inf')
    opt.step()
    assert all(torch.equal(p.detach(), k) for p, k in zip(ps, keep))
    assert sc.stats() == dict(scale=1.0, tracker=0, skipped=1, steps=SGD_STEPS + 1)


def test_guarded_sgd_state_dict_round_trip_and_torch_sgd_dicts():
    from latent2im_amd import optim
    rs = np.random.RandomState(9)
    ps, qs, opt, ref = _pair([(3, 8, 512)], rs, 1e-3)
    gs = [(rs.randn(3, 8, 512)).astype(np.float32) for _ in range(4)]
    for g in gs[:2]:
        ps[0].grad, qs[0].grad = T(g), torch.from_numpy(g.copy())
        opt.step()
        ref.step()
    # round trip: a second GuardedSGD that loads the first one's dict goes on exactly as the first
    p2 = torch.nn.Parameter(ps[0].detach().clone())
    opt2 = optim.GuardedSGD([p2], lr=1e-3, momentum=0.9)
    f = io.BytesIO()
    torch.save(opt.state_dict(), f)                        # through a file: load_state_dict alone would share the first one's tensors
    f.seek(0)
    opt2.load_state_dict(torch.load(f))
    assert float(opt2.state[p2]['step']) == 2.0 and torch.equal(opt2.state[p2]['momentum_buffer'], opt.state[ps[0]]['momentum_buffer'])
    # a dict saved by torch.optim.SGD (a buffer, no step): step becomes 1 — the momentum form, not a fresh buffer
    p3 = torch.nn.Parameter(T(qs[0].detach().numpy()))
    opt3 = optim.GuardedSGD([p3], lr=1e-3, momentum=0.9)
    opt3.load_state_dict(ref.state_dict())
    assert 'step' not in opt3.state[p3]
    for g in gs[2:]:
        for p, o in ((ps[0], opt), (p2, opt2), (p3, opt3)):
            p.grad = T(g)
            o.step()
        qs[0].grad = torch.from_numpy(g.copy())
        ref.step()
    assert torch.equal(p2.detach(), ps[0].detach())
    assert float(opt3.state[p3]['step']) == 3.0 and opt3.state[p3]['step'].is_cuda
    bound = sgd_bound(qs[0].detach().numpy())
    for p in (ps[0], p3):
        assert float((p.detach().cpu().double() - qs[0].detach().double()).abs().max()) <= bound


def test_guarded_sgd_input_checks():
    from latent2im_amd import _lib, optim
    p = torch.nn.Parameter(torch.zeros(8, device=DEV))
    p.grad = torch.ones(8, device=DEV)
    for kw in (dict(nesterov=True), dict(dampening=0.5), dict(weight_decay=0.1), dict(maximize=True)):
        opt = optim.GuardedSGD([p], lr=0.1, momentum=0.9)
        opt.param_groups[0].update(kw)
        with pytest.raises(NotImplementedError):
            opt.step()
    with pytest.raises(NotImplementedError):
        optim.GuardedSGD([p], lr=0.1, momentum=0.9).step(lambda: 0.0)
    assert float(p.sum()) == 0.0
    h = torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.float16))
    h.grad = torch.ones(8, device=DEV, dtype=torch.float16)
    with pytest.raises(_lib.L2IError):
        optim.GuardedSGD([h], lr=0.1, momentum=0.9).step()
    c = torch.nn.Parameter(torch.zeros(8))
    c.grad = torch.ones(8)
    with pytest.raises(_lib.L2IError):
        optim.GuardedSGD([c], lr=0.1, momentum=0.9).step()
