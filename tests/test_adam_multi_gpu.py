"""l2i_nonfinite_flag_multi_f32 + l2i_adam_guarded_multi_f32 (csrc/l2i_optim.hip) and GuardedAdam's multi-tensor step on the GPU: bit for bit
against the single-tensor entry points, against torch.optim.Adam, the guard, the chunking, the launch budget, capture, argument errors.

Tensor sizes: a block covers 4096 elements of one tensor (MB in l2i_optim.hip), so 1, 63, 4096, 4097 and 3 * 4096 + 3 are one lane, less than a
wave, one block exactly, one block and one element, several blocks and a scalar tail.  Two more start 4 bytes off a 16-byte boundary: one with all
four operands off by the same amount (scalar head, 16-byte body, scalar tail) and one with the parameter alone off (element by element).  Every
operand lives inside a buffer with sentinels around it."""
import ctypes

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, optim
from tests import adam_multi_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MB = 4096
#        n, element offset of (p, g, m, v) inside their 16-byte-aligned buffers
CASES = ((1, (4, 4, 4, 4)), (63, (4, 4, 4, 4)), (MB, (4, 4, 4, 4)), (MB + 1, (4, 4, 4, 4)), (3 * MB + 3, (4, 4, 4, 4)), (MB + 6, (5, 5, 5, 5)),
         (2 * MB + 2, (5, 4, 4, 4)))
STEPS0 = (0.0, 3.0, 1.0, 7.0, 2.0, 5.0, 11.0)
HP = dict(lr=1e-3, beta1=0.5, beta2=0.99, eps=1e-8)
SENTINEL = 12345.0
PAD = 12


class Tensors:
    """The operands of a step: p, g, m, v views inside sentinel-padded buffers, one float32 step counter a tensor, the guard words, the scale."""

    def __init__(self, seed, cases=CASES, steps0=STEPS0, scale_p=0.05):
        rs = np.random.RandomState(seed)
        self.rows, self.bufs = [], []
        for (n, offs), s0 in zip(cases, steps0):
            row = {}
            for key, off in zip('pgmv', offs):
                buf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV)
                view = buf[off:off + n]
                assert view.data_ptr() % 16 == (4 * off) % 16
                if key == 'p':
                    view.copy_(torch.from_numpy((rs.standard_normal(n) * scale_p).astype(np.float32)))
                elif key == 'm':
                    view.copy_(torch.from_numpy((rs.standard_normal(n) * 0.01 * (s0 > 0)).astype(np.float32)))
                elif key == 'v':
                    view.copy_(torch.from_numpy((rs.standard_normal(n) ** 2 * 1e-4 * (s0 > 0)).astype(np.float32)))
                row[key] = view
                self.bufs.append((buf, off, n))
            row['step'] = torch.full((), s0, device=DEV)
            self.rows.append(row)
        self.state = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.scale = torch.tensor([1.0, 1.0], device=DEV)

    def set_grads(self, rs, mag=None):
        for r in self.rows:
            n = r['g'].numel()
            r['g'].copy_(torch.from_numpy((rs.standard_normal(n) * (10.0 ** rs.uniform(-4, 0) if mag is None else mag)).astype(np.float32)))

    def sentinels_intact(self):
        return all(bool((b[:off] == SENTINEL).all()) and bool((b[off + n:] == SENTINEL).all()) for b, off, n in self.bufs)

    def snapshot(self):
        return ([{k: r[k].clone() for k in ('p', 'm', 'v', 'step')} for r in self.rows], self.state.clone(), self.scale.clone())

    def table(self, rows=None):
        rows = self.rows if rows is None else rows
        return (_lib.AdamTensor * len(rows))(*[_lib.AdamTensor(r['p'].data_ptr(), r['g'].data_ptr(), r['m'].data_ptr(), r['v'].data_ptr(), r['step'].data_ptr(),
                                                               r['p'].numel()) for r in rows]), len(rows)


GUARD = dict(growth=2.0, backoff=0.5, interval=2000, max_scale=256.0)


def step_new(t, guard=GUARD, hp=HP):
    table, count = t.table()
    _lib.call('l2i_nonfinite_flag_multi_f32', table, count, _lib.ptr(t.state))
    _lib.call('l2i_adam_guarded_multi_f32', table, count, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], _lib.ptr(t.state), _lib.ptr(t.scale),
              guard['growth'], guard['backoff'], guard['interval'], guard['max_scale'], 1)


def step_old(t, guard=GUARD, hp=HP):
    """The per-tensor path: a flag launch a gradient, then one single-block update a tensor, the last one advancing the scale state.  The
    single-tensor kernel takes any 4-byte-aligned pointer."""
    for r in t.rows:
        _lib.call('l2i_nonfinite_flag_f32', r['g'].data_ptr(), r['g'].numel(), _lib.ptr(t.state))
    for i, r in enumerate(t.rows):
        _lib.call('l2i_adam_guarded_f32', r['p'].data_ptr(), r['g'].data_ptr(), r['m'].data_ptr(), r['v'].data_ptr(), r['step'].data_ptr(), r['p'].numel(),
                  hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], 0, _lib.ptr(t.state), _lib.ptr(t.scale), guard['growth'], guard['backoff'],
                  guard['interval'], guard['max_scale'], 1 if i == len(t.rows) - 1 else 0)


def same(a, b):
    (ra, sa, ca), (rb, sb, cb) = a, b
    return all(torch.equal(x[k], y[k]) for x, y in zip(ra, rb) for k in x) and torch.equal(sa, sb) and torch.equal(ca, cb)


def test_bit_equal_to_the_single_tensor_path_over_three_steps():
    new, old = Tensors(0), Tensors(0)
    assert same(new.snapshot(), old.snapshot())
    ra, rb = np.random.RandomState(10), np.random.RandomState(10)
    for it in range(3):
        new.set_grads(ra)
        old.set_grads(rb)
        step_new(new)
        step_old(old)
        torch.cuda.synchronize()
        assert same(new.snapshot(), old.snapshot()), it
    assert [float(r['step']) for r in new.rows] == [s + 3 for s in STEPS0]
    assert new.state.tolist() == [0, 3, 0, 3] and new.scale.tolist() == [1.0, 1.0]
    assert new.sentinels_intact() and old.sentinels_intact()


def test_six_steps_against_torch_adam():
    """Parameters at the MLP walk's own scale (tests/emu.py::seeded_state: 1 / sqrt(512) for the matrices, 0.1 for the biases), counters at 0 as
    torch's: the largest difference of any parameter under 1e-6, the bar tests/test_h8_gpu.py holds the guarded Adam to."""
    t = Tensors(1, steps0=(0.0,) * len(CASES))
    ps = [torch.nn.Parameter(r['p'].detach().cpu().clone()) for r in t.rows]
    ref = torch.optim.Adam(ps, lr=HP['lr'], betas=(HP['beta1'], HP['beta2']), eps=HP['eps'])
    rs = np.random.RandomState(11)
    for it in range(6):
        t.set_grads(rs)
        for p, r in zip(ps, t.rows):
            p.grad = r['g'].detach().cpu().clone()
        ref.step()
        step_new(t)
    torch.cuda.synchronize()
    errs = [float((r['p'].cpu() - p.detach()).abs().max()) for r, p in zip(t.rows, ps)]
    print(errs)
    assert max(errs) < 1e-6, errs
    assert all(float(r['step']) == 6.0 for r in t.rows) and t.sentinels_intact()


def test_guard_skips_every_tensor_and_the_scale_state_follows_the_model():
    """An inf in the last element of the last tensor, then a NaN in the first element of the first: nothing moves, no counter advances, SKIPPED + 1,
    the scale halves, FOUND is cleared; the next clean steps update, and growth after interval = 2 clean steps stops at max_scale.  The guard words
    and the scale after every step are the numpy model's (tests/adam_multi_ref.py)."""
    guard = dict(growth=2.0, backoff=0.5, interval=2, max_scale=1.0)
    t = Tensors(2)
    m_state, m_scale = R.new_state()
    m_rows = [dict(p=r['p'].cpu().numpy().copy(), m=r['m'].cpu().numpy().copy(), v=r['v'].cpu().numpy().copy(), step=np.float32(s0), g=None)
              for r, s0 in zip(t.rows, STEPS0)]
    rs = np.random.RandomState(12)
    applied = 0
    for kind in ('inf', 'nan', 'clean', 'clean', 'clean', 'clean', 'clean'):
        t.set_grads(rs, mag=1.0)
        if kind == 'inf':
            t.rows[-1]['g'][-1] = float('inf')
        if kind == 'nan':
            t.rows[0]['g'][0] = float('nan')
        for mr, r in zip(m_rows, t.rows):
            mr['g'] = r['g'].cpu().numpy()
        before = t.snapshot()
        step_new(t, guard)
        R.step(m_rows, HP['lr'], HP['beta1'], HP['beta2'], HP['eps'], m_state, m_scale, growth=2.0, backoff=0.5, interval=2, max_scale=1.0)
        torch.cuda.synchronize()
        after = t.snapshot()
        assert t.state.tolist() == m_state.tolist() and t.scale.tolist() == m_scale.tolist(), (kind, t.state.tolist(), m_state.tolist())
        if kind == 'clean':
            applied += 1
            assert all(not torch.equal(a['p'], b['p']) for a, b in zip(after[0], before[0]))
        else:
            assert all(torch.equal(a[k], b[k]) for a, b in zip(after[0], before[0]) for k in a), kind
        assert [float(r['step']) for r in t.rows] == [s + applied for s in STEPS0]
    # inf: scale 0.5, nan: 0.25; clean x2 -> 0.5, x2 -> 1.0, fifth clean: tracker 1; growth past max_scale = 1 is refused
    assert t.state.tolist() == [0, 1, 2, 7] and t.scale.tolist() == [1.0, 1.0]
    t.set_grads(rs, mag=1.0)
    step_new(t, guard)
    assert t.state.tolist() == [0, 0, 2, 8] and t.scale.tolist() == [1.0, 1.0]            # interval reached at the cap: 2.0 > max_scale
    assert t.sentinels_intact()


def _params(rs, shapes):
    ps = [torch.nn.Parameter(torch.from_numpy((rs.standard_normal(s) * 0.05).astype(np.float32)).to(DEV)) for s in shapes]
    return ps


def test_guarded_adam_chunks_per_group_and_per_sixteen_tensors(monkeypatch):
    """19 tensors in a first group (two chunks) and 3 in a second with another lr: GuardedAdam.step against the same optimiser driven down the
    per-tensor path (one l2i_adam_guarded_f32 a tensor), bit for bit, three steps one of which is skipped; the scale state advances once a step."""
    shapes = [(n,) for n in (1, 63, MB, MB + 1, 2 * MB + 3)] + [(7, 9)] * 14 + [(33,), (5, 11), (MB + 2,)]
    assert len(shapes[:19]) > _lib.ADAM_MAX_TENSORS
    rs = np.random.RandomState(3)
    pa = _params(rs, shapes)
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    sa = optim.LossScaler(dict(R=0, V=0, D=0, G=0), DEV, growth_interval=2, max_log2=3)
    sb = optim.LossScaler(dict(R=0, V=0, D=0, G=0), DEV, growth_interval=2, max_log2=3)
    groups = lambda ps: [dict(params=ps[:19], lr=1e-3), dict(params=ps[19:], lr=5e-3)]
    oa = optim.GuardedAdam(groups(pa), betas=(0.5, 0.99), scaler=sa)
    ob = optim.GuardedAdam(groups(pb), betas=(0.5, 0.99), scaler=sb)
    seen = []
    real = _lib.call

    def counting(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    for it in range(3):
        for p, q in zip(pa, pb):
            p.grad = torch.from_numpy(rs.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV)
            if it == 1 and p is pa[17]:
                p.grad.view(-1)[0] = float('inf')                            # in the second chunk of the first group: everything is skipped
            q.grad = p.grad.clone()
        del seen[:]
        monkeypatch.setattr(_lib, 'call', counting)
        oa.step()
        monkeypatch.setattr(_lib, 'call', real)
        assert seen == ['l2i_nonfinite_flag_multi_f32'] * 3 + ['l2i_adam_guarded_multi_f32'] * 3, seen
        # the per-tensor path on the twin
        todo = [(q, g, ob._state_of(q)) for g in ob.param_groups for q in g['params']]
        state, scale = ob._flags(torch.device(DEV))
        for q, _, _ in todo:
            _lib.call('l2i_nonfinite_flag_f32', _lib.fptr(q.grad), q.numel(), _lib.ptr(state))
        for i, (q, g, st) in enumerate(todo):
            _lib.call('l2i_adam_guarded_f32', _lib.fptr(q.data), _lib.fptr(q.grad), _lib.fptr(st['exp_avg']), _lib.fptr(st['exp_avg_sq']), _lib.fptr(st['step']),
                      q.numel(), float(g['lr']), 0.5, 0.99, float(g['eps']), 0, _lib.ptr(state), _lib.ptr(scale), 2.0, 0.5, 2, 8.0, 1 if i == len(todo) - 1 else 0)
        torch.cuda.synchronize()
        for p, q in zip(pa, pb):
            assert torch.equal(p.detach(), q.detach())
            assert all(torch.equal(oa.state[p][k], ob.state[q][k]) for k in ('exp_avg', 'exp_avg_sq', 'step'))
        assert sa.stats() == sb.stats() and sa.stats()['steps'] == it + 1
    assert sa.stats() == dict(scale=0.5, tracker=1, skipped=1, steps=3)
    assert all(float(oa.state[p]['step']) == 2.0 for p in pa)


def test_launch_budget(monkeypatch):
    seen = []
    real = _lib.call

    def counting(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    rs = np.random.RandomState(4)
    six = _params(rs, [(1024, 512), (1024,), (1024, 1024), (1024,), (512, 1024), (512,)])       # the MLP walk's six tensors
    one = _params(rs, [(1, 512)])
    for ps in (six, one):
        for p in ps:
            p.grad = torch.randn_like(p)
    o6, o1 = optim.GuardedAdam(six, lr=1e-3, betas=(0.5, 0.99)), optim.GuardedAdam(one, lr=1e-3, betas=(0.5, 0.99))
    monkeypatch.setattr(_lib, 'call', counting)
    o6.step()
    assert len(seen) <= 2 and seen == ['l2i_nonfinite_flag_multi_f32', 'l2i_adam_guarded_multi_f32'], seen
    del seen[:]
    o1.step()
    assert seen == ['l2i_adam_guarded_f32'], seen
    monkeypatch.setattr(_lib, 'call', real)
    torch.cuda.synchronize()
    assert all(float(o6.state[p]['step']) == 1.0 for p in six) and float(o1.state[one[0]]['step']) == 1.0


def test_two_runs_give_equal_bits_and_a_captured_step_replays_like_eager_steps():
    runs = []
    for _ in range(2):
        t = Tensors(5)
        rs = np.random.RandomState(13)
        for it in range(3):
            t.set_grads(rs)
            step_new(t)
        torch.cuda.synchronize()
        runs.append(t.snapshot())
    assert same(*runs)
    # GuardedAdam's multi-tensor step inside a torch.cuda.graph, replayed three times on static gradients, against three eager steps
    shapes = [(n,) for n in (1, 63, MB, MB + 1, 3 * MB + 3)] + [(17, 5)]
    rs = np.random.RandomState(6)
    pa = _params(rs, shapes)
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    for p, q in zip(pa, pb):
        p.grad = torch.from_numpy(rs.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV)
        q.grad = p.grad.clone()
    sa = optim.LossScaler(dict(R=0, V=0, D=0, G=0), DEV, growth_interval=2, max_log2=3)
    sb = optim.LossScaler(dict(R=0, V=0, D=0, G=0), DEV, growth_interval=2, max_log2=3)
    oa, ob = optim.GuardedAdam(pa, lr=1e-3, betas=(0.5, 0.99), scaler=sa), optim.GuardedAdam(pb, lr=1e-3, betas=(0.5, 0.99), scaler=sb)
    oa.init_state()                                                          # state and guard words outside the graph's pool
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step()
    torch.cuda.synchronize()
    assert all(float(oa.state[p]['step']) == 0.0 for p in pa)               # recorded, not run
    for _ in range(3):
        graph.replay()
        ob.step()
    torch.cuda.synchronize()
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach()) and float(oa.state[p]['step']) == 3.0
        assert all(torch.equal(oa.state[p][k], ob.state[q][k]) for k in ('exp_avg', 'exp_avg_sq', 'step'))
    assert sa.stats() == sb.stats() == dict(scale=2.0, tracker=1, skipped=0, steps=3)


def test_argument_errors():
    t = Tensors(7, cases=CASES[:2], steps0=STEPS0[:2])
    table, count = t.table()
    st, sc = _lib.ptr(t.state), _lib.ptr(t.scale)
    tail = (st, sc, 2.0, 0.5, 2, 8.0, 1)
    with pytest.raises(_lib.L2IError):
        _lib.call('l2i_nonfinite_flag_multi_f32', None, 2, st)
    with pytest.raises(_lib.L2IError):
        _lib.call('l2i_adam_guarded_multi_f32', None, 2, 1e-3, 0.5, 0.99, 1e-8, *tail)
    big = (_lib.AdamTensor * (_lib.ADAM_MAX_TENSORS + 1))(*([table[0]] * (_lib.ADAM_MAX_TENSORS + 1)))
    for tab, n in ((table, 0), (table, -1), (big, _lib.ADAM_MAX_TENSORS + 1)):
        with pytest.raises(_lib.L2IError):
            _lib.call('l2i_nonfinite_flag_multi_f32', tab, n, st)
        with pytest.raises(_lib.L2IError):
            _lib.call('l2i_adam_guarded_multi_f32', tab, n, 1e-3, 0.5, 0.99, 1e-8, *tail)
    for b1, b2 in ((1.0, 0.99), (0.5, 1.0), (-0.1, 0.99), (float('nan'), 0.99)):
        with pytest.raises(_lib.L2IError):
            _lib.call('l2i_adam_guarded_multi_f32', table, count, 1e-3, b1, b2, 1e-8, *tail)
    with pytest.raises(_lib.L2IError):
        _lib.call('l2i_adam_guarded_multi_f32', table, count, 1e-3, 0.5, 0.99, 1e-8, None, sc, 2.0, 0.5, 2, 8.0, 1)      # null state
    hole = (_lib.AdamTensor * 2)(table[0], _lib.AdamTensor(table[1].p, table[1].g, None, table[1].v, table[1].step, table[1].n))
    with pytest.raises(_lib.L2IError):
        _lib.call('l2i_adam_guarded_multi_f32', hole, 2, 1e-3, 0.5, 0.99, 1e-8, *tail)
    torch.cuda.synchronize()
    assert t.state.tolist() == [0, 0, 0, 0] and all(float(r['step']) == s for r, s in zip(t.rows, STEPS0)) and t.sentinels_intact()
    assert ctypes.sizeof(_lib.AdamTensor) == 48
