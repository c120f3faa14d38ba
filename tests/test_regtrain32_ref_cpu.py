"""tests/regtrain32_ref.py on the CPU: a float32 evaluation of every model stays inside its derived bound on every case, every seeded mistake
breaks a bound on the cases that list it (so the bounds are not vacuous) and is listed by some case, and the restated launch geometry proves
that the cases reach the paths they are named for: the second trip of the weight gradient's row loop, the 64-chunk cap of the BatchNorm
reductions, the second trip of the elementwise kernels' grid-stride loop."""
import pytest
import torch

from tests import regtrain16_ref as rr
from tests import regtrain32_ref as r32

WGRAD = {c.name: c for c in r32.WGRAD_CASES}
BN = {c.name: c for c in r32.BN_CASES}
_MODELS = {}


def bn_model(name):
    if name not in _MODELS:
        _MODELS[name] = r32.bn_model(BN[name])
    return _MODELS[name]


@pytest.mark.parametrize('name', list(WGRAD))
def test_wgrad_float32_inside_bound(name):
    case = WGRAD[name]
    x, gy, dw0 = r32.wgrad_data(case)
    want, bound = r32.wgrad(case, x, gy, dw0)
    got, _ = r32.wgrad(case, x, gy, dw0, dt=torch.float32)
    err, b, ratio = r32.worst(got, want, bound)
    print('rt32 wgrad %s float32 emulation: error %.3g bound %.3g ratio %.3g' % (name, err, b, ratio))
    assert got.dtype == torch.float32 and tuple(want.shape) == (case.cout, case.cin, case.kh, case.kw)
    assert ratio <= 1.0
    assert float(want.abs().max()) > 0
    if dw0 is not None:                                    # the starting value matters: most of it is far above the bound
        assert float(dw0.abs().median()) > 100 * float(bound.max())


@pytest.mark.parametrize('name,mistake', [(c.name, m) for c in r32.WGRAD_CASES for m in c.mistakes])
def test_wgrad_mistake_breaks_bound(name, mistake):
    case = WGRAD[name]
    x, gy, dw0 = r32.wgrad_data(case)
    want, bound = r32.wgrad(case, x, gy, dw0)
    wrong, _ = r32.wgrad(case, x, gy, dw0, _mistake=mistake)
    _, _, ratio = r32.worst(wrong, want, bound)
    print('rt32 wgrad %s mistake %s: ratio %.3g' % (name, mistake, ratio))
    assert ratio > 1.0


def test_every_mistake_is_listed():
    assert {m for c in r32.WGRAD_CASES for m in c.mistakes} == set(r32.WGRAD_MISTAKES)
    assert {m for c in r32.BN_CASES for m in c.mistakes} == set(r32.BN_MISTAKES)
    assert set(r32.WGRAD_MISTAKES[:5]) <= set(rr.MISTAKES) and set(r32.BN_MISTAKES[:3]) <= set(rr.MISTAKES)


def test_the_16_bit_model_is_what_it_was():
    """The arguments the fp32 model added to rr.wgrad default to the square, zero-started call; 'f32' bounds carry no half ulp of a store."""
    case = rr.WGRAD_CASES[2]
    x, gy = rr.wgrad_data(case)
    a = rr.wgrad(x, gy, case.k, case.stride, case.pad, 1.0, 'f16')
    b = rr.wgrad(x, gy, case.k, case.stride, case.pad, 1.0, 'f16', kw=case.k, pad_x=case.pad, dw0=torch.zeros(case.cout, case.cin, case.k, case.k))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    M = torch.tensor([0.0, 1.0, 3.5], dtype=torch.float64)
    assert torch.equal(rr.bound_store(M, M, 3, 'f32'), r32.U23 * 3 * M)
    assert torch.equal(rr.bound_store(M, M, 3, 'bf16'), rr.bound16(M, M, 3, 'bf16'))
    assert float(rr.bound_store(M, M, 3, 'f32')[0]) == 0.0 < float(rr.bound_store(M, M, 3, 'f16')[0])


@pytest.mark.parametrize('name', list(BN))
def test_bn_float32_inside_bounds(name):
    case, m = BN[name], bn_model(name)
    d, n = m['d'], m['n']
    mean, invstd, scale, shift = m['small']
    # stats: another summation order in float64 (the kernel sums in float64 too), the starting value added last instead of first
    (s, q), (bs, bq) = m['stats']
    xx = r32._d(d['x'])
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    flat = xx.permute(1, 0, 2, 3).reshape(case.c, -1)[:, perm]
    s0, q0 = (d['s0'], d['q0']) if case.preload else (0.0, 0.0)
    r_stats = max(r32.worst(flat.cumsum(1)[:, -1] + s0, s, bs)[2], r32.worst((flat * flat).cumsum(1)[:, -1] + q0, q, bq)[2])
    # apply, and the whole forward on float32 scale / shift
    want, bound = m['apply']
    got, _ = r32.bn_apply(d['x'], scale, shift, m['res'], case.relu, dt=torch.float32)
    r_apply = r32.worst(got, want, bound)[2]
    r_fwd = r32.worst(got, *m['forward'])[2]
    # backward
    (sd, sq), (bd, bq2) = m['reduce']
    (sd32, sq32), _ = r32.bn_bwd_reduce(d['gy'], m['out'], d['x'], mean, invstd, d.get('sd0'), d.get('sq0'), dt=torch.float32)
    r_red = max(r32.worst(sd32, sd, bd)[2], r32.worst(sq32, sq, bq2)[2])
    m_dy, m_dyxh = m['means']
    want_b, bound_b, dym = m['bwd']
    got_b, _, dym32 = r32.bn_bwd_apply(d['gy'], m['out'], d['x'], mean, invstd, d['gamma'], m_dy, m_dyxh, dt=torch.float32)
    r_bwd = r32.worst(got_b, want_b, bound_b)[2]
    print('rt32 bn %s float32 emulation: stats %.3g apply %.3g forward %.3g bwd_reduce %.3g bwd_apply %.3g' % (name, r_stats, r_apply, r_fwd, r_red, r_bwd))
    assert got.dtype == torch.float32 and got_b.dtype == torch.float32
    assert max(r_stats, r_apply, r_fwd, r_red, r_bwd) <= 1.0
    assert torch.equal(dym32.double(), dym) and torch.equal(r32.masked_dy(d['gy'], m['out']).double(), dym)
    if case.out_mask:                                      # the mask is what a ReLU leaves: zeros of both signs, and not only zeros
        o = m['out']
        zeros = int((o == 0).sum())
        assert 0.3 * o.numel() < zeros < 0.7 * o.numel() or o.numel() < 64
        assert bool((torch.signbit(o) & (o == 0)).any()) and bool((~torch.signbit(o) & (o == 0)).any())
        assert torch.equal(dym == 0, ~(o > 0).expand_as(dym) | (r32._d(d['gy']) == 0))


@pytest.mark.parametrize('name,mistake', [(c.name, m) for c in r32.BN_CASES for m in c.mistakes])
def test_bn_mistake_breaks_bounds(name, mistake):
    case, m = BN[name], bn_model(name)
    d, n = m['d'], m['n']
    mean, invstd, scale, shift = m['small']
    m_dy, m_dyxh = m['means']
    ratios = {}
    if mistake in ('chunk_tail_dropped', 'sums_overwritten'):
        (s, q), (bs, bq) = m['stats']
        (ws, wq), _ = r32.bn_stats(d['x'], d.get('s0'), d.get('q0'), _mistake=mistake)
        ratios.update(sum=r32.worst(ws, s, bs)[2], sumsq=r32.worst(wq, q, bq)[2])
    if mistake == 'residual_after_relu':
        assert case.residual and case.relu
        wrong, _ = r32.bn_apply(d['x'], scale, shift, m['res'], case.relu, _mistake=mistake)
        ratios.update(y=r32.worst(wrong, *m['apply'])[2])
    if mistake == 'unbiased_variance':
        wrong, _ = r32.bn_forward(d['x'], d['gamma'], d['beta'], m['res'], case.relu, _mistake=mistake)
        ratios.update(forward=r32.worst(wrong, *m['forward'])[2])
    if mistake in ('mask_wrong_operand', 'mask_ge_zero', 'chunk_tail_dropped', 'sums_overwritten'):
        assert case.out_mask or not mistake.startswith('mask')
        (sd, sq), (bd, bq) = m['reduce']
        (wd, wq), _ = r32.bn_bwd_reduce(d['gy'], m['out'], d['x'], mean, invstd, d.get('sd0'), d.get('sq0'), _mistake=mistake)
        ratios.update(sum_dy=r32.worst(wd, sd, bd)[2], sum_dyxh=r32.worst(wq, sq, bq)[2])
    if mistake in ('mask_wrong_operand', 'mask_ge_zero'):
        want, bound, dym = m['bwd']
        wrong, _, wdym = r32.bn_bwd_apply(d['gy'], m['out'], d['x'], mean, invstd, d['gamma'], m_dy, m_dyxh, _mistake=mistake)
        ratios.update(dx=r32.worst(wrong, want, bound)[2])
        if mistake == 'mask_ge_zero':                      # the masked dy is held bit for bit: it must differ
            assert not torch.equal(wdym, dym)
    print('rt32 bn %s mistake %s: ratios %s' % (name, mistake, ' '.join('%s %.3g' % kv for kv in ratios.items())))
    assert ratios and min(ratios.values()) > 1.0


def test_wgrad_cases_reach_the_paths_they_name():
    g = {name: r32.wgrad_geom(c) for name, c in WGRAD.items()}
    ow = {name: r32.out_size(c.w, c.kw, c.stride, c.pad_x) for name, c in WGRAD.items()}
    # the row loop: 64 tiles, 64 row groups, 260 rows, 256 in the first trip and 4 in the second
    rl = g['row_loop']
    assert (rl['tiles'], rl['row_groups'], rl['rows'], rl['per_trip'], rl['trips'], rl['last_trip_rows']) == (64, 64, 260, 256, 2, 4)
    assert 0 < rl['last_trip_rows'] < rl['per_trip']       # waves with and without a second row share the launch
    assert all(v['trips'] == 1 for name, v in g.items() if name != 'row_loop')
    # idle waves, one row per wave, an odd OW on ragged channels
    assert g['one_pixel']['idle_waves'] == 3 and g['ragged_3rows']['idle_waves'] == 1
    assert g['ragged_3x3']['rows'] == 4 and g['ragged_3x3']['idle_waves'] == 0
    for name in ('ragged_3x3', 'ragged_3rows'):
        assert ow[name] % 2 == 1 and WGRAD[name].cin % 32 and WGRAD[name].cout % 32 and WGRAD[name].cin > 32 and WGRAD[name].cout > 64
    # several row groups add into one dw
    assert g['row_groups_meet']['row_groups'] == 12 and g['row_groups_meet']['tiles'] == 1
    # the three kernel widths, both strides, rectangular kernels and paddings, a starting value
    assert {c.kw for c in r32.WGRAD_CASES} == {1, 3, 7} and {c.stride for c in r32.WGRAD_CASES} == {1, 2}
    st = WGRAD['stem']
    assert (st.kh, st.kw, st.stride, st.pad_y, st.cin, st.cout, st.b, st.h, st.w) == (7, 7, 2, 3, 3, 40, 2, 13, 11)
    assert {(c.kh, c.kw, c.pad_y, c.pad_x) for c in r32.WGRAD_CASES if c.kh != c.kw} == {(1, 3, 0, 1), (3, 1, 1, 0)}
    assert [c.name for c in r32.WGRAD_CASES if c.dw0] == ['accumulate']
    shape = lambda c: (c.kh, c.stride, c.pad_y, c.cin, c.cout, c.b, c.h, c.w)
    for name16, name32 in (('border_3x3', 'border_3x3'), ('border_3x3', 'accumulate'), ('odd_3x3_s2', 'odd_3x3_s2'), ('s2_1x1', 's2_1x1'), ('slices_3x3', 'row_groups_meet')):
        c16 = {c.name: c for c in rr.WGRAD_CASES}[name16]
        assert shape(WGRAD[name32]) == (c16.k, c16.stride, c16.pad, c16.cin, c16.cout, c16.b, c16.h, c16.w)


def test_bn_cases_reach_the_paths_they_name():
    n_of = lambda c: c.b * c.hw[0] * c.hw[1]
    red = {c.name: r32.bn_reduce_geom(n_of(c)) for c in r32.BN_CASES}
    elem = {c.name: r32.bn_elem_geom(n_of(c) * c.c) for c in r32.BN_CASES}
    assert [c[:8] for c in r32.BN_CASES[:6]] == [tuple(c) for c in rr.BN_CASES]
    # one chunk; several chunks meeting in the atomics with a ragged tail; the cap with whole trips; the cap with a tail
    for name in ('c8_hw1', 'c8_hw35', 'c72_hw35', 'c72_hw1', 'preloaded'):
        assert red[name]['chunks'] == 1 and elem[name]['trips'] == 1
    assert red['c8_big'] == dict(chunks=7, capped=False, trips=16, tail=27648 % (7 * 256)) and red['c8_big']['tail'] > 0
    assert red['c72_big']['chunks'] == 3 and not red['c72_big']['capped']
    assert n_of(BN['cap']) == 294912 and red['cap'] == dict(chunks=64, capped=True, trips=18, tail=0)
    assert red['cap_tail'] == dict(chunks=64, capped=True, trips=17, tail=8256)
    # the second trip of the grid-stride loop: more than 2048 * 256 elements
    assert n_of(BN['c72_big']) * 72 == 663552 and n_of(BN['cap']) * 3 == 884736
    for name in ('c72_big', 'cap', 'cap_tail'):
        assert elem[name] == dict(grid=2048, trips=2)
    assert elem['c8_big']['trips'] == 1
    # a case a mistake of the chunk tail is listed for has one
    for c in r32.BN_CASES:
        if 'chunk_tail_dropped' in c.mistakes:
            assert n_of(c) % 4096 and n_of(c) > 4096, c.name
    # every operand combination the trainer uses, forward and backward, and relu = 0 with a residual
    fwd = {(c.residual, c.relu) for c in r32.BN_CASES}
    bwd = {(c.out_mask, c.want_masked) for c in r32.BN_CASES}
    both = {(c.residual, c.relu, c.out_mask, c.want_masked) for c in r32.BN_CASES}
    for combo in r32.TRAINER_COMBOS:
        assert combo in both, combo
    assert set(r32.EXTRA_COMBOS) <= fwd and (False, True) in bwd
    assert [c.name for c in r32.BN_CASES if c.preload] == ['preloaded']
    d = r32.bn_data(BN['preloaded'])
    assert all(float(d[k].abs().min()) > 0 for k in ('s0', 'q0', 'sd0', 'sq0'))
