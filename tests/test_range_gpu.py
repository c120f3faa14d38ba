"""l2i_range_stats against tests/range_ref.py word for word; nets16.RangeMonitor against the PROBE it stands in for; the calibration of the fp16
gradient exponents on the 64^2 StyleGAN2 graph (synthetic weights, batch 2, five scene attributes, every loss term on) — recovery from wrong starts, what
it does to the walk gradient, that it leaves no trace — the monitor inside a replayed hipGraph, and the driver flags on the PGGAN face graph.

L2I_RANGE_CALIBRATION=<file>: the figures of test_calibration_changes_what_the_walk_learns_from (profiles/range_calibration.txt)."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import yaml

from latent2im_amd import _lib, capture, constants, conv, graph, kernels16, nets16, selfcheck, synth
from latent2im_amd import pggan as pg
from tests import emu
from tests import range_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
SIZE, BATCH = 64, 2
ATTRS = ['dirty', 'daylight', 'night', 'sunrisesunset', 'dawndusk']
TORCH_OF = {rr.F16: torch.float16, rr.BF16: torch.bfloat16, rr.F32: torch.float32}
_NETS = {}


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------------------
def _src_constants():
    src = open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'l2i_range.hip')).read()
    return {k: int(v) for k, v in re.findall(r'constexpr int (RANGE_\w+) = (\d+);', src)}


def _device(bits, kind, offset=0):
    """The patterns as a device tensor of the kind that starts ``offset`` elements past a 16-byte boundary (a contiguous slice)."""
    bits = np.ascontiguousarray(bits, dtype=rr.NP_BITS[kind])
    signed = bits.view(np.int16 if kind != rr.F32 else np.int32)
    buf = torch.zeros(bits.size + 8, dtype=torch.int16 if kind != rr.F32 else torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + bits.size] = torch.from_numpy(signed).to(DEV)
    t = buf.view(TORCH_OF[kind])[offset:offset + bits.size]
    assert t.is_contiguous() and t.data_ptr() % 16 == (offset * t.element_size()) % 16
    return t


def _row():
    return torch.zeros(rr.WORDS, dtype=torch.int64, device=DEV)


def _host(row):
    return row.cpu().numpy().view(np.uint64)


def _patterns(kind, n, seed):
    rs = np.random.RandomState(seed)
    if kind == rr.F32:
        bits = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        sp = rr.specials(kind)[0]
        bits[:min(n, sp.size)] = sp[:min(n, sp.size)]
        return bits
    return rs.permutation(65536).astype(np.uint16)[np.arange(n) % 65536]


def _mismatch(got, want):
    return [(int(i), int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0]]


@pytest.mark.parametrize('kind', [rr.F16, rr.BF16], ids=['f16', 'bf16'])
def test_every_16_bit_pattern(kind):
    bits = np.arange(65536, dtype=np.uint16)
    row = kernels16.range_stats(_device(bits, kind), _row())
    assert not _mismatch(_host(row), rr.row(bits, kind))
    sp, _ = rr.specials(kind)
    assert not _mismatch(_host(kernels16.range_stats(_device(sp, kind), _row())), rr.row(sp, kind))


@pytest.mark.parametrize('offset', [0, 1, 3, 5])
@pytest.mark.parametrize('kind', [rr.F16, rr.BF16, rr.F32], ids=['f16', 'bf16', 'f32'])
def test_sizes_and_starts(kind, offset):
    """Head, body and tail of the 16-byte walk: n below, at and above one vector, a partial block, several blocks; four starts off the boundary."""
    for n in (1, 7, 8, 9, 511, 4096):
        bits = _patterns(kind, n, seed=n + offset)
        got = _host(kernels16.range_stats(_device(bits, kind, offset), _row()))
        assert not _mismatch(got, rr.row(bits, kind)), (n, offset)


@pytest.mark.parametrize('kind', [rr.F16, rr.F32], ids=['f16', 'f32'])
def test_a_size_past_the_block_cap(kind):
    """RANGE_MAX_BLOCKS blocks of RANGE_THREADS lanes take RANGE_DEPTH 16-byte vectors a lane and pass: the grid-stride loop turns over beyond
    1024 * 256 * 4 = 2^20 vectors, i.e. n > 2^23 16-bit or 2^22 fp32 elements.  n = that + 4099 vectors' worth + 5, three elements off the boundary."""
    c = _src_constants()
    assert c['RANGE_MAX_BLOCKS'] * c['RANGE_VEC_PER_BLOCK'] == c['RANGE_MAX_BLOCKS'] * c['RANGE_THREADS'] * c['RANGE_DEPTH'] == 2 ** 20
    per = 4 if kind == rr.F32 else 8
    n = (2 ** 20 + 4099) * per + 5
    bits = _patterns(kind, n, seed=99)
    got = _host(kernels16.range_stats(_device(bits, kind, 3), _row()))
    assert not _mismatch(got, rr.row(bits, kind))


def test_rows_add_tags_keep_apart_and_streams_commute():
    a, b = _patterns(rr.F16, 5000, 1), _patterns(rr.BF16, 777, 2)
    ta, tb = _device(a, rr.F16, 1), _device(b, rr.BF16, 5)
    mon = nets16.RangeMonitor(DEV, capacity=2)
    mon.add('x', ta)
    mon.add('y', tb)
    mon.add('x', ta[:100].contiguous())
    want_x = rr.row(a[:100], rr.F16, into=rr.row(a, rr.F16))
    assert not _mismatch(_host(mon.table[0]), want_x) and not _mismatch(_host(mon.table[1]), rr.row(b, rr.BF16))
    with pytest.raises(RuntimeError, match='full'):
        mon.add('z', ta)
    r = mon.read()
    assert r['x']['calls'] == 2 and r['x']['n'] == 5100 and r['y']['n'] == 777
    assert r['x'] == nets16.reduce_row(want_x.astype(np.int64), rr.F16) and r['y'] == nets16.reduce_row(rr.row(b, rr.BF16).astype(np.int64), rr.BF16)
    mon.clear()
    assert int(mon.table.abs().sum()) == 0
    # two streams into one row at once against the same calls in sequence
    big = _device(_patterns(rr.F16, 300000, 3), rr.F16)
    seq = _row()
    for _ in range(4):
        kernels16.range_stats(big, seq)
        kernels16.range_stats(ta, seq)
    torch.cuda.synchronize()
    par, s1, s2 = _row(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for s, t in ((s1, big), (s2, ta)):
        with torch.cuda.stream(s):
            for _ in range(4):
                kernels16.range_stats(t, par)
    torch.cuda.synchronize()
    assert not _mismatch(_host(par), _host(seq))


def test_refusals():
    t = torch.zeros(16, dtype=torch.float16, device=DEV)
    lib = _lib.load()
    row = _row()
    for args in ((None, t.data_ptr(), 16, 0), (row.data_ptr(), None, 16, 0), (row.data_ptr(), t.data_ptr(), 0, 0), (row.data_ptr(), t.data_ptr(), 16, 3),
                 (row.data_ptr(), t.data_ptr(), -4, 1)):
        assert lib.l2i_range_stats(*args, None) == -1, args
    with pytest.raises(_lib.L2IError):
        kernels16.range_stats(t.to(torch.float64), row)
    with pytest.raises(_lib.L2IError):
        kernels16.range_stats(torch.zeros(4, 8, dtype=torch.float16, device=DEV).t(), row)
    torch.cuda.synchronize()
    assert int(row.abs().sum()) == 0


# ---- graphs -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _f16_path():
    keep = (conv.PRECISION, constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS, nets16.PROBE, nets16.MONITOR, nets16.F16_SCALES_FLAG)
    rng = np.random.get_state()
    conv.PRECISION, constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS = 'f16', SIZE, BATCH, True
    yield
    conv.PRECISION, constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS, nets16.PROBE, nets16.MONITOR, nets16.F16_SCALES_FLAG = keep
    np.random.set_state(rng)


def _sg2(key='table', log2=None):
    """A SceneGraph on the shared frozen networks of ``key`` with a fresh seeded walk and the scaler started over (at ``log2``: default the table's)."""
    if key not in _NETS:
        _NETS[key] = graph.load_networks(SIZE, torch.device(DEV, torch.cuda.current_device()))
    with open(os.path.join(ROOT, 'dataset', 'attributes_scene.txt')) as f:
        table = {n: i for i, n in enumerate(l.strip() for l in f if l.strip())}
    g = graph.SceneGraph(lr=1e-3, walk_type='linear', loss='l2', trainEmbed=False, attrList=list(ATTRS), attrTable=table, layers=None,
                         stylegan_opts=types.SimpleNamespace(latent='w'), nets=_NETS[key])
    with torch.no_grad():
        g.walk.w.copy_(torch.from_numpy(synth.walk_init(len(ATTRS), g.module.netG.n_latent, seed=7)))
    sc = g.loss_scaler
    sc.state.zero_()
    sc.scale.copy_(torch.tensor([1.0, 1.0]))
    if key == 'table' or log2 is not None:
        sc.log2.update(log2 if log2 is not None else nets16.loss_scale_for(SIZE, BATCH))
    g.weight_sources['loss_scale_log2'] = dict(sc.log2)
    return g


ZS = synth.z_sample(BATCH, seed=21)
ALPHA = np.ones((BATCH, 5)) * np.random.RandomState(22).uniform(-1, 1, 5)


def _grad_step(g):
    torch.manual_seed(11)
    r = selfcheck.run_step(g, ZS, ALPHA, clamp=True, optimize=False)
    torch.cuda.synchronize()
    return r


def _counting(monkeypatch):
    seen, real = [], _lib.call

    def call(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(_lib, 'call', call)
    return seen


def _compare_with_probe(rows, probe):
    """max equal exactly; PROBE's zero share (a float32 quotient) names the monitor's integer count; PROBE's median inside the median octave.  A tag
    the step passes several times (both generator passes) is one row here and several PROBE entries: maximum of the maxima, sum of the counts."""
    by_tag = {}
    for tag, shape, mx, med, zf in probe:
        by_tag.setdefault(tag, []).append((int(np.prod(shape)), mx, med, zf))
    assert set(rows) == set(by_tag), (sorted(set(rows) ^ set(by_tag)))
    for tag, ents in sorted(by_tag.items()):
        r = rows[tag]
        assert r['calls'] == len(ents) and r['n'] == sum(e[0] for e in ents), tag
        assert r['max'] == max(e[1] for e in ents), (tag, r['max'], ents)
        assert r['zeros'] == sum(round(e[3] * e[0]) for e in ents), (tag, r['zeros'], ents)
        if len(ents) == 1:
            n, mx, med, zf = ents[0]
            assert abs(r['zeros'] / n - zf) <= 2.0 ** -22 * zf, tag
            if r['median_octave'] is None:
                assert med == 0.0
            else:
                assert 2.0 ** r['median_octave'] <= med < 2.0 ** (r['median_octave'] + 1), (tag, med, r['median_octave'])
        print('%-16s n %9d  max 2^%6.2f  median octave %s  below normal %.4f  zeros %.4f' % (tag, r['n'], r['max_log2'] if r['max_log2'] is not None else float('nan'),
                                                                                         r['median_octave'], r['below_normal'], r['zeros'] / r['n']))


def test_monitor_sees_what_probe_sees_stylegan2(monkeypatch):
    g = _sg2()
    seen = _counting(monkeypatch)
    _grad_step(g)
    assert 'l2i_range_stats' not in seen and len(seen) > 50                  # both hooks None: not one call added to the step
    nets16.PROBE, nets16.MONITOR = [], nets16.RangeMonitor(DEV)
    del seen[:]
    _grad_step(g)
    rows = nets16.MONITOR.read()
    assert seen.count('l2i_range_stats') == sum(r['calls'] for r in rows.values()) == len(nets16.PROBE)
    assert {nets16.branch_of(t) for t in rows} == {'R', 'V', 'D', 'G', None}
    _compare_with_probe(rows, nets16.PROBE)


def _pggan(dt='f16'):
    constants.BATCH_SIZE = BATCH
    key = 'pg'
    if key not in _NETS:
        _NETS[key] = pg.load_networks(torch.device(DEV, torch.cuda.current_device()))
    g = pg.faceGraph(lr=1e-3, walk_type='NNz', loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': 31}, layers=None, pgan_opts=None,
                     nets=_NETS[key])
    emu.seeded_state(g.walk, 81)
    g.loss_scaler.state.zero_()
    g.loss_scaler.scale.copy_(torch.tensor([1.0, 1.0]))
    return g


def test_monitor_sees_what_probe_sees_pggan(monkeypatch):
    g = _pggan()
    z = torch.Tensor(synth.z_sample(BATCH, seed=40)).to(DEV)
    ad = torch.full((BATCH, 1), 0.3, device=DEV)
    seen = _counting(monkeypatch)
    pg.walk_forward_backward(g, z, ad, no_content_loss=False)
    assert 'l2i_range_stats' not in seen and len(seen) > 50
    nets16.PROBE, nets16.MONITOR = [], nets16.RangeMonitor(DEV)
    pg.walk_forward_backward(g, z, ad, no_content_loss=False)
    torch.cuda.synchronize()
    rows = nets16.MONITOR.read()
    assert {nets16.branch_of(t) for t in rows} == {'R', 'V', 'G', None} and any(t.startswith('PG.g_') for t in rows)
    _compare_with_probe(rows, nets16.PROBE)


# ---- 3. - 5. calibration ----------------------------------------------------------------------------------------------------------------------------------
def _calibrate(g):
    return g.calibrate_scales(2, clamp=True)


def _branch_maxima(g):
    nets16.MONITOR = mon = nets16.RangeMonitor(DEV)
    try:
        _grad_step(g)
    finally:
        nets16.MONITOR = None
    return nets16.branch_summary(mon.read())


def test_calibration_recovers_from_wrong_starts():
    table = nets16.loss_scale_for(SIZE, BATCH)
    home = _calibrate(_sg2())['chosen']
    print('table %s -> %s' % (table, home))
    for off in (-24, 16):
        g = _sg2(log2={k: v + off for k, v in table.items()})
        rec = _calibrate(g)
        print('start table%+d: %s -> %s in %d rounds' % (off, rec['start'], rec['chosen'], rec['rounds']))
        assert rec['start'] == {k: v + off for k, v in table.items()} and g.loss_scaler.log2 == rec['chosen'] == g.weight_sources['loss_scale_log2']
        assert all(abs(rec['chosen'][k] - home[k]) <= 1 for k in 'RVDG'), (rec['chosen'], home)
        top = _branch_maxima(g)
        print({k: 'max 2^%.2f at %s' % (np.log2(v['max']), v['tag']) for k, v in top.items()})
        assert set(top) == set('RVDG') and all(v['nonfinite'] == 0 and 2.0 ** 3 <= v['max'] <= 2.0 ** 7 for v in top.values()), top


PARITY_OFFSET = -24          # octaves under the table at which the uncalibrated walk gradient is measured (see the test)


def _parity(g, ref):
    a, b = g.double().reshape(-1), ref.double().reshape(-1)
    return float((a * b).sum() / (a.norm() * b.norm())), float((a - b).norm() / b.norm())


def test_calibration_changes_what_the_walk_learns_from():
    """The walk gradient of one step (same z, alpha) under the table's exponents, under the table + PARITY_OFFSET, and after calibrating from that
    start, on the 16-bit parity bar of tests/test_h8_gpu.py (cosine > 0.998 and rel-L2 < 0.06) against the first: the uncalibrated leg fails it, the
    calibrated one passes."""
    table = nets16.loss_scale_for(SIZE, BATCH)
    ref = _grad_step(_sg2())['grad']
    g = _sg2(log2={k: v + PARITY_OFFSET for k, v in table.items()})
    low = _parity(_grad_step(g)['grad'], ref)
    rec = _calibrate(g)
    cal = _parity(_grad_step(g)['grad'], ref)
    again = _parity(_grad_step(_sg2())['grad'], ref)
    lines = ['# walk gradient of one 64^2 batch-2 fp16 step against the same step under the table exponents %s (tests/test_range_gpu.py)' % table,
             'table, run again:          cosine %.6f  rel-L2 %.6f' % again,
             'table %+d, uncalibrated:   cosine %.6f  rel-L2 %.6f' % ((PARITY_OFFSET,) + low),
             'calibrated from there:     cosine %.6f  rel-L2 %.6f   exponents %s (%d rounds)' % (cal + (rec['chosen'], rec['rounds']))]
    print('\n'.join(lines))
    if os.environ.get('L2I_RANGE_CALIBRATION'):
        with open(os.environ['L2I_RANGE_CALIBRATION'], 'w') as f:
            f.write('\n'.join(lines) + '\n')
    assert not (low[0] > 0.998 and low[1] < 0.06), low
    assert cal[0] > 0.998 and cal[1] < 0.06, cal


def _state(g):
    g.optimizers.init_state()
    st = [p.detach().clone() for p in g.walk.parameters()]
    for p in g.walk.parameters():
        st += [g.optimizers.state[p][k].detach().clone() for k in ('step', 'exp_avg', 'exp_avg_sq')]
    return st + [g.loss_scaler.scale.clone(), g.loss_scaler.state.clone()]


def _same_rng(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_calibration_leaves_no_trace():
    table = nets16.loss_scale_for(SIZE, BATCH)
    g = _sg2(log2={k: v - 8 for k, v in table.items()})
    np.random.seed(5)
    before, rng, dev_rng = _state(g), np.random.get_state(), torch.cuda.get_rng_state()
    rec = _calibrate(g)
    assert rec['chosen'] != rec['start']
    after = _state(g)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and all(p.grad is None for p in g.walk.parameters())
    assert _same_rng(rng, np.random.get_state()) and torch.equal(dev_rng, torch.cuda.get_rng_state())
    assert nets16.MONITOR is None and getattr(g, '_captured_step', None) is None

    def three(gr):
        out = []
        torch.manual_seed(17)
        for i in range(3):
            r = selfcheck.run_step(gr, synth.z_sample(BATCH, seed=60 + i), ALPHA * (0.5 + 0.25 * i), clamp=True)
            torch.cuda.synchronize()
            out.append((r['loss'].clone(), r['grad'].clone(), gr.walk.w.detach().clone()))
        return out
    mine = three(g)
    nets16.F16_SCALES_FLAG = nets16.parse_f16_scales(','.join('%s=%d' % kv for kv in rec['chosen'].items()))
    fresh = _sg2(key='flag')
    nets16.F16_SCALES_FLAG = None
    assert fresh.loss_scaler.log2 == rec['chosen'] and fresh.loss_scaler is not g.loss_scaler
    for i, (a, b) in enumerate(zip(mine, three(fresh))):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (i, [float((x.double() - y.double()).abs().max()) for x, y in zip(a, b)])
    g._captured_step = object()
    with pytest.raises(RuntimeError, match='captured'):
        _calibrate(g)


# ---- 6. replay -----------------------------------------------------------------------------------------------------------------------------------------------
def test_monitor_is_recorded_into_the_hipgraph():
    """The eager step and the captured one run on two graph objects over the same frozen networks, as in the project's other capture tests: a graph
    whose walk still hangs in a live autograd graph of an eager step on the default stream must not be captured (capture.CapturedZStep's note on
    gradient accumulators), so nothing of the eager step but its loss and the monitor's rows is kept."""
    nets16.MONITOR = mon = nets16.RangeMonitor(DEV)
    eager = dict(loss=float(_grad_step(_sg2())['loss']))
    eager_rows = mon.read()
    g = _sg2()
    step = capture.CapturedStep(g, BATCH, 5, clamp=True)
    mon.clear()
    r = step(ZS, ALPHA, optimize=False)
    torch.cuda.synchronize()
    one, loss = mon.read(), float(r['loss'])
    for _ in range(2):
        step(ZS, ALPHA, optimize=False)
    torch.cuda.synchronize()
    three = mon.read()
    assert set(one) == set(three) == set(eager_rows) and len(one) > 20
    for tag in one:
        assert one[tag]['calls'] == eager_rows[tag]['calls'] >= 1 and one[tag]['n'] == eager_rows[tag]['n']
        assert three[tag]['calls'] == 3 * one[tag]['calls'] and three[tag]['n'] == 3 * one[tag]['n'], tag
    print('loss: eager %.9g, replayed %.9g' % (float(eager['loss']), loss))
    assert loss == float(eager['loss'])


# ---- 7. driver -----------------------------------------------------------------------------------------------------------------------------------------------
def _driver_argv(models, precision, *extra):
    return ['--model', 'pggan', '--transform', 'face', '--no_gan_loss', '--synthetic_weights', '--num_samples', '4', '--batch_size', '2', '--n_epoch', '1',
            '--learning_rate', '1e-3', '--attrList', 'Smiling', '--attrPath', os.path.join(ROOT, 'dataset', 'attributes_celeba.txt'), '--models_dir', models,
            '--overwrite_config', '--seed', '3', '--model_save_freq', '1000', '--precision', precision] + list(extra)


def test_driver_calibrates_and_watches(tmp_path, capsys):
    from latent2im_amd import trainer
    models = str(tmp_path / 'models')
    trainer.main(multi_attr=False, argv=_driver_argv(models, 'f16', '--f16_calibrate', '2', '--f16_watch', '1'))
    out = os.path.join(models, 'pggan_face_NNz_lr0.001_l2')
    rec = json.load(open(os.path.join(out, 'f16_scales.json')))
    assert set(rec) >= {'start', 'chosen', 'tags'} and rec['start'] == nets16.pggan_scale_for(constants.PG_RESOLUTION, 2)
    assert rec['chosen']['D'] == rec['start']['D'] and any(t.startswith('PG.g_') for t in rec['tags'])
    opt = yaml.load(open(os.path.join(out, 'opt.yml')), Loader=yaml.FullLoader)
    assert opt['weight_sources']['loss_scale_log2'] == rec['chosen'] and opt['f16_calibrate'] == 2 and opt['f16_watch'] == 1
    log = open(os.path.join(out, 'log.txt')).read()
    assert log.count('T, epc, bst, lss, alpha') == 2 and log.count('range G:') == 2 and log.count('range fwd:') == 2
    assert "'loss_scale_log2'" in log
    walk = torch.load(os.path.join(out, 'model_w_1_final_walk_module.ckpt'), map_location='cpu', weights_only=False)
    assert all(bool(torch.isfinite(p).all()) for p in walk.parameters())
    assert nets16.MONITOR is None and nets16.F16_SCALES_FLAG is None
    # the same flags under --hip_graph: calibration (eager probe steps on this graph) comes first, then the step is captured with the monitor in it
    replays, real = [], capture.CapturedZStep.__call__
    capture.CapturedZStep.__call__ = lambda self, *a, **k: replays.append(1) or real(self, *a, **k)
    try:
        trainer.main(multi_attr=False, argv=_driver_argv(str(tmp_path / 'm3'), 'f16', '--f16_calibrate', '2', '--f16_watch', '1', '--hip_graph'))
    finally:
        capture.CapturedZStep.__call__ = real
    out3 = os.path.join(str(tmp_path / 'm3'), 'pggan_face_NNz_lr0.001_l2')
    log3 = open(os.path.join(out3, 'log.txt')).read()
    assert len(replays) == 2 and log3.count('range G:') == 2 and json.load(open(os.path.join(out3, 'f16_scales.json')))['chosen'] == rec['chosen']
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        trainer.main(multi_attr=False, argv=_driver_argv(str(tmp_path / 'm2'), 'bf16', '--f16_calibrate', '2'))
    assert e.value.code == 2 and 'needs --precision f16' in capsys.readouterr().err
