"""The range histogram's model (tests/range_ref.py) against hand-made rows and numpy's own converts, and against the mistakes it claims to catch; the
host side of the monitor (nets16.reduce_row), the exponent rule and the calibration loop on fake measurements; the three driver flags; the header
and the binding."""
import math
import os
import re

import numpy as np
import pytest
import torch

from latent2im_amd import _lib, kernels16, nets16
from latent2im_amd.options import TrainOptions
from tests import range_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [rr.F16, rr.BF16, rr.F32]


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_row_on_hand_made_specials(kind):
    bits, want = rr.specials(kind)
    got = rr.row(bits, kind)
    full = np.zeros(rr.WORDS, dtype=np.uint64)
    for k, v in want.items():
        full[k] = v
    assert np.array_equal(got, full), [(i, int(got[i]), int(full[i])) for i in np.nonzero(got != full)[0]]


def test_row_agrees_with_numpys_converts_on_every_16_bit_pattern():
    """An independent route to the same integers: numpy converts fp16 -> fp32 exactly; bf16 is the upper half of an fp32 word."""
    u = np.arange(65536, dtype=np.uint16)
    as32 = u.view(np.float16).astype(np.float32).view(np.uint32) & 0x7fffffff
    nan = (u & 0x7c00 == 0x7c00) & (u & 0x3ff != 0)                  # (numpy quiets signalling NaNs: compare their field only)
    mine = rr.f16_abs_bits(u)
    assert np.array_equal(mine[~nan], as32[~nan]) and bool(((mine[nan] >> 23) == 255).all())
    assert np.array_equal(rr.abs_bits(u, rr.BF16), (u.astype(np.uint32) << 16) & 0x7fffffff)
    r = rr.row(u, rr.F16)
    assert int(r[:256].sum()) == 65536 and int(r[rr.ZEROS]) == 2 and int(r[255]) == 2 * 1024 and int(r[0]) == 2
    assert [int(r[103 + p]) for p in range(10)] == [2 << p for p in range(10)]            # subnormals with top bit p: 2^p patterns, two signs
    assert all(int(r[e]) == 2048 for e in range(113, 143)) and int(r[rr.MAX]) == 0x477fe000


@pytest.mark.parametrize('kind', KINDS)
def test_row_adds_and_keeps_the_maximum(kind):
    bits, _ = rr.specials(kind)
    small = np.array([0x3c00 if kind == rr.F16 else 0x3f80 if kind == rr.BF16 else 0x3f800000], dtype=rr.NP_BITS[kind])
    a, b = rr.row(bits, kind), rr.row(small, kind)
    for first, second in ((bits, small), (small, bits)):
        both = rr.row(second, kind, into=rr.row(first, kind))
        assert np.array_equal(both[:257], a[:257] + b[:257]) and int(both[rr.MAX]) == max(int(a[rr.MAX]), int(b[rr.MAX]))
        assert int(both[rr.CALLS]) == 2 and int(both[rr.N]) == bits.size + 1


@pytest.mark.parametrize('name,wrong', rr.MISTAKES, ids=[m[0] for m in rr.MISTAKES])
def test_planted_mistakes_are_told_apart(name, wrong):
    """Every slip differs from the model on the hand-made specials of at least one kind, in one call or in the second call into one row."""
    caught = []
    for kind in KINDS:
        bits, _ = rr.specials(kind)
        one = not np.array_equal(wrong(bits, kind), rr.row(bits, kind))
        two = not np.array_equal(wrong(bits, kind, into=rr.row(bits, kind)), rr.row(bits, kind, into=rr.row(bits, kind)))
        caught.append(one or two)
    assert any(caught), name
    if name == 'fp16 subnormals binned at 0':
        assert caught == [True, False, False]
    if name == 'bf16 read as fp16':
        assert caught == [False, True, False]


# ---- reduce_row -----------------------------------------------------------------------------------------------------------------------------------------
def _f32bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def test_reduce_row_on_synthetic_rows():
    k16, k32 = kernels16.RANGE_KINDS[torch.float16], kernels16.RANGE_KINDS[torch.float32]
    r = np.zeros(260, dtype=np.int64)
    r[0], r[256] = 10, 7                       # 7 zeros, 3 fp32 subnormals
    r[110], r[113], r[127], r[255] = 5, 4, 8, 2
    r[257], r[258], r[259] = _f32bits(1.75), 3, 29
    o = nets16.reduce_row(r, k16)
    assert (o['n'], o['zeros'], o['nonfinite'], o['calls']) == (29, 7, 2, 3)
    assert o['max'] == 1.75 and o['max_log2'] == math.log2(1.75)
    # 20 finite non-zero entries: 3 @ field 0, 5 @ 110, 4 @ 113, 8 @ 127: the tenth sits in field 113 -> 2^-14
    assert o['median_octave'] == 113 - 127
    assert o['below_normal'] == (3 + 5) / 20                       # fp16: everything under field 113
    assert nets16.reduce_row(r, k32)['below_normal'] == 3 / 20     # fp32 / bf16: field 0 less the zeros
    r[127] = 13                                                    # 25 entries: the 13th is the first of field 127
    assert nets16.reduce_row(r, k16)['median_octave'] == 0
    r[127] = 12                                                    # 24 entries: the lower median is the 12th, the last of field 113
    assert nets16.reduce_row(r, k16)['median_octave'] == -14


def test_reduce_row_of_an_empty_and_of_an_all_zero_map():
    for zeros in (0, 64):
        r = np.zeros(260, dtype=np.int64)
        r[0] = r[256] = r[259] = zeros
        o = nets16.reduce_row(r, 0)
        assert o['max'] == 0.0 and o['max_log2'] is None and o['median_octave'] is None and o['below_normal'] == 0.0 and o['n'] == zeros


def test_reduce_row_agrees_with_what_the_probe_computes():
    """PROBE's numbers from the same tensor: max equal, zero share equal, torch's (lower) median inside the octave."""
    g = torch.Generator().manual_seed(5)
    for count in (1, 2, 7, 64, 1001):
        t = (torch.randn(count, generator=g) * torch.exp2(torch.randint(-20, 3, (count,), generator=g).float())).to(torch.float16)
        t[::5] = 0
        o = nets16.reduce_row(rr.row(t.view(torch.int16).numpy().view(np.uint16), rr.F16).astype(np.int64), 0)
        a = t.float().abs()
        nz = a[a > 0]
        frac = float((a == 0).float().mean())                  # a float32 quotient: it names the integer count exactly for maps under 2^22 zeros
        assert o['max'] == float(a.max()) and round(frac * o['n']) == o['zeros'] and abs(o['zeros'] / o['n'] - frac) <= 2.0 ** -22 * frac
        if nz.numel():
            assert 2.0 ** o['median_octave'] <= float(nz.median()) < 2.0 ** (o['median_octave'] + 1)


# ---- the rule and the loop ---------------------------------------------------------------------------------------------------------------------------------
def test_branch_tags_and_the_exponent_rule():
    assert [nets16.branch_of(t) for t in ('R.G0', 'R.G15', 'V.d4', 'V.g1', 'D.g@64', 'D.g_last', 'G.dx0@4', 'PG.g_out@128', 'PG.g_a1@4')] == list('RRVVDDGGG')
    assert [nets16.branch_of(t) for t in ('R.fwd.out', 'V.fwd.c1', 'D.fwd.out@32', 'G.fwd.y0@4', 'PG.fwd.a2@8', 'P.fwd.tap0', 'P.g.tap1')] == [None] * 7
    assert nets16.scale_exponent(2.0 ** -9) == 14 and nets16.scale_exponent(2.0 ** -11.4) == 16 and nets16.scale_exponent(2.0 ** -11.6) == 17
    assert nets16.scale_exponent(2.0 ** 14.3) == -9
    rows = {'R.G0': dict(max=3.0, nonfinite=0), 'R.G3': dict(max=40.0, nonfinite=1), 'R.fwd.out': dict(max=1e4, nonfinite=9), 'V.g1': dict(max=0.0, nonfinite=0)}
    s = nets16.branch_summary(rows, dyn=0.5)
    assert set(s) == {'R', 'V'} and s['R'] == dict(max=40.0, tag='R.G3', nonfinite=1, dyn=0.5) and s['V']['max'] == 0.0


def _fake(true_log2, calls, dyn=1.0, absent=()):
    """A linear branch: the stored maximum is the true one times the scale; above 2^16 it is stored as inf, under 2^-25 as zero."""
    def measure(log2):
        calls.append(dict(log2))
        out = {}
        for k, t in true_log2.items():
            if k in absent:
                continue
            stored = t + log2[k] + math.log2(dyn)
            out[k] = dict(max=0.0 if stored < -25 else 2.0 ** min(stored, 15.9), nonfinite=int(stored >= 16), dyn=dyn, tag=k)
        return out
    return measure


def test_loop_settles_in_one_round_from_the_right_start():
    calls = []
    chosen, hist = nets16.calibrate_scales(dict(R=14, V=26), _fake(dict(R=-9.0, V=-21.2), calls))
    assert chosen == dict(R=14, V=26) and len(calls) == 1 and len(hist) == 1


def test_loop_applies_the_rule_and_confirms_it():
    calls = []
    chosen, _ = nets16.calibrate_scales(dict(R=-10, G=12), _fake(dict(R=-9.3, G=-7.0), calls))
    assert chosen == dict(R=14, G=12) and len(calls) == 2 and calls[1] == dict(R=14, G=12)
    calls = []
    chosen, _ = nets16.calibrate_scales(dict(R=14), _fake(dict(R=-9.0), calls, dyn=0.25))        # stored under 2^14 * 2^-2: the rule divides both out
    assert chosen == dict(R=14) and len(calls) == 1


def test_loop_overflow_then_settle():
    calls = []
    chosen, hist = nets16.calibrate_scales(dict(R=30), _fake(dict(R=-9.0), calls))               # 2^21 stored: inf
    assert chosen == dict(R=14) and [c['R'] for c in calls] == [30, 22, 14] and hist[0][1]['R']['nonfinite'] == 1


def test_loop_all_zero_then_settle():
    calls = []
    chosen, _ = nets16.calibrate_scales(dict(V=-10), _fake(dict(V=-22.0), calls))                # 2^-32 stored: flushed
    assert chosen == dict(V=27) and [c['V'] for c in calls] == [-10, -2, 27]


def test_loop_raises_with_what_it_saw_when_a_branch_never_settles():
    flip = []

    def measure(log2):                                    # a branch that is not linear: whatever the scale, non-finite
        flip.append(1)
        return dict(D=dict(max=1.0, nonfinite=3, dyn=1.0, tag='D.g@8'))
    with pytest.raises(RuntimeError, match=r'D not settled after 4 rounds.*16'):
        nets16.calibrate_scales(dict(D=16), measure)
    assert len(flip) == 4


def test_loop_leaves_an_absent_branch_at_its_start():
    calls = []
    chosen, _ = nets16.calibrate_scales(dict(R=14, V=3, D=-40, G=12), _fake(dict(R=-9.0, V=-9.0, D=-9.0, G=-7.0), calls, absent=('V', 'D')))
    assert chosen == dict(R=14, V=3, D=-40, G=12) and len(calls) == 1


def test_loop_decides_on_what_reduce_returns():
    seen = []

    def reduce(s):                                        # another rank saw an overflow in R
        seen.append(1)
        return {k: dict(v, nonfinite=1 if k == 'R' and len(seen) == 1 else v['nonfinite']) for k, v in s.items()}
    calls = []
    chosen, _ = nets16.calibrate_scales(dict(R=14), _fake(dict(R=-9.0), calls), reduce=reduce)
    assert [c['R'] for c in calls] == [14, 6, 14] and chosen == dict(R=14)


def test_watch_report_lines_and_warnings():
    ok = dict(n=100, zeros=0, nonfinite=0, calls=1, max=32.0, max_log2=5.0, median_octave=-3, below_normal=0.0)
    rows = {'R.G0': ok, 'R.G15': dict(ok, max=8.0, max_log2=3.0, median_octave=-9, below_normal=0.01), 'R.fwd.out': dict(ok, max=3000.0, max_log2=11.55),
            'G.dx0@4': dict(ok, median_octave=-17, below_normal=0.7), 'D.g@8': dict(ok, max=4096.0, max_log2=12.0), 'V.g1': dict(ok, nonfinite=2)}
    lines = dict((t.split(':')[0], (lvl, t)) for lvl, t in nets16.watch_report(rows))
    assert list(lines) == ['range D', 'range G', 'range R', 'range V', 'range fwd']
    assert lines['range R'][0] == 'info' and 'max 2^5.0 (R.G0)' in lines['range R'][1] and '2^-9 (R.G15)' in lines['range R'][1] and '0.01 (R.G15)' in lines['range R'][1]
    assert lines['range fwd'][0] == 'info'                                   # forward maps are reported, never warned about
    assert lines['range G'][0] == 'warning' and 'median of G.dx0@4 under 2^-14' in lines['range G'][1]
    assert lines['range D'][0] == 'warning' and '2^11' in lines['range D'][1]
    assert lines['range V'][0] == 'warning' and 'non-finite 2' in lines['range V'][1]


# ---- flags ----------------------------------------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, *extra):
    argv = ['--model', 'pggan', '--transform', 'face', '--models_dir', str(tmp_path), '--overwrite_config'] + list(extra)
    return TrainOptions().parse(print_opt=False, argv=argv)


def test_flags_parse_on_the_f16_path(tmp_path):
    opt = _parse(tmp_path, '--precision', 'f16', '--f16_scales', 'R=11,G=-3', '--f16_calibrate', '4', '--f16_watch', '50')
    assert opt.f16_scales == dict(R=11, G=-3) and opt.f16_calibrate == 4 and opt.f16_watch == 50
    opt = _parse(tmp_path, '--precision', 'f16')                      # unset: the namespace (and opt.yml) of a run without them is what it was
    assert not any(hasattr(opt, k) for k in ('f16_scales', 'f16_calibrate', 'f16_watch'))
    p = TrainOptions().initialize()
    assert (p.get_default('f16_scales'), p.get_default('f16_calibrate'), p.get_default('f16_watch')) == (None, 0, 0)
    assert _parse(tmp_path, '--precision', 'bf16', '--f16_watch', '3').f16_watch == 3
    assert nets16.parse_f16_scales('R=11,V=22,D=16,G=12') == dict(R=11, V=22, D=16, G=12)


@pytest.mark.parametrize('extra,why', [
    (['--precision', 'bf16', '--f16_calibrate', '2'], 'needs --precision f16'),
    (['--f16_calibrate', '2'], 'needs --precision f16'),
    (['--precision', 'bf16', '--f16_scales', 'R=1'], 'needs --precision f16'),
    (['--precision', 'f32', '--f16_watch', '1'], 'f16 or bf16'),
    (['--precision', 'f16', '--f16_scales', 'X=1'], 'distinct keys'),
    (['--precision', 'f16', '--f16_scales', 'R=1,R=2'], 'distinct keys'),
    (['--precision', 'f16', '--f16_scales', 'R=1.5'], 'integer'),
    (['--precision', 'f16', '--f16_calibrate', '-1'], '>= 0')])
def test_forbidden_flag_combinations_are_parser_errors(tmp_path, capsys, extra, why):
    with pytest.raises(SystemExit) as e:
        _parse(tmp_path, *extra)
    assert e.value.code == 2 and why in capsys.readouterr().err


def test_scales_flag_beats_the_environment_and_the_table(monkeypatch):
    table = nets16.loss_scale_for(256, 4)
    assert table == dict(R=16, V=28, D=18, G=14)
    monkeypatch.setattr(nets16, 'F16_SCALES_FLAG', dict(V=3))
    assert nets16.loss_scale_for(256, 4) == dict(table, V=3)
    assert nets16.pggan_scale_for(256, 2) == dict(nets16.loss_scale_for(128, 2), G=18)
    monkeypatch.setattr(nets16, 'F16_SCALES_FLAG', dict(G=-1, R=0))
    assert nets16.pggan_scale_for(256, 2)['G'] == -1
    monkeypatch.setenv('L2I_F16_SCALES', '1,2,3,4')
    assert nets16.loss_scale_for(64, 1) == dict(R=0, V=2, D=3, G=-1) and nets16.pggan_scale_for(256, 2) == dict(R=0, V=2, D=3, G=-1)
    monkeypatch.setattr(nets16, 'F16_SCALES_FLAG', None)
    assert nets16.loss_scale_for(64, 1) == dict(R=1, V=2, D=3, G=4)


# ---- header and binding -----------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_abi_did_not_move():
    h = open(os.path.join(ROOT, 'include', 'l2i.h')).read()
    assert re.search(r'int l2i_range_stats\(uint64_t\* row, const void\* x, int64_t n, int kind, void\* stream\);', h)
    defs = dict(re.findall(r'#define (L2I_RANGE_\w+|L2I_ABI_VERSION) (\d+)', h))
    assert defs == dict(L2I_RANGE_F16='0', L2I_RANGE_BF16='1', L2I_RANGE_F32='2', L2I_RANGE_WORDS='260', L2I_RANGE_ZEROS='256', L2I_RANGE_MAX='257',
                        L2I_RANGE_CALLS='258', L2I_RANGE_N='259', L2I_ABI_VERSION='12')
    assert (kernels16.RANGE_WORDS, kernels16.RANGE_ZEROS, kernels16.RANGE_MAX, kernels16.RANGE_CALLS, kernels16.RANGE_N) == (rr.WORDS, rr.ZEROS, rr.MAX, rr.CALLS, rr.N)
    assert kernels16.RANGE_KINDS == {torch.float16: rr.F16, torch.bfloat16: rr.BF16, torch.float32: rr.F32}


def test_binding_and_build_know_the_entry():
    assert _lib.ABI_VERSION == 12 and 'l2i_range_stats' in _lib.EXPORTS and 'l2i_range_stats_f16' not in _lib.EXPORTS
    res, args = _lib._SIGNATURES['l2i_range_stats']
    assert res is _lib.c_i and args == [_lib.c_p, _lib.c_p, _lib.c_l, _lib.c_i, _lib.c_p]
    mk = open(os.path.join(ROOT, 'latent2im_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS := .*\bl2i_range\.hip\b', mk, re.M) and 'l2i_range_f16.o' not in mk
    for f in ('l2i_stream.hip', 'l2i_stream_h8.hip'):
        assert 'range_stats' not in open(os.path.join(ROOT, 'latent2im_amd', 'csrc', f)).read()


def test_probe_points_are_silent_without_a_hook(monkeypatch):
    """Both hooks None: `_probe` touches neither its tensor nor the library."""
    assert nets16.PROBE is None and nets16.MONITOR is None and not nets16._probing()
    monkeypatch.setattr(_lib, 'call', lambda *a, **k: (_ for _ in ()).throw(AssertionError('library call')))
    nets16._probe('R.G0', object())
    seen = []
    monkeypatch.setattr(nets16, 'MONITOR', type('M', (), dict(add=lambda self, tag, t: seen.append(tag)))())
    assert nets16._probing()
    nets16._probe('R.G0', object())
    assert seen == ['R.G0']
