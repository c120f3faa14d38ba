"""tests/segmv_ref.py on the CPU: the hand-built table is consistent and reaches the code the product's tables do not, a float32 evaluation of
the kernel's arithmetic in its own order and in the reversed one stays inside the derived bounds at every batch size, and each planted mistake
leaves them on a named (batch, segment) row."""
import ctypes

import numpy as np
import pytest

from latent2im_amd import _lib
from tests import segmv_ref as S

TAB = S.build()
_cache = {}


def _row(B):
    if B not in _cache:
        ops = S.make_inputs(TAB, B)
        _cache[B] = (ops, S.run(TAB['segs'], TAB['blocks'], B, **ops))
    return _cache[B]


def _segment_masks(B):
    """segment id -> mask of its out elements."""
    masks = {}
    for sg, sp in zip(TAB['segs'], S.SPECS):
        m = np.zeros(TAB['size']['out'](B), bool)
        idx = sg.out_off_c + B * sg.out_off_b + np.arange(B)[:, None] * sg.out_bstride + np.arange(sg.rows)[None, :]
        m[idx] = True
        masks[sp.id] = m
    return masks


def test_table_is_the_one_the_issue_describes():
    segs = TAB['segs']
    assert [(s.rows, s.epi, [(s.part[i].K, s.part[i].pre) for i in range(s.nparts)]) for s in segs] == [
        (1, 3, [(4, 0)]), (64, 0, [(64, 0)]), (65, 1, [(20, 1)]), (96, 2, [(512, 0), (68, 2)]), (40, 3, [(36, 3)]), (130, 0, [(512, 0)])]
    assert segs[1].rgb_off_b < 0 and segs[5].rgb_off_b >= 0 and segs[5].rgb_w_off != 0 and segs[4].part[0].aux_off != 0
    for s in segs:
        assert s.out_bstride > s.rows and s.out_off_c != 0 and s.out_off_b != 0
        for i in range(s.nparts):
            pt = s.part[i]
            assert pt.w_pitch > s.rows and pt.in_off_c != 0 and pt.in_off_b != 0 and pt.K % 4 == 0 and pt.K <= 512
    assert segs[3].e_off_c != 0 and segs[3].e_off_b != 0 and segs[3].e_bstride > segs[3].rows
    assert S.wave_ranges(4) == [(0, 4), (4, 4), (4, 4), (4, 4)]
    assert S.wave_ranges(20) == [(0, 8), (8, 16), (16, 20), (20, 20)]
    assert S.wave_ranges(68) == [(0, 20), (20, 40), (40, 60), (60, 68)] and S.wave_ranges(512)[3] == (384, 512)
    blocks = TAB['blocks']
    assert sorted(blocks) == [(i, rb) for i, sp in enumerate(S.SPECS) for rb in range((sp.rows + 63) // 64)] and blocks != sorted(blocks)
    assert ctypes.sizeof(_lib.SegmvSeg) * len(segs) == S.raw_table(segs).size
    back = S.parse_table(S.raw_table(segs))
    assert [(b.rows, b.part[0].w_off, b.part[1].K) for b in back] == [(s.rows, s.part[0].w_off, s.part[1].K) for s in segs]


@pytest.mark.parametrize('B', S.BATCHES)
def test_no_two_blocks_write_one_element_and_nothing_overlaps(B):
    ops, ref = _row(B)                                       # run() asserts every index inside its buffer and every element written once
    masks = _segment_masks(B)
    total = sum(m.astype(int) for m in masks.values())
    assert total.max() == 1 and np.array_equal(total.astype(bool), ref['out_mask'])
    assert ref['out_mask'].sum() == B * sum(sp.rows for sp in S.SPECS) and not ref['out_mask'].all()          # gaps and stride padding stay unowned
    assert ref['wmod_mask'].sum() == B * 3 * 130 and not ref['wmod_mask'][:2 * B].any()
    assert np.isfinite(ref['out'][ref['out_mask']]).all() and np.isnan(ref['out'][~ref['out_mask']]).all()
    # the inputs of different parts do not overlap either
    used = np.zeros(TAB['size']['in'](B), int)
    for sg in TAB['segs']:
        for i in range(sg.nparts):
            pt = sg.part[i]
            foot = 3 * pt.K if pt.pre == 3 else pt.in_bstride
            used[pt.in_off_c + B * pt.in_off_b:pt.in_off_c + B * pt.in_off_b + B * foot] += 1
    assert used.max() == 1
    # the all-zero sample: rsqrt(1e-8)
    z = S.zero_sample(B)
    sg = TAB['segs'][2]
    got = ref['out'][sg.out_off_c + B * sg.out_off_b + z * sg.out_bstride + np.arange(sg.rows)]
    assert np.allclose(got, 1.0 / np.sqrt(S.EPS32), rtol=1e-12)


@pytest.mark.parametrize('order', ['kernel', 'reversed'])
@pytest.mark.parametrize('B', S.BATCHES)
def test_float32_arithmetic_is_inside_the_bounds(B, order):
    ops, ref = _row(B)
    out, wm = S.float32(TAB['segs'], TAB['blocks'], B, order=order, **ops)
    assert np.array_equal(np.isnan(out), ~ref['out_mask']) and np.array_equal(np.isnan(wm), ~ref['wmod_mask'])
    for sid, m in _segment_masks(B).items():
        r = S.ratio(out, ref['out'], ref['out_bound'], m)
        print('segmv f32 B=%d %s %s ratio %.3f' % (B, order, sid, r))
        assert r <= 1.0, (B, order, sid, r)
    r = S.ratio(wm, ref['wmod'], ref['wmod_bound'], ref['wmod_mask'])
    print('segmv f32 B=%d %s wmod ratio %.3f' % (B, order, r))
    assert r <= 1.0


# mistake -> (batch, segment or 'wmod') on which it must leave the bounds
CAUGHT_ON = {'second_part_dropped': (1, 'rows96_two_parts'), 'tail_k_dropped': (8, 'rows96_two_parts'), 'second_pass_stale': (9, 'rows1_k4'),
             'pre2_unsquared': (1, 'rows96_two_parts'), 'epi1_eps_dropped': (9, 'rows65_k20_demod'), 'off_b_unscaled': (17, 'rows64_k64_bias'),
             'pre3_plane_order': (8, 'rows40_k36_rgbred'), 'rgb_from_unbiased': (1, 'wmod')}


@pytest.mark.parametrize('mistake', S.MISTAKES)
def test_planted_mistake_exceeds_the_bounds(mistake):
    B, where = CAUGHT_ON[mistake]
    ops, ref = _row(B)
    bad = S.run(TAB['segs'], TAB['blocks'], B, mistake=mistake, **ops)
    if where == 'wmod':
        r = S.ratio(bad['wmod'], ref['wmod'], ref['wmod_bound'], ref['wmod_mask'])
        assert S.ratio(bad['out'], ref['out'], ref['out_bound'], ref['out_mask']) == 0.0          # only wmod tells
    else:
        r = S.ratio(bad['out'], ref['out'], ref['out_bound'], _segment_masks(B)[where])
    print('segmv mistake %s on B=%d %s: ratio %.3g' % (mistake, B, where, r))
    assert r > 1.0, (mistake, B, where, r)


def test_tail_mistake_is_seen_on_every_short_segment():
    """K = 4, 20 and 36 run in the 4-step tail alone; K = 68 in both loops; K = 64 and 512 in the 16-step loop alone."""
    B = 8
    ops, ref = _row(B)
    bad = S.run(TAB['segs'], TAB['blocks'], B, mistake='tail_k_dropped', **ops)
    seen = {sid: S.ratio(bad['out'], ref['out'], ref['out_bound'], m) > 1.0 for sid, m in _segment_masks(B).items()}
    assert seen == {'rows1_k4': True, 'rows64_k64_bias': False, 'rows65_k20_demod': True, 'rows96_two_parts': True, 'rows40_k36_rgbred': True,
                    'rows130_k512_torgb': False}


def test_every_mistake_is_in_the_table():
    assert set(CAUGHT_ON) == set(S.MISTAKES) and len(S.MISTAKES) == 8
    assert {b for b, _ in CAUGHT_ON.values()} <= set(S.BATCHES)


def test_probe_returns_rsqrt_alone():
    pr = S.probe()
    ref = S.run(pr['segs'], pr['blocks'], S.PROBE_B, pr['inp'], pr['w'], n_out=S.PROBE_B)
    # (the probe's reference rounds x + 1e-8 to float32 as the device does, the table model does not: they differ by that one rounding)
    assert ref['out_mask'].all() and np.all(np.abs(ref['out'] - pr['want']) <= 0.5 * S.U * ref['out'] * (1 + 1e-6))
    assert pr['inp'].reshape(-1, 4)[0, 0] == 0 and abs(pr['want'][0] - 1e4) < 1e-2
    got = pr['want'].astype(np.float32)                     # a correctly rounded rsqrt is within half a unit
    assert S.ulps(got, pr['want']).max() <= 0.5
    assert S.ulps(np.nextafter(got, np.float32(np.inf)), pr['want']).max() <= 1.5
    assert S.RSQRT_ULPS >= 2 and (S.RSQRT_MEASURED is None or S.RSQRT_ULPS == int(np.ceil(S.RSQRT_MEASURED)) + 1)
