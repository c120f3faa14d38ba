"""l2i_segmented_matvec_f32 (csrc/l2i_modulation.hip) through its raw entry point against tests/segmv_ref.py: the hand-built six-segment table at
B in {1, 8, 9, 17}, twice on fresh sentinel-guarded `out` and `wmod`; per segment the worst error as a share of its derived bound, every
element no block owns still the sentinel, equal bits of the two launches; the device rsqrtf measured through an epi-1 segment that returns it
alone; refused calls that write nothing.  Every row prints `segmv B=<B> <segment> err bound ratio`."""
import math

import numpy as np
import pytest
import torch

from latent2im_amd import _lib
from tests import contract_gpu as cg
from tests import segmv_ref as S
from tests import stream_ref as sr

pytestmark = pytest.mark.gpu

E_ARG = -1
TAB = S.build()


def _table(segs, blocks):
    raw = cg.dev(torch.from_numpy(S.raw_table(segs)))
    bs = cg.dev(torch.tensor(blocks, dtype=torch.int32).reshape(-1))
    return raw, bs, len(blocks)


def _launch(out, wmod, ops, raw, bs, nblocks, B):
    F = _lib.fptr
    g = lambda k: F(ops.get(k))
    _lib.call('l2i_segmented_matvec_f32', F(out), g('inp'), g('in2'), g('w'), g('bias'), g('e1'), g('e2'), F(wmod), g('wrgb'), _lib.ptr(raw), _lib.ptr(bs),
              nblocks, B)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _held(tag, got, want, bound, mask):
    m = torch.from_numpy(mask)
    err, bnd, ratio = sr.worst(got.cpu()[m], torch.from_numpy(want)[m], torch.from_numpy(bound)[m])
    print('segmv %s err %.3e bound %.3e ratio %.3f' % (tag, err, bnd, ratio))
    return ratio


@pytest.mark.parametrize('B', S.BATCHES)
def test_table_rows(B):
    ops = S.make_inputs(TAB, B)
    ref = S.run(TAB['segs'], TAB['blocks'], B, **ops)
    dops = {k: cg.dev(torch.from_numpy(v)) for k, v in ops.items() if isinstance(v, np.ndarray)}
    raw, bs, nblocks = _table(TAB['segs'], TAB['blocks'])
    runs = []
    for _ in range(2):
        obuf, out = cg.guarded((ops['n_out'],))
        wbuf, wmod = cg.guarded((ops['n_wmod'],))
        _launch(out, wmod, dops, raw, bs, nblocks, B)
        torch.cuda.synchronize()
        assert cg.untouched(obuf, out) and cg.untouched(wbuf, wmod), 'the launch wrote outside out / wmod'
        runs.append((out, wmod))
    out, wmod = runs[0]
    # every element the model's masks do not own — the gaps and the stride padding inside the views — still holds the sentinel
    assert bool((out.cpu()[torch.from_numpy(~ref['out_mask'])] == sr.SENTINEL).all()), 'out: an element no block owns was written'
    assert bool((wmod.cpu()[torch.from_numpy(~ref['wmod_mask'])] == sr.SENTINEL).all()), 'wmod: an element no block owns was written'
    bad = []
    for sg, sp in zip(TAB['segs'], S.SPECS):
        m = np.zeros(ops['n_out'], bool)
        m[sg.out_off_c + B * sg.out_off_b + np.arange(B)[:, None] * sg.out_bstride + np.arange(sg.rows)[None, :]] = True
        if _held('B=%d %s' % (B, sp.id), out, ref['out'], ref['out_bound'], m) > 1.0:
            bad.append(sp.id)
    if _held('B=%d wmod' % B, wmod, ref['wmod'], ref['wmod_bound'], ref['wmod_mask']) > 1.0:
        bad.append('wmod')
    assert not bad, bad
    assert torch.equal(_bits(out), _bits(runs[1][0])) and torch.equal(_bits(wmod), _bits(runs[1][1])), 'two launches differ'
    cg.release()


def test_rsqrt_is_within_its_allowance():
    """The device rsqrtf in units of the last place against float64, over the arguments of S.probe(): the figure RSQRT_ULPS is set from."""
    pr = S.probe()
    raw, bs, nblocks = _table(pr['segs'], pr['blocks'])
    dops = dict(inp=cg.dev(torch.from_numpy(pr['inp'])), w=cg.dev(torch.from_numpy(pr['w'])))
    obuf, out = cg.guarded((S.PROBE_B,))
    _launch(out, None, dops, raw, bs, nblocks, S.PROBE_B)
    torch.cuda.synchronize()
    assert cg.untouched(obuf, out)
    got = out.cpu().numpy()
    ulps = S.ulps(got, pr['want'])
    i = int(ulps.argmax())
    print('segmv rsqrtf worst %.4f ulp at x = %.9g (got %.9g, float64 %.17g); mean %.4f ulp; allowance %d ulp'
          % (ulps[i], pr['inp'].reshape(-1, 4)[i, 0], got[i], pr['want'][i], ulps.mean(), S.RSQRT_ULPS))
    assert np.isfinite(got).all()
    assert math.ceil(ulps.max()) + 1 <= S.RSQRT_ULPS, ulps.max()
    cg.release()


def test_refusals():
    """A null out / in / w / segs / block_seg, nblocks <= 0 or B <= 0: L2I_E_ARG before any launch, nothing written."""
    B = 2
    ops = S.make_inputs(TAB, B)
    dops = {k: cg.dev(torch.from_numpy(v)) for k, v in ops.items() if isinstance(v, np.ndarray)}
    raw, bs, nblocks = _table(TAB['segs'], TAB['blocks'])
    obuf, out = cg.guarded((ops['n_out'],))
    wbuf, wmod = cg.guarded((ops['n_wmod'],))
    F, P = _lib.fptr, _lib.ptr
    full = dict(out=F(out), inp=F(dops['inp']), in2=F(dops['in2']), w=F(dops['w']), bias=F(dops['bias']), e1=F(dops['e1']), e2=F(dops['e2']),
                wmod=F(wmod), wrgb=F(dops['wrgb']), segs=P(raw), block_seg=P(bs), nblocks=nblocks, B=B)

    def refuse(**change):
        a = dict(full, **change)
        cg.refused(E_ARG, 'l2i_segmented_matvec_f32', a['out'], a['inp'], a['in2'], a['w'], a['bias'], a['e1'], a['e2'], a['wmod'], a['wrgb'], a['segs'],
                   a['block_seg'], a['nblocks'], a['B'], outs=(obuf, wbuf))
    for name in ('out', 'inp', 'w', 'segs', 'block_seg'):
        refuse(**{name: None})
    for change in (dict(nblocks=0), dict(nblocks=-3), dict(B=0), dict(B=-1)):
        refuse(**change)
    cg.release()
