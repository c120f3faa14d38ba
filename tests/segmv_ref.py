"""Float64 model of l2i_segmented_matvec_f32 (include/l2i.h, csrc/l2i_modulation.hip) that executes device-format segment tables, the bounds the
kernel is held to, a numpy float32 restatement of its arithmetic, a hand-built table that reaches the code the product's tables do not, and the
planted mistakes.  tests/test_segmv_ref_cpu.py pins all of it on the CPU, tests/test_segmv_contract_gpu.py holds the kernel to it;
tests/emu.py:emulate_segmented_matvec delegates here.

    out[b, r] = epi( sum over parts  sum_k pre(in)[b, k] * w[w_off + k * w_pitch + r] )          (pre and epi: include/l2i.h)

`run` returns, per output element, the value, the mask of elements written, and the bound.  M = sum_k |pre(x)_k| |W_kr| over both parts (plus
|bias| for epi 0); for pre 3 |pre(x)_k| is the sum of the three absolute products.  The bounds count roundings, u = 2^-24; none is fitted:
  acc        the contraction is K_tot fused multiply-adds in four chains that meet in three additions: in any order
             |acc - exact| <= (K_tot + C_SUM + p) u M, C_SUM = 4 (the three additions, one for second-order terms), p the roundings the
             staged input carries against |pre(x)|: pre 0: 0; pre 1 (v v): 1; pre 2 ((v d) d): 2; pre 3 (three products, two additions): 3
  epi 3      the bound of acc;  epi 0: one more addition, (K_tot + C_SUM + p + 1) u M with |bias| in M
  epi 1      v = rsqrt(s), s = fl(acc + fl32(1e-8)): relative.  d v / v = -1/2 d s / s, d s <= bound(acc) + u |s|, and the device rsqrtf is not
             correctly rounded: RSQRT_ULPS units in the last place of v, one such unit at most 2 u |v|.
             |got - v| <= |v| (bound(acc) / (2 s) + u / 2 + 2 u RSQRT_ULPS + u)          (the last u: second order)
  epi 2      v = e1 - e2 acc by propagation: |e2| bound(acc) + u t + u (|e1| + t), t = |e2| (|acc| + bound(acc)): the product's rounding, then the
             subtraction's (one rounding less where the compiler fuses the two)
  wmod       wr v, one more product: |wr| bound(v) + u |wr| (|v| + bound(v))
RSQRT_ULPS is the one measured constant: tests/test_segmv_contract_gpu.py sweeps 4096 arguments over [1e-9, 1e3] (and 0) through an epi-1
segment with K = 4 and one-hot weights, which returns rsqrtf(x + 1e-8) alone, and requires ceil(worst) + 1 <= RSQRT_ULPS.  Measured on an
MI355X: see RSQRT_MEASURED below.

A plain module: no fixtures, no GPU, no kernel code."""
import collections
import ctypes

import numpy as np

from latent2im_amd import _lib

U = 2.0 ** -24
C_SUM = 4
PRE_ROUNDINGS = {0: 0, 1: 1, 2: 2, 3: 3}
RSQRT_ULPS = 2                # ceil(RSQRT_MEASURED) + 1
RSQRT_MEASURED = 0.7809       # worst |rsqrtf - float64| in units of the last place of the result over probe(), MI355X (mean 0.27)
EPS32 = float(np.float32(1e-8))
BATCHES = (1, 8, 9, 17)
MISTAKES = ('second_part_dropped', 'tail_k_dropped', 'second_pass_stale', 'pre2_unsquared', 'epi1_eps_dropped', 'off_b_unscaled', 'pre3_plane_order',
            'rgb_from_unbiased')

# id, rows, ((K, pre), ..), epi, ToRGB weights
Spec = collections.namedtuple('Spec', 'id rows parts epi rgb')
SPECS = (
    Spec('rows1_k4', 1, ((4, 0),), 3, False),                          # three of the four waves get no work
    Spec('rows64_k64_bias', 64, ((64, 0),), 0, False),                # a quarter of exactly one 16-step
    Spec('rows65_k20_demod', 65, ((20, 1),), 1, False),               # quarter 8: waves at 0-8, 8-16, 16-20, 20-20; a second row block of one row
    Spec('rows96_two_parts', 96, ((512, 0), (68, 2)), 2, False),      # quarter 20 = 16 + 4: a tail after the 16-step loop
    Spec('rows40_k36_rgbred', 40, ((36, 3),), 3, False),              # quarter 12: the tail alone
    Spec('rows130_k512_torgb', 130, ((512, 0),), 0, True),            # three row blocks, the last of two rows
)
BLOCK_ORDER = (7, 2, 9, 0, 4, 6, 1, 8, 3, 5)        # the (segment, row block) list is launched in this order


def wave_ranges(K):
    """The k range of each of the four waves, restated from the kernel."""
    kq = (((K >> 2) + 3) >> 2) << 2
    return [(min(w * kq, K), min(min(w * kq, K) + kq, K)) for w in range(4)]


def build():
    """-> dict(segs: [SegmvSeg], blocks: [(segment, row block)] shuffled, size: {buffer: B -> elements}, region: segment id -> the input span of
    its first part as (constant half, per-sample half, per-sample footprint)).  Every segment has w_pitch > rows, out_bstride > rows and
    non-zero constant and per-sample halves of its input and output offsets (e_off too where it is read)."""
    segs, region = [], {}
    in_c, in_b, out_c, out_b, w_off, bias_off = 3, 2, 5, 1, 3, 2
    aux = 6
    rgb_w_off = aux + 3 * 36 + 1
    wrgb_size = rgb_w_off + 3 * 130 + 2
    for si, sp in enumerate(SPECS):
        sg = _lib.SegmvSeg()
        sg.rows, sg.nparts, sg.epi = sp.rows, len(sp.parts), sp.epi
        sg.out_off_c, sg.out_off_b, sg.out_bstride = out_c, out_b, sp.rows + 3
        out_c, out_b = out_c + 4, out_b + sg.out_bstride
        sg.bias_off = bias_off
        if sp.epi == 0:
            bias_off += sp.rows + 3
        sg.e_off_c, sg.e_off_b, sg.e_bstride = 7, 11, sp.rows + 2
        sg.rgb_off_b, sg.rgb_w_off = (2, rgb_w_off) if sp.rgb else (-1, 0)
        for pi, (K, pre) in enumerate(sp.parts):
            foot = 3 * K if pre == 3 else K + 5
            pitch = sp.rows + 1 + pi
            sg.part[pi] = _lib.SegmvPart(K, in_c, in_b, 0 if pre == 3 else foot, pitch, pre, aux if pre == 3 else 0, 0, w_off)
            if pi == 0:
                region[sp.id] = (in_c, in_b, foot)
            in_c, in_b, w_off = in_c + 8, in_b + foot, w_off + K * pitch + 3
        segs.append(sg)
    blocks = [(i, rb) for i, sp in enumerate(SPECS) for rb in range((sp.rows + 63) // 64)]
    assert len(blocks) == len(BLOCK_ORDER)
    blocks = [blocks[i] for i in BLOCK_ORDER]
    fin_c, fin_b, fout_c, fout_b, fw, fbias = in_c, in_b, out_c, out_b, w_off, bias_off
    size = {'in': lambda B: fin_c + B * fin_b + 8, 'out': lambda B: fout_c + B * fout_b + 9, 'w': lambda B: fw + 5, 'bias': lambda B: fbias + 4,
            'e': lambda B: 7 + B * 11 + B * 98 + 6, 'wrgb': lambda B: wrgb_size, 'wmod': lambda B: B * 2 + B * 3 * 130 + 7}
    return dict(segs=segs, blocks=blocks, size=size, region=region)


def raw_table(segs):
    """The device bytes of a segment list (uint8 numpy)."""
    arr = (_lib.SegmvSeg * len(segs))(*segs)
    return np.frombuffer(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr)), dtype=np.uint8).copy()


def parse_table(raw):
    raw = bytes(np.asarray(raw, dtype=np.uint8).tobytes())
    return (_lib.SegmvSeg * (len(raw) // ctypes.sizeof(_lib.SegmvSeg))).from_buffer_copy(raw)


def make_inputs(tab, B, seed=0):
    """float32 operands for the hand-built table at batch B: N(0, 1) inputs, weights N(0, 1) / sqrt(K) (non-negative for the demodulation
    segment, whose bound is relative), in2 in [0.5, 1.5).  The demodulation segment's input of one sample is all zeros: rsqrt(1e-8) there."""
    rng = np.random.RandomState(100 * seed + B)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    n = {k: fn(B) for k, fn in tab['size'].items()}
    ops = dict(inp=f(rng.standard_normal(n['in'])), in2=f(rng.uniform(0.5, 1.5, n['in'])), w=f(rng.standard_normal(n['w']) / 8),
               bias=f(rng.standard_normal(n['bias'])), e1=f(rng.standard_normal(n['e'])), e2=f(rng.standard_normal(n['e'])),
               wrgb=f(rng.standard_normal(n['wrgb'])))
    for sg, sp in zip(tab['segs'], SPECS):
        if sp.epi == 1:
            pt = sg.part[0]
            span = slice(int(pt.w_off), int(pt.w_off) + pt.K * pt.w_pitch)
            ops['w'][span] = np.abs(ops['w'][span])
    c, pb, foot = tab['region']['rows65_k20_demod']
    zero = zero_sample(B)
    ops['inp'][c + B * pb + zero * foot:c + B * pb + (zero + 1) * foot] = 0.0
    ops['n_out'], ops['n_wmod'] = n['out'], n['wmod']
    return ops


def zero_sample(B):
    """The sample whose demodulation input is all zeros: the single sample of the second accumulator pass where there is one."""
    return 8 if B > 8 else B - 1


def _idx(a, i):
    i = np.asarray(i)
    assert i.min() >= 0 and i.max() < a.shape[0], 'a table offset leaves its buffer'
    return a[i]


def run(segs, blocks, B, inp, w, in2=None, bias=None, e1=None, e2=None, wrgb=None, n_out=None, n_wmod=None, mistake=None):
    """Execute the table in float64, block by block as the grid does.  -> dict(out, out_mask, out_bound, out_M, wmod, wmod_mask, wmod_bound);
    elements no block writes are NaN in out / wmod and False in the masks.  Two blocks that write one element are an AssertionError."""
    assert mistake is None or mistake in MISTAKES
    d = lambda a: None if a is None else np.asarray(a, dtype=np.float64).reshape(-1)
    i1, i2, W, bi, E1, E2, wr = d(inp), d(in2), d(w), d(bias), d(e1), d(e2), d(wrgb)
    out, ob, oM, om = np.full(n_out, np.nan), np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, bool)
    wm = wb = wmask = None
    if n_wmod is not None:
        wm, wb, wmask = np.full(n_wmod, np.nan), np.zeros(n_wmod), np.zeros(n_wmod, bool)
    bcol = np.arange(B)[:, None]
    bsrc = bcol % 8 if mistake == 'second_pass_stale' else bcol
    Bs = 1 if mistake == 'off_b_unscaled' else B
    for si, rb in blocks:
        sg = segs[si]
        r = np.arange(rb * 64, min(rb * 64 + 64, sg.rows))
        assert len(r) > 0, 'a block past the rows of its segment'
        acc, M = np.zeros((B, len(r))), np.zeros((B, len(r)))
        ktot = p = 0
        for pi in range(1 if mistake == 'second_part_dropped' else sg.nparts):
            pt = sg.part[pi]
            assert pt.K % 4 == 0 and 0 < pt.K <= 512
            base = pt.in_off_c + Bs * pt.in_off_b
            k = np.arange(pt.K)[None, :]
            if pt.pre == 3:
                plane = (lambda q: pt.aux_off + k * 3 + q) if mistake == 'pre3_plane_order' else (lambda q: pt.aux_off + q * pt.K + k)
                terms = [_idx(i2, base + (bsrc * pt.K + k) * 3 + q) * _idx(wr, plane(q)) for q in range(3)]
                x, ax = sum(terms), sum(np.abs(t) for t in terms)
            else:
                idx = base + bsrc * pt.in_bstride + k
                x = _idx(i1, idx)
                if pt.pre == 1:
                    x = x * x
                elif pt.pre == 2:
                    x = x * _idx(i2, idx) * (1.0 if mistake == 'pre2_unsquared' else _idx(i2, idx))
                ax = np.abs(x)
            Wm = _idx(W, pt.w_off + k.T * pt.w_pitch + r[None, :])
            if mistake == 'tail_k_dropped':
                keep = np.zeros(pt.K)
                for k0, k1 in wave_ranges(pt.K):
                    keep[k0:k0 + (k1 - k0) // 16 * 16] = 1.0
                x = x * keep
            acc, M = acc + x @ Wm, M + ax @ np.abs(Wm)
            ktot, p = ktot + pt.K, max(p, PRE_ROUNDINGS[pt.pre])
        bacc = (ktot + C_SUM + p) * U * M
        v, bv = acc, bacc
        if sg.epi == 0:
            bb = _idx(bi, sg.bias_off + r)[None, :]
            v, M = acc + bb, M + np.abs(bb)
            bv = (ktot + C_SUM + p + 1) * U * M
        elif sg.epi == 1:
            s = acc + (0.0 if mistake == 'epi1_eps_dropped' else EPS32)
            with np.errstate(divide='ignore', invalid='ignore'):
                v = 1.0 / np.sqrt(s)
                bv = np.abs(v) * (0.5 * bacc / s + 0.5 * U + 2 * U * RSQRT_ULPS + U)
        elif sg.epi == 2:
            ei = sg.e_off_c + B * sg.e_off_b + bcol * sg.e_bstride + r[None, :]
            a1, a2 = _idx(E1, ei), _idx(E2, ei)
            v = a1 - a2 * acc
            t = np.abs(a2) * (np.abs(acc) + bacc)
            bv = np.abs(a2) * bacc + U * t + U * (np.abs(a1) + t)
        oi = sg.out_off_c + B * sg.out_off_b + bcol * sg.out_bstride + r[None, :]
        assert oi.min() >= 0 and oi.max() < n_out, 'an output offset leaves its buffer'
        assert not om[oi].any(), 'two blocks write the same output'
        out[oi], ob[oi], oM[oi], om[oi] = v, bv, M, True
        if sg.epi == 0 and sg.rgb_off_b >= 0:
            src = acc if mistake == 'rgb_from_unbiased' else v
            for q in range(3):
                wi = B * sg.rgb_off_b + bcol * 3 * sg.rows + q * sg.rows + r[None, :]
                assert wi.min() >= 0 and wi.max() < n_wmod, 'a wmod offset leaves its buffer'
                assert not wmask[wi].any(), 'two blocks write the same wmod element'
                wq = _idx(wr, sg.rgb_w_off + q * sg.rows + r)[None, :]
                wm[wi], wb[wi], wmask[wi] = wq * src, np.abs(wq) * bv + U * np.abs(wq) * (np.abs(v) + bv), True
    return dict(out=out, out_mask=om, out_bound=ob, out_M=oM, wmod=wm, wmod_mask=wmask, wmod_bound=wb)


def ratio(got, want, bound, mask):
    """Worst |got - want| / bound over the elements of ``mask``; a non-finite value the model does not have is infinitely far out."""
    got = np.asarray(got, dtype=np.float64)[mask]
    want, bound = want[mask], bound[mask]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        err = np.abs(got - want)
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(q, nan=np.inf, posinf=np.inf).max()) if q.size else 0.0


# ---- the kernel's arithmetic in numpy float32 --------------------------------------------------------------------------------------------------
def _fma(x, w, acc):
    return (x.astype(np.float64) * w.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def float32(segs, blocks, B, inp, w, in2=None, bias=None, e1=None, e2=None, wrgb=None, n_out=None, n_wmod=None, order='kernel'):
    """The kernel's float32 arithmetic: 'kernel': four chains of fused multiply-adds over wave_ranges(K), k ascending, met as
    (a0 + a1) + (a2 + a3); 'reversed': one chain, k descending.  -> (out, wmod) float32, NaN where nothing is written."""
    f32 = np.float32
    out = np.full(n_out, np.nan, f32)
    wm = None if n_wmod is None else np.full(n_wmod, np.nan, f32)
    bcol = np.arange(B)[:, None]
    for si, rb in blocks:
        sg = segs[si]
        r = np.arange(rb * 64, min(rb * 64 + 64, sg.rows))
        chains = [np.zeros((B, len(r)), f32) for _ in range(4)]
        for pi in range(sg.nparts):
            pt = sg.part[pi]
            base = pt.in_off_c + B * pt.in_off_b
            k = np.arange(pt.K)[None, :]
            if pt.pre == 3:
                t = [in2[base + (bcol * pt.K + k) * 3 + q] * wrgb[pt.aux_off + q * pt.K + k] for q in range(3)]
                x = (t[0] + t[1]) + t[2]
            else:
                idx = base + bcol * pt.in_bstride + k
                x = inp[idx]
                if pt.pre == 1:
                    x = x * x
                elif pt.pre == 2:
                    x = (x * in2[idx]) * in2[idx]
            Wm = w[pt.w_off + k.T * pt.w_pitch + r[None, :]]
            assert x.dtype == f32 and Wm.dtype == f32
            if order == 'kernel':
                for c, (k0, k1) in enumerate(wave_ranges(pt.K)):
                    for kk in range(k0, k1):
                        chains[c] = _fma(x[:, kk:kk + 1], Wm[kk:kk + 1, :], chains[c])
            else:
                for kk in range(pt.K - 1, -1, -1):
                    chains[0] = _fma(x[:, kk:kk + 1], Wm[kk:kk + 1, :], chains[0])
        v = (chains[0] + chains[1]) + (chains[2] + chains[3])
        if sg.epi == 0:
            v = v + bias[sg.bias_off + r][None, :]
        elif sg.epi == 1:
            v = (1.0 / np.sqrt((v + f32(1e-8)).astype(np.float64))).astype(f32)
        elif sg.epi == 2:
            ei = sg.e_off_c + B * sg.e_off_b + bcol * sg.e_bstride + r[None, :]
            v = e1[ei] - e2[ei] * v
        out[sg.out_off_c + B * sg.out_off_b + bcol * sg.out_bstride + r[None, :]] = v
        if sg.epi == 0 and sg.rgb_off_b >= 0:
            for q in range(3):
                wm[B * sg.rgb_off_b + bcol * 3 * sg.rows + q * sg.rows + r[None, :]] = wrgb[sg.rgb_w_off + q * sg.rows + r][None, :] * v
    return out, wm


# ---- the rsqrtf probe ---------------------------------------------------------------------------------------------------------------------------
PROBE_B = 4096


def probe():
    """A one-segment table (rows 1, K 4, pre 0, epi 1) whose one-hot weight column makes out[b] = rsqrtf(fl(x_b + 1e-8)), and its PROBE_B
    arguments: 0, then log-uniform over [1e-9, 1e3] (the demodulation sums of the rows lie in [0, 1e2]).
    -> dict(segs, blocks, inp [PROBE_B * 4], w [4], want float64 [PROBE_B])."""
    sg = _lib.SegmvSeg()
    sg.rows, sg.nparts, sg.epi, sg.out_bstride, sg.rgb_off_b = 1, 1, 1, 1, -1
    sg.part[0] = _lib.SegmvPart(4, 0, 0, 4, 1, 0, 0, 0, 0)
    rng = np.random.RandomState(7)
    x = np.exp(rng.uniform(np.log(1e-9), np.log(1e3), PROBE_B)).astype(np.float32)
    x[0] = 0.0
    inp = np.zeros((PROBE_B, 4), np.float32)
    inp[:, 0] = x
    s = (x + np.float32(1e-8)).astype(np.float64)          # one IEEE addition, as on the device
    return dict(segs=[sg], blocks=[(0, 0)], inp=inp.reshape(-1), w=np.array([1, 0, 0, 0], np.float32), want=1.0 / np.sqrt(s))


def ulps(got, want):
    """|got - want| in units of the last place of fl32(want)."""
    want32 = np.abs(want.astype(np.float32))
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(want32).astype(np.float64)
