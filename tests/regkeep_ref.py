"""Float64 model of l2i_reg_bce_keep_f32 (include/l2i.h, csrc/l2i_loss.hip): the regressor head with its BCE term (tests/regbce_ref.py's model, by
import) and the attribute-preservation term of walk training, with the bounds the kernel is held to, a numpy float32 restatement of its arithmetic,
the cases and the planted mistakes.  tests/test_regkeep_ref_cpu.py pins them on the CPU, tests/test_regkeep_contract_gpu.py holds the kernel to them.

    p1[b, j]  = sum_i feat1[b, i] fc_w[keep[j], i] + fc_b[keep[j]],   p0 likewise on feat0,   d = p1 - p0
    keep      = sum_bj |d| / (B M)
    g_keep    = sign(d) / (B M)        0 where d = 0 (torch.abs's subgradient) and where d is NaN (keep is then NaN)
    reg, g_bce: regbce_ref's loss and g_pred on feat1, cols, target  (K = 0: reg = 0, no BCE part)
    loss      = (reg, keep, c_reg reg + w_keep keep)
    g_feat[b] = sum_k c_reg g_bce[b, k] fc_w[cols[k]] + sum_j w_keep g_keep[b, j] fc_w[keep[j]]

The bounds count roundings, u = 2^-24; none is fitted.
  p1, p0  regbce_ref's d p (the same summation: ceil(F / 256) fused multiply-adds a thread, the wave butterfly, the four waves, the bias):
          d p <= u (ceil(F / 256) + 16) sum|x w| + u |p|;  0 where sum|x w| = 0 (p IS the bias)
  d       fl32(p1 - p0):  dd = d p1 + d p0 + u |d|;  0 where feat1[b] and feat0[b] are bitwise equal (one routine, one order: p1 and p0 are the same bits)
  keep    sum_bj dd / (B M) + 2^-50 keep (the float64 sum of fp32 values and the division)
  sign    decided where d = 0 exactly or |d| > dd.  The cases hold no undecided entry (every |d| is 0 or > 2 dd: make_case looks for a draw where
          that holds and test_regkeep_ref_cpu.py asserts it), so g_keep has no bound of its own: its two roundings (1 / (B M) to fp32, times w_keep)
          are counted in g_feat
  g_feat  K + M fused multiply-adds in any order, the BCE coefficient c_reg g (one more rounding), the keep coefficient (two):
          c_reg (regbce's d g |w| part) + u (K + M + 2) sum_k |c_reg g_k w_ki| + u (K + M + 3) sum_j |w_keep g_keep_j w_ji|
  loss[2] c_reg d reg + w_keep d keep + 2^-50 (|c_reg reg| + |w_keep keep|)

A plain module: no fixtures, no GPU, no kernel code."""
import collections

import numpy as np

from tests import regbce_ref as R

U = R.U
EPS = R.EPS
KINDS = ('exact', 'random', 'equal_rows', 'nan')
MISTAKES = ('mean_over_b_only', 'sign0_is_1', 'keep_cols_ignored', 'p0_from_feat1', 'w_keep_dropped', 'c_reg_dropped', 'nan_clamped', 'bias_one_side')

Shape = collections.namedtuple('Shape', 'B F A K M cols keep c_reg w_keep')
_perm70 = np.random.RandomState(70).permutation(70)
SHAPES = (
    Shape(1, 256, 4, 1, 1, (0,), (2,), 1.0, 0.5),
    Shape(3, 300, 40, 5, 35, (1, 3, 9, 20, 38), tuple(i for i in range(40) if i not in (1, 3, 9, 20, 38)), 10.0, 0.5),          # F is no multiple of 256
    Shape(8, 2048, 40, 1, 39, (31,), tuple(i for i in range(40) if i != 31), 10.0, 0.5),                                          # the workload's head
    Shape(2, 2048, 70, 0, 64, (), tuple(int(c) for c in _perm70[:63]) + (int(_perm70[5]),), 0.0, 0.25),                           # no BCE part; unsorted, one column twice
    Shape(2, 512, 130, 64, 64, tuple(range(0, 128, 2)), tuple(range(1, 129, 2)), 10.0, 2.0),                                      # both caps
)
Case = collections.namedtuple('Case', 'id shape kind tf64')
CASES = tuple(Case('%dx%dx%dx%dx%d_%s_%s' % (s.B, s.F, s.A, s.K, s.M, kind, 'f64' if tf64 else 'f32'), s, kind, tf64)
              for s in SHAPES for kind in KINDS for tf64 in (True, False))


def _draw(case, attempt):
    s = case.shape
    rng = np.random.RandomState(100000 * attempt + s.F + 7 * s.K + 13 * s.M + KINDS.index(case.kind))
    fc_w = (rng.standard_normal((s.A, s.F)) / np.sqrt(s.F)).astype(np.float32)
    cols, keep = np.array(s.cols, dtype=np.int64), np.array(s.keep, dtype=np.int64)
    y = rng.uniform(0, 1, (s.B, s.K))
    pick = rng.uniform(size=y.shape)
    y[pick < 1 / 6] = 0.0
    y[pick > 5 / 6] = 1.0
    y.reshape(-1)[:2] = (1.0, 0.0)[:y.size]
    target = y if case.tf64 else y.astype(np.float32)
    nan_row, equal = None, ()
    if case.kind == 'exact':
        feat1 = np.zeros((s.B, s.F), np.float32)
        feat0 = feat1.copy()
        fc_b = R.EDGES[np.arange(s.A) % 8].copy()
    else:
        used = np.concatenate([cols, keep])
        feats = []
        for _ in range(2):
            f = rng.standard_normal((s.B, s.F))
            dots = f @ fc_w[used].astype(np.float64).T
            feats.append((f * (0.39 / np.abs(dots).max(1, keepdims=True))).astype(np.float32))
        feat1, feat0 = feats
        fc_b = rng.uniform(-1, 1, s.A).astype(np.float32)
        fc_b[cols] = 0.5
        if case.kind == 'equal_rows':
            equal = tuple(range(0, s.B, 2))                     # every other row, the first among them
            feat0[list(equal)] = feat1[list(equal)]
        if case.kind == 'nan':
            nan_row = s.B - 1
            feat1[nan_row, s.F // 3] = np.nan
    return dict(feat1=feat1, feat0=feat0, fc_w=fc_w, fc_b=fc_b, cols=cols, keep=keep, target=target, nan_row=nan_row, equal_rows=equal,
                c_reg=float(s.c_reg), w_keep=float(s.w_keep))


def make_case(case):
    """-> dict(feat1, feat0 [B, F], fc_w [A, F], fc_b [A] float32, cols [K], keep [M] int64, target [B, K] float64 or float32, nan_row, equal_rows,
    c_reg, w_keep).  'exact': both feature sets 0 and fc_b[a] = EDGES[a % 8]: every p is its bias bit for bit, d = 0.  'random': fc_b = 0.5 on the
    trained columns (p in [0.1, 0.9], as regbce_ref) and uniform in [-1, 1] elsewhere, every feature row rescaled so that its float64 |dot| <= 0.39 over
    the columns in use.  'equal_rows': 'random' with every other row of feat0 bitwise feat1's.  'nan': 'random' with one NaN feature in feat1's last
    row.  The first draw with no undecided sign (every |d| 0 or > 2 dd) is taken."""
    for attempt in range(32):
        c = _draw(case, attempt)
        m = model(c)
        if m['margin_ok']:
            return c
    raise AssertionError('no draw without an undecided sign for %s' % case.id)


def _bce_operands(c):
    return dict(feat=c['feat1'], fc_w=c['fc_w'], fc_b=c['fc_b'], cols=c['cols'], target=c['target'], nan_row=c['nan_row'])


def model(c, mistake=None):
    """-> dict, float64: preds / preds_bound (None on an exact case), pkeep [B, M, 2] / pkeep_bound (None on an exact case), loss [3] / loss_bound [3],
    g_feat / g_feat_bound, d, dd, g_keep, undecided (count), margin_ok (every |d| 0 or > 2 dd)."""
    assert mistake is None or mistake in MISTAKES
    feat1, feat0, fc_w, fc_b = (np.asarray(c[k], dtype=np.float64) for k in ('feat1', 'feat0', 'fc_w', 'fc_b'))
    B, F = feat1.shape
    K, M = len(c['cols']), len(c['keep'])
    c_reg, w_keep = c['c_reg'], c['w_keep']
    with np.errstate(invalid='ignore', divide='ignore'):
        if K:
            bce = R.model(_bce_operands(c))
            wc = np.abs(fc_w[c['cols']])
            g = bce['g_pred']
            dg_w = bce['g_feat_bound'] - U * (K + 1) * (np.abs(g) @ wc)                       # regbce's (d g) |w| part
            reg, reg_bound = bce['loss'], bce['loss_bound']
            cg = 1.0 if mistake == 'c_reg_dropped' else c_reg
            gf_bce, gfb_bce = cg * bce['g_feat'], c_reg * dg_w + U * (K + M + 2) * c_reg * (np.abs(g) @ wc)
        else:
            bce, reg, reg_bound, gf_bce, gfb_bce = None, 0.0, 0.0, 0.0, 0.0
        keep_cols = np.arange(M) if mistake == 'keep_cols_ignored' else c['keep']
        wk = fc_w[keep_cols]
        bk = fc_b[keep_cols][None, :]
        p1 = feat1 @ wk.T + bk
        p0 = p1.copy() if mistake == 'p0_from_feat1' else feat0 @ wk.T + (0.0 if mistake == 'bias_one_side' else bk)
        M1, M0 = np.abs(feat1) @ np.abs(wk).T, np.abs(feat0) @ np.abs(wk).T
        chain = -(-F // 256) + 16
        dp1 = np.where(M1 == 0, 0.0, U * chain * M1 + U * np.abs(p1))
        dp0 = np.where(M0 == 0, 0.0, U * chain * M0 + U * np.abs(p0))
        d = p1 - p0
        same = (np.asarray(c['feat1']).view(np.int32) == np.asarray(c['feat0']).view(np.int32)).all(1)          # bitwise equal rows: d is exactly 0
        dd = np.where(same[:, None], 0.0, dp1 + dp0 + U * np.abs(d))
        n = B if mistake == 'mean_over_b_only' else B * M
        absd = np.where(np.isnan(d), 0.0, np.abs(d)) if mistake == 'nan_clamped' else np.abs(d)
        keep = absd.sum() / n
        keep_bound = dd.sum() / (B * M) + 2.0 ** -50 * np.abs(d).sum() / (B * M)
        sign = np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0))
        if mistake == 'sign0_is_1':
            sign = np.where(d >= 0, 1.0, np.where(d < 0, -1.0, 0.0))
        g_keep = sign / n
        fin = ~np.isnan(d)
        undecided = int(((np.abs(d) > 0) & (np.abs(d) <= dd) & fin).sum())
        margin_ok = bool(((d == 0) | (np.abs(d) > 2 * dd) | ~fin).all())
        wg = 1.0 if mistake == 'w_keep_dropped' else w_keep
        g_feat = gf_bce + wg * (g_keep @ wk)
        g_feat_bound = gfb_bce + U * (K + M + 3) * w_keep * (np.abs(sign / (B * M)) @ np.abs(fc_w[c['keep']]))
        total = c_reg * reg + w_keep * keep if K else w_keep * keep
        total_bound = c_reg * reg_bound + w_keep * keep_bound + 2.0 ** -50 * (abs(c_reg * reg) + abs(w_keep * keep))
    exact = bool((M1 == 0).all() and (M0 == 0).all())
    return dict(preds=None if bce is None else bce['preds'], preds_bound=None if bce is None else bce['preds_bound'],
                pkeep=np.stack([p1, p0], -1), pkeep_bound=None if exact else np.stack([dp1, dp0], -1),
                loss=np.array([reg, keep, total]), loss_bound=np.array([reg_bound, keep_bound, total_bound]),
                g_feat=np.broadcast_to(g_feat, (B, F)).copy(), g_feat_bound=np.broadcast_to(g_feat_bound, (B, F)).copy(),
                d=d, dd=dd, g_keep=g_keep, undecided=undecided, margin_ok=margin_ok)


ratio = R.ratio


# ---- the kernel's arithmetic in numpy float32 --------------------------------------------------------------------------------------------------
def _dots32(x, w, order):
    """x [B, F] . w [M, F] -> [B, M] float32.  'kernel': thread t adds the features t, t + 256, .. ascending, a butterfly over each wave's 64 lanes,
    (w0 + w1) + (w2 + w3); 'reversed': one chain over the features descending."""
    B, F = x.shape
    M = w.shape[0]
    if order == 'kernel':
        lanes = np.zeros((B, M, 256), np.float32)
        for i0 in range(0, F, 256):
            n = min(256, F - i0)
            lanes[:, :, :n] = R._fma(x[:, None, i0:i0 + n], w[None, :, i0:i0 + n], lanes[:, :, :n])
        v = lanes.reshape(B, M, 4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[..., np.arange(64) ^ off]
        return (v[:, :, 0, 0] + v[:, :, 1, 0]) + (v[:, :, 2, 0] + v[:, :, 3, 0])
    s = np.zeros((B, M), np.float32)
    for i in range(F - 1, -1, -1):
        s = R._fma(x[:, None, i], w[None, :, i], s)
    return s


def float32(c, order='kernel'):
    """The kernel's arithmetic in numpy float32, in its own order ('kernel': g_feat over k then j ascending, the loss over b then j ascending) or in
    another ('reversed') -> dict(preds, pkeep, loss [3] float64, g_feat)."""
    f32 = np.float32
    feat1, feat0, fc_w, fc_b, cols, keep = c['feat1'], c['feat0'], c['fc_w'], c['fc_b'], c['cols'], c['keep']
    B, F = feat1.shape
    K, M = len(cols), len(keep)
    c_reg, w_keep = f32(c['c_reg']), f32(c['w_keep'])
    with np.errstate(invalid='ignore', divide='ignore'):
        coef, rows, preds, reg = [], [], None, 0.0
        if K:
            bce = R.float32(_bce_operands(c), order)
            preds, reg = bce['preds'], bce['loss']
            y = np.asarray(c['target'], dtype=np.float64)
            inv_n = 1.0 / (float(B) * float(K))
            a, cc = (-y * inv_n).astype(f32), (-(1.0 - y) * inv_n).astype(f32)
            q = f32(1.0) - preds
            g = (np.where(preds >= EPS, a / preds, f32(0)) - np.where(q >= EPS, cc / q, f32(0))).astype(f32)
            coef += [(c_reg * g[:, k]).astype(f32) for k in range(K)]
            rows += [fc_w[cols[k]] for k in range(K)]
        wk = fc_w[keep]
        p1 = (_dots32(feat1, wk, order) + fc_b[keep][None, :]).astype(f32)
        p0 = (_dots32(feat0, wk, order) + fc_b[keep][None, :]).astype(f32)
        d = (p1 - p0).astype(f32)
        inv_m = f32(1.0 / (float(B) * float(M)))
        gk = (w_keep * np.where(d > 0, inv_m, np.where(d < 0, -inv_m, f32(0)))).astype(f32)
        coef += [gk[:, j] for j in range(M)]
        rows += [wk[j] for j in range(M)]
        gf = np.zeros((B, F), f32)
        for i in (range(K + M) if order == 'kernel' else range(K + M - 1, -1, -1)):
            gf = R._fma(coef[i][:, None], rows[i][None, :], gf)
        absd = np.abs(d).astype(np.float64).reshape(-1)
        acc = 0.0
        for v in (absd if order == 'kernel' else absd[::-1]):
            acc += v
        keep_loss = acc * (1.0 / (float(B) * float(M)))
        total = float(c_reg) * reg + float(w_keep) * keep_loss if K else float(w_keep) * keep_loss
    return dict(preds=preds, pkeep=np.stack([p1, p0], -1), loss=np.array([reg, keep_loss, total]), g_feat=gf)
