"""Float64 model of l2i_reg_bce_f32 (include/l2i.h, csrc/l2i_loss.hip): the regressor head, its BCE term and d loss / d feat, with the bounds the
kernel is held to, a numpy float32 restatement of its arithmetic, the cases and the planted mistakes.  tests/test_regbce_ref_cpu.py pins them on
the CPU, tests/test_regbce_contract_gpu.py holds the kernel to them.

    p[b, k]   = sum_i feat[b, i] fc_w[cols[k], i] + fc_b[cols[k]],   q = 1 - p
    loss      = -mean_bk( y log(max(p, eps)) + (1 - y) log(max(q, eps)) )                       eps = fp32(1e-12)
    g_pred    = a / p [p >= eps] - c / q [q >= eps],   a = -y / (B K),  c = -(1 - y) / (B K)      (torch.clamp passes the gradient where >= eps)
    g_feat[b] = sum_k g_pred[b, k] fc_w[cols[k]]
A NaN prediction is NaN in preds, makes the loss NaN (torch.clamp keeps a NaN, and so does its log) and contributes 0 to g_feat (both
comparisons are false).

The bounds count roundings, u = 2^-24; none is fitted.
  p       each of 256 threads runs a chain of ceil(F / 256) fused multiply-adds; a 64-lane butterfly (6 additions), the four waves (2) and the
          bias (1) follow:  d p <= u (ceil(F / 256) + 16) sum|x w| + u |p|;  d p = 0 where sum|x w| = 0 (feat[b] = 0: p IS the bias)
  q       fl(1 - p):  d q = d p + u |q|
  g_pred  first order through a / p and c / q, a and c rounded to fp32 (u), the division (u), the subtraction (u on the sum of the two):
          d g = |a| d p / p^2 + |c| d q / q^2 + 3 u (|a / p| + |c / q|)                                  (terms the clamp stops drop out)
  g_feat  d g_feat[b, i] <= sum_k (d g_k |w_ki| + u (K + 1) |g_k w_ki|)                              (K fused multiply-adds, in any order)
  loss    sum_bk (|y| d log p + |1 - y| d log q) / (B K), d log p = d p / (p - d p) + 2 u LOGF_ULPS |log p| where p >= eps and
          2 u LOGF_ULPS |log eps| where the clamp holds; the float64 products and the float64 sum add 2^-50 of sum|terms|.
LOGF_ULPS is the one measured constant: the device logf is not correctly rounded.  tests/test_regbce_contract_gpu.py measures it on exact
rows — B = K = 1, feat = 0, y = 1, so that loss = -logf(max(fc_b, eps)) alone — at LOG_PROBE arguments over the range the cases use, and
requires ceil(worst) + 1 <= LOGF_ULPS.  Measured on an MI355X: see LOGF_MEASURED below.

A plain module: no fixtures, no GPU, no kernel code."""
import collections

import numpy as np

U = 2.0 ** -24
EPS = np.float32(1e-12)
LOGF_ULPS = 3                 # ceil(LOGF_MEASURED) + 1
LOGF_MEASURED = 1.9150        # worst |logf - float64| in units of the last place of the result over log_probe(), MI355X (mean 0.54)
# the biases of the exact rows: the clamp's edge, just below it, beyond it; 1 - p at its edge (q = 2^-24 passes), on it (q = 0), beyond it; the middle
EDGES = np.array([EPS, np.nextafter(EPS, np.float32(0)), 0.0, -0.25, 1.0 - 2.0 ** -24, 1.0, 1.5, 0.5], dtype=np.float32)
EDGE_NAMES = ('eps', 'below_eps', 'zero', 'negative', 'one_minus_u', 'one', 'above_one', 'half')
MISTAKES = ('clamp_grad_passes', 'boundary_excluded', 'mean_over_b_only', 'cols_ignored', 'bias_dropped', 'nan_clamped')
KINDS = ('exact', 'random', 'nan')

Shape = collections.namedtuple('Shape', 'B F A K cols')
_perm70 = np.random.RandomState(70).permutation(70)
SHAPES = (
    Shape(1, 256, 4, 1, (0,)),
    Shape(3, 300, 40, 5, (1, 3, 9, 20, 38)),                                   # F is no multiple of 256
    Shape(8, 2048, 40, 40, tuple(range(40))),
    Shape(2, 2048, 70, 64, tuple(int(c) for c in _perm70[:63]) + (int(_perm70[5]),)),      # unsorted, one column twice
)
Case = collections.namedtuple('Case', 'id shape kind tf64')
CASES = tuple(Case('%dx%dx%dx%d_%s_%s' % (s.B, s.F, s.A, s.K, kind, 'f64' if tf64 else 'f32'), s, kind, tf64)
              for s in SHAPES for kind in KINDS for tf64 in (True, False))


def make_case(case, seed=0):
    """-> dict(feat [B, F], fc_w [A, F], fc_b [A] float32, cols [K] int64, target [B, K] float64 or float32, nan_row).
    'exact': feat = 0 and fc_b[a] = EDGES[a % 8], so p = fc_b[cols] bit for bit.  'random': fc_b = 0.5 and every feat[b] rescaled so that the
    float64 |dot| <= 0.39 over the selected columns: p stays in [0.1, 0.9], more than 0.1 from either clamp edge.  'nan': 'random' with one NaN
    feature in the last row.  A sixth of the targets are exactly 0, a sixth exactly 1."""
    s = case.shape
    rng = np.random.RandomState(1000 * seed + s.F + 7 * s.K + KINDS.index(case.kind))
    fc_w = (rng.standard_normal((s.A, s.F)) / np.sqrt(s.F)).astype(np.float32)
    cols = np.array(s.cols, dtype=np.int64)
    y = rng.uniform(0, 1, (s.B, s.K))
    pick = rng.uniform(size=y.shape)
    y[pick < 1 / 6] = 0.0
    y[pick > 5 / 6] = 1.0
    y.reshape(-1)[:2] = (1.0, 0.0)[:y.size]
    target = y if case.tf64 else y.astype(np.float32)
    nan_row = None
    if case.kind == 'exact':
        feat = np.zeros((s.B, s.F), np.float32)
        fc_b = EDGES[np.arange(s.A) % 8].copy()
    else:
        feat = rng.standard_normal((s.B, s.F))
        dots = feat @ fc_w[cols].astype(np.float64).T
        feat = (feat * (0.39 / np.abs(dots).max(1, keepdims=True))).astype(np.float32)
        fc_b = np.full(s.A, 0.5, np.float32)
        if case.kind == 'nan':
            nan_row = s.B - 1
            feat[nan_row, s.F // 3] = np.nan
    return dict(feat=feat, fc_w=fc_w, fc_b=fc_b, cols=cols, target=target, nan_row=nan_row)


def model(c, mistake=None):
    """-> dict(preds, preds_bound (None on rows where p is the bias bit for bit), loss, loss_bound, g_feat, g_feat_bound), float64."""
    assert mistake is None or mistake in MISTAKES
    feat, fc_w, fc_b, y = (np.asarray(c[k], dtype=np.float64) for k in ('feat', 'fc_w', 'fc_b', 'target'))
    B, F = feat.shape
    K = len(c['cols'])
    cols = np.arange(K) if mistake == 'cols_ignored' else c['cols']
    eps = float(EPS)
    w = fc_w[cols]                                          # [K, F]
    with np.errstate(invalid='ignore', divide='ignore'):
        p = feat @ w.T + (0.0 if mistake == 'bias_dropped' else fc_b[cols][None, :])
        Mp = np.abs(feat) @ np.abs(w).T
        dp = np.where(Mp == 0, 0.0, U * (-(-F // 256) + 16) * Mp + U * np.abs(p))
        q = 1.0 - p
        dq = dp + U * np.abs(q)
        n = B if mistake == 'mean_over_b_only' else B * K
        a, cc = -y / n, -(1.0 - y) / n
        if mistake == 'clamp_grad_passes':
            pp, pq = ~np.isnan(p), ~np.isnan(p)
        elif mistake == 'boundary_excluded':
            pp, pq = p > eps, q > eps
        else:
            pp, pq = p >= eps, q >= eps
        tp, tq = np.where(pp, a / p, 0.0), np.where(pq, cc / q, 0.0)
        g = tp - tq
        dg = np.where(pp, np.abs(a) * dp / p ** 2, 0.0) + np.where(pq, np.abs(cc) * dq / q ** 2, 0.0) + 3 * U * (np.abs(tp) + np.abs(tq))
        g_feat = g @ w
        g_feat_bound = dg @ np.abs(w) + U * (K + 1) * (np.abs(g) @ np.abs(w))
        isn = np.isnan(p)
        pc = np.where(isn, eps if mistake == 'nan_clamped' else np.nan, np.maximum(p, eps))
        qc = np.where(isn, eps if mistake == 'nan_clamped' else np.nan, np.maximum(q, eps))
        lp, lq = np.log(pc), np.log(qc)
        dlp = np.where(p >= eps, dp / (p - dp), 0.0) + 2 * U * LOGF_ULPS * np.abs(lp)
        dlq = np.where(q >= eps, dq / (q - dq), 0.0) + 2 * U * LOGF_ULPS * np.abs(lq)
        loss = -(y * lp + (1.0 - y) * lq).sum() / n
        loss_bound = ((np.abs(y) * dlp + np.abs(1.0 - y) * dlq).sum() + 2.0 ** -50 * (np.abs(y * lp) + np.abs((1.0 - y) * lq)).sum()) / (B * K)
    exact = bool((Mp == 0).all())
    return dict(preds=p, preds_bound=None if exact else dp, loss=float(loss), loss_bound=float(loss_bound), g_feat=g_feat, g_feat_bound=g_feat_bound,
                g_pred=g)


def ratio(got, want, bound):
    """Worst |got - want| / bound with NaNs required where the model has them; an error against a zero bound, or a stray non-finite value, is
    infinitely far out.  bound None: equal bits of the float32 values (NaN equal to NaN)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return float('inf')
    if bound is None:
        return 0.0 if np.array_equal(got[~wn].astype(np.float32).view(np.int32), want[~wn].astype(np.float32).view(np.int32)) else float('inf')
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        err = np.abs(got - want)[~wn]
        r = np.where(err == 0, 0.0, err / bound[~wn])
    return float(np.nan_to_num(r, nan=np.inf, posinf=np.inf).max()) if r.size else 0.0


# ---- the kernel's arithmetic in numpy float32 --------------------------------------------------------------------------------------------------
def _fma(x, w, acc):
    return (x.astype(np.float64) * w.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def float32(c, order='kernel'):
    """'kernel': thread t adds the features t, t + 256, .. ascending, a butterfly over each wave's 64 lanes (xor 32, 16, .. 1), (w0 + w1) + (w2 + w3),
    the bias; g_feat with k ascending.  'reversed': one chain over the features descending; g_feat with k descending.
    -> dict(preds, loss, g_feat): float32, float64, float32."""
    f32 = np.float32
    feat, fc_w, fc_b, cols = c['feat'], c['fc_w'], c['fc_b'], c['cols']
    y = np.asarray(c['target'], dtype=np.float64)
    B, F = feat.shape
    K = len(cols)
    w = fc_w[cols]
    with np.errstate(invalid='ignore', divide='ignore'):
        if order == 'kernel':
            lanes = np.zeros((B, K, 256), f32)
            for i0 in range(0, F, 256):
                n = min(256, F - i0)
                lanes[:, :, :n] = _fma(feat[:, None, i0:i0 + n], w[None, :, i0:i0 + n], lanes[:, :, :n])
            v = lanes.reshape(B, K, 4, 64)
            for off in (32, 16, 8, 4, 2, 1):
                v = v + v[..., np.arange(64) ^ off]
            s = (v[:, :, 0, 0] + v[:, :, 1, 0]) + (v[:, :, 2, 0] + v[:, :, 3, 0])
        else:
            s = np.zeros((B, K), f32)
            for i in range(F - 1, -1, -1):
                s = _fma(feat[:, None, i], w[None, :, i], s)
        p = s + fc_b[cols][None, :]
        inv_n = 1.0 / (float(B) * float(K))
        a, cc = (-y * inv_n).astype(f32), (-(1.0 - y) * inv_n).astype(f32)
        q = f32(1.0) - p
        g = np.where(p >= EPS, a / p, f32(0)) - np.where(q >= EPS, cc / q, f32(0))
        g = g.astype(f32)
        gf = np.zeros((B, F), f32)
        for k in (range(K) if order == 'kernel' else range(K - 1, -1, -1)):
            gf = _fma(g[:, k:k + 1], w[k][None, :], gf)
        pc, qc = np.where(p < EPS, EPS, p), np.where(q < EPS, EPS, q)          # a NaN stays
        loss = -(y * np.log(pc).astype(np.float64) + (1.0 - y) * np.log(qc).astype(np.float64)).sum() * inv_n
    return dict(preds=p, loss=float(loss), g_feat=gf)


# ---- the logf probe ----------------------------------------------------------------------------------------------------------------------------
LOG_PROBE = 512


def log_probe():
    """The LOG_PROBE biases whose logf the exact rows return alone (B = K = 1, feat = 0, y = 1: loss = -logf(max(bias, eps))): the values the
    exact rows take, then uniform over [0.1, 0.9], where the random rows' p and q lie.  -> (bias float32, want float64 = log(max(bias, eps)))."""
    rng = np.random.RandomState(11)
    b = rng.uniform(0.1, 0.9, LOG_PROBE).astype(np.float32)
    edge = np.array([EPS, 2.0 ** -24, 1.0 - 2.0 ** -24, 1.25, 1.5, 0.5, 1.0], dtype=np.float32)
    b[:len(edge)] = edge
    return b, np.log(np.maximum(b, EPS).astype(np.float64))


def ulps(got, want):
    """|got - want| in units of the last place of fl32(want) (of the smallest normal number at want = 0)."""
    want32 = np.maximum(np.abs(want.astype(np.float32)), np.finfo(np.float32).tiny)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(want32).astype(np.float64)
