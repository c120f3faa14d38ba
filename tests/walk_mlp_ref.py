"""The float64 model of the PGGAN graph's MLP walk (WalkMlpZ3, graphs/pggan/transform_base.py:167-188) and of the two kernels it runs on
(l2i_linear_rows_f32 / l2i_linear_rows_bwd_f32, csrc/l2i_walk.hip): numpy forward and backward, each result with a per-element bound on what a
float32 evaluation IN ANY SUMMATION ORDER may differ by.  Test infrastructure: never imported by the product.

    z_new = z + alpha * L3(lrelu(L2(lrelu(L1(z)))))         L_i(x) = x W_i^T + b_i,  lrelu(v) = v > 0 ? v : 0.2 v,  alpha [B, 1]

Bounds, with u = 2^-24 (round to nearest, float32) and gamma_m = m u / (1 - m u) <= 1.0001 m u for every m used here:

forward   v = sum_k x_k w_k + b: K products and K additions in some order.  Every term passes through at most K + 1 roundings (its product, then at
          most K additions: Higham, Accuracy and Stability, 3.1-3.2 — a fused multiply-add only removes roundings), so
              |v^ - v| <= gamma_{K+1} (sum_k |x_k||w_k| + |b|) <= E := (K + 4) u (sum_k |x_k||w_k| + |b|).
          LRELU: lrelu is 1-Lipschitz for |slope| <= 1, so a mask that flips under the rounding of v is inside E; the product v * slope is one more
              rounding:  |y^ - y| <= E + u |y|.
          WALK:  y = r + a v: the product (u |a v|) and the addition (u |y|), or one rounding if they are fused:  |y^ - y| <= |a| E + u |a v| + u |y|.
backward  g' = g * m exactly in the model (m = 1, slope or a[b]); the kernel rounds it once.
          gW[n, k] = sum_b g'[b, n] x[b, k]: B products, B - 1 additions, the rounding of g':  <= gamma_{B+1} S <= (B + 3) u sum_b |g'||x|.
          gb[n] = sum_b g'[b, n]: B - 1 additions and the rounding of g':  <= (B + 3) u sum_b |g'|.
          gx[b, k] = sum_n g'[b, n] W[n, k] (+ add[b, k]): N products, N additions at most, the rounding of g' — in slices or not, the order is free:
              <= gamma_{N+2} S <= (N + 4) u (sum_n |g'||W| + |add|).
          The mask is taken from the sign of the given y (y > 0 ? 1 : slope; y == 0 takes the slope, as an in-place LeakyReLU's backward does):
          for given inputs it is exact, so no bound is needed for it at the kernel level.
composed  (walk_forward / walk_backward: three layers, the operands of layer i + 1 carry layer i's error) first-order propagation of the operand
          errors through the absolute values of the exact operands plus the second-order term where both factors carry an error.  A mask may flip
          where |h| <= its own bound: there g' may be off by |g| (1 - slope) on top.
"""
import numpy as np

U = 2.0 ** -24
SLOPE = 0.2
NONE, LRELU, WALK = 0, 1, 2
MISTAKES = ('bias_dropped', 'slope_001', 'alpha_on_z', 'mask_ge', 'w_transposed', 'gb_over_n')


def _d(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def lrelu(v, slope=SLOPE):
    return np.where(v > 0, v, v * slope)


def linear_fwd(x, W, b, epi=NONE, slope=SLOPE, res=None, a=None, mistake=None):
    """(y, bound) of l2i_linear_rows_f32: x [B, K], W [N, K], b [N]; WALK: res [B, N], a [B]."""
    x, W, b, res, a = _d(x), _d(W), _d(b), _d(res), _d(a)
    K = x.shape[1]
    if mistake == 'w_transposed':
        W = W.T
    if mistake == 'bias_dropped':
        b = np.zeros_like(b)
    if mistake == 'slope_001':
        slope = 0.01
    v = x @ W.T + b
    E = (K + 4) * U * (np.abs(x) @ np.abs(W).T + np.abs(b))
    if epi == LRELU:
        y = lrelu(v, slope)
        return y, E + U * np.abs(y)
    if epi == WALK:
        a = a.reshape(-1, 1)
        y = res + a * v
        if mistake == 'alpha_on_z':
            y = a * (res + v)
        return y, np.abs(a) * E + U * np.abs(a * v) + U * np.abs(y)
    return v, E


def gprime(g, epi, slope=SLOPE, y=None, a=None, mistake=None):
    g = _d(g)
    if mistake == 'slope_001':
        slope = 0.01
    if epi == LRELU:
        y = _d(y)
        return g * np.where((y >= 0) if mistake == 'mask_ge' else (y > 0), 1.0, slope)
    if epi == WALK:
        return _d(a).reshape(-1, 1) * g
    return g


def linear_bwd(g, x, W, epi=NONE, slope=SLOPE, y=None, a=None, want_gx=True, gx_add=None, mistake=None):
    """dict name -> (value, bound) of l2i_linear_rows_bwd_f32: gw [N, K], gb [N] and, when asked, gx [B, K]."""
    x, W, gx_add = _d(x), _d(W), _d(gx_add)
    B, N = np.shape(g)
    gp = gprime(g, epi, slope, y, a, mistake)
    if mistake == 'w_transposed':
        W = W.T
    out = {'gw': (gp.T @ x, (B + 3) * U * (np.abs(gp).T @ np.abs(x)))}
    gb = gp.sum(0)
    if mistake == 'gb_over_n':
        gb = np.resize(gp.sum(1), N)               # the sum over the wrong axis, recycled to the right length
    out['gb'] = (gb, (B + 3) * U * np.abs(gp).sum(0))
    if want_gx:
        add = 0.0 if gx_add is None else gx_add
        out['gx'] = (gp @ W + add, (N + 4) * U * (np.abs(gp) @ np.abs(W) + np.abs(add)))
    return out


def _np64(p):
    if hasattr(p, 'detach'):
        p = p.detach().cpu().numpy()
    return np.asarray(p, dtype=np.float64)


def params64(P):
    """The six parameters as float64 arrays (w1, b1, w2, b2, w3, b3) from a state dict with the reference's keys, or from a sequence."""
    if isinstance(P, dict):
        P = [P['linear.%d.%s' % (i, n)] for i in (0, 2, 4) for n in ('weight', 'bias')]
    return [_np64(p) for p in P]


def walk_forward(z, alpha, P, mistake=None):
    """dict of (value, bound): h1, h2, z_new — the bounds composed over the layers."""
    w1, b1, w2, b2, w3, b3 = params64(P)
    z, a = _d(z), _d(alpha).reshape(-1)
    h1, e1 = linear_fwd(z, w1, b1, LRELU, mistake=None if mistake == 'w_transposed' else mistake)
    h2, e2 = linear_fwd(h1, w2, b2, LRELU, mistake=mistake)
    e2 = e2 + e1 @ np.abs(w2 if mistake != 'w_transposed' else w2.T).T                       # lrelu is 1-Lipschitz
    zn, e3 = linear_fwd(h2, w3, b3, WALK, res=z, a=a, mistake=None if mistake == 'w_transposed' else mistake)
    e3 = e3 + np.abs(a).reshape(-1, 1) * (e2 @ np.abs(w3).T)
    return {'h1': (h1, e1), 'h2': (h2, e2), 'z_new': (zn, e3)}


def _bwd_composed(g, eg, x, ex, W, epi, y=None, ey=None, a=None, want_gx=True, gx_add=None):
    """linear_bwd where g, x (and y, for the mask) carry errors eg, ex, ey: the own bound (restated at the perturbed operands: the (B + 3) u and (N + 4) u factors on the
    propagated terms) plus first- and second-order propagation.  Returns dict name -> (value, bound)."""
    B, N = g.shape
    gp = gprime(g, epi, SLOPE, y, a)
    if epi == LRELU:
        egp = eg * np.where(y > 0, 1.0, SLOPE) + np.where(np.abs(y) <= ey, (np.abs(g) + eg) * (1.0 - SLOPE), 0.0)     # a mask that may flip
    elif epi == WALK:
        egp = np.abs(a).reshape(-1, 1) * eg
    else:
        egp = eg
    own = linear_bwd(g, x, W, epi, SLOPE, y, a, want_gx, gx_add)
    out = {'gw': (own['gw'][0], own['gw'][1] + egp.T @ np.abs(x) + np.abs(gp).T @ ex + egp.T @ ex + (B + 3) * U * (egp.T @ np.abs(x) + np.abs(gp).T @ ex + egp.T @ ex)),
           'gb': (own['gb'][0], own['gb'][1] + egp.sum(0) * (1.0 + (B + 3) * U))}
    if want_gx:
        out['gx'] = (own['gx'][0], own['gx'][1] + (egp @ np.abs(W)) * (1.0 + (N + 4) * U))
    return out


def walk_backward(z, alpha, P, g, want_gz=True):
    """Gradients of sum(z_new * g) (g [B, dim_z] = the gradient arriving at z_new, exact as given) with the composed bounds:
    dict name -> (value, bound) for linear.0.weight ... linear.4.bias and, when asked, 'z'."""
    w1, b1, w2, b2, w3, b3 = params64(P)
    z, a, g = _d(z), _d(alpha).reshape(-1), _d(g)
    f = walk_forward(z, a, P)
    (h1, e1), (h2, e2) = f['h1'], f['h2']
    zero = np.zeros_like
    l3 = _bwd_composed(g, zero(g), h2, e2, w3, WALK, a=a)
    l2 = _bwd_composed(l3['gx'][0], l3['gx'][1], h1, e1, w2, LRELU, y=h2, ey=e2)
    l1 = _bwd_composed(l2['gx'][0], l2['gx'][1], z, zero(z), w1, LRELU, y=h1, ey=e1, want_gx=want_gz, gx_add=g if want_gz else None)
    out = {'linear.0.weight': l1['gw'], 'linear.0.bias': l1['gb'], 'linear.2.weight': l2['gw'], 'linear.2.bias': l2['gb'],
           'linear.4.weight': l3['gw'], 'linear.4.bias': l3['gb']}
    if want_gz:
        out['z'] = l1['gx']
    return out


def share(got, want, bound):
    """Largest |got - want| / bound over the elements (an element with bound 0 must match exactly: inf otherwise)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0
