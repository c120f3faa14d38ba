"""One numpy model of what the resident regressor trainer adds on the device (csrc/l2i_repack.hip, the finalize kernels of csrc/l2i_train.hip):
the gather that rewrites every packed form of a convolution weight, the fixed-order float64 Winograd weight transform, the uint8 -> float32
normalisation of a device-resident batch and the [C]-sized BatchNorm algebra, with the bounds the GPU tests hold the kernels to.  Bounds are
derived from unit roundoff here and nowhere tuned: where a value is an exact function of its inputs the condition is bit equality.

Shared by tests/test_regtrain_ref_cpu.py (the model against the torch packing code of latent2im_amd/conv.py, no GPU) and the GPU tests of the
kernels."""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32 (round to nearest): |fl(x) - x| <= U32 |x|
MAX_TAPS = 49

# conv kinds every repack test walks: (name, Cout, Cin, K, stride, padding)
KINDS = (('1x1 16->40', 40, 16, 1, 1, 0), ('3x3 s1 16->16', 16, 16, 3, 1, 1), ('3x3 s2 p1 16->32', 32, 16, 3, 2, 1),
         ('1x1 s2 16->64', 64, 16, 1, 2, 0), ('7x7 s2 p3 3->64', 64, 3, 7, 2, 3))


def round_up(n, m):
    return (n + m - 1) // m * m


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
def gather(w, taps, swap, pad_to=32, oihw=False, mistake=None):
    """l2i_repack_taps_f32 as an index map.  w [Cout, Cin, K, K]; rows = Cout if swap else Cin, cols the other one; cols_p = cols rounded up
    to ``pad_to`` (32: conv.pack_weight; 4: the dense packs of the VALU kernels).
    packed:  dst[r, t, c] = w[r, c, ky_t, kx_t] if swap else w[c, r, ky_t, kx_t] for c < cols, 0 for cols <= c < cols_p
    oihw:    dst[r, c, t] likewise, no padding.
    ``mistake``: one of MISTAKES — a wrong kernel the mistake table must catch."""
    w = np.asarray(w, dtype=np.float32)
    cout, cin, k, _ = w.shape
    if mistake == 'swapped role':
        swap = not swap                      # (with unequal channel counts the result does not even have the shape)
    rows, cols = (cout, cin) if swap else (cin, cout)
    cols_p = cols if oihw else round_up(cols, pad_to)
    fill = np.float32(np.nan) if mistake == 'unfilled padding' else np.float32(0)
    dst = np.full((rows, len(taps), cols_p), fill, dtype=np.float32)
    for t, (ky, kx) in enumerate(taps):
        if mistake == 'missed flip':
            ky, kx = k - 1 - ky, k - 1 - kx
        if mistake == 'wrong parity tap' and t == len(taps) - 1:
            ky = (ky + 1) % k
        plane = w[:, :, ky, kx]                                   # [Cout, Cin]
        dst[:, t, :cols] = plane if swap else plane.T
    return dst.transpose(0, 2, 1).copy() if oihw else dst


MISTAKES = ('swapped role', 'missed flip', 'wrong parity tap', 'unfilled padding')


def taps_forward(k):
    return [(ky, kx) for ky in range(k) for kx in range(k)]


def taps_grad_s1(k):
    """The stride-1 input gradient is the correlation with the flipped, role-swapped weight."""
    return [(k - 1 - ky, k - 1 - kx) for ky in range(k) for kx in range(k)]


def phase_axis(k, pad, parity):
    """Taps of a stride-2 transposed conv (o = 2 i + t - pad) that land on outputs of this parity, in correlation order (the last first), or None."""
    k0 = (parity + pad) % 2
    ks = list(range(k0, k, 2))
    return ks[::-1] if ks else None


def taps_parity(k, pad, py, px):
    ty, tx = phase_axis(k, pad, py), phase_axis(k, pad, px)
    return None if ty is None or tx is None else [(a, b) for a in ty for b in tx]


# ---- Winograd weight transforms ------------------------------------------------------------------------------------------------------------
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64)


def wino_u(w, G):
    """U = G g G^T [Cout, Cin, M, M] in float64 in the kernel's order: rows first (k ascending), then columns (l ascending), each product and
    sum a float64 operation of its own (numpy's elementwise * and + never fuse), zeros of G multiplied like every entry; rounded once to fp32."""
    g = np.asarray(w, dtype=np.float32).astype(np.float64)
    M = G.shape[0]
    T = np.empty(g.shape[:2] + (M, 3), dtype=np.float64)
    for i in range(M):
        for l in range(3):
            T[:, :, i, l] = (G[i, 0] * g[:, :, 0, l] + G[i, 1] * g[:, :, 1, l]) + G[i, 2] * g[:, :, 2, l]
    U = np.empty(g.shape[:2] + (M, M), dtype=np.float64)
    for i in range(M):
        for j in range(M):
            U[:, :, i, j] = (T[:, :, i, 0] * G[j, 0] + T[:, :, i, 1] * G[j, 1]) + T[:, :, i, 2] * G[j, 2]
    return U.astype(np.float32)


def conv_view(w, swap, flip):
    """The [cout', cin', 3, 3] weight of the launch a pack belongs to: roles swapped and taps reversed for the stride-1 gradient."""
    w = np.asarray(w, dtype=np.float32)
    if swap:
        w = w.transpose(1, 0, 2, 3)
    return np.ascontiguousarray(w[:, :, ::-1, ::-1] if flip else w)


def wino2_pack(w, swap=False, flip=False):
    """conv.pack_weight_wino's layout [Cin, 4 (i), CoutP, 4 (j)] of the model's U."""
    U = wino_u(conv_view(w, swap, flip), G2)
    cout, cin = U.shape[:2]
    p = np.zeros((cin, 4, round_up(cout, 32), 4), dtype=np.float32)
    p[:, :, :cout, :] = U.transpose(1, 2, 0, 3)
    return p


def wino4_pack(w, swap=False, flip=False):
    """conv.pack_weight_wino4's layout [Cin/4][CoutP/16][ [6 i][4 k][16 m][4 j] ++ [6 i][4 k][16 m][2 j] ] of the model's U."""
    U0 = wino_u(conv_view(w, swap, flip), G4)
    cout, cin = U0.shape[:2]
    coutp = round_up(cout, 32)
    U = np.zeros((coutp, cin, 6, 6), dtype=np.float32)
    U[:cout] = U0
    U = U.reshape(coutp // 16, 16, cin // 4, 4, 6, 6).transpose(2, 0, 4, 3, 1, 5)          # [c4, mb, i, k, m, j]
    a = U[..., :4].reshape(cin // 4, coutp // 16, -1)
    b = U[..., 4:].reshape(cin // 4, coutp // 16, -1)
    return np.concatenate([a, b], axis=2)


def ulp_distance(a, b):
    """Distance in units in the last place between two float32 arrays (finite values of equal sign or zero)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return np.abs(key(a) - key(b))


def derived_tensors(fc):
    """{name: tensor} of everything a conv.FrozenConv2d derived from its weight — what repack_ must rewrite where it lies (the forward launch's
    w_src is the weight itself: not a pack)."""
    out = {}
    for i, L in enumerate(fc.fwd + fc.bwd):
        if L is None:
            continue
        for a in ('w', 'w4', 'wino', 'wino4') + (('w_src',) if i > 0 else ()):
            if getattr(L, a) is not None:
                out['launch%d.%s' % (i, a)] = getattr(L, a)
    for name, F in (('fused', fc.bwd_fused), ('small', fc.bwd_small)):
        if F is not None:
            out[name + '.w'] = F.w
            if getattr(F, 'w_src', None) is not None:
                out[name + '.w_src'] = F.w_src
    return out


# ---- the device-resident batch -------------------------------------------------------------------------------------------------------------
def normalise(u8):
    """l2i_batch_from_u8_f32 per element: fl(fl(u / 255) - 0.5) * 2 in float32 (the last product is exact)."""
    a = np.asarray(u8, dtype=np.uint8).astype(np.float32) / np.float32(255.0)
    return (a - np.float32(0.5)) * np.float32(2.0)


def batch_from_u8(src, labels, idx):
    """out[b] = normalise(src[idx[b]]), label[b] = labels[idx[b]]; an index outside [0, N) gives zeros."""
    src = np.asarray(src, dtype=np.uint8)
    out = np.zeros((len(idx),) + src.shape[1:], dtype=np.float32)
    lab = np.zeros((len(idx), labels.shape[1]), dtype=np.float32)
    for b, j in enumerate(idx):
        if 0 <= j < len(src):
            out[b], lab[b] = normalise(src[j]), labels[j]
    return out, lab


# ---- BatchNorm finalize ----------------------------------------------------------------------------------------------------------------------
def bn_finalize(s, q, n, weight, bias, running_mean, running_var, eps=1e-5, momentum=0.1):
    """l2i_bn_finalize_f32: float64 sums s, q over n values per channel -> dict of float32 arrays.  Every operation is one numpy operation."""
    s, q = np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    m64 = s / n
    var = np.maximum(q / n - m64 * m64, 0.0)
    mean, invstd = f32(m64), f32(1.0 / np.sqrt(var + eps))
    scale = f32(weight) * invstd
    shift = f32(bias) - mean * scale
    keep, mom = np.float32(1.0 - momentum), np.float32(momentum)
    rm = f32(running_mean) * keep + mom * mean
    rv = f32(running_var) * keep + mom * f32(var * (n / max(n - 1, 1)))
    return dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv)


def bn_bwd_finalize(s, q, n):
    """l2i_bn_bwd_finalize_f32: exact conversions of the float64 sums and of their quotients by n."""
    s, q = np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return dict(d_bias=s.astype(np.float32), d_weight=q.astype(np.float32), m_dy=(s / n).astype(np.float32), m_dyxh=(q / n).astype(np.float32))


def bn_finalize_bounds(ref, running_var, momentum=0.1):
    """Absolute bounds on |kernel - model| (and |today's torch expression - model|) per output, given an invstd that is within 1 ulp of the
    model's (a correctly rounded float64 1 / sqrt and torch's rsqrt both are: each is within a few float64 ulps of the true value before the
    one rounding to float32, which can at most move the result to the neighbouring float32).  u = U32; an ulp is at most 2 u |x|.
      invstd   1 ulp:                          2 u |invstd|
      scale    = fl(weight * invstd'):         |weight| * 2 u |invstd| propagated, + u |scale| for the final rounding on either side -> (2 + 2) u |scale|
      shift    = fl(bias - fl(mean * scale')): the product moves by <= 4 u |mean scale| with scale', + u for its rounding on either side (2 u);
                                               the difference is rounded once on either side: 2 u |shift| -> 6 u |mean scale| + 2 u |shift|
      running  = fl(fl(r * keep) + fl(m * x)): the inputs are bit-equal (mean and the unbiased variance are exact conversions), so the sides differ
                                               only by contraction of one product into the sum (torch's add_ with alpha may fuse it): the product's
                                               rounding u |m x| and the sum's rounding on either side 2 u |result|."""
    a = lambda k: np.abs(np.asarray(ref[k], dtype=np.float64))
    ms = np.abs(np.asarray(ref['mean'], dtype=np.float64) * np.asarray(ref['scale'], dtype=np.float64))
    mom = momentum
    var_u = np.abs((np.asarray(ref['running_var'], dtype=np.float64) - (1 - mom) * np.asarray(running_var, dtype=np.float64)))      # = mom * unbiased variance
    return dict(invstd=2 * U32 * a('invstd'), scale=4 * U32 * a('scale'), shift=6 * U32 * ms + 2 * U32 * a('shift'),
                running_mean=U32 * mom * a('mean') + 2 * U32 * a('running_mean') + 1e-45,
                running_var=U32 * 1.0001 * var_u + 2 * U32 * a('running_var') + 1e-45)
