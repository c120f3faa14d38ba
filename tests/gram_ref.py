"""Float64 numpy model of l2i_gram_loss_f32 and l2i_gram_bwd_f32 (include/l2i.h), written once: tests/test_gram_ref_cpu.py pins it to
BP.py's expressions, tests/test_gram_gpu.py holds the kernels to it.

The model is written the way the kernels are built (32-wide tile pairs i <= j, HW slices, a mirror, a mask, a coefficient, an optional add)
so that each of those steps can be broken on purpose: ``MISTAKES`` names the planted faults, and the CPU test shows that every one of them is
visible at the shapes the GPU test runs.
"""
import numpy as np

# (B, C, H, W) of the GPU contract and what each exercises
SHAPES = [
    (1, 64, 64, 64),      # many HW slices
    (2, 128, 8, 8),       # HW smaller than a slice
    (3, 32, 7, 9),        # scalar path, ragged tail, one tile
    (1, 512, 4, 12),      # 136 tile pairs, few pixels
    (2, 96, 20, 12),      # three tiles a side
]

MISTAKES = ('no_mirror', 'last_slice_dropped', 'no_relu', 'no_mask', 'wrong_norm', 'coef_off_by_2', 'accumulate_overwrites', 'scale_of_sample_0')

U = 2.0 ** -24          # unit roundoff of fp32
SLICE = 256             # the model's HW slice (only 'last_slice_dropped' can see it)


def make_case(shape, seed=0):
    """Inputs of one shape as float32 arrays: c (about half active), a target Gram of another map, a symmetric D for the backward, the trunk
    gradient to accumulate into, the upstream scale as one element and as one per sample."""
    b, ch, h, w = shape
    r = np.random.RandomState(1000 * seed + ch + h * w)
    c = r.randn(b, ch, h * w).astype(np.float32)
    other = np.maximum(r.randn(b, ch, h * w), 0.0)
    gt = (other @ other.transpose(0, 2, 1) / (ch * h * w)).astype(np.float32)
    d = r.randn(b, ch, ch) * 0.1
    d = (0.5 * (d + d.transpose(0, 2, 1))).astype(np.float32)
    d = np.maximum(d, d.transpose(0, 2, 1))                # symmetric to the bit
    g0 = r.randn(b, ch, h * w).astype(np.float32)
    scale = np.array([0.7310585975646973], dtype=np.float32)
    scale_b = (0.5 + r.rand(b)).astype(np.float32) * np.where(np.arange(b) % 2, -1, 1).astype(np.float32)
    return dict(c=c, gt=gt, d=d, g0=g0, scale=scale, scale_b=scale_b)


def gram_loss(c, gt=None, mistake=None):
    """c [B, C, HW] -> dict(G, D, loss, absG): G = relu(c) relu(c)^T / (C HW); with gt also D = G - gt and loss[b] = C^2 sum D^2.  absG =
    sum_k |F_ik F_jk| / (C HW), the scale of the summation error bound."""
    assert mistake in (None,) + MISTAKES
    c = np.asarray(c, dtype=np.float64)
    b, ch, hw = c.shape
    f = c if mistake == 'no_relu' else np.maximum(c, 0.0)
    norm = float(ch * hw) if mistake != 'wrong_norm' else float(hw)
    t = ch // 32
    edges = list(range(0, hw, SLICE)) + [hw]
    if mistake == 'last_slice_dropped' and len(edges) > 1:
        edges = edges[:-1] if len(edges) > 2 else [0, max(hw - hw // 4 - 1, 0)]     # a single slice loses its tail instead
    G = np.zeros((b, ch, ch))
    A = np.zeros((b, ch, ch))
    for i in range(t):
        for j in range(i, t):
            fi, fj = f[:, 32 * i:32 * i + 32], f[:, 32 * j:32 * j + 32]
            tile = np.zeros((b, 32, 32))
            atile = np.zeros((b, 32, 32))
            for s0, s1 in zip(edges[:-1], edges[1:]):
                tile += fi[:, :, s0:s1] @ fj[:, :, s0:s1].transpose(0, 2, 1)
                atile += np.abs(fi[:, :, s0:s1]) @ np.abs(fj[:, :, s0:s1]).transpose(0, 2, 1)
            G[:, 32 * i:32 * i + 32, 32 * j:32 * j + 32] = tile / norm
            A[:, 32 * i:32 * i + 32, 32 * j:32 * j + 32] = atile / norm
            if j != i and mistake != 'no_mirror':
                G[:, 32 * j:32 * j + 32, 32 * i:32 * i + 32] = (tile / norm).transpose(0, 2, 1)
                A[:, 32 * j:32 * j + 32, 32 * i:32 * i + 32] = (atile / norm).transpose(0, 2, 1)
    out = dict(G=G, absG=A, D=None, loss=None)
    if gt is not None:
        D = G - np.asarray(gt, dtype=np.float64)
        out['D'] = D
        out['loss'] = float(ch * ch) * (D * D).sum((1, 2))
    return out


def gram_bwd(c, d, scale=None, g0=None, mistake=None):
    """-> dict(g, absg): g = [g0 +] coef * scale * (c > 0) * (d relu(c)), coef = 4 C / HW, scale of 1 element (every sample) or B (one per
    sample); absg = coef |scale| sum_k |d_ik F_kp|."""
    assert mistake in (None,) + MISTAKES
    c = np.asarray(c, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    b, ch, hw = c.shape
    f = c if mistake == 'no_relu' else np.maximum(c, 0.0)
    coef = 4.0 * ch / hw * (0.5 if mistake == 'coef_off_by_2' else 1.0)
    s = np.ones(1) if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
    assert s.size in (1, b)
    if mistake == 'scale_of_sample_0':
        s = s[:1]
    s = np.broadcast_to(s, (b,)).reshape(b, 1, 1)
    v = coef * s * (d @ f)
    a = coef * np.abs(s) * (np.abs(d) @ np.abs(f))
    if mistake != 'no_mask':
        v = np.where(c > 0, v, 0.0)
        a = np.where(c > 0, a, 0.0)
    if g0 is not None and mistake != 'accumulate_overwrites':
        v = v + np.asarray(g0, dtype=np.float64)
    return dict(g=v, absg=a)


def gram_bound(ref, hw):
    """|G - model| allowed per entry: the any-order summation bound over HW terms, + 2 for the product's and the normaliser's roundings."""
    return (hw + 2) * U * ref['absG']


def loss_bound(ref, ch, hw, gt):
    """|loss - model| allowed per sample: relative (C^2 + HW + 4) u on the sums, plus what an error of gram_bound (+ one rounding of the
    subtraction) in every D entry moves the loss by: C^2 sum (2 |D| e + e^2)."""
    e = gram_bound(ref, hw)
    e = e + U * (np.abs(ref['D']) + e)
    return (ch * ch + hw + 4) * U * ref['loss'] + float(ch * ch) * (2.0 * np.abs(ref['D']) * e + e * e).sum((1, 2))


def bwd_bound(ref, ch, g0=None):
    """|g - model| allowed per entry: the summation bound over the C-long sums (+ 2: coef * scale and its product with the sum), and one
    rounding of the add when accumulating."""
    bound = (ch + 2) * U * ref['absg']
    if g0 is not None:
        bound = bound + U * (np.abs(ref['g']) + bound)
    return bound
