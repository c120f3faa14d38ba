"""The float64 model of the identity-preservation loss of walk training (--id_loss; latent2im_amd/facenet.py:FaceIdFn, csrc/l2i_face.hip) and of
the three kernels it adds, each kernel result with a per-element bound on what a float32 evaluation IN ANY SUMMATION ORDER may differ by.  Test
infrastructure: never imported by the product.

    level(x) = ((x + 1) * 0.5) * 255 in float32 (the operation order of clip_ims),  u = min(max(level, 0), 255), NaN -> 0
    r        = Ry u Rx^T per plane, horizontal pass first; Rx, Ry = the 22-bit tables of tests/facenet_ref.resize_tables / 2^22
    e        = F.normalize(w_t^T mean_hw(trunk(r)) + bias)
    loss_id  = mean_b (1 - cos(e1_b, e0_b)),  e0 a constant

Bounds, with u = 2^-24 and gamma_m <= 1.0001 m u (Higham, Accuracy and Stability, 3.1-3.2; a fused multiply-add only removes roundings):

resize_lin   level is evaluated in float32 by the model as by the kernel, so u_in is exact; a coefficient k 2^-22 is exact in float32 (|k| < 2^24).
             Every input passes the horizontal sum (kx products and additions), one store, and the vertical sum (ky):
                 |r^ - r| <= (kx + ky + 4) u sum |wy||wx||u_in|.
adjoint      gx = 127.5 [0 < level < 255] Rx^T (Ry^T gy): the same two sums over the inverse taps (kx', ky' = the most outputs one input pixel
             feeds) and the product with 127.5: (kx' + ky' + 4) u 127.5 sum |wy||wx||gy| where the mask passes, 0 where it does not (the mask is a
             function of the float32 level: exact for given inputs).
head_bwd     first-order propagation through p = mean_hw feat (HW additions, one product), t = w_t^T p + bias (C), the three dot products of length
             E (|t|^2, |v|^2, e . v^), g_t = -g (v^ - c e) / n and the C x E mat-vec g_p = w_t g_t; the constants are rounded up (m + 4 for a sum of
             m terms) to cover the second-order terms, which are u times smaller.
"""
import numpy as np
import torch
import torch.nn.functional as F

from latent2im_amd import face_specs as specs
from tests import facenet_ref as R

U = 2.0 ** -24
FACE = 160
MISTAKES_RESIZE = ('tables_swapped',)
MISTAKES_ADJOINT = ('tables_swapped', 'no_127_5', 'mask_ignored')
MISTAKES_HEAD = ('e0_leak', 'proj_dropped', 'no_inv_hw')


# ---- tables -----------------------------------------------------------------------------------------------------------------------------------
def dense(in_size, out_size):
    """(R [out, in] float64 = the taps / 2^22, k = the most taps of one output, k' = the most outputs one input feeds)."""
    b, c = R.resize_tables(in_size, out_size)
    m = np.zeros((out_size, in_size))
    for o, (first, n) in enumerate(b):
        m[o, first:first + n] = c[o, :n].astype(np.float64) / float(1 << 22)
    return m, int(b[:, 1].max()), int((m != 0).sum(0).max())


def inverse_tables(in_size, out_size):
    """The inverse tables the adjoint kernel reads, built from the forward ones by brute force: bounds int32 [in, 2] = (first output, count),
    coefficients int32 [in, k']."""
    b, c = R.resize_tables(in_size, out_size)
    hit = [[] for _ in range(in_size)]
    for o, (first, n) in enumerate(b):
        for t in range(n):
            hit[first + t].append((o, int(c[o, t])))
    k = max(1, max(len(h) for h in hit))
    ib, ic = np.zeros((in_size, 2), np.int32), np.zeros((in_size, k), np.int32)
    for i, h in enumerate(hit):
        if h:
            assert [o for o, _ in h] == list(range(h[0][0], h[0][0] + len(h)))
            ib[i] = (h[0][0], len(h))
            ic[i, :len(h)] = [v for _, v in h]
    return ib, ic


# ---- the two resize kernels ---------------------------------------------------------------------------------------------------------------------
def level(x):
    """((x + 1) * 0.5) * 255 in float32, as float64."""
    x = np.asarray(x, np.float32)
    return ((x + np.float32(1.0)) * np.float32(0.5) * np.float32(255.0)).astype(np.float64)


def clip255(x):
    with np.errstate(invalid='ignore'):
        t = level(x)
        return np.where(np.isnan(t), 0.0, np.minimum(np.maximum(t, 0.0), 255.0))


def _fit(m, cols):
    """m [out, n] -> [out, cols]: taps past the image read nothing, pixels past the table are never read."""
    out = np.zeros((m.shape[0], cols))
    out[:, :min(cols, m.shape[1])] = m[:, :min(cols, m.shape[1])]
    return out


def _matrices(h, w, oh, ow, mistake):
    """(Ry [oh, h], Rx [ow, w], ky, kx, ky', kx'); 'tables_swapped': each pass reads the other axis' table (visible where H != W)."""
    ry, ky, kyi = dense(h, oh)
    rx, kx, kxi = dense(w, ow)
    if mistake == 'tables_swapped':
        ry, rx = _fit(dense(w, oh)[0], h), _fit(dense(h, ow)[0], w)
    return ry, rx, ky, kx, kyi, kxi


def resize_lin(x, out_hw=(FACE, FACE), mistake=None):
    """(r, bound) of l2i_face_resize_lin_f32: x [..., H, W] -> [..., OH, OW]."""
    ry, rx, ky, kx, _, _ = _matrices(x.shape[-2], x.shape[-1], out_hw[0], out_hw[1], mistake)
    u = clip255(x)
    return ry @ u @ rx.T, (kx + ky + 4) * U * (np.abs(ry) @ np.abs(u) @ np.abs(rx).T)


def pass_mask(x):
    t = level(x)
    with np.errstate(invalid='ignore'):
        return (t > 0.0) & (t < 255.0)


def resize_lin_bwd(gy, x, mistake=None):
    """(gx, bound) of l2i_face_resize_lin_bwd_f32: gy [..., OH, OW], x [..., H, W]."""
    gy = np.asarray(gy, np.float64)
    ry, rx, _, _, ky, kx = _matrices(x.shape[-2], x.shape[-1], gy.shape[-2], gy.shape[-1], mistake)
    m = np.ones(x.shape, bool) if mistake == 'mask_ignored' else pass_mask(x)
    s = 1.0 if mistake == 'no_127_5' else 127.5
    return s * m * (ry.T @ gy @ rx), (kx + ky + 4) * U * 127.5 * m * (np.abs(ry).T @ np.abs(gy) @ np.abs(rx))


# ---- the head ---------------------------------------------------------------------------------------------------------------------------------
def head(feat, w_t, bias):
    """feat [B, C, HW] -> (e [B, E], t [B, E], n [B, 1], p [B, C]) in float64 (l2i_face_head_f32)."""
    p = np.asarray(feat, np.float64).mean(2)
    t = p @ np.asarray(w_t, np.float64) + np.asarray(bias, np.float64)
    n = np.maximum(np.sqrt((t * t).sum(1, keepdims=True)), 1e-12)
    return t / n, t, n, p


def head_bwd(feat, w_t, bias, v, g_dist, mistake=None):
    """(g_feat [B, C, HW], bound) of l2i_face_head_bwd_f32."""
    feat, w_t, bias, v = (np.asarray(a, np.float64) for a in (feat, w_t, bias, v))
    g = np.asarray(g_dist, np.float64).reshape(-1, 1)
    B, C, HW = feat.shape
    E = w_t.shape[1]
    e, t, n, p = head(feat, w_t, bias)
    vn = np.sqrt((v * v).sum(1, keepdims=True))
    vh = v / vn
    c = (e * vh).sum(1, keepdims=True)
    d = vh - (0.0 if mistake == 'proj_dropped' else c * e)
    g_t = -g * d / n
    if mistake == 'e0_leak':                             # the gradient that belongs to v lands on t as well
        g_t = g_t - g * (e - c * vh) / vn
    g_p = g_t @ w_t.T
    g_feat = np.repeat((g_p if mistake == 'no_inv_hw' else g_p / HW)[:, :, None], HW, 2)
    # bounds
    aw = np.abs(w_t)
    dp = (HW + 1) * U * np.abs(feat).sum(2) / HW
    dt = (C + 4) * U * (np.abs(p) @ aw + np.abs(bias)) + dp @ aw
    dn = ((E + 4) / 2.0 + 1) * U * n + (np.abs(t) * dt).sum(1, keepdims=True) / n
    de = dt / n + np.abs(t) * dn / n ** 2 + U * np.abs(e)
    dvh = ((E + 4) / 2.0 + 2) * U * np.abs(vh)
    dc = (E + 4) * U * (np.abs(e) * np.abs(vh)).sum(1, keepdims=True) + (np.abs(vh) * de).sum(1, keepdims=True) + (np.abs(e) * dvh).sum(1, keepdims=True)
    dd = dvh + dc * np.abs(e) + np.abs(c) * de + U * np.abs(c * e) + U * np.abs(d)
    dgt = np.abs(g) / n * dd + np.abs(g_t) * (dn / n + 3 * U)
    dgp = (E + 4) * U * (np.abs(g_t) @ aw.T) + dgt @ aw.T
    bound = dgp / HW + U * np.abs(g_p) / HW
    return g_feat, np.repeat(bound[:, :, None], HW, 2)


# ---- the whole term in torch (autograd) ---------------------------------------------------------------------------------------------------------
def embed_t(P, x):
    """tests/facenet_ref.embed restated on tensors: that one takes its input through numpy (``torch.as_tensor(np.asarray(x))``), which detaches
    it, so it is not autograd-clean; the layers are its own (``_bconv``), P: name -> tensor of x's dtype."""
    for name, _, _, _, stride, pad in specs.FACENET_STEM:
        x = R._bconv(P, name, x, stride, pad)
        if name == 'conv2d_2b':
            x = F.max_pool2d(x, 3, 2)
    for prefix, kind, scale, relu in specs.FACENET_TRUNK:
        branches = specs.FACENET_MIXED[prefix] if kind == 'mixed' else specs.FACENET_BLOCKS[kind][1]
        outs = []
        for br in branches:
            y = x
            for suffix, _, _, _, stride, pad in br:
                y = R._bconv(P, prefix + '.' + suffix, y, stride, pad)
            outs.append(y)
        if kind == 'mixed':
            x = torch.cat(outs + [F.max_pool2d(x, 3, 2)], 1)
        else:
            y = F.conv2d(torch.cat(outs, 1), P[prefix + '.conv2d.weight'], P[prefix + '.conv2d.bias'])
            x = y * scale + x
            if relu:
                x = F.relu(x)
    x = F.adaptive_avg_pool2d(x, 1).flatten(1)
    x = x @ P['last_linear.weight'].t()
    x = F.batch_norm(x, P['last_bn.running_mean'], P['last_bn.running_var'], P['last_bn.weight'], P['last_bn.bias'], False, 0.0, specs.FACENET_BN_EPS)
    return F.normalize(x, p=2, dim=1)


def resize_lin_t(x, dtype, out_hw=(FACE, FACE)):
    """resize_lin on a tensor (autograd), all of it in ``dtype``: in float64 the level differs from the kernel's float32 one by its two roundings,
    which the clamp does not amplify; the mask could differ only for a pixel within that of a clamp edge (the fixture's maker asserts none is)."""
    ry = torch.as_tensor(dense(x.shape[-2], out_hw[0])[0], dtype=dtype)
    rx = torch.as_tensor(dense(x.shape[-1], out_hw[1])[0], dtype=dtype)
    t = (x.to(dtype) + 1.0) * 0.5 * 255.0
    u = torch.nan_to_num(torch.clamp(t, 0.0, 255.0), nan=0.0)
    return ry @ u @ rx.t()


def id_loss(loss_of_r, x0, x1, dtype=torch.float64):
    """(loss, d loss / d x1, d loss / d r1, e0, e1) of loss = mean_b (1 - cos(e(r1), e(r0).detach())) with e = ``loss_of_r``'s embedding function:
    x0, x1 float32 arrays [B, 3, R, R]."""
    x1 = torch.tensor(np.asarray(x1, np.float32)).to(dtype).requires_grad_(True)
    with torch.no_grad():
        e0 = loss_of_r(resize_lin_t(torch.tensor(np.asarray(x0, np.float32)), dtype))
    r1 = resize_lin_t(x1, dtype)
    r1.retain_grad()
    e1 = loss_of_r(r1)
    loss = (1.0 - F.cosine_similarity(e1, e0, dim=1)).mean()
    loss.backward()
    return loss.item(), x1.grad.double().numpy(), r1.grad.double().numpy(), e0.double().numpy(), e1.detach().double().numpy()


def face_params(state, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items() if not k.endswith('num_batches_tracked')}


# ---- the fixture (tests/golden/make_faceid.py) --------------------------------------------------------------------------------------------------
CASES = (('up64', 64, 11), ('down256', 256, 12))          # (name, R, seed): batch 2, images 0.8 N(0, 1) so that clamping is exercised


def case_images(res, seed, batch=2):
    rs = np.random.RandomState(seed)
    n0, n1 = rs.randn(batch, 3, res, res), rs.randn(batch, 3, res, res)
    x0 = (0.8 * n0).astype(np.float32)
    x1 = (0.8 * (0.9 * n0 + np.sqrt(1 - 0.81) * n1)).astype(np.float32)          # the edit: correlated with the original, 0.8 N(0, 1) itself
    return x0, x1


def gradient_rule(dev32):
    """The pass rule of tests/test_facenet_gpu.py::test_embeddings_vs_float64 for a quantity relative to its largest magnitude: twice the
    float32 restatement's own deviation (the factor 2 is for the other summation order), floored at 1e-4."""
    return max(2.0 * dev32, 1e-4)


def loss_bound(loss_dev32, E=specs.FACENET_EMBED):
    """|loss^ - loss|: twice the float32 restatement's own deviation of the loss (the rule of the gradient), floored at what float32 alone costs
    the last step, the dot product of two unit vectors of length E in any order: (E + 4) u sum |e1||e0| <= (E + 4) u = 3.1e-5."""
    return max(2.0 * loss_dev32, (E + 4) * U)
