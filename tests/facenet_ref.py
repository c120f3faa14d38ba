"""CPU restatements the face-identity tests compare against (plain torch / numpy; of the product only the layer table face_specs.py):

* ``resize_tables`` / ``resize_uint8``: PIL's ``Image.resize((160, 160))`` of an RGB image (bicubic a = -0.5, antialias support
  2 * max(in/out, 1), coefficients normalised in double and rounded to 22-bit fixed point, horizontal pass to a uint8 intermediate, then the
  vertical pass) — pinned to PIL bit for bit by tests/test_facenet_cpu.py.
* ``clip_ims``: the reference's float32 quantisation (graph.clip_ims / eval.py).
* ``embed``: facenet_pytorch ``InceptionResnetV1`` in eval mode restated from the public architecture, in any float dtype (float64 is the
  oracle), from the state dict by its key names.
* ``cosine``: scipy.spatial.distance.cosine as scipy 1.15 computes it (``correlation(u, v, centered=False)``), restated so that the suite
  does not load scipy (and a second OpenBLAS) into the test process; pinned to values scipy printed (tests/test_facenet_cpu.py).
* ``identity_metric``: eval.py:170-209 (cosine distance per bucket entry, sums and 1 - mean per non-empty bucket).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from latent2im_amd import face_specs as specs


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_tables(in_size, out_size):
    """(bounds int32 [out, 2] = (first tap, tap count), coefficients int32 [out, ksize]) of one axis."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) / filterscale) for x in range(xmax)]
        ww = sum(w)
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[i, x] = int(-0.5 + k * (1 << 22)) if k < 0 else int(0.5 + k * (1 << 22))
        bounds[i] = (xmin, xmax)
    return bounds, kk


def _pass(img, bounds, kk):
    """One axis (the last) of uint8 [..., in] -> uint8 [..., out]."""
    out = np.empty(img.shape[:-1] + (bounds.shape[0],), np.uint8)
    src = img.astype(np.int64)
    for i, (xmin, n) in enumerate(bounds):
        acc = (1 << 21) + (src[..., xmin:xmin + n] * kk[i, :n].astype(np.int64)).sum(-1)
        out[..., i] = np.clip(acc >> 22, 0, 255)
    return out


def resize_uint8(img_chw, size=160):
    """uint8 [C, H, W] -> uint8 [C, size, size], PIL's resize of the HWC image."""
    c, h, w = img_chw.shape
    if (h, w) == (size, size):
        return img_chw.copy()
    mid = _pass(img_chw, *resize_tables(w, size))                                   # horizontal
    return np.swapaxes(_pass(np.swapaxes(mid, 1, 2), *resize_tables(h, size)), 1, 2)      # vertical


def clip_ims(ims):
    return np.uint8(np.clip(((ims + 1) / 2.0) * 255, 0, 255))


def face_input(img_f32_nchw, size=160):
    """The reference's identity input: clip_ims, PIL resize, raw 0..255 float values [B, 3, size, size] (float32)."""
    q = clip_ims(np.asarray(img_f32_nchw, dtype=np.float32))
    return np.stack([resize_uint8(x, size) for x in q]).astype(np.float32)


def _bconv(P, prefix, x, stride, pad):
    w = P[prefix + '.conv.weight']
    x = F.conv2d(x, w, stride=stride, padding=pad)
    x = F.batch_norm(x, P[prefix + '.bn.running_mean'], P[prefix + '.bn.running_var'], P[prefix + '.bn.weight'], P[prefix + '.bn.bias'],
                     False, 0.0, specs.FACENET_BN_EPS)
    return F.relu(x)


def embed(state, x, dtype=torch.float64):
    """[B, 3, 160, 160] raw 0..255 -> unit embeddings [B, 512] (InceptionResnetV1.forward, classify=False, eval mode)."""
    P = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items() if not k.endswith('num_batches_tracked')}
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    for name, _, _, _, stride, pad in specs.FACENET_STEM:
        x = _bconv(P, name, x, stride, pad)
        if name == 'conv2d_2b':
            x = F.max_pool2d(x, 3, 2)
    for prefix, kind, scale, relu in specs.FACENET_TRUNK:
        branches = specs.FACENET_MIXED[prefix] if kind == 'mixed' else specs.FACENET_BLOCKS[kind][1]
        outs = []
        for br in branches:
            y = x
            for suffix, _, _, _, stride, pad in br:
                y = _bconv(P, prefix + '.' + suffix, y, stride, pad)
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
    x = F.batch_norm(x, P['last_bn.running_mean'], P['last_bn.running_var'], P['last_bn.weight'], P['last_bn.bias'], False, 0.0,
                     specs.FACENET_BN_EPS)
    return F.normalize(x, p=2, dim=1)


def cosine(u, v):
    """scipy 1.15 ``cosine(u, v)`` of two 1-D float64 vectors: 1 - uv / sqrt(uu * vv), clipped to [0, 2] (the dot products as numpy sums,
    not BLAS calls)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    assert u.ndim == 1 and u.shape == v.shape, 'Input vector should be 1-D'
    uv, uu, vv = float(np.sum(u * v)), float(np.sum(u * u)), float(np.sum(v * v))
    return float(np.clip(1.0 - uv / math.sqrt(uu * vv), 0.0, 2.0))


def identity_metric(pairs_per_call):
    """eval.py:170-209.  ``pairs_per_call``: one entry per (batch, target attribute) call, each three lists (buckets) of
    (edited embedding, original embedding).  ``sim`` is never reset; returns (results, results_avg, bucket sizes)."""
    sim = [[], [], []]
    for call in pairs_per_call:
        for k in range(3):
            for e, o in call[k]:
                sim[k].append(cosine(np.asarray(e, np.float64).reshape(-1), np.asarray(o, np.float64).reshape(-1)))
    results, results_avg = [], []
    for k in range(3):
        if len(sim[k]) == 0:
            continue
        results.append(np.sum(sim[k]))
        results_avg.append(1 - np.mean(sim[k]))
    return results, results_avg, [len(s) for s in sim]
