"""CPU tool: evaluates the float64 model of the identity-preservation loss (tests/faceid_ref.py: the differentiable resize, the face network of
tests/facenet_ref.py with torch autograd, 1 - cos) on seeded synthetic face weights (face_specs.facenet_state) and writes tests/golden/faceid.npz.

Cases (faceid_ref.CASES), batch 2, images 0.8 N(0, 1) regenerated from their seeds (faceid_ref.case_images), so that the clamp of the quantiser is
exercised (between 5 % and 50 % of the pixels, asserted):  up64 (64^2, the resize upscales)  and  down256 (256^2).  Per case:

    <case>.loss       loss_id, float64
    <case>.g_x1       d loss / d x1 in float64 — up64 only: at 256^2 it would be 3 MB, over the limit of a committed file.  down256 keeps
    <case>.g_r        d loss / d r (the face network's input [2, 3, 160, 160]) of the float64 model as float32 instead; the tests push it through
                      the float64 adjoint of the resize (faceid_ref.resize_lin_bwd), a linear map pinned on its own (the maker asserts that it
                      gives autograd's d loss / d x1 to 1e-12), and
    <case>.g_x1_probe 4096 seeded entries of the float64 d loss / d x1 (both cases) hold that composition to the stored gradient
    <case>.g_dev32    max |g32 - g64| / max |g64| of d loss / d x1, g32 = the same model run in float32 torch: the yardstick of the GPU test
    <case>.loss_dev32, <case>.emb_dev32   |loss32 - loss64| (the yardstick of the loss) and max |e32 - e64| over both halves' embeddings
    <case>.clamped    the share of pixels of x1 the quantiser clamps

    python tests/golden/make_faceid.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

PROBE = 4096


def probe_index(n, seed):
    return np.sort(np.random.RandomState(seed + 1000).choice(n, PROBE, replace=False))


def evaluate(state, res, seed, dtype):
    from tests import faceid_ref as M
    P = M.face_params(state, dtype)
    x0, x1 = M.case_images(res, seed)
    return (x0, x1) + M.id_loss(lambda r: M.embed_t(P, r), x0, x1, dtype)


def main():
    from latent2im_amd import constants, face_specs
    from tests import faceid_ref as M
    torch.manual_seed(0)
    state = face_specs.facenet_state(seed=constants.SYNTH_SEED_F)
    out = {}
    for name, res, seed in M.CASES:
        x0, x1, loss, gx, gr, e0, e1 = evaluate(state, res, seed, torch.float64)
        _, _, loss32, gx32, _, e032, e132 = evaluate(state, res, seed, torch.float32)
        lv = M.level(x1)
        clamped = float(((lv <= 0) | (lv >= 255)).mean())
        assert 0.05 < clamped < 0.5, clamped
        # float32 forms the level with two roundings (<= 2 * 2^-24 * 255 = 3.1e-5): no pixel may sit that close to a clamp edge, or its mask would depend on them
        assert min(np.abs(lv).min(), np.abs(lv - 255.0).min()) > 4e-5, 'a pixel sits on the clamp edge'
        back, _ = M.resize_lin_bwd(gr, x1)
        assert np.abs(back - gx).max() <= 1e-12 * np.abs(gx).max(), 'autograd and the adjoint model disagree'
        out[name + '.loss'] = np.float64(loss)
        if res <= 64:
            out[name + '.g_x1'] = gx
        else:
            out[name + '.g_r'] = gr.astype(np.float32)
        out[name + '.g_x1_probe'] = gx.reshape(-1)[probe_index(gx.size, seed)]
        out[name + '.g_dev32'] = np.float64(np.abs(gx32 - gx).max() / np.abs(gx).max())
        out[name + '.loss_dev32'] = np.float64(abs(loss32 - loss))
        out[name + '.emb_dev32'] = np.float64(max(np.abs(e032 - e0).max(), np.abs(e132 - e1).max()))
        out[name + '.clamped'] = np.float64(clamped)
        print('%s: loss %.6f, max |g_x1| %.3e, g_dev32 %.3e, loss_dev32 %.3e, emb_dev32 %.3e, clamped %.3f'
              % (name, loss, np.abs(gx).max(), out[name + '.g_dev32'], out[name + '.loss_dev32'], out[name + '.emb_dev32'], clamped))
    path = os.path.join(HERE, 'faceid.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
