"""CPU tool (build container only): runs the reference's own WalkMlpZ3 (graphs/pggan/transform_base.py:167-188, loaded through
tests/golden/ref_shim.py) in float32 with autograd and writes tests/golden/walk_mlp.npz.

    s.*    dim_z = 64, B = 3: z, alpha, r, z_new and the gradients of sum(z_new * r) with respect to the six parameters and z, all in full
    l.*    dim_z = 512, B = 4: z, alpha, r, z_new and the bias gradients in full; of the three weight gradients the row and the column sums

Weights do not travel: make_golden.seeded_module_state's rule (tests/emu.seeded_state regenerates them) with SEEDS below.

    python tests/golden/make_walk_mlp.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CASES = {'s': dict(dim_z=64, B=3, seed=71, data_seed=72), 'l': dict(dim_z=512, B=4, seed=73, data_seed=74)}


def case_inputs(c):
    """z, alpha (mixed signs, |alpha| < 1: what get_alphas hands the walk) and the probe r of a case."""
    rs = np.random.RandomState(c['data_seed'])
    z = rs.standard_normal((c['B'], c['dim_z'])).astype(np.float32)
    alpha = rs.uniform(-1, 1, (c['B'], 1)).astype(np.float32)
    r = rs.standard_normal((c['B'], c['dim_z'])).astype(np.float32)
    return z, alpha, r


def reference_walk_class():
    from tests.golden import ref_shim
    ref_shim.install()
    pk = ref_shim._pkg('graphs.pggan', os.path.join(ref_shim.REF, 'graphs', 'pggan'))
    sys.modules['graphs.pggan.pggan_256'] = types.ModuleType('graphs.pggan.pggan_256')
    pk.pggan_256 = sys.modules['graphs.pggan.pggan_256']
    ref_shim._load('graphs.pggan.constants', os.path.join(ref_shim.REF, 'graphs', 'pggan', 'constants.py'))
    tb = ref_shim._load('graphs.pggan.transform_base', os.path.join(ref_shim.REF, 'graphs', 'pggan', 'transform_base.py'))
    return tb.WalkMlpZ3


if __name__ == '__main__':
    from tests.golden.make_golden import seeded_module_state
    Walk = reference_walk_class()
    out = {}
    for tag, c in CASES.items():
        walk = Walk(c['dim_z'], 6, 1, ['Smiling'])
        assert list(walk.state_dict()) == ['linear.%d.%s' % (i, n) for i in (0, 2, 4) for n in ('weight', 'bias')]
        seeded_module_state(walk, c['seed'])
        z, alpha, r = (torch.from_numpy(a) for a in case_inputs(c))
        z.requires_grad_(True)
        z_new = walk(z, alpha)
        (z_new * r).sum().backward()
        out.update({tag + '.z': z.detach().numpy(), tag + '.alpha': alpha.numpy(), tag + '.r': r.numpy(), tag + '.z_new': z_new.detach().numpy(),
                    tag + '.grad.z': z.grad.numpy()})
        for k, p in walk.named_parameters():
            gr = p.grad.numpy()
            if tag == 's' or gr.ndim == 1:
                out['%s.grad.%s' % (tag, k)] = gr
            else:
                out['%s.grad.%s.rowsum' % (tag, k)] = gr.astype(np.float64).sum(1)
                out['%s.grad.%s.colsum' % (tag, k)] = gr.astype(np.float64).sum(0)
    path = os.path.join(HERE, 'walk_mlp.npz')
    np.savez_compressed(path, **out)
    print('wrote %s %.1f KB' % (path, os.path.getsize(path) / 1024))
