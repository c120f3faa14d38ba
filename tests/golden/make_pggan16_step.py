"""CPU tool: evaluates the config-1 step at the graph's own size (tests/pggan16_ref.STEP: 256^2, batch 2, the strong-walk case of
tests/test_pggan_gpu.py) in exact float64 and, per 16-bit element type, on the whole-step rounding model (tests/pggan16_ref.step_forward:
generator, ResNet-50 and VGG-19 with the storage rounding of nets16 restated), and writes tests/golden/pggan16_step.npz:

    grad_w, loss_reg, loss_cont, loss_total      the exact float64 step
    <dt>.model.<quantity>.<figure>               the unperturbed model's distance to the exact step
    <dt>.allowed.<quantity>.<figure>             inversion16_ref.allowed: max(2 x the model's spread, gradq-only), relative to the MODEL
    <dt>.spread.<quantity>.<figure>              the spread itself (the condition inversion16_ref.SPREAD_CAP is checked on)
    <dt>.norm_ratio                              |model gradient| / |exact gradient|  (turns a bar relative to the model into one relative to exact)
    <dt>.loss_reg, <dt>.loss_cont                the model's loss terms
    <dt>.cont_abs_allowed                        the content term's absolute bar (below)
    fingerprint                                  crc32 of the seeds / case and of the three network states

The content term is a mean squared difference of two maps that are each rounded to the element type.  Its bar is absolute:
|model - exact| + allowed(loss_rel) |model|  +  (2 u_h)^2 mean_taps mean(a^2 + b^2): the last term is the square of one rounding step
(2 u_h relative) of each of the two maps, the size below which the difference carries no information.

    python tests/golden/make_pggan16_step.py        # about five minutes of CPU (12 model evaluations, float64)
"""
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle                                             # noqa: E402
from latent2im_amd import nets16, synth                   # noqa: E402
from tests import inversion16_ref as I16                  # noqa: E402
from tests import pggan16_ref as R                        # noqa: E402


def fingerprint():
    S = R.STEP
    crc = zlib.crc32(json.dumps(S, sort_keys=True).encode())
    for st in (synth.pggan_generator_state(seed=S['g_seed']), synth.resnet50_state(seed=S['r_seed']), synth.vgg19_prefix_state(seed=S['v_seed'])):
        for k in sorted(st):
            crc = zlib.crc32(np.ascontiguousarray(st[k]).tobytes(), zlib.crc32(k.encode(), crc))
    return crc


def scales():
    """The static exponents the fp16 step runs under: nets16.pggan_scale_for's table itself.  An L2I_F16_SCALES override is refused, not
    removed: the environment is read, never changed."""
    S = R.STEP
    assert not os.environ.get('L2I_F16_SCALES'), 'L2I_F16_SCALES overrides the table this fixture is made for: unset it'
    return nets16.pggan_scale_for(S['resolution'], S['batch'])


if __name__ == '__main__':
    torch.set_num_threads(min(32, oracle.host_cpus()))
    P, PR, PV, z, walk0 = R.step_inputs()
    out = {}
    exact = None
    for dt in R.DTYPES:
        t0 = time.time()
        m = I16.measure(lambda rd: R.step_forward(P, PR, PV, z, walk0, rd), dt, log2=scales() if dt == 'f16' else None)
        if exact is None:
            exact = R.step_forward(P, PR, PV, z, walk0, I16.Rounding(None))
            for k in ('grad_w', 'loss_reg', 'loss_cont', 'loss_total'):
                out[k] = exact[k].numpy()
        base = m['base']
        for name, fig in R.STEP_FIGURES:
            out['%s.model.%s.%s' % (dt, name, fig)] = np.float64(m['exact'][name][fig])
            out['%s.allowed.%s.%s' % (dt, name, fig)] = np.float64(I16.allowed(m, name, fig))
            out['%s.spread.%s.%s' % (dt, name, fig)] = np.float64(m['spread'][name][fig])
        out['%s.norm_ratio' % dt] = np.float64(base['grad_w'].norm() / exact['grad_w'].norm())
        out['%s.loss_reg' % dt], out['%s.loss_cont' % dt] = base['loss_reg'].numpy(), base['loss_cont'].numpy()
        cm, ce = float(base['loss_cont']), float(exact['loss_cont'])
        out['%s.cont_abs_allowed' % dt] = np.float64(abs(cm - ce) + I16.allowed(m, 'loss_cont', 'loss_rel') * abs(cm)
                                                     + (2.0 * R.UH[dt]) ** 2 * float(exact['taps_sq'].mean()))
        print('%s: %.0f s' % (dt, time.time() - t0), {k: float(v) for k, v in out.items() if k.startswith(dt) and np.ndim(v) == 0}, flush=True)
    out['fingerprint'] = np.asarray(fingerprint(), dtype=np.int64)
    path = os.path.join(ROOT, 'tests', 'golden', 'pggan16_step.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
