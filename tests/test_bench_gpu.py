"""bench.py's timed path on the GPU: what the timed steps compute (and --dump-outputs writes) does not depend on how many steps the clock
added to the warm-up."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', ['c3', 'c5'])
def test_time_based_warm_up_steps_leave_the_timed_steps_unchanged(monkeypatch, cfg):
    """Two workloads of the same arguments (64^2, batch 4, generator noise on): one warms up with its 2 counted steps only, the other with
    2 seconds' worth of extra steps.  warm_up restores the walk, Adam, the loss scale and both RNGs after the extra steps, so the three steps
    after it return the same loss, walk gradient and images and leave the same walk (c3: eager, fp32; c5: hipGraph-replayed, fp16)."""
    from latent2im_amd import constants, conv
    b = _bench()
    for mod, name in ((conv, 'PRECISION'), (constants, 'SYNTH_NOISE_STRENGTH'), (constants, 'resolution'), (constants, 'BATCH_SIZE'),
                      (constants, 'ALLOW_SYNTHETIC_WEIGHTS')):
        monkeypatch.setattr(mod, name, getattr(mod, name))
    constants.SYNTH_NOISE_STRENGTH = b.NOISE_STRENGTH
    runs = []
    for seconds in (0.0, 2.0):
        wl = b.Workload(cfg, 'f16' if cfg == 'c5' else 'f32', 64, 4, None, 1, 5, cfg == 'c5')
        step = wl.stepper()
        n = b.warm_up(step, 2, seconds, workload=wl)
        for i in range(3):
            r = step(2 + i)
        torch.cuda.synchronize()
        runs.append(dict(n=n, loss=float(r['loss']), grad=r['grad'].detach().double().cpu().numpy(), x1=r['x1'].detach().double().cpu().numpy(),
                         walk=wl.g.walk.w.detach().double().cpu().numpy()))
        wl.release()
    short, long_ = runs
    assert short['n'] == 2 and long_['n'] > 2, (short['n'], long_['n'])
    assert abs(short['loss'] - long_['loss']) <= 1e-6 * abs(short['loss']), (short['loss'], long_['loss'])
    for k in ('grad', 'x1', 'walk'):
        np.testing.assert_allclose(long_[k], short[k], rtol=1e-5, atol=1e-6 * np.abs(short[k]).max(), err_msg=k)
