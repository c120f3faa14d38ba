"""Gradient-map magnitudes of the PGGAN-256 generator inside the config-1 walk step, the input of nets16.pggan_scale_for's G exponent.

The magnitudes are a property of the function, not of the device: they are measured on the CPU oracle (oracle/pggan.py, float32) with autograd
hooks on every map the 16-bit generator stores a gradient for — the two pre-norm maps of a block (hooks on the outputs of oracle.pggan._equal_conv),
the normalised map between its convs and the upsampled block input (hooks on the inputs of the same function).  Two kinds of run:

    step   the config-1 step (pggan.walk_training_step's sequence on the oracle: half-resolution logits, regressor column, clamp-pair alphas, z
           walk, broadcasting BCE + 0.05 content) on the synthetic weights `--synthetic_weights` trains on, one attribute, alpha_delta 0.3
    probe  sum(img * probe) with a standard-normal probe at a (step, alpha) of the generator alone: tests/test_pggan16_gpu.py's loss

Per run it prints every hooked map (max and median |g| as log2), the largest map and the exponent that puts it at 2^5, and the smallest map's
median after that scaling (it has to stay a normal fp16 number, >= 2^-14).

    python tools/probe_pggan16.py [--steps 256x1,256x4,256x8,256x2] [--probes 2:0.0,2:0.4,2:-1,0:0.0,1:1.0] [--out profiles/pggan16_gradient_ranges.txt]

``--gpu`` confirms the step figures on the device: the same step (same synthetic weights, z and walk draw) through pggan.faceGraph under
conv.PRECISION 'f16' with nets16.PROBE collecting the generator's h8 gradient maps as they are stored, under the exponents of
nets16.pggan_scale_for.  It prints every map unscaled beside the CPU rows' format, the largest map as stored (the rule puts it near 2^5) and the
smallest median as stored (>= 2^-14), and appends to ``--out`` instead of replacing it.

    python tools/probe_pggan16.py --gpu --steps 256x1,256x4,256x8 --out profiles/pggan16_gradient_ranges.txt
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lg(v):
    return math.log2(v) if v > 0 else float('-inf')


class Hooks:
    """Wraps oracle.pggan._equal_conv while active: records (tag, shape, max |g|, median |g| of the non-zero entries) per hooked map."""

    def __init__(self):
        self.rows = []

    def _hook(self, tag, t):
        if t.requires_grad:
            def fn(g):
                a = g.detach().abs().reshape(-1)
                nz = a[a > 0]
                self.rows.append((tag, tuple(g.shape), float(a.max()), float(nz.median()) if nz.numel() else 0.0))
            t.register_hook(fn)

    def __enter__(self):
        from oracle import pggan as opg
        self.opg, self.orig = opg, opg._equal_conv

        def wrapped(P, name, x, padding):
            if x.dim() == 4 and x.shape[2] > 1:                  # (the 4x4 stage reads the fp32 code: no stored gradient map)
                self._hook('in  %s' % name, x)
            y = self.orig(P, name, x, padding)
            self._hook('out %s' % name, y)
            return y
        opg._equal_conv = wrapped
        return self

    def __exit__(self, *exc):
        self.opg._equal_conv = self.orig


def report(title, rows, lines):
    lines.append(title)
    for tag, shape, mx, med in rows:
        lines.append('  %-34s %-18s max 2^%6.1f  median 2^%6.1f' % (tag, 'x'.join(map(str, shape)), lg(mx), lg(med)))
    top = max(r[2] for r in rows)
    exp = 5 - int(round(lg(top)))
    low = min(r[3] for r in rows if r[3] > 0)
    lines.append('  largest gradient map 2^%.1f -> exponent %d; smallest median 2^%.1f, scaled 2^%.1f (fp16 normals end at 2^-14)' % (lg(top), exp, lg(low), lg(low) + exp))
    print('\n'.join(lines[-(len(rows) + 2):]), flush=True)
    return exp


def probe_step(resolution, batch, lines):
    from latent2im_amd import constants, synth
    from oracle import nets as onets
    from oracle import pggan as opg
    from oracle import step as ostep
    step = int(round(math.log2(resolution))) - 2
    dt = torch.float32
    P = ostep.to_torch(synth.pggan_generator_state(seed=constants.SYNTH_SEED_G), dt)
    PR = ostep.to_torch(synth.resnet50_state(seed=constants.SYNTH_SEED_R), dt)
    PV = ostep.to_torch(synth.vgg19_prefix_state(seed=constants.SYNTH_SEED_V), dt)
    walk = torch.tensor(np.random.RandomState(0).normal(0.0, 0.02, [1, 512]), dtype=dt).requires_grad_(True)
    z = torch.from_numpy(synth.z_sample(batch, seed=0)).to(dt)
    half = lambda img: torch.nn.functional.avg_pool2d(img, 2)
    with torch.no_grad():
        x0 = half(opg.generator_forward(P, z[:, :511], step=step, alpha=0.0))
        target, eps = ostep.get_alphas_clamp(onets.resnet50_forward(PR, x0)[:, [31]], torch.full((batch, 1), 0.3, dtype=dt))
    with Hooks() as h:
        x1 = half(opg.generator_forward(P, opg.walk_linear_z_free(z, eps, walk)[:, :511], step=step, alpha=0.0))
        reg = opg.reg_loss_quirk(onets.resnet50_forward(PR, x1)[:, [31]], target)
        cont, _ = ostep.content_loss(PV, x0, x1)
        opg.total_loss(reg, cont, None, no_content_loss=False, no_gan_loss=True).backward()
    return report('## step: %d^2, batch %d (reg %.4g, content %.4g, max |dL/dwalk| 2^%.1f)' % (resolution, batch, float(reg), float(cont), lg(float(walk.grad.abs().max()))),
                  h.rows, lines)


def probe_probe(step, alpha, lines, batch=2):
    from latent2im_amd import synth
    from oracle import pggan as opg
    from oracle import step as ostep
    dt = torch.float32
    P = ostep.to_torch(synth.pggan_generator_state(seed=11), dt)
    z = torch.from_numpy(synth.z_sample(batch, seed=3)[:, :511]).to(dt).requires_grad_(True)
    with Hooks() as h:
        img = opg.generator_forward(P, z, step=step, alpha=alpha)
        (img * torch.randn(img.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(dt)).sum().backward()
    return report('## probe: step %d (%d^2), alpha %g, batch %d' % (step, 4 * 2 ** step, alpha, batch), h.rows, lines)


def probe_step_gpu(resolution, batch, lines):
    """The step of probe_step on the device at fp16, nets16.PROBE on: the stored (scaled) maps of the generator's backward."""
    from latent2im_amd import constants, conv, nets16, synth
    from latent2im_amd import pggan as pg
    assert resolution == constants.PG_RESOLUTION, 'the graph runs the in-repo generator at %d^2 only' % constants.PG_RESOLUTION
    conv.PRECISION, constants.ALLOW_SYNTHETIC_WEIGHTS, constants.BATCH_SIZE = 'f16', True, batch
    np.random.seed(0)                                           # the walk draw of probe_step: N(0, 0.02) from RandomState(0)
    graph = pg.faceGraph(lr=1e-3, walk_type='linear', loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': 31}, layers=None, pgan_opts=None)
    exp = graph.loss_scaler.log2['G']
    nets16.PROBE = []
    try:
        loss, *_ = pg.walk_training_step(graph, synth.z_sample(batch, seed=0), np.full((batch, 1), 0.3), no_content_loss=False)
        torch.cuda.synchronize()
        rows = [r for r in nets16.PROBE if r[0].startswith('PG.g_')]
    finally:
        nets16.PROBE = None
    st = graph.loss_scaler.stats()
    lines.append('## GPU step (fp16, nets16.PROBE): %d^2, batch %d, exponents %s (reg %.4g, content %.4g, max |dL/dwalk| 2^%.1f, scaler %s)'
                 % (resolution, batch, graph.loss_scaler.log2, float(graph.last_terms['reg']), float(graph.last_terms['cont']),
                    lg(float(graph.walk.w.grad.abs().max())), st))
    k = 2.0 ** -exp * (1.0 / st['scale'])                      # stored = true * 2^G * dynamic (the dynamic factor is 1 on a first step)
    for tag, shape, mx, med, zeros in rows:
        lines.append('  %-34s %-18s max 2^%6.1f  median 2^%6.1f   as stored: max 2^%5.1f  median 2^%5.1f  zeros %.3f'
                     % (tag, 'x'.join(map(str, shape)), lg(mx * k), lg(med * k), lg(mx), lg(med), zeros))
    top = max(r[2] for r in rows)
    low = min(r[3] for r in rows if r[3] > 0)
    lines.append('  largest gradient map 2^%.1f, as stored 2^%.1f (G exponent %d; the data alone would give %d); smallest median 2^%.1f, as stored 2^%.1f '
                 '(fp16 normals end at 2^-14)' % (lg(top * k), lg(top), exp, 5 - int(round(lg(top * k))), lg(low * k), lg(low)))
    print('\n'.join(lines[-(len(rows) + 2):]), flush=True)
    assert st['skipped'] == 0, st
    del graph
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpu', action='store_true', help='confirm the step figures on the device (fp16, nets16.PROBE); appends to --out')
    ap.add_argument('--steps', default='256x1,256x4,256x8,256x2')
    ap.add_argument('--probes', default='2:0.0,2:0.4,2:-1,0:0.0,1:1.0')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    if a.gpu:
        lines = ['# the same steps on the MI355X at fp16: the h8 gradient maps of nets16._PG16Fn.backward as stored (tools/probe_pggan16.py --gpu)']
        for s in [s for s in a.steps.split(',') if s]:
            r, b = s.split('x')
            probe_step_gpu(int(r), int(b), lines)
        if a.out:
            with open(a.out, 'a') as f:
                f.write('\n'.join(lines) + '\n')
        return
    lines = ['# PGGAN-256 generator, gradient maps of the config-1 step and of the generator test\'s probe loss on the float32 CPU oracle (autograd hooks);',
             '# tools/probe_pggan16.py.  exponent = 5 - round(log2 of the largest map): nets16.pggan_scale_for (G) and tests/test_pggan16_gpu.py']
    for s in [s for s in a.steps.split(',') if s]:
        r, b = s.split('x')
        probe_step(int(r), int(b), lines)
    for s in [s for s in a.probes.split(',') if s]:
        st, al = s.split(':')
        probe_probe(int(st), float(al), lines)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
