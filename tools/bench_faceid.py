"""Measurements of the identity-preservation loss of walk training (--id_loss) on the MI355X -> profiles/faceid_bench.txt.

    python tools/bench_faceid.py [--out profiles/faceid_bench.txt] [--parent DIR] [--rounds 3] [--steps 10] [--warmup 3] [--skip step1024]

Every step figure is one CHILD process (a fresh graph, synthetic weights, batch 8, full loss): ``--warmup`` steps, then ``--steps`` steps between
two device synchronisations.  Children of the configurations that are compared run ALTERNATING, ``--rounds`` times each; a gap counts as a
difference only where it is larger than both sides' run-to-run spread.

  no regression   the W = 0 step of this tree against the step of ``--parent`` (a checkout of the parent commit with its library built; without
                  the option this row is not measured and says so), 256^2, fp32 and bf16
  cost            the W = 0.5 step against the W = 0 step at 256^2 and 1024^2 (fp32), with the branch's share of the step
  kernels         l2i_face_resize_lin_f32 / _bwd_f32 in GB/s of the bytes they must move (forward: x + r; adjoint: gy + x for the clamp mask + gx; fp32), beside torch's
                  F.interpolate(mode='bicubic', antialias=True) forward and backward on the device
  eval gap        mean |loss_id's distance - pair_distances' byte-exact distance| on the same images (reported, not asserted)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child_step(a):
    sys.path.insert(0, a.root or ROOT)
    import numpy as np
    import torch
    from latent2im_amd import conv, selfcheck, synth
    conv.PRECISION = a.precision
    g = selfcheck.build_graph(a.res, ['Smiling'], a.batch)
    if a.id:
        g.id_weight = a.id
    zs, alpha = synth.z_sample(a.batch, seed=0), np.ones((a.batch, 1)) * 0.19

    def steps(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            selfcheck.run_step(g, zs, alpha)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n
    steps(a.warmup)
    ms = 1e3 * steps(a.steps)
    branch = None
    if a.id:                                            # the branch alone on the step's own images: forward + backward of the term
        from latent2im_amd import capture
        feed, _ = capture.forward(g, torch.Tensor(zs).to(g.device), torch.tensor(alpha).float().to(g.device))
        x0, x1 = feed['org'].detach(), feed['logit'].detach().requires_grad_(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(a.warmup + a.steps):
            if i == a.warmup:
                e0.record()
            g.get_id_loss(x0, x1).backward()
        e1.record()
        torch.cuda.synchronize()
        branch = e0.elapsed_time(e1) / a.steps
    print(json.dumps(dict(ms=ms, branch_ms=branch)))


def _child_kernels(a):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from latent2im_amd import facenet
    out = {}

    def timed(fn, n=50):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    for res in (256, 1024):
        x = (0.8 * torch.randn(8, 3, res, res, device='cuda')).requires_grad_(True)
        gy = torch.randn(8, 3, 160, 160, device='cuda')
        gb = (x.numel() + gy.numel()) * 4 / 1e9                   # forward: reads x, writes r
        gb_bwd = (2 * x.numel() + gy.numel()) * 4 / 1e9           # adjoint: reads gy and x (the clamp mask), writes gx
        y = F.interpolate(x, size=(160, 160), mode='bicubic', antialias=True)
        out[res] = dict(gbytes=gb, gbytes_bwd=gb_bwd,
                        lin_fwd_ms=timed(lambda: facenet.face_input_lin(x.detach())), lin_bwd_ms=timed(lambda: facenet.face_input_lin_bwd(gy, x.detach())),
                        torch_fwd_ms=timed(lambda: F.interpolate(x.detach(), size=(160, 160), mode='bicubic', antialias=True)),
                        torch_bwd_ms=timed(lambda: torch.autograd.grad(y, x, gy, retain_graph=True)))
    # the eval / training gap on synthetic weights: smooth random images and a perturbed copy
    from latent2im_amd import constants, face_specs
    net = facenet.InceptionResnetV1(face_specs.facenet_state(seed=constants.SYNTH_SEED_F), device='cuda')
    base = F.interpolate(torch.randn(8, 3, 8, 8, device='cuda'), size=(256, 256), mode='bicubic', align_corners=False)
    x0 = (0.5 * base + 0.05 * torch.randn_like(base)).clamp(-1.2, 1.2)
    x1 = (x0 + 0.1 * F.interpolate(torch.randn(8, 3, 16, 16, device='cuda'), size=(256, 256), mode='bicubic', align_corners=False)).clamp(-1.2, 1.2)
    lin = net.id_distances(x1, x0).double()
    byte = net.pair_distances(x1, x0)[0]
    out['gap'] = dict(mean_abs_gap=float((lin - byte).abs().mean()), mean_distance=float(byte.mean()))
    print(json.dumps(out))


def _run(argv):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError('child %s failed (%d)' % (argv, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def _alternate(configs, rounds, a):
    """configs: name -> child argv; every config once a round, in turn -> name -> list of results."""
    res = {k: [] for k in configs}
    for _ in range(rounds):
        for k, argv in configs.items():
            res[k].append(_run(['--child', 'step', '--steps', str(a.steps), '--warmup', str(a.warmup)] + argv))
            print('[%s] %s: %.2f ms/step' % (' '.join(argv), k, res[k][-1]['ms']), file=sys.stderr, flush=True)
    return res


def _fmt(rs):
    ms = [r['ms'] for r in rs]
    return 'ms/step %s  (median %.2f, spread %.2f)' % (' '.join('%.2f' % m for m in ms), sorted(ms)[len(ms) // 2], max(ms) - min(ms))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--child', default=None)
    p.add_argument('--root', default=None)
    p.add_argument('--precision', default='f32')
    p.add_argument('--res', type=int, default=256)
    p.add_argument('--batch', type=int, default=8)
    p.add_argument('--id', type=float, default=0.0)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--parent', default=None)
    p.add_argument('--skip', default='')
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'faceid_bench.txt'))
    a = p.parse_args()
    if a.child == 'step':
        return _child_step(a)
    if a.child == 'kernels':
        return _child_kernels(a)
    lines = ['# tools/bench_faceid.py: the identity loss of walk training on the MI355X; batch 8, synthetic weights, full loss (reg + content + GAN)',
             '# each figure: one child process, %d warm-up + %d timed steps between device synchronisations; configurations alternate, %d rounds' % (a.warmup, a.steps, a.rounds)]
    for prec in ('f32', 'bf16'):
        cfg = {'this W=0': ['--precision', prec, '--res', '256']}
        if a.parent:
            cfg['parent'] = ['--precision', prec, '--res', '256', '--root', os.path.abspath(a.parent)]
        r = _alternate(cfg, a.rounds, a)
        lines.append('no regression, 256^2 %s:' % prec)
        lines += ['    %-10s %s' % (k, _fmt(v)) for k, v in r.items()]
        if not a.parent:
            lines.append('    parent     not measured (no --parent checkout given)')
    for res in (256, 1024):
        if 'step%d' % res in a.skip:
            lines.append('cost, %d^2 f32: not measured (skipped)' % res)
            continue
        r = _alternate({'W=0': ['--res', str(res)], 'W=0.5': ['--res', str(res), '--id', '0.5']}, a.rounds, a)
        lines.append('cost, %d^2 f32:' % res)
        lines += ['    %-10s %s' % (k, _fmt(v)) for k, v in r.items()]
        br = [x['branch_ms'] for x in r['W=0.5']]
        step = sorted(x['ms'] for x in r['W=0.5'])[len(br) // 2]
        lines.append('    branch alone (forward + backward of the term, device events): %s ms = %.1f %% of the W=0.5 step'
                     % (' '.join('%.2f' % b for b in br), 100.0 * sorted(br)[len(br) // 2] / step))
    k = _run(['--child', 'kernels'])
    for res in ('256', '1024'):
        v = k[res]
        lines.append('kernels, batch 8 x 3 x %s^2 -> 160^2 (%.4f GB moved at least): resize_lin %.3f ms = %.0f GB/s, its adjoint (%.4f GB) %.3f ms = %.0f GB/s; '
                     'F.interpolate(bicubic, antialias) forward %.3f ms, backward %.3f ms'
                     % (res, v['gbytes'], v['lin_fwd_ms'], v['gbytes'] / v['lin_fwd_ms'] * 1e3, v['gbytes_bwd'], v['lin_bwd_ms'], v['gbytes_bwd'] / v['lin_bwd_ms'] * 1e3,
                        v['torch_fwd_ms'], v['torch_bwd_ms']))
    lines.append('eval / training gap (256^2, 8 pairs, synthetic weights): mean |loss_id distance - pair_distances| = %.3e at a mean distance of %.4f (reported, not asserted)'
                 % (k['gap']['mean_abs_gap'], k['gap']['mean_distance']))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
