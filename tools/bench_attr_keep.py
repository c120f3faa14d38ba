"""Measurements of the attribute-preservation loss of walk training (--attr_keep) on the MI355X -> profiles/attr_keep_bench.txt.

    python tools/bench_attr_keep.py [--out profiles/attr_keep_bench.txt] [--parent DIR] [--rounds 3] [--steps 10] [--warmup 3]

Every step figure is one CHILD process (a fresh graph, synthetic weights, batch 8, full loss) under its own time limit: ``--warmup`` steps, then
``--steps`` steps between two device synchronisations.  Children of the configurations that are compared run ALTERNATING, ``--rounds`` times each;
a gap counts as a difference only where it is larger than both sides' run-to-run spread, and both spreads are printed.

  no regression   the W = 0 step of this tree against the step of ``--parent`` (a checkout of the parent commit with its library built; without
                  the option this row is not measured and says so), 256^2, fp32 and bf16
  cost            the W = 0.5 step against the W = 0 step at 256^2 (fp32)
  launch          l2i_reg_bce_keep_f32 alone at B = 8, F = 2048, K = 1, M = 39 in microseconds (device events over back-to-back launches), beside
                  l2i_reg_bce_f32 at the same B, F, K
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 300


def _child_step(a):
    sys.path.insert(0, a.root or ROOT)
    import numpy as np
    import torch
    from latent2im_amd import conv, selfcheck, synth
    conv.PRECISION = a.precision
    kw = dict(attr_keep=a.keep) if a.keep else {}
    g = selfcheck.build_graph(a.res, ['Smiling'], a.batch, **kw)
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
    keep = g.last_terms.get('keep')
    print(json.dumps(dict(ms=ms, keep=None if keep is None else float(keep))))


def _child_launch(a):
    sys.path.insert(0, ROOT)
    import torch
    from latent2im_amd import _lib
    B, F, A, K, M = 8, 2048, 40, 1, 39
    gen = torch.Generator().manual_seed(0)
    dev = 'cuda'
    feat1, feat0 = (torch.randn(B, F, generator=gen).to(dev) * 0.01 for _ in range(2))
    fc_w, fc_b = (torch.randn(A, F, generator=gen) / F ** 0.5).to(dev), torch.full((A,), 0.5).to(dev)
    cols, keep = torch.tensor([31]).to(dev), torch.tensor([i for i in range(A) if i != 31]).to(dev)
    target = torch.rand(B, K, generator=gen).double().to(dev)
    loss, preds, pkeep, g = (torch.empty(3, dtype=torch.float64, device=dev), torch.empty(B, K, device=dev), torch.empty(B, M, 2, device=dev),
                             torch.empty(B, F, device=dev))
    P = _lib.ptr

    def keep_launch():
        _lib.call('l2i_reg_bce_keep_f32', P(loss), P(preds), P(pkeep), P(g), P(feat1), P(feat0), P(fc_w), P(fc_b), P(cols), P(target), 1, P(keep), B, F, K, M,
                  10.0, 0.5, 1e-12)

    def bce_launch():
        _lib.call('l2i_reg_bce_f32', P(loss), P(preds), P(g), P(feat1), P(fc_w), P(fc_b), P(cols), P(target), 1, B, F, K, 1e-12)

    def timed(fn, n=200):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n
    out = dict(keep_us=[timed(keep_launch) for _ in range(3)], bce_us=[timed(bce_launch) for _ in range(3)])
    print(json.dumps(out))


def _run(argv):
    """One child under its own time limit; a child that fails or runs out of time ends the whole measurement."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT_S)
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
    p.add_argument('--keep', type=float, default=0.0)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--parent', default=None)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attr_keep_bench.txt'))
    a = p.parse_args()
    if a.child == 'step':
        return _child_step(a)
    if a.child == 'launch':
        return _child_launch(a)
    lines = ['# tools/bench_attr_keep.py: the attribute-preservation loss of walk training on the MI355X; batch 8, synthetic weights, full loss (reg + content + GAN)',
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
    r = _alternate({'W=0': ['--res', '256'], 'W=0.5': ['--res', '256', '--keep', '0.5']}, a.rounds, a)
    lines.append('cost, 256^2 f32:')
    lines += ['    %-10s %s' % (k, _fmt(v)) for k, v in r.items()]
    lines.append('    keep term of the W=0.5 runs (synthetic weights): %s' % ' '.join('%.6g' % x['keep'] for x in r['W=0.5']))
    k = _run(['--child', 'launch'])
    lines.append('launch alone, B = 8, F = 2048, K = 1, M = 39 (200 back-to-back launches between device events, three repeats): l2i_reg_bce_keep_f32 %s us; '
                 'l2i_reg_bce_f32 (B = 8, F = 2048, K = 1) %s us' % (' '.join('%.1f' % x for x in k['keep_us']), ' '.join('%.1f' % x for x in k['bce_us'])))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
