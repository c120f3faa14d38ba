"""Timing of BASELINE config 1 (the PGGAN-256 z-walk step) per precision on one GPU, in tools/bench_invert.py's protocol: HIP events, 5 warm-up
calls, median of 20, three alternating runs a side.

(a) l2i_pixelnorm_act_h8 / l2i_pixelnorm_act_bwd_h8 at the generator's own shapes (step 6, alpha 0: blocks 0 .. 5, C x H = 512 x 4, 512 x 8,
    512 x 16, 512 x 32, 256 x 64, 128 x 128), batch 4 and 8, the four variants the generator launches (forward 1x and with the fused 2x upsample,
    backward 1x and with the fused 2x2 window sum), on inputs rotated through more than the last-level cache holds; GB/s of the least traffic
    (every operand once, two bytes an element) against 6.3 TB/s achievable.
(b) pggan.walk_training_step at 256^2, batch 4 and 8, f32 (the fp32 classes) / f16 / bf16, with and without the content term, synthetic
    weights: ms per step with all runs, the ratio to f32 and whether it lies inside the two sides' spread, the library calls of one step, and the
    three parts a step is made of timed alone (generator forward, regressor forward, one generator forward + backward) to say what holds a leg.
(c) --walk: pggan.WalkMlpZ3 (dim_z 512) forward + backward at batch 4 and 8 on the l2i_linear_rows kernels against the plain-torch composite on the
    same device and the same weights (the module's own nn.Sequential on rocBLAS plus autograd), with the library calls / torch ops of each side;
    then the config-1 step with the default walk ('NNz': WalkMlpZ3) against 'linear', per precision.  A side counts as faster only when the gap
    exceeds both spreads.

(d) --hip_graph: the config-1 step launched eagerly (pggan.walk_training_step) against replayed (capture.CapturedZStep, static inputs already on
    the device, as the eager side's are), MLP and linear walk, f32 / f16 / bf16, batch 4 and 8, the two sides sharing the frozen networks.
    --parent DIR: a checkout of the parent commit with its own library built; the eager step of parent and branch is then compared on one
    protocol and one code path: each checkout's own --walk leg in child processes, parent and branch alternating, two children a side (same lease;
    every child contributes three runs to its side's spread).
(e) --adam: GuardedAdam's step alone on the MLP walk's six tensors (2.1 M parameters): l2i_nonfinite_flag_multi_f32 + l2i_adam_guarded_multi_f32
    against the per-tensor path (six l2i_nonfinite_flag_f32 + six l2i_adam_guarded_f32 launches), us and GB/s of the least traffic (the gradient
    twice, parameter and moments read and written: 32 bytes an element).

    python tools/bench_pggan.py [--out profiles/pggan16_bench.txt] [--skip_step] [--skip_kernels]
    python tools/bench_pggan.py --walk --skip_step --skip_kernels --out profiles/walk_mlp_bench.txt
    python tools/bench_pggan.py --hip_graph --parent ../parent --skip_step --skip_kernels --out profiles/pggan_graph_bench.txt
    python tools/bench_pggan.py --adam --skip_step --skip_kernels --out profiles/adam_multi_bench.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
MAPS = ((512, 4), (512, 8), (512, 16), (512, 32), (256, 64), (128, 128))
PRECS = ('f32', 'f16', 'bf16')


def timed(fn, warmup=5, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def count_calls(fn):
    """Library entry-point calls (latent2im_amd._lib.call and the conv launches) made by one run of ``fn``."""
    from latent2im_amd import _lib, conv
    n = [0]
    real_call, real_launch = _lib.call, conv._launch

    def call(*a, **k):
        n[0] += 1
        return real_call(*a, **k)

    def launch(*a, **k):
        n[0] += 1
        return real_launch(*a, **k)
    _lib.call, conv._launch = call, launch
    try:
        fn()
    finally:
        _lib.call, conv._launch = real_call, real_launch
    return n[0]


def kernel_rows(b, ch, hw, prec, lines):
    """The four launches of one map shape; cold inputs (each operand rotates through > 512 MiB, twice the last-level cache)."""
    from latent2im_amd import kernels16 as K16
    dtype = torch.float16 if prec == 'f16' else torch.bfloat16
    n = b * ch * hw * hw

    def rot(shape_n, make):
        copies = max(3, min(256, -(-(512 << 20) // (shape_n * 2))))
        return [make() for _ in range(copies)]
    x = rot(n, lambda: torch.randn(b, ch // 8, hw, hw, 8, device='cuda').to(dtype))
    g1 = rot(n, lambda: torch.randn(b, ch // 8, hw, hw, 8, device='cuda').to(dtype))
    g2 = rot(4 * n, lambda: torch.randn(b, ch // 8, 2 * hw, 2 * hw, 8, device='cuda').to(dtype))
    turn = [0]

    def nxt(pool):
        turn[0] += 1
        return pool[turn[0] % len(pool)]
    cases = (('fwd up 1', 2 * n, lambda: K16.pixelnorm_act(nxt(x), 0.2)),
             ('fwd up 2', 5 * n, lambda: K16.pixelnorm_act(nxt(x), 0.2, up=2)),
             ('bwd pool 1', 3 * n, lambda: K16.pixelnorm_act_bwd(nxt(g1), nxt(x), 0.2)),
             ('bwd pool 2', 6 * n, lambda: K16.pixelnorm_act_bwd(nxt(g2), nxt(x), 0.2, pool=2)))
    for name, elems, fn in cases:
        runs = [timed(fn) for _ in range(3)]
        m = statistics.median(runs)
        lines.append('%-4s B %d  C %3d  %3d^2  %-10s %8.1f us (runs %s)  %6.0f GB/s = %4.1f %% of 6.3 TB/s'
                     % (prec, b, ch, hw, name, m * 1e6, ' '.join('%.1f' % (v * 1e6) for v in runs), 2.0 * elems / m / 1e9, 100 * 2.0 * elems / m / HBM))
        print(lines[-1], flush=True)


def _graph(prec, batch, walk_type='linear'):
    from latent2im_amd import constants, conv
    from latent2im_amd import pggan as pg
    conv.PRECISION, constants.ALLOW_SYNTHETIC_WEIGHTS, constants.BATCH_SIZE = prec, True, batch
    np.random.seed(0)
    return pg.faceGraph(lr=1e-3, walk_type=walk_type, loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': 31}, layers=None, pgan_opts=None)


def step_rows(batch, lines):
    from latent2im_amd import conv, synth
    from latent2im_amd import pggan as pg
    graphs = {p: _graph(p, batch) for p in PRECS}
    z = torch.Tensor(synth.z_sample(batch, seed=0)).cuda()
    ad = torch.full((batch, 1), 0.3, device='cuda')

    def side(p, fn):
        def run():
            conv.PRECISION = p
            return fn(graphs[p])
        return run
    for content in (True, False):
        step = lambda g: pg.walk_training_step(g, z, ad, no_content_loss=not content)
        runs = {p: [] for p in PRECS}
        for _ in range(3):                                                   # alternating runs: the spread of each side is its run-to-run noise
            for p in PRECS:
                runs[p].append(timed(side(p, step)))
        med = {p: statistics.median(v) for p, v in runs.items()}
        calls = {p: count_calls(side(p, step)) for p in PRECS}
        for p in PRECS:
            row = '%-4s step 256^2  batch %d  %-15s %8.2f ms (runs %s)   %d library calls' % (
                p, batch, 'content on' if content else 'content off', 1e3 * med[p], ' '.join('%.2f' % (1e3 * v) for v in runs[p]), calls[p])
            if p != 'f32':
                ratio = med['f32'] / med[p]
                lo = min(runs['f32']) / max(runs['f32']) * min(runs[p]) / max(runs[p])
                hi = max(runs['f32']) / min(runs['f32']) * max(runs[p]) / min(runs[p])
                row += '   f32 / %s %.3f%s' % (p, ratio, "  INSIDE the two sides' spread" if lo <= ratio <= hi else '')
                sc = graphs[p].loss_scaler
                row += '' if sc is None else '   scaler %s' % sc.stats()
            lines.append(row)
            print(row, flush=True)
    # the parts of a step alone: what holds a leg that is not faster
    zg = z.clone().requires_grad_(True)

    def gen_both(g):
        zg.grad = None
        g.get_logits({'z': zg}).sum().backward()
    with torch.no_grad():
        x0 = {p: side(p, lambda g: g.get_logits({'z': z}))() for p in PRECS}
    parts = (('generator forward (no grad)', lambda g: _nograd(lambda: g.get_logits({'z': z}))),
             ('generator forward + backward', gen_both),
             ('regressor forward (no grad)', None))
    for name, fn in parts:
        for p in PRECS:
            f = side(p, fn) if fn is not None else side(p, lambda g, p=p: _nograd(lambda: g.get_reg_preds(x0[p])))
            runs_p = [timed(f) for _ in range(3)]
            lines.append('%-4s part 256^2  batch %d  %-30s %8.2f ms (runs %s)   %d library calls'
                         % (p, batch, name, 1e3 * statistics.median(runs_p), ' '.join('%.2f' % (1e3 * v) for v in runs_p), count_calls(f)))
            print(lines[-1], flush=True)
    conv.PRECISION = 'f32'


def _verdict(a, b):
    """'a faster' / 'b faster' only when the two sides' runs do not overlap, else 'inside the spread'."""
    if max(a) < min(b):
        return 'first faster (gap exceeds both spreads)'
    if max(b) < min(a):
        return 'second faster (gap exceeds both spreads)'
    return "INSIDE the two sides' spread"


def walk_rows(batch, lines):
    """(c): the walk alone, kernels against the torch composite, then the step per walk type and precision."""
    from latent2im_amd import conv, synth
    from latent2im_amd import pggan as pg
    torch.manual_seed(0)
    walk = pg.WalkMlpZ3(512, 6, 1, ['Smiling']).cuda()
    z = torch.Tensor(synth.z_sample(batch, seed=0)).cuda()
    al = torch.full((batch, 1), 0.3, device='cuda')
    r = torch.randn(batch, 512, device='cuda')

    def hip():
        walk.zero_grad(set_to_none=True)
        (walk(z, al) * r).sum().backward()

    def composite():
        walk.zero_grad(set_to_none=True)
        ((z + al * walk.linear(z)) * r).sum().backward()
    runs = {'hip': [], 'torch': []}
    for _ in range(3):
        runs['hip'].append(timed(hip))
        runs['torch'].append(timed(composite))
    for name, fn in (('hip', hip), ('torch', composite)):
        lines.append('walk dim_z 512  batch %d  fwd + bwd  %-28s %8.1f us (runs %s)   %d library calls'
                     % (batch, 'l2i_linear_rows kernels' if name == 'hip' else 'nn.Sequential + autograd', 1e6 * statistics.median(runs[name]),
                        ' '.join('%.1f' % (1e6 * v) for v in runs[name]), count_calls(fn)))
        print(lines[-1], flush=True)
    lines.append('walk dim_z 512  batch %d  kernels / composite %.3f   %s' % (batch, statistics.median(runs['hip']) / statistics.median(runs['torch']),
                                                                             _verdict(runs['hip'], runs['torch'])))
    print(lines[-1], flush=True)
    ad = torch.full((batch, 1), 0.3, device='cuda')
    for p in PRECS:
        graphs = {w: _graph(p, batch, w) for w in ('NNz', 'linear')}
        step = lambda g: pg.walk_training_step(g, z, ad, no_content_loss=False)
        sruns = {w: [] for w in graphs}
        for _ in range(3):
            for w in graphs:
                conv.PRECISION = p
                sruns[w].append(timed(lambda: step(graphs[w])))
        for w in graphs:
            lines.append('%-4s step 256^2  batch %d  content on  walk %-6s %8.2f ms (runs %s)   %d library calls'
                         % (p, batch, w, 1e3 * statistics.median(sruns[w]), ' '.join('%.2f' % (1e3 * v) for v in sruns[w]), count_calls(lambda: step(graphs[w]))))
            print(lines[-1], flush=True)
        lines.append('%-4s step 256^2  batch %d  NNz / linear %.3f   %s' % (p, batch, statistics.median(sruns['NNz']) / statistics.median(sruns['linear']),
                                                                          _verdict(sruns['NNz'], sruns['linear'])))
        print(lines[-1], flush=True)
        del graphs
        torch.cuda.empty_cache()
    conv.PRECISION = 'f32'


def graph_rows(batch, lines, results):
    """(d): eager against replayed, per precision and walk type; ``results[(prec, walk, batch)]`` = the eager runs (for the parent comparison)."""
    from latent2im_amd import capture, constants, conv, synth
    from latent2im_amd import pggan as pg
    zs = synth.z_sample(batch, seed=0)
    z = torch.Tensor(zs).cuda()
    ad_np = np.full((batch, 1), 0.3)
    ad = torch.full((batch, 1), 0.3, device='cuda')
    for p in PRECS:
        conv.PRECISION, constants.ALLOW_SYNTHETIC_WEIGHTS, constants.BATCH_SIZE = p, True, batch
        nets = pg.load_networks(torch.device('cuda', torch.cuda.current_device()))
        for w in ('NNz', 'linear'):
            np.random.seed(0)
            mk = lambda: pg.faceGraph(lr=1e-3, walk_type=w, loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': 31}, layers=None,
                                      pgan_opts=None, nets=nets)
            ge, gc_ = mk(), mk()
            eager_fn = lambda: pg.walk_training_step(ge, z, ad, no_content_loss=False)
            alone = timed(eager_fn)                                          # before anything is captured in this process for these networks
            step = capture.CapturedZStep(gc_, batch, 1)
            step.load(zs, ad_np)
            sides = {'eager': eager_fn, 'replayed': lambda: step()}
            runs = {k: [] for k in sides}
            for _ in range(3):
                for k, fn in sides.items():
                    runs[k].append(timed(fn))
            results[(p, w, batch)] = runs['eager']
            for k, fn in sides.items():
                row = '%-4s step 256^2  batch %d  content on  walk %-6s %-8s %8.2f ms (runs %s)   %d library calls' % (
                    p, batch, w, k, 1e3 * statistics.median(runs[k]), ' '.join('%.2f' % (1e3 * v) for v in runs[k]), count_calls(fn))
                sc = ge.loss_scaler
                if k == 'eager':
                    row += '   (one run before the capture: %.2f ms)' % (1e3 * alone)
                lines.append(row + ('' if sc is None else '   scaler %s' % sc.stats()))
                print(lines[-1], flush=True)
            lines.append('%-4s step 256^2  batch %d  walk %-6s replayed / eager %.3f   %s' % (
                p, batch, w, statistics.median(runs['replayed']) / statistics.median(runs['eager']), _verdict(runs['replayed'], runs['eager'])))
            print(lines[-1], flush=True)
            del ge, gc_, step, sides, eager_fn
        del nets
        torch.cuda.empty_cache()
    conv.PRECISION = 'f32'


def child_walk_rows(tree, tag):
    """The --walk leg of the checkout at ``tree`` (the parent's, or this one) in a child process of its own -> {(prec, walk, batch): [runs in s]}
    from its step rows, and the rows themselves."""
    import re
    import subprocess
    import tempfile
    out = os.path.join(tempfile.mkdtemp(), 'parent_walk.txt')
    tool = os.path.join(os.path.abspath(tree), 'tools', 'bench_pggan.py')
    subprocess.run([sys.executable, tool, '--walk', '--skip_step', '--skip_kernels', '--out', out], cwd=os.path.abspath(tree), check=True,
                   stdout=subprocess.DEVNULL, timeout=600)
    runs, rows = {}, []
    for line in open(out):
        m = re.match(r'(\w+)\s+step 256\^2\s+batch (\d+)\s+content on\s+walk (\w+)\s+[\d.]+ ms \(runs ([\d. ]+)\)', line)
        if m:
            runs[(m.group(1), m.group(3), int(m.group(2)))] = [1e-3 * float(v) for v in m.group(4).split()]
            rows.append('%-16s %s' % (tag, line.rstrip()))
    return runs, rows


def adam_rows(lines):
    """(e): the guarded update alone on the MLP walk's six tensors."""
    from latent2im_amd import _lib, optim
    torch.manual_seed(0)
    shapes = [(1024, 512), (1024,), (1024, 1024), (1024,), (512, 1024), (512,)]
    ps = [torch.nn.Parameter(torch.randn(*s, device='cuda') * 0.05) for s in shapes]
    for q in ps:
        q.grad = torch.randn_like(q)
    n = sum(q.numel() for q in ps)
    sc = optim.LossScaler(dict(R=0, V=0, D=0, G=0), 'cuda')
    opt = optim.GuardedAdam(ps, lr=1e-3, betas=(0.5, 0.99), scaler=sc)
    opt.init_state()

    def per_tensor():
        state, scale = _lib.ptr(sc.state), _lib.ptr(sc.scale)
        for q in ps:
            _lib.call('l2i_nonfinite_flag_f32', _lib.fptr(q.grad), q.numel(), state)
        for i, q in enumerate(ps):
            st = opt.state[q]
            _lib.call('l2i_adam_guarded_f32', _lib.fptr(q.data), _lib.fptr(q.grad), _lib.fptr(st['exp_avg']), _lib.fptr(st['exp_avg_sq']), _lib.fptr(st['step']),
                      q.numel(), 1e-3, 0.5, 0.99, 1e-8, 0, state, scale, 2.0, 0.5, sc.growth_interval, sc.max_scale, 1 if i == len(ps) - 1 else 0)
    sides = {'multi-tensor (2 calls, 3 kernels)': opt.step, 'per tensor (12 calls, 12 kernels)': per_tensor}
    runs = {k: [] for k in sides}
    for _ in range(3):
        for k, fn in sides.items():
            runs[k].append(timed(fn))
    for k, fn in sides.items():
        m = statistics.median(runs[k])
        lines.append('guarded Adam, MLP walk (6 tensors, %d parameters)  %-34s %8.1f us (runs %s)  %6.0f GB/s  %d library calls'
                     % (n, k, 1e6 * m, ' '.join('%.1f' % (1e6 * v) for v in runs[k]), 32.0 * n / m / 1e9, count_calls(fn)))
        print(lines[-1], flush=True)
    a, b = list(runs.values())
    lines.append('guarded Adam  multi-tensor / per tensor %.3f   %s' % (statistics.median(a) / statistics.median(b), _verdict(a, b)))
    print(lines[-1], flush=True)
    lines.append('scaler after the timing: %s' % sc.stats())


def _nograd(fn):
    with torch.no_grad():
        return fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip_step', action='store_true')
    ap.add_argument('--skip_kernels', action='store_true')
    ap.add_argument('--walk', action='store_true', help='(c): the MLP walk on its kernels against the torch composite, and the step per walk type')
    ap.add_argument('--hip_graph', action='store_true', help='(d): the config-1 step eager against replayed from the captured graph')
    ap.add_argument('--parent', default=None, help='(d): a built checkout of the parent commit: its --walk leg and this checkout\'s run alternately in child processes')
    ap.add_argument('--adam', action='store_true', help="(e): the guarded Adam step alone on the MLP walk's six tensors")
    args = ap.parse_args()
    lines = ['# tools/bench_pggan.py on %s' % torch.cuda.get_device_name(0),
             '# HIP events, 5 warm-up calls, median of 20, three alternating runs a side; kernels: cold inputs (> 512 MiB rotated per operand), GB/s of '
             'the least traffic (every operand once, two bytes an element)']

    def flush():
        if args.out:                                                         # section by section: a long run leaves what it measured
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    if not args.skip_step:
        for batch in (4, 8):
            step_rows(batch, lines)
            flush()
            torch.cuda.empty_cache()
    if args.walk:
        for batch in (4, 8):
            walk_rows(batch, lines)
            flush()
    if args.hip_graph:
        results = {}
        for batch in (4, 8):
            graph_rows(batch, lines, results)
            flush()
        if args.parent:
            # branch against parent, eager, on the same protocol and code path: each side's own --walk leg in child processes, alternating
            sides = {'parent': {}, 'branch': {}}
            for rnd in (1, 2):
                for name, tree in (('parent', args.parent), ('branch', ROOT)):
                    runs, rows = child_walk_rows(tree, '%s (child %d)' % (name, rnd))
                    lines.extend(rows)
                    for key, v in runs.items():
                        sides[name].setdefault(key, []).extend(v)
                    flush()
            for key in sorted(sides['branch']):
                if key in sides['parent']:
                    b, a = sides['branch'][key], sides['parent'][key]
                    lines.append('%-4s step 256^2  batch %d  walk %-6s eager: branch %.2f ms / parent %.2f ms = %.3f   %s' % (
                        key[0], key[2], key[1], 1e3 * statistics.median(b), 1e3 * statistics.median(a), statistics.median(b) / statistics.median(a),
                        _verdict(b, a)))
                    print(lines[-1], flush=True)
        flush()
    if args.adam:
        adam_rows(lines)
        flush()
    if not args.skip_kernels:
        for prec in ('f16', 'bf16'):
            for b in (4, 8):
                for ch, hw in MAPS:
                    kernel_rows(b, ch, hw, prec, lines)
                flush()
    flush()


if __name__ == '__main__':
    main()
