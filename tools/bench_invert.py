"""Timing of the inversion path (BP.py) on one GPU.  HIP events, warm-up, median of repeats.

(a) l2i_gram_loss_f32 + l2i_gram_bwd_f32 per launch at BP's four tap shapes for 256^2 (C x HW = 64 x 65536, 128 x 16384, 256 x 4096,
    512 x 1024), batch 1 and 8, beside the composite they replace — relu, torch.bmm (rocBLAS), the loss, autograd's backward — in three
    alternating runs, on inputs rotated through more than the last-level cache holds; algorithmic GB/s = (read c for the forward, read c +
    write g for the backward) / time against 6.3 TB/s achievable.  Then Vgg16Gram.loss with its image gradient at 256^2, batch 1 and 8.
(b) inversion iterations/s at 256^2, batch 1 and 8, synthetic weights, noise drawn per iteration.

    python tools/bench_invert.py [--out profiles/invert_bench.txt] [--skip_step]

``--precision f16`` / ``bf16`` (or a list: ``f32,f16,bf16``) times the 16-bit path instead:
(a) l2i_gram_loss_h8 + l2i_gram_bwd_h8 beside the fp32 pair at the same eight tap shapes, same protocol; GB/s against the least traffic of the
    16-bit pair, which is half the fp32 bytes for c and g.  Then Vgg16Gram16.loss with its image gradient.
(b) inversion iterations/s per precision at 256^2 (batch 1 and 8) and 1024^2 (batch 1), with the library calls of one iteration counted.

    python tools/bench_invert.py --precision f32,f16,bf16 --out profiles/invert16_bench.txt

``--hipgraph`` times the replayed iteration (Inverter(capture=True)) against the eager loop of the same build instead: iterations/s per precision
at the same three shapes, three alternating runs a side (5 warm-up calls, median of 20 calls of 10 iterations each), the ratio with all runs, and
the library calls and graph launches of one iteration on each side.

    python tools/bench_invert.py --precision f32,f16,bf16 --hipgraph --out profiles/invert_graph_bench.txt
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAPS = ((64, 65536), (128, 16384), (256, 4096), (512, 1024))
HBM = 6.3e12


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


def composite(c, gt):
    x = c.detach().requires_grad_()
    f = torch.relu(x).flatten(2)
    g = f.bmm(f.transpose(1, 2)) / (f.shape[1] * f.shape[2])
    loss = (torch.sum((gt - g).pow(2), [1, 2]) * (f.shape[1] ** 2)).sum()
    loss.backward()
    return x.grad


def kernels_row(b, ch, hw, lines):
    from latent2im_amd import kernels as K
    # cold inputs: the calls rotate through enough copies of c that one round is over 512 MiB, twice the 256 MiB of last-level cache
    copies = max(3, min(256, -(-(512 << 20) // (b * ch * hw * 4))))
    cs = [torch.randn(b, ch, hw, device='cuda') for _ in range(copies)]
    gt = K.gram_loss(torch.randn(b, ch, hw, device='cuda'))
    one = torch.ones(b, device='cuda')
    out = torch.empty_like(cs[0])
    turn = [0]

    def nxt():
        turn[0] = (turn[0] + 1) % copies
        return cs[turn[0]]

    def fused():                                         # as the product calls them: the wrappers allocate G, D and the partials per call
        c = nxt()
        _, d, _ = K.gram_loss(c, gt)
        K.gram_bwd(c, d, scale=one, out=out)

    mine, theirs = [], []
    for _ in range(3):                                   # alternating runs: the spread of each side is its run-to-run noise
        mine.append(timed(fused))
        theirs.append(timed(lambda: composite(nxt(), gt)))
    bytes_alg = 3.0 * cs[0].numel() * 4                  # the least traffic: c read by each kernel, g written once (partials, G, D not counted)
    m, t = statistics.median(mine), statistics.median(theirs)
    lines.append('B %d  C %4d  HW %6d   fused %8.1f us (runs %s)  %6.0f GB/s = %4.1f %% of 6.3 TB/s   rocBLAS composite %8.1f us (runs %s)   fused / composite %.2f'
                 % (b, ch, hw, m * 1e6, ' '.join('%.1f' % (v * 1e6) for v in mine), bytes_alg / m / 1e9, 100 * bytes_alg / m / HBM, t * 1e6,
                    ' '.join('%.1f' % (v * 1e6) for v in theirs), m / t))
    print(lines[-1], flush=True)


def kernels16_row(b, ch, hw, prec, lines):
    """The h8 pair of ``prec`` beside the fp32 pair on the same values, alternating runs, cold inputs (each side rotates through > 512 MiB)."""
    from latent2im_amd import conv, kernels as K, kernels16 as K16
    dtype = torch.float16 if prec == 'f16' else torch.bfloat16
    h, w = (hw // 256, 256) if hw >= 256 else (1, hw)
    copies32 = max(3, min(256, -(-(512 << 20) // (b * ch * hw * 4))))
    copies16 = max(3, min(512, -(-(512 << 20) // (b * ch * hw * 2))))
    c32 = [torch.randn(b, ch, hw, device='cuda') for _ in range(copies32)]
    c16 = [conv.to_h8(torch.randn(b, ch, h, w, device='cuda'), dtype=dtype) for _ in range(copies16)]
    gt = K.gram_loss(torch.randn(b, ch, hw, device='cuda'))
    one = torch.ones(b, device='cuda')
    out32, out16 = torch.empty_like(c32[0]), torch.empty_like(c16[0])
    turn = [0, 0]

    def f32():
        turn[0] = (turn[0] + 1) % copies32
        _, d, _ = K.gram_loss(c32[turn[0]], gt)
        K.gram_bwd(c32[turn[0]], d, scale=one, out=out32)

    def h8():
        turn[1] = (turn[1] + 1) % copies16
        _, d, _ = K16.gram_loss(c16[turn[1]], gt)
        K16.gram_bwd(c16[turn[1]], d, scale=one, out=out16)

    mine, theirs = [], []
    for _ in range(3):
        mine.append(timed(h8))
        theirs.append(timed(f32))
    bytes_alg = 3.0 * c16[0].numel() * 2                  # c read by each kernel, g written once, two bytes an element
    m, t = statistics.median(mine), statistics.median(theirs)
    lines.append('%-4s B %d  C %4d  HW %6d   h8 pair %8.1f us (runs %s)  %6.0f GB/s = %4.1f %% of 6.3 TB/s   fp32 pair %8.1f us (runs %s)   h8 / fp32 %.2f'
                 % (prec, b, ch, hw, m * 1e6, ' '.join('%.1f' % (v * 1e6) for v in mine), bytes_alg / m / 1e9, 100 * bytes_alg / m / HBM, t * 1e6,
                    ' '.join('%.1f' % (v * 1e6) for v in theirs), m / t))
    print(lines[-1], flush=True)


def _networks(size, prec):
    """(generator, VGG-16 Gram network) of one precision on synthetic weights (conv.PRECISION is set for the 16-bit classes)."""
    from latent2im_amd import conv, synth, vgg16_specs
    if prec == 'f32':
        from latent2im_amd.generator import Generator
        from latent2im_amd.perceptual16 import Vgg16Gram
    else:
        conv.PRECISION = prec
        from latent2im_amd.nets16 import Generator
        from latent2im_amd.perceptual16 import Vgg16Gram16 as Vgg16Gram
    return Generator(synth.generator_state(size, seed=100, noise_strength=0.5), size, device='cuda'), Vgg16Gram(vgg16_specs.vgg16_state(), device='cuda')


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


def vgg_row(b, lines, size=256, prec='f32'):
    """Vgg16Gram.loss and its image gradient as the inversion calls them: ten convs, three pools, four Gram terms each way."""
    if prec != 'f32':
        net = _networks(32, prec)[1]
        grams = net.target_grams(torch.rand(b, 3, size, size, device='cuda') * 2 - 1)
        x = (torch.rand(b, 3, size, size, device='cuda') * 2 - 1).requires_grad_()

        def both16():
            x.grad = None
            net.loss(x, grams).sum().backward()
        runs = [timed(both16) for _ in range(3)]
        lines.append('%-4s Vgg16Gram16 loss + image gradient %d^2  batch %d   %.2f ms (runs %s)' % (prec, size, b, 1e3 * statistics.median(runs), ' '.join('%.2f' % (1e3 * v) for v in runs)))
        print(lines[-1], flush=True)
        return
    from latent2im_amd import vgg16_specs
    from latent2im_amd.perceptual16 import Vgg16Gram
    net = Vgg16Gram(vgg16_specs.vgg16_state(), device='cuda')
    grams = net.target_grams(torch.rand(b, 3, size, size, device='cuda') * 2 - 1)
    x = (torch.rand(b, 3, size, size, device='cuda') * 2 - 1).requires_grad_()
    coef = torch.linspace(0.5, 1.5, b, device='cuda')

    def both():
        x.grad = None
        (net.loss(x, grams) * coef).sum().backward()

    runs = [timed(both) for _ in range(3)]
    lines.append('Vgg16Gram loss + image gradient %d^2  batch %d   %.2f ms (runs %s)' % (size, b, 1e3 * statistics.median(runs), ' '.join('%.2f' % (1e3 * v) for v in runs)))
    print(lines[-1], flush=True)


def step_row(b, lines, size=256):
    from latent2im_amd import synth, vgg16_specs
    from latent2im_amd.generator import Generator
    from latent2im_amd.invert import Inverter
    from latent2im_amd.perceptual16 import Vgg16Gram
    gen = Generator(synth.generator_state(size, seed=100, noise_strength=0.5), size, device='cuda')
    inv = Inverter(gen, Vgg16Gram(vgg16_specs.vgg16_state(), device='cuda'), lr=0.01, optim='Adam', n_mean_latent=256)
    batch = torch.rand(b, 3, size, size, device='cuda') * 2 - 1
    n = 10
    t = timed(lambda: inv.invert(batch, n), warmup=1, reps=5)
    lines.append('inversion %d^2  batch %d   %.2f iterations/s (%.1f ms per iteration, median of 5 runs of %d)' % (size, b, n / t, 1e3 * t / n, n))
    print(lines[-1], flush=True)


def step16_row(size, b, prec, lines, n=10):
    """Iterations/s of one precision (noise drawn per iteration), three runs of the median-of-5 timing, and the library calls of one iteration."""
    from latent2im_amd import conv
    from latent2im_amd.invert import Inverter
    gen, vgg = _networks(size, prec)
    inv = Inverter(gen, vgg, lr=0.01, optim='Adam', n_mean_latent=256, batch=b)
    batch = torch.rand(b, 3, size, size, device='cuda') * 2 - 1
    runs = [timed(lambda: inv.invert(batch, n), warmup=1, reps=5) for _ in range(3)]
    calls = (count_calls(lambda: inv.invert(batch, 3)) - count_calls(lambda: inv.invert(batch, 1))) // 2
    t = statistics.median(runs)
    lines.append('%-4s inversion %4d^2  batch %d   %7.2f iterations/s (%.1f ms per iteration; runs %s iterations/s)   %d library calls per iteration%s'
                 % (prec, size, b, n / t, 1e3 * t / n, ' '.join('%.2f' % (n / v) for v in runs), calls,
                    '' if inv.scaler is None else '   scaler %s' % inv.scaler.stats()))
    print(lines[-1], flush=True)
    conv.PRECISION = 'f32'


def count_replays(fn):
    """hipGraph launches (torch.cuda.CUDAGraph.replay) made by one run of ``fn``."""
    n = [0]
    real = torch.cuda.CUDAGraph.replay

    def replay(self):
        n[0] += 1
        return real(self)
    torch.cuda.CUDAGraph.replay = replay
    try:
        fn()
    finally:
        torch.cuda.CUDAGraph.replay = real
    return n[0]


def graph_row(size, b, prec, lines, n=10):
    """Iterations/s of the eager loop and of the replayed one (noise drawn per iteration on both), alternating, and what one iteration issues."""
    from latent2im_amd import conv
    from latent2im_amd.invert import Inverter
    batch = torch.rand(b, 3, size, size, device='cuda') * 2 - 1
    sides = {}
    for name, cap in (('eager', False), ('replayed', True)):                 # a pair of networks a side: an fp16 Inverter attaches its scaler to them
        gen, vgg = _networks(size, prec)
        sides[name] = Inverter(gen, vgg, lr=0.01, optim='Adam', n_mean_latent=256, batch=b, capture=cap)
    sides['replayed'].invert(batch, 1)                                       # the capture, outside every timing
    runs = {k: [] for k in sides}
    for _ in range(3):                                                       # alternating runs: the spread of each side is its run-to-run noise
        for k, inv in sides.items():
            runs[k].append(timed(lambda: inv.invert(batch, n)))
    med = {k: statistics.median(v) for k, v in runs.items()}
    its = {k: [n / v for v in vs] for k, vs in runs.items()}
    ratios = [e / r for e, r in zip(runs['eager'], runs['replayed'])]        # replayed / eager in iterations/s, run by run
    lo, hi = min(its['eager']) / max(its['eager']), max(its['eager']) / min(its['eager'])
    r_lo, r_hi = min(its['replayed']) / max(its['replayed']), max(its['replayed']) / min(its['replayed'])
    ratio = med['eager'] / med['replayed']
    inside = lo * r_lo <= ratio <= hi * r_hi
    calls, launches = {}, {}
    for k, inv in sides.items():
        calls[k] = (count_calls(lambda: inv.invert(batch, 3)) - count_calls(lambda: inv.invert(batch, 1))) // 2
        launches[k] = (count_replays(lambda: inv.invert(batch, 3)) - count_replays(lambda: inv.invert(batch, 1))) // 2
    lines.append('%-4s inversion %4d^2  batch %d   eager %7.2f it/s (%.2f ms; runs %s)   replayed %7.2f it/s (%.2f ms; runs %s)   replayed / eager %.2f (runs %s)%s'
                 '   per iteration: eager %d library calls + %d graph launches, replayed %d + %d%s'
                 % (prec, size, b, n / med['eager'], 1e3 * med['eager'] / n, ' '.join('%.2f' % v for v in its['eager']), n / med['replayed'],
                    1e3 * med['replayed'] / n, ' '.join('%.2f' % v for v in its['replayed']), ratio, ' '.join('%.2f' % v for v in ratios),
                    '  INSIDE the two sides\' spread' if inside else '', calls['eager'], launches['eager'], calls['replayed'], launches['replayed'],
                    '' if sides['replayed'].scaler is None else '   scaler %s' % sides['replayed'].scaler.stats()))
    print(lines[-1], flush=True)
    conv.PRECISION = 'f32'


def main16(precs, args, lines):
    for prec in [p for p in precs if p != 'f32']:
        for b in (1, 8):
            for ch, hw in TAPS:
                kernels16_row(b, ch, hw, prec, lines)
        for b in (1, 8):
            vgg_row(b, lines, prec=prec)
    if not args.skip_step:
        for size, b in ((256, 1), (256, 8), (1024, 1)):
            for prec in precs:
                step16_row(size, b, prec, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip_step', action='store_true')
    ap.add_argument('--precision', default='f32', help='f32 (the fp32 pair against the rocBLAS composite), or f16 / bf16 / a comma list with f32: the 16-bit path against fp32')
    ap.add_argument('--hipgraph', action='store_true', help='iterations/s of the replayed iteration (Inverter(capture=True)) against the eager loop')
    ap.add_argument('--shapes', default='256x1,256x8,1024x1', help='--hipgraph: comma list of SIZExBATCH')
    args = ap.parse_args()
    precs = args.precision.split(',')
    assert all(p in ('f32', 'f16', 'bf16') for p in precs), precs
    lines = ['# tools/bench_invert.py --precision %s%s on %s' % (args.precision, ' --hipgraph' if args.hipgraph else '', torch.cuda.get_device_name(0))]
    if args.hipgraph:
        lines.append('# eager = Inverter(capture=False), replayed = Inverter(capture=True): HIP events around invert(batch, 10), 5 warm-up calls, median of 20, '
                     'three alternating runs a side; ms = per iteration')
        shapes = [tuple(int(v) for v in t.split('x')) for t in args.shapes.split(',')]
        for size, b in shapes:
            for prec in precs:
                graph_row(size, b, prec, lines)
                if args.out:                                                 # row by row: a long run leaves what it measured
                    with open(args.out, 'w') as f:
                        f.write('\n'.join(lines) + '\n')
        return
    if precs != ['f32']:
        main16(precs, args, lines)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    for b in (1, 8):
        for ch, hw in TAPS:
            kernels_row(b, ch, hw, lines)
    for b in (1, 8):
        vgg_row(b, lines)
    if not args.skip_step:
        for b in (1, 8):
            step_row(b, lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
