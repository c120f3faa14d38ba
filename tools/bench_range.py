"""python tools/bench_range.py [--out profiles/range_stats_bench.txt]: what the range monitor costs.

A. l2i_range_stats (kernels16.range_stats) against what nets16._probe does in torch (a float copy, abs, the masked median, four host reads) on three
   fp16 h8 maps of the config-5 step (1024^2, batch 8): the largest generator map, a mid-size ResNet-50 map and a 64^2 one.  HIP events, 5 warm-up
   calls, median of 20, three alternating runs a side; every call reads another copy of the map, the copies together exceed 512 MiB, so that no
   call finds its input in the Infinity Cache.  GB/s = the map's bytes over the time, against the 6.3 TB/s this project takes as achievable.
B. The eager fp16 StyleGAN2 step at 256^2, batch 4 with a monitor set (and never read) and without: library calls added and ms per step, same protocol."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latent2im_amd import _lib, conv, kernels16, nets16, selfcheck, synth           # noqa: E402

READ_RATE = 6.3e12
MAPS = [('generator 1024^2 x 32ch', (8, 4, 1024, 1024, 8)), ('ResNet-50 layer2 128^2 x 512ch', (8, 64, 128, 128, 8)), ('ResNet-50 layer3 64^2 x 1024ch', (8, 128, 64, 64, 8))]


def timed(fn, warm=5, reps=20):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(warm + i)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def gradient_like(shape, seed):
    """A map shaped like a stored fp16 gradient: log-normal magnitudes around 2^-6 over ~10 octaves, a quarter exact zeros (masks, padding)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    t = torch.randn(shape, device='cuda', generator=g) * torch.exp2(torch.randn(shape, device='cuda', generator=g) * 2.5 - 6)
    t = t * (torch.rand(shape, device='cuda', generator=g) > 0.25)
    return t.to(torch.float16)


def part_a(out):
    out.append('A. one map: l2i_range_stats vs the torch probe of nets16._probe (ms, median of 20; three alternating runs)')
    for name, shape in MAPS:
        n = int(np.prod(shape))
        copies = max(2, (512 * 2 ** 20) // (2 * n) + 1)
        maps = [gradient_like(shape, 10 + i) for i in range(copies)]
        row = torch.zeros(kernels16.RANGE_WORDS, dtype=torch.int64, device='cuda')
        sink = []

        def kernel(i):
            kernels16.range_stats(maps[i % copies], row)

        def probe(i):
            nets16.PROBE = sink
            try:
                nets16._probe('bench', maps[i % copies])
            finally:
                nets16.PROBE = None
        runs = [(timed(kernel), timed(probe)) for _ in range(3)]
        for k, p in runs:
            out.append('  %-32s %6.1f MB x %d copies   range_stats %8.1f us  %7.1f GB/s (%4.1f %% of 6.3 TB/s)   torch probe %9.1f us   x%.0f'
                       % (name, 2 * n / 1e6, copies, k * 1e3, 2 * n / (k * 1e-3) / 1e9, 100 * 2 * n / (k * 1e-3) / READ_RATE, p * 1e3, p / k))
        del maps


def part_b(out):
    conv.PRECISION = 'f16'
    attrs = ['dirty', 'daylight', 'night', 'sunrisesunset', 'dawndusk']
    g = selfcheck.build_graph(256, attrs, 4, lr=1e-3, transform='scene')
    zs = [synth.z_sample(4, seed=40 + i) for i in range(8)]
    al = np.ones((4, 5)) * np.random.RandomState(3).uniform(-1, 1, 5)
    mon = nets16.RangeMonitor('cuda')
    seen, real = [], _lib.call

    def counting(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)

    def step(i):
        selfcheck.run_step(g, zs[i % 8], al, clamp=True)
    calls = {}
    for label, m in (('off', None), ('on', mon)):
        nets16.MONITOR = m
        _lib.call = counting
        del seen[:]
        step(0)
        _lib.call = real
        calls[label] = (len(seen), seen.count('l2i_range_stats'))
    runs = []
    for _ in range(3):
        pair = []
        for m in (None, mon):
            nets16.MONITOR = m
            pair.append(timed(step))
        runs.append(pair)
    nets16.MONITOR = None
    out.append('B. eager fp16 StyleGAN2 step, 256^2, batch 4, five attributes, all loss terms: --f16_watch off / on (monitor set, never read)')
    out.append('  library calls a step (conv launches not counted): %d / %d, of them l2i_range_stats: %d / %d' % (calls['off'][0], calls['on'][0], calls['off'][1], calls['on'][1]))
    for off, on in runs:
        out.append('  ms per step (median of 20): off %.3f   on %.3f   (%+.2f %%)' % (off, on, 100 * (on - off) / off))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'range_stats_bench.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_range.py measures on the GPU'
    lines = ['# tools/bench_range.py on %s, kernel sources %s' % (torch.cuda.get_device_name(0), _lib.source_hash())]
    part_a(lines)
    part_b(lines)
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)
