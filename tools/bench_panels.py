"""python tools/bench_panels.py [--out profiles/panels_bench.txt] [--sizes 256,1024] [--skip-driver]: what showing a trained walk costs.

B = 8 samples, P = 7 panels, strips (G = B grids of 1 x P tiles, pad 0), at 256^2 and 1024^2.  Every figure is measured on the GPU; no figure is
fixed in advance, and the claim under test is only that the new path is slower at no measured shape.

A. l2i_panels_u8 against the torch composite on the device, ((x + 1) / 2 * 255).clamp(0, 255).to(uint8) + permute + cat into the same strips.
   HIP events, 5 warm-up calls, median of 20, three alternating runs a side; every call reads another copy of the panels, the copies together
   exceed 512 MiB, so that no call finds its input in the Infinity Cache.  GB/s = the bytes the job needs (4 read + 1 written per value: 15 per
   pixel) over the time, for both sides; the composite moves more than that, which is the point.
B. The kernel plus one uint8 device-to-host copy against the host path of graph.vis_multi_image_batch_alphas (per panel: fp32 device-to-host
   copy, numpy clip_ims; per sample: np.concatenate): host clock around work that ends on the host, median of 5, alternating.
C. One batch of vis_w.py: graph.vis_multi_image_batch_alphas (the method a plain invocation runs, unchanged by this work: the parent commit's
   path) against graph.vis_sweep_strips (sweep + l2i_panels_u8), for fp32 networks and for --precision f16 — where the parent, which never set
   the precision, ran an f16-trained walk on fp32 networks.  Synthetic weights; host clock, median of 3 after one warm-up, alternating; PNG
   encoding replaced by a no-op in the timed runs (it is the same bytes on both sides and, at 1024^2, several times everything else), then one
   run a side with it."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latent2im_amd import conv, kernels, selfcheck           # noqa: E402

B, P = 8, 7
RATE = 6.3e12          # the HBM rate this project takes as achievable


def event_ms(fn, warm=5, reps=20):
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


def host_ms(fn, warm=1, reps=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def composite(x, R):
    """The strips [B, R, P * R, 3] uint8 of x [P * B, 3, R, R] with torch ops on the device."""
    q = ((x + 1) / 2 * 255).clamp(0, 255).to(torch.uint8).view(P, B, 3, R, R)
    return torch.cat([q[p].permute(0, 2, 3, 1) for p in range(P)], 2)


def host_path(x, R):
    """What graph.vis_multi_image_batch_alphas does with its P panels: fp32 copies, numpy clip_ims, one concatenate per sample."""
    ims = [np.uint8(np.clip(((x[p * B:(p + 1) * B].cpu().numpy() + 1) / 2.0) * 255, 0, 255)) for p in range(P)]
    return [np.concatenate([im[i].transpose(1, 2, 0) for im in ims], axis=1) for i in range(B)]


def parts_ab(out, R):
    n = P * B * 3 * R * R
    copies = max(2, (512 * 2 ** 20) // (4 * n) + 1)
    gen = torch.Generator(device='cuda').manual_seed(R)
    xs = [torch.rand((P * B, 3, R, R), device='cuda', generator=gen) * 2.4 - 1.2 for _ in range(copies)]
    tiles = torch.tensor([p * B + i for i in range(B) for p in range(P)], dtype=torch.int32, device='cuda')
    dst = torch.empty(B, R, P * R, 3, dtype=torch.uint8, device='cuda')
    same = torch.equal(kernels.panels_u8(xs[0], tiles, B, 1, P, out=dst), composite(xs[0], R))
    host = host_path(xs[0], R)
    same_host = all(np.array_equal(dst[i].cpu().numpy(), host[i]) for i in range(B))
    out.append('%d^2: %d values (%.1f MB fp32 in, %.1f MB uint8 out), %d input copies; kernel == composite: %s, == host path: %s'
               % (R, n, 4 * n / 1e6, n / 1e6, copies, same, same_host))
    need = 5.0 * n
    for run in range(3):
        k = event_ms(lambda i: kernels.panels_u8(xs[i % copies], tiles, B, 1, P, out=dst))
        c = event_ms(lambda i: composite(xs[i % copies], R))
        out.append('  A run %d  l2i_panels_u8 %8.4f ms  %7.1f GB/s (%4.1f %% of %.1f TB/s)   torch composite %8.4f ms  %7.1f GB/s of needed bytes   composite / kernel %.2f'
                   % (run, k, need / k / 1e6, 100 * need / (k * 1e-3) / RATE, RATE / 1e12, c, need / c / 1e6, c / k))
    for run in range(3):
        k = host_ms(lambda: kernels.panels_u8(xs[0], tiles, B, 1, P, out=dst).cpu().numpy())
        h = host_ms(lambda: host_path(xs[0], R))
        out.append('  B run %d  kernel + uint8 copy %9.3f ms (min %.3f max %.3f)   host path %9.3f ms (min %.3f max %.3f)   host / kernel %.2f'
                   % ((run,) + k + h + (h[0] / k[0],)))


def part_c(out, R, encode_once=True):
    from PIL import Image
    z = np.random.RandomState(1).randn(B, 512).astype(np.float32)
    real_save = Image.Image.save
    graphs = {}
    for precision in ('f32', 'f16'):
        conv.PRECISION = precision
        graphs[precision] = selfcheck.build_graph(R, ['Smiling'], B)
    conv.PRECISION = 'f32'
    g32 = graphs['f32']
    alphas = [a * np.ones((B, g32.Nsliders)) for a in np.linspace(0, 1, P)]
    with tempfile.TemporaryDirectory() as tmp:
        def old(g):
            return lambda: g.vis_multi_image_batch_alphas({'z': z}, os.path.join(tmp, 'old'), alphas, None, 0, name='Smiling')

        def new(g):
            return lambda: g.vis_sweep_strips({'z': z}, os.path.join(tmp, 'new'), alphas, None, 0, name='Smiling')

        sides = [('parent path, fp32 networks', old(graphs['f32'])), ('sweep + panels, fp32 networks', new(graphs['f32'])),
                 ('parent method on f16 networks', old(graphs['f16'])), ('sweep + panels, --precision f16', new(graphs['f16']))]
        Image.Image.save = lambda self, *a, **k: None
        try:
            for _, fn in sides:
                fn()                                            # warm-up: code objects, weight packs, allocator
            res = {name: [] for name, _ in sides}
            for run in range(3):
                for name, fn in sides:
                    res[name].append(host_ms(fn, warm=0, reps=1)[0])
        finally:
            Image.Image.save = real_save
        out.append('%d^2  C. one batch of %d samples x %d panels, ms (median of 3 alternating runs; PNG encoding off)' % (R, B, P))
        med = {name: float(np.median(v)) for name, v in res.items()}
        for name, _ in sides:
            out.append('    %-34s %9.2f ms   (runs: %s)' % (name, med[name], ' '.join('%.2f' % v for v in res[name])))
        out.append('    fp32: parent / new %.2f;   f16-trained walk: parent (fp32 networks) / new (--precision f16) %.2f;   f16 networks: old method / new %.2f'
                   % (med[sides[0][0]] / med[sides[1][0]], med[sides[0][0]] / med[sides[3][0]], med[sides[2][0]] / med[sides[3][0]]))
        if encode_once:
            enc = {name: host_ms(fn, warm=0, reps=1)[0] for name, fn in sides[:2]}
            out.append('    with PNG encoding (one run a side): parent %.1f ms, new %.1f ms' % (enc[sides[0][0]], enc[sides[1][0]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'panels_bench.txt'))
    ap.add_argument('--sizes', default='256,1024')
    ap.add_argument('--skip-driver', action='store_true', help='parts A and B only')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_panels.py measures on the GPU: none is visible')
    out = ['tools/bench_panels.py on %s; B = %d, P = %d; kernel sources %s' % (torch.cuda.get_device_name(0), B, P, __import__('latent2im_amd')._lib.source_hash())]
    saved = conv.PRECISION
    try:
        for R in [int(s) for s in a.sizes.split(',')]:
            parts_ab(out, R)
            if not a.skip_driver:
                part_c(out, R)
            torch.cuda.empty_cache()
    finally:
        conv.PRECISION = saved
    text = '\n'.join(out) + '\n'
    print(text)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
