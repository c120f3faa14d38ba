"""Timing of the regressor trainer's step (scene_regressor_256.py) at the workload's own size — batch 32 at 256^2 — on one GPU: is the step
host-bound, and what do the resident model and the hipGraph replay buy?  HIP events, 5 warm-up calls, median of 20, three alternating runs per
side in one call; the sides start from the same state and their first three losses must agree within 2e-3 (the loss bar of the step tests).

  eager       regressor_train.train_step: 53 FrozenConv2d rebuilt per step, BatchNorm algebra in torch, torch.optim.Adam (the default path)
  resident    train_step_resident: gradient arena, finalize kernels, in-place repack, GuardedAdam — still one launch at a time from Python
  replayed    capture.CapturedRegressorStep, inputs staged from the host through the pinned ring
  replayed+dd the same graph fed by a DeviceDataset index, beside `PIL+replayed`: the PIL loader decoding 32 PNGs on the main thread for it

Also: the in-place repack of the whole net (53 repack_ calls) as GB/s of its least traffic — every pack written once, the weight read once per
pack — against 6.3 TB/s, with the time per launch.

    python tools/bench_regressor_train.py [--out profiles/regressor_train_graph_bench.txt] [--batch 32] [--size 256]
    python tools/bench_regressor_train.py --only resident --steps 3      # one side, a few steps: the run to put under a kernel trace

--precision f32,f16,bf16 (profiles/regressor_train16_bench.txt): the resident fp32 step beside the 16-bit trainer
(regressor_train.TrainableResNet50H8) of each listed element type, same method; the first three losses of each side; the host's share of a step
(the time Python and the torch packing ops take to ISSUE it, against the time the GPU takes to run it).  --wgrad_table: every distinct weight-
gradient shape of ResNet-50 at that batch and size, l2i_conv2d_wgrad_h8 (fp16) against l2i_conv2d_wgrad_f32 on the same maps cast to fp32.
L2I_LIB=<another build> --precision f32 times the fp32 side on that build (the parent's, for the comparison of the same session).
--only f16 / bf16 runs a few steps of the 16-bit trainer alone (the run to put under a kernel trace); with --hip_graph those steps are replays of
capture.CapturedRegressorStep.  --precision ... --hip_graph adds, per 16-bit side, the same step replayed from a hipGraph (its own model, same
state), and the in-place repack of the 16-bit planes alone (replan(): GPU time and GB/s of its least traffic).  --stem_table: conv1's weight
gradient alone, l2i_conv2d_wgrad_img_h8 against cast_from_h8 + l2i_conv2d_wgrad_f32 on the same maps, both element types
(profiles/regressor_train16_repro_bench.txt).  L2I_LIB=<the parent's build> runs the same Python on the parent's kernels: the 16-bit trainer then
takes the path it had (fp32 atomics for conv1, torch repack) and --hip_graph / --stem_table have nothing to run.
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def png_set(root, n, size):
    from PIL import Image
    rs = np.random.RandomState(1)
    os.makedirs(os.path.join(root, 'a'))
    names = []
    with open(os.path.join(root, 'annotations.tsv'), 'w') as f:
        for i in range(n):
            names.append('a/%03d.png' % i)
            Image.fromarray(rs.randint(0, 256, size=(size + 24, size + 64, 3)).astype(np.uint8)).save(os.path.join(root, names[-1]))
            f.write(names[-1] + '\t' + '\t'.join('%.4f,1.0' % v for v in rs.rand(40)) + '\n')
    with open(os.path.join(root, 'training.txt'), 'w') as f:
        f.write('\n'.join(names) + '\n')


def wgrad_shapes(size):
    """Every distinct (k, stride, pad, cin, cout, input side) the h8 weight-gradient kernel runs in one step of ResNet-50 on ``size``^2 images."""
    from latent2im_amd.specs import RESNET50_LAYERS
    out, inpl, hw = [], 64, size // 4
    for planes, blocks, stride in RESNET50_LAYERS:
        for b in range(blocks):
            s = stride if b == 0 else 1
            rows = [(1, 1, 0, inpl, planes, hw), (3, s, 1, planes, planes, hw), (1, 1, 0, planes, 4 * planes, hw // s)]
            if b == 0:
                rows.append((1, s, 0, inpl, 4 * planes, hw))
            for r in rows:
                if r not in out:
                    out.append(r)
            inpl, hw = 4 * planes, hw // s
    return out


def wgrad_table(B, S, say):
    from latent2im_amd import _lib
    from latent2im_amd import kernels16 as K16
    say('weight gradient per shape, batch %d at %d^2: l2i_conv2d_wgrad_h8 (fp16 maps) against l2i_conv2d_wgrad_f32 (the same maps cast to fp32); %s' % (B, S, torch.cuda.get_device_name(0)))
    say('  %-34s %10s %9s %10s %9s %7s  %s' % ('k s  cin -> cout, map', 'h8 ms', 'TFLOP/s', 'f32 ms', 'TFLOP/s', 'f32/h8', 'slices x tiles x taps'))
    g = torch.Generator(device='cuda').manual_seed(1)
    slower = []
    for k, s, pad, cin, cout, h in wgrad_shapes(S):
        oh = (h + 2 * pad - k) // s + 1
        x = torch.randn(B, cin // 8, h, h, 8, device='cuda', generator=g).to(torch.float16)
        gy = (torch.randn(B, cout // 8, oh, oh, 8, device='cuda', generator=g) * 0.1).to(torch.float16)
        x32, gy32 = K16.cast_from_h8(x), K16.cast_from_h8(gy)
        ws = torch.empty(K16.wgrad_ws_bytes(B, cin, h, h, cout, oh, oh, k, s, pad, x.dtype) // 4, device='cuda')
        dw, dw32 = torch.empty(cout, cin, k, k, device='cuda'), torch.zeros(cout, cin, k, k, device='cuda')
        t16 = timed(lambda: K16.conv_wgrad(x, gy, k, s, pad, out=dw, ws=ws))
        t32 = timed(lambda: _lib.call('l2i_conv2d_wgrad_f32', _lib.fptr(dw32), _lib.fptr(x32), _lib.fptr(gy32), B, cin, h, h, cout, oh, oh, k, k, s, pad, pad))
        flop = 2.0 * B * oh * oh * cin * cout * k * k
        tiles = ((cin + 63) // 64) * ((cout + 63) // 64)
        say('  %dx%d s%d %4d -> %4d, %3d^2 -> %3d^2 %10.3f %9.1f %10.3f %9.1f %7.1f  %d x %d x %d'
            % (k, k, s, cin, cout, h, oh, t16 * 1e3, flop / t16 / 1e12, t32 * 1e3, flop / t32 / 1e12, t32 / t16, ws.numel() // (4096 * tiles * k * k), tiles, k * k))
        if t16 > t32:
            slower.append((k, s, cin, cout, h))
    say('  rows on which the new kernel is slower: %s' % (slower or 'none'))


def stem_table(B, S, say):
    """conv1's weight gradient alone at batch B, S^2: the fixed-order kernel on the h8 gradient map as it lies against the pair it replaces (the
    map cast to fp32, then the fp32 atomics kernel), alternating runs in one process."""
    from latent2im_amd import _lib
    from latent2im_amd import kernels16 as K16
    say('stem weight gradient alone, batch %d at %d^2: l2i_conv2d_wgrad_img_h8 against cast_from_h8 + l2i_conv2d_wgrad_f32; %s' % (B, S, torch.cuda.get_device_name(0)))
    if not _lib.has('l2i_conv2d_wgrad_img_h8'):
        return say('  this library has no l2i_conv2d_wgrad_img_h8')
    g = torch.Generator(device='cuda').manual_seed(1)
    oh = (S - 1) // 2 + 1
    x = torch.randn(B, 3, S, S, device='cuda', generator=g) * 0.5
    least = B * 64 * oh * oh * 2 + x.numel() * 4
    flop = 2.0 * B * oh * oh * 64 * 147
    for dtype in (torch.float16, torch.bfloat16):
        gy = (torch.randn(B, 8, oh, oh, 8, device='cuda', generator=g) * 0.1).to(dtype)
        nbytes = K16.wgrad_img_ws_bytes(B, S, S, dtype)
        ws, dw, dw32 = torch.empty(nbytes // 4, device='cuda'), torch.empty(64, 3, 7, 7, device='cuda'), torch.zeros(64, 3, 7, 7, device='cuda')

        def pair():
            dw32.zero_()
            _lib.call('l2i_conv2d_wgrad_f32', _lib.fptr(dw32), _lib.fptr(x), _lib.fptr(K16.cast_from_h8(gy)), B, 3, S, S, 64, oh, oh, 7, 7, 2, 3, 3)
        new = lambda: K16.conv_wgrad_img(x, gy, out=dw, ws=ws)
        runs = {'new': [], 'pair': []}
        for _ in range(3):
            runs['new'].append(timed(new))
            runs['pair'].append(timed(pair))
        tn, tp = statistics.median(runs['new']), statistics.median(runs['pair'])
        spread = max((max(v) - min(v)) / statistics.median(v) for v in runs.values())
        rel = float((dw - dw32).norm() / dw32.norm())
        say('  %-8s new %s ms (median %.3f) = %.0f GB/s of the %.1f MB least traffic (%.1f %% of 6.3 TB/s), %.1f TFLOP/s; %d slices, %.1f MB workspace'
            % (str(dtype).split('.')[1], ' '.join('%.3f' % (t * 1e3) for t in runs['new']), tn * 1e3, least / tn / 1e9, least / 1e6, 100 * least / tn / HBM,
               flop / tn / 1e12, nbytes // K16.WGRAD_IMG_SLICE_BYTES, nbytes / 1e6))
        say('  %-8s cast + fp32 atomics %s ms (median %.3f); pair / new %.2fx; largest run-to-run spread %.1f %%; relative L2 difference of the two dw %.2e'
            % ('', ' '.join('%.3f' % (t * 1e3) for t in runs['pair']), tp * 1e3, tp / tn, 100 * spread, rel))


def precision_bench(precisions, B, S, st, data, label, say, hip_graph=False, data_h=None, label_h=None):
    """The resident fp32 step and the 16-bit trainer of each listed element type: losses, step times, the host's share."""
    import time
    from latent2im_amd import _lib
    from latent2im_amd import regressor_train as RT
    say('regressor training step, batch %d at %d^2, sides %s; %s; library %s' % (B, S, ', '.join(precisions), torch.cuda.get_device_name(0), os.path.basename(os.path.dirname(_lib.LIB_PATH)) or '.'))
    sides = {}
    for p in precisions:
        m = RT.make_model(st, precision=p, resident=True, **({} if p == 'f32' else dict(image_size=S, batch=B)))
        o = RT.make_optimizer(m, guarded=True)
        sides[p] = (m, o, (lambda m=m, o=o: RT.train_step_resident(m, o, data, label)))
        if hip_graph and p != 'f32':
            from latent2im_amd import capture
            if not (m.stem_kernel and m.planes_kernel):
                say('  %s: this library has no in-place repack: the 16-bit step cannot be recorded' % p)
                continue
            m2 = RT.make_model(st, precision=p, resident=True, image_size=S, batch=B)
            o2 = RT.make_optimizer(m2, guarded=True)
            g = capture.CapturedRegressorStep(m2, o2, B, S)
            sides[p + '+graph'] = (m2, o2, (lambda g=g: g(data_h, label_h)))
    for p, (m, o, fn) in sides.items():
        say('  first three losses, %-5s %s%s' % (p, ' '.join('%.6f' % float(fn()) for _ in range(3)), '' if p == 'f32' else '   (static scale 2^%d)' % m.loss_scale_log2))
    runs = {p: [] for p in sides}
    for _ in range(3):
        for p in sides:
            runs[p].append(timed(sides[p][2]))
    say('  step time, median of 20 after 5 warm-up calls, three alternating runs (ms):')
    for p, v in runs.items():
        say('    %-5s %s   median %.1f ms  = %.1f images/s' % (p, ' '.join('%7.1f' % (t * 1e3) for t in v), statistics.median(v) * 1e3, B / statistics.median(v)))
    med = {p: statistics.median(v) for p, v in runs.items()}
    say('  largest run-to-run spread of a side: %.1f %%' % (100 * max((max(v) - min(v)) / statistics.median(v) for v in runs.values())))
    for p in sides:
        if p != 'f32' and 'f32' in med:
            say('  f32 resident / %-5s %.2fx' % (p, med['f32'] / med[p]))
        if p.endswith('+graph'):
            say('  %s eager / replayed %.2fx' % (p[:-6], med[p[:-6]] / med[p]))
    say('  host share: time to ISSUE one step from Python (no synchronisation inside; median of 10) against the GPU time above')
    for p, (m, o, fn) in sides.items():
        hs, rp = [], []
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            hs.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.replan()
            rp.append(time.perf_counter() - t0)
        say('    %-5s issue %.1f ms of which replan() %.1f ms; GPU %.1f ms: %s' % (p, statistics.median(hs) * 1e3, statistics.median(rp) * 1e3, med[p] * 1e3,
                                                                                    'HOST-BOUND' if statistics.median(hs) > 0.9 * med[p] else 'GPU-bound'))
        if p != 'f32':
            say('    %-5s scaler %s' % (p, o.scaler.stats()))
        if p in ('f16', 'bf16'):
            # the repack alone: every plane written once, every master weight read once per plane set made from it
            byt = sum(t.numel() * 2 for cv in m._convs()[1:] for t in (cv.h8.fwd_planes, cv.h8.bwd_planes)) + m.stem.img.planes.numel() * 2
            byt += sum(cv.weight.numel() * 4 * 2 for cv in m._convs()[1:]) + m.stem.weight.numel() * 4
            t = timed(m.replan)
            say('    %-5s replan() alone: %s, %.1f MB least traffic, GPU %.3f ms = %.0f GB/s (%.1f %% of 6.3 TB/s)'
                % (p, 'one launch over %d segments' % m.planes.nseg if m.planes is not None else 'torch ops per convolution', byt / 1e6, t * 1e3, byt / t / 1e9,
                   100 * byt / t / HBM))


def ranges(say):
    """The largest stored map per stage of one fp16 step (nets16.RangeMonitor / l2i_range_stats on the h8 maps themselves) at the two shapes the
    static exponent was chosen on: what regtrain_scale_for puts near 2^5."""
    from latent2im_amd import nets16, synth
    from latent2im_amd import regressor_train as RT
    st = synth.resnet50_state(seed=300)
    say('stored ranges of one fp16 regressor step (synthetic weights, seed 300; data randn * 0.5, RandomState(5)); gradient maps are stored x 2^e')
    for B, S in ((8, 128), (32, 256)):
        rs = np.random.RandomState(5)
        data, label = torch.from_numpy(rs.randn(B, 3, S, S).astype(np.float32) * 0.5).cuda(), torch.from_numpy(rs.rand(B, 40).astype(np.float32)).cuda()
        m = RT.TrainableResNet50H8(st, device='cuda', precision='f16', image_size=S, batch=B)
        o = RT.make_optimizer(m, guarded=True)
        m.monitor = nets16.RangeMonitor('cuda')
        RT.train_step_resident(m, o, data, label)
        rows = m.monitor.read()
        e = m.loss_scale_log2
        say('  batch %d at %d^2, e = %d (regtrain_scale_for):' % (B, S, e))
        for tag in sorted(rows):
            r = rows[tag]
            say('    %-12s max 2^%6.2f  median octave 2^%d  below-normal share %.3g  non-finite %d' % (tag, r['max_log2'], r['median_octave'], r['below_normal'], r['nonfinite']))
        gmax = max(r['max_log2'] for t, r in rows.items() if t.startswith('T.g.'))
        amax = max(r['max_log2'] for t, r in rows.items() if t.startswith('T.fwd.'))
        say('    largest stored gradient 2^%.2f = true 2^%.2f -> the rule 5 - round(log2 true max) gives e = %d; largest stored activation %.1f'
            % (gmax, gmax - e, 5 - int(round(gmax - e)), 2.0 ** amax))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ranges', action='store_true', help='stored ranges of one fp16 step at 8 x 128^2 and 32 x 256^2 (the static exponent rule)')
    ap.add_argument('--precision', help='comma list of f32, f16, bf16: the 16-bit comparison instead of the fp32 sides')
    ap.add_argument('--wgrad_table', action='store_true', help='the per-shape weight-gradient table')
    ap.add_argument('--stem_table', action='store_true', help="conv1's weight gradient alone: the fixed-order h8 kernel against cast + fp32 atomics")
    ap.add_argument('--hip_graph', action='store_true', help='with --precision: add the 16-bit step replayed from a hipGraph; with --only f16 / bf16: replay')
    ap.add_argument('--out')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--only', choices=('eager', 'resident', 'replayed', 'f16', 'bf16'))
    ap.add_argument('--steps', type=int, default=3)
    a = ap.parse_args()
    from latent2im_amd import capture, synth
    from latent2im_amd import regressor_train as RT
    from tests import regtrain_ref as rr
    B, S = a.batch, a.size
    st = synth.resnet50_state(seed=300)
    rs = np.random.RandomState(5)
    data_h, label_h = torch.from_numpy(rs.randn(B, 3, S, S).astype(np.float32) * 0.5), torch.from_numpy(rs.rand(B, 40).astype(np.float32))
    data, label = data_h.cuda(), label_h.cuda()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, 'a' if (a.precision or a.wgrad_table or a.ranges or a.stem_table) else 'w') as f:
                f.write('\n'.join(lines) + '\n')

    if a.precision or a.wgrad_table or a.ranges or a.stem_table:
        if a.ranges:
            ranges(say)
        if a.precision:
            precision_bench(a.precision.split(','), B, S, st, data, label, say, hip_graph=a.hip_graph, data_h=data_h, label_h=label_h)
        if a.stem_table:
            stem_table(B, S, say)
        if a.wgrad_table:
            wgrad_table(B, S, say)
        return finish()

    def make(side):
        if side in ('f16', 'bf16'):
            m = RT.TrainableResNet50H8(st, device='cuda', precision=side, image_size=S, batch=B)
            o = RT.make_optimizer(m, guarded=True)
            if a.hip_graph:
                g16 = capture.CapturedRegressorStep(m, o, B, S)
                return m, (lambda: g16(data_h, label_h))
            return m, (lambda: RT.train_step_resident(m, o, data, label))
        if side == 'eager':
            m = RT.TrainableResNet50(st, device='cuda')
            o = RT.make_optimizer(m)
            return m, (lambda: RT.train_step(m, o, data, label))
        m = RT.TrainableResNet50(st, device='cuda', resident=True)
        o = RT.make_optimizer(m, guarded=True)
        if side == 'resident':
            return m, (lambda: RT.train_step_resident(m, o, data, label))
        g = capture.CapturedRegressorStep(m, o, B, S)
        return m, (lambda: g(data_h, label_h))

    if a.only:
        _, fn = make(a.only)
        for _ in range(a.steps):
            loss = fn()
        print('%s: %d steps, last loss %.6f' % (a.only, a.steps, float(loss)))
        return
    say('regressor training step, batch %d at %d^2, fp32; %s' % (B, S, torch.cuda.get_device_name(0)))
    sides = {k: make(k) for k in ('eager', 'resident', 'replayed')}
    losses = {k: [float(fn()) for _ in range(3)] for k, (_, fn) in sides.items()}
    for k, v in losses.items():
        say('  first three losses, %-9s %s' % (k, ' '.join('%.6f' % x for x in v)))
    for k in ('resident', 'replayed'):
        assert np.allclose(losses[k], losses['eager'], rtol=2e-3, atol=1e-6), (k, losses)
    # the device dataset against the PIL loader, feeding the same recorded step
    tmp = tempfile.mkdtemp()
    png_set(tmp, 2 * B, S)
    train = RT.CustomDataset(tmp, RT.load_labelfile(os.path.join(tmp, 'annotations.tsv')), os.path.join(tmp, 'training.txt'), image_size=S)
    dd = RT.DeviceDataset(train)
    m = RT.TrainableResNet50(st, device='cuda', resident=True)
    gdd = capture.CapturedRegressorStep(m, RT.make_optimizer(m, guarded=True), B, S, dataset=dd)
    order = [np.random.RandomState(i).permutation(len(train))[:B] for i in range(8)]
    count = [0]

    def replay_dd():
        count[0] += 1
        return gdd(idx=dd.indices(order[count[0] % 8]))

    m2 = RT.TrainableResNet50(st, device='cuda', resident=True)
    gpil = capture.CapturedRegressorStep(m2, RT.make_optimizer(m2, guarded=True), B, S)

    def replay_pil():
        count[0] += 1
        batch = [train[j] for j in order[count[0] % 8]]
        return gpil(torch.stack([b[0] for b in batch]), torch.stack([b[1] for b in batch]))

    runs = {k: [] for k in ('eager', 'resident', 'replayed', 'replayed+dd', 'PIL+replayed')}
    fns = dict({k: fn for k, (_, fn) in sides.items()}, **{'replayed+dd': replay_dd, 'PIL+replayed': replay_pil})
    for _ in range(3):                                                  # alternating runs
        for k in runs:
            runs[k].append(timed(fns[k]))
    say('  step time, median of 20 after 5 warm-up calls, three alternating runs (ms):')
    for k, v in runs.items():
        say('    %-13s %s   median %.1f ms  = %.1f images/s' % (k, ' '.join('%7.1f' % (t * 1e3) for t in v), statistics.median(v) * 1e3, B / statistics.median(v)))
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = max((max(v) - min(v)) / statistics.median(v) for v in runs.values())
    say('  largest run-to-run spread of a side: %.1f %%' % (100 * spread))
    for k in ('resident', 'replayed'):
        say('  eager / %-9s %.2fx' % (k, med['eager'] / med[k]))
    say('  PIL+replayed / replayed+dd %.2fx' % (med['PIL+replayed'] / med['replayed+dd']))
    # the repack alone
    model = sides['resident'][0]
    convs = model._convs()
    packs = [t for cv in convs for t in rr.derived_tensors(cv.fc).values()]
    byt = sum(t.numel() * 4 for t in packs) + sum(cv.weight.numel() * 4 * len(rr.derived_tensors(cv.fc)) for cv in convs)
    t = timed(model.replan)
    say('  in-place repack of the net: %d launches, %.1f MB least traffic, %.3f ms = %.0f GB/s (%.1f %% of 6.3 TB/s), %.1f us per launch' %
        (len(packs), byt / 1e6, t * 1e3, byt / t / 1e9, 100 * byt / t / HBM, t * 1e6 / len(packs)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        model.replan()
    t = timed(g.replay)
    say('  the same replayed from a graph: %.3f ms = %.0f GB/s (%.1f %% of 6.3 TB/s)' % (t * 1e3, byt / t / 1e9, 100 * byt / t / HBM))
    finish()


if __name__ == '__main__':
    main()
