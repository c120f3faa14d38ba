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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--only', choices=('eager', 'resident', 'replayed'))
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

    def make(side):
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
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
