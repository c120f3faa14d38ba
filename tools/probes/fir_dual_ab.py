"""The discriminator-backward FIR launches that gained a second output (l2i_upfirdn2d_dual_f32), with and without it, at the c3 step's shapes (batch 8,
size 1024): the FIR that ends block bi's backward produces the gradient of block bi - 1 — the zero-insertion kernel behind the compact skip path
(maps >= 192), the staged 4x4 kernel below.  Two alternating repetitions each (single, dual, single, dual), median of 5 timings of 3 launches.
GB moved = what the launch has to read and write once; the dual launch adds one mask read and one write of the output size."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from latent2im_amd import kernels as K, synth

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
# (channels of g, output size, compact): the five levels whose consumer is >= 32 wide
LEVELS = [(64, 512, True), (128, 256, True), (256, 128, False), (512, 64, False), (512, 32, False)]


def timed(fn, n=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 3)
    return float(np.median(ts))


kf = torch.tensor(synth.fir_kernel(), device='cuda')
print('batch %d; ms per launch, repetitions in the order run: single, dual, single, dual' % B, flush=True)
tot = [0.0, 0.0]
for c, h, compact in LEVELS:
    x = torch.randn(B, c, h // 2 if compact else h, h // 2 if compact else h, device='cuda')
    addend, mask2 = torch.randn(B, c, h, h, device='cuda'), torch.randn(B, c, h, h, device='cuda')
    y, y2 = torch.empty_like(addend), torch.empty_like(addend)
    kw = dict(up=(2, 2), pad=(2, 1, 2, 1)) if compact else dict(pad=(2, 1, 2, 1))
    single = lambda: K.upfirdn2d(x, kf, addend=addend, out=y, **kw)
    dual = lambda: K.upfirdn2d(x, kf, addend=addend, out=y, mask2=mask2, mask2_vals=(1.0, 0.2), out2=y2, **kw)
    t = [timed(f) for f in (single, dual, single, dual)]
    gb1 = (x.numel() + 2 * y.numel()) * 4 / 1e9
    gb2 = gb1 + 2 * y.numel() * 4 / 1e9
    tot[0] += min(t[0], t[2])
    tot[1] += min(t[1], t[3])
    print('%4d ch @%-4d %-6s single %.4f %.4f ms (%.2f GB, %.2f TB/s)  dual %.4f %.4f ms (%.2f GB, %.2f TB/s)  added %.4f ms' % (
        c, h, 'up2k4' if compact else 'k4', t[0], t[2], gb1, gb1 / min(t[0], t[2]), t[1], t[3], gb2, gb2 / min(t[1], t[3]),
        min(t[1], t[3]) - min(t[0], t[2])), flush=True)
print('sum of the faster repetitions: single %.4f ms, dual %.4f ms, added %.4f ms' % (tot[0], tot[1], tot[1] - tot[0]))
