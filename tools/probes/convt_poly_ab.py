"""Stride-2 transposed 3x3 conv, fp32: the direct kernel (tile_hint 9: convt_mfma_kernel, its automatic tile) against the 25-product kernel (tile_hint 10:
convt_poly_kernel) on the transposed shapes of the c3 step at batch 8 — the generator's up layers (forward form: in_scale, out_scale, outputs padded
by 3) and the input gradients of the stride-2 convs of the discriminator (pad 0, masked, outputs padded by 3) and of ResNet-50 (pad 1, masked, and
'plain': unmasked, the mask applied by the launch that produces the gradient).  The
two kernels are interleaved in one process, two alternating repetitions each (A B A B), so the spread between repetitions of one kernel stands beside
the difference between the kernels.  ms per launch and TFLOP/s of the dense form (2 B Cout Cin 9 H W).  This file fixes kPolyRules
(csrc/l2i_convt_poly.hip): a shape enters the table only where both repetitions of the new kernel beat both of the direct kernel."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from latent2im_amd import _lib, conv

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
SHAPES = [  # cin, cout, res, pad, masked, extra
    (512, 512, 32, 0, False, 3), (512, 256, 64, 0, False, 3), (256, 128, 128, 0, False, 3), (128, 64, 256, 0, False, 3), (64, 32, 512, 0, False, 3),
    (512, 512, 32, 0, True, 3), (512, 256, 64, 0, True, 3), (256, 128, 128, 0, True, 3), (128, 64, 256, 0, True, 3), (64, 32, 512, 0, True, 3),
    (128, 128, 64, 1, True, 1), (256, 256, 32, 1, True, 1), (128, 128, 128, 1, True, 1), (256, 256, 64, 1, True, 1), (512, 512, 32, 1, True, 1),
    (128, 128, 128, 1, None, 1), (256, 256, 64, 1, None, 1), (512, 512, 32, 1, None, 1),          # None: no prologue or epilogue operand at all
]


def timed(fn, n):
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


print('batch %d; ms per launch (TFLOP/s dense), repetitions in the order run: direct, poly, direct, poly' % B, flush=True)
for cin, cout, res, pad, masked, extra in SHAPES:
    w = torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5
    fc = conv.FrozenConv2d(w, 2, pad, transposed=True, device='cuda')
    x = torch.randn(B, cin, res, res, device='cuda')
    oh, ow = fc.out_hw(res, res)
    y = torch.empty(B, cout, oh + extra, ow + extra, device='cuda')
    if masked is None:
        kw = {}
    elif masked:
        kw = dict(in_mask=torch.randn(B, cin, res, res, device='cuda'), mask=(1.0, 0.2))
    else:
        kw = dict(in_scale=torch.rand(B, cin, device='cuda') + 0.5, out_scale=torch.rand(B, cout, device='cuda') + 0.5)
    run = lambda hint: fc.forward(x, out=y, tile_hint=hint, **kw)
    run(_lib.CONVT_HINT_DIRECT)
    y0 = y.clone()
    run(_lib.CONVT_HINT_POLY)
    dev = float((y - y0).abs().max()) / float(y0.abs().max())
    t = [timed(lambda: run(h), 5) for h in (_lib.CONVT_HINT_DIRECT, _lib.CONVT_HINT_POLY, _lib.CONVT_HINT_DIRECT, _lib.CONVT_HINT_POLY)]
    fl = 2.0 * B * cout * cin * 9 * res * res
    wins = max(t[1], t[3]) < min(t[0], t[2])
    print('%4d->%-4d @%-4d pad %d %-8s direct %.4f %.4f ms (%.0f TF)  poly %.4f %.4f ms (%.0f TF)  poly/direct %.3f  %s  max dev %.1e' % (
        cin, cout, res, pad, 'plain' if masked is None else ('masked' if masked else 'forward'), t[0], t[2], fl / min(t[0], t[2]) / 1e9, t[1], t[3], fl / min(t[1], t[3]) / 1e9,
        (t[1] + t[3]) / (t[0] + t[2]), 'POLY' if wins else 'direct', dev), flush=True)
