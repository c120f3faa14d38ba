"""Writes tests/golden/regtrain16_emulation.npz: what 16-bit STORAGE alone does to the regressor training step, measured on the CPU.

The emulation is oracle/nets.py's resnet50_train_forward restated in float64 torch with three additions, and nothing of any kernel:
  store     a straight-through rounding to the element type (fp16 or bf16, round to nearest even) of the value on the way forward and of the
            gradient on the way back, at every point where the GPU path (regressor_train.TrainableResNet50H8) stores an h8 map: every conv output,
            every BatchNorm output, every block output; the two gradient maps a downsample block stores before it adds them round on the way back;
  weights   the conv weights are rounded on the way forward, the gradient reaches the master unrounded (the image is NOT rounded, although
            conv.ImgConvH8 rounds it inside the kernel: it is no stored map; with it rounded too the fp16 losses come out 0.078609 0.049711 0.036842,
            the first within 4e-7 of float64 by the accident of one signed sum, and the gradient figures move in their third digit);
  scale     the gradient entering the maps is multiplied by 2^e (regressor_train.regtrain_scale_for for fp16, 0 for bf16) and the parameter
            gradients behind them are divided by it; the fc, the loss and Adam(1e-4) stay float64.
Inputs: tests/test_regressor_graph_gpu.py's `ref` fixture (RandomState(5), synth.resnet50_state(seed=300), data 8 x 3 x 128 x 128 randn * 0.5, labels
rand).  Per element type the file holds the emulation's relative L2 deviation from the float64 oracle gradient for each of the 161 parameters,
the aggregate relative L2 and cosine over all gradients concatenated, and the losses of three Adam steps; plus the float64 losses.

    python tests/golden/make_regtrain16.py            # rewrites the file (a few minutes of CPU)

tests/test_regtrain16_ref_cpu.py re-runs step 1 for fp16 through `emulate` and checks the file against it; tests/test_regtrain16_gpu.py takes its
bars from the file."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'regtrain16_emulation.npz')
RESNET50_LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))
DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16}
SHAPE = (8, 128)              # batch, image side


def inputs():
    """(state, data, label) of test_regressor_graph_gpu's `ref` fixture."""
    from latent2im_amd import synth
    rs = np.random.RandomState(5)
    st = synth.resnet50_state(seed=300)
    data = torch.from_numpy(rs.randn(8, 3, 128, 128).astype(np.float32) * 0.5)
    label = torch.from_numpy(rs.rand(8, 40).astype(np.float32))
    return st, data, label


def _rounders(dtype):
    rnd = lambda t: t.to(dtype).to(torch.float64)

    class Store(torch.autograd.Function):             # value forward, gradient backward
        @staticmethod
        def forward(ctx, t):
            return rnd(t)

        @staticmethod
        def backward(ctx, g):
            return rnd(g)

    class Fwd(torch.autograd.Function):               # weights: value forward only
        @staticmethod
        def forward(ctx, t):
            return rnd(t)

        @staticmethod
        def backward(ctx, g):
            return g

    class Bwd(torch.autograd.Function):               # a gradient map stored on its own
        @staticmethod
        def forward(ctx, t):
            return t.clone()

        @staticmethod
        def backward(ctx, g):
            return rnd(g)

    class Scale(torch.autograd.Function):             # the loss scale: the gradient below is multiplied by s
        @staticmethod
        def forward(ctx, t, s):
            ctx.s = s
            return t.clone()

        @staticmethod
        def backward(ctx, g):
            return g * ctx.s, None
    return Store.apply, Fwd.apply, Bwd.apply, Scale.apply


def block16(P, x, p, s, down, rounders, running=True, momentum=0.1):
    """One bottleneck block ``p`` ('layer2.0') of stride ``s`` with the stores (``rounders`` = _rounders(dtype)), ``down``: with a downsample branch.
    ``running`` False: ``P`` holds no running statistics (tests/test_regtrain16_block_gpu.py runs single blocks through this)."""
    store, wr, gstore, _ = rounders

    def bn(prefix, t):
        return F.batch_norm(t, P[prefix + '.running_mean'] if running else None, P[prefix + '.running_var'] if running else None,
                            P[prefix + '.weight'], P[prefix + '.bias'], training=True, momentum=momentum, eps=1e-5)
    conv = lambda t, name, **kw: store(F.conv2d(t, wr(P[name]), **kw))
    idt = x
    xin = gstore(x) if down else x                               # a downsample block stores conv1's input gradient before it adds the other branch
    o = store(F.relu(bn(p + '.bn1', conv(xin, p + '.conv1.weight'))))
    o = store(F.relu(bn(p + '.bn2', conv(o, p + '.conv2.weight', stride=s, padding=1))))
    o = conv(o, p + '.conv3.weight')
    if down:
        xd = gstore(x) if s == 2 else x                          # stride 2: the compact gradient is stored too, then zero-inserted and added
        idt = store(bn(p + '.downsample.1', conv(xd, p + '.downsample.0.weight', stride=s)))
    return store(F.relu(bn(p + '.bn3', o) + idt))


def forward16(P, x, dtype, scale, momentum=0.1):
    """resnet50_train_forward with the stores; the parameter gradients below the head come out multiplied by ``scale``."""
    rounders = _rounders(dtype)
    store, wr, _, scaled = rounders
    x = store(F.conv2d(x, wr(P['conv1.weight']), stride=2, padding=3))
    x = store(F.relu(F.batch_norm(x, P['bn1.running_mean'], P['bn1.running_var'], P['bn1.weight'], P['bn1.bias'], training=True, momentum=momentum, eps=1e-5)))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, (planes, blocks, stride) in enumerate(RESNET50_LAYERS):
        for b in range(blocks):
            x = block16(P, x, 'layer%d.%d' % (li + 1, b), stride if b == 0 else 1, b == 0, rounders, momentum=momentum)
    x = scaled(F.adaptive_avg_pool2d(x, 1).flatten(1), scale)
    return F.linear(x, P['fc.weight'], P['fc.bias'])


def emulate(state, data, label, elem, log2_scale, steps=1, lr=1e-4):
    """(losses [steps], gradients of step 1 by name) of the 16-bit emulation, float64."""
    from oracle import step as ostep
    P = {k: v.clone() for k, v in ostep.to_torch(state, torch.float64).items()}
    names = [k for k, v in P.items() if v.dtype.is_floating_point and not k.endswith('running_mean') and not k.endswith('running_var')]
    for k in names:
        P[k].requires_grad_(True)
    opt = torch.optim.Adam([P[k] for k in names], lr=lr)
    scale = float(2.0 ** log2_scale)
    losses, first = [], None
    for _ in range(steps):
        preds = forward16(P, data.double(), DTYPES[elem], scale)
        opt.zero_grad()
        loss = F.mse_loss(preds, label.double()).mean()
        loss.backward()
        for k in names:
            if not k.startswith('fc.'):
                P[k].grad.div_(scale)
        if first is None:
            first = {k: P[k].grad.detach().clone() for k in names}
        opt.step()
        losses.append(float(loss.detach()))
    return losses, first


def deviations(grads, g64):
    """(names, per-parameter relative L2, aggregate relative L2, aggregate cosine) of ``grads`` against the float64 oracle gradient."""
    names = list(g64)
    rel = np.array([float((grads[k].double() - g64[k]).norm() / (g64[k].norm() + 1e-300)) for k in names])
    a = torch.cat([grads[k].double().reshape(-1) for k in names])
    b = torch.cat([g64[k].reshape(-1) for k in names])
    return names, rel, float((a - b).norm() / b.norm()), float(torch.dot(a, b) / (a.norm() * b.norm()))


def oracle64(state, data, label, steps):
    from oracle import nets as onets
    from oracle import step as ostep
    P = {k: v.clone() for k, v in ostep.to_torch(state, torch.float64).items()}
    _, g = onets.resnet50_train_step(P, data.double(), label.double(), lr=1e-4, steps=1)
    P = {k: v.clone() for k, v in ostep.to_torch(state, torch.float64).items()}
    lo, _ = onets.resnet50_train_step(P, data.double(), label.double(), lr=1e-4, steps=steps)
    return [float(x) for x in lo], g


def static_log2(elem):
    from latent2im_amd.regressor_train import regtrain_scale_for
    return regtrain_scale_for(SHAPE[1], SHAPE[0]) if elem == 'f16' else 0


def main():
    torch.manual_seed(0)
    state, data, label = inputs()
    loss64, g64 = oracle64(state, data, label, 3)
    out = dict(loss_f64=np.array(loss64))
    for elem in ('f16', 'bf16'):
        e = static_log2(elem)
        losses, grads = emulate(state, data, label, elem, e, steps=3)
        names, rel, agg, cos = deviations(grads, g64)
        per_cos = np.array([float(torch.dot(grads[k].double().reshape(-1), g64[k].reshape(-1)) / (grads[k].double().norm() * g64[k].norm() + 1e-300)) for k in names])
        print('%s e=%d: per-parameter cosine min / median %.3f / %.3f, relative L2 max / median %.3f / %.3f, aggregate L2 %.4f cosine %.4f, losses %s (float64 %s)'
              % (elem, e, per_cos.min(), np.median(per_cos), rel.max(), np.median(rel), agg, cos, ' '.join('%.6f' % v for v in losses), ' '.join('%.6f' % v for v in loss64)))
        out.update({elem + '_rel_l2': rel.astype(np.float32), elem + '_agg_l2': np.float64(agg), elem + '_agg_cos': np.float64(cos), elem + '_losses': np.array(losses),
                    elem + '_log2_scale': np.int64(e)})
    out['names'] = np.array(names)
    np.savez_compressed(PATH, **out)
    print('wrote %s (%d bytes)' % (PATH, os.path.getsize(PATH)))


if __name__ == '__main__':
    main()
