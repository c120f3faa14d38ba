"""Evidence that a host-side change moved nothing: the recorded and eager steps of a built checkout, dumped so that two checkouts can be compared.

    python tools/probes/step_evidence.py dump TREE OUTDIR        library-call names in order (_lib.call and conv._launch hooked, as
                                                                 tests/test_pggan_graph_gpu.py::_counting does) of one eager step and one recording of
                                                                 the 64^2 batch-2 StyleGAN2 step and the 256^2 batch-2 PGGAN step in fp32 and f16 and of
                                                                 one recorded inversion at 32^2 -> OUTDIR/calls.json; loss, x1 and the walk of three
                                                                 fp32 replays of each from fixed seeds -> OUTDIR/bits.pt
    python tools/probes/step_evidence.py compare A A2 B          A, A2: two dumps of the parent, B: this checkout's -> the report
    python tools/probes/step_evidence.py time TREE TAG           the eager fp16 MLP-walk step of tools/bench_pggan.py (256^2, batch 4): three runs

TREE is the root of a built checkout (this one or the parent commit's); ``dump`` and ``time`` import that tree's package, one process a tree.
profiles/walk_graph_refactor.txt is this tool's output."""
import json
import os
import sys


def _enter(tree):
    tree = os.path.abspath(tree)
    os.chdir(tree)
    sys.path[:0] = [tree, os.path.join(tree, 'tools')]
    import latent2im_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(latent2im_amd.__file__))) == tree, latent2im_amd.__file__
    return tree


def dump(tree, outdir):
    outdir = os.path.abspath(outdir)
    tree = _enter(tree)
    os.makedirs(outdir, exist_ok=True)
    import numpy as np
    import torch
    from latent2im_amd import _lib, capture, constants, conv, selfcheck, synth, trainer
    from latent2im_amd import pggan as pg
    from latent2im_amd import vgg16_specs as V
    from latent2im_amd.generator import Generator
    from latent2im_amd.invert import Inverter
    from latent2im_amd.perceptual16 import Vgg16Gram
    dev = torch.device('cuda', torch.cuda.current_device())
    seen = [None]
    real_call, real_launch = _lib.call, conv._launch

    def call(name, *a, **k):
        if seen[0] is not None:
            seen[0].append(name)
        return real_call(name, *a, **k)

    def launch(*a, **k):
        if seen[0] is not None:
            seen[0].append('conv launch')
        return real_launch(*a, **k)
    _lib.call, conv._launch = call, launch

    def listed(fn):
        seen[0] = []
        try:
            r = fn()
            torch.cuda.synchronize()
        finally:
            out, seen[0] = seen[0], None
        return out, r

    def sg2_graph():
        torch.manual_seed(0)
        return selfcheck.build_graph(64, ['Smiling'], 2, lr=1e-3)

    def pg_graph(nets, walk_type='NNz'):
        np.random.seed(81)
        g = pg.faceGraph(lr=1e-3, walk_type=walk_type, loss='l2', trainEmbed=False, attrList=['Smiling'], attrTable={'Smiling': 31}, layers=None,
                         pgan_opts=None, nets=nets)
        if walk_type != 'linear':
            with torch.no_grad():
                for p in g.walk.parameters():
                    p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(81 + p.numel())).to(p.device) * 0.02)
        if g.loss_scaler is not None:                                        # the scaler travels with the shared networks
            g.loss_scaler.state.zero_()
            g.loss_scaler.scale.fill_(1.0)
        return g

    def keep(loss, x1, walk, **more):
        return dict(loss=torch.as_tensor(loss).detach().cpu().clone(), x1=x1.detach().cpu().clone(), walk=walk.detach().cpu().clone(), **more)

    calls, bits = {}, {}
    zs = [synth.z_sample(2, seed=40 + i) for i in range(3)]
    al_w = [np.full((2, 1), v) for v in (0.19, 0.6, 0.35)]
    al_z = [np.full((2, 1), v) for v in (0.3, -0.2, 0.5)]
    flat = lambda g: torch.cat([p.detach().reshape(-1) for p in g.walk.parameters()])
    for dt in ('f32', 'f16'):
        conv.PRECISION = dt
        g = sg2_graph()
        calls['sg2 %s eager' % dt], _ = listed(lambda: selfcheck.run_step(g, zs[0], al_w[0]))
        g = sg2_graph()
        torch.manual_seed(1)
        calls['sg2 %s recording' % dt], step = listed(lambda: capture.CapturedStep(g, 2, 1))
        if dt == 'f32':
            for i in range(3):
                r = step(zs[i], al_w[i])
                torch.cuda.synchronize()
                bits['sg2 step %d' % i] = keep(r['loss'], r['x1'], g.walk.w)
        constants.ALLOW_SYNTHETIC_WEIGHTS, constants.BATCH_SIZE = True, 2
        nets = pg.load_networks(dev)
        g = pg_graph(nets)
        calls['pggan %s eager' % dt], _ = listed(lambda: pg.walk_training_step(g, zs[0], al_z[0], no_content_loss=False))
        g = pg_graph(nets)
        calls['pggan %s recording' % dt], step = listed(lambda: capture.CapturedZStep(g, 2, 1))
        if dt == 'f32':
            for i in range(3):
                r = step(zs[i], al_z[i])
                torch.cuda.synchronize()
                bits['pggan step %d' % i] = keep(r['loss'], r['x1'], flat(g))
            g = pg_graph(nets, 'linear')                                     # the driver's --hip_graph route, alpha from the global numpy RNG
            opt = type('O', (), dict(hip_graph=True, no_content_loss=False, no_gan_loss=True))()
            np.random.seed(9)
            for i in range(3):
                loss, at, x0, x1 = trainer.train_step(g, zs[i], ['Smiling'], opt=opt)
                torch.cuda.synchronize()
                bits['pggan train_step %d' % i] = keep(loss, x1, g.walk.w, alpha=torch.as_tensor(np.asarray(at)))
        del g, step, nets
        torch.cuda.empty_cache()
    conv.PRECISION = 'f32'
    size = 32
    rs = np.random.RandomState(21 + size)
    nl = 2 * int(np.log2(size)) - 2
    noise = [torch.from_numpy(rs.randn(1, 1, 4 << ((li + 1) // 2), 4 << ((li + 1) // 2))).float().to(dev) for li in range(nl - 1)]
    target = torch.from_numpy(rs.uniform(-1, 1, (1, 3, size, size))).float().to(dev)
    w0 = torch.from_numpy(0.3 * rs.randn(1, nl, 512)).float().to(dev)
    inv = Inverter(Generator(synth.generator_state(size, seed=100, noise_strength=0.5), size, device=dev), Vgg16Gram(V.vgg16_state(), device=dev), lr=0.01,
                   optim='Adam', n_mean_latent=64, batch=1, capture=True)
    calls['inversion f32 recording + 3 replays'], (w, curve) = listed(lambda: inv.invert(target, 3, noise=noise, w=w0))
    bits['inversion'] = keep(curve, inv.last_image, w)
    with open(os.path.join(outdir, 'calls.json'), 'w') as f:
        json.dump(calls, f)
    torch.save(bits, os.path.join(outdir, 'bits.pt'))
    print('dumped', tree, {k: len(v) for k, v in calls.items()}, flush=True)


def compare(pa, pb, ch):
    import torch
    ca, cc = (json.load(open(os.path.join(d, 'calls.json'))) for d in (pa, ch))
    ba, bb, bc = (torch.load(os.path.join(d, 'bits.pt')) for d in (pa, pb, ch))
    ok = True
    print('## library-call sequences (names in order): parent against this commit')
    for k in ca:
        same = ca[k] == cc.get(k)
        ok &= same
        print('%-40s parent %4d calls   this commit %4d calls   %s' % (k, len(ca[k]), len(cc.get(k, [])), 'identical, name by name' if same else 'DIFFERENT'))
    print()
    print('## fp32 replays, three steps from the same seeds: torch.equal(parent, this commit), and the parent against a second run of itself')
    for k in ba:
        for name in ba[k]:
            a, b, c = ba[k][name], bb[k][name], bc[k][name]
            eq, self_eq = torch.equal(a, c), torch.equal(a, b)
            d, ds, ref = float((a.double() - c.double()).abs().max()), float((a.double() - b.double()).abs().max()), float(a.double().abs().max())
            bar = {'loss': 1e-6 + 1e-5 * ref, 'x1': 1e-5 + 1e-4 * ref}.get(name, 1e-3 * ref)      # the capture tests' fp32 bars, where the parent differs from itself
            ok &= eq or (not self_eq and d <= bar)
            print('%-24s %-6s %-18s bit-identical %-5s (parent twice: %-5s)   max|d| %.3e (parent twice %.3e) of %.3e' % (k, name, tuple(a.shape), eq, self_eq, d, ds, ref))
    print()
    print('RESULT', 'nothing moved' if ok else 'SOMETHING MOVED')
    return 0 if ok else 1


def time_step(tree, tag):
    _enter(tree)
    import torch
    import bench_pggan as B
    from latent2im_amd import conv, synth
    from latent2im_amd import pggan as pg
    g = B._graph('f16', 4, 'NNz')
    z = torch.Tensor(synth.z_sample(4, seed=0)).cuda()
    ad = torch.full((4, 1), 0.3, device='cuda')
    conv.PRECISION = 'f16'
    step = lambda: pg.walk_training_step(g, z, ad, no_content_loss=False)
    runs = [B.timed(step) for _ in range(3)]
    print('%-8s f16  step 256^2  batch 4  content on  walk NNz  eager  runs %s ms   %d library calls'
          % (tag, ' '.join('%.3f' % (1e3 * v) for v in runs), B.count_calls(step)), flush=True)


if __name__ == '__main__':
    sys.exit({'dump': dump, 'compare': compare, 'time': time_step}[sys.argv[1]](*sys.argv[2:]))
