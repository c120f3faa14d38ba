"""Gradient-map magnitudes of one 16-bit inversion iteration (invert.Inverter on nets16.Generator + perceptual16.Vgg16Gram16), the input of
nets16.invert_scale_for.  Runs on bf16 elements — fp32's exponent range, no scale applied, so the maps are seen at their true size — with the
nets16.PROBE hook, on synthetic weights, from the mean latent towards the image of a seeded W+ (the start of every inversion).  Per shape it prints
every probed map (max and median |g| as log2) and, per branch (P = VGG-16 Gram, G = generator), the largest map and the exponent that puts it at 2^5.

    python tools/probe_invert16.py [--shapes 32x1,32x8,64x1,64x8,256x1,256x8,1024x1] [--out profiles/invert16_gradient_ranges.txt]
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lg(v):
    return math.log2(v) if v > 0 else float('-inf')


def probe(size, batch, lines):
    from latent2im_amd import constants, nets16
    from latent2im_amd.bp import load_networks
    from latent2im_amd.invert import Inverter
    constants.ALLOW_SYNTHETIC_WEIGHTS = True
    gen, vgg = load_networks(size, 'cuda', 'bf16')
    inv = Inverter(gen, vgg, n_mean_latent=256, batch=batch)
    torch.manual_seed(7)
    with torch.no_grad():
        w_star = gen.style(torch.randn(batch, 512, device='cuda')).unsqueeze(1).repeat(1, gen.n_latent, 1).contiguous()
        target = gen.synthesis(w_star).clamp(-1, 1)
    grams = vgg.target_grams(target)
    w = inv.start_latent(batch).requires_grad_()
    nets16.PROBE = []
    try:
        loss, _ = inv.loss(w, target, grams)
        loss.backward()
        rows = list(nets16.PROBE)
    finally:
        nets16.PROBE = None
    lines.append('## %d^2, batch %d: loss %.4g, max |dL/dW+| 2^%.1f' % (size, batch, float(loss), lg(float(w.grad.abs().max()))))
    top = {}
    for tag, shape, mx, med, zero in rows:
        if '.fwd.' in tag:
            lines.append('  %-16s %-24s max 2^%6.1f  median 2^%6.1f   (forward map)' % (tag, 'x'.join(map(str, shape)), lg(mx), lg(med)))
            continue
        lines.append('  %-16s %-24s max 2^%6.1f  median 2^%6.1f  zeros %4.1f %%' % (tag, 'x'.join(map(str, shape)), lg(mx), lg(med), 100 * zero))
        top[tag[0]] = max(top.get(tag[0], 0.0), mx)
    for br in sorted(top):
        lines.append('  branch %s: largest gradient map 2^%.1f -> exponent %d' % (br, lg(top[br]), 5 - int(round(lg(top[br])))))
    print('\n'.join(lines[-(len(rows) + 1 + len(top)):]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='32x1,32x8,64x1,64x8,256x1,256x8,1024x1')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = ['# one inversion iteration on bf16 elements (unscaled), synthetic weights: gradient maps by nets16.PROBE; tools/probe_invert16.py',
             '# exponent = 5 - round(log2 of the branch\'s largest map): nets16.invert_scale_for']
    for item in a.shapes.split(','):
        size, batch = (int(v) for v in item.split('x'))
        probe(size, batch, lines)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
