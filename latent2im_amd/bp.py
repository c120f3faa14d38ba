"""Driver of the inversion (reference BP.py:29-60 flags, :286-357 data loading, saving and main), on latent2im_amd.invert.Inverter.

torchvision is not a dependency: the data pipeline of BP.py:339-350 (ImageFolder + Resize(resolution) + CenterCrop(resolution) + ToTensor +
Normalize(0.5, 0.5)) is restated on PIL, and ``save_image(nrow=1, normalize=True, range=(-1, 1))`` on numpy.  Checkpoints come from
``constants`` (g_path, vgg16_path) and ``--synthetic_weights`` asks for seeded random-init networks, as on train.py.  ``--block`` is parsed
and unused, as in the reference; the loss plot (matplotlib) is not drawn, ``loss_back.npy`` holds the curve.
"""
import argparse
import os

import numpy as np
import torch

from . import constants

IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')


def image_folder(path):
    """torchvision.datasets.ImageFolder's file list: the images of every class sub-folder, classes and files in sorted order."""
    classes = sorted(d for d in os.listdir(path) if os.path.isdir(os.path.join(path, d)))
    if not classes:
        raise FileNotFoundError('no class sub-folders in %r (the reference reads an ImageFolder: %s/<class>/<image>)' % (path, path))
    files = []
    for c in classes:
        for root, _, names in sorted(os.walk(os.path.join(path, c), followlinks=True)):
            files += [os.path.join(root, n) for n in sorted(names) if n.lower().endswith(IMG_EXTENSIONS)]
    return files


def load_image(path, resolution):
    """Resize(resolution) (shorter side, bilinear, long side int(resolution * long / short)), CenterCrop(resolution) (offsets
    int(round((size - resolution) / 2))), ToTensor (/ 255), Normalize(0.5, 0.5) -> float32 [3, resolution, resolution] in [-1, 1]."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert('RGB')
        w, h = im.size
        if (w <= h and w != resolution) or (h <= w and h != resolution):
            if w <= h:
                nw, nh = resolution, int(resolution * h / w)
            else:
                nw, nh = int(resolution * w / h), resolution
            im = im.resize((nw, nh), Image.BILINEAR)
        w, h = im.size
        top, left = int(round((h - resolution) / 2.0)), int(round((w - resolution) / 2.0))
        im = im.crop((left, top, left + resolution, top + resolution))
        a = np.asarray(im, dtype=np.uint8)
    t = torch.from_numpy(a.copy()).permute(2, 0, 1).float().div(255.0)
    return (t - 0.5) / 0.5


def save_image(t, path, pad=2):
    """torchvision.utils.save_image(t, path, nrow=1, normalize=True, range=(-1, 1)): one column of images, 2 pixels of padding."""
    from PIL import Image
    t = t.detach().float().cpu().clamp(-1, 1).add(1).div(2)
    b, c, h, w = t.shape
    grid = torch.zeros(c, b * (h + pad) + pad, w + 2 * pad)
    for i in range(b):
        grid[:, pad + i * (h + pad): pad + i * (h + pad) + h, pad:pad + w] = t[i]
    a = grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    Image.fromarray(a).save(path)


def build_parser():
    p = argparse.ArgumentParser(description='Backprop')
    p.add_argument('--latent_dim', type=int, default=512)
    p.add_argument('--batch_size', type=int, default=1)
    p.add_argument('--n-batch', type=int, default=1)
    p.add_argument('--chain-length', type=int, default=500)
    p.add_argument('--ckpt_path', type=str, default='./mnist_generator.pth')
    p.add_argument('--num_samples', type=int, default=9)
    p.add_argument('--not_use_gpu', action='store_true')
    p.add_argument('--gpu', type=str, default='0')
    p.add_argument('--n_loops', type=int, default=500)
    p.add_argument('--resolution', type=int, default=256, help='image resolution (the reference allows 128, 256, 512; any generator size here)')
    p.add_argument('--block', action='store_true', help='parsed and unused, as in the reference')
    p.add_argument('--optimizer', type=str, choices=['Adam', 'GD'], default='Adam')
    p.add_argument('--dataset', type=str, choices=['ffhq', 'scene', 'anime'])
    p.add_argument('--path', type=str)
    p.add_argument('--save_path', type=str, default='./results')
    p.add_argument('--lr', type=float, default=0.01)
    p.add_argument('--synthetic_weights', action='store_true',
                   help='run on seeded random-init G / VGG-16 when the checkpoint paths of constants.py do not exist')
    p.add_argument('--precision', type=str, choices=['f32', 'f16', 'bf16'], default='f32',
                   help='element type of the feature maps: f32, or the 16-bit h8 path with IEEE fp16 (loss-scaled; Adam only on the eager loop, Adam or GD with --hipgraph) or bf16 maps; latents and images are saved as fp32 either way')
    p.add_argument('--hipgraph', action='store_true',
                   help='replay the iteration (forward, backward, optimiser update, loss record) from one hipGraph per batch size; off: the eager loop')
    return p


def load_networks(resolution, device, precision='f32'):
    """The generator and the VGG-16 Gram network of one precision: the fp32 pair, or ('f16' / 'bf16') the 16-bit pair (conv.PRECISION is set: the
    16-bit classes and kernels16 read their element type from it)."""
    from . import conv, graph, synth, vgg16_specs
    if precision == 'f32':
        from .generator import Generator
        from .perceptual16 import Vgg16Gram
    else:
        assert precision in conv.H8_PRECISIONS, precision
        conv.PRECISION = precision
        from .nets16 import Generator
        from .perceptual16 import Vgg16Gram16 as Vgg16Gram
    if graph._checkpoint_or_synthetic('generator (g_path)', constants.g_path):
        g_state = graph._to_numpy_state(torch.load(constants.g_path, map_location='cpu')['g_ema'])
    else:
        g_state = synth.generator_state(resolution, seed=constants.SYNTH_SEED_G, noise_strength=constants.SYNTH_NOISE_STRENGTH)
    if graph._checkpoint_or_synthetic('VGG-16 (vgg16_path; the reference downloads torchvision weights)', constants.vgg16_path):
        v_state = vgg16_specs.load_vgg16_state(torch.load(constants.vgg16_path, map_location='cpu'))
    else:
        v_state = vgg16_specs.vgg16_state()
    return Generator(g_state, resolution, device=device), Vgg16Gram(v_state, device=device)


def main(argv=None):
    from . import dist
    from .invert import Inverter
    args = build_parser().parse_args(argv)
    dist.select_gpu(args.gpu)
    if args.synthetic_weights:
        constants.ALLOW_SYNTHETIC_WEIGHTS = True
    device = 'cuda'
    gen, vgg = load_networks(args.resolution, device, args.precision)
    inv = Inverter(gen, vgg, lr=args.lr, optim=args.optimizer, batch=args.batch_size, capture=args.hipgraph)
    files = image_folder(args.path)
    os.makedirs(os.path.join(args.save_path, 'latent'), exist_ok=True)
    curve = np.zeros(0)
    for i, start in enumerate(range(0, len(files), args.batch_size)):
        batch = torch.stack([load_image(f, args.resolution) for f in files[start:start + args.batch_size]])
        save_image(batch, os.path.join(args.save_path, 'org_%d.png' % i))
        w, curve = inv.invert(batch.to(device), args.n_loops)
        print('[%d / %d] loss %.3f -> %.3f' % (i + 1, -(-len(files) // args.batch_size), curve[0], curve[-1]))
        save_image(inv.last_image, os.path.join(args.save_path, '%d_final.png' % i))
        np.save(os.path.join(args.save_path, 'loss_back.npy'), curve)                 # BP.py:290: rewritten per batch, the last one stays
        np.save(os.path.join(args.save_path, 'latent', '%d_w.npy' % i), w.cpu().numpy())
    return curve
