"""Inference driver: load a trained walk and sweep alpha over ``num_panels`` values (reference vis_w.py:21-118,
options/vis_options.py).  Forward-only reuse of the training kernels.

A plain invocation writes one strip per sample through graph.vis_multi_image_batch_alphas, as ever.  ``--precision`` (the 16-bit networks a
walk was trained on), ``--attr`` (one attribute of a multi-attribute walk), ``--combine A,B`` (the two-attribute grid of the reference's
vis_multi_image_batch_alphas_combine) and ``--pad`` take the device path instead: graph.sweep (the original image and its regressor pass once
per batch, not once per panel) and one l2i_panels_u8 launch that quantises and lays out every panel, so the host receives finished uint8."""
import argparse
import os

import yaml

from . import constants, dist, hostutil


class VisOptions:
    def __init__(self):
        self.initialized = False
        self.parser = argparse.ArgumentParser('Visualization Parser')

    def initialize(self):
        p = self.parser
        p.add_argument('config_file', type=argparse.FileType(mode='r'), help='configuration yml file (opt.yml of the training run)')
        p.add_argument('--save_path_w', type=str)
        p.add_argument('--save_path_gan', type=str)
        p.add_argument('--gpu', default='', type=str)
        p.add_argument('--noise_seed', type=int, default=0, help='noise seed for z samples')
        p.add_argument('--output_dir', help='where to save output; overrides output_dir of the config file')
        p.add_argument('--attrList', type=str)
        p.add_argument('--attrPath', type=str, default='')
        self.initialized = True
        return p

    def parse(self, argv=None):
        if not self.initialized:
            self.initialize()
        opt = self.parser.parse_args(argv)
        data = yaml.load(opt.config_file, Loader=yaml.FullLoader)
        for k, v in data.items():
            if isinstance(v, dict):
                data[k] = argparse.Namespace(**v)
        self.opt, self.data = opt, argparse.Namespace(**data)
        return self.opt, self.data


def load_given_w(path, device):
    """One ``*_w.npy`` of BP.py ([B, n_latent, 512]) or a directory of them (sorted) -> one [N, n_latent, 512] tensor."""
    import numpy as np
    import torch
    files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith('_w.npy')) if os.path.isdir(path) else [path]
    if not files:
        raise FileNotFoundError('no *_w.npy in %r' % path)
    return torch.from_numpy(np.concatenate([np.load(f).astype(np.float32) for f in files], 0)).to(device)


PRECISIONS = ('f32', 'f16', 'bf16', 'train')


def add_precision_flag(parser):
    parser.add_argument('--precision', type=str, default=None, choices=PRECISIONS,
                        help='the networks to run the walk on: f32 (what runs without the flag), the 16-bit path f16 / bf16, or train = what the '
                             'training run recorded in its opt.yml')


def resolve_precision(flag, conf):
    """--precision against the training run's opt.yml: 'train' is the value recorded there (f32 when it recorded none); no flag leaves
    conv.PRECISION as the process has it."""
    from . import conv
    if flag is None:
        return conv.PRECISION
    return (getattr(conf, 'precision', None) or 'f32') if flag == 'train' else flag


def attr_index(name, conf, what):
    """The attribute-table index of ``name``, which must be one of the walk's own attributes (opt.yml attrList)."""
    own = [a for a in (conf.attrList or '').strip().split(',') if a]
    if name not in own:
        raise SystemExit('%s: %r is not an attribute of this walk (attrList: %s)' % (what, name, ','.join(own)))
    return hostutil.set_graph_kwargs(conf)['attrTable'][name]


def main(argv=None):
    from . import conv
    v = VisOptions()
    v.initialize()
    v.parser.add_argument('--num_samples', type=int, default=10)
    v.parser.add_argument('--num_panels', type=int, default=7)
    v.parser.add_argument('--max_alpha', type=float, default=1)
    v.parser.add_argument('--min_alpha', type=float, default=0)
    v.parser.add_argument('--layers', type=str, default=None)
    v.parser.add_argument('--trainEmbed', action='store_true')
    v.parser.add_argument('--updateGAN', action='store_true')
    v.parser.add_argument('--given_w', type=str, default=None,
                          help='a *_w.npy written by BP.py, or a directory of them: edit these inverted images instead of sampled ones '
                               '(--num_samples becomes the number of files)')
    add_precision_flag(v.parser)
    v.parser.add_argument('--attr', type=str, default=None, help='move only this attribute of a multi-attribute walk')
    v.parser.add_argument('--combine', type=str, default=None,
                          help='A,B: one num_panels x num_panels grid per sample, rows follow A and columns follow B (two attributes of the walk)')
    v.parser.add_argument('--pad', type=int, default=None, help='gutter in pixels between panels (white); default 0 for strips, 1 for --combine')
    opt, conf = v.parse(argv)
    device_path = opt.precision is not None or opt.attr is not None or opt.combine is not None or opt.pad is not None
    if opt.attr is not None and opt.combine is not None:
        raise SystemExit('--attr and --combine are two ways to choose attributes: give one')
    if opt.pad is not None and opt.pad < 0:
        raise SystemExit('--pad must be >= 0')
    index_ = None
    if opt.attr is not None:
        index_ = [attr_index(opt.attr, conf, '--attr')]          # a list: the other attributes keep a zero delta (graph.vis_sweep_strips)
    if opt.combine is not None:
        pair = [a.strip() for a in opt.combine.split(',')]
        if len(pair) != 2 or pair[0] == pair[1]:
            raise SystemExit('--combine takes two different attributes A,B (got %r)' % opt.combine)
        index_ = [attr_index(a, conf, '--combine') for a in pair]
    dist.select_gpu(opt.gpu)                         # before the first torch.cuda call (vis_w.py / eval.py set CUDA_VISIBLE_DEVICES)
    dist.init_from_env()
    if getattr(conf, 'synthetic_weights', False):    # the training run's explicit choice travels in its opt.yml
        constants.ALLOW_SYNTHETIC_WEIGHTS = True
    if getattr(conf, 'resolution', None):
        constants.resolution = conf.resolution
    if getattr(conf, 'batch_size', None):
        constants.BATCH_SIZE = conf.batch_size
    output_dir = opt.output_dir if opt.output_dir else os.path.join(conf.output_dir, 'images')
    os.makedirs(output_dir, exist_ok=True)
    saved = conv.PRECISION
    conv.PRECISION = resolve_precision(opt.precision, conf)       # before the graph is built: load_networks picks the network classes by it
    try:
        return _write_sweeps(opt, conf, output_dir, index_, device_path)
    finally:
        conv.PRECISION = saved


def _write_sweeps(opt, conf, output_dir, index_, device_path):
    """main's work under the precision it set: build the graph, load the walk, write every batch's files; returns the written paths."""
    from . import graph as graph_mod
    g = graph_mod.find_model_using_name(conf.model, conf.transform)(**hostutil.set_graph_kwargs(conf))
    if device_path and not hasattr(g, 'sweep'):
        raise SystemExit('--precision / --attr / --combine / --pad sweep the StyleGAN2 graph; the %s graph has no sweep' % conf.model)
    g.load_multi_models(opt.save_path_w, None, trainEmbed=opt.trainEmbed, updateGAN=opt.updateGAN)
    given = None
    if opt.given_w:
        given = load_given_w(opt.given_w, g.device)
        opt.num_samples = given.shape[0]
    graph_inputs = hostutil.graph_input(g, opt.num_samples, seed=opt.noise_seed)
    epochs = opt.save_path_w.split('/')[-1].split('_')[2]
    filename = os.path.join(output_dir, 'w_{}_seed{}'.format(epochs, opt.noise_seed))
    name = opt.attr or conf.attrList.strip().split(',')[0]
    layers = None if opt.layers in (None, 'None') else [int(i) for i in opt.layers.split(',')]
    bs = constants.BATCH_SIZE
    written = []
    for batch_start in range(0, opt.num_samples, bs):
        s = slice(batch_start, min(opt.num_samples, batch_start + bs))
        batch = hostutil.batch_input(graph_inputs, s)
        new_filename = filename + '_{}_max{}_min{}'.format(name, opt.max_alpha, opt.min_alpha)
        # the per-layer list get_w returns, of this batch's saved latents
        given_w = None if given is None else [given[s][:, i].contiguous() for i in range(given.shape[1])]
        ag, at = g.vis_image_batch(batch, new_filename, s.start, num_panels=opt.num_panels, max_alpha=opt.max_alpha,
                                   min_alpha=opt.min_alpha, wgt=True)
        if opt.combine is not None:
            written += g.vis_multi_image_batch_alphas_combine(batch, filename + '_max{}_min{}'.format(opt.max_alpha, opt.min_alpha), alphas_to_graph=ag,
                                                              alphas_to_target=at, batch_start=s.start, layers=layers, name=name,
                                                              given_w=given_w, index_=index_, pad=1 if opt.pad is None else opt.pad)
        elif device_path:
            written += g.vis_sweep_strips(batch, new_filename, alphas_to_graph=ag, alphas_to_target=at, batch_start=s.start, layers=layers,
                                          name=name, given_w=given_w, index_=index_, pad=opt.pad or 0)
        else:
            written += g.vis_multi_image_batch_alphas(batch, new_filename, alphas_to_graph=ag, alphas_to_target=at, layers=layers,
                                                      batch_start=s.start, name=name, wgt=False, wmask=False, trainEmbed=opt.trainEmbed,
                                                      computeL2=False, given_w=given_w)
    with open(os.path.join(output_dir, 'index.html'), 'w') as f:      # utils/html.make_html
        f.write('<html><body>' + ''.join('<p>%s<br><img src="%s"></p>' % (os.path.basename(w), os.path.relpath(w, output_dir)) for w in written)
                + '</body></html>')
    return written
