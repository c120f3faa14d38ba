"""Parameter layout and seeded synthetic weights of the face network of eval.py's identity metric (facenet_pytorch ``InceptionResnetV1``,
reference eval.py:29-32), kept apart from specs.py / synth.py: those two files are inputs of the oracle cache's fingerprint
(tests/oracle_cache.py), and the walk-training oracle does not depend on the face network.

Pure python + numpy (no torch), like specs.py, so that the layout can be unit-tested on any box.
"""
import math
from collections import OrderedDict

import numpy as np

from .specs import _bn
from .synth import _rs


# facenet_pytorch InceptionResnetV1 (the face network of the reference's eval.py:29-32), restated from the public architecture:
# (name, cin, cout, (kh, kw), stride, (pad_y, pad_x)) of every BasicConv2d (conv without bias + BatchNorm2d(eps=1e-3) + ReLU)
FACENET_STEM = (('conv2d_1a', 3, 32, (3, 3), 2, (0, 0)), ('conv2d_2a', 32, 32, (3, 3), 1, (0, 0)), ('conv2d_2b', 32, 64, (3, 3), 1, (1, 1)),
                ('conv2d_3b', 64, 80, (1, 1), 1, (0, 0)), ('conv2d_4a', 80, 192, (3, 3), 1, (0, 0)), ('conv2d_4b', 192, 256, (3, 3), 2, (0, 0)))
# residual blocks: branches as lists of BasicConv2d (suffix, cin, cout, k, stride, pad), then the 1x1 ``conv2d`` (with bias) back to the trunk width
FACENET_BLOCKS = {
    'block35': (256, [[('branch0', 256, 32, (1, 1), 1, (0, 0))],
                      [('branch1.0', 256, 32, (1, 1), 1, (0, 0)), ('branch1.1', 32, 32, (3, 3), 1, (1, 1))],
                      [('branch2.0', 256, 32, (1, 1), 1, (0, 0)), ('branch2.1', 32, 32, (3, 3), 1, (1, 1)), ('branch2.2', 32, 32, (3, 3), 1, (1, 1))]]),
    'block17': (896, [[('branch0', 896, 128, (1, 1), 1, (0, 0))],
                      [('branch1.0', 896, 128, (1, 1), 1, (0, 0)), ('branch1.1', 128, 128, (1, 7), 1, (0, 3)), ('branch1.2', 128, 128, (7, 1), 1, (3, 0))]]),
    'block8': (1792, [[('branch0', 1792, 192, (1, 1), 1, (0, 0))],
                      [('branch1.0', 1792, 192, (1, 1), 1, (0, 0)), ('branch1.1', 192, 192, (1, 3), 1, (0, 1)), ('branch1.2', 192, 192, (3, 1), 1, (1, 0))]]),
}
# reduction blocks: conv branches, then a MaxPool2d(3, stride 2) branch of the input last
FACENET_MIXED = {
    'mixed_6a': [[('branch0', 256, 384, (3, 3), 2, (0, 0))],
                 [('branch1.0', 256, 192, (1, 1), 1, (0, 0)), ('branch1.1', 192, 192, (3, 3), 1, (1, 1)), ('branch1.2', 192, 256, (3, 3), 2, (0, 0))]],
    'mixed_7a': [[('branch0.0', 896, 256, (1, 1), 1, (0, 0)), ('branch0.1', 256, 384, (3, 3), 2, (0, 0))],
                 [('branch1.0', 896, 256, (1, 1), 1, (0, 0)), ('branch1.1', 256, 256, (3, 3), 2, (0, 0))],
                 [('branch2.0', 896, 256, (1, 1), 1, (0, 0)), ('branch2.1', 256, 256, (3, 3), 1, (1, 1)), ('branch2.2', 256, 256, (3, 3), 2, (0, 0))]],
}
# trunk order after the stem's maxpool_3a (between conv2d_2b and conv2d_3b): (prefix, kind, residual scale, final ReLU)
FACENET_TRUNK = ([('repeat_1.%d' % i, 'block35', 0.17, True) for i in range(5)] + [('mixed_6a', 'mixed', None, None)]
                 + [('repeat_2.%d' % i, 'block17', 0.10, True) for i in range(10)] + [('mixed_7a', 'mixed', None, None)]
                 + [('repeat_3.%d' % i, 'block8', 0.20, True) for i in range(5)] + [('block8', 'block8', 1.0, False)])
FACENET_EMBED = 512          # last_linear 1792 -> 512 (no bias) + last_bn (BatchNorm1d, eps 1e-3)
FACENET_BN_EPS = 1e-3
FACENET_IGNORED = ('logits.',)      # the classifier head of the checkpoint (8631 vggface2 identities): unused by the embedding


def _basic_conv(spec, prefix, cin, cout, k):
    spec[prefix + '.conv.weight'] = (cout, cin) + tuple(k)
    _bn(spec, prefix + '.bn', cout)


def facenet_spec():
    """state_dict layout of facenet_pytorch ``InceptionResnetV1(pretrained='vggface2')`` without its ``logits.*`` classifier, in
    registration order."""
    spec = OrderedDict()
    for name, cin, cout, k, _, _ in FACENET_STEM:
        _basic_conv(spec, name, cin, cout, k)
    for prefix, kind, _, _ in FACENET_TRUNK:
        if kind == 'mixed':
            branches, width = FACENET_MIXED[prefix], None
        else:
            width, branches = FACENET_BLOCKS[kind]
        for br in branches:
            for suffix, cin, cout, k, _, _ in br:
                _basic_conv(spec, prefix + '.' + suffix, cin, cout, k)
        if width is not None:
            cat = sum(br[-1][2] for br in branches)
            spec[prefix + '.conv2d.weight'] = (width, cat, 1, 1)
            spec[prefix + '.conv2d.bias'] = (width,)
    spec['last_linear.weight'] = (FACENET_EMBED, 1792)
    _bn(spec, 'last_bn', FACENET_EMBED)
    return spec


def facenet_state(seed=600):
    """name -> ndarray for facenet_pytorch ``InceptionResnetV1`` (specs.facenet_spec: no ``logits.*``).  He-normal convs (fan_in); BN
    running statistics are those a trained network would hold for O(1) activations: the mean of each conv output over inputs of mean m is
    m * sum(w) (m = 127.5 for the first conv, which reads RAW 0..255 pixels: eval.py feeds them without fixed_image_standardization;
    0.4 ~ E[relu(N(0, 1))] inside the trunk; 1 for last_bn, the pooled trunk's level), and the first conv's variance is that of
    pixels spread ~60 around mid-grey.  Without the centring every image's embedding would be dominated by one shared direction (the
    constant part of the input) and nearly parallel to every other (tests/test_facenet_gpu.py: not degenerate)."""
    out = OrderedDict()
    spec = facenet_spec()
    for name, shape in spec.items():
        r = _rs('F.' + name, seed)
        if name.endswith('num_batches_tracked'):
            out[name] = np.zeros((), dtype=np.int64)
            continue
        if name.endswith('running_var') or name.endswith('running_mean'):
            continue                                           # from the weights below
        if name.endswith('bn.weight') or name == 'last_bn.weight':
            v = r.uniform(0.8, 1.2, shape)
        elif name.endswith('bn.bias') or name == 'last_bn.bias' or name.endswith('conv2d.bias'):
            v = 0.05 * r.randn(*shape)
        elif name == 'last_linear.weight':
            v = r.randn(*shape) / math.sqrt(shape[1])
        else:                                                  # conv weights: He normal, fan_in; the residual 1x1 at half that variance
            fan_in = shape[1] * shape[2] * shape[3]
            v = r.randn(*shape) * math.sqrt((1.0 if name.endswith('conv2d.weight') else 2.0) / fan_in)
        out[name] = np.ascontiguousarray(v, dtype=np.float32).reshape(shape)
    for name in spec:
        if not name.endswith('running_mean'):
            continue
        bn = name[:-len('.running_mean')]
        w = out[bn[:-len('.bn')] + '.conv.weight' if bn.endswith('.bn') else 'last_linear.weight'].astype(np.float64)
        w = w.reshape(w.shape[0], -1)
        first = bn.startswith('conv2d_1a.')
        level = 127.5 if first else (1.0 if bn == 'last_bn' else 0.4)
        r = _rs('F.' + name, seed)
        out[name] = (level * w.sum(1) + 0.1 * r.randn(w.shape[0])).astype(np.float32)
        r = _rs('F.' + bn + '.running_var', seed)
        out[bn + '.running_var'] = (r.uniform(0.5, 1.5, w.shape[0]) * ((w * w).sum(1) * 3600.0 if first else 1.0)).astype(np.float32)
    return OrderedDict((k, out[k]) for k in spec)
