"""Layer table, state-dict layout and seeded synthetic weights of the VGG-16 prefix behind BP.py's Gram loss (torchvision
``vgg16().features[0:23]``, reference perceptual_vgg/vgg.py:8-21), kept apart from specs.py / synth.py as face_specs.py is: those two files are
inputs of the oracle cache's fingerprint (tests/oracle_cache.py), and the walk-training oracle does not depend on this network.

Pure python + numpy (no torch), so that the layout can be unit-tested on any box.
"""
import math
from collections import OrderedDict

import numpy as np

from .synth import _rs

# features[0:23]: ('conv', features index, cin, cout) = Conv2d(3x3, stride 1, pad 1) + ReLU, ('pool',) = MaxPool2d(2, 2), ('tap',) = an output of
# Vgg16.forward (relu1_2, relu2_2, relu3_3, relu4_3: perceptual_vgg/vgg.py:14-21, 27-37)
VGG16_LAYERS = (('conv', 0, 3, 64), ('conv', 2, 64, 64), ('tap',), ('pool',),
                ('conv', 5, 64, 128), ('conv', 7, 128, 128), ('tap',), ('pool',),
                ('conv', 10, 128, 256), ('conv', 12, 256, 256), ('conv', 14, 256, 256), ('tap',), ('pool',),
                ('conv', 17, 256, 512), ('conv', 19, 512, 512), ('conv', 21, 512, 512), ('tap',))
VGG16_CONVS = tuple(l[1:] for l in VGG16_LAYERS if l[0] == 'conv')       # (features index, cin, cout)
VGG16_IGNORED = ('classifier.',)          # the ImageNet head of the checkpoint, unused by the features
VGG16_FEATURES_LEN = 31                   # torchvision's vgg16().features: convs beyond index 21 (24, 26, 28) exist in a checkpoint and are unused


def vgg16_spec():
    """name -> shape of the parameters the prefix reads, in registration order, named as in the prefix itself (``N.weight`` / ``N.bias``)."""
    spec = OrderedDict()
    for idx, cin, cout in VGG16_CONVS:
        spec['%d.weight' % idx] = (cout, cin, 3, 3)
        spec['%d.bias' % idx] = (cout,)
    return spec


def vgg16_state(seed=700):
    """Seeded synthetic weights: He-normal convs (std sqrt(2 / fan_in), torchvision's own initialisation of VGG) and biases of 0.05 N(0, 1).  With
    a ReLU between them He-normal layers hand the second moment on unchanged, so the pre-ReLU level of every layer is about sqrt(2) times the
    RMS of the [-1, 1] image, with a lift after each max-pool.  Measured on a uniform [-1, 1] 64 x 64 image (RMS 0.58), pre-ReLU standard
    deviation / fraction of active ReLUs at the four taps: see VGG16_SYNTH_LEVELS below."""
    out = OrderedDict()
    for name, shape in vgg16_spec().items():
        r = _rs('V16.' + name, seed)
        if name.endswith('bias'):
            v = 0.05 * r.randn(*shape)
        else:
            v = r.randn(*shape) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


# (tap, pre-ReLU standard deviation, fraction of active ReLUs) of vgg16_state() on a seeded uniform [-1, 1] 64 x 64 image: O(1), about half active
VGG16_SYNTH_LEVELS = (('relu1_2', 0.75, 0.49), ('relu2_2', 1.13, 0.49), ('relu3_3', 1.33, 0.49), ('relu4_3', 1.41, 0.51))


def load_vgg16_state(sd):
    """A torchvision ``vgg16`` state dict (``features.N.weight`` / ``features.N.bias``, ``classifier.*`` ignored) or one of its ``features``
    alone (``N.weight``) -> the prefix's own ``N.weight`` / ``N.bias`` dict.  The key layout and every shape are checked: a VGG-19 or a
    batch-norm VGG file is refused by name."""
    keys = [k for k in sd if not k.startswith(VGG16_IGNORED)]
    prefixed = [k.startswith('features.') for k in keys]
    if any(prefixed) and not all(prefixed):
        raise KeyError('VGG-16 state dict: unexpected keys %s' % sorted(k for k, p in zip(keys, prefixed) if not p)[:4])
    strip = len('features.') if keys and prefixed[0] else 0
    have = {k[strip:]: sd[k] for k in keys}
    spec = vgg16_spec()
    missing = [k for k in spec if k not in have]
    if missing:
        raise KeyError('VGG-16 state dict: missing %s' % missing[:4])
    allowed = set(spec) | {'%d.%s' % (i, p) for i in (24, 26, 28) for p in ('weight', 'bias')}
    extra = sorted(set(have) - allowed)
    if extra:
        raise KeyError('VGG-16 state dict: unexpected keys %s (vgg16().features has convs at 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)' % extra[:4])
    out = OrderedDict()
    for name, shape in spec.items():
        a = np.asarray(have[name].detach().cpu().numpy() if hasattr(have[name], 'detach') else have[name], dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError('VGG-16 state dict: %s has shape %s, expected %s' % (name, tuple(a.shape), tuple(shape)))
        out[name] = np.ascontiguousarray(a)
    return out
