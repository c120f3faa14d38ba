"""Plain-torch model of BP.py's inversion loss, in float64 or float32 on the CPU: VGG-16 ``features[0:23]`` (perceptual_vgg/vgg.py:8-21) with
F.conv2d / F.max_pool2d, gram (BP.py:68-73), perceptual_loss (BP.py:173-184) and the total loss of one iteration (BP.py:144-152), on the oracle's
generator (oracle.sg2.generator_synthesis, imported and not modified).  tests/test_inversion_gpu.py holds latent2im_amd.perceptual16 /
latent2im_amd.invert to it."""
import torch
import torch.nn.functional as F

from latent2im_amd import vgg16_specs as V
from oracle import sg2
from oracle import step as ostep

# indices into vgg16().features: the 3x3 convs, the 2x2 max-pools (every other index below 23 is a ReLU) and the ReLUs Vgg16 taps
# (perceptual_vgg/vgg.py:8-21: slices [0:4], [4:9], [9:16], [16:23])
FEATURES_CONV = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)
FEATURES_POOL = (4, 9, 16)
FEATURES_TAP = (3, 8, 15, 22)


def vgg_state(state, dtype):
    return ostep.to_torch(state, dtype)


def vgg16_taps(PV, img):
    """The four taps relu1_2, relu2_2, relu3_3, relu4_3 of ``img`` (no normalisation: BP.py:174-175 feeds the [-1, 1] image)."""
    x, taps = img, []
    for i in range(23):                                   # torchvision vgg16().features[0:23], restated: not read from the module under test
        if i in FEATURES_CONV:
            x = F.conv2d(x, PV['%d.weight' % i], PV['%d.bias' % i], padding=1)
        elif i in FEATURES_POOL:
            x = F.max_pool2d(x, 2, 2)
        else:
            x = torch.relu(x)
        if i in FEATURES_TAP:
            taps.append(x)
    return taps


def gram(x):
    bs, ch, h, w = x.shape
    f = x.reshape(bs, ch, w * h)
    return f.bmm(f.transpose(1, 2)) / (ch * h * w)


def perceptual_loss(PV, batch, logit):
    """BP.py:173-184 -> [B]."""
    p = torch.zeros(batch.shape[0], dtype=batch.dtype)
    for gd, gl in zip([gram(t) for t in vgg16_taps(PV, batch)], [gram(t) for t in vgg16_taps(PV, logit)]):
        p = p + torch.sum((gd - gl).pow(2), [1, 2]) * (gd.shape[1] * gd.shape[2])
    return p


def total_loss(PG, PV, w, batch, noise=None):
    """BP.py:144-152: (sum((out - batch)^2, [1, 2, 3]) / (3 H W) + perceptual_loss.mean()).sum(), and the image."""
    out = sg2.generator_synthesis(PG, w, noise)
    n = batch.shape[2] * batch.shape[3] * 3
    nll = torch.sum((out - batch).pow(2), [1, 2, 3]) / n
    return (nll + perceptual_loss(PV, batch, out).mean()).sum(), out


def adam_run(PG, PV, w0, batch, noise, n_loops, lr):
    """``n_loops`` iterations of BP.py:137-158 with torch.optim.Adam(betas=(0.5, 0.9)) -> (loss curve as floats, final W+)."""
    w = w0.detach().clone().requires_grad_()
    opt = torch.optim.Adam([w], lr=lr, betas=(0.5, 0.9))
    curve = []
    for _ in range(n_loops):
        loss, _ = total_loss(PG, PV, w, batch, noise)
        opt.zero_grad()
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    return curve, w.detach()
