"""reference perceptual_vgg/vgg.py — ``Vgg16`` is latent2im_amd.perceptual16.Vgg16Gram (the taps exist there as pre-ReLU conv outputs feeding
the Gram kernels, not as returned feature maps)."""
from latent2im_amd.perceptual16 import Vgg16Gram as Vgg16  # noqa: F401
