"""reference graphs/pggan/transform_base.py — WalkLinearZ_free (:86-102), WalkMlpZ3 (:167-188) and the PGGAN TransformGraph (:211-640); walk
checkpoints pickle this module path (latent2im_amd/pggan.py sets ``__module__`` of both walks)."""
from latent2im_amd.pggan import PGGAN, ContentLoss, PixelTransform, TransformGraph, WalkLinearZ_free, WalkMlpZ3  # noqa: F401
