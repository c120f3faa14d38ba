"""latent2im_amd.bp.load_image against a float64 restatement of the four transforms of BP.py:339-350: Resize(resolution) (shorter side, bilinear,
antialiased as PIL does it), CenterCrop(resolution), ToTensor, Normalize(0.5, 0.5)."""
import numpy as np
import pytest


def _triangle_matrix(n_in, n_out):
    """[n_out, n_in] weights of a bilinear resize with the filter's support widened by the scale when shrinking: output pixel i is centred at
    (i + 0.5) * n_in / n_out, input pixel x at x + 0.5, weight max(0, 1 - |distance| / max(scale, 1)), rows normalised."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    centre = (np.arange(n_out, dtype=np.float64)[:, None] + 0.5) * scale
    w = np.maximum(0.0, 1.0 - np.abs(np.arange(n_in, dtype=np.float64)[None, :] + 0.5 - centre) / fs)
    return w / w.sum(1, keepdims=True)


def _load_ref(a, resolution):
    """``a`` uint8 [H, W, 3] -> float64 [3, resolution, resolution], without any intermediate rounding."""
    h, w = a.shape[:2]
    x = a.astype(np.float64)
    if not ((w <= h and w == resolution) or (h <= w and h == resolution)):
        nw, nh = (resolution, int(resolution * h / w)) if w <= h else (int(resolution * w / h), resolution)
        x = np.einsum('ow,hwc->hoc', _triangle_matrix(w, nw), x)
        x = np.einsum('oh,hwc->owc', _triangle_matrix(h, nh), x)
        h, w = nh, nw
    top, left = int(round((h - resolution) / 2.0)), int(round((w - resolution) / 2.0))
    x = x[top:top + resolution, left:left + resolution]
    return ((x / 255.0 - 0.5) / 0.5).transpose(2, 0, 1)


# (width, height, resolution): landscape and portrait shrunk, enlarged, and the crop-only case
@pytest.mark.parametrize('w,h,res', [(48, 40, 32), (40, 48, 32), (20, 28, 32), (48, 40, 40), (33, 33, 32)])
def test_load_image_vs_float64_transforms(tmp_path, w, h, res):
    """The loader's resize rounds to 8 bits after its horizontal pass (half a level) and after its vertical pass, which is a convex combination
    of the first pass's values (their half level stays a half level) plus its own rounding: one level of 2 / 255 at the most, none of which the
    restatement shares.  1e-5 covers the resize's 22-bit fixed-point weights and the float32 division.  Crop-only inputs agree to float32."""
    from PIL import Image
    from latent2im_amd import bp
    r = np.random.RandomState(w * 100 + h)
    a = (r.rand(h, w, 3) * 255).astype(np.uint8)
    path = str(tmp_path / 'im.png')
    Image.fromarray(a).save(path)
    got = bp.load_image(path, res)
    ref = _load_ref(a, res)
    assert tuple(got.shape) == (3, res, res) == ref.shape
    err = float(np.abs(got.double().numpy() - ref).max())
    print('load_image %dx%d -> %d: max deviation %.3e (one level is %.3e)' % (w, h, res, err, 2 / 255))
    if min(w, h) == res:
        assert err <= 1e-6
    else:
        assert err <= 2 / 255 + 1e-5
