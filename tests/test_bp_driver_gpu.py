"""BP.py's driver end to end on a temporary image folder (synthetic weights), and the host-side file conventions it shares with vis_w.py."""
import os

import numpy as np
import pytest


def _folder(tmp_path, n=3):
    from PIL import Image
    root = tmp_path / 'data'
    (root / 'faces').mkdir(parents=True)
    r = np.random.RandomState(3)
    for i in range(n):
        Image.fromarray((r.rand(40, 48, 3) * 255).astype(np.uint8)).save(str(root / 'faces' / ('im%d.png' % i)))      # 48 wide, 40 high
    return str(root)


@pytest.mark.gpu
def test_bp_main_writes_its_files(tmp_path):
    from latent2im_amd import bp, constants
    out = str(tmp_path / 'results')
    before = constants.ALLOW_SYNTHETIC_WEIGHTS
    try:
        curve = bp.main(['--resolution', '32', '--n_loops', '3', '--synthetic_weights', '--path', _folder(tmp_path), '--save_path', out,
                         '--batch_size', '1', '--optimizer', 'Adam', '--dataset', 'ffhq'])
    finally:
        constants.ALLOW_SYNTHETIC_WEIGHTS = before
    assert curve.shape == (3,) and np.isfinite(curve).all()
    n_latent = 2 * 5 - 2
    for i in range(3):
        assert os.path.isfile(os.path.join(out, 'org_%d.png' % i)) and os.path.isfile(os.path.join(out, '%d_final.png' % i))
        assert np.load(os.path.join(out, 'latent', '%d_w.npy' % i)).shape == (1, n_latent, 512)
    assert np.load(os.path.join(out, 'loss_back.npy')).shape == (3,)


def test_image_folder_and_loader_geometry(tmp_path):
    """Class sub-folders in sorted order; the shorter side is resized to the resolution and the centre is cropped; values in [-1, 1]."""
    from PIL import Image
    from latent2im_amd import bp
    root = _folder(tmp_path)
    files = bp.image_folder(root)
    assert [os.path.basename(f) for f in files] == ['im0.png', 'im1.png', 'im2.png']
    t = bp.load_image(files[0], 32)
    assert tuple(t.shape) == (3, 32, 32) and float(t.min()) >= -1.0 and float(t.max()) <= 1.0
    with Image.open(files[0]) as im:                       # 48 x 40 -> 38 x 32 (int(32 * 48 / 40)) -> columns 3 .. 34
        ref = np.asarray(im.convert('RGB').resize((38, 32), Image.BILINEAR), dtype=np.float64)[:, 3:35]
    np.testing.assert_allclose(t.permute(1, 2, 0).double().numpy(), (ref / 255.0 - 0.5) / 0.5, atol=1e-6)
    with pytest.raises(FileNotFoundError):
        bp.image_folder(os.path.join(root, 'faces'))
    same = bp.load_image(files[0], 40)                    # the shorter side already has the resolution: crop only
    with Image.open(files[0]) as im:
        np.testing.assert_allclose(same.permute(1, 2, 0).double().numpy(), (np.asarray(im, dtype=np.float64)[:, 4:44] / 255.0 - 0.5) / 0.5, atol=1e-6)
