"""Inference on trained walks: graph.apply_alpha_combine (several attributes at once), graph.sweep (every panel from one pass over the
original), the two-attribute grid writer, the new flags of vis.py / evaluate.py and make_samples on the device.  Synthetic weights, generator
noise strength 0: the same latent gives the same image, so "the same launches" is checked bit for bit on the fp32 images."""
import os

import numpy as np
import pytest
import torch

from tests import panels_ref as pr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTRS = ['Smiling', 'Young']
B, P = 2, 3


def _restore(saved):
    from latent2im_amd import constants, conv
    os.chdir(saved[0])
    constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS, conv.PRECISION = saved[1:]


def _save():
    from latent2im_amd import constants, conv
    return (os.getcwd(), constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS, conv.PRECISION)


def _graph(resolution, precision='f32'):
    from latent2im_amd import conv, selfcheck
    conv.PRECISION = precision
    return selfcheck.build_graph(resolution, ATTRS, B)


def _inputs(g, seed=11):
    r = np.random.RandomState(seed)
    z = r.randn(B, 512).astype(np.float32)
    alphas = [a * np.ones((B, g.Nsliders)) for a in np.linspace(0, 1, P)]
    return {'z': z}, alphas


def _check_sweep_equals_the_single_calls(g):
    """sweep with chunk = B against apply_alpha (index_ None and an int) and apply_alpha_combine (a list), bit for bit."""
    inputs, alphas = _inputs(g)
    smiling, young = g.attrTable['Smiling'], g.attrTable['Young']
    for index_ in (None, young):
        panels, a_org, out_zs = g.sweep(inputs, alphas, index_=index_, chunk=B)
        assert tuple(panels.shape) == (P, B, 3, g.img_size, g.img_size) and panels.dtype == torch.float32 and panels.is_cuda
        for p, ag in enumerate(alphas):
            img, a1, org = g.apply_alpha({'z': torch.Tensor(inputs['z']).to(g.device)}, ag, index_=index_)
            assert torch.equal(panels[p], img.float()), (index_, p)
            assert torch.equal(a_org, a1) and torch.equal(out_zs, org.float())
        assert not torch.equal(panels[0], panels[P - 1])                       # the walk does edit
    pairs = [[a1, a2] for a1 in alphas for a2 in alphas]
    panels, a_org, out_zs = g.sweep(inputs, pairs, index_=[smiling, young])    # chunk defaults to B
    assert panels.shape[0] == P * P
    for p, pair in enumerate(pairs):
        img, a1, org = g.apply_alpha_combine({'z': torch.Tensor(inputs['z']).to(g.device)}, pair, index_=[smiling, young])
        assert torch.equal(panels[p], img.float()), p
        assert torch.equal(a_org, a1) and torch.equal(out_zs, org.float())
    return inputs, alphas, pairs, panels


def test_sweep_is_the_single_calls_bit_for_bit_and_chunks_within_one_level():
    saved = _save()
    try:
        g = _graph(32)
        inputs, alphas, pairs, panels = _check_sweep_equals_the_single_calls(g)
        # another launch shape (3 images a generator call, the last call ragged): the same arithmetic, within one 8-bit level
        chunked, _, _ = g.sweep(inputs, pairs, index_=[g.attrTable['Smiling'], g.attrTable['Young']], chunk=3)
        a, b = g.clip_ims(panels.cpu().numpy()).astype(np.int64), g.clip_ims(chunked.cpu().numpy()).astype(np.int64)
        print('chunk=3 against chunk=B: largest difference %d levels' % np.abs(a - b).max())
        assert np.abs(a - b).max() <= 1
        with pytest.raises(ValueError):
            g.sweep(inputs, alphas, chunk=0)
    finally:
        _restore(saved)


@pytest.mark.parametrize('precision', ('f16', 'bf16'))
def test_sweep_is_the_single_calls_bit_for_bit_on_the_16_bit_path(precision):
    saved = _save()
    try:
        _check_sweep_equals_the_single_calls(_graph(64, precision))
    finally:
        _restore(saved)


def test_apply_alpha_combine_is_the_reference_delta():
    saved = _save()
    try:
        g = _graph(32)
        inputs, alphas = _inputs(g, seed=12)
        smiling, young = g.attrTable['Smiling'], g.attrTable['Young']
        z = torch.Tensor(inputs['z']).to(g.device)
        ag = [0.9 * np.ones((B, 1)), 0.2 * np.ones((B, 1))]
        with torch.no_grad():                                                  # the reference's statement on the graph's own pieces
            w = g.get_w(z)
            org = g.get_logits({'w': w})
            a_org = g.get_reg_preds(org)
            delta = torch.zeros_like(a_org)
            for k, col in enumerate((0, 1)):                                   # Smiling, Young are walk columns 0, 1
                delta[:, col] = torch.Tensor(ag[k][:, 0]).to(g.device) - a_org[:, col]
            want = g.get_logits({'w': g.walk(w, alpha=delta, layers=None)})
        got, a1, org1 = g.apply_alpha_combine({'z': z}, ag, index_=[smiling, young])
        assert torch.equal(got, want) and torch.equal(a1, a_org) and torch.equal(org1, org)
        assert not torch.equal(got, org)
        # the order of index_ pairs targets with attributes, not with columns
        swapped, _, _ = g.apply_alpha_combine({'z': z}, [ag[1], ag[0]], index_=[young, smiling])
        assert torch.equal(swapped, want)
        # moving only Smiling leaves Young's delta at zero: the result is the walk applied to that delta
        with torch.no_grad():
            d1 = torch.zeros_like(a_org)
            d1[:, 0] = torch.Tensor(ag[0][:, 0]).to(g.device) - a_org[:, 0]
            assert g._combine_delta(a_org, [ag[0]], [smiling])[:, 1].abs().max().item() == 0
            assert torch.equal(g._combine_delta(a_org, [ag[0]], [smiling]), d1)
            want1 = g.get_logits({'w': g.walk(w, alpha=d1, layers=None)})
        only, _, _ = g.apply_alpha_combine({'z': z}, [ag[0]], index_=[smiling])
        assert torch.equal(only, want1) and not torch.equal(only, want)
        # a zeroed walk: every tile is the original
        with torch.no_grad():
            g.walk.w.zero_()
        same, _, org2 = g.apply_alpha_combine({'z': z}, ag, index_=[smiling, young])
        assert torch.equal(same, org2) and torch.equal(org2, org)
    finally:
        _restore(saved)


def test_combine_writer_files_gutters_and_tiles(tmp_path):
    from PIL import Image
    saved = _save()
    try:
        g = _graph(32)
        inputs, alphas = _inputs(g, seed=13)
        idx = [g.attrTable['Smiling'], g.attrTable['Young']]
        R = 32
        written = g.vis_multi_image_batch_alphas_combine(inputs, str(tmp_path / 'w_1'), alphas, list(np.linspace(0, 1, P)), batch_start=4, index_=idx)
        names = sorted(os.path.relpath(w, str(tmp_path)) for w in written)
        want_names = sorted(['w_1_idx%d_idx%d_sample%d.png' % (idx[0], idx[1], 4 + i) for i in range(B)]
                            + [os.path.join('org_img', 'w_1_idx%d_idx%d_sample%d_org.png' % (idx[0], idx[1], 4 + i)) for i in range(B)])
        assert names == want_names and all(os.path.isfile(w) for w in written)
        pairs = [[a1, a2] for a1 in alphas for a2 in alphas]
        panels, _, out_zs = g.sweep(inputs, pairs, index_=idx)
        panels, out_zs = panels.cpu().numpy(), out_zs.cpu().numpy()
        side = P * (R + 1) - 1
        for i in range(B):
            grid = np.asarray(Image.open(str(tmp_path / ('w_1_idx%d_idx%d_sample%d.png' % (idx[0], idx[1], 4 + i)))))
            assert grid.shape == (side, side, 3)
            for k in range(1, P):                                              # imgrid's white gutters
                assert (grid[k * (R + 1) - 1] == 255).all() and (grid[:, k * (R + 1) - 1] == 255).all()
            for r in range(P):                                                 # row: Smiling's alpha, column: Young's
                for c in range(P):
                    tile = grid[r * (R + 1):r * (R + 1) + R, c * (R + 1):c * (R + 1) + R]
                    assert np.array_equal(tile, pr.clip_ims(panels[r * P + c, i]).transpose(1, 2, 0)), (i, r, c)
            org = np.asarray(Image.open(str(tmp_path / 'org_img' / ('w_1_idx%d_idx%d_sample%d_org.png' % (idx[0], idx[1], 4 + i)))))
            assert np.array_equal(org, pr.clip_ims(out_zs[i]).transpose(1, 2, 0))
        with pytest.raises(ValueError):
            g.vis_multi_image_batch_alphas_combine(inputs, str(tmp_path / 'w_1'), alphas, None, batch_start=0, index_=[idx[0]])
    finally:
        _restore(saved)


def test_make_samples_on_the_device_writes_the_host_paths_png(tmp_path):
    from PIL import Image
    from latent2im_amd import trainer
    (tmp_path / 'results').mkdir()
    x = np.random.RandomState(2).uniform(-1.2, 1.2, size=(5, 3, 8, 8)).astype(np.float32)
    x.reshape(-1)[:778] = pr.quant_inputs()
    trainer.make_samples(torch.as_tensor(x).to(DEV), str(tmp_path), 0, 10, 5, name='dev')
    got = np.asarray(Image.open(str(tmp_path / 'results' / '0_10_dev.png')))
    with np.errstate(over='ignore'):                                                      # (+-3e38 are among the boundary values)
        img = np.uint8(np.clip(((x + 1) / 2.0) * 255, 0, 255)).transpose(0, 2, 3, 1)      # the host path's formula: cols = floor(sqrt(5)) = 2
    want = np.zeros((3 * 8, 2 * 8, 3), np.uint8)
    for i in range(5):
        r, c = divmod(i, 2)
        want[r * 8:(r + 1) * 8, c * 8:(c + 1) * 8] = img[i]
    assert got.shape == want.shape and np.array_equal(got, want)
    with np.errstate(over='ignore'):
        trainer.make_samples(torch.as_tensor(x), str(tmp_path), 0, 10, 5, name='host')       # a CPU tensor keeps the host path
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'results' / '0_10_host.png'))), want)


def _train(tmp_path_factory, resolution):
    from latent2im_amd import trainer
    models = str(tmp_path_factory.mktemp('models%d' % resolution))
    argv = ['--model', 'stylegan_v2_real', '--transform', 'face', '--num_samples', '4', '--learning_rate', '1e-3', '--latent', 'w',
            '--walk_type', 'linear', '--loss', 'l2', '--attrList', ','.join(ATTRS), '--attrPath', './dataset/attributes_celeba.txt',
            '--models_dir', models, '--overwrite_config', '--resolution', str(resolution), '--batch_size', '4', '--n_epoch', '1', '--seed', '3',
            '--model_save_freq', '1', '--synthetic_weights']
    saved = _save()
    os.chdir(ROOT)
    try:
        trainer.main(multi_attr=False, argv=argv)
    finally:
        _restore(saved)
    out = os.path.join(models, 'stylegan_v2_real_face_linear_lr0.001_l2_w')
    return os.path.join(out, 'opt.yml'), os.path.join(out, 'model_w_1_final_walk_module.ckpt')


@pytest.fixture(scope='module')
def trained32(tmp_path_factory):
    return _train(tmp_path_factory, 32)


@pytest.fixture(scope='module')
def trained64(tmp_path_factory):
    return _train(tmp_path_factory, 64)


def _vis(trained, tmp_path, sub, extra, samples=2, panels=3):
    from latent2im_amd import conv, vis
    yml, ck = trained
    saved = _save()
    os.chdir(ROOT)
    try:
        conv.PRECISION = 'f32'
        written = vis.main([yml, '--save_path_w', ck, '--num_samples', str(samples), '--num_panels', str(panels), '--noise_seed', '1',
                            '--output_dir', str(tmp_path / sub)] + extra)
        assert conv.PRECISION == 'f32'                                          # restored, whatever the flag asked for
        return written
    finally:
        _restore(saved)


def test_vis_flags_write_files_and_the_plain_invocation_is_unchanged(trained32, tmp_path):
    from PIL import Image
    plain = _vis(trained32, tmp_path, 'plain', [])
    assert len(plain) == 2
    strips = [np.asarray(Image.open(p)) for p in plain]
    assert all(s.shape == (32, 96, 3) for s in strips)
    # the device path with every attribute pinned to the same alpha (--pad 0 is the only flag) writes the same strips under the same names
    dev = _vis(trained32, tmp_path, 'dev', ['--pad', '0'])
    assert [os.path.basename(p) for p in dev] == [os.path.basename(p) for p in plain]
    for a, p in zip(strips, dev):
        assert np.array_equal(a, np.asarray(Image.open(p)))
    attr = _vis(trained32, tmp_path, 'attr', ['--attr', 'Young', '--pad', '2'])
    assert len(attr) == 2 and all('_Young_' in os.path.basename(p) for p in attr)
    moved = [np.asarray(Image.open(p)) for p in attr]
    assert all(m.shape == (32, 3 * 34 - 2, 3) for m in moved)
    assert all((m[:, 32:34] == 255).all() and (m[:, 66:68] == 255).all() for m in moved)
    assert any((m[:, 68:100] != s[:, 64:96]).any() for m, s in zip(moved, strips))          # only Young moves: another edit than all at once
    comb = _vis(trained32, tmp_path, 'comb', ['--combine', 'Smiling,Young'])
    assert len(comb) == 4 and all(os.path.isfile(p) for p in comb)
    grids = [p for p in comb if os.path.basename(os.path.dirname(p)) != 'org_img']
    assert len(grids) == 2 and all(np.asarray(Image.open(p)).shape == (3 * 33 - 1, 3 * 33 - 1, 3) for p in grids)
    assert os.path.isfile(str(tmp_path / 'comb' / 'index.html'))
    for bad in ('Smiling,Male', 'Smiling', 'Smiling,Smiling'):
        with pytest.raises(SystemExit):
            _vis(trained32, tmp_path, 'bad', ['--combine', bad])
    with pytest.raises(SystemExit):
        _vis(trained32, tmp_path, 'bad', ['--attr', 'Male'])


def test_vis_and_evaluate_on_the_16_bit_path(trained64, tmp_path):
    from PIL import Image
    from latent2im_amd import conv, evaluate
    f16 = _vis(trained64, tmp_path, 'f16', ['--precision', 'f16'])
    assert len(f16) == 2 and all(np.asarray(Image.open(p)).shape == (64, 192, 3) for p in f16)
    trained = _vis(trained64, tmp_path, 'train', ['--precision', 'train'], samples=1)       # opt.yml recorded no precision: f32
    assert len(trained) == 1
    yml, ck = trained64
    res = {}
    for precision in ('f32', 'f16'):
        saved = _save()
        os.chdir(ROOT)
        try:
            conv.PRECISION = 'f32'
            res[precision] = evaluate.main([yml, '--save_path_w', ck, '--num_samples', '2', '--num_panels', '2', '--identity', 'off',
                                            '--output_dir', str(tmp_path / ('eval_' + precision)), '--precision', precision])
            assert conv.PRECISION == 'f32'
        finally:
            _restore(saved)
    assert set(res['f16']) == set(res['f32']) and res['f16']['index_'] == res['f32']['index_']
    assert len(res['f16']['bucket_sizes']) == 3
