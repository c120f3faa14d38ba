"""vis_w.py --given_w: a W+ saved by BP.py goes through the graph's ``given_w`` argument instead of a sampled z."""
import os

import numpy as np
import pytest
import torch

from latent2im_amd import synth

DEV = 'cuda'


@pytest.mark.gpu
def test_vis_w_given_w_writes_the_latents_own_image(tmp_path):
    """train.py (one epoch at 32^2, synthetic weights) leaves opt.yml and a walk; vis_w.py --given_w on a directory of two ``*_w.npy`` writes
    one strip per file.  A panel shows G(w + (alpha - alpha_org) * walk): with the walk set to zero every panel, the alpha = 0 one included, is
    the generator's own image of the saved latent; with the trained walk the strip is what the graph's apply_alpha makes of that latent."""
    from PIL import Image
    from latent2im_amd import constants, selfcheck, trainer, vis
    from latent2im_amd.generator import Generator
    models = str(tmp_path / 'models')
    argv = ['--model', 'stylegan_v2_real', '--transform', 'face', '--num_samples', '4', '--learning_rate', '1e-3', '--latent', 'w',
            '--walk_type', 'linear', '--loss', 'l2', '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt',
            '--models_dir', models, '--overwrite_config', '--resolution', '32', '--batch_size', '4', '--n_epoch', '1', '--seed', '3',
            '--model_save_freq', '1', '--synthetic_weights']
    before = (os.getcwd(), constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS)
    os.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        trainer.main(multi_attr=False, argv=argv)
        out = os.path.join(models, 'stylegan_v2_real_face_linear_lr0.001_l2_w')
        ck = os.path.join(out, 'model_w_1_final_walk_module.ckpt')
        walk = torch.load(ck, map_location='cpu', weights_only=False)
        with torch.no_grad():
            walk.w.zero_()
        ck0 = os.path.join(out, 'model_w_0_zero_walk_module.ckpt')
        torch.save(walk, ck0)

        r = np.random.RandomState(8)
        lat = tmp_path / 'latent'
        lat.mkdir()
        ws = [(0.5 * r.randn(1, 8, 512)).astype(np.float32) for _ in range(2)]                    # what BP.py writes: [1, n_latent, 512]
        for i, w in enumerate(ws):
            np.save(str(lat / ('%d_w.npy' % i)), w)
        gen = Generator(synth.generator_state(32, seed=constants.SYNTH_SEED_G), 32, device=DEV)
        with torch.no_grad():
            own = gen.synthesis(torch.from_numpy(np.concatenate(ws, 0)).to(DEV)).cpu().numpy()
        own = np.uint8(np.clip((own + 1) / 2.0 * 255, 0, 255)).transpose(0, 2, 3, 1)           # graph.clip_ims, [2, 32, 32, 3]

        common = [os.path.join(out, 'opt.yml'), '--num_samples', '7', '--num_panels', '3', '--noise_seed', '1']
        written = vis.main(common + ['--save_path_w', ck0, '--given_w', str(lat), '--output_dir', str(tmp_path / 'zero')])
        assert len(written) == 2                                                                  # --num_samples became the number of files
        for i, path in enumerate(written):
            strip = np.asarray(Image.open(path))
            assert strip.shape == (32, 96, 3)
            for p in range(3):
                assert np.array_equal(strip[:, 32 * p:32 * p + 32], own[i]), (i, p)

        one = vis.main(common + ['--save_path_w', ck, '--given_w', str(lat / '1_w.npy'), '--output_dir', str(tmp_path / 'one')])
        assert len(one) == 1
        strip = np.asarray(Image.open(one[0])).astype(np.int64)
        assert strip.shape == (32, 96, 3)
        gr = selfcheck.build_graph(32, ['Smiling'], 4)
        trained = torch.load(ck, map_location='cpu', weights_only=False)
        with torch.no_grad():
            gr.walk.w.copy_(trained.w.to(gr.device))
        w1 = torch.from_numpy(ws[1]).to(DEV)
        layers_w = [w1[:, i].contiguous() for i in range(8)]
        panels = []
        for p, alpha in enumerate(np.linspace(0, 1, 3)):                                          # --min_alpha 0 --max_alpha 1, three panels
            img, _, img0 = gr.apply_alpha({'z': torch.zeros(1, 512)}, np.full((1, 1), alpha), given_w=layers_w)
            want = gr.clip_ims(img.cpu().numpy())[0].transpose(1, 2, 0).astype(np.int64)
            panels.append(want)
            assert np.abs(strip[:, 32 * p:32 * p + 32] - want).max() <= 1, p                      # 8-bit levels: the same arithmetic, two graphs
            got0 = gr.clip_ims(img0.cpu().numpy())[0].transpose(1, 2, 0).astype(np.int64)
            assert np.abs(got0 - own[1].astype(np.int64)).max() <= 1                              # the unedited image is the latent's own
        assert (panels[0] != panels[2]).any()                                                     # the trained walk does edit
    finally:
        os.chdir(before[0])
        constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS = before[1:]
