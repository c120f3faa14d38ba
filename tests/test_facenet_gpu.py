"""The identity-preservation half of eval.py on the MI355X: the device resize against PIL, the HIP face network against the float64 CPU
restatement (tests/facenet_ref.py), its checkpoint path, and evaluate.main(--identity on) end to end."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from latent2im_amd import _lib, constants, face_specs, facenet, kernels
from tests import facenet_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _images(n, size, seed):
    """Unrelated fp32 images in [-1, 1]: smooth random fields with their own brightness, contrast and colour, plus a little noise."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        base = torch.tensor(rs.randn(1, 3, 8, 8))
        up = F.interpolate(base, size=(size, size), mode='bicubic', align_corners=False)[0].numpy()
        out.append(rs.uniform(-0.5, 0.5) + rs.uniform(0.2, 0.8) * up + 0.1 * rs.randn(3, size, size))
    return np.stack(out).astype(np.float32)


@pytest.fixture(scope='module')
def state():
    return face_specs.facenet_state(seed=constants.SYNTH_SEED_F)


@pytest.fixture(scope='module')
def net(state):
    return facenet.InceptionResnetV1(state, device=DEV)


@pytest.mark.parametrize('n', (1024, 256, 64, 32))
def test_resize_bit_identical(n):
    rs = np.random.RandomState(n)
    x = rs.uniform(-1.2, 1.2, (3, 3, n, n)).astype(np.float32)
    x[:, :, : n // 4] = 1.2                       # saturated, flat and exactly-representable edges of clip_ims
    x[:, :, n // 4: n // 3] = -1.0
    x[1, 0, :, : n // 5] = np.float32(0.0039215689)
    got = facenet.face_input(torch.from_numpy(x).to(DEV)).cpu().numpy()
    want = R.face_input(x)
    assert got.shape == (3, 3, 160, 160)
    np.testing.assert_array_equal(got, want)
    try:
        from PIL import Image
    except ImportError:
        return
    q = R.clip_ims(x)
    pil = np.stack([np.asarray(Image.fromarray(im.transpose(1, 2, 0)).resize((160, 160))).transpose(2, 0, 1) for im in q]).astype(np.float32)
    np.testing.assert_array_equal(got, pil)


def test_resize_equal_size_is_a_copy():
    x = np.random.RandomState(1).uniform(-1.2, 1.2, (2, 3, 160, 160)).astype(np.float32)
    got = facenet.face_input(torch.from_numpy(x).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(got, R.clip_ims(x).astype(np.float32))


def test_embeddings_vs_float64(state, net, monkeypatch):
    """Batch 5 at 160^2 against the float64 restatement; bound max(2 x the fp32 restatement's own deviation, 1e-4)."""
    x = R.face_input(_images(5, 160, 3))
    want = R.embed(state, x, torch.float64)
    dev32 = (R.embed(state, x, torch.float32).double() - want).abs().max().item()

    def refuse(*a, **k):
        raise AssertionError('torch.nn.functional.conv2d on the identity path')
    monkeypatch.setattr(F, 'conv2d', refuse)
    monkeypatch.setattr(torch, 'conv2d', refuse)
    got = net.embed(torch.from_numpy(x).to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    err = (got.double().cpu() - want).abs().max().item()
    bound = max(2 * dev32, 1e-4)
    print('facenet embeddings: max |gpu - float64| %.3g, fp32 restatement %.3g, bound %.3g' % (err, dev32, bound))
    assert got.shape == (5, 512)
    assert err <= bound
    np.testing.assert_allclose(got.norm(dim=1).cpu().numpy(), 1.0, atol=1e-5)


def test_pair_distances_are_scipys(state, net):
    ims = torch.from_numpy(_images(6, 64, 4)).to(DEV)
    d, emb = net.pair_distances(ims[:3], ims[3:])
    assert d.dtype == torch.float64 and d.shape == (3,)
    e = emb.double().cpu().numpy()
    want = [R.cosine(e[i], e[i + 3]) for i in range(3)]
    np.testing.assert_allclose(d.cpu().numpy(), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(emb.cpu().numpy(), net.embed(facenet.face_input(ims)).cpu().numpy(), rtol=0, atol=1e-6)


def test_not_degenerate(net):
    """Over 8 unrelated images the embeddings stay apart: the metric can tell images apart on the synthetic weights."""
    e = net.embed(facenet.face_input(torch.from_numpy(_images(8, 64, 5)).to(DEV))).double()
    c = (e @ e.t()).cpu().numpy()
    np.fill_diagonal(c, -1.0)
    print('largest pairwise cosine of 8 unrelated images: %.4f' % c.max())
    assert c.max() < 0.99


def test_checkpoint_file(state, net, tmp_path):
    """A facenet_pytorch-format file (plain state_dict with logits.* and num_batches_tracked) gives the embeddings of the same weights handed
    over directly."""
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in state.items()}
    sd['logits.weight'] = torch.randn(8631, 512)
    sd['logits.bias'] = torch.zeros(8631)
    path = str(tmp_path / '20180402-114759-vggface2.pt')
    torch.save(sd, path)
    loaded, src = facenet.load(path, device=DEV)
    assert src == path
    x = facenet.face_input(torch.from_numpy(_images(3, 64, 6)).to(DEV))
    assert torch.equal(loaded.embed(x), net.embed(x))


def test_refusals():
    lib = _lib.load()
    x = torch.zeros(64, device=DEV)
    i = torch.zeros(64, device=DEV, dtype=torch.int32)
    p, q = _lib.ptr(x), _lib.ptr(i)
    s = _lib.stream_ptr()
    E_UNSUPPORTED = -3
    assert lib.l2i_face_resize_f32(p, p, 3, 1024, 1024, 320, 320, q, q, 27, q, q, 27, s) == E_UNSUPPORTED       # output > 256
    assert lib.l2i_face_resize_f32(p, p, 3, 4096, 4096, 160, 160, q, q, 103, q, q, 103, s) == E_UNSUPPORTED     # vertical support > LDS
    assert lib.l2i_face_resize_f32(p, p, 3, 8192, 64, 160, 160, q, q, 5, q, q, 5, s) == E_UNSUPPORTED           # input > 4096
    assert lib.l2i_face_resize_f32(p, p, 3, 64, 64, 160, 160, q, q, 300, q, q, 5, s) == E_UNSUPPORTED           # taps > 256
    assert lib.l2i_face_head_f32(p, None, p, p, p, 2, 4096, 9, 512, 0, s) == E_UNSUPPORTED                      # C > 2048
    assert lib.l2i_face_head_f32(p, None, p, p, p, 2, 1792, 9, 1024, 0, s) == E_UNSUPPORTED                     # E > 512
    assert lib.l2i_face_head_f32(p, None, p, p, p, 4, 1792, 9, 512, 2, s) == -1                                # pairs without dist
    with pytest.raises(_lib.L2IError, match='UNSUPPORTED|built for'):
        kernels.face_head(torch.zeros(2, 4096, 3, 3, device=DEV), torch.zeros(4096, 512, device=DEV), torch.zeros(512, device=DEV))


def _train(tmp_path, resolution=64):
    from latent2im_amd import trainer
    models = str(tmp_path / 'models')
    argv = ['--model', 'stylegan_v2_real', '--transform', 'face', '--num_samples', '4', '--learning_rate', '1e-3', '--latent', 'w',
            '--walk_type', 'linear', '--loss', 'l2', '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt',
            '--models_dir', models, '--overwrite_config', '--resolution', str(resolution), '--batch_size', '4', '--n_epoch', '1', '--seed', '3',
            '--model_save_freq', '1', '--synthetic_weights']
    trainer.main(multi_attr=False, argv=argv)
    out = os.path.join(models, 'stylegan_v2_real_face_linear_lr0.001_l2_w')
    return os.path.join(out, 'opt.yml'), os.path.join(out, 'model_w_1_final_walk_module.ckpt')


def test_eval_identity_end_to_end(state, tmp_path, monkeypatch, capsys):
    """evaluate.main(--identity on) at 64^2 on synthetic weights, 4 samples x 5 panels: the identity numbers against the host restatement
    (clip_ims -> PIL / numpy resize -> float64 CPU network -> scipy's cosine) over the same images, bucket sizes against the attribute buckets, the
    attribute results against an --identity off run, and the same numbers from a facenet-format checkpoint given by --facenet_ckpt."""
    from latent2im_amd import evaluate, graph
    os.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    saved = constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS
    try:
        cfg, ck = _train(tmp_path)
        calls = []
        method = graph.TransformGraph.vis_multi_image_batch_alphas_compute_multi_attr_identity

        def record(self, *a, **k):
            r = method(self, *a, **k)
            calls.append(r)
            return r
        monkeypatch.setattr(graph.TransformGraph, 'vis_multi_image_batch_alphas_compute_multi_attr_identity', record)
        argv = [cfg, '--save_path_w', ck, '--num_samples', '4', '--num_panels', '5', '--attrPath', './dataset/attributes_celeba.txt',
                '--target_attrList', 'Smiling']
        capsys.readouterr()
        on = evaluate.main(argv + ['--identity', 'on'])
        printed = capsys.readouterr().out
        assert printed.index('[IDENTITY PRESERVATION] Results on 3 epsilon segments') < printed.index('[ATTRIBUTE PRESERVATION]')
        assert len(calls) == 1
        off = evaluate.main(argv + ['--identity', 'off'])
        assert 'IDENTITY' not in capsys.readouterr().out and 'identity' not in off and len(calls) == 1
        for key in ('results', 'results_avg', 'bucket_sizes', 'index_'):
            assert np.array_equal(np.asarray(on[key]), np.asarray(off[key])), key
        assert on['identity_bucket_sizes'] == on['bucket_sizes'] and sum(on['bucket_sizes']) > 0
        assert len(on['identity_avg']) == len(on['identity']) == sum(1 for b in on['bucket_sizes'] if b)

        _, _, imgs, orgs, dists = calls[0]
        pairs = [[], [], []]
        for k in range(3):
            assert len(imgs[k]) == len(dists[k])
            if imgs[k]:
                xe = np.stack([R.resize_uint8(im) for im in imgs[k]]).astype(np.float64)
                xo = np.stack([R.resize_uint8(im) for im in orgs[k]]).astype(np.float64)
                e = R.embed(state, np.concatenate([xe, xo]), torch.float64).numpy()
                n = len(imgs[k])
                pairs[k] = list(zip(e[:n], e[n:]))
        want, want_avg, sizes = R.identity_metric([pairs])
        assert sizes == on['identity_bucket_sizes']
        print('identity: device %s, host restatement %s' % (on['identity_avg'], want_avg))
        np.testing.assert_allclose(on['identity'], want, rtol=0, atol=1e-4)
        np.testing.assert_allclose(on['identity_avg'], want_avg, rtol=0, atol=1e-4)

        sd = {k: torch.as_tensor(np.asarray(v)) for k, v in state.items()}
        sd['logits.weight'] = torch.zeros(8631, 512)
        sd['logits.bias'] = torch.zeros(8631)
        path = str(tmp_path / 'vggface2.pt')
        torch.save(sd, path)
        from_file = evaluate.main(argv + ['--identity', 'auto', '--facenet_ckpt', path])
        assert from_file['identity'] == on['identity'] and from_file['identity_avg'] == on['identity_avg']
    finally:
        constants.resolution, constants.BATCH_SIZE, constants.ALLOW_SYNTHETIC_WEIGHTS = saved
