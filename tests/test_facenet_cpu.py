"""The identity-preservation half of eval.py, host side: PIL's resize restated and pinned, the product's coefficient tables, the facenet state
dict layout and loader, the metric's aggregation and the --identity option."""
import numpy as np
import pytest
import torch

from latent2im_amd import constants, evaluate, face_specs, facenet
from tests import facenet_ref as R

SIZES = (1024, 256, 200, 160, 64, 32)


def _image(n, seed):
    """Random uint8 [3, n, n] with flat, saturated (0 / 255) and mid-grey regions: the clip8 edges of both passes."""
    x = np.random.RandomState(seed).randint(0, 256, (3, n, n)).astype(np.uint8)
    x[:, : n // 4] = 255
    x[:, n // 4: n // 3] = 0
    x[0, :, : n // 5] = 128
    x[1, n // 2:, n // 2:] = 255
    return x


@pytest.mark.parametrize('n', SIZES)
def test_resize_restatement_is_pil(n):
    Image = pytest.importorskip('PIL.Image')
    x = _image(n, n)
    want = np.asarray(Image.fromarray(x.transpose(1, 2, 0)).resize((160, 160))).transpose(2, 0, 1)
    np.testing.assert_array_equal(R.resize_uint8(x), want)


@pytest.mark.parametrize('n', SIZES)
def test_product_tables_are_the_restatements(n):
    b, c = facenet.resize_tables(n, 160)
    rb, rc = R.resize_tables(n, 160)
    assert b.dtype == np.int32 and c.dtype == np.int32
    np.testing.assert_array_equal(b, rb)
    np.testing.assert_array_equal(c, rc)
    assert (b[:, 0] >= 0).all() and (b.sum(1) <= n).all() and (b[:, 1] <= c.shape[1]).all()      # every tap inside the image and the table


def test_synthetic_state_layout():
    spec = face_specs.facenet_spec()
    st = face_specs.facenet_state()
    assert list(st) == list(spec)
    assert all(tuple(np.shape(st[k])) == tuple(v) for k, v in spec.items())
    convs = [k for k in spec if k.endswith('conv.weight') or k.endswith('conv2d.weight')]
    assert len(convs) == 132
    for k in ('conv2d_1a.conv.weight', 'repeat_1.0.branch1.0.conv.weight', 'repeat_2.3.conv2d.bias', 'mixed_7a.branch0.1.bn.running_mean',
              'last_bn.running_var', 'block8.conv2d.weight', 'repeat_2.9.branch1.2.conv.weight'):
        assert k in spec, k
    assert spec['repeat_2.0.branch1.1.conv.weight'] == (128, 128, 1, 7) and spec['repeat_2.0.branch1.2.conv.weight'] == (128, 128, 7, 1)
    assert spec['last_linear.weight'] == (512, 1792) and not any(k.startswith('logits.') for k in spec)
    np.testing.assert_array_equal(face_specs.facenet_state()['repeat_3.4.conv2d.weight'], st['repeat_3.4.conv2d.weight'])      # seeded


def test_checkpoint_keys(tmp_path):
    st = face_specs.facenet_state()
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in st.items()}
    sd['logits.weight'] = torch.zeros(8631, 512)
    sd['logits.bias'] = torch.zeros(8631)
    path = str(tmp_path / 'vggface2.pt')
    torch.save(sd, path)
    got = facenet.load_state(path)
    assert set(got) == {k for k in st if not k.endswith('num_batches_tracked')}
    np.testing.assert_array_equal(got['mixed_6a.branch1.2.bn.running_var'], st['mixed_6a.branch1.2.bn.running_var'])
    no_nbt = {k: v for k, v in sd.items() if not k.endswith('num_batches_tracked')}
    assert set(facenet.check_state(no_nbt)) == set(got)
    missing = dict(sd)
    del missing['repeat_1.2.branch2.1.bn.running_mean']
    with pytest.raises(KeyError, match='missing'):
        facenet.check_state(missing)
    extra = dict(sd)
    extra['repeat_1.2.branch3.0.conv.weight'] = torch.zeros(1)
    with pytest.raises(KeyError, match='unexpected'):
        facenet.check_state(extra)
    bad = dict(sd)
    bad['last_linear.weight'] = torch.zeros(512, 1536)
    with pytest.raises(ValueError, match='last_linear.weight'):
        facenet.check_state(bad)


def test_cosine_restatement_is_scipys():
    """R.cosine against what scipy 1.15's scipy.spatial.distance.cosine returned for these vectors (unrelated, nearly equal, opposite,
    parallel: the clip at 0 and 2)."""
    rs = np.random.RandomState(11)
    u, v = rs.randn(4, 512), rs.randn(4, 512)
    v[1] = u[1] + 1e-3 * v[1]
    v[2] = -u[2]
    v[3] = u[3] * 2.5
    scipy_says = (0.9902523709476202, 4.452845987490406e-07, 2.0, 2.220446049250313e-16)
    for i, want in enumerate(scipy_says):
        assert abs(R.cosine(u[i], v[i]) - want) <= 1e-15, i
    with pytest.raises(AssertionError, match='1-D'):
        R.cosine(u[:1], v[:1])                       # scipy >= 1.15 refuses the reference's (1, 512) arguments too


def test_metric_matches_eval_py():
    """eval.py:170-209 over three (batch, target attribute) calls with an empty bucket: main()'s accumulation (sim[k] += dists[k]) and
    facenet.identity_preservation against the restatement's loop."""
    rs = np.random.RandomState(0)

    def unit(n):
        e = rs.randn(n, 512).astype(np.float32)
        return e / np.linalg.norm(e, axis=1, keepdims=True)
    calls = []
    for sizes in ((3, 0, 2), (1, 0, 4), (0, 0, 1)):
        call = []
        for n in sizes:
            e, o = unit(n), unit(n)
            o[:n // 2] = e[:n // 2] + 0.01 * rs.randn(n // 2, 512)
            call.append(list(zip(e, o)))
        calls.append(call)
    sim = [[], [], []]
    for call in calls:
        dists = [[R.cosine(np.float64(e), np.float64(o)) for e, o in call[k]] for k in range(3)]
        for k in range(3):
            sim[k] += dists[k]
    res, avg = facenet.identity_preservation(sim)
    want_res, want_avg, sizes = R.identity_metric(calls)
    assert sizes == [4, 0, 7] and len(res) == len(avg) == 2
    np.testing.assert_allclose(res, want_res, rtol=0, atol=1e-12)
    np.testing.assert_allclose(avg, want_avg, rtol=0, atol=1e-12)


def test_identity_option(tmp_path, capsys):
    cfg = tmp_path / 'opt.yml'
    cfg.write_text('model: stylegan_v2_real\n')
    parser = evaluate.eval_options().parser
    opt = parser.parse_args([str(cfg)])
    opt.config_file.close()
    assert opt.identity == 'auto' and opt.facenet_ckpt is None
    opt = parser.parse_args([str(cfg), '--identity', 'off', '--facenet_ckpt', '/x/vggface2.pt'])
    opt.config_file.close()
    assert opt.identity == 'off' and opt.facenet_ckpt == '/x/vggface2.pt'
    with pytest.raises(SystemExit):
        parser.parse_args([str(cfg), '--identity', 'yes'])
    capsys.readouterr()

    ck = tmp_path / 'vggface2.pt'
    ck.write_bytes(b'')
    missing = str(tmp_path / 'nowhere.pt')
    saved = constants.ALLOW_SYNTHETIC_WEIGHTS
    try:
        for allow in (False, True):
            constants.ALLOW_SYNTHETIC_WEIGHTS = allow
            assert facenet.identity_mode('off', str(ck)) is False
            assert facenet.identity_mode('auto', str(ck)) is True
            assert facenet.identity_mode('on', str(ck)) is True
            assert capsys.readouterr().err == ''
            assert facenet.identity_mode('auto', missing) is False            # auto never falls back to synthetic weights
            err = capsys.readouterr().err
            assert err.count('\n') == 1 and 'identity' in err
            assert facenet.identity_mode('auto', '') is False
            capsys.readouterr()
        constants.ALLOW_SYNTHETIC_WEIGHTS = True
        assert facenet.identity_mode('on', missing) is True
        constants.ALLOW_SYNTHETIC_WEIGHTS = False
        with pytest.raises(FileNotFoundError, match='face network'):
            facenet.identity_mode('on', missing)
    finally:
        constants.ALLOW_SYNTHETIC_WEIGHTS = saved
