"""The float64 model of the identity loss (tests/faceid_ref.py) held to itself on the CPU: the adjoint is the adjoint, autograd agrees with the
hand-written backward, the unclamped resize stays beside the byte path it restates, the fixture reproduces, every planted mistake leaves the
bounds, and the driver flag parses."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from latent2im_amd import constants, face_specs
from latent2im_amd.options import TrainOptions
from tests import facenet_ref as R
from tests import faceid_ref as M
from tests.golden import make_faceid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'faceid.npz')
SHAPES = ((32, 32), (160, 160), (200, 200), (96, 64), (256, 256))


@pytest.mark.parametrize('h,w', SHAPES)
def test_adjoint_is_the_adjoint(h, w):
    """<R u, y> = <u, R^T y> to 1e-12 relative in float64 (every pixel inside the clamp, where the map is 127.5 (x + 1) -> R)."""
    rs = np.random.RandomState(h + w)
    x = rs.uniform(-0.9, 0.9, (2, h, w)).astype(np.float32)
    y = rs.randn(2, 160, 160)
    r, _ = M.resize_lin(x)
    gx, _ = M.resize_lin_bwd(y, x)
    lhs, rhs = (r * y).sum(), (M.level(x) * gx / 127.5).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize('in_size', (32, 64, 96, 160, 200, 256, 1024))
def test_product_inverse_tables(in_size):
    """The inverse tables the product hands the adjoint kernel are the forward tables transposed (brute force), and hold every forward tap once."""
    from latent2im_amd import facenet
    ib, ic = facenet.inverse_tables(in_size, 160)
    jb, jc = M.inverse_tables(in_size, 160)
    assert np.array_equal(ib, jb) and np.array_equal(ic, jc)
    fb, fc = R.resize_tables(in_size, 160)
    assert ib[:, 1].sum() == fb[:, 1].sum() and np.array_equal(facenet.resize_tables(in_size, 160)[1], fc)


def _small_problem(seed=0, size=6, out=4, C=5, E=3):
    rs = np.random.RandomState(seed)
    x0 = rs.uniform(-0.9, 0.9, (2, 1, size, size))
    x1 = rs.uniform(-1.4, 1.4, (2, 1, size, size))
    x1[np.abs(np.abs(x1) - 1.0) < 0.05] = 0.3                     # away from the clamp edges: gradcheck differentiates numerically
    x1 = x1.astype(np.float32).astype(np.float64)                 # float32 values: the numpy model forms the level in float32
    A = torch.tensor(rs.randn(C * 4, out * out))                  # the trunk's stand-in: a fixed linear map r -> feat [C, HW = 4]
    w_t, bias = rs.randn(C, E), rs.randn(E)
    return x0, x1, A, w_t, bias, out, C


def _small_embed(A, w_t, bias, C):
    wt, b = torch.tensor(w_t), torch.tensor(bias)

    def f(r):
        feat = (r.reshape(r.shape[0], -1) @ A.t()).reshape(r.shape[0], C, 4)
        return F.normalize(feat.mean(2) @ wt + b, p=2, dim=1)
    return f


def test_gradcheck_resize_and_head():
    """torch.autograd.gradcheck at its float64 defaults on resize + head with the trunk replaced by a fixed random linear map, and the hand-written
    backward (head_bwd, then the map's transpose, then resize_lin_bwd) against autograd."""
    x0, x1, A, w_t, bias, out, C = _small_problem()
    emb = _small_embed(A, w_t, bias, C)
    with torch.no_grad():
        e0 = emb(M.resize_lin_t(torch.tensor(x0), torch.float64, (out, out)))

    def loss(x):
        return (1.0 - F.cosine_similarity(emb(M.resize_lin_t(x, torch.float64, (out, out))), e0, dim=1)).mean()
    xt = torch.tensor(x1, requires_grad=True)
    assert torch.autograd.gradcheck(loss, (xt,))
    want, = torch.autograd.grad(loss(xt), xt)
    x1f = x1.astype(np.float32)
    r, _ = M.resize_lin(x1f, (out, out))
    feat = (r.reshape(2, -1) @ A.numpy().T).reshape(2, C, 4)
    g_feat, _ = M.head_bwd(feat, w_t, bias, e0.numpy(), np.full(2, 0.5))
    g_r = (g_feat.reshape(2, -1) @ A.numpy()).reshape(2, 1, out, out)
    got, _ = M.resize_lin_bwd(g_r, x1f)
    # (the numpy model forms the level in float32, torch here in float64: r differs by 2^-23 relative, and so does a smooth function of it)
    assert np.abs(got - want.numpy()).max() <= 1e-6 * np.abs(want.numpy()).max()


@pytest.mark.parametrize('h,w', SHAPES)
def test_linear_resize_stays_beside_the_byte_path(h, w):
    """Without the uint8 intermediate, the roundings and the clips the result differs from PIL's bytes by what those drop: truncating the input
    to a byte (< 1 level, times sum |wx| sum |wy|), rounding the intermediate (0.5 level, times sum |wy|) and the result (0.5) — as long as
    neither pass of the byte path clips, which a mid-grey image guarantees."""
    rs = np.random.RandomState(h * 7 + w)
    x = rs.uniform(-0.5, 0.5, (1, 3, h, w)).astype(np.float32)
    want = R.face_input(x) if h == w else np.stack([_byte_path(im) for im in R.clip_ims(x)]).astype(np.float32)
    got, _ = M.resize_lin(x)
    ry, rx = M.dense(h, 160)[0], M.dense(w, 160)[0]
    sy, sx = np.abs(ry).sum(1)[:, None], np.abs(rx).sum(1)[None, :]
    bound = sx * sy + 0.5 * sy + 0.5
    assert (np.abs(got - want) <= bound + 1e-9).all(), np.abs(got - want).max()
    assert np.abs(got - want).max() > 0.0 or (h, w) == (160, 160)


def _byte_path(img_chw):
    """facenet_ref.resize_uint8 for a non-square image (it takes both tables from the image's own sides)."""
    c, h, w = img_chw.shape
    mid = R._pass(img_chw, *R.resize_tables(w, 160))
    return np.swapaxes(R._pass(np.swapaxes(mid, 1, 2), *R.resize_tables(h, 160)), 1, 2)


def test_fixture_reproduces():
    fx = np.load(GOLDEN)
    state = face_specs.facenet_state(seed=constants.SYNTH_SEED_F)
    for name, res, seed in M.CASES:
        x0, x1, loss, gx, gr, e0, e1 = make_faceid.evaluate(state, res, seed, torch.float64)
        assert abs(loss - float(fx[name + '.loss'])) <= 1e-10
        scale = np.abs(gx).max()
        assert np.abs(gx.reshape(-1)[make_faceid.probe_index(gx.size, seed)] - fx[name + '.g_x1_probe']).max() <= 1e-9 * scale
        if name + '.g_x1' in fx:
            assert np.abs(gx - fx[name + '.g_x1']).max() <= 1e-9 * scale
        else:
            assert np.abs(gr - fx[name + '.g_r']).max() <= 1e-6 * np.abs(gr).max()              # stored as float32
            back, _ = M.resize_lin_bwd(fx[name + '.g_r'].astype(np.float64), x1)
            assert np.abs(back - gx).max() <= 1e-6 * scale
        assert 0.05 < float(fx[name + '.clamped']) < 0.5
        lv = M.level(x1)
        assert abs(float(((lv <= 0) | (lv >= 255)).mean()) - float(fx[name + '.clamped'])) < 1e-12


# ---- planted mistakes -----------------------------------------------------------------------------------------------------------------------------
def _leaves(value, want, bound):
    return bool((np.abs(value - want) > bound).any())


def test_planted_mistakes_leave_the_bounds():
    rs = np.random.RandomState(5)
    x = (0.8 * rs.randn(2, 96, 64)).astype(np.float32)             # H != W: an axis swap shows
    r, rb = M.resize_lin(x)
    for m in M.MISTAKES_RESIZE:
        assert _leaves(M.resize_lin(x, mistake=m)[0], r, rb), m
    gy = rs.randn(2, 160, 160)
    g, gb = M.resize_lin_bwd(gy, x)
    for m in M.MISTAKES_ADJOINT:
        assert _leaves(M.resize_lin_bwd(gy, x, mistake=m)[0], g, gb), m
    feat, w_t, bias = rs.randn(3, 64, 4), rs.randn(64, 32) / 8.0, 0.05 * rs.randn(32)
    v, gd = rs.randn(3, 32), rs.uniform(0.2, 1.0, 3)
    h, hb = M.head_bwd(feat, w_t, bias, v, gd)
    for m in M.MISTAKES_HEAD:
        assert _leaves(M.head_bwd(feat, w_t, bias, v, gd, mistake=m)[0], h, hb), m
    assert not _leaves(r, r, rb) and not _leaves(g, g, gb) and not _leaves(h, h, hb)


def test_float32_evaluations_stay_inside_the_bounds():
    """The bounds are not vacuous the other way either: plain float32 numpy evaluations of the three kernels' formulas lie inside them."""
    rs = np.random.RandomState(6)
    x = (0.8 * rs.randn(2, 96, 64)).astype(np.float32)
    ry, rx = M.dense(96, 160)[0].astype(np.float32), M.dense(64, 160)[0].astype(np.float32)
    r, rb = M.resize_lin(x)
    assert (np.abs((ry @ M.clip255(x).astype(np.float32) @ rx.T).astype(np.float64) - r) <= rb).all()
    gy = rs.randn(2, 160, 160).astype(np.float32)
    g, gb = M.resize_lin_bwd(gy, x)
    g32 = np.float32(127.5) * M.pass_mask(x) * (ry.T @ gy @ rx)
    assert (np.abs(g32.astype(np.float64) - g) <= gb).all()
    feat, w_t, bias = rs.randn(3, 64, 4).astype(np.float32), (rs.randn(64, 32) / 8.0).astype(np.float32), (0.05 * rs.randn(32)).astype(np.float32)
    v, gd = rs.randn(3, 32).astype(np.float32), rs.uniform(0.2, 1.0, 3).astype(np.float32)
    h, hb = M.head_bwd(feat, w_t, bias, v, gd)
    p = feat.mean(2, dtype=np.float32)
    t = p @ w_t + bias
    n = np.sqrt((t * t).sum(1, keepdims=True))
    e, vh = t / n, v / np.sqrt((v * v).sum(1, keepdims=True))
    c = (e * vh).sum(1, keepdims=True)
    gp = ((-gd[:, None] * (vh - c * e) / n) @ w_t.T) / np.float32(4)
    assert gp.dtype == np.float32 and (np.abs(np.repeat(gp[:, :, None], 4, 2).astype(np.float64) - h) <= hb).all()


def test_gradient_does_not_leak_into_the_original():
    """e0 is a constant: the whole-term model's gradient w.r.t. x1 is the same whether or not x0 carries a graph, and a leak (x0 = x1's own
    tensor, not detached) changes it."""
    x0, x1, A, w_t, bias, out, C = _small_problem(3)
    emb = _small_embed(A, w_t, bias, C)
    x = torch.tensor(x1, requires_grad=True)

    def term(detach):
        e0 = emb(M.resize_lin_t(x * 0.5, torch.float64, (out, out)))
        return (1.0 - F.cosine_similarity(emb(M.resize_lin_t(x, torch.float64, (out, out))), e0.detach() if detach else e0, dim=1)).mean()
    clean, = torch.autograd.grad(term(True), x)
    leaky, = torch.autograd.grad(term(False), x)
    with torch.no_grad():
        e0 = emb(M.resize_lin_t(x * 0.5, torch.float64, (out, out)))
    r, _ = M.resize_lin(x1.astype(np.float32), (out, out))
    assert (clean - leaky).abs().max() > 1e-3 * clean.abs().max()
    want = clean
    feat = (r.reshape(2, -1) @ A.numpy().T).reshape(2, C, 4)
    g_r = (M.head_bwd(feat, w_t, bias, e0.numpy(), np.full(2, 0.5))[0].reshape(2, -1) @ A.numpy()).reshape(2, 1, out, out)
    assert np.abs(M.resize_lin_bwd(g_r, x1.astype(np.float32))[0] - want.numpy()).max() <= 1e-6 * want.abs().max().item()


# ---- the flag -------------------------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, *extra, print_opt=False):
    argv = ['--model', 'stylegan_v2_real', '--transform', 'face', '--models_dir', str(tmp_path), '--overwrite_config'] + list(extra)
    return TrainOptions().parse(print_opt=print_opt, argv=argv)


def test_id_loss_flag(tmp_path, capsys):
    import yaml
    from latent2im_amd import hostutil
    p = TrainOptions().initialize()
    assert p.get_default('id_loss') == 0.0 and p.get_default('facenet_ckpt') is None
    opt = _parse(tmp_path)                                        # unset: the namespace (and opt.yml) of a run without the flag is what it was
    assert getattr(opt, 'id_loss', 0.0) == 0.0 and not hasattr(opt, 'id_loss') and not hasattr(opt, 'facenet_ckpt')
    assert 'id_weight' not in hostutil.set_graph_kwargs(opt)
    opt = _parse(tmp_path, '--id_loss', '0.5', '--facenet_ckpt', '/nowhere/face.pt', print_opt=True)
    capsys.readouterr()
    assert opt.id_loss == 0.5 and opt.facenet_ckpt == '/nowhere/face.pt'
    kw = hostutil.set_graph_kwargs(opt)
    assert kw['id_weight'] == 0.5 and kw['facenet_ckpt'] == '/nowhere/face.pt'
    with open(os.path.join(opt.output_dir, 'opt.yml')) as f:
        dump = yaml.load(f, Loader=yaml.FullLoader)
    assert dump['id_loss'] == 0.5 and dump['facenet_ckpt'] == '/nowhere/face.pt'
    cfg = tmp_path / 'again.yml'
    cfg.write_text(yaml.dump(dump))
    again = _parse(tmp_path, '--config_file', str(cfg))           # the round trip through opt.yml
    assert again.id_loss == 0.5 and again.facenet_ckpt == '/nowhere/face.pt'
    for bad, why in ((['--id_loss', '-1'], '>= 0'), (['--facenet_ckpt', 'x.pt'], 'needs --id_loss')):
        with pytest.raises(SystemExit):
            _parse(tmp_path, *bad)
        assert why in capsys.readouterr().err
