"""graph.WalkGraph, the base of both walk graphs, and the one --hip_graph route of trainer.train_step, without a GPU: the routing runs on stub
graphs that offer the two methods train_step asks a graph for (``captured_step`` / ``eager_step``) and count what reaches them."""
import numpy as np
import pytest

from latent2im_amd import graph, pggan, trainer


class _Recorded:
    """What a graph's captured_step returns, as far as train_step uses it: ``.z`` of the recorded batch, and the call."""

    def __init__(self, batch):
        self.z = np.zeros((batch, 512))
        self.calls = []

    def __call__(self, zs, alpha):
        self.calls.append((zs.shape[0], np.asarray(alpha).copy()))
        return dict(loss='replayed', x0='x0', x1='x1')


class _WStub:
    """The StyleGAN2 kind: records a step for every flag combination."""
    device = 'cpu'

    def __init__(self):
        self.built, self.eager = [], []

    def get_train_alpha(self, zs_batch, N_attr=40, trainEmbed=False):
        a = np.random.uniform(0, 1, N_attr)
        return np.ones((zs_batch.shape[0], 1)) * a, a, None

    def captured_step(self, batch, n_attr, **flags):
        self.built.append((batch, n_attr, flags))
        return _Recorded(batch)

    def eager_step(self, zs_batch, alpha, **kw):
        self.eager.append((zs_batch.shape[0], np.asarray(alpha).copy(), kw))
        return 'eager', 'x0', 'x1'


class _ZStub(_WStub):
    """The PGGAN kind: no recorded step with the GAN term on."""

    def captured_step(self, batch, n_attr, **flags):
        st = super().captured_step(batch, n_attr, **flags)
        return st if flags['no_gan_loss'] else None


def _opt(**kw):
    return type('O', (), dict(dict(hip_graph=True, no_content_loss=False, no_gan_loss=True), **kw))()


@pytest.fixture
def seeded():
    state = np.random.get_state()
    np.random.seed(5)
    yield np.random.RandomState(5)                                           # the same stream, to predict the draws
    np.random.set_state(state)


@pytest.mark.parametrize('stub', [_WStub, _ZStub])
def test_full_batches_replay_ragged_ones_and_train_embed_run_eagerly(stub, seeded):
    g, opt, attrs = stub(), _opt(no_content_loss=True), ['Smiling', 'Young']
    full, ragged = np.zeros((4, 512)), np.zeros((3, 512))
    want = [seeded.uniform(0, 1, 2) for _ in range(5)]                       # one draw of the global numpy RNG a step, on every route
    r = trainer.train_step(g, full, attrs, layers=['2', '3'], opt=opt, multi_attr=True)
    assert r[0] == 'replayed' and r[2:] == ('x0', 'x1') and np.array_equal(r[1], want[0])
    # built once, from train_step's own arguments: nothing was put on the graph beforehand
    assert g.built == [(4, 2, dict(clamp=True, layers=['2', '3'], no_content_loss=True, no_gan_loss=True))]
    assert not hasattr(g, '_captured_opts') and len(g._captured_step.calls) == 1 and g.eager == []
    assert g._captured_step.calls[0][0] == 4 and np.array_equal(g._captured_step.calls[0][1], np.ones((4, 1)) * want[0])
    r = trainer.train_step(g, full, attrs, layers=['2', '3'], opt=opt, multi_attr=True)
    assert r[0] == 'replayed' and np.array_equal(r[1], want[1]) and len(g.built) == 1 and len(g._captured_step.calls) == 2
    r = trainer.train_step(g, ragged, attrs, layers=['2', '3'], opt=opt, multi_attr=True)           # ragged: eager, no rebuild
    assert r[0] == 'eager' and np.array_equal(r[1], want[2]) and len(g.built) == 1 and len(g._captured_step.calls) == 2
    n, alpha, kw = g.eager[0]
    assert n == 3 and np.array_equal(alpha, np.ones((3, 1)) * want[2])
    assert kw == dict(clamp=True, layers=['2', '3'], no_content_loss=True, no_gan_loss=True, trainEmbed=False, updateGAN=False)
    r = trainer.train_step(g, full, attrs, trainEmbed=True, opt=opt)                                # trainEmbed: eager
    assert r[0] == 'eager' and len(g.eager) == 2 and g.eager[1][2]['trainEmbed'] is True and len(g._captured_step.calls) == 2
    r = trainer.train_step(g, full, attrs, opt=_opt(hip_graph=False))                               # no --hip_graph: eager
    assert r[0] == 'eager' and np.array_equal(r[1], want[4]) and len(g.eager) == 3 and len(g._captured_step.calls) == 2
    assert g.eager[2][2] == dict(clamp=False, layers=None, no_content_loss=False, no_gan_loss=True, trainEmbed=False, updateGAN=False)


def test_gan_term_replays_on_the_w_graph_and_runs_eagerly_on_the_z_graph(seeded):
    opt, full = _opt(no_gan_loss=False), np.zeros((4, 512))
    w = _WStub()
    assert trainer.train_step(w, full, ['Smiling'], opt=opt)[0] == 'replayed'
    assert w.built[0][2]['no_gan_loss'] is False and w.eager == []
    z = _ZStub()
    assert trainer.train_step(z, full, ['Smiling'], opt=opt)[0] == 'eager'
    assert z._captured_step is None and z.eager[0][2]['no_gan_loss'] is False
    assert trainer.train_step(z, full, ['Smiling'], opt=_opt())[0] == 'replayed'                    # the GAN term off again: recorded now
    assert len(z.built) == 2 and len(z._captured_step.calls) == 1
    # the GAN term back on after the recording: not the recorded step's flags, so eager (where the PGGAN graph raises), and nothing is re-recorded
    assert trainer.train_step(z, full, ['Smiling'], opt=opt)[0] == 'eager'
    assert len(z.built) == 2 and len(z._captured_step.calls) == 1 and len(z.eager) == 2


def test_a_graph_without_a_captured_step_is_refused_before_it_is_touched():
    class _Bare:
        def __getattr__(self, name):
            if name != 'captured_step':
                raise AssertionError('touched %s' % name)
            raise AttributeError(name)
    with pytest.raises(NotImplementedError, match='hip_graph'):
        trainer.train_step(_Bare(), np.zeros((2, 512)), ['Smiling'], opt=_opt())


def test_both_graphs_share_the_base():
    base = graph.WalkGraph
    for cls in (graph.TransformGraph, pggan.TransformGraph, graph.faceGraph, pggan.SceneGraph):
        assert issubclass(cls, base)
        for name in ('calibrate_scales', 'optimizeParametersAll', '_attr_columns', 'get_reg_preds', 'walk_update', 'save_multi_models'):
            assert getattr(cls, name) is getattr(base, name), (cls, name)
        assert cls.optimize_parameters is base.optimizeParametersAll
    for cls in (graph.TransformGraph, pggan.TransformGraph):                 # where the reference's graphs differ, each keeps its own
        for name in ('get_logits', 'get_alphas', 'get_reg_loss', 'get_content_loss', 'get_w_loss', 'clip_ims', 'apply_alpha', 'eager_step',
                     'captured_step', '_probe_step'):
            assert name in vars(cls) and name not in vars(base), (cls, name)
    assert pggan.faceGraph.__module__ == 'latent2im_amd.pggan' and graph.faceGraph.__module__ == 'latent2im_amd.graph'
    assert issubclass(pggan.faceGraph, pggan.PixelTransform) and issubclass(graph.SceneGraph, graph.PixelTransform)


def test_the_stylegan2_graph_spells_the_one_optimiser_slot_both_ways():
    g = object.__new__(graph.TransformGraph)
    first, second = object(), object()
    g.optimizers = first
    assert g.optimizer is first and vars(g) == {'optimizer': first}
    g.optimizer = second
    assert g.optimizers is second
    assert not hasattr(pggan.TransformGraph, 'optimizers')
