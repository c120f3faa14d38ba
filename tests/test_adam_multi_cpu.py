"""The multi-tensor guarded Adam without a GPU: the header, the ctypes table and the ABI; the numpy model of one guarded step
(tests/adam_multi_ref.py) against torch.optim.Adam on the CPU and against a hand-written skip / growth sequence; the option surface of the captured
config-1 step."""
import ctypes
import os
import re

import numpy as np
import torch

from latent2im_amd import _lib
from tests import adam_multi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, 'include', 'l2i.h')).read()
SIZES = (1, 63, 4096, 4097, 3 * 4096 + 3, 7)


def _args(name):
    m = re.search(r'int %s\(([^;]*?)\);' % name, HDR, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def test_header_declares_the_table_and_both_entry_points():
    m = re.search(r'typedef struct l2i_adam_tensor \{([^}]*)\} l2i_adam_tensor;', HDR)
    assert m and [f.strip() for f in m.group(1).split(';') if f.strip()] == ['float* p', 'const float* g', 'float* m', 'float* v', 'float* step', 'int64_t n']
    assert int(re.search(r'#define L2I_ADAM_MAX_TENSORS (\d+)', HDR).group(1)) == _lib.ADAM_MAX_TENSORS == 16
    flag, adam = _args('l2i_nonfinite_flag_multi_f32'), _args('l2i_adam_guarded_multi_f32')
    assert flag == ['const l2i_adam_tensor* tensors', 'int32_t count', 'int32_t* state', 'void* stream']
    assert adam == ['const l2i_adam_tensor* tensors', 'int32_t count', 'float lr', 'float beta1', 'float beta2', 'float eps', 'int32_t* state', 'float* scale',
                    'float growth', 'float backoff', 'int32_t interval', 'float max_scale', 'int32_t last', 'void* stream']


def test_ctypes_table_binds_them_and_the_abi_is_unchanged():
    I, F, P = ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
    T = ctypes.POINTER(_lib.AdamTensor)
    assert _lib._SIGNATURES['l2i_nonfinite_flag_multi_f32'] == (I, [T, I, P, P])
    assert _lib._SIGNATURES['l2i_adam_guarded_multi_f32'] == (I, [T, I, F, F, F, F, P, P, F, F, I, F, I, P])
    assert {'l2i_nonfinite_flag_multi_f32', 'l2i_adam_guarded_multi_f32'} <= set(_lib.EXPORTS)
    assert [n for n, _ in _lib.AdamTensor._fields_] == ['p', 'g', 'm', 'v', 'step', 'n'] and ctypes.sizeof(_lib.AdamTensor) == 48
    assert _lib.ABI_VERSION == 12 == int(re.search(r'#define L2I_ABI_VERSION (\d+)', HDR).group(1))
    assert len(_lib._SIGNATURES['l2i_adam_guarded_f32'][1]) == 19               # the single-tensor entry is as it was
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'l2i_nonfinite_flag_multi_f32') and hasattr(lib, 'l2i_adam_guarded_multi_f32')


def _tensors(rs, steps=None):
    ts = []
    for i, n in enumerate(SIZES):
        ts.append(dict(p=rs.standard_normal(n).astype(np.float32), g=None, m=np.zeros(n, np.float32), v=np.zeros(n, np.float32),
                       step=np.float32(0 if steps is None else steps[i])))
    return ts


def test_model_follows_torch_adam_for_six_steps():
    rs = np.random.RandomState(0)
    ts = _tensors(rs)
    ps = [torch.nn.Parameter(torch.from_numpy(t['p'].copy())) for t in ts]
    opt = torch.optim.Adam(ps, lr=1e-3, betas=(0.5, 0.99))
    state, scale = R.new_state()
    for it in range(6):
        for t, p in zip(ts, ps):
            t['g'] = (rs.standard_normal(t['p'].shape) * 10.0 ** rs.uniform(-3, 1)).astype(np.float32)
            p.grad = torch.from_numpy(t['g'].copy())
        opt.step()
        R.step(ts, 1e-3, 0.5, 0.99, 1e-8, state, scale, chunk=4, interval=2000, max_scale=256.0)
        err = max(float(np.abs(t['p'] - p.detach().numpy()).max()) for t, p in zip(ts, ps))
        assert err < 1e-6, (it, err)
        assert all(float(t['step']) == it + 1 for t in ts)
    assert state.tolist() == [0, 6, 0, 6] and scale.tolist() == [1.0, 1.0]
    # the moments: at most four roundings a step on either side (two products, a sum, torch's lerp), six steps, each half an ulp of the largest
    # element seen: 24 * 2^-24 of it
    for t, p in zip(ts, ps):
        st = opt.state[p]
        for mine, theirs in ((t['m'], st['exp_avg'].numpy()), (t['v'], st['exp_avg_sq'].numpy())):
            assert np.abs(mine - theirs).max() <= 24 * 2.0 ** -24 * max(1.0, float(np.abs(theirs).max()))


def test_model_skip_backoff_and_growth_sequence():
    """By hand, interval 2, max_scale 2: clean (tracker 1), clean (growth to 2), clean, clean (growth refused at the cap: 4 > 2), inf in the last
    tensor (skip: nothing moves, no counter advances, scale 1, skipped 1), NaN in the first (skip, scale 0.5), clean (updates), clean (growth to 1)."""
    rs = np.random.RandomState(1)
    ts = _tensors(rs, steps=[0, 3, 1, 7, 2, 5])
    state, scale = R.new_state()
    kw = dict(interval=2, max_scale=2.0)
    want = [('clean', [0, 1, 0, 1], 1.0), ('clean', [0, 0, 0, 2], 2.0), ('clean', [0, 1, 0, 3], 2.0), ('clean', [0, 0, 0, 4], 2.0),
            ('inf', [0, 0, 1, 5], 1.0), ('nan', [0, 0, 2, 6], 0.5), ('clean', [0, 1, 2, 7], 0.5), ('clean', [0, 0, 2, 8], 1.0)]
    applied = 0
    for kind, st_want, sc_want in want:
        for t in ts:
            t['g'] = rs.standard_normal(t['p'].shape).astype(np.float32)
        if kind == 'inf':
            ts[-1]['g'][-1] = np.inf
        if kind == 'nan':
            ts[0]['g'][0] = np.nan
        before = [{k: np.array(t[k]).copy() for k in ('p', 'm', 'v', 'step')} for t in ts]
        R.step(ts, 1e-3, 0.5, 0.99, 1e-8, state, scale, chunk=4, **kw)
        assert state.tolist() == st_want and scale.tolist() == [sc_want, 1.0 / sc_want], (kind, state, scale)
        moved = [not np.array_equal(t['p'], b['p']) for t, b in zip(ts, before)]
        if kind == 'clean':
            applied += 1
            assert all(moved)
        else:
            assert not any(moved) and all(np.array_equal(t[k], b[k]) for t, b in zip(ts, before) for k in ('m', 'v', 'step'))
        assert [float(t['step']) for t in ts] == [s + applied for s in (0, 3, 1, 7, 2, 5)]
    assert all(np.isfinite(t['p']).all() for t in ts)


def test_train_options_accept_hip_graph_with_the_pggan_model(tmp_path):
    from latent2im_amd.options import TrainOptions
    opt = TrainOptions().parse(print_opt=False, argv=['--model', 'pggan', '--transform', 'face', '--no_gan_loss', '--synthetic_weights', '--hip_graph', '--precision', 'f16',
                                                      '--models_dir', str(tmp_path), '--attrList', 'Smiling', '--attrPath', './dataset/attributes_celeba.txt'])
    assert opt.hip_graph is True and opt.model == 'pggan' and opt.precision == 'f16'
    from latent2im_amd import capture, pggan, trainer
    assert hasattr(capture, 'CapturedZStep') and hasattr(pggan.TransformGraph, 'captured_step')
    assert callable(pggan.walk_forward_backward) and callable(pggan.walk_update) and callable(trainer._captured_batch)
