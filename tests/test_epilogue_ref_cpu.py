"""The float64 epilogue model (tests/epilogue_ref.py) against independently written compositions, and the case table against the mistakes it
claims to catch: a case that cannot see its own target mistake is a bug in the table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import epilogue_ref as er

# the shape of the generic-kernel route of tests/test_epilogue_contract_gpu.py
CIN, COUT, H, W, B = 40, 48, 20, 20, 2
LOOSEST_BOUND = 3e-5          # the F(4x4) family's; the exact-fp32 families assert 5e-6


def _problem(seed, fields):
    rs = np.random.RandomState(1000 + seed)
    wt = torch.from_numpy((rs.randn(COUT, CIN, 3, 3) / np.sqrt(CIN * 9)).astype(np.float32))
    x, kw, y_prev, _ = er.make_inputs(seed, fields, (B, CIN, H, W), COUT, (B, COUT, H, W))
    return wt, x, kw, y_prev


def D(t):
    return t.double()


def bc(t):
    return D(t)[:, :, None, None]


def test_product_combinations_written_inline():
    """The three combinations every kernel family's own test uses, the res_sub term and the +-0.0 rule, composed by hand."""
    rs = np.random.RandomState(5)
    T = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    wt = T(COUT, CIN, 3, 3) / 19.0
    x, s, d = T(B, CIN, H, W), torch.rand(B, CIN) + 0.5, torch.rand(B, COUT) + 0.5
    nz, bias = T(B, 1, H, W), T(COUT)
    msk, res, rmk, omk, prev, sub = T(B, CIN, H, W), *(T(B, COUT, H, W) for _ in range(5))
    c64 = lambda t: F.conv2d(t, D(wt), padding=1)
    # 1: style scale, demodulation, noise, bias, leaky ReLU
    want = F.leaky_relu(c64(D(x) * bc(s)) * bc(d) + D(nz) * 0.3 + D(bias)[None, :, None, None], 0.2) * 2 ** 0.5
    got = er.conv_epi_ref(x, wt, 1, 1, in_scale=s, out_scale=d, noise=nz, noise_w=0.3, bias=bias, act=er.ACT_LRELU, slope=0.2, gain=2 ** 0.5)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    # 2: masked input, bias, masked residual, ReLU
    xm = D(x) * torch.where(msk > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.2, dtype=torch.float64))
    want = torch.relu(c64(xm) + D(bias)[None, :, None, None] + torch.where(rmk > 0, D(res), torch.zeros_like(D(res))))
    got = er.conv_epi_ref(x, wt, 1, 1, in_mask=msk, mask=(1.0, 0.2), bias=bias, residual=res, res_mask=rmk, act=er.ACT_RELU)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    # 3: output mask, output gain, accumulate
    want = torch.where(omk > 0, c64(D(x)), torch.zeros_like(D(res))) * 0.5 + D(prev)
    got = er.conv_epi_ref(x, wt, 1, 1, y_prev=prev, out_mask=omk, out_gain=0.5, accumulate=True)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    # res_sub: the residual term is res_coef * res_coef_dev[0] * (residual - res_sub), masked; a NULL res_coef_dev reads as 1
    want = c64(D(x)) + torch.where(omk > 0, 0.25 * 2.0 * (D(res) - D(sub)), torch.zeros_like(D(res)))
    got = er.conv_epi_ref(x, wt, 1, 1, residual=res, res_sub=sub, res_coef=0.25, res_coef_dev=torch.full((1,), 2.0), res_mask=omk)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    want = c64(D(x)) + 0.25 * (D(res) - D(sub))
    got = er.conv_epi_ref(x, wt, 1, 1, residual=res, res_sub=sub, res_coef=0.25)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_both_zeros_take_the_negative_branch():
    rs = np.random.RandomState(7)
    wt = torch.from_numpy((rs.randn(COUT, CIN, 3, 3) / 19.0).astype(np.float32))
    x = torch.from_numpy(rs.randn(B, CIN, H, W).astype(np.float32))
    res = torch.from_numpy(rs.randn(B, COUT, H, W).astype(np.float32))
    c = F.conv2d(D(x), D(wt), padding=1)
    for zero in (0.0, -0.0):
        my, mx = torch.full((B, COUT, H, W), zero), torch.full((B, CIN, H, W), zero)
        assert float(er.conv_epi_ref(x, wt, 1, 1, out_mask=my).abs().max()) == 0.0
        assert torch.equal(er.conv_epi_ref(x, wt, 1, 1, residual=res, res_mask=my), c)
        assert torch.allclose(er.conv_epi_ref(x, wt, 1, 1, in_mask=mx, mask=(3.0, 0.5)), 0.5 * c, rtol=0, atol=1e-12)
    m = er.masks_like(rs, (B, COUT, H, W))
    zeros = float((m == 0).float().mean())
    assert 0.25 < zeros < 0.42 and bool(torch.signbit(m[m == 0]).any()) and not bool(torch.signbit(m[m == 0]).all())
    assert torch.equal(er.conv_epi_ref(x, wt, 1, 1, out_mask=m), c * (m == 1.0))


def test_windows_and_transposed_form():
    """Pixels outside a strided window keep y_prev bit for bit; the transposed form is F.conv_transpose2d with zero rows / columns beyond it."""
    rs = np.random.RandomState(9)
    wt = torch.from_numpy((rs.randn(20, 12, 2, 1) / 5.0).astype(np.float32))
    x = torch.from_numpy(rs.randn(2, 12, 8, 8).astype(np.float32))
    prev = torch.from_numpy(rs.randn(2, 20, 17, 17).astype(np.float32))
    got = er.conv_epi_ref(x, wt, 1, (1, 0), step=2, off=(0, 1), y_prev=prev, out_gain=0.5)
    win = er.window(prev.shape, 2, (0, 1))
    assert torch.equal(got[:, :, ~win], D(prev)[:, :, ~win])
    assert torch.allclose(got[:, :, 0::2, 1::2], 0.5 * F.conv2d(D(x), D(wt), padding=(1, 0)), rtol=0, atol=1e-12)
    w3 = torch.from_numpy((rs.randn(20, 12, 3, 3) / 10.0).astype(np.float32))
    got = er.conv_epi_ref(x, w3, 2, 1, transposed=True, y_prev=torch.zeros(2, 20, 16, 18), bias=torch.ones(20))
    nat = F.conv_transpose2d(D(x), D(w3).transpose(0, 1), stride=2, padding=1, output_padding=1)      # row / column 15 = 2*7 + 2 - 1 is still reached
    assert nat.shape[2:] == (16, 16) and float(nat[:, :, 15].abs().max()) > 0 and torch.allclose(got[:, :, :, :16], nat + 1.0, rtol=0, atol=1e-12)
    assert torch.equal(got[:, :, :, 16:], torch.ones(2, 20, 16, 2, dtype=torch.float64))
    # ... which makes it the input gradient of the stride-2 conv whose input has that size
    xr = torch.zeros(2, 20, 16, 16, dtype=torch.float64, requires_grad=True)
    gref, = torch.autograd.grad(F.conv2d(xr, D(w3).transpose(0, 1), stride=2, padding=1), xr, D(x))
    assert torch.allclose(er.conv_epi_ref(x, w3, 2, 1, transposed=True, y_prev=torch.zeros(2, 20, 16, 16)), gref, rtol=0, atol=1e-12)


@pytest.mark.parametrize('name,mistake', [(n, m) for n, (_, ms) in er.CASES.items() for m in ms])
def test_each_case_sees_the_mistake_it_is_aimed_at(name, mistake):
    """The mistake, made in the reference, moves the result by more than 100x the loosest family bound on the case's own inputs."""
    fields = er.case_fields(name)
    wt, x, kw, y_prev = _problem(sorted(er.CASES).index(name), fields)
    good = er.conv_epi_ref(x, wt, 1, 1, y_prev=y_prev, **kw)
    bad = er.conv_epi_ref(x, wt, 1, 1, y_prev=y_prev, _mistake=mistake, **kw)
    moved = float((bad - good).abs().max() / good.abs().max())
    assert moved > 100 * LOOSEST_BOUND, (name, mistake, moved)


def test_every_combination_names_a_mistake_and_every_mistake_has_a_case():
    assert all(ms for _, ms in er.COMBO_CASES.values())
    assert {m for _, ms in er.CASES.values() for m in ms} == set(er.MISTAKES)
    for name, (fields, _) in er.CASES.items():
        assert all(f in er.FIELDS or f in er.MODIFIERS for f in fields), name


def test_everything_case_is_well_formed():
    f = er.everything(set(er.FIELDS))
    assert 'in_mask' in f and 'relu_in' not in f and 'lrelu' in f and 'relu' not in f and 'sq' in f
    assert er.everything({'in_scale', 'res_mask', 'res_sub', 'out_gain'}) == ('in_scale', 'out_gain')
    assert er.runs_on(('residual', 'neg_residual'), {'residual'}) and not er.runs_on(('residual', 'res_mask'), {'residual'})
