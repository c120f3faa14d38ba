"""Float64 model of the four fp32 entry points of csrc/l2i_pggan.hip (l2i_pixelnorm_act_f32, l2i_pixelnorm_act_bwd_f32, l2i_upsample2x_nearest_f32,
l2i_pool2x2_f32), the bounds they are held to, a numpy float32 restatement of the kernels' arithmetic, the rows and the planted mistakes.
tests/test_pggan32_ref_cpu.py pins the bounds and the table on the CPU, tests/test_pggan32_contract_gpu.py holds the kernels to them.

The formulas are tests/pggan16_ref.py's (pixelnorm_act, pixelnorm_act_bwd with pool = 1 and no addend), imported, on [B, C, HW] arrays:

    forward    y  = lrelu(x / sqrt(mean_c x^2 + eps), slope)
    backward   dx = r g' - x r^3 sum_c(g' x) / C,  r = 1 / sqrt(mean_c x^2 + eps),  g' = gy (x > 0 ? 1 : slope)

The bounds are pggan16_ref's with the 16-bit storage rounding u_h replaced by the one fp32 rounding of the last operation, u = 2^-24; they are
derived by counting roundings (pggan16_ref's docstring has the count), none is measured.
  forward    |got - y|  <= (k_f(C) + 1) u |y|,        k_f(C) = C / 2 + 8
  backward   |got - dx| <= u |dx| + k_b(C) u A,       k_b(C) = 5 C / 2 + 32,  A = r sum|g' terms| + |x| r^3 sum_c |g' x| / C
A NaN in one channel of one pixel makes that pixel's whole column NaN in y and dx (the sum over C carries it) and nothing else: the model has
NaN exactly there, and `split_nan` takes those elements out of the comparison after requiring the kernel's NaNs to sit where the model's do.

Upsample and pool have no bound: y = fl(x * scale) at the four positions, y = fl(scale * ((a + b) + (c + d))) with a, b the upper and c, d the
lower pair of the window — one product after exact-order sums, nothing for a compiler to contract — are compared bit for bit with `up_float32`
and `pool_float32`.

Launch geometry, restated from the entry points: l2i_grid_for(n, 256, 256 * 16) caps the grid at 4096 blocks of 256 threads, so more than
CAP = 1048576 work items (float4 groups or single pixels for PixelNorm, pairs of pixels for upsample and pool) run the grid-stride loop.
The PixelNorm pair takes 16-byte accesses when HW % 4 == 0 and every pointer is on a 16-byte boundary, single floats otherwise.

A plain module: no fixtures, no GPU, no kernel code."""
import collections

import numpy as np

from tests import pggan16_ref as R16

U = 2.0 ** -24
EPS = 1e-8
SLOPE = 0.2
CAP = 256 * 16 * 256                      # work items one pass of the capped grid covers
SCALES = (1.0, 0.25, 0.3)
MISTAKES = ('eps_dropped', 'mask_from_gy_sign', 'sum_term_dropped', 'zero_takes_one', 'mean_over_padded_c')
FWD_MISTAKES = ('eps_dropped', 'mean_over_padded_c')

k_f, k_b = R16.k_f, R16.k_b

# off = (y / dx, x, gy) element offsets of the base pointers from a 16-byte boundary; nan: one NaN in one channel of one pixel
Row = collections.namedtuple('Row', 'id B C HW slope off nan')
ROWS = (
    Row('latent_3x511x1', 3, 511, 1, 1.0, (0, 0, 0), False),
    Row('vec_2x512x16', 2, 512, 16, SLOPE, (0, 0, 0), True),
    Row('vec_1x37x36', 1, 37, 36, SLOPE, (0, 0, 0), False),                # 36 % 4 == 0: the vector path with an odd C; 1x37x35 is its scalar twin
    Row('scalar_hw_1x8x15', 1, 8, 15, SLOPE, (0, 0, 0), False),
    Row('scalar_hw_1x37x35', 1, 37, 35, SLOPE, (0, 0, 0), False),
    Row('off_y_2x16x64', 2, 16, 64, SLOPE, (1, 0, 0), False),
    Row('off_x_2x16x64', 2, 16, 64, SLOPE, (0, 1, 0), False),
    Row('off_both_2x16x64', 2, 16, 64, SLOPE, (1, 1, 1), False),
    Row('vec_cap_2x2x2097408', 2, 2, 2097408, SLOPE, (0, 0, 0), False),
    Row('scalar_cap_1x2x1048835', 1, 2, 1048835, SLOPE, (0, 0, 0), False),
)
BIG = ('vec_cap_2x2x2097408', 'scalar_cap_1x2x1048835')
# (planes, H, W) of the upsample's input and of the pool's output: one pair, an odd number of pairs per row, several blocks, past the cap
Map = collections.namedtuple('Map', 'id planes H W')
MAPS = (Map('1x1x2', 1, 1, 2), Map('6x4x6', 6, 4, 6), Map('4x16x16', 4, 16, 16), Map('3x37x130', 3, 37, 130), Map('cap_3x5x139812', 3, 5, 139812))
BIG_MAP = 'cap_3x5x139812'


def path(row):
    """'vector' or 'scalar', as the entry point decides."""
    return 'vector' if row.HW % 4 == 0 and not any(row.off) else 'scalar'


def work_items(row):
    return row.B * (row.HW // 4 if path(row) == 'vector' else row.HW)


def map_work_items(m):
    return m.planes * m.H * (m.W // 2)


def make_case(row, seed=0):
    """float32 x, gy [B, C, HW]: N(0, 1) and N(0, 1/4); a tenth of x exactly 0 with gy != 0 there; the last pixel's column all zero with its
    gradients scaled by 1/8 (r = 1 / sqrt(eps) = 1e4 there); the first pixel's column at 1e-5 magnitudes (mean square 1e-10 against eps = 1e-8);
    row.nan: NaN in channel C / 3 of pixel (0, 5), whose float4 holds the pixels 4..7.  -> dict(x, gy, zero, small, nan)."""
    rng = np.random.RandomState(1000 * seed + 7 * row.C + row.HW % 9973 + 3 * row.B)
    shape = (row.B, row.C, row.HW)
    x = rng.standard_normal(shape).astype(np.float32)
    gy = (0.5 * rng.standard_normal(shape)).astype(np.float32)
    gy[gy == 0] = 0.5
    x[rng.uniform(size=shape) < 0.1] = 0.0
    zero = small = nan = None
    if row.B * row.HW >= 2:
        zero = (row.B - 1, row.HW - 1)
        x[zero[0], :, zero[1]] = 0.0
        gy[zero[0], :, zero[1]] *= np.float32(0.125)
        small = (0, 0)
        x[0, :, 0] *= np.float32(1e-5)
    if row.nan:
        assert row.HW >= 8
        nan = (0, row.C // 3, 5)
        x[nan] = np.nan
    return dict(x=x, gy=gy, zero=zero, small=small, nan=nan)


def forward(row, case, mistake=None):
    """-> (y float64, bound)."""
    assert mistake in (None,) + MISTAKES
    y = R16.pixelnorm_act(case['x'], None, slope=row.slope, eps=EPS, mistake=mistake if mistake in FWD_MISTAKES else None)
    return y, (k_f(row.C) + 1.0) * U * np.abs(y)


def backward(row, case, mistake=None):
    """-> (dx float64, bound)."""
    assert mistake in (None,) + MISTAKES
    x, gy = case['x'].astype(np.float64), case['gy'].astype(np.float64)
    if mistake == 'zero_takes_one':                        # x == 0 gets the factor 1: the model's slope at that element undone
        gy = np.where(x == 0, gy / row.slope, gy)
        mistake = None
    ref = R16.pixelnorm_act_bwd(gy, x, None, pool=1, addend=None, slope=row.slope, eps=EPS, mistake=mistake)
    return ref['dx'], U * np.abs(ref['dx']) + k_b(row.C) * U * ref['A']


def split_nan(got, want, bound):
    """-> (where the NaNs of got are the NaNs of want, got, want, bound with those elements replaced by zeros)."""
    got = np.asarray(got, dtype=np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    z = lambda a: np.where(wn | gn, 0.0, a)
    return bool(np.array_equal(gn, wn)), z(got), z(want), z(bound)


def ratio(got, want, bound):
    """Worst |got - want| / bound; a NaN the model does not have (or lacks) counts as infinitely far out."""
    same, got, want, bound = split_nan(got, want, bound)
    if not same:
        return float('inf')
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.abs(got - want) / bound
    q = np.where(np.abs(got - want) == 0, 0.0, q)
    return float(np.nan_to_num(q, nan=np.inf, posinf=np.inf).max())


# ---- the kernels' arithmetic in numpy float32 -------------------------------------------------------------------------------------------------
def _column_sum(terms, order):
    acc = np.zeros(terms[:, 0].shape, np.float32)
    ch = terms.shape[1]
    for c in (range(ch) if order == 'kernel' else range(ch - 1, -1, -1)):
        acc = acc + terms[:, c]
    return acc[:, None]


def fwd_float32(row, case, order='kernel'):
    """Channels ascending ('kernel') or descending, sqrtf, then a division."""
    f32 = np.float32
    x = case['x']
    with np.errstate(invalid='ignore'):
        r = np.sqrt(_column_sum(x * x, order) / f32(row.C) + f32(EPS))
        t = x / r
        return np.where(t > 0, t, t * f32(row.slope))


def bwd_float32(row, case, order='kernel'):
    f32 = np.float32
    x, gy = case['x'], case['gy']
    with np.errstate(invalid='ignore'):
        gp = np.where(x > 0, gy, gy * f32(row.slope))
        r = f32(1.0) / np.sqrt(_column_sum(x * x, order) / f32(row.C) + f32(EPS))
        k = r * r * r * _column_sum(gp * x, order) / f32(row.C)
        return r * gp - x * k


def map_input(m, pool, seed=0):
    """float32 input of the upsample ([planes, H, W]) or of the pool ([planes, 2H, 2W]) with a tenth of exact zeros."""
    rng = np.random.RandomState(1000 * seed + 31 * m.planes + m.W % 9973 + (5 if pool else 0))
    shape = (m.planes, 2 * m.H, 2 * m.W) if pool else (m.planes, m.H, m.W)
    x = rng.standard_normal(shape).astype(np.float32)
    x[rng.uniform(size=shape) < 0.1] = 0.0
    return x


def up_float32(x, scale):
    return (x * np.float32(scale)).repeat(2, axis=1).repeat(2, axis=2)


def pool_float32(x, scale):
    return np.float32(scale) * ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2]))
