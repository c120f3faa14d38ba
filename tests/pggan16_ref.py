"""Float64 model of l2i_pixelnorm_act_h8 / l2i_pixelnorm_act_bwd_h8 (include/l2i.h, csrc/l2i_pggan_h8.hip) on inputs already rounded to the 16-bit
element type, the bounds the kernels are held to, a numpy float32 restatement of the kernels' arithmetic, and the table of planted mistakes.
tests/test_pggan16_ref_cpu.py pins the bounds and the table on the CPU, tests/test_pggan16_kernels_gpu.py holds the kernels to them.

Arrays are logical NCHW [B, C, H, W]; to_h8 / from_h8 restate the h8 layout [B, C/8, H, W, 8].

    forward    y  = lrelu(x / sqrt(mean_c x^2 + eps), slope)                       (up = 2: every result at its four positions)
    backward   dx = r g' - x r^3 sum_c(g' x) / C,  r = 1 / sqrt(mean_c x^2 + eps),  g' = g (x > 0 ? 1 : slope),
               g  = gy (pool = 2: the sum of gy's 2x2 window) + addend

The bounds are derived by counting roundings, not measured.  u = 2^-24 (fp32), u_h = 2^-11 (fp16) or 2^-8 (bf16).
  forward    |got - y| <= u_h |y| + k_f(C) u |y|  (+ 2^-25 for fp16: half the subnormal quantum of the store)
             k_f(C) = C / 2 + 8.  The sum of C squares has C roundings of products and C - 1 of additions on positive terms: relative error
             <= C u in any order.  / C and + eps add 2 u; the square root halves all that and adds its own rounding (counted 2 u: one ulp);
             the division x / r (2 u) and the slope product (u) follow: (C + 2) / 2 + 2 + 2 + 1 <= C / 2 + 6, and 2 more for the second-order
             term u_h k_f u of the final rounding and the fused multiply-adds a compiler may or may not form.
  backward   |got - dx| <= u_h |dx| + k_b(C) u A  (+ 2^-25 for fp16),  A = r sum|g' terms| + |x| r^3 sum_c |g' x| / C
             A is the result with every term replaced by its absolute value (dx cancels, so the error scales with A and not with |dx|).
             k_b(C) = 5 C / 2 + 32.  r carries C / 2 + 6 as above (reciprocal instead of division).  First term: g has at most 3 additions
             (window, addend) and the slope product, then r g': C / 2 + 11.  Second term: r^3 is 3 (C / 2 + 6) + 2; sum_c g' x has 4 u per g',
             u per product and C - 1 additions in any order, against sum |g' x|: C + 4; / C (2 u), x k (u) and the subtraction (u on A):
             5 C / 2 + 28 in all, 4 more as above.  The 2^-25 is the forward's: dx goes through the same fp16 store, and below 2^-14 that store
             rounds to a fixed quantum of 2^-24, so no bound relative to |dx| can hold there (dx cancels and does reach subnormals).
"""
import numpy as np
import torch

DTYPES = ('f16', 'bf16')
TORCH = {'f16': torch.float16, 'bf16': torch.bfloat16}
U = 2.0 ** -24
UH = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}
EPS = 1e-8
SLOPE = 0.2

# (B, C, H, W): the widest column with fewer pixels than a wave; one pixel past a wave and an odd width; several full blocks; one slot per wave;
# slot counts below four and not divisible by four (the narrow path), a single pixel
SHAPES = ((2, 512, 4, 4), (1, 256, 5, 13), (2, 128, 16, 16), (1, 64, 32, 32), (1, 32, 3, 5), (3, 24, 2, 2), (1, 8, 1, 1))
MISTAKES = ('mean_over_padded_c', 'eps_dropped', 'mask_from_gy_sign', 'pool_as_mean', 'sum_term_dropped', 'rounded_twice')
FWD_MISTAKES = ('mean_over_padded_c', 'eps_dropped', 'rounded_twice')


def k_f(ch):
    return 0.5 * ch + 8.0


def k_b(ch):
    return 2.5 * ch + 32.0


def round16(a, dt):
    """Round a float array to the element type (through float32, nearest even) -> float32."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(TORCH[dt]).float().numpy()


def to_h8(a):
    """[B, C, H, W] -> [B, C/8, H, W, 8]: channel 8 g + e of a pixel at [g][h][w][e]."""
    b, ch, h, w = a.shape
    assert ch % 8 == 0
    return np.ascontiguousarray(a.reshape(b, ch // 8, 8, h, w).transpose(0, 1, 3, 4, 2))


def from_h8(a):
    b, g8, h, w, _ = a.shape
    return np.ascontiguousarray(a.transpose(0, 1, 4, 2, 3).reshape(b, g8 * 8, h, w))


def up2(a):
    return a.repeat(2, axis=2).repeat(2, axis=3)


def pool2(a):
    return (a[:, :, 0::2, 0::2] + a[:, :, 0::2, 1::2]) + (a[:, :, 1::2, 0::2] + a[:, :, 1::2, 1::2])


def make_case(shape, dt, kind='mixed', seed=0):
    """x, gy1 (1x), gy2 (2x), addend, all rounded to the element type.  'mixed': N(0, 1) with a tenth of the entries exactly zero and, where the map
    has more than one pixel, one all-zero column (the gradients around it are small: dx = g' / sqrt(eps) = 1e4 g' there must stay inside
    fp16); 'big' (fp16's range): |x| in [2^14, 2^16)."""
    b, ch, h, w = shape
    rng = np.random.RandomState(1000 * seed + 7 * ch + h * w + (3 if dt == 'f16' else 0))
    x = rng.standard_normal((b, ch, h, w))
    if kind == 'big':
        x = np.sign(x) * 2.0 ** 15 * rng.uniform(0.5, 1.9, x.shape)
    else:
        x[rng.uniform(size=x.shape) < 0.1] = 0.0
    gy1 = 0.5 * rng.standard_normal((b, ch, h, w))
    gy2 = 0.5 * rng.standard_normal((b, ch, 2 * h, 2 * w))
    add = 0.5 * rng.standard_normal((b, ch, h, w))
    for a in (gy1, gy2, add):
        a[rng.uniform(size=a.shape) < 0.1] = 0.0
    zero = None
    if kind == 'mixed' and b * h * w > 1:
        zero = (b - 1, h - 1, w // 2)
        zb, zh, zw = zero
        x[zb, :, zh, zw] = 0.0
        gy1[zb, :, zh, zw] *= 0.125
        add[zb, :, zh, zw] *= 0.125
        gy2[zb, :, 2 * zh:2 * zh + 2, 2 * zw:2 * zw + 2] *= 0.125
    return dict(x=round16(x, dt), gy1=round16(gy1, dt), gy2=round16(gy2, dt), addend=round16(add, dt), zero=zero, shape=shape, dt=dt)


def _mean_sq(x, mistake):
    ch = x.shape[1]
    div = (ch + 31) // 32 * 32 if mistake == 'mean_over_padded_c' else ch
    return (x * x).sum(1, keepdims=True) / div


def pixelnorm_act(x, dt, slope=SLOPE, eps=EPS, mistake=None):
    """-> y [B, C, H, W] float64 (the 1x map; the 2x map is up2 of it).  With a mistake: what the faulty kernel would store."""
    assert mistake in (None,) + MISTAKES
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        y = x / np.sqrt(_mean_sq(x, mistake) + (0.0 if mistake == 'eps_dropped' else eps))
        if mistake == 'rounded_twice':
            y = round16(y, dt).astype(np.float64)
        y = np.where(y > 0, y, y * slope)
        if mistake == 'rounded_twice':
            y = round16(y, dt).astype(np.float64)
    return y


def fwd_bound(y, dt):
    ch = y.shape[1]
    return UH[dt] * np.abs(y) + k_f(ch) * U * np.abs(y) + (2.0 ** -25 if dt == 'f16' else 0.0)


def pixelnorm_act_bwd(gy, x, dt, pool=1, addend=None, slope=SLOPE, eps=EPS, mistake=None):
    """-> dict(dx, A): the exact float64 gradient on these inputs and its absolute-term companion (module docstring)."""
    assert mistake in (None,) + MISTAKES and pool in (1, 2)
    x = np.asarray(x, dtype=np.float64)
    gy = np.asarray(gy, dtype=np.float64)
    ch = x.shape[1]
    g, absg = (pool2(gy), pool2(np.abs(gy))) if pool == 2 else (gy, np.abs(gy))
    if mistake == 'pool_as_mean' and pool == 2:
        g = g / 4
    if addend is not None:
        g, absg = g + np.asarray(addend, dtype=np.float64), absg + np.abs(addend)
    if mistake == 'rounded_twice':
        g = round16(g, dt).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        fac = np.where((g > 0) if mistake == 'mask_from_gy_sign' else (x > 0), 1.0, slope)
        gp, absgp = g * fac, absg * fac
        r = 1.0 / np.sqrt(_mean_sq(x, mistake) + (0.0 if mistake == 'eps_dropped' else eps))
        s = 0.0 if mistake == 'sum_term_dropped' else (gp * x).sum(1, keepdims=True)
        dx = r * gp - x * r ** 3 * s / ch
        a = r * absgp + np.abs(x) * r ** 3 * np.abs(gp * x).sum(1, keepdims=True) / ch
        if mistake == 'rounded_twice':
            dx = round16(dx, dt).astype(np.float64)
    return dict(dx=dx, A=a)


def bwd_bound(ref, dt):
    ch = ref['dx'].shape[1]
    return UH[dt] * np.abs(ref['dx']) + k_b(ch) * U * ref['A'] + (2.0 ** -25 if dt == 'f16' else 0.0)


def share(got, ref, bound):
    """Worst |got - ref| as a share of its bound; a NaN or an infinity that the model does not have counts as infinitely far out."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        q = np.abs(got - ref) / (bound + np.finfo(np.float64).tiny)
    q = np.where(np.isfinite(got) | ~np.isfinite(ref), q, np.inf)
    return float(np.nan_to_num(q, nan=np.inf).max())


# ---- the kernels' arithmetic in numpy float32 ------------------------------------------------------------------------------------------------
def _column_sum(terms, order):
    """Sum [B, C, H, W] float32 terms over C in float32.  'kernel': csrc/l2i_pggan_h8.hip's order (C >= 32: wave w takes the slots w, w + 4, ..
    ascending, eight channels of a slot ascending, then ((w0 + w1) + w2) + w3; fewer than four slots: ascending); 'ascending' / 'descending'."""
    b, ch, h, w = terms.shape
    f32 = np.float32
    if order == 'kernel' and ch >= 32:
        parts = []
        for wave in range(4):
            acc = np.zeros((b, h, w), f32)
            for s in range(wave, ch // 8, 4):
                for e in range(8):
                    acc = acc + terms[:, 8 * s + e]
            parts.append(acc)
        return (((parts[0] + parts[1]) + parts[2]) + parts[3])[:, None]
    acc = np.zeros((b, h, w), f32)
    for c in (range(ch - 1, -1, -1) if order == 'descending' else range(ch)):
        acc = acc + terms[:, c]
    return acc[:, None]


def fwd_float32(x, dt, slope=SLOPE, eps=EPS, order='kernel'):
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    r = np.sqrt(_column_sum(x * x, order) / f32(x.shape[1]) + f32(eps))
    t = x / r
    return round16(np.where(t > 0, t, t * f32(slope)), dt)


def bwd_float32(gy, x, dt, pool=1, addend=None, slope=SLOPE, eps=EPS, order='kernel'):
    f32 = np.float32
    x, gy = np.asarray(x, dtype=f32), np.asarray(gy, dtype=f32)
    ch = f32(x.shape[1])
    g = pool2(gy) if pool == 2 else gy
    if addend is not None:
        g = g + np.asarray(addend, dtype=f32)
    gp = np.where(x > 0, g, g * f32(slope))
    r = f32(1.0) / np.sqrt(_column_sum(x * x, order) / ch + f32(eps))
    k = r * r * r * _column_sum(gp * x, order) / ch
    return round16(r * gp - x * k, dt)


# ---- the generator with its storage rounding --------------------------------------------------------------------------------------------------
def _pn_act(x):
    import torch.nn.functional as F
    return F.leaky_relu(x / torch.sqrt(torch.mean(x * x, dim=1, keepdim=True) + EPS), SLOPE)


def _stored(R, t):
    """A map the GPU stores whose 1x gradient it never stores (the fused pool sums it in fp32): rounded (and perturbed) forward, gradient untouched."""
    keep, R.gradq = R.gradq, False
    try:
        return R.q(t, 'G')
    finally:
        R.gradq = keep


def _grad_stored(R, t):
    """A map whose forward values need no rounding of their own (copies of stored values, or an fp32 image) but whose gradient the GPU stores in h8."""
    from tests import inversion16_ref as I16
    return I16._GradQ.apply(t, R.T, 2.0 ** R.log2.get('G', 0)) if (R.T is not None and R.gradq) else t


def generator_forward(P, z, step, alpha, R):
    """oracle/pggan.generator_forward (label 0) with the storage rounding of nets16.PGGenerator restated through tests/inversion16_ref.Rounding:
    the scaled 3x3 conv weights and the to_rgb weights through R.w; every map the GPU stores through R.q(.., 'G') — the h8 copy of the 4x4 stage's
    fp32 output, every conv output after its bias, every PixelNorm + LeakyReLU output; the upsampled block output and the to_rgb outputs carry a
    stored (h8) gradient only.  The restructurings of the product are kept (to_rgb before the upsample; alpha = 0 skips the last block): they
    decide WHICH maps are stored."""
    import math

    import torch.nn.functional as F

    def econv(name, x):
        w = P[name + '.conv.weight_orig']
        return F.conv2d(x, R.w(w * math.sqrt(2.0 / (w.shape[1] * w.shape[2] * w.shape[3]))), P[name + '.conv.bias'], padding=1)

    def rgb(i, t):
        return _grad_stored(R, F.conv2d(t, R.w(P['to_rgb.%d.weight' % i]))) + P['to_rgb.%d.bias' % i].reshape(1, -1, 1, 1)

    x = z / torch.sqrt(torch.mean(z * z, dim=1, keepdim=True) + EPS)
    x = torch.cat([x, P['label_embed.weight'][0:1].expand(z.shape[0], -1)], 1).unsqueeze(2).unsqueeze(3)
    blend = step > 0 and 0 <= alpha < 1
    last = step - 1 if (blend and alpha == 0) else step
    two = blend and alpha != 0
    up = prev = out = None
    for i in range(last + 1):
        if i == 0:
            w0 = P['progression.0.conv.0.conv.weight_orig']
            a1 = R.q(F.conv2d(x, w0 * math.sqrt(2.0 / (w0.shape[1] * 16)), P['progression.0.conv.0.conv.bias'], padding=3), 'G')      # fp32 GEMM, then the cast
        else:
            a1 = R.q(econv('progression.%d.conv.0' % i, up), 'G')
        h1 = R.q(_pn_act(a1), 'G')
        a2 = R.q(econv('progression.%d.conv.3' % i, h1), 'G')
        if i == last:
            out = R.q(_pn_act(a2), 'G')
        else:
            o = _stored(R, _pn_act(a2))
            if two and i == last - 1:
                prev = _grad_stored(R, o)
            up = _grad_stored(R, F.interpolate(o, scale_factor=2, mode='nearest'))
    if not blend:
        return rgb(step, out)
    if alpha == 0:
        return F.interpolate(rgb(step - 1, out), scale_factor=2, mode='nearest')
    return (1 - alpha) * F.interpolate(rgb(step - 1, prev), scale_factor=2, mode='nearest') + alpha * rgb(step, out)


GEN_SETTINGS = ((2, 0.0), (2, 0.4), (2, -1), (0, 0.0), (1, 1.0))          # (step, alpha): alpha = 0 skip, a blended last block, plain to_rgb, the 4x4 stage, alpha = 1
# G exponents of the settings under the probe loss sum(img * probe): tools/probe_pggan16.py (profiles/pggan16_gradient_ranges.txt), 5 - round(log2 largest map)
GEN_LOG2 = {(2, 0.0): 3, (2, 0.4): 4, (2, -1): 3, (0, 0.0): 5, (1, 1.0): 4}


def generator_inputs():
    from latent2im_amd import synth
    P = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.pggan_generator_state(seed=11).items()}
    z = torch.from_numpy(synth.z_sample(2, seed=3)[:, :511]).double()
    return P, z


def generator_probe(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)


def measure_generator(P, z, step, alpha, dt):
    """inversion16_ref.measure on the z gradient of sum(img * probe), and the image figure measured the same way: max |delta| over the largest
    pixel — spread (three perturbed runs against the unperturbed model), and the model's distance to the exact image."""
    from tests import inversion16_ref as I16
    images = []

    def run(R):
        zz = z.clone().requires_grad_(True)
        img = generator_forward(P, zz, step, alpha, R)
        g, = torch.autograd.grad((img * generator_probe(img.shape)).sum(), zz)
        images.append(img.detach())
        return dict(grad_z=g)
    m = I16.measure(run, dt, log2={'G': GEN_LOG2[(step, alpha)]} if dt == 'f16' else None)
    base, exact, pert = images[0], images[1], images[3:]
    fig = lambda a, b: float((a - b).abs().max() / b.abs().max())
    m['image'] = dict(base=base, spread=max(fig(p, base) for p in pert), exact=fig(base, exact))
    return m


# ---- the whole config-1 step with its storage rounding -------------------------------------------------------------------------------------------
# The strong-walk case of tests/test_pggan_gpu.py at the graph's own size: seed-11 generator, walk_w0 x 50, regressor seed 300, VGG seed 400,
# no_gan_loss, content loss on; 256^2 (step 6, alpha 0), batch 2.  tests/golden/make_pggan16_step.py evaluates it into tests/golden/pggan16_step.npz.
STEP = dict(g_seed=11, r_seed=300, v_seed=400, z_seed=0, batch=2, walk_gain=50.0, alpha_delta=0.3, attr=31, step=6, alpha=0.0, resolution=256)
STEP_FIGURES = (('grad_w', 'rel_l2'), ('grad_w', 'one_minus_cos'), ('loss_reg', 'loss_rel'), ('loss_cont', 'loss_rel'))


def resnet50_q(PR, x, R):
    """oracle/nets16._resnet50_q with the folded conv weights rounded to R's element type (oracle.nets16._fold rounds to bfloat16 whatever the
    element type; the fp16 path stores fp16 weights) and every stored map through R.q(.., 'R').  The image is rounded where the stem kernel reads
    it, from an exact fp32 value (R.w); its gradient leaves the stem in fp32."""
    import torch.nn.functional as F
    from oracle.nets import RESNET50_LAYERS
    from oracle.nets16 import _fold
    q = lambda t: R.q(t, 'R')

    def fold(conv, bn):
        w, b = _fold(PR, conv, bn, round_w=False)
        return R.w(w), b
    w, b = fold('conv1', 'bn1')
    x = q(F.relu(F.conv2d(R.w(x), w, b, stride=2, padding=3)))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, (planes, blocks, stride) in enumerate(RESNET50_LAYERS):
        for bi in range(blocks):
            p = 'layer%d.%d' % (li + 1, bi)
            s = stride if bi == 0 else 1
            w1, b1 = fold(p + '.conv1', p + '.bn1')
            w2, b2 = fold(p + '.conv2', p + '.bn2')
            w3, b3 = fold(p + '.conv3', p + '.bn3')
            y1 = q(F.relu(F.conv2d(x, w1, b1)))
            y2 = q(F.relu(F.conv2d(y1, w2, b2, stride=s, padding=1)))
            idt = x
            if bi == 0:
                wd, bd = fold(p + '.downsample.0', p + '.downsample.1')
                idt = q(F.conv2d(x, wd, bd, stride=s))
            x = q(F.relu(F.conv2d(y2, w3, b3) + idt))
    x = F.adaptive_avg_pool2d(x, 1).flatten(1)
    return F.linear(x, PR['fc.weight'].double(), PR['fc.bias'].double())


def vgg19_taps_q(PV, img, R):
    """oracle/nets.vgg19_taps with the storage rounding of nets16.VGG19Prefix: 1 / std folded into conv1_1's weights, the four conv weights and the
    mean-subtracted image rounded to the element type (R.w), every conv output after its bias — the pre-ReLU map the GPU stores — through
    R.q(.., 'V').  The pooled map is a maximum of stored values."""
    import torch.nn.functional as F
    from oracle.nets import VGG_MEAN, VGG_STD
    mean = torch.tensor(VGG_MEAN, dtype=img.dtype).reshape(1, 3, 1, 1)
    std = torch.tensor(VGG_STD, dtype=img.dtype).reshape(1, 3, 1, 1)
    q = lambda t: R.q(t, 'V')
    c1 = q(F.conv2d(R.w(img - mean), R.w((PV['0.weight'].float() / std.float()).to(img.dtype)), PV['0.bias'], padding=1))
    c2 = q(F.conv2d(F.relu(c1), R.w(PV['2.weight']), PV['2.bias'], padding=1))
    c3 = q(F.conv2d(F.max_pool2d(F.relu(c2), 2, 2), R.w(PV['5.weight']), PV['5.bias'], padding=1))
    c4 = q(F.conv2d(F.relu(c3), R.w(PV['7.weight']), PV['7.bias'], padding=1))
    return [c1, c2, c3, c4]


def step_inputs():
    """-> (P, PR, PV, z, walk0) float64 of the STEP case."""
    import os

    from latent2im_amd import synth
    from oracle import step as ostep
    dt = torch.float64
    P = {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in synth.pggan_generator_state(seed=STEP['g_seed']).items()}
    PR, PV = ostep.to_torch(synth.resnet50_state(seed=STEP['r_seed']), dt), ostep.to_torch(synth.vgg19_prefix_state(seed=STEP['v_seed']), dt)
    z = torch.from_numpy(np.asarray(synth.z_sample(STEP['batch'], seed=STEP['z_seed']))).to(dt)
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pggan.npz'), allow_pickle=False)
    walk0 = torch.from_numpy(np.asarray(golden['walk_w0'])).to(dt) * STEP['walk_gain']
    return P, PR, PV, z, walk0


def step_forward(P, PR, PV, z, walk0, R):
    """The step of pggan.walk_training_step up to the walk gradient on the rounding model (R = Rounding(None): the exact float64 step of
    oracle/pggan.py + oracle/nets.py + oracle/step.py).  -> dict(grad_w, loss_reg, loss_cont, loss_total, taps_sq): names as
    inversion16_ref.measure reads them; taps_sq = per tap the mean of a^2 + b^2 over the two images' maps (the content term's absolute-size rule)."""
    import torch.nn.functional as F
    from oracle import pggan as opg
    from oracle import step as ostep

    def logits(zz):
        img = generator_forward(P, zz[:, :511], STEP['step'], STEP['alpha'], R)
        return F.interpolate(img, size=(img.shape[2] // 2, img.shape[3] // 2), mode='bilinear', align_corners=False)       # fp32 on the GPU: not rounded
    with torch.no_grad():
        x0 = logits(z)
        a0 = resnet50_q(PR, x0, R)[:, [STEP['attr']]]
        fo = vgg19_taps_q(PV, x0, R)
    target, eps = ostep.get_alphas_clamp(a0, torch.full((z.shape[0], 1), STEP['alpha_delta'], dtype=z.dtype))
    walk = walk0.detach().clone().requires_grad_(True)
    x1 = logits(opg.walk_linear_z_free(z, eps, walk))
    reg = opg.reg_loss_quirk(resnet50_q(PR, x1, R)[:, [STEP['attr']]], target)
    fs = vgg19_taps_q(PV, x1, R)
    cont = sum(F.mse_loss(a.detach(), b) for a, b in zip(fo, fs)) / len(fo)
    loss = opg.total_loss(reg, cont, None, no_content_loss=False, no_gan_loss=True)
    grad, = torch.autograd.grad(loss, walk)
    taps_sq = torch.stack([(a.detach() ** 2 + b.detach() ** 2).mean() for a, b in zip(fo, fs)])
    return dict(grad_w=grad, loss_reg=reg.detach().reshape(1), loss_cont=cont.detach().reshape(1), loss_total=loss.detach().reshape(1),
                image=x1.detach(), taps_sq=taps_sq)


def angle(one_minus_cos):
    """1 - cos -> the angle in radians.  Angles obey the triangle inequality on the sphere, 1 - cos does not: the step test adds angles."""
    return float(np.arccos(np.clip(1.0 - one_minus_cos, -1.0, 1.0)))
