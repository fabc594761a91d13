"""Float64 references of the BatchNorm chain (csrc/batchnorm.hip) and of the statistics rows its producers write
(csrc/conv3d.hip, csrc/lateral.hip, csrc/window_shift.hip), in plain torch on the CPU, and the generators of the inputs
of tests/test_gpu_bn_kernels.py.  tests/test_bn_ref_cpu.py pins both: the references against F.batch_norm and its
autograd in double, the inputs against the preconditions the GPU tests rely on.  Never imported by the package.

Every reference takes the operands the kernel sees (fp32 or bf16 values, as float64) and works in float64 throughout.
Per-level tables are [L, C]; activations of a level are [m, C].

Exactly summable operands (the statistics producers, the 512 * 512 + 37 level of the backward kernels): small integers
and dyadic coefficients, so that every partial sum in any order is an integer multiple of a stated power of two below
2^24 times that power: fp32 addition is then exact whatever the order, and the kernel's rows must EQUAL float64.
`exact_ok` is that precondition."""
import functools

import torch
import torch.nn.functional as F

U22 = 2.0 ** -22
U24 = 2.0 ** -24
DBL = 2.0 ** -45    # a few hundred double ulps: the device's double sqrt / divide / sums (kernel_util docstring)
EPS = float(torch.tensor(1e-5, dtype=torch.float32))   # the float the kernels get, as a double
MOMENTUM = 0.1


def rnd(t, prec):
    """The operand as the kernel sees it (fp32 or bf16 values), in float64."""
    return (t.float().bfloat16() if prec == 'bf16' else t.float()).double()


# ----------------------------------------------------------------------------------------------- references
def finalize(parts, counts, gamma, beta, eps=EPS):
    """sfvos_bn_finalize.  parts: per level the fp32 rows [rows, 2, C]; counts: values per channel and level.
    The kernel's formula: var = s2 / count - m^2 clamped at 0.  Also returns what the allowances need: the magnitudes of
    the sums and dv = 2^-45 * (s2 / count + m^2), by which the double arithmetic may move var."""
    out = {k: [] for k in ('mean', 'var', 'rstd', 'scale', 'shift', 'var_unbiased', 'a1', 'dv', 'rstd_lo', 'rstd_hi')}
    g, b = gamma.double(), beta.double()
    for p, n in zip(parts, counts):
        p = p.double()
        s1, s2, a1 = p[:, 0].sum(0), p[:, 1].sum(0), p[:, 0].abs().sum(0)
        m = s1 / n
        raw = s2 / n - m * m
        var = raw.clamp_min(0.0)
        dv = DBL * (s2.abs() / n + m * m)
        r = 1.0 / torch.sqrt(var + eps)
        out['mean'].append(m)
        out['var'].append(var)
        out['rstd'].append(r)
        out['rstd_lo'].append(1.0 / torch.sqrt((raw + dv).clamp_min(0.0) + eps))
        out['rstd_hi'].append(1.0 / torch.sqrt((raw - dv).clamp_min(0.0) + eps))
        out['scale'].append(g * r)
        out['shift'].append(b - m * (g * r))
        out['var_unbiased'].append(var * n / (n - 1.0) if n > 1 else var)
        out['a1'].append(a1 / n)
        out['dv'].append(dv)
    return {k: torch.stack(v) for k, v in out.items()}


def running(rm, rv, means, vars_unbiased, n, momentum=MOMENTUM):
    """sfvos_bn_running_update: n updates in order.  (1 - momentum) is the kernel's fp32 difference.  Returns the new
    running mean / var and their magnitudes (the same on absolute values)."""
    mom = float(torch.tensor(momentum, dtype=torch.float32))
    om = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(momentum, dtype=torch.float32))
    m, v = rm.double().clone(), rv.double().clone()
    am, av = m.abs(), v.abs()
    for i in range(n):
        m = om * m + mom * means[i].double()
        v = om * v + mom * vars_unbiased[i].double()
        am = om * am + mom * means[i].double().abs()
        av = om * av + mom * vars_unbiased[i].double().abs()
    return m, v, am, av


def apply(x, scale, shift, relu):
    """sfvos_bn_apply on one level: (y, mag)."""
    y = x * scale + shift
    return (y.clamp_min(0.0) if relu else y), (x * scale).abs() + shift.abs()


def ambiguous(x, scale, shift):
    """Elements whose ReLU mask fp32 `x * scale + shift > 0` (possibly one FMA) may differ from float64's: the value is
    within rounding of zero without being exactly zero (an exact zero is exact in fp32 too: the product equals -shift)."""
    v = x * scale + shift
    return (v != 0) & (v.abs() <= U22 * ((x * scale).abs() + shift.abs()))


def masked(dy, x, scale, shift, relu):
    """dz = dy where the ReLU passed (threshold_backward: gradient 0 where the output is 0, exact zeros included)."""
    return torch.where(x * scale + shift > 0, dy, torch.zeros_like(dy)) if relu else dy


def bwd_sums(dz, x, mean, rstd):
    """sfvos_bn_bwd_reduce on one level: (sum dz, sum dz * xhat) [2, C] and their magnitudes."""
    xh, axh = (x - mean) * rstd, (x.abs() + mean.abs()) * rstd
    return torch.stack([dz.sum(0), (dz * xh).sum(0)]), torch.stack([dz.abs().sum(0), (dz.abs() * axh).sum(0)])


def bwd_coeffs(sdz, sdzx, count, gamma, mean, rstd, train):
    """sfvos_bn_bwd_finalize: dx = cA * dz + cB * x + cK.  Train: dx = g * (dz - mean(dz) - xhat * mean(dz * xhat)) with
    g = gamma * rstd, xhat = (x - mean) * rstd; eval: dx = g * dz.  Returns (cA, cB, cK)."""
    g = gamma.double() * rstd
    if not train:
        return g, torch.zeros_like(g), torch.zeros_like(g)
    m1, m2 = sdz / count, sdzx / count
    return g, -g * m2 * rstd, g * m2 * rstd * mean - g * m1


def bwd_dx(dz, x, cA, cB, cK):
    """sfvos_bn_bwd_apply on one level: (dx, mag)."""
    return cA * dz + cB * x + cK, (cA * dz).abs() + (cB * x).abs() + cK.abs()


def exact_ok(values, unit=1.0, limit=2.0 ** 24):
    """values [n, C]: every value is an integer multiple of `unit` and, per column, the sum of the magnitudes is below
    limit * unit: every partial sum of a column, in any order and any partition, is exact in fp32."""
    q = values.double() / unit
    return bool((q == q.round()).all()) and float(q.abs().sum(0).max()) < limit


# ----------------------------------------------------------------------------------------------- BN-chain inputs
BN_LEVELS = [1, 37, 513, 759]            # one position; below one run; one run + 1; two runs, the second of 247
BN_CS = [32, 64, 192, 224, 256]
BIG_LEVELS = [512 * 512 + 37, 5]         # beyond BNB_MAX_ROWS: block 0 walks two runs; then a level after the cap
FIN_ROWS = [1, 31, 32, 33, 127, 128, 129, 400]     # rows per level: the 4 x 32 unroll of column_sum and both tails
FIN_COUNTS = [1, 640, 33, 700, 2000, 129, 5000, 1201]


def bwd_row_lanes(C, prec):
    """Row lanes of a bn_bwd block: 256 threads over C / (4 or 8) chunks."""
    return 256 // (C // (8 if prec == 'bf16' else 4))


def bwd_chain(C, prec):
    """Longest chain of fp32 additions into one partial row for levels of at most 512 * rows positions: a lane adds at
    most ceil(512 / rl) positions, then rl lanes are added through LDS."""
    rl = bwd_row_lanes(C, prec)
    return -(-512 // rl) + rl


def finalize_inputs(C, seed=3):
    """Partial rows of the eight FIN_ROWS levels from data x [count, C] cut into `rows` pieces (fp32 piece sums of float64
    sums), gamma, beta.  Channel 3 is constant (variance 0 or rounding-negative), channel 5 has a mean 1000 x its standard
    deviation.  Level 0: one value per channel."""
    g = torch.Generator().manual_seed(seed + C)
    gamma = (torch.rand(C, generator=g) + 0.5).float()
    beta = (torch.randn(C, generator=g) * 0.2).float()
    parts = []
    for l, (rows, n) in enumerate(zip(FIN_ROWS, FIN_COUNTS)):
        x = torch.randn(n, C, generator=g, dtype=torch.float64) * (0.5 + 0.3 * l) + 0.1 * l
        x[:, 3] = 1.7
        x[:, 5] = (0.5 + 0.3 * l) * (1000.0 + torch.randn(n, generator=g, dtype=torch.float64))
        x = x.float().double()
        piece = torch.arange(n) * rows // n
        s = torch.zeros(rows, 2, C, dtype=torch.float64)
        s[:, 0].index_add_(0, piece, x)
        s[:, 1].index_add_(0, piece, x * x)
        parts.append(s.float())
    return parts, FIN_COUNTS, gamma, beta


def bwd_inputs(C, prec, relu, seed=7, levels=BN_LEVELS):
    """x, dy per level ([m, C] float64, values of `prec`), and float64-chosen per-level tables rounded to fp32: mean, rstd,
    scale = gamma * rstd, shift = beta - mean * scale, gamma.  |dy| in [0.5, 1.5]: the smallest non-zero |dz| is far
    above the bound of a level's sum.  Channel 1: shift = 0 and x = +-0.0 at every third position (gradient 0 there).
    Ambiguous elements (see `ambiguous`) get dy = 0; `n_amb` counts them per level and channel."""
    g = torch.Generator().manual_seed(seed + C)
    L = len(levels)
    gamma = (torch.rand(C, generator=g) + 0.5).float().double()
    mean = (torch.randn(L, C, generator=g) * 0.5).float().double()
    rstd = (1.0 / (0.5 + torch.rand(L, C, generator=g))).float().double()
    beta = torch.randn(C, generator=g) * 0.2
    scale = (gamma * rstd).float().double()
    shift = (beta - mean * scale).float().double()
    shift[:, 1] = 0.0
    xs, dys, n_amb = [], [], []
    for l, m in enumerate(levels):
        x = mean[l] + torch.randn(m, C, generator=g, dtype=torch.float64) / rstd[l]
        x[0::3, 1] = 0.0
        x[3::6, 1] = -0.0
        x = rnd(x, prec)
        dy = (0.5 + torch.rand(m, C, generator=g, dtype=torch.float64)) * \
            (torch.randint(0, 2, (m, C), generator=g) * 2 - 1)
        dy = rnd(dy, prec)
        amb = ambiguous(x, scale[l], shift[l]) if relu else torch.zeros_like(x, dtype=torch.bool)
        dy[amb] = 0.0
        xs.append(x)
        dys.append(dy)
        n_amb.append(amb.sum(0))
    return dict(x=xs, dy=dys, mean=mean, rstd=rstd, scale=scale, shift=shift, gamma=gamma, n_amb=n_amb)


@functools.lru_cache(maxsize=None)
def big_inputs(C=32, seed=23):
    """The 512 * 512 + 37 level and a 5-position level behind it, exactly summable: x in {-2..2}, dy in {-1, 0, 1}, integer
    mean in {-1, 0, 1}, rstd = 0.5, scale = 0.5, shift in {-0.25, 0, 0.25} (x * scale + shift is a multiple of 0.25: exact,
    never ambiguous), cA = 0.5, cB = 0.25, cK in {-1, 0, 1}.  dz * xhat is a multiple of 0.5, dx a multiple of 0.25.
    bf16 holds every value."""
    g = torch.Generator().manual_seed(seed)
    L = len(BIG_LEVELS)
    xs = [torch.randint(-2, 3, (m, C), generator=g).double() for m in BIG_LEVELS]
    dys = [torch.randint(-1, 2, (m, C), generator=g).double() for m in BIG_LEVELS]
    mean = torch.randint(-1, 2, (L, C), generator=g).double()
    shift = torch.randint(-1, 2, (L, C), generator=g).double() * 0.25
    cK = torch.randint(-1, 2, (L, C), generator=g).double()
    full = torch.full((L, C), 0.5, dtype=torch.float64)
    return dict(x=xs, dy=dys, mean=mean, rstd=full, scale=full.clone(), shift=shift, cA=full.clone(),
                cB=full * 0.5, cK=cK)


def bwd_finalize_inputs(C, seed=29):
    """Levels of 1, 400, 2 and 33 partial rows (5, 400 * 512 - 100, 700 and 33 * 512 positions) and random fp32 rows of the
    size pass 1 writes for them, gamma, mean, rstd."""
    levels = [5, 400 * 512 - 100, 700, 33 * 512]
    rows = [1, 400, 2, 33]
    g = torch.Generator().manual_seed(seed + C)
    parts = [(torch.randn(r, 2, C, generator=g) * (m / r) ** 0.5).float() for r, m in zip(rows, levels)]
    gamma = (torch.rand(C, generator=g) + 0.5).float().double()
    mean = (torch.randn(len(levels), C, generator=g) * 0.5).float().double()
    rstd = (1.0 / (0.5 + torch.rand(len(levels), C, generator=g))).float().double()
    return levels, rows, parts, gamma, mean, rstd


# ----------------------------------------------------------------------------------------------- statistics producers
def stats(v):
    """[B, C, T, H, W] -> (S1, S2) per channel, float64."""
    v = v.double()
    return v.sum((0, 2, 3, 4)), (v * v).sum((0, 2, 3, 4))


CONV_CASES = [
    # name            B   T  t_alloc t_off shapes                       cin cout kt taps  precisions
    ('fs 4+2+1',      1,  9,  9,  0, [(24, 42), (17, 48), (12, 21)], 256,  32,  3, 9, ('fp32', 'bf16')),  # tall / padded tiles
    ('fs two clips',  2,  8,  8,  0, [(40, 10), (3, 5)],              32,  32,  2, 9, ('fp32', 'bf16')),  # tall tiles only
    ('fs1',           1,  3,  3,  0, [(9, 33)],                       32,  32,  3, 9, ('bf16',)),         # conv3d_fs1
    ('wide TT3',      1,  4,  4,  0, [(12, 21)],                     256, 192,  2, 9, ('fp32', 'bf16')),
    ('wide ragged',   1,  3,  3,  0, [(9, 17), (5, 40)],             256, 224,  2, 9, ('fp32', 'bf16')),  # ragged channel block
    ('wide 128-tile', 1,  2,  2,  0, [(6, 33)],                      256, 256,  2, 9, ('bf16',)),         # one output frame
    ('mask head',    33,  1,  1,  0, [(7, 7)],                       256, 256,  1, 9, ('fp32', 'bf16')),
    ('mid 1x1',       1,  9,  9,  0, [(18, 16), (4, 35)],             32,  64,  5, 1, ('fp32', 'bf16')),  # t_out 5
    ('lateral t2',    2, 21, 21,  0, [(9, 13), (3, 3), (1, 2)],       32,  64, 20, 1, ('bf16',)),
    ('lateral t1',    1,  8,  8,  0, [(16, 33)],                      32,  64,  8, 1, ('bf16',)),
    ('lateral t3',    1, 22, 22,  0, [(24, 42), (12, 21), (6, 11)],   32,  64, 20, 1, ('bf16',)),
    ('lateral reg',   1, 41, 41,  0, [(7, 9)],                        32,  64, 41, 1, ('bf16',)),         # the register tap
    ('window inside', 2,  3,  7,  2, [(6, 10), (3, 7)],               64,  32,  2, 9, ('fp32', 'bf16')),  # t_offset > 0
    ('window beyond', 2,  7,  4, -2, [(6, 10), (3, 7)],               64,  32,  3, 9, ('fp32', 'bf16')),  # zero frames
    ('beyond, fs',    1,  9,  5, -1, [(12, 21), (5, 9)],             256,  32,  3, 9, ('fp32', 'bf16')),
]
CONV_NONZERO = 432.0    # non-zero weights per output channel, on average (1 in 16 of 256 x 27): sets the density


@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    """Integer operands of a CONV_CASES row and the float64 conv: x in {-1, 0, 1}, w in {-1, 0, 1} with about CONV_NONZERO
    non-zero weights per output channel, bias in {-2..2}.  Returns (xs [B, cin, t_alloc, H, W], w, bias, refs): refs per
    level is conv + bias before any ReLU, on the frame window [t_off, t_off + T) with zero frames outside the buffer."""
    case = next(c for c in CONV_CASES if c[0] == name)
    _, B, T, t_alloc, t_off, shapes, cin, cout, kt, taps, _ = case
    g = torch.Generator().manual_seed(101 + len(name) + cin + cout + kt)
    k = 3 if taps == 9 else 1
    density = min(1.0, CONV_NONZERO / (cin * kt * taps))
    w = torch.randint(0, 2, (cout, cin, kt, k, k), generator=g) * 2 - 1
    w = (w * (torch.rand(w.shape, generator=g) < density)).double()
    bias = torch.randint(-2, 3, (cout,), generator=g).double()
    xs = [torch.randint(-1, 2, (B, cin, t_alloc, H, W), generator=g).double() for (H, W) in shapes]
    refs = []
    for x in xs:
        win = torch.zeros(B, cin, T, x.shape[3], x.shape[4], dtype=torch.float64)
        for t in range(T):
            if 0 <= t_off + t < t_alloc:
                win[:, :, t] = x[:, :, t_off + t]
        refs.append(F.conv3d(win, w, bias, padding=(0, 1, 1) if taps == 9 else 0))
    return xs, w, bias, refs


def conv_mag(name):
    """Largest magnitude of any output of the case: conv of |x| with |w| plus |bias|."""
    case = next(c for c in CONV_CASES if c[0] == name)
    taps = case[9]
    xs, w, bias, _ = conv_inputs(name)
    t_off, T, t_alloc = case[4], case[2], case[3]
    worst = 0.0
    for x in xs:
        win = torch.zeros(x.shape[0], x.shape[1], T, x.shape[3], x.shape[4], dtype=torch.float64)
        for t in range(T):
            if 0 <= t_off + t < t_alloc:
                win[:, :, t] = x[:, :, t_off + t].abs()
        worst = max(worst, float(F.conv3d(win, w.abs(), bias.abs(), padding=(0, 1, 1) if taps == 9 else 0).max()))
    return worst


SHIFT_SHAPES = [(24, 42), (5, 9), (1, 1)]     # (24, 42): two runs per frame, the second of 496 positions
SHIFT_CASES = [
    # name        B  T   shapes          C    precisions
    ('c32',       2, 5,  SHIFT_SHAPES,   32,  ('fp32', 'bf16')),
    ('c192',      2, 5,  SHIFT_SHAPES,   192, ('fp32', 'bf16')),
    ('c256',      2, 5,  SHIFT_SHAPES,   256, ('fp32', 'bf16')),
    ('many runs', 2, 60, [(40, 52)],     32,  ('bf16',)),     # 600 runs > WS_MAX_ROWS = 512: workgroups walk two runs
]


@functools.lru_cache(maxsize=None)
def shift_inputs(name, s):
    """Integer frames in {-8..8} ({-2..2} for the many-runs case): prev [B, T, hw, C] and fresh [B, s, hw, C] per level."""
    _, B, T, shapes, C, _ = next(c for c in SHIFT_CASES if c[0] == name)
    g = torch.Generator().manual_seed(211 + C + T + s)
    a = 2 if name == 'many runs' else 8
    prev = [torch.randint(-a, a + 1, (B, T, h * w, C), generator=g).double() for h, w in shapes]
    fresh = [torch.randint(-a, a + 1, (B, s, h * w, C), generator=g).double() for h, w in shapes]
    return prev, fresh
