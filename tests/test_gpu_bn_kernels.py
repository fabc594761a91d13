"""GPU: the BatchNorm chain kernel by kernel through the C ABI -- the statistics rows written by sfvos_conv3d (conv3d.hip,
lateral.hip) and sfvos_shift_frames, then sfvos_bn_finalize, sfvos_bn_running_update, sfvos_bn_apply, sfvos_bn_bwd_reduce,
sfvos_bn_bwd_finalize and sfvos_bn_bwd_apply -- each fed float64-chosen inputs (never another kernel's output) and
compared with the float64 references of tests/bn_ref.py under the criteria of tests/kernel_util.py (its docstring):

    |got - ref|  <=  u_out * |ref|  +  2 * (K + 1) * 2^-22 * mag

with K stated beside each case and u_out = 0 for every statistics or partial row; `got == ref` where the operands are
exactly summable (bn_ref.exact_ok, asserted in tests/test_bn_ref_cpu.py: the accumulation term is then zero); the cast
plus the reference at var +- 2^-45 * (s2 / count + m^2) for rstd and what follows from it; ReLU masks within rounding
of zero get dy = 0 in the input instead of being left out.  Guard bands, sentinel-filled outputs, NaN-filled partial
buffers, pitches wider than C with the tested slice at a channel offset, coefficient tables with coef_stride > C."""
import ctypes

import pytest
import torch

import bn_ref as R
from kernel_util import (DT, PRECS, SENT, TDT, U22, U_OUT, Out, P, S, check, check_abs, check_exact, from_pyr, levels,  # noqa: F401
                         lib, make_desc, to_pyr)

pytestmark = pytest.mark.gpu

U24, DBL = R.U24, R.DBL
OFF = 32            # channel offset of the tested slice in an activation buffer
TOFF = 8            # ... in a coefficient table
NAN = float('nan')


def summary(kernel, worst):
    print('%-22s worst error/bound %.4f over %d checks' % (kernel, max(worst), len(worst)))


class Tables:
    """Per-level coefficient tables [L][cs] with cs > C: every table NaN-filled between guard bands, the values at
    column TOFF."""

    def __init__(self, L, C):
        self.L, self.C, self.cs, self.t = L, C, C + 24, {}

    def put(self, name, vals=None):
        o = Out((self.L, self.cs), torch.float32, fill=NAN)
        if vals is not None:
            o.t[:, TOFF:TOFF + self.C] = vals.float().cuda()
        self.t[name] = o
        return self.p(name)

    def p(self, name):
        return P(self.t[name].t, TOFF)

    def get(self, name):
        t = self.t[name].cpu()
        assert bool(torch.isnan(t[:, :TOFF]).all()) and bool(torch.isnan(t[:, TOFF + self.C:]).all()), \
            '%s: wrote outside its %d channels' % (name, self.C)
        return t[:, TOFF:TOFF + self.C].double()


def act_in(levels_, prec, C):
    """Levels [m, C] float64 -> device [M, C + 2 * OFF] of `prec` (7 elsewhere); the slice starts at column OFF."""
    flat = torch.full((sum(v.shape[0] for v in levels_), C + 2 * OFF), 7.0)
    flat[:, OFF:OFF + C] = torch.cat(levels_).float()
    return flat.to(TDT[prec]).cuda()


def act_out(M, prec, C):
    return Out((M, C + 2 * OFF), TDT[prec])


def act_get(o, C):
    t = o.cpu()
    assert bool((t[:, :OFF] == SENT).all()) and bool((t[:, OFF + C:] == SENT).all()), 'wrote outside its channel slice'
    return t[:, OFF:OFF + C].double()


def split(t, ms):
    return list(torch.split(t, ms))


def level_rows(part, rows_pl):
    """Per level the float64 sum of its rows (exact: a double holds any sum of < 2^29 floats of one binade range)."""
    return [p.double().sum(0) for p in torch.split(part, list(rows_pl))]


# ------------------------------------------------------------------------------------------ statistics producers
CONV_PARAMS = [(c[0], p) for c in R.CONV_CASES for p in c[10]]


@pytest.mark.parametrize('name,prec', CONV_PARAMS)
def test_conv3d_statistics_rows_and_y_are_exact_on_integer_operands(lib, name, prec):
    """Integer x, w and bias (bn_ref.conv_inputs): every partial sum is exact in fp32 in any order, so for each level and
    channel the float64 sum of the level's rows EQUALS S1 and S2 of the float64 conv, and y equals it too (bf16 holds
    |v| <= 256).  One dropped or doubled position, the ragged edge of a tile, changes S2 by at least 1.  The ReLU epilogue
    excludes statistics in this ABI (the entry point refuses the pair): its run checks y alone."""
    _, B, T, t_alloc, t_off, shapes, cin, cout, kt, taps, _ = next(c for c in R.CONV_CASES if c[0] == name)
    xs, w, bias, refs = R.conv_inputs(name)
    ld_x, ld_y = cin + 32, cout + 2 * OFF
    xd = to_pyr([x.float() for x in xs], prec, ld_x)
    d, t_out = make_desc(lib, prec, B, T, shapes, cin, cout, kt, taps, 0, ld_x, ld_y, t_alloc=t_alloc, t_offset=t_off)
    wp = torch.empty(w.numel(), dtype=TDT[prec], device='cuda')
    wd, bd = w.float().cuda(), bias.float().cuda()
    lib.call('sfvos_pack_weights_fwd', P(wd), P(wp), d.dtype, cout, cin, kt, taps, S())
    M = sum(B * t_out * H * W for H, W in shapes)
    rows_pl = (ctypes.c_int * lib.MAX_LEVELS)()
    rows = lib.load().sfvos_conv3d_stat_rows(ctypes.byref(d), rows_pl)
    assert rows > 0 and sum(rows_pl[:len(shapes)]) == rows and all(r > 0 for r in rows_pl[:len(shapes)])
    part = Out((rows, 2, cout), torch.float32, fill=NAN)
    y = act_out(M, prec, cout)
    lib.call('sfvos_conv3d', ctypes.byref(d), P(xd), P(wp), P(bd), P(y.t, OFF), P(part.t), S())
    torch.cuda.synchronize()
    got = from_pyr(act_get(y, cout), B, cout, t_out, shapes)
    sums = level_rows(part.cpu(), rows_pl[:len(shapes)])
    for l, ref in enumerate(refs):
        check_exact('conv %s %s y level %d' % (name, prec, l), got[l], ref)
        s1, s2 = R.stats(ref)
        check_exact('conv %s %s S1 level %d' % (name, prec, l), sums[l][0], s1)
        check_exact('conv %s %s S2 level %d' % (name, prec, l), sums[l][1], s2)
    d.relu = 1
    assert lib.load().sfvos_conv3d(ctypes.byref(d), P(xd), P(wp), P(bd), P(y.t, OFF), P(part.t), S()) != 0
    y = act_out(M, prec, cout)
    lib.call('sfvos_conv3d', ctypes.byref(d), P(xd), P(wp), P(bd), P(y.t, OFF), None, S())
    torch.cuda.synchronize()
    got = from_pyr(act_get(y, cout), B, cout, t_out, shapes)
    for l, ref in enumerate(refs):
        check_exact('conv %s %s relu y level %d' % (name, prec, l), got[l], ref.clamp_min(0.0))


SHIFT_PARAMS = [(c[0], p) for c in R.SHIFT_CASES for p in c[5]]


@pytest.mark.parametrize('name,prec', SHIFT_PARAMS)
def test_shift_frames_statistics_rows_are_exact_on_integer_frames(lib, name, prec):
    """Integer frames: out is the shifted copy, and per level and channel the float64 sum of the level's rows EQUALS S1 and
    S2 of the copied values, for s = 1 and s = T - 1.  `many runs`: 600 runs on 512 workgroups."""
    _, B, T, shapes, C, _ = next(c for c in R.SHIFT_CASES if c[0] == name)
    pyr = lib.make_pyramid(shapes)
    rows_pl = (ctypes.c_int * lib.MAX_LEVELS)()
    rows = lib.load().sfvos_shift_frames_stat_rows(ctypes.byref(pyr), B, T, C, rows_pl)
    assert rows > 0 and sum(rows_pl[:len(shapes)]) == rows
    if name == 'many runs':
        assert rows == 512 and B * T * -(-shapes[0][0] * shapes[0][1] // 512) == 600
    ld = C + 2 * OFF
    for s in (1, T - 1):
        prev, fresh = R.shift_inputs(name, s)
        pd, fd = act_in([p.reshape(-1, C) for p in prev], prec, C), act_in([f.reshape(-1, C) for f in fresh], prec, C)
        out = act_out(pd.shape[0], prec, C)
        part = Out((rows, 2, C), torch.float32, fill=NAN)
        lib.call('sfvos_shift_frames', P(pd, OFF), P(fd, OFF), P(out.t, OFF), DT(lib, prec), ctypes.byref(pyr), B, T, s, C,
                 ld, P(part.t), S())
        torch.cuda.synchronize()
        got = split(act_get(out, C), [p.numel() // C for p in prev])
        sums = level_rows(part.cpu(), rows_pl[:len(shapes)])
        for l, (p, f) in enumerate(zip(prev, fresh)):
            want = torch.cat([p[:, s:], f], 1).reshape(-1, C)
            check_exact('shift %s %s s %d out level %d' % (name, prec, s, l), got[l], want)
            check_exact('shift %s %s s %d S1 level %d' % (name, prec, s, l), sums[l][0], want.sum(0))
            check_exact('shift %s %s s %d S2 level %d' % (name, prec, s, l), sums[l][1], (want * want).sum(0))


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('C', [32, 224])
def test_bn_finalize(lib, C):
    """Eight levels of 1, 31, 32, 33, 127, 128, 129 and 400 random fp32 rows (the 4 x 32 unroll of column_sum and both its
    tails), count 1 in level 0, a constant channel (variance clamped) and one with mean = 1000 x its standard deviation.
    The sums, the division and the square root are double arithmetic: allowance = the cast to float (2^-24 |ref|) plus
    2^-45 times the magnitude of the terms; for rstd the second part is the reference evaluated at var +- dv,
    dv = 2^-45 * (s2 / count + m^2).  scale and shift are fp32 arithmetic on the kernel's own rstd and mean: checked
    against those (one product: K = 0; product and subtraction: K = 1) and against float64 throughout, where the
    allowances of rstd and mean are carried through."""
    parts, counts, gamma, beta = R.finalize_inputs(C)
    f = R.finalize(parts, counts, gamma, beta)
    L = len(parts)
    part = torch.cat(parts).cuda()
    rows_pl = (ctypes.c_int * lib.MAX_LEVELS)(*R.FIN_ROWS)
    cnt = (ctypes.c_int64 * lib.MAX_LEVELS)(*counts)
    tb = Tables(L, C)
    gd, bd = gamma.cuda(), beta.cuda()
    lib.call('sfvos_bn_finalize', P(part), L, rows_pl, cnt, P(gd), P(bd), R.EPS, C, tb.put('mean'), tb.put('rstd'),
             tb.put('scale'), tb.put('shift'), tb.put('varu'), tb.cs, S())
    torch.cuda.synchronize()
    mean, rstd, scale, shift, varu = (tb.get(k) for k in ('mean', 'rstd', 'scale', 'shift', 'varu'))
    g64, b64 = gamma.double(), beta.double()
    a_mean = U24 * f['mean'].abs() + DBL * f['a1']
    a_rstd = (U24 + DBL) * f['rstd'] + torch.maximum(f['rstd_hi'] - f['rstd'], f['rstd'] - f['rstd_lo'])
    n = torch.tensor(counts, dtype=torch.float64)[:, None]
    unb = torch.where(n > 1, n / (n - 1).clamp_min(1), torch.ones_like(n))
    worst = [check_abs('bn_finalize C %d mean' % C, mean, f['mean'], a_mean),
             check_abs('bn_finalize C %d rstd' % C, rstd, f['rstd'], a_rstd),
             check_abs('bn_finalize C %d var_unbiased' % C, varu, f['var_unbiased'],
                       (U24 + DBL) * f['var_unbiased'] + f['dv'] * unb),
             check('bn_finalize C %d scale | own rstd' % C, scale, g64 * rstd, (g64 * rstd).abs(), 0, 0.0),
             check('bn_finalize C %d shift | own mean' % C, shift, b64 - mean * scale, b64.abs() + (mean * scale).abs(),
                   1, 0.0)]
    a_scale = 2 * U22 * f['scale'].abs() + g64.abs() * a_rstd
    mag_shift = b64.abs() + (f['mean'] * f['scale']).abs()
    worst += [check_abs('bn_finalize C %d scale | float64' % C, scale, f['scale'], a_scale),
              check_abs('bn_finalize C %d shift | float64' % C, shift, f['shift'],
                        4 * U22 * mag_shift + f['mean'].abs() * a_scale + f['scale'].abs() * a_mean)]
    summary('bn_finalize', worst)


@pytest.mark.parametrize('C', [32, 224])
@pytest.mark.parametrize('n', [0, 1, 8])
def test_bn_running_update_alone_and_folded_into_bn_apply(lib, C, n):
    """running = (1 - momentum) * running + momentum * batch, n times: one product chain of two roundings and one addition
    per update, K = 2 n (n = 0: the values come back unchanged).  num_batches_tracked += n.  The update folded into
    sfvos_bn_apply gives the same bits; running = NULL (and num_batches_tracked = NULL) leave what they name untouched."""
    g = torch.Generator().manual_seed(13 + C)
    means = torch.randn(8, C, generator=g).float()
    varsu = (torch.rand(8, C, generator=g) + 0.1).float()
    rm0, rv0 = torch.randn(C, generator=g).float(), (torch.rand(C, generator=g) + 0.5).float()
    m, v, am, av = R.running(rm0, rv0, means, varsu, n)
    tb = Tables(8, C)
    tb.put('means', means.double())
    tb.put('vars', varsu.double())
    rm, rv = Out((C,)), Out((C,))
    rm.t.copy_(rm0), rv.t.copy_(rv0)
    nbt = torch.full((), 3, dtype=torch.int64, device='cuda')
    lib.call('sfvos_bn_running_update', P(rm.t), P(rv.t), tb.p('means'), tb.p('vars'), n, tb.cs, C, R.MOMENTUM, P(nbt), S())
    torch.cuda.synchronize()
    worst = [check('running_update C %d n %d mean' % (C, n), rm.cpu(), m, am, 2 * n, 0.0),
             check('running_update C %d n %d var' % (C, n), rv.cpu(), v, av, 2 * n, 0.0)]
    assert int(nbt) == 3 + n
    if n == 0:
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    # folded into the apply launch: one level of 5 positions
    rm2, rv2 = Out((C,)), Out((C,))
    rm2.t.copy_(rm0), rv2.t.copy_(rv0)
    nbt2 = torch.full((), 3, dtype=torch.int64, device='cuda')
    run = lib.BnRunning()
    run.running_mean, run.running_var = rm2.t.data_ptr(), rv2.t.data_ptr()
    run.means, run.vars_unbiased = tb.p('means').value, tb.p('vars').value
    run.num_batches_tracked, run.n_updates, run.momentum = nbt2.data_ptr(), n, R.MOMENTUM
    lv = levels(lib, [5])
    x = torch.ones((5, C), device='cuda')
    y = Out((5, C))
    lib.call('sfvos_bn_apply', P(x), C, P(y.t), C, lib.F32, ctypes.byref(lv), C, tb.p('means'), tb.p('vars'), tb.cs, 0,
             ctypes.byref(run), S())
    torch.cuda.synchronize()
    assert torch.equal(rm2.cpu(), rm.cpu()) and torch.equal(rv2.cpu(), rv.cpu()) and int(nbt2) == 3 + n
    y1 = y.cpu()
    y = Out((5, C))
    lib.call('sfvos_bn_apply', P(x), C, P(y.t), C, lib.F32, ctypes.byref(lv), C, tb.p('means'), tb.p('vars'), tb.cs, 0, None,
             S())
    lib.call('sfvos_bn_running_update', P(rm.t), P(rv.t), tb.p('means'), tb.p('vars'), 0, tb.cs, C, R.MOMENTUM, None, S())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), y1) and torch.equal(rm2.cpu(), rm.cpu()) and torch.equal(rv2.cpu(), rv.cpu())
    assert int(nbt2) == 3 + n and int(nbt) == 3 + n
    summary('bn_running_update', worst)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('C', R.BN_CS)
def test_bn_apply(lib, prec, C):
    """y = act(x * scale_l + shift_l) per element: one product and one addition, K = 1, mag = |x * scale| + |shift|, u_out by
    dtype; levels of 1, 37, 513 and 759 positions with their own coefficients; ReLU off and on."""
    d = R.bwd_inputs(C, prec, 0)
    ms, L = R.BN_LEVELS, len(R.BN_LEVELS)
    lv = levels(lib, ms)
    tb = Tables(L, C)
    tb.put('scale', d['scale'])
    tb.put('shift', d['shift'])
    xd = act_in(d['x'], prec, C)
    worst = []
    for relu in (0, 1):
        y = act_out(sum(ms), prec, C)
        lib.call('sfvos_bn_apply', P(xd, OFF), C + 2 * OFF, P(y.t, OFF), C + 2 * OFF, DT(lib, prec), ctypes.byref(lv), C,
                 tb.p('scale'), tb.p('shift'), tb.cs, relu, None, S())
        torch.cuda.synchronize()
        got = split(act_get(y, C), ms)
        for l in range(L):
            ref, mag = R.apply(d['x'][l], d['scale'][l], d['shift'][l], relu)
            worst.append(check('bn_apply %s C %d relu %d level %d' % (prec, C, relu, l), got[l], ref, mag, 1, U_OUT[prec]))
    summary('bn_apply', worst)


# ------------------------------------------------------------------------------------------ backward
def bwd_tables(d, L, C, names=('scale', 'shift', 'mean', 'rstd')):
    tb = Tables(L, C)
    for k in names:
        tb.put(k, d[k])
    return tb


def expected_rows(ms):
    return [min(-(-m // 512), 512) for m in ms]


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('C', R.BN_CS)
def test_bn_bwd_reduce(lib, C, prec, relu):
    """Per level the float64 sum of the rows against sum dz and sum dz * xhat in float64, u_out = 0.  K: a lane adds at most
    ceil(512 / rl) positions of a run, then the rl = 256 / (C / 4 or 8) lanes are added through LDS -- C 32: 48 (fp32) /
    72 (bf16), 64: 48 / 48, 192: 108 / 62, 224: 132 / 66, 256: 132 / 72.  mean, rstd, scale and shift are chosen in
    float64; ambiguous masks carry dy = 0 (bn_ref.bwd_inputs); the bound stays below the smallest |dz| (CPU pin)."""
    d = R.bwd_inputs(C, prec, relu)
    ms, L = R.BN_LEVELS, len(R.BN_LEVELS)
    lv = levels(lib, ms)
    rows = lib.load().sfvos_bn_bwd_rows(ctypes.byref(lv))
    assert rows == sum(expected_rows(ms))
    tb = bwd_tables(d, L, C)
    xd, dyd = act_in(d['x'], prec, C), act_in(d['dy'], prec, C)
    part = Out((rows, 2, C), torch.float32, fill=NAN)
    lib.call('sfvos_bn_bwd_reduce', P(dyd, OFF), C + 2 * OFF, P(xd, OFF), C + 2 * OFF, DT(lib, prec), ctypes.byref(lv), C,
             tb.p('scale'), tb.p('shift'), tb.p('mean'), tb.p('rstd'), tb.cs, relu, P(part.t), S())
    torch.cuda.synchronize()
    sums = level_rows(part.cpu(), expected_rows(ms))
    K = R.bwd_chain(C, prec)
    worst = []
    for l in range(L):
        dz = R.masked(d['dy'][l], d['x'][l], d['scale'][l], d['shift'][l], relu)
        ref, mag = R.bwd_sums(dz, d['x'][l], d['mean'][l], d['rstd'][l])
        worst.append(check('bn_bwd_reduce %s C %d relu %d K %d level %d' % (prec, C, relu, K, l), sums[l], ref, mag, K, 0.0))
    summary('bn_bwd_reduce', worst)


def big_device(prec):
    b = R.big_inputs()
    return b, act_in(b['x'], prec, 32), act_in(b['dy'], prec, 32)


@pytest.mark.parametrize('prec', PRECS)
def test_bn_bwd_reduce_beyond_the_row_cap_is_exact(lib, prec):
    """Levels of 512 * 512 + 37 and 5 positions, C 32: 513 runs on the 512 blocks of the capped level (block 0 walks two),
    and the block table behind it.  Exactly summable operands (bn_ref.big_inputs): the sums EQUAL float64."""
    b, xd, dyd = big_device(prec)
    ms, C = R.BIG_LEVELS, 32
    lv = levels(lib, ms)
    rows = lib.load().sfvos_bn_bwd_rows(ctypes.byref(lv))
    assert rows == 512 + 1
    tb = bwd_tables(b, len(ms), C)
    part = Out((rows, 2, C), torch.float32, fill=NAN)
    lib.call('sfvos_bn_bwd_reduce', P(dyd, OFF), C + 2 * OFF, P(xd, OFF), C + 2 * OFF, DT(lib, prec), ctypes.byref(lv), C,
             tb.p('scale'), tb.p('shift'), tb.p('mean'), tb.p('rstd'), tb.cs, 1, P(part.t), S())
    torch.cuda.synchronize()
    sums = level_rows(part.cpu(), [512, 1])
    for l in range(len(ms)):
        dz = R.masked(b['dy'][l], b['x'][l], b['scale'][l], b['shift'][l], 1)
        ref, _ = R.bwd_sums(dz, b['x'][l], b['mean'][l], b['rstd'][l])
        check_exact('bn_bwd_reduce %s big level %d' % (prec, l), sums[l], ref)


@pytest.mark.parametrize('train', [1, 0])
@pytest.mark.parametrize('C', [32, 224])
def test_bn_bwd_finalize(lib, C, train):
    """From given random rows (levels of 1, 400, 2 and 33 rows): sum_dz, sum_dzx and the coefficients of pass 2, train and
    eval.  Double arithmetic only: allowance = the cast (2^-24 |ref|) + 2^-45 x the magnitude of the terms (the sums of
    |row|, carried through the formula).  Eval: cB = cK = 0 exactly."""
    ms, rows_pl, parts, gamma, mean, rstd = R.bwd_finalize_inputs(C)
    L = len(ms)
    lv = levels(lib, ms)
    assert lib.load().sfvos_bn_bwd_rows(ctypes.byref(lv)) == sum(rows_pl) and expected_rows(ms) == rows_pl
    tb = Tables(L, C)
    tb.put('mean', mean)
    tb.put('rstd', rstd)
    part = torch.cat(parts).cuda()
    gd = gamma.float().cuda()
    lib.call('sfvos_bn_bwd_finalize', P(part), ctypes.byref(lv), P(gd), tb.p('mean'), tb.p('rstd'), tb.cs, C, train,
             tb.put('cA'), tb.put('cB'), tb.put('cK'), tb.put('sdz'), tb.put('sdzx'), S())
    torch.cuda.synchronize()
    s = torch.stack([p.double().sum(0) for p in parts])            # [L, 2, C]
    a = torch.stack([p.double().abs().sum(0) for p in parts])
    n = torch.tensor(ms, dtype=torch.float64)[:, None]
    cA, cB, cK = R.bwd_coeffs(s[:, 0], s[:, 1], n, gamma, mean, rstd, train)
    g = cA.abs()
    am1, am2 = a[:, 0] / n, a[:, 1] / n
    tag = 'bn_bwd_finalize C %d train %d ' % (C, train)
    worst = [check_abs(tag + 'sum_dz', tb.get('sdz'), s[:, 0], U24 * s[:, 0].abs() + DBL * a[:, 0]),
             check_abs(tag + 'sum_dzx', tb.get('sdzx'), s[:, 1], U24 * s[:, 1].abs() + DBL * a[:, 1]),
             check_abs(tag + 'cA', tb.get('cA'), cA, (U24 + DBL) * g)]
    if train:
        worst += [check_abs(tag + 'cB', tb.get('cB'), cB, U24 * cB.abs() + DBL * g * am2 * rstd),
                  check_abs(tag + 'cK', tb.get('cK'), cK, U24 * cK.abs() + DBL * (g * am2 * rstd * mean.abs() + g * am1))]
    else:
        check_exact(tag + 'cB', tb.get('cB'), cB)
        check_exact(tag + 'cK', tb.get('cK'), cK)
    summary('bn_bwd_finalize', worst)


def run_bwd_apply(lib, prec, ms, C, tb, xd, dyd, relu, bias, dgamma, dbeta, accumulate):
    M = sum(ms)
    lv = levels(lib, ms)
    dx = act_out(M, prec, C)
    lib.call('sfvos_bn_bwd_apply', P(dyd, OFF), C + 2 * OFF, P(xd, OFF), C + 2 * OFF, P(dx.t, OFF), C + 2 * OFF,
             DT(lib, prec), ctypes.byref(lv), C, tb.p('scale'), tb.p('shift'), tb.cs, relu, tb.p('cA'), tb.p('cB'),
             tb.p('cK'), P(bias.t) if bias else None, tb.p('sdz'), tb.p('sdzx'), P(dgamma.t) if dgamma else None,
             P(dbeta.t) if dbeta else None, accumulate, S())
    torch.cuda.synchronize()
    return act_get(dx, C)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('C', R.BN_CS)
def test_bn_bwd_apply(lib, C, prec, relu):
    """dx = cA * dz + cB * x + cK per element: three terms, K = 3, mag = |cA dz| + |cB x| + |cK|, u_out by dtype.  The
    coefficients are the train-mode ones of the float64 sums, rounded to fp32, so the column sums of dx cancel to about 0:
    the bias rows are compared with the float64 column sums of the UNROUNDED reference dx through the mag bound (K = 3 +
    the chain of the reduction, as in bn_bwd_reduce), u_out = 0.  dgamma / dbeta: the double sum over the levels of the
    given tables, cast, plus what the buffer held when accumulate is set: K = 1.  Either pointer NULL, bias_part NULL: the
    other outputs keep their bits."""
    d = R.bwd_inputs(C, prec, relu)
    ms, L = R.BN_LEVELS, len(R.BN_LEVELS)
    dzs = [R.masked(d['dy'][l], d['x'][l], d['scale'][l], d['shift'][l], relu) for l in range(L)]
    s = torch.stack([R.bwd_sums(dzs[l], d['x'][l], d['mean'][l], d['rstd'][l])[0] for l in range(L)])
    n = torch.tensor(ms, dtype=torch.float64)[:, None]
    co = [c.float().double() for c in R.bwd_coeffs(s[:, 0], s[:, 1], n, d['gamma'], d['mean'], d['rstd'], 1)]
    g = torch.Generator().manual_seed(37 + C)
    sdz, sdzx = torch.randn(L, C, generator=g).double() * 20, torch.randn(L, C, generator=g).double() * 20
    tb = bwd_tables(dict(d, cA=co[0], cB=co[1], cK=co[2], sdz=sdz, sdzx=sdzx), L, C,
                    ('scale', 'shift', 'cA', 'cB', 'cK', 'sdz', 'sdzx'))
    xd, dyd = act_in(d['x'], prec, C), act_in(d['dy'], prec, C)
    rows = sum(expected_rows(ms))
    bias = Out((rows, C), torch.float32, fill=NAN)
    old = torch.randn(C, generator=g).float()
    dg, db = Out((C,)), Out((C,))
    dx = run_bwd_apply(lib, prec, ms, C, tb, xd, dyd, relu, bias, dg, db, 0)
    K = 3 + R.bwd_chain(C, prec)
    tag = 'bn_bwd_apply %s C %d relu %d ' % (prec, C, relu)
    worst = []
    got, bsum = split(dx, ms), level_rows(bias.cpu(), expected_rows(ms))
    for l in range(L):
        ref, mag = R.bwd_dx(dzs[l], d['x'][l], co[0][l], co[1][l], co[2][l])
        worst.append(check(tag + 'dx level %d' % l, got[l], ref, mag, 3, U_OUT[prec]))
        worst.append(check(tag + 'bias rows K %d level %d' % (K, l), bsum[l], ref.sum(0), mag.sum(0), K, 0.0))
    worst += [check(tag + 'dgamma', dg.cpu(), sdzx.float().double().sum(0), sdzx.abs().sum(0), 1, 0.0),
              check(tag + 'dbeta', db.cpu(), sdz.float().double().sum(0), sdz.abs().sum(0), 1, 0.0)]
    # accumulate, dgamma NULL, bias_part NULL
    db2 = Out((C,))
    db2.t.copy_(old)
    dx2 = run_bwd_apply(lib, prec, ms, C, tb, xd, dyd, relu, None, None, db2, 1)
    worst.append(check(tag + 'dbeta +=', db2.cpu(), old.double() + sdz.float().double().sum(0),
                       old.double().abs() + sdz.abs().sum(0), 1, 0.0))
    # accumulate, dbeta NULL
    dg2, bias2 = Out((C,)), Out((rows, C), torch.float32, fill=NAN)
    dg2.t.copy_(old)
    dx3 = run_bwd_apply(lib, prec, ms, C, tb, xd, dyd, relu, bias2, dg2, None, 1)
    worst.append(check(tag + 'dgamma +=', dg2.cpu(), old.double() + sdzx.float().double().sum(0),
                       old.double().abs() + sdzx.abs().sum(0), 1, 0.0))
    assert torch.equal(dx2, dx) and torch.equal(dx3, dx) and torch.equal(bias2.cpu(), bias.cpu())
    summary('bn_bwd_apply', worst)


@pytest.mark.parametrize('prec', PRECS)
def test_bn_bwd_apply_beyond_the_row_cap_is_exact(lib, prec):
    """The 512 * 512 + 37 level and the 5-position level behind it with dyadic coefficients: dx is a multiple of 0.25 that
    bf16 holds, its column sums are exact in any order: dx and the per-level sums of the bias rows EQUAL float64."""
    b, xd, dyd = big_device(prec)
    ms, C = R.BIG_LEVELS, 32
    tb = bwd_tables(dict(b, sdz=b['cK'], sdzx=b['cK']), len(ms), C, ('scale', 'shift', 'cA', 'cB', 'cK', 'sdz', 'sdzx'))
    bias = Out((513, C), torch.float32, fill=NAN)
    dx = split(run_bwd_apply(lib, prec, ms, C, tb, xd, dyd, 1, bias, None, None, 0), ms)
    bsum = level_rows(bias.cpu(), [512, 1])
    for l in range(len(ms)):
        dz = R.masked(b['dy'][l], b['x'][l], b['scale'][l], b['shift'][l], 1)
        ref, _ = R.bwd_dx(dz, b['x'][l], b['cA'][l], b['cB'][l], b['cK'][l])
        check_exact('bn_bwd_apply %s big dx level %d' % (prec, l), dx[l], ref)
        check_exact('bn_bwd_apply %s big bias rows level %d' % (prec, l), bsum[l], ref.sum(0))
