"""CPU: pins of tests/bn_ref.py, the float64 references and input generators of tests/test_gpu_bn_kernels.py.  The
references, chained, equal F.batch_norm (+ ReLU) and its autograd in double; the generated inputs meet the preconditions
the GPU tests rely on (exact summability, few ambiguous ReLU masks, bounds below one dropped position)."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('train', [1, 0])
def test_references_chained_equal_batch_norm_and_its_autograd_in_double(train, relu):
    """finalize -> apply -> masked -> bwd_sums -> bwd_coeffs -> bwd_dx against F.batch_norm per level, to 1e-12 (the
    cA / cB / cK form is easy to get wrong by a sign); eval mode takes the coefficients from running statistics."""
    g = torch.Generator().manual_seed(2)
    C, ms = 8, [1, 37, 300] if not train else [5, 37, 300]   # (train mode: a level of one value has no variance)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    xs = [torch.randn(m, C, generator=g, dtype=torch.float64) * (1 + l) + 0.3 * l for l, m in enumerate(ms)]
    dys = [torch.randn(m, C, generator=g, dtype=torch.float64) for m in ms]
    # fp64 "partial rows": three pieces per level
    parts = []
    for x in xs:
        cuts = [x[:len(x) // 3], x[len(x) // 3:len(x) // 2], x[len(x) // 2:]]
        parts.append(torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in cuts]))
    f = R.finalize(parts, ms, gamma, beta, eps=1e-5)
    gsum, bsum = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    run_m, run_v = rm.clone(), rv.clone()
    for l, (x, dy) in enumerate(zip(xs, dys)):
        if train:
            mean, rstd, scale, shift = f['mean'][l], f['rstd'][l], f['scale'][l], f['shift'][l]
        else:
            mean, rstd = rm, 1.0 / torch.sqrt(rv + 1e-5)
            scale, shift = gamma * rstd, beta - rm * gamma * rstd
        xr = x.clone().requires_grad_(True)
        y = F.batch_norm(xr.t().reshape(1, C, -1), run_m, run_v, gr, br, bool(train), 0.1, 1e-5)
        y = F.relu(y) if relu else y
        y.backward(dy.t().reshape(1, C, -1))
        got_y, _ = R.apply(x, scale, shift, relu)
        assert float((got_y - y.detach().reshape(C, -1).t()).abs().max()) < 1e-12
        dz = R.masked(dy, x, scale, shift, relu)
        sums, _ = R.bwd_sums(dz, x, mean, rstd)
        cA, cB, cK = R.bwd_coeffs(sums[0], sums[1], float(len(x)), gamma, mean, rstd, train)
        dx, _ = R.bwd_dx(dz, x, cA, cB, cK)
        assert float((dx - xr.grad).abs().max()) < 1e-12 * max(1.0, float(xr.grad.abs().max()))
        gsum += sums[1]
        bsum += sums[0]
    assert float((gsum - gr.grad).abs().max()) < 1e-12 * float(gr.grad.abs().max())
    assert float((bsum - br.grad).abs().max()) < 1e-12 * float(br.grad.abs().max())
    if train:   # running statistics: one update per level, unbiased variance
        m, v, _, _ = R.running(rm, rv, f['mean'], f['var_unbiased'], len(ms), momentum=0.1)
        # (R.running uses the kernel's fp32 momentum: 0.1f differs from 0.1 by 1.5e-9)
        assert float((m - run_m).abs().max()) < 1e-7 and float((v - run_v).abs().max()) < 1e-7


def test_finalize_reference_uses_the_kernels_formula_and_clamps():
    parts, counts, gamma, beta = R.finalize_inputs(32)
    assert [p.shape[0] for p in parts] == R.FIN_ROWS and len(parts) == 8 and counts[0] == 1
    f = R.finalize(parts, counts, gamma, beta)
    assert bool((f['var'] >= 0).all()) and bool(torch.isfinite(f['rstd']).all())
    assert bool((f['var'][:, 3] < 1e-6).all())                              # the constant channel
    ratio = f['mean'][1:, 5].abs() / torch.sqrt(f['var'][1:, 5])            # mean about 1000 x the standard deviation
    assert bool((ratio > 300).all()) and bool((ratio < 3000).all())
    assert bool((f['var_unbiased'][0] == f['var'][0]).all())                # count 1
    assert bool((f['rstd_lo'] <= f['rstd']).all()) and bool((f['rstd'] <= f['rstd_hi']).all())


@pytest.mark.parametrize('name', [c[0] for c in R.CONV_CASES])
def test_conv_statistics_cases_are_exactly_summable(name):
    """Integers; every output magnitude below 2^24; per level and channel sum |v| and sum v^2 below 2^24 (any partition
    into rows is then exact); |v| <= 256, so a bf16 y holds it; the ReLU variant is a subset of the same sums."""
    xs, w, bias, refs = R.conv_inputs(name)
    assert R.conv_mag(name) < 2.0 ** 24
    for ref in refs:
        assert bool((ref == ref.round()).all()) and float(ref.abs().max()) <= 256
        a1 = ref.abs().sum((0, 2, 3, 4))
        s1, s2 = R.stats(ref)
        assert float(a1.max()) < 2.0 ** 24 and float(s2.max()) < 2.0 ** 24
        assert float(s2.min()) > 0        # no dead channel: every statistics column carries something


@pytest.mark.parametrize('name', [c[0] for c in R.SHIFT_CASES])
def test_shift_statistics_cases_are_exactly_summable(name):
    _, B, T, shapes, C, _ = next(c for c in R.SHIFT_CASES if c[0] == name)
    for s in (1, T - 1):
        prev, fresh = R.shift_inputs(name, s)
        for p, f in zip(prev, fresh):
            v = torch.cat([p[:, s:], f], 1).reshape(-1, C)
            assert bool((v == v.round()).all()) and float(v.abs().max()) <= 256
            assert float(v.abs().sum(0).max()) < 2.0 ** 24 and float((v * v).sum(0).max()) < 2.0 ** 24


def test_big_level_case_is_exactly_summable():
    """dz and dx sums of the 512 * 512 + 37 level: dz integers, dz * xhat multiples of 0.5, dx multiples of 0.25, each sum
    of magnitudes below 2^24 units; masks are never within rounding of zero."""
    b = R.big_inputs()
    for l in range(len(R.BIG_LEVELS)):
        x, dy = b['x'][l], b['dy'][l]
        assert not bool(R.ambiguous(x, b['scale'][l], b['shift'][l]).any())
        dz = R.masked(dy, x, b['scale'][l], b['shift'][l], 1)
        xh = (x - b['mean'][l]) * b['rstd'][l]
        dx, mag = R.bwd_dx(dz, x, b['cA'][l], b['cB'][l], b['cK'][l])
        assert R.exact_ok(dz) and R.exact_ok(dz * xh, 0.5) and R.exact_ok(dx, 0.25) and R.exact_ok(mag, 0.25)
        assert float(dx.abs().max()) <= 4       # bf16 holds multiples of 0.25 up to 4
        assert bool((dz != dy).any()) and bool((dz != 0).any())


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('C', R.BN_CS)
def test_masked_cases_have_few_ambiguous_elements_and_bounds_below_one_position(C, prec):
    """At most 0.1 % of the elements of any channel are ambiguous (they get dy = 0); the bound of every level's sum of dz
    is below the smallest non-zero |dz| of the level: one dropped or doubled position cannot hide."""
    d = R.bwd_inputs(C, prec, 1)
    total = sum(R.BN_LEVELS)
    assert float(torch.stack(d['n_amb']).sum(0).max()) <= 1e-3 * total
    K = R.bwd_chain(C, prec)
    for relu in (0, 1):
        d = R.bwd_inputs(C, prec, relu)
        for l, (x, dy) in enumerate(zip(d['x'], d['dy'])):
            dz = R.masked(dy, x, d['scale'][l], d['shift'][l], relu)
            if relu:
                assert bool((dz[:, 1][x[:, 1] <= 0] == 0).all()) and bool((dz[:, 1][x[:, 1] > 0] != 0).all())
                assert bool((dz[0::3, 1] == 0).all())          # x = +-0.0 with shift 0: gradient 0
            sums, mags = R.bwd_sums(dz, x, d['mean'][l], d['rstd'][l])
            bound = 2.0 * (K + 1) * R.U22 * mags[0]
            nz = dz.abs()[dz != 0]
            if nz.numel():
                assert float(bound.max()) < float(nz.min()), (l, float(bound.max()), float(nz.min()))
