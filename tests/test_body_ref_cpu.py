"""CPU (no GPU): tests/body_ref.py, the torch-core restatement the GPU tests of the ResNet body compare against, pinned
against torch's own operators; and the preconditions of the exact GPU cases, asserted on the reference."""
import pytest
import torch
import torch.nn.functional as F

import body_ref as R


@pytest.mark.parametrize('eps', [0.0, 1e-5])
def test_frozen_norm_is_batch_norm_in_eval_mode(eps):
    g = torch.Generator().manual_seed(1)
    x = torch.randn((2, 6, 5, 7), generator=g, dtype=torch.float64)
    w, b = torch.randn(6, generator=g), torch.randn(6, generator=g)
    rm, rv = torch.randn(6, generator=g), 0.5 + torch.rand(6, generator=g)
    got = R.frozen_bn(x, w, b, rm, rv, eps)
    # F.batch_norm(training=False); its Python wrapper refuses eps = 0 in recent releases, the operator behind it does not
    ref = torch.batch_norm(x, w.double(), b.double(), rm.double(), rv.double(), False, 0.0, eps, False)
    if eps > 0:
        assert torch.equal(ref, F.batch_norm(x, rm.double(), rv.double(), w.double(), b.double(), False, 0.0, eps))
    assert float((got - ref).abs().max()) < 1e-12
    # the two epsilons differ by what the formula says
    d = R.frozen_bn(x, w, b, rm, rv, 1e-5) - R.frozen_bn(x, w, b, rm, rv, 0.0)
    ds = (w.double() * ((rv.double() + 1e-5).rsqrt() - rv.double().rsqrt())).reshape(1, -1, 1, 1)
    assert float((d - (x - rm.double().reshape(1, -1, 1, 1)) * ds).abs().max()) < 1e-12


def test_output_sides_of_stride_two_ops():
    for h in range(1, 701):
        x = torch.zeros(1, 1, h, 3)
        want = (h - 1) // 2 + 1
        assert R.out_side(h) == want
        if h in (1, 2, 3, 4, 5, 6, 7, 69, 70, 700):      # torch's own operators agree (a few sizes: they are slow)
            assert F.max_pool2d(x, 3, 2, 1).shape[2] == want
            assert F.conv2d(x, torch.zeros(1, 1, 7, 7), None, 2, 3).shape[2] == want
            assert F.conv2d(x, torch.zeros(1, 1, 3, 3), None, 2, 1).shape[2] == want
            assert F.conv2d(x, torch.zeros(1, 1, 1, 1), None, 2, 0).shape[2] == want


def test_state_surface_counts():
    want = R.expected_state()
    convs = [k for k, s in want.items() if len(s) == 4]
    assert len(want) == 265 and len(convs) == 53
    n = 0
    for k in convs:
        s = want[k]
        n += s[0] * s[1] * s[2] * s[3]
    assert n == 23454912
    assert sum(s[0] for k, s in want.items() if k.endswith('running_var')) == 26560
    shapes = R.conv_shapes((192, 336))
    assert len(shapes) == 52 and shapes[-1][1:3] == (24, 42)
    macs = sum(((h - 1) // s + 1) * ((w - 1) // s + 1) * ci * co * t for _, h, w, ci, co, t, s in shapes)
    macs += 384 * 672 * 147 * 64
    assert 83e9 < macs < 85e9


def test_restatement_runs_and_halves_every_level():
    sd = R.random_state(2)
    body = R.ResNetBody(sd)
    x = torch.randn(1, 3, 70, 100, generator=torch.Generator().manual_seed(3))
    out = body(x)
    assert [tuple(v.shape[1:]) for v in out.values()] == [(256, 18, 25), (512, 9, 13), (1024, 5, 7), (2048, 3, 4)]
    assert all(bool(torch.isfinite(v).all()) and float(v.min()) >= 0 for v in out.values())
    assert 0.05 < float(out['3'].std()) < 50          # the random state keeps the activations of order one
    x64 = body(x.double())
    assert float((x64['3'] - out['3'].double()).abs().max()) < 1e-3 * float(x64['3'].abs().max())


def test_exact_cases_meet_their_preconditions():
    import test_gpu_body_kernels as K
    for case in K.EXACT[:12]:
        x, wt, scale, shift, resid, ref, mag, pre, amag = K._exact_reference(case)
        assert float(amag.max()) < 2 ** 24 and float(pre.abs().max()) <= 256
        assert bool((2 * pre == (2 * pre).round()).all())
        assert set(scale.tolist()) <= {0.5, 1.0, 2.0}
        per_out = float((wt != 0).flatten(1).sum(1).float().mean())
        assert per_out <= 90, per_out
