"""CPU (no GPU): the size rule of sfvos_amd.GeneralizedRCNNTransform and the two formulations of tests/transform_ref.py
against each other -- the float64 F.interpolate reference the GPU tests compare with, and the header's fp32 index and weight
arithmetic with float64 blending, which supplies `mag`, `D_h` and `D_w` of their bound -- plus the preconditions of the exact
cases and the nearest rule of the masks."""
import pytest
import torch
import torch.nn.functional as F

import transform_ref as R


def _transform():
    from sfvos_amd import GeneralizedRCNNTransform
    return GeneralizedRCNNTransform


def test_davis_frame_size_and_batch_shape():
    T = _transform()
    assert T.resize_size((480, 854)) == (749, 1333)
    assert T.batch_shape([T.resize_size((480, 854))]) == (768, 1344)
    assert T.batch_shape([(749, 1333), (800, 1200), (33, 46)]) == (800, 1344)
    assert T.batch_shape([(58, 83)], 32) == (64, 96) and T.batch_shape([(64, 96)]) == (64, 96)
    assert T.batch_shape([(5, 7)], 1) == (5, 7)


def test_resize_size_is_interpolates_output_shape():
    """Over landscape, portrait and square sizes, with min_size binding and with max_size binding."""
    T = _transform()
    sizes = [(h, w) for h in range(97, 1400, 83) for w in range(101, 1500, 79)]
    sizes += [(w, h) for h, w in sizes[::7]] + [(n, n) for n in (1, 2, 37, 480, 800, 1333, 2000)]
    sizes += [(480, 854), (854, 480), (1080, 1920), (100, 3000), (3000, 100)]
    assert len(sizes) > 300
    bound = set()
    for h, w in sizes:
        for mn, mx in ((800, 1333), (64, 96)):
            lo, hi = float(min(h, w)), float(max(h, w))
            s = min(mn / lo, mx / hi)
            bound.add(mn / lo < mx / hi)
            out = F.interpolate(torch.zeros(1, 1, h, w), scale_factor=s, mode='bilinear', recompute_scale_factor=True,
                                align_corners=False)
            assert T.resize_size((h, w), mn, mx) == tuple(out.shape[-2:]), (h, w, mn, mx)
    assert bound == {True, False}


def test_min_size_tuple_and_training_draw():
    T = _transform()
    t = T(min_size=(48, 64), max_size=200)
    assert t.min_size == (48, 64)
    torch.manual_seed(0)
    drawn = {t.torch_choice(t.min_size) for _ in range(64)}
    assert drawn == {48, 64}
    assert T(min_size=48).min_size == (48,)
    with pytest.raises(ValueError):
        T(image_std=(0.2, 0.0, 0.2))
    with pytest.raises(ValueError):
        T(image_mean=(0.5, 0.5))


@pytest.mark.parametrize('src,size,shape', R.GENERAL_CASES, ids=str)
def test_fp32_index_formulation_agrees_with_interpolate_within_the_lambda_term(src, size, shape):
    x = R.random_image(3, 2, *src)
    ref = R.reference_image(x, size, shape)
    out, mag, dh, dw, _ = R.formula_image(x, size, shape)
    allow = R.lambda_term(dh, dw, *src)
    err = (out - ref).abs()
    assert bool((err <= allow).all()), float((err / allow.clamp_min(1e-300)).max())
    inside = allow[:, :, :size[0], :size[1]]
    print('%s -> %s: worst |formula - interpolate| / lambda term %.4f; lambda term / bound at most %.3f' % (
        src, size, float((err[:, :, :size[0], :size[1]] / inside).max()),
        float((inside / R.bound(mag, dh, dw, *src)[:, :, :size[0], :size[1]]).max())))
    # the pad: zero in both, and nothing allowed
    assert float(ref[:, :, size[0]:].abs().max()) == 0 and float(ref[:, :, :, size[1]:].abs().max()) == 0
    assert float(allow[:, :, size[0]:].max()) == 0 and float(mag[:, :, :, size[1]:].max()) == 0


@pytest.mark.parametrize('src,size,shape', R.EXACT_CASES, ids=str)
def test_exact_cases_are_exact(src, size, shape):
    """Every weight a multiple of 1/8, every normalised value a multiple of 1/4 below 32, so every product and sum of the
    blend is a multiple of 2^-8 below 2^16: exact in fp32 in any order, and the two formulations agree to the bit."""
    for axis in (0, 1):
        assert size[axis] in (src[axis], 2 * src[axis], 4 * src[axis]) or 2 * size[axis] == src[axis]
        assert size[axis] <= shape[axis]
    x = R.exact_image(5, 3, *src)
    v = R.normalize64(x, R.EXACT_MEAN, R.EXACT_STD)
    assert R.is_dyadic(v, 2) and float(v.abs().max()) < 32
    ref = R.reference_image(x, size, shape, R.EXACT_MEAN, R.EXACT_STD)
    out, _, _, _, weights = R.formula_image(x, size, shape, R.EXACT_MEAN, R.EXACT_STD)
    for l in weights:
        assert R.is_dyadic(l, 3) and float(l.min()) >= 0 and float(l.max()) <= 1
    assert R.is_dyadic(ref, 8) and float(ref.abs().max()) < 2 ** 16
    assert torch.equal(out, ref)
    assert torch.equal(ref.float().double(), ref)


def test_exact_cases_cover_the_group_boundary():
    ow4 = {size[1] % 4 for _, size, _ in R.EXACT_CASES}
    assert ow4 == {0, 1, 2, 3}
    assert any(size[1] == shape[1] for _, size, shape in R.EXACT_CASES)
    assert any(size[0] == shape[0] for _, size, shape in R.EXACT_CASES)
    assert any(shape[1] - size[1] > size[1] for _, size, shape in R.EXACT_CASES)
    assert any(shape[1] % 4 for _, _, shape in R.EXACT_CASES)
    assert {src for src, _, _ in R.EXACT_CASES} >= {(1, 1), (2, 3), (5, 7)}
    ratios = set()
    for src, size, _ in R.EXACT_CASES:
        ratios |= {size[a] / src[a] for a in (0, 1)}
    assert ratios == {1.0, 2.0, 4.0, 0.5}


@pytest.mark.parametrize('src,size', R.MASK_CASES, ids=str)
def test_nearest_formula_is_interpolate(src, size):
    for G in (0, 3):
        m = R.random_masks(9, G, *src)
        ref = R.reference_masks(m, size)
        assert ref.dtype == torch.uint8 and tuple(ref.shape) == (G,) + tuple(size)
        assert torch.equal(R.formula_masks(m, size), ref)


def test_nearest_fp32_pair():
    """floorf(d * scale) in fp32 against d * in // out: the pair of the module docstring differs, the nearest formula and
    F.interpolate both take the fp32 value, and a mask whose rows are their own index shows it."""
    p = R.NEAREST_FP32_PAIR
    idx = R.nearest_index(p['n_in'], p['n_out'])
    exact = torch.arange(p['n_out']) * p['n_in'] // p['n_out']
    assert int(idx[p['d']]) == p['fp32'] and int(exact[p['d']]) == p['integer']
    assert [int(d) for d in (idx != exact).nonzero().flatten()] == [p['d']]
    assert ((p['n_in'], p['n_in']), (p['n_out'], p['n_out'])) in R.MASK_CASES
    rows = torch.arange(p['n_in'], dtype=torch.uint8)[None, :, None].expand(1, p['n_in'], p['n_in']).contiguous()
    got = R.reference_masks(rows, (p['n_out'], p['n_out']))
    assert int(got[0, p['d'], 0]) == p['fp32']
    # no pair with smaller sides: every in, out < 26 agrees with the integer rule
    for n_in in range(1, 26):
        for n_out in range(1, 26):
            assert torch.equal(R.nearest_index(n_in, n_out),
                               (torch.arange(n_out) * n_in // n_out).clamp_max(n_in - 1)), (n_in, n_out)
