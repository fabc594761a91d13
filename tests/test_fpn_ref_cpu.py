"""CPU (no GPU): pins the torch-core restatement of the feature pyramid network (tests/fpn_ref.py) that the GPU tests
compare with, and the one rule of `nearest` the lateral kernel relies on."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import fpn_ref as R

SHAPES = [(19, 27), (10, 14), (5, 7), (3, 4)]


def test_identity_weights_give_sums_of_upsampled_inputs():
    """Every inner block the identity (C -> C), every layer block the centre tap's identity: level l of the output is
    x_l + up(x_{l+1} + up(x_{l+2} + ...)), with up(v)[i][j] = v[i >> 1][j >> 1]."""
    C, B = 4, 2
    fpn = R.FeaturePyramidNetwork([C] * 4, C).double()
    with torch.no_grad():
        for inner, layer in zip(fpn.inner_blocks, fpn.layer_blocks):
            inner.weight.copy_(torch.eye(C).view(C, C, 1, 1))
            layer.weight.zero_()
            layer.weight[:, :, 1, 1] = torch.eye(C)
    g = torch.Generator().manual_seed(5)
    x = OrderedDict((str(l), torch.randint(-8, 9, (B, C, h, w), generator=g).double()) for l, (h, w) in enumerate(SHAPES))
    with torch.no_grad():
        out, inners = fpn(x, return_inner=True)
    assert list(out.keys()) == ['0', '1', '2', '3', 'pool']
    want = None
    for l in (3, 2, 1, 0):
        h, w = SHAPES[l]
        xl = x[str(l)]
        if want is not None:
            ii = torch.arange(h) >> 1
            jj = torch.arange(w) >> 1
            xl = xl + want[:, :, ii][:, :, :, jj]
        want = xl
        assert torch.equal(out[str(l)], want) and torch.equal(inners[l], want), l
    assert torch.equal(out['pool'], out['3'][:, :, ::2, ::2]) and tuple(out['pool'].shape[-2:]) == (2, 2)


def test_nearest_reads_index_shifted_by_one_for_2n_and_2n_minus_1():
    for n in range(1, 701):
        src = torch.arange(n, dtype=torch.float32).view(1, 1, n, 1)
        for out in (2 * n, 2 * n - 1):
            got = F.interpolate(src, size=(out, 1), mode='nearest').view(-1).long()
            assert torch.equal(got, torch.arange(out) >> 1), (n, out)
            got = F.interpolate(src.view(1, 1, 1, n), size=(1, out), mode='nearest').view(-1).long()
            assert torch.equal(got, torch.arange(out) >> 1), (n, out)


def test_pool_sizes():
    for h in range(1, 40):
        for w in (1, 2, 7, 42):
            y = R.last_level_max_pool(torch.zeros(1, 1, h, w))
            assert tuple(y.shape[-2:]) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    x = torch.arange(35.).view(1, 1, 5, 7)
    assert torch.equal(R.last_level_max_pool(x), x[:, :, ::2, ::2])
