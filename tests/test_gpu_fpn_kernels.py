"""GPU: the two kernels of csrc/fpn.hip alone, through the C ABI, fp32 and bf16, every output between guard bands.

sfvos_fpn_lateral, per-element criterion of kernel_util with K = c_in + 1 (c_in products and the bias in one chain; the
top map is one more addend, inside the factor 2 of the criterion): operands as the kernel sees them (x and W rounded to
the compute dtype, the top map as stored).  Exact cases (check_exact): x, W in {-1, 0, 1}, bias and top small integers,
W sparse enough that every magnitude sum stays <= 256 (asserted), so each partial sum in any order is an integer below
2^24 and a bf16 store is exact; W is random, hence asymmetric: a transposed fragment map fails.

Shapes: 5x7 = 35 positions (one 32-position tile and a ragged one), 33x65 (rows aligned to no tile), tops that are
2 n - 1 and 2 n of the level; c_in 32 / 96 (not a multiple of 64) / 2048 (the split of the channels over the waves of a
workgroup, taken when the positions alone do not fill the chip); c_out 32 / 256; 96x168 and 130x130 with c_out 256 are
the sizes at which the channel slice per workgroup becomes 64 and 128 on a 256-CU device; 192x336 is DAVIS level 0
(position indices beyond 2^16, the full grid)."""
import pytest
import torch

from kernel_util import DT, PRECS, SENT, TDT, U_OUT, Out, P, S, check, check_exact, lib, rnd  # noqa: F401

pytestmark = pytest.mark.gpu


def _top_of(h, w, kind):
    if kind is None:
        return None
    return ((h + 1) // 2, (w + 1) // 2)      # the only size with h in {2 n, 2 n - 1}


def _strided(x, wide):
    """x [B, C, h, w] on the device, dense or as a slice of a wider tensor (batch, channel and row strides all differ
    from the dense ones; stride_w stays 1)."""
    if not wide:
        return x.cuda()
    B, C, h, w = x.shape
    big = torch.full((B, C + 8, h + 1, w + 3), 1e30, dtype=torch.float32, device='cuda')
    v = big[:, 8:, :h, :w]
    v.copy_(x)
    assert v.stride(1) != h * w and v.stride(3) == 1
    return v


def _run(lib, prec, xd, wt, bias, top, top_hw, c_out, ld_extra):
    B, c_in, h, w = xd.shape
    ld_y = c_out + ld_extra
    y = Out((B * h * w, ld_y), TDT[prec])
    wd = wt.to(TDT[prec]).cuda().contiguous()
    bd = bias.float().cuda()
    td = None if top is None else top.to(TDT[prec]).cuda().contiguous()
    th, tw = top_hw if top is not None else (0, 0)
    lib.call('sfvos_fpn_lateral', P(xd), xd.stride(0), xd.stride(1), xd.stride(2), xd.stride(3), B, c_in, h, w, P(wd),
             P(bd), c_out, None if td is None else P(td), th, tw, 0 if td is None else td.shape[1], P(y.t), ld_y,
             DT(lib, prec), S())
    torch.cuda.synchronize()
    got = y.cpu()
    if ld_extra:
        assert bool((got[:, c_out:] == SENT).all()), 'wrote the neighbouring columns'
    return got[:, :c_out].float()


def _reference(x, wt, bias, top, top_hw, f=torch.float64):
    """(ref, mag) [B h w, c_out] in dtype f; x [B, C, h, w], wt [c_out, C], top [B th tw, ld] or None."""
    B, C, h, w = x.shape
    xs = x.permute(0, 2, 3, 1).reshape(-1, C).to(f)
    ref = xs @ wt.to(f).t() + bias.to(f)
    mag = xs.abs() @ wt.to(f).abs().t() + bias.to(f).abs()
    if top is not None:
        th, tw = top_hw
        ii, jj = torch.arange(h) >> 1, torch.arange(w) >> 1
        t = top[:, :wt.shape[0]].to(f).reshape(B, th, tw, -1)[:, ii][:, :, jj].reshape(B * h * w, -1)
        ref, mag = ref + t, mag + t.abs()
    return ref, mag


# (c_in, c_out, B, h, w, top: None / 'top', x a slice of a wider tensor, extra columns of y)
CASES = [
    (32, 32, 1, 5, 7, None, False, 0),
    (96, 256, 2, 5, 7, 'top', True, 64),
    (2048, 256, 2, 5, 7, 'top', False, 0),
    (2048, 32, 1, 6, 8, 'top', True, 32),
    (96, 32, 2, 6, 8, 'top', False, 32),
    (32, 256, 2, 6, 8, None, True, 0),
    (32, 256, 1, 33, 65, None, False, 0),
    (96, 256, 2, 33, 65, 'top', True, 64),
    (2048, 256, 1, 33, 65, 'top', False, 0),
    (96, 32, 2, 33, 65, 'top', False, 0),
]
IDS = ['cin%d-cout%d-B%d-%dx%d-%s%s%s' % (c[0], c[1], c[2], c[3], c[4], c[5], '-slice' if c[6] else '',
                                            '-ld+%d' % c[7] if c[7] else '') for c in CASES]


def _operands(case, seed, exact):
    c_in, c_out, B, h, w, kind, _, _ = case
    g = torch.Generator().manual_seed(seed)
    top_hw = _top_of(h, w, kind)
    ld_top = c_out + 32
    if exact:
        x = torch.randint(-1, 2, (B, c_in, h, w), generator=g).float()
        keep = torch.rand((c_out, c_in), generator=g) < min(1.0, 80.0 / c_in)
        wt = torch.randint(-1, 2, (c_out, c_in), generator=g).float() * keep
        bias = torch.randint(-3, 4, (c_out,), generator=g).float()
        top = None if kind is None else torch.randint(-8, 9, (B * top_hw[0] * top_hw[1], ld_top), generator=g).float()
    else:
        x = torch.randn((B, c_in, h, w), generator=g)
        wt = torch.randn((c_out, c_in), generator=g) / c_in ** 0.5
        bias = torch.randn((c_out,), generator=g)
        top = None if kind is None else torch.randn((B * top_hw[0] * top_hw[1], ld_top), generator=g)
    return x, wt, bias, top, top_hw


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_lateral_against_float64(lib, case, prec):
    x, wt, bias, top, top_hw = _operands(case, 11, False)
    if top is not None:
        top = rnd(top, prec)         # the stored values
    got = _run(lib, prec, _strided(x, case[6]), wt, bias, top, top_hw, case[1], case[7])
    ref, mag = _reference(rnd(x, prec), rnd(wt, prec), bias, top, top_hw)
    check('fpn_lateral %s %s' % (prec, IDS[CASES.index(case)]), got, ref, mag, case[0] + 1, U_OUT[prec])


EXACT = CASES + [
    (64, 256, 1, 96, 168, 'top', False, 0),      # 64-channel slices per workgroup
    (64, 256, 1, 130, 130, 'top', False, 0),     # 128-channel slices
    (256, 256, 1, 192, 336, 'top', False, 0),    # DAVIS level 0
]
EXACT_IDS = IDS + ['slices64-96x168', 'slices128-130x130', 'davis-level0-192x336']


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', EXACT, ids=EXACT_IDS)
def test_lateral_exact(lib, case, prec):
    x, wt, bias, top, top_hw = _operands(case, 12, True)
    # integers below 2^24 are exact in fp32: the float32 matmul IS the float64 one (and much faster on the CPU)
    ref, mag = _reference(x, wt, bias, top, top_hw, torch.float32)
    assert float(mag.max()) <= 256 and bool((ref == ref.round()).all())
    assert not torch.equal(wt[:32, :32], wt[:32, :32].t())
    got = _run(lib, prec, _strided(x, case[6]), wt, bias, top, top_hw, case[1], case[7])
    check_exact('fpn_lateral exact %s %s' % (prec, EXACT_IDS[EXACT.index(case)]), got, ref)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('h,w', [(5, 7), (6, 8), (1, 1)])
def test_pool_exact(lib, h, w, prec):
    B = 2
    C = 40 if prec == 'bf16' else 20          # 5 chunks of 16 bytes: not a multiple of 32 channels
    ld_src, ld_dst = C + 24, C + 8
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator().manual_seed(13)
    src = torch.randint(-128, 129, (B, h, w, ld_src), generator=g).float()
    dst = Out((B * oh * ow, ld_dst), TDT[prec])
    sd = src.to(TDT[prec]).cuda()
    lib.call('sfvos_fpn_pool', P(sd), ld_src, P(dst.t), ld_dst, B, h, w, C, DT(lib, prec), S())
    torch.cuda.synchronize()
    got = dst.cpu().float()
    assert (oh, ow) == ((3, 4) if h > 1 else (1, 1))
    check_exact('fpn_pool %s %dx%d' % (prec, h, w), got[:, :C], src[:, ::2, ::2, :C].reshape(-1, C))
    assert bool((got[:, C:] == SENT).all()), 'wrote the neighbouring columns'
