"""GPU: the kernels of csrc/body.hip alone, through the C ABI, fp32 and bf16, every output between guard bands.

sfvos_conv2d, exact cases (check_exact): x and W in {-1, 0, 1}, W random (hence asymmetric across taps and channels,
asserted: a transposed fragment map or a mirrored tap fails) and thinned to about 80 non-zeros per output, scale in
{1/2, 1, 2}, integer shift in [-3, 3], integer residual in [-8, 8].  Then every partial sum, in any order and any partition
into K splits, is an integer below 2^24, the affine gives a multiple of 1/2 and |v| <= 256 (asserted on the reference), so
fp32 arithmetic and a bf16 store are exact: got == ref.  Shapes: the smallest at which each mechanism can go wrong -- odd
sides, both parities under stride 2, one and several 64-position tiles, tile edges on both axes (33x65), the few-positions
path whose K is split over workgroups (3x4), and one shape per tile configuration sfvos_conv2d_plan returns for a
768x1344 frame (test_body_entry_points_cpu.py asserts the coverage).

Random operands, one case per tap / stride combination, under `check` with u_out = U_OUT[prec], K = c_in * taps + 2
(c_in * taps products in one chain, the shift and the residual) and mag = |scale| sum |x||W| + |shift| + |residual|;
operands as the kernel sees them (x, W, residual rounded to the compute dtype).

sfvos_body_stem: exact on {-1, 0, 1} images read through the strides of a slice of a wider tensor; one random case with
K = 148.  sfvos_maxpool3x3s2: exact on integers in [-128, 128] with all-negative windows at the borders (a zero padding
would win there)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from kernel_util import DT, PRECS, SENT, TDT, U_OUT, Out, P, S, check, check_exact, lib, rnd  # noqa: F401

pytestmark = pytest.mark.gpu

# (taps, stride, c_in, c_out, B, h, w, residual, relu, extra columns of y, extra columns of the residual)
EXACT = [
    (1, 1, 64, 256, 2, 9, 13, True, 1, 64, 32),
    (1, 1, 256, 64, 1, 9, 13, False, 1, 0, 0),
    (1, 2, 256, 512, 1, 9, 13, False, 0, 0, 0),
    (1, 2, 256, 512, 1, 8, 12, False, 0, 0, 0),
    (9, 1, 64, 64, 1, 5, 7, False, 1, 0, 0),
    (9, 1, 64, 64, 1, 33, 65, False, 1, 0, 0),
    (9, 2, 128, 128, 1, 9, 13, False, 1, 0, 0),
    (9, 2, 128, 128, 1, 10, 14, False, 1, 0, 0),
    (9, 1, 512, 512, 1, 3, 4, False, 1, 0, 0),
    (1, 1, 2048, 512, 1, 3, 4, False, 1, 0, 0),
    (1, 2, 1024, 2048, 1, 5, 7, False, 0, 0, 0),
    (1, 1, 512, 2048, 2, 3, 4, True, 1, 0, 0),
    # one shape per configuration of the plan on a 256-CU device
    (1, 1, 64, 256, 1, 96, 168, True, 1, 0, 0),       # 128 x 128 tiles
    (9, 1, 64, 64, 2, 96, 168, False, 1, 0, 0),       # 64 x 128 tiles
    (9, 1, 256, 256, 1, 48, 84, False, 1, 0, 0),      # 64 x 64 tiles, no split
    (9, 2, 512, 512, 1, 48, 84, False, 1, 0, 0),      # 64 x 64 tiles, K split (layer4.0.conv2 of a 768x1344 frame)
]


def case_id(c):
    return '%dx%d-s%d-%dto%d-B%d-%dx%d%s%s%s' % (3 if c[0] == 9 else 1, 3 if c[0] == 9 else 1, c[1], c[2], c[3], c[4],
                                                  c[5], c[6], '-res' if c[7] else '', '-relu' if c[8] else '',
                                                  '-ld+%d' % c[9] if c[9] else '')


EXACT_IDS = [case_id(c) for c in EXACT]

RANDOM = [
    (1, 1, 128, 192, 2, 9, 13, True, 1, 0, 0),
    (1, 2, 256, 128, 1, 9, 12, False, 0, 0, 0),
    (9, 1, 64, 128, 1, 7, 9, True, 1, 0, 0),
    (9, 2, 128, 64, 2, 10, 13, False, 1, 0, 0),
]
RANDOM_IDS = [case_id(c) for c in RANDOM]


def _operands(case, seed, exact):
    taps, stride, c_in, c_out, B, h, w, res, _, _, ld_r = case
    k = 3 if taps == 9 else 1
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    g = torch.Generator().manual_seed(seed)
    if exact:
        x = torch.randint(-1, 2, (B, c_in, h, w), generator=g).float()
        keep = torch.rand((c_out, c_in, k, k), generator=g) < min(1.0, 80.0 / (c_in * taps))
        wt = torch.randint(-1, 2, (c_out, c_in, k, k), generator=g).float() * keep
        scale = 2.0 ** torch.randint(-1, 2, (c_out,), generator=g).float()
        shift = torch.randint(-3, 4, (c_out,), generator=g).float()
        resid = torch.randint(-8, 9, (B * oh * ow, c_out + ld_r), generator=g).float() if res else None
    else:
        x = torch.randn((B, c_in, h, w), generator=g)
        wt = torch.randn((c_out, c_in, k, k), generator=g) / (c_in * taps) ** 0.5
        scale = 0.5 + torch.rand((c_out,), generator=g)
        shift = torch.randn((c_out,), generator=g)
        resid = torch.randn((B * oh * ow, c_out + ld_r), generator=g) if res else None
    return x, wt, scale, shift, resid


def _reference(case, x, wt, scale, shift, resid, f):
    """(ref, mag, pre-ReLU ref) [B oh ow, c_out] in dtype f."""
    taps, stride, _, c_out = case[:4]
    pad = 1 if taps == 9 else 0
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, c_out)   # noqa: E731
    acc = flat(F.conv2d(x.to(f), wt.to(f), None, stride, pad))
    amag = flat(F.conv2d(x.to(f).abs(), wt.to(f).abs(), None, stride, pad))
    ref = acc * scale.to(f) + shift.to(f)
    mag = amag * scale.to(f).abs() + shift.to(f).abs()
    if resid is not None:
        ref, mag = ref + resid[:, :c_out].to(f), mag + resid[:, :c_out].to(f).abs()
    return (ref.clamp_min(0) if case[8] else ref), mag, ref, amag


def _run(lib, prec, case, x, wt, scale, shift, resid, ld_x_extra=0):
    taps, stride, c_in, c_out, B, h, w, _, relu, ld_extra, ld_r = case
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    dt = DT(lib, prec)
    xd = torch.full((B * h * w, c_in + ld_x_extra), 3.0, dtype=TDT[prec], device='cuda')
    xd[:, :c_in] = x.permute(0, 2, 3, 1).reshape(-1, c_in).to(TDT[prec]).cuda()
    wd = wt.permute(0, 2, 3, 1).reshape(c_out, -1).to(TDT[prec]).contiguous().cuda()
    sc, sh = scale.float().cuda(), shift.float().cuda()
    rd = None if resid is None else resid.to(TDT[prec]).cuda().contiguous()
    y = Out((B * oh * ow, c_out + ld_extra), TDT[prec])
    nbytes = lib.load().sfvos_conv2d_workspace_bytes(dt, B, h, w, c_in, c_out, taps, stride)
    sp = ctypes.c_int()
    plan = lib.load().sfvos_conv2d_plan(dt, B, h, w, c_in, c_out, taps, stride, 0, ctypes.byref(sp))
    assert (nbytes > 0) == (sp.value > 1) == (plan >= 3)
    ws = Out((max(nbytes // 4, 1),), torch.float32, fill=float('nan'))
    lib.call('sfvos_conv2d', P(xd), xd.shape[1], P(wd), P(sc), P(sh), None if rd is None else P(rd), c_out + ld_r, P(y.t),
             c_out + ld_extra, B, h, w, c_in, c_out, taps, stride, relu, dt, P(ws.t) if nbytes else None, S())
    torch.cuda.synchronize()
    assert ws.guards_ok(), 'wrote outside the workspace'
    got = y.cpu()
    if ld_extra:
        assert bool((got[:, c_out:] == SENT).all()), 'wrote the neighbouring columns'
    return got[:, :c_out].float(), plan, sp.value


_EXACT_REF = {}


def _exact_reference(case):
    """Operands and reference of an exact case, computed once for both precisions and never modified."""
    if case not in _EXACT_REF:
        ops = _operands(case, 21, True)
        # integers below 2^24 are exact in fp32: the float32 conv IS the float64 one (and much faster on the CPU)
        _EXACT_REF[case] = ops + _reference(case, *ops, torch.float32)
    return _EXACT_REF[case]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', EXACT, ids=EXACT_IDS)
def test_conv2d_exact(lib, case, prec):
    x, wt, scale, shift, resid, ref, mag, pre, amag = _exact_reference(case)
    assert float(amag.max()) < 2 ** 24 and float(pre.abs().max()) <= 256 and bool((2 * pre == (2 * pre).round()).all())
    if case[0] == 9:
        assert not torch.equal(wt, wt.flip(2)) and not torch.equal(wt, wt.flip(3)) and not torch.equal(
            wt, wt.transpose(2, 3))
    assert not torch.equal(wt[:64, :64, 0, 0], wt[:64, :64, 0, 0].t())
    got, plan, splits = _run(lib, prec, case, x, wt, scale, shift, resid, ld_x_extra=64 if case[9] else 0)
    check_exact('conv2d exact %s %s (plan %d, %d splits)' % (prec, case_id(case), plan, splits), got, ref)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', RANDOM, ids=RANDOM_IDS)
def test_conv2d_against_float64(lib, case, prec):
    x, wt, scale, shift, resid = _operands(case, 22, False)
    x, wt = rnd(x, prec), rnd(wt, prec)
    if resid is not None:
        resid = rnd(resid, prec)
    got, _, _ = _run(lib, prec, case, x, wt, scale, shift, resid)
    ref, mag, _, _ = _reference(case, x, wt, scale, shift, resid, torch.float64)
    check('conv2d %s %s' % (prec, case_id(case)), got, ref, mag, case[2] * case[0] + 2, U_OUT[prec])


@pytest.mark.parametrize('prec', PRECS)
def test_conv2d_split_is_deterministic(lib, prec):
    case = (9, 1, 512, 512, 1, 3, 4, False, 1, 0, 0)
    x, wt, scale, shift, resid = _operands(case, 23, False)
    a, plan, splits = _run(lib, prec, case, x, wt, scale, shift, resid)
    b, _, _ = _run(lib, prec, case, x, wt, scale, shift, resid)
    assert plan == 5 and splits > 1
    assert torch.equal(a, b)


# ---- stem ----

def _stem_weight(wt, prec):
    """[64, 3, 7, 7] -> the [64][176] image sfvos_body_stem reads."""
    return F.pad(F.pad(wt, (0, 1)).reshape(64, 168), (0, 8)).to(TDT[prec]).contiguous().cuda()


def _stem_run(lib, prec, x, wt, scale, shift, ld_extra):
    B, _, h, w = x.shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    big = torch.full((B, 5, h + 2, w + 5), 1e30, dtype=torch.float32, device='cuda')   # finite: 0 * 1e30 would still be 0
    xd = big[:, 1:4, 1:h + 1, 3:w + 3]
    xd.copy_(x)
    assert xd.stride(3) == 1 and xd.stride(1) != h * w
    y = Out((B * oh * ow, 64 + ld_extra), TDT[prec])
    wd, sc, sh = _stem_weight(wt, prec), scale.float().cuda(), shift.float().cuda()    # held until the kernel has run
    lib.call('sfvos_body_stem', P(xd), xd.stride(0), xd.stride(1), xd.stride(2), xd.stride(3), B, h, w, P(wd), P(sc),
             P(sh), P(y.t), 64 + ld_extra, DT(lib, prec), S())
    torch.cuda.synchronize()
    got = y.cpu()
    if ld_extra:
        assert bool((got[:, 64:] == SENT).all()), 'wrote the neighbouring columns'
    return got[:, :64].float()


def _stem_reference(x, wt, scale, shift, f):
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 64)   # noqa: E731
    acc = flat(F.conv2d(x.to(f), wt.to(f), None, 2, 3))
    amag = flat(F.conv2d(x.to(f).abs(), wt.to(f).abs(), None, 2, 3))
    pre = acc * scale.to(f) + shift.to(f)
    return pre.clamp_min(0), amag * scale.to(f).abs() + shift.to(f).abs(), pre


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('B,h,w', [(2, 70, 100), (1, 64, 96)])
def test_stem_exact(lib, B, h, w, prec):
    g = torch.Generator().manual_seed(24)
    x = torch.randint(-1, 2, (B, 3, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (64, 3, 7, 7), generator=g).float() * (torch.rand((64, 3, 7, 7), generator=g) < 0.6)
    scale = 2.0 ** torch.randint(-1, 2, (64,), generator=g).float()
    shift = torch.randint(-3, 4, (64,), generator=g).float()
    ref, mag, pre = _stem_reference(x, wt, scale, shift, torch.float32)
    assert float(pre.abs().max()) <= 256 and bool((2 * pre == (2 * pre).round()).all())
    assert not torch.equal(wt, wt.flip(2)) and not torch.equal(wt, wt.flip(3)) and not torch.equal(wt, wt.transpose(2, 3))
    got = _stem_run(lib, prec, x, wt, scale, shift, 64 if B == 2 else 0)
    check_exact('body_stem exact %s %dx%dx%d' % (prec, B, h, w), got, ref)


@pytest.mark.parametrize('prec', PRECS)
def test_stem_against_float64(lib, prec):
    g = torch.Generator().manual_seed(25)
    x = rnd(torch.randn((2, 3, 37, 51), generator=g), prec)
    wt = rnd(torch.randn((64, 3, 7, 7), generator=g) / 147 ** 0.5, prec)
    scale, shift = 0.5 + torch.rand((64,), generator=g), torch.randn((64,), generator=g)
    got = _stem_run(lib, prec, x, wt, scale, shift, 0)
    ref, mag, _ = _stem_reference(x, wt, scale, shift, torch.float64)
    check('body_stem %s 2x37x51' % prec, got, ref, mag, 148, U_OUT[prec])


# ---- pool ----

@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('h,w', [(5, 7), (6, 8), (1, 1)])
def test_maxpool_exact(lib, h, w, prec):
    B = 2
    C = 40 if prec == 'bf16' else 20          # 5 chunks of 16 bytes: not a multiple of 32 channels
    ld_src, ld_dst = C + 24, C + 8
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator().manual_seed(26)
    src = torch.randint(-128, 129, (B, h, w, ld_src), generator=g).float()
    src[0] = -src[0].abs() - 1                # image 0: every window all-negative, the borders' too
    src[1, 0], src[1, :, 0] = -src[1, 0].abs() - 1, -src[1, :, 0].abs() - 1
    dst = Out((B * oh * ow, ld_dst), TDT[prec])
    sd = src.to(TDT[prec]).cuda()
    lib.call('sfvos_maxpool3x3s2', P(sd), ld_src, P(dst.t), ld_dst, B, h, w, C, DT(lib, prec), S())
    torch.cuda.synchronize()
    got = dst.cpu().float()
    ref = F.max_pool2d(src[..., :C].permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, C)
    assert float(ref[:oh * ow].max()) < 0
    check_exact('maxpool3x3s2 %s %dx%d' % (prec, h, w), got[:, :C], ref)
    assert bool((got[:, C:] == SENT).all()), 'wrote the neighbouring columns'
