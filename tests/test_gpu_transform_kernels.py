"""GPU: the kernels of csrc/transform.hip alone, through the C ABI.  Every destination is pre-filled with NaN and lies
inside a wider allocation: one guard row below and at least four guard columns to the right of every Hp x Wp plane (NaN,
must stay NaN), and kernel_util's guard bands around the whole.

sfvos_transform_image, exact cases (transform_ref.EXACT_CASES, preconditions asserted in test_transform_ref_cpu.py): small
integer pixels, integer mean, power-of-two std, out = in, 2 in, 4 in, in / 2, so every weight is a multiple of 1/8 and every
intermediate exact: got == the float64 F.interpolate reference, the pad is +0.0 to the bit.  Batch 1, and batch 3 read
through a non-contiguous batch stride.

General cases (transform_ref.GENERAL_CASES, random images in [0, 1], ImageNet mean / std): per element
    |got - ref| <= 8 * 2^-24 * mag + 2^-22 * h * D_h + 2^-22 * w * D_w
with ref the float64 F.interpolate reference and mag, D_h, D_w from the second formulation (transform_ref's docstring
derives the terms; none is measured).  Worst error / bound observed on an MI355X: 0.171 (37x53 -> 58x83), 0.163
(50x70 -> 33x46), from bytes 0.074 (5x7 -> 8x11) and 0.171 (37x53 -> 58x83); the second formulation itself lies at 0.18 /
0.17 of the lambda term from the reference (test_transform_ref_cpu.py), so what is seen is the fp32 source coordinate, as
derived; every exact case equal, the pad +0.0, a second run bit-identical.

Byte source: [N, h, w, 3] frames read in place through their strides; the result is bit-identical to the fp32 path on
u.float() / 255 computed by torch on the GPU.  The divisor is passed as a tensor: with a Python scalar torch multiplies by
the reciprocal on the GPU, which differs from the correctly rounded quotient -- ToTensor's on the CPU, and the kernel's --
for 126 of the 256 byte values (measured on an MI355X); the test asserts that the quotients it feeds are the CPU's.

sfvos_transform_masks: equal to F.interpolate on the CPU (transform_ref.MASK_CASES, among them the pair where fp32 and
integer index arithmetic differ), G = 0 and G = 3, bytes around the output untouched."""
import pytest
import torch

import transform_ref as R
from kernel_util import Out, P, S, check_abs, check_exact, lib  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float('nan')


class Dest:
    """[B, 3, Hp, Wp] fp32 inside a NaN-filled [B, 3, Hp + 1, Ws] allocation (Ws >= Wp + 4, a multiple of 4)."""

    def __init__(self, B, Hp, Wp):
        self.shape = (B, 3, Hp, Wp)
        Ws = (Wp + 3) // 4 * 4 + 4
        self.out = Out((B, 3, Hp + 1, Ws), fill=NAN)
        self.t = self.out.t

    def strides(self):
        return self.t.stride(0), self.t.stride(1), self.t.stride(2)

    def result(self):
        """The Hp x Wp planes on the CPU, after checking that everything around them is untouched."""
        _, _, Hp, Wp = self.shape
        full = self.out.cpu()
        assert bool(torch.isnan(full[:, :, Hp:]).all()), 'wrote below the tensor'
        assert bool(torch.isnan(full[:, :, :, Wp:]).all()), 'wrote right of the tensor'
        return full[:, :, :Hp, :Wp]


def run_image(lib, src, u8, hw, size, shape, mean, std):
    """src: device [B, 3, h, w] fp32 or [B, h, w, 3] uint8, any strides -> the [B, 3, Hp, Wp] result on the CPU."""
    B = src.shape[0]
    if u8:
        sb, sh, sw, sc = src.stride()
    else:
        sb, sc, sh, sw = src.stride()
    d = Dest(B, *shape)
    db, dc, dh = d.strides()
    lib.call('sfvos_transform_image', P(src), lib.U8 if u8 else lib.F32, sb, sc, sh, sw, B, hw[0], hw[1], *(
        tuple(mean) + tuple(std) + (P(d.t), db, dc, dh, size[0], size[1], shape[0], shape[1], S())))
    torch.cuda.synchronize()
    return d.result()


def assert_pad_is_plus_zero(got, size):
    bits = got.contiguous().view(torch.int32)
    assert bool((bits[:, :, size[0]:] == 0).all()) and bool((bits[:, :, :, size[1]:] == 0).all()), 'pad is not +0.0'


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('src,size,shape', R.EXACT_CASES, ids=str)
def test_transform_image_exact(lib, src, size, shape, batch):
    x = R.exact_image(5, batch, *src)
    ref = R.reference_image(x, size, shape, R.EXACT_MEAN, R.EXACT_STD)
    if batch == 1:
        xd = x.cuda()
    else:                                   # every second image of a wider allocation, the others NaN
        wide = torch.full((batch, 2) + tuple(x.shape[1:]), NAN, device='cuda')
        wide[:, 0] = x.cuda()
        xd = wide[:, 0]
        assert xd.stride(0) == 2 * 3 * src[0] * src[1]
    got = run_image(lib, xd, False, src, size, shape, R.EXACT_MEAN, R.EXACT_STD)
    check_exact('transform_image %s -> %s in %s, batch %d' % (src, size, shape, batch), got, ref)
    assert_pad_is_plus_zero(got, size)


@pytest.mark.parametrize('src,size,shape', R.GENERAL_CASES, ids=str)
def test_transform_image_general(lib, src, size, shape):
    x = R.random_image(3, 2, *src)
    ref = R.reference_image(x, size, shape)
    _, mag, dh, dw, _ = R.formula_image(x, size, shape)
    got = run_image(lib, x.cuda(), False, src, size, shape, R.MEAN, R.STD)
    check_abs('transform_image %s -> %s in %s' % (src, size, shape), got, ref, R.bound(mag, dh, dw, *src))
    assert_pad_is_plus_zero(got, size)
    again = run_image(lib, x.cuda(), False, src, size, shape, R.MEAN, R.STD)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'not bit-identical from run to run'


@pytest.mark.parametrize('src,size,shape', [((5, 7), (8, 11), (8, 12)), ((37, 53), (58, 83), (64, 96))], ids=str)
def test_transform_image_bytes_equal_the_fp32_path(lib, src, size, shape):
    g = torch.Generator().manual_seed(17)
    u = torch.randint(0, 256, (2,) + src + (3,), generator=g, dtype=torch.uint8)
    u[0, 0, 0], u[0, 0, 1] = torch.tensor([0, 255, 1], dtype=torch.uint8), torch.tensor([254, 127, 128], dtype=torch.uint8)
    ud = u.cuda()
    assert ud.stride() == (src[0] * src[1] * 3, src[1] * 3, 3, 1)
    x = (ud.float() / torch.tensor(255.0, device='cuda')).permute(0, 3, 1, 2).contiguous()
    # the division torch made is IEEE's: every byte against the CPU's quotient
    table = torch.arange(256, dtype=torch.float32)
    assert torch.equal((table.cuda() / torch.tensor(255.0, device='cuda')).cpu(), table / torch.tensor(255.0))
    a = run_image(lib, ud, True, src, size, shape, R.MEAN, R.STD)
    b = run_image(lib, x, False, src, size, shape, R.MEAN, R.STD)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert_pad_is_plus_zero(a, size)
    # and it is the transform of the converted image
    ref = R.reference_image(x.cpu(), size, shape)
    _, mag, dh, dw, _ = R.formula_image(x.cpu(), size, shape)
    check_abs('transform_image bytes %s -> %s' % (src, size), a, ref, R.bound(mag, dh, dw, *src))


@pytest.mark.parametrize('G', [0, 3])
@pytest.mark.parametrize('src,size', R.MASK_CASES, ids=str)
def test_transform_masks(lib, src, size, G):
    m = R.random_masks(9, G, *src)
    if G and src[0] == R.NEAREST_FP32_PAIR['n_in']:
        m[0] = torch.arange(src[0], dtype=torch.uint8)[:, None].expand(src).contiguous()      # rows hold their own index
    ref = R.reference_masks(m, size)
    n = G * size[0] * size[1]
    buf = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device='cuda')
    md = m.cuda()
    lib.call('sfvos_transform_masks', P(md) if G else None, G, src[0], src[1], P(buf, 64), size[0], size[1], S())
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:64] == 0xA5).all()) and bool((host[64 + n:] == 0xA5).all()), 'wrote outside its buffer'
    got = host[64:64 + n].view((G,) + tuple(size))
    assert torch.equal(got, ref), '%d of %d bytes differ' % (int((got != ref).sum()), n)
    if G and src[0] == R.NEAREST_FP32_PAIR['n_in']:
        p = R.NEAREST_FP32_PAIR
        assert int(got[0, p['d'], 0]) == p['fp32'] != p['integer']


def test_transform_masks_unaligned_destination(lib):
    """A destination that starts at an odd address: the word store gives way to byte stores, same bytes."""
    src, size = (37, 53), (58, 83)
    m = R.random_masks(4, 2, *src)
    ref = R.reference_masks(m, size)
    n = 2 * size[0] * size[1]
    buf = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device='cuda')
    md = m.cuda()
    lib.call('sfvos_transform_masks', P(md), 2, src[0], src[1], P(buf, 61), size[0], size[1], S())
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:61] == 0xA5).all()) and bool((host[61 + n:] == 0xA5).all())
    assert torch.equal(host[61:61 + n].view((2,) + size), ref)
