"""Torch-core restatement of what torchvision's GeneralizedRCNNTransform does to the pixels (normalize, resize, batch_images'
zero pad, the nearest resize of the target masks), for the tests of csrc/transform.hip and sfvos_amd.transform.
torchvision is absent here: PARITY UNPINNED BY THE REFERENCE.  Its core is torch's own F.interpolate on the CPU.

reference_image   normalize in float64, F.interpolate(scale_factor=..., mode='bilinear', recompute_scale_factor=True,
                  align_corners=False) in float64, zero pad: what every GPU result is compared with.
formula_image     the second formulation: the index and weight arithmetic of include/sfvos.h in fp32 (torch's fp32 CPU
                  ops, every operation rounded on its own), normalisation and blending in float64.  It also returns the
                  terms of the GPU tests' bound:
                      |got - ref| <= 8 * 2^-24 * mag + 2^-22 * h * D_h + 2^-22 * w * D_w
                  mag = sum over the four taps of weight * (|x| + |mean|) / std; the 8 covers one subtract, one divide, the
                  two weight products and three blend roundings, doubled.  D_h (D_w): the largest difference between
                  vertically (horizontally) adjacent normalised source values among the taps and their neighbours one
                  further out in both directions; each term bounds the few fp32 roundings of the source coordinate
                  (each <= 2^-24 * in) times the local slope, and since the interpolant is continuous and the neighbours
                  are included, a floor that falls on the other side of an integer stays inside it.
reference_masks   F.interpolate(mask[:, None].float(), size=size)[:, 0].byte().
formula_masks     the header's nearest rule, min((int)floorf(d * scale), in - 1) with scale = (float)in / (float)out in fp32.

fp32 against integer arithmetic in the nearest rule: a search over every in, out <= 2048 and every d < out finds 1728
values of `in` with at least one (out, d) where floorf(d * scale) in fp32 differs from d * in // out; the pair with the
smallest sides is in = 26, out = 22 at d = 11 (d * in / out = 13 exactly, fp32 gives 12.999999 -> 12).  NEAREST_FP32_PAIR is
among the mask cases of the GPU tests; torch's own nearest kernel takes the fp32 value there, as the kernel does."""
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
NEAREST_FP32_PAIR = dict(n_in=26, n_out=22, d=11, fp32=12, integer=13)
U24 = 2.0 ** -24
U22 = 2.0 ** -22

# the mask cases of tests/test_gpu_transform_kernels.py: (h, w) -> (oh, ow); the last is NEAREST_FP32_PAIR on both axes
MASK_CASES = [((5, 7), (8, 11)), ((37, 53), (58, 83)), ((50, 70), (33, 46)), ((26, 26), (22, 22))]
# its general image cases: (h, w) -> (oh, ow) in (Hp, Wp)
GENERAL_CASES = [((37, 53), (58, 83), (64, 96)), ((50, 70), (33, 46), (64, 64))]


def _f32_as_f64(values):
    """The fp32 values the kernel receives, as float64."""
    return torch.tensor(values, dtype=torch.float32).double()


def normalize64(x, mean=MEAN, std=STD):
    """(x - mean) / std in float64; x [N, 3, h, w] (any floating dtype), mean / std as the fp32 values the kernel gets."""
    return (x.double() - _f32_as_f64(mean)[None, :, None, None]) / _f32_as_f64(std)[None, :, None, None]


def interpolate64(v, size):
    """F.interpolate with recompute_scale_factor=True to (oh, ow): the scale factors (out + 0.5) / in floor to the size."""
    h, w = v.shape[-2:]
    out = F.interpolate(v, scale_factor=((size[0] + 0.5) / h, (size[1] + 0.5) / w), mode='bilinear',
                        recompute_scale_factor=True, align_corners=False)
    assert tuple(out.shape[-2:]) == tuple(size), (out.shape, size)
    return out


def pad64(v, shape):
    out = v.new_zeros(v.shape[:2] + tuple(shape))
    out[..., :v.shape[2], :v.shape[3]] = v
    return out


def reference_image(x, size, shape, mean=MEAN, std=STD):
    """x [N, 3, h, w] -> float64 [N, 3, Hp, Wp]."""
    return pad64(interpolate64(normalize64(x, mean, std), size), shape)


def source_index(n_in, n_out):
    """The header's fp32 arithmetic for one axis -> (i0, i1 int64, l0, l1 float32) of every output index."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    d = torch.arange(n_out, dtype=torch.float32)
    src = (scale * (d + 0.5) - 0.5).clamp_min(0.0)
    assert src.dtype == torch.float32
    i0 = src.to(torch.int64)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = src - i0.to(torch.float32)
    l0 = 1.0 - l1
    return i0, i1, l0, l1


def _adjacent_max(v, axis, lo, hi, other_lo, other_hi):
    """Per output pixel, max |v[r + 1] - v[r]| along `axis` (2: rows, 3: columns) over the pairs r in {lo - 1, lo, hi} and
    the positions {other_lo - 1, other_lo, other_hi, other_hi + 1} of the other axis, all clamped to the image.  lo / hi:
    the taps' indices along `axis` per output index, other_lo / other_hi: along the other axis.  None for one row / column."""
    n, m = v.shape[axis], v.shape[5 - axis]
    if n == 1:
        return None
    diff = (v.narrow(axis, 1, n - 1) - v.narrow(axis, 0, n - 1)).abs()          # pair r = (r, r + 1)
    best = None
    for r in (lo - 1, lo, hi):
        rr = r.clamp(0, n - 2)
        for c in (other_lo - 1, other_lo, other_hi, other_hi + 1):
            cc = c.clamp(0, m - 1)
            g = diff[:, :, rr][:, :, :, cc] if axis == 2 else diff[:, :, cc][:, :, :, rr]
            best = g if best is None else torch.maximum(best, g)
    return best


def formula_image(x, size, shape, mean=MEAN, std=STD):
    """-> (out, mag, D_h, D_w, weights), float64 [N, 3, Hp, Wp] each (zero in the pad); weights = (ly0, ly1, lx0, lx1)
    fp32 vectors.  x [N, 3, h, w]."""
    h, w = x.shape[-2:]
    oh, ow = size
    v = normalize64(x, mean, std)
    a = (x.double().abs() + _f32_as_f64(mean).abs()[None, :, None, None]) / _f32_as_f64(std)[None, :, None, None]
    y0, y1, ly0, ly1 = source_index(h, oh)
    x0, x1, lx0, lx1 = source_index(w, ow)
    wy0, wy1 = ly0.double()[:, None], ly1.double()[:, None]
    wx0, wx1 = lx0.double()[None, :], lx1.double()[None, :]

    def blend(t):
        left = wy0 * t[:, :, y0][:, :, :, x0] + wy1 * t[:, :, y1][:, :, :, x0]
        right = wy0 * t[:, :, y0][:, :, :, x1] + wy1 * t[:, :, y1][:, :, :, x1]
        return wx0 * left + wx1 * right

    out, mag = blend(v), blend(a)
    zero = torch.zeros_like(out)
    dh = _adjacent_max(v, 2, y0, y1, x0, x1)
    dw = _adjacent_max(v, 3, x0, x1, y0, y1)
    dh = zero if dh is None else dh
    dw = zero if dw is None else dw
    return (pad64(out, shape), pad64(mag, shape), pad64(dh, shape), pad64(dw, shape), (ly0, ly1, lx0, lx1))


def bound(mag, dh, dw, h, w):
    """The per-element bound of the GPU tests (module docstring); h, w: the SOURCE sides."""
    return 8 * U24 * mag + U22 * h * dh + U22 * w * dw


def lambda_term(dh, dw, h, w):
    return U22 * h * dh + U22 * w * dw


def reference_masks(masks, size):
    """masks uint8 [G, h, w] -> uint8 [G, oh, ow], as torchvision's transform resizes them."""
    return F.interpolate(masks[:, None].float(), size=tuple(size))[:, 0].byte()


def nearest_index(n_in, n_out):
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    d = torch.arange(n_out, dtype=torch.float32)
    return torch.floor(d * scale).to(torch.int64).clamp_max(n_in - 1)


def formula_masks(masks, size):
    return masks[:, nearest_index(masks.shape[1], size[0])][:, :, nearest_index(masks.shape[2], size[1])]


def random_image(seed, n, h, w):
    """Images as ToTensor makes them, in [0, 1], fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, h, w), generator=g, dtype=torch.float32)


def random_masks(seed, G, h, w):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((G, h, w), generator=g) < 0.5).to(torch.uint8) * torch.randint(1, 255, (G, 1, 1), generator=g,
                                                                                      dtype=torch.uint8)


# ---- exact cases: small integers, integer mean, power-of-two std, out = in, 2 in, 4 in, in / 2 ----
EXACT_MEAN = (3.0, -2.0, 5.0)
EXACT_STD = (0.5, 2.0, 4.0)


def exact_image(seed, n, h, w):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (n, 3, h, w), generator=g).float()


def is_dyadic(t, bits):
    """Every element an integer multiple of 2^-bits with a magnitude below 2^(24 - bits): exact in fp32 with room."""
    s = t.double() * 2.0 ** bits
    return bool((s == s.round()).all()) and bool((s.abs() < 2.0 ** 24).all())


# (source h, w) -> (oh, ow) in (Hp, Wp): out = in, 2 in, 4 in, in / 2 per axis; ow % 4 takes 0, 1, 2 and 3, so the boundary
# between the image and the pad falls inside a thread's four pixels; ow == Wp; oh == Hp; a pad wider than the image; Wp no
# multiple of 4.  Each runs with batch 1 and with batch 3 behind a non-contiguous batch stride.
EXACT_CASES = [
    ((1, 1), (1, 1), (1, 1)),        # ow % 4 = 1, ow == Wp, oh == Hp, one group of one pixel
    ((1, 1), (4, 4), (8, 12)),       # pad wider than the image
    ((1, 1), (2, 1), (3, 2)),
    ((2, 3), (2, 3), (2, 4)),        # ow % 4 = 3, oh == Hp
    ((2, 3), (4, 6), (5, 8)),        # ow % 4 = 2
    ((2, 3), (8, 12), (8, 12)),      # ow == Wp and oh == Hp
    ((2, 3), (1, 3), (3, 7)),        # in / 2 along h; Wp % 4 = 3
    ((4, 10), (2, 5), (4, 8)),       # in / 2 on both axes, ow % 4 = 1
    ((5, 7), (5, 7), (6, 9)),        # ow % 4 = 3, Wp % 4 = 1
    ((5, 7), (10, 14), (12, 16)),    # ow % 4 = 2
    ((5, 7), (20, 28), (32, 32)),
    ((5, 7), (10, 28), (10, 300)),   # more than one workgroup per plane; oh == Hp
]
