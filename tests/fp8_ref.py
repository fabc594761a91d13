"""Float64 references of the e4m3 path (precision='fp8', BASELINE config 5) -- the three quantisers
(sfvos_frames_to_groups_fp8, sfvos_pack_weights_fp8, sfvos_bn_apply_fp8: csrc/elementwise.hip, csrc/batchnorm.hip, all three
through pack<SFVOS_FP8> of csrc/elt_util.h) and sfvos_conv3d with SFVOS_FP8 operands (csrc/conv3d.hip) -- in plain torch on
the CPU, and the generators of the inputs of tests/test_gpu_fp8_kernels.py.  tests/test_fp8_ref_cpu.py pins both: the codec
against torch.float8_e4m3fn, the conv against F.conv3d in double, the inputs against the preconditions the GPU tests rely
on.  Never imported by the package.

OCP e4m3, written from the format: 256 codes, value = (-1)^s * 2^(e - 7) * (1 + m / 8) for e = 1..15, subnormals
2^-6 * m / 8 for e = 0, 0x7f / 0xff are NaN, the largest finite value is 448 (0x7e); there is no infinity.  Encoding is
round to nearest, ties to the even code, found in float64 on the sorted table of the 127 non-negative values.  The
library's contract (include/sfvos.h): finite |v| > 448 and +-inf give +-448, NaN stays a NaN code, -0 keeps its sign.

Conv inputs, exactly summable (kernel_util's docstring): x codes q in {-1, 0, 1} standing for x = q / act_scale with
act_scale a power of two; w = j * 2^-k(n), j in {-1, 0, 1}, k(n) = n mod 4, one pilot weight of +-7 per output channel, so
that the weight scale 448 / max|w[n]| = 64 * 2^k(n) is an exact power of two that differs between neighbouring channels and
w * ws is j * 64 or +-448, both e4m3 values.  Then every product q * wq, every partial sum of them in any order (multiples
of 64 below 2^24), the de-quantisation acc * row1 + row0, the bf16 store and S1 / S2 are exact, and the kernel must EQUAL
float64.  The bias is b / act_scale with b in {-2..2}: y is then S * 2^-k / act_scale + b / act_scale with |S + b 2^k| <= 256
units of 2^-k / act_scale, which bf16 holds (an integer bias beside act_scale = 32 would need S + 256 b, ten significand
bits).  `full`: q in [-15, 15], j in [-14, 14] with a pilot of +-14 (ws = 32 * 2^k): all four significand bits of both
operands in use; y is no longer exact in bf16, S1 and the accumulator still are.  `random`: normal x and w, quantised by
the references here."""
import functools

import numpy as np
import torch

from bn_ref import CONV_NONZERO, stats  # noqa: F401  (stats: S1 / S2 of a level)
from conv_bwd_ref import window         # noqa: F401  (frames [t_off, t_off + T), zero frames outside the buffer)

E4M3_MAX = 448.0
NAN_CODE = 0x7f
FILL = 0x7e          # the byte around every x buffer of the conv tests: 448, so that a frame read after all is not zero


# ----------------------------------------------------------------------------------------------- the codec
def _positive_table():
    v = []
    for code in range(0x7f):
        e, m = code >> 3, code & 7
        v.append(2.0 ** -6 * m / 8.0 if e == 0 else 2.0 ** (e - 7) * (1.0 + m / 8.0))
    return torch.tensor(v, dtype=torch.float64)


POS = _positive_table()      # POS[code] for code 0 .. 0x7e, ascending; POS[0x7e] = 448


def e4m3_decode(codes):
    """uint8 codes -> float64 values (NaN for 0x7f / 0xff, -0.0 for 0x80)."""
    c = codes.to(torch.int64)
    mag = c & 0x7f
    v = POS[mag.clamp_max(0x7e)]
    v = torch.where(mag == 0x7f, torch.full_like(v, float('nan')), v)
    return torch.where((c & 0x80) != 0, -v, v)


def e4m3_encode(v):
    """Values (any float dtype) -> uint8 codes: nearest e4m3 value in float64, ties to the even code; |v| > 448 and +-inf
    saturate to +-448; NaN gives 0x7f with the sign of the NaN; the sign of -0 and of values that round to 0 is kept."""
    v = v.double()
    a = v.abs().clamp_max(E4M3_MAX)
    nan = torch.isnan(v)
    a = torch.where(nan, torch.zeros_like(a), a)
    hi = torch.searchsorted(POS, a.contiguous()).clamp(1, 0x7e)     # first table entry >= a (at least 1: lo exists)
    lo = hi - 1
    dl, dh = a - POS[lo], POS[hi] - a
    take_hi = (dh < dl) | ((dh == dl) & (hi % 2 == 0))
    code = torch.where(take_hi, hi, lo)
    code = torch.where(nan, torch.full_like(code, NAN_CODE), code)
    code = code | (torch.signbit(v).to(torch.int64) << 7)
    return code.to(torch.uint8)


def canon(codes):
    """Both NaN codes as 0x7f (the contract leaves the sign of a NaN open)."""
    return torch.where(codes == 0xff, torch.full_like(codes, NAN_CODE), codes)


def _edge_values():
    f32 = np.float32
    pos = POS.numpy()
    vals = [pos.astype(np.float32)]
    mid = ((pos[:-1] + pos[1:]) / 2.0).astype(np.float32)            # five significand bits: exact in fp32
    vals += [mid, np.nextafter(mid, f32(0)), np.nextafter(mid, f32(np.inf))]
    tie0 = f32(2.0 ** -10)                                           # halfway between 0 and 2^-9: rounds to (even) 0
    vals.append(np.array([tie0, np.nextafter(tie0, f32(np.inf)), f32(448), np.nextafter(f32(448), f32(np.inf)), 449, 464,
                          465, 480, 1e6, 3e38, np.inf, np.nan, 0.0], dtype=np.float32))
    v = np.concatenate(vals)
    return torch.from_numpy(np.concatenate([v, -v]))


EDGE_VALUES = _edge_values()     # fp32, both signs


# ----------------------------------------------------------------------------------------------- quantiser references
def quantise(src, scale):
    """sfvos_frames_to_groups_fp8 on fp32 src: (codes, count).  The product is the kernel's fp32 multiply; the count is
    the number of elements with |src * scale| > 448 in fp32 (infinities count, NaN does not)."""
    v = src.float() * torch.tensor(scale, dtype=torch.float32)
    return e4m3_encode(v), int((v.abs() > E4M3_MAX).sum())


def pack_weights_ref(w, bias, act_scale):
    """sfvos_pack_weights_fp8 in fp32: ws[n] = 448 / max|w[n]| (1 for an all-zero channel); rows [3][c_out] = (bias or
    zeros, 1 / (act_scale * ws), ws); codes = encode(w * ws) in w's shape."""
    w = w.float()
    amax = w.abs().reshape(w.shape[0], -1).amax(1)
    ws = torch.where(amax > 0, torch.tensor(E4M3_MAX, dtype=torch.float32) / amax, torch.ones_like(amax))
    row1 = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(act_scale, dtype=torch.float32) * ws)
    row0 = torch.zeros_like(ws) if bias is None else bias.float()
    return torch.stack([row0, row1, ws]), e4m3_encode(w * ws.reshape(-1, 1, 1, 1, 1))


def bn_apply_fp8_ref(x, scale, shift, relu, act_scale):
    """sfvos_bn_apply_fp8 on one level, float64: v = act(x * scale + shift) * act_scale and the two ends of the interval the
    kernel's fp32 value lies in -- fp32 `x * scale + shift`, possibly one FMA, errs by at most 2^-22 (|x scale| + |shift|)
    (bn_ref.ambiguous); act and the multiplication by a power-of-two act_scale add nothing.  Returns (v, lo, hi): codes must
    be encode(lo) or encode(hi) (equal to encode(v) where lo == hi), and the count of |.| > 448 lies between those of the
    ends taken towards and away from zero (sat_bounds)."""
    pre = x * scale + shift
    d = 2.0 ** -22 * ((x * scale).abs() + shift.abs())
    act = (lambda t: t.clamp_min(0.0)) if relu else (lambda t: t)
    return act(pre) * act_scale, act(pre - d) * act_scale, act(pre + d) * act_scale


def sat_bounds(lo, hi):
    """Fewest and most elements beyond +-448 when each value may sit anywhere in [lo, hi]."""
    inner = torch.where((lo <= 0) & (hi >= 0), torch.zeros_like(lo), torch.minimum(lo.abs(), hi.abs()))
    outer = torch.maximum(lo.abs(), hi.abs())
    return int((inner > E4M3_MAX).sum()), int((outer > E4M3_MAX).sum())


# ----------------------------------------------------------------------------------------------- the conv
def conv_ref(win, w, bias):
    """The float64 3x3 conv (zero pad 1 in space, none in time) of a frame window [B, cin, T, H, W] with w [cout, cin, kt, 3,
    3]: one matmul per temporal and spatial tap on shifted channels-last views.  [B, cout, T - kt + 1, H, W]."""
    B, cin, T, H, W = win.shape
    cout, _, kt = w.shape[:3]
    t_out = T - kt + 1
    xp = torch.zeros(B, T, H + 2, W + 2, cin, dtype=torch.float64)
    xp[:, :, 1:1 + H, 1:1 + W] = win.double().permute(0, 2, 3, 4, 1)
    y = torch.zeros(B * t_out * H * W, cout, dtype=torch.float64)
    w = w.double()
    for dt in range(kt):
        for kh in range(3):
            for kw in range(3):
                y += xp[:, dt:dt + t_out, kh:kh + H, kw:kw + W].reshape(-1, cin) @ w[:, :, dt, kh, kw].t()
    if bias is not None:
        y += bias.double()
    return y.reshape(B, t_out, H, W, cout).permute(0, 4, 1, 2, 3).contiguous()


LV_RAGGED = [(9, 17), (5, 40), (1, 2)]     # ragged 4 x 32 (and 8 x 32) tiles
LV_SMALL = [(6, 10), (3, 4)]
# 15 pixel tiles of 8 x 32 per clip on 534 pixels: with five clips the 75 tiles are enough for the planner to choose blocks of
# 4, 2 and 1 frames for seven output frames (below about 70 tiles it takes 2 + 2 + 2 + 1)
LV_MANY_TILES = [(9, 33), (1, 33), (1, 33), (1, 40), (2, 33), (1, 65)]

# name -> (body, B, T, t_alloc, t_off, shapes, cin, cout, kt, layout, gen, act_scale, frame blocks)
# body: 'fs' = the frame-split kernel (c_out 32: 8 x 32 pixel tiles, blocks of 4, 2 and 1 output frames), 'wide' = 128-channel
# blocks of at most two frames on 4 x 32 tiles.  layout: 'grouped' = [cin / 64][M][64] bytes, 'ndhwc' = [M][cin + 64],
# 'bn' = [M][256] written by sfvos_bn_apply_fp8 in two channel slices (192 + 64).  frame blocks: what the planner must
# return for the case to reach the instance it names (test_fp8_ref_cpu.py: rows per level = blocks * tiles).
CONV_CASES = {
    'fs 4+2+1, cin 256':   ('fs', 5, 9, 9, 0, LV_MANY_TILES, 256, 32, 3, 'grouped', 'exact', 32.0, 3),
    'fs 2+2+2+1, cin 256': ('fs', 1, 9, 9, 0, [(24, 42), (17, 48), (12, 21)], 256, 32, 3, 'grouped', 'exact', 1.0, 4),
    'fs cin 64':           ('fs', 2, 5, 5, 0, [(9, 17), (3, 5)], 64, 32, 2, 'grouped', 'exact', 32.0, 2),
    'fs cin 192':          ('fs', 2, 5, 5, 0, [(9, 17), (3, 5)], 192, 32, 2, 'grouped', 'exact', 1.0, 2),
    'fs kt 11, cin 128':   ('fs', 1, 14, 14, 0, [(10, 33)], 128, 32, 11, 'grouped', 'exact', 32.0, 2),
    'fs window inside':    ('fs', 2, 3, 7, 2, [(6, 10), (3, 7)], 64, 32, 2, 'grouped', 'exact', 1.0, 1),
    'fs window beyond':    ('fs', 2, 7, 4, -2, [(6, 10), (3, 7)], 64, 32, 3, 'grouped', 'exact', 32.0, 3),
    'fs ndhwc':            ('fs', 1, 4, 4, 0, [(9, 17), (3, 5)], 128, 32, 2, 'ndhwc', 'exact', 1.0, 2),
    'fs full':             ('fs', 1, 2, 2, 0, LV_SMALL, 64, 32, 1, 'grouped', 'full', 1.0, 1),
    'fs random':           ('fs', 1, 3, 3, 0, LV_SMALL, 64, 32, 2, 'grouped', 'random', 32.0, 1),
    'wide c64 t1':         ('wide', 1, 2, 2, 0, LV_RAGGED, 128, 64, 2, 'grouped', 'exact', 32.0, 1),
    'wide c192 t3':        ('wide', 1, 4, 4, 0, [(12, 21), (5, 9)], 256, 192, 2, 'grouped', 'exact', 1.0, 2),
    'wide c224 two clips': ('wide', 2, 3, 3, 0, LV_RAGGED, 256, 224, 2, 'grouped', 'exact', 32.0, 1),
    'wide c256 t2':        ('wide', 1, 3, 3, 0, [(6, 33)], 128, 256, 2, 'grouped', 'exact', 1.0, 1),
    'wide window inside':  ('wide', 2, 3, 7, 2, [(6, 10), (3, 7)], 128, 192, 2, 'grouped', 'exact', 32.0, 1),
    'wide window beyond':  ('wide', 2, 7, 4, -2, [(6, 10), (3, 7)], 128, 64, 3, 'grouped', 'exact', 1.0, 3),
    'wide ndhwc from bn':  ('wide', 1, 3, 3, 0, [(9, 17), (3, 5)], 256, 192, 2, 'bn', 'exact', 1.0, 1),
    'wide mask head':      ('wide', 33, 1, 1, 0, [(7, 7)], 256, 256, 1, 'grouped', 'exact', 32.0, 1),
    'wide full':           ('wide', 1, 2, 2, 0, LV_SMALL, 64, 64, 1, 'grouped', 'full', 1.0, 1),
    'wide random':         ('wide', 1, 3, 3, 0, LV_SMALL, 64, 192, 2, 'grouped', 'random', 32.0, 1),
}
TILE_ROWS = {'fs': 8, 'wide': 4}


def _seed(name):
    return 2000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def unit(name):
    """[cout] the power of two every y of an exact / full case is an integer multiple of: 2^-k(n) / act_scale."""
    cout, act = CONV_CASES[name][7], CONV_CASES[name][11]
    return 2.0 ** -(torch.arange(cout) % 4).double() / act


@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    """dict of a CONV_CASES row: q per level [B, cin, t_alloc, H, W] float64 (the values the x codes decode to: x * act_scale),
    xcodes per level (uint8, same shape), w [cout, cin, kt, 3, 3] and bias as fp32, wq = decode(encode(w * ws)) / ws in
    float64 (the weights the conv multiplies), rows = pack_weights_ref's [3][cout], and per level ref (conv + bias before
    any ReLU, on the frame window with zero frames outside the buffer), mag (the same on absolute values; random case only:
    the others compare exactly) and acc_mag (a bound of the accumulator's magnitude: max |q| times the largest sum of
    |wq * ws| of an output channel)."""
    _, B, T, t_alloc, t_off, shapes, cin, cout, kt, _, gen, act, _ = CONV_CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    wshape = (cout, cin, kt, 3, 3)
    k = (torch.arange(cout) % 4).double()
    if gen == 'random':
        w = (torch.randn(wshape, generator=g) / float(np.sqrt(cin * kt * 9))).float()
        w[3] *= 7.0
        bias = (torch.randn(cout, generator=g) * 0.1).float()
        xcodes = [quantise(torch.randn(B, cin, t_alloc, H, W, generator=g), act)[0] for H, W in shapes]
    else:
        a, pilot = (1, 7.0) if gen == 'exact' else (14, 14.0)
        density = min(1.0, CONV_NONZERO / (cin * kt * 9))
        j = torch.randint(-a, a + 1, wshape, generator=g).double()
        j = j * (torch.rand(wshape, generator=g) < density)
        flat = j.reshape(cout, -1)
        at = torch.randint(0, flat.shape[1], (cout,), generator=g)
        flat[torch.arange(cout), at] = pilot * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1).double()
        w = (flat.reshape(wshape) * (2.0 ** -k).reshape(-1, 1, 1, 1, 1)).float()
        bias = (torch.randint(-2, 3, (cout,), generator=g).double() / act).float()
        aq = 1 if gen == 'exact' else 15
        xcodes = [e4m3_encode(torch.randint(-aq, aq + 1, (B, cin, t_alloc, H, W), generator=g).double()) for H, W in shapes]
    rows, wcodes = pack_weights_ref(w, bias, act)
    ws = rows[2].double().reshape(-1, 1, 1, 1, 1)
    wq = e4m3_decode(wcodes) / ws
    qs = [e4m3_decode(c) for c in xcodes]
    refs, mags = [], []
    for q in qs:
        win = window(q / act, t_off, T)
        refs.append(conv_ref(win, wq, bias.double()))
        if gen == 'random':
            mags.append(conv_ref(win.abs(), wq.abs(), bias.double().abs()))
    acc = max(float(q.abs().max()) for q in qs) * float((wq * ws).abs().reshape(cout, -1).sum(1).max())
    return dict(q=qs, xcodes=xcodes, w=w, bias=bias, wq=wq, rows=rows, wcodes=wcodes, ref=refs, mag=mags, acc_mag=acc)


# ----------------------------------------------------------------------------------------------- bn_apply_fp8 inputs
def bf16_exact(v):
    return v.float().bfloat16().float() == v.float()


def bn_exact_inputs(C, levels, act_scale, relu, seed=41):
    """Exact case: x small-integer bf16 in [-8, 8], scale 2^e with e in {-1, 0, 1}, shift an integer in [-3, 3]: fp32 with
    or without FMA equals float64.  Channel 2 has scale 1 and shift 0 and carries every EDGE_VALUES / act_scale that bf16
    holds (NaN only without ReLU: fmaxf(NaN, 0) is 0 by IEEE maxNum, torch's relu keeps the NaN -- the contract names
    neither), cycled over the positions of each level.  Per level x [m, C], and scale, shift [L, C], float64."""
    g = torch.Generator().manual_seed(seed + C)
    L = len(levels)
    scale = 2.0 ** torch.randint(-1, 2, (L, C), generator=g).double()
    shift = torch.randint(-3, 4, (L, C), generator=g).double()
    scale[:, 2], shift[:, 2] = 1.0, 0.0
    e = EDGE_VALUES / act_scale
    e = e[bf16_exact(e) | torch.isnan(e)]
    if relu:
        e = e[~torch.isnan(e)]
    xs, at = [], 0
    for m in levels:
        x = torch.randint(-8, 9, (m, C), generator=g).double()
        idx = (at + torch.arange(m)) % e.numel()
        x[:, 2] = e[idx].double()
        at += m
        xs.append(x)
    return xs, scale, shift
