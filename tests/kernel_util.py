"""What the per-kernel GPU tests (test_gpu_kernels.py, test_gpu_maskhead_kernels.py, test_gpu_boxhead_kernels.py,
test_gpu_bn_kernels.py, test_gpu_conv_bwd_kernels.py, test_gpu_fp8_kernels.py) share: pointers and streams for the C ABI, pyramid buffers, level tables, guarded outputs, the
`lib` fixture and the per-element pass criterion; relmax / rel_l2 also serve the module-level GPU tests.

Pass criterion, per element (never max error / max |ref|: a wrong small element hides under a large neighbour there).
For an output that is a sum of K products, with `ref` and `mag` (the same operation on the absolute values of all
operands, bias included) both in float64:

    |got - ref|  <=  u_out * |ref|  +  2 * (K + 1) * 2^-22 * mag

u_out = 2^-8 where the kernel stores bf16 (round to nearest of an 8-bit significand), 0 where it stores fp32.  The second
term is derived, not measured: any order of K fp32 additions rounded to nearest errs by at most K * 2^-24 * mag; the
factor 4 admits MFMA adders that truncate; the factor 2 carries the accumulation error through the final rounding and
the bias add (and, where one operand is bf16 and the other fp32, the rounding of each product).  K is the longest chain
of fp32 additions one product passes through, stated beside each case.  After ReLU the same bound holds with the
pre-ReLU ref (|relu(a) - relu(b)| <= |a - b|); the ReLU cases here take u_out * |ref| from the post-ReLU ref, which is
smaller (0 where ref < 0: there only the accumulation term is left).

Transcendental kernels (mask_logits prob, mask_bce_loss, mask_bce_loss_grad): the allowance is 2^-20 (16 fp32 ulps)
times the float64 sum of the magnitudes of the terms of the kernel's formula.  The 16 is not derived (no ulp bounds for
expf / log1pf are documented with the toolchain): it stands for three roundings and two device-library calls.  One term
is added to the magnitude of a sigmoid: 2^-126 / 2^-20, i.e. an absolute 2^-126, because 1 / (1 + expf(-z)) overflows its
intermediate for z < -88.72, where the result lies below fp32's normal range and carries no relative precision (the
kernel returns exactly 0 there).  prob is compared twice (check_prob): with the float64 sigmoid of the kernel's own
returned logits under that bare allowance, and with the float64 sigmoid of the float64 logit, where the allowance also
carries the distance the derived bound of the logit moves the sigmoid (|sigmoid(z +- zb) - sigmoid(z)|, evaluated, so it
vanishes at the saturated ends).  Worst observed error / allowance on an MI355X: prob 0.12 against its own logits (2 of
the 16 ulps) and 0.058 against the float64 logit, loss 0.017, loss gradient 0.23.  Worst observed error / bound of the
others, per kernel: at most 0.13 where the store is fp32 (the MSE gradient; sums of products at most 0.082), 0.30-0.996
where it is bf16 (that term is the exact rounding bound: approached, not exceeded; every bf16 store rounds to nearest).

The BatchNorm chain (test_gpu_bn_kernels.py, references in bn_ref.py) adds three cases of the same criterion.

Exactly summable operands (check_exact): where the chain is long -- every statistics row of a conv, any level of more
than a few thousand positions -- the K * mag term exceeds what one dropped or doubled position changes and proves
nothing.  There the operands are small integers and power-of-two coefficients for which every partial sum, in any order
and any partition into rows, is an integer multiple of a stated power of two below 2^24 of it: every fp32 addition is
exact, the accumulation term is derived to be ZERO, and the test asserts got == ref (u_out = 0 for statistics and
partial rows, which are sums of the unrounded fp32 values on the bf16 path too; a bf16 y holds |v| <= 256 exactly).
The precondition is asserted on the float64 reference (test_bn_ref_cpu.py: integers or the stated dyadic multiple,
every mag below 2^24, per level sum |v| and sum v^2 below 2^24).  A failure by a non-integer or by less than one product
would be a finding about the adder, not about the test.

Double arithmetic (bn_finalize, bn_bwd_finalize: sums, division, square root in double, cast to float): the allowance
is the cast, 2^-24 * |ref|, plus 2^-45 times the float64 magnitude of the terms of the kernel's formula.  For rstd =
1 / sqrt(var + eps) the second part is the reference evaluated at var +- dv, dv = 2^-45 * (s2 / count + m^2), as
check_prob evaluates the sigmoid at z +- zb; the reference uses the kernel's formula (s2 / count - m^2, clamped at 0) on
the same fp32 rows summed in float64.  The 2^-45 is not derived: it stands for a few hundred double ulps of the device's
double sqrt and divide and of the order of the double sums, for which the toolchain documents no bound.  scale and
shift, fp32 arithmetic on the kernel's own rstd and mean, are compared twice as prob is: with those returned values
(K = 0 / K = 1) and with float64 throughout, the allowances of rstd and mean carried through.

ReLU masks: the kernels define the mask as fp32 `x * scale + shift > 0`, possibly one FMA; float64 can disagree where
that value is within rounding of zero.  Such elements (|x sc + sh| <= 2^-22 (|x sc| + |sh|) and not exactly 0) are not
left out: they get dy = 0 in the input, so both outcomes give the same result (at most 0.1 % of a channel, asserted on
the CPU; none occurs for the committed seeds).  Exact zeros are not ambiguous: the gradient there is 0.

Worst observed error / bound of the BatchNorm chain on an MI355X, per kernel: every exact case equal (24 conv cases with
y, S1, S2 per level, the ReLU y, 7 shift cases, the 512 * 512 + 37 level of bn_bwd_reduce and bn_bwd_apply); bn_finalize
0.996 and bn_bwd_finalize 0.9994 (the cast is the exact rounding bound: approached, not exceeded), scale / shift of
bn_finalize 0.12 / 0.061 against the kernel's own rstd and mean, 0.18 / 0.092 against float64; bn_running_update 0.048;
bn_apply 0.062 (fp32), 0.996 (bf16); bn_bwd_reduce 0.0045; bn_bwd_apply dx 0.087 (fp32), 0.996 (bf16), its bias rows
0.0025, dgamma / dbeta 0.093.

The backward half of the conv (test_gpu_conv_bwd_kernels.py, references in conv_bwd_ref.py): exactly summable operands
throughout.  Weight gradient: x and dy in {-1, 0, 1} (any number of positions below 2^24; the largest case sums 65 520), or
integers in [-127, 127] -- all 8 significand bits of bf16 -- where a case has at most 1000 positions (1000 * 127^2 < 2^24);
the sum runs over positions, tiles, shares, slabs and the sixteen split groups of wgrad_reduce_kernel, all integers below
2^24, so grad_w EQUALS float64, also accumulated onto an integer-filled grad_w, and a second run is bit-identical.  Data
gradient: dy and w in {-1, 0, 1}, about 432 non-zero weights per element of dx, dx an integer of |v| <= 256 with and
without the accumulate prefill in [-8, 8], so the bf16 store is exact too.  The preconditions are asserted on the float64
reference (test_conv_bwd_ref_cpu.py).  One random-operand case per precision (144 positions, normal x and dy) takes the
criterion above with u_out = 0 and K = 144: the only place the full 24-bit fp32 operands pass through the MFMAs.

Worst observed on an MI355X: every exact case equal (38 weight-gradient shapes over wgrad.hip's instances, lateral_wgrad.hip
and wgrad_t1.hip, 56 with the precisions; 15 data-gradient shapes, 22 with the precisions, each with and without accumulate);
the random weight gradient 0.0031 (fp32) and 0.0016 (bf16) of its bound.

The e4m3 path (test_gpu_fp8_kernels.py, references in fp8_ref.py: an OCP e4m3 codec written from the format, pinned against
torch.float8_e4m3fn in test_fp8_ref_cpu.py).  Quantisers (sfvos_frames_to_groups_fp8, sfvos_pack_weights_fp8,
sfvos_bn_apply_fp8): one fp32 product and one rounding to the nearest e4m3 value, ties to even, so codes and saturation
counts EQUAL the reference -- on every e4m3 value, every midpoint and its two fp32 neighbours, 2^-10, around +-448, 1e6, 3e38,
+-inf (all +-448), NaN (a NaN code) and +-0.  Where sfvos_bn_apply_fp8 gets arbitrary fp32 coefficients, its value lies
within 2^-22 (|x scale| + |shift|) * act_scale of float64 (the ReLU-mask interval above; act_scale a power of two), a code
must be the encoding of one end of that interval and the count lie between the counts at the two ends; nothing is left out.
The e4m3 conv: exactly summable operands -- x codes in {-1, 0, 1} standing for q / act_scale, weights j * 2^-k(n) with a
pilot of +-7, so that the per-channel weight scale is a power of two, w * ws an e4m3 value and every product a multiple of 64
below 2^24 -- make y (|y| <= 256 units of 2^-k / act_scale), S1, S2 and the ReLU run EQUAL float64; full-significand operands
(q in [-15, 15], j in [-14, 14]) keep the accumulation term zero and leave the bf16 store, |y - ref| <= 2^-8 |ref|, S1 equal,
S2 under `check` with u_out = 0 and K = c_in * kt * 9; one random case per conv body under `check` with u_out = 2^-8 and
K = c_in * kt * 9 + 1 (the + 1: the rounding of the de-quantisation factor).  The weight image is opaque: a conv over one-hot
x reads back decode(encode(w * ws)) / ws for each of its 73 728 weights.

Worst observed on an MI355X: every code and count equal (9 frames_to_groups_fp8 cases; 12 exact sfvos_bn_apply_fp8 cases; the
random ones with 0 codes outside the interval, 1-13 elements per case with two admissible codes, the count at both ends the
same and met); the three rows of sfvos_pack_weights_fp8 and the image read back equal; every exact conv case equal (16 cases,
y, S1, S2 and the ReLU y per level: v_mfma_scale_f32_32x32x64_f8f6f4 adds integer products below 2^24 exactly); full
significand y 0.9961 (the rounding bound of the store: approached, not exceeded), S2 0.0005; random y 0.46 (frame-split) and
0.59 (wide), S1 0.0009, S2 0.0001.  Before pack<SFVOS_FP8> clamped to +-448 the same tests failed: v_cvt_pk_fp8_f32 alone gave
the NaN code 0x7f for every value that rounds beyond 448 (values up to 464 still round to 448) and for +-inf."""
import ctypes

import numpy as np
import pytest
import torch

TDT = {'fp32': torch.float32, 'bf16': torch.bfloat16}
PRECS = ['fp32', 'bf16']
U_OUT = {'fp32': 0.0, 'bf16': 2.0 ** -8}
U22 = 2.0 ** -22
TRANS = 2.0 ** -20          # allowance of the transcendental kernels, relative to the magnitudes of their terms
FLT_MIN = 2.0 ** -126
GUARD = 64                  # elements in front of and behind every output (keeps 16-byte alignment)
SENT = -768.0               # exact in bf16


@pytest.fixture(scope='module')
def lib():
    from sfvos_amd import _lib
    _lib.check(_lib.load().sfvos_check_device(), 'sfvos_check_device')
    return _lib


def P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def relmax(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def DT(lib, prec):
    return lib.F32 if prec == 'fp32' else lib.BF16


def rnd(t, prec):
    """The operand as the kernel sees it, fp32 on the CPU."""
    return t.bfloat16().float() if prec == 'bf16' else t.float()


class Out:
    """A device output of `shape` between two guard bands, everything sentinel-filled (NaN for workspaces)."""

    def __init__(self, shape, dtype=torch.float32, fill=SENT):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENT, dtype=dtype, device='cuda')
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        if fill != SENT:
            self.t.fill_(fill)

    def guards_ok(self):
        b = self.buf
        return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.n:] == SENT).all())

    def cpu(self):
        assert self.guards_ok(), 'wrote outside its buffer'
        return self.t.cpu()


def check(name, got, ref, mag, K, u_out):
    """The per-element criterion of the module docstring; prints the worst error / bound and where it is."""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double(), mag.detach().double()
    assert got.shape == ref.shape == mag.shape, (name, got.shape, ref.shape, mag.shape)
    assert bool(torch.isfinite(got).all()), '%s: %d non-finite elements' % (name, int((~torch.isfinite(got)).sum()))
    bound = u_out * ref.abs() + 2.0 * (K + 1) * U22 * mag
    return _ratio(name, (got - ref).abs(), bound)


def check_abs(name, got, ref, allow):
    got, ref, allow = got.detach().double().cpu(), ref.detach().double(), allow.detach().double()
    assert got.shape == ref.shape == allow.shape, (name, got.shape, ref.shape, allow.shape)
    assert bool(torch.isfinite(got).all()), '%s: non-finite elements' % name
    return _ratio(name, (got - ref).abs(), allow)


def check_exact(name, got, ref):
    """Exactly summable operands (docstring): the accumulation term of the criterion is derived to be zero, so got == ref.
    Prints how many elements differ and by how much at most."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    diff = (got - ref).abs()
    bad = ~(got == ref)      # NaN differs
    n = int(bad.sum())
    where = ()
    if n:
        worst = int(torch.where(bad, diff.nan_to_num(float('inf')), -torch.ones_like(diff)).reshape(-1).argmax())
        where = tuple(int(i) for i in np.unravel_index(worst, tuple(diff.shape))) if diff.dim() else ()
    print('%-46s exact: %d of %d differ%s' % (name, n, got.numel(), '' if not n else ', most at %s: got %r, ref %r' % (
        where, float(got[where]), float(ref[where]))))
    assert n == 0, '%s: %d of %d elements differ from float64, most at %s: got %r, ref %r' % (
        name, n, got.numel(), where, float(got[where]), float(ref[where]))
    return 0.0


def levels(_lib, ms):
    """sfvos_levels of a flat pyramid buffer with ms[l] positions in level l."""
    lv = _lib.Levels()
    lv.n_levels = len(ms)
    for i, m in enumerate(ms):
        lv.m[i] = m
    return lv


def _ratio(name, err, bound):
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))   # 0 / 0 passes, x / 0 fails
    if ratio.numel() == 0:
        return 0.0
    worst = int(ratio.reshape(-1).argmax())
    w = float(ratio.reshape(-1)[worst])
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape))) if ratio.dim() else ()
    print('%-46s worst error/bound %.4f at %s (%d of %d above)' % (name, w, idx, int((ratio > 1).sum()), ratio.numel()))
    assert w <= 1.0, '%s: error/bound %.3f at %s, %d of %d elements above the bound' % (
        name, w, idx, int((ratio > 1).sum()), ratio.numel())
    return w


def make_desc(_lib, prec, B, T, shapes, cin, cout, kt, taps, pad_t, ld_x, ld_y, acc=0, t_alloc=None, t_offset=0):
    d = _lib.ConvDesc()
    d.dtype = _lib.F32 if prec == 'fp32' else _lib.BF16
    d.batch, d.t_in, d.c_in, d.c_out, d.kt, d.taps, d.pad_t = B, T, cin, cout, kt, taps, pad_t
    d.t_alloc, d.t_offset = (T if t_alloc is None else t_alloc), t_offset
    d.ld_x, d.ld_y, d.accumulate = ld_x, ld_y, acc
    d.pyr = _lib.make_pyramid(shapes)
    return d, T + 2 * pad_t - kt + 1


def to_pyr(levels, prec, ld=None, fill=7.0):
    """list over levels of [B,C,T,H,W] fp32 cpu -> flat pyramid buffer [M, ld] on the device."""
    C = levels[0].shape[1]
    ld = ld or C
    rows = []
    for x in levels:
        rows.append(x.permute(0, 2, 3, 4, 1).reshape(-1, C))
    flat = torch.full((sum(r.shape[0] for r in rows), ld), fill, dtype=torch.float32)
    flat[:, :C] = torch.cat(rows, 0)
    return flat.to(TDT[prec]).cuda()


def from_pyr(flat, B, C, T, shapes):
    """flat [M, ld] device -> list of [B,C,T,H,W] fp32 cpu (first C channels)."""
    out, off = [], 0
    f = flat.float().cpu()
    for (H, W) in shapes:
        n = B * T * H * W
        out.append(f[off:off + n, :C].reshape(B, T, H, W, C).permute(0, 4, 1, 2, 3))
        off += n
    return out
