"""GPU: the e4m3 path (precision='fp8', BASELINE config 5) kernel by kernel through the C ABI -- sfvos_frames_to_groups_fp8,
sfvos_pack_weights_fp8, sfvos_bn_apply_fp8 and sfvos_conv3d with SFVOS_FP8 operands -- each fed float64-chosen inputs and
compared with the references of tests/fp8_ref.py (an e4m3 codec written from the format, pinned in
tests/test_fp8_ref_cpu.py), under the criteria of tests/kernel_util.py (its docstring, e4m3 paragraph):

  codes and saturation counts   EQUAL.  A quantiser is one fp32 product and one rounding to nearest even; its inputs sit
                                on every e4m3 value, every midpoint and the fp32 neighbours of each, around +-448, at
                                +-inf, NaN and +-0.  sfvos_bn_apply_fp8 on random coefficients: a code equals the
                                encoding of either end of the interval fp32 `x * scale + shift` (with or without FMA)
                                lies in, the count lies between the counts at the two ends; nothing is left out.
  conv, exactly summable        y, S1, S2 and the ReLU run EQUAL float64 (check_exact).
  conv, full significand        |y - ref| <= 2^-8 |ref| (the bf16 store; the accumulation term is zero), S1 equal, S2
                                under kernel_util.check with u_out = 0, K = c_in * kt * 9.
  conv, random                  kernel_util.check with u_out = 2^-8, K = c_in * kt * 9 + 1.

Guard bands, sentinel bytes, NaN-filled statistics rows, y in a channel slice of a wider buffer, and x between two frames of
byte 0x7e (448) in front and behind: a frame beyond the window read after all would not meet zeros."""
import ctypes

import pytest
import torch

import bn_ref
import fp8_ref as R
from kernel_util import (GUARD, SENT, Out, P, S, check, check_abs, check_exact, from_pyr, levels, lib,  # noqa: F401
                         make_desc)

pytestmark = pytest.mark.gpu

OFF = 32            # channel offset of the tested slice in an activation buffer
TOFF = 8            # ... in a coefficient table
BSENT = 0x5a        # sentinel byte of e4m3 outputs
NAN = float('nan')


class ByteOut:
    """A device byte buffer of `shape` between two guard bands, everything BSENT."""

    def __init__(self, shape, fill=BSENT):
        self.n = 1
        for s in shape:
            self.n *= int(s)
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=torch.uint8, device='cuda')
        self.fill = fill
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)

    def cpu(self):
        b = self.buf
        assert bool((b[:GUARD] == self.fill).all()) and bool((b[GUARD + self.n:] == self.fill).all()), 'wrote outside its buffer'
        return self.t.cpu()


def table(vals, C):
    """[L, C] float64 -> NaN-filled device table [L][C + 24] with the values at column TOFF; (tensor, pointer, stride)."""
    L = vals.shape[0]
    o = Out((L, C + 24), torch.float32, fill=NAN)
    o.t[:, TOFF:TOFF + C] = vals.float().cuda()
    return o, P(o.t, TOFF), C + 24


def equal_codes(name, got, want):
    got, want = R.canon(got), R.canon(want)
    bad = got != want
    n = int(bad.sum())
    first = ''
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        first = ', first at %d: got 0x%02x, want 0x%02x' % (i, int(got.reshape(-1)[i]), int(want.reshape(-1)[i]))
    print('%-46s codes: %d of %d differ%s' % (name, n, got.numel(), first))
    assert n == 0, '%s: %d of %d codes differ%s' % (name, n, got.numel(), first)


# ------------------------------------------------------------------------------------------ sfvos_frames_to_groups_fp8
@pytest.mark.parametrize('scale', [1.0, 32.0, 0.37])
@pytest.mark.parametrize('shape', [(3, 64, 7, 13), (2, 128, 8, 8), (1, 64, 1, 1)])
def test_frames_to_groups_fp8_codes_and_count_are_equal(lib, shape, scale):
    """The strided [C, T, H, W] view of a frame stack cut out of a larger tensor with huge borders; a normal body wide enough
    to saturate, EDGE_VALUES / scale scattered over it; groups further apart than their T * H * W * 64 bytes, the bytes between
    them untouched.  Codes and the count equal the reference; the count adds to what the counter held, NULL is accepted, a
    second run gives the same bytes and doubles the count."""
    T, C, H, W = shape
    g = torch.Generator().manual_seed(91 + C + H)
    frames = torch.randn(T, C, H, W, generator=g) * (150.0 / scale)
    n = frames.numel()
    e = R.EDGE_VALUES / torch.tensor(scale, dtype=torch.float32)
    where = torch.randperm(n, generator=g)[:min(n, e.numel())]
    frames.view(-1)[where] = e[torch.randperm(e.numel(), generator=g)[:where.numel()]]
    big = torch.full((T, C, H + 2, W + 3), 1e30)
    big[:, :, 1:H + 1, 2:W + 2] = frames
    view = big.cuda()[:, :, 1:H + 1, 2:W + 2].unsqueeze(0).transpose(1, 2)[0]     # [C, T, H, W]
    pos, G = T * H * W, C // 64
    gs = pos * 64 + 128
    codes, count = R.quantise(frames, scale)
    assert count > 0 or n == 64
    want = codes.permute(0, 2, 3, 1).reshape(pos, G, 64).permute(1, 0, 2)

    def run(dst, sat):
        lib.call('sfvos_frames_to_groups_fp8', P(view), view.stride(1), view.stride(0), view.stride(2), view.stride(3),
                 P(dst.t), T, C, H, W, gs, scale, None if sat is None else P(sat), S())
        torch.cuda.synchronize()
        got = dst.cpu().view(G, gs)
        assert bool((got[:, pos * 64:] == BSENT).all()), 'wrote between the groups'
        return got[:, :pos * 64].reshape(G, pos, 64)

    name = 'frames_to_groups_fp8 %s scale %g' % (shape, scale)
    dst, sat = ByteOut((G * gs,)), torch.full((1,), 5, dtype=torch.int32, device='cuda')
    first = run(dst, sat)
    equal_codes(name, first, want)
    assert int(sat) == 5 + count, (int(sat), 5 + count)
    again = run(dst, sat)
    assert torch.equal(again, first) and int(sat) == 5 + 2 * count
    equal_codes(name + ' no counter', run(ByteOut((G * gs,)), None), want)
    print('%-46s count %d equal' % (name, count))


# ------------------------------------------------------------------------------------------ sfvos_pack_weights_fp8
@pytest.mark.parametrize('cout,cin,kt,with_bias', [(64, 64, 2, True), (32, 128, 1, False), (224, 64, 3, True)])
def test_pack_weights_fp8_rows_equal_the_fp32_reference(lib, cout, cin, kt, with_bias):
    """Rows 0, 1 and 2 of bias_descale: the bias (zeros for NULL), 1 / (act_scale * ws) and ws = 448 / max|w[n]| as fp32
    arithmetic (a maximum has no rounding; the divisions round to nearest); channel 5 is all zero: ws = 1."""
    g = torch.Generator().manual_seed(17 + cout)
    w = torch.randn(cout, cin, kt, 3, 3, generator=g) * torch.rand(cout, 1, 1, 1, 1, generator=g) * 3.0
    w[5] = 0.0
    bias = torch.randn(cout, generator=g) if with_bias else None
    act = 32.0 if with_bias else 0.37
    rows, _ = R.pack_weights_ref(w, bias, act)
    wd, bd = w.cuda(), (bias.cuda() if with_bias else None)
    wp, out = ByteOut((w.numel(),)), Out((3, cout), torch.float32, fill=NAN)
    lib.call('sfvos_pack_weights_fp8', P(wd), None if bd is None else P(bd), P(wp.t), P(out.t), cout, cin, kt, 9, act, S())
    torch.cuda.synchronize()
    got = out.cpu()
    assert float(rows[2, 5]) == 1.0
    for r, what in enumerate(('bias', 'descale', 'weight scale')):
        check_exact('pack_weights_fp8 c_out %d row %d (%s)' % (cout, r, what), got[r], rows[r])
    assert not bool((wp.cpu() == BSENT).all())


def test_pack_weights_fp8_image_read_back_through_the_conv(lib):
    """The image is opaque, so the conv reads it: x holds one code of 1.0 per input channel, channel c at its own pixel of a
    24 x 24 frame (3 pixels apart: the 3 x 3 neighbourhoods are disjoint) in the middle frame of three, so every output is
    one weight -- decode(encode(w * ws)) / ws -- or zero.  w holds every EDGE_VALUES of |e| <= 448 times 2^-(n mod 3): ws is
    2^(n mod 3), w * ws the edge value itself, and the bf16 y holds the four significant bits exactly."""
    cout, cin, kt, H, W, T = 64, 64, 2, 24, 24, 3
    e = R.EDGE_VALUES[R.EDGE_VALUES.abs() <= 448.0]
    per_n = cin * kt * 9
    assert per_n >= e.numel()
    idx = (torch.arange(per_n)[None, :] + 37 * torch.arange(cout)[:, None]) % e.numel()
    w = (e[idx] * (2.0 ** -(torch.arange(cout) % 3).float())[:, None]).reshape(cout, cin, kt, 3, 3)
    rows, wcodes = R.pack_weights_ref(w, None, 1.0)
    assert torch.equal(rows[2], 2.0 ** (torch.arange(cout) % 3).float())
    assert torch.equal(R.canon(wcodes), R.canon(R.e4m3_encode(e[idx]).reshape(w.shape)))
    q = torch.zeros(1, cin, T, H, W, dtype=torch.float64)
    c = torch.arange(cin)
    q[0, c, 1, 3 * (c // 8) + 1, 3 * (c % 8) + 1] = 1.0
    ref = R.conv_ref(q, R.e4m3_decode(wcodes) / rows[2].double().reshape(-1, 1, 1, 1, 1), None)
    assert int((ref != 0).sum()) == int((R.e4m3_decode(wcodes) != 0).sum())           # every non-zero weight is read once
    M = T * H * W
    xd = R.e4m3_encode(q)[0].permute(1, 2, 3, 0).reshape(1, M, 64).contiguous().cuda()
    wd = w.cuda()
    wp, bd = ByteOut((w.numel(),)), Out((3, cout), torch.float32, fill=NAN)
    lib.call('sfvos_pack_weights_fp8', P(wd), None, P(wp.t), P(bd.t), cout, cin, kt, 9, 1.0, S())
    d, t_out = make_desc(lib, 'bf16', 1, T, [(H, W)], cin, cout, kt, 9, 0, 64, cout + 2 * OFF)
    d.dtype, d.x_group_stride = lib.FP8, M * 64
    y = Out((t_out * H * W, cout + 2 * OFF), torch.bfloat16)
    lib.call('sfvos_conv3d', ctypes.byref(d), P(xd), P(wp.t), P(bd.t), P(y.t, OFF), None, S())
    torch.cuda.synchronize()
    check_exact('pack_weights_fp8 rows', bd.cpu(), rows)
    wp.cpu()
    check_exact('pack_weights_fp8 image through the conv', from_pyr(act_get(y, cout), 1, cout, t_out, [(H, W)])[0], ref[0:1])


# ------------------------------------------------------------------------------------------ sfvos_bn_apply_fp8
def act_in(levels_, C):
    """Levels [m, C] float64 -> device bf16 [M, C + 2 * OFF] (7 elsewhere); the slice starts at column OFF."""
    flat = torch.full((sum(v.shape[0] for v in levels_), C + 2 * OFF), 7.0)
    flat[:, OFF:OFF + C] = torch.cat(levels_).float()
    return flat.bfloat16().cuda()


def act_get(o, C):
    t = o.cpu()
    assert bool((t[:, :OFF] == SENT).all()) and bool((t[:, OFF + C:] == SENT).all()), 'wrote outside its channel slice'
    return t[:, OFF:OFF + C]


def run_bn_apply_fp8(lib, xs, scale, shift, relu, act, sat, running=None):
    """-> codes [M, C] on the CPU; y is a channel slice (offset 32) of a [M][256]-byte buffer."""
    ms, C = [x.shape[0] for x in xs], xs[0].shape[1]
    lv = levels(lib, ms)
    xd = act_in(xs, C)
    sc, sh = table(scale, C), table(shift, C)
    y = ByteOut((sum(ms), 256))
    lib.call('sfvos_bn_apply_fp8', P(xd, OFF), C + 2 * OFF, P(y.t, OFF), 256, ctypes.byref(lv), C, sc[1], sh[1], sc[2], relu,
             act, None if sat is None else P(sat), None if running is None else ctypes.byref(running), S())
    torch.cuda.synchronize()
    got = y.cpu()
    assert bool((got[:, :OFF] == BSENT).all()) and bool((got[:, OFF + C:] == BSENT).all()), 'wrote outside its channel slice'
    return got[:, OFF:OFF + C]


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('C', [16, 64, 192])
def test_bn_apply_fp8_exact_coefficients_codes_and_count_are_equal(lib, C, relu):
    """Small-integer bf16 x, power-of-two scale, integer shift: fp32 with or without FMA agrees with float64, so every code
    and the count EQUAL the reference -- on values that saturate (act_scale 32: up to 19 * 32) and on every
    EDGE_VALUES / act_scale bf16 holds, in channel 2."""
    ms = bn_ref.BN_LEVELS
    for act in (1.0, 32.0):
        xs, scale, shift = R.bn_exact_inputs(C, ms, act, relu)
        v = torch.cat([R.bn_apply_fp8_ref(x, scale[l], shift[l], relu, act)[0] for l, x in enumerate(xs)])
        count = int((v.abs() > 448.0).sum())
        assert count > 0
        sat = torch.full((1,), 5, dtype=torch.int32, device='cuda')
        got = run_bn_apply_fp8(lib, xs, scale, shift, relu, act, sat)
        name = 'bn_apply_fp8 exact C %d relu %d act_scale %g' % (C, relu, act)
        equal_codes(name, got, R.e4m3_encode(v))
        assert int(sat) == 5 + count, (int(sat), 5 + count)
        equal_codes(name + ' no counter', run_bn_apply_fp8(lib, xs, scale, shift, relu, act, None), R.e4m3_encode(v))
        print('%-46s count %d equal' % (name, count))


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('C', [16, 64, 192])
def test_bn_apply_fp8_random_coefficients_within_the_fp32_interval(lib, C, relu):
    """Random bf16 x and fp32 coefficients (bn_ref.bwd_inputs), act_scale 128 (a power of two: its product is exact; wide
    enough to saturate): the kernel's fp32 value lies within 2^-22 (|x scale| + |shift|) * act_scale of float64, so its code
    is the encoding of one end of that interval -- equal to both wherever they agree, which is all but a handful -- and the
    count lies between the counts at the two ends.  The running-statistics update folded into the launch gives the bits of
    sfvos_bn_running_update; running = NULL gives the same codes."""
    ms, L, act = bn_ref.BN_LEVELS, len(bn_ref.BN_LEVELS), 128.0
    d = bn_ref.bwd_inputs(C, 'bf16', 0)
    ends = [R.bn_apply_fp8_ref(x, d['scale'][l], d['shift'][l], relu, act) for l, x in enumerate(d['x'])]
    lo, hi = torch.cat([e[1] for e in ends]), torch.cat([e[2] for e in ends])
    clo, chi = R.e4m3_encode(lo), R.e4m3_encode(hi)
    least, most = R.sat_bounds(lo, hi)
    assert least > 0
    # running statistics: rows of a coefficient table, L updates in order
    g = torch.Generator().manual_seed(5 + C)
    means, varsu = table(torch.randn(L, C, generator=g).double(), C), table(torch.rand(L, C, generator=g).double() + 0.1, C)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rm, rv, rm2, rv2 = Out((C,)), Out((C,)), Out((C,)), Out((C,))
    for o, v in ((rm, rm0), (rm2, rm0), (rv, rv0), (rv2, rv0)):
        o.t.copy_(v)
    nbt, nbt2 = (torch.full((), 3, dtype=torch.int64, device='cuda') for _ in range(2))
    run = lib.BnRunning()
    run.running_mean, run.running_var = rm.t.data_ptr(), rv.t.data_ptr()
    run.means, run.vars_unbiased = means[1].value, varsu[1].value
    run.num_batches_tracked, run.n_updates, run.momentum = nbt.data_ptr(), L, bn_ref.MOMENTUM
    sat = torch.zeros(1, dtype=torch.int32, device='cuda')
    got = run_bn_apply_fp8(lib, d['x'], d['scale'], d['shift'], relu, act, sat, run)
    lib.call('sfvos_bn_running_update', P(rm2.t), P(rv2.t), means[1], varsu[1], L, means[2], C, bn_ref.MOMENTUM, P(nbt2), S())
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu(), rm2.cpu()) and torch.equal(rv.cpu(), rv2.cpu()) and int(nbt) == int(nbt2) == 3 + L
    assert not torch.equal(rm.cpu(), rm0)
    g_, a, b = R.canon(got), R.canon(clo), R.canon(chi)
    bad = (g_ != a) & (g_ != b)
    name = 'bn_apply_fp8 random C %d relu %d' % (C, relu)
    print('%-46s codes: %d of %d outside the interval (%d with two admissible codes); count %d in [%d, %d]' % (
        name, int(bad.sum()), got.numel(), int((a != b).sum()), int(sat), least, most))
    assert int(bad.sum()) == 0
    assert least <= int(sat) <= most
    assert torch.equal(run_bn_apply_fp8(lib, d['x'], d['scale'], d['shift'], relu, act, None), got)
    assert torch.equal(rm.cpu(), rm2.cpu())


# ------------------------------------------------------------------------------------------ sfvos_conv3d, SFVOS_FP8
def x_operand(lib, name, c):
    """The x codes of a case on the device, FILL (0x7e = 448) bytes for two frames of the largest level in front of and behind
    them (and in the channel padding of the plain layout): (buffer, pointer, ld_x, x_group_stride)."""
    _, B, T, t_alloc, t_off, shapes, cin, cout, kt, layout, gen, act, _ = R.CONV_CASES[name]
    rows = torch.cat([x.permute(0, 2, 3, 4, 1).reshape(-1, cin) for x in c['xcodes']])      # [M, cin], level-major
    M, pad = rows.shape[0], 2 * max(H * W for H, W in shapes)
    if layout == 'grouped':
        buf = torch.full((cin // 64, M + 2 * pad, 64), R.FILL, dtype=torch.uint8)
        buf[:, pad:pad + M] = rows.reshape(M, cin // 64, 64).permute(1, 0, 2)
        buf = buf.cuda()
        return buf, P(buf, pad * 64), 64, (M + 2 * pad) * 64
    if layout == 'ndhwc':
        ld = cin + 64
        buf = torch.full((M + 2 * pad, ld), R.FILL, dtype=torch.uint8)
        buf[pad:pad + M, :cin] = rows
        buf = buf.cuda()
        return buf, P(buf, pad * ld), ld, 0
    # 'bn': sfvos_bn_apply_fp8 writes the [M][256] bytes in two channel slices (192 + 64), from bf16 q with scale 1, shift 0
    assert cin == 256
    buf = torch.full((M + 2 * pad, 256), R.FILL, dtype=torch.uint8, device='cuda')
    q = torch.cat([x.permute(0, 2, 3, 4, 1).reshape(-1, cin) for x in c['q']])
    lv = levels(lib, [M])
    one, zero = table(torch.ones(1, 256, dtype=torch.float64), 256), table(torch.zeros(1, 256, dtype=torch.float64), 256)
    for c0, cn in ((0, 192), (192, 64)):
        xs = q[:, c0:c0 + cn].float().bfloat16().contiguous().cuda()
        lib.call('sfvos_bn_apply_fp8', P(xs), cn, P(buf, pad * 256 + c0), 256, ctypes.byref(lv), cn, one[1], zero[1], one[2], 0,
                 1.0, None, None, S())
    torch.cuda.synchronize()
    assert torch.equal(buf[pad:pad + M].cpu(), rows) and bool((buf[:pad] == R.FILL).all()) and bool((buf[pad + M:] == R.FILL).all())
    return buf, P(buf, pad * 256), 256, 0


@pytest.mark.parametrize('name', list(R.CONV_CASES))
def test_conv3d_e4m3_operands_against_float64(lib, name):
    """Every CONV_CASES row of fp8_ref.py: the weight image and the (bias, descale) rows from sfvos_pack_weights_fp8 (rows
    equal to the reference), x codes chosen on the CPU; y in a channel slice between sentinels, NaN-filled statistics rows
    whose per-level float64 sums are S1 and S2 of the values written, then the ReLU epilogue without statistics."""
    body, B, T, t_alloc, t_off, shapes, cin, cout, kt, layout, gen, act, blocks = R.CONV_CASES[name]
    c = R.conv_inputs(name)
    xbuf, xp, ld_x, gstride = x_operand(lib, name, c)     # xbuf: keeps the buffer behind xp alive
    wd, bd = c['w'].cuda(), c['bias'].cuda()
    wp, rows3 = ByteOut((c['w'].numel(),)), Out((3, cout), torch.float32, fill=NAN)
    lib.call('sfvos_pack_weights_fp8', P(wd), P(bd), P(wp.t), P(rows3.t), cout, cin, kt, 9, act, S())
    ld_y = cout + 2 * OFF
    d, t_out = make_desc(lib, 'bf16', B, T, shapes, cin, cout, kt, 9, 0, ld_x, ld_y, t_alloc=t_alloc, t_offset=t_off)
    d.dtype, d.x_group_stride = lib.FP8, gstride
    M = sum(B * t_out * H * W for H, W in shapes)
    rows_pl = (ctypes.c_int * lib.MAX_LEVELS)()
    rows = lib.load().sfvos_conv3d_stat_rows(ctypes.byref(d), rows_pl)
    th = R.TILE_ROWS[body]
    assert [rows_pl[l] for l in range(len(shapes))] == [blocks * B * -(-H // th) * -(-W // 32) for H, W in shapes]
    part = Out((rows, 2, cout), torch.float32, fill=NAN)
    y = Out((M, ld_y), torch.bfloat16)
    lib.call('sfvos_conv3d', ctypes.byref(d), xp, P(wp.t), P(rows3.t), P(y.t, OFF), P(part.t), S())
    torch.cuda.synchronize()
    wp.cpu()
    check_exact('e4m3 conv %s (bias, descale, ws) rows' % name, rows3.cpu(), c['rows'])
    got = from_pyr(act_get(y, cout), B, cout, t_out, shapes)
    sums = [p.double().sum(0) for p in torch.split(part.cpu(), list(rows_pl[:len(shapes)]))]
    K = cin * kt * 9
    tag = 'e4m3 conv %s ' % name
    for l, ref in enumerate(c['ref']):
        s1, s2 = R.stats(ref)
        if gen == 'exact':
            check_exact(tag + 'y level %d' % l, got[l], ref)
            check_exact(tag + 'S1 level %d' % l, sums[l][0], s1)
            check_exact(tag + 'S2 level %d' % l, sums[l][1], s2)
        elif gen == 'full':
            check_abs(tag + 'y level %d' % l, got[l], ref, 2.0 ** -8 * ref.abs())
            check_exact(tag + 'S1 level %d' % l, sums[l][0], s1)
            check(tag + 'S2 level %d' % l, sums[l][1], s2, s2, K, 0.0)
        else:
            # S1 / S2 sum the unrounded fp32 values over n positions: each value within the conv's bound of float64, then n
            # additions (K + n); a square carries twice the relative error of its value (2 K + n + 2 on the squared magnitudes)
            mag = c['mag'][l]
            n = ref.numel() // cout
            check(tag + 'y level %d' % l, got[l], ref, mag, K + 1, 2.0 ** -8)
            check(tag + 'S1 level %d' % l, sums[l][0], s1, mag.sum((0, 2, 3, 4)), K + 1 + n, 0.0)
            check(tag + 'S2 level %d' % l, sums[l][1], s2, (mag * mag).sum((0, 2, 3, 4)), 2 * K + n + 2, 0.0)
    d.relu = 1
    assert lib.load().sfvos_conv3d(ctypes.byref(d), xp, P(wp.t), P(rows3.t), P(y.t, OFF), P(part.t), S()) != 0
    y = Out((M, ld_y), torch.bfloat16)
    lib.call('sfvos_conv3d', ctypes.byref(d), xp, P(wp.t), P(rows3.t), P(y.t, OFF), None, S())
    torch.cuda.synchronize()
    got = from_pyr(act_get(y, cout), B, cout, t_out, shapes)
    for l, ref in enumerate(c['ref']):
        r = ref.clamp_min(0.0)
        if gen == 'exact':
            check_exact(tag + 'relu y level %d' % l, got[l], r)
        elif gen == 'full':
            check_abs(tag + 'relu y level %d' % l, got[l], r, 2.0 ** -8 * r)
        else:
            check(tag + 'relu y level %d' % l, got[l], r, c['mag'][l], K + 1, 2.0 ** -8)


# ------------------------------------------------------------------------------------------ module level
def test_pack_fp8_saturates_planted_elements_and_counts_them():
    """SlowFastLayers.pack_fp8 on the small pyramid with N planted out-of-range elements (|x| * fp8_input_scale > 448,
    finite and infinite, both signs): the packed clip holds +-448 there and no NaN code anywhere, fp8_saturated() returns N
    and then 0."""
    from golden_util import SMALL_LEVELS
    from sfvos_amd import SlowFastLayers
    dev = torch.device('cuda:0')
    m = SlowFastLayers(256, dev, 3, 7, precision='fp8').to(dev)
    assert m.fp8_input_scale == 32.0
    g = torch.Generator().manual_seed(3)
    T, C = 7, 256
    feats = {k: (torch.randn(T, C, h, w, generator=g) * 3.0).clamp(-13.9, 13.9) for k, (h, w) in SMALL_LEVELS.items()}
    assert all(float(v.abs().max()) * 32.0 < 448.0 for v in feats.values())
    planted = [14.5, -14.5, 20.0, -1e6, float('inf'), -float('inf'), 3e38, -15.0, 14.000001]
    spots = []
    for i, val in enumerate(planted):
        k = list(SMALL_LEVELS)[i % 2]
        h, w = SMALL_LEVELS[k]
        at = (i % T, (37 * i + 5) % C, (3 * i) % h, (5 * i + 1) % w)
        feats[k][at] = val
        spots.append((k, at, val))
    clip = m.pack_fp8([{k: v.to(dev) for k, v in feats.items()}])
    torch.cuda.synchronize()
    data = clip.data.cpu()                                   # [C / 64, M, 64], level-major
    assert not bool(((data & 0x7f) == 0x7f).any()), '%d NaN codes in the packed clip' % int(((data & 0x7f) == 0x7f).sum())
    off = {}
    at0 = 0
    for k, (h, w) in SMALL_LEVELS.items():
        off[k] = at0
        at0 += T * h * w
    for k, (t, ch, y, x), val in spots:
        h, w = SMALL_LEVELS[k]
        code = int(data[ch // 64, off[k] + (t * h + y) * w + x, ch % 64])
        assert code == (0x7e if val > 0 else 0xfe), (k, (t, ch, y, x), val, hex(code))
    want = torch.cat([R.quantise(feats[k], 32.0)[0].permute(0, 2, 3, 1).reshape(-1, C) for k in SMALL_LEVELS])
    equal_codes('pack_fp8 small pyramid', data.permute(1, 0, 2).reshape(-1, C), want)
    assert m.fp8_saturated() == len(planted)
    assert m.fp8_saturated() == 0
