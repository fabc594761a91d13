"""GPU: the backward half of the conv through the C ABI -- sfvos_conv3d_wgrad (wgrad.hip with its split-K reduction,
lateral_wgrad.hip, wgrad_t1.hip) and the data-gradient paths of sfvos_conv3d (pad_t = kt - 1: tap skipping, the
single-frame-block wide plan, conv3d_fs1s_kernel, lateral_dgrad_try, the accumulate read-modify-write) -- compared with the
float64 references of tests/conv_bwd_ref.py.

Every case but one feeds exactly summable integer operands (conv_bwd_ref's docstring; preconditions asserted on the float64
reference in tests/test_conv_bwd_ref_cpu.py): every partial sum in any order is an integer below 2^24, every fp32 addition
is exact, and the kernel must EQUAL float64 (kernel_util.check_exact).  One dropped 16-pixel tile row at a ragged edge, a
ring frame read one slot late for one tap, a share that skips its last tile, a slab left out of the reduction: each changes
at least one element by at least one product.  The one random-operand case per precision takes kernel_util.check with
u_out = 0 and K = the number of positions.

Set-up of every case: grad_w / dx between guard bands (kernel_util.Out), the workspace NaN-filled before every call, pitches
wider than the channel counts with 7.0 in the padding (the grouped x layout has no pitch), two frames of 7.0 in front of and
behind x (a zero frame of a window beyond the buffer must never be read), channels of dx beyond c_in
sentinel-filled and checked.  Every weight-gradient case issues its three calls -- accumulate = 0, accumulate = 1 into an
integer-filled grad_w, accumulate = 0 again -- back to back on the stream, the NaN refill of the shared workspace between
them, with no host synchronisation before the last one is queued: the entry point does not synchronise, so stream order
alone has to keep the slabs of one call from the next.  The second plain run must be bit-identical to the first."""
import ctypes

import pytest
import torch

import conv_bwd_ref as R
from kernel_util import SENT, TDT, Out, P, S, check, check_exact, from_pyr, lib, make_desc, to_pyr  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float('nan')
PAD = 40      # pitch padding: c_in 96 + 40 covers the 32 channels a ragged c tile would read past the tensor


def grouped(xd, cin):
    """[M, cin] -> the channel-group-major layout [cin / 32][M][32]."""
    M = xd.shape[0]
    return xd.view(M, cin // 32, 32).permute(1, 0, 2).contiguous()


WGRAD_PARAMS = [(n, p) for n, c in R.WGRAD_CASES.items() for p in c[9]]


@pytest.mark.parametrize('name,prec', WGRAD_PARAMS)
def test_conv3d_wgrad_equals_float64(lib, name, prec):
    B, T, t_alloc, t_off, shapes, cin, cout, kt, taps, _, gen, flags = R.WGRAD_CASES[name]
    xs, dys, ref, mag = R.wgrad_inputs(name, prec if gen == 'random' else 'fp32')
    pre = R.wgrad_prefill(name)
    ld_x, ld_y = cin + PAD, cout + PAD
    dyd = to_pyr([v.float() for v in dys], prec, ld_y)
    if 'grouped' in flags:
        xd = grouped(to_pyr([v.float() for v in xs], prec), cin)
        d, _ = make_desc(lib, prec, B, T, shapes, cin, cout, kt, taps, 0, 32, ld_y, t_alloc=t_alloc, t_offset=t_off)
        d.x_group_stride = xd.shape[1] * 32
    else:
        # two frames of 7.0 in front of and behind x: a zero frame of a window beyond the buffer that was read after all
        # would not meet zeros by luck
        junk = torch.full((2 * max(h * w for h, w in shapes), ld_x), 7.0, dtype=TDT[prec], device='cuda')
        xall = torch.cat([junk, to_pyr([v.float() for v in xs], prec, ld_x), junk])
        xd = xall[junk.shape[0]:xall.shape[0] - junk.shape[0]]
        d, _ = make_desc(lib, prec, B, T, shapes, cin, cout, kt, taps, 0, ld_x, ld_y, t_alloc=t_alloc, t_offset=t_off)
    nbytes = lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Out((nbytes // 4,), torch.float32, fill=NAN)
    first, again = Out(ref.shape), Out(ref.shape)
    acc = Out(ref.shape)
    acc.t.copy_(pre.float())
    for out, accumulate in ((first, 0), (acc, 1), (again, 0)):     # back to back: no host synchronisation in between
        ws.t.fill_(NAN)
        lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(out.t), accumulate, P(ws.t), S())
    torch.cuda.synchronize()
    assert ws.guards_ok(), 'wrote outside its workspace'
    got = first.cpu()
    tag = 'wgrad %s %s' % (name, prec)
    if gen == 'random':
        K = R.wgrad_positions(name)
        check(tag, got, ref, mag, K, 0.0)
        check(tag + ' accumulate', acc.cpu(), pre + ref, pre.abs() + mag, K + 1, 0.0)
    else:
        check_exact(tag, got, ref)
        check_exact(tag + ' accumulate', acc.cpu(), pre + ref)
    assert torch.equal(got, again.cpu()), 'the weight gradient must be bit-identical from run to run'


DGRAD_PARAMS = [(n, p) for n, c in R.DGRAD_CASES.items() for p in c[7]]


@pytest.mark.parametrize('name,prec', DGRAD_PARAMS)
def test_conv3d_dgrad_equals_float64_with_and_without_accumulate(lib, name, prec):
    B, T, shapes, cin, cout, kt, taps, _ = R.DGRAD_CASES[name]
    dys, w, refs, _, pre = R.dgrad_inputs(name)
    t_out = T - kt + 1
    ld_dy, ld_dx = cout + PAD, cin + PAD
    dyd = to_pyr([v.float() for v in dys], prec, ld_dy)
    # the data-gradient conv: channels swapped, pad_t = kt - 1
    d, t_back = make_desc(lib, prec, B, t_out, shapes, cout, cin, kt, taps, kt - 1, ld_dy, ld_dx)
    assert t_back == T
    wp = torch.empty(w.numel(), dtype=TDT[prec], device='cuda')
    wd = w.float().cuda()
    lib.call('sfvos_pack_weights_dgrad', P(wd), P(wp), d.dtype, cout, cin, kt, taps, S())
    M = sum(B * T * H * W for H, W in shapes)
    plain, acc = Out((M, ld_dx), TDT[prec]), Out((M, ld_dx), TDT[prec])
    acc.t[:, :cin] = to_pyr(pre, prec)
    lib.call('sfvos_conv3d', ctypes.byref(d), P(dyd), P(wp), None, P(plain.t), None, S())
    d.accumulate = 1
    lib.call('sfvos_conv3d', ctypes.byref(d), P(dyd), P(wp), None, P(acc.t), None, S())
    torch.cuda.synchronize()
    for out, what, add in ((plain, '', None), (acc, ' accumulate', pre)):
        flat = out.cpu()
        assert bool((flat[:, cin:].float() == SENT).all()), 'wrote channels of dx beyond c_in'
        got = from_pyr(flat, B, cin, T, shapes)
        for l, ref in enumerate(refs):
            check_exact('dgrad %s %s%s level %d' % (name, prec, what, l), got[l], ref if add is None else ref + add[l])
