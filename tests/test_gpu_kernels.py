"""GPU: every libsfvos kernel, called through the C ABI (ctypes), against a plain PyTorch fp32
reference of the same op computed on the CPU.  Pyramids of 1-3 levels exercise the grouped
launches.  Tolerances: fp32 path 1e-4 relative to the tensor scale (exact-f32 MFMA, only summation
order differs); bf16 path 2e-2 (bf16 operands, f32 accumulate) -- stated per assert."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_util import TDT, P, S, from_pyr, lib, make_desc, relmax, to_pyr  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = {'fp32': 1e-4, 'bf16': 2e-2}

CONV_CASES = [
    # B  T   shapes                      cin cout kt taps
    (1, 4, [(12, 21)], 256, 192, 2, 9),
    (1, 3, [(9, 17), (5, 40)], 256, 224, 2, 9),
    (2, 7, [(6, 10), (3, 5), (1, 2)], 64, 32, 3, 9),
    (1, 13, [(20, 19)], 32, 32, 2, 9),             # t_out 12 -> three frame blocks of 4
    (1, 14, [(5, 33), (9, 9)], 32, 32, 4, 9),      # t_out 11
    (1, 9, [(18, 16), (4, 35)], 32, 64, 5, 1),     # lateral, t_out 5
    (1, 5, [(7, 40)], 32, 64, 3, 1),
    (1, 3, [(10, 12), (3, 3)], 64, 32, 2, 1),      # lateral dgrad shape (narrow, 1x1)
    # lateral forward with t_out <= 3 (bf16: the dedicated kernel of lateral.hip; fp32: generic)
    (2, 21, [(9, 13), (3, 3), (1, 2)], 32, 64, 20, 1),   # t_out 2, kt 20, ragged tiles and idle waves
    (1, 8, [(16, 33)], 32, 64, 8, 1),                    # t_out 1
    (1, 22, [(24, 42), (12, 21), (6, 11)], 32, 64, 20, 1),  # t_out 3: the first lateral of cfg (2,1,4)
    # weight images beyond 80 KB (bf16: one 12-wave workgroup per compute unit): kt 21 = conv_f2s2 of (4,64), kt 40 = all
    # of the LDS, kt 41 = conv_f2s1 of (4,64): 40 taps in LDS + the last one in registers
    (1, 22, [(12, 21), (5, 7)], 32, 64, 21, 1),
    (2, 41, [(9, 13), (2, 2)], 32, 64, 40, 1),
    (1, 43, [(24, 42), (6, 11)], 32, 64, 41, 1),
    (1, 41, [(7, 9)], 32, 64, 41, 1),                    # t_out 1 with the register tap
    # frame-split kernel: ragged 32-px tile columns (42 = 32 + 10, 48 = 32 + 16, 21, 10 and 5 px: the last column of
    # every level is partly padding) and a ragged last tile row (17 = 2 x 8 + 1); 4-, 2- and 1-frame blocks
    # (t_out 7 = 4 + 2 + 1)
    (1, 9, [(24, 42), (17, 48), (12, 21)], 256, 32, 3, 9),
    (2, 8, [(40, 10), (3, 5)], 32, 32, 2, 9),
    # the 3x3 convs of the mask head: one frame (kt = t_in = 1), batch = RoIs, one 14x14 or 7x7 level
    (1, 1, [(14, 14)], 256, 256, 1, 9),
    (9, 1, [(14, 14)], 256, 256, 1, 9),
    (33, 1, [(7, 7)], 256, 256, 1, 9),
    (33, 1, [(14, 14)], 256, 32, 1, 9),
]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', CONV_CASES)
def test_conv3d_forward_bias_stats(lib, prec, case):
    B, T, shapes, cin, cout, kt, taps = case
    g = torch.Generator().manual_seed(1234)
    k = 3 if taps == 9 else 1
    w = torch.randn(cout, cin, kt, k, k, generator=g) / np.sqrt(cin * kt * taps)
    bias = torch.randn(cout, generator=g) * 0.1
    xs = [torch.randn(B, cin, T, H, W, generator=g) for (H, W) in shapes]
    if prec == 'bf16':  # the reference sees the same rounded operands
        xs, w = [x.bfloat16().float() for x in xs], w.bfloat16().float()
    refs = [F.conv3d(x, w, bias, padding=(0, 1, 1) if taps == 9 else 0) for x in xs]
    ld_x, ld_y = cin + 32, cout + 64
    xd = to_pyr(xs, prec, ld_x)
    d, t_out = make_desc(lib, prec, B, T, shapes, cin, cout, kt, taps, 0, ld_x, ld_y)
    wp = torch.empty(w.numel(), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_pack_weights_fwd', P(w.cuda()), P(wp), d.dtype, cout, cin, kt, taps, S())
    M = sum(B * t_out * H * W for H, W in shapes)
    y = torch.full((M, ld_y), -3.0, dtype=TDT[prec], device='cuda')
    rows_pl = (ctypes.c_int * lib.MAX_LEVELS)()
    rows = lib.load().sfvos_conv3d_stat_rows(ctypes.byref(d), rows_pl)
    assert rows > 0 and sum(rows_pl[:len(shapes)]) == rows
    part = torch.full((rows, 2, cout), 1e9, dtype=torch.float32, device='cuda')
    lib.call('sfvos_conv3d', ctypes.byref(d), P(xd), P(wp), P(bias.cuda()), P(y), P(part), S())
    torch.cuda.synchronize()
    got = from_pyr(y, B, cout, t_out, shapes)
    r0 = 0
    for l, ref in enumerate(refs):
        assert relmax(got[l], ref) < TOL[prec], 'level %d' % l
        s = part[r0:r0 + rows_pl[l]].double().sum(0).cpu()
        r0 += rows_pl[l]
        n = ref.numel() // cout
        assert float((s[0] - ref.double().sum((0, 2, 3, 4))).abs().max()) / n < 1e-3 * float(ref.abs().max())
        assert relmax(s[1], (ref.double() ** 2).sum((0, 2, 3, 4))) < (1e-4 if prec == 'fp32' else 2e-2)
    assert torch.all(y[:, cout:].float() == -3.0), 'wrote outside its channel slice'


def test_lateral_forward_window_and_relu_epilogue(lib):
    """lateral forward kernel (lateral.hip): frames [t_offset, t_offset + t_in) of a longer buffer, no bias, ReLU."""
    B, Ta, T, off, shapes, kt = 2, 9, 6, 2, [(5, 21), (2, 3)], 4
    g = torch.Generator().manual_seed(77)
    w = (torch.randn(64, 32, kt, 1, 1, generator=g) / np.sqrt(32 * kt)).bfloat16().float()
    xs = [torch.randn(B, 32, Ta, H, W, generator=g).bfloat16().float() for (H, W) in shapes]
    refs = [F.relu(F.conv3d(x[:, :, off:off + T], w, None)) for x in xs]
    xd = to_pyr(xs, 'bf16', 40)
    d, t_out = make_desc(lib, 'bf16', B, T, shapes, 32, 64, kt, 1, 0, 40, 64, t_alloc=Ta, t_offset=off)
    d.relu = 1
    wp = torch.empty(w.numel(), dtype=torch.bfloat16, device='cuda')
    lib.call('sfvos_pack_weights_fwd', P(w.cuda()), P(wp), d.dtype, 64, 32, kt, 1, S())
    M = sum(B * t_out * H * W for H, W in shapes)
    y = torch.full((M, 64), -3.0, dtype=torch.bfloat16, device='cuda')
    lib.call('sfvos_conv3d', ctypes.byref(d), P(xd), P(wp), None, P(y), None, S())
    torch.cuda.synchronize()
    got = from_pyr(y, B, 64, t_out, shapes)
    for l, ref in enumerate(refs):
        assert relmax(got[l], ref) < TOL['bf16'], 'level %d' % l


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_conv3d_reads_a_frame_window_of_a_longer_clip(lib, prec):
    """t_alloc/t_offset: the slow pathway reads its centre frames out of the fast clip's buffer."""
    B, Tf, sp, off, shapes, cin, cout, kt = 2, 7, 3, 2, [(6, 10), (3, 7)], 64, 32, 2
    g = torch.Generator().manual_seed(5)
    w = torch.randn(cout, cin, kt, 3, 3, generator=g) / np.sqrt(cin * kt * 9)
    xs = [torch.randn(B, cin, Tf, H, W, generator=g) for (H, W) in shapes]
    if prec == 'bf16':
        xs, w = [x.bfloat16().float() for x in xs], w.bfloat16().float()
    refs = [F.conv3d(x[:, :, off:off + sp], w, None, padding=(0, 1, 1)) for x in xs]
    xd = to_pyr(xs, prec)
    d, t_out = make_desc(lib, prec, B, sp, shapes, cin, cout, kt, 9, 0, cin, cout, t_alloc=Tf, t_offset=off)
    wp = torch.empty(w.numel(), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_pack_weights_fwd', P(w.cuda()), P(wp), d.dtype, cout, cin, kt, 9, S())
    y = torch.empty((sum(B * t_out * H * W for H, W in shapes), cout), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_conv3d', ctypes.byref(d), P(xd), P(wp), None, P(y), None, S())
    for a, b in zip(from_pyr(y, B, cout, t_out, shapes), refs):
        assert relmax(a, b) < TOL[prec]
    # weight gradient through the same window
    dys = [torch.randn(B, cout, t_out, H, W, generator=g) for (H, W) in shapes]
    if prec == 'bf16':
        dys = [v.bfloat16().float() for v in dys]
    wz = torch.zeros_like(w, requires_grad=True)
    for x, dy in zip(xs, dys):
        F.conv3d(x[:, :, off:off + sp], wz, None, padding=(0, 1, 1)).backward(dy)
    dyd = to_pyr(dys, prec)
    ws = torch.empty(lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device='cuda')
    gw = torch.empty(w.shape, dtype=torch.float32, device='cuda')
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 0, P(ws), S())
    assert relmax(gw.cpu(), wz.grad) < TOL[prec]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', [(2, 7, 4, -2, [(6, 10), (3, 7)], 64, 32, 3),      # 2 zero frames in front, 1 behind
                                  (1, 5, 3, 1, [(9, 17)], 256, 192, 2),             # window [1, 6) of a 3-frame buffer
                                  (1, 9, 5, -1, [(12, 21), (5, 9)], 256, 32, 3)])   # frame-split kernel
def test_conv3d_window_beyond_the_buffer_reads_zero_frames(lib, prec, case):
    """t_offset < 0 or t_offset + t_in > t_alloc: the frames of the window that the buffer does not hold are zero
    frames (model.py:215-225 pads windows beyond the ends of a sequence with zero features) that are never read --
    forward conv and weight gradient against F.conv3d on explicitly zero-padded clips."""
    B, t_in, t_alloc, t_off, shapes, cin, cout, kt = case
    g = torch.Generator().manual_seed(17)
    w = torch.randn(cout, cin, kt, 3, 3, generator=g) / np.sqrt(cin * kt * 9)
    xs = [torch.randn(B, cin, t_alloc, H, W, generator=g) for (H, W) in shapes]
    if prec == 'bf16':
        xs, w = [x.bfloat16().float() for x in xs], w.bfloat16().float()

    def window(x):
        full = torch.zeros(B, cin, t_in, x.shape[3], x.shape[4])
        for t in range(t_in):
            if 0 <= t_off + t < t_alloc:
                full[:, :, t] = x[:, :, t_off + t]
        return full
    wins = [window(x) for x in xs]
    refs = [F.conv3d(v, w, None, padding=(0, 1, 1)) for v in wins]
    xd = to_pyr(xs, prec)
    d, t_out = make_desc(lib, prec, B, t_in, shapes, cin, cout, kt, 9, 0, cin, cout, t_alloc=t_alloc, t_offset=t_off)
    wp = torch.empty(w.numel(), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_pack_weights_fwd', P(w.cuda()), P(wp), d.dtype, cout, cin, kt, 9, S())
    y = torch.empty((sum(B * t_out * H * W for H, W in shapes), cout), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_conv3d', ctypes.byref(d), P(xd), P(wp), None, P(y), None, S())
    for a, b in zip(from_pyr(y, B, cout, t_out, shapes), refs):
        assert relmax(a, b) < TOL[prec]
    dys = [torch.randn(B, cout, t_out, H, W, generator=g) for (H, W) in shapes]
    if prec == 'bf16':
        dys = [v.bfloat16().float() for v in dys]
    wz = torch.zeros_like(w, requires_grad=True)
    for v, dy in zip(wins, dys):
        F.conv3d(v, wz, None, padding=(0, 1, 1)).backward(dy)
    dyd = to_pyr(dys, prec)
    ws = torch.empty(lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device='cuda')
    gw = torch.empty(w.shape, dtype=torch.float32, device='cuda')
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 0, P(ws), S())
    assert relmax(gw.cpu(), wz.grad) < TOL[prec]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', [(1, 4, [(12, 21)], 256, 192, 2, 9), (1, 13, [(10, 19), (4, 5)], 32, 32, 2, 9),
                                  (1, 9, [(9, 16)], 32, 64, 5, 1), (1, 7, [(6, 10), (2, 3)], 256, 32, 3, 9),
                                  # lateral data gradients with <= 3 slow frames: the dedicated bf16 kernel (lateral.hip)
                                  (1, 7, [(9, 16), (5, 7)], 32, 64, 5, 1), (2, 12, [(6, 10), (3, 3)], 32, 64, 11, 1),
                                  (1, 20, [(7, 9)], 32, 64, 20, 1),
                                  # kt = 41 (the (4,64) configuration): the weight image exceeds the LDS budget
                                  (1, 43, [(5, 9), (2, 2)], 32, 64, 41, 1),
                                  # ... kt = 21 / 40: images of 84 / 160 KB (12-wave workgroups); kt 42: beyond (from L2)
                                  (1, 22, [(12, 21), (3, 3)], 32, 64, 21, 1), (2, 41, [(6, 7)], 32, 64, 40, 1),
                                  (1, 43, [(4, 9)], 32, 64, 42, 1),
                                  # fast_conv3's shape (all frames -> one): single-frame blocks, one temporal tap each
                                  (2, 12, [(9, 37), (4, 5)], 32, 32, 12, 9),
                                  # the 3x3 convs of the mask head (kt = t_in = 1, batch = RoIs)
                                  (9, 1, [(14, 14)], 256, 256, 1, 9), (33, 1, [(7, 7)], 256, 32, 1, 9),
                                  (1, 1, [(7, 7)], 256, 256, 1, 9)])
def test_conv3d_dgrad_and_accumulate(lib, prec, case):
    B, T, shapes, cin, cout, kt, taps = case
    g = torch.Generator().manual_seed(99)
    k = 3 if taps == 9 else 1
    w = torch.randn(cout, cin, kt, k, k, generator=g) / np.sqrt(cout * kt * taps)
    t_out = T - kt + 1
    xs = [torch.randn(B, cin, T, H, W, generator=g, requires_grad=True) for (H, W) in shapes]
    dys = [torch.randn(B, cout, t_out, H, W, generator=g) for (H, W) in shapes]
    if prec == 'bf16':
        w, dys = w.bfloat16().float(), [v.bfloat16().float() for v in dys]
    for x, dy in zip(xs, dys):
        F.conv3d(x, w, None, padding=(0, 1, 1) if taps == 9 else 0).backward(dy)
    dyd = to_pyr(dys, prec)
    # the data-gradient conv: channels swapped, pad_t = kt-1
    d, t_back = make_desc(lib, prec, B, t_out, shapes, cout, cin, kt, taps, kt - 1, cout, cin)
    assert t_back == T
    wp = torch.empty(w.numel(), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_pack_weights_dgrad', P(w.cuda()), P(wp), d.dtype, cout, cin, kt, taps, S())
    dx = torch.empty((sum(B * T * H * W for H, W in shapes), cin), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_conv3d', ctypes.byref(d), P(dyd), P(wp), None, P(dx), None, S())
    for a, x in zip(from_pyr(dx, B, cin, T, shapes), xs):
        assert relmax(a, x.grad) < TOL[prec]
    d.accumulate = 1  # second call adds: dx == 2 * grad
    lib.call('sfvos_conv3d', ctypes.byref(d), P(dyd), P(wp), None, P(dx), None, S())
    for a, x in zip(from_pyr(dx, B, cin, T, shapes), xs):
        assert relmax(a, 2 * x.grad) < 2 * TOL[prec]


@pytest.mark.parametrize('case', [(1, 6, [(12, 21), (5, 9)], 256, 32, 3, 9),    # frame-split kernel
                                  (2, 4, [(9, 17), (3, 3)], 256, 192, 2, 9),    # wide kernel, two clips
                                  (1, 5, [(10, 12)], 64, 32, 2, 9)])
def test_grouped_input_layout_is_bit_identical(lib, case):
    """x stored as 64-byte channel groups (sfvos_frames_to_groups, sfvos_conv_desc.x_group_stride): the conv
    (with a frame window, as the slow pathway reads the fast clip) and the weight gradient must give exactly
    the bits they give for the same values in pyramid NDHWC -- only the addresses differ."""
    B, T, shapes, cin, cout, kt, taps = case
    g = torch.Generator().manual_seed(321)
    w = torch.randn(cout, cin, kt, 3, 3, generator=g) / np.sqrt(cin * kt * taps)
    xs = [torch.randn(B, cin, T, H, W, generator=g) for (H, W) in shapes]
    x_nd = to_pyr(xs, 'bf16')
    M = x_nd.shape[0]
    # grouped buffer built by the library from the planar frames (one call per level and clip)
    x_gr = torch.full((cin // 32, M, 32), 5.0, dtype=torch.bfloat16, device='cuda')
    off = 0
    for x in xs:
        H, W = x.shape[3], x.shape[4]
        xc = x.cuda()
        for b in range(B):
            s = xc[b]  # [C,T,H,W]
            lib.call('sfvos_frames_to_groups', P(s), s.stride(1), s.stride(0), s.stride(2), s.stride(3),
                     P(x_gr, (off + b * T * H * W) * 32), lib.BF16, T, cin, H, W, M * 32, S())
        off += B * T * H * W
    assert torch.equal(x_gr.permute(1, 0, 2).reshape(M, cin), x_nd), 'frames_to_groups != NDHWC values'
    t_win, t_off = T - 1, 1  # read frames [1, T) of the buffer
    outs, grads = [], []
    for x, gs in ((x_nd, 0), (x_gr, M * 32)):
        d, t_out = make_desc(lib, 'bf16', B, t_win, shapes, cin, cout, kt, taps, 0, cin if gs == 0 else 32, cout,
                             t_alloc=T, t_offset=t_off)
        d.x_group_stride = gs
        wp = torch.empty(w.numel(), dtype=torch.bfloat16, device='cuda')
        lib.call('sfvos_pack_weights_fwd', P(w.cuda()), P(wp), d.dtype, cout, cin, kt, taps, S())
        Mo = sum(B * t_out * H * W for H, W in shapes)
        y = torch.zeros((Mo, cout), dtype=torch.bfloat16, device='cuda')
        lib.call('sfvos_conv3d', ctypes.byref(d), P(x), P(wp), None, P(y), None, S())
        outs.append(y)
        dy = (torch.randn(Mo, cout, generator=torch.Generator().manual_seed(5)) * 0.1).bfloat16().cuda()
        ws = torch.empty(lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device='cuda')
        gw = torch.empty(w.shape, dtype=torch.float32, device='cuda')
        lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(x), P(dy), P(gw), 0, P(ws), S())
        grads.append(gw)
    torch.cuda.synchronize()
    assert float(outs[0].float().abs().max()) > 0.1
    assert torch.equal(outs[0], outs[1]), 'conv differs between the two input layouts'
    assert torch.equal(grads[0], grads[1]), 'weight gradient differs between the two input layouts'
    ref = [F.conv3d(x.bfloat16().float()[:, :, t_off:], w.bfloat16().float(), None, padding=(0, 1, 1)) for x in xs]
    for a, r in zip(from_pyr(outs[1], B, cout, t_win - kt + 1, shapes), ref):
        assert relmax(a, r) < TOL['bf16']


WGRAD_CASES = [
    (1, 4, [(12, 21), (6, 10)], 256, 32, 2, 9),    # cfg (1,2,4): c_out 32, c_in 256
    (1, 3, [(9, 17)], 256, 192, 2, 9),             # cfg (2,2,2)
    (1, 3, [(6, 10), (3, 4)], 256, 224, 2, 9),     # ragged n blocks
    (1, 5, [(12, 21), (6, 10)], 256, 32, 2, 9),    # cfg (1,2,4) with an even number of output frames: bf16 frame-paired stages
    (2, 8, [(7, 19), (13, 5)], 64, 32, 3, 9),      # the same: two clips, c_in 64 (one c block), t_out 6, 3 of 4 taps live
    (2, 13, [(7, 19), (9, 3)], 32, 32, 11, 9),     # c_in 32: f32 cfg (1,1,8), kt 11 -> two dt groups; bf16 4 taps x 2 row halves: three
    (1, 6, [(21, 19), (40, 10)], 32, 32, 3, 9),    # the same, levels taller than the 16-row tile: both row halves live, 3 of 4 taps
    (1, 9, [(18, 16)], 32, 64, 5, 1),              # cfg (2,1,4) lateral
    (1, 24, [(5, 33), (2, 2)], 32, 64, 20, 1),
    # the 3x3 convs of the mask head (kt = t_in = 1, batch = RoIs)
    (1, 1, [(14, 14)], 256, 256, 1, 9),
    (9, 1, [(14, 14)], 256, 256, 1, 9),
    (33, 1, [(7, 7)], 256, 32, 1, 9),
]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', WGRAD_CASES)
def test_conv3d_wgrad(lib, prec, case):
    B, T, shapes, cin, cout, kt, taps = case
    g = torch.Generator().manual_seed(7)
    k = 3 if taps == 9 else 1
    w = torch.zeros(cout, cin, kt, k, k, requires_grad=True)
    t_out = T - kt + 1
    xs = [torch.randn(B, cin, T, H, W, generator=g) for (H, W) in shapes]
    dys = [torch.randn(B, cout, t_out, H, W, generator=g) for (H, W) in shapes]
    if prec == 'bf16':
        xs, dys = [v.bfloat16().float() for v in xs], [v.bfloat16().float() for v in dys]
    for x, dy in zip(xs, dys):
        F.conv3d(x, w, None, padding=(0, 1, 1) if taps == 9 else 0).backward(dy)
    ref = w.grad
    ld_x, ld_y = cin + 32, cout + 32
    xd, dyd = to_pyr(xs, prec, ld_x), to_pyr(dys, prec, ld_y)
    d, _ = make_desc(lib, prec, B, T, shapes, cin, cout, kt, taps, 0, ld_x, ld_y)
    nbytes = lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    gw = torch.full(ref.shape, 5.0, dtype=torch.float32, device='cuda')
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 0, P(ws), S())
    assert relmax(gw.cpu(), ref) < TOL[prec]
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 1, P(ws), S())
    assert relmax(gw.cpu(), 2 * ref) < 2 * TOL[prec]


# Pyramids with more pixel tiles than the split-K count make_wgrad_plan picks: every workgroup sweeps SEVERAL tiles, so
# the x-ring prefetch across tile (and level) boundaries, the `q0 += dt_live - 1` frame wrap and the `xi_q <= need`
# reload path of wgrad_kernel run -- the configuration of the benchmark (700+ tiles, 2-12 per workgroup).
WGRAD_MULTI_TILE_CASES = [
    (1, 13, [(96, 168), (24, 42)], 256, 32, 11, 9),   # cfg (1,2,4): fast_conv1's shape, kt 11 = 4 + 4 + 3 taps
    (1, 3, [(96, 168), (12, 21)], 256, 192, 2, 9),    # cfg (2,2,2): slow_conv1/2's shape
    (1, 14, [(96, 168), (24, 42)], 256, 32, 11, 9),   # fast_conv1's shape with t_out 4: bf16 frame pairs, ring advancing two frames per stage
    (1, 14, [(160, 170)], 32, 32, 11, 9),             # fast_conv2's shape (t_out 4): f32 cfg (1,1,8), bf16 4 taps x 2 row halves
    (1, 22, [(96, 168), (5, 9)], 32, 64, 20, 1),      # cfg (2,1,4): the first lateral, kt 20
]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', WGRAD_MULTI_TILE_CASES)
def test_conv3d_wgrad_several_tiles_per_workgroup(lib, prec, case):
    B, T, shapes, cin, cout, kt, taps = case
    g = torch.Generator().manual_seed(11)
    k = 3 if taps == 9 else 1
    w = torch.zeros(cout, cin, kt, k, k, requires_grad=True)
    t_out = T - kt + 1
    xs = [torch.randn(B, cin, T, H, W, generator=g) for (H, W) in shapes]
    dys = [torch.randn(B, cout, t_out, H, W, generator=g) for (H, W) in shapes]
    if prec == 'bf16':
        xs, dys = [v.bfloat16().float() for v in xs], [v.bfloat16().float() for v in dys]
    for x, dy in zip(xs, dys):
        F.conv3d(x, w, None, padding=(0, 1, 1) if taps == 9 else 0).backward(dy)
    ref = w.grad
    xd, dyd = to_pyr(xs, prec), to_pyr(dys, prec)
    d, _ = make_desc(lib, prec, B, T, shapes, cin, cout, kt, taps, 0, cin, cout)
    nbytes = lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d))
    psplit = nbytes // (4 * ref.numel())
    th = 4 if prec == 'fp32' else 8
    if prec == 'bf16' and cin == 32 and taps == 9:
        th = 16   # the row-split configuration of wgrad_kernel: 16-row tiles, two waves per (tap) group
    elif prec == 'bf16' and taps == 9 and t_out % 2 == 0 and t_out >= 4:
        th = 6    # frame-paired stages (two output frames per stage, 16x16x32 MFMAs): 6-row tiles
    ntiles = sum(B * -(-H // th) * -(-W // 16) for H, W in shapes)
    per = -(-ntiles // psplit)
    if taps == 1 and prec == 'bf16':   # lateral_wgrad.hip: 16-position tiles, one slab per workgroup (its own test below)
        ntiles = sum(B * -(-(H * W) // 16) for H, W in shapes)
        per = -(-ntiles // min(256, max(1, ntiles // 8)))
    assert per >= 2, 'case does not sweep several tiles per workgroup (ntiles %d, split %d)' % (ntiles, psplit)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    gw = torch.full(ref.shape, 5.0, dtype=torch.float32, device='cuda')
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 0, P(ws), S())
    e = relmax(gw.cpu(), ref)
    print('wgrad %s %s: %d tiles, split %d, %d tiles per workgroup, max err / scale %.2e' % (case, prec, ntiles, psplit, per, e))
    assert e < TOL[prec]


# The lateral convs' own weight-gradient kernel (lateral_wgrad.hip, bf16, 32 -> 64 channels, t_out <= 3, kt <= 48): all taps
# per workgroup, LDS ring with counted waits.  Cases: every t_out, taps per wave 1..6 (kt 1..48) incl. the benchmark's
# (20, 3) / (11, 2) and configuration 4's (41, 3) / (21, 2); level sizes that are not multiples of the 16-position tile;
# two clips; pitches wider than the channel count; a frame window inside a longer buffer; more tiles than workgroups
# (several stages per workgroup, ring wrap) and fewer (workgroups with a single stage).
LAT_WGRAD_CASES = [
    # B  t_alloc t_off T   shapes                          kt
    (1, 22, 0, 22, [(96, 168), (24, 42), (12, 21)], 20),   # t_out 3: conv_f2s1 of (4,32), 20k positions
    (1, 12, 0, 12, [(48, 84), (5, 9)], 11),                # t_out 2: conv_f2s2 of (4,32)
    (1, 43, 0, 43, [(24, 42), (12, 21)], 41),              # t_out 3: conv_f2s1 of (4,64): 6 taps per wave, ring of 3
    (1, 22, 0, 22, [(24, 42)], 21),                        # t_out 2: conv_f2s2 of (4,64)
    (2, 9, 2, 6, [(5, 21), (2, 3), (1, 1)], 4),            # window [2, 8) of 9 frames, two clips, tiny ragged levels
    (1, 1, 0, 1, [(7, 9)], 1),                             # kt 1, t_out 1 (equal pathway sizes)
    (2, 50, 1, 48, [(3, 11)], 48),                         # the largest kt the kernel takes, t_out 1
    (1, 7, 0, 7, [(13, 17)], 5),                           # t_out 3, kt 5
]


@pytest.mark.parametrize('case', LAT_WGRAD_CASES)
def test_lateral_wgrad_kernel(lib, case):
    B, Ta, off, T, shapes, kt = case
    g = torch.Generator().manual_seed(19)
    w = torch.zeros(64, 32, kt, 1, 1, requires_grad=True)
    t_out = T - kt + 1
    xs = [torch.randn(B, 32, Ta, H, W, generator=g).bfloat16().float() for (H, W) in shapes]
    dys = [torch.randn(B, 64, t_out, H, W, generator=g).bfloat16().float() for (H, W) in shapes]
    for x, dy in zip(xs, dys):
        F.conv3d(x[:, :, off:off + T], w, None).backward(dy)
    ref = w.grad
    ld_x, ld_y = 40, 96
    xd, dyd = to_pyr(xs, 'bf16', ld_x), to_pyr(dys, 'bf16', ld_y)
    d, _ = make_desc(lib, 'bf16', B, T, shapes, 32, 64, kt, 1, 0, ld_x, ld_y, t_alloc=Ta, t_offset=off)
    nbytes = lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device='cuda')   # stale slabs must not leak
    gw = torch.full(ref.shape, 5.0, dtype=torch.float32, device='cuda')
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 0, P(ws), S())
    e = relmax(gw.cpu(), ref)
    print('lateral wgrad %s: max err / scale %.2e' % (case, e))
    assert e < TOL['bf16']
    first = gw.clone()
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 1, P(ws), S())
    assert relmax(gw.cpu(), 2 * ref) < 2 * TOL['bf16']
    gw2 = torch.empty_like(gw)
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw2), 0, P(ws), S())
    assert torch.equal(first, gw2), 'the weight gradient must be bit-identical from run to run'


# The weight gradient of a kt x 3 x 3 conv 32 -> 32 with ONE output frame (wgrad_t1.hip, bf16: fast_conv3): one temporal
# tap per workgroup, the eight waves split a 16 x 16 tile's rows and are summed through LDS.  Cases: the benchmark's kt = 12
# and configuration 4's kt = 22; level sizes that are not multiples of the tile (ragged right / bottom edges, a level smaller
# than one tile); two clips; pitches wider than the channel count; a frame window inside a longer buffer; more tiles than
# shares (ring wrap, level and clip boundaries inside a share) and fewer.
T1_WGRAD_CASES = [
    # B  t_alloc t_off shapes                             kt
    (1, 12, 0, [(96, 168), (24, 42), (12, 21)], 12),      # fast_conv3 of (4,32): 66 + 6 + 2 tiles over 21 shares
    (1, 22, 0, [(48, 84), (12, 21)], 22),                 # fast_conv3 of (4,64)
    (2, 7, 2, [(17, 33), (5, 3), (1, 1)], 4),             # window [2, 6) of 7 frames, two clips, ragged and tiny levels
    (1, 2, 0, [(16, 16)], 2),                             # one tile, kt 2
    (2, 3, 0, [(40, 50)], 3),                             # 12 tiles per clip, two clips
]


@pytest.mark.parametrize('case', T1_WGRAD_CASES)
def test_one_output_frame_wgrad_kernel(lib, case):
    B, Ta, off, shapes, kt = case
    g = torch.Generator().manual_seed(23)
    w = torch.zeros(32, 32, kt, 3, 3, requires_grad=True)
    xs = [torch.randn(B, 32, Ta, H, W, generator=g).bfloat16().float() for (H, W) in shapes]
    dys = [torch.randn(B, 32, 1, H, W, generator=g).bfloat16().float() for (H, W) in shapes]
    for x, dy in zip(xs, dys):
        F.conv3d(x[:, :, off:off + kt], w, None, padding=(0, 1, 1)).backward(dy)
    ref = w.grad
    ld_x, ld_y = 40, 64
    xd, dyd = to_pyr(xs, 'bf16', ld_x), to_pyr(dys, 'bf16', ld_y)
    d, _ = make_desc(lib, 'bf16', B, kt, shapes, 32, 32, kt, 9, 0, ld_x, ld_y, t_alloc=Ta, t_offset=off)
    nbytes = lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device='cuda')   # stale slabs must not leak
    gw = torch.full(ref.shape, 5.0, dtype=torch.float32, device='cuda')
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 0, P(ws), S())
    e = relmax(gw.cpu(), ref)
    print('one-output-frame wgrad %s: max err / scale %.2e' % (case, e))
    assert e < TOL['bf16']
    first = gw.clone()
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw), 1, P(ws), S())
    assert relmax(gw.cpu(), 2 * ref) < 2 * TOL['bf16']
    gw2 = torch.empty_like(gw)
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw2), 0, P(ws), S())
    assert torch.equal(first, gw2), 'the weight gradient must be bit-identical from run to run'


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_add_inplace_and_mse_loss(lib, prec):
    """sfvos_add_inplace (gradient fan-in of the slow window) and the stand-in loss (value + gradient) against torch."""
    g = torch.Generator().manual_seed(21)
    a, b = torch.randn(5 * 1024 + 8, generator=g), torch.randn(5 * 1024 + 8, generator=g)
    ad, bd = a.to(TDT[prec]).cuda(), b.to(TDT[prec]).cuda()
    want = (ad.float() + bd.float()).to(TDT[prec])
    lib.call('sfvos_add_inplace', P(ad), P(bd), lib.F32 if prec == 'fp32' else lib.BF16, ad.numel(), S())
    assert torch.equal(ad, want)
    if prec == 'bf16':
        return
    from sfvos_amd import MSEProxyLoss
    shapes = [(1, 256, 12, 21), (1, 256, 6, 10), (2, 8, 3, 5)]
    outs = [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes]
    tgts = {str(i): torch.randn(s, generator=g).cuda() for i, s in enumerate(shapes)}
    loss = MSEProxyLoss(tgts)({str(i): o for i, o in enumerate(outs)})
    ref_in = [o.detach().cpu().double().requires_grad_(True) for o in outs]
    ref = sum(((o - tgts[str(i)].cpu().double()) ** 2).mean() for i, o in enumerate(ref_in))
    assert abs(loss.item() - ref.item()) < 1e-6 * abs(ref.item())
    (loss * 3.0).backward()
    (ref * 3.0).backward()
    for o, r in zip(outs, ref_in):
        assert relmax(o.grad.cpu(), r.grad) < 1e-6


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(5, 256, 7, 13), (3, 256, 8, 36), (2, 64, 12, 21)])   # odd planes / 16-byte-aligned planes
def test_layout_roundtrip_and_strided_source(lib, prec, shape):
    T, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    frames = torch.randn(T, C, H, W, generator=g)
    # the reference hands over stack(frames).transpose(1, 2): a non-contiguous [C,T,H,W] view
    view = frames.cuda().unsqueeze(0).transpose(1, 2)[0]          # [C,T,H,W], strides of the frame stack
    dt = lib.F32 if prec == 'fp32' else lib.BF16
    dst = torch.empty((T, H, W, C), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_frames_to_ndhwc', P(view), view.stride(1), view.stride(0), view.stride(2), view.stride(3), P(dst),
             dt, T, C, H, W, C, S())
    ref = frames.permute(0, 2, 3, 1)
    assert relmax(dst.float().cpu(), ref) < (1e-7 if prec == 'fp32' else 8e-3)
    back = torch.zeros((T, C, H, W), dtype=torch.float32, device='cuda')
    lib.call('sfvos_ndhwc_to_frames', P(dst), dt, P(back), back.stride(0), back.stride(1), back.stride(2),
             back.stride(3), T, C, H, W, C, 0, S())
    assert torch.equal(back.cpu(), dst.float().cpu().permute(0, 3, 1, 2))
    lib.call('sfvos_ndhwc_to_frames', P(dst), dt, P(back), back.stride(0), back.stride(1), back.stride(2),
             back.stride(3), T, C, H, W, C, 1, S())
    assert torch.equal(back.cpu(), 2 * dst.float().cpu().permute(0, 3, 1, 2))
    M = H * W
    planar = torch.empty((C, M), dtype=torch.float32, device='cuda')
    lib.call('sfvos_ndhwc_to_planar', P(dst[0]), dt, P(planar), M, C, C, S())
    assert torch.equal(planar.cpu(), dst[0].float().cpu().reshape(M, C).t())
    again = torch.empty((M, C), dtype=TDT[prec], device='cuda')
    lib.call('sfvos_planar_to_ndhwc', P(planar), P(again), dt, M, C, C, S())
    assert torch.equal(again.cpu(), dst[0].reshape(M, C).cpu())


def _levels(lib, ms):
    lv = lib.Levels()
    lv.n_levels = len(ms)
    for i, m in enumerate(ms):
        lv.m[i] = m
    return lv


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('C,relu', [(192, 1), (224, 0), (32, 1), (64, 1)])
def test_batchnorm_forward_backward_per_level(lib, prec, C, relu):
    ms = [3 * 11 * 23, 700, 37]          # three levels with their own statistics
    L, M = len(ms), sum(ms)
    g = torch.Generator().manual_seed(11)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    xs = [torch.randn(m, C, generator=g) * (1.0 + 0.7 * i) + 0.3 * i for i, m in enumerate(ms)]
    dys = [torch.randn(m, C, generator=g) for m in ms]
    if prec == 'bf16':
        xs, dys = [v.bfloat16().float() for v in xs], [v.bfloat16().float() for v in dys]
    dt = lib.F32 if prec == 'fp32' else lib.BF16
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = torch.zeros(C), torch.ones(C)
    ref_y, ref_dx = [], []
    for x, dy in zip(xs, dys):   # the reference: one BN call per level, running stats updated in order
        xr = x.clone().requires_grad_(True)
        yr = F.batch_norm(xr.t().reshape(1, C, -1), rm, rv, gr, br, True, 0.1, 1e-5)
        yr = F.relu(yr) if relu else yr
        yr.backward(dy.t().reshape(1, C, -1))
        ref_y.append(yr.detach().reshape(C, -1).t())
        ref_dx.append(xr.grad)
    # forward statistics from one "partial row" (sum, sumsq) per level
    part = torch.stack([torch.stack([x.double().sum(0), (x.double() ** 2).sum(0)]) for x in xs]).float().cuda()
    cf = torch.zeros((L, 10, C), dtype=torch.float32, device='cuda')
    cs = 10 * C
    gd, bd = gamma.cuda(), beta.cuda()
    rows_pl = (ctypes.c_int * lib.MAX_LEVELS)(*([1] * L))
    lv = _levels(lib, ms)
    lib.call('sfvos_bn_finalize', P(part), L, rows_pl, lv.m, P(gd), P(bd), 1e-5, C, P(cf[0, 0]), P(cf[0, 1]),
             P(cf[0, 2]), P(cf[0, 3]), P(cf[0, 4]), cs, S())
    rmd, rvd = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    nbt = torch.full((), 3, dtype=torch.int64, device='cuda')
    lib.call('sfvos_bn_running_update', P(rmd), P(rvd), P(cf[0, 0]), P(cf[0, 4]), L, cs, C, 0.1, P(nbt), S())
    assert relmax(rmd.cpu(), rm) < 1e-5 and relmax(rvd.cpu(), rv) < 1e-5 and int(nbt) == 3 + L
    ld = C + 32
    xd = torch.cat(xs).to(TDT[prec]).cuda()
    y = torch.full((M, ld), 9.0, dtype=TDT[prec], device='cuda')
    # the same running-statistics update folded into the BN-apply launch (sfvos_bn_running): bitwise the same result
    rm2, rv2 = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    nbt2 = torch.full((), 3, dtype=torch.int64, device='cuda')
    run = lib.BnRunning()
    run.running_mean, run.running_var, run.means, run.vars_unbiased = (rm2.data_ptr(), rv2.data_ptr(),
                                                                       cf[0, 0].data_ptr(), cf[0, 4].data_ptr())
    run.num_batches_tracked, run.n_updates, run.momentum = nbt2.data_ptr(), L, 0.1
    lib.call('sfvos_bn_apply', P(xd), C, P(y, 32), ld, dt, ctypes.byref(lv), C, P(cf[0, 2]), P(cf[0, 3]), cs, relu,
             ctypes.byref(run), S())
    assert torch.equal(rm2, rmd) and torch.equal(rv2, rvd) and int(nbt2) == 3 + L
    assert relmax(y[:, 32:].float().cpu(), torch.cat(ref_y)) < (1e-5 if prec == 'fp32' else 8e-3)
    assert torch.all(y[:, :32].float() == 9.0)
    y2 = torch.full((M, ld), 9.0, dtype=TDT[prec], device='cuda')
    lib.call('sfvos_bn_apply', P(xd), C, P(y2, 32), ld, dt, ctypes.byref(lv), C, P(cf[0, 2]), P(cf[0, 3]), cs, relu, None,
             S())
    assert torch.equal(y2, y) and int(nbt2) == 3 + L   # NULL: no update
    # backward
    dyd = torch.zeros((M, ld), dtype=TDT[prec], device='cuda')
    dyd[:, 32:] = torch.cat(dys).to(TDT[prec])
    rows = lib.load().sfvos_bn_bwd_rows(ctypes.byref(lv))
    assert rows >= L
    bpart = torch.empty((rows, 2, C), dtype=torch.float32, device='cuda')
    lib.call('sfvos_bn_bwd_reduce', P(dyd, 32), ld, P(xd), C, dt, ctypes.byref(lv), C, P(cf[0, 2]), P(cf[0, 3]),
             P(cf[0, 0]), P(cf[0, 1]), cs, relu, P(bpart), S())
    dg, db = torch.full((C,), 2.0, device='cuda'), torch.full((C,), -1.0, device='cuda')
    lib.call('sfvos_bn_bwd_finalize', P(bpart), ctypes.byref(lv), P(gd), P(cf[0, 0]), P(cf[0, 1]), cs, C, 1,
             P(cf[0, 5]), P(cf[0, 6]), P(cf[0, 7]), P(cf[0, 8]), P(cf[0, 9]), S())
    dx = torch.empty((M, C), dtype=TDT[prec], device='cuda')
    biasp = torch.empty((rows, C), dtype=torch.float32, device='cuda')
    lib.call('sfvos_bn_bwd_apply', P(dyd, 32), ld, P(xd), C, P(dx), C, dt, ctypes.byref(lv), C, P(cf[0, 2]),
             P(cf[0, 3]), cs, relu, P(cf[0, 5]), P(cf[0, 6]), P(cf[0, 7]), P(biasp), P(cf[0, 8]), P(cf[0, 9]), P(dg),
             P(db), 1, S())   # accumulate: dgamma / dbeta are ADDED to what the buffers held
    assert relmax(dg.cpu() - 2.0, gr.grad) < 1e-4 and relmax(db.cpu() + 1.0, br.grad) < 1e-4
    assert relmax(dx.float().cpu(), torch.cat(ref_dx)) < (1e-4 if prec == 'fp32' else 1e-2)
    dbias = torch.empty(C, device='cuda')
    lib.call('sfvos_reduce_rows', P(biasp), rows, C, P(dbias), 0, S())
    assert float(dbias.abs().max()) < 1e-2 * float(dx.float().abs().sum(0).max())  # sums to ~0 in train mode
    if prec == 'fp32':  # (bf16: the kernel sums dx before rounding it for storage)
        assert relmax(dbias.cpu() + 1.0, dx.float().sum(0).cpu() + 1.0) < 1e-3


def test_bn_apply_fp8_feeds_an_e4m3_conv_in_ndhwc(lib):
    """sfvos_bn_apply_fp8 writes act(x*scale+shift)*act_scale as e4m3 into a channel slice of an [M][256]-byte buffer
    (the slow pathway's concat), and sfvos_conv3d reads that buffer as plain-NDHWC e4m3 operands (ld_x = 256 bytes)."""
    g = torch.Generator().manual_seed(31)
    B, T, shapes, C = 1, 3, [(7, 19), (4, 6)], 256
    ms = [B * T * H * W for H, W in shapes]
    M = sum(ms)
    lv = _levels(lib, ms)
    x = torch.randn(M, C, generator=g).bfloat16()
    scale = torch.rand(len(shapes), 10, C, generator=g) + 0.5
    shift = torch.randn(len(shapes), 10, C, generator=g) * 0.3
    cf = torch.zeros(len(shapes), 10, C)
    cf[:, 2], cf[:, 3] = scale[:, 2], shift[:, 3]
    cfd, xd = cf.cuda(), x.cuda()
    act = 32.0
    y = torch.full((M, C), 0x7f, dtype=torch.uint8, device='cuda')
    sat = torch.zeros(1, dtype=torch.int32, device='cuda')
    # two channel slices, as slow_conv (192) and the lateral (64) write them
    for c0, cn in ((0, 192), (192, 64)):
        xs_ = xd[:, c0:c0 + cn].contiguous()
        lib.call('sfvos_bn_apply_fp8', P(xs_), cn, P(y, c0), C, ctypes.byref(lv), cn, P(cfd[0, 2], c0), P(cfd[0, 3], c0),
                 10 * C, 1, act, P(sat), None, S())
    f8 = torch.float8_e4m3fn
    lvl = torch.cat([torch.full((m,), i) for i, m in enumerate(ms)])
    ref = torch.relu(x.float() * cf[lvl, 2] + cf[lvl, 3]) * act
    want = ref.clamp(max=448.0).to(f8)
    gotq = y.cpu().view(f8).float()
    diff = gotq != want.float()   # an fma in the kernel may round a tie the other way: at most one e4m3 step, rarely
    assert float(diff.float().mean()) < 1e-3
    assert float(((gotq - want.float()).abs() / want.float().abs().clamp_min(2.0 ** -9)).max()) <= 0.126
    assert abs(int(sat) - int((ref > 448.0).sum())) <= 2
    # the e4m3 buffer as the x operand of a wide 3x3 conv
    cout, kt = 192, 2
    w = torch.randn(cout, C, kt, 3, 3, generator=g) / np.sqrt(C * kt * 9)
    wp = torch.empty(w.numel(), dtype=torch.uint8, device='cuda')
    bd = torch.empty((3, cout), dtype=torch.float32, device='cuda')
    w_dev = w.cuda()
    lib.call('sfvos_pack_weights_fp8', P(w_dev), None, P(wp), P(bd), cout, C, kt, 9, act, S())
    d, t_out = make_desc(lib, 'bf16', B, T, shapes, C, cout, kt, 9, 0, C, cout)
    d.dtype = lib.FP8
    Mo = sum(B * t_out * H * W for H, W in shapes)
    out = torch.zeros((Mo, cout), dtype=torch.bfloat16, device='cuda')
    lib.call('sfvos_conv3d', ctypes.byref(d), P(y), P(wp), P(bd), P(out), None, S())
    ws = 448.0 / w.abs().amax(dim=(1, 2, 3, 4))
    wq = (w * ws[:, None, None, None, None]).to(f8).float() / ws[:, None, None, None, None]
    xq = gotq / act
    off = 0
    xs5 = []
    for (H, W), m in zip(shapes, ms):
        xs5.append(xq[off:off + m].reshape(B, T, H, W, C).permute(0, 4, 1, 2, 3))
        off += m
    refs = [F.conv3d(v, wq, None, padding=(0, 1, 1)) for v in xs5]
    for a, r in zip(from_pyr(out, B, cout, t_out, shapes), refs):
        assert relmax(a, r) < 1e-2


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('shapes', [[(12, 21), (6, 11), (3, 6)], [(8, 16), (4, 8)]])   # odd sizes / vectorisable
def test_pyramid_layout_passes_in_one_launch(lib, prec, shapes):
    """sfvos_pyramid_to_frames / sfvos_frames_to_pyramid: all levels in one launch, bit-identical to the per-level
    sfvos_ndhwc_to_frames / sfvos_frames_to_ndhwc calls (and accumulate adds)."""
    B, C, ld = 2, 64, 72
    dt = lib.F32 if prec == 'fp32' else lib.BF16
    g = torch.Generator().manual_seed(2)
    planes = [torch.randn(B, C, H, W, generator=g).cuda() for (H, W) in shapes]
    M = sum(B * H * W for H, W in shapes)
    arr = (lib.PlanarLevel * len(shapes))()
    for i, t in enumerate(planes):
        arr[i].ptr = t.data_ptr()
        arr[i].stride_t, arr[i].stride_c, arr[i].stride_h, arr[i].stride_w = t.stride()
        arr[i].h, arr[i].w = t.shape[2], t.shape[3]
    got = torch.full((M, ld), 5.0, dtype=TDT[prec], device='cuda')
    ref = torch.full((M, ld), 5.0, dtype=TDT[prec], device='cuda')
    lib.call('sfvos_frames_to_pyramid', arr, len(shapes), P(got), dt, B, C, ld, S())
    off = 0
    for t, (H, W) in zip(planes, shapes):
        lib.call('sfvos_frames_to_ndhwc', P(t), t.stride(0), t.stride(1), t.stride(2), t.stride(3), P(ref, off * ld), dt,
                 B, C, H, W, ld, S())
        off += B * H * W
    assert torch.equal(got, ref)
    back = [torch.ones(B, C, H, W, device='cuda') for (H, W) in shapes]
    for i, t in enumerate(back):
        arr[i].ptr = t.data_ptr()
    lib.call('sfvos_pyramid_to_frames', P(got), dt, arr, len(shapes), B, C, ld, 1, S())   # accumulate onto ones
    off = 0
    for t, (H, W) in zip(back, shapes):
        want = got[off:off + B * H * W, :C].float().reshape(B, H, W, C).permute(0, 3, 1, 2) + 1.0
        assert torch.equal(t, want)
        off += B * H * W
    with pytest.raises(RuntimeError):
        lib.call('sfvos_frames_to_pyramid', arr, 0, P(got), dt, B, C, ld, S())


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_pack_weights_batch_equals_the_single_calls(lib, prec):
    """sfvos_pack_weights_batch: every image bit-identical to its sfvos_pack_weights_fwd / _dgrad call."""
    g = torch.Generator().manual_seed(8)
    shapes = [(32, 256, 11, 9, 0), (192, 256, 2, 9, 0), (64, 32, 20, 1, 0), (32, 32, 12, 9, 1), (64, 32, 5, 1, 1),
              (224, 256, 2, 9, 1)]
    items = (lib.PackItem * len(shapes))()
    ws, got, ref = [], [], []
    for i, (co, ci, kt, taps, dg) in enumerate(shapes):
        w = torch.randn(co, ci, kt, 3 if taps == 9 else 1, 3 if taps == 9 else 1, generator=g).cuda()
        a = torch.zeros(w.numel(), dtype=TDT[prec], device='cuda')
        b = torch.zeros(w.numel(), dtype=TDT[prec], device='cuda')
        ws.append(w); got.append(a); ref.append(b)
        items[i].w, items[i].packed = w.data_ptr(), a.data_ptr()
        items[i].c_out, items[i].c_in, items[i].kt, items[i].taps, items[i].dgrad = co, ci, kt, taps, dg
        lib.call('sfvos_pack_weights_dgrad' if dg else 'sfvos_pack_weights_fwd', P(w), P(b),
                 lib.F32 if prec == 'fp32' else lib.BF16, co, ci, kt, taps, S())
    lib.call('sfvos_pack_weights_batch', items, len(shapes), lib.F32 if prec == 'fp32' else lib.BF16, S())
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError):
        lib.call('sfvos_pack_weights_batch', items, 0, lib.F32, S())


def test_sgd_step_and_scale(lib):
    n = 100003
    g = torch.Generator().manual_seed(5)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=1e-3, momentum=0.9, weight_decay=1e-4)
    pd, gd, buf = p.cuda(), gr.cuda(), torch.zeros(n, device='cuda')
    for step in range(3):
        pr.grad = gr.clone()
        opt.step()
        lib.call('sfvos_sgd_step', P(pd), P(gd), P(buf), n, 1e-3, 0.9, 1e-4, 1 if step == 0 else 0, S())
        assert float((pd.cpu() - pr.detach()).abs().max()) < 1e-6
    lib.call('sfvos_scale', P(gd), n, 0.25, S())
    assert torch.equal(gd.cpu(), gr * 0.25)


def test_bad_arguments_report_errors(lib):
    d, _ = make_desc(lib, 'fp32', 1, 4, [(8, 8)], 48, 32, 2, 9, 0, 48, 32)  # c_in not a multiple of 32
    assert lib.load().sfvos_conv3d_stat_rows(ctypes.byref(d), None) < 0
    assert b'multiples of 32' in lib.load().sfvos_last_error()
    d, _ = make_desc(lib, 'fp32', 1, 4, [(8, 8)], 64, 32, 2, 9, 0, 64, 32, t_alloc=3)  # window outside a frame RING
    d.x_frame_stride = 64
    assert lib.load().sfvos_conv3d_stat_rows(ctypes.byref(d), None) < 0
    d, _ = make_desc(lib, 'fp32', 1, 4, [(8, 8)], 64, 32, 2, 9, 0, 64, 32, t_alloc=0)
    assert lib.load().sfvos_conv3d_stat_rows(ctypes.byref(d), None) < 0
    with pytest.raises(RuntimeError):
        lib.call('sfvos_scale', None, 10, 1.0, S())


@pytest.mark.parametrize('n', [0, 1, 5])
def test_mask_union_matches_the_reference_numpy_loop(lib, n):
    """davis_evaluate.py:36-42: total = OR_k (mask_k >= 0.5)[0]; comparison + OR only -> bit-exact.  Values sit on
    and around the threshold, including exactly 0.5."""
    from sfvos_amd import union_mask
    g = torch.Generator().manual_seed(8)
    H, W = 37, 53
    masks = torch.rand(n, 1, H, W, generator=g)
    if n:
        masks[0, 0, :4] = 0.5
        masks[-1, 0, 4:8] = float(np.nextafter(np.float32(0.5), np.float32(0)))
    total = np.zeros((H, W), dtype=bool)
    for m in masks:                                  # the reference's loop, verbatim semantics
        total = np.logical_or(total, (m.numpy() >= 0.5)[0])
    got = union_mask(masks.cuda())
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), total)


@pytest.mark.parametrize('case', [(1, 6, [(12, 21), (5, 9)], 256, 32, 3), (2, 5, [(9, 17)], 64, 32, 2),
                                  (1, 14, [(10, 33)], 128, 32, 11),
                                  # the wide kernel (slow pathway): 192 / 224 / 256 output channels, 1-3 output frames
                                  (1, 4, [(12, 21), (6, 10)], 256, 192, 2), (1, 2, [(9, 35)], 256, 224, 2),
                                  (2, 3, [(6, 10), (3, 5)], 128, 256, 2)])
def test_conv3d_fp8_operands_match_a_dequantised_reference(lib, case):
    """SFVOS_FP8 (BASELINE config 5): e4m3 x (64-channel groups) and e4m3 weight image with per-output-channel scales,
    f32 accumulate, bf16 result -- the frame-split kernel (c_out 32) and the wide kernel (c_out 192-256).  The
    reference convolves the SAME quantised values (torch.float8_e4m3fn round trip) in fp32, so only summation order
    and the bf16 store differ: 1e-2."""
    B, T, shapes, cin, cout, kt = case
    g = torch.Generator().manual_seed(77)
    w = torch.randn(cout, cin, kt, 3, 3, generator=g) / np.sqrt(cin * kt * 9)
    w[3] *= 7.0                                                     # channels with different ranges
    bias = torch.randn(cout, generator=g) * 0.1
    xs = [torch.randn(B, cin, T, H, W, generator=g) for (H, W) in shapes]
    act_scale = 32.0
    M = sum(B * T * H * W for H, W in shapes)
    x_gr = torch.zeros((cin // 64, M, 64), dtype=torch.uint8, device='cuda')
    off = 0
    for x in xs:
        H, W = x.shape[3], x.shape[4]
        xc = x.cuda()
        for b in range(B):
            s = xc[b]
            lib.call('sfvos_frames_to_groups_fp8', P(s), s.stride(1), s.stride(0), s.stride(2), s.stride(3),
                     P(x_gr, (off + b * T * H * W) * 64), T, cin, H, W, M * 64, act_scale, None, S())
        off += B * T * H * W
    wp = torch.empty(w.numel(), dtype=torch.uint8, device='cuda')
    bd = torch.empty((3, cout), dtype=torch.float32, device='cuda')
    w_dev, bias_dev = w.cuda(), bias.cuda()   # keep both alive: two temporaries would share one freed block
    lib.call('sfvos_pack_weights_fp8', P(w_dev), P(bias_dev), P(wp), P(bd), cout, cin, kt, 9, act_scale, S())
    d, t_out = make_desc(lib, 'bf16', B, T, shapes, cin, cout, kt, 9, 0, 64, cout)
    d.dtype = lib.FP8
    d.x_group_stride = M * 64
    Mo = sum(B * t_out * H * W for H, W in shapes)
    y = torch.zeros((Mo, cout), dtype=torch.bfloat16, device='cuda')
    rows = lib.load().sfvos_conv3d_stat_rows(ctypes.byref(d), None)
    part = torch.zeros((rows, 2, cout), dtype=torch.float32, device='cuda')
    lib.call('sfvos_conv3d', ctypes.byref(d), P(x_gr), P(wp), P(bd), P(y), P(part), S())
    torch.cuda.synchronize()
    # reference on the same quantised operands
    f8 = torch.float8_e4m3fn
    ws = 448.0 / w.abs().amax(dim=(1, 2, 3, 4))
    wq = (w * ws[:, None, None, None, None]).to(f8).float() / ws[:, None, None, None, None]
    assert torch.allclose(bd[2].cpu(), ws, rtol=1e-6) and torch.allclose(bd[1].cpu(), 1.0 / (act_scale * ws), rtol=1e-6)
    refs = [F.conv3d((x * act_scale).to(f8).float() / act_scale, wq, bias, padding=(0, 1, 1)) for x in xs]
    got = from_pyr(y, B, cout, t_out, shapes)
    for a, r in zip(got, refs):
        assert relmax(a, r) < 1e-2
    # and the quantisation error itself against the unquantised conv, for the record (not a gate): ~3-5 %
    full = [F.conv3d(x, w, bias, padding=(0, 1, 1)) for x in xs]
    err = max(float((a.double() - f.double()).norm() / f.double().norm()) for a, f in zip(got, full))
    print('e4m3 conv rel-L2 error vs fp32 operands: %.3f' % err)
    assert err < 0.1
