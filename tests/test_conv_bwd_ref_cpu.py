"""CPU: pins of tests/conv_bwd_ref.py, the float64 references and input generators of
tests/test_gpu_conv_bwd_kernels.py.  wgrad_ref and dgrad_ref equal the autograd of F.conv3d in double; every case meets
the preconditions of exact comparison (integers, sums of |products| below 2^24, |dx| <= 256 for bf16 before and after the
accumulate); the 'several' cases give every split-K workgroup at least two tiles by the planner's own numbers (without a
device it assumes 256 compute units); every reference is computed in bounded time.

Largest reference time measured on 8 CPU threads: 0.5 s ('cfg0 several': 99 matmuls of [32 x 12 852] by [12 852 x 256]);
every data-gradient reference 0.1 s or less.  The limit asserted is 5 s."""
import ctypes
import time

import pytest
import torch
import torch.nn.functional as F

import conv_bwd_ref as R

REF_SECONDS = 5.0


def timed(cached, name):
    """(result, seconds) of an uncached call; a time beyond the limit is taken once more, so that a loaded machine does not
    fail what the amount of work does not."""
    best = float('inf')
    for _ in range(2):
        cached.cache_clear()
        t0 = time.perf_counter()
        out = cached(name)
        best = min(best, time.perf_counter() - t0)
        if best < REF_SECONDS:
            break
    return out, best


@pytest.mark.parametrize('taps,t_alloc,t_off', [(9, 4, 0), (1, 5, 0), (9, 3, -1), (1, 4, 2)])
def test_wgrad_ref_equals_autograd_of_conv3d_in_double(taps, t_alloc, t_off):
    """Random float64 operands, two levels, two clips; (9, 3, -1) and (1, 4, 2): the window [t_off, t_off + 4) sticks out
    of the buffer in front / behind, the missing frames are zero frames."""
    g = torch.Generator().manual_seed(3 + taps + t_alloc)
    B, T, cin, cout, kt, k = 2, 4, 5, 3, 2, 3 if taps == 9 else 1
    shapes = [(4, 5), (1, 2)]
    xs = [torch.randn(B, cin, t_alloc, H, W, generator=g, dtype=torch.float64) for H, W in shapes]
    dys = [torch.randn(B, cout, T - kt + 1, H, W, generator=g, dtype=torch.float64) for H, W in shapes]
    wins = [R.window(x, t_off, T) for x in xs]
    if t_off < 0:
        assert bool((wins[0][:, :, 0] == 0).all()) and bool((wins[0][:, :, 1] == xs[0][:, :, 0]).all())
    w = torch.zeros(cout, cin, kt, k, k, dtype=torch.float64, requires_grad=True)
    for v, dy in zip(wins, dys):
        F.conv3d(v, w, None, padding=(0, 1, 1) if taps == 9 else 0).backward(dy)
    got = R.wgrad_ref(wins, dys, kt, taps)
    assert float((got - w.grad).abs().max()) < 1e-12 * float(w.grad.abs().max())


@pytest.mark.parametrize('taps,kt', [(9, 3), (1, 2)])
def test_dgrad_ref_equals_autograd_of_conv3d_in_double(taps, kt):
    g = torch.Generator().manual_seed(5 + taps)
    B, T, cin, cout, k = 2, 4, 5, 3, 3 if taps == 9 else 1
    shapes = [(4, 5), (1, 2)]
    w = torch.randn(cout, cin, kt, k, k, generator=g, dtype=torch.float64)
    dys = [torch.randn(B, cout, T - kt + 1, H, W, generator=g, dtype=torch.float64) for H, W in shapes]
    got = R.dgrad_ref(dys, w, kt, taps)
    for (H, W), dy, dx in zip(shapes, dys, got):
        x = torch.zeros(B, cin, T, H, W, dtype=torch.float64, requires_grad=True)
        F.conv3d(x, w, None, padding=(0, 1, 1) if taps == 9 else 0).backward(dy)
        assert dx.shape == x.grad.shape
        assert float((dx - x.grad).abs().max()) < 1e-12 * float(x.grad.abs().max())


@pytest.mark.parametrize('name', list(R.WGRAD_CASES))
def test_wgrad_cases_are_exactly_summable_and_quick_to_reference(name):
    """Integer operands of the stated range, an integer reference, every sum of |products| (plus the accumulate prefill)
    below 2^24; full-significand cases stay within 1000 positions; no element of the reference is left without any
    contribution in the small cases (a dead element would check nothing).  The reference takes bounded time."""
    B, T, t_alloc, t_off, shapes, cin, cout, kt, taps, precs, gen, flags = R.WGRAD_CASES[name]
    (xs, dys, ref, mag), seconds = timed(R.wgrad_inputs, name)
    print('%-24s %6d positions, reference in %.2f s' % (name, R.wgrad_positions(name), seconds))
    assert seconds < REF_SECONDS
    k = 3 if taps == 9 else 1
    assert ref.shape == mag.shape == (cout, cin, kt, k, k)
    assert cin % 32 == 0 and set(precs) <= set(R.BOTH)
    if gen == 'random':
        assert R.wgrad_positions(name) <= 300
        for v in R.wgrad_inputs(name, 'bf16')[0]:      # the bf16 run's operands are bf16 values
            assert bool((v == v.bfloat16().float()).all())
        assert float(mag.min()) > 0 and bool((ref.abs() <= mag).all())
        return
    a = 1 if gen == 'ternary' else 127
    for v in xs + dys:
        assert v.dtype == torch.int8 and int(v.abs().max()) <= a
        if v.numel() >= 4096:
            assert int(v.min()) == -a and int(v.max()) == a
    if gen == 'full':
        assert R.wgrad_positions(name) <= R.FULL_MAX_POSITIONS
        assert float(ref.abs().max()) > 2.0 ** 16     # sums that need more than 16 significand bits
    assert R.integers_ok(ref, mag + R.PREFILL)
    assert float((ref.abs() <= mag).double().min()) == 1.0
    pre = R.wgrad_prefill(name)
    assert pre.shape == ref.shape and R.integers_ok(pre, pre.abs()) and float(pre.abs().max()) == R.PREFILL
    # a temporal tap that meets a frame of the buffer carries something; one that meets zero frames only is exactly zero
    per_tap = ref.abs().sum((0, 1, 3, 4))
    for dt in range(kt):
        real = any(0 <= t_off + dt + t < t_alloc for t in range(T - kt + 1))
        assert (float(per_tap[dt]) > 0) == real, (dt, float(per_tap[dt]))


@pytest.mark.parametrize('name', list(R.DGRAD_CASES))
def test_dgrad_cases_are_exactly_summable_and_quick_to_reference(name):
    """Ternary dy and w, integer dx with every sum of |products| below 2^24, and |dx| <= 256 with and without the prefill
    of the accumulate run, so a bf16 store is exact."""
    B, T, shapes, cin, cout, kt, taps, precs = R.DGRAD_CASES[name]
    (dys, w, refs, mags, pre), seconds = timed(R.dgrad_inputs, name)
    print('%-24s reference in %.2f s' % (name, seconds))
    assert seconds < REF_SECONDS
    assert int(w.abs().max()) == 1 and all(int(dy.abs().max()) == 1 for dy in dys)
    nonzero = float(w.double().abs().sum((0, 2, 3, 4)).mean())
    assert 0.5 * min(R.CONV_NONZERO, cout * kt * taps) <= nonzero <= 1.2 * R.CONV_NONZERO
    for (H, W), ref, mag, p in zip(shapes, refs, mags, pre):
        assert ref.shape == p.shape == (B, cin, T, H, W)
        assert R.integers_ok(ref, mag + R.PREFILL) and R.integers_ok(p, p.abs())
        assert float(ref.abs().max()) <= R.BF16_EXACT and float((ref + p).abs().max()) <= R.BF16_EXACT
        assert float(ref.abs().max()) > 0


def plan_tile_height(prec, cin, cout, kt, taps, t_out):
    """Tile height of make_wgrad_plan (csrc/wgrad.hip) for the configurations of the 'several' cases."""
    if prec == 'fp32':
        return 4
    if taps == 1:
        return 8
    if cin <= 32:
        return 4 if (t_out == 1 and kt > 1) else 16     # cfg 4 / the row-split cfg 2
    return 6 if (t_out % 2 == 0 and t_out >= 4) else 8  # frame pairs / row pairs


SEVERAL = [(n, p) for n, c in R.WGRAD_CASES.items() if 'several' in c[11] for p in c[9]]


@pytest.mark.parametrize('name,prec', SEVERAL)
def test_several_cases_sweep_at_least_two_tiles_per_workgroup(name, prec):
    """The split count is the workspace size over the size of one slab (the lateral and one-output-frame kernels decline
    these shapes, so the generic kernel's workspace is the whole of it)."""
    from sfvos_amd import _lib
    lib = _lib.load()
    B, T, t_alloc, t_off, shapes, cin, cout, kt, taps, _, _, _ = R.WGRAD_CASES[name]
    d = _lib.ConvDesc()
    d.dtype = _lib.F32 if prec == 'fp32' else _lib.BF16
    d.batch, d.t_in, d.c_in, d.c_out, d.kt, d.taps, d.pad_t = B, T, cin, cout, kt, taps, 0
    d.t_alloc, d.t_offset, d.ld_x, d.ld_y, d.accumulate = t_alloc, t_off, cin, cout, 0
    d.pyr = _lib.make_pyramid(shapes)
    nbytes = int(lib.sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d)))
    slab = 4 * cout * cin * kt * taps
    assert nbytes > 0 and nbytes % slab == 0
    split = nbytes // slab
    th = plan_tile_height(prec, cin, cout, kt, taps, T - kt + 1)
    tiles = sum(B * -(-H // th) * -(-W // 16) for H, W in shapes)
    print('%-20s %s: %d tiles of %d rows, split %d, %.1f tiles per workgroup' % (name, prec, tiles, th, split, tiles / split))
    assert split >= 2 and tiles / split >= 2
