"""CPU: pins of tests/fp8_ref.py, the references and input generators of tests/test_gpu_fp8_kernels.py.  The e4m3 codec
written from the format equals torch.float8_e4m3fn on every code and on EDGE_VALUES clamped to +-448 (torch's cast does not
saturate: the clamp is the library's contract); conv_ref equals F.conv3d in double; every exact case meets the
preconditions of exact comparison on its float64 reference (quantised operands decode to the originals, power-of-two weight
scales, |y| <= 256 integer units, per level sum |v| and sum v^2 below 2^24 units, accumulator below 2^24); every case
reaches the kernel instance it names by the planner's own numbers (sfvos_conv3d_stat_rows; without a device the planner
assumes 256 compute units, the MI355X's count)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fp8_ref as R

F8 = torch.float8_e4m3fn
LIMIT = 2.0 ** 24


def test_decode_equals_torch_on_all_256_codes_and_encode_inverts_it():
    codes = torch.arange(256, dtype=torch.uint8)
    mine, theirs = R.e4m3_decode(codes), codes.view(F8).double()
    nan = torch.isnan(theirs)
    assert nan.tolist() == [c in (0x7f, 0xff) for c in range(256)]
    assert torch.equal(torch.isnan(mine), nan) and torch.equal(mine[~nan], theirs[~nan])
    assert torch.equal(torch.signbit(mine), torch.signbit(theirs))
    assert float(mine[0x7e]) == 448.0 and float(mine[0x01]) == 2.0 ** -9 and float(mine[0x38]) == 1.0
    assert torch.equal(R.canon(R.e4m3_encode(mine)), R.canon(codes))       # every value encodes to its own code, -0 too


def test_encode_equals_torch_on_the_edge_values_clamped_to_448():
    e = R.EDGE_VALUES
    assert e.dtype == torch.float32 and e.numel() > 1000
    assert bool(torch.isinf(e).any()) and bool(torch.isnan(e).any()) and bool((e == 449).any()) and bool((e == -3e38).any())
    want = e.clamp(-448.0, 448.0).to(F8).view(torch.uint8)                  # clamp passes NaN through
    got = R.e4m3_encode(e)
    assert torch.equal(R.canon(got), R.canon(want))
    # the contract, spelt out
    enc = lambda v: int(R.e4m3_encode(torch.tensor([v], dtype=torch.float32))[0])
    assert enc(449.0) == 0x7e and enc(-1e6) == 0xfe and enc(float('inf')) == 0x7e and enc(float('-inf')) == 0xfe
    assert enc(464.0) == 0x7e and enc(465.0) == 0x7e and enc(float('nan')) & 0x7f == 0x7f
    assert enc(-0.0) == 0x80 and enc(0.0) == 0x00 and enc(2.0 ** -10) == 0x00 and enc(-2.0 ** -10) == 0x80
    up = float(torch.nextafter(torch.tensor(2.0 ** -10), torch.tensor(1.0)))
    assert enc(up) == 0x01
    assert enc(1.0625) == 0x38 and enc(1.1875) == 0x3a                      # ties to the even code, down and up


def test_quantise_counts_in_fp32_and_pack_weights_ref_rows():
    src = torch.tensor([14.0, 14.000001, -15.0, float('inf'), float('nan'), 0.0, -0.0])
    codes, n = R.quantise(src, 32.0)
    assert n == 3 and codes.tolist()[:4] == [0x7e, 0x7e, 0xfe, 0x7e] and codes.tolist()[5:] == [0x00, 0x80]
    w = torch.zeros(3, 64, 1, 3, 3)
    w[0, 0, 0, 0, 0], w[0, 1, 0, 0, 0], w[2, 5, 0, 1, 1] = -7.0, 1.0, 0.4375
    rows, wc = R.pack_weights_ref(w, None, 32.0)
    assert rows[2].tolist() == [64.0, 1.0, 1024.0] and rows[0].tolist() == [0.0, 0.0, 0.0]
    assert rows[1].tolist() == [2.0 ** -11, 2.0 ** -5, 2.0 ** -15]
    assert int(wc[0, 0, 0, 0, 0]) == 0xfe and float(R.e4m3_decode(wc)[0, 1, 0, 0, 0]) == 64.0 and int(wc[2, 5, 0, 1, 1]) == 0x7e


@pytest.mark.parametrize('kt', [1, 3])
def test_conv_ref_equals_conv3d_in_double(kt):
    g = torch.Generator().manual_seed(9 + kt)
    x = torch.randn(2, 5, 4, 4, 7, generator=g, dtype=torch.float64)
    w = torch.randn(3, 5, kt, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(3, generator=g, dtype=torch.float64)
    want = F.conv3d(x, w, b, padding=(0, 1, 1))
    got = R.conv_ref(x, w, b)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
    assert float((R.conv_ref(x, w, None) - F.conv3d(x, w, None, padding=(0, 1, 1))).abs().max()) < 1e-12


def test_bn_reference_interval_and_saturation_bounds():
    x = torch.tensor([[1.0, -2.0, 14.0, 14.0]], dtype=torch.float64)
    sc, sh = torch.tensor([1.0, 1.0, 1.0, 1.0 + 2.0 ** -20]).double(), torch.tensor([0.0, 1.0, 0.0, 0.0]).double()
    v, lo, hi = R.bn_apply_fp8_ref(x, sc, sh, 1, 32.0)
    assert v[0].tolist()[:3] == [32.0, 0.0, 448.0] and bool((lo <= v).all()) and bool((v <= hi).all())
    assert R.sat_bounds(lo, hi) == (1, 2)            # 448 itself may or may not be exceeded within the interval
    xs, scale, shift = R.bn_exact_inputs(16, [1, 37, 513, 759], 32.0, 0)
    e = R.EDGE_VALUES / 32.0
    carried = torch.cat([x_[:, 2] for x_ in xs])
    for val in (448.0 / 32, 464.0 / 32, 480.0 / 32, float('inf'), -float('inf'), 2.0 ** -15, 1.0625 / 32):
        assert bool((carried == val).any()), val
    assert bool(torch.isnan(carried).any())
    assert not bool(torch.isnan(torch.cat([x_[:, 2] for x_ in R.bn_exact_inputs(16, [1, 37, 513, 759], 32.0, 1)[0]])).any())
    for x_ in xs:
        assert bool((R.bf16_exact(x_) | torch.isnan(x_)).all())


def _tiles(body, B, H, W):
    th = R.TILE_ROWS[body]
    return B * -(-H // th) * -(-W // 32)


@pytest.mark.parametrize('name', list(R.CONV_CASES))
def test_conv_case_reaches_its_instance_and_is_exactly_summable(name):
    from sfvos_amd import _lib
    body, B, T, t_alloc, t_off, shapes, cin, cout, kt, layout, gen, act, blocks = R.CONV_CASES[name]
    # ---- the instance, by the planner's numbers: rows per level = frame blocks x pixel tiles of the body's tile height
    d = _lib.ConvDesc()
    d.dtype, d.batch, d.t_in, d.c_in, d.c_out, d.kt, d.taps, d.pad_t = _lib.FP8, B, T, cin, cout, kt, 9, 0
    d.t_alloc, d.t_offset, d.ld_y = t_alloc, t_off, cout + 64
    d.pyr = _lib.make_pyramid(shapes)
    M = sum(B * t_alloc * H * W for H, W in shapes)
    if layout == 'grouped':
        d.ld_x, d.x_group_stride = 64, (M + 64) * 64
    else:
        d.ld_x = 256 if layout == 'bn' else cin + 64
    rows_pl = (ctypes.c_int * _lib.MAX_LEVELS)()
    rows = _lib.load().sfvos_conv3d_stat_rows(ctypes.byref(d), rows_pl)
    assert rows > 0, _lib.load().sfvos_last_error()
    assert (body == 'fs') == (cout == 32) and cin % 64 == 0
    t_out = T - kt + 1
    if body == 'wide':
        assert blocks == -(-t_out // 2)            # at most two frames per block
    assert [rows_pl[l] for l in range(len(shapes))] == [blocks * _tiles(body, B, H, W) for H, W in shapes], \
        (name, list(rows_pl[:len(shapes)]))
    # ---- the operands
    c = R.conv_inputs(name)
    ws = c['rows'][2].double()
    for q, codes, ref in zip(c['q'], c['xcodes'], c['ref']):
        assert not bool(torch.isnan(q).any()) and ref.shape == (B, cout, t_out) + tuple(q.shape[3:])
        assert torch.equal(R.e4m3_encode(q), codes)
    if gen == 'random':
        assert all(m.shape == r.shape and bool((m >= r.abs()).all()) for m, r in zip(c['mag'], c['ref']))
        return
    # quantised operands decode to the originals; every ws is a power of two that differs between neighbours
    assert torch.equal(c['wq'].float(), c['w']) and torch.equal(c['wq'], c['w'].double())
    assert bool((torch.log2(ws) == torch.log2(ws).round()).all()) and bool((ws[1:] != ws[:-1]).all())
    assert sorted(set(ws.tolist())) == ([64.0, 128.0, 256.0, 512.0] if gen == 'exact' else [32.0, 64.0, 128.0, 256.0])
    assert torch.equal(c['rows'][1].double(), 1.0 / (act * ws))
    qmax = 1 if gen == 'exact' else 15
    assert all(float(q.abs().max()) == qmax and bool((q == q.round()).all()) for q in c['q'])
    assert float((c['wq'] * ws.reshape(-1, 1, 1, 1, 1)).abs().max()) == 448.0
    u = R.unit(name).reshape(1, -1, 1, 1, 1)
    worst_y = worst_s1 = worst_s2 = 0.0
    assert c['acc_mag'] < LIMIT
    for ref in c['ref']:
        v = ref / u
        assert bool((v == v.round()).all())
        s1, s2 = v.abs().sum((0, 2, 3, 4)), (v * v).sum((0, 2, 3, 4))
        worst_y, worst_s1, worst_s2 = max(worst_y, float(v.abs().max())), max(worst_s1, float(s1.max())), \
            max(worst_s2, float(s2.max()))
        assert float(s1.max()) < LIMIT
        assert bool((ref != 0).any((0, 2, 3, 4)).all())          # no dead output channel
    print('%-22s |y| <= %g units, sum |v| <= %g, sum v^2 <= %g, accumulator <= %g' % (
        name, worst_y, worst_s1, worst_s2, c['acc_mag']))
    if gen == 'exact':
        assert worst_y <= 256.0 and worst_s2 < LIMIT
    else:
        assert cin * kt == 64 and shapes == R.LV_SMALL and worst_y > 256.0     # the smallest c_in * kt; y needs its tolerance
