"""Float64 references of the backward half of the conv -- the weight gradient (csrc/wgrad.hip, csrc/lateral_wgrad.hip,
csrc/wgrad_t1.hip) and the data gradient (sfvos_conv3d with pad_t = kt - 1: csrc/conv3d.hip, csrc/lateral.hip) -- in plain
torch on the CPU, and the generators of the inputs of tests/test_gpu_conv_bwd_kernels.py.  tests/test_conv_bwd_ref_cpu.py
pins both: the references against the autograd of F.conv3d in double, the inputs against the preconditions the GPU tests
rely on.  Never imported by the package.

Exactly summable operands (kernel_util's docstring): every operand is a small integer, so every product and every partial
sum, in any order and any partition into tiles, shares, slabs and split groups, is an integer below 2^24: every fp32
addition is exact and the kernel must EQUAL float64.  Two generators:

  ternary           x, dy in {-1, 0, 1}: |product| <= 1, so any number of positions below 2^24 is exact (the largest case
                    here sums 65 520).  Sees every dropped, doubled or misplaced position, frame, tile, share and slab;
                    cannot see a fault in the value bits.
  full significand  x, dy integers in [-127, 127]: exact in bf16, all 8 significand bits in use, so dropped or misrouted
                    mantissa bits in the transposed LDS reads show.  Only for cases of at most 1000 positions
                    (1000 * 127^2 < 2^24).

Data gradient: dy ternary, w ternary with about bn_ref.CONV_NONZERO non-zeros per output element (as bn_ref.conv_inputs),
the accumulate run pre-fills dx with integers in [-8, 8]; a bf16 dx holds |v| <= 256 exactly.

Case inputs are cached as int8 (the float64 copies of the large cases would hold hundreds of MB); references as float64."""
import functools

import torch

from bn_ref import CONV_NONZERO

LIMIT = 2.0 ** 24
FULL_MAX_POSITIONS = 1000     # 1000 * 127^2 = 16 129 000 < 2^24
PREFILL = 8                   # |prefill| of the accumulate runs
BF16_EXACT = 256.0            # bf16 holds every integer up to here

BOTH = ('fp32', 'bf16')
BF = ('bf16',)


# ----------------------------------------------------------------------------------------------- references
def window(x, t_off, T):
    """Frames [t_off, t_off + T) of x [B, C, t_alloc, H, W]; frames outside the buffer are zero frames."""
    B, C, t_alloc, H, W = x.shape
    win = torch.zeros(B, C, T, H, W, dtype=torch.float64)
    for t in range(T):
        if 0 <= t_off + t < t_alloc:
            win[:, :, t] = x[:, :, t_off + t]
    return win


def wgrad_ref(x_windows, dys, kt, taps):
    """dW[n][c][dt][kh][kw] = sum_{b,t,h,w} dy[b,n,t,h,w] * x[b,c,t+dt,h+kh-1,w+kw-1] (1x1: no spatial shift), summed over
    the levels: one float64 matmul per level, dt and spatial tap.  x_windows: per level [B, cin, T, H, W] (the frame window,
    zero frames already in place); dys: per level [B, cout, T - kt + 1, H, W]."""
    k = 3 if taps == 9 else 1
    pad = k // 2
    cin, cout = x_windows[0].shape[1], dys[0].shape[1]
    dw = torch.zeros(cout, cin, kt, k, k, dtype=torch.float64)
    for x, dy in zip(x_windows, dys):
        B, _, T, H, W = x.shape
        t_out = T - kt + 1
        assert dy.shape == (B, cout, t_out, H, W)
        xp = torch.zeros(B, T, H + 2 * pad, W + 2 * pad, cin, dtype=torch.float64)     # channels last: cheap shifted views
        xp[:, :, pad:pad + H, pad:pad + W] = x.double().permute(0, 2, 3, 4, 1)
        a = dy.double().permute(1, 0, 2, 3, 4).reshape(cout, -1)                          # [n, positions]
        for dt in range(kt):
            for kh in range(k):
                for kw in range(k):
                    b = xp[:, dt:dt + t_out, kh:kh + H, kw:kw + W].reshape(-1, cin)       # [positions, c]
                    dw[:, :, dt, kh, kw] += a @ b
    return dw


def dgrad_ref(dys, w, kt, taps):
    """The float64 transposed conv: dx[b,c,t+dt,h+kh-1,w+kw-1] += sum_n dy[b,n,t,h,w] * w[n,c,dt,kh,kw]; per level
    [B, cin, t_out + kt - 1, H, W]."""
    k = 3 if taps == 9 else 1
    pad = k // 2
    cout, cin = w.shape[0], w.shape[1]
    w = w.double()
    out = []
    for dy in dys:
        B, _, t_out, H, W = dy.shape
        a = dy.double().permute(0, 2, 3, 4, 1).reshape(-1, cout)                          # [positions, n]
        dxp = torch.zeros(B, t_out + kt - 1, H + 2 * pad, W + 2 * pad, cin, dtype=torch.float64)
        for dt in range(kt):
            for kh in range(k):
                for kw in range(k):
                    dxp[:, dt:dt + t_out, kh:kh + H, kw:kw + W] += (a @ w[:, :, dt, kh, kw]).reshape(B, t_out, H, W, cin)
        out.append(dxp[:, :, pad:pad + H, pad:pad + W].permute(0, 4, 1, 2, 3).contiguous())
    return out


def integers_ok(ref, mag, limit=LIMIT):
    """The precondition of check_exact on a float64 reference and its magnitude (the same sum on absolute values):
    integer-valued, every per-element sum of |products| below 2^24."""
    return bool((ref == ref.round()).all()) and float(mag.max()) < limit


# ----------------------------------------------------------------------------------------------- weight-gradient cases
LV_SMALL = [(6, 10), (3, 4)]         # 72 positions per frame: the full-significand cases
LV_RAGGED = [(9, 17), (5, 40)]       # no multiple of any tile height / width

# name -> (B, T, t_alloc, t_off, shapes, cin, cout, kt, taps, precisions, generator, flags)
# flags: 'several' = more tiles than split-K workgroups (test_conv_bwd_ref_cpu.py asserts tiles / split >= 2 with the
# planner's own numbers), 'grouped' = x in the channel-group-major layout, 'random' = the one random-operand case.
WGRAD_CASES = {
    # ---- wgrad.hip, every workgroup sweeps several tiles (x ring across tile and level boundaries)
    'cfg0 several':         (1, 13, 13, 0, [(48, 84), (12, 21)], 256, 32, 11, 9, BOTH, 'ternary', ('several',)),
    'cfg0 fpr1 several':    (1, 14, 14, 0, [(48, 84), (12, 21)], 256, 32, 11, 9, BOTH, 'ternary', ('several',)),   # t_out 4: frame pairs, 6-row tiles
    'cfg1 several':         (2, 3, 3, 0, [(40, 50), (12, 21)], 256, 192, 2, 9, BOTH, 'ternary', ('several',)),
    'cfg1 fpr1 several':    (1, 5, 5, 0, [(48, 84), (5, 9)], 256, 192, 2, 9, BOTH, 'ternary', ('several',)),       # t_out 4
    'cfg2 several':         (2, 12, 12, 0, [(96, 168), (12, 21)], 32, 32, 11, 9, BOTH, 'ternary', ('several',)),   # bf16 KS 2; f32 two dt groups
    '1x1 several':          (1, 23, 23, 0, [(96, 136), (5, 9)], 32, 64, 20, 1, BOTH, 'ternary', ('several',)),     # t_out 4 > 3: generic 1x1
    'cfg4 several':         (1, 12, 12, 0, [(68, 256)], 32, 64, 12, 9, BF, 'ternary', ('several',)),               # c_out 64: wgrad_t1 declines
    # ---- wgrad.hip, the remaining instances and edges
    'cfg0 fpr2 odd t_out':  (1, 4, 4, 0, LV_RAGGED, 256, 32, 2, 9, BOTH, 'ternary', ()),                           # t_out 3
    'cfg1 fpr2 t_out 2':    (1, 3, 3, 0, LV_RAGGED, 256, 192, 2, 9, BOTH, 'ternary', ()),
    'ragged c and n tiles': (1, 3, 3, 0, LV_RAGGED, 96, 224, 2, 9, BOTH, 'ternary', ()),                           # NTC = NTN = 2
    '1x1 idle n tile':      (1, 4, 4, 0, [(9, 17), (3, 3)], 64, 32, 2, 1, BOTH, 'ternary', ()),                    # c_out 32 under NTN = 2
    '1x1 t_offset -1':      (1, 5, 4, -1, LV_RAGGED, 32, 64, 3, 1, BOTH, 'ternary', ()),                           # lateral_wgrad declines
    '1x1 beyond the end':   (1, 5, 4, 1, LV_RAGGED, 32, 64, 3, 1, BOTH, 'ternary', ()),
    'cfg4 window beyond':   (1, 4, 3, -1, [(40, 50)], 32, 32, 4, 9, BF, 'ternary', ()),                            # wgrad_t1 declines
    'cfg2 tall and short':  (1, 4, 4, 0, [(21, 19), (5, 33)], 32, 32, 3, 9, BOTH, 'ternary', ()),                  # t_out 2; > 16 rows, < 8 rows
    'cfg0 grouped':         (1, 5, 6, 1, [(9, 17), (5, 8)], 256, 32, 2, 9, BF, 'ternary', ('grouped',)),           # t_out 4: frame pairs
    'cfg1 grouped':         (2, 3, 4, 1, [(9, 17), (3, 3)], 256, 192, 2, 9, BF, 'ternary', ('grouped',)),
    'tiny levels':          (2, 3, 3, 0, [(1, 1), (1, 2)], 64, 32, 2, 9, BOTH, 'ternary', ()),
    # ---- lateral_wgrad.hip (bf16, 32 -> 64, 1x1, t_out <= 3)
    'lat kt1 t1':           (1, 1, 1, 0, [(7, 9)], 32, 64, 1, 1, BF, 'ternary', ()),
    'lat kt5 t3':           (1, 7, 7, 0, [(13, 17)], 32, 64, 5, 1, BF, 'ternary', ()),
    'lat kt11 t2':          (1, 12, 12, 0, [(9, 13), (5, 9)], 32, 64, 11, 1, BF, 'ternary', ()),
    'lat kt15 t2':          (1, 16, 16, 0, [(5, 21)], 32, 64, 15, 1, BF, 'ternary', ()),                           # the last one-group kt
    'lat kt16 t3':          (1, 18, 18, 0, [(5, 21)], 32, 64, 16, 1, BF, 'ternary', ()),                           # the first two-group kt
    'lat kt20 t3 many':     (1, 22, 22, 0, [(48, 84), (5, 9)], 32, 64, 20, 1, BF, 'ternary', ()),                  # 8 tiles per share
    'lat kt20 t1 one tile': (1, 20, 20, 0, [(3, 5)], 32, 64, 20, 1, BF, 'ternary', ()),                            # fewer tiles than workgroups
    'lat kt41 t3':          (1, 43, 43, 0, [(7, 9), (5, 9)], 32, 64, 41, 1, BF, 'ternary', ()),
    'lat kt48 t1 window':   (2, 48, 50, 1, [(3, 11)], 32, 64, 48, 1, BF, 'ternary', ()),                           # two clips, window in a longer buffer
    'lat two clips ragged': (2, 6, 9, 2, [(5, 21), (2, 3), (1, 1)], 32, 64, 4, 1, BF, 'ternary', ()),
    # ---- wgrad_t1.hip (bf16, 32 -> 32, 3x3, one output frame)
    't1 kt2 window':        (2, 2, 5, 2, [(17, 33), (5, 3), (1, 1)], 32, 32, 2, 9, BF, 'ternary', ()),             # ragged edges, a level below a tile
    't1 kt12 several':      (1, 12, 12, 0, [(48, 84), (12, 21)], 32, 32, 12, 9, BF, 'ternary', ()),                # 4 tiles per share
    't1 kt22':              (1, 22, 22, 0, [(20, 19), (5, 3)], 32, 32, 22, 9, BF, 'ternary', ()),
    # ---- full significand, at most 1000 positions: one per kernel file and MFMA form
    'full 32x32x16 cfg4':   (1, 3, 3, 0, LV_SMALL, 32, 64, 3, 9, BF, 'full', ()),
    'full 32x32x16 1x1':    (1, 6, 6, 0, LV_SMALL, 32, 64, 3, 1, BOTH, 'full', ()),                                # t_out 4; fp32: 32x32x2
    'full frame pairs':     (1, 5, 5, 0, LV_SMALL, 64, 32, 2, 9, BOTH, 'full', ()),                                # cfg 0, t_out 4; fp32: 32x32x2
    'full row pairs cfg1':  (1, 3, 3, 0, LV_SMALL, 64, 64, 2, 9, BOTH, 'full', ()),                                # t_out 2
    'full row pairs cfg2':  (1, 4, 4, 0, LV_SMALL, 32, 32, 3, 9, BOTH, 'full', ()),                                # KS 2, t_out 2
    'full lateral':         (1, 6, 6, 0, LV_SMALL, 32, 64, 5, 1, BF, 'full', ()),                                  # t_out 2
    'full t1':              (1, 2, 2, 0, LV_SMALL, 32, 32, 2, 9, BF, 'full', ()),
    # ---- random operands (the only place fp32's 24-bit operands are exercised): the derived bound of kernel_util.check
    'random':               (1, 3, 3, 0, LV_SMALL, 64, 64, 2, 9, BOTH, 'random', ('random',)),                     # 144 positions
}


def wgrad_positions(name):
    """Positions one element of dW sums over: batch * t_out * all levels."""
    B, T, _, _, shapes, _, _, kt, _, _, _, _ = WGRAD_CASES[name]
    return B * (T - kt + 1) * sum(h * w for h, w in shapes)


def _seed(name):
    return 1000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _draw(shape, gen, g):
    a = 1 if gen == 'ternary' else 127
    return torch.randint(-a, a + 1, shape, generator=g).to(torch.int8)


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name, prec='fp32'):
    """(xs, dys, ref, mag) of a WGRAD_CASES row: xs per level [B, cin, t_alloc, H, W], dys per level [B, cout, t_out, H, W],
    ref = wgrad_ref on the frame window, mag = the same on absolute values (ternary cases: its upper bound, the number of
    positions).  Integer cases: int8 operands, the same for both
    precisions.  'random': normal operands rounded to `prec`, as float32."""
    B, T, t_alloc, t_off, shapes, cin, cout, kt, taps, _, gen, _ = WGRAD_CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    t_out = T - kt + 1
    if gen == 'random':
        def rnd(t):
            return t.bfloat16().float() if prec == 'bf16' else t
        xs = [rnd(torch.randn(B, cin, t_alloc, H, W, generator=g)) for (H, W) in shapes]
        dys = [rnd(torch.randn(B, cout, t_out, H, W, generator=g)) for (H, W) in shapes]
    else:
        xs = [_draw((B, cin, t_alloc, H, W), gen, g) for (H, W) in shapes]
        dys = [_draw((B, cout, t_out, H, W), gen, g) for (H, W) in shapes]
    wins = [window(x.double(), t_off, T) for x in xs]
    ref = wgrad_ref(wins, [dy.double() for dy in dys], kt, taps)
    if gen == 'ternary':
        # every |product| is 0 or 1: the number of positions bounds the sum (spares the large cases a second reference)
        mag = torch.full_like(ref, float(wgrad_positions(name)))
    else:
        mag = wgrad_ref([w_.abs() for w_ in wins], [dy.double().abs() for dy in dys], kt, taps)
    return xs, dys, ref, mag


@functools.lru_cache(maxsize=None)
def wgrad_prefill(name):
    """Integers in [-PREFILL, PREFILL] for the accumulate run, float64 in grad_w's shape."""
    _, _, _, _, _, cin, cout, kt, taps, _, _, _ = WGRAD_CASES[name]
    k = 3 if taps == 9 else 1
    g = torch.Generator().manual_seed(_seed(name) + 7)
    return torch.randint(-PREFILL, PREFILL + 1, (cout, cin, kt, k, k), generator=g).double()


# ----------------------------------------------------------------------------------------------- data-gradient cases
LV_WAVE = [(1, 1), (3, 3), (7, 9)]   # 1, 9 and 63 positions: below and astride the 32-position wave unit of lateral_dgrad

# name -> (B, T, shapes, cin, cout, kt, taps, precisions) of the FORWARD conv; the data gradient is the conv
# cout -> cin with pad_t = kt - 1 on the t_out = T - kt + 1 frames of dy
DGRAD_CASES = {
    'wide single-frame':   (1, 4, [(12, 21), (5, 9)], 256, 192, 2, 9, BOTH),     # t_out 3: the single-frame-block plan, MT 2 / TH 8
    'wide multi-frame':    (1, 3, [(9, 17), (3, 5)], 256, 256, 1, 9, BOTH),      # kt 1: no padded tap, blocks of 2 + 1 frames kept
    'wide to 32':          (1, 7, [(6, 10), (2, 3)], 256, 32, 3, 9, BOTH),       # forward 256 -> 32, kt 3, t_out 5
    'frame-split multi':   (1, 6, [(10, 19), (4, 5)], 32, 32, 2, 9, BOTH),       # family 3: dx of 6 frames in blocks of 4 + 2
    'fs1s':                (2, 12, [(9, 37), (4, 5)], 32, 32, 12, 9, BOTH),      # 12 frames -> 1: conv3d_fs1s_kernel (bf16)
    'narrow 1x1 t5':       (1, 9, [(9, 16), (3, 5)], 32, 64, 5, 1, BOTH),        # family 0: t_in 5 > 3
    'lat c64 t1 kt5':      (1, 5, LV_WAVE, 32, 64, 5, 1, BF),
    'lat c64 t2 kt20':     (2, 21, LV_WAVE, 32, 64, 20, 1, BF),
    'lat c64 t3 kt41':     (1, 43, LV_WAVE, 32, 64, 41, 1, BF),                  # the register tap
    'lat c64 t1 kt42':     (1, 42, LV_WAVE, 32, 64, 42, 1, BF),                  # weights from L2
    'lat c32 t3 kt5':      (1, 7, LV_WAVE, 32, 32, 5, 1, BF),
    'lat c32 t1 kt20':     (1, 20, LV_WAVE, 32, 32, 20, 1, BF),
    'lat c32 t2 kt41':     (2, 42, LV_WAVE, 32, 32, 41, 1, BF),
    'lat c32 t3 kt42':     (1, 44, LV_WAVE, 32, 32, 42, 1, BF),
    'mask head':           (33, 1, [(7, 7)], 256, 256, 1, 9, BOTH),
}


@functools.lru_cache(maxsize=None)
def dgrad_inputs(name):
    """(dys, w, refs, mags, prefill) of a DGRAD_CASES row: dys per level [B, cout, t_out, H, W] in {-1, 0, 1} (int8), w
    [cout, cin, kt, k, k] in {-1, 0, 1} with about CONV_NONZERO non-zeros per element of dx, refs = dgrad_ref per level
    [B, cin, T, H, W], mags the same on absolute values, prefill per level integers in [-PREFILL, PREFILL]."""
    B, T, shapes, cin, cout, kt, taps, _ = DGRAD_CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    k = 3 if taps == 9 else 1
    t_out = T - kt + 1
    density = min(1.0, CONV_NONZERO / (cout * kt * taps))
    w = torch.randint(0, 2, (cout, cin, kt, k, k), generator=g) * 2 - 1
    w = (w * (torch.rand(w.shape, generator=g) < density)).to(torch.int8)
    dys = [_draw((B, cout, t_out, H, W), 'ternary', g) for (H, W) in shapes]
    refs = dgrad_ref([dy.double() for dy in dys], w.double(), kt, taps)
    mags = dgrad_ref([dy.double().abs() for dy in dys], w.double().abs(), kt, taps)
    pre = [torch.randint(-PREFILL, PREFILL + 1, r.shape, generator=g).double() for r in refs]
    return dys, w, refs, mags, pre
