"""GPU: the roi_heads training-target kernels (csrc/roi_targets.hip) one by one through the C ABI, against
tests/roi_targets_ref.py.  Guard bands and sentinel fills around every output, NaN-filled workspace, two runs compared
with torch.equal; no element is left out.  PARITY UNPINNED BY THE REFERENCE.

match.  On quarter-pixel boxes with coordinates below 512 every fp32 subtraction, product and sum of the IoU is exact
(sides below 2^11 quarter pixels, areas below 2^22 sixteenths) and the one division is correctly rounded on both sides;
with dyadic thresholds the fp32 quotient compares with them as the rational does (x >= 2^-k rounds to >= 2^-k, x < 2^-k
rounds to <= 2^-k only if it was at most half an ulp below, which a ratio of integers below 2^23 cannot be).  So
`matched`, `labels` and `max_iou` EQUAL the restatement.  On real-valued boxes max_iou is checked per element against the
float64 IoU of the same fp32 boxes with K = 4 and mag = the IoU: the operands are exact fp32 numbers, so each side, area
and the intersection carry one rounding apiece (relative 2^-24 each, 5 in the numerator chain), the union = (area_a +
area_b) - inter two more whose absolute error (area_a + area_b) 2^-24 is at most twice that relative to the union (inter
<= min area), and the division one: about 11 x 2^-24 of the IoU against the criterion's 2 (4 + 1) 2^-22 = 40 x 2^-24.
The decisions are then checked against the restatement's rule applied to the kernel's OWN max_iou, and the float64 IoU
of the matched box must lie within that allowance of the float64 maximum.

sample.  No arithmetic but the regression targets: everything equals the restatement's stable sort; regression_targets
per element under the allowance tests/test_gpu_boxhead_kernels.py uses for sfvos_box_encode.

mask_targets.  Per element against float64 on the restatement's fp32 geometry (tests/roi_targets_ref.py says why) with
K = 4 grid_h grid_w (the additions one product passes through) and mag = the target itself: every term is >= 0, and an
interpolation weight 1 - l is exact for l >= 1/2 and within 2^-24 of itself below, so no term loses relative accuracy."""
import itertools

import pytest
import torch

import roi_targets_ref as T
from kernel_util import SENT, TRANS, U22, Out, P, S, check, check_abs, lib  # noqa: F401
from test_box_branch_cpu import quarter_pixel_boxes

pytestmark = pytest.mark.gpu
ISENT = int(SENT)


# ---- match ------------------------------------------------------------------------------------------------------------

def run_match(lib, props, gt, gl, high, low, want_iou=True):
    n_p, G = props.shape[0], gt.shape[0]
    N = n_p + G
    pd, gd, ld = props.float().cuda(), gt.float().cuda(), gl.to(torch.int64).cuda()
    outs = []
    for _ in range(2):
        matched, labels, iou = Out((max(N, 1),), torch.int32), Out((max(N, 1),), torch.int64), Out((max(N, 1),))
        lib.call('sfvos_roi_match', P(pd) if n_p else None, n_p, P(gd) if G else None, P(ld) if G else None, G, high, low,
                 P(matched.t), P(labels.t), P(iou.t) if want_iou else None, S())
        torch.cuda.synchronize()
        outs.append((matched.cpu()[:N], labels.cpu()[:N], iou.cpu()[:N]))
        if not want_iou:
            assert bool((outs[-1][2] == SENT).all())
    for a, b in zip(*outs):
        assert torch.equal(a, b), 'two runs differ'
    return outs[0]


def exact_inputs(n_p, G, seed):
    """Ground truth on the quarter-pixel grid; proposals = ground-truth boxes moved and resized by quarter pixels (IoU from
    0 to 1 around the thresholds) and a fifth of unrelated boxes."""
    gt = quarter_pixel_boxes(G, seed, 120).float()
    g = torch.Generator().manual_seed(1000 + seed)
    props = quarter_pixel_boxes(n_p, seed + 1, 120).float()
    if G:
        src = gt[torch.randint(0, G, (n_p,), generator=g)]
        jit = torch.randint(-60, 61, (n_p, 4), generator=g).float() / 4
        near = src + jit
        near = torch.cat([torch.minimum(near[:, :2], near[:, 2:] - 0.25), near[:, 2:]], 1).clamp(0, 500)
        keep = torch.rand(n_p, generator=g) < 0.2
        props = torch.where(keep[:, None], props, near)
    labels = torch.randint(1, 8, (G,), generator=g)
    return props, gt, labels


MATCH_CASES = [(N, G) for N, G in itertools.product([1, 63, 64, 65, 300], [0, 1, 3, 65]) if G <= N]


@pytest.mark.parametrize('N,G', MATCH_CASES)
def test_match_is_exact_on_quarter_pixel_boxes(lib, N, G):
    props, gt, gl = exact_inputs(N - G, G, 7 * N + G)
    seen = set()
    for high, low in ((0.5, 0.5), (0.5, 0.25), (0.75, 0.125)):
        matched, labels, iou = run_match(lib, props, gt, gl, high, low)
        want = T.match(props, gt, gl, high, low)
        assert torch.equal(iou, want['max_iou']), (N, G, high, low)
        assert torch.equal(matched.long(), want['matched']) and torch.equal(labels, want['labels']), (N, G, high, low)
        seen |= set(labels.tolist())
        if G:      # the ground-truth rows match themselves (or an identical box in front of them) with IoU 1
            assert bool((iou[N - G:] == 1.0).all()) and bool((labels[N - G:] >= 1).all())
            assert torch.equal(gt[matched[N - G:].long()], gt)
    if N - G >= 50 and G:
        assert -1 in seen and 0 in seen, 'the inputs must reach every outcome'
    run_match(lib, props, gt, gl, 0.5, 0.5, want_iou=False)      # max_iou may be NULL


def test_match_ties_thresholds_and_degenerate_boxes(lib):
    gt = torch.tensor([[0., 0., 8., 8.], [8., 0., 16., 8.], [0., 0., 8., 8.], [100., 100., 101., 101.]])
    gl = torch.tensor([3, 5, 6, 7])
    props = torch.tensor([[0., 0., 8., 4.],       # IoU exactly 0.5 with boxes 0 and 2: positive, the lower index
                          [4., 0., 12., 8.],      # 1/3 with boxes 0, 1 and 2
                          [0., 0., 8., 3.],       # 0.375
                          [50., 50., 50., 60.],   # zero area
                          [40., 40., 41., 41.],   # touches nothing
                          [8., 0., 16., 8.]])     # box 1 itself
    matched, labels, iou = run_match(lib, props, gt, gl, 0.5, 0.5)
    assert matched.tolist() == [0, 0, 0, 0, 0, 1, 0, 1, 0, 3] and labels.tolist() == [3, 0, 0, 0, 0, 5, 3, 5, 3, 7]
    assert iou.tolist()[:6] == [0.5, float(torch.tensor(1.0) / 3), 0.375, 0.0, 0.0, 1.0]
    matched, labels, _ = run_match(lib, props, gt, gl, 0.5, 0.3)
    assert labels.tolist() == [3, -1, -1, 0, 0, 5, 3, 5, 3, 7] and matched.tolist() == [0, 0, 0, 0, 0, 1, 0, 1, 0, 3]
    want = T.match(props, gt, gl, 0.5, 0.3)
    assert torch.equal(matched.long(), want['matched']) and torch.equal(labels, want['labels'])
    # no ground truth: background everywhere
    matched, labels, iou = run_match(lib, props, gt[:0], gl[:0], 0.5, 0.5)
    assert matched.tolist() == [0] * 6 and labels.tolist() == [0] * 6 and iou.tolist() == [0.0] * 6


@pytest.mark.parametrize('N,G', [(300, 3), (1500, 65)])
def test_match_on_real_valued_boxes(lib, N, G):
    g = torch.Generator().manual_seed(N)
    gt = quarter_pixel_boxes(G, N, 200).float() + torch.rand(G, 4, generator=g) * 0.2
    src = gt[torch.randint(0, G, (N - G,), generator=g)]
    scale = (src[:, 2:] - src[:, :2]).repeat(1, 2)
    props = src + torch.randn(N - G, 4, generator=g) * 0.3 * scale
    props = torch.cat([torch.minimum(props[:, :2], props[:, 2:] - 1), props[:, 2:]], 1)
    gl = torch.randint(1, 8, (G,), generator=g)
    high, low = 0.5, 0.3
    matched, labels, iou = run_match(lib, props, gt, gl, high, low)
    ref = T.match(props, gt, gl, high, low)
    best64 = ref['iou64'].max(1).values
    check('roi_match max_iou N %d G %d' % (N, G), iou, best64, best64, 4, 0.0)
    own_matched, own_labels = T.decide(iou, matched.long(), gl, high, low)
    assert torch.equal(labels, own_labels) and torch.equal(matched.long(), own_matched)
    hit = iou >= high
    assert 0.1 * N < int(hit.sum()) < 0.9 * N and int((labels == -1).sum()) > 0
    allow = 2.0 * (4 + 1) * U22 * best64
    got64 = ref['iou64'][torch.arange(N), matched.long()]
    assert bool((got64[hit] >= (best64 - allow)[hit]).all())
    print('   %d matched, %d ignored, %d background; %d decisions differ from the fp32 restatement'
          % (int(hit.sum()), int((labels == -1).sum()), int((labels == 0).sum()), int((labels != ref['labels']).sum())))


# ---- sample -----------------------------------------------------------------------------------------------------------

def run_sample(lib, labels, matched, keys, props, gt, batch, fraction):
    """-> (S, P, index, boxes, labels, matched, targets, pos_slot) on the cpu, whole padded rows."""
    n_p, G = props.shape[0], gt.shape[0]
    N = n_p + G
    ld, md, kd = labels.to(torch.int64).cuda(), matched.to(torch.int32).cuda(), keys.float().cuda()
    pd, gd = props.float().cuda(), gt.float().cuda()
    nbytes = lib.load().sfvos_roi_sample_workspace_bytes(N)
    assert nbytes >= 4 * N
    runs = []
    for _ in range(2):
        ws = Out((nbytes // 4,), torch.float32, fill=float('nan'))
        cnt = Out((2,), torch.int32)
        outs = [Out((batch,), torch.int32), Out((batch, 4)), Out((batch,), torch.int64), Out((batch,), torch.int32),
                Out((batch, 4)), Out((batch,), torch.int32)]
        lib.call('sfvos_roi_sample', P(ld), P(md), P(kd), P(pd) if n_p else None, n_p, P(gd) if G else None, G, batch,
                 fraction, 10.0, 10.0, 5.0, 5.0, P(ws.t), P(cnt.t), *([P(o.t) for o in outs] + [S()]))
        torch.cuda.synchronize()
        assert ws.guards_ok(), 'wrote outside the workspace'
        runs.append([cnt.cpu()] + [o.cpu() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a, b), 'two runs differ'
    cnt = runs[0][0]
    return (int(cnt[0]), int(cnt[1])) + tuple(runs[0][1:])


def check_sample(lib, labels, keys, batch, fraction, seed, tag):
    N = labels.numel()
    G = min(3, N)
    n_p = N - G
    g = torch.Generator().manual_seed(seed)
    gt = quarter_pixel_boxes(G, seed, 100).float()
    props = quarter_pixel_boxes(n_p, seed + 1, 100).float() + torch.rand(n_p, 4, generator=g) * 0.2
    matched = torch.randint(0, G, (N,), generator=g)
    Sg, Pg, index, boxes, olab, omat, targets, pos_slot = run_sample(lib, labels, matched, keys, props, gt, batch, fraction)
    want_index, want_pos = T.sample(labels, keys, batch, fraction)
    Sw, Pw = want_index.numel(), want_pos.numel()
    assert (Sg, Pg) == (Sw, Pw), (tag, Sg, Pg, Sw, Pw)
    assert torch.equal(index[:Sw].long(), want_index), tag
    assert torch.equal(pos_slot[:Pw].long(), want_pos), tag
    cand = torch.cat([props, gt], 0)
    assert torch.equal(boxes[:Sw], cand[want_index]) and torch.equal(olab[:Sw], labels[want_index]), tag
    assert torch.equal(omat[:Sw].long(), matched[want_index]), tag
    # rows behind the counts: -1 in index, untouched everywhere else
    assert bool((index[Sw:] == -1).all()) and bool((boxes[Sw:] == SENT).all()) and bool((targets[Sw:] == SENT).all())
    assert bool((olab[Sw:] == ISENT).all()) and bool((omat[Sw:] == ISENT).all()) and bool((pos_slot[Pw:] == ISENT).all())
    if Sw:
        r, p = gt[matched[want_index]].double(), cand[want_index].double()
        want = T.encode(r, p)
        pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
        gcx, gcy = (r[:, 0] + r[:, 2]).abs() / 2, (r[:, 1] + r[:, 3]).abs() / 2
        pcx, pcy = (p[:, 0] + p[:, 2]).abs() / 2, (p[:, 1] + p[:, 3]).abs() / 2
        allow = TRANS * torch.stack([10 * (gcx + pcx) / pw, 10 * (gcy + pcy) / ph, 5 * (want[:, 2].abs() / 5 + 1),
                                     5 * (want[:, 3].abs() / 5 + 1)], 1)
        check_abs('roi_sample targets %s' % tag, targets[:Sw], want, allow)
    return Sw, Pw


def random_labels(N, seed, p_pos=0.3, p_ign=0.1):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(N, generator=g)
    lab = torch.where(u < p_pos, torch.randint(1, 8, (N,), generator=g), torch.zeros(N, dtype=torch.int64))
    return torch.where(u > 1 - p_ign, -torch.ones(N, dtype=torch.int64), lab)


@pytest.mark.parametrize('N', [1, 5, 64, 65, 700, 2003])
def test_sample_sizes(lib, N):
    labels = random_labels(N, N)
    g = torch.Generator().manual_seed(N + 1)
    keys = torch.rand(N, generator=g)
    for batch, fraction in ((8, 0.25), (512, 0.25), (64, 0.0), (64, 1.0), (4096, 0.5)):
        check_sample(lib, labels, keys, batch, fraction, N, 'N %d batch %d fraction %g' % (N, batch, fraction))


def fixed_labels(n_pos, n_neg, n_ign, seed):
    lab = torch.cat([torch.randint(1, 8, (n_pos,), generator=torch.Generator().manual_seed(seed)),
                     torch.zeros(n_neg, dtype=torch.int64), -torch.ones(n_ign, dtype=torch.int64)])
    return lab[torch.randperm(lab.numel(), generator=torch.Generator().manual_seed(seed + 1))]


REGIMES = {'positives under the quota': ((40, 600, 60), (512, 40)), 'positives over the quota': ((300, 1650, 53), (512, 128)),
           'too few negatives': ((30, 100, 570), (130, 30)), 'no positives': ((0, 690, 10), (512, 0)),
           'no negatives': ((200, 0, 500), (128, 128)), 'every label -1': ((0, 0, 65), (0, 0))}


@pytest.mark.parametrize('regime', sorted(REGIMES))
def test_sample_regimes(lib, regime):
    (n_pos, n_neg, n_ign), want = REGIMES[regime]
    labels = fixed_labels(n_pos, n_neg, n_ign, 5)
    keys = torch.rand(labels.numel(), generator=torch.Generator().manual_seed(6))
    assert check_sample(lib, labels, keys, 512, 0.25, 9, regime) == want


@pytest.mark.parametrize('kind', ['all equal', 'duplicated', 'nan', 'signed zeros and infinities'])
def test_sample_key_order(lib, kind):
    N = 700
    labels = random_labels(N, 3)
    g = torch.Generator().manual_seed(4)
    keys = {'all equal': torch.full((N,), 0.5), 'duplicated': torch.randint(0, 4, (N,), generator=g).float() / 4,
            'nan': torch.rand(N, generator=g), 'signed zeros and infinities': torch.rand(N, generator=g) - 0.5}[kind]
    if kind == 'nan':
        pos = torch.where(labels >= 1)[0]
        keys[pos[:3]] = float('nan')          # behind every number: chosen only when the quota takes every positive
        keys[torch.where(labels == 0)[0][0]] = float('nan')
    if kind.startswith('signed'):
        keys[::7] = 0.0
        keys[3::7] = -0.0
        keys[5::50] = float('inf')
        keys[6::50] = float('-inf')
    for batch, fraction in ((64, 0.25), (512, 0.25), (1024, 0.5)):
        check_sample(lib, labels, keys, batch, fraction, 2, '%s batch %d' % (kind, batch))


# ---- mask targets -----------------------------------------------------------------------------------------------------

def special_boxes(H, W):
    return torch.tensor([[5.0, 4.0, 33.0, 32.0],                  # integer-aligned side of 28
                         [2.0, 1.0, 59.0, 58.0],                  # side of 57: grid 3 at M = 28, ragged
                         [10.25, 7.5, 10.75, 7.875],              # sub-pixel: sides clamped to 1
                         [-6.5, 5.0, 12.0, 20.0],                 # out of the left border
                         [8.0, -9.25, 30.0, 11.0],                # the top
                         [W - 15.5, 6.0, W + 9.0, 25.0],          # the right
                         [4.0, H - 11.0, 29.0, H + 13.5],         # the bottom
                         [W + 3.0, H + 2.0, W + 40.0, H + 30.0],  # wholly outside
                         [0.0, 0.0, float(W), float(H)]])         # the full image: unequal grids per axis


def run_mask_targets(lib, masks, boxes, matched, M):
    G, H, W = masks.shape
    Pn = boxes.shape[0]
    md, bd, xd = masks.contiguous().cuda(), boxes.float().cuda(), matched.to(torch.int32).cuda()
    outs = []
    for _ in range(2):
        out = Out((Pn, M, M))
        lib.call('sfvos_mask_targets', P(md), int(masks.dtype == torch.uint8), G, H, W, P(bd), P(xd), Pn, M, P(out.t), S())
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]), 'two runs differ'
    return outs[0]


@pytest.mark.parametrize('M,shape,Pn', list(itertools.product([28, 4], [(37, 53), (97, 131)], [1, 9, 130])))
def test_mask_targets(lib, M, shape, Pn):
    H, W = shape
    g = torch.Generator().manual_seed(H + Pn + M)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    masks = torch.stack([((yy - H * 0.5) ** 2 / (H * 0.35) ** 2 + (xx - W * 0.45) ** 2 / (W * 0.3) ** 2 < 1),   # a blob
                         torch.rand(H, W, generator=g) > 0.5,                                                    # salt and pepper
                         (xx + 2 * yy) % 9 < 4]).to(torch.uint8)                                                 # stripes
    sp = special_boxes(H, W)
    if Pn == 1:
        boxes = sp[1:2]
    else:
        c = torch.rand(Pn - 9, 2, generator=g) * torch.tensor([W, H], dtype=torch.float32)
        s = 0.3 + torch.rand(Pn - 9, 2, generator=g) * torch.tensor([W * 0.9, H * 0.9])
        boxes = torch.cat([sp, torch.cat([c - s / 2, c + s / 2], 1)], 0)
    matched = torch.arange(Pn) % 3
    got = run_mask_targets(lib, masks, boxes, matched, M)
    ref, grids = T.roi_align_adaptive(masks, boxes, matched, M)
    K = (4 * grids[:, 0] * grids[:, 1]).double()[:, None, None]
    check_abs('mask_targets M %d %dx%d P %d' % (M, H, W, Pn), got, ref, 2.0 * (K + 1) * U22 * ref)
    assert torch.equal(run_mask_targets(lib, masks.float(), boxes, matched, M), got), 'uint8 and fp32 masks differ'
    assert float(run_mask_targets(lib, torch.zeros_like(masks), boxes, matched, M).abs().max()) == 0.0
    if Pn >= 9:
        assert float(got[7].abs().max()) == 0.0 and float(ref[7].abs().max()) == 0.0     # wholly outside
        assert (grids[8, 0] != grids[8, 1] or (H, W, M) == (37, 53, 28)) and float(got[:7].max()) > 0
        if M == 28:
            assert grids[0].tolist() == [1, 1] and grids[1].tolist() == [3, 3] and grids[2].tolist() == [1, 1]
        # a match outside [0, G): zeros, nothing read
        bad = matched.clone()
        bad[0], bad[1] = -1, 3
        got_bad = run_mask_targets(lib, masks, boxes, bad, M)
        assert float(got_bad[:2].abs().max()) == 0.0 and torch.equal(got_bad[2:], got[2:])


def test_mask_targets_without_boxes_is_a_no_op(lib):
    out = Out((4,))
    lib.call('sfvos_mask_targets', None, 1, 0, 8, 8, None, None, 0, 28, None, S())
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENT).all())
