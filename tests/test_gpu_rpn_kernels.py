"""GPU: the region-proposal kernels (csrc/rpn.hip) one by one through the C ABI.

select: compared for equality with the restatement's stable descending sort (tests/rpn_ref.py: ties by index, -0 == +0,
NaN last) of the same fp32 values.  decode: boxes per element against the float64 formula under the allowance
test_gpu_boxhead_kernels.py uses for box_decode (2^-20 on the magnitudes of the terms, weights 1), scores under
kernel_util's transcendental allowance.  NMS + merge: compared for equality with the restatement's index list on
quarter-pixel boxes (areas, intersections and unions exact in fp32; IEEE division on both sides, so the restatement runs
in fp32 where the threshold is 0.7 and in either precision where it is dyadic).  Guard bands and sentinel fills around
every output, NaN-filled workspace; no element is left out.  PARITY UNPINNED BY THE REFERENCE."""
import ctypes

import pytest
import torch

import rpn_ref as R
from test_box_branch_cpu import quarter_pixel_boxes
from kernel_util import TRANS, Out, P, S, check_abs, lib  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- select ------------------------------------------------------------------------------------------------------------

def run_select(lib, levels, shapes, A, k):
    """levels: list of [B, H W A] fp32 cpu -> (counts [L B], index [L B, k]) cpu."""
    B = levels[0].shape[0]
    flat = torch.cat([v.reshape(-1) for v in levels]).cuda()
    pyr = lib.make_pyramid(shapes)
    S_ = len(shapes) * B
    counts, index = Out((S_,), torch.int32), Out((S_, k), torch.int32)
    lib.call('sfvos_rpn_select', P(flat), ctypes.byref(pyr), B, A, k, P(counts.t), P(index.t), S())
    torch.cuda.synchronize()
    return counts.cpu(), index.cpu()


def check_select(lib, levels, shapes, A, k, tag):
    B = levels[0].shape[0]
    counts, index = run_select(lib, levels, shapes, A, k)
    for l, v in enumerate(levels):
        for b in range(B):
            s = l * B + b
            want = R.select(v[b], k)
            assert int(counts[s]) == want.numel(), (tag, s, int(counts[s]), want.numel())
            got = index[s, :want.numel()].to(torch.int64)
            if not torch.equal(got, want):
                bad = int((got != want).nonzero()[0])
                raise AssertionError('%s segment %d: rank %d is anchor %d (%r), want %d (%r)' % (
                    tag, s, bad, int(got[bad]), float(v[b][got[bad]]) if 0 <= got[bad] < v[b].numel() else None,
                    int(want[bad]), float(v[b][want[bad]])))
            assert bool((index[s, want.numel():] == -1).all()), tag
    return counts, index


def test_select_small_levels_k_above_n(lib):
    """B = 2, A = 3, levels 1x1, 2x3, 5x7 at k = 1000: everything, sorted."""
    g = torch.Generator().manual_seed(1)
    shapes = [(1, 1), (2, 3), (5, 7)]
    levels = [torch.randn(2, h * w * 3, generator=g) for h, w in shapes]
    check_select(lib, levels, shapes, 3, 1000, 'small')


@pytest.mark.parametrize('k', [5, 6, 7])
def test_select_six_anchors(lib, k):
    v = torch.tensor([[0.5, -1.0, 2.0, 0.5, 3.0, -1.0], [1.0, 1.0, 1.0, 0.0, 2.0, 1.0]])
    check_select(lib, [v], [(1, 2)], 3, k, 'six k=%d' % k)


BIG = (150, 160)    # 72 000 values per image: more than 2^16


@pytest.mark.parametrize('k', [1000, 2000])
@pytest.mark.parametrize('case', ['normal', 'eighths', 'equal'])
def test_select_large_level(lib, case, k):
    g = torch.Generator().manual_seed(2)
    n = BIG[0] * BIG[1] * 3
    v = torch.randn(2, n, generator=g)
    if case == 'eighths':      # the k-th place falls inside a tie group
        v = (v * 8).round() / 8
    elif case == 'equal':
        v = torch.full((2, n), -0.375)
        v[1, 5::7] = 1.0        # image 1: 10 286 ones in front of the ties
    check_select(lib, [v], [BIG], 3, k, '%s k=%d' % (case, k))


def test_select_special_values_and_rerun(lib):
    """+0, -0, denormals, +-inf and NaNs: values compare as floats, NaN ranks below every number."""
    g = torch.Generator().manual_seed(3)
    n = 30 * 45 * 3           # 4050: k = n stays inside the limit of 4096
    v = torch.randn(2, n, generator=g)
    v[:, 100:160] = 0.0
    v[:, 130:190:2] = -0.0
    v[:, 200:210] = torch.tensor([1e-40, -1e-40, 1e-45, -1e-45, 3e-39, -3e-39, 1e-38, -1e-38, 2e-44, -2e-44])
    v[:, 300], v[:, 17], v[:, 3900] = float('inf'), float('inf'), float('-inf')
    v[:, 50:60] = float('nan')
    v[1, 3000:3003] = -float('nan')
    v[1] = torch.where(torch.rand(n, generator=g) < 0.5, v[1], -v[1].abs())
    small = torch.tensor([[float('nan'), 0.0, -0.0, float('-inf'), float('nan'), -1e-45],
                          [float('-inf'), float('nan'), float('inf'), -0.0, 0.0, float('nan')]])
    for k in (4050, 4045, 3000, 64):      # k = n, k inside the NaN / -inf tail, inside the body
        a = check_select(lib, [v, small], [(30, 45), (1, 2)], 3, k, 'special k=%d' % k)
        b = run_select(lib, [v, small], [(30, 45), (1, 2)], 3, k)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    big = torch.randn(1, BIG[0] * BIG[1] * 3, generator=g)
    a, b = run_select(lib, [big], [BIG], 3, 2000), run_select(lib, [big], [BIG], 3, 2000)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- decode ------------------------------------------------------------------------------------------------------------

def test_decode_against_float64(lib):
    shapes, tensor, images, A, B, k = [(5, 7), (3, 4)], (64, 96), [(60, 90), (64, 96)], 3, 2, 70
    sizes, ratios = ((32,), (64,)), ((0.5, 1.0, 2.0),) * 2
    g = torch.Generator().manual_seed(4)
    n = [h * w * A for h, w in shapes]
    logits = [torch.randn(B, m, generator=g) * 3 for m in n]
    deltas = [torch.randn(B, m, 4, generator=g) * torch.tensor([0.3, 0.3, 0.4, 0.4]) for m in n]
    counts = torch.tensor([70, 64, 36, 30], dtype=torch.int32)          # s = l B + b
    index = torch.full((4, k), -1, dtype=torch.int32)
    for s in range(4):
        m = n[s // B]
        perm = torch.randperm(m, generator=g)[:int(counts[s])].to(torch.int32)
        perm[0], perm[1] = m - 1, 0                                      # last row and column of the level; the first
        perm[2:] = torch.tensor([i for i in torch.randperm(m, generator=g).tolist() if i not in (0, m - 1)]
                                [:int(counts[s]) - 2], dtype=torch.int32)
        index[s, :int(counts[s])] = perm
    # segment 0: rank 3 dw = 10 (clamped); rank 4 pushed out of the image on the left (width 0: invalid); rank 5
    # logit -200 (score exactly 0: invalid); rank 6 a box over the whole image (crosses all four borders)
    i3, i4, i5, i6 = (int(index[0, r]) for r in (3, 4, 5, 6))
    deltas[0][0, i3] = torch.tensor([0.1, -0.1, 10.0, 0.2])
    deltas[0][0, i4] = torch.tensor([-40.0, 0.0, 0.0, 0.0])
    logits[0][0, i5] = -200.0
    deltas[0][0, i6] = torch.tensor([0.0, 0.0, 4.0, 4.0])
    obj = torch.cat([v.reshape(-1) for v in logits]).cuda()
    dl = torch.cat([v.reshape(-1) for v in deltas]).cuda()
    base = torch.stack(R.base_anchors(sizes, ratios)).cuda()
    imsz = torch.tensor(images, dtype=torch.float32).cuda()
    pyr = lib.make_pyramid(shapes)
    boxes, lg, sc, va = Out((4, k, 4)), Out((4, k)), Out((4, k)), Out((4, k), torch.int32)
    c_d, i_d = counts.cuda(), index.cuda()
    lib.call('sfvos_rpn_decode', P(obj), P(dl), P(c_d), P(i_d), ctypes.byref(pyr), B, A, k, P(base), tensor[0], tensor[1],
             P(imsz), R.BBOX_XFORM_CLIP, 1e-3, 0.0, P(boxes.t), P(lg.t), P(sc.t), P(va.t), S())
    torch.cuda.synchronize()
    boxes, lg, sc, va = boxes.cpu(), lg.cpu(), sc.cpu(), va.cpu()
    anchors = R.grid_anchors(shapes, tensor, sizes, ratios)
    for s in range(4):
        l, b, c = s // B, s % B, int(counts[s])
        idx = index[s, :c].to(torch.int64)
        a, d, z = anchors[l][idx].double(), deltas[l][b][idx].double(), logits[l][b][idx].double()
        want = R.clip_boxes(R.decode(d, a), images[b])
        allow = R.decode_allowance(d, a, TRANS)
        tag = 'rpn_decode segment %d ' % s
        check_abs(tag + 'boxes', boxes[s, :c], want, allow)
        ws_ = torch.sigmoid(z)
        check_abs(tag + 'scores', sc[s, :c], ws_, TRANS * ws_ + 2.0 ** -126)
        assert torch.equal(lg[s, :c].double(), z)
        bx = boxes[s, :c]
        own = ((bx[:, 2] - bx[:, 0]) >= 1e-3) & ((bx[:, 3] - bx[:, 1]) >= 1e-3) & (sc[s, :c] > 0)
        assert torch.equal(va[s, :c].bool(), own), tag
        H, W = images[b]
        assert bool((bx[:, 0::2] >= 0).all()) and bool((bx[:, 0::2] <= W).all()) and bool((bx[:, 1::2] <= H).all())
        # behind the count: zeros, invalid
        assert bool((boxes[s, c:] == 0).all()) and bool((sc[s, c:] == 0).all()) and bool((va[s, c:] == 0).all())
    assert float(boxes[0, 3, 2] - boxes[0, 3, 0]) > 80 and int(va[0, 3]) == 1          # clamped, then clipped
    assert boxes[0, 4, 0] == 0 and boxes[0, 4, 2] == 0 and int(va[0, 4]) == 0          # side below min_size
    assert float(sc[0, 5]) == 0.0 and int(va[0, 5]) == 0                               # sigmoid(-200) is exactly 0
    assert boxes[0, 6].tolist() == [0.0, 0.0, 90.0, 60.0] and int(va[0, 6]) == 1        # all four borders
    assert int(va.sum()) > 150


# ---- NMS + merge ---------------------------------------------------------------------------------------------------------

def run_nms(lib, boxes, logits, valid, counts, L, B, k, thr, post):
    """boxes [L B, k, 4], logits / valid [L B, k], counts [L B] (cpu) -> (count [B], index [B, post], boxes, scores)."""
    nbytes = lib.load().sfvos_rpn_workspace_bytes(L, B, k)
    assert nbytes > 0
    ws = Out((nbytes // 4 + 1,), torch.float32, fill=float('nan'))
    ob, osc, oi, cnt = Out((B, post, 4)), Out((B, post)), Out((B, post), torch.int32), Out((B,), torch.int32)
    bx, lg = boxes.float().cuda(), logits.float().cuda()
    sc = torch.sigmoid(logits.float()).cuda()
    va, cn = valid.to(torch.int32).cuda(), counts.to(torch.int32).cuda()
    lib.call('sfvos_rpn_nms', P(bx), P(lg), P(sc), P(va), P(cn), L, B, k, thr, post, P(ws.t), P(ob.t), P(osc.t), P(oi.t),
             P(cnt.t), S())
    torch.cuda.synchronize()
    assert ws.guards_ok(), 'wrote outside the workspace'
    return cnt.cpu(), oi.cpu(), ob.cpu(), osc.cpu()


def ref_nms(boxes, logits, valid, counts, L, B, k, thr, post, dtype=torch.float32):
    """Per image the list of l * k + rank, by the restatement."""
    out = []
    for b in range(B):
        kept = []
        for l in range(L):
            s, c = l * B + b, int(counts[l * B + b])
            kept.append(R.nms_in_order(boxes[s, :c].to(dtype), valid[s, :c].bool(), thr))
        order = R.merge([logits[l * B + b][kept[l]] for l in range(L)], post)
        out.append([l * k + kept[l][p] for l, p in order])
    return out


def check_nms(lib, boxes, logits, valid, counts, L, B, k, thr, post, tag, dtype=torch.float32):
    want = ref_nms(boxes, logits, valid, counts, L, B, k, thr, post, dtype)
    cnt, oi, ob, osc = run_nms(lib, boxes, logits, valid, counts, L, B, k, thr, post)
    scores = torch.sigmoid(logits.float())        # the array run_nms hands to the kernel
    for b in range(B):
        d = int(cnt[b])
        assert d == len(want[b]), (tag, b, d, len(want[b]))
        assert oi[b, :d].tolist() == want[b], (tag, b)
        for r, e in enumerate(want[b]):
            s = (e // k) * B + b
            assert torch.equal(ob[b, r], boxes[s, e % k].float()), (tag, b, r)
            assert float(osc[b, r]) == float(scores[s, e % k]), (tag, b, r)
        # the tail behind the count is zero
        assert bool((oi[b, d:] == -1).all()) and bool((ob[b, d:] == 0).all()) and bool((osc[b, d:] == 0).all()), tag
    return cnt, oi


def segments(ns, k, seed, span=40, B=1):
    """Quarter-pixel boxes for segments of sizes ns (s = l B + b), descending distinct logits."""
    S_ = len(ns)
    boxes, logits = torch.zeros(S_, k, 4), torch.zeros(S_, k)
    valid = torch.zeros(S_, k, dtype=torch.int32)
    g = torch.Generator().manual_seed(seed)
    for s, n in enumerate(ns):
        boxes[s, :n] = quarter_pixel_boxes(n, seed * 100 + s, span).float()
        logits[s, :n] = torch.sort(torch.randn(n, generator=g) * 2, descending=True).values
        valid[s, :n] = 1
    return boxes, logits, valid, torch.tensor(ns, dtype=torch.int32)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 128, 129, 2000])
def test_nms_segment_sizes(lib, n):
    k = max(n, 70)
    boxes, logits, valid, counts = segments([n, max(n // 2, 1)], k, 5 + n, span=40 if n < 2000 else 90)
    if n >= 63:
        valid[0, 5::11] = 0       # invalid candidates neither survive nor suppress
    cnt, _ = check_nms(lib, boxes, logits, valid, counts, 2, 1, k, 0.7, k * 2, 'sizes n=%d' % n)
    print('nms n=%d: %d kept of %d + %d' % (n, int(cnt[0]), n, max(n // 2, 1)))
    a = run_nms(lib, boxes, logits, valid, counts, 2, 1, k, 0.7, k * 2)
    b = run_nms(lib, boxes, logits, valid, counts, 2, 1, k, 0.7, k * 2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('at', [10, 62])
def test_nms_chain_inside_and_across_a_block(lib, at):
    """A suppresses B; B alone would suppress C; A does not: C is kept.  at = 10: all three in block 0; at = 62: A and B
    in block 0, C in block 1."""
    k = 130
    boxes, logits, valid, counts = segments([130], k, 7, span=20)
    boxes[0, :, :] += torch.tensor([200., 0., 200., 0.])             # away from the chain
    A_, B_, C_ = [0., 0., 10., 10.], [2., 0., 12., 10.], [4.25, 0., 14.25, 10.]
    boxes[0, at], boxes[0, at + 1], boxes[0, at + 2] = torch.tensor(A_), torch.tensor(B_), torch.tensor(C_)
    iou = R.box_iou(boxes[0, at:at + 3].double(), boxes[0, at:at + 3].double())
    assert iou[0, 1] > 0.5 and iou[1, 2] > 0.5 and iou[0, 2] < 0.5
    _, oi = check_nms(lib, boxes, logits, valid, counts, 1, 1, k, 0.5, k, 'chain at %d' % at, torch.float64)
    kept = set(oi[0].tolist())
    assert at in kept and at + 1 not in kept and at + 2 in kept


def test_nms_dyadic_threshold_levels_identical_disjoint(lib):
    k = 70
    # level 0: IoU exactly 0.75 is not suppressed, just above it is; level 1: the same boxes again (levels never
    # suppress each other); level 2: 70 identical boxes -> one kept; level 3: a disjoint grid -> all kept
    boxes, logits = torch.zeros(4, k, 4), torch.zeros(4, k)
    valid, counts = torch.zeros(4, k, dtype=torch.int32), torch.tensor([3, 3, 70, 64], dtype=torch.int32)
    trio = torch.tensor([[0., 0., 8., 8.], [0., 0., 8., 6.], [0., 0., 8., 6.25]])
    assert float(R.box_iou(trio[1:2].double(), trio[:1].double())) == 0.75
    boxes[0, :3], boxes[1, :3] = trio, trio
    logits[0, :3], logits[1, :3] = torch.tensor([3., 2., 1.]), torch.tensor([3., 2., 1.])
    boxes[2, :70] = torch.tensor([5., 5., 9.5, 7.25])
    logits[2, :70] = torch.linspace(2.5, -2.5, 70)
    gy, gx = torch.meshgrid(torch.arange(8.), torch.arange(8.), indexing='ij')
    boxes[3, :64] = torch.stack([gx.reshape(-1) * 10, gy.reshape(-1) * 10, gx.reshape(-1) * 10 + 9.75,
                                 gy.reshape(-1) * 10 + 9.75], 1)
    logits[3, :64] = torch.linspace(4., -4., 64)
    for s in range(4):
        valid[s, :int(counts[s])] = 1
    cnt, oi = check_nms(lib, boxes, logits, valid, counts, 4, 1, k, 0.75, 200, 'dyadic', torch.float64)
    got = oi[0, :int(cnt[0])].tolist()
    assert [e for e in got if e < k] == [0, 1] and [e for e in got if k <= e < 2 * k] == [k, k + 1]
    assert [e for e in got if 2 * k <= e < 3 * k] == [2 * k] and len([e for e in got if e >= 3 * k]) == 64
    assert got.index(0) + 1 == got.index(k)     # equal logits: the lower level first


@pytest.mark.parametrize('post', [40, 150, 700])
def test_nms_post_limit_and_two_images(lib, post):
    """post_nms_top_n reached in the middle of a block of the scan (40: inside block 0 of every segment) and in the middle
    of the merge; two images with different counts (B = 2, three levels)."""
    k = 300
    ns = [300, 200, 150, 1, 129, 64]          # s = l B + b
    boxes, logits, valid, counts = segments(ns, k, 9, span=60)
    logits[3, 0] = 0.25
    valid[1, ::3] = 0
    cnt, _ = check_nms(lib, boxes, logits, valid, counts, 3, 2, k, 0.7, post, 'post %d' % post)
    print('post %d: counts %s' % (post, cnt.tolist()))
    assert int(cnt[0]) <= post and int(cnt[1]) <= post
    if post == 40:
        assert cnt.tolist() == [40, 40]
    if post == 700:
        assert int(cnt[0]) != int(cnt[1]) and int(cnt[0]) < 700
