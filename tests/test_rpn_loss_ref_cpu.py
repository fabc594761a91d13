"""CPU: the restatement tests/rpn_loss_ref.py against independent definitions -- the IoU against a pixel count on integer
boxes, BCE and smooth-L1 against torch.nn.functional, the low-quality rule on a hand-worked example (the ground-truth box
that no anchor overlaps included), the sampler's counts in every regime, the label counts of the committed match cases
and the margin-safe share of the real-valued ones."""
import pytest
import torch
import torch.nn.functional as F

import rpn_loss_ref as T
import rpn_ref as R


def test_anchors_are_the_per_level_grid_in_level_h_w_a_order():
    for name, (shapes, tensor) in T.PYRAMIDS.items():
        anc = T.anchors(shapes, tensor, *T.ANCHOR_SIZES[name])
        assert anc.shape == (3 * sum(h * w for h, w in shapes), 4)
    anc = T.anchors(*T.DAVIS, *T.ANCHOR_SIZES['davis'])
    m = T.match(anc, torch.tensor(T.CASE_DAVIS))
    assert anc.shape[0] == 257796 and torch.equal(m['max_iou'], m['iou64'].max(1).values.float())
    assert (int((m['labels'] == 1).sum()), int((m['labels'] == 0).sum())) == (9, 257203)
    assert torch.equal(T.anchors(*T.SMALL), torch.cat(R.grid_anchors(R.SHAPES, R.TENSOR, R.SIZES, R.RATIOS), 0))
    assert T.anchors(*T.SMALL).shape[0] == 3825 and T.anchors(*T.LARGE).shape[0] == 61200


def test_iou_is_a_pixel_count_on_integer_boxes():
    g = torch.Generator().manual_seed(0)
    xy = torch.randint(0, 20, (40, 2), generator=g)
    wh = torch.randint(1, 20, (40, 2), generator=g)
    boxes = torch.cat([xy, xy + wh], 1)
    yy, xx = torch.meshgrid(torch.arange(40), torch.arange(40), indexing='ij')
    cover = [(xx >= b[0]) & (xx < b[2]) & (yy >= b[1]) & (yy < b[3]) for b in boxes]
    want = torch.tensor([[float((a & b).sum()) / float((a | b).sum()) for b in cover[20:]] for a in cover[:20]],
                        dtype=torch.float64)
    assert torch.allclose(T.box_iou(boxes[:20].double(), boxes[20:].double()), want, rtol=0, atol=1e-15)
    assert torch.equal(T.box_iou(boxes[:20].float(), boxes[20:].float()), want.float())     # one rounded division


@pytest.mark.parametrize('beta', [0.0, 1.0 / 9])
def test_loss_terms_are_torchs(beta):
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(50, generator=g, dtype=torch.float64) * 5, torch.tensor([0., 200., -200., 1e-9, -30.])])
    z = (torch.rand(x.numel(), generator=g) < 0.5).double()
    got, mag = T.bce_with_logits(x, z)
    assert torch.allclose(got, F.binary_cross_entropy_with_logits(x, z, reduction='none'), rtol=1e-12, atol=1e-300)
    assert bool((mag >= got.abs()).all())
    d = torch.cat([torch.randn(60, generator=g, dtype=torch.float64) * 0.2, torch.tensor([0., 1 / 9, -1 / 9, 0.111, 5.])])
    got, mag = T.smooth_l1(d, beta)
    want = F.smooth_l1_loss(d, torch.zeros_like(d), beta=beta, reduction='none') if beta else \
        F.l1_loss(d, torch.zeros_like(d), reduction='none')
    assert torch.allclose(got, want, rtol=1e-12, atol=0) and bool((mag >= got).all())


def test_encode_is_the_box_coder():
    anc = torch.tensor([[0., 0., 10., 20.], [5., 5., 9., 7.]])
    gt = torch.tensor([[1., 2., 11., 22.], [5., 5., 13., 6.]])
    want = torch.tensor([[0.1, 0.1, 0.0, 0.0], [0.5, -0.25, 0.6931471805599453, -0.6931471805599453]], dtype=torch.float64)
    assert torch.allclose(T.encode(gt, anc), want, rtol=1e-15, atol=1e-15)
    assert bool((T.encode_allowance(gt, anc, 1.0) > 0).all())


def test_low_quality_rule_by_hand():
    """Four anchors, three ground-truth boxes, thresholds 0.7 / 0.3.
      anchor 0 = gt 0                              IoU 1                      positive at the threshold
      anchor 1 overlaps gt 1 by half               IoU 32 / 96 with gt 1      ignored, then positive: it is gt 1's best
      anchor 2 overlaps gt 1 by half, mirrored     IoU 32 / 96 with gt 1      the same IoU: a tie at `highest`, positive too
      anchor 3 overlaps gt 0 by a quarter          IoU 16 / 112               background
    gt 2 overlaps no anchor: highest = 0 and EVERY anchor has IoU 0 with it -- all four become positive, and each keeps
    its own argmax (anchor 3: gt 0) as match."""
    anc = torch.tensor([[0., 0., 8., 8.], [20., 0., 28., 8.], [28., 0., 36., 8.], [4., 4., 12., 12.]])
    gt = torch.tensor([[0., 0., 8., 8.], [24., 0., 32., 8.]])
    m = T.match(anc, gt, 0.7, 0.3, False)
    assert m['labels'].tolist() == [1, -1, -1, 0] and m['matched'].tolist() == [0, 0, 0, 0]
    assert m['max_iou'].tolist() == [1.0, float(torch.tensor(32.) / 96), float(torch.tensor(32.) / 96),
                                     float(torch.tensor(16.) / 112)]
    m = T.match(anc, gt, 0.7, 0.3, True)
    assert m['labels'].tolist() == [1, 1, 1, 0] and m['matched'].tolist() == [0, 1, 1, 0] and m['pos_high'] == 1
    far = torch.cat([gt, torch.tensor([[100., 100., 110., 110.]])])
    m = T.match(anc, far, 0.7, 0.3, True)
    assert m['labels'].tolist() == [1, 1, 1, 1] and m['matched'].tolist() == [0, 1, 1, 0]
    m = T.match(anc, far, 0.7, 0.3, False)
    assert m['labels'].tolist() == [1, -1, -1, 0]
    # no ground truth: everything background
    m = T.match(anc, gt[:0])
    assert m['labels'].tolist() == [0] * 4 and m['matched'].tolist() == [0] * 4 and m['max_iou'].tolist() == [0.0] * 4


@pytest.mark.parametrize('name', sorted(T.CASES))
def test_label_counts_of_the_committed_cases(name):
    pyramid, gt, want = T.CASES[name]
    m = T.match(T.anchors(*T.PYRAMIDS[pyramid]), torch.tensor(gt))
    lab = m['labels']
    got = (m['pos_high'], int((lab == 1).sum()), int((lab == 0).sum()), int((lab == -1).sum()))
    print(name, got)
    assert all(w is None or w == g for w, g in zip(want, got)), (got, want)
    assert sum(got[1:]) == lab.numel()
    if name == 'b':      # no anchor reaches 0.7: every positive is a tie at `highest`
        assert got[0] == 0 and got[1] == 110
    if name == 'c':
        assert got[0] > 128
    # exact arithmetic: the fp32 IoU is the correctly rounded float64 one
    assert torch.equal(m['max_iou'], m['iou64'].max(1).values.float())


@pytest.mark.parametrize('pyramid,seed,G', T.REAL_CASES)
def test_margin_safe_share_of_the_real_valued_cases(pyramid, seed, G):
    anc, gt = T.real_case(pyramid, seed, G)
    m = T.match(anc, gt)
    safe = T.margin_safe(m['iou64'])
    share = 1.0 - float(safe.double().mean())
    print(pyramid, seed, G, 'left out: %.4f %%' % (100 * share))
    assert share <= T.MAX_UNSAFE_SHARE
    lab = m['labels']
    assert int((lab == 1).sum()) > 0 and int((lab == 0).sum()) > 0 and int((lab == -1).sum()) > 0


REGIMES = {'positives over the cap': ((300, 3000, 100), (256, 128)), 'positives under the cap': ((40, 3000, 100), (256, 40)),
           'too few negatives': ((30, 100, 3000), (130, 30)), 'no positives': ((0, 3000, 100), (256, 0)),
           'no negatives': ((500, 0, 0), (128, 128)), 'everything ignored': ((0, 0, 700), (0, 0))}


def regime_labels(n_pos, n_neg, n_ign, seed, N=None):
    lab = torch.cat([torch.ones(n_pos, dtype=torch.int64), torch.zeros(n_neg, dtype=torch.int64),
                     -torch.ones(n_ign, dtype=torch.int64)])
    if N is not None:
        lab = torch.cat([lab, -torch.ones(N - lab.numel(), dtype=torch.int64)])
    return lab[torch.randperm(lab.numel(), generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize('regime', sorted(REGIMES))
def test_sampler_counts(regime):
    (n_pos, n_neg, n_ign), (S, P) = REGIMES[regime]
    labels = regime_labels(n_pos, n_neg, n_ign, 3)
    keys = torch.rand(labels.numel(), generator=torch.Generator().manual_seed(4))
    pos, neg = T.sample(labels, keys, 256, 0.5)
    assert (pos.numel() + neg.numel(), pos.numel()) == (S, P)
    assert bool((labels[pos] == 1).all()) and bool((labels[neg] == 0).all())
    assert bool((pos[1:] > pos[:-1]).all()) and bool((neg[1:] > neg[:-1]).all())
    # the chosen keys are the smallest of their class
    for chosen, cls in ((pos, 1), (neg, 0)):
        rest = torch.ones_like(labels, dtype=torch.bool)
        rest[chosen] = False
        rest &= labels == cls
        if chosen.numel() and bool(rest.any()):
            assert float(keys[chosen].max()) <= float(keys[rest].min())


def test_sampler_order_of_special_keys():
    labels = torch.tensor([1, 1, 1, 1, 1, 1, 0, -1])
    keys = torch.tensor([float('nan'), 0.0, -0.0, float('-inf'), float('inf'), 0.0, 0.5, -1.0])
    for n, want in ((1, [3]), (2, [1, 3]), (3, [1, 2, 3]), (4, [1, 2, 3, 5]), (5, [1, 2, 3, 4, 5]), (6, [0, 1, 2, 3, 4, 5])):
        pos, neg = T.sample(labels, keys, 2 * n, 0.5)
        assert pos.tolist() == want and neg.tolist() == [6]
    pos, _ = T.sample(torch.ones(10, dtype=torch.int64), torch.full((10,), 0.5), 8, 0.5)
    assert pos.tolist() == [0, 1, 2, 3]


def test_rpn_losses_are_torchs_on_the_sampled_anchors():
    anc = T.anchors(*T.SMALL)
    N = anc.shape[0]
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(2, N, generator=g, dtype=torch.float64) * 3
    deltas = torch.randn(2, N, 4, generator=g, dtype=torch.float64) * 0.3
    gts = [torch.tensor(T.CASE_A), torch.zeros((0, 4))]
    keys = [torch.rand(N, generator=g), torch.rand(N, generator=g)]
    for beta in (0.0, 1.0 / 9):
        r = T.rpn_losses(logits, deltas, anc, gts, keys, beta=beta)
        assert r['counts'] == [(256, 49), (256, 0)]
        lab, reg, tgt = [], [], []
        for b in range(2):
            idx, P = r['index'][b], r['counts'][b][1]
            lab.append((torch.arange(idx.numel()) < P).double())
            m = T.match(anc, gts[b])
            reg.append(deltas[b][idx[:P]])
            tgt.append(T.encode(gts[b].float()[m['matched'][idx[:P]]], anc[idx[:P]]) if P else torch.zeros((0, 4)).double())
        x = torch.cat([logits[b][r['index'][b]] for b in range(2)])
        want_obj = F.binary_cross_entropy_with_logits(x, torch.cat(lab))
        a, t = torch.cat(reg), torch.cat(tgt)
        want_box = (F.smooth_l1_loss(a, t, beta=beta, reduction='sum') if beta else F.l1_loss(a, t, reduction='sum')) / 512
        assert abs(r['loss_objectness'] - float(want_obj)) <= 1e-12 * float(want_obj)
        assert abs(r['loss_rpn_box_reg'] - float(want_box)) <= 1e-12 * float(want_box)


def test_per_image_undoes_the_level_major_storage():
    B, A = 2, 3
    shapes = R.SHAPES
    P = B * sum(h * w for h, w in shapes)
    obj = torch.arange(P * A, dtype=torch.float64).view(P, A)
    lg, dd = T.per_image(obj, torch.zeros(P, 4 * A, dtype=torch.float64), shapes, B, A)
    assert lg.shape == (B, 3825) and dd.shape == (B, 3825, 4)
    # image 1, level 1, position 7, anchor 2
    n = A * (24 * 40 + 7) + 2
    assert float(lg[1, n]) == float(obj[B * 24 * 40 + 12 * 20 + 7, 2])
