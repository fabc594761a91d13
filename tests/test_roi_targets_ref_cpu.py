"""CPU (no GPU): tests/roi_targets_ref.py, the restatement the GPU tests of the roi_heads training targets compare
with, against definitions that do not share its code: the IoU against a pixel count, the adaptive RoIAlign on inputs
whose result is known in closed form, the sampler's counts in every regime and, with a seeded generator, its
uniformity."""
import math

import torch

import roi_targets_ref as T


def test_iou_against_a_pixel_count_on_integer_boxes():
    g = torch.Generator().manual_seed(4)
    lo = torch.randint(0, 20, (40, 2), generator=g)
    sz = torch.randint(1, 14, (40, 2), generator=g)
    boxes = torch.cat([lo, lo + sz], 1).double()
    canvas = torch.zeros((40, 36, 36), dtype=torch.bool)
    for i, b in enumerate(boxes.long().tolist()):
        canvas[i, b[1]:b[3], b[0]:b[2]] = True
    inter = (canvas[:, None] & canvas[None]).flatten(2).sum(2).double()
    union = (canvas[:, None] | canvas[None]).flatten(2).sum(2).double()
    assert torch.equal(T.box_iou(boxes, boxes), inter / union)
    assert float(inter.min()) == 0 and bool(((inter > 0) & (inter < union)).any())


def test_match_rules_on_a_hand_made_case():
    gt = torch.tensor([[0., 0., 8., 8.], [8., 0., 16., 8.], [100., 100., 101., 101.]])
    lab = torch.tensor([3, 5, 7])
    props = torch.tensor([[0., 0., 8., 4.],      # IoU exactly 0.5 with box 0: positive
                          [4., 0., 12., 8.],     # IoU 1/3 with boxes 0 and 1: the lower index, background at (0.5, 0.5)
                          [0., 0., 8., 3.],      # 0.375: ignored at (0.5, 0.3)
                          [50., 50., 50., 60.],  # zero area: IoU 0
                          [40., 40., 41., 41.]])
    m = T.match(props, gt, lab, 0.5, 0.5)
    assert m['matched'].tolist() == [0, 0, 0, 0, 0, 0, 1, 2] and m['labels'].tolist() == [3, 0, 0, 0, 0, 3, 5, 7]
    assert m['arg'].tolist()[:3] == [0, 0, 0] and float(m['max_iou'][0]) == 0.5 and float(m['max_iou'][2]) == 0.375
    assert abs(float(m['max_iou'][1]) - 1 / 3) < 1e-7 and float((m['iou64'][1, :2] - 1 / 3).abs().max()) < 1e-15
    assert m['max_iou'].tolist()[5:] == [1.0, 1.0, 1.0]
    m = T.match(props, gt, lab, 0.5, 0.3)
    assert m['labels'].tolist() == [3, -1, -1, 0, 0, 3, 5, 7] and m['matched'].tolist() == [0, 0, 0, 0, 0, 0, 1, 2]
    m = T.match(props, gt[:0], lab[:0])
    assert m['labels'].tolist() == [0] * 5 and m['matched'].tolist() == [0] * 5


def test_adaptive_roi_align_on_closed_forms():
    M = 4
    ones = torch.ones((2, 37, 53), dtype=torch.uint8)
    boxes = torch.tensor([[3., 5., 30., 33.], [10.25, 2.5, 11.0, 3.0], [0., 0., 53., 37.], [60., 5., 80., 20.],
                          [5., -30., 20., -2.], [-9., 40., -2., 60.]])
    out, grids = T.roi_align_adaptive(ones, boxes, torch.tensor([0, 1, 0, 1, 0, 1]), M)
    assert float((out[:3] - 1.0).abs().max()) < 1e-12             # inside: the weights of a sample sum to 1
    assert float(out[3:].abs().max()) == 0.0                      # wholly outside: exactly 0
    assert grids.tolist()[:3] == [[7, 7], [1, 1], [10, 14]]
    # a box with sides of M k pixels on the integer grid: every bin is a k x k block of pixels, sampled at the pixel
    # centres of a grid of k x k; the sample at (y + .5, x + .5) is the mean of the 2 x 2 pixels around it
    g = torch.Generator().manual_seed(8)
    mask = (torch.rand((1, 37, 53), generator=g) > 0.5).to(torch.uint8)
    for k in (1, 3):
        x0, y0 = 7, 4
        box = torch.tensor([[float(x0), float(y0), float(x0 + M * k), float(y0 + M * k)]])
        out, grids = T.roi_align_adaptive(mask, box, torch.tensor([0]), M)
        assert grids.tolist() == [[k, k]]
        m = mask[0].double()
        quad = (m[:-1, :-1] + m[:-1, 1:] + m[1:, :-1] + m[1:, 1:]) / 4       # value of the sample at (y + .5, x + .5)
        want = quad[y0:y0 + M * k, x0:x0 + M * k].reshape(M, k, M, k).mean((1, 3))
        assert float((out[0] - want).abs().max()) < 1e-12
    # shifted by half a pixel the samples fall on the pixels themselves: the k x k block means of the mask
    for k in (1, 3):
        box = torch.tensor([[6.5, 3.5, 6.5 + M * k, 3.5 + M * k]])
        out, _ = T.roi_align_adaptive(mask, box, torch.tensor([0]), M)
        want = mask[0].double()[4:4 + M * k, 7:7 + M * k].reshape(M, k, M, k).mean((1, 3))
        assert torch.equal(out[0], want)


def _labels(n_pos, n_neg, n_ign, seed=0):
    lab = torch.cat([torch.full((n_pos,), 2), torch.zeros(n_neg, dtype=torch.int64), -torch.ones(n_ign, dtype=torch.int64)])
    return lab[torch.randperm(lab.numel(), generator=torch.Generator().manual_seed(seed))]


def test_sampler_counts_in_every_regime():
    g = torch.Generator().manual_seed(1)
    cases = [((40, 900, 30), (40, 472)),      # positives under the quota
             ((300, 600, 10), (128, 384)),    # over the quota
             ((30, 100, 50), (30, 100)),      # too few negatives: S < batch
             ((0, 700, 5), (0, 512)),         # no positives
             ((200, 0, 5), (128, 0)),         # no negatives
             ((0, 0, 64), (0, 0))]            # every label -1
    for (np_, nn_, ni), (wp, wn) in cases:
        lab = _labels(np_, nn_, ni)
        keys = torch.rand(lab.numel(), generator=g)
        index, pos_slot = T.sample(lab, keys, 512, 0.25)
        assert index.numel() == wp + wn and pos_slot.numel() == wp
        assert bool((index[1:] > index[:-1]).all()) and int((lab[index] == 0).sum()) == wn
        assert not bool((lab[index] < 0).any())
        # the chosen positives are those with the smallest keys
        pos = torch.where(lab >= 1)[0]
        if wp:
            chosen = set(index[pos_slot].tolist())
            cut = max(float(keys[i]) for i in chosen)
            assert all((float(keys[i]) <= cut) == (int(i) in chosen) for i in pos)
    # ties and NaN: equal keys fall back on the index, a NaN key comes last
    lab = torch.tensor([1, 1, 1, 1, 0, 0, 0, 0])
    keys = torch.tensor([0.5, float('nan'), 0.5, -0.0, 0.25, 0.25, float('inf'), 0.0])
    index, pos_slot = T.sample(lab, keys, 5, 0.6)
    assert index.tolist() == [0, 2, 3, 4, 7] and pos_slot.tolist() == [0, 1, 2]
    assert T.sample(lab, keys, 8, 1.0)[0].tolist() == list(range(8)) and T.sample(lab, keys, 3, 0.0)[0].tolist() == [4, 5, 7]


def test_sampler_is_uniform_over_the_positives():
    """Independent uniform keys: every positive is chosen with probability n_pos / #pos.  2000 seeded draws; each of the
    12 frequencies must lie within four binomial standard deviations of 1/3."""
    lab = _labels(12, 24, 4, seed=3)
    pos = torch.where(lab >= 1)[0]
    g = torch.Generator().manual_seed(11)
    draws, hits = 2000, torch.zeros(lab.numel())
    for _ in range(draws):
        index, pos_slot = T.sample(lab, torch.rand(lab.numel(), generator=g), 16, 0.25)
        assert pos_slot.numel() == 4 and index.numel() == 16
        hits[index[pos_slot]] += 1
    p = 4 / 12
    bound = 4 * math.sqrt(p * (1 - p) / draws)
    freq = hits[pos] / draws
    print('frequencies of the 12 positives: %s, bound %.4f around %.4f' % (['%.3f' % f for f in freq.tolist()], bound, p))
    assert float((freq - p).abs().max()) <= bound
    assert float(hits[lab < 1].sum()) == 0
