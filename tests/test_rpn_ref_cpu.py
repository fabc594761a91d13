"""CPU: self-checks of tests/rpn_ref.py, the torch-core restatement of torchvision's RegionProposalNetwork that the GPU
tests of sfvos_amd.rpn compare against -- the base-anchor table, anchors under unequal strides, the decode of zero
deltas, the NMS against a plain double loop, the selection order against a Python sort, and the margin safety of every
committed seed of the module test (16 of 16: no seed is left out).  sfvos_amd.AnchorGenerator is host code and is held to
the same table here.  PARITY UNPINNED BY THE REFERENCE (torchvision is not installed)."""
import math

import torch

import rpn_ref as R
from test_box_branch_cpu import quarter_pixel_boxes

# half-extents (x, y) of the anchors of the default generator, per size: ratio 0.5, 1, 2
TABLE = {32: [(23, 11), (16, 16), (11, 23)], 64: [(45, 23), (32, 32), (23, 45)], 128: [(91, 45), (64, 64), (45, 91)],
         256: [(181, 91), (128, 128), (91, 181)], 512: [(362, 181), (256, 256), (181, 362)]}


def _table():
    return torch.tensor([[[-x, -y, x, y] for x, y in TABLE[s]] for s in (32, 64, 128, 256, 512)], dtype=torch.float32)


def test_base_anchors_are_the_published_table():
    got = torch.stack(R.base_anchors())
    assert got.dtype == torch.float32 and torch.equal(got, _table())
    from sfvos_amd import AnchorGenerator
    assert torch.equal(AnchorGenerator().base_anchors(), _table())
    assert AnchorGenerator().num_anchors_per_location() == [3] * 5


def test_anchors_under_unequal_strides():
    """tensor 64 x 96, level 5 x 7: strides 64 // 5 = 12 and 96 // 7 = 13."""
    from sfvos_amd import AnchorGenerator
    a = R.grid_anchors([(5, 7)], (64, 96), ((32,),), ((0.5, 1.0, 2.0),))[0]
    assert a.shape == (105, 4)
    assert a[0].tolist() == [-23, -11, 23, 11]
    assert a[-1].tolist() == [6 * 13 - 11, 4 * 12 - 23, 6 * 13 + 11, 4 * 12 + 23]
    assert a[3 * (2 * 7 + 5) + 1].tolist() == [5 * 13 - 16, 2 * 12 - 16, 5 * 13 + 16, 2 * 12 + 16]
    b = AnchorGenerator(((32,),), ((0.5, 1.0, 2.0),)).grid_anchors([(5, 7)], (64, 96))[0]
    assert torch.equal(a, b)


def test_zero_deltas_decode_to_the_clipped_anchors():
    a = R.grid_anchors([(6, 10)], (96, 160), ((128,),), ((0.5, 1.0, 2.0),))[0]
    z = torch.zeros(a.shape[0])
    boxes, scores, valid = R.candidates(z, torch.zeros(a.shape[0], 4), a, torch.arange(a.shape[0]), (90, 150))
    assert torch.equal(boxes, R.clip_boxes(a, (90, 150)))
    assert bool((boxes[:, 0::2] >= 0).all()) and bool((boxes[:, 0::2] <= 150).all()) and bool((boxes[:, 1::2] <= 90).all())
    assert bool((scores == 0.5).all()) and bool(valid.all())
    # dw above the clamp: width = exp(log(1000 / 16)) * w
    d = torch.tensor([[0., 0., 10., 0.]], dtype=torch.float64)
    b = R.decode(d, torch.tensor([[0., 0., 16., 16.]], dtype=torch.float64))
    assert abs(float(b[0, 2] - b[0, 0]) - 1000.0) < 1e-9 and float(b[0, 3] - b[0, 1]) == 16.0


def _loop_nms(boxes, valid, thr):
    b = boxes.tolist()

    def iou(p, q):
        w = max(min(p[2], q[2]) - max(p[0], q[0]), 0.0)
        h = max(min(p[3], q[3]) - max(p[1], q[1]), 0.0)
        inter = w * h
        return inter / ((p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - inter)
    keep = []
    for i in range(len(b)):
        if valid[i] and all(not iou(b[k], b[i]) > thr for k in keep):
            keep.append(i)
    return keep


def test_vectorised_nms_is_the_double_loop():
    for seed in (0, 1):
        boxes = quarter_pixel_boxes(200, 20 + seed)
        valid = torch.ones(200, dtype=torch.bool)
        if seed:
            valid[::7] = False
        for thr in (0.7, 0.5, 0.75):
            assert R.nms_in_order(boxes, valid, thr) == _loop_nms(boxes, valid, thr)


def test_selection_is_a_python_sort_on_a_tie_heavy_vector():
    g = torch.Generator().manual_seed(5)
    v = (torch.randn(500, generator=g) * 2).round() / 2
    v[3], v[77] = 0.0, -0.0
    v[10], v[400] = float('inf'), float('-inf')
    v[20], v[21] = float('nan'), float('nan')

    def key(i):
        x = float(v[i])
        return (1, 0.0, i) if math.isnan(x) else (0, -x + 0.0, i)
    want = sorted(range(500), key=key)
    assert R.order_desc(v).tolist() == want
    for k in (1, 37, 498, 500, 900):
        assert R.select(v, k).tolist() == want[:min(k, 500)]
    assert want[0] == 10 and want[-2:] == [20, 21] and want[-3] == 400
    zeros = [i for i in want if float(v[i]) == 0.0]
    assert zeros == sorted(zeros) and 3 in zeros and 77 in zeros      # -0 == +0: ties by index alone


def test_merge_goes_by_logit_then_level():
    got = R.merge([torch.tensor([3.0, 1.0, 0.0]), torch.tensor([3.0, 2.0, -0.0]), torch.tensor([5.0])], 6)
    assert got == [(2, 0), (0, 0), (1, 0), (1, 1), (0, 1), (0, 2)]


def test_every_committed_seed_is_margin_safe():
    """No pair of same-level candidates has a float64 IoU within 1e-5 of the threshold and no candidate side lies within
    1e-5 of min_size: 16 of 16 seeds, both modes, both images, with the operands as given (fp32) and rounded to bf16."""
    anchors = R.grid_anchors(R.SHAPES, R.TENSOR, R.SIZES, R.RATIOS)
    safe = 0
    for seed in R.SEEDS:
        feats, sd = R.module_case(seed)
        worst_iou, worst_side = float('inf'), float('inf')
        for rnd in (lambda t: t, lambda t: t.bfloat16().float()):
            lg, dl = R.head_flat({k: rnd(v) for k, v in sd.items()}, {k: rnd(v) for k, v in feats.items()}, torch.float32)
            for mode in ('training', 'testing'):
                for b, size in enumerate(R.IMAGES):
                    di, ds = R.margin_report([z[b] for z in lg], [d[b] for d in dl], anchors, size, R.PRE[mode])
                    worst_iou, worst_side = min(worst_iou, di), min(worst_side, ds)
        print('seed %2d: IoU margin %.3e, side margin %.3e' % (seed, worst_iou, worst_side))
        safe += worst_iou > R.MARGIN and worst_side > R.MARGIN
    assert len(R.SEEDS) == 16 and safe == 16, safe
