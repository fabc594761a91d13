"""CPU: the surface of the box branch (sfvos_amd.BoxBranch and friends) and self-checks of its torch-core restatement
tests/box_branch_ref.py -- the names and shapes a reference checkpoint's `roi_heads.box_head.*` /
`roi_heads.box_predictor.*` slice needs, strict loads both ways, no CPU fallback, the restatement against independent
definitions (brute-force NMS, decode(encode(b)) = b, F.cross_entropy / F.smooth_l1_loss), and the margin-safety count of
the detection test's inputs (tests/test_gpu_boxhead_kernels.py compares only margin-safe seeds and may skip at most 2 of
16; the count is verified here, without a GPU).  PARITY UNPINNED BY THE REFERENCE (torchvision is not installed)."""
import pytest
import torch
import torch.nn.functional as F

import box_branch_ref as R

WANT = {'box_head.fc6.weight': (1024, 12544), 'box_head.fc6.bias': (1024,),
        'box_head.fc7.weight': (1024, 1024), 'box_head.fc7.bias': (1024,),
        'box_predictor.cls_score.weight': (2, 1024), 'box_predictor.cls_score.bias': (2,),
        'box_predictor.bbox_pred.weight': (8, 1024), 'box_predictor.bbox_pred.bias': (8,)}


def test_state_dict_keys_and_shapes_are_torchvisions():
    from sfvos_amd import BoxBranch
    m, o = BoxBranch(2, 'fp32'), R.RefBoxBranch(2)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == WANT
    assert got == {k: tuple(v.shape) for k, v in o.state_dict().items()}
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in o.named_parameters()]


def test_strict_load_both_ways_and_of_a_checkpoint_slice():
    import io
    from sfvos_amd import BoxBranch
    g = torch.Generator().manual_seed(1)
    ckpt = {'slow_fast.bn_f1.weight': torch.ones(32)}
    ckpt.update({'maskrcnn_model.roi_heads.' + k: torch.randn(s, generator=g) for k, s in WANT.items()})
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=True)
    prefix = 'maskrcnn_model.roi_heads.'
    sl = {k[len(prefix):]: v for k, v in loaded.items() if k.startswith(prefix)}
    m = BoxBranch(2, 'bf16')
    m.load_state_dict(sl, strict=True)
    o = R.RefBoxBranch(2)
    o.load_state_dict(m.state_dict(), strict=True)
    m2 = BoxBranch(2, 'fp32')
    m2.load_state_dict(o.state_dict(), strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sl[k]), k


def test_default_initialisation_is_nn_linears():
    """torchvision leaves TwoMLPHead / FastRCNNPredictor at nn.Linear's default initialisation: same generator state,
    same values."""
    from sfvos_amd import BoxBranch
    torch.manual_seed(3)
    m = BoxBranch(2, 'fp32')
    torch.manual_seed(3)
    o = R.RefBoxBranch(2)
    for (k, a), (_, b) in zip(m.state_dict().items(), o.state_dict().items()):
        assert torch.equal(a, b), k


def test_cpu_input_raises():
    from sfvos_amd import BoxBranch, RoIHeadsInference, decode_boxes, encode_boxes, fastrcnn_loss, resize_boxes
    m = BoxBranch()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.forward_features(torch.zeros(2, 256, 7, 7))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m({'0': torch.zeros(1, 256, 8, 8)}, [torch.tensor([[0., 0., 4., 4.]])], [(32, 32)])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fastrcnn_loss(torch.zeros(2, 2), torch.zeros(2, 8), [torch.zeros(2, dtype=torch.int64)], [torch.zeros(2, 4)])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        encode_boxes(torch.ones(1, 4), torch.ones(1, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        decode_boxes(torch.ones(1, 8), torch.ones(1, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        resize_boxes(torch.ones(1, 4), (4, 4), (8, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        RoIHeadsInference()({'0': torch.zeros(1, 256, 8, 8)}, [torch.tensor([[0., 0., 4., 4.]])], [(32, 32)])
    with pytest.raises(ValueError):
        BoxBranch(num_classes=9)


def test_bindings_cover_the_box_entry_points():
    from sfvos_amd import _lib
    assert _lib.ABI_REVISION >= 302
    for name in ('sfvos_dense', 'sfvos_pack_dense_fwd', 'sfvos_pack_dense_dgrad', 'sfvos_dense_wgrad',
                 'sfvos_box_predictor', 'sfvos_box_predictor_bwd', 'sfvos_fastrcnn_loss', 'sfvos_fastrcnn_loss_grad',
                 'sfvos_box_decode', 'sfvos_box_encode', 'sfvos_detections', 'sfvos_box_scale'):
        assert name in _lib.SIGNATURES, name


# ---- the restatement against independent definitions --------------------------------------------------------------------

def _brute_nms(boxes, scores, thr):
    """Definition: walk the boxes by descending score (ties: lower index); keep one unless an already kept one
    overlaps it by IoU > thr.  O(n^2) in plain Python numbers."""
    b = boxes.tolist()
    order = sorted(range(len(b)), key=lambda i: (-float(scores[i]), i))

    def iou(p, q):
        w = max(min(p[2], q[2]) - max(p[0], q[0]), 0.0)
        h = max(min(p[3], q[3]) - max(p[1], q[1]), 0.0)
        inter = w * h
        return inter / ((p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - inter)
    keep = []
    for i in order:
        if all(not iou(b[k], b[i]) > thr for k in keep):
            keep.append(i)
    return keep


def quarter_pixel_boxes(n, seed, span=40):
    """Boxes on a quarter-pixel grid: areas, intersections and unions are exact in fp32 and float64 alike."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(0, 4 * span, (n, 2), generator=g).double() / 4
    wh = torch.randint(4, 4 * span, (n, 2), generator=g).double() / 4
    return torch.cat([xy, xy + wh], 1)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restated_nms_is_the_brute_force_definition(seed):
    boxes = quarter_pixel_boxes(300, seed)
    g = torch.Generator().manual_seed(100 + seed)
    scores = torch.rand(300, generator=g, dtype=torch.float64)
    if seed == 2:
        scores = (scores * 8).floor() / 8          # many ties
    # pairs at exactly IoU 0.5 are not suppressed: [0,0,2,1] and [0,0,1,1] (inter 1, union 2)
    boxes[:2] = torch.tensor([[200., 200., 202., 201.], [200., 200., 201., 201.]], dtype=torch.float64)
    assert float(R.box_iou(boxes[:1], boxes[1:2])) == 0.5
    assert R.nms(boxes, scores, 0.5).tolist() == _brute_nms(boxes, scores, 0.5)
    labels = torch.randint(0, 3, (300,), generator=g)
    want = []
    for c in range(3):
        sel = [i for i in range(300) if int(labels[i]) == c]
        want += [sel[k] for k in _brute_nms(boxes[sel], scores[sel], 0.5)]
    want.sort(key=lambda i: (-float(scores[i]), i))
    assert R.batched_nms(boxes, scores, labels, 0.5).tolist() == want


def test_restated_coder_round_trips_and_clamps():
    g = torch.Generator().manual_seed(4)
    p = quarter_pixel_boxes(64, 5) + torch.rand(64, 4, generator=g, dtype=torch.float64) * 0.1
    b = quarter_pixel_boxes(64, 6)
    back = R.decode_boxes(R.encode_boxes(b, p), p)[:, 0]
    assert float((back - b).abs().max()) < 1e-9
    big = torch.tensor([[0., 0., 100., 100.]], dtype=torch.float64)
    out = R.decode_boxes(big, torch.tensor([[0., 0., 10., 10.]], dtype=torch.float64))[0, 0]
    assert abs(float(out[2] - out[0]) - 10 * 1000.0 / 16) < 1e-9       # dw clamped at log(1000 / 16)
    r = R.resize_boxes(torch.tensor([[1., 2., 3., 4.]]), (10, 20), (20, 60))
    assert r.tolist() == [[3., 4., 9., 8.]]


def test_restated_loss_is_cross_entropy_plus_smooth_l1():
    g = torch.Generator().manual_seed(7)
    N, K = 40, 3
    logits = torch.randn(N, K, generator=g, dtype=torch.float64) * 3
    deltas = torch.randn(N, 4 * K, generator=g, dtype=torch.float64)
    labels = torch.randint(0, K, (N,), generator=g)
    targets = torch.randn(N, 4, generator=g, dtype=torch.float64)
    lc, lb = R.fastrcnn_loss(logits, deltas, [labels[:10], labels[10:]], [targets[:10], targets[10:]])
    assert abs(float(lc) - float(F.cross_entropy(logits, labels))) < 1e-12
    want = 0.0
    for i in range(N):
        if labels[i] > 0:
            d = deltas[i, 4 * int(labels[i]):4 * int(labels[i]) + 4]
            want += float(F.smooth_l1_loss(d, targets[i], beta=1 / 9, reduction='sum'))
    assert abs(float(lb) - want / N) < 1e-12
    # by hand: |d| < beta -> d^2 / (2 beta), else |d| - beta / 2
    d = (deltas[0, 4:8] - targets[0]).abs()
    hand = torch.where(d < 1 / 9, 0.5 * d * d * 9, d - 0.5 / 9).sum()
    assert abs(float(F.smooth_l1_loss(deltas[0, 4:8], targets[0], beta=1 / 9, reduction='sum')) - float(hand)) < 1e-12


def test_detection_inputs_are_margin_safe():
    """The condition of the GPU detection test, counted here on float64 candidates: at most 2 of the 16 seeds may be
    unsafe at delta = 1e-5 (and every seed yields the full 100 detections, so the top-k cut is exercised)."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    safe = 0
    for seed in range(16):
        logits, deltas, props = R.detection_inputs(seed)
        b, s, l = R.candidates(logits, deltas, props, R.IMAGE)
        ok, base = R.margin_safe(b, s, l)
        assert base.numel() == 100, (seed, base.numel())
        safe += bool(ok)
        print('seed %d: %d detections, margin-safe %s' % (seed, base.numel(), ok))
    print('%d of 16 seeds margin-safe at delta = %g' % (safe, R.MARGIN))
    assert safe >= 14
