"""Torch-core restatement of the box branch of torchvision's Mask R-CNN `roi_heads`, for the tests of
sfvos_amd.BoxBranch.  Written from torchvision's published behaviour (models/detection/faster_rcnn.py: TwoMLPHead,
FastRCNNPredictor; roi_heads.py: fastrcnn_loss, postprocess_detections; _utils.py: BoxCoder; ops/boxes.py: box_iou, nms,
batched_nms, clip_boxes_to_image, remove_small_boxes; transform.py: resize_boxes).  torchvision is not installed where
this project builds or runs: PARITY UNPINNED BY THE REFERENCE.  Never imported by the package.

Every function works in the dtype of its inputs (float64 in the kernel tests).  `detection_inputs` is the generator of
the detection test's inputs and `margin_safe` its margin rule (tests/test_box_branch_cpu.py counts the safe seeds)."""
import math

import torch
import torch.nn.functional as F
from torch import nn

BBOX_XFORM_CLIP = math.log(1000.0 / 16)
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


class TwoMLPHead(nn.Module):
    def __init__(self, in_channels=12544, representation_size=1024):
        super(TwoMLPHead, self).__init__()
        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)

    def forward(self, x):
        x = x.flatten(start_dim=1)
        return F.relu(self.fc7(F.relu(self.fc6(x))))


class FastRCNNPredictor(nn.Module):
    def __init__(self, in_channels=1024, num_classes=2):
        super(FastRCNNPredictor, self).__init__()
        self.cls_score = nn.Linear(in_channels, num_classes)
        self.bbox_pred = nn.Linear(in_channels, num_classes * 4)

    def forward(self, x):
        x = x.flatten(start_dim=1)
        return self.cls_score(x), self.bbox_pred(x)


class RefBoxBranch(nn.Module):
    """box_head + box_predictor on RoIAligned features [N,256,7,7] (the RoIAlign is oracle/roi_align_ref.py's)."""

    def __init__(self, num_classes=2):
        super(RefBoxBranch, self).__init__()
        self.box_head = TwoMLPHead(256 * 7 * 7, 1024)
        self.box_predictor = FastRCNNPredictor(1024, num_classes)

    def forward(self, roi_features):
        return self.box_predictor(self.box_head(roi_features))


def fastrcnn_loss(class_logits, box_regression, labels, regression_targets):
    labels = torch.cat(list(labels), 0) if isinstance(labels, (list, tuple)) else labels
    regression_targets = torch.cat(list(regression_targets), 0) if isinstance(regression_targets, (list, tuple)) \
        else regression_targets
    classification_loss = F.cross_entropy(class_logits, labels)
    pos = torch.where(labels > 0)[0]
    labels_pos = labels[pos]
    N = class_logits.shape[0]
    box_regression = box_regression.reshape(N, box_regression.size(-1) // 4, 4)
    box_loss = F.smooth_l1_loss(box_regression[pos, labels_pos], regression_targets[pos], beta=1 / 9, reduction='sum')
    return classification_loss, box_loss / labels.numel()


def encode_boxes(reference_boxes, proposals, weights=BOX_WEIGHTS):
    wx, wy, ww, wh = weights
    ex_w = proposals[:, 2] - proposals[:, 0]
    ex_h = proposals[:, 3] - proposals[:, 1]
    ex_cx = proposals[:, 0] + 0.5 * ex_w
    ex_cy = proposals[:, 1] + 0.5 * ex_h
    gt_w = reference_boxes[:, 2] - reference_boxes[:, 0]
    gt_h = reference_boxes[:, 3] - reference_boxes[:, 1]
    gt_cx = reference_boxes[:, 0] + 0.5 * gt_w
    gt_cy = reference_boxes[:, 1] + 0.5 * gt_h
    return torch.stack([wx * (gt_cx - ex_cx) / ex_w, wy * (gt_cy - ex_cy) / ex_h, ww * torch.log(gt_w / ex_w),
                        wh * torch.log(gt_h / ex_h)], 1)


def decode_boxes(rel_codes, boxes, weights=BOX_WEIGHTS, clip=BBOX_XFORM_CLIP):
    """[N,4K] codes, [N,4] boxes -> [N,K,4]"""
    wx, wy, ww, wh = weights
    w = boxes[:, 2] - boxes[:, 0]
    h = boxes[:, 3] - boxes[:, 1]
    cx = boxes[:, 0] + 0.5 * w
    cy = boxes[:, 1] + 0.5 * h
    dx, dy = rel_codes[:, 0::4] / wx, rel_codes[:, 1::4] / wy
    dw, dh = (rel_codes[:, 2::4] / ww).clamp(max=clip), (rel_codes[:, 3::4] / wh).clamp(max=clip)
    pcx, pcy = dx * w[:, None] + cx[:, None], dy * h[:, None] + cy[:, None]
    pw, ph = torch.exp(dw) * w[:, None], torch.exp(dh) * h[:, None]
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 2)


def clip_boxes_to_image(boxes, size):
    h, w = size
    out = boxes.clone()
    out[..., 0::2] = out[..., 0::2].clamp(0, w)
    out[..., 1::2] = out[..., 1::2].clamp(0, h)
    return out


def box_iou(a, b):
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b[None] - inter)


def nms(boxes, scores, iou_threshold):
    """Greedy NMS: indices kept, in descending score; ties in score keep the lower index first."""
    order = scores.argsort(descending=True, stable=True)
    m = box_iou(boxes[order], boxes[order])
    n = order.numel()
    supp = torch.zeros(n, dtype=torch.bool)
    keep = []
    for i in range(n):
        if supp[i]:
            continue
        keep.append(int(order[i]))
        supp |= m[i] > iou_threshold
    return torch.tensor(keep, dtype=torch.int64)


def batched_nms(boxes, scores, idxs, iou_threshold):
    """Classes never suppress each other (torchvision's _batched_nms_vanilla: NMS per class, then by score)."""
    keep = torch.zeros(scores.numel(), dtype=torch.bool)
    for c in torch.unique(idxs):
        sel = torch.where(idxs == c)[0]
        keep[sel[nms(boxes[sel], scores[sel], iou_threshold)]] = True
    kept = torch.where(keep)[0]
    return kept[scores[kept].argsort(descending=True, stable=True)]


def candidates(class_logits, box_regression, proposals, image_shape):
    """decode + softmax + clip, class 0 dropped: boxes [M(K-1),4], scores, labels of postprocess_detections."""
    K = class_logits.shape[1]
    boxes = clip_boxes_to_image(decode_boxes(box_regression, proposals), image_shape)
    scores = F.softmax(class_logits, -1)
    labels = torch.arange(K).view(1, -1).expand_as(scores)
    return boxes[:, 1:].reshape(-1, 4), scores[:, 1:].reshape(-1), labels[:, 1:].reshape(-1)


def select_detections(boxes, scores, labels, score_thresh=0.05, nms_thresh=0.5, detections_per_img=100, min_size=1e-2):
    """Candidate indices of the detections, in the order postprocess_detections returns them."""
    idx = torch.where(scores > score_thresh)[0]
    ws, hs = boxes[idx, 2] - boxes[idx, 0], boxes[idx, 3] - boxes[idx, 1]
    idx = idx[(ws >= min_size) & (hs >= min_size)]
    keep = batched_nms(boxes[idx], scores[idx], labels[idx], nms_thresh)[:detections_per_img]
    return idx[keep]


def postprocess_detections(class_logits, box_regression, proposals, image_shapes, score_thresh=0.05, nms_thresh=0.5,
                           detections_per_img=100):
    out, lo = [], 0
    for props, shape in zip(proposals, image_shapes):
        hi = lo + props.shape[0]
        b, s, l = candidates(class_logits[lo:hi], box_regression[lo:hi], props, shape)
        k = select_detections(b, s, l, score_thresh, nms_thresh, detections_per_img)
        out.append({'boxes': b[k], 'scores': s[k], 'labels': l[k], 'index': k})
        lo = hi
    return out


def resize_boxes(boxes, original_size, new_size):
    rh, rw = [torch.tensor(n, dtype=torch.float32) / torch.tensor(o, dtype=torch.float32)
              for n, o in zip(new_size, original_size)]
    x1, y1, x2, y2 = boxes.unbind(1)
    return torch.stack([x1 * rw.to(boxes.dtype), y1 * rh.to(boxes.dtype), x2 * rw.to(boxes.dtype),
                        y2 * rh.to(boxes.dtype)], 1)


# ---- inputs of the detection test -------------------------------------------------------------------------------------

IMAGE = (480, 854)
GT = [[100., 80., 380., 400.], [420., 150., 700., 330.], [600., 40., 690., 120.]]


def detection_inputs(seed, n=1000, dtype=torch.float64):
    """n proposals: three quarters jittered +-25 % around three ground-truth boxes in a 480 x 854 image, the rest
    uniform with sides 16-216 px; logits N(0, 2^2) with +2 on the jittered ones' foreground; deltas N(0, 1) for the
    centres, N(0, 0.5^2) for the sizes.  Two classes."""
    H, W = IMAGE
    g = torch.Generator().manual_seed(seed)
    gt = torch.tensor(GT, dtype=dtype)
    which = torch.randint(0, 4, (n,), generator=g)
    props = torch.empty(n, 4, dtype=dtype)
    for i in range(n):
        if which[i] < 3:
            b = gt[which[i]]
            bw, bh = b[2] - b[0], b[3] - b[1]
            j = (torch.rand(4, generator=g, dtype=dtype) - 0.5) * 0.5
            props[i] = torch.stack([b[0] + j[0] * bw, b[1] + j[1] * bh, b[2] + j[2] * bw, b[3] + j[3] * bh])
        else:
            c = torch.rand(2, generator=g, dtype=dtype) * torch.tensor([W, H], dtype=dtype)
            s = 16 + torch.rand(2, generator=g, dtype=dtype) * 200
            props[i] = torch.stack([c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2])
    props[:, 0::2] = props[:, 0::2].clamp(0, W)
    props[:, 1::2] = props[:, 1::2].clamp(0, H)
    logits = torch.randn(n, 2, generator=g, dtype=dtype) * 2.0
    logits[which < 3, 1] += 2.0
    deltas = torch.randn(n, 8, generator=g, dtype=dtype) * torch.tensor([1., 1., .5, .5] * 2, dtype=dtype)
    return logits, deltas, props


MARGIN = 1e-5   # about 100 fp32 ulps of an IoU


def margin_safe(boxes, scores, labels, detections_per_img=100, delta=MARGIN):
    """(safe, detections): safe when the selection is the same list at (score, IoU) thresholds (0.05 +- delta,
    0.5 +- delta) in all four combinations."""
    base = select_detections(boxes, scores, labels, 0.05, 0.5, detections_per_img)
    safe = all(torch.equal(select_detections(boxes, scores, labels, 0.05 + ds, 0.5 + dn, detections_per_img), base)
               for ds in (-delta, delta) for dn in (-delta, delta))
    return safe, base
