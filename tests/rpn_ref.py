"""Torch-core restatement of torchvision's RegionProposalNetwork in inference, for the tests of sfvos_amd.rpn.  Written
from torchvision's published behaviour (models/detection/rpn.py: RPNHead, RegionProposalNetwork.filter_proposals;
anchor_utils.py: AnchorGenerator; _utils.py: BoxCoder(1, 1, 1, 1).decode; ops/boxes.py: clip_boxes_to_image,
remove_small_boxes, nms, batched_nms).  torchvision is not installed where this project builds or runs: PARITY UNPINNED BY
THE REFERENCE.  Never imported by the package.

Order, everywhere: objectness logit descending, ties by (level, anchor index) ascending; values compare as floats
(-0 == +0, +-inf ordinary) and NaN ranks below every number.  This deviates from torch.topk (NaN first) and pins what
torchvision leaves unspecified (ties, saturated sigmoids): the merge over levels goes by logit, not by its sigmoid.

Every function works in the dtype of its inputs.  `module_case` generates the inputs of the module test and
`margin_report` is its margin rule (tests/test_rpn_ref_cpu.py asserts it for every committed seed)."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

BBOX_XFORM_CLIP = math.log(1000.0 / 16)
DEFAULT_SIZES = ((32,), (64,), (128,), (256,), (512,))
DEFAULT_RATIOS = ((0.5, 1.0, 2.0),) * 5


class RPNHead(nn.Module):
    def __init__(self, in_channels=256, num_anchors=3):
        super(RPNHead, self).__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, 3, 1, 1)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, 1, 1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, 1, 1)

    def hidden(self, x):
        return [F.relu(self.conv(f)) for f in x]

    def forward(self, x):
        t = self.hidden(x)
        return [self.cls_logits(f) for f in t], [self.bbox_pred(f) for f in t]


def base_anchors(sizes=DEFAULT_SIZES, ratios=DEFAULT_RATIOS):
    """list over levels of [A, 4] fp32: torch's CPU ops, rounded half to even."""
    out = []
    for s, r in zip(sizes, ratios):
        scales = torch.as_tensor(s, dtype=torch.float32)
        ar = torch.as_tensor(r, dtype=torch.float32)
        h_r = torch.sqrt(ar)
        w_r = 1 / h_r
        ws = (w_r[:, None] * scales[None, :]).view(-1)
        hs = (h_r[:, None] * scales[None, :]).view(-1)
        out.append((torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round())
    return out


def grid_anchors(shapes, tensor_size, sizes=DEFAULT_SIZES, ratios=DEFAULT_RATIOS):
    """list over levels of [H W A, 4] fp32 anchors in (h, w, a) order; strides = tensor_size // (H, W)."""
    out = []
    for (H, W), base in zip(shapes, base_anchors(sizes, ratios)):
        sh, sw = tensor_size[0] // H, tensor_size[1] // W
        rows = []
        for h in range(H):
            for w in range(W):
                rows.append(base + torch.tensor([w * sw, h * sh, w * sw, h * sh], dtype=torch.float32))
        out.append(torch.cat(rows, 0))
    return out


def flatten_head(t):
    """[B, A c, H, W] -> [B, H W A, c] (c = 1: [B, H W A]): torchvision's permute_and_flatten."""
    B, AC, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, -1)


def order_desc(v):
    """Indices of v by descending value, ties (and -0 / +0) by index, NaN last (by index)."""
    nan = torch.isnan(v)
    o = torch.where(nan, torch.full_like(v, float('-inf')), v).argsort(descending=True, stable=True)
    return o[nan[o].to(torch.int8).argsort(stable=True)]


def select(v, k):
    return order_desc(v)[:min(int(k), v.numel())]


def decode(deltas, anchors, clip=BBOX_XFORM_CLIP):
    """BoxCoder(1, 1, 1, 1).decode_single: [N, 4] deltas, [N, 4] anchors -> [N, 4]."""
    w = anchors[:, 2] - anchors[:, 0]
    h = anchors[:, 3] - anchors[:, 1]
    cx = anchors[:, 0] + 0.5 * w
    cy = anchors[:, 1] + 0.5 * h
    dx, dy = deltas[:, 0], deltas[:, 1]
    dw, dh = deltas[:, 2].clamp(max=clip), deltas[:, 3].clamp(max=clip)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)


def decode_allowance(deltas, anchors, trans=2.0 ** -20):
    """Per-element allowance of a decoded coordinate against float64, as tests/test_gpu_boxhead_kernels.py derives it for
    box_decode (weights 1 here): `trans` on the magnitudes of its terms (|dx| w + |cx| + exp(dw) w / 2), and the rounding
    of the exponent's argument carried through exp (|dw| 2^-24 times the half size).  Clipping is monotone: the
    allowance of the unclipped value holds."""
    d, a = deltas.double(), anchors.double()
    w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    cx, cy = a[:, 0] + 0.5 * w, a[:, 1] + 0.5 * h
    dw, dh = d[:, 2].clamp(max=BBOX_XFORM_CLIP), d[:, 3].clamp(max=BBOX_XFORM_CLIP)
    mx = d[:, 0].abs() * w + cx.abs() + 0.5 * torch.exp(dw) * w * (1 + dw.abs() * 2.0 ** -4)
    my = d[:, 1].abs() * h + cy.abs() + 0.5 * torch.exp(dh) * h * (1 + dh.abs() * 2.0 ** -4)
    return trans * torch.stack([mx, my, mx, my], 1)


def clip_boxes(boxes, size):
    h, w = size
    out = boxes.clone()
    out[:, 0::2] = out[:, 0::2].clamp(0, w)
    out[:, 1::2] = out[:, 1::2].clamp(0, h)
    return out


def box_iou(a, b):
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b[None] - inter)


def nms_in_order(boxes, valid, thr):
    """Greedy NMS over boxes visited in the order given; invalid ones are skipped.  -> kept positions."""
    n = boxes.shape[0]
    m = box_iou(boxes, boxes) > thr
    supp = ~valid.clone()
    keep = []
    for i in range(n):
        if supp[i]:
            continue
        keep.append(i)
        supp |= m[i]
    return keep


def candidates(logits, deltas, anchors, idx, image_size, min_size=1e-3, score_thresh=0.0):
    """The selected anchors idx of one segment -> (boxes, scores, valid)."""
    boxes = clip_boxes(decode(deltas[idx], anchors[idx].to(deltas.dtype)), image_size)
    scores = torch.sigmoid(logits[idx])
    valid = ((boxes[:, 2] - boxes[:, 0]) >= min_size) & ((boxes[:, 3] - boxes[:, 1]) >= min_size) & (scores > score_thresh)
    return boxes, scores, valid


def merge(kept_logits, post):
    """kept_logits: list over levels of the kept candidates' logits (each descending) -> [(level, place)] of the first
    `post` by (logit descending, level, place)."""
    items = [(-float(z) + 0.0, l, p) for l, zs in enumerate(kept_logits) for p, z in enumerate(zs)]
    items.sort()
    return [(l, p) for _, l, p in items[:post]]


def filter_proposals(logits, deltas, anchors, image_size, pre, post, nms_thresh=0.7, score_thresh=0.0, min_size=1e-3):
    """One image.  logits: list over levels of [n_l]; deltas: list of [n_l, 4]; anchors: list of [n_l, 4] ->
    dict(level, rank, anchor: int lists; boxes [n, 4]; scores [n]) of the proposals in order."""
    per = []
    for z, d, a in zip(logits, deltas, anchors):
        idx = select(z, pre)
        boxes, scores, valid = candidates(z, d, a, idx, image_size, min_size, score_thresh)
        keep = nms_in_order(boxes, valid, nms_thresh)
        per.append((idx, boxes, scores, keep, z[idx]))
    order = merge([zs[keep] for _, _, _, keep, zs in per], post)
    out = dict(level=[], rank=[], anchor=[], boxes=[], scores=[])
    for l, p in order:
        idx, boxes, scores, keep, _ = per[l]
        r = keep[p]
        out['level'].append(l); out['rank'].append(r); out['anchor'].append(int(idx[r]))
        out['boxes'].append(boxes[r]); out['scores'].append(scores[r])
    dt = deltas[0].dtype
    out['boxes'] = torch.stack(out['boxes']) if out['boxes'] else torch.zeros(0, 4, dtype=dt)
    out['scores'] = torch.stack(out['scores']) if out['scores'] else torch.zeros(0, dtype=dt)
    return out


# ---- inputs of the module test -----------------------------------------------------------------------------------------

SHAPES = [(24, 40), (12, 20), (6, 10), (3, 5)]
TENSOR = (96, 160)
IMAGES = [(90, 150), (96, 160)]
SIZES = ((32,), (64,), (128,), (256,))
RATIOS = ((0.5, 1.0, 2.0),) * 4
PRE = dict(training=50, testing=30)
POST = dict(training=30, testing=50)
SEEDS = [0, 3, 5, 8, 9, 13, 18, 19, 20, 21, 22, 23, 24, 26, 31, 34]   # picked on the CPU: all margin-safe
MARGIN = 1e-5   # about 100 fp32 ulps of an IoU


def module_case(seed, batch=2, channels=256):
    """(features: OrderedDict of [B, C, H, W] fp32, state dict of an RPNHead(C, 3)): N(0, 1) features; conv weights
    N(0, 0.02^2), cls_logits N(0, 0.1^2), bbox_pred N(0, 0.03^2), small biases."""
    g = torch.Generator().manual_seed(1000 + seed)
    feats = OrderedDict((str(l), torch.randn(batch, channels, H, W, generator=g)) for l, (H, W) in enumerate(SHAPES))
    sd = OrderedDict()
    sd['conv.weight'] = torch.randn(channels, channels, 3, 3, generator=g) * 0.02
    sd['conv.bias'] = torch.randn(channels, generator=g) * 0.1
    sd['cls_logits.weight'] = torch.randn(3, channels, 1, 1, generator=g) * 0.1
    sd['cls_logits.bias'] = torch.randn(3, generator=g) * 0.1
    sd['bbox_pred.weight'] = torch.randn(12, channels, 1, 1, generator=g) * 0.03
    sd['bbox_pred.bias'] = torch.randn(12, generator=g) * 0.05
    return feats, sd


def head_flat(head, feats, dtype=torch.float64):
    """Head outputs of the restatement as per-level [B, n_l] logits and [B, n_l, 4] deltas in `dtype`."""
    h = RPNHead(head['conv.weight'].shape[0], head['cls_logits.weight'].shape[0]).to(dtype)
    h.load_state_dict({k: v.to(dtype) for k, v in head.items()})
    with torch.no_grad():
        lg, dl = h([f.to(dtype) for f in feats.values()])
    B = lg[0].shape[0]
    return [flatten_head(t) for t in lg], [flatten_head(t).view(B, -1, 4) for t in dl]


def margin_report(logits, deltas, anchors, image_size, pre, nms_thresh=0.7, min_size=1e-3, delta=MARGIN):
    """Smallest distance of a same-level candidate pair's float64 IoU from the threshold, and of a candidate side from
    min_size, over the selected candidates of one image (both must exceed delta for a margin-safe case)."""
    d_iou, d_side = float('inf'), float('inf')
    for z, d, a in zip(logits, deltas, anchors):
        idx = select(z, pre)
        boxes, _, _ = candidates(z.double(), d.double(), a.double(), idx, image_size, min_size)
        iou = box_iou(boxes, boxes)
        iou = iou[~torch.isnan(iou)]
        d_iou = min(d_iou, float((iou - nms_thresh).abs().min()))
        sides = torch.cat([boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]])
        d_side = min(d_side, float((sides - min_size).abs().min()))
    return d_iou, d_side
