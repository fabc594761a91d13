"""Torch-core restatement of the training call of torchvision's RegionProposalNetwork, for the tests of
csrc/rpn_targets.hip and of sfvos_amd.RegionProposalNetwork.compute_loss.  Written from torchvision's published behaviour
(models/detection/rpn.py: assign_targets_to_anchors, compute_loss; _utils.py: Matcher with allow_low_quality_matches and
set_low_quality_matches_, BalancedPositiveNegativeSampler, BoxCoder(1, 1, 1, 1).encode; ops/boxes.py: box_iou).
torchvision is not installed where this project builds or runs: PARITY UNPINNED BY THE REFERENCE.  Never imported by the
package.

Values are float64.  What DECIDES something is fp32 in the kernels' operation order, every operation rounded on its own
(torch's CPU element-wise ops are separate IEEE operations): the IoU, which ground-truth box wins, the side of a threshold
it falls on, and the equality with `highest` of the low-quality rule.  The sampler has no arithmetic: a stable sort on
(NaN flag, key, index), the idea of roi_targets_ref.sample.

Anchor order: torchvision's per-image concatenation (level, h, w, a)."""
import torch

import rpn_ref as R

SMALL = (R.SHAPES, R.TENSOR)                                          # 3825 anchors
LARGE = ([(96, 160), (48, 80), (24, 40), (12, 20)], (384, 640))      # 61 200 anchors: several workgroups per image
DAVIS = ([(192, 336), (96, 168), (48, 84), (24, 42), (12, 21)], (768, 1344))      # 257 796 anchors, five levels
PYRAMIDS = {'small': SMALL, 'large': LARGE, 'davis': DAVIS}
ANCHOR_SIZES = {'small': (R.SIZES, R.RATIOS), 'large': (R.SIZES, R.RATIOS), 'davis': (R.DEFAULT_SIZES, R.DEFAULT_RATIOS)}
# three quarter-pixel boxes of the DAVIS frame (areas and their sums stay below 2^24 sixteenths: the IoU is exact)
CASE_DAVIS = [[100.5, 80.25, 420.0, 400.75], [600.0, 150.5, 1100.25, 600.0], [820.25, 300.0, 870.5, 360.75]]
HIGH, LOW = 0.7, 0.3
MARGIN = R.MARGIN

# ground truth on quarter-pixel coordinates (anchors are integers): every area and intersection is exact in fp32
CASE_A = [[10.25, 12.5, 70.75, 60.25], [80., 20., 150.5, 90.25], [30.25, 40.5, 41.75, 52.25]]
CASE_B = [[50.25, 50.25, 53.5, 54.75]]
CASE_C = [[16 * x + .25, 16 * y + .5, 16 * x + 32.75, 16 * y + 31.25] for y in range(4) for x in range(8)]
CASE_D = [[0., 0., 160., 96.]]
CASE_E = [[40.25, 50.5, 280.75, 240.25], [320., 80., 600.5, 360.25], [120.25, 160.5, 131.75, 172.25]]
CASE_F = [CASE_E[0], [700., 700., 710.5, 712.25]]
# name -> (pyramid, ground truth, expected (pos at >= 0.7, pos after the low-quality rule, neg, ignored); None = not stated)
CASES = {'a': ('small', CASE_A, (7, 49, 3383, 393)), 'b': ('small', CASE_B, (0, 110, None, None)),
         'c': ('small', CASE_C, (160, None, None, None)), 'd': ('small', CASE_D, (3, None, None, None)),
         'e': ('large', CASE_E, (5, 39, 60773, None)), 'f': ('large', CASE_F, (None, 61200, 0, None))}


def anchors(shapes, tensor_size, sizes=R.SIZES, ratios=R.RATIOS):
    """[N, 4] fp32 anchors of one image in (level, h, w, a) order; strides = tensor_size // (H, W)."""
    out = []
    for (H, W), base in zip(shapes, R.base_anchors(sizes, ratios)):
        sh, sw = tensor_size[0] // H, tensor_size[1] // W
        ys, xs = torch.arange(H, dtype=torch.int64) * sh, torch.arange(W, dtype=torch.int64) * sw
        sy, sx = torch.meshgrid(ys, xs, indexing='ij')
        shifts = torch.stack([sx, sy, sx, sy], -1).reshape(-1, 1, 4).float()
        out.append((shifts + base.view(1, -1, 4)).reshape(-1, 4))
    return torch.cat(out, 0)


def box_iou(a, b):
    """[n,4] x [g,4] -> [n,g] in the dtype of the inputs: inter / ((area_a + area_b) - inter), unclamped areas,
    intersection sides clamped at 0."""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.min(a[:, None, 2], b[None, :, 2]) - torch.max(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    h = (torch.min(a[:, None, 3], b[None, :, 3]) - torch.max(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = w * h
    return inter / ((area_a[:, None] + area_b[None]) - inter)


def match(anc, gt, high=HIGH, low=LOW, allow_low_quality=True):
    """Matcher + the labels of assign_targets_to_anchors -> dict: 'labels' (1 / 0 / -1), 'matched' (the ground-truth index
    of a positive, 0 elsewhere: Matcher's -1 / -2 clamped), 'max_iou' (fp32, the deciding value: the lowest index wins a
    tie, a NaN never wins), 'pos_high' (positives before the low-quality rule), 'iou64' [N, G]."""
    anc, gt = anc.float(), gt.float().reshape(-1, 4)
    N, G = anc.shape[0], gt.shape[0]
    if G == 0:
        z = torch.zeros(N, dtype=torch.int64)
        return {'labels': z, 'matched': z.clone(), 'max_iou': torch.zeros(N), 'pos_high': 0,
                'iou64': torch.zeros((N, 0), dtype=torch.float64)}
    iou = box_iou(anc, gt)
    iou = torch.where(torch.isnan(iou), torch.full_like(iou, float('-inf')), iou)
    best = iou.max(1).values
    ar = torch.arange(G).expand(N, G)
    arg = torch.where(iou == best[:, None], ar, torch.full_like(ar, G)).min(1).values
    hit = best >= high
    labels = torch.where(hit, 1, torch.where(best < low, 0, -1))
    matched = torch.where(hit, arg, torch.zeros_like(arg))
    pos_high = int(hit.sum())
    if allow_low_quality:
        # set_low_quality_matches_: every anchor that reaches the best IoU some ground-truth box has with any anchor
        highest = iou.max(0).values
        lq = ((iou == highest[None]) & (iou > float('-inf'))).any(1)
        labels = torch.where(lq, torch.ones_like(labels), labels)
        matched = torch.where(lq, arg, matched)
    return {'labels': labels, 'matched': matched, 'max_iou': best, 'pos_high': pos_high,
            'iou64': box_iou(anc.double(), gt.double())}


def margin_safe(iou64, high=HIGH, low=LOW, allow_low_quality=True, margin=MARGIN):
    """[N] bool: the anchor's largest float64 IoU is farther than `margin` from both thresholds, and its gap to `highest`
    of every ground-truth box is exactly 0 or larger than margin."""
    best = iou64.max(1).values
    safe = ((best - high).abs() > margin) & ((best - low).abs() > margin)
    if allow_low_quality:
        gap = iou64.max(0).values[None] - iou64
        safe &= ((gap == 0) | (gap > margin)).all(1)
    return safe


def real_case(pyramid, seed, G):
    """(anchors, gt [G, 4] fp32): real-valued ground truth inside the tensor, sides from 8 px to half the tensor."""
    shapes, tensor = PYRAMIDS[pyramid]
    g = torch.Generator().manual_seed(4000 + seed)
    th, tw = float(tensor[0]), float(tensor[1])
    wh = 8 + torch.rand(G, 2, generator=g) * torch.tensor([tw / 2 - 8, th / 2 - 8])
    xy = torch.rand(G, 2, generator=g) * (torch.tensor([tw, th]) - wh)
    return anchors(shapes, tensor, *ANCHOR_SIZES[pyramid]), torch.cat([xy, xy + wh], 1).float()


# (pyramid, seed, G) of the real-valued match cases: picked on the CPU, the restatement alone leaves out at most 0.5 % of
# the anchors of each (tests/test_rpn_loss_ref_cpu.py asserts the share)
REAL_CASES = [('small', 0, 3), ('small', 1, 65), ('large', 2, 3), ('large', 3, 20)]
MAX_UNSAFE_SHARE = 0.005


def quarter_pixel_gt(pyramid, G, seed):
    """G random boxes on the quarter-pixel grid inside the tensor."""
    _, tensor = PYRAMIDS[pyramid]
    g = torch.Generator().manual_seed(5000 + seed)
    wh = torch.stack([torch.randint(16, 2 * tensor[1], (G,), generator=g),
                      torch.randint(16, 2 * tensor[0], (G,), generator=g)], 1)
    lim = torch.tensor([4 * tensor[1], 4 * tensor[0]]) - wh
    xy = (torch.rand(G, 2, generator=g) * lim).floor()
    return (torch.cat([xy, xy + wh], 1) / 4).float()


def sample(labels, keys, batch_size_per_image=256, positive_fraction=0.5):
    """BalancedPositiveNegativeSampler over explicit keys -> (pos, neg): the chosen anchors of each class in ascending
    index.  Of each class the anchors with the smallest (key, index) pairs are chosen; -0 == +0; a NaN key ranks behind
    every number; label -1 is never chosen."""
    pos, neg = torch.where(labels >= 1)[0], torch.where(labels == 0)[0]
    n_pos = min(pos.numel(), int(batch_size_per_image * positive_fraction))
    n_neg = min(neg.numel(), batch_size_per_image - n_pos)

    def smallest(idx, n):
        k = keys[idx].double()
        nan = torch.isnan(k)
        k = torch.where(nan, torch.zeros_like(k), k)
        o = torch.argsort(k, stable=True)
        o = o[torch.argsort(nan[o].to(torch.int64), stable=True)]
        return torch.sort(idx[o[:n]]).values
    return smallest(pos, n_pos), smallest(neg, n_neg)


def encode(reference_boxes, anc):
    """BoxCoder(1, 1, 1, 1).encode_single in float64."""
    g, p = reference_boxes.double(), anc.double()
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    pcx, pcy = p[:, 0] + 0.5 * pw, p[:, 1] + 0.5 * ph
    gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    gcx, gcy = g[:, 0] + 0.5 * gw, g[:, 1] + 0.5 * gh
    return torch.stack([(gcx - pcx) / pw, (gcy - pcy) / ph, torch.log(gw / pw), torch.log(gh / ph)], 1)


def encode_allowance(reference_boxes, anc, trans):
    """Per-element allowance of an encoded target, the one tests/test_gpu_roi_targets_kernels.py uses for
    sfvos_roi_sample with weights (1, 1, 1, 1): `trans` times the magnitudes of the terms."""
    r, p = reference_boxes.double(), anc.double()
    want = encode(r, p)
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gcx, gcy = (r[:, 0] + r[:, 2]).abs() / 2, (r[:, 1] + r[:, 3]).abs() / 2
    pcx, pcy = (p[:, 0] + p[:, 2]).abs() / 2, (p[:, 1] + p[:, 3]).abs() / 2
    return trans * torch.stack([(gcx + pcx) / pw, (gcy + pcy) / ph, want[:, 2].abs() + 1, want[:, 3].abs() + 1], 1)


def bce_with_logits(x, z):
    """max(x, 0) - x z + log1p(exp(-|x|)) in float64, and the magnitude of its terms."""
    x, z = x.double(), z.double()
    soft = torch.log1p(torch.exp(-x.abs()))
    return x.clamp(min=0) - x * z + soft, x.clamp(min=0) + (x * z).abs() + soft


def smooth_l1(d, beta):
    """torch's smooth_l1_loss of the differences d in float64 (beta = 0: |d|), and the magnitude of its terms."""
    d = d.double()
    a = d.abs()
    if beta == 0:
        return a, a
    return torch.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta), torch.where(a < beta, 0.5 * d * d / beta,
                                                                                  a + 0.5 * beta)


def loss_terms(logits, deltas, index, n_pos, targets, beta):
    """One image: logits [N], deltas [N, 4], index = its sampled anchors (the n_pos positives first), targets [n_pos, 4]
    -> (bce [S], box [S] (0 for a negative), magnitude of bce, magnitude of box) in float64."""
    x = logits.double()[index]
    z = (torch.arange(index.numel()) < n_pos).double()
    bce, bce_mag = bce_with_logits(x, z)
    box, box_mag = torch.zeros_like(bce), torch.zeros_like(bce)
    if n_pos:
        v, m = smooth_l1(deltas.double()[index[:n_pos]] - targets.double(), beta)
        box[:n_pos], box_mag[:n_pos] = v.sum(1), m.sum(1)
    return bce, box, bce_mag, box_mag


def per_image(obj, dl, shapes, batch, A=3):
    """Head outputs in the pyramid's level-major storage, objectness [P, A] and deltas [P, 4A] -> ([B, N], [B, N, 4]) in
    the anchor order of an image."""
    lg, dd, off = [], [], 0
    for H, W in shapes:
        n = batch * H * W
        lg.append(obj[off:off + n].reshape(batch, H * W * A))
        dd.append(dl[off:off + n].reshape(batch, H * W * A, 4))
        off += n
    return torch.cat(lg, 1), torch.cat(dd, 1)


def rpn_losses(logits, deltas, anc, gt_boxes, keys, batch_size_per_image=256, positive_fraction=0.5, beta=1.0 / 9,
               high=HIGH, low=LOW):
    """compute_loss of torchvision's RPN on explicit keys.  logits [B, N], deltas [B, N, 4], gt_boxes and keys: one tensor
    per image -> dict: 'loss_objectness', 'loss_rpn_box_reg' (float64), 'counts' [(S, P)], 'index', and the per-term
    magnitudes 'bce_mag', 'box_mag' and 'target_allow' (per positive row: the summed allowance of its four targets at
    trans = 1) from which a test derives its bound."""
    sums, counts, index, mags, allow = [0.0, 0.0], [], [], [[], []], []
    for b, (gt, k) in enumerate(zip(gt_boxes, keys)):
        gt = gt.float().reshape(-1, 4)
        m = match(anc, gt, high, low, True)
        pos, neg = sample(m['labels'], k, batch_size_per_image, positive_fraction)
        idx = torch.cat([pos, neg])
        ref = gt[m['matched'][pos]] if gt.shape[0] else torch.zeros((pos.numel(), 4))
        tgt = encode(ref, anc[pos])
        bce, box, bm, xm = loss_terms(logits[b], deltas[b], idx, pos.numel(), tgt, beta)
        sums[0] += float(bce.sum()); sums[1] += float(box.sum())
        counts.append((idx.numel(), pos.numel())); index.append(idx)
        mags[0].append(bm); mags[1].append(xm)
        allow.append(encode_allowance(ref, anc[pos], 1.0).sum(1))
    s_tot = sum(s for s, _ in counts)
    nan = float('nan')
    return {'loss_objectness': sums[0] / s_tot if s_tot else nan, 'loss_rpn_box_reg': sums[1] / s_tot if s_tot else nan,
            'counts': counts, 'index': index, 'bce_mag': torch.cat(mags[0]), 'box_mag': torch.cat(mags[1]),
            'target_allow': torch.cat(allow), 's_tot': s_tot}
