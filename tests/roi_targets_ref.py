"""Torch-core restatement of the training targets of torchvision's `roi_heads`, for the tests of sfvos_amd.roi_heads and
csrc/roi_targets.hip.  Written from torchvision's published behaviour (models/detection/roi_heads.py:
select_training_samples, add_gt_proposals, assign_targets_to_proposals, project_masks_on_boxes; _utils.py: Matcher,
BalancedPositiveNegativeSampler, BoxCoder; ops/boxes.py: box_iou; ops/roi_align.py with sampling_ratio <= 0).  torchvision
is not installed where this project builds or runs: PARITY UNPINNED BY THE REFERENCE.  Never imported by the package.

Values are float64.  What DECIDES something is fp32 in the kernels' operation order, every operation rounded on its own
(torch's CPU element-wise ops are separate IEEE operations), because a decision taken in float64 can differ from a correct
fp32 one by construction:
  * the matcher's IoU (which ground-truth box wins, on which side of a threshold it falls);
  * the geometry of the adaptive RoIAlign: bin size, grid = ceil(bin) and every sample coordinate (which two rows /
    columns a sample interpolates between, whether it lies outside).  The interpolation weights, the pixel values, the
    sums and the division are float64 on those fp32 coordinates (y - floor(y) is exact in both).
The sampler has no arithmetic: a stable sort on (NaN flag, key, index)."""
import torch

import box_branch_ref as BR


def box_iou(a, b):
    """[n,4] x [g,4] -> [n,g] in the dtype of the inputs: inter / (area_a + area_b - inter), unclamped areas,
    intersection sides clamped at 0."""
    return BR.box_iou(a, b)


def decide(max_iou, arg, gt_labels, high, low):
    """Matcher(high, low, allow_low_quality_matches=False) + assign_targets_to_proposals on a candidate's largest IoU and
    its ground-truth index -> (matched int64, labels int64): background 0, ignored -1, matched clamped at 0."""
    hit = max_iou >= high
    matched = torch.where(hit, arg, torch.zeros_like(arg))
    lab = gt_labels[matched] if gt_labels.numel() else torch.zeros_like(arg)
    labels = torch.where(hit, lab, torch.where(max_iou < low, torch.zeros_like(arg), -torch.ones_like(arg)))
    return matched, labels


def match(proposals, gt_boxes, gt_labels, high=0.5, low=0.5):
    """Candidates = proposals followed by gt_boxes.  -> dict: 'matched', 'labels' (int64), 'max_iou' (fp32, the deciding
    value: the lowest index wins a tie, a NaN never wins), 'arg' (the winning index), 'iou64' ([N,G] float64)."""
    cand = torch.cat([proposals, gt_boxes], 0).float()
    N, G = cand.shape[0], gt_boxes.shape[0]
    if G == 0:
        z = torch.zeros(N, dtype=torch.int64)
        return {'matched': z, 'labels': z.clone(), 'max_iou': torch.zeros(N), 'arg': z.clone(),
                'iou64': torch.zeros((N, 0), dtype=torch.float64)}
    iou = box_iou(cand, gt_boxes.float())
    iou = torch.where(torch.isnan(iou), torch.full_like(iou, float('-inf')), iou)
    best = iou.max(1).values
    ar = torch.arange(G).expand(N, G)
    arg = torch.where(iou == best[:, None], ar, torch.full_like(ar, G)).min(1).values
    matched, labels = decide(best, arg, gt_labels, high, low)
    return {'matched': matched, 'labels': labels, 'max_iou': best, 'arg': arg,
            'iou64': box_iou(cand.double(), gt_boxes.double())}


def sample(labels, keys, batch_size_per_image=512, positive_fraction=0.25):
    """BalancedPositiveNegativeSampler over explicit keys -> (index, pos_slot): the chosen candidates in ascending index
    and the rows among them whose label is >= 1.  Of each class the candidates with the smallest (key, index) pairs are
    chosen; a NaN key ranks behind every number."""
    pos, neg = torch.where(labels >= 1)[0], torch.where(labels == 0)[0]
    n_pos = min(pos.numel(), int(batch_size_per_image * positive_fraction))
    n_neg = min(neg.numel(), batch_size_per_image - n_pos)

    def smallest(idx, n):
        k = keys[idx].double()
        nan = torch.isnan(k)
        k = torch.where(nan, torch.zeros_like(k), k)
        o = torch.argsort(k, stable=True)
        o = o[torch.argsort(nan[o].to(torch.int64), stable=True)]
        return idx[o[:n]]
    index = torch.sort(torch.cat([smallest(pos, n_pos), smallest(neg, n_neg)])).values
    return index, torch.where(labels[index] >= 1)[0]


def encode(reference_boxes, proposals):
    return BR.encode_boxes(reference_boxes.double(), proposals.double())


def select_training_samples(proposals, gt_boxes, gt_labels, keys, batch_size_per_image=512, positive_fraction=0.25,
                            high=0.5, low=0.5):
    """One image -> dict: 'index', 'pos_slot', 'boxes' (fp32 rows of the candidate list), 'matched', 'labels' (int64),
    'regression_targets' (float64; against a box of zeros when there is no ground truth, as torchvision substitutes)."""
    m = match(proposals, gt_boxes, gt_labels, high, low)
    index, pos_slot = sample(m['labels'], keys, batch_size_per_image, positive_fraction)
    cand = torch.cat([proposals, gt_boxes], 0).float()
    gt = gt_boxes.float() if gt_boxes.shape[0] else torch.zeros((1, 4))
    boxes, matched = cand[index], m['matched'][index]
    return {'index': index, 'pos_slot': pos_slot, 'boxes': boxes, 'matched': matched, 'labels': m['labels'][index],
            'regression_targets': encode(gt[matched], boxes)}


def _axis_samples(start, extent, M, size):
    """fp32 geometry of one axis of one box -> (lo, hi, wlo, whi (float64), valid, grid)."""
    f = torch.float32
    bin_size = extent / torch.tensor(float(M), dtype=f)
    grid = int(torch.ceil(bin_size))
    p = torch.arange(M, dtype=f).repeat_interleave(grid)
    i = torch.arange(grid, dtype=f).repeat(M)
    y = (start + p * bin_size) + ((i + 0.5) * bin_size) / torch.tensor(float(grid), dtype=f)
    valid = ~((y < -1.0) | (y > float(size)))
    y = torch.where(y <= 0, torch.zeros_like(y), y)
    lo = y.to(torch.int64)
    edge = lo >= size - 1
    lo = torch.where(edge, torch.full_like(lo, size - 1), lo)
    hi = torch.where(edge, lo, lo + 1)
    y = torch.where(edge, lo.to(f), y)
    l = y.double() - lo.double()
    return lo.clamp(0, size - 1), hi.clamp(0, size - 1), 1.0 - l, l, valid, grid


def roi_align_adaptive(masks, boxes, matched, M):
    """roi_align(masks[:, None], [matched, boxes], (M, M), 1.0, sampling_ratio=-1, aligned=False)[:, 0] -> ([P,M,M]
    float64, grids [P,2] = (grid_h, grid_w)).  Rules of bilinear_interpolate: a sample with y < -1, y > H, x < -1 or
    x > W adds 0; coordinates clamp at 0; the last row / column interpolates with itself."""
    G, H, W = masks.shape
    mk = masks.double()
    one = torch.tensor(1.0)
    out, grids = [], []
    for box, g in zip(boxes.float(), matched.tolist()):
        rw, rh = torch.maximum(box[2] - box[0], one), torch.maximum(box[3] - box[1], one)
        ylo, yhi, wyl, wyh, vy, gh = _axis_samples(box[1], rh, M, H)
        xlo, xhi, wxl, wxh, vx, gw = _axis_samples(box[0], rw, M, W)
        f = mk[g]
        val = (wyl[:, None] * wxl[None, :]) * f[ylo[:, None], xlo[None, :]] + \
              (wyl[:, None] * wxh[None, :]) * f[ylo[:, None], xhi[None, :]] + \
              (wyh[:, None] * wxl[None, :]) * f[yhi[:, None], xlo[None, :]] + \
              (wyh[:, None] * wxh[None, :]) * f[yhi[:, None], xhi[None, :]]
        val = val * (vy[:, None] & vx[None, :]).double()
        out.append(val.reshape(M, gh, M, gw).sum((1, 3)) / float(max(gh * gw, 1)))
        grids.append((gh, gw))
    if not out:
        return torch.zeros((0, M, M), dtype=torch.float64), torch.zeros((0, 2), dtype=torch.int64)
    return torch.stack(out), torch.tensor(grids)


def project_masks_on_boxes(gt_masks, boxes, matched_idxs, M):
    return roi_align_adaptive(gt_masks, boxes, matched_idxs, M)[0]
