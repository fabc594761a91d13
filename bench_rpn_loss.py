#!/usr/bin/env python
"""Timing of the RPN training call's loss chain (reference code/helpers/model.py:329-335 with targets; the two losses
enter total_loss at :361-368) on the DAVIS pyramid (192x336 ... 12x21, batch tensor 768x1344, 257 796 anchors), one
frame with 3 ground-truth boxes, 256 sampled anchors:

  * per entry point (device events around each call, median): sfvos_rpn_match (both launches of the low-quality rule),
    sfvos_rpn_sample (five histogram launches, gather, emit), sfvos_rpn_loss
  * the whole chain `RegionProposalNetwork.compute_loss` with explicit keys           -> rpn_losses_ms_per_frame
  * the same computation in plain PyTorch operations in the same process, on anchors that are already in memory: IoU
    matrix, two max, where, randperm, gathers, binary_cross_entropy_with_logits, smooth_l1_loss

    python bench_rpn_loss.py [--steps 30 --warmup 5]

Prints ONE JSON line.  Not the headline metric (bench.py is)."""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from bench_rpn import TENSOR, median_ms  # noqa: E402

GT = [[100.5, 80.25, 420.0, 400.75], [600.0, 150.5, 1100.25, 600.0], [820.25, 300.0, 870.5, 360.75]]
BATCH, FRACTION, HIGH, LOW, BETA = 256, 0.5, 0.7, 0.3, 1.0 / 9


def eager_chain(anchors, gt, obj, dl):
    """torchvision's assign_targets_to_anchors + sampler + compute_loss in PyTorch operations (one image)."""
    area_a = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    area_g = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    wh = (torch.min(gt[:, None, 2:], anchors[None, :, 2:]) - torch.max(gt[:, None, :2], anchors[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = inter / (area_g[:, None] + area_a[None] - inter)                  # [G, N]
    best, matches = iou.max(0)
    all_matches = matches.clone()
    matches = torch.where(best < LOW, torch.full_like(matches, -1), matches)
    matches = torch.where((best >= LOW) & (best < HIGH), torch.full_like(matches, -2), matches)
    highest = iou.max(1).values
    lq = torch.where(iou == highest[:, None])[1]
    matches[lq] = all_matches[lq]
    labels = (matches >= 0).float()
    labels = torch.where(matches == -1, torch.zeros_like(labels), labels)
    labels = torch.where(matches == -2, torch.full_like(labels, -1.0), labels)
    matched_gt = gt[matches.clamp(min=0)]
    pos, neg = torch.where(labels >= 1)[0], torch.where(labels == 0)[0]
    n_pos = min(pos.numel(), int(BATCH * FRACTION))
    n_neg = min(neg.numel(), BATCH - n_pos)
    pos = pos[torch.randperm(pos.numel(), device=pos.device)[:n_pos]]
    neg = neg[torch.randperm(neg.numel(), device=neg.device)[:n_neg]]
    idx = torch.cat([pos, neg])
    a, g = anchors[pos], matched_gt[pos]
    aw, ah, gw, gh = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    tgt = torch.stack([(g[:, 0] + 0.5 * gw - a[:, 0] - 0.5 * aw) / aw, (g[:, 1] + 0.5 * gh - a[:, 1] - 0.5 * ah) / ah,
                       torch.log(gw / aw), torch.log(gh / ah)], 1)
    box = F.smooth_l1_loss(dl[pos], tgt, beta=BETA, reduction='sum') / idx.numel()
    return F.binary_cross_entropy_with_logits(obj[idx], labels[idx]), box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    from sfvos_amd import RegionProposalNetwork, _lib, davis_pyramid
    from sfvos_amd._lib import _ptr, _stream
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    _lib.check(lib.sfvos_check_device(), 'sfvos_check_device')
    gen = torch.Generator(device=dev).manual_seed(11)
    shapes = [hw for _, hw in davis_pyramid()]
    A, B = 3, 1
    N = A * sum(h * w for h, w in shapes)
    rpn = RegionProposalNetwork(batch_size_per_image=BATCH, positive_fraction=FRACTION, fg_iou_thresh=HIGH,
                                bg_iou_thresh=LOW, smooth_l1_beta=BETA).to(dev).train()
    obj = torch.randn((N // A, A), generator=gen, device=dev) * 3
    dl = torch.randn((N // A, 4 * A), generator=gen, device=dev) * 0.3
    gt = torch.tensor(GT, device=dev)
    keys = torch.rand(N, generator=gen, device=dev)
    targets = [dict(boxes=gt)]
    pyr = _lib.make_pyramid(shapes)
    base = rpn.anchor_generator.device_table(dev)
    anchor_args = (ctypes.byref(pyr), A, _ptr(base), TENSOR[0], TENSOR[1])
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    ws = torch.empty(lib.sfvos_rpn_targets_workspace_bytes(ctypes.byref(pyr), A, 3, BATCH), dtype=torch.uint8, device=dev)
    labels, matched = torch.empty(N, **i32), torch.empty(N, **i32)
    counts, index, reg = torch.empty((B, 2), **i32), torch.empty((B, BATCH), **i32), torch.empty((B, BATCH, 4), **f32)
    out = torch.empty(2, **f32)

    def match():
        _lib.call('sfvos_rpn_match', *anchor_args, _ptr(gt), 3, HIGH, LOW, 1, _ptr(ws), _ptr(matched), _ptr(labels), None,
                  _stream())

    def sample():
        _lib.call('sfvos_rpn_sample', _ptr(labels), _ptr(matched), _ptr(keys), N, *anchor_args, _ptr(gt), 3, BATCH,
                  FRACTION, _ptr(ws), _ptr(counts), _ptr(index), _ptr(reg), _stream())

    def loss():
        _lib.call('sfvos_rpn_loss', _ptr(obj), _ptr(dl), ctypes.byref(pyr), B, A, _ptr(index), _ptr(counts), _ptr(reg),
                  BATCH, BETA, None, _ptr(out), _stream())

    def chain():
        return rpn.compute_loss(obj, dl, shapes, B, TENSOR, targets, [keys])

    anchors = torch.cat([a.to(dev) for a in rpn.anchor_generator.grid_anchors(shapes, TENSOR)], 0)
    obj_img, dl_img = obj.reshape(-1), dl.reshape(-1, 4)       # B = 1: the level-major storage is the image's order

    def eager():
        return eager_chain(anchors, gt, obj_img, dl_img)

    with torch.no_grad():
        want = {k: float(v) for k, v in chain().items()}
        ms = median_ms([match, sample, loss, chain, eager], args.steps, args.warmup)
        again = {k: float(v) for k, v in chain().items()}
        eg = [float(v) for v in eager()]
    r = dict(zip(['match', 'sample', 'loss', 'compute_loss', 'torch_eager_ops'], ms))
    res = {'metric': 'rpn_losses_ms_per_frame', 'unit': 'ms', 'data': 'synthetic', 'value': r['compute_loss'],
           'what': 'RPN anchor targets + sampler + losses, DAVIS pyramid %s, tensor %dx%d, %d anchors, 3 ground-truth '
                   'boxes, %d sampled, one frame' % (shapes, TENSOR[0], TENSOR[1], N, BATCH),
           'entry_points_ms': {k: r[k] for k in ('match', 'sample', 'loss')},
           'rpn_losses_ms_per_frame': r['compute_loss'], 'torch_eager_ops_ms': r['torch_eager_ops'],
           'sampled': counts.cpu().tolist(), 'losses': want, 'losses_equal_from_run_to_run': again == want,
           'torch_eager_losses_other_sample': eg}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
