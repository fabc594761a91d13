#!/usr/bin/env python
"""Timing of the training targets of roi_heads (reference code/helpers/model.py:346 with targets), one DAVIS frame
(image 749x1333 after torchvision's transform): 2000 proposals (rpn_post_nms_top_n_train), 3 ground-truth objects with
uint8 masks, 512 sampled RoIs (box_batch_size_per_image), 128 of them positive.

  * `select_training_samples` + `project_masks_on_boxes`, ms per frame        -> roi_heads_train_targets_ms_per_frame
    (device-event medians; the first includes its one device-to-host copy of the counts), and the three entry points
    alone through the C ABI
  * the full `RoIHeads` training forward + backward on the DAVIS pyramid, bf16 and fp32
  * as a yardstick, in the same process on the same GPU right after this package's, the same target computation in plain
    PyTorch-ROCm operations (concatenation, IoU matrix, max, randperm sampler, BoxCoder.encode, and the adaptive RoIAlign
    as gathers over a [P, M, grid_h, M, grid_w] sample lattice padded to the largest grid) -- what a user of the package
    had to write before; torchvision is not installed, so this is no torchvision timing

    python bench_roi_train.py [--steps 20 --warmup 5] [--precisions bf16 fp32] [--no-yardstick]

Prints ONE JSON line.  Not the headline metric (bench.py is)."""
import argparse
import json
import os
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

IMAGE = (749, 1333)
GT = [[100., 80., 520., 600.], [640., 150., 1180., 630.], [900., 40., 1090., 320.]]
M = 28


def scene(n, gen, dev):
    """n proposals: three quarters jittered around the three objects, the rest anywhere; elliptic uint8 masks."""
    H, W = IMAGE
    gt = torch.tensor(GT, device=dev)
    src = gt[torch.randint(0, 3, (n,), generator=gen, device=dev)]
    side = (src[:, 2:] - src[:, :2]).repeat(1, 2)
    near = src + torch.randn(n, 4, generator=gen, device=dev) * 0.15 * side
    c = torch.rand(n, 2, generator=gen, device=dev) * torch.tensor([W, H], dtype=torch.float32, device=dev)
    s = 16 + torch.rand(n, 2, generator=gen, device=dev) * 400
    far = torch.cat([c - s / 2, c + s / 2], 1)
    props = torch.where((torch.arange(n, device=dev) % 4 == 3)[:, None], far, near)
    props = torch.cat([torch.minimum(props[:, :2], props[:, 2:] - 2), props[:, 2:]], 1)
    props[:, 0::2] = props[:, 0::2].clamp(0, W)
    props[:, 1::2] = props[:, 1::2].clamp(0, H)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev).float(), torch.arange(W, device=dev).float(), indexing='ij')
    masks = torch.stack([(((xx - (b[0] + b[2]) / 2) / ((b[2] - b[0]) / 2)) ** 2 +
                          ((yy - (b[1] + b[3]) / 2) / ((b[3] - b[1]) / 2)) ** 2) < 1 for b in gt]).to(torch.uint8)
    return props, {'boxes': gt, 'labels': torch.ones(3, dtype=torch.int64, device=dev), 'masks': masks}


def event_median(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return round(ts[len(ts) // 2], 4)


# ---- the yardstick: torchvision's algorithm in torch operations on the device ------------------------------------------------

def eager_select(props, target, batch, fraction):
    gt, gl = target['boxes'], target['labels']
    cand = torch.cat([props, gt], 0)
    area_a = (cand[:, 2] - cand[:, 0]) * (cand[:, 3] - cand[:, 1])
    area_b = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    wh = (torch.min(cand[:, None, 2:], gt[None, :, 2:]) - torch.max(cand[:, None, :2], gt[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = inter / (area_a[:, None] + area_b[None] - inter)
    vals, matched = iou.max(1)
    labels = torch.where(vals >= 0.5, gl[matched], torch.zeros_like(matched))
    matched = torch.where(vals >= 0.5, matched, torch.zeros_like(matched))
    pos, neg = torch.where(labels >= 1)[0], torch.where(labels == 0)[0]
    n_pos = min(pos.numel(), int(batch * fraction))
    n_neg = min(neg.numel(), batch - n_pos)
    pos = pos[torch.randperm(pos.numel(), device=pos.device)[:n_pos]]
    neg = neg[torch.randperm(neg.numel(), device=neg.device)[:n_neg]]
    keep = torch.zeros_like(labels, dtype=torch.bool)
    keep[pos] = True
    keep[neg] = True
    idx = torch.where(keep)[0]
    boxes, m, lab = cand[idx], matched[idx], labels[idx]
    g = gt[m]
    pw, ph = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    pcx, pcy = boxes[:, 0] + 0.5 * pw, boxes[:, 1] + 0.5 * ph
    gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    gcx, gcy = g[:, 0] + 0.5 * gw, g[:, 1] + 0.5 * gh
    reg = torch.stack([10 * (gcx - pcx) / pw, 10 * (gcy - pcy) / ph, 5 * torch.log(gw / pw), 5 * torch.log(gh / ph)], 1)
    return boxes, m, lab, reg


def _eager_axis(start, extent, size, gmax):
    dev = start.device
    bin_ = extent / M
    grid = torch.ceil(bin_)
    p = torch.arange(M, device=dev, dtype=torch.float32)[None, :, None]
    i = torch.arange(gmax, device=dev, dtype=torch.float32)[None, None, :]
    y = start[:, None, None] + p * bin_[:, None, None] + (i + 0.5) * bin_[:, None, None] / grid[:, None, None]
    valid = (i < grid[:, None, None]) & ~((y < -1.0) | (y > float(size)))
    y = y.clamp(min=0)
    lo = y.long()
    edge = lo >= size - 1
    lo = torch.where(edge, torch.full_like(lo, size - 1), lo)
    hi = torch.where(edge, lo, lo + 1)
    y = torch.where(edge, lo.float(), y)
    l = y - lo.float()
    v = valid.float()
    return lo, hi, (1 - l) * v, l * v, grid


def eager_mask_targets(masks, boxes, matched):
    """roi_align(masks[:, None].float(), [matched, boxes], (M, M), 1.0, -1)[:, 0], every bin padded to the largest grid."""
    G, H, W = masks.shape
    f = masks.float()
    rw, rh = (boxes[:, 2] - boxes[:, 0]).clamp(min=1), (boxes[:, 3] - boxes[:, 1]).clamp(min=1)
    gh_max, gw_max = int(torch.ceil(rh / M).max()), int(torch.ceil(rw / M).max())
    ylo, yhi, wyl, wyh, gh = _eager_axis(boxes[:, 1], rh, H, gh_max)     # [P, M, gh_max]
    xlo, xhi, wxl, wxh, gw = _eager_axis(boxes[:, 0], rw, W, gw_max)
    mi = matched[:, None, None, None, None]
    Y = lambda t: t[:, :, :, None, None]     # noqa: E731
    X = lambda t: t[:, None, None, :, :]     # noqa: E731
    val = Y(wyl) * X(wxl) * f[mi, Y(ylo), X(xlo)] + Y(wyl) * X(wxh) * f[mi, Y(ylo), X(xhi)] + \
        Y(wyh) * X(wxl) * f[mi, Y(yhi), X(xlo)] + Y(wyh) * X(wxh) * f[mi, Y(yhi), X(xhi)]
    return val.sum((2, 4)) / (gh * gw).clamp(min=1)[:, None, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--precisions', nargs='+', default=['bf16', 'fp32'], choices=['bf16', 'fp32'])
    ap.add_argument('--proposals', type=int, default=2000)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--no-yardstick', action='store_true')
    args = ap.parse_args()
    from sfvos_amd import RoIHeads, _lib, davis_pyramid, project_masks_on_boxes, select_training_samples
    from sfvos_amd._lib import _ptr, _stream
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    _lib.check(_lib.load().sfvos_check_device(), 'sfvos_check_device')
    torch.manual_seed(63)
    gen = torch.Generator(device=dev).manual_seed(7)
    props, target = scene(args.proposals, gen, dev)
    N, G, batch = args.proposals + 3, 3, args.batch
    keys = [torch.rand(N, generator=gen, device=dev)]
    out = {'metric': 'roi_heads_train_targets_ms_per_frame', 'unit': 'ms', 'data': 'synthetic',
           'setting': '%d proposals, G = 3, %dx%d uint8 masks, %d sampled' % ((args.proposals,) + IMAGE + (batch,))}
    state = {}

    def own_select():
        state['sel'] = select_training_samples([props], [target], keys, batch_size_per_image=batch)

    t_sel = event_median(own_select, args.steps, args.warmup)
    labels = state['sel'][2][0]
    pos = torch.where(labels > 0)[0]                 # the selection of the positives is outside both timed regions
    own_pb, own_pm = state['sel'][0][0][pos].contiguous(), state['sel'][1][0][pos].contiguous()

    def own_masks():
        state['mt'] = project_masks_on_boxes(target['masks'], own_pb, own_pm, M)

    t_mask = event_median(own_masks, args.steps, args.warmup)
    out['sampled'], out['positives'] = int(labels.numel()), int((labels > 0).sum())
    out['value'] = round(t_sel + t_mask, 4)
    out['select_training_samples_ms'], out['project_masks_on_boxes_ms'] = t_sel, t_mask
    # the entry points alone
    lib = _lib.load()
    i32 = dict(dtype=torch.int32, device=dev)
    matched, lab = torch.empty(N, **i32), torch.empty(N, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.sfvos_roi_sample_workspace_bytes(N), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, **i32)
    o = (torch.empty(batch, **i32), torch.empty((batch, 4), device=dev), torch.empty(batch, dtype=torch.int64, device=dev),
         torch.empty(batch, **i32), torch.empty((batch, 4), device=dev), torch.empty(batch, **i32))
    gt, gl = target['boxes'], target['labels']

    def k_match():
        _lib.call('sfvos_roi_match', _ptr(props), N - G, _ptr(gt), _ptr(gl), G, 0.5, 0.5, _ptr(matched), _ptr(lab), None,
                  _stream())

    def k_sample():
        _lib.call('sfvos_roi_sample', _ptr(lab), _ptr(matched), _ptr(keys[0]), _ptr(props), N - G, _ptr(gt), G, batch, 0.25,
                  10.0, 10.0, 5.0, 5.0, _ptr(ws), _ptr(counts), *([_ptr(t) for t in o] + [_stream()]))

    mb = state['sel'][0][0][torch.where(labels > 0)[0]].contiguous()
    mm = state['sel'][1][0][torch.where(labels > 0)[0]].to(torch.int32).contiguous()
    mt = torch.empty((mb.shape[0], M, M), device=dev)

    def k_masks():
        _lib.call('sfvos_mask_targets', _ptr(target['masks']), 1, G, IMAGE[0], IMAGE[1], _ptr(mb), _ptr(mm), mb.shape[0], M,
                  _ptr(mt), _stream())

    out['entry_points_ms'] = {'sfvos_roi_match': event_median(k_match, args.steps, args.warmup),
                              'sfvos_roi_sample': event_median(k_sample, args.steps, args.warmup),
                              'sfvos_mask_targets': event_median(k_masks, args.steps, args.warmup)}
    if not args.no_yardstick:
        def eager_sel():
            state['esel'] = eager_select(props, target, batch, 0.25)

        e_sel = event_median(eager_sel, args.steps, args.warmup)
        eb, em, elb, _ = state['esel']
        epos = torch.where(elb > 0)[0]
        eager_pb, eager_pm = eb[epos].contiguous(), em[epos].contiguous()

        def eager_masks():
            state['emt'] = eager_mask_targets(target['masks'], eager_pb, eager_pm)

        e_mask = event_median(eager_masks, args.steps, args.warmup)
        # same inputs -> same targets: the eager lattice on this package's sample
        check = eager_mask_targets(target['masks'], mb, mm.long())
        out['pytorch_eager'] = {'value': round(e_sel + e_mask, 4), 'select_training_samples_ms': e_sel,
                                'project_masks_on_boxes_ms': e_mask,
                                'note': 'the eager RoIAlign gathers a [P, 28, grid_h_max, 28, grid_w_max] lattice padded to '
                                        'the largest grid of the batch (one read-back for the two maxima): simple to write, '
                                        'not the fastest eager form; both sides get the positives already selected',
                                'max_abs_difference_of_the_mask_targets': float((check - state['mt']).abs().max())}
    # the whole training step of roi_heads
    feats = OrderedDict((k, torch.randn((1, 256, h, w), generator=gen, device=dev)) for k, (h, w) in davis_pyramid())
    for prec in args.precisions:
        heads = RoIHeads(2, prec, box_batch_size_per_image=batch).to(dev)

        def train_step():
            for p in heads.parameters():
                p.grad = None
            _, losses = heads(feats, [props], [IMAGE], [target], keys)
            sum(losses.values()).backward()

        out['roi_heads_train_step_ms_' + prec] = event_median(train_step, max(args.steps // 2, 3), max(args.warmup // 2, 2))
        del heads
    print(json.dumps(out))


if __name__ == '__main__':
    main()
