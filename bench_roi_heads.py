#!/usr/bin/env python
"""Timing of the box branch of roi_heads on the fused maps (reference code/helpers/model.py:346-347), DAVIS pyramid of
a 480x854 frame (image 749x1333 after torchvision's transform), one frame:

  * evaluation: `RoIHeadsInference` = BoxBranch.detect at 1000 proposals (rpn_post_nms_top_n_test) + mask RoIAlign +
    MaskBranch.predict on the detections, ms per frame                      -> roi_heads_eval_ms_per_frame
  * training: BoxBranch.forward + fastrcnn_loss + backward at 512 sampled RoIs (box_batch_size_per_image), ms per frame
                                                                            -> box_branch_train_ms_per_frame
  * fc6 alone at both shapes: time, TFLOP/s and the share of the bound DESIGN.md section 4 names for it (the MFMA rate
    of the data type; operations and bytes are computed from the shapes here)
  * as a yardstick, in the same process on the same GPU right after this package's, the same box chain in plain
    PyTorch-ROCm (F.linear, softmax, decode and a greedy NMS written with torch operations on the device; torchvision is not
    installed, so this is no torchvision timing)

    python bench_roi_heads.py [--steps 10 --warmup 3] [--precisions bf16 fp32] [--no-yardstick]

Prints ONE JSON line.  Not the headline metric (bench.py is)."""
import argparse
import json
import math
import os
import sys
import time
from collections import OrderedDict

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

IMAGE = (749, 1333)
PEAK_TFLOPS = {'bf16': 2516.6, 'fp32': 157.3}     # MI355X matrix peak (spec): the bound of fc6 at M = 512 / 1000


def proposals(n, gen, dev):
    H, W = IMAGE
    c = torch.rand(n, 2, generator=gen, device=dev) * torch.tensor([W, H], dtype=torch.float32, device=dev)
    s = 16 + torch.rand(n, 2, generator=gen, device=dev) * 400
    b = torch.cat([c - s / 2, c + s / 2], 1)
    b[:, 0::2] = b[:, 0::2].clamp(0, W)
    b[:, 1::2] = b[:, 1::2].clamp(0, H)
    return b


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.time() - t0) / steps * 1e3


def torch_decode(deltas, props):
    w, h = props[:, 2] - props[:, 0], props[:, 3] - props[:, 1]
    cx, cy = props[:, 0] + 0.5 * w, props[:, 1] + 0.5 * h
    clip = math.log(1000.0 / 16)
    dx, dy = deltas[:, 0::4] / 10, deltas[:, 1::4] / 10
    dw, dh = (deltas[:, 2::4] / 5).clamp(max=clip), (deltas[:, 3::4] / 5).clamp(max=clip)
    pcx, pcy = dx * w[:, None] + cx[:, None], dy * h[:, None] + cy[:, None]
    pw, ph = torch.exp(dw) * w[:, None], torch.exp(dh) * h[:, None]
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 2)


def torch_postprocess(logits, deltas, props, max_det):
    """postprocess_detections in torch operations on the device (one class besides the background)."""
    H, W = IMAGE
    boxes = torch_decode(deltas, props)
    boxes = torch.stack([boxes[..., 0].clamp(0, W), boxes[..., 1].clamp(0, H), boxes[..., 2].clamp(0, W),
                         boxes[..., 3].clamp(0, H)], -1)[:, 1]
    scores = F.softmax(logits, -1)[:, 1]
    ok = (scores > 0.05) & (boxes[:, 2] - boxes[:, 0] >= 1e-2) & (boxes[:, 3] - boxes[:, 1] >= 1e-2)
    boxes, scores = boxes[ok], scores[ok]
    order = scores.argsort(descending=True, stable=True)
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(b[:, None, 2:], b[None, :, 2:]) - torch.max(b[:, None, :2], b[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    over = inter / (area[:, None] + area[None] - inter) > 0.5
    n = b.shape[0]
    keep = torch.ones(n, dtype=torch.bool, device=b.device)
    later = torch.arange(n, device=b.device)
    for i in range(n):     # greedy, without reading anything back
        keep = keep & ~(over[i] & keep[i] & (later > i))
    kept = order[keep][:max_det]
    return boxes[kept], scores[kept]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precisions', nargs='+', default=['bf16', 'fp32'], choices=['bf16', 'fp32'])
    ap.add_argument('--proposals', type=int, default=1000)
    ap.add_argument('--rois', type=int, default=512)
    ap.add_argument('--no-yardstick', action='store_true')
    args = ap.parse_args()
    from sfvos_amd import BoxBranch, RoIHeadsInference, _lib, davis_pyramid, fastrcnn_loss
    from sfvos_amd.module import _ptr, _stream
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(63)
    gen = torch.Generator(device=dev).manual_seed(7)
    feats = OrderedDict((k, torch.randn((1, 256, h, w), generator=gen, device=dev)) for k, (h, w) in davis_pyramid())
    props_eval = [proposals(args.proposals, gen, dev)]
    props_train = [proposals(args.rois, gen, dev)]
    labels = [torch.randint(0, 2, (args.rois,), generator=gen, device=dev)]
    targets = [torch.randn(args.rois, 4, generator=gen, device=dev)]
    out = {'metric': 'ms per frame, box branch of roi_heads (DAVIS pyramid, %d proposals / %d sampled RoIs)'
                     % (args.proposals, args.rois), 'unit': 'ms', 'data': 'synthetic'}
    for prec in args.precisions:
        tdt = torch.bfloat16 if prec == 'bf16' else torch.float32
        dt_id = _lib.BF16 if prec == 'bf16' else _lib.F32
        heads = RoIHeadsInference(2, prec, box_detections_per_img=10).to(dev)     # model.py:187
        with torch.no_grad():
            heads.box.box_predictor.cls_score.weight.mul_(8.0)    # scores away from 0.5, boxes away from the proposals
            heads.box.box_predictor.bbox_pred.weight.mul_(8.0)
        res = {}
        ndet = []

        def eval_frame():
            ndet.append(heads(feats, props_eval, [IMAGE])[0]['boxes'].shape[0])

        def detect_only():
            heads.box.detect(feats, props_eval, [IMAGE])

        res['roi_heads_eval_ms_per_frame'] = round(timed(eval_frame, args.steps, args.warmup), 3)
        res['detect_ms_per_frame'] = round(timed(detect_only, args.steps, args.warmup), 3)
        res['detections'] = ndet[-1]
        train = BoxBranch(2, prec).to(dev)

        def train_step():
            for p in train.parameters():
                p.grad = None
            lc, lb = fastrcnn_loss(*train(feats, props_train, [IMAGE]), labels, targets)
            (lc + lb).backward()

        res['box_branch_train_ms_per_frame'] = round(timed(train_step, args.steps, args.warmup), 3)
        # fc6 alone at both shapes
        fc6 = train.box_head.fc6
        image = train.box_head._packed(fc6, dt_id, tdt, 49)
        lib = _lib.load()
        for m in (args.proposals, args.rois):
            x = torch.randn(m, 12544, generator=gen, device=dev).to(tdt)
            y = torch.empty(m, 1024, dtype=tdt, device=dev)
            nbytes = lib.sfvos_dense_workspace_bytes(dt_id, m, 1024, 12544)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)

            def run():
                _lib.call('sfvos_dense', _ptr(x), _ptr(image), _ptr(fc6.bias.detach()), _ptr(y), dt_id, m, 1024, 12544,
                          1, _ptr(ws), _stream())
            ms = timed(run, max(args.steps, 20), args.warmup)
            flop = 2.0 * m * 12544 * 1024
            es = 2 if prec == 'bf16' else 4
            res['fc6_m%d' % m] = {'ms': round(ms, 4), 'gflop': round(flop / 1e9, 2),
                                  'mbytes': round((12544 * 1024 + m * 12544 + m * 1024) * es / 1e6, 1),
                                  'splits': lib.sfvos_dense_splits(dt_id, m, 1024, 12544),
                                  'tflops': round(flop / ms / 1e9, 1),
                                  'share_of_mfma_peak': round(flop / ms / 1e9 / PEAK_TFLOPS[prec], 4)}
        if not args.no_yardstick:
            # the same box chain in plain PyTorch on the same GPU: RoI features of this package's RoIAlign (not timed)
            sd = {k: v.detach().to(tdt) for k, v in heads.box.state_dict().items()}
            with torch.no_grad():
                roi_e = heads.box.box_roi_pool(feats, props_eval, [IMAGE]).flatten(1).to(tdt)
                roi_t = train.box_roi_pool(feats, props_train, [IMAGE]).flatten(1).to(tdt)

            def chain(x, w):
                h = F.relu(F.linear(x, w['box_head.fc6.weight'], w['box_head.fc6.bias']))
                h = F.relu(F.linear(h, w['box_head.fc7.weight'], w['box_head.fc7.bias']))
                return (F.linear(h, w['box_predictor.cls_score.weight'], w['box_predictor.cls_score.bias']).float(),
                        F.linear(h, w['box_predictor.bbox_pred.weight'], w['box_predictor.bbox_pred.bias']).float())

            def torch_eval():
                with torch.no_grad():
                    lg, dl = chain(roi_e, sd)
                    torch_postprocess(lg, dl, props_eval[0], 10)

            def own_box_chain():      # the same span of this package: head, predictor, postprocess (no RoIAlign)
                with torch.no_grad():
                    lg, dl = heads.box.forward_features(roi_e.view(-1, 256, 7, 7).float())
                    heads.box.select(*heads.box.candidates(lg, dl, props_eval[0], IMAGE))

            wt = {k: v.clone().requires_grad_(True) for k, v in sd.items()}

            def torch_train():
                for p in wt.values():
                    p.grad = None
                lg, dl = chain(roi_t, wt)
                lab = labels[0]
                pos = torch.where(lab > 0)[0]
                lb = F.smooth_l1_loss(dl.view(-1, 2, 4)[pos, lab[pos]], targets[0][pos], beta=1 / 9, reduction='sum')
                (F.cross_entropy(lg, lab) + lb / lab.numel()).backward()

            roi_tf = roi_t.view(-1, 256, 7, 7).float()

            def own_train_chain():
                for p in train.parameters():
                    p.grad = None
                lc, lb = fastrcnn_loss(*train.forward_features(roi_tf), labels, targets)
                (lc + lb).backward()

            res['box_chain_eval_ms'] = {'sfvos': round(timed(own_box_chain, args.steps, args.warmup), 3),
                                        'pytorch_eager': round(timed(torch_eval, args.steps, args.warmup), 3)}
            res['box_chain_train_ms'] = {'sfvos': round(timed(own_train_chain, args.steps, args.warmup), 3),
                                         'pytorch_eager': round(timed(torch_train, args.steps, args.warmup), 3)}
        out[prec] = res
        del heads, train
    print(json.dumps(out))


if __name__ == '__main__':
    main()
