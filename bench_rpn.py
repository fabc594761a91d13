#!/usr/bin/env python
"""Timing of the region proposal network (reference code/helpers/model.py:236-240, called at :329-335) on the DAVIS
pyramid (192x336 ... 12x21, batch tensor 768x1344, image 749x1333), one frame, bf16 and fp32, at the testing
(pre / post NMS top-n 1000 / 1000) and the training (2000 / 2000) setting:

  * two hand-overs, ms per frame: fp32 NCHW maps (`propose_padded`: layout pass + head + filter) and a resident
    PackedClip (`propose_packed`: the head conv reads the frame in place)          -> rpn_ms_per_frame
  * per stage (device events around each launch group, median): head conv, predictor, select, decode, NMS + merge;
    for the select also the achieved GB/s over the objectness it has to read once
  * at the testing setting an A/B leg, interleaved in the same process: the same candidates (4 x 1000 + 756) through
    the blocked scan of sfvos_rpn_nms and through the existing sfvos_detections (labels = levels, max_det = 1000)

    python bench_rpn.py [--steps 20 --warmup 5] [--precisions bf16 fp32]

Prints ONE JSON line.  Not the headline metric (bench.py is)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

IMAGE = (749, 1333)
TENSOR = (768, 1344)
SETTINGS = {'testing': (1000, 1000), 'training': (2000, 2000)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fns, steps, warmup):
    """Median device time of each callable; the callables of one round run right behind each other (interleaved)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(steps):
        for i, fn in enumerate(fns):
            times[i].append(event_ms(fn))
    return [round(statistics.median(t), 4) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--precisions', nargs='+', default=['bf16', 'fp32'], choices=['bf16', 'fp32'])
    args = ap.parse_args()
    from sfvos_amd import PackedClip, RegionProposalNetwork, RPNHead, _lib, davis_pyramid
    from sfvos_amd._lib import _ptr, _stream
    from sfvos_amd.rpn import BBOX_XFORM_CLIP
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    _lib.check(lib.sfvos_check_device(), 'sfvos_check_device')
    gen = torch.Generator(device=dev).manual_seed(11)
    shapes = [hw for _, hw in davis_pyramid()]
    feats = OrderedDict((k, torch.randn((1, 256, h, w), generator=gen, device=dev)) for k, (h, w) in davis_pyramid())
    L, B, A = len(shapes), 1, 3
    out = {'metric': 'rpn_ms_per_frame', 'unit': 'ms', 'data': 'synthetic',
           'what': 'RPN head + proposal filter, DAVIS pyramid %s, tensor %dx%d, image %dx%d, one frame'
                   % (shapes, TENSOR[0], TENSOR[1], IMAGE[0], IMAGE[1])}
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    for prec in args.precisions:
        tdt = torch.bfloat16 if prec == 'bf16' else torch.float32
        torch.manual_seed(63)
        rpn = RegionProposalNetwork(head=RPNHead(256, A, prec), precision=prec).to(dev)
        with torch.no_grad():                       # logits and deltas of a trained head's size, not of its init's
            rpn.head.cls_logits.weight.mul_(20.0)
            rpn.head.bbox_pred.weight.mul_(5.0)
        for p in rpn.parameters():
            p.requires_grad_(False)
        head = rpn.head
        # a resident clip of 3 stored frames (the centre one is read)
        levels = [torch.randn(B, 3, h, w, 256, generator=gen, device=dev).to(tdt) for h, w in shapes]
        levels = [torch.cat([x[:, :1], f.permute(0, 2, 3, 1).to(tdt)[:, None], x[:, 2:]], 1)
                  for x, f in zip(levels, feats.values())]
        clip = PackedClip.from_levels(levels, layout='grouped' if prec == 'bf16' else 'ndhwc')
        pyr = _lib.make_pyramid(shapes)
        res = {}
        for mode, (k, post) in SETTINGS.items():
            rpn.train(mode == 'training')
            flat = head.maps_to_pyramid(list(feats.values()))
            t = head.conv_pyramid(flat, shapes, B)
            obj, dl = head.predict(t)
            S = L * B
            counts, index = torch.empty(S, **i32), torch.empty((S, k), **i32)
            boxes, logits = torch.empty((S, k, 4), **f32), torch.empty((S, k), **f32)
            scores, valid = torch.empty((S, k), **f32), torch.empty((S, k), **i32)
            ws = torch.empty(lib.sfvos_rpn_workspace_bytes(L, B, k), dtype=torch.uint8, device=dev)
            ob, osc = torch.empty((B, post, 4), **f32), torch.empty((B, post), **f32)
            oi, cnt = torch.empty((B, post), **i32), torch.empty(B, **i32)
            base = rpn.anchor_generator.device_table(dev)
            sizes = rpn._sizes_on([IMAGE], dev)

            def select():
                _lib.call('sfvos_rpn_select', _ptr(obj), ctypes.byref(pyr), B, A, k, _ptr(counts), _ptr(index), _stream())

            def decode():
                _lib.call('sfvos_rpn_decode', _ptr(obj), _ptr(dl), _ptr(counts), _ptr(index), ctypes.byref(pyr), B, A, k,
                          _ptr(base), TENSOR[0], TENSOR[1], _ptr(sizes), BBOX_XFORM_CLIP, rpn.min_size, rpn.score_thresh,
                          _ptr(boxes), _ptr(logits), _ptr(scores), _ptr(valid), _stream())

            def nms():
                _lib.call('sfvos_rpn_nms', _ptr(boxes), _ptr(logits), _ptr(scores), _ptr(valid), _ptr(counts), L, B, k,
                          rpn.nms_thresh, post, _ptr(ws), _ptr(ob), _ptr(osc), _ptr(oi), _ptr(cnt), _stream())

            stages = [lambda: head.conv_pyramid(flat, shapes, B), lambda: head.predict(t), select, decode, nms,
                      lambda: rpn.propose_padded(feats, [IMAGE], TENSOR),
                      lambda: rpn.propose_packed(clip, 1, [IMAGE], TENSOR)]
            names = ['head_conv', 'predictor', 'select', 'decode', 'nms_merge', 'from_nchw_maps', 'from_packed_clip']
            with torch.no_grad():
                ms = median_ms(stages, args.steps, args.warmup)
            r = dict(zip(names, ms))
            r['select_gbps'] = round(obj.numel() * 4 / (r['select'] * 1e-3) / 1e9, 2)
            r['candidates'] = int(counts.sum())
            r['valid'] = int(valid.sum())
            r['proposals'] = int(cnt[0])
            r['rpn_ms_per_frame'] = {'from_nchw_maps': r.pop('from_nchw_maps'), 'from_packed_clip': r.pop('from_packed_clip')}
            if mode == 'testing':
                # A/B: the same candidates through sfvos_detections (labels = levels, max_det = post)
                cs = counts.tolist()
                cb = torch.cat([boxes[s, :c] for s, c in enumerate(cs)]).contiguous()
                csx = torch.cat([scores[s, :c] for s, c in enumerate(cs)]).contiguous()
                cl = torch.cat([torch.full((c,), s, dtype=torch.int64, device=dev) for s, c in enumerate(cs)])
                n = cb.shape[0]
                dws = torch.empty(lib.sfvos_detections_workspace_bytes(n), dtype=torch.uint8, device=dev)
                dcnt = torch.empty(1, **i32)
                db, ds = torch.empty((post, 4), **f32), torch.empty(post, **f32)
                dlab = torch.empty(post, dtype=torch.int64, device=dev)
                di, dr = torch.empty(post, **i32), torch.empty(post, **i32)

                def detections():
                    _lib.call('sfvos_detections', _ptr(cb), _ptr(csx), _ptr(cl), n, 1, rpn.score_thresh, rpn.min_size,
                              rpn.nms_thresh, post, 1.0, 1.0, _ptr(dws), _ptr(dcnt), _ptr(db), _ptr(ds), _ptr(dlab),
                              _ptr(di), _ptr(dr), _stream())

                ab = median_ms([nms, detections], args.steps, args.warmup)
                r['ab_nms_%d_candidates' % n] = {'sfvos_rpn_nms': ab[0], 'sfvos_detections': ab[1],
                                                 'kept': [int(cnt[0]), int(dcnt[0])],
                                                 'note': 'sfvos_detections also ranks the candidates; sfvos_rpn_nms '
                                                         'takes them ranked by sfvos_rpn_select'}
            res[mode] = r
        out[prec] = res
        del rpn
    print(json.dumps(out))


if __name__ == '__main__':
    main()
