#!/usr/bin/env python
"""Timing of the feature pyramid network (reference code/helpers/model.py:204, the `fpn` half of the backbone) on the
body's maps at DAVIS size (image tensor 768x1344): C2 256x192x336, C3 512x96x168, C4 1024x48x84, C5 2048x24x42, one
frame, bf16 and fp32:

  * two hand-overs, ms per frame: fp32 NCHW maps out (`forward`: FPN + one unpack launch) and a resident PackedClip
    (`write_frames`: every level written in place)                                    -> fpn_ms_per_frame
  * per stage (device events around each launch, median after warm-up): the four lateral launches, the four 3x3 convs,
    the pool; with the algorithmic bytes and FLOPs of each, computed from the shapes here.  Printed and named as such:
    `hbm_share` of a lateral launch = its algorithmic bytes / 6.3 TB/s (what a copy kernel achieves on this part; the
    specification says 8) / its time; `mfma_share` of a 3x3 conv = its FLOPs / the MFMA peak of the dtype (bf16 2.5
    PFLOP/s dense, fp32 157.3 TFLOP/s) / its time
  * the yardstick, in the same process and alternating with the legs above: the same chain in plain PyTorch ops
    (F.conv2d, F.interpolate(mode='nearest'), F.max_pool2d) on NCHW tensors, fp32 and bf16 (the bf16 leg includes the
    cast of C2..C5, as the lateral kernel reads them as fp32)

    python bench_fpn.py [--steps 20 --warmup 5] [--precisions bf16 fp32]

Prints ONE JSON line.  Not the headline metric (bench.py is)."""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

TENSOR = (768, 1344)
BODY = [(256, 192, 336), (512, 96, 168), (1024, 48, 84), (2048, 24, 42)]
OUT = 256
HBM_ACHIEVABLE = 6.3e12
MFMA_PEAK = {'bf16': 2.5e15, 'fp32': 157.3e12}


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


def algorithmic(prec):
    """Per stage: (bytes each operand has to cross HBM once, FLOPs), from the shapes alone."""
    es = 2 if prec == 'bf16' else 4
    out = OrderedDict()
    for l, (c, h, w) in enumerate(BODY):
        p = h * w
        top = 0 if l == len(BODY) - 1 else BODY[l + 1][1] * BODY[l + 1][2] * OUT * es
        out['lateral%d' % l] = (p * c * 4 + OUT * c * es + OUT * 4 + top + p * OUT * es, 2 * p * c * OUT)
    for l, (c, h, w) in enumerate(BODY):
        p = h * w
        out['conv%d' % l] = (2 * p * OUT * es + 9 * OUT * OUT * es + OUT * 4, 2 * p * 9 * OUT * OUT)
    h, w = (BODY[-1][1] - 1) // 2 + 1, (BODY[-1][2] - 1) // 2 + 1
    out['pool'] = (2 * h * w * OUT * es, 0)
    return out


def torch_chain(x, inner_w, inner_b, layer_w, layer_b, dtype):
    """torchvision's forward in plain PyTorch ops; x: fp32 NCHW maps (cast here), weights already in dtype."""
    x = [m.to(dtype) for m in x]
    last = F.conv2d(x[-1], inner_w[-1], inner_b[-1])
    res = [F.conv2d(last, layer_w[-1], layer_b[-1], padding=1)]
    for l in range(len(x) - 2, -1, -1):
        last = F.conv2d(x[l], inner_w[l], inner_b[l]) + F.interpolate(last, size=x[l].shape[-2:], mode='nearest')
        res.insert(0, F.conv2d(last, layer_w[l], layer_b[l], padding=1))
    res.append(F.max_pool2d(res[-1], 1, 2, 0))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--precisions', nargs='+', default=['bf16', 'fp32'], choices=['bf16', 'fp32'])
    args = ap.parse_args()
    from sfvos_amd import FeaturePyramidNetwork, PackedClip, _lib
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    _lib.check(_lib.load().sfvos_check_device(), 'sfvos_check_device')
    gen = torch.Generator(device=dev).manual_seed(11)
    x = OrderedDict((str(l), torch.randn((1, c, h, w), generator=gen, device=dev)) for l, (c, h, w) in enumerate(BODY))
    maps = list(x.values())
    out = {'metric': 'fpn_ms_per_frame', 'unit': 'ms', 'data': 'synthetic',
           'what': 'FPN (4 lateral launches, 4 3x3 convs, pool) on C2..C5 %s of a %dx%d tensor, one frame'
                   % (BODY, TENSOR[0], TENSOR[1]),
           'bounds': 'hbm_share: algorithmic bytes / 6.3 TB/s (achievable copy rate) / time; mfma_share: FLOPs / MFMA '
                     'peak of the dtype (bf16 2.5 PFLOP/s, fp32 157.3 TFLOP/s) / time'}
    with torch.no_grad():
        for prec in args.precisions:
            tdt = torch.bfloat16 if prec == 'bf16' else torch.float32
            torch.manual_seed(63)
            fpn = FeaturePyramidNetwork([c for c, _, _ in BODY], OUT, precision=prec).to(dev)
            for p in fpn.parameters():
                p.requires_grad_(False)
            shapes = fpn.level_shapes([(h, w) for _, h, w in BODY])
            M = sum(h * w for h, w in shapes)
            seq = PackedClip(torch.zeros((3 * M, OUT), dtype=tdt, device=dev), shapes, 1, 3)
            flat, _, inner = fpn.forward_pyramid(x, return_inner=True)
            pos = [sum(h * w for h, w in shapes[:l]) for l in range(len(shapes))]
            iw = [c.weight.to(tdt) for c in fpn.inner_blocks]
            ib = [c.bias.to(tdt) for c in fpn.inner_blocks]
            lw = [c.weight.to(tdt) for c in fpn.layer_blocks]
            lb = [c.bias.to(tdt) for c in fpn.layer_blocks]
            stages, names = [], []
            for l in range(4):
                top = inner[l + 1] if l < 3 else None
                top_hw = shapes[l + 1] if l < 3 else (0, 0)
                stages.append(lambda l=l, top=top, top_hw=top_hw: fpn._lateral(l, maps[l], top, top_hw, inner[l]))
                names.append('lateral%d' % l)
            for l in range(4):
                stages.append(lambda l=l: fpn._layer(l, inner[l], 1, shapes[l], flat, pos[l]))
                names.append('conv%d' % l)
            stages.append(lambda: fpn._subsample(1, shapes[3], flat, pos[3], pos[4]))
            names.append('pool')
            whole = [lambda: fpn(x), lambda: fpn.write_frames(x, seq, 1),
                     lambda: torch_chain(maps, iw, ib, lw, lb, tdt)]
            ms = median_ms(stages + whole, args.steps, args.warmup)
            alg = algorithmic(prec)
            r = OrderedDict()
            for n, t in zip(names, ms):
                nbytes, flops = alg[n]
                e = {'ms': t, 'bytes': nbytes, 'flops': flops, 'gbps': round(nbytes / (t * 1e-3) / 1e9, 1)}
                if n.startswith('lateral'):
                    e['hbm_share'] = round(nbytes / HBM_ACHIEVABLE / (t * 1e-3), 3)
                if n.startswith('conv'):
                    e['tflops'] = round(flops / (t * 1e-3) / 1e12, 1)
                    e['mfma_share'] = round(flops / MFMA_PEAK[prec] / (t * 1e-3), 3)
                r[n] = e
            r['sum_of_stages_ms'] = round(sum(ms[:len(names)]), 4)
            r['fpn_ms_per_frame'] = {'to_nchw_maps': ms[-3], 'write_frames': ms[-2]}
            r['pytorch_ops_ms_per_frame'] = ms[-1]
            # same values as the yardstick, loosely: a sanity check of the leg, not a test (tests/test_gpu_fpn.py is)
            ref = torch_chain(maps, iw, ib, lw, lb, tdt)
            got = fpn(x)
            r['max_rel_diff_to_pytorch_ops'] = round(max(
                float((a.float() - b).abs().max() / b.abs().max()) for a, b in zip(ref, got.values())), 5)
            out[prec] = r
            del fpn
    print(json.dumps(out))


if __name__ == '__main__':
    main()
