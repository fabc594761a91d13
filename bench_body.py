#!/usr/bin/env python
"""Timing of the ResNet-50 body (reference code/helpers/model.py:204, the `body` half of the backbone) on one
1x3x768x1344 frame, bf16 and fp32:

  * body_ms_per_frame: `ResNetBody.forward` (stem, pool, 52 conv launches + the combines of the K-split shapes, four
    unpack launches to fp32 NCHW), median of device-event times
  * per stage (device events around each group of launches, median after warm-up): stem, pool, layer1..layer4, unpack;
    with the algorithmic FLOPs and bytes of each, computed from the shapes here (every operand crosses HBM once);
    `mfma_share` = FLOPs / the MFMA peak of the dtype (bf16 2.5 PFLOP/s dense, fp32 157.3 TFLOP/s) / time
  * backbone_ms_per_frame: `BackboneWithFPN.forward` (body + FPN, fp32 NCHW maps out)
  * the yardstick, in the same process and alternating with the legs above: the same chain in plain PyTorch ops
    (F.conv2d, the frozen norm as a per-channel multiply-add, F.relu, F.max_pool2d) in NCHW and in channels_last; the
    faster of the two is reported as `pytorch_ops_ms_per_frame`, both are listed

    python bench_body.py [--steps 10 --warmup 3] [--precisions bf16 fp32]

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


def half(s):
    return ((s[0] - 1) // 2 + 1, (s[1] - 1) // 2 + 1)


def algorithmic(body, prec):
    """Per stage: (FLOPs, bytes each operand has to cross HBM once), from the shapes alone."""
    es = 2 if prec == 'bf16' else 4
    out = OrderedDict()
    h1 = half(TENSOR)
    p1 = h1[0] * h1[1]
    out['stem'] = (2 * p1 * 147 * 64, 3 * TENSOR[0] * TENSOR[1] * 4 + 64 * 147 * es + p1 * 64 * es)
    hw = half(h1)
    out['pool'] = (0, (p1 + hw[0] * hw[1]) * 64 * es)
    for li in range(1, 5):
        flops = nbytes = 0
        for blk in getattr(body, 'layer%d' % li):
            convs = [(blk.conv1, hw), (blk.conv2, hw)]
            ohw = half(hw) if blk.stride == 2 else hw
            convs.append((blk.conv3, ohw))
            if blk.downsample is not None:
                convs.append((blk.downsample[0], hw))
            for conv, ihw in convs:
                o = half(ihw) if conv.stride[0] == 2 else ihw
                taps = conv.kernel_size[0] * conv.kernel_size[1]
                flops += 2 * o[0] * o[1] * conv.in_channels * conv.out_channels * taps
                nbytes += (ihw[0] * ihw[1] * conv.in_channels + o[0] * o[1] * conv.out_channels
                           + taps * conv.in_channels * conv.out_channels) * es
            nbytes += ohw[0] * ohw[1] * blk.conv3.out_channels * es      # the residual
            hw = ohw
        out['layer%d' % li] = (flops, nbytes)
    return out


def torch_chain(x, params, dtype, channels_last):
    """torchvision's forward in plain PyTorch ops; params: (weight, scale, shift) per conv in dtype, in launch order."""
    it = iter(params)

    def conv_bn(t, stride, pad):
        w, sc, sh = next(it)
        return F.conv2d(t, w, None, stride, pad) * sc + sh

    t = x.to(dtype)
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    t = F.max_pool2d(F.relu(conv_bn(t, 2, 3)), 3, 2, 1)
    outs = []
    for li, n in enumerate((3, 4, 6, 3)):
        for bi in range(n):
            s = 2 if (li > 0 and bi == 0) else 1
            identity = conv_bn(t, s, 0) if bi == 0 else t
            o = F.relu(conv_bn(t, 1, 0))
            o = F.relu(conv_bn(o, s, 1))
            t = F.relu(conv_bn(o, 1, 0) + identity)
        outs.append(t.float().contiguous())
    return outs


def chain_params(body, dtype, channels_last):
    def one(conv, bn):
        sc, sh = bn.coefficients()
        w = conv.weight.detach().to(dtype)
        if channels_last:
            w = w.contiguous(memory_format=torch.channels_last)
        return w, sc.to(dtype).reshape(1, -1, 1, 1), sh.to(dtype).reshape(1, -1, 1, 1)

    params = [one(body.conv1, body.bn1)]
    for li in range(1, 5):
        for blk in getattr(body, 'layer%d' % li):
            if blk.downsample is not None:
                params.append(one(blk.downsample[0], blk.downsample[1]))
            params += [one(blk.conv1, blk.bn1), one(blk.conv2, blk.bn2), one(blk.conv3, blk.bn3)]
    return params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precisions', nargs='+', default=['bf16', 'fp32'], choices=['bf16', 'fp32'])
    args = ap.parse_args()
    from sfvos_amd import BackboneWithFPN, _lib
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    _lib.check(_lib.load().sfvos_check_device(), 'sfvos_check_device')
    gen = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn((1, 3) + TENSOR, generator=gen, device=dev)
    out = {'metric': 'body_ms_per_frame', 'unit': 'ms', 'data': 'synthetic',
           'what': 'ResNet-50 body (stem, pool, 52 convs with frozen norms, unpack) on one 1x3x%dx%d frame' % TENSOR,
           'bounds': 'mfma_share: algorithmic FLOPs / MFMA peak of the dtype (bf16 2.5 PFLOP/s, fp32 157.3 TFLOP/s) / time'}
    with torch.no_grad():
        for prec in args.precisions:
            tdt = torch.bfloat16 if prec == 'bf16' else torch.float32
            torch.manual_seed(63)
            net = BackboneWithFPN(precision=prec).to(dev)
            for p in net.parameters():
                p.requires_grad_(False)
            body = net.body
            for m in body.modules():          # frozen-norm buffers that keep the activations of order one
                if hasattr(m, 'running_var'):
                    m.running_var.uniform_(0.5, 2.0)
                    m.weight.uniform_(0.3, 0.7)
            stem, hw1 = body._stem(x)
            pooled, hw2 = body._pool(stem, 1, hw1)
            ins, cur, hw = [], pooled, hw2
            for li in range(1, 5):
                ins.append((cur, hw))
                cur, hw = body._layer(li, cur, 1, hw)
            maps, shapes = body.forward_channels_last(x)
            names = ['stem', 'pool', 'layer1', 'layer2', 'layer3', 'layer4', 'unpack']
            stages = [lambda: body._stem(x), lambda: body._pool(stem, 1, hw1)]
            stages += [lambda li=li: body._layer(li, ins[li - 1][0], 1, ins[li - 1][1]) for li in range(1, 5)]
            stages.append(lambda: body._unpack(maps, shapes, 1))
            pn, pc = chain_params(body, tdt, False), chain_params(body, tdt, True)
            fpn_w = [(c.weight.to(tdt), c.bias.to(tdt)) for c in list(net.fpn.inner_blocks) + list(net.fpn.layer_blocks)]

            def torch_backbone(params, cl):
                c = [m.to(tdt) for m in torch_chain(x, params, tdt, cl)]
                last = F.conv2d(c[3], *fpn_w[3])
                res = [F.conv2d(last, *fpn_w[7], padding=1)]
                for l in (2, 1, 0):
                    last = F.conv2d(c[l], *fpn_w[l]) + F.interpolate(last, size=c[l].shape[-2:], mode='nearest')
                    res.insert(0, F.conv2d(last, *fpn_w[4 + l], padding=1))
                res.append(F.max_pool2d(res[-1], 1, 2, 0))
                return [r.float() for r in res]

            whole = [lambda: body(x), lambda: net(x), lambda: torch_chain(x, pn, tdt, False),
                     lambda: torch_chain(x, pc, tdt, True), lambda: torch_backbone(pn, False),
                     lambda: torch_backbone(pc, True)]
            ms = median_ms(stages + whole, args.steps, args.warmup)
            alg = algorithmic(body, prec)
            r = OrderedDict()
            for n, t in zip(names, ms):
                e = {'ms': t}
                if n in alg:
                    flops, nbytes = alg[n]
                    e.update(flops=flops, bytes=nbytes, gbps=round(nbytes / (t * 1e-3) / 1e9, 1))
                    if flops:
                        e['tflops'] = round(flops / (t * 1e-3) / 1e12, 1)
                        e['mfma_share'] = round(flops / MFMA_PEAK[prec] / (t * 1e-3), 3)
                else:
                    nbytes = sum(m.numel() for m in maps) * (4 + maps[0].element_size())
                    e.update(bytes=nbytes, gbps=round(nbytes / (t * 1e-3) / 1e9, 1))
                r[n] = e
            k = len(names)
            r['sum_of_stages_ms'] = round(sum(ms[:k]), 4)
            r['total_gflop'] = round(sum(f for f, _ in alg.values()) / 1e9, 1)
            r['body_ms_per_frame'] = ms[k]
            r['backbone_ms_per_frame'] = ms[k + 1]
            r['pytorch_ops'] = {'body_nchw': ms[k + 2], 'body_channels_last': ms[k + 3], 'backbone_nchw': ms[k + 4],
                                'backbone_channels_last': ms[k + 5]}
            r['pytorch_ops_ms_per_frame'] = min(ms[k + 2], ms[k + 3])
            r['pytorch_ops_backbone_ms_per_frame'] = min(ms[k + 4], ms[k + 5])
            # same values as the yardstick, loosely: a sanity check of the leg, not a test (tests/test_gpu_body.py is)
            ref = torch_chain(x, pn, tdt, False)
            got = body(x)
            r['max_rel_diff_to_pytorch_ops'] = round(max(
                float((a - b).abs().max() / b.abs().max()) for a, b in zip(got.values(), ref)), 5)
            out[prec] = r
            del net, body
    print(json.dumps(out))


if __name__ == '__main__':
    main()
