#!/usr/bin/env python
"""Timing of the image transform (reference code/helpers/model.py:283, `maskrcnn_model.transform(images)`) at DAVIS size:
480x854 frames -> 749x1333 inside a 3x768x1344 fp32 tensor, one frame and a batch of 8, from fp32 [N, 3, h, w] images and
from uint8 [N, h, w, 3] frames:

  * ms per frame of GeneralizedRCNNTransform on one tensor (one sfvos_transform_image launch + the torch.empty of the
    batch) and of the bare entry point into a preallocated batch                        -> transform_ms_per_frame
  * the algorithmic bytes, computed from the shapes here (the source once, the padded fp32 tensor once), and
    `hbm_share` = those bytes / 6.3 TB/s (what a copy kernel achieves on this part; the specification says 8) / the
    entry point's time
  * the nearest resize of 3 target masks (480x854 -> 749x1333 bytes) beside F.interpolate(...).byte()
  * the yardstick, in the same process and alternating with the legs above: the same chain in plain PyTorch ops on the
    GPU, as torchvision runs it -- sub, div, F.interpolate(bilinear) per frame, new_full, copy_ -- and for the byte
    source the permute / float / div(255) of ToTensor in front of it

    python bench_transform.py [--steps 50 --warmup 10]

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

FRAME = (480, 854)
HBM_ACHIEVABLE = 6.3e12
MASKS = 3


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


def torch_chain(x, mean, std, size, shape):
    """torchvision's normalize + resize + batch_images in plain PyTorch ops; x: fp32 [N, 3, h, w]."""
    frames = []
    for img in x:
        img = (img - mean[:, None, None]) / std[:, None, None]
        frames.append(F.interpolate(img[None], size=size, mode='bilinear', align_corners=False)[0])
    batch = frames[0].new_full((len(frames), 3) + tuple(shape), 0)
    for img, pad in zip(frames, batch):
        pad[:, :img.shape[1], :img.shape[2]].copy_(img)
    return batch


def to_tensor(u):
    """ToTensor on the GPU: uint8 [N, h, w, 3] -> fp32 [N, 3, h, w] in [0, 1]."""
    return u.permute(0, 3, 1, 2).float().div(255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8])
    args = ap.parse_args()
    from sfvos_amd import GeneralizedRCNNTransform, _lib
    from sfvos_amd.transform import resize_masks
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    _lib.check(_lib.load().sfvos_check_device(), 'sfvos_check_device')
    t = GeneralizedRCNNTransform().eval()
    size = t.resize_size(FRAME)
    shape = t.batch_shape([size])
    h, w = FRAME
    mean = torch.tensor(t.image_mean, device=dev)
    std = torch.tensor(t.image_std, device=dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    out = OrderedDict([('metric', 'transform_ms_per_frame'), ('unit', 'ms'), ('data', 'synthetic'),
                       ('what', '%dx%d frames -> %dx%d in a 3x%dx%d fp32 tensor (normalize, bilinear resize, zero pad)'
                        % (h, w, size[0], size[1], shape[0], shape[1])),
                       ('bounds', 'hbm_share: algorithmic bytes (source once + padded tensor once) / 6.3 TB/s '
                                  '(achievable copy rate) / the entry point\'s time')])
    for n in args.batches:
        u = torch.randint(0, 256, (n, h, w, 3), generator=gen, device=dev, dtype=torch.uint8)
        # the fp32 source: the bytes over 255 by a true division (a tensor divisor), what ToTensor gives on the CPU
        x = (u.permute(0, 3, 1, 2).float() / torch.tensor(255.0, device=dev)).contiguous()
        dst = torch.empty((n, 3) + shape, dtype=torch.float32, device=dev)

        def entry(src, u8):
            t._launch(src, u8, FRAME, n, dst, size)

        fns = [lambda: t(x), lambda: entry(x, False), lambda: torch_chain(x, mean, std, size, shape),
               lambda: t(u), lambda: entry(u, True), lambda: torch_chain(to_tensor(u), mean, std, size, shape)]
        ms = median_ms(fns, args.steps, args.warmup)
        r = OrderedDict()
        for name, (mod, ent, ref), src_bytes in (('fp32', ms[:3], 4), ('uint8', ms[3:], 1)):
            nbytes = n * (3 * h * w * src_bytes + 3 * shape[0] * shape[1] * 4)
            r[name] = OrderedDict([
                ('transform_ms_per_frame', round(mod / n, 4)), ('entry_point_ms_per_frame', round(ent / n, 4)),
                ('pytorch_ops_ms_per_frame', round(ref / n, 4)), ('bytes_per_frame', nbytes // n),
                ('gbps', round(nbytes / (ent * 1e-3) / 1e9, 1)),
                ('hbm_share', round(nbytes / HBM_ACHIEVABLE / (ent * 1e-3), 3))])
        # same values as the yardstick, loosely: a sanity check of the leg, not a test (tests/test_gpu_transform.py is)
        ref = torch_chain(x, mean, std, size, shape)
        r['max_abs_diff_to_pytorch_ops'] = round(float((t(x)[0].tensors - ref).abs().max()), 7)
        r['uint8_equals_fp32_path'] = bool(torch.equal(t(u)[0].tensors, t(x)[0].tensors))
        out['batch%d' % n] = r
    masks = (torch.rand((MASKS, h, w), generator=gen, device=dev) < 0.5).to(torch.uint8)
    ms = median_ms([lambda: resize_masks(masks, size),
                    lambda: F.interpolate(masks[:, None].float(), size=size)[:, 0].byte()], args.steps, args.warmup)
    nbytes = MASKS * (h * w + size[0] * size[1])
    out['masks'] = OrderedDict([('what', '%d masks %dx%d -> %dx%d bytes' % (MASKS, h, w, size[0], size[1])),
                                ('ms', ms[0]), ('pytorch_ops_ms', ms[1]), ('bytes', nbytes),
                                ('equal', bool(torch.equal(resize_masks(masks, size), F.interpolate(
                                    masks[:, None].float(), size=size)[:, 0].byte())))])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
