#!/usr/bin/env python
"""Training throughput of sfvos_amd.SlowFastWindows (first-layer reuse across consecutive training windows) next to
the plain path on the same resident sequence: the reference's cycle (code/helpers/model.py:316-374) -- per centre
frame forward, loss, backward(), and the optimiser step after every second frame -- at (4,32), DAVIS pyramid of a
480x854 frame, bf16, a resident sequence of synthetic frames.

    python bench_windows.py [--sp 4 --fp 32] [--frames 12] [--pairs 10] [--warmup 2]

reuse=True and reuse=False pairs alternate in one process and are timed with device events after warm-up.  A second
pass turns the kernel timer on for fast_conv1 / slow_conv1 forward and the shift: their times on the first clip of a
pair (after a step: computed whole) and on the second (reused).

Prints ONE JSON line, metric `train_windows_ms_per_clip`.  Not the headline metric (bench.py is)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS = 8.0   # MI355X HBM3E specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sp', type=int, default=4)
    ap.add_argument('--fp', type=int, default=32)
    ap.add_argument('--frames', type=int, default=12, help='frames of the resident sequence')
    ap.add_argument('--pairs', type=int, default=10, help='timed pairs of clips per arm')
    ap.add_argument('--warmup', type=int, default=2, help='untimed pairs per arm')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32'])
    args = ap.parse_args()
    from sfvos_amd import FusedSGD, MSEProxyLoss, PackedClip, SlowFastLayers, SlowFastWindows, davis_pyramid
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(63)
    model = SlowFastLayers(256, dev, args.sp, args.fp, precision=args.precision).to(dev).train()
    opt = FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4).attach(model)
    pyr = davis_pyramid()
    keys = [k for k, _ in pyr]
    gen = torch.Generator(device=dev).manual_seed(7)
    bf16 = args.precision == 'bf16'
    tdt = torch.bfloat16 if bf16 else torch.float32
    levels = [torch.randn((1, args.frames, h, w, 256), generator=gen, device=dev).to(tdt) for _, (h, w) in pyr]
    seq = PackedClip.from_levels(levels, keys=keys, layout='grouped' if bf16 else 'ndhwc')
    del levels
    loss_fn = MSEProxyLoss({k: torch.randn((1, 256, h, w), generator=gen, device=dev) for k, (h, w) in pyr})
    wins = {True: SlowFastWindows(model, seq, reuse=True), False: SlowFastWindows(model, seq, reuse=False)}
    centres = [c for c in range(args.frames - 1)]
    cursor = {True: 0, False: 0}
    reused_seen = {True: [], False: []}

    def pair(reuse):
        i = centres[cursor[reuse] % len(centres)]
        cursor[reuse] += 2
        win = wins[reuse]
        for c in (i, i + 1):
            loss_fn(win.enhance(c)).backward()
            reused_seen[reuse].append(win.reused['f1'])
        opt.step()
        opt.zero_grad()

    opt.zero_grad()
    for _ in range(args.warmup):
        for reuse in (True, False):
            pair(reuse)
    torch.cuda.synchronize()
    times = {True: [], False: []}
    for _ in range(args.pairs):
        for reuse in (True, False):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pair(reuse)
            e1.record()
            times[reuse].append((e0, e1))
    torch.cuda.synchronize()
    ms = {r: sum(a.elapsed_time(b) for a, b in v) / (2 * len(v)) for r, v in times.items()}

    # kernel timer pass: the first clip of a pair is computed whole, the second reuses
    timer = model.enable_kernel_timer(['conv_fwd/f1', 'conv_fwd/s1', 'shift/f1', 'shift/s1'])
    kt = {'fresh': {}, 'reused': {}}
    for _ in range(3):
        i = centres[cursor[True] % len(centres)]
        cursor[True] += 2
        for c, kind in ((i, 'fresh'), (i + 1, 'reused')):
            timer.reset()
            loss_fn(wins[True].enhance(c)).backward()
            for name, (_, t) in timer.summary().items():
                kt[kind].setdefault(name, []).append(t)
        opt.step()
        opt.zero_grad()
    model._timer = None
    kt = {kind: {n: sorted(v)[len(v) // 2] for n, v in d.items()} for kind, d in kt.items()}   # medians

    plan = model.plan
    positions = sum(h * w for _, (h, w) in pyr)
    esize = 2 if bf16 else 4
    t_f1 = plan.layer('f1').t_out
    # the shift reads t_out frames (t_out - 1 from the previous window, 1 new) and writes t_out frames
    shift_bytes = 2 * t_f1 * positions * 32 * esize
    sh = kt['reused'].get('shift/f1')
    rate = shift_bytes / (sh * 1e-3) / 1e12 if sh else None
    res = {
        'metric': 'train_windows_ms_per_clip',
        'value': round(ms[True], 4),
        'note': 'not the headline metric (bench.py is): SlowFastWindows reuse=True, reference training cycle',
        'plain_ms_per_clip': round(ms[False], 4),
        'ratio_reuse_over_plain': round(ms[True] / ms[False], 4),
        'config': dict(sp=args.sp, fp=args.fp, precision=args.precision, frames=args.frames, pairs=args.pairs,
                       pyramid='davis', positions_per_frame=positions),
        'reused_f1_frames_per_pair': sorted(set(reused_seen[True])),
        'kernel_ms_fresh_clip': {k: round(v, 4) for k, v in kt['fresh'].items()},
        'kernel_ms_reused_clip': {k: round(v, 4) for k, v in kt['reused'].items()},
        'f1_fwd_reused_over_fresh': round(kt['reused']['conv_fwd/f1'] / kt['fresh']['conv_fwd/f1'], 4),
        'shift_f1_bytes': shift_bytes,
        'shift_f1_tbps_event_timed': round(rate, 3) if rate else None,
        'shift_f1_fraction_of_hbm_peak': round(rate / HBM_PEAK_TBPS, 3) if rate else None,
    }
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
