"""Cost of gradient accumulation and global-norm clipping: the bench.py training step at batch 8 x 416^2,
host-launched.  python tools/grad_accum_cost.py [accumulate_steps (1 = off)] [grad_clip_norm (0 = off)] [micro-steps] [--plain-too]
--plain-too also steps a second, default model (no accumulation, no clipping) in the same process, one optimiser step of each in
turn, so that under `rocprofv3 --kernel-trace --stats -- python tools/grad_accum_cost.py ... --plain-too` the stats file holds
grad_sumsq_kernel<false / true>, grad_clip_scale_kernel and the scaled Adam kernel NEXT TO the plain one of the same run, the yardstick (optim_kernel<3, EMA, SCALED>:
the Adam kind of the optimiser template of csrc/optim.hip).
`tools/grad_accum_cost.py --rates STATS.csv ...` prints each of them as bytes / time (bytes counted here from the arena size)."""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + '/object-detection-yolov3_amd')

ARENA_FLOATS = 61790400            # YoloV3(…, [416, 416, 3], 2, bench.ANCHORS).arena_floats (checked below when a model is built)
# fp32 arena streams per launch: reads + writes
STREAMS = {'optim_kernel<3, false, false>': 7, 'optim_kernel<3, false, true>': 7, 'optim_kernel<3, true, false>': 9, 'optim_kernel<3, true, true>': 9,
           'grad_sumsq_kernel<false>': 1, 'grad_sumsq_kernel<true>': 3}


def rates(paths):
    """kernel_stats.csv files of rocprofv3 --stats: Name, Calls, TotalDurationNs, AverageNs, ..., MinNs, MaxNs."""
    import csv
    for path in paths:
        print(path)
        for row in csv.DictReader(open(path)):
            name = row['Name']
            key = next((k for k in STREAMS if name.replace('void ', '').startswith(k + '(')), None)
            if key is None and 'grad_clip_scale_kernel' not in name:
                continue
            avg, lo, hi = float(row['AverageNs']) / 1e3, float(row['MinNs']) / 1e3, float(row['MaxNs']) / 1e3
            if key is None:
                print('  %-30s calls %4s  average %8.1f us  min %8.1f  max %8.1f' % ('grad_clip_scale_kernel', row['Calls'], avg, lo, hi))
                continue
            nbytes = STREAMS[key] * ARENA_FLOATS * 4
            note = ''
            if key == 'grad_sumsq_kernel<true>':
                note = '  (3 streams assumed; the first micro-step of each optimiser step moves 2: the min is that launch)'
            print('  %-30s calls %4s  average %8.1f us  min %8.1f  max %8.1f  %d x %.1f MB  %.2f TB/s%s'
                  % (key, row['Calls'], avg, lo, hi, STREAMS[key], ARENA_FLOATS * 4 / 1e6, nbytes / (avg * 1e-6) / 1e12, note))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--rates':
        return rates(sys.argv[2:])
    import numpy as np
    import torch
    import bench
    from yolo3.model import YoloV3
    argv = [a for a in sys.argv[1:] if a != '--plain-too']
    plain_too = len(argv) != len(sys.argv) - 1
    k = int(argv[0]) if len(argv) > 0 else 1
    clip = float(argv[1]) if len(argv) > 1 else 0.0
    steps = int(argv[2]) if len(argv) > 2 else 32
    steps -= steps % k                     # whole optimiser steps
    yolo = YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1, accumulate_steps=k, grad_clip_norm=clip or None)
    assert yolo.arena_floats == ARENA_FLOATS
    images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    gts = [torch.from_numpy(x).cuda() for x in bench.synth_labels(np.random.default_rng(3), 8)]
    for _ in range(max(4, k)):
        loss = yolo.train_step((images, gts))
    torch.cuda.synchronize()
    if plain_too:          # profile mode: the step time printed below is not a figure
        plain = YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1)
        for i in range(steps):
            yolo.train_step((images, gts))
            if i % k == k - 1:
                plain.train_step((images, gts))
        torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        loss = yolo.train_step((images, gts))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / steps
    norm = 'norm %.6g scale %.6g' % (float(yolo.last_grad_norm), float(yolo.grad_scale_dev)) if yolo.last_grad_norm is not None else 'no norm'
    print('accumulate_steps %d grad_clip_norm %g: %.3f ms per micro-step, %.1f images/s over %d micro-steps, loss %.6f, %s, arena %d floats'
          % (k, clip, dt * 1e3, 8 / dt, steps, float(loss), norm, yolo.arena_floats))


if __name__ == '__main__':
    main()
