"""Cost of opt-in multi-scale training on one MI355X.

python tools/multiscale_cost.py --labels [reps]
    y3_format_labels at 8 x 416^2 with the training anchors, K = 1 and K = 80, a few boxes per image (2 warm-up + reps launches
    each, one stream), HIP event times of the entry; under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/multiscale_cost.py --labels [reps]
    the kernel_stats.csv row of format_labels_kernel is the kernel time (both K in one row), and
    python tools/multiscale_cost.py --trace DIR/.../*_kernel_trace.csv [reps]  splits the launches by K in launch order.
python tools/multiscale_cost.py --plans [steps]
    one model with train_sizes = every square multiple of 32 in 320..608, batch 8 (bench.py's anchors and classes): per size the
    device memory its training plan holds (torch.cuda.memory_allocated around the plan's construction: activations, gradients,
    labels, workspaces) and the host-launched train_step time (5 warm-up + steps timed, random images, a few boxes per image)."""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

ANCHORS = [(64, 384), (384, 64)]
N, IMG = 8, 416
WARMUP = 2
SIDES = list(range(320, 609, 32))


def boxes_for(rng, n, side, k):
    counts = rng.integers(1, 7, n).astype(np.int32)
    boxes = np.zeros((n, int(counts.max()), 5), np.int32)
    for i, c in enumerate(counts):
        wh = rng.integers(20, side // 2, (c, 2))
        xy = np.stack([rng.integers(0, side - wh[:, 0]), rng.integers(0, side - wh[:, 1])], 1)
        boxes[i, :c] = np.concatenate([xy, wh, rng.integers(0, k, (c, 1))], 1)
    return boxes, counts


def labels(reps):
    import torch
    from yolo3.imagereader import format_labels_device
    print('%-4s %12s %10s %10s %10s' % ('K', 'MB written', 'median us', 'min us', 'max us'))
    for k in (1, 80):
        boxes, counts = boxes_for(np.random.default_rng(3), N, IMG, k)
        b, c = torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda()
        times = []
        for r in range(WARMUP + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = format_labels_device(b, c, (IMG, IMG, 3), ANCHORS, k)
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                times.append(e0.elapsed_time(e1) * 1e3)
        mb = sum(o.numel() for o in out) * 4 / 1e6
        print('%-4d %12.2f %10.1f %10.1f %10.1f' % (k, mb, np.median(times), min(times), max(times)))


def from_trace(path, reps):
    with open(path) as fh:
        recs = [r for r in csv.DictReader(fh) if 'format_labels_kernel' in r['Kernel_Name']]
    recs.sort(key=lambda r: int(r['Start_Timestamp']))
    per = WARMUP + reps
    if len(recs) != 2 * per:
        raise SystemExit('%d format_labels_kernel launches in the trace, expected %d' % (len(recs), 2 * per))
    print('%-4s %10s %10s %10s' % ('K', 'median us', 'min us', 'max us'))
    for i, k in enumerate((1, 80)):
        us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in recs[i * per + WARMUP:(i + 1) * per]]
        print('%-4d %10.2f %10.2f %10.2f' % (k, np.median(us), min(us), max(us)))


def plans(steps):
    import torch
    from yolo3.imagereader import format_labels_device
    from yolo3.model import YoloV3
    k = 2
    yolo = YoloV3(N, [IMG, IMG, 3], k, ANCHORS, learning_rate=1e-4, seed=1, train_sizes=[(s, s) for s in SIDES])
    print('YoloV3.train_step, batch %d, host-launched, conv_arithmetic %s; memory = what the training plan of that size allocates' % (N, yolo.conv_arithmetic))
    print('%-6s %12s %12s %12s' % ('side', 'plan MiB', 'ms per step', 'images/s'))
    for side in SIDES:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        yolo._plan(N, True, size=(side, side))
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated() - before
        images = torch.randn(N, 3, side, side, generator=torch.Generator().manual_seed(side)).cuda()
        boxes, counts = boxes_for(np.random.default_rng(side), N, side, k)
        gts = format_labels_device(torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda(), (side, side, 3), ANCHORS, k)
        for _ in range(5):
            yolo.train_step((images, gts))
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            yolo.train_step((images, gts))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / steps
        print('%-6d %12.1f %12.3f %12.1f' % (side, held / 2**20, dt * 1e3, N / dt))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else 20)
    elif args and args[0] == '--plans':
        plans(int(args[1]) if len(args) > 1 else 20)
    else:
        labels(int(args[1]) if len(args) > 1 else 20)
