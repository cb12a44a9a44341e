"""Cost of the opt-in ignore mask against each image's ground-truth boxes (y3_truth_boxes + y3_loss_fwd_bwd_truth):
the loss launch with either mask at the three scales of 8 x 416^2 x 3 anchors (K = 2; 85 176 (cell, anchor) pairs in all), random
logits, about 10 and about 100 boxes per image.  `reference` (y3_loss_fwd_bwd) runs first and is the yardstick.

python tools/ignore_mask_cost.py [reps]
    launches the configurations in a fixed order (2 warm-up + reps launches each, one stream): per box count the gather on the
    finest label tensor, then per scale the reference entry and the truth entry; prints HIP event times of each whole entry.
rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/ignore_mask_cost.py [reps]
    the same launches under the tracer;  python tools/ignore_mask_cost.py --trace DIR/.../*_kernel_trace.csv [reps]
    then attributes the traced truth_boxes_kernel and loss_kernel launches to the configurations by launch order.
python tools/ignore_mask_cost.py --step [steps]
    YoloV3.train_step at 8 x 416^2 (bench.py's model, about 10 boxes per image, host-launched) with the mask off and on, alternated."""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

ANCHORS = [(32, 32), (128, 128), (256, 256)]
N, IMG, K = 8, 416, 2
WARMUP = 2
BOX_COUNTS = (10, 100)
CAP = 1024


def make_labels(per_image, seed=3):
    from yolo3.imagereader import format_boxes
    rng = np.random.default_rng(seed)
    labs = [[], [], []]
    for _ in range(N):
        wh = rng.integers(12, IMG // 4, (per_image, 2))
        xy = np.stack([rng.integers(0, IMG - wh[:, 0]), rng.integers(0, IMG - wh[:, 1])], 1)
        lab = format_boxes(np.concatenate([xy, wh, rng.integers(0, K, (per_image, 1))], 1).astype(np.int32), (IMG, IMG, 3), ANCHORS, K)
        for i in range(3):
            labs[i].append(lab[i])
    return [np.stack(l) for l in labs]


def _timed(fn, reps):
    import torch
    times = []
    for r in range(WARMUP + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= WARMUP:
            times.append(a.elapsed_time(b) * 1e3)
    return np.median(times), min(times), max(times)


def run(reps):
    import torch
    from yolo3 import _hip
    lib = _hip.lib
    A, D = len(ANCHORS), len(ANCHORS) * (5 + K)
    ld = (D + 3) // 4 * 4
    anc = _hip.float_array([v for a in ANCHORS for v in a])
    st = torch.cuda.current_stream().cuda_stream
    print('%-6s %-6s %-10s %10s %10s %10s  %s' % ('boxes', 'cells', 'entry', 'median us', 'min us', 'max us', 'note'))
    for per_image in BOX_COUNTS:
        gts = [torch.from_numpy(g).cuda().contiguous() for g in make_labels(per_image)]
        boxes = torch.zeros(N, CAP, 4, device='cuda')
        counts = torch.zeros(N, dtype=torch.int32, device='cuda')
        ignored = torch.zeros(1, device='cuda')
        fine = gts[2]
        t = _timed(lambda: _hip.check(lib.y3_truth_boxes(fine.data_ptr(), N, fine.numel() // (N * (5 + K)), 5 + K, boxes.data_ptr(),
                                                         counts.data_ptr(), CAP, st), 'y3_truth_boxes'), reps)
        print('%-6d %-6s %-10s %10.1f %10.1f %10.1f  lists of %s boxes' % (per_image, '52x52', 'gather', *t, counts.tolist()))
        g = torch.Generator().manual_seed(1)
        for si, s in enumerate((32, 16, 8)):
            G = IMG // s
            fm = (torch.randn(N, G, G, ld, generator=g) * 1.2).cuda()
            dfm = torch.zeros(N, G, G, ld, device='cuda')
            ws = torch.zeros(max(int(lib.y3_loss_workspace_bytes()), int(lib.y3_loss_truth_workspace_bytes(N))) // 4 + 4, device='cuda')
            loss4 = torch.zeros(4, device='cuda')
            tf_, td = _hip.Tensor(fm.data_ptr(), N, G, G, D, ld), _hip.Tensor(dfm.data_ptr(), N, G, G, D, ld)
            gt = gts[si]
            t = _timed(lambda: _hip.check(lib.y3_loss_fwd_bwd(tf_, gt.data_ptr(), anc, A, K, IMG, IMG, float(N), loss4.data_ptr(), td, ws.data_ptr(), st),
                                          'y3_loss_fwd_bwd'), reps)
            print('%-6d %-6s %-10s %10.1f %10.1f %10.1f' % (per_image, '%dx%d' % (G, G), 'reference', *t))
            ignored.zero_()
            t = _timed(lambda: _hip.check(lib.y3_loss_fwd_bwd_truth(tf_, gt.data_ptr(), anc, A, K, IMG, IMG, float(N), 0, 1.0, boxes.data_ptr(),
                                                                    counts.data_ptr(), CAP, 0.5, loss4.data_ptr(), ignored.data_ptr(), td, ws.data_ptr(),
                                                                    st), 'y3_loss_fwd_bwd_truth'), reps)
            print('%-6d %-6s %-10s %10.1f %10.1f %10.1f  ignored per launch %d of %d pairs' % (per_image, '%dx%d' % (G, G), 'truth', *t,
                                                                                             int(float(ignored) / (WARMUP + reps)), N * G * G * A))


def from_trace(path, reps):
    with open(path) as fh:
        recs = [r for r in csv.DictReader(fh) if 'loss_kernel' in r['Kernel_Name'] or 'truth_boxes_kernel' in r['Kernel_Name']]
    recs.sort(key=lambda r: int(r['Start_Timestamp']))
    per = WARMUP + reps
    cf = [(b, what, s) for b in BOX_COUNTS for what, s in [('gather', 8)] + [(m, s) for s in (32, 16, 8) for m in ('reference', 'truth')]]
    if len(recs) != per * len(cf):
        raise SystemExit('%d kernels in the trace, expected %d' % (len(recs), per * len(cf)))
    print('%-6s %-6s %-10s %-34s %10s %10s %10s' % ('boxes', 'cells', 'entry', 'kernel', 'median us', 'min us', 'max us'))
    for i, (b, what, s) in enumerate(cf):
        chunk = recs[i * per + WARMUP:(i + 1) * per]
        us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in chunk]
        name = chunk[0]['Kernel_Name']
        name = name[name.index('void ') + 5:] if 'void ' in name else name
        print('%-6d %-6s %-10s %-34s %10.2f %10.2f %10.2f' % (b, '%dx%d' % (IMG // s, IMG // s), what, name[:34], np.median(us), min(us), max(us)))


def step_time(steps):
    import torch
    from yolo3.model import YoloV3
    images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    gts = [torch.from_numpy(x).cuda() for x in make_labels(10)]
    models = {mask: YoloV3(8, [416, 416, 3], 2, ANCHORS, learning_rate=1e-4, seed=1, ignore_mask=mask) for mask in ('reference', 'truth')}
    for yolo in models.values():
        for _ in range(5):
            yolo.train_step((images, gts))
    torch.cuda.synchronize()
    print('YoloV3.train_step, batch 8 x 416^2, about 10 boxes per image, host-launched, %d steps per window, windows alternated' % steps)
    for rnd in range(3):
        for mask, yolo in models.items():
            t = time.perf_counter()
            for _ in range(steps):
                loss = yolo.train_step((images, gts))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / steps
            extra = '' if mask == 'reference' else ', ignored %d, longest list %d' % (int(yolo.last_ignored), int(yolo.last_truth_max))
            print('window %d  %-9s %.3f ms per step, %.1f images/s, loss %.6f%s' % (rnd, mask, dt * 1e3, 8 / dt, float(loss), extra))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else 20)
    elif args and args[0] == '--step':
        step_time(int(args[1]) if len(args) > 1 else 40)
    else:
        run(int(args[0]) if args else 20)
