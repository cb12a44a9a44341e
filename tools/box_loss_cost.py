"""Cost of the opt-in IoU box-regression losses (y3_loss_fwd_bwd_ex): the loss launch of each kind at the three
scales of 8 x 416^2 x 3 anchors (K = 2; 13^2, 26^2 and 52^2 cells: 85 176 (cell, anchor) pairs in all), random logits, a few boxes
per image.  `mse` runs first and is the yardstick: it is the kernel y3_loss_fwd_bwd launches.

python tools/box_loss_cost.py [reps]
    launches the 12 configurations in a fixed order (2 warm-up + reps launches each, one stream) and prints HIP event times of
    the whole entry (clear + present + loss + finalize kernels).
rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/box_loss_cost.py [reps]
    the same launches under the tracer;  python tools/box_loss_cost.py --trace DIR/.../*_kernel_trace.csv [reps]
    then attributes the traced loss_kernel launches to the configurations by launch order and prints their kernel times.
python tools/box_loss_cost.py --step [steps]
    YoloV3.train_step at 8 x 416^2 (bench.py's model and labels, host-launched) for mse and ciou, alternated, ms per step."""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

KINDS = ('mse', 'giou', 'diou', 'ciou')
ANCHORS = [(32, 32), (128, 128), (256, 256)]
N, IMG, K = 8, 416, 2
WARMUP = 2


def configs():
    return [(s, kind) for s in (32, 16, 8) for kind in KINDS]


def make_labels():
    from yolo3.imagereader import format_boxes
    rng = np.random.default_rng(3)
    labs = [[], [], []]
    for _ in range(N):
        k = int(rng.integers(1, 7))
        wh = rng.integers(20, IMG // 2, (k, 2))
        xy = np.stack([rng.integers(0, IMG - wh[:, 0]), rng.integers(0, IMG - wh[:, 1])], 1)
        lab = format_boxes(np.concatenate([xy, wh, rng.integers(0, K, (k, 1))], 1).astype(np.int32), (IMG, IMG, 3), ANCHORS, K)
        for i in range(3):
            labs[i].append(lab[i])
    return [np.stack(l) for l in labs]


def run(reps):
    import torch
    from yolo3 import _hip
    A, D = len(ANCHORS), len(ANCHORS) * (5 + K)
    ld = (D + 3) // 4 * 4
    gts = make_labels()
    anc = _hip.float_array([v for a in ANCHORS for v in a])
    g = torch.Generator().manual_seed(1)
    st = torch.cuda.current_stream().cuda_stream
    print('%-6s %-5s %10s %10s %10s  %9s %9s  %s' % ('cells', 'kind', 'median us', 'min us', 'max us', 'positives', 'pairs', 'loss4 of one launch'))
    for si, s in enumerate((32, 16, 8)):
        G = IMG // s
        fm = (torch.randn(N, G, G, ld, generator=g) * 1.2).cuda()
        dfm = torch.zeros(N, G, G, ld, device='cuda')
        gt = torch.from_numpy(gts[si]).cuda().contiguous()
        ws = torch.zeros(int(_hip.lib.y3_loss_workspace_bytes()) // 4 + 4, device='cuda')
        loss4 = torch.zeros(4, device='cuda')
        tf_, td = _hip.Tensor(fm.data_ptr(), N, G, G, D, ld), _hip.Tensor(dfm.data_ptr(), N, G, G, D, ld)
        for kind in KINDS:
            times = []
            for r in range(WARMUP + reps):
                loss4.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _hip.check(_hip.lib.y3_loss_fwd_bwd_ex(tf_, gt.data_ptr(), anc, A, K, IMG, IMG, float(N), KINDS.index(kind), 1.0, loss4.data_ptr(),
                                                       td, ws.data_ptr(), st), 'y3_loss_fwd_bwd_ex')
                b.record()
                b.synchronize()
                if r >= WARMUP:
                    times.append(a.elapsed_time(b) * 1e3)
            print('%-6s %-5s %10.1f %10.1f %10.1f  %9d %9d  %s' % ('%dx%d' % (G, G), kind, np.median(times), min(times), max(times),
                                                                  int((gt[..., 4] != 0).sum()), N * G * G * A, [round(v, 4) for v in loss4.tolist()]))


def from_trace(path, reps):
    with open(path) as fh:
        recs = [r for r in csv.DictReader(fh) if 'loss_kernel' in r['Kernel_Name']]
    recs.sort(key=lambda r: int(r['Start_Timestamp']))
    per = WARMUP + reps
    cf = configs()
    if len(recs) != per * len(cf):
        raise SystemExit('%d loss kernels in the trace, expected %d' % (len(recs), per * len(cf)))
    print('%-6s %-5s %-28s %10s %10s %10s' % ('cells', 'kind', 'kernel', 'median us', 'min us', 'max us'))
    for i, (s, kind) in enumerate(cf):
        chunk = recs[i * per + WARMUP:(i + 1) * per]
        us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in chunk]
        name = chunk[0]['Kernel_Name']
        name = name[name.index('void ') + 5:] if 'void ' in name else name
        print('%-6s %-5s %-28s %10.2f %10.2f %10.2f' % ('%dx%d' % (IMG // s, IMG // s), kind, name[:28], np.median(us), min(us), max(us)))


def step_time(steps):
    import torch
    import bench
    from yolo3.model import YoloV3
    images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    gts = [torch.from_numpy(x).cuda() for x in bench.synth_labels(np.random.default_rng(3), 8)]
    models = {kind: YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1, box_loss=kind) for kind in ('mse', 'ciou')}
    for yolo in models.values():
        for _ in range(5):
            yolo.train_step((images, gts))
    torch.cuda.synchronize()
    print('YoloV3.train_step, batch 8 x 416^2, host-launched, %d steps per window, windows alternated' % steps)
    for rnd in range(3):
        for kind, yolo in models.items():
            t = time.perf_counter()
            for _ in range(steps):
                loss = yolo.train_step((images, gts))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / steps
            print('window %d  %-5s %.3f ms per step, %.1f images/s, loss %.6f' % (rnd, kind, dt * 1e3, 8 / dt, float(loss)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else 20)
    elif args and args[0] == '--step':
        step_time(int(args[1]) if len(args) > 1 else 40)
    else:
        run(int(args[0]) if args else 20)
