"""Cost of the opt-in focal loss and class-label smoothing (y3_loss_fwd_bwd_focal): the loss launch at the three scales
of 8 x 416^2 x 3 anchors (K = 2; 13^2, 26^2 and 52^2 cells: 85 176 (cell, anchor) pairs in all), random logits, a few boxes per image,
the reference's mask.  `plain` runs first at every scale and is the yardstick: neutral arguments through the same entry, which is the
FOCAL == false kernel y3_loss_fwd_bwd launches.  `focal` is gamma 2, alpha 0.25 on both terms with label smoothing 0.1.

python tools/focal_loss_cost.py [reps]
    launches the 6 configurations in a fixed order (2 warm-up + reps launches each, one stream) and prints HIP event times of the
    whole entry (clear + present + loss + finalize kernels).
rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/focal_loss_cost.py [reps]
    the same launches under the tracer;  python tools/focal_loss_cost.py --trace DIR/.../*_kernel_trace.csv [reps]
    then attributes the traced loss_kernel launches to the configurations by launch order and prints their kernel times.
python tools/focal_loss_cost.py --step [steps]
    YoloV3.train_step at 8 x 416^2 (bench.py's model and labels, host-launched) without and with the flags, alternated, ms per step.
rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/focal_loss_cost.py --default-steps [steps]
    a model built without the arguments takes `steps` training steps: its kernel list;  python tools/focal_loss_cost.py --kernels
    A_kernel_stats.csv B_kernel_stats.csv then prints both lists (kernel name, calls) side by side, differing rows marked."""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np   # noqa: E402

from box_loss_cost import ANCHORS, IMG, K, N, WARMUP, make_labels   # noqa: E402

SETTINGS = (('plain', (0.0, 0.0, 0.0, 0.0, 0.0)), ('focal', (2.0, 0.25, 2.0, 0.25, 0.1)))
FOCAL_KW = dict(focal_gamma=2.0, focal_alpha=0.25, focal_terms='both', label_smoothing=0.1)


def configs():
    return [(s, name) for s in (32, 16, 8) for name, _ in SETTINGS]


def run(reps):
    import torch
    from yolo3 import _hip
    A, D = len(ANCHORS), len(ANCHORS) * (5 + K)
    ld = (D + 3) // 4 * 4
    gts = make_labels()
    anc = _hip.float_array([v for a in ANCHORS for v in a])
    g = torch.Generator().manual_seed(1)
    st = torch.cuda.current_stream().cuda_stream
    print('%-6s %-6s %10s %10s %10s  %9s %9s  %s' % ('cells', 'terms', 'median us', 'min us', 'max us', 'positives', 'pairs', 'loss4 of one launch'))
    for si, s in enumerate((32, 16, 8)):
        G = IMG // s
        fm = (torch.randn(N, G, G, ld, generator=g) * 1.2).cuda()
        dfm = torch.zeros(N, G, G, ld, device='cuda')
        gt = torch.from_numpy(gts[si]).cuda().contiguous()
        ws = torch.zeros(int(_hip.lib.y3_loss_workspace_bytes()) // 4 + 4, device='cuda')
        loss4 = torch.zeros(4, device='cuda')
        tf_, td = _hip.Tensor(fm.data_ptr(), N, G, G, D, ld), _hip.Tensor(dfm.data_ptr(), N, G, G, D, ld)
        for name, args in SETTINGS:
            times = []
            for r in range(WARMUP + reps):
                loss4.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _hip.check(_hip.lib.y3_loss_fwd_bwd_focal(tf_, gt.data_ptr(), anc, A, K, IMG, IMG, float(N), 0, 1.0, None, None, 1, 0.5,
                                                          loss4.data_ptr(), None, td, ws.data_ptr(), *args, st), 'y3_loss_fwd_bwd_focal')
                b.record()
                b.synchronize()
                if r >= WARMUP:
                    times.append(a.elapsed_time(b) * 1e3)
            print('%-6s %-6s %10.1f %10.1f %10.1f  %9d %9d  %s' % ('%dx%d' % (G, G), name, np.median(times), min(times), max(times),
                                                                  int((gt[..., 4] != 0).sum()), N * G * G * A, [round(v, 4) for v in loss4.tolist()]))


def from_trace(path, reps):
    with open(path) as fh:
        recs = [r for r in csv.DictReader(fh) if 'loss_kernel' in r['Kernel_Name']]
    recs.sort(key=lambda r: int(r['Start_Timestamp']))
    per = WARMUP + reps
    cf = configs()
    if len(recs) != per * len(cf):
        raise SystemExit('%d loss kernels in the trace, expected %d' % (len(recs), per * len(cf)))
    print('%-6s %-6s %-40s %10s %10s %10s' % ('cells', 'terms', 'kernel', 'median us', 'min us', 'max us'))
    for i, (s, name) in enumerate(cf):
        chunk = recs[i * per + WARMUP:(i + 1) * per]
        us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in chunk]
        kernel = chunk[0]['Kernel_Name']
        kernel = kernel[kernel.index('void ') + 5:] if 'void ' in kernel else kernel
        print('%-6s %-6s %-40s %10.2f %10.2f %10.2f' % ('%dx%d' % (IMG // s, IMG // s), name, kernel[:40], np.median(us), min(us), max(us)))


def step_time(steps):
    import torch
    import bench
    from yolo3._hip import lib
    from yolo3.model import YoloV3
    images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    gts = [torch.from_numpy(x).cuda() for x in bench.synth_labels(np.random.default_rng(3), 8)]
    models = {'plain': YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1),
              'focal': YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1, **FOCAL_KW)}
    entries = ('y3_loss_fwd_bwd', 'y3_loss_fwd_bwd_ex', 'y3_loss_fwd_bwd_truth', 'y3_loss_fwd_bwd_focal')
    for name, yolo in models.items():
        for _ in range(5):
            yolo.train_step((images, gts))
        print('%-5s loss calls of the plan: %s' % (name, [[e for e in entries if c[0] is getattr(lib, e)][0] for c in yolo._plan(8, True).loss_calls]))
    torch.cuda.synchronize()
    print('YoloV3.train_step, batch 8 x 416^2, host-launched, %d steps per window, windows alternated' % steps)
    for rnd in range(3):
        for name, yolo in models.items():
            t = time.perf_counter()
            for _ in range(steps):
                loss = yolo.train_step((images, gts))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / steps
            print('window %d  %-5s %.3f ms per step, %.1f images/s, loss %.6f' % (rnd, name, dt * 1e3, 8 / dt, float(loss)))


def default_steps(steps):
    import torch
    import bench
    from yolo3.model import YoloV3
    images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    gts = [torch.from_numpy(x).cuda() for x in bench.synth_labels(np.random.default_rng(3), 8)]
    yolo = YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1)
    for _ in range(steps):
        loss = yolo.train_step((images, gts))
    torch.cuda.synchronize()
    print('%d default training steps, loss %.6f' % (steps, float(loss)))


def kernel_lists(path_a, path_b):
    def calls(path):
        with open(path) as fh:
            return {r['Name']: int(r['Calls']) for r in csv.DictReader(fh)}
    a, b = calls(path_a), calls(path_b)
    print('%-110s %8s %8s' % ('kernel', 'calls A', 'calls B'))
    for name in sorted(set(a) | set(b)):
        mark = '' if a.get(name) == b.get(name) else '   <-- differs'
        print('%-110s %8s %8s%s' % (name[:110], a.get(name, '-'), b.get(name, '-'), mark))
    print('%d kernels in A, %d in B, %d rows differ' % (len(a), len(b), sum(1 for n in set(a) | set(b) if a.get(n) != b.get(n))))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else 20)
    elif args and args[0] == '--default-steps':
        default_steps(int(args[1]) if len(args) > 1 else 5)
    elif args and args[0] == '--kernels':
        kernel_lists(args[1], args[2])
    elif args and args[0] == '--step':
        step_time(int(args[1]) if len(args) > 1 else 40)
    else:
        run(int(args[0]) if args else 20)
