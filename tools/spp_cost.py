"""Cost of the opt-in YOLOv3-SPP block (y3_spp_fwd, y3_spp_fwd_bf16, y3_spp_bwd and the 2048 -> 512 1x1 layer behind the pools, DESIGN
§3.18) at 8 x 13 x 13 and 8 x 19 x 19 x 512, the block's shapes at 8 x 416^2 and 8 x 608^2.

python tools/spp_cost.py [reps]
    per grid, in a fixed order: a device-to-device copy of the 2048-wide buffer (the yardstick), the three pooling entries in the
    model's layout (source = slice 0, pools = slice [512, 2048) of one buffer; backward with accumulate = 1), and the new layer's
    forward (training form: leaky-relu + statistics), data gradient and kernel gradient as the model's policy launches them (fp32
    MFMA kernels: a 1x1 layer of under 5 000 pixels); 2 warm-up + reps launches each, one stream, HIP event times of the whole entry.
    A one-element y3_fill separates the blocks, so that a trace can be cut at it.
rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/spp_cost.py [reps]
    the same launches under the tracer;  python tools/spp_cost.py --trace DIR/.../*_kernel_trace.csv [reps]  then cuts the trace at
    the fill_kernel markers and prints, per block, every kernel with the median / min / max of its timed launches.
python tools/spp_cost.py --step [steps]
    YoloV3.train_step and predict (fp32 and bf16) at 8 x 416^2 (bench.py's model, images and labels, host-launched) with spp off and
    on, alternated in one process.
rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/spp_cost.py --default-steps [steps]
    a model built without the keyword takes `steps` training steps: its kernel list;  python tools/spp_cost.py --kernels
    A_kernel_stats.csv B_kernel_stats.csv prints two such lists side by side (focal_loss_cost.kernel_lists)."""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np   # noqa: E402

N, C, GRIDS, WARMUP = 8, 512, (13, 19), 2
ENTRIES = ('copy', 'spp_fwd', 'spp_fwd_bf16', 'spp_bwd', 'conv_fwd', 'conv_dgrad', 'conv_wgrad')


def run(reps):
    import torch
    from yolo3 import _hip
    lib, T = _hip.lib, _hip.Tensor
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    mark = torch.zeros(4, device='cuda')

    def marker():
        _hip.check(lib.y3_fill(mark.data_ptr(), 1, 0.0, st), 'y3_fill')

    print('%-7s %-13s %10s %10s %10s  %s' % ('grid', 'entry', 'median us', 'min us', 'max us', 'bytes moved'))
    for G in GRIDS:
        M = N * G * G
        cat = torch.randn(M, 4 * C, generator=g).cuda()
        cat2 = torch.empty_like(cat)
        cat16 = cat.to(torch.bfloat16)
        dcat = torch.randn(M, 4 * C, generator=g).cuda()
        y = torch.empty(M, C, device='cuda')
        dz = torch.randn(M, C, generator=g).cuda()
        w = (torch.randn(4 * C, C, generator=g) * 0.02).cuda()
        bias = torch.zeros(C, device='cuda')
        dw = torch.empty(4 * C, C, device='cuda')
        view = lambda t, c, ld, off=0: T(t.data_ptr() + t.element_size() * off, N, G, G, c, ld)
        X, P, WIDE = view(cat, C, 4 * C), view(cat, 3 * C, 4 * C, C), view(cat, 4 * C, 4 * C)
        X16, P16 = view(cat16, C, 4 * C), view(cat16, 3 * C, 4 * C, C)
        DX, DP, DWIDE = view(dcat, C, 4 * C), view(dcat, 3 * C, 4 * C, C), view(dcat, 4 * C, 4 * C)
        Y, DZ = view(y, C, C), view(dz, C, C)
        tiles = int(lib.y3_conv2d_stats_tiles_x(M, 4 * C, 1, C, 0))
        stats = torch.empty(tiles * 2 * C, device='cuda')
        fws_b = int(lib.y3_conv2d_fwd_workspace_x(M, 4 * C, 1, C, 0))
        dws_b = int(lib.y3_conv2d_dgrad_workspace_x(DZ, 1, 1, DWIDE, 0))
        wws_b = int(lib.y3_conv2d_wgrad_workspace_x(WIDE, DZ, 1, 1, 0))
        fws, dws, wws = (torch.zeros(b // 4 + 4, device='cuda') for b in (fws_b, dws_b, wws_b))
        calls = {
            'copy': (lambda: cat2.copy_(cat), 2 * M * 4 * C * 4),
            'spp_fwd': (lambda: _hip.check(lib.y3_spp_fwd(X, P, st), 'y3_spp_fwd'), M * 4 * C * 4),
            'spp_fwd_bf16': (lambda: _hip.check(lib.y3_spp_fwd_bf16(X16, P16, st), 'y3_spp_fwd_bf16'), M * 4 * C * 2),
            'spp_bwd': (lambda: _hip.check(lib.y3_spp_bwd(X, DP, DX, 1, st), 'y3_spp_bwd'), M * 6 * C * 4),
            'conv_fwd': (lambda: _hip.check(lib.y3_conv2d_fwd(WIDE, w.data_ptr(), bias.data_ptr(), 1, 1, Y, _hip.EPI_LRELU, 0.2, None, None, None,
                                                              stats.data_ptr(), fws.data_ptr(), fws_b, st), 'y3_conv2d_fwd'), (M * 5 * C + 4 * C * C) * 4),
            'conv_dgrad': (lambda: _hip.check(lib.y3_conv2d_dgrad(DZ, w.data_ptr(), 1, 1, DWIDE, 0, dws.data_ptr(), dws_b, st), 'y3_conv2d_dgrad'),
                           (M * 5 * C + 4 * C * C) * 4),
            'conv_wgrad': (lambda: _hip.check(lib.y3_conv2d_wgrad_x(WIDE, DZ, 1, 1, dw.data_ptr(), 0, wws.data_ptr(), wws_b, st), 'y3_conv2d_wgrad_x'),
                           (M * 5 * C + 4 * C * C) * 4),
        }
        torch.cuda.synchronize()
        for name in ENTRIES:
            fn, moved = calls[name]
            marker()
            times = []
            for r in range(WARMUP + reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if r >= WARMUP:
                    times.append(a.elapsed_time(b) * 1e3)
            print('%-7s %-13s %10.1f %10.1f %10.1f  %d' % ('%dx%d' % (G, G), name, np.median(times), min(times), max(times), moved))
        marker()      # closes the grid's last block: what follows (the next grid's set-up) belongs to no entry
    torch.cuda.synchronize()


def from_trace(path, reps):
    with open(path) as fh:
        recs = sorted(csv.DictReader(fh), key=lambda r: int(r['Start_Timestamp']))
    blocks, cur = [], None
    for r in recs:
        if r['Kernel_Name'].startswith('fill_kernel'):
            cur = []
            blocks.append(cur)
        elif cur is not None:
            cur.append(r)
    want = len(GRIDS) * (len(ENTRIES) + 1)
    if len(blocks) != want:
        raise SystemExit('%d blocks between fill_kernel markers, expected %d' % (len(blocks), want))
    print('%-7s %-13s %-60s %5s %10s %10s %10s' % ('grid', 'entry', 'kernel', 'calls', 'median us', 'min us', 'max us'))
    for i, block in enumerate(blocks):
        if i % (len(ENTRIES) + 1) == len(ENTRIES):
            continue      # behind a grid's closing marker
        G, entry = GRIDS[i // (len(ENTRIES) + 1)], ENTRIES[i % (len(ENTRIES) + 1)]
        names = []
        for r in block:
            if r['Kernel_Name'] not in names:
                names.append(r['Kernel_Name'])
        for name in names:
            mine = [r for r in block if r['Kernel_Name'] == name]
            per = len(mine) // (WARMUP + reps) or 1
            us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in mine[WARMUP * per:]]
            short = name[name.index('void ') + 5:] if 'void ' in name else name
            print('%-7s %-13s %-60s %5d %10.2f %10.2f %10.2f' % ('%dx%d' % (G, G), entry, short[:60], len(mine), np.median(us), min(us), max(us)))


def _bench_inputs():
    import torch
    import bench
    images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    gts = [torch.from_numpy(x).cuda() for x in bench.synth_labels(np.random.default_rng(3), 8)]
    return bench, images, gts


def step_time(steps):
    import torch
    from yolo3.model import YoloV3
    bench, images, gts = _bench_inputs()
    models = {'plain': YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1),
              'spp': YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1, spp=True)}
    for name, yolo in models.items():
        for _ in range(5):
            yolo.train_step((images, gts))
            yolo.predict(images)
            yolo.predict(images, precision='bf16')
        plan = yolo._plan(8, True)
        print('%-5s %d conv layers, %d forward + %d backward launches per step, %d trainable values' % (
            name, len(yolo.specs), len(plan.fwd), sum(1 for e in plan.bwd if not isinstance(e[0], str) or e[0] == 'side_call'),
            sum(int(np.prod(w.shape)) for w in yolo.trainable_weights())))
    torch.cuda.synchronize()
    runs = (('train_step', lambda y: y.train_step((images, gts))), ('predict fp32', lambda y: y.predict(images)),
            ('predict bf16', lambda y: y.predict(images, precision='bf16')))
    print('batch 8 x 416^2, host-launched, %d calls per window, windows alternated' % steps)
    for what, call in runs:
        for rnd in range(3):
            for name, yolo in models.items():
                t = time.perf_counter()
                for _ in range(steps):
                    call(yolo)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t) / steps
                print('%-12s window %d  %-5s %.3f ms per call, %.1f images/s' % (what, rnd, name, dt * 1e3, 8 / dt))


def default_steps(steps):
    import torch
    from yolo3.model import YoloV3
    bench, images, gts = _bench_inputs()
    yolo = YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1)
    for _ in range(steps):
        loss = yolo.train_step((images, gts))
    torch.cuda.synchronize()
    print('%d default training steps, loss %.6f' % (steps, float(loss)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else 20)
    elif args and args[0] == '--default-steps':
        default_steps(int(args[1]) if len(args) > 1 else 5)
    elif args and args[0] == '--kernels':
        from focal_loss_cost import kernel_lists
        kernel_lists(args[1], args[2])
    elif args and args[0] == '--step':
        step_time(int(args[1]) if len(args) > 1 else 40)
    else:
        run(int(args[0]) if args else 20)
