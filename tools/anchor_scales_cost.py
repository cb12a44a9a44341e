"""Cost of the opt-in per-scale anchor assignment at 8 x 416^2 with Darknet's nine anchors, 3 / 3 / 3.

python tools/anchor_scales_cost.py [reps]
    per K in (2, 80): y3_format_labels beside y3_format_labels_scales (about 10 boxes per image), y3_decode_fwd beside
    y3_decode_fwd_scales (random feature maps), and after each a device copy of the same output bytes as the yardstick;
    2 warm-up + reps launches each, one stream; prints HIP event times of each whole entry.
rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/anchor_scales_cost.py [reps]
    the same launches under the tracer: the kernel_stats.csv rows of the four kernels are the kernel times (both K in one row).
python tools/anchor_scales_cost.py --step [steps]
    YoloV3.train_step and predict (host-launched, K = 2) with every anchor on every scale and with one scale per anchor,
    alternated in one process: three windows each, and the spread of each mode's own windows."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

ANCHORS = [(10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326)]
TABLE = [2, 2, 2, 1, 1, 1, 0, 0, 0]
N, IMG = 8, 416
WARMUP = 2


def make_boxes(per_image, K, seed=3):
    rng = np.random.default_rng(seed)
    wh = rng.integers(8, IMG // 2, (N, per_image, 2))
    xy = np.stack([rng.integers(0, IMG - wh[..., 0]), rng.integers(0, IMG - wh[..., 1])], -1)
    return np.concatenate([xy, wh, rng.integers(0, K, (N, per_image, 1))], -1).astype(np.int32)


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
    from yolo3.imagereader import format_labels_device
    lib = _hip.lib
    A = len(ANCHORS)
    anc, tab = _hip.float_array([v for a in ANCHORS for v in a]), _hip.int_array(TABLE)
    st = torch.cuda.current_stream().cuda_stream
    print('%-4s %-26s %12s %10s %10s %10s' % ('K', 'entry', 'out MB', 'median us', 'min us', 'max us'))

    def line(K, what, nbytes, t):
        print('%-4d %-26s %12.2f %10.1f %10.1f %10.1f' % (K, what, nbytes / 1e6, *t))

    def copy_of(K, nbytes, reps):
        src, dst = torch.zeros(nbytes // 4, device='cuda'), torch.empty(nbytes // 4, device='cuda')
        line(K, '  device copy, same bytes', nbytes, _timed(lambda: dst.copy_(src), reps))
    for K in (2, 80):
        boxes = torch.from_numpy(make_boxes(10, K)).cuda()
        counts = torch.full((N,), 10, dtype=torch.int32, device='cuda')
        for what, kw, a_per in (('y3_format_labels', {}, [A] * 3), ('y3_format_labels_scales', dict(anchor_scale=TABLE), [3] * 3)):
            nbytes = 4 * sum(N * (IMG // s) ** 2 * a * (5 + K) for s, a in zip((32, 16, 8), a_per))
            line(K, what, nbytes, _timed(lambda: format_labels_device(boxes, counts, (IMG, IMG, 3), ANCHORS, K, **kw), reps))
            copy_of(K, nbytes, reps)
        g = torch.Generator().manual_seed(1)
        for what, a_per in (('y3_decode_fwd', [A] * 3), ('y3_decode_fwd_scales', [3] * 3)):
            fms, views = [], []
            for s, a in zip((32, 16, 8), a_per):
                G, c = IMG // s, a * (5 + K)
                ld = (c + 3) // 4 * 4
                fms.append((torch.randn(N, G, G, ld, generator=g) * 1.2).cuda())
                views.append(_hip.Tensor(fms[-1].data_ptr(), N, G, G, c, ld))
            arr = (_hip.Tensor * 3)(*views)
            nb = sum((IMG // s) ** 2 * a for s, a in zip((32, 16, 8), a_per))
            out = torch.empty(N, nb, 5 + K, device='cuda')
            if what == 'y3_decode_fwd':
                fn = lambda: _hip.check(lib.y3_decode_fwd(arr, 3, anc, A, K, IMG, IMG, out.data_ptr(), st), what)
            else:
                fn = lambda: _hip.check(lib.y3_decode_fwd_scales(arr, anc, tab, A, K, IMG, IMG, out.data_ptr(), st), what)
            line(K, what + ' (%d rows)' % (N * nb), out.numel() * 4, _timed(fn, reps))
            copy_of(K, out.numel() * 4, reps)


def step_time(steps):
    import torch
    from yolo3.imagereader import format_labels_device
    from yolo3.model import YoloV3
    K = 2
    images = torch.randn(N, 3, IMG, IMG, generator=torch.Generator().manual_seed(100)).cuda()
    boxes = torch.from_numpy(make_boxes(10, K)).cuda()
    counts = torch.full((N,), 10, dtype=torch.int32, device='cuda')
    models, labels = {}, {}
    for mode, table in (('all', None), ('scale', TABLE)):
        models[mode] = YoloV3(N, [IMG, IMG, 3], K, ANCHORS, learning_rate=1e-4, seed=1, **({} if table is None else dict(anchor_scales=table)))
        labels[mode] = format_labels_device(boxes, counts, (IMG, IMG, 3), ANCHORS, K, **({} if table is None else dict(anchor_scale=table)))
        for _ in range(5):
            models[mode].train_step((images, labels[mode]))
            models[mode].predict(images)
    torch.cuda.synchronize()
    print('batch %d x %d^2, nine anchors, K = %d, about 10 boxes per image, host-launched, %d calls per window, windows alternated; rows per image: '
          'all %d, scale %d' % (N, IMG, K, steps, models['all'].number_output_boxes, models['scale'].number_output_boxes))
    for what in ('train_step', 'predict'):
        seen = {m: [] for m in models}
        for rnd in range(3):
            for mode, yolo in models.items():
                t = time.perf_counter()
                for _ in range(steps):
                    if what == 'train_step':
                        yolo.train_step((images, labels[mode]))
                    else:
                        yolo.predict(images)
                torch.cuda.synchronize()
                seen[mode].append((time.perf_counter() - t) / steps * 1e3)
                print('%-10s window %d  %-5s %.3f ms per call' % (what, rnd, mode, seen[mode][-1]))
        spread = {m: max(v) - min(v) for m, v in seen.items()}
        diff = np.median(seen['all']) - np.median(seen['scale'])
        print('%-10s medians: all %.3f ms, scale %.3f ms; spread of its own windows: all %.3f, scale %.3f; difference %.3f ms: %s'
              % (what, np.median(seen['all']), np.median(seen['scale']), spread['all'], spread['scale'], diff,
                 'resolved' if abs(diff) > 2 * max(spread.values()) else 'NOT resolved (within twice the spread)'))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--step':
        step_time(int(args[1]) if len(args) > 1 else 20)
    else:
        run(int(args[0]) if args else 20)
