"""Cost of the opt-in letterbox front end on one MI355X.

python tools/letterbox_cost.py [reps]
    two batches of uint8 images into the 8 x 416^2 network input: 8 x 1080 x 1920 x 3 (a reduction by 4.6) and 8 x 416 x 416 x 3
    (the identity): y3_letterbox_zscore_nhwc (resample + content statistics + normalise into NHWC) and y3_letterbox_batch (fill +
    resample into the planar frame), beside two yardsticks: a device-to-device copy_ of the same source bytes and one of the
    8 x 416^2 x 4 NHWC input; y3_letterbox_unmap over the 8 x 10647 decode rows.  Prints the byte counts per pass and HIP event
    times (2 warm-up + reps launches each, one stream); under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/letterbox_cost.py [reps]
    the kernel times are in the trace, and
python tools/letterbox_cost.py --trace DIR/.../*_kernel_trace.csv [reps]
    prints them per kernel and grid: launches, median, min and max in microseconds, the launches of one grid cut in launch order
    into parts of 2 + reps.
python tools/letterbox_cost.py --e2e [reps]
    the loop body of inference.py per batch of 8 images of 416^2 (upload, z-score, network, NMS, results on the host), without and
    with --letterbox, alternated in one process, random weights, fp32: milliseconds per image."""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

N, SIDE = 8, 416
WARMUP = 2
ANCHORS = [(10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326)]


def run(reps):
    import torch
    from yolo3 import _hip, letterbox
    lib, check = _hip.lib, _hip.check
    st = torch.cuda.current_stream().cuda_stream
    print('%-12s %-34s %12s %10s %10s' % ('source', 'entry', 'MB moved', 'median us', 'min us'))
    for h, w in ((1080, 1920), (SIDE, SIDE)):
        rng = np.random.default_rng(h)
        records, total = letterbox.pack_layout([(h, w, 3)] * N, 1, SIDE, SIDE)
        src = torch.from_numpy(rng.integers(0, 256, total, dtype=np.uint8)).cuda()
        src2 = torch.empty_like(src)
        x0 = torch.empty(N, SIDE, SIDE, 4, device='cuda')
        x1 = torch.empty_like(x0)
        planar = torch.empty(N, 3, SIDE, SIDE, device='cuda')
        ws = torch.empty(int(lib.y3_letterbox_workspace_bytes(N, SIDE, SIDE, 3)) // 8 + 2, dtype=torch.float64, device='cuda')
        rows = torch.rand(N, 10647, 7, device='cuda') * SIDE
        dst = _hip.Tensor(x0.data_ptr(), N, SIDE, SIDE, 4, 4)
        nh, nw = int(records[0]['new_h']), int(records[0]['new_w'])
        content = N * 3 * nh * nw * 4 / 1e6
        bands = -(-nh // 8)
        reread = (bands * (8 * h / nh + 2 * max(h / nh, 1))) / h          # source rows read per source row: bands overlap by the support
        src_mb, in_mb = total / 1e6, x0.numel() * 4 / 1e6
        entries = [('letterbox_zscore_nhwc', lambda: check(lib.y3_letterbox_zscore_nhwc(src.data_ptr(), 0, 3, N, records.ctypes.data, dst, ws.data_ptr(),
                                                                                        st)), src_mb * reread + 3 * content + in_mb),
                   ('letterbox_batch', lambda: check(lib.y3_letterbox_batch(src.data_ptr(), 0, 3, N, records.ctypes.data, SIDE, SIDE, 0.0,
                                                                            planar.data_ptr(), st)), src_mb * reread + planar.numel() * 4 / 1e6),
                   ('copy_ of the source bytes', lambda: src2.copy_(src), 2 * src_mb),
                   ('copy_ of the NHWC input', lambda: x1.copy_(x0), 2 * in_mb),
                   ('letterbox_unmap', lambda: check(lib.y3_letterbox_unmap(rows.data_ptr(), N, 10647, 7, records.ctypes.data, 1, st)),
                    2 * N * 10647 * 16 / 1e6)]
        print('# %d x %d x %d x 3 uint8 = %.2f MB -> content %d x %d; resample pass reads the source %.3f x (%.2f MB), stages %.2f MB of '
              'content, statistics read it once, the last pass reads it and writes %.2f MB of NHWC input'
              % (N, h, w, src_mb, nh, nw, reread, src_mb * reread, content, in_mb))
        for name, fn, moved in entries:
            times = []
            for r in range(WARMUP + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= WARMUP:
                    times.append(e0.elapsed_time(e1) * 1e3)
            print('%-12s %-34s %12.2f %10.1f %10.1f' % ('%dx%d' % (h, w), name, moved, np.median(times), min(times)))


def e2e(reps):
    import torch
    from yolo3 import bbox_utils, imagereader
    from yolo3.model import YoloV3
    yolo = YoloV3(N, [SIDE, SIDE, 3], 2, ANCHORS, seed=1, use_graph=True)
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8) for _ in range(N)]

    def plain():
        x = torch.from_numpy(np.stack([np.ascontiguousarray(im.astype(np.float32).transpose((2, 0, 1))) for im in imgs])).cuda()
        rows = yolo.predict(imagereader.zscore_normalize_device(x))
        return bbox_utils.detect(rows, 32, clip_wh=(SIDE, SIDE))

    def boxed():
        rows, _ = yolo.predict_letterbox(imgs)
        return bbox_utils.detect(rows, 32, clip_wh=None)

    times = {'plain': [], 'letterbox': []}
    for r in range(WARMUP + reps):
        for name, fn in (('plain', plain), ('letterbox', boxed)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3 / N)
    for name, t in times.items():
        print('%-10s %8.3f ms per image (median of %d batches of %d), min %.3f' % (name, np.median(t), len(t), N, min(t)))


def from_trace(path, reps=None):
    groups = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            key = (r['Kernel_Name'].split('(')[0][-60:], r.get('Grid_Size_X', r.get('Grid_Size', '')), r.get('Grid_Size_Y', ''), r.get('Grid_Size_Z', ''))
            groups.setdefault(key, []).append((int(r['Start_Timestamp']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    print('%-60s %-18s %-6s %8s %10s %10s %10s' % ('kernel', 'grid', 'part', 'launches', 'median us', 'min us', 'max us'))
    for key in sorted(groups):
        us = [t for _, t in sorted(groups[key])]
        step = (WARMUP + reps) if reps else len(us)
        parts = [us[i:i + step] for i in range(0, len(us), step)]
        for p, part in enumerate(parts):
            print('%-60s %-18s %-6d %8d %10.2f %10.2f %10.2f' % (key[0], 'x'.join(k for k in key[1:] if k), p, len(part), np.median(part), min(part), max(part)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else None)
    elif args and args[0] == '--e2e':
        e2e(int(args[1]) if len(args) > 1 else 10)
    else:
        run(int(args[0]) if args else 20)
