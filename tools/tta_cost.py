"""Cost of test-time augmentation on one MI355X.

python tools/tta_cost.py [repetitions] [fp32|bf16]
    Two synthetic 416 x 416 x 3 images, random-init weights (seed 1), K = 2, graph replay, min box 32.  Per setting -- none, flips,
    d4 (the TTA settings with box voting at IoU 0.5 and the consensus score) -- the whole of z-score -> network -> NMS (-> vote)
    -> detections on the host, host clock around a device synchronise, one warm-up each, then the settings ALTERNATED in one
    process.  Prints median, minimum and maximum per image.  After that it launches the yardsticks of the kernel table once per
    repetition: y3_copy over a tensor of the size of the d4 network input (a device-to-device copy of the bytes the views kernel
    writes) and an in-place torch multiply over the d4 decode rows (an elementwise kernel over the rows y3_tta_unmap maps).  Under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/tta_cost.py 3
    the kernel times are in the trace, and
python tools/tta_cost.py --trace DIR/.../*_kernel_trace.csv
    prints the TTA kernels, the NMS kernel and the yardsticks: launches, median, min and max in microseconds."""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

K = 2
ANCHORS = [(64, 384), (384, 64)]      # bench.py's
IMG, N, MIN_BOX = 416, 2, 32


def run(reps, precision):
    import torch
    from yolo3 import _hip, bbox_utils, imagereader
    from yolo3.model import YoloV3
    y = YoloV3(N, [IMG, IMG, 3], K, ANCHORS, seed=1, use_graph=True)
    y.inference_precision = precision
    raw = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (N, 3, IMG, IMG)).astype(np.float32)).cuda()

    def one(tta):
        x = imagereader.zscore_normalize_device(raw)
        if tta == 'none':
            return bbox_utils.detect(y.predict(x), MIN_BOX, clip_wh=(IMG, IMG))
        views = bbox_utils.TTA_VIEWS[tta]
        out = []
        for s0 in range(0, N, bbox_utils.tta_group_size(views)):
            rows = y.predict_tta(x[s0:s0 + bbox_utils.tta_group_size(views)], views)
            out += bbox_utils.detect_tta(rows, len(views), MIN_BOX, clip_wh=(IMG, IMG), vote_iou=0.5, score='consensus')
        return out

    settings = ('none', 'flips', 'd4')
    times = {s: [] for s in settings}
    dets = {s: one(s) for s in settings}                # warm-up: code objects, plans, graphs, buffers
    torch.cuda.synchronize()
    for _ in range(reps):
        for s in settings:
            t1 = time.perf_counter()
            one(s)
            torch.cuda.synchronize()
            times[s].append((time.perf_counter() - t1) * 1e3 / N)
    nb = y._plan(N, False, precision == 'bf16').nb
    print('precision %s, %d rows per view; detections per image: %s' % (precision, nb, ', '.join(
        '%s %s' % (s, [0 if d[0] is None else d[0].shape[0] for d in dets[s]]) for s in settings)))
    print('%-8s %8s %12s %10s %10s   (ms per image)' % ('tta', 'runs', 'median', 'min', 'max'))
    for s in settings:
        t = times[s]
        print('%-8s %8d %12.2f %10.2f %10.2f' % (s, len(t), np.median(t), min(t), max(t)))
    # yardsticks, for the kernel trace
    a = torch.zeros(N * 8, IMG, IMG, 4, device='cuda')
    b = torch.empty_like(a)
    rows = torch.zeros(N * 8, nb, 5 + K, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(reps):
        _hip.check(_hip.lib.y3_copy(_hip.view(a, N * 8, IMG, IMG, 4), _hip.view(b, N * 8, IMG, IMG, 4), st), 'y3_copy')
        rows.mul_(1.5)
    torch.cuda.synchronize()


def from_trace(path):
    groups = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r['Kernel_Name'].split('(')[0]
            if not any(s in name for s in ('tta_', 'vote_', 'nms_kernel', 'copy_add', 'copy_kernel', 'MulFunctor', 'nchw_to_nhwc')):
                continue
            grid = 'x'.join(r.get('Grid_Size_' + a, '?') for a in 'XYZ') if 'Grid_Size_X' in r else r.get('Grid_Size', '')
            groups.setdefault((name[-60:], grid), []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print('%-60s %-16s %8s %10s %10s %10s' % ('kernel', 'grid (threads)', 'launches', 'median us', 'min us', 'max us'))
    for key in sorted(groups):
        us = groups[key]
        print('%-60s %-16s %8d %10.2f %10.2f %10.2f' % (key[0], key[1], len(us), np.median(us), min(us), max(us)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1])
    else:
        run(int(args[0]) if args else 9, args[1] if len(args) > 1 else 'fp32')
