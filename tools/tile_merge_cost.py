"""Cost of the device merge of tiled inference on one MI355X.

python tools/tile_merge_cost.py [images]
    bench.py's tiled_4k case (one synthetic 4096 x 4096 x 3 uint8 image, 608 x 608 tiles, random-init weights, bf16 convs):
    the whole of inference_image_tiled per image, host clock around a device synchronise, with merge_device 'cpu' and 'gpu'
    ALTERNATED in one process (after one warm-up image each), then 'gpu' with seam_margin 8 and merge_nms hard.  Prints the
    median, minimum and maximum per setting and checks that the two merges return the same array.  Under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/tile_merge_cost.py 3
    the kernel times are in the trace, and
python tools/tile_merge_cost.py --trace DIR/.../*_kernel_trace.csv
    prints the merge and NMS kernels: launches, median, min and max in microseconds."""
import contextlib
import csv
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

K = 2
ANCHORS = [(64, 384), (384, 64)]      # bench.py's


def run(images):
    import torch
    import inference_tiled
    from yolo3.model import YoloV3
    y = YoloV3(25, [608, 608, 3], K, ANCHORS, seed=1, use_graph=True)
    y.inference_precision = 'bf16'
    mdl = y.get_keras_model()
    big = np.random.default_rng(4).integers(0, 256, (4096, 4096, 3), dtype=np.uint8)
    settings = [('cpu', {}), ('gpu', {'merge_device': 'gpu'}), ('gpu + margin 8 + hard', {'merge_device': 'gpu', 'seam_margin': 8.0, 'merge_nms': 'hard'})]
    times = {name: [] for name, _ in settings}
    results = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for name, kw in settings:          # warm-up: code objects, plans, buffers
            results[name] = inference_tiled.inference_image_tiled(mdl, big, [608, 608], 32, **kw)
        torch.cuda.synchronize()
        for _ in range(images):
            for name, kw in settings:
                t1 = time.perf_counter()
                inference_tiled.inference_image_tiled(mdl, big, [608, 608], 32, **kw)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t1) * 1e3)
    assert np.array_equal(results['cpu'], results['gpu'])
    print('detections: cpu %d, gpu %d (identical arrays), gpu + margin 8 + hard %d' % (
        results['cpu'].shape[0], results['gpu'].shape[0], results['gpu + margin 8 + hard'].shape[0]))
    print('%-24s %8s %10s %10s %10s' % ('merge', 'images', 'median ms', 'min ms', 'max ms'))
    for name, _ in settings:
        t = times[name]
        print('%-24s %8d %10.2f %10.2f %10.2f' % (name, len(t), np.median(t), min(t), max(t)))
    d = np.asarray(times['gpu']) - np.asarray(times['cpu'])
    print('gpu - cpu, paired per repetition: median %+.2f ms, min %+.2f, max %+.2f' % (np.median(d), d.min(), d.max()))


def from_trace(path):
    groups = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r['Kernel_Name'].split('(')[0]
            if not any(s in name for s in ('tile_merge', 'nms_kernel', 'soft_nms')):
                continue
            groups.setdefault((name[-70:], r.get('Grid_Size_X', r.get('Grid_Size', ''))), []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print('%-70s %-10s %8s %10s %10s %10s' % ('kernel', 'grid x', 'launches', 'median us', 'min us', 'max us'))
    for key in sorted(groups):
        us = groups[key]
        print('%-70s %-10s %8d %10.2f %10.2f %10.2f' % (key[0], key[1], len(us), np.median(us), min(us), max(us)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1])
    else:
        run(int(args[0]) if args else 9)
