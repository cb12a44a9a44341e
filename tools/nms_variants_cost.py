"""Cost of the NMS variants (y3_nms_per_class_ex): every method at 8 x 416^2, K = 1 and 2, on two kinds of rows
  random  rows of a random-weight network (nearly every row passes the 0.1 score threshold: the worst case)
  sparse  tests/golden/nms_sparse416_k2.npz (a trained-like candidate count) for all 8 images; K = 1 keeps its first class

python tools/nms_variants_cost.py [reps]
    launches the 16 configurations in a fixed order (2 warm-up + reps launches each, one stream) and prints event times.
rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/nms_variants_cost.py [reps]
    the same launches under the tracer;  python tools/nms_variants_cost.py --trace DIR/.../*_kernel_trace.csv [reps]
    then attributes the traced NMS kernels to the configurations by launch order and prints their kernel times.
python tools/nms_variants_cost.py --eval N
    evaluate.py's evaluation loop (metrics.evaluate_examples: z-score, network, NMS, matching) on N synthetic 416^2 images
    of a random-weight model, images/s per method (one warm-up pass first)."""
import csv
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

METHODS = ('hard', 'diou', 'soft-linear', 'soft-gaussian')
CODES = {m: i for i, m in enumerate(METHODS)}
WARMUP = 2


def configs():
    return [(kind, k, m) for kind in ('random', 'sparse') for k in (1, 2) for m in METHODS]


def make_rows(kind, k):
    import torch
    if kind == 'sparse':
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'nms_sparse416_k2.npz'))
        return torch.from_numpy(np.stack([z['rows'][:, :5 + k]] * 8)).cuda()
    import bench
    from yolo3.model import YoloV3
    yolo = YoloV3(8, [416, 416, 3], k, bench.ANCHORS, seed=1)
    x = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    return yolo.predict(x).contiguous()


def run(reps):
    import torch
    from yolo3 import _hip
    rows_cache = {}
    print('%-7s %2s %-14s %10s %10s %10s  %s' % ('rows', 'K', 'method', 'median us', 'min us', 'max us', 'kept per (image, class), image 0'))
    for kind, k, m in configs():
        if (kind, k) not in rows_cache:
            rows_cache[(kind, k)] = make_rows(kind, k)
        rows = rows_cache[(kind, k)]
        n, nb, _ = rows.shape
        idx = torch.empty(n, k, nb, dtype=torch.int32, device='cuda')
        cnt = torch.zeros(n, k, dtype=torch.int32, device='cuda')
        sc = torch.empty(n, k, nb, dtype=torch.float32, device='cuda')
        wsb = int(_hip.lib.y3_nms_workspace_bytes_ex(n, nb, k, CODES[m]))
        ws = torch.empty(max(wsb, 4) // 4 + 4, dtype=torch.float32, device='cuda')
        st = torch.cuda.current_stream().cuda_stream
        times = []
        for r in range(WARMUP + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _hip.check(_hip.lib.y3_nms_per_class_ex(rows.data_ptr(), n, nb, k, CODES[m], 32.0, 0.1, 0.3, 0.5, 416.0, 416.0, idx.data_ptr(),
                                                    cnt.data_ptr(), sc.data_ptr(), nb, ws.data_ptr(), wsb, st), 'y3_nms_per_class_ex')
            b.record()
            b.synchronize()
            if r >= WARMUP:
                times.append(a.elapsed_time(b) * 1e3)
        cand = int(((rows[0, :, 5:] * rows[0, :, 4:5]).sqrt() >= 0.1).sum())
        print('%-7s %2d %-14s %10.1f %10.1f %10.1f  %s (candidates of image 0, all classes: %d of %d rows)'
              % (kind, k, m, np.median(times), min(times), max(times), cnt[0].tolist(), cand, nb))


def from_trace(path, reps):
    with open(path) as fh:
        recs = [r for r in csv.DictReader(fh) if 'nms_kernel' in r['Kernel_Name']]
    recs.sort(key=lambda r: int(r['Start_Timestamp']))
    per = WARMUP + reps
    cf = configs()
    if len(recs) != per * len(cf):
        raise SystemExit('%d NMS kernels in the trace, expected %d' % (len(recs), per * len(cf)))
    print('%-7s %2s %-14s %-28s %10s %10s %10s' % ('rows', 'K', 'method', 'kernel', 'median us', 'min us', 'max us'))
    for i, (kind, k, m) in enumerate(cf):
        chunk = recs[i * per + WARMUP:(i + 1) * per]
        us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in chunk]
        name = chunk[0]['Kernel_Name']
        name = name[name.index('void ') + 5:] if 'void ' in name else name
        print('%-7s %2d %-14s %-28s %10.1f %10.1f %10.1f' % (kind, k, m, name[:28], np.median(us), min(us), max(us)))


def eval_loop(n_images):
    import torch
    import build_lmdb
    import evaluate
    from yolo3 import lmdbio
    from yolo3.model import YoloV3
    import bench
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
        items = []
        for i in range(n_images):
            g = int(rng.integers(3, 12))
            wh = rng.integers(30, 120, (g, 2))
            xy = np.stack([rng.integers(0, 416 - wh[:, 0]), rng.integers(0, 416 - wh[:, 1])], 1)
            boxes = np.concatenate([xy, wh, rng.integers(0, 2, (g, 1))], 1).astype(np.int32)
            items.append(build_lmdb.make_record(rng.integers(0, 256, (416, 416, 3), dtype=np.uint8), boxes, i, 'img%04d' % i))
        db = os.path.join(tmp, 'eval.lmdb')
        lmdbio.write_environment(db, items)
        model = os.path.join(tmp, 'model.npz')
        YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, seed=1).save_weights(model)
        evaluate.evaluate(evaluate.database_examples(db), model, 32, batch_size=8)        # warm-up
        print('evaluate.py loop, %d images of 416^2, batch 8, random-weight model, K = 2, --min-box-size 32' % n_images)
        print('%-14s %10s %10s %10s %12s' % ('--nms', 'seconds', 'images/s', 'mAP50', 'detections'))
        for m in METHODS:
            res, count, secs = evaluate.evaluate(evaluate.database_examples(db), model, 32, batch_size=8, nms=m)
            torch.cuda.synchronize()
            det = int(res['tp'][:, 0].sum() + res['fp'][:, 0].sum())
            print('%-14s %10.3f %10.1f %10.4f %12d' % (m, secs, count / secs, res['map50'], det))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else 10)
    elif args and args[0] == '--eval':
        eval_loop(int(args[1]))
    else:
        run(int(args[0]) if args else 10)
