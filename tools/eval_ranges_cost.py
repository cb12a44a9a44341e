"""Cost of the evaluation by area range on one MI355X, against the existing evaluation kernels in the same run.

python tools/eval_ranges_cost.py [repetitions]
    Two inputs: the decode rows of 8 x 416 x 416 images (random-init weights, 2 classes, 20 random GT boxes per image), fed
    with add_batch, and the pool of one synthetic 4096 x 4096 image cut into 608 x 608 tiles (bf16 convs), fed with add_pool.
    Each goes `repetitions` times through a default evaluator, one with curves (A = 1) and one with the COCO ranges and
    curves (A = 4), ALTERNATED, then result() once each; prints the pool sizes.  Run under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/eval_ranges_cost.py 5
    (a run of its own, no counters) for the kernel times, and
python tools/eval_ranges_cost.py --trace DIR/.../*_kernel_trace.csv
    prints every eval_* kernel by grid and workgroup size: launches, median, min and max in microseconds.  The ten COCO
    thresholds give the match kernels 640 threads at A = 1 and 1024 at A = 4; the AP grids are classes x A x 10.
python tools/eval_ranges_cost.py --default
    the same inputs through the default evaluator alone: its trace must hold eval_offsets_kernel, eval_match_kernel and
    eval_ap_kernel and no *_ranges kernel.
python tools/eval_ranges_cost.py --cli DIR [images]
    writes a synthetic lmdb of 416 x 416 images and a random-init model into DIR and runs evaluate.py on it three times
    without and three times with --area-ranges coco --operating-points --pr-curves, alternated; prints evaluate.py's own
    'Evaluated ...' lines (host clock around a device synchronise, model load excluded)."""
import csv
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)
import numpy as np   # noqa: E402

K = 2
ANCHORS = [(64, 384), (384, 64)]      # bench.py's


def random_gt(rng, count, size):
    wh = rng.integers(12, 160, (count, 2))
    xy = np.stack([rng.integers(0, size - wh[:, 0]), rng.integers(0, size - wh[:, 1])], 1)
    return np.concatenate([xy, wh, rng.integers(0, K, (count, 1))], 1)


def run(reps, default_only=False):
    import torch
    import inference_tiled
    from yolo3 import metrics
    from yolo3.model import YoloV3
    rng = np.random.default_rng(4)
    settings = [('default', {}), ('A = 1, curves', {'curves': True}), ('A = 4 (coco), curves', {'area_ranges': 'coco', 'curves': True})]
    if default_only:
        settings = settings[:1]

    y = YoloV3(8, [416, 416, 3], K, ANCHORS, seed=1)
    rows = y.predict(torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(4)).cuda()).clone()
    gts = [random_gt(rng, 20, 416) for _ in range(8)]
    evs = [metrics.DetectionEvaluator(K, **kw) for _, kw in settings]
    for _ in range(reps + 1):                 # the first pass warms up; every pass is in the trace
        for ev in evs:
            ev.add_batch(rows, gts, 32, clip_wh=(416, 416))
    for (name, _), ev in zip(settings, evs):
        res = ev.result()
        print('rows 8 x 416^2: %-22s pool %6d entries, mAP50 %.4f' % (name, ev._used, res['map50']))
    torch.cuda.synchronize()

    y = YoloV3(25, [608, 608, 3], K, ANCHORS, seed=1, use_graph=True)
    y.inference_precision = 'bf16'
    big = rng.integers(0, 256, (4096, 4096, 3), dtype=np.uint8)
    pool, count, _ = inference_tiled.tiled_pool_device(y.get_keras_model(), big, [608, 608], 32)
    gt = random_gt(rng, 400, 4096)
    evs = [metrics.DetectionEvaluator(K, **kw) for _, kw in settings]
    for _ in range(reps + 1):
        for ev in evs:
            ev.add_pool(pool, count, gt)
    for (name, _), ev in zip(settings, evs):
        res = ev.result()
        print('tiled 4096^2:   %-22s pool %6d entries (%d per image), mAP50 %.4f' % (name, ev._used, count, res['map50']))
    torch.cuda.synchronize()


def from_trace(path):
    groups = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r['Kernel_Name'].split('(')[0]
            if 'eval_' not in name:
                continue
            key = (name[-40:], r.get('Grid_Size_X', r.get('Grid_Size', '')), r.get('Workgroup_Size_X', r.get('Workgroup_Size', '')))
            groups.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print('%-40s %-10s %-10s %8s %10s %10s %10s' % ('kernel', 'grid x', 'block x', 'launches', 'median us', 'min us', 'max us'))
    for key in sorted(groups):
        us = groups[key]
        print('%-40s %-10s %-10s %8d %10.2f %10.2f %10.2f' % (key + (len(us), np.median(us), min(us), max(us))))


def cli(out_dir, images):
    import build_lmdb
    from yolo3 import lmdbio
    from yolo3.model import YoloV3
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(5)
    items = []
    for i in range(images):
        img = rng.integers(0, 256, (416, 416, 3), dtype=np.uint8)
        items.append(build_lmdb.make_record(img, random_gt(rng, int(rng.integers(1, 12)), 416).astype(np.int32), i, 'img%04d' % i))
    db = os.path.join(out_dir, 'test-syn.lmdb')
    lmdbio.write_environment(db, items)
    model = os.path.join(out_dir, 'model.npz')
    YoloV3(8, [416, 416, 3], K, ANCHORS, seed=1).save_weights(model)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    base = [sys.executable, os.path.join(PKG, 'evaluate.py'), '--saved-model-filepath', model, '--database', db]
    flags = ['--area-ranges', 'coco', '--operating-points', os.path.join(out_dir, 'op.csv'), '--pr-curves', os.path.join(out_dir, 'pr.csv')]
    for rep in range(3):
        for name, extra in (('without', []), ('with   ', flags)):
            r = subprocess.run(base + extra, env=env, capture_output=True, text=True, check=True)
            print(name, [ln for ln in r.stdout.splitlines() if ln.startswith('Evaluated')][0])


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1])
    elif args and args[0] == '--cli':
        cli(args[1], int(args[2]) if len(args) > 2 else 96)
    elif args and args[0] == '--default':
        run(1, default_only=True)
    else:
        run(int(args[0]) if args else 5)
