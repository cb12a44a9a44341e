"""Cost of the per-class score cut and the confusion matrix on one MI355X, beside eval_match_kernel on the same
inputs in the same run.

python tools/confusion_cost.py [repetitions]
    tools/eval_ranges_cost.py's two inputs: the decode rows of 8 x 416 x 416 images (random-init weights, 2 classes, 20 random GT
    boxes per image), fed with add_batch, and the pool of one synthetic 4096 x 4096 image cut into 608 x 608 tiles (bf16 convs,
    400 GT boxes), fed with add_pool.  Each goes `repetitions` times through a default evaluator, one with confusion=True and one
    with class_score_thresholds=0.3 and confusion=True, ALTERNATED; prints the pool sizes and the matrices' sums.  Run under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/confusion_cost.py 5
    (a run of its own, no counters) for the kernel times, and
python tools/confusion_cost.py --trace DIR/.../*_kernel_trace.csv
    prints eval_offsets / eval_match / eval_pool_rank / eval_confusion / keep_cut by grid and workgroup size: launches, median, min
    and max in microseconds.
python tools/confusion_cost.py --cli DIR [images]
    writes a synthetic lmdb of 416 x 416 images and a random-init model into DIR, runs evaluate.py once with --operating-points and
    then three times without and three times with --score-thresholds op.csv --confusion-matrix cm.csv, alternated; prints
    evaluate.py's own 'Evaluated ...' lines (host clock around a device synchronise, model load excluded)."""
import csv
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_ranges_cost as erc   # noqa: E402  (puts the repository and the package on sys.path)
import numpy as np   # noqa: E402

KERNELS = ('eval_offsets_kernel', 'eval_match_kernel', 'eval_pool_rank_kernel', 'eval_confusion_kernel', 'keep_cut_kernel')


def run(reps):
    import torch
    import inference_tiled
    from yolo3 import metrics
    from yolo3.model import YoloV3
    K = erc.K
    rng = np.random.default_rng(4)
    settings = [('default', {}), ('confusion', {'confusion': True}), ('cut 0.3 + confusion', {'class_score_thresholds': 0.3, 'confusion': True})]

    def report(label, evs, extra=''):
        for (name, _), ev in zip(settings, evs):
            res = ev.result()
            print('%s %-20s pool %6d entries%s, mAP50 %.4f, matrix sum at IoU 0.5 %s' % (
                label, name, ev._used, extra, res['map50'], int(res['confusion_op'].sum()) if 'confusion_op' in res else '-'))
        torch.cuda.synchronize()

    y = YoloV3(8, [416, 416, 3], K, erc.ANCHORS, seed=1)
    rows = y.predict(torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(4)).cuda()).clone()
    gts = [erc.random_gt(rng, 20, 416) for _ in range(8)]
    evs = [metrics.DetectionEvaluator(K, **kw) for _, kw in settings]
    for _ in range(reps + 1):                 # the first pass warms up; every pass is in the trace
        for ev in evs:
            ev.add_batch(rows, gts, 32, clip_wh=(416, 416))
    report('rows 8 x 416^2:', evs)

    y = YoloV3(25, [608, 608, 3], K, erc.ANCHORS, seed=1, use_graph=True)
    y.inference_precision = 'bf16'
    big = rng.integers(0, 256, (4096, 4096, 3), dtype=np.uint8)
    pool, count, _ = inference_tiled.tiled_pool_device(y.get_keras_model(), big, [608, 608], 32)
    gt = erc.random_gt(rng, 400, 4096)
    evs = [metrics.DetectionEvaluator(K, **kw) for _, kw in settings]
    for _ in range(reps + 1):
        for ev in evs:
            ev.add_pool(pool, count, gt)
    report('tiled 4096^2:  ', evs, ' (%d per image)' % count)


def from_trace(path):
    groups = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = next((k for k in KERNELS if k in r['Kernel_Name']), None)
            if name is None:
                continue
            key = (name, r.get('Grid_Size_X', r.get('Grid_Size', '')), r.get('Workgroup_Size_X', r.get('Workgroup_Size', '')))
            groups.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print('%-24s %-10s %-10s %8s %10s %10s %10s' % ('kernel', 'grid x', 'block x', 'launches', 'median us', 'min us', 'max us'))
    for key in sorted(groups):
        us = groups[key]
        print('%-24s %-10s %-10s %8d %10.2f %10.2f %10.2f' % (key + (len(us), np.median(us), min(us), max(us))))


def cli(out_dir, images):
    import build_lmdb
    from yolo3 import lmdbio
    from yolo3.model import YoloV3
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(5)
    items = []
    for i in range(images):
        img = rng.integers(0, 256, (416, 416, 3), dtype=np.uint8)
        items.append(build_lmdb.make_record(img, erc.random_gt(rng, int(rng.integers(1, 12)), 416).astype(np.int32), i, 'img%04d' % i))
    db = os.path.join(out_dir, 'test-syn.lmdb')
    lmdbio.write_environment(db, items)
    model = os.path.join(out_dir, 'model.npz')
    YoloV3(8, [416, 416, 3], erc.K, erc.ANCHORS, seed=1).save_weights(model)
    env = dict(os.environ, PYTHONPATH=erc.PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    base = [sys.executable, os.path.join(erc.PKG, 'evaluate.py'), '--saved-model-filepath', model, '--database', db]
    op = os.path.join(out_dir, 'op.csv')
    subprocess.run(base + ['--operating-points', op], env=env, capture_output=True, text=True, check=True)
    flags = ['--score-thresholds', op, '--confusion-matrix', os.path.join(out_dir, 'cm.csv')]
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
    else:
        run(int(args[0]) if args else 5)
