"""GPU tests of test-set mAP across ranks and in training: DetectionEvaluator.merge against one evaluator fed every image
in order (bit for bit) and against tests/eval_reference.py, all_gather_evaluator over two gloo ranks, evaluate.py under a
two-rank launcher, and train.py --test_map / --model_selection against evaluate.py on the model they saved."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_reference as ref
from test_gpu_metrics import _random_set, _compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')


def make_set(seed, n, K):
    """TP-rich random detections (jittered from GT, a few score levels, so exact score ties across images), several
    classes, some images without GT and some without detections (tests/test_gpu_metrics.py's generator)."""
    return _random_set(np.random.default_rng(seed), n, K)


def feed(ev, dets, gts, batch):
    for b0 in range(0, len(dets), batch):
        d = dets[b0:b0 + batch]
        ev.add_detections([x[0] for x in d], [x[1] for x in d], [x[2] for x in d], gts[b0:b0 + batch], [x[3] for x in d])


def _same(a, b):
    """result() dicts and matches() bit for bit."""
    ra, rb = a.result(), b.result()
    for k in ('ap', 'recall', 'tp', 'fp', 'npos', 'map'):
        assert np.array_equal(ra[k], rb[k], equal_nan=(ra[k].dtype.kind == 'f')), k
    for x, y in zip(a.matches(), b.matches()):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert a.num_images == b.num_images
    assert np.array_equal(a.image_counts().cpu().numpy(), b.image_counts().cpu().numpy())


def _single(dets, gts, K, batch=4):
    from yolo3 import metrics
    ev = metrics.DetectionEvaluator(K)
    feed(ev, dets, gts, batch)
    return ev


def test_merge_strided_and_explicit_orders_are_bit_identical_to_one_evaluator():
    from yolo3 import metrics
    for seed in range(6):
        rng = np.random.default_rng(50 + seed)
        K = int(rng.integers(2, 4))
        n = int(rng.integers(7, 16))
        dets, gts = make_set(seed, n, K)
        one = _single(dets, gts, K)
        want = ref.evaluate(dets, gts, K)
        assert want['tp'][:, 0].sum() > 0                                   # the set has TPs at IoU 0.5
        _compare(one, one.result(), want)
        for W in (2, 3):
            evs = []
            for r in range(W):
                ev = metrics.DetectionEvaluator(K)
                feed(ev, dets[r::W], gts[r::W], batch=1 + (r + seed) % 3)
                evs.append(ev)
            merged = metrics.DetectionEvaluator.merge([e.state() for e in evs])
            _same(merged, one)
            _compare(merged, merged.result(), want)
        # uneven explicit split: state r holds an arbitrary subset in an arbitrary local order
        perm = rng.permutation(n)
        owner = np.split(perm, np.sort(rng.choice(np.arange(1, n), 2, replace=False)))
        evs, where = [], {}
        for r, imgs in enumerate(owner):
            ev = metrics.DetectionEvaluator(K)
            feed(ev, [dets[g] for g in imgs], [gts[g] for g in imgs], batch=2)
            evs.append(ev)
            where.update({int(g): (r, i) for i, g in enumerate(imgs)})
        merged = metrics.DetectionEvaluator.merge([e.state() for e in evs], order=[where[g] for g in range(n)])
        _same(merged, one)


def test_tie_case_needs_the_global_order():
    """Equal scores in different images: image 1 a FP, image 2 a TP, both 0.5.  Split over two ranks (images 0, 2 | 1, 3),
    a rank-major concatenation puts the TP first (AP 1.0); the single-process order puts the FP first (AP 0.5)."""
    from yolo3 import metrics
    box = np.array([[10, 10, 40, 40]], np.float32)
    far = np.array([[100, 100, 130, 130]], np.float32)
    one_gt = np.array([[10, 10, 30, 30, 0]], np.int64)
    no_gt = np.zeros((0, 5), np.int64)
    s, lab = np.array([0.5], np.float32), np.array([0], np.int32)
    dets = [(None,) * 4, (far, s, lab, None), (box, s, lab, None), (None,) * 4]
    gts = [no_gt, no_gt, one_gt, no_gt]
    one = _single(dets, gts, 1)
    assert one.result()['ap'][0, 0] == pytest.approx(0.5, abs=1e-6)
    evs = []
    for r in range(2):
        ev = metrics.DetectionEvaluator(1)
        feed(ev, dets[r::2], gts[r::2], batch=2)
        evs.append(ev)
    states = [e.state() for e in evs]
    _same(metrics.DetectionEvaluator.merge(states), one)
    rank_major = metrics.DetectionEvaluator.merge(states, order=[(0, 0), (0, 1), (1, 0), (1, 1)])
    assert rank_major.result()['ap'][0, 0] == pytest.approx(1.0, abs=1e-6)


def test_merge_rejects_incompatible_evaluators():
    from yolo3 import metrics
    a = metrics.DetectionEvaluator(2)
    for b in (metrics.DetectionEvaluator(3), metrics.DetectionEvaluator(2, [0.5]), metrics.DetectionEvaluator(2, max_detections=10)):
        with pytest.raises(ValueError):
            metrics.DetectionEvaluator.merge([a.state(), b.state()])
    feed(a, *make_set(1, 2, 2), batch=2)
    with pytest.raises(ValueError):                                          # 0 + 2 images is no strided split
        metrics.DetectionEvaluator.merge([metrics.DetectionEvaluator(2).state(), a.state()])


def _free_port():
    from test_gpu_dist import _free_port as fp
    return fp()


def _env():
    return dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))


def _two_ranks(args):
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen(['timeout', '-k', '10', '600', sys.executable, os.path.join(ROOT, 'tests', 'map_worker.py')] + args,
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=700)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    return [np.load(os.path.join(args[0], 'rank%d.npz' % r)) for r in range(2)]


def test_all_gather_evaluator_two_gloo_ranks(tmp_path):
    seed, n, K = 7, 11, 3
    zs = _two_ranks([str(tmp_path), str(seed), str(n), str(K)])
    dets, gts = make_set(seed, n, K)
    one = _single(dets, gts, K)
    res = one.result()
    cls, score, mask = one.matches()
    for r, z in enumerate(zs):
        for k in ('ap', 'recall', 'tp', 'fp', 'npos'):
            assert np.array_equal(z[k], res[k], equal_nan=(res[k].dtype.kind == 'f')), (r, k)
        assert np.array_equal(z['cls'], cls) and np.array_equal(z['score'], score) and np.array_equal(z['mask'], mask)
        assert int(z['num_images']) == n and np.array_equal(z['counts'], one.image_counts().cpu().numpy())


def test_train_map_pass_restores_each_replicas_moving_statistics(tmp_path):
    """After a data-parallel step the two replicas hold different BN moving statistics; the pass swaps their mean in and
    must hand every replica its own values back (and touch no weight), while both ranks get the same merged result."""
    from test_gpu_cli import _write_dataset
    tmp = str(tmp_path)
    _write_dataset(tmp, 15, (160, 160, 3))
    zs = _two_ranks([tmp, 'train', os.path.join(tmp, 'test-syn.lmdb')])
    assert not np.array_equal(zs[0]['own'], zs[1]['own'])
    for z in zs:
        assert np.array_equal(z['after'], z['own']) and bool(z['weights_kept']) and int(z['n']) == 5
        assert np.array_equal(z['mean'], zs[0]['mean']) and z['npos'].sum() > 0
        for k in ('ap', 'tp50', 'fp50', 'npos'):
            assert np.array_equal(z[k], zs[0][k], equal_nan=True), k


def _run(args, timeout=900):
    r = subprocess.run(['timeout', '-k', '10', str(timeout)] + args, env=_env(), capture_output=True, text=True, timeout=timeout + 60)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _torchrun(nproc):
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc), '--master-addr', '127.0.0.1',
            '--master-port', str(_free_port())]


def _evaluate_cli(model, db, batch, out_csv, ranks=1, min_box=8):
    args = [os.path.join(PKG, 'evaluate.py'), '--saved-model-filepath', model, '--database', db, '--batch-size', str(batch),
            '--min-box-size', str(min_box), '--output-file', out_csv]
    if ranks == 1:
        return _run([sys.executable] + args)
    return _run(_torchrun(ranks) + args + ['--backend', 'gloo'])


def _table(stdout):
    lines = stdout.splitlines()
    i = next(k for k, ln in enumerate(lines) if ln.split()[:2] == ['class', 'npos'])
    j = next(k for k, ln in enumerate(lines) if ln.startswith('mAP50 = '))
    return lines[i:j + 1]


def test_evaluate_cli_two_gloo_ranks_equals_one_process(tmp_path):
    from test_gpu_cli import _write_dataset
    from yolo3.model import YoloV3
    tmp = str(tmp_path)
    size = (256, 256, 3)
    _write_dataset(tmp, 9, size)                                             # 9 train records: ranks take 5 and 4
    model = os.path.join(tmp, 'model.npz')
    YoloV3(4, list(size), 2, [(48, 48), (90, 60), (60, 90)], seed=7).save_weights(model)
    db = os.path.join(tmp, 'train-syn.lmdb')
    one = _evaluate_cli(model, db, 1, os.path.join(tmp, 'one.csv'))
    two = _evaluate_cli(model, db, 1, os.path.join(tmp, 'two.csv'), ranks=2)
    assert 'Evaluated 9 images' in one.stdout and two.stdout.count('Evaluated 9 images') == 1     # rank 0 alone prints
    assert _table(two.stdout) == _table(one.stdout)
    a, b = open(os.path.join(tmp, 'one.csv')).read(), open(os.path.join(tmp, 'two.csv')).read()
    assert a == b and a.count('\n') == 2 + 2


# ---- train.py --test_map ------------------------------------------------------------------------------------------------
def _train(tmp, out, extra, ranks=1):
    args = [os.path.join(PKG, 'train.py'), '--batch_size', '2', '--test_every_n_steps', '2', '--train_database', os.path.join(tmp, 'train-syn.lmdb'),
            '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out, '--early_stopping', '5', '--use_augmentation', '0',
            '--max_epochs', '2', '--reader_count', '1', '--learning_rate', '1e-3'] + extra
    if ranks == 1:
        return _run([sys.executable] + args)
    return _run(_torchrun(ranks) + args + ['--backend', 'gloo'])


def _map_csv(out):
    lines = open(os.path.join(out, 'test_map.csv')).read().splitlines()
    assert lines[0] == 'epoch,map50,map50_95,tp50,fp50,npos'
    rows = [ln.split(',') for ln in lines[1:]]
    return [(int(r[0]), float(r[1]), float(r[2]), int(r[3]), int(r[4]), int(r[5])) for r in rows]


def _check_row_against_evaluate(row, csv_path):
    from test_gpu_metrics import _read_csv
    _, rows = _read_csv(csv_path)
    mean = rows['mean']
    classes = [v for k, v in rows.items() if k != 'mean']
    assert row[5] == mean['npos'] and row[5] > 0
    assert row[3] == sum(c['tp'] for c in classes) and row[4] == sum(c['fp'] for c in classes)
    assert row[1] == mean['ap@0.50'] and row[2] == mean['ap'], (row, mean)


def test_train_test_map_one_process(tmp_path):
    from test_gpu_cli import _write_dataset
    tmp = str(tmp_path)
    _write_dataset(tmp, 15, (160, 160, 3))                                   # 5 test records: batches of 2, 2 and a tail of 1
    base = _train(tmp, os.path.join(tmp, 'base'), [])                          # default: no pass, no new file, no new line
    assert 'mAP' not in base.stdout and not os.path.exists(os.path.join(tmp, 'base', 'test_map.csv'))
    assert base.stdout.count('Test loss improved') >= 1 and base.stdout.count('Test Epoch: ') == 2
    out = os.path.join(tmp, 'map')
    r = _train(tmp, out, ['--test_map', '1', '--test_map_min_box_size', '8'])
    rows = _map_csv(out)
    assert [x[0] for x in rows] == [0, 1]
    assert r.stdout.count('mAP pass took') == 2 and r.stdout.count('(5 images,') == 2
    losses = [float(v) for v in open(os.path.join(out, 'test_loss.csv')).read().split()]
    assert len(losses) == 2
    best = int(np.argmin(losses))                                            # the epoch the checkpoint holds (first minimum)
    ev = _evaluate_cli(os.path.join(out, 'saved_model'), os.path.join(tmp, 'test-syn.lmdb'), 2, os.path.join(tmp, 'eval.csv'))
    assert 'Evaluated 5 images' in ev.stdout
    _check_row_against_evaluate(rows[best], os.path.join(tmp, 'eval.csv'))

    # --model_selection map50: checkpoint on the first maximum of mAP50, early stopping on it
    out2 = os.path.join(tmp, 'sel')
    r2 = _train(tmp, out2, ['--model_selection', 'map50', '--test_map_min_box_size', '8'])
    rows2 = _map_csv(out2)
    assert [x[0] for x in rows2] == [0, 1] and len(open(os.path.join(out2, 'test_loss.csv')).read().split()) == 2
    assert os.path.exists(os.path.join(out2, 'checkpoint', 'ckpt.npz')) and os.path.exists(os.path.join(out2, 'saved_model', 'yolov3.npz'))
    assert 'Test map50 improved' in r2.stdout and 'Test loss improved' not in r2.stdout
    best2 = int(np.argmax([x[1] for x in rows2]))
    assert r2.stdout.splitlines().count('Best epoch: {}'.format(best2)) >= 1
    _evaluate_cli(os.path.join(out2, 'saved_model'), os.path.join(tmp, 'test-syn.lmdb'), 2, os.path.join(tmp, 'eval2.csv'))
    _check_row_against_evaluate(rows2[best2], os.path.join(tmp, 'eval2.csv'))


def test_train_test_map_two_gloo_ranks(tmp_path):
    """Two ranks: each evaluates its keys[rank::2] share with the MEAN moving statistics swapped in; the row of the
    checkpointed epoch equals evaluate.py on the exported model under two ranks with the same batch size."""
    from test_gpu_cli import _write_dataset
    tmp = str(tmp_path)
    _write_dataset(tmp, 15, (160, 160, 3))
    out = os.path.join(tmp, 'map')
    r = _train(tmp, out, ['--test_map', '1', '--test_map_min_box_size', '8'], ranks=2)
    rows = _map_csv(out)
    assert [x[0] for x in rows] == [0, 1]
    assert r.stdout.count('mAP pass took') == 2 * 2 and r.stdout.count('(5 images,') == 2 * 2     # both ranks print the merged count
    losses = [float(v) for v in open(os.path.join(out, 'test_loss.csv')).read().split()]
    best = int(np.argmin(losses))
    _evaluate_cli(os.path.join(out, 'saved_model'), os.path.join(tmp, 'test-syn.lmdb'), 2, os.path.join(tmp, 'eval.csv'), ranks=2)
    _check_row_against_evaluate(rows[best], os.path.join(tmp, 'eval.csv'))
