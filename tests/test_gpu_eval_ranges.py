"""GPU tests of the metric by area range, the best-F1 cut and the PR curve (y3_eval_match_ranges / y3_eval_ap_ranges,
yolo3.metrics.DetectionEvaluator(area_ranges=..., curves=...), evaluate.py) against the NumPy restatement of
tests/eval_ranges_reference.py: TP and ignore masks, every integer count, best_n / best_tp / best_score and both PR curve
arrays bit for bit; AP and recall within the 1e-6 of test_gpu_metrics.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_reference as ref
import eval_ranges_reference as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
INF = float('inf')
EIGHT_RANGES = rr.TEST_RANGES + [(0.0, 100.0), (100.0, 400.0), (400.0, 1600.0), (64.0, 900.0)]
THIRTY_TWO = [float(v) for v in np.linspace(0.05, 0.98, 32).astype(np.float32)]


def _feed(ev, dets, gts, batch=8):
    for b0 in range(0, len(dets), batch):
        d = dets[b0:b0 + batch]
        ev.add_detections([x[0] for x in d], [x[1] for x in d], [x[2] for x in d], gts[b0:b0 + batch], [x[3] for x in d])
    return ev


def _evaluate(dets, gts, K, thresholds, ranges, max_det=None, batch=8, curves=True):
    from yolo3 import metrics
    ev = _feed(metrics.DetectionEvaluator(K, thresholds, max_det, area_ranges=ranges, curves=curves), dets, gts, batch)
    return ev, ev.result()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def _compare_result(res, want):
    assert _same(res['npos_area'], want['npos_area'])
    for k in ('tp', 'fp', 'ign'):
        assert _same(res[k + '_area'], want[k]), (k, np.nonzero(res[k + '_area'] != want[k]))
    for k in ('ap', 'recall'):
        got = res[k + '_area']
        assert np.array_equal(np.isnan(got), np.isnan(want[k])), k
        assert np.allclose(got, want[k], rtol=0, atol=1e-6, equal_nan=True), (k, np.nanmax(np.abs(got - want[k])))
    if 'best_score' in res:
        assert _same(res['best_tp'], want['best_tp']), np.nonzero(res['best_tp'] != want['best_tp'])
        assert _same(res['best_tp'] + res['best_fp'], want['best_n'])
        assert res['best_score'].dtype == np.float32 and _same(res['best_score'], want['best_score'])
        for k in ('pr_precision', 'pr_score'):
            assert res[k].dtype == np.float32 and _same(res[k], want[k]), (k, np.nonzero(~((res[k] == want[k]) | np.isnan(want[k]))))


def _compare(ev, res, want):
    cls, score, tp, ign = ev.matches()
    assert np.array_equal(cls, want['classes']) and np.array_equal(score, want['scores'])
    assert _same(tp, want['tp_masks']), np.nonzero(tp != want['tp_masks'])
    assert _same(ign, want['ign_masks']), np.nonzero(ign != want['ign_masks'])
    _compare_result(res, want)


# ---- (range, threshold) pair counts: 1 pair, 40 (a third pass of the 16 waves), 256 -----------------------------------
def test_one_pair_random_sets():
    """A * T = 1 with a bounded range, 24 sets, max_detections on some."""
    seen = np.zeros(4, np.int64)
    for seed in range(24):
        dets, gts, K = rr.seeded_set(seed)
        max_det = [None, 3][seed % 2] if seed % 3 == 0 else None
        ranges = [rr.TEST_RANGES[1 + seed % 3]]
        ev, res = _evaluate(dets, gts, K, [0.5], ranges, max_det, batch=1 + seed % 5)
        want = rr.evaluate(dets, gts, K, [0.5], ranges, max_det)
        _compare(ev, res, want)
        seen += want['outcomes'][0]
    assert np.all(seen > 0)


def test_forty_pairs_random_sets_reach_every_outcome():
    """COCO's ten thresholds x four ranges; through the reference: every outcome and the fall-through of rule 2 occur in
    every bounded range."""
    tot, fell = np.zeros((4, 4), np.int64), np.zeros(4, np.int64)
    for seed in range(8):
        dets, gts, K = rr.seeded_set(seed)
        ev, res = _evaluate(dets, gts, K, ref.COCO, rr.TEST_RANGES, batch=1 + seed % 4)
        want = rr.evaluate(dets, gts, K, ref.COCO, rr.TEST_RANGES)
        _compare(ev, res, want)
        tot += want['outcomes']
        fell += want['fell']
    assert np.all(tot[1:] > 0) and np.all(fell[1:] > 0), (tot, fell)


def test_256_pairs():
    dets, gts, K = rr.seeded_set(1, n=12, K=2)
    ev, res = _evaluate(dets, gts, K, THIRTY_TWO, EIGHT_RANGES, batch=4)
    want = rr.evaluate(dets, gts, K, THIRTY_TWO, EIGHT_RANGES)
    _compare(ev, res, want)
    assert np.all(want['outcomes'][1:] > 0) and want['tp_masks'].max() >= 2 ** 31             # bit 31 of a mask word is in use


# ---- many GT boxes / detections per (image, class) ------------------------------------------------------------------------
def test_many_gt_and_detections_per_class():
    """300 GT boxes in one (image, class), in and out of every range, with duplicates: every lane owns several boxes of both
    tiers; more than 64 detections in the segment: a second staging chunk."""
    dets, gts, K = rr.seeded_set(10, n=3, K=2, max_gt=300, max_extra=40)
    gts[0] = np.concatenate([gts[0], np.tile(np.array([[10, 10, 20, 20, 1]]), (70, 1)), np.tile(np.array([[10, 10, 12, 12, 1]]), (70, 1))])
    extra = rr.xywh_to_corners(np.array([[10, 10, 20, 20]] * 5 + [[11, 10, 20, 20]] * 3 + [[10, 10, 12, 12]] * 80))
    d0 = dets[0]
    assert d0[0] is not None
    dets[0] = (np.concatenate([d0[0], extra]), np.concatenate([d0[1], np.full(len(extra), 0.5, np.float32)]),
               np.concatenate([d0[2], np.ones(len(extra), np.int32)]), None)
    per_class = np.bincount(gts[0][:, 4].astype(np.int64))
    assert per_class.max() > 128 and np.bincount(dets[0][2]).max() > 64
    area = gts[0][gts[0][:, 4] == 1][:, 2] * gts[0][gts[0][:, 4] == 1][:, 3]
    assert (area <= 256).sum() > 64 and (area > 256).sum() > 64
    thr = [0.1, 0.5, 0.9]
    ev, res = _evaluate(dets, gts, K, thr, rr.TEST_RANGES)
    want = rr.evaluate(dets, gts, K, thr, rr.TEST_RANGES)
    _compare(ev, res, want)
    assert np.all(want['fell'][1:] > 0)


# ---- long class segments of the sorted pool, pool growth -------------------------------------------------------------------
def test_long_segments_chunk_boundaries_and_pool_growth():
    """Class segments of more than 256 sorted entries: ignored entries on both sides of a 256-entry chunk boundary and an
    equal-score run across one; more than 1024 entries over several batches, so the [M, A] pools grow twice."""
    dets, gts, K = rr.seeded_set(11, n=140, K=2)
    rng = np.random.default_rng(11)
    dets = [d if d[0] is None else (d[0], np.where(rng.random(len(d[1])) < 0.8, d[1], rng.random(len(d[1])).astype(np.float32)), d[2], None)
            for d in dets]
    thr = [0.5, 0.75]
    ev, res = _evaluate(dets, gts, K, thr, rr.TEST_RANGES, batch=17)
    assert ev._keys.numel() > 1024 and ev._tp.shape == (ev._keys.numel(), 4)
    want = rr.evaluate(dets, gts, K, thr, rr.TEST_RANGES)
    _compare(ev, res, want)
    # what the kernel's chunks see: the class-sorted pool (score descending, stable)
    for c in range(K):
        sel = np.nonzero(want['classes'] == c)[0]
        sel = sel[np.argsort(-want['scores'][sel].astype(np.float64), kind='stable')]
        assert len(sel) > 512
        sc = want['scores'][sel]
        assert sc[255] == sc[256] and sc[511] == sc[512]                       # equal-score runs across both chunk boundaries
        for a in (1, 2, 3):
            ign = want['ign_masks'][sel, a] & 1
            assert ign[:256].any() and ign[256:512].any() and not ign[:256].all() and not ign[256:512].all()
    assert np.all(want['best_n'][:, :, :] > 0)


def test_over_cap_batch_is_refused_and_leaves_the_state_untouched():
    from yolo3 import metrics
    from yolo3._hip import HipError
    dets, gts, K = rr.seeded_set(2, n=3, K=1)
    ev, before = _evaluate(dets, gts, K, [0.5], rr.TEST_RANGES)
    m0 = ev.matches()
    rng = np.random.default_rng(2)
    big = np.concatenate([rng.integers(0, 2000, (4097, 2)), rng.integers(4, 30, (4097, 2)), np.zeros((4097, 1), np.int64)], 1)
    with pytest.raises(HipError, match='4096'):
        ev.add_detections([dets[0][0]], [dets[0][1]], [dets[0][2]], [big])
    after = ev.result()
    for a, b in zip(m0, ev.matches()):
        assert np.array_equal(a, b)
    assert ev.num_images == 3 and _same(before['npos_area'], after['npos_area'])
    for k in ('ap_area', 'tp_area', 'fp_area', 'ign_area', 'best_score', 'pr_score'):
        assert _same(before[k], after[k]), k
    ev.add_detections([dets[0][0]], [dets[0][1]], [dets[0][2]], [big[:4096]])                    # exactly the cap fits
    assert ev.result()['npos_area'][0, 0] == before['npos_area'][0, 0] + 4096


# ---- the existing path ----------------------------------------------------------------------------------------------------------
def test_all_range_is_the_default_evaluator_bit_for_bit():
    from yolo3 import metrics
    for seed, thr, max_det in ((1, ref.COCO, None), (4, [0.5], 3), (11, [0.3, 0.5, 0.9], None)):
        dets, gts, K = rr.seeded_set(seed, n=40 if seed == 11 else None, K=2 if seed == 11 else None)
        old = _feed(metrics.DetectionEvaluator(K, thr, max_det), dets, gts, 5)
        r_old = old.result()
        for kw in (dict(area_ranges=[(-INF, INF)]), dict(curves=True)):
            new = _feed(metrics.DetectionEvaluator(K, thr, max_det, **kw), dets, gts, 5)
            r_new = new.result()
            c0, s0, tp0 = old.matches()
            c1, s1, tp1, ign1 = new.matches()
            assert np.array_equal(c0, c1) and np.array_equal(s0, s1) and np.array_equal(tp0, tp1[:, 0]) and not ign1.any()
            for k, v in r_old.items():
                assert np.asarray(v).tobytes() == np.asarray(r_new[k]).tobytes() and np.asarray(v).dtype == np.asarray(r_new[k]).dtype, k
            assert not r_new['ign_area'].any() and ('pr_score' in r_new) == ('curves' in kw)
            assert set(new.state()) - set(old.state()) == {'ign', 'npos_area', 'area_ranges', 'area_names', 'curves'}
        assert set(old.state()) == {'keys', 'tp', 'image_counts', 'npos', 'num_images', 'iou_thresholds', 'num_classes', 'max_detections'}


# ---- the three input paths ---------------------------------------------------------------------------------------------------
def _synthetic_rows(rng, n, nb, K, gts, size):
    rows = np.zeros((n, nb, 5 + K), np.float32)
    for i in range(n):
        g = gts[i]
        for r in range(nb):
            if len(g) and r % 3 != 2:
                x, y, w, h, _ = g[r % len(g)]
                rows[i, r, :4] = np.array([x, y, x + w, y + h], np.float32) + rng.integers(-6, 7, 4).astype(np.float32) + \
                    rng.random(4).astype(np.float32)
            else:
                x0, y0 = rng.uniform(-20, size, 2)
                rows[i, r, :4] = [x0, y0, x0 + rng.uniform(2, 60), y0 + rng.uniform(2, 60)]
        rows[i, :, 4] = rng.choice(np.array([0.3, 0.6, 0.9], np.float32), nb)
        rows[i, :, 5:] = rng.random((nb, K)).astype(np.float32)
    return rows


def test_input_paths_agree_and_use_the_clipped_area():
    from yolo3 import bbox_utils, metrics
    rng = np.random.default_rng(5)
    K, n, nb, size = 2, 6, 300, 256
    gts = []
    for i in range(n):
        g = int(rng.integers(0, 20))
        gts.append(np.concatenate([rng.integers(0, size - 40, (g, 2)), rng.integers(12, 40, (g, 2)), rng.integers(0, K, (g, 1))], 1))
    rows_host = _synthetic_rows(rng, n, nb, K, gts, size)
    rows = torch.from_numpy(rows_host).cuda()
    ranges = [(-INF, INF), (0.0, 400.0), (400.0, 900.0), (900.0, 1e10)]
    out = bbox_utils.detect(rows, 8, clip_wh=(size, size))
    moved = 0                                         # kept detections whose range changes with the clip
    for i, o in enumerate(out):
        if o[0] is not None:
            raw, cl = rr.area_f32(rows_host[i, o[3], :4]), rr.area_f32(o[0])
            moved += sum(int((rr.in_range(raw, lo, hi) != rr.in_range(cl, lo, hi)).sum()) for lo, hi in ranges[1:])
    assert moved > 0
    for max_det in (None, 5):
        kw = dict(area_ranges=ranges, curves=True)
        dev = metrics.DetectionEvaluator(K, ref.COCO, max_det, **kw)
        dev.add_batch(rows[:4], gts[:4], 8, clip_wh=(size, size))
        dev.add_batch(rows[4:], gts[4:], 8, clip_wh=(size, size))
        host = metrics.DetectionEvaluator(K, ref.COCO, max_det, **kw)
        host.add_detections([o[0] for o in out], [o[1] for o in out], [o[2] for o in out], gts, [o[3] for o in out])
        want = rr.evaluate(out, gts, K, ref.COCO, ranges, max_det)
        assert np.all(want['outcomes'][1:] > 0)
        rd, rh = dev.result(), host.result()
        _compare(dev, rd, want)
        _compare(host, rh, want)
        for k in rd:
            assert np.asarray(rd[k]).tobytes() == np.asarray(rh[k]).tobytes(), k
        # the tiled pipeline's path: each image's detections as a device pool x0, y0, x1, y1, score, class
        pool_ev = metrics.DetectionEvaluator(K, ref.COCO, max_det, **kw)
        for o, g in zip(out, gts):
            if o[0] is None:
                pool_ev.add_pool(torch.zeros(1, 6, device='cuda'), 0, g)
            else:
                pool = torch.from_numpy(np.concatenate([o[0], o[1][:, None], o[2][:, None].astype(np.float32)], 1)).cuda()
                pool_ev.add_pool(pool, len(o[0]), g)
        by_position = [(o[0], o[1], o[2], None) for o in out]
        _compare(pool_ev, pool_ev.result(), rr.evaluate(by_position, gts, K, ref.COCO, ranges, max_det))


# ---- merging --------------------------------------------------------------------------------------------------------------------
RESULT_KEYS = ('ap_area', 'recall_area', 'tp_area', 'fp_area', 'ign_area', 'npos_area', 'best_score', 'best_tp', 'best_fp', 'pr_precision',
               'pr_score', 'ap', 'npos')


def test_merge_of_strided_halves_is_the_single_evaluator():
    from yolo3 import metrics
    dets, gts, K = rr.seeded_set(9, n=11, K=3)
    thr = [0.5, 0.75]
    kw = dict(area_ranges=rr.TEST_RANGES, curves=True)
    one, r_one = _evaluate(dets, gts, K, thr, rr.TEST_RANGES, batch=4)
    halves = [_feed(metrics.DetectionEvaluator(K, thr, **kw), dets[r::2], gts[r::2], 3) for r in range(2)]
    merged = metrics.DetectionEvaluator.merge([h.state() for h in halves])
    assert merged.area_names == one.area_names and merged.curves and merged.num_images == 11
    for a, b in zip(one.matches(), merged.matches()):
        assert np.array_equal(a, b)
    r_m = merged.result()
    for k in r_one:
        assert np.asarray(r_one[k]).tobytes() == np.asarray(r_m[k]).tobytes(), k
    _compare(merged, r_m, rr.evaluate(dets, gts, K, thr, rr.TEST_RANGES))
    # refused: other ranges, ranges against none, curves against none
    a = halves[0].state()
    for other in (metrics.DetectionEvaluator(K, thr, area_ranges=rr.TEST_RANGES[:3], curves=True), metrics.DetectionEvaluator(K, thr),
                  metrics.DetectionEvaluator(K, thr, area_ranges=rr.TEST_RANGES),
                  metrics.DetectionEvaluator(K, thr, area_ranges=[(-INF, INF), (0, 256), (256, 901), (900, 1e10)], curves=True)):
        with pytest.raises(ValueError, match='area_ranges'):
            metrics.DetectionEvaluator.merge([a, _feed(other, dets[1::2], gts[1::2], 3).state()])


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_all_gather_evaluator_two_gloo_ranks(tmp_path):
    seed, n, K = 9, 11, 3
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen(['timeout', '-k', '10', '600', sys.executable, os.path.join(ROOT, 'tests', 'eval_ranges_worker.py'),
                                       str(tmp_path), str(seed), str(n), str(K)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    outs = [p.communicate(timeout=700)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    dets, gts, _ = rr.seeded_set(seed, n, K)
    one, res = _evaluate(dets, gts, K, [0.5, 0.75], rr.TEST_RANGES, batch=4)
    cls, score, tp, ign = one.matches()
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r))
        assert int(z['num_images']) == n and np.array_equal(z['counts'], one.image_counts().cpu().numpy())
        assert np.array_equal(z['cls'], cls) and np.array_equal(z['score'], score)
        assert np.array_equal(z['tp_masks'], tp) and np.array_equal(z['ign_masks'], ign)
        for k in RESULT_KEYS:
            assert z[k].tobytes() == np.asarray(res[k]).tobytes(), k


# ---- evaluate.py end to end -------------------------------------------------------------------------------------------------------
def _write_dataset(tmp, n, size, K=2, seed=5):
    """tests/test_gpu_cli.py's synthetic lmdb recipe."""
    sys.path.insert(0, PKG)
    import build_lmdb
    from yolo3 import lmdbio
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n):
        img = rng.integers(0, 256, size, dtype=np.uint8)
        k = int(rng.integers(1, 4))
        wh = rng.integers(40, 120, (k, 2))
        xy = np.stack([rng.integers(0, size[1] - wh[:, 0]), rng.integers(0, size[0] - wh[:, 1])], 1)
        boxes = np.concatenate([xy, wh, rng.integers(0, K, (k, 1))], 1).astype(np.int32)
        items.append(build_lmdb.make_record(img, boxes, i, 'img%03d' % i))
    lmdbio.write_environment(os.path.join(tmp, 'train-syn.lmdb'), items)


def _csv_rows(path):
    lines = open(path).read().splitlines()
    head = lines[0].split(',')
    return head, [dict(zip(head, ln.split(','))) for ln in lines[1:]]


def _num(cell):
    return float(cell) if cell != '' else float('nan')


def test_evaluate_cli_writes_operating_points_and_pr_curves(tmp_path):
    from yolo3 import bbox_utils, imagereader, lmdbio
    from yolo3.isg_ai_pb import ImageYoloBoxesPair
    from yolo3.model import YoloV3
    tmp = str(tmp_path)
    size, K = (256, 256, 3), 2
    _write_dataset(tmp, 10, size, K)
    model_file = os.path.join(tmp, 'model.npz')
    YoloV3(4, list(size), K, [(48, 48), (90, 60), (60, 90)], seed=7).save_weights(model_file)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    db = os.path.join(tmp, 'train-syn.lmdb')
    e = lmdbio.Environment(db)
    examples = []
    for key in e.keys():
        img, boxes = ImageYoloBoxesPair().ParseFromString(e.get(key)).to_arrays()
        examples.append((img, np.asarray(boxes).reshape(-1, 5)))
    e.close()
    thr = [0.1, 0.3, 0.5]
    names = ['all', '0:4900', '4900:inf']
    ranges = [(-INF, INF), (0.0, 4900.0), (4900.0, INF)]
    files = {k: os.path.join(tmp, k + '.csv') for k in ('out', 'op', 'pr', 'op_tta', 'pr_tta')}
    base = ['timeout', '-k', '10', '600', sys.executable, os.path.join(PKG, 'evaluate.py'), '--saved-model-filepath', model_file, '--database',
            db, '--batch-size', '4', '--min-box-size', '8', '--iou-thresholds'] + [str(t) for t in thr] + ['--area-ranges'] + names
    r = subprocess.run(base + ['--output-file', files['out'], '--operating-points', files['op'], '--pr-curves', files['pr']], env=env,
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in names:
        assert any(ln.startswith('area ') and name in ln and 'AP50 = ' in ln and 'AR = ' in ln for ln in r.stdout.splitlines()), r.stdout[-2000:]

    model = YoloV3.from_file(model_file).get_keras_model()
    dets = []
    for b0 in range(0, len(examples), 4):
        imgs = [ex[0] for ex in examples[b0:b0 + 4]]
        x = torch.from_numpy(np.stack([np.ascontiguousarray(im.astype(np.float32).transpose((2, 0, 1))) for im in imgs])).cuda()
        dets += bbox_utils.detect(model(imagereader.zscore_normalize_device(x), training=False), 8, clip_wh=(size[1], size[0]))
    want = rr.evaluate(dets, [ex[1] for ex in examples], K, thr, ranges)

    head, rows = _csv_rows(files['op'])
    assert head == ['class', 'range', 'iou_threshold', 'score_threshold', 'precision', 'recall', 'f1', 'tp', 'fp', 'npos']
    assert len(rows) == K * len(names) * len(thr)
    it = iter(rows)
    for c in range(K):
        for a, name in enumerate(names):
            for t in range(len(thr)):
                row = next(it)
                n_best, tp, npos = int(want['best_n'][a, c, t]), int(want['best_tp'][a, c, t]), int(want['npos_area'][c, a])
                assert (row['class'], row['range'], np.float32(row['iou_threshold'])) == (str(c), name, np.float32(thr[t]))
                assert (int(row['tp']), int(row['fp']), int(row['npos'])) == (tp, n_best - tp, npos)
                assert np.array_equal(np.float32(_num(row['score_threshold'])), want['best_score'][a, c, t], equal_nan=True)
                if n_best > 0:
                    assert _num(row['precision']) == tp / n_best and _num(row['recall']) == tp / npos and _num(row['f1']) == 2 * tp / (n_best + npos)
    head, rows = _csv_rows(files['pr'])
    assert head == ['class', 'range', 'iou_threshold', 'recall', 'precision', 'score'] and len(rows) == K * len(names) * len(thr) * 101
    got_p = np.array([_num(row['precision']) for row in rows], np.float32).reshape(K, len(names), len(thr), 101).transpose(1, 0, 2, 3)
    got_s = np.array([_num(row['score']) for row in rows], np.float32).reshape(K, len(names), len(thr), 101).transpose(1, 0, 2, 3)
    assert _same(got_p, want['pr_precision']) and _same(got_s, want['pr_score'])
    assert [float(row['recall']) for row in rows[:101]] == [j / 100 for j in range(101)]
    head, rows = _csv_rows(files['out'])
    assert head[:8] == ['class', 'npos', 'tp', 'fp', 'precision', 'recall', 'f1', 'ap'] and head[8:] == ['ap@%.2f' % t for t in thr] + \
        ['ap_' + n for n in names]
    for c in range(K):
        for a, name in enumerate(names):
            w = want['ap'][a, c].mean()
            assert np.isclose(_num(rows[c]['ap_' + name]), w, rtol=0, atol=1e-6, equal_nan=True), (c, name)
    assert rows[K]['class'] == 'mean'

    # the flags pass through the test-time augmentation path (pooled views matched by add_pool)
    r = subprocess.run(base + ['--tta', 'hflip', '--operating-points', files['op_tta'], '--pr-curves', files['pr_tta']], env=env,
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'TTA: hflip' in r.stdout and sum(ln.startswith('area ') for ln in r.stdout.splitlines()) == len(names)
    head, rows = _csv_rows(files['op_tta'])
    assert len(rows) == K * len(names) * len(thr) and [int(row['npos']) for row in rows] == [int(want['npos_area'][c, a]) for c in range(K)
                                                                                         for a in range(len(names)) for _ in thr]
    assert len(_csv_rows(files['pr_tta'])[1]) == K * len(names) * len(thr) * 101
