"""CPU tests of the per-class score cut and the confusion matrix: the NumPy restatement
(tests/confusion_reference.py) on the worked example, its invariants and its agreement with the class-wise reference for one class;
metrics.load_score_thresholds against evaluate.write_operating_points; bbox_utils.filter_class_scores; host-side validation of
the new entry points and of DetectionEvaluator's new arguments."""
import os

import numpy as np
import pytest

import confusion_reference as cr
import eval_reference as ref
import eval_ranges_reference as rr

INF = float('inf')


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_worked_example():
    want = cr.confusion([cr.WORKED_DET], [cr.WORKED_GT], 2, [0.5, 0.9])
    assert want['confusion'][0].tolist() == [[0, 1, 0], [0, 1, 0], [2, 0, 0]]           # d0 steals g0, d1 becomes background
    assert want['confusion'][1].tolist() == [[0, 1, 0], [0, 0, 1], [2, 1, 0]]
    assert want['steals'].tolist() == [1, 1]
    # the class-wise metric counts d1 as a TP at both thresholds
    cw = ref.evaluate([cr.WORKED_DET], [cr.WORKED_GT], 2, [0.5, 0.9])
    assert cw['tp'][0].tolist() == [1, 1]


def test_reference_keeps_the_row_and_column_sums():
    for seed in range(6):
        K = (1, 2, 5)[seed % 3]
        dets, gts = cr.seeded_set(seed, 4, K)
        for max_det in (None, 3):
            want = cr.confusion(dets, gts, K, [0.3, 0.5, 0.75], max_det)
            M = want['confusion']
            assert np.array_equal(M[:, :K, :].sum(2), np.tile(want['npos'], (3, 1)))
            assert np.array_equal(M[:, :, :K].sum(1), np.tile(want['entries'], (3, 1)))
            assert not M[:, K, K].any() and M.min() >= 0


def test_one_class_is_the_classwise_matching():
    """K = 1: class-agnostic and class-wise matching coincide, so M[t, 0, 0] is the TP count at every threshold."""
    for seed in range(8):
        dets, gts, _ = rr.seeded_set(seed, K=1)
        thr = ref.COCO
        max_det = 3 if seed % 3 == 0 else None
        M = cr.confusion(dets, gts, 1, thr, max_det)['confusion']
        cw = ref.evaluate(dets, gts, 1, thr, max_det)
        assert np.array_equal(M[:, 0, 0], cw['tp'][0]) and np.array_equal(M[:, 1, 0], cw['fp'][0])
        assert np.array_equal(M[:, 0, 1], cw['npos'][0] - cw['tp'][0])


def test_pooled_order_breaks_score_ties_by_class_then_keep_rank():
    det = (np.zeros((5, 4), np.float32), np.array([0.5, 0.5, 0.9, 0.5, 0.5], np.float32), np.array([1, 0, 1, 0, 1], np.int32), None)
    order, tie = cr.pooled_order(det, 2)
    assert order == [2, 3, 1, 4, 0] and tie              # class 0 first; inside a class the higher row index first
    assert cr.pooled_order(det, 2, max_det=1) == ([2, 3], False)


def test_cut_counts_is_a_prefix_rule():
    sc = np.array([[0.9, 0.5, 0.5, 0.2], [0.9, 0.1, 0.8, 0.0]], np.float32)
    assert cr.cut_counts([4, 4], sc, [0.5, 0.5]).tolist() == [3, 1]          # equal to the threshold: kept; a later 0.8 is not looked at
    assert cr.cut_counts([9, -2], sc, [-INF, -INF]).tolist() == [4, 0]       # stored count above max_keep / below 0
    assert cr.cut_counts([4, 4], sc, [1.0, 0.9]).tolist() == [0, 1]


# ---- load_score_thresholds -------------------------------------------------------------------------------------------------------
def _operating_result(best_score, names=('all', 'small')):
    A, K, T = best_score.shape
    z = np.zeros((A, K, T))
    return {'ap': np.zeros((K, T)), 'area_names': list(names), 'iou_thresholds': np.asarray(ref.COCO[:T], np.float32), 'best_score': best_score,
            'best_precision': z, 'best_recall': z, 'best_f1': z, 'best_tp': z.astype(np.int64), 'best_fp': z.astype(np.int64),
            'npos_area': np.ones((K, A), np.int64)}


def test_load_score_thresholds_round_trips_an_operating_points_file(tmp_path):
    import evaluate
    from yolo3 import metrics
    rng = np.random.default_rng(3)
    best = rng.random((2, 3, 2)).astype(np.float32)
    best[0, 1, 0] = np.float32(np.nan)                        # a class without entries or ground truth: an empty cell
    best[1, 2, 1] = np.float32(1e-7)
    path = os.path.join(str(tmp_path), 'op.csv')
    evaluate.write_operating_points(_operating_result(best), path)
    got = metrics.load_score_thresholds(path, 3)
    assert got.dtype == np.float32 and got[1] == -INF
    assert got[[0, 2]].tobytes() == best[0, [0, 2], 0].tobytes()
    got = metrics.load_score_thresholds(path, 3, 'small', ref.COCO[1])
    assert got.tobytes() == best[1, :, 1].tobytes()
    assert metrics.load_score_thresholds(path, 3, iou=0.5).tobytes() == metrics.load_score_thresholds(path, 3).tobytes()
    # a number: one cut for every class
    assert metrics.load_score_thresholds('0.25', 3).tolist() == [0.25] * 3 and metrics.load_score_thresholds(0.5, 2).tolist() == [0.5, 0.5]
    assert metrics.load_score_thresholds('-inf', 2).tolist() == [-INF, -INF]
    # refusals name what is missing
    with pytest.raises(ValueError, match='medium'):
        metrics.load_score_thresholds(path, 3, 'medium')
    with pytest.raises(ValueError, match='0.9'):
        metrics.load_score_thresholds(path, 3, 'all', 0.9)
    with pytest.raises(ValueError, match='4 classes'):
        metrics.load_score_thresholds(path, 4)
    with pytest.raises(ValueError, match='2 classes'):
        metrics.load_score_thresholds(path, 2)
    for bad in ('nan', float('nan'), 'inf', [0.1, float('nan')], [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError):
            metrics.load_score_thresholds(bad, 2)
    lines = open(path).read().splitlines()
    holed = os.path.join(str(tmp_path), 'holed.csv')
    open(holed, 'w').write('\n'.join(ln for ln in lines if not ln.startswith('1,all,')) + '\n')
    with pytest.raises(ValueError, match='class 1 is missing'):
        metrics.load_score_thresholds(holed, 3)
    nan_file = os.path.join(str(tmp_path), 'nan.csv')
    open(nan_file, 'w').write('\n'.join(lines[:1] + [ln.replace(ln.split(',')[3], 'nan', 1) if ln.startswith('0,all,') else ln
                                                    for ln in lines[1:]]) + '\n')
    with pytest.raises(ValueError, match='finite'):
        metrics.load_score_thresholds(nan_file, 3)


# ---- filter_class_scores ---------------------------------------------------------------------------------------------------------
def test_filter_class_scores():
    from yolo3 import bbox_utils
    thr = bbox_utils.check_class_thresholds([0.5, np.float32(0.3), -INF], 3)
    boxes = np.arange(24, dtype=np.float32).reshape(6, 4)
    scores = np.array([0.5, 0.49999997, 0.3, 0.29999998, 0.0, 0.9], np.float32)
    labels = np.array([0, 0, 1, 1, 2, 1], np.int32)
    rows = np.arange(6, dtype=np.int32) + 10
    dets = [(boxes, scores, labels, rows), (None, None, None, None), (boxes[:2], np.array([0.1, 0.2], np.float32), np.array([0, 1], np.int32), None),
            (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), None)]
    out = bbox_utils.filter_class_scores(dets, thr)
    assert out[0][1].tolist() == scores[[0, 2, 4, 5]].tolist() and out[0][2].tolist() == [0, 1, 2, 1]      # exactly at the threshold: kept
    assert np.array_equal(out[0][0], boxes[[0, 2, 4, 5]]) and out[0][3].tolist() == [10, 12, 14, 15]
    assert out[1] == (None,) * 4 and out[2] == (None,) * 4 and out[3] == (None,) * 4
    want = cr.filter_dets(dets, thr)
    for a, b in zip(out, want):
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))
    # the [M, 6] array of the tiled pipeline, float64 holding float32 scores
    arr = np.concatenate([boxes, scores[:, None], labels[:, None]], 1).astype(np.float64)
    got = bbox_utils.filter_class_scores(arr, thr)
    assert got.dtype == np.float64 and np.array_equal(got, arr[[0, 2, 4, 5]])
    assert bbox_utils.filter_class_scores(arr[:0], thr).shape == (0, 6)
    with pytest.raises(ValueError):
        bbox_utils.filter_class_scores(np.zeros((3, 5)), thr)


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_class_thresholds_are_checked():
    from yolo3 import bbox_utils
    assert bbox_utils.check_class_thresholds(0.25, 3).tolist() == [0.25] * 3
    got = bbox_utils.check_class_thresholds([0.1, -INF], 2)
    assert got.dtype == np.float32 and got.tolist() == [float(np.float32(0.1)), -INF]
    for bad, K in ((float('nan'), 2), ([0.1, float('nan')], 2), (INF, 1), ([0.1], 2), ([0.1, 0.2, 0.3], 2), ([[0.1, 0.2]], 2), ('x', 1)):
        with pytest.raises(ValueError):
            bbox_utils.check_class_thresholds(bad, K)


def test_evaluator_arguments_and_merge_refusals():
    from yolo3 import metrics
    for bad in (float('nan'), [0.1], [0.1, 0.2, 0.3], INF):
        with pytest.raises(ValueError):
            metrics.DetectionEvaluator(2, device='cpu', class_score_thresholds=bad)
    plain = metrics.DetectionEvaluator(2, device='cpu')
    assert plain.class_score_thresholds is None and not plain.confusion
    assert set(plain.state()) == {'keys', 'tp', 'image_counts', 'npos', 'num_images', 'iou_thresholds', 'num_classes', 'max_detections'}
    ev = metrics.DetectionEvaluator(2, [0.5, 0.75], device='cpu', class_score_thresholds=0.3, confusion=True)
    st = ev.state()
    assert set(st) - set(plain.state()) == {'class_score_thresholds', 'confusion'}
    assert st['class_score_thresholds'].tolist() == [float(np.float32(0.3))] * 2 and tuple(st['confusion'].shape) == (2, 3, 3)
    merged = metrics.DetectionEvaluator.merge([st, ev.state()], device='cpu')
    assert merged.confusion and merged.class_score_thresholds.tobytes() == st['class_score_thresholds'].tobytes()
    others = (metrics.DetectionEvaluator(2, [0.5, 0.75], device='cpu', confusion=True),
              metrics.DetectionEvaluator(2, [0.5, 0.75], device='cpu', class_score_thresholds=[0.3, 0.31], confusion=True),
              metrics.DetectionEvaluator(2, [0.5, 0.75], device='cpu', class_score_thresholds=0.3))
    for other in others:
        with pytest.raises(ValueError, match='class_score_thresholds'):
            metrics.DetectionEvaluator.merge([st, other.state()], device='cpu')
        with pytest.raises(ValueError, match='confusion'):
            metrics.DetectionEvaluator.merge([other.state(), st], device='cpu')


def test_entry_points_reject_bad_arguments_without_device():
    from yolo3 import _hip
    L = _hip.lib
    assert L.y3_keep_cut(None, 64, 4, 2, 8, 64, None) == -1 and b'null' in L.y3_last_error()
    assert L.y3_keep_cut(64, None, 4, 2, 8, 64, None) == -1 and L.y3_keep_cut(64, 64, 4, 2, 8, None, None) == -1
    assert L.y3_keep_cut(64, 64, 0, 2, 8, 64, None) == -1 and L.y3_keep_cut(64, 64, 4, 0, 8, 64, None) == -1
    assert L.y3_keep_cut(64, 64, 4, 2, 0, 64, None) == -1
    assert L.y3_keep_cut(64, 64, 5, 2, 8, 64, None) == -1 and b'whole images' in L.y3_last_error()

    assert L.y3_eval_confusion_workspace_bytes(100) == 400 and L.y3_eval_confusion_workspace_bytes(0) == 0
    assert L.y3_eval_confusion_workspace_bytes(-1) == 0
    good = dict(rows=64, n=1, nb=4, ld=7, K=2, keep_idx=64, keep_cnt=64, keep_score=64, max_keep=4, max_det=4, gt=64, gt_cnt=64, max_gt=3,
                per_image=3, thr=_hip.float_array([0.5]), T=1, offsets=64, total=5, ws=64, wb=20, out=64)

    def confusion(**kw):
        a = dict(good, **kw)
        return L.y3_eval_confusion(a['rows'], a['n'], a['nb'], a['ld'], a['K'], -1.0, -1.0, a['keep_idx'], a['keep_cnt'], a['keep_score'],
                                   a['max_keep'], a['max_det'], a['gt'], a['gt_cnt'], a['max_gt'], a['per_image'], a['thr'], a['T'],
                                   a['offsets'], a['total'], a['ws'], a['wb'], a['out'], None)
    for k in ('rows', 'keep_idx', 'keep_cnt', 'keep_score', 'gt', 'gt_cnt', 'thr', 'offsets', 'out'):
        assert confusion(**{k: None}) == -1 and b'null' in L.y3_last_error(), k
    assert confusion(T=0) == -1 and b'thresholds' in L.y3_last_error()
    assert confusion(T=33) == -1
    assert confusion(per_image=4097, max_gt=5000) == -1 and b'4096' in L.y3_last_error() and b'one image' in L.y3_last_error()
    assert confusion(ws=None) == -1 and b'workspace' in L.y3_last_error()
    assert confusion(wb=19) == -1 and b'workspace' in L.y3_last_error()
    assert confusion(n=0) == -1 and confusion(max_det=0) == -1 and confusion(ld=3) == -1 and confusion(total=-1) == -1
    assert confusion(thr=_hip.float_array([0.0])) == -1 and confusion(thr=_hip.float_array([float('nan')])) == -1
