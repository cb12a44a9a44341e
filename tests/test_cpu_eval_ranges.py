"""CPU tests of the metric by area range, the best-F1 cut and the PR curve: the NumPy restatement
(tests/eval_ranges_reference.py) against the existing reference and on hand-worked cases, one per rule; the shared random sets;
host-side argument validation of the y3_eval_*_ranges entry points and of DetectionEvaluator's new arguments."""
import math

import numpy as np
import pytest

import eval_reference as ref
import eval_ranges_reference as rr

INF = float('inf')


def _det(boxes_xywh, scores, labels=None):
    b = np.asarray(boxes_xywh, np.float64).reshape(-1, 4)
    return rr.xywh_to_corners(b), np.asarray(scores, np.float32), np.zeros(len(b), np.int32) if labels is None else np.asarray(labels, np.int32), None


def _gt(boxes_xywh, labels=None):
    b = np.asarray(boxes_xywh, np.int64).reshape(-1, 4)
    return np.concatenate([b, np.zeros((len(b), 1), np.int64) if labels is None else np.asarray(labels, np.int64).reshape(-1, 1)], 1)


def test_all_range_equals_the_existing_reference():
    for seed in range(24):
        dets, gts, K = rr.seeded_set(seed, mutate=seed >= 12)
        thr = ref.COCO if seed % 2 else [0.5]
        max_det = 3 if seed % 6 == 0 else None
        want = ref.evaluate(dets, gts, K, thr, max_det)
        got = rr.evaluate(dets, gts, K, thr, [(-INF, INF)], max_det)
        assert np.array_equal(got['tp_masks'][:, 0], want['masks']) and not got['ign_masks'].any()
        assert np.array_equal(got['classes'], want['classes']) and np.array_equal(got['scores'], want['scores'])
        assert np.array_equal(got['npos_area'][:, 0], want['npos'])
        for k in ('ap', 'recall', 'tp', 'fp'):
            assert np.array_equal(got[k][0], want[k], equal_nan=True), k
        assert got['outcomes'][0, rr.IGN_GT] == 0 and got['outcomes'][0, rr.IGN_AREA] == 0 and got['fell'][0] == 0


def test_shared_sets_reach_every_outcome_in_every_bounded_range():
    """The generator copied from test_gpu_metrics.py, on the ranges the GPU tests use: TP, GT-ignored, area-ignored, FP and
    the fall-through of rule 2 all occur in each of the three bounded ranges."""
    tot, fell = np.zeros((4, 4), np.int64), np.zeros(4, np.int64)
    for seed in range(24):
        dets, gts, K = rr.seeded_set(seed)
        r = rr.evaluate(dets, gts, K, [0.5, 0.75], rr.TEST_RANGES)
        tot += r['outcomes']
        fell += r['fell']
    print('outcomes per range (FP, TP, GT-ignored, area-ignored):', tot.tolist(), 'fall-through:', fell.tolist())
    assert np.all(tot[1:] > 0) and np.all(fell[1:] > 0)
    assert tot[0, rr.IGN_GT] == 0 and tot[0, rr.IGN_AREA] == 0 and fell[0] == 0


def test_rule1_in_range_box_wins_over_a_better_out_of_range_box():
    # GT 0 (20x20 = 400, out of [0, 256]) fits the detection exactly; GT 1 (16x16 = 256, in range) overlaps with IoU 0.64
    gt = [_gt([[0, 0, 20, 20], [0, 0, 16, 16]])]
    dets = [_det([[0, 0, 20, 20]], [0.9])]
    r = rr.evaluate(dets, gt, 1, [0.5], [(0, 256), (-INF, INF)])
    assert r['tp_masks'].tolist() == [[1, 1]] and r['ign_masks'].tolist() == [[0, 0]]
    assert r['npos_area'].tolist() == [[1, 2]] and r['ap'][0, 0, 0] == 1.0
    # at t = 0.7 the in-range box is out of reach: the detection takes GT 0 and is ignored in [0, 256], a TP overall
    r = rr.evaluate(dets, gt, 1, [0.7], [(0, 256), (-INF, INF)])
    assert r['tp_masks'].tolist() == [[0, 1]] and r['ign_masks'].tolist() == [[1, 0]]
    assert r['ap'][0, 0, 0] == 0.0 and r['recall'][0, 0, 0] == 0.0 and r['ign'][0, 0, 0] == 1          # npos 1, nothing left: AP 0


def test_rule2_fall_through_consumes_the_out_of_range_box():
    # range [0, 100]: GT 0 10x10 (in), GT 1 12x12 = 144 (out).  d0 takes GT 0 (TP).  d1 = GT 0 again: its only in-range box
    # is matched, so it falls through to GT 1 (IoU 100 / 144 >= 0.5): ignored, GT 1 consumed.  d2 = GT 1 exactly: nothing
    # left to take, own area 144 out of range: ignored by rule 3.  In the unbounded range d1 takes GT 1 as a TP and d2 is an FP.
    gt = [_gt([[0, 0, 10, 10], [0, 0, 12, 12]])]
    dets = [_det([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 12, 12]], [0.9, 0.8, 0.7])]
    r = rr.evaluate(dets, gt, 1, [0.5], [(0, 100), (-INF, INF)])
    assert r['tp_masks'].tolist() == [[1, 1], [0, 1], [0, 0]] and r['ign_masks'].tolist() == [[0, 0], [1, 0], [1, 0]]
    assert r['fell'].tolist() == [1, 0] and r['outcomes'][0].tolist() == [0, 1, 1, 1]
    # consumption shows with an in-range detection after it: d2' (9x9 inside, IoU with GT 1 = 81 / 144 >= 0.5, with GT 0 0.81)
    dets = [_det([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 9, 9]], [0.9, 0.8, 0.7])]
    r = rr.evaluate(dets, gt, 1, [0.5], [(0, 100)])
    assert r['tp_masks'][:, 0].tolist() == [1, 0, 0] and r['ign_masks'][:, 0].tolist() == [0, 1, 0]       # both GT gone: d2' is an FP
    assert r['fp'][0, 0, 0] == 1 and r['tp'][0, 0, 0] == 1 and r['ign'][0, 0, 0] == 1
    # without d1 the out-of-range GT 1 is still free and d2' is ignored instead
    dets = [_det([[0, 0, 10, 10], [0, 0, 9, 9]], [0.9, 0.7])]
    r = rr.evaluate(dets, gt, 1, [0.5], [(0, 100)])
    assert r['ign_masks'][:, 0].tolist() == [0, 1] and r['fp'][0, 0, 0] == 0


def test_rule3_and_rule4_edges_are_closed():
    # no GT near: a 10x10 detection is exactly on hi of [0, 100] and on lo of [100, 400]: in range in both, an FP in both;
    # an 11x10 one is out of [0, 100] (ignored) and in [100, 400] (FP)
    gt = [_gt([[100, 100, 10, 10]])]
    dets = [_det([[0, 0, 10, 10], [30, 0, 11, 10]], [0.9, 0.8])]
    r = rr.evaluate(dets, gt, 1, [0.5], [(0, 100), (100, 400)])
    assert r['ign_masks'].tolist() == [[0, 0], [1, 0]] and not r['tp_masks'].any()
    assert r['fp'][:, 0, 0].tolist() == [1, 2] and r['ign'][:, 0, 0].tolist() == [1, 0]
    # the GT box on the shared edge counts in both ranges
    assert r['npos_area'].tolist() == [[1, 1]]


def test_all_ignored_with_gt_is_zero_and_no_gt_in_range_is_nan():
    gt = [_gt([[0, 0, 10, 10], [50, 50, 30, 30]], [0, 1])]
    dets = [_det([[100, 100, 30, 30], [50, 50, 30, 30]], [0.9, 0.8], [0, 1])]
    r = rr.evaluate(dets, gt, 2, [0.5], [(0, 100), (400, 1000)])
    # class 0 in [0, 100]: npos 1, its only detection (900) is area-ignored -> AP 0, recall 0, no operating point
    assert r['ap'][0, 0, 0] == 0.0 and r['recall'][0, 0, 0] == 0.0 and r['ign'][0, 0, 0] == 1 and r['fp'][0, 0, 0] == 0
    assert r['best_n'][0, 0, 0] == 0 and math.isnan(r['best_score'][0, 0, 0])
    assert np.all(r['pr_precision'][0, 0, 0] == 0) and np.all(np.isnan(r['pr_score'][0, 0, 0]))
    # class 1 in [0, 100] and class 0 in [400, 1000]: npos 0 -> NaN, best_n 0
    for a, c in ((0, 1), (1, 0)):
        assert r['npos_area'][c, a] == 0 and math.isnan(r['ap'][a, c, 0]) and math.isnan(r['recall'][a, c, 0])
        assert r['best_n'][a, c, 0] == 0 and math.isnan(r['best_score'][a, c, 0])
        assert np.all(np.isnan(r['pr_precision'][a, c, 0])) and np.all(np.isnan(r['pr_score'][a, c, 0]))
    assert r['fp'][1, 0, 0] == 1                                              # the 900 px class-0 stray is an FP in [400, 1000]
    assert r['ap'][1, 1, 0] == 1.0 and r['best_n'][1, 1, 0] == 1 and r['best_score'][1, 1, 0] == np.float32(0.8)


def _flags(scores, tp, npos):
    return rr.best_cut(np.asarray(scores, np.float32), np.asarray(tp, bool), npos)


def test_best_cut_cannot_split_an_equal_score_run():
    # TP TP | TP FP FP (one run of 0.5) with npos 3: cutting inside the run after its TP would give F1 = 6 / 6 = 1, but a
    # score threshold takes the whole run or none of it: k = 2 -> 4 / 5 = 0.8, k = 5 -> 6 / 8 = 0.75
    n, tp, sc = _flags([0.9, 0.8, 0.5, 0.5, 0.5], [1, 1, 1, 0, 0], 3)
    assert (n, tp, sc) == (2, 2, np.float32(0.8))
    # the same list with distinct scores does cut there
    assert _flags([0.9, 0.8, 0.5, 0.4, 0.3], [1, 1, 1, 0, 0], 3) == (3, 3, np.float32(0.5))


def test_best_cut_f1_tie_takes_the_smaller_k():
    # npos 2, TP FP TP: F1(1) = 2 / 3, F1(2) = 2 / 4, F1(3) = 4 / 5 -> k = 3
    assert _flags([0.9, 0.8, 0.7], [1, 0, 1], 2) == (3, 2, np.float32(0.7))
    # npos 3, TP FP FP TP TP: F1(1) = 2 / 4, F1(4) = 4 / 7, F1(5) = 6 / 8 -> k = 5
    assert _flags([0.9, 0.8, 0.7, 0.6, 0.5], [1, 0, 0, 1, 1], 3)[0] == 5
    # an exact tie: npos 2, TP FP FP TP: F1(1) = 2 / 3 = F1(4) = 4 / 6 (the same fp64 quotient) -> k = 1
    assert np.float64(2) / np.float64(3) == np.float64(4) / np.float64(6)
    assert _flags([0.9, 0.8, 0.7, 0.6], [1, 0, 0, 1], 2) == (1, 1, np.float32(0.9))
    # no TP at all: every F1 is 0, the first candidate wins; the leading equal-score pair is one candidate
    assert _flags([0.9, 0.9, 0.7], [0, 0, 0], 2) == (2, 0, np.float32(0.9))
    assert _flags([], [], 2)[0] == 0 and _flags([0.9], [1], 0)[0] == 0


def test_pr_curve_points():
    # npos 4, TP FP TP: envelope 1, 2/3, 2/3 (test_cpu_metrics' case): j <= 25 -> 1 at score 0.9, j <= 50 -> 2/3 at 0.7, then never
    prec, sc = rr.pr_curve(np.array([0.9, 0.8, 0.7], np.float32), np.array([1, 0, 1], bool), 4)
    assert np.all(prec[:26] == 1) and np.all(prec[26:51] == np.float32(2) / np.float32(3)) and np.all(prec[51:] == 0)
    assert np.all(sc[:26] == np.float32(0.9)) and np.all(sc[26:51] == np.float32(0.7)) and np.all(np.isnan(sc[51:]))
    ap, _ = ref.average_precision(np.array([1, 0, 1], bool), 4)
    assert abs(float(prec.astype(np.float64).mean()) - ap) < 1e-7
    # recall 0 is reached at the first entry even when that is an FP
    prec, sc = rr.pr_curve(np.array([0.9, 0.8], np.float32), np.array([0, 1], bool), 1)
    assert sc[0] == np.float32(0.9) and prec[0] == 0.5 and sc[1] == np.float32(0.8)


def test_entry_points_reject_bad_arguments_without_device():
    from yolo3 import _hip
    L = _hip.lib
    good = dict(rows=64, n=1, nb=4, ld=7, K=2, keep_idx=64, keep_cnt=64, keep_score=64, max_keep=4, max_det=4, gt=64, gt_cnt=64, max_gt=3,
                per_class=3, thr=_hip.float_array([0.5]), T=1, lo=_hip.float_array([0.0]), hi=_hip.float_array([1.0]), A=1, offsets=64,
                key=64, tp=64, ign=64, cap=16)

    def match(**kw):
        a = dict(good, **kw)
        return L.y3_eval_match_ranges(a['rows'], a['n'], a['nb'], a['ld'], a['K'], -1.0, -1.0, a['keep_idx'], a['keep_cnt'], a['keep_score'],
                                      a['max_keep'], a['max_det'], a['gt'], a['gt_cnt'], a['max_gt'], a['per_class'], a['thr'], a['T'],
                                      a['lo'], a['hi'], a['A'], a['offsets'], a['key'], a['tp'], a['ign'], a['cap'], None)
    for k in ('rows', 'gt', 'thr', 'lo', 'hi', 'tp', 'ign', 'key', 'offsets'):
        assert match(**{k: None}) == -1 and b'null' in L.y3_last_error(), k
    assert match(T=0) == -1 and b'thresholds' in L.y3_last_error()
    assert match(A=0) == -1 and b'area ranges' in L.y3_last_error()
    assert match(A=9, lo=_hip.float_array([0.0] * 9), hi=_hip.float_array([1.0] * 9)) == -1 and b'area ranges' in L.y3_last_error()
    assert match(lo=_hip.float_array([1.0])) == -1 and b'lo < hi' in L.y3_last_error()                     # lo == hi
    assert match(lo=_hip.float_array([2.0])) == -1
    assert match(lo=_hip.float_array([float('nan')])) == -1 and match(hi=_hip.float_array([float('nan')])) == -1
    assert match(A=2, lo=_hip.float_array([0.0, 5.0]), hi=_hip.float_array([1.0, 4.0])) == -1 and b'range 1' in L.y3_last_error()
    assert match(n=-1) == -1 and match(max_det=0) == -1 and match(ld=3) == -1 and match(cap=-1) == -1
    assert match(per_class=4097, max_gt=5000) == -1 and b'4096' in L.y3_last_error()
    assert match(thr=_hip.float_array([0.0])) == -1 and match(thr=_hip.float_array([float('nan')])) == -1

    ws = L.y3_eval_ap_ranges_workspace_bytes(100, 4, 10)
    assert ws == 100 * 4 * 10 * 2 * 4
    assert L.y3_eval_ap_ranges_workspace_bytes(-1, 4, 10) == 0 and L.y3_eval_ap_ranges_workspace_bytes(100, 0, 10) == 0
    o = 64

    def ap(keys=64, tp=64, ign=64, m=100, K=2, A=4, T=10, npos=64, w=64, wb=ws, outs=(o,) * 8):
        return L.y3_eval_ap_ranges(keys, tp, ign, m, K, A, T, npos, w, wb, *outs, None, None, None)
    assert ap(npos=None) == -1 and b'null' in L.y3_last_error()
    for i in range(8):
        assert ap(outs=tuple(None if j == i else o for j in range(8))) == -1 and b'null' in L.y3_last_error(), i
    assert ap(ign=None) == -1 and b'null' in L.y3_last_error()
    assert ap(w=None) == -1
    assert ap(wb=ws - 1) == -1 and b'workspace' in L.y3_last_error()
    assert ap(A=0) == -1 and b'area ranges' in L.y3_last_error()
    assert ap(A=9, wb=ws * 3) == -1 and b'area ranges' in L.y3_last_error()
    assert ap(T=0) == -1 and ap(T=33, wb=ws * 4) == -1 and ap(m=-1) == -1 and ap(K=0) == -1


def test_evaluator_arguments_are_checked_before_any_device_work():
    from yolo3 import metrics
    rng, names = metrics.check_area_ranges('coco')
    assert names == ['all', 'small', 'medium', 'large'] and rng.dtype == np.float32
    assert rng.tolist() == [[-INF, INF], [0.0, 1024.0], [1024.0, 9216.0], [9216.0, float(np.float32(1e10))]]
    assert metrics.check_area_ranges([(0, 5), (5, INF)])[1] == ['0:5', '5:inf']
    assert metrics.check_area_ranges([(0, 5)], ['tiny'])[1] == ['tiny']
    for bad in ('voc', [], [(0, 1)] * 9, [(1, 1)], [(2, 1)], [(float('nan'), 1)], [(0, float('nan'))], [1, 2, 3], [(0, 1, 2)]):
        with pytest.raises(ValueError):
            metrics.check_area_ranges(bad)
    with pytest.raises(ValueError):
        metrics.check_area_ranges([(0, 1)], ['a', 'b'])
    for kw in (dict(area_ranges=[(3, 2)]), dict(area_names=['x']), dict(area_names=['x'], curves=True), dict(area_ranges='coco', area_names=['x'])):
        with pytest.raises(ValueError):
            metrics.DetectionEvaluator(2, device='cpu', **kw)
    ev = metrics.DetectionEvaluator(2, device='cpu', curves=True)                # curves alone: the one range (-inf, inf), named 'all'
    assert ev.area_names == ['all'] and ev.area_ranges.tolist() == [[-INF, INF]] and ev.state()['tp'].shape == (0, 1)
    assert metrics.DetectionEvaluator(2, device='cpu').area_ranges is None


def test_summarize_ranges_picks_the_range_named_all_and_derives_the_operating_point():
    from yolo3 import metrics
    A, K, T = 2, 2, 1
    out = {'ap': np.array([[[0.25], [np.nan]], [[0.5], [1.0]]], np.float32), 'recall': np.array([[[0.5], [np.nan]], [[0.5], [1.0]]], np.float32),
           'tp': np.array([[[1], [0]], [[2], [1]]]), 'fp': np.array([[[1], [0]], [[2], [0]]]), 'ign': np.array([[[2], [1]], [[0], [0]]]),
           'best_n': np.array([[[1], [0]], [[3], [1]]]), 'best_tp': np.array([[[1], [0]], [[2], [1]]]),
           'best_score': np.array([[[0.9], [np.nan]], [[0.4], [0.7]]], np.float32),
           'pr_precision': np.zeros((A, K, T, 101), np.float32), 'pr_score': np.zeros((A, K, T, 101), np.float32)}
    npos = np.array([[2, 4], [0, 1]])
    r = metrics.summarize_ranges(out, npos, [0.5], np.array([[0, 9], [-INF, INF]], np.float32), ['small', 'all'], True)
    assert r['npos'].tolist() == [4, 1] and r['ap'].tolist() == [[0.5], [1.0]] and r['map50'] == 0.75 and r['tp50'].tolist() == [2, 1]
    assert r['map_area'].tolist() == [[0.25], [0.75]] and r['map50_area'].tolist() == [0.25, 0.75] and r['ar_area'].tolist() == [0.5, 0.75]
    assert np.all(np.isnan(r['map50_95_area']))
    assert r['best_fp'].tolist() == [[[0], [0]], [[1], [0]]]
    assert r['best_precision'][0, 0, 0] == 1.0 and math.isnan(r['best_precision'][0, 1, 0]) and r['best_precision'][1, 0, 0] == 2 / 3
    assert r['best_recall'][0, 0, 0] == 0.5 and math.isnan(r['best_recall'][0, 1, 0]) and r['best_recall'][1, 0, 0] == 0.5
    assert r['best_f1'][0, 0, 0] == 2 / 3 and math.isnan(r['best_f1'][0, 1, 0]) and r['best_f1'][1, 0, 0] == 4 / 7
    r = metrics.summarize_ranges(out, npos, [0.5], np.array([[0, 9], [9, 99]], np.float32), ['a', 'b'], False)
    assert r['npos'].tolist() == [2, 0] and 'best_f1' not in r and 'pr_score' not in r
