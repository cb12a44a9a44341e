"""NumPy restatement of the metric by area range, the best-F1 operating point and the PR curve, written from
the definition there, plus the random detection sets the CPU and GPU tests share.

- area of a box = fp32 (x1 - x0) * (y1 - y0); in range iff lo <= area <= hi (both ends closed);
- per (image, class, range, t), in keep order, over the unmatched same-class GT boxes with IoU >= t: an in-range one of
  largest IoU (ties: highest GT index) -> TP; else an out-of-range one of largest IoU (same tie rule), consumed -> ignored;
  else ignored if the detection's own area is out of range; else FP;
- per (class, range, t): ignored entries dropped, the rest ranked by score descending (ties: image, keep rank); AP as
  eval_reference.average_precision; best cut = the candidate cut (k = n, or score(d_{k+1}) < score(d_k)) of largest fp64
  F1 = 2 TP(k) / (k + npos), ties: smallest k; curve = fp32 envelope precision and first-reached score at recall j / 100.
"""
import numpy as np

from eval_reference import average_precision, gt_to_corners, iou_f32, keep_order

INF = float('inf')
TEST_RANGES = [(-INF, INF), (0.0, 256.0), (256.0, 900.0), (900.0, 1e10)]     # the generator's boxes have sides 4..40
FP, TP, IGN_GT, IGN_AREA = 0, 1, 2, 3


def area_f32(boxes):
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def in_range(area, lo, hi):
    return (np.float32(lo) <= area) & (area <= np.float32(hi))


def match_ranges(det_boxes, gt_boxes, thr, lo, hi):
    """det_boxes [M,4] in keep order, gt_boxes [G,4] (one class, GT order) -> (outcome [M] of FP / TP / IGN_GT / IGN_AREA,
    fell [M]: rule 2 fired although an in-range GT box with IoU >= thr existed, already matched)."""
    m, g = len(det_boxes), len(gt_boxes)
    gin = in_range(area_f32(gt_boxes), lo, hi) if g else np.zeros(0, bool)
    din = in_range(area_f32(det_boxes), lo, hi) if m else np.zeros(0, bool)
    matched = np.zeros(g, bool)
    out = np.zeros(m, np.int64)
    fell = np.zeros(m, bool)
    for j in range(m):
        iou = iou_f32(det_boxes[j], gt_boxes) if g else np.zeros(0, np.float32)
        reach = iou >= np.float32(thr)
        ok = ~matched & reach
        for tier, code in ((ok & gin, TP), (ok & ~gin, IGN_GT)):
            if tier.any():
                pick = int(np.nonzero(tier & (iou == iou[tier].max()))[0].max())
                matched[pick] = True
                out[j] = code
                fell[j] = code == IGN_GT and bool((reach & gin).any())
                break
        else:
            out[j] = FP if din[j] else IGN_AREA
    return out, fell


def best_cut(scores, tp, npos):
    """scores / tp of the non-ignored ranked list -> (best_n, best_tp, best_score)."""
    n = len(scores)
    if n == 0 or npos == 0:
        return 0, 0, np.float32('nan')
    tp_cum = np.cumsum(np.asarray(tp, np.int64))
    best = None
    for k in range(1, n + 1):
        if k < n and not scores[k] < scores[k - 1]:
            continue
        f1 = np.float64(2 * tp_cum[k - 1]) / np.float64(k + npos)
        if best is None or f1 > best[0]:
            best = (f1, k)
    k = best[1]
    return k, int(tp_cum[k - 1]), np.float32(scores[k - 1])


def pr_curve(scores, tp, npos):
    """-> (precision float32 [101], score float32 [101])."""
    prec = np.full(101, np.nan, np.float32)
    sc = np.full(101, np.nan, np.float32)
    if npos == 0:
        return prec, sc
    prec[:] = 0
    n = len(scores)
    if n == 0:
        return prec, sc
    tp_cum = np.cumsum(np.asarray(tp, np.int64))
    p32 = tp_cum.astype(np.float32) / np.arange(1, n + 1).astype(np.float32)
    env = np.maximum.accumulate(p32[::-1])[::-1]
    for j in range(101):
        hit = np.nonzero(100 * tp_cum >= j * npos)[0]
        if hit.size:
            prec[j] = env[hit[0]]
            sc[j] = scores[hit[0]]
    return prec, sc


def evaluate(dets, gts, num_classes, thresholds, ranges, max_det=None):
    """dets / gts as eval_reference.evaluate; ranges: (lo, hi) pairs.  Returns dict (A ranges, K classes, T thresholds):
    tp_masks, ign_masks uint32 [M,A] in (image, class, keep rank) order, classes, scores [M], npos_area [K,A], ap, recall
    [A,K,T], tp, fp, ign, best_n, best_tp [A,K,T] ints, best_score float32 [A,K,T], pr_precision, pr_score float32 [A,K,T,101],
    outcomes [A,4] (entries x thresholds per outcome code), fell [A]."""
    K, T, A = num_classes, len(thresholds), len(ranges)
    npos = np.zeros((K, A), np.int64)
    pooled = [[] for _ in range(K)]                # (score, image, rank, tp masks [A], ign masks [A])
    tpm, igm, classes, scores_out = [], [], [], []
    outcomes = np.zeros((A, 4), np.int64)
    fell_n = np.zeros(A, np.int64)
    for i, (det, gt) in enumerate(zip(dets, gts)):
        gbox, gcls = gt_to_corners(gt)
        ga = area_f32(gbox)
        for a, (lo, hi) in enumerate(ranges):
            npos[:, a] += np.bincount(gcls[in_range(ga, lo, hi)], minlength=K)[:K]
        if det[0] is None:
            continue
        boxes = np.asarray(det[0], np.float32).reshape(-1, 4)
        sc = np.asarray(det[1], np.float32).reshape(-1)
        lab = np.asarray(det[2]).astype(np.int64).reshape(-1)
        rid = np.arange(len(sc)) if len(det) < 4 or det[3] is None else np.asarray(det[3], np.int64)
        for c in range(K):
            sel = np.nonzero(lab == c)[0]
            order = sel[keep_order(sc[sel], rid[sel])] if sel.size else sel
            if max_det is not None:
                order = order[:max_det]
            mt = np.zeros((len(order), A), np.uint32)
            mi = np.zeros((len(order), A), np.uint32)
            for a, (lo, hi) in enumerate(ranges):
                for t, thr in enumerate(thresholds):
                    out, fell = match_ranges(boxes[order], gbox[gcls == c], thr, lo, hi)
                    mt[:, a] |= (out == TP).astype(np.uint32) << np.uint32(t)
                    mi[:, a] |= ((out == IGN_GT) | (out == IGN_AREA)).astype(np.uint32) << np.uint32(t)
                    outcomes[a] += np.bincount(out, minlength=4)
                    fell_n[a] += int(fell.sum())
            for r, o in enumerate(order):
                pooled[c].append((float(sc[o]), i, r, mt[r], mi[r]))
                tpm.append(mt[r])
                igm.append(mi[r])
                classes.append(c)
                scores_out.append(sc[o])
    shape = (A, K, T)
    res = {'ap': np.zeros(shape), 'recall': np.zeros(shape), 'tp': np.zeros(shape, np.int64), 'fp': np.zeros(shape, np.int64),
           'ign': np.zeros(shape, np.int64), 'best_n': np.zeros(shape, np.int64), 'best_tp': np.zeros(shape, np.int64),
           'best_score': np.zeros(shape, np.float32), 'pr_precision': np.zeros(shape + (101,), np.float32),
           'pr_score': np.zeros(shape + (101,), np.float32)}
    for c in range(K):
        entries = sorted(pooled[c], key=lambda e: (-e[0], e[1], e[2]))
        for a in range(A):
            for t in range(T):
                kept = [e for e in entries if not (int(e[4][a]) >> t) & 1]
                flags = np.array([(int(e[3][a]) >> t) & 1 for e in kept], bool)
                scs = np.array([e[0] for e in kept], np.float32)
                n_c = int(npos[c, a])
                res['ap'][a, c, t], res['recall'][a, c, t] = average_precision(flags, n_c)
                res['tp'][a, c, t] = int(flags.sum())
                res['fp'][a, c, t] = len(kept) - int(flags.sum())
                res['ign'][a, c, t] = len(entries) - len(kept)
                res['best_n'][a, c, t], res['best_tp'][a, c, t], res['best_score'][a, c, t] = best_cut(scs, flags, n_c)
                res['pr_precision'][a, c, t], res['pr_score'][a, c, t] = pr_curve(scs, flags, n_c)
    res.update(npos_area=npos, tp_masks=np.asarray(tpm, np.uint32).reshape(-1, A), ign_masks=np.asarray(igm, np.uint32).reshape(-1, A),
               classes=np.asarray(classes, np.int32), scores=np.asarray(scores_out, np.float32), outcomes=outcomes, fell=fell_n)
    return res


# ---- the random sets of tests/test_gpu_metrics.py (its generator, copied) ----------------------------------------------
def xywh_to_corners(b):
    b = np.asarray(b, np.float64).reshape(-1, 4)
    return np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32)


def random_set(rng, n, K, max_gt=12, max_extra=10, dup=True):
    """Integer boxes (IoU ties), scores from a few levels (score ties), duplicated GT boxes, detections jittered from GT
    plus strays, some images without GT and some without detections."""
    dets, gts = [], []
    for i in range(n):
        g = int(rng.integers(0, max_gt + 1)) if rng.random() > 0.15 else 0
        wh = rng.integers(4, 40, (g, 2))
        xy = rng.integers(0, 200, (g, 2))
        gt = np.concatenate([xy, wh, rng.integers(0, K, (g, 1))], 1)
        if dup and g > 1 and rng.random() < 0.5:
            gt = np.concatenate([gt, gt[rng.integers(0, g, int(rng.integers(1, 4)))]])
        gts.append(gt.astype(np.int64))
        if rng.random() < 0.15:
            dets.append((None, None, None, None))
            continue
        src = gt[rng.integers(0, len(gt), int(rng.integers(0, 2 * len(gt) + 1)))] if len(gt) else np.zeros((0, 5), np.int64)
        jit = src[:, :4] + rng.integers(-4, 5, (len(src), 4))
        jit[:, 2:] = np.maximum(jit[:, 2:], 1)
        e = int(rng.integers(0, max_extra + 1))
        stray = np.concatenate([rng.integers(0, 200, (e, 2)), rng.integers(2, 40, (e, 2))], 1)
        boxes = np.concatenate([jit, stray]).astype(np.float32)
        labels = np.concatenate([src[:, 4], rng.integers(0, K, e)]).astype(np.int32)
        if rng.random() < 0.3 and len(labels):
            labels = np.where(rng.random(len(labels)) < 0.2, rng.integers(0, K, len(labels)), labels).astype(np.int32)
        scores = rng.choice(np.array([0.2, 0.35, 0.5, 0.8, 0.95], np.float32), len(boxes))
        if len(boxes) == 0:
            dets.append((np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), None))
        else:
            dets.append((xywh_to_corners(boxes), scores, labels, None))
    return dets, gts


def mutate_for_fall_through(rng, dets, gts):
    """The plain generator never lets a detection fall through to an out-of-range box (rule 2 after the in-range box is
    taken): its GT boxes seldom overlap unless identical.  Per image with detections, up to three GT boxes get a same-class
    copy grown by 1..6 px per side (so some pairs straddle an area edge) and two extra detections on the original box."""
    dets, gts = list(dets), list(gts)
    for i, (det, gt) in enumerate(zip(dets, gts)):
        if det[0] is None or len(gt) == 0:
            continue
        pick = gt[rng.integers(0, len(gt), int(rng.integers(1, 4)))]
        grown = pick.copy()
        grown[:, 2:4] += rng.integers(1, 7, (len(pick), 2))
        gts[i] = np.concatenate([gt, grown])
        extra = np.repeat(pick, 2, axis=0)
        dets[i] = (np.concatenate([det[0], xywh_to_corners(extra[:, :4])]),
                   np.concatenate([det[1], rng.choice(np.array([0.5, 0.8], np.float32), len(extra))]),
                   np.concatenate([det[2], extra[:, 4].astype(np.int32)]), None)
    return dets, gts


def seeded_set(seed, n=None, K=None, mutate=True, **kw):
    """Set number ``seed`` of the sets the tests share: (dets, gts, K); n images and K classes drawn from the seed unless
    given, kw to random_set."""
    rng = np.random.default_rng(5000 + seed)
    K = int(rng.integers(1, 4)) if K is None else K
    dets, gts = random_set(rng, int(rng.integers(1, 12)) if n is None else n, K, **kw)
    if mutate:
        dets, gts = mutate_for_fall_through(rng, dets, gts)
    return dets, gts, K
