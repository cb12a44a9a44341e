"""Plain-loop NumPy float32 restatement of the per-class score cut and the confusion matrix, written from the
definition there, plus the detection sets the CPU and GPU tests share.

Score cut: a keep list (one (image, class), keep order) of stored count c, with m = min(max(c, 0), max_keep), keeps the longest
prefix j < m with score[j] >= thr[class] (fp32).

Confusion matrix, K classes, index K = background:
- the detections of an image are, per class, the first max_det entries in keep order (score descending, ties: higher row index);
- they are pooled in one order: score descending (fp32), ties: lower class first, then keep rank;
- per IoU threshold t, in that order, a detection takes the still-unmatched GT box of ANY class with the largest fp32 IoU
  (inter / ((a + b) - inter)), equal IoU: the highest GT index, if that IoU >= t;
- M[t, g, p] += 1 for a detection of class p on a GT box of class g, M[t, K, p] += 1 for an unmatched detection,
  M[t, g, K] += 1 for a GT box left unmatched; M[t, K, K] = 0.
"""
import numpy as np

from eval_reference import gt_to_corners, iou_f32, keep_order


def cut_counts(keep_cnt, keep_score, thr, max_keep=None):
    """keep_cnt int [S] (S = images * K segments, class = s % K), keep_score float32 [S, width], thr float32 [K] -> int32 [S]."""
    cnt = np.asarray(keep_cnt).reshape(-1)
    sc = np.asarray(keep_score, np.float32).reshape(cnt.size, -1)
    thr = np.asarray(thr, np.float32).reshape(-1)
    max_keep = sc.shape[1] if max_keep is None else max_keep
    out = np.zeros(cnt.size, np.int32)
    for s in range(cnt.size):
        m = min(max(int(cnt[s]), 0), max_keep)
        j = 0
        while j < m and sc[s, j] >= thr[s % thr.size]:
            j += 1
        out[s] = j
    return out


def filter_dets(dets, thr):
    """The detections with float32 score >= thr[label], per image, in their order; an image left empty -> (None,)*4."""
    thr = np.asarray(thr, np.float32)
    out = []
    for det in dets:
        if det[0] is None:
            out.append((None, None, None, None))
            continue
        keep = [i for i in range(len(det[1])) if np.float32(det[1][i]) >= thr[int(det[2][i])]]
        if not keep:
            out.append((None, None, None, None))
            continue
        out.append(tuple(None if v is None else np.asarray(v)[keep] for v in det))
    return out


def pooled_order(det, num_classes, max_det=None):
    """One image's detections (boxes, scores, labels, row_index or None) -> positions in pooled order, and whether two entries
    of different classes tie in score."""
    sc = np.asarray(det[1], np.float32).reshape(-1)
    lab = np.asarray(det[2]).astype(np.int64).reshape(-1)
    rid = np.arange(len(sc)) if len(det) < 4 or det[3] is None else np.asarray(det[3], np.int64)
    entries = []                                    # (score, class, keep rank, position)
    for c in range(num_classes):
        sel = np.nonzero(lab == c)[0]
        order = sel[keep_order(sc[sel], rid[sel])] if sel.size else sel
        if max_det is not None:
            order = order[:max_det]
        for r, o in enumerate(order):
            entries.append((float(sc[o]), c, r, int(o)))
    entries.sort(key=lambda e: (-e[0], e[1], e[2]))
    tie = any(a[0] == b[0] and a[1] != b[1] for a, b in zip(entries, entries[1:]))
    return [e[3] for e in entries], tie


def match_image(boxes, labels, order, gbox, gcls, thr, K, M):
    """Adds one image's counts at one threshold to M [K+1, K+1]; returns the GT index each pooled detection took (-1: none)."""
    matched = np.zeros(len(gbox), bool)
    took = []
    for o in order:
        p = int(labels[o])
        pick = -1
        if len(gbox):
            iou = iou_f32(boxes[o], gbox)
            ok = ~matched & (iou >= np.float32(thr))
            if ok.any():
                best = iou[ok].max()
                pick = int(np.nonzero(ok & (iou == best))[0].max())
        if pick >= 0:
            matched[pick] = True
            M[int(gcls[pick]), p] += 1
        else:
            M[K, p] += 1
        took.append(pick)
    for g in np.nonzero(~matched)[0]:
        M[int(gcls[g]), K] += 1
    return took


def confusion(dets, gts, num_classes, thresholds, max_det=None):
    """dets / gts as eval_reference.evaluate.  Returns dict: confusion int64 [T, K+1, K+1], npos [K], entries [K] (detections that
    entered, per class), score_ties (images with a cross-class score tie in the pooled order), steals [T] (detections left on
    background although a same-class GT box with IoU >= t exists that a detection of another class took)."""
    K, T = num_classes, len(thresholds)
    M = np.zeros((T, K + 1, K + 1), np.int64)
    npos = np.zeros(K, np.int64)
    entries = np.zeros(K, np.int64)
    ties = 0
    steals = np.zeros(T, np.int64)
    for det, gt in zip(dets, gts):
        gbox, gcls = gt_to_corners(gt)
        npos += np.bincount(gcls, minlength=K)[:K]
        if det[0] is None:
            boxes, labels, order = np.zeros((0, 4), np.float32), np.zeros(0, np.int64), []
        else:
            boxes = np.asarray(det[0], np.float32).reshape(-1, 4)
            labels = np.asarray(det[2]).astype(np.int64).reshape(-1)
            order, tie = pooled_order(det, K, max_det)
            ties += int(tie)
            entries += np.bincount(labels[order], minlength=K)[:K] if len(order) else 0
        for t, thr in enumerate(thresholds):
            took = match_image(boxes, labels, order, gbox, gcls, thr, K, M[t])
            for o, pick in zip(order, took):
                if pick >= 0 or not len(gbox):
                    continue
                iou = iou_f32(boxes[o], gbox)
                mine = np.nonzero((gcls == labels[o]) & (iou >= np.float32(thr)))[0]
                # a same-class box in reach, taken by a detection of ANOTHER class
                if any(labels[order[took.index(g)]] != labels[o] for g in mine if g in took):
                    steals[t] += 1
    return {'confusion': M, 'npos': npos, 'entries': entries, 'score_ties': ties, 'steals': steals}


# ---- the sets the tests share ------------------------------------------------------------------------------------------------
def random_image(rng, K, n_det, n_gt, size=64):
    """One image: boxes on a quarter-pixel grid, duplicated boxes, scores from a few levels shared by all classes (score ties
    across classes), detections mostly copied or nudged from GT boxes of any class (IoU ties, off-diagonal matches)."""
    q = np.float32(0.25)
    xy = rng.integers(0, size * 4, (n_gt, 2)) * q
    wh = rng.integers(8, 96, (n_gt, 2)) * q
    gt = np.concatenate([xy, wh, rng.integers(0, K, (n_gt, 1))], 1).astype(np.float64)
    if n_gt > 1:                                                   # duplicated GT boxes, some of another class
        d = rng.integers(0, n_gt, max(1, n_gt // 8))
        gt[d] = gt[rng.integers(0, n_gt, len(d))]
        gt[d, 4] = rng.integers(0, K, len(d))
    if n_det == 0:
        return (None, None, None, None), gt
    boxes = np.zeros((n_det, 4), np.float32)
    labels = rng.integers(0, K, n_det).astype(np.int32)
    for i in range(n_det):
        u = rng.random()
        if n_gt and u < 0.8:
            g = gt[rng.integers(0, n_gt)]
            nudge = rng.integers(-3, 4, 4) * q if u > 0.4 else np.zeros(4, np.float32)
            boxes[i] = np.array([g[0], g[1], g[0] + g[2], g[1] + g[3]], np.float32) + nudge.astype(np.float32)
            if rng.random() < 0.7:
                labels[i] = int(g[4])
        else:
            x, y = rng.integers(0, size * 4, 2) * q
            boxes[i] = [x, y, x + rng.integers(8, 96) * q, y + rng.integers(8, 96) * q]
    boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2] + q)
    if n_det > 2:
        d = rng.integers(0, n_det, max(1, n_det // 6))             # duplicated detections, same box and score, maybe another class
        boxes[d] = boxes[rng.integers(0, n_det, len(d))]
    scores = rng.choice(np.array([0.15, 0.3, 0.45, 0.6, 0.75, 0.9], np.float32), n_det)
    return (boxes, scores, labels, None), gt


DET_COUNTS = (0, 1, 64, 65, 130)
GT_COUNTS = (0, 1, 64, 65, 300)


def seeded_set(seed, n, K):
    """Set number ``seed``: n images with detection / GT counts cycling through DET_COUNTS x GT_COUNTS (offset by the seed), plus the
    constructed pair of IoU exactly 0.5 ([0,0,2,1] against [0,0,1,1]) appended to the first image that has detections."""
    rng = np.random.default_rng(7000 + seed)
    dets, gts = [], []
    for i in range(n):
        k = seed * 7 + i * 3
        det, gt = random_image(rng, K, DET_COUNTS[k % 5], GT_COUNTS[(k // 5 + i) % 5])
        dets.append(det)
        gts.append(gt)
    for i, det in enumerate(dets):
        if det[0] is not None:
            far = np.float32(1000)
            dets[i] = (np.concatenate([det[0], np.array([[far, far, far + 2, far + 1]], np.float32)]),
                       np.concatenate([det[1], np.array([0.5], np.float32)]), np.concatenate([det[2], np.array([0], np.int32)]), None)
            gts[i] = np.concatenate([gts[i], np.array([[1000, 1000, 1, 1, K - 1]], np.float64)])
            break
    return dets, gts


WORKED_GT = np.array([[0, 0, 10, 10, 0], [20, 0, 10, 10, 1]], np.float64)
WORKED_DET = (np.array([[0, 0, 10, 10], [0, 0, 10, 10], [20, 0, 30, 8], [50, 50, 60, 60]], np.float32),
              np.array([0.9, 0.8, 0.7, 0.6], np.float32), np.array([1, 0, 1, 0], np.int32), None)
