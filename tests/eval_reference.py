"""NumPy reference of the detection metric, written from the metric's definition:

- GT X,Y,W,H,C -> corners (X, Y, X+W, Y+H); detections per (image, class) in keep order (score descending, ties: higher
  row index), cut to max_det;
- IoU fp32, no +1: inter = max(yb-yt,0) * max(xr-xl,0), iou = inter / ((area_det + area_gt) - inter);
- per (image, class, t): each detection in turn takes the unmatched same-class GT box of largest IoU (ties: highest GT
  index) if IoU >= t;
- per (class, t): pool over images, sort by score descending, ties (image order, keep rank); precision = tp_cum /
  (rank+1), envelope = suffix max, AP = mean over j = 0..100 of envelope[first index with 100 tp_cum >= j npos] (0 if
  none); npos = 0 -> NaN; no detections -> 0.
"""
import numpy as np

COCO = [float(np.float32(0.5) + np.float32(0.05) * np.float32(k)) for k in range(10)]


def gt_to_corners(gt_xywhc):
    g = np.asarray(gt_xywhc, np.float64).reshape(-1, 5)
    return np.stack([g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]], 1).astype(np.float32), g[:, 4].astype(np.int64)


def iou_f32(det, gts):
    """det [4], gts [G,4] -> float32 [G]."""
    d = np.asarray(det, np.float32)
    g = np.asarray(gts, np.float32).reshape(-1, 4)
    a_det = (d[2] - d[0]) * (d[3] - d[1])
    a_gt = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    xl = np.maximum(d[0], g[:, 0])
    yt = np.maximum(d[1], g[:, 1])
    xr = np.minimum(d[2], g[:, 2])
    yb = np.minimum(d[3], g[:, 3])
    inter = np.maximum(yb - yt, np.float32(0)) * np.maximum(xr - xl, np.float32(0))
    with np.errstate(divide='ignore', invalid='ignore'):
        return (inter / ((a_det + a_gt) - inter)).astype(np.float32)


def keep_order(scores, row_index):
    """positions sorted by score descending, ties: higher row index first."""
    scores = np.asarray(scores, np.float32)
    row_index = np.asarray(row_index, np.int64)
    return np.array(sorted(range(len(scores)), key=lambda i: (-float(scores[i]), -int(row_index[i]))), np.int64)


def greedy_match(det_boxes, gt_boxes, thr):
    """det_boxes [M,4] in keep order, gt_boxes [G,4] (one class, GT order) -> TP flags [M]."""
    m, g = len(det_boxes), len(gt_boxes)
    matched = np.zeros(g, bool)
    tp = np.zeros(m, bool)
    for j in range(m):
        if g == 0:
            break
        iou = iou_f32(det_boxes[j], gt_boxes)
        ok = ~matched & (iou >= np.float32(thr))
        if not ok.any():
            continue
        best = iou[ok].max()
        pick = int(np.nonzero(ok & (iou == best))[0].max())
        matched[pick] = True
        tp[j] = True
    return tp


def average_precision(tp_sorted, npos):
    """tp_sorted: TP flags of one class in final rank order -> (AP, final recall)."""
    if npos == 0:
        return float('nan'), float('nan')
    n = len(tp_sorted)
    if n == 0:
        return 0.0, 0.0
    tp_cum = np.cumsum(tp_sorted.astype(np.int64))
    precision = tp_cum / np.arange(1, n + 1, dtype=np.float64)
    envelope = np.maximum.accumulate(precision[::-1])[::-1]
    terms = []
    for j in range(101):
        hit = np.nonzero(100 * tp_cum >= j * npos)[0]
        terms.append(envelope[hit[0]] if hit.size else 0.0)
    return float(np.mean(terms)), float(tp_cum[-1]) / npos


def evaluate(dets, gts, num_classes, thresholds=COCO, max_det=None):
    """dets: per image (boxes [M,4] corners, scores [M], labels [M], row_index [M] or None = array position), or a tuple
    whose boxes is None for no detections; gts: per image [G,5] X,Y,W,H,C.
    Returns dict: ap, recall [K,T], tp, fp [K,T] ints, npos [K], masks (uint32 TP mask of every kept detection in
    (image, class, keep rank) order), classes, scores (same order)."""
    K, T = num_classes, len(thresholds)
    npos = np.zeros(K, np.int64)
    pooled = [[] for _ in range(K)]                # (score, image, rank, mask)
    masks, classes, scores_out = [], [], []
    for i, (det, gt) in enumerate(zip(dets, gts)):
        gbox, gcls = gt_to_corners(gt)
        npos += np.bincount(gcls, minlength=K)[:K]
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
            mask = np.zeros(len(order), np.uint32)
            for t, thr in enumerate(thresholds):
                tp = greedy_match(boxes[order], gbox[gcls == c], thr)
                mask |= tp.astype(np.uint32) << np.uint32(t)
            for r, (o, mk) in enumerate(zip(order, mask)):
                pooled[c].append((float(sc[o]), i, r, int(mk)))
                masks.append(int(mk))
                classes.append(c)
                scores_out.append(sc[o])
    ap = np.zeros((K, T))
    rec = np.zeros((K, T))
    tpn = np.zeros((K, T), np.int64)
    fpn = np.zeros((K, T), np.int64)
    for c in range(K):
        entries = sorted(pooled[c], key=lambda e: (-e[0], e[1], e[2]))
        for t in range(T):
            flags = np.array([(e[3] >> t) & 1 for e in entries], bool)
            ap[c, t], rec[c, t] = average_precision(flags, int(npos[c]))
            tpn[c, t] = int(flags.sum())
            fpn[c, t] = len(flags) - int(flags.sum())
    return {'ap': ap, 'recall': rec, 'tp': tpn, 'fp': fpn, 'npos': npos, 'masks': np.asarray(masks, np.uint32),
            'classes': np.asarray(classes, np.int32), 'scores': np.asarray(scores_out, np.float32)}
