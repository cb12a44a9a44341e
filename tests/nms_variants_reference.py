"""NumPy restatements of the opt-in NMS variants of y3_nms_per_class_ex (include/yolo3hip.h).

diou and soft-linear are float32 in the kernels' operation order (the library builds with -ffp-contract=off), so the
GPU must reproduce them bit for bit; soft-gaussian is float64 (the device expf is not NumPy's exp to the last ulp).
Candidate selection and the IoU are oracle.nms's (filter_small_boxes_mask, compute_iou), the clip is y3_nms_per_class's.
Every function returns, per class, (rows int32 [M], scores [M]) in emission order.
"""
import numpy as np

from oracle import nms as onms

F = np.float32
METHODS = ('hard', 'diou', 'soft-linear', 'soft-gaussian')


def candidates(rows, cls, min_box, score_thr, clip_wh=None):
    """Candidates of class ``cls`` of one image's rows [Nb, 5+K]: (row indices, clipped boxes [M,4] f32, scores [M] f32)."""
    rows = np.asarray(rows, np.float32)
    b = rows[:, 0:4].copy()
    if clip_wh is not None:
        b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], F(0)), F(clip_wh[0]))
        b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], F(0)), F(clip_wh[1]))
    score = np.sqrt(rows[:, 5 + cls] * rows[:, 4])
    mask = onms.filter_small_boxes_mask(b, F(min_box)) & (score >= F(score_thr))
    idx = np.nonzero(mask)[0]
    return idx.astype(np.int64), b[idx], score[idx]


def order_keys(scores, idx):
    """(score bits << 32) | row of positive float32 scores: larger = earlier."""
    return (np.asarray(scores, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def _areas(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def diou_value(k, ka, b, a):
    """iou - rho2 / c2 of kept box k (area ka) against boxes b (areas a), float32, the kernel's operation order."""
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = onms.compute_iou(k, b, ka, a)
        h = F(0.5)
        dx = (b[:, 0] + b[:, 2]) * h - (k[0] + k[2]) * h
        dy = (b[:, 1] + b[:, 3]) * h - (k[1] + k[3]) * h
        rho2 = dx * dx + dy * dy
        ex = np.maximum(k[2], b[:, 2]) - np.minimum(k[0], b[:, 0])
        ey = np.maximum(k[3], b[:, 3]) - np.minimum(k[1], b[:, 1])
        c2 = ex * ex + ey * ey
        return iou - rho2 / c2


def greedy(idx, boxes, scores, iou_thr, criterion='hard'):
    """Greedy NMS in key order; candidate j survives kept k iff value(k, j) <= iou_thr (NaN drops)."""
    order = np.argsort(order_keys(scores, idx), kind='stable')[::-1]
    b, s, r = boxes[order], scores[order], idx[order]
    area = _areas(b)
    thr = F(iou_thr)
    rem = np.arange(len(order))
    keep = []
    while rem.size:
        i = rem[0]
        keep.append(i)
        rem = rem[1:]
        if not rem.size:
            break
        if criterion == 'diou':
            v = diou_value(b[i], area[i], b[rem], area[rem])
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                v = onms.compute_iou(b[i], b[rem], area[i], area[rem])
        rem = rem[v <= thr]
    keep = np.asarray(keep, np.int64)
    return r[keep].astype(np.int32), s[keep]


def soft(idx, boxes, scores, iou_thr, score_thr, method, sigma=0.5, max_keep=None):
    """Soft-NMS: pick the live candidate with the largest key, emit (row, current score), decay the others by their IoU
    with the pick, drop NaN IoU or score < score_thr.  soft-linear: float32, bit for bit; soft-gaussian: float64."""
    gauss = method == 'soft-gaussian'
    dt = np.float64 if gauss else np.float32
    s = np.asarray(scores, dt).copy()
    b32 = np.asarray(boxes, np.float32)
    b = b32.astype(dt)
    area = _areas(b)
    live = np.ones(len(idx), bool)
    out_r, out_s = [], []
    thr = dt(score_thr)
    while live.any() and (max_keep is None or len(out_r) < max_keep):
        cand = np.nonzero(live)[0]
        if gauss:
            j = cand[np.lexsort((idx[cand], s[cand]))[-1]]
        else:
            j = cand[np.argmax(order_keys(s[cand], idx[cand]))]
        out_r.append(int(idx[j]))
        out_s.append(s[j])
        live[j] = False
        o = np.nonzero(live)[0]
        if not o.size:
            break
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            iou = onms.compute_iou(b[j], b[o], area[j], area[o])
            if gauss:
                t = s[o] * np.exp(-(iou * iou) / np.float64(sigma))
            else:
                t = np.where(iou > F(iou_thr), s[o] * (F(1) - iou), s[o]).astype(np.float32)
        s[o] = t
        live[o[np.isnan(iou) | ~(t >= thr)]] = False
    return np.asarray(out_r, np.int32), np.asarray(out_s, dt)


def per_class(rows, method, min_box, score_thr=0.1, iou_thr=0.3, sigma=0.5, clip_wh=None, max_keep=None):
    """One image's rows [Nb, 5+K] -> per class (rows int32, scores) in emission order, truncated to max_keep."""
    rows = np.asarray(rows, np.float32)
    out = []
    for c in range(rows.shape[1] - 5):
        idx, b, s = candidates(rows, c, min_box, score_thr, clip_wh)
        if method in ('hard', 'diou'):
            r, sc = greedy(idx, b, s, iou_thr, method)
            if max_keep is not None:
                r, sc = r[:max_keep], sc[:max_keep]
        else:
            r, sc = soft(idx, b, s, iou_thr, score_thr, method, sigma, max_keep)
        out.append((r, sc))
    return out


def soft_gaussian_margins(rows, min_box, score_thr, iou_thr, sigma, clip_wh=None):
    """Smallest relative gap, over every emission of every class, between the picked score and the runner-up and between
    any live decayed score and score_thr (float64): how far the inputs are from a float32 rounding deciding the outcome."""
    rows = np.asarray(rows, np.float32)
    worst = np.inf
    for c in range(rows.shape[1] - 5):
        idx, b32, s32 = candidates(rows, c, min_box, score_thr, clip_wh)
        s = s32.astype(np.float64)
        b = b32.astype(np.float64)
        area = _areas(b)
        live = np.ones(len(idx), bool)
        while live.any():
            cand = np.nonzero(live)[0]
            srt = np.sort(s[cand])[::-1]
            if srt.size > 1:
                worst = min(worst, (srt[0] - srt[1]) / srt[0])
            j = cand[np.argmax(s[cand])]
            live[j] = False
            o = np.nonzero(live)[0]
            if not o.size:
                break
            with np.errstate(divide='ignore', invalid='ignore'):
                iou = onms.compute_iou(b[j], b[o], area[j], area[o])
            t = s[o] * np.exp(-(iou * iou) / sigma)
            worst = min(worst, float(np.min(np.abs(t - score_thr) / score_thr)))
            s[o] = t
            live[o[np.isnan(iou) | ~(t >= score_thr)]] = False
    return worst
