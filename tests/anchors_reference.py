"""Plain-loop restatement of the anchor statistics (y3_anchor_stats / yolo3.anchors.anchor_stats), for the tests only.

One box and one anchor at a time: the IoU of the co-centred sizes in float32, one NumPy float32 scalar operation per step of
imagereader.format_boxes' expression; q = np.rint(iou * 2^24); the best anchor is the first maximum of the IoU; the sums are Python
ints.  Shares no code with yolo3/anchors.py."""
import numpy as np

F = np.float32
TWO24 = 16777216


def iou(w, h, aw, ah):
    w, h, aw, ah = F(w), F(h), F(aw), F(ah)
    two, zero = F(2.0), F(0.0)
    lo_w = min(F(w / two), F(aw / two))
    hi_w = max(F(-w / two), F(-aw / two))
    iw = max(F(lo_w - hi_w), zero)
    lo_h = min(F(h / two), F(ah / two))
    hi_h = max(F(-h / two), F(-ah / two))
    ih = max(F(lo_h - hi_h), zero)
    inter = F(iw * ih)
    union = F(F(F(w * h) + F(aw * ah)) - inter)
    return F(inter / union)


def q_of(v):
    return int(np.rint(F(F(v) * F(TWO24))))


def stats(wh, cands, thr_q, per_anchor):
    """-> (list [P][k][5] or [P][2] of Python ints, skipped, labels of set 0 as a list (255: skipped))."""
    cands = np.asarray(cands, np.float32)
    P, k = cands.shape[:2]
    out = [[[0] * 5 for _ in range(k)] for _ in range(P)] if per_anchor else [[0, 0] for _ in range(P)]
    skipped, labels = 0, []
    for w, h in np.asarray(wh).tolist():
        if not (1 <= w <= 65535 and 1 <= h <= 65535):
            skipped += 1
            labels.append(255)
            continue
        for p in range(P):
            best, best_iou = 0, None
            for a in range(k):
                v = iou(w, h, cands[p, a, 0], cands[p, a, 1])
                if a == 0 or v > best_iou:
                    best, best_iou = a, v
            q = q_of(best_iou)
            if per_anchor:
                row = out[p][best]
                row[0] += 1
                row[1] += w
                row[2] += h
                row[3] += q
                row[4] += int(q >= thr_q)
            else:
                out[p][0] += q
                out[p][1] += int(q >= thr_q)
            if p == 0:
                labels.append(best)
    return out, skipped, labels


def mixture(n=20000, seed=0):
    """The synthetic sizes of the fitting tests: four centres, each times exp(N(0, 0.25)) per axis, rounded, at least 1."""
    rng = np.random.default_rng(seed)
    centres = np.array([(12, 12), (40, 90), (200, 60), (300, 300)], np.float64)
    c = centres[rng.integers(0, 4, n)]
    return np.maximum(np.rint(c * np.exp(rng.normal(0.0, 0.25, (n, 2)))), 1).astype(np.int64)
