"""NumPy restatements of the device merge of tiled inference (y3_tile_merge / y3_nms_labelled, include/yolo3hip.h).

The pool is built from the host functions of inference_tiled.py: ``merge_tile`` is merge_tile_detections with the seam
margin added (margin 0 is that function, test_cpu_tile_merge.py holds them equal) and finalize_predictions is used as it
is.  The labelled NMS is built on tests/nms_variants_reference.py: the same greedy / soft loops over the rows of one class.
"""
import numpy as np

import inference_tiled as it
import nms_variants_reference as ref

F = np.float32
E = it.EDGE_EFFECT_RANGE


def merge_tile(boxes, scores, class_label, tile_x, tile_y, tile_size, img_size, margin=0.0):
    """merge_tile_detections with ``margin``: the ghost band a centre is rejected in starts margin pixels further out.
    The two shifted limits are float32 operations: float32(E) - float32(margin) and float32(size - E) + float32(margin)."""
    scores = scores.reshape((-1, 1))
    class_label = class_label.reshape((-1, 1))
    cx = (boxes[:, 2] + boxes[:, 0]) / 2.0
    cy = (boxes[:, 3] + boxes[:, 1]) / 2.0
    cxg, cyg = cx + tile_x, cy + tile_y
    lo = F(E) - F(margin)
    hi_y, hi_x = F(tile_size[0] - E) + F(margin), F(tile_size[1] - E) + F(margin)
    invalid = ((cyg > E) & (cy < lo)) | ((cyg <= img_size[0] - E) & (cy >= hi_y)) | \
              ((cxg > E) & (cx < lo)) | ((cxg <= img_size[1] - E) & (cx >= hi_x))
    boxes, scores, class_label = boxes[~invalid, :], scores[~invalid], class_label[~invalid]
    if boxes.shape[0] == 0:
        return None
    boxes = boxes.copy()
    boxes[:, 0] += tile_x
    boxes[:, 2] += tile_x
    boxes[:, 1] += tile_y
    boxes[:, 3] += tile_y
    return boxes, scores, class_label


def tile_detections(rows, keep_idx, keep_cnt, keep_score):
    """What bbox_utils.detect_async's collect() hands the host merge, from a batch's rows [n, nb, ld] and keep lists: per
    tile (boxes [M,4] f32, scores [M] f32, labels [M] i32), class-major, keep order inside a class; None for an empty tile."""
    out = []
    n, K = keep_cnt.shape
    for t in range(n):
        b, s, lab = [], [], []
        for c in range(K):
            m = int(keep_cnt[t, c])
            idx = keep_idx[t, c, :m].astype(np.int64)
            b.append(rows[t, idx, 0:4].astype(np.float32))
            s.append(keep_score[t, c, :m].astype(np.float32))
            lab.append(np.full(m, c, np.int32))
        b, s, lab = np.concatenate(b), np.concatenate(s), np.concatenate(lab)
        out.append((b, s, lab) if b.shape[0] else None)
    return out


def pool(dets, xs, ys, tile_size, img_size, margin=0.0, host=False):
    """The merged pool float64 [M, 6] of one image: dets = per tile tile_detections' entry, xs / ys the clamped origins.
    host=True uses merge_tile_detections itself (margin must be 0)."""
    bl, sl, ll = [], [], []
    for k, d in enumerate(dets):
        if d is None:
            continue
        if host:
            assert margin == 0
            r = it.merge_tile_detections(d[0], d[1], d[2], xs[k], ys[k], tile_size, img_size)
        else:
            r = merge_tile(d[0], d[1], d[2], xs[k], ys[k], tile_size, img_size, margin)
        if r is not None:
            bl.append(r[0])
            sl.append(r[1])
            ll.append(r[2])
    return it.finalize_predictions(bl, sl, ll, img_size)


def nms_labelled(pool_rows, K, method, iou_thr=0.3, score_thr=0.1, sigma=0.5):
    """Class-wise NMS over pool rows [M, 6] (float32 values): per class (pool row indices int32, scores) in keep order.
    'none': every row of the class by key (score descending, ties: higher row first); hard / diou: every row of the class
    is a candidate; soft: those with score >= score_thr.  A row whose score is not > 0 is never a candidate."""
    p = np.asarray(pool_rows, np.float32).reshape(-1, 6)
    out = []
    for c in range(K):
        idx = np.nonzero((p[:, 5] == F(c)) & (p[:, 4] > F(0)))[0].astype(np.int64)      # only a positive score is a candidate
        if method.startswith('soft'):
            idx = idx[p[idx, 4] >= F(score_thr)]
        b, s = p[idx, 0:4], p[idx, 4]
        if method == 'none':
            order = np.argsort(ref.order_keys(s, idx), kind='stable')[::-1]
            out.append((idx[order].astype(np.int32), s[order]))
        elif method in ('hard', 'diou'):
            out.append(ref.greedy(idx, b, s, iou_thr, method) if idx.size else (np.zeros(0, np.int32), np.zeros(0, np.float32)))
        else:
            out.append(ref.soft(idx, b, s, iou_thr, score_thr, method, sigma))
    return out


def gather_kept(pool_rows, per_class):
    """The kept rows as a new pool: class-major, keep order, column 4 = the (decayed) keep score."""
    p = np.asarray(pool_rows)
    parts = []
    for r, s in per_class:
        q = p[np.asarray(r, np.int64)].copy()
        q[:, 4] = np.asarray(s, np.float32)
        parts.append(q)
    return np.concatenate(parts) if parts else p[:0].copy()
