"""Detection accuracy: COCO-style 101-point AP / mAP of the ``detect`` path against ground truth, on the GPU.

Not in the reference.  The metric (yolo3hip.h ``y3_eval_*``):

- ground truth X,Y,W,H,C (build_lmdb.py / bbox_utils.load_boxes_to_xywhc) -> corners (X, Y, X+W, Y+H);
- detections = the NMS keep lists (descending score, ties: higher row index), optionally cut to ``max_detections``
  per (image, class);
- per image, class and IoU threshold t, in keep order, a detection takes the unmatched GT box of its class with the
  largest fp32 IoU (``y3_compute_iou``'s arithmetic; equal IoU: highest GT index) if that IoU >= t: a TP;
- per (class, t) over all images, sorted by score descending (ties: image order, then keep rank): the 101-point
  interpolated AP; a class without GT has AP NaN and is left out of every mean.

Matching runs on the device (``y3_eval_match``) straight on ``nms_device``'s keep lists; each batch appends its
(key, TP mask) entries to device pools at positions fixed by an exclusive prefix over the keep counts
(``y3_eval_offsets``: the one count the host reads per batch).  ``result()`` sorts the pools once (torch.sort,
stable) and runs ``y3_eval_ap``.

Across processes: ``state()`` exports the pools with the number of entries each image added, ``merge``
concatenates several states' per-image blocks in global image order (the single-process pool order, so the merged
result is bit-identical to one evaluator that saw every image), and ``all_gather_evaluator`` does that over a
torch.distributed group.  ``evaluate_examples`` is the batching loop evaluate.py and train.py --test_map share.

Opt-in: ``area_ranges`` scores every class once per closed range of box area with COCO's ignore rule
(``y3_eval_match_ranges``), ``curves`` adds the best-F1 score cut and the 101-point PR curve per (class, range, threshold)
(``y3_eval_ap_ranges``).  Without them the three kernels above run exactly as before.

Opt-in: ``class_score_thresholds`` cuts every keep list at its class's score threshold on the device before
matching (``y3_keep_cut``; ``load_score_thresholds`` reads the cuts from an operating-points csv), ``confusion`` also matches
each image class-agnostically and counts the [T, K+1, K+1] confusion matrix (``y3_eval_confusion``).
"""
import csv
import zlib


import numpy as np
import torch

from ._hip import lib, check, float_array
from . import bbox_utils, imagereader, lmdbio
from .isg_ai_pb import ImageYoloBoxesPair

COCO_IOU_THRESHOLDS = tuple(float(np.float32(0.5) + np.float32(0.05) * np.float32(k)) for k in range(10))
MAX_GT_PER_CLASS = 4096     # Y3_EVAL_MAX_GT: the GT boxes of one (image, class) are staged in LDS
MAX_AREA_RANGES = 8         # Y3_EVAL_MAX_RANGES
MAX_GT_PER_IMAGE = 4096     # with confusion=True the GT boxes of one IMAGE, all classes, are staged in LDS
COCO_AREA_RANGES = (('all', -np.inf, np.inf), ('small', 0.0, 32.0 ** 2), ('medium', 32.0 ** 2, 96.0 ** 2), ('large', 96.0 ** 2, 1e10))


def check_area_ranges(area_ranges, area_names=None):
    """'coco' or a sequence of (lo, hi) -> (float32 [A,2], names [A]).  1..8 ranges, lo < hi, +-inf allowed, NaN refused;
    area_names: one name per range (default: the preset's, else 'LO:HI')."""
    if isinstance(area_ranges, str):
        if area_ranges != 'coco':
            raise ValueError("area_ranges: 'coco' or a sequence of (lo, hi), got {!r}".format(area_ranges))
        names = [r[0] for r in COCO_AREA_RANGES]
        area_ranges = [r[1:] for r in COCO_AREA_RANGES]
    else:
        names = None
    try:
        rng = np.asarray(area_ranges, np.float32)
    except (TypeError, ValueError):
        raise ValueError('area_ranges: a sequence of (lo, hi) pairs, got {!r}'.format(area_ranges))
    if rng.ndim != 2 or rng.shape[1] != 2 or not 1 <= rng.shape[0] <= MAX_AREA_RANGES:
        raise ValueError('area_ranges: 1..{} (lo, hi) pairs, got shape {}'.format(MAX_AREA_RANGES, rng.shape))
    if not np.all(rng[:, 0] < rng[:, 1]):                          # a NaN bound fails the comparison too
        raise ValueError('area_ranges: every range needs lo < hi (no NaN), got {}'.format(rng.tolist()))
    if area_names is not None:
        names = [str(v) for v in area_names]
        if len(names) != rng.shape[0]:
            raise ValueError('{} area_names for {} ranges'.format(len(names), rng.shape[0]))
    elif names is None:
        names = ['{:g}:{:g}'.format(lo, hi) for lo, hi in rng]
    return rng, names


def gt_corners(boxes_xywhc):
    """[G,5] X,Y,W,H,C -> float32 [G,5] x0,y0,x1,y1,C."""
    b = np.asarray(boxes_xywhc, np.float64).reshape(-1, 5)
    out = np.empty((b.shape[0], 5), np.float32)
    out[:, 0] = b[:, 0]
    out[:, 1] = b[:, 1]
    out[:, 2] = b[:, 0] + b[:, 2]
    out[:, 3] = b[:, 1] + b[:, 3]
    out[:, 4] = b[:, 4]
    return out


def decode_pool_key(keys):
    """int64 pool keys -> (class int32, score float32) (inverse of the key y3_eval_match writes)."""
    keys = np.asarray(keys, np.int64)
    cls = (keys >> 32).astype(np.int32)
    mono = (~(keys & 0xffffffff)) & 0xffffffff
    bits = np.where(mono >= 2**31, mono - 2**31, (~mono) & 0xffffffff).astype(np.uint32)
    return cls, bits.view(np.float32)


class DetectionEvaluator:
    """Accumulates matches over batches of images; ``result()`` gives AP / recall / TP / FP per (class, threshold).

    iou_thresholds: 1..32 values in (0, 1], fp32 (default: COCO's 0.50:0.05:0.95).  max_detections: keep at most this
    many detections per (image, class) in score order (default: every entry NMS kept).  area_ranges: 'coco' or 1..8
    (lo, hi) closed ranges of box area, area_names their names: AP / recall / TP / FP per range with the ignore rule of DESIGN
    §3.16.  curves: also the best-F1 score cut and the PR curve per (class, range, threshold); without ranges over the one
    range (-inf, inf).  Either option switches matching and AP to the *_ranges kernels; ``state``, ``matches`` and ``result``
    then carry one TP and one ignore mask per entry and range.  class_score_thresholds: a number or K values (finite or -inf):
    every input path's keep lists are cut to the entries with score >= their class's threshold before matching, so every number
    is that of the cut lists.  confusion: also count the class-agnostic confusion matrix of the same lists; at
    most 4096 GT boxes per image then."""

    def __init__(self, num_classes, iou_thresholds=COCO_IOU_THRESHOLDS, max_detections=None, device=None, area_ranges=None, area_names=None,
                 curves=False, class_score_thresholds=None, confusion=False):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError('num_classes must be >= 1')
        thr = np.asarray(iou_thresholds, np.float32).reshape(-1)
        if not 1 <= thr.size <= 32 or not np.all((thr > 0) & (thr <= 1)):
            raise ValueError('iou_thresholds: 1..32 values in (0, 1], got {}'.format(list(thr)))
        self.iou_thresholds = thr
        if max_detections is not None and int(max_detections) < 1:
            raise ValueError('max_detections must be >= 1')
        self.max_detections = None if max_detections is None else int(max_detections)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._thr_host = float_array(thr)
        self.curves = bool(curves)
        self._ranged = area_ranges is not None or self.curves
        self.area_ranges, self.area_names = None, None
        if area_ranges is None and area_names is not None:
            raise ValueError('area_names go with area_ranges')
        if self._ranged:
            self.area_ranges, self.area_names = check_area_ranges([COCO_AREA_RANGES[0][1:]], ['all']) if area_ranges is None else \
                check_area_ranges(area_ranges, area_names)
            self._lo_host = float_array(self.area_ranges[:, 0])
            self._hi_host = float_array(self.area_ranges[:, 1])
        self.confusion = bool(confusion)
        self.class_score_thresholds = None if class_score_thresholds is None else \
            bbox_utils.check_class_thresholds(class_score_thresholds, self.num_classes)
        self._cut_dev = None if self.class_score_thresholds is None else torch.from_numpy(self.class_score_thresholds).to(self.device)
        self.reset()

    def reset(self):
        self._keys = torch.empty(0, dtype=torch.int64, device=self.device)
        self._tp = torch.empty(self._mask_shape(0), dtype=torch.int32, device=self.device)
        self._ign = torch.empty(self._mask_shape(0), dtype=torch.int32, device=self.device) if self._ranged else None
        self._npos_area = np.zeros((self.num_classes, len(self.area_ranges)), np.int64) if self._ranged else None
        self._used = 0
        self._counts = []         # per batch: int32 device [n] = pool entries each image added (image order)
        self._npos = np.zeros(self.num_classes, np.int64)
        self.num_images = 0
        self._confusion = torch.zeros(len(self.iou_thresholds), self.num_classes + 1, self.num_classes + 1, dtype=torch.int64,
                                      device=self.device) if self.confusion else None

    # ---- input paths ----------------------------------------------------------------------------------------------
    def add_batch(self, rows, gt_boxes_per_image, min_box_size, clip_wh=None, iou_threshold=0.3, score_threshold=0.1, nms='hard',
                  nms_sigma=0.5):
        """rows: CUDA float32 [N, Nb, 5+K] (the network's decode rows); gt_boxes_per_image: N arrays [G,5] X,Y,W,H,C.
        Runs the ``detect`` path's NMS (``bbox_utils.nms_device``, same clip / small-box filter / thresholds; method
        ``nms`` of bbox_utils.NMS_METHODS, Gaussian parameter ``nms_sigma``) and matches its keep lists on the device;
        no detection leaves the GPU."""
        bbox_utils.check_nms_args(nms, nms_sigma, score_threshold)
        assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 3
        n, nb, d = rows.shape
        if d - 5 != self.num_classes:
            raise ValueError('rows carry {} classes, the evaluator {}'.format(d - 5, self.num_classes))
        gt = self._gt_batch(gt_boxes_per_image, n)
        rows = rows.contiguous()
        keep_idx, keep_cnt, keep_score = bbox_utils.nms_device(rows, min_box_size, iou_threshold, score_threshold, clip_wh, method=nms,
                                                                sigma=nms_sigma)
        cw, chh = (float(clip_wh[0]), float(clip_wh[1])) if clip_wh is not None else (-1.0, -1.0)
        self._match(rows, n, nb, d, cw, chh, keep_idx, keep_cnt, keep_score, nb, gt)

    def add_detections(self, boxes, scores, labels, gt, row_index=None):
        """Host detections from any source, one entry per image: boxes [M,4] corners x0,y0,x1,y1, scores [M], labels [M]
        int class ids, gt [G,5] X,Y,W,H,C; an image's boxes may be None (no detections, as ``bbox_utils.detect`` returns).
        Sorted on the host into keep order (score descending, ties: higher row index; row_index: per image [M] ints, e.g.
        ``detect``'s keep rows, default the position in the array) and matched by the same kernels as ``add_batch``
        (no clip)."""
        n = len(boxes)
        if row_index is None:
            row_index = [None] * n
        if not (len(scores) == len(labels) == len(gt) == len(row_index) == n) or n == 0:
            raise ValueError('boxes, scores, labels and gt need one entry per image (at least one image)')
        K = self.num_classes
        per = []
        for i in range(n):
            if boxes[i] is None:                  # bbox_utils.detect's (None,)*4 for an image without detections
                per.append((np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)))
                continue
            b = np.asarray(boxes[i], np.float32).reshape(-1, 4)
            s = np.asarray(scores[i], np.float32).reshape(-1)
            lab = np.asarray(labels[i]).reshape(-1)
            if not (b.shape[0] == s.shape[0] == lab.shape[0]):
                raise ValueError('image {}: {} boxes, {} scores, {} labels'.format(i, b.shape[0], s.shape[0], lab.shape[0]))
            if not (np.all(np.isfinite(b)) and np.all(np.isfinite(s))):
                raise ValueError('image {}: non-finite box or score'.format(i))
            if lab.size and (lab.min() < 0 or lab.max() >= K or np.any(lab != np.round(lab))):
                raise ValueError('image {}: labels outside 0..{}'.format(i, K - 1))
            rid = np.arange(b.shape[0]) if row_index[i] is None else np.asarray(row_index[i], np.int64).reshape(-1)
            if rid.shape[0] != b.shape[0]:
                raise ValueError('image {}: {} row indices for {} boxes'.format(i, rid.shape[0], b.shape[0]))
            per.append((b, s, lab.astype(np.int64), rid))
        mb = max(1, max(p[0].shape[0] for p in per))
        rows = np.zeros((n, mb, 4), np.float32)
        keep_idx = np.zeros((n, K, mb), np.int32)
        keep_cnt = np.zeros((n, K), np.int32)
        keep_score = np.zeros((n, K, mb), np.float32)
        for i, (b, s, lab, rid) in enumerate(per):
            rows[i, :b.shape[0]] = b
            for c in range(K):
                idx = np.nonzero(lab == c)[0]
                order = idx[np.lexsort((-rid[idx], -s[idx].astype(np.float64)))]     # score desc, then higher row index first
                keep_idx[i, c, :order.size] = order
                keep_score[i, c, :order.size] = s[order]
                keep_cnt[i, c] = order.size
        gtb = self._gt_batch(gt, n)
        dev = self.device
        self._match(torch.from_numpy(rows).to(dev), n, mb, 4, -1.0, -1.0, torch.from_numpy(keep_idx).to(dev),
                    torch.from_numpy(keep_cnt).to(dev), torch.from_numpy(keep_score).to(dev), mb, gtb)

    def add_pool(self, pool, count, gt_xywhc, nms='none', iou_threshold=0.3, score_threshold=0.1, nms_sigma=0.5):
        """One whole image from the tiled pipeline: pool CUDA float32 [>= count, 6] = x0, y0, x1, y1, score, class
        (inference_tiled.tiled_pool_device), its first ``count`` rows valid; gt_xywhc [G,5] X,Y,W,H,C.  nms: 'none' or a
        method of bbox_utils.NMS_METHODS run class-wise over the pool first (bbox_utils.nms_labelled_device; the soft methods
        replace the scores by the decayed ones), as inference_image_tiled(..., merge_nms=nms) does.  The detections are then
        put in keep order on the device (y3_nms_labelled with Y3_NMS_NONE: score descending, ties: higher row first) and
        matched; no detection leaves the GPU.  The state afterwards is, bit for bit, that of ``add_detections`` on the array
        inference_image_tiled returns for the same settings.  Rows whose class is outside 0..K-1 are ignored."""
        if nms != 'none':
            bbox_utils.check_nms_args(nms, nms_sigma, score_threshold)
        assert pool.is_cuda and pool.dtype == torch.float32 and pool.dim() == 2 and pool.shape[1] == 6 and 0 <= int(count) <= pool.shape[0]
        K = self.num_classes
        gt = self._gt_batch([gt_xywhc], 1)
        pool = pool[:int(count)].contiguous()
        if nms != 'none' and pool.shape[0]:
            kept = bbox_utils.nms_labelled_device(pool, K, nms, iou_threshold, score_threshold, nms_sigma)
            pool = bbox_utils.gather_kept(pool, *kept)
        m = pool.shape[0]
        keep_idx, keep_cnt, keep_score = bbox_utils.nms_labelled_device(pool, K, 'none')
        if m == 0:
            pool = torch.zeros(1, 6, dtype=torch.float32, device=self.device)
        self._match(pool, 1, max(m, 1), 6, -1.0, -1.0, keep_idx, keep_cnt, keep_score, max(m, 1), gt)

    # ---- device plumbing ------------------------------------------------------------------------------------------
    def _gt_batch(self, gt_list, n):
        if len(gt_list) != n:
            raise ValueError('{} ground-truth entries for {} images'.format(len(gt_list), n))
        K = self.num_classes
        corners = [gt_corners(g) for g in gt_list]
        npos = np.zeros(K, np.int64)
        worst = 0
        for i, g in enumerate(corners):
            if not np.all(np.isfinite(g)):
                raise ValueError('image {}: non-finite ground truth'.format(i))
            c = g[:, 4]
            if c.size and (c.min() < 0 or c.max() >= K or np.any(c != np.round(c))):
                raise ValueError('image {}: ground-truth classes outside 0..{}'.format(i, K - 1))
            per = np.bincount(c.astype(np.int64), minlength=K)
            npos += per
            worst = max(worst, int(per.max()) if per.size else 0)
        max_gt = max(1, max(g.shape[0] for g in corners))
        buf = np.zeros((n, max_gt, 5), np.float32)
        cnt = np.zeros(n, np.int32)
        for i, g in enumerate(corners):
            buf[i, :g.shape[0]] = g
            cnt[i] = g.shape[0]
        return buf, cnt, max_gt, worst, npos

    def _mask_shape(self, entries):
        return (entries, len(self.area_ranges)) if self._ranged else (entries,)

    def _npos_in_ranges(self, buf, cnt):
        """int64 [K, A]: the in-range GT boxes per class, by the match kernel's fp32 area arithmetic."""
        out = np.zeros_like(self._npos_area)
        for g, c in zip(buf, cnt):
            g = g[:c]
            area = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])                     # float32, as gar in the kernel
            for a, (lo, hi) in enumerate(self.area_ranges):
                out[:, a] += np.bincount(g[(lo <= area) & (area <= hi), 4].astype(np.int64), minlength=self.num_classes)
        return out

    def _match(self, rows, n, nb, ld, clip_w, clip_h, keep_idx, keep_cnt, keep_score, max_keep, gt):
        buf, cnt, max_gt, worst, npos = gt
        dev = self.device
        st = torch.cuda.current_stream(dev).cuda_stream
        K = self.num_classes
        max_det = max_keep if self.max_detections is None else min(self.max_detections, max_keep)
        if self._cut_dev is not None:                 # a private copy: nms_device's cached buffers belong to the caller
            keep_cnt = bbox_utils.cut_keep_lists(keep_cnt.clone(), keep_score, self._cut_dev)
        offsets = torch.empty(n * K + 1, dtype=torch.int32, device=dev)
        check(lib.y3_eval_offsets(keep_cnt.data_ptr(), n * K, max_keep, max_det, offsets.data_ptr(), st), 'y3_eval_offsets')
        gt_dev = torch.from_numpy(buf).to(dev)
        cnt_dev = torch.from_numpy(cnt).to(dev)
        total = int(offsets[n * K].item())                                # the one host read of the batch
        self._reserve(self._used + total)             # only grows capacity: a refused batch below (GT over the LDS cap) adds nothing
        used = self._used
        if self.confusion:
            # first: it refuses an image over the LDS cap (which every (image, class) over the cap is too) before anything is counted
            ws_bytes = int(lib.y3_eval_confusion_workspace_bytes(total))
            ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.int32, device=dev)
            check(lib.y3_eval_confusion(rows.data_ptr(), n, nb, ld, K, clip_w, clip_h, keep_idx.data_ptr(), keep_cnt.data_ptr(),
                                        keep_score.data_ptr(), max_keep, max_det, gt_dev.data_ptr(), cnt_dev.data_ptr(), max_gt,
                                        int(cnt.max()) if cnt.size else 0, self._thr_host, len(self.iou_thresholds), offsets.data_ptr(), total,
                                        ws.data_ptr(), ws_bytes, self._confusion.data_ptr(), st), 'y3_eval_confusion')
        if self._ranged:
            A = len(self.area_ranges)
            check(lib.y3_eval_match_ranges(rows.data_ptr(), n, nb, ld, K, clip_w, clip_h, keep_idx.data_ptr(), keep_cnt.data_ptr(),
                                           keep_score.data_ptr(), max_keep, max_det, gt_dev.data_ptr(), cnt_dev.data_ptr(), max_gt, worst,
                                           self._thr_host, len(self.iou_thresholds), self._lo_host, self._hi_host, A, offsets.data_ptr(),
                                           self._keys.data_ptr() + 8 * used, self._tp.data_ptr() + 4 * A * used,
                                           self._ign.data_ptr() + 4 * A * used, self._keys.numel() - used, st), 'y3_eval_match_ranges')
            self._npos_area += self._npos_in_ranges(buf, cnt)
        else:
            check(lib.y3_eval_match(rows.data_ptr(), n, nb, ld, K, clip_w, clip_h, keep_idx.data_ptr(), keep_cnt.data_ptr(),
                                    keep_score.data_ptr(), max_keep, max_det, gt_dev.data_ptr(), cnt_dev.data_ptr(), max_gt, worst,
                                    self._thr_host, len(self.iou_thresholds), offsets.data_ptr(), self._keys.data_ptr() + 8 * used,
                                    self._tp.data_ptr() + 4 * used, self._keys.numel() - used, st), 'y3_eval_match')
        self._used += total
        self._counts.append(torch.diff(offsets[0::K]))               # image i's entries: offsets[(i+1)K] - offsets[iK]
        self._npos += npos
        self.num_images += n

    def _reserve(self, need):
        cap = self._keys.numel()
        if need <= cap and cap > 0:                   # never empty: y3_eval_match takes the pool even for a batch without detections
            return
        cap = max(need, 2 * cap, 1024)
        keys = torch.empty(cap, dtype=torch.int64, device=self.device)
        tp = torch.empty(self._mask_shape(cap), dtype=torch.int32, device=self.device)
        keys[:self._used] = self._keys[:self._used]
        tp[:self._used] = self._tp[:self._used]
        self._keys, self._tp = keys, tp
        if self._ranged:
            ign = torch.empty(self._mask_shape(cap), dtype=torch.int32, device=self.device)
            ign[:self._used] = self._ign[:self._used]
            self._ign = ign

    # ---- state across processes -----------------------------------------------------------------------------------
    def image_counts(self):
        """int32 device [num_images]: pool entries each image added, in image order (they sum to the pool size)."""
        if len(self._counts) != 1:
            self._counts = [torch.cat(self._counts) if self._counts else torch.empty(0, dtype=torch.int32, device=self.device)]
        return self._counts[0]

    def state(self):
        """What ``merge`` / ``all_gather_evaluator`` combine (device tensors are copies): keys int64 [M], tp int32 [M] = the
        pools in (image, class, keep rank) order, image_counts int32 [num_images], npos int64 [K] (NumPy), num_images,
        iou_thresholds (float32), num_classes, max_detections.  With area ranges or curves: tp is [M, A] and the state also
        holds ign int32 [M, A], npos_area int64 [K, A], area_ranges float32 [A, 2], area_names, curves.  With
        class_score_thresholds: those (float32 [K]); with confusion: confusion int64 device [T, K+1, K+1]."""
        st = {'keys': self._keys[:self._used].clone(), 'tp': self._tp[:self._used].clone(), 'image_counts': self.image_counts().clone(),
              'npos': self._npos.copy(), 'num_images': self.num_images, 'iou_thresholds': self.iou_thresholds.copy(),
              'num_classes': self.num_classes, 'max_detections': self.max_detections}
        if self._ranged:
            st.update(ign=self._ign[:self._used].clone(), npos_area=self._npos_area.copy(), area_ranges=self.area_ranges.copy(),
                      area_names=list(self.area_names), curves=self.curves)
        if self.class_score_thresholds is not None:
            st['class_score_thresholds'] = self.class_score_thresholds.copy()
        if self.confusion:
            st['confusion'] = self._confusion.clone()
        return st

    @classmethod
    def merge(cls, states, order='strided', device=None):
        """A new evaluator holding the images of every state, its pool in GLOBAL image order.  order: 'strided' (W states:
        global image g is local image g // W of state g % W, the keys[rank::world] split of ImageReader(num_shards=W) and
        inference.py), or an explicit sequence of (state, local image) pairs naming every image once.  ``result()`` sorts
        stably, so equal scores rank by pool position: rebuilding the single-process order makes the merged result
        bit-identical to one evaluator fed all images in that order.  States must share thresholds, classes,
        max_detections, area ranges, curves, class_score_thresholds and the confusion flag; the confusion matrices are summed."""
        states = list(states)
        if not states:
            raise ValueError('merge needs at least one state')
        s0 = states[0]
        thr0 = np.asarray(s0['iou_thresholds'], np.float32)
        for i, s in enumerate(states[1:], 1):
            thr = np.asarray(s['iou_thresholds'], np.float32)
            if s['num_classes'] != s0['num_classes'] or s['max_detections'] != s0['max_detections'] or not np.array_equal(thr, thr0):
                raise ValueError('state {} does not match state 0: classes {} / {}, max_detections {} / {}, iou_thresholds {} / {}'.format(
                    i, s['num_classes'], s0['num_classes'], s['max_detections'], s0['max_detections'], list(thr), list(thr0)))
            if not _same_ranges(s, s0):
                raise ValueError('state {} does not match state 0: area_ranges {} / {}, curves {} / {}'.format(
                    i, _ranges_list(s), _ranges_list(s0), s.get('curves', False), s0.get('curves', False)))
            if not _same_cuts(s, s0) or ('confusion' in s) != ('confusion' in s0):
                raise ValueError('state {} does not match state 0: class_score_thresholds {} / {}, confusion {} / {}'.format(
                    i, _cuts_list(s), _cuts_list(s0), 'confusion' in s, 'confusion' in s0))
        state_index, local_index = global_image_order([int(s['num_images']) for s in states], order)
        ranged = s0.get('area_ranges') is not None
        ev = cls(s0['num_classes'], thr0, s0['max_detections'], device, area_ranges=s0['area_ranges'] if ranged else None,
                 area_names=s0['area_names'] if ranged else None, curves=bool(s0.get('curves', False)),
                 class_score_thresholds=s0.get('class_score_thresholds'), confusion='confusion' in s0)
        dev = ev.device
        counts = []
        for i, s in enumerate(states):
            c = s['image_counts'].to(dev, torch.int64)
            if c.numel() != int(s['num_images']) or int(c.sum()) != s['keys'].numel() or tuple(s['tp'].shape) != ev._mask_shape(s['keys'].numel()) \
                    or (ranged and tuple(s['ign'].shape) != tuple(s['tp'].shape)):
                raise ValueError('state {}: {} image counts summing to {} for {} images and {} keys / {} TP masks'.format(
                    i, c.numel(), int(c.sum()), s['num_images'], s['keys'].numel(), s['tp'].numel()))
            counts.append(c)
        total = sum(s['keys'].numel() for s in states)
        idx, cnt = pool_gather_index(counts, state_index, local_index, total)
        ev._reserve(total)
        if total:
            ev._keys[:total] = torch.cat([s['keys'].to(dev) for s in states])[idx]
            ev._tp[:total] = torch.cat([s['tp'].to(dev) for s in states])[idx]
            if ranged:
                ev._ign[:total] = torch.cat([s['ign'].to(dev) for s in states])[idx]
        ev._used = total
        ev._counts = [cnt.to(torch.int32)]
        ev._npos = np.sum([np.asarray(s['npos'], np.int64) for s in states], axis=0)
        if ranged:
            ev._npos_area = np.sum([np.asarray(s['npos_area'], np.int64) for s in states], axis=0)
        ev.num_images = int(state_index.size)
        if ev.confusion:
            for i, s in enumerate(states):
                if tuple(s['confusion'].shape) != tuple(ev._confusion.shape):
                    raise ValueError('state {}: confusion matrix of shape {}, expected {}'.format(i, tuple(s['confusion'].shape),
                                                                                                 tuple(ev._confusion.shape)))
                ev._confusion += s['confusion'].to(dev, torch.int64)
        return ev

    # ---- output ---------------------------------------------------------------------------------------------------
    def matches(self):
        """Pool entries in (image, class, keep rank) order: (class int32 [M], score float32 [M], TP mask uint32 [M]); with
        area ranges or curves (class, score, TP masks uint32 [M, A], ignore masks uint32 [M, A])."""
        keys = self._keys[:self._used].cpu().numpy()
        cls, score = decode_pool_key(keys)
        if self._ranged:
            return cls, score, self._tp[:self._used].cpu().numpy().view(np.uint32), self._ign[:self._used].cpu().numpy().view(np.uint32)
        return cls, score, self._tp[:self._used].cpu().numpy().view(np.uint32)

    def result(self):
        """dict of NumPy arrays (K = classes, T = thresholds):
        ap, recall [K,T] (NaN where npos == 0), tp, fp [K,T], npos [K], iou_thresholds [T], map [T] (mean AP over classes
        with npos > 0), map50 (t = 0.5; NaN if 0.5 is not a threshold), map50_95 (mean over classes and the ten COCO
        thresholds; NaN unless those are the thresholds), map_all (mean over classes and all thresholds), and at the
        operating-point threshold op_threshold (0.5, else the first one): tp50, fp50, precision50 (TP / (TP+FP), 0 without
        detections), recall50 (TP / npos, NaN without GT), f1_50 (0 when precision + recall is 0).
        With area ranges or curves (A = ranges) the keys above are those of the first range named 'all', else of
        range 0, and the dict adds area_ranges [A,2], area_names, ap_area, recall_area, tp_area, fp_area, ign_area [A,K,T],
        npos_area [K,A], map_area [A,T], map50_area, map50_95_area, ar_area [A] (mean final recall over the classes with GT and
        the thresholds); with curves also best_score, best_precision, best_recall, best_f1, best_tp, best_fp [A,K,T] (the best-F1
        score cut: keep score >= best_score; NaN / 0 without entries or GT) and pr_precision, pr_score [A,K,T,101].
        With class_score_thresholds the dict carries them (float32 [K]); with confusion it adds confusion int64 [T,K+1,K+1] (rows
        true, columns predicted, index K = background: row K the unmatched detections, column K the missed GT boxes; over all box
        areas) and confusion_op [K+1,K+1], the matrix at op_threshold."""
        res = self._result_ranges() if self._ranged else self._result_plain()
        if self.class_score_thresholds is not None:
            res['class_score_thresholds'] = self.class_score_thresholds.copy()
        if self.confusion:
            res['confusion'] = self._confusion.cpu().numpy()
            res['confusion_op'] = res['confusion'][int(np.nonzero(self.iou_thresholds == np.float32(res['op_threshold']))[0][0])].copy()
        return res

    def _result_plain(self):
        dev = self.device
        st = torch.cuda.current_stream(dev).cuda_stream
        K, T, m = self.num_classes, len(self.iou_thresholds), self._used
        keys, order = torch.sort(self._keys[:m], stable=True)
        tp = self._tp[:m][order].contiguous()
        keys = keys.contiguous()
        npos = torch.from_numpy(self._npos.astype(np.int32)).to(dev)
        ws_bytes = int(lib.y3_eval_ap_workspace_bytes(m, T))
        ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device=dev)
        ap = torch.empty(K, T, dtype=torch.float32, device=dev)
        rec = torch.empty(K, T, dtype=torch.float32, device=dev)
        tpc = torch.empty(K, T, dtype=torch.int32, device=dev)
        fpc = torch.empty(K, T, dtype=torch.int32, device=dev)
        check(lib.y3_eval_ap(keys.data_ptr() if m else None, tp.data_ptr() if m else None, m, K, T, npos.data_ptr(), ws.data_ptr(),
                             ws_bytes, ap.data_ptr(), rec.data_ptr(), tpc.data_ptr(), fpc.data_ptr(), st), 'y3_eval_ap')
        return summarize(ap.cpu().numpy().astype(np.float64), rec.cpu().numpy().astype(np.float64), tpc.cpu().numpy().astype(np.int64),
                         fpc.cpu().numpy().astype(np.int64), self._npos.copy(), self.iou_thresholds)

    def _result_ranges(self):
        dev = self.device
        st = torch.cuda.current_stream(dev).cuda_stream
        K, T, A, m = self.num_classes, len(self.iou_thresholds), len(self.area_ranges), self._used
        keys, order = torch.sort(self._keys[:m], stable=True)
        tp = self._tp[:m][order].contiguous()
        ign = self._ign[:m][order].contiguous()
        keys = keys.contiguous()
        npos = torch.from_numpy(self._npos_area.astype(np.int32)).to(dev)
        ws_bytes = int(lib.y3_eval_ap_ranges_workspace_bytes(m, A, T))
        ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device=dev)
        f = {k: torch.empty(K, A, T, dtype=torch.float32, device=dev) for k in ('ap', 'recall', 'best_score')}
        i = {k: torch.empty(K, A, T, dtype=torch.int32, device=dev) for k in ('tp', 'fp', 'ign', 'best_n', 'best_tp')}
        pr = [torch.empty(K, A, T, 101, dtype=torch.float32, device=dev) for _ in range(2)] if self.curves else None
        check(lib.y3_eval_ap_ranges(keys.data_ptr() if m else None, tp.data_ptr() if m else None, ign.data_ptr() if m else None, m, K, A, T,
                                    npos.data_ptr(), ws.data_ptr(), ws_bytes, f['ap'].data_ptr(), f['recall'].data_ptr(), i['tp'].data_ptr(),
                                    i['fp'].data_ptr(), i['ign'].data_ptr(), i['best_n'].data_ptr(), i['best_tp'].data_ptr(),
                                    f['best_score'].data_ptr(), pr[0].data_ptr() if pr else None, pr[1].data_ptr() if pr else None, st),
              'y3_eval_ap_ranges')
        out = {k: v.cpu().numpy().transpose(1, 0, 2) for k, v in f.items()}                      # [K,A,T] -> [A,K,T]
        out.update({k: v.cpu().numpy().astype(np.int64).transpose(1, 0, 2) for k, v in i.items()})
        if pr:
            out['pr_precision'], out['pr_score'] = (v.cpu().numpy().transpose(1, 0, 2, 3) for v in pr)
        return summarize_ranges(out, self._npos_area.copy(), self.iou_thresholds, self.area_ranges, self.area_names, self.curves)


def _ranges_list(state):
    r = state.get('area_ranges')
    return None if r is None else np.asarray(r, np.float32).tolist()


def _cuts_list(state):
    c = state.get('class_score_thresholds')
    return None if c is None else np.asarray(c, np.float32).tolist()


def _same_cuts(s, s0):
    a, b = s.get('class_score_thresholds'), s0.get('class_score_thresholds')
    if (a is None) != (b is None):
        return False
    return a is None or np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def load_score_thresholds(spec, num_classes, range_name='all', iou=0.5):
    """Per-class score thresholds -> float32 [num_classes].  spec: a number (or its text), one cut for every class, or the path of a
    csv written by evaluate.py --operating-points: per class the score_threshold cell of the row whose range is ``range_name`` and
    whose np.float32(iou_threshold) equals np.float32(iou), parsed as np.float32(float(cell)) (the writer prints
    repr(float(float32)), so the bits round-trip).  An empty cell (a class without entries or ground truth) gives -inf: no cut
    beyond the pipeline's base threshold.  ValueError names a missing class, range or IoU row, a NaN, or a wrong class count."""
    K = int(num_classes)
    if not isinstance(spec, str):
        return bbox_utils.check_class_thresholds(spec, K)
    try:
        value = float(spec)
    except ValueError:
        value = None
    if value is not None:
        return bbox_utils.check_class_thresholds(value, K)
    with open(spec, newline='') as fh:
        rows = list(csv.DictReader(fh))
    for col in ('class', 'range', 'iou_threshold', 'score_threshold'):
        if not rows or col not in rows[0]:
            raise ValueError('{}: not an operating-points csv (no rows or no {!r} column)'.format(spec, col))
    if not any(r['range'] == range_name for r in rows):
        raise ValueError('{}: no rows of range {!r} (it has {})'.format(spec, range_name, sorted({r['range'] for r in rows})))
    rows = [r for r in rows if r['range'] == range_name]
    if not any(np.float32(float(r['iou_threshold'])) == np.float32(iou) for r in rows):
        raise ValueError('{}: no rows of IoU threshold {!r} in range {!r} (it has {})'.format(
            spec, iou, range_name, sorted({float(r['iou_threshold']) for r in rows})))
    rows = [r for r in rows if np.float32(float(r['iou_threshold'])) == np.float32(iou)]
    classes = sorted(int(r['class']) for r in rows)
    if classes != list(range(len(classes))) or len(classes) != K:
        missing = sorted(set(range(K)) - set(classes))
        raise ValueError('{}: rows of classes {} for a model of {} classes{}'.format(
            spec, classes, K, ' (class {} is missing)'.format(missing[0]) if missing else ''))
    thr = np.empty(K, np.float32)
    for r in rows:
        cell = r['score_threshold'].strip()
        thr[int(r['class'])] = np.float32(float(cell)) if cell else np.float32(-np.inf)
    return bbox_utils.check_class_thresholds(thr, K)


def _same_ranges(s, s0):
    a, b = s.get('area_ranges'), s0.get('area_ranges')
    if (a is None) != (b is None) or bool(s.get('curves', False)) != bool(s0.get('curves', False)):
        return False
    return a is None or np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))


def summarize_ranges(out, npos_area, iou_thresholds, area_ranges, area_names, curves):
    """The result dict of a DetectionEvaluator with area ranges or curves from the [A,K,T] numbers of y3_eval_ap_ranges."""
    thr = np.asarray(iou_thresholds, np.float32)
    A = len(area_names)
    a0 = area_names.index('all') if 'all' in area_names else 0
    ap, rec = out['ap'].astype(np.float64), out['recall'].astype(np.float64)
    res = summarize(ap[a0], rec[a0], out['tp'][a0], out['fp'][a0], npos_area[:, a0].copy(), thr)
    res.update(area_ranges=np.asarray(area_ranges, np.float32).copy(), area_names=list(area_names), ap_area=ap, recall_area=rec,
               tp_area=out['tp'], fp_area=out['fp'], ign_area=out['ign'], npos_area=npos_area)
    hits = np.nonzero(thr == np.float32(0.5))[0]
    coco = thr.size == 10 and np.array_equal(thr, np.asarray(COCO_IOU_THRESHOLDS, np.float32))
    res['map_area'] = np.full((A, thr.size), np.nan)
    res['map50_area'], res['map50_95_area'], res['ar_area'] = (np.full(A, np.nan) for _ in range(3))
    for a in range(A):
        valid = npos_area[:, a] > 0
        if not valid.any():
            continue
        res['map_area'][a] = ap[a][valid].mean(axis=0)
        if hits.size:
            res['map50_area'][a] = res['map_area'][a, hits[0]]
        if coco:
            res['map50_95_area'][a] = ap[a][valid].mean()
        res['ar_area'][a] = rec[a][valid].mean()
    if curves:
        n, t = out['best_n'], out['best_tp']
        npos = npos_area.T[:, :, None].astype(np.float64)                                         # [A,K,1]
        with np.errstate(invalid='ignore', divide='ignore'):
            res.update(best_score=out['best_score'], best_tp=t, best_fp=n - t, best_precision=np.where(n > 0, t / np.maximum(n, 1), np.nan),
                       best_recall=np.where(npos > 0, t / np.maximum(npos, 1), np.nan),
                       best_f1=np.where(npos > 0, 2.0 * t / np.maximum(n + npos, 1), np.nan),
                       pr_precision=out['pr_precision'], pr_score=out['pr_score'])
    return res


def summarize(ap, recall, tp, fp, npos, iou_thresholds):
    """The result dict of DetectionEvaluator.result() from the per-(class, threshold) numbers."""
    thr = np.asarray(iou_thresholds, np.float32)
    valid = npos > 0
    with np.errstate(invalid='ignore', divide='ignore'):
        per_t = ap[valid].mean(axis=0) if valid.any() else np.full(thr.size, np.nan)
        hits = np.nonzero(thr == np.float32(0.5))[0]
        op = int(hits[0]) if hits.size else 0
        t50, f50 = tp[:, op], fp[:, op]
        prec = np.where(t50 + f50 > 0, t50 / np.maximum(t50 + f50, 1), 0.0)
        rec = np.where(valid, t50 / np.maximum(npos, 1), np.nan)
        s = prec + rec
        ok = valid & (s > 0)
        f1 = np.where(valid, 0.0, np.nan)
        f1[ok] = 2 * prec[ok] * rec[ok] / s[ok]
    coco = thr.size == 10 and np.array_equal(thr, np.asarray(COCO_IOU_THRESHOLDS, np.float32))
    return {
        'ap': ap, 'recall': recall, 'tp': tp, 'fp': fp, 'npos': npos, 'iou_thresholds': thr, 'map': per_t,
        'map50': float(per_t[hits[0]]) if hits.size else float('nan'),
        'map50_95': float(ap[valid].mean()) if coco and valid.any() else float('nan'),
        'map_all': float(ap[valid].mean()) if valid.any() else float('nan'),
        'op_threshold': float(thr[op]), 'tp50': t50, 'fp50': f50, 'precision50': prec, 'recall50': rec, 'f1_50': f1,
    }


def global_image_order(num_images, order='strided'):
    """(state index, local image index): int64 arrays [N], entry g = where global image g lives.  num_images: images per
    state.  'strided': W states, global image g = local image g // W of state g % W; state s must hold ceil((N - s) / W)
    of the N images.  Otherwise ``order`` is a sequence of (state, local image) pairs naming every image exactly once."""
    counts = [int(v) for v in num_images]
    W, N = len(counts), sum(counts)
    if W == 0:
        raise ValueError('no states')
    if isinstance(order, str):
        if order != 'strided':
            raise ValueError("order must be 'strided' or a sequence of (state, local image) pairs, got {!r}".format(order))
        want = [(N - s + W - 1) // W for s in range(W)]
        if counts != want:
            raise ValueError('image counts {} are not a strided split of {} images over {} states ({})'.format(counts, N, W, want))
        g = np.arange(N, dtype=np.int64)
        return g % W, g // W
    pairs = np.asarray(list(order), np.int64).reshape(-1, 2)
    s, loc = pairs[:, 0].copy(), pairs[:, 1].copy()
    if pairs.shape[0] != N or np.any((s < 0) | (s >= W)) or np.any(loc < 0) or np.any(loc >= np.asarray(counts, np.int64)[np.clip(s, 0, W - 1)]):
        raise ValueError('order must name each of the {} images of {} states (counts {}) once'.format(N, W, counts))
    base = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    if np.unique(base[s] + loc).size != N:
        raise ValueError('order names an image twice')
    return s, loc


def pool_gather_index(image_counts, state_index, local_index, total):
    """Index plumbing of ``merge``: image_counts = per state int64 tensor [images of the state] (pool entries per image);
    state_index / local_index = global_image_order.  Returns (index int64 [total] into the state-major concatenation of the
    pools that puts the per-image blocks in global order, entries per image int64 [N] in global order)."""
    dev = image_counts[0].device
    flat = torch.cat(image_counts)                                     # every image, state-major
    base = np.concatenate([[0], np.cumsum([c.numel() for c in image_counts])[:-1]]).astype(np.int64)
    img = torch.from_numpy(base[np.asarray(state_index, np.int64)] + np.asarray(local_index, np.int64)).to(dev)
    starts = torch.cumsum(flat, 0) - flat                              # each image's first entry in the concatenated pool
    cnt, first = flat[img], starts[img]
    within = torch.arange(total, dtype=torch.int64, device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt, output_size=total)
    return torch.repeat_interleave(first, cnt, output_size=total) + within, cnt


def _cut_words(state):
    """The meta words of all_gather_evaluator behind the existing ones: confusion flag, number of class score thresholds (0: none),
    CRC-32 of their fp32 bytes; a fixed length whatever the class count."""
    c = state.get('class_score_thresholds')
    return [int('confusion' in state), 0 if c is None else int(np.asarray(c).size),
            0 if c is None else zlib.crc32(np.asarray(c, np.float32).tobytes())]


def all_gather_evaluator(ev, group=None):
    """COLLECTIVE over ``group`` (default: the default process group): EVERY rank must call it, with its own evaluator,
    and every rank gets back the merged evaluator (``merge`` of the ranks' states in rank order, order='strided': rank r
    evaluated images r, r + W, ... of the global order).  Never call it from rank 0 alone: the other ranks would never
    join and rank 0 waits forever.  Sizes are gathered first, then the zero-padded pools, trimmed after.  Works on nccl
    (device tensors) and gloo (staged through host memory)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    st = ev.state()
    dev = ev.device if dist.get_backend(group) == 'nccl' else torch.device('cpu')

    def gather(t):
        out = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(out, t.contiguous(), group=group)
        return out

    thr = np.zeros(32, np.float32)
    T = st['iou_thresholds'].size
    thr[:T] = st['iou_thresholds']
    md = -1 if st['max_detections'] is None else st['max_detections']
    ranged = 'area_ranges' in st
    A = st['area_ranges'].shape[0] if ranged else 0
    rng = np.zeros((2, MAX_AREA_RANGES), np.float32)
    if ranged:
        rng[:, :A] = st['area_ranges'].T
    meta = torch.tensor([st['keys'].numel(), st['num_images'], st['num_classes'], md, T] + thr.view(np.int32).tolist() +
                        [A, int(st.get('curves', False))] + rng.reshape(-1).view(np.int32).tolist() + _cut_words(st),
                        dtype=torch.int64, device=dev)
    metas = [m.cpu().numpy() for m in gather(meta)]
    for r, m in enumerate(metas):                    # every rank sees every meta row: all raise together, before shapes diverge
        if not np.array_equal(m[2:55], metas[0][2:55]):
            raise ValueError('rank {} evaluates with classes / max_detections / thresholds {} and area ranges / curves {} against rank 0\'s {} '
                             'and {}'.format(r, m[2:5], m[37:39], metas[0][2:5], metas[0][37:39]))
        if not np.array_equal(m[55:], metas[0][55:]):
            raise ValueError('rank {} evaluates with confusion / class_score_thresholds (count, checksum) {} against rank 0\'s {}'.format(
                r, m[55:], metas[0][55:]))
    max_m = max(1, max(int(m[0]) for m in metas))
    max_n = max(1, max(int(m[1]) for m in metas))

    def padded(t, size):
        p = torch.zeros(size, dtype=t.dtype, device=dev)
        p[:t.numel()] = t.to(dev).reshape(-1)
        return p

    keys = gather(padded(st['keys'], max_m))
    W = max(A, 1)                                            # mask words per entry
    tp = gather(padded(st['tp'], max_m * W))
    counts = gather(padded(st['image_counts'], max_n))
    npos = gather(torch.from_numpy(st['npos']).to(dev))
    states = [{'keys': keys[r][:int(m[0])], 'tp': tp[r][:int(m[0]) * W], 'image_counts': counts[r][:int(m[1])], 'npos': npos[r].cpu().numpy(),
               'num_images': int(m[1]), 'iou_thresholds': st['iou_thresholds'], 'num_classes': st['num_classes'],
               'max_detections': st['max_detections']} for r, m in enumerate(metas)]
    if ranged:
        ign = gather(padded(st['ign'], max_m * W))
        npos_area = gather(torch.from_numpy(st['npos_area']).to(dev))
        for r, (s, m) in enumerate(zip(states, metas)):
            s.update(tp=s['tp'].reshape(-1, A), ign=ign[r][:int(m[0]) * A].reshape(-1, A), npos_area=npos_area[r].cpu().numpy(),
                     area_ranges=st['area_ranges'], area_names=st['area_names'], curves=st['curves'])
    if 'class_score_thresholds' in st:
        for s in states:
            s['class_score_thresholds'] = st['class_score_thresholds']
    if 'confusion' in st:
        for s, c in zip(states, gather(st['confusion'].to(dev))):
            s['confusion'] = c
    return DetectionEvaluator.merge(states, 'strided', device=ev.device)


# ---- the evaluation loop shared by evaluate.py and train.py --test_map -----------------------------------------------
def database_examples(path, num_shards=1, shard_index=0):
    """(name, HWC image, [G,5] X,Y,W,H,C) of the records keys[shard_index::num_shards] of an lmdb written by build_lmdb.py,
    in env.keys() order (= ImageReader.keys_flat); the records as stored, no augmentation, no image decode."""
    env = lmdbio.Environment(path)
    try:
        for i, key in enumerate(env.keys()):
            if i % num_shards != shard_index:
                continue
            img, boxes = ImageYoloBoxesPair().ParseFromString(env.get(key)).to_arrays()
            yield key.decode('ascii'), img, np.asarray(boxes).reshape(-1, 5)
    finally:
        env.close()


def evaluate_examples(yolo, examples, evaluator, min_box_size, batch_size, precision=None, nms='hard', nms_sigma=0.5, tta='none',
                      tta_vote_iou=None, tta_score='keep', letterbox=False):
    """Feeds (name, HWC image, [G,5] X,Y,W,H,C) examples through ``yolo`` (a YoloV3: per-image z-score -> predict ->
    clip -> small-box filter -> NMS, inference.py's path) into ``evaluator``, ``batch_size`` images per call, the short
    tail as one smaller call.  precision: predict()'s ('fp32' / 'bf16'; default yolo.inference_precision).  nms /
    nms_sigma: the NMS method (bbox_utils.NMS_METHODS) and its Gaussian parameter.  tta / tta_vote_iou / tta_score: test-time
    augmentation (bbox_utils.check_tta_args): the views of max(1, 16 // k) images per network call, each image's
    pooled and optionally voted detections matched as a device pool (add_pool with nms='none'); 'none' is the path above.
    letterbox: the images may differ in size; each is letterboxed into the model input on the device and its rows come back in its
    own pixels, clipped (YoloV3.predict_letterbox; at most 16 images per network call), where the ground truth is;
    not with tta.  Returns the number of images added."""
    if batch_size < 1:
        raise ValueError('batch_size must be >= 1')
    bbox_utils.check_nms_args(nms, nms_sigma)
    views = bbox_utils.check_tta_args(tta, tta_vote_iou, tta_score)
    if letterbox and tta != 'none':
        raise ValueError('letterbox does not go with tta')
    batch, count = [], 0

    def flush():
        imgs = [b[1] for b in batch]
        if letterbox:
            step = yolo.LETTERBOX_MAX_BATCH
            for s0 in range(0, len(batch), step):
                rows, _ = yolo.predict_letterbox(imgs[s0:s0 + step], precision=precision)
                evaluator.add_batch(rows, [b[2] for b in batch[s0:s0 + step]], min_box_size, clip_wh=None, nms=nms, nms_sigma=nms_sigma)
            batch.clear()
            return
        if any(im.shape != imgs[0].shape for im in imgs):
            raise RuntimeError('images must share one size (the model input is fixed): {}'.format({im.shape for im in imgs}))
        height, width = imgs[0].shape[:2]
        x = torch.from_numpy(np.stack([np.ascontiguousarray(im.astype(np.float32).transpose((2, 0, 1))) for im in imgs])).to(yolo.device)
        x = imagereader.zscore_normalize_device(x)
        if tta == 'none':
            rows = yolo.predict(x, precision=precision)
            evaluator.add_batch(rows, [b[2] for b in batch], min_box_size, clip_wh=(width, height), nms=nms, nms_sigma=nms_sigma)
        else:
            bbox_utils.check_tta_args(tta, tta_vote_iou, tta_score, (height, width))
            step = bbox_utils.tta_group_size(views)
            for s0 in range(0, len(batch), step):
                rows = yolo.predict_tta(x[s0:s0 + step], views, precision=precision)
                pools = bbox_utils.detect_tta_pools(rows, len(views), min_box_size, clip_wh=(width, height), method=nms, sigma=nms_sigma,
                                                    vote_iou=tta_vote_iou, score=tta_score)
                for (pool, m), ex in zip(pools, batch[s0:s0 + step]):
                    evaluator.add_pool(pool, m, ex[2], nms='none')        # re-establishes keep order under the final scores
        batch.clear()

    for ex in examples:
        batch.append(ex)
        count += 1
        if len(batch) == batch_size:
            flush()
    if batch:
        flush()
    return count
