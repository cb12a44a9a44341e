"""Host mirror of the reference's bbox_utils.py (NMS part on the GPU).

per_class_nms / filter_small_boxes keep the reference signatures
(bbox_utils.py:240-281) but run the class-wise NMS kernel (csrc/detect.hip);
``detect`` is the fused entry the CLIs use: clip -> small-box filter ->
class-wise NMS on device-resident ``[N, Nb, 5+K]`` rows, no host round trip
of the candidates.  CSV writers follow bbox_utils.py:47-62 and 284-300.
"""
import numpy as np
import torch

from ._hip import lib, check, HipError


# opt-in NMS variants (y3_nms_per_class_ex); 'hard' is the reference's greedy NMS and the default everywhere
NMS_METHODS = ('hard', 'diou', 'soft-linear', 'soft-gaussian')
_NMS_CODES = {'hard': 0, 'diou': 1, 'soft-linear': 2, 'soft-gaussian': 3}     # Y3_NMS_* (yolo3hip.h)


def check_nms_args(method, sigma=0.5, score_threshold=0.1):
    """Host-side validation of an NMS method and its parameters (the library checks them again): ValueError on an
    unknown method, soft-NMS with score_threshold <= 0 (nothing would ever drop), Gaussian soft-NMS with sigma <= 0."""
    if method not in _NMS_CODES:
        raise ValueError('nms method must be one of {}, got {!r}'.format(', '.join(NMS_METHODS), method))
    if method.startswith('soft') and not float(score_threshold) > 0:
        raise ValueError('{} needs score_threshold > 0, got {}'.format(method, score_threshold))
    if method == 'soft-gaussian' and not float(sigma) > 0:
        raise ValueError('soft-gaussian needs sigma > 0, got {}'.format(sigma))


class _NmsBuffers:
    def __init__(self, n, nb, k, device):
        self.key = (n, nb, k, str(device))
        self.keep_idx = torch.empty(n, k, nb, dtype=torch.int32, device=device)
        self.keep_cnt = torch.zeros(n, k, dtype=torch.int32, device=device)
        self.keep_score = torch.empty(n, k, nb, dtype=torch.float32, device=device)
        self.ws_bytes = int(lib.y3_nms_workspace_bytes(n, nb, k))          # >= every method's y3_nms_workspace_bytes_ex
        self.ws = torch.empty(self.ws_bytes // 4 + 4, dtype=torch.float32, device=device)


_cache = {}
_copy_streams = {}


def nms_device(rows, min_box_size=0.0, iou_threshold=0.3, score_threshold=0.1, clip_wh=None, private_outputs=False, method='hard',
               sigma=0.5):
    """rows: CUDA float32 [N, Nb, 5+K].  Returns (keep_idx[N,K,Nb] int32,
    keep_cnt[N,K] int32, keep_score[N,K,Nb]) device tensors; entries beyond
    keep_cnt are undefined.  The outputs are per-shape cached buffers that the next call overwrites unless
    private_outputs is set (the workspace is always shared: launches on one stream run in order).
    method: one of NMS_METHODS ('hard': y3_nms_per_class; the others: y3_nms_per_class_ex, whose keep_score holds the
    decayed scores of the soft methods); sigma: the Gaussian soft-NMS parameter."""
    check_nms_args(method, sigma, score_threshold)
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 3
    rows = rows.contiguous()
    n, nb, d = rows.shape
    k = d - 5
    st_obj = torch.cuda.current_stream(rows.device)
    key = (n, nb, k, str(rows.device), st_obj.cuda_stream)       # one workspace per stream: launches on a stream run in order
    buf = _cache.get(key)
    if buf is None:
        buf = _cache[key] = _NmsBuffers(n, nb, k, rows.device)
    if private_outputs:
        keep_idx, keep_cnt, keep_score = torch.empty_like(buf.keep_idx), torch.zeros_like(buf.keep_cnt), torch.empty_like(buf.keep_score)
    else:
        keep_idx, keep_cnt, keep_score = buf.keep_idx, buf.keep_cnt, buf.keep_score
    cw, chh = (float(clip_wh[0]), float(clip_wh[1])) if clip_wh is not None else (-1.0, -1.0)
    if method == 'hard':
        check(lib.y3_nms_per_class(rows.data_ptr(), n, nb, k, float(min_box_size), float(score_threshold), float(iou_threshold), cw, chh,
                                   keep_idx.data_ptr(), keep_cnt.data_ptr(), keep_score.data_ptr(), nb, buf.ws.data_ptr(),
                                   buf.ws_bytes, st_obj.cuda_stream), 'y3_nms_per_class')
    else:
        check(lib.y3_nms_per_class_ex(rows.data_ptr(), n, nb, k, _NMS_CODES[method], float(min_box_size), float(score_threshold),
                                      float(iou_threshold), float(sigma), cw, chh, keep_idx.data_ptr(), keep_cnt.data_ptr(),
                                      keep_score.data_ptr(), nb, buf.ws.data_ptr(), buf.ws_bytes, st_obj.cuda_stream), 'y3_nms_per_class_ex')
    return keep_idx, keep_cnt, keep_score


def check_class_thresholds(thresholds, num_classes):
    """A number (one cut for every class) or num_classes values -> float32 [num_classes].  Each is finite or -inf (no cut);
    ValueError on NaN, +inf, or another length."""
    try:
        thr = np.asarray(thresholds, np.float32)
    except (TypeError, ValueError):
        raise ValueError('class score thresholds: a number or {} numbers, got {!r}'.format(num_classes, thresholds))
    if thr.ndim == 0:
        thr = np.full(int(num_classes), thr, np.float32)
    if thr.ndim != 1 or thr.size != int(num_classes):
        raise ValueError('class score thresholds: a number or {} numbers, got shape {}'.format(num_classes, thr.shape))
    if np.any(np.isnan(thr)) or np.any(thr == np.inf):
        raise ValueError('class score thresholds must be finite or -inf, got {}'.format(thr.tolist()))
    return np.ascontiguousarray(thr)


def cut_keep_lists(keep_cnt, keep_score, class_thr_dev):
    """Per-class score cut on NMS keep lists, in place on the device (y3_keep_cut, current stream): keep_cnt int32 [..., K] and
    keep_score float32 [..., K, max_keep] as nms_device / nms_labelled_device return them, class_thr_dev CUDA float32 [K] (the
    values of check_class_thresholds).  Every count becomes the length of the longest prefix of its list with score >= the class's
    threshold; nothing else is written.  The caller owns keep_cnt: cut a copy of nms_device's cached buffer."""
    assert keep_cnt.is_cuda and keep_cnt.dtype == torch.int32 and keep_cnt.is_contiguous()
    assert keep_score.is_cuda and keep_score.dtype == torch.float32 and keep_score.is_contiguous()
    assert class_thr_dev.is_cuda and class_thr_dev.dtype == torch.float32 and class_thr_dev.is_contiguous() and class_thr_dev.dim() == 1
    k = class_thr_dev.numel()
    if keep_cnt.dim() < 1 or keep_cnt.shape[-1] != k or tuple(keep_score.shape[:-1]) != tuple(keep_cnt.shape):
        raise ValueError('keep_cnt {} / keep_score {} are not keep lists of {} classes'.format(tuple(keep_cnt.shape), tuple(keep_score.shape), k))
    check(lib.y3_keep_cut(keep_score.data_ptr(), keep_cnt.data_ptr(), keep_cnt.numel(), k, keep_score.shape[-1], class_thr_dev.data_ptr(),
                          torch.cuda.current_stream(keep_cnt.device).cuda_stream), 'y3_keep_cut')
    return keep_cnt


def filter_class_scores(dets, thr):
    """Host twin of cut_keep_lists for pipelines that end in host arrays.  dets: a list of per-image (boxes [M,4], score [M],
    label [M], keep [M]) tuples or (None,)*4 (``detect`` / ``detect_tta``), or one float [M, 6] array x0, y0, x1, y1, score, class
    (inference_image_tiled).  thr: check_class_thresholds' float32 [K].  Keeps the rows with np.float32(score) >=
    np.float32(thr[label]), in their order; an image left empty becomes (None,)*4."""
    thr = np.asarray(thr, np.float32).reshape(-1)
    if isinstance(dets, np.ndarray):
        if dets.ndim != 2 or dets.shape[1] != 6:
            raise ValueError('a detection array is [M, 6] = x0, y0, x1, y1, score, class, got shape {}'.format(dets.shape))
        return dets[dets[:, 4].astype(np.float32) >= thr[dets[:, 5].astype(np.int64)]]
    out = []
    for det in dets:
        if det[0] is None:
            out.append((None, None, None, None))
            continue
        keep = np.asarray(det[1]).astype(np.float32).reshape(-1) >= thr[np.asarray(det[2]).astype(np.int64).reshape(-1)]
        out.append(tuple(None if v is None else np.asarray(v)[keep] for v in det) if keep.any() else (None, None, None, None))
    return out


def detect_async(rows, min_box_size, iou_threshold=0.3, score_threshold=0.1, clip_wh=None, method='hard', sigma=0.5,
                 class_score_thresholds=None):
    """Enqueue clip -> small-box filter -> class-wise NMS for a batch and return a ``collect()`` callable; nothing
    synchronises until it is called, so the caller can queue the next batch's network first.  ``rows`` must stay
    untouched until then (pass a clone of a buffer that the next forward overwrites).  method / sigma: see nms_device.
    class_score_thresholds: a number or K values (check_class_thresholds); the keep lists are then cut per class on the device
    (cut_keep_lists) behind the NMS, before the counts are read."""
    keep_idx, keep_cnt, keep_score = nms_device(rows, min_box_size, iou_threshold, score_threshold, clip_wh, private_outputs=True,
                                                method=method, sigma=sigma)
    n, nb, d = rows.shape
    k = d - 5
    if class_score_thresholds is not None:
        cut_keep_lists(keep_cnt, keep_score, torch.from_numpy(check_class_thresholds(class_score_thresholds, k)).to(rows.device))
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(rows.device))

    def collect():
        # the copies run on a stream of their own behind the NMS's event: queued on the NMS's stream they would also
        # wait for whatever the caller has put on it since (the next batches of a tiled image)
        cs = _copy_streams.get(str(rows.device))
        if cs is None:
            cs = _copy_streams[str(rows.device)] = torch.cuda.Stream(device=rows.device)
        cs.wait_event(done)
        with torch.cuda.stream(cs):
            return _collect()

    def _collect():
        cnt = keep_cnt.cpu().numpy()                       # the only synchronisation point besides the final copies
        out = [(None, None, None, None)] * n
        total = int(cnt.sum())
        if total == 0:
            return out
        # flat (image, class, slot) positions of every kept entry, class-major inside an image like bbox_utils.py:252-263
        ii = np.repeat(np.arange(n), cnt.sum(1))
        cc = np.concatenate([np.repeat(np.arange(k), cnt[i]) for i in range(n)])
        jj = np.concatenate([np.arange(c) for c in cnt.reshape(-1)])
        lin = torch.from_numpy((ii * k + cc) * nb + jj).to(rows.device)
        idx = keep_idx.view(-1)[lin].long()
        boxes = rows[torch.from_numpy(ii).to(rows.device), idx, 0:4]
        if clip_wh is not None:
            boxes[:, 0::2] = boxes[:, 0::2].clamp(0, float(clip_wh[0]))
            boxes[:, 1::2] = boxes[:, 1::2].clamp(0, float(clip_wh[1]))
        boxes, sc, idx = boxes.cpu().numpy(), keep_score.view(-1)[lin].cpu().numpy(), idx.cpu().numpy().astype(np.int32)
        lab = cc.astype('int32')
        ends = np.cumsum(cnt.sum(1))
        for i in range(n):
            a, b = int(ends[i] - cnt[i].sum()), int(ends[i])
            if b > a:
                out[i] = (boxes[a:b], sc[a:b], lab[a:b], idx[a:b])
        return out
    return collect


# ---- tiled inference: the tiles' detections merged on the device (y3_tile_merge / y3_nms_labelled) ------------
MERGE_NMS_METHODS = ('none',) + NMS_METHODS
_MERGE_NMS_CODES = dict(_NMS_CODES, none=4)         # Y3_NMS_NONE
TILE_POOL_ROWS = 8192                               # first capacity of a pool; an image that needs more is merged again


def check_merge_args(merge_device='cpu', seam_margin=0.0, merge_nms='none', merge_nms_sigma=0.5, edge=96):
    """Host-side validation of the merge options of inference_image_tiled / evaluate.py --tiled: ValueError on an unknown
    device or method, a margin outside [0, edge), Gaussian sigma <= 0, and a margin or a merge NMS without the device merge
    (the host merge has neither)."""
    if merge_device not in ('cpu', 'gpu'):
        raise ValueError("merge_device must be 'cpu' or 'gpu', got {!r}".format(merge_device))
    if merge_nms not in MERGE_NMS_METHODS:
        raise ValueError('merge_nms must be one of {}, got {!r}'.format(', '.join(MERGE_NMS_METHODS), merge_nms))
    if not 0 <= float(seam_margin) < edge:
        raise ValueError('seam_margin must be in [0, {}), got {}'.format(edge, seam_margin))
    if merge_nms == 'soft-gaussian' and not float(merge_nms_sigma) > 0:
        raise ValueError('soft-gaussian needs merge_nms_sigma > 0, got {}'.format(merge_nms_sigma))
    if merge_device != 'gpu' and (float(seam_margin) != 0 or merge_nms != 'none'):
        raise ValueError("seam_margin and merge_nms need merge_device='gpu'")


class TilePool:
    """The whole-image detections of one tiled image on the device: rows float32 [cap, 6] = x0, y0, x1, y1, score, class and
    count int32 [2] = {rows written, rows needed}.  ``merge_tiles_device`` appends a batch of tiles; ``finish`` reads the
    count (the image's one host read) and merges the retained batches again if the pool was too small.  cap: the first
    capacity in rows (default TILE_POOL_ROWS).
    stream: the stream every merge of this pool runs on (default: the current one), so batches append in call order however
    their networks were scheduled."""

    def __init__(self, tile_size, img_size, margin=0.0, edge=96, cap=None, device=None, stream=None):
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.tile_size = (int(tile_size[0]), int(tile_size[1]))
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.margin, self.edge = float(margin), int(edge)
        self.stream = torch.cuda.current_stream(self.device) if stream is None else stream
        self.batches = []             # (rows, keep_idx, keep_cnt, keep_score, table slice, voted or None): kept for the retry and alive until finish
        self.ws = None
        self._alloc(max(1, int(TILE_POOL_ROWS if cap is None else cap)))

    def _alloc(self, cap):
        self.cap = cap
        self.rows = torch.empty(cap, 6, dtype=torch.float32, device=self.device)
        self.count = torch.zeros(2, dtype=torch.int32, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        if self.stream != cur:
            self.stream.wait_stream(cur)                  # the allocations and the zero fill above
            self.rows.record_stream(self.stream)
            self.count.record_stream(self.stream)

    def _launch(self, batch):
        rows, keep_idx, keep_cnt, keep_score, table, voted = batch
        n, nb, ld = rows.shape
        k, max_keep = keep_idx.shape[1], keep_idx.shape[2]
        ws_bytes = int(lib.y3_tile_merge_workspace_bytes(n, k))
        if self.ws is None or self.ws.numel() * 4 < ws_bytes:
            with torch.cuda.stream(self.stream):          # a larger one replaces it behind the launches that use the old one
                self.ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.int32, device=self.device)
        if voted is not None:         # the boxes and scores of box voting instead of rows[keep_idx] and keep_score (tile TTA)
            check(lib.y3_tile_merge_voted(voted.data_ptr(), n, nb, k, keep_idx.data_ptr(), keep_cnt.data_ptr(), max_keep, table.data_ptr(),
                                          self.tile_size[0], self.tile_size[1], self.img_size[0], self.img_size[1], self.edge, self.margin,
                                          self.rows.data_ptr(), self.cap, self.count.data_ptr(), self.ws.data_ptr(), self.ws.numel() * 4,
                                          self.stream.cuda_stream), 'y3_tile_merge_voted')
            return
        check(lib.y3_tile_merge(rows.data_ptr(), n, nb, ld, k, keep_idx.data_ptr(), keep_cnt.data_ptr(), keep_score.data_ptr(), max_keep,
                                table.data_ptr(), self.tile_size[0], self.tile_size[1], self.img_size[0], self.img_size[1], self.edge,
                                self.margin, self.rows.data_ptr(), self.cap, self.count.data_ptr(), self.ws.data_ptr(), self.ws.numel() * 4,
                                self.stream.cuda_stream), 'y3_tile_merge')

    def finish(self):
        """-> (rows [M, 6] device view of the pool, M).  Synchronises with the merge stream and reads the count."""
        cur = torch.cuda.current_stream(self.device)
        if self.stream != cur:
            cur.wait_stream(self.stream)
        need = int(self.count[1].item())
        if need >= 2 ** 31 - 1:
            raise HipError('y3_tile_merge: the detections of one image do not fit an int32 count')
        if need > self.cap:                               # nothing was written past cap; the counts were: merge again, all of it
            # on the current stream: the batch tensors and the workspace were allocated on the slot streams and the merge stream, so
            # they are recorded on this one before its launches use them (they may be freed while those are still pending)
            self.stream = cur
            for t in [t for batch in self.batches for t in batch if t is not None] + ([self.ws] if self.ws is not None else []):
                t.record_stream(cur)
            self._alloc(need)
            for batch in self.batches:
                self._launch(batch)
        self.batches = []
        return self.rows[:need], need


def merge_tiles_device(pool, rows, keep_idx, keep_cnt, keep_score, table_dev, done=None, voted=None):
    """Append one batch of tiles to ``pool`` (y3_tile_merge): rows CUDA float32 [n, Nb, 5+K] and nms_device(...,
    private_outputs=True)'s outputs for them, table_dev int32 [n, 6] = this batch's rows of the device tile table.
    done: an event recorded behind the batch's NMS; the pool's stream waits for it.  Nothing is read back.
    voted: vote_device(..., private_output=True)'s [n, K, max_keep, 6] for the batch; the kept entries then take their boxes and
    scores from it (y3_tile_merge_voted), and the pool retains it for its retry."""
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 3 and rows.is_contiguous()
    assert table_dev.dtype == torch.int32 and table_dev.is_contiguous() and table_dev.shape == (rows.shape[0], 6)
    assert keep_idx.shape[0] == rows.shape[0] and keep_cnt.shape == keep_idx.shape[:2] and keep_score.shape == keep_idx.shape
    if done is not None:
        pool.stream.wait_event(done)
    if voted is not None:
        assert voted.is_cuda and voted.dtype == torch.float32 and voted.is_contiguous() and tuple(voted.shape) == tuple(keep_idx.shape) + (6,)
    batch = (rows, keep_idx, keep_cnt, keep_score, table_dev, voted)
    for t in batch:
        if t is not None:
            t.record_stream(pool.stream)
    pool.batches.append(batch)
    pool._launch(batch)


def nms_labelled_device(pool_rows, num_classes, method='hard', iou_threshold=0.3, score_threshold=0.1, sigma=0.5):
    """Class-wise NMS over pool rows CUDA float32 [M, 6] = x0, y0, x1, y1, score, class (y3_nms_labelled) on the current
    stream.  method: 'none' (every row, in keep order: score descending, ties: higher row first) or one of NMS_METHODS;
    hard / diou / none take every row of a class as a candidate, the soft methods those with score >= score_threshold and
    return decayed scores.  Returns device (keep_idx [K, max(M, 1)] int32 pool rows, keep_cnt [K], keep_score)."""
    if method not in _MERGE_NMS_CODES:
        raise ValueError('merge nms method must be one of {}, got {!r}'.format(', '.join(MERGE_NMS_METHODS), method))
    if method != 'none':
        check_nms_args(method, sigma, score_threshold)
    assert pool_rows.is_cuda and pool_rows.dtype == torch.float32 and pool_rows.dim() == 2 and pool_rows.shape[1] == 6
    pool_rows = pool_rows.contiguous()
    m, k, dev = pool_rows.shape[0], int(num_classes), pool_rows.device
    keep_idx = torch.empty(k, max(m, 1), dtype=torch.int32, device=dev)
    keep_cnt = torch.zeros(k, dtype=torch.int32, device=dev)
    keep_score = torch.empty(k, max(m, 1), dtype=torch.float32, device=dev)
    if m == 0:
        return keep_idx, keep_cnt, keep_score
    code = _MERGE_NMS_CODES[method]
    ws_bytes = int(lib.y3_nms_workspace_bytes_ex(1, m, k, code))
    ws = torch.empty(ws_bytes // 4 + 4, dtype=torch.float32, device=dev)
    thr = float(score_threshold) if method.startswith('soft') else -np.inf
    check(lib.y3_nms_labelled(pool_rows.data_ptr(), m, k, code, thr, float(iou_threshold), float(sigma), keep_idx.data_ptr(),
                              keep_cnt.data_ptr(), keep_score.data_ptr(), m, ws.data_ptr(), ws_bytes,
                              torch.cuda.current_stream(dev).cuda_stream), 'y3_nms_labelled')
    return keep_idx, keep_cnt, keep_score


def gather_kept(pool_rows, keep_idx, keep_cnt, keep_score):
    """The kept rows of nms_labelled_device as a new pool [M', 6] on the device: class-major, keep order inside a class,
    column 4 = keep_score (the decayed score of the soft methods).  Reads the K keep counts."""
    cnt = keep_cnt.cpu().numpy().astype(np.int64)
    k, width = keep_idx.shape
    if int(cnt.sum()) == 0:
        return pool_rows[:0].clone()
    lin = np.concatenate([c * width + np.arange(cnt[c]) for c in range(k)])
    lin = torch.from_numpy(lin).to(pool_rows.device)
    out = pool_rows[keep_idx.view(-1)[lin].long()]        # a copy
    out[:, 4] = keep_score.view(-1)[lin]
    return out


def detect(rows, min_box_size, iou_threshold=0.3, score_threshold=0.1, clip_wh=None, method='hard', sigma=0.5, class_score_thresholds=None):
    """inference.py:62-79 for a batch: returns, per image, (boxes[M,4], score[M],
    label[M] int32, keep[M] row indices) as NumPy arrays, or (None,)*4.  method / sigma: see nms_device;
    class_score_thresholds: see detect_async."""
    return detect_async(rows, min_box_size, iou_threshold, score_threshold, clip_wh, method, sigma, class_score_thresholds)()


# ---- test-time augmentation: pooled views, box voting (y3_box_vote) -------------------------------------------
# a view is a 3-bit code: 4 = transpose (applied first), 1 = flip x, 2 = flip y (Y3_TTA_*, yolo3hip.h); 0 is the identity
TTA_VIEWS = {'none': (0,), 'hflip': (0, 1), 'flips': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}
TTA_SCORES = ('keep', 'consensus')
_VOTE_SCORE_CODES = {'keep': 0, 'consensus': 1}      # Y3_VOTE_SCORE_*
TTA_MAX_BATCH = 16                                   # images x views per network call (YoloV3.TTA_MAX_BATCH)


def check_tta_args(tta='none', vote_iou=None, score='keep', img_size=None):
    """Host-side validation of the test-time augmentation options: ValueError on an unknown view set, a transposing set
    ('d4') on a non-square input (img_size = (H, W), when known), vote_iou outside (0, 1] (None: no voting) and a consensus
    score without voting (there would be no member sets to count).  Returns the set's view codes."""
    if tta not in TTA_VIEWS:
        raise ValueError('tta must be one of {}, got {!r}'.format(', '.join(TTA_VIEWS), tta))
    if score not in TTA_SCORES:
        raise ValueError('tta score must be one of {}, got {!r}'.format(', '.join(TTA_SCORES), score))
    views = TTA_VIEWS[tta]
    if img_size is not None and int(img_size[0]) != int(img_size[1]) and any(v & 4 for v in views):
        raise ValueError('tta {!r} transposes the image, which needs a square input, got {} x {}'.format(tta, int(img_size[0]), int(img_size[1])))
    if vote_iou is not None and not 0 < float(vote_iou) <= 1:
        raise ValueError('tta vote_iou must be in (0, 1], got {}'.format(vote_iou))
    if score == 'consensus' and vote_iou is None:
        raise ValueError('a consensus score needs box voting (give a vote_iou)')
    return views


def tta_group_size(views):
    """Images per network call under test-time augmentation: as many as keep images x views within TTA_MAX_BATCH."""
    return max(1, TTA_MAX_BATCH // len(views))


_vote_cache = {}


def vote_device(rows, keep_idx, keep_cnt, keep_score, views, vote_iou, min_box_size=0.0, score_threshold=0.1, clip_wh=None, score='keep',
                private_output=False):
    """Box voting (y3_box_vote) on the current stream.  rows: CUDA float32 [N, k * Nb, 5+K], the unmapped rows of k = ``views``
    views per image (YoloV3.predict_tta); keep_idx / keep_cnt / keep_score: nms_device's outputs for them; min_box_size,
    score_threshold, clip_wh: what nms_device got.  Returns out [N, K, max_keep, 6] = x0, y0, x1, y1, score, class on the
    device, valid for j < keep_cnt; the rest is uninitialised.  Like nms_device's outputs, out and the workspace are buffers
    cached per shape and stream: the next call of that shape overwrites out unless private_output is set."""
    if score not in _VOTE_SCORE_CODES:
        raise ValueError('tta score must be one of {}, got {!r}'.format(', '.join(TTA_SCORES), score))
    if not 0 < float(vote_iou) <= 1:
        raise ValueError('tta vote_iou must be in (0, 1], got {}'.format(vote_iou))
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 3 and rows.is_contiguous()
    n, nb, d = rows.shape
    k, max_keep, views = d - 5, keep_idx.shape[2], int(views)
    assert keep_idx.shape[:2] == (n, k) and keep_cnt.shape == (n, k) and keep_score.shape == keep_idx.shape
    assert keep_idx.is_contiguous() and keep_cnt.is_contiguous() and keep_score.is_contiguous()
    if views < 1 or nb % views:
        raise ValueError('{} rows per image are not {} views of equal length'.format(nb, views))
    st_obj = torch.cuda.current_stream(rows.device)
    key = (n, nb, k, max_keep, str(rows.device), st_obj.cuda_stream)      # one workspace per stream: launches on a stream run in order
    buf = _vote_cache.get(key)
    if buf is None:
        ws_bytes = int(lib.y3_box_vote_workspace_bytes(n, nb, k))
        buf = _vote_cache[key] = (torch.empty(n, k, max_keep, 6, dtype=torch.float32, device=rows.device), ws_bytes,
                                  torch.empty(ws_bytes // 4 + 1, dtype=torch.float32, device=rows.device))
    out, ws_bytes, ws = buf
    if private_output:
        out = torch.empty_like(out)
    cw, chh = (float(clip_wh[0]), float(clip_wh[1])) if clip_wh is not None else (-1.0, -1.0)
    check(lib.y3_box_vote(rows.data_ptr(), n, nb, k, keep_idx.data_ptr(), keep_cnt.data_ptr(), keep_score.data_ptr(), max_keep,
                          float(min_box_size), float(score_threshold), cw, chh, float(vote_iou), views, nb // views, _VOTE_SCORE_CODES[score],
                          out.data_ptr(), ws.data_ptr(), ws_bytes, st_obj.cuda_stream), 'y3_box_vote')
    return out


def detect_tta_pools(rows, views, min_box_size, iou_threshold=0.3, score_threshold=0.1, clip_wh=None, method='hard', sigma=0.5,
                     vote_iou=None, score='keep', with_rows=False):
    """The detections of the pooled views, left on the device.  rows: CUDA float32 [N, k * Nb, 5+K] from YoloV3.predict_tta
    with k = ``views`` views.  The pooled rows of an image go through the chosen NMS (nms_device) as one image's rows; with
    vote_iou every kept box is then replaced by the vote of its members (vote_device) and, with score='consensus', its score
    by the mean over the views of the best member score.  Returns one (pool [M, 6] = x0, y0, x1, y1, score, class, M) per
    image, class-major and in keep order inside a class (DetectionEvaluator.add_pool's input); with_rows: also the [M] kept row
    indices.  Without vote_iou the pool holds what ``detect`` returns for the same rows.  Reads the keep counts: one
    synchronisation; the gathers that follow are indexed by positions computed from them on the host."""
    rows = rows.contiguous()
    n, nb, d = rows.shape
    k = d - 5
    keep_idx, keep_cnt, keep_score = nms_device(rows, min_box_size, iou_threshold, score_threshold, clip_wh, private_outputs=True,
                                                method=method, sigma=sigma)
    if vote_iou is not None:
        out = vote_device(rows, keep_idx, keep_cnt, keep_score, views, vote_iou, min_box_size, score_threshold, clip_wh, score)
    else:
        if score != 'keep':
            raise ValueError('a consensus score needs box voting (give a vote_iou)')
        out = None
    return _tta_pools(rows, (keep_idx, keep_cnt, keep_score), out, clip_wh, with_rows)


def _tta_pools(rows, keep, out, clip_wh, with_rows):
    """detect_tta_pools behind its launches: the keep lists (and the voted array, or None) of rows -> the per-image pools."""
    keep_idx, keep_cnt, keep_score = keep
    n, k = keep_cnt.shape
    cnt = keep_cnt.cpu().numpy().astype(np.int64)                       # the one host read: everything below is sized from it
    per_image = cnt.sum(1)
    max_keep = keep_idx.shape[2]
    # flat (image, class, slot) positions of every kept entry, class-major inside an image, as detect_async's collect builds them
    ii = np.repeat(np.arange(n), per_image)
    cc = np.concatenate([np.repeat(np.arange(k), cnt[i]) for i in range(n)])
    jj = np.concatenate([np.arange(c) for c in cnt.reshape(-1)])
    lin = torch.from_numpy((ii * k + cc) * max_keep + jj).to(rows.device)
    kept = keep_idx.view(-1)[lin].long()
    if out is not None:
        flat = out.view(-1, 6)[lin]                                     # a copy: the cached out may be overwritten after this
    else:
        boxes = rows[torch.from_numpy(ii).to(rows.device), kept, 0:4]
        if clip_wh is not None:
            boxes[:, 0::2] = boxes[:, 0::2].clamp(0, float(clip_wh[0]))
            boxes[:, 1::2] = boxes[:, 1::2].clamp(0, float(clip_wh[1]))
        flat = torch.cat([boxes, keep_score.view(-1)[lin][:, None], torch.from_numpy(cc.astype(np.float32)).to(rows.device)[:, None]], dim=1)
    ends = np.cumsum(per_image)
    pools = []
    for i in range(n):
        a, b = int(ends[i] - per_image[i]), int(ends[i])
        pools.append((flat[a:b], b - a, kept[a:b]) if with_rows else (flat[a:b], b - a))
    return pools


def detect_tta_async(rows, views, min_box_size, iou_threshold=0.3, score_threshold=0.1, clip_wh=None, method='hard', sigma=0.5, vote_iou=None,
                     score='keep'):
    """detect_async for the pooled views: enqueues the NMS (and, with vote_iou, the box voting) of detect_tta_pools on the current
    stream and returns a ``collect()`` callable that gives what detect_tta returns for the same rows; nothing synchronises until
    it is called.  ``rows`` must stay untouched until then.  Every output is private to the call, so any number may be pending."""
    rows = rows.contiguous()
    keep = nms_device(rows, min_box_size, iou_threshold, score_threshold, clip_wh, private_outputs=True, method=method, sigma=sigma)
    if vote_iou is not None:
        out = vote_device(rows, *keep, views, vote_iou, min_box_size, score_threshold, clip_wh, score, private_output=True)
    else:
        if score != 'keep':
            raise ValueError('a consensus score needs box voting (give a vote_iou)')
        out = None
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(rows.device))

    def collect():
        cs = _copy_streams.get(str(rows.device))        # behind the event, not behind what the caller has queued since: detect_async
        if cs is None:
            cs = _copy_streams[str(rows.device)] = torch.cuda.Stream(device=rows.device)
        cs.wait_event(done)
        with torch.cuda.stream(cs):
            return _tta_host(_tta_pools(rows, keep, out, clip_wh, True))
    return collect


def detect_tta(rows, views, min_box_size, iou_threshold=0.3, score_threshold=0.1, clip_wh=None, method='hard', sigma=0.5, vote_iou=None,
               score='keep'):
    """``detect`` for the pooled views of YoloV3.predict_tta (see detect_tta_pools): per image (boxes [M,4], score [M],
    label [M] int32, keep [M] row indices into the image's k * Nb rows) as NumPy arrays, or (None,)*4."""
    return _tta_host(detect_tta_pools(rows, views, min_box_size, iou_threshold, score_threshold, clip_wh, method, sigma, vote_iou, score,
                                      with_rows=True))


def _tta_host(pools):
    """Pools with their kept rows -> detect's per-image tuples."""
    out = []
    for pool, m, kept in pools:
        if m == 0:
            out.append((None, None, None, None))
            continue
        p = pool.cpu().numpy()
        out.append((np.ascontiguousarray(p[:, 0:4]), np.ascontiguousarray(p[:, 4]), p[:, 5].astype(np.int32), kept.cpu().numpy().astype(np.int32)))
    return out


def per_class_nms(boxes, objectness, class_probs, iou_threshold=0.3, score_threshold=0.1):
    """bbox_utils.py:240-271 (same signature and (None, None, None) convention)."""
    boxes = np.asarray(boxes, np.float32)
    rows = np.concatenate([boxes, np.asarray(objectness, np.float32).reshape(-1, 1), np.asarray(class_probs, np.float32)], axis=1)
    if rows.shape[0] == 0:
        return None, None, None
    r = torch.from_numpy(rows).cuda()[None]
    b, s, l, _ = detect(r, -np.inf, iou_threshold, score_threshold)[0]
    return b, s, l


def single_class_nms(boxes, scores, iou_threshold):
    """bbox_utils.py:217-237: keep indices (selection order) into ``boxes``."""
    boxes = np.asarray(boxes, np.float32)
    scores = np.asarray(scores, np.float32).reshape(-1, 1)
    m = boxes.shape[0]
    if m == 0:
        return []
    rows = torch.from_numpy(np.ascontiguousarray(np.concatenate([boxes, scores], axis=1))).cuda()
    keep_idx = torch.empty(m, dtype=torch.int32, device=rows.device)
    keep_cnt = torch.zeros(1, dtype=torch.int32, device=rows.device)
    keep_score = torch.empty(m, dtype=torch.float32, device=rows.device)
    ws_bytes = int(lib.y3_nms_workspace_bytes(1, m, 1))
    ws = torch.empty(ws_bytes // 4 + 4, dtype=torch.float32, device=rows.device)
    st = torch.cuda.current_stream(rows.device).cuda_stream
    check(lib.y3_nms_single_class(rows.data_ptr(), m, float(iou_threshold), keep_idx.data_ptr(), keep_cnt.data_ptr(), keep_score.data_ptr(),
                                  ws.data_ptr(), ws_bytes, st), 'y3_nms_single_class')
    return [int(v) for v in keep_idx[:int(keep_cnt.item())].cpu().numpy()]


def compute_iou(box, boxes, box_area=None, boxes_area=None):
    """bbox_utils.py:200-214: IoU of one corner box [4] against boxes [M,4] (no +1) on the GPU, float32 in the
    reference's operation order -> ndarray [M].  box_area / boxes_area are accepted for signature compatibility; the
    reference only ever passes the areas of these same boxes (bbox_utils.py:232), which the kernel recomputes."""
    boxes = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 4))
    if boxes.shape[0] == 0:
        return np.zeros((0,), np.float32)
    b = torch.from_numpy(np.ascontiguousarray(np.asarray(box, np.float32).reshape(4))).cuda()
    bb = torch.from_numpy(boxes).cuda()
    out = torch.empty(boxes.shape[0], dtype=torch.float32, device=bb.device)
    check(lib.y3_compute_iou(b.data_ptr(), bb.data_ptr(), boxes.shape[0], 4, out.data_ptr(), torch.cuda.current_stream(bb.device).cuda_stream),
          'y3_compute_iou')
    return out.cpu().numpy()


def filter_small_boxes(boxes, min_size):
    """bbox_utils.py:274-281: rows [M, >=4] = x0, y0, x1, y1, ... -> the rows with width AND height strictly greater
    than min_size, original order.  The selection runs on the GPU (y3_filter_small_boxes); the CLIs use the path fused
    into the NMS launch (``detect``) instead."""
    boxes = np.asarray(boxes)
    if boxes.shape[0] == 0:
        return boxes
    rows = torch.from_numpy(np.ascontiguousarray(boxes[:, :4], dtype=np.float32)).cuda()
    idx = torch.empty(rows.shape[0], dtype=torch.int32, device=rows.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=rows.device)
    check(lib.y3_filter_small_boxes(rows.data_ptr(), rows.shape[0], 4, float(min_size), idx.data_ptr(), cnt.data_ptr(),
                                    torch.cuda.current_stream(rows.device).cuda_stream), 'y3_filter_small_boxes')
    return boxes[idx[:int(cnt.item())].cpu().numpy().astype(np.int64), :]


def load_boxes_to_xywhc(filepath):
    """bbox_utils.py:106-124: CSV with header X,Y,W,H,C (skipinitialspace) -> float [n,5]; missing file -> [0,5]."""
    import csv
    import os
    rows = []
    if os.path.exists(filepath):
        with open(filepath) as fh:
            for row in csv.DictReader(fh, skipinitialspace=True):
                rows.append([int(row['X']), int(row['Y']), int(row['W']), int(row['H']), int(row['C'])])
    return np.asarray(rows, dtype=np.float64).reshape(-1, 5)


def load_boxes_to_ltrbc(filepath):
    """bbox_utils.py:83-103: as above with W,H converted to inclusive right / bottom."""
    a = load_boxes_to_xywhc(filepath)
    a[:, 2] = a[:, 0] + a[:, 2] - 1
    a[:, 3] = a[:, 1] + a[:, 3] - 1
    return a


def write_boxes_from_xywhc(boxes, csv_filename):
    """bbox_utils.py:47-62."""
    with open(csv_filename, 'w') as fh:
        fh.write('X,Y,W,H,C\n')
        for k in range(boxes.shape[0]):
            fh.write('{:d},{:d},{:d},{:d},{:d}\n'.format(int(boxes[k, 0]), int(boxes[k, 1]), int(boxes[k, 2]), int(boxes[k, 3]), int(boxes[k, 4])))


def write_boxes_from_ltrbc(boxes, csv_filename):
    """bbox_utils.py:65-80: [left, top, right, bottom, class] -> X,Y,W,H,C with W = right - left + 1."""
    with open(csv_filename, 'w') as fh:
        fh.write('X,Y,W,H,C\n')
        for k in range(boxes.shape[0]):
            x, y = boxes[k, 0], boxes[k, 1]
            fh.write('{:d},{:d},{:d},{:d},{:d}\n'.format(x, y, boxes[k, 2] - x + 1, boxes[k, 3] - y + 1, boxes[k, 4]))


def write_boxes_from_ltrbpc(boxes, csv_filename):
    """bbox_utils.py:284-300: W = x2 - x + 1."""
    with open(csv_filename, 'w') as fh:
        fh.write('X,Y,W,H,P,C\n')
        for k in range(boxes.shape[0]):
            x = int(boxes[k, 0])
            y = int(boxes[k, 1])
            w = int(boxes[k, 2] - x + 1)
            h = int(boxes[k, 3] - y + 1)
            fh.write('{:d},{:d},{:d},{:d},{:f},{:d}\n'.format(x, y, w, h, boxes[k, 4], int(boxes[k, 5])))
