"""Anchors fitted to a dataset (not in the reference, whose find_anchor_sizes.py clusters (H, W) by Euclidean distance).

The criterion that assigns a box to an anchor is the IoU of the co-centred sizes (imagereader.format_boxes, y3_format_labels), so
the anchors are fitted to that criterion: IoU k-means (Lloyd steps on the IoU assignment) followed by a mutation search.  The one hot
loop -- n boxes x P candidate sets x k anchors -- is y3_anchor_stats (csrc/anchors.hip) or its NumPy restatement below; the score of
a box is the INTEGER q = rint(iou * 2^24), so every sum is exact, independent of order, and identical on both devices: all the
host arithmetic of fit_anchors is shared, and `cpu` and `gpu` return the same bytes.

Sizes are (w, h) throughout, as the anchors of YoloV3 and train.py are; find_anchor_sizes.load_sizes keeps the reference's (H, W)."""
import json
import math
import os

import numpy as np

Q_ONE = 1 << 24          # q of IoU 1
MAX_ANCHORS = 16         # Y3_MAX_ANCHORS
MAX_CANDIDATES = 1024    # Y3_ANCHOR_MAX_CANDIDATES: P * k of one call
MAX_SIDE = 65535         # a box with w or h outside [1, MAX_SIDE] is skipped
_CPU_CHUNK = 1 << 18     # IoUs of one NumPy chunk (temporaries that stay in cache)


def kmeans(X, k, rng, n_init=10, max_iter=300, tol=1e-4):
    """-> (centers [k,2], labels [n], inertia).  k-means++ init, Lloyd, best of n_init.  (Euclidean: find_anchor_sizes.py's default
    metric, which mirrors the reference's sklearn KMeans; fit_anchors puts its centres into the start pool.)"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    if n < k:
        raise ValueError('need at least %d boxes for %d clusters, got %d' % (k, k, n))
    best = None
    scale = tol * float(np.mean(np.var(X, axis=0))) if n > 1 else 0.0       # sklearn's tolerance scaling
    for _ in range(n_init):
        centers = np.empty((k, X.shape[1]))
        centers[0] = X[rng.integers(n)]
        d2 = ((X - centers[0]) ** 2).sum(1)
        for j in range(1, k):
            tot = d2.sum()
            idx = rng.integers(n) if tot <= 0 else int(np.searchsorted(np.cumsum(d2), rng.random() * tot))
            centers[j] = X[min(idx, n - 1)]
            d2 = np.minimum(d2, ((X - centers[j]) ** 2).sum(1))
        for _ in range(max_iter):
            dist = ((X[:, None, :] - centers[None, :, :]) ** 2).sum(2)
            labels = dist.argmin(1)
            new = centers.copy()
            for j in range(k):
                m = labels == j
                if m.any():
                    new[j] = X[m].mean(0)
            shift = float(((new - centers) ** 2).sum())
            centers = new
            if shift <= scale:
                break
        dist = ((X[:, None, :] - centers[None, :, :]) ** 2).sum(2)
        labels = dist.argmin(1)
        inertia = float(dist[np.arange(n), labels].sum())
        if best is None or inertia < best[2]:
            best = (centers, labels, inertia)
    return best


def thr_to_q(thr):
    """The IoU threshold on the q scale: rint(thr * 2^24), which must land in [0, 2^24]."""
    thr = float(thr)
    if not (0.0 <= thr <= 1.0):
        raise ValueError('the IoU threshold must lie in [0, 1], got {!r}'.format(thr))
    return int(np.rint(thr * Q_ONE))


def _as_sizes(wh):
    wh = np.asarray(wh)
    if wh.ndim != 2 or wh.shape[1] != 2:
        raise ValueError('sizes must be [n, 2] = (w, h), got shape {}'.format(wh.shape))
    if wh.shape[0] < 1 or wh.shape[0] > 2 ** 31 - 1:
        raise ValueError('need between 1 and 2^31 - 1 boxes, got {}'.format(wh.shape[0]))
    if wh.dtype.kind not in 'iu':
        raise ValueError('sizes must be integers (pixels), got dtype {}'.format(wh.dtype))
    # (an int32 that wrapped would pass for a valid size: sizes outside int32 become 0, which is skipped like them)
    wide = wh.astype(np.int64)
    return np.ascontiguousarray(np.where((wide < -2 ** 31) | (wide >= 2 ** 31), 0, wide).astype(np.int32))


def _as_candidates(cands):
    c = np.asarray(cands, dtype=np.float32)
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or c.shape[2] != 2:
        raise ValueError('candidates must be [P, k, 2] or [k, 2] = (w, h), got shape {}'.format(c.shape))
    P, k = c.shape[:2]
    if not 1 <= k <= MAX_ANCHORS:
        raise ValueError('k = {} outside 1..{}'.format(k, MAX_ANCHORS))
    if P < 1 or P * k > MAX_CANDIDATES:
        raise ValueError('P = {} sets of {} anchors: P * k must lie in 1..{}'.format(P, k, MAX_CANDIDATES))
    if not (np.isfinite(c).all() and (c > 0).all()):
        raise ValueError('anchor sizes must be positive and finite')
    return np.ascontiguousarray(c)


def iou_f32(wh, anchors):
    """float32 IoU of every box against every anchor, co-centred: wh [n, 2] x anchors [..., 2] -> [n, ...].  format_boxes' float32
    expression, step by step (y3_anchor_stats evaluates the same)."""
    wh = np.asarray(wh).astype(np.float32)
    a = np.asarray(anchors, dtype=np.float32)
    shape = (wh.shape[0],) + (1,) * (a.ndim - 1)
    w, h = wh[:, 0].reshape(shape), wh[:, 1].reshape(shape)
    aw, ah = a[..., 0][None], a[..., 1][None]
    iw = np.maximum(np.minimum(w / 2.0, aw / 2.0) - np.maximum(-w / 2.0, -aw / 2.0), np.float32(0.0))
    ih = np.maximum(np.minimum(h / 2.0, ah / 2.0) - np.maximum(-h / 2.0, -ah / 2.0), np.float32(0.0))
    inter = iw * ih
    iou = inter / (w * h + aw * ah - inter)
    assert iou.dtype == np.float32
    return iou


def _q(iou):
    return np.rint(iou * np.float32(Q_ONE)).astype(np.int32)


def iou_q(wh, anchors):
    """q = rint(iou_f32 * 2^24) (int32, to nearest even; the product by 2^24 is exact in float32), in [0, 2^24]."""
    return _q(iou_f32(wh, anchors))


class _Stats:
    """One set of box sizes, scored against candidate sets again and again: on the host, or resident on the device."""

    def __init__(self, wh, device):
        if device not in ('cpu', 'gpu'):
            raise ValueError("device must be 'cpu' or 'gpu', got {!r}".format(device))
        self.device = device
        self.wh = _as_sizes(wh)
        self.n = self.wh.shape[0]
        if device == 'cpu':
            self.valid = ((self.wh >= 1) & (self.wh <= MAX_SIDE)).all(axis=1)
            self.kept = self.wh if self.valid.all() else self.wh[self.valid]
        else:
            import torch
            self.wh_dev = torch.from_numpy(self.wh).cuda()
            self.ws = None

    def __call__(self, cands, thr_q, per_anchor, labels=False):
        """-> (stats int64 [P, k, 5] or [P, 2], skipped, labels uint8 [n] or None)."""
        c = _as_candidates(cands)
        thr_q = int(thr_q)
        if not 0 <= thr_q <= Q_ONE:
            raise ValueError('thr_q {} outside 0..2^24'.format(thr_q))
        if labels and c.shape[0] != 1:
            raise ValueError('labels need one candidate set, got {}'.format(c.shape[0]))
        return (self._cpu if self.device == 'cpu' else self._gpu)(c, thr_q, bool(per_anchor), bool(labels))

    def _cpu(self, c, thr_q, per_anchor, labels):
        P, k = c.shape[:2]
        out = np.zeros((P * k, 5) if per_anchor else (P, 2), np.int64)
        lab = np.full(self.n, 255, np.uint8) if labels else None
        kept_lab = np.empty(self.kept.shape[0], np.uint8) if labels else None
        rows = max(1, _CPU_CHUNK // (P * k))
        slot = (np.arange(P) * k)[None]
        for i0 in range(0, self.kept.shape[0], rows):
            wh = self.kept[i0:i0 + rows]
            iou = iou_f32(wh, c)                                        # [r, P, k]
            best = iou.argmax(axis=2)                                   # first maximum of the IoU itself, not of q
            qb = _q(np.take_along_axis(iou, best[..., None], axis=2)[..., 0])
            hit = qb >= thr_q
            if per_anchor:
                idx = (best + slot).ravel()
                m = P * k
                out[:, 0] += np.bincount(idx, minlength=m)
                # float64 weights: a chunk's sums stay below 2^18 * 2^24, exact
                out[:, 1] += np.bincount(idx, weights=np.repeat(wh[:, 0].astype(np.float64), P), minlength=m).astype(np.int64)
                out[:, 2] += np.bincount(idx, weights=np.repeat(wh[:, 1].astype(np.float64), P), minlength=m).astype(np.int64)
                out[:, 3] += np.bincount(idx, weights=qb.ravel().astype(np.float64), minlength=m).astype(np.int64)
                out[:, 4] += np.bincount(idx, weights=hit.ravel().astype(np.float64), minlength=m).astype(np.int64)
            else:
                out[:, 0] += qb.sum(axis=0, dtype=np.int64)
                out[:, 1] += hit.sum(axis=0, dtype=np.int64)
            if labels:
                kept_lab[i0:i0 + rows] = best[:, 0]
        if labels:
            lab[self.valid] = kept_lab
        return out.reshape((P, k, 5) if per_anchor else (P, 2)), int(self.n - self.kept.shape[0]), lab

    def _gpu(self, c, thr_q, per_anchor, labels):
        import torch
        from ._hip import lib, check
        P, k = c.shape[:2]
        need = int(lib.y3_anchor_stats_workspace_bytes(P, k))
        if self.ws is None or self.ws.numel() * 8 < need:
            self.ws = torch.empty(need // 8, dtype=torch.int64, device='cuda')
        words = (P * k * 5 if per_anchor else P * 2) + 1
        out = torch.empty(words, dtype=torch.int64, device='cuda')
        lab = torch.empty(self.n, dtype=torch.uint8, device='cuda') if labels else None
        cand = torch.from_numpy(c).cuda()
        check(lib.y3_anchor_stats(self.wh_dev.data_ptr(), self.n, cand.data_ptr(), P, k, thr_q, int(per_anchor), out.data_ptr(),
                                  lab.data_ptr() if labels else None, self.ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
              'y3_anchor_stats')
        host = out.cpu().numpy()
        return (host[:-1].reshape((P, k, 5) if per_anchor else (P, 2)).copy(), int(host[-1]), lab.cpu().numpy() if labels else None)


def anchor_stats(wh, cands, thr=0.5, per_anchor=False, labels=False, device='cpu', thr_q=None):
    """Scores P candidate anchor sets against n box sizes.  wh: integers [n, 2] = (w, h); cands: [P, k, 2] or [k, 2] = (w, h).
    -> (stats, skipped) or, with labels=True (one set only), (stats, skipped, labels):
      per_anchor: stats int64 [P, k, 5] = count, sum w, sum h, sum q, count(q >= thr_q) over the boxes whose best anchor it is;
      else:       stats int64 [P, 2]    = sum q, count(q >= thr_q) over all boxes;
      skipped = boxes with w or h outside [1, 65535] (they contribute nothing else); labels uint8 [n]: the best anchor (the
      first maximum of the IoU: the slot format_boxes writes), 255 for a skipped box.
    thr_q (an integer on the q scale) overrides thr.  device 'cpu' is NumPy, 'gpu' is y3_anchor_stats: the same integers."""
    st = _Stats(wh, device)(cands, thr_to_q(thr) if thr_q is None else thr_q, per_anchor, labels)
    return st if labels else st[:2]


def scale_sizes(wh, scale=1.0):
    """Sizes times `scale`, rounded half to even, at least 1 (the boxes of images that are resized before training)."""
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError('scale must be positive and finite, got {!r}'.format(scale))
    wh = np.asarray(wh)
    if wh.ndim != 2 or wh.shape[1] != 2 or wh.dtype.kind not in 'iu':
        raise ValueError('sizes must be integers [n, 2] = (w, h)')
    return np.maximum(np.rint(wh.astype(np.float64) * scale), 1.0).astype(np.int64)


def _sort_anchors(a):
    a = np.asarray(a, np.float32)
    area = a[:, 0].astype(np.float64) * a[:, 1].astype(np.float64)
    return a[np.lexsort((a[:, 0], area))]


def fit_anchors(wh, k, seed=0, n_init=8, lloyd_iters=30, evolve=1000, population=64, mutation_prob=0.9, sigma=0.1, thr=0.5, scale=1.0,
                device='cpu'):
    """k anchors for the box sizes wh (integers [n, 2] = (w, h)): IoU k-means, then a mutation search; see the module docstring.

    1. sizes x scale, rounded half to even, at least 1; sizes above 65535 are left out (counted in 'skipped').
    2. start pool: n_init sets of k boxes of pairwise distinct sizes, drawn from Generator(Philox(key=seed)) (boxes, so a frequent
       size is drawn more often), plus the centres of the Euclidean `kmeans` (default_rng(seed)) as float32 (w, h).
    3. Lloyd, all sets together (one per-anchor stats call per iteration): centre = float32(sum w / count), float32(sum h / count)
       by fp64 division, an empty cluster keeps its centre.  The mean does not maximise the IoU, so each set keeps its BEST iterate
       by sum q (ties: the earlier).  Stops when no set changes, or after lloyd_iters updates.
    4. search: the elite is the best set; generation g draws `population` mutants from Philox(key=seed, counter=(0, 0, 0, g + 1))
       (the generation sits in the counter's top word: no two generations share a stretch of the stream): each value times, with
       probability mutation_prob, exp(sigma N(0, 1)) clipped to [0.5, 2], fp64, rounded to float32, at least 1.  One totals call per
       generation; the mutant of largest sum q strictly above the elite's replaces it (lowest index on ties).
       ceil(evolve / population) generations; evolve = 0: none.
    -> dict: anchors [[w, h]] sorted by area then width, fitness = sum q / (n 2^24), recall at thr, table (per anchor: count,
    mean_iou, recall), history (elite sum q per generation), start_sum_q (sum q of each start set, the Euclidean centres last),
    lloyd_sum_q (elite before the search), sum_q, n, skipped, settings.  Identical for device 'cpu' and 'gpu'."""
    k, n_init, lloyd_iters, evolve, population = int(k), int(n_init), int(lloyd_iters), int(evolve), int(population)
    if not 1 <= k <= MAX_ANCHORS:
        raise ValueError('k = {} outside 1..{}'.format(k, MAX_ANCHORS))
    if n_init < 0 or lloyd_iters < 0 or evolve < 0:
        raise ValueError('n_init, lloyd_iters and evolve must be >= 0')
    if (n_init + 1) * k > MAX_CANDIDATES:
        raise ValueError('(n_init + 1) * k = {} above {}'.format((n_init + 1) * k, MAX_CANDIDATES))
    if population < 1 or population * k > MAX_CANDIDATES:
        raise ValueError('population {} x k {}: must lie in 1..{}'.format(population, k, MAX_CANDIDATES))
    if not 0.0 <= float(mutation_prob) <= 1.0 or not (math.isfinite(float(sigma)) and float(sigma) >= 0):
        raise ValueError('mutation_prob must lie in [0, 1] and sigma must be >= 0')
    thr_q = thr_to_q(thr)
    sizes = scale_sizes(wh, scale)
    keep = (sizes <= MAX_SIDE).all(axis=1)
    skipped = int((~keep).sum())
    sizes = sizes[keep].astype(np.int32)
    n = sizes.shape[0]
    uniq, counts = np.unique(sizes, axis=0, return_counts=True)
    if uniq.shape[0] < k:
        raise ValueError('{} anchors need at least {} distinct box sizes, got {}'.format(k, k, uniq.shape[0]))
    stats = _Stats(sizes, device)

    # 2. start pool
    rng = np.random.Generator(np.random.Philox(key=seed))
    weight = counts / counts.sum()
    pool = [uniq[rng.choice(uniq.shape[0], size=k, replace=False, p=weight)].astype(np.float32) for _ in range(n_init)]
    centers = kmeans(sizes[:, ::-1].astype(np.float64), k, np.random.default_rng(seed))[0]         # on (H, W), as the tool runs it
    pool.append(np.maximum(centers[:, ::-1], 1e-3).astype(np.float32))
    cur = np.stack(pool)                                                                           # [S, k, 2]

    # 3. Lloyd
    best, best_q, start_q = cur.copy(), None, None
    for it in range(lloyd_iters + 1):
        st = stats(cur, thr_q, True)[0]
        sq = st[:, :, 3].sum(axis=1)
        if best_q is None:
            best_q, start_q = sq.copy(), sq.copy()
        else:
            better = sq > best_q
            best[better], best_q[better] = cur[better], sq[better]
        if it == lloyd_iters:
            break
        cnt = st[:, :, 0]
        filled = cnt > 0
        den = np.where(filled, cnt, 1).astype(np.float64)
        new = cur.copy()
        new[..., 0] = np.where(filled, (st[:, :, 1] / den).astype(np.float32), cur[..., 0])
        new[..., 1] = np.where(filled, (st[:, :, 2] / den).astype(np.float32), cur[..., 1])
        if np.array_equal(new, cur):
            break
        cur = new

    # 4. mutation search
    e = int(np.argmax(best_q))
    elite, elite_q = best[e].copy(), int(best_q[e])
    lloyd_q = elite_q
    history = []
    for g in range(-(-evolve // population)):
        rg = np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, 0, g + 1]))
        hit = rg.random((population, k, 2)) < mutation_prob
        factor = np.clip(np.exp(sigma * rg.standard_normal((population, k, 2))), 0.5, 2.0)
        mutants = np.maximum((elite.astype(np.float64)[None] * np.where(hit, factor, 1.0)).astype(np.float32), np.float32(1.0))
        sq = stats(mutants, thr_q, False)[0][:, 0]
        m = int(np.argmax(sq))
        if int(sq[m]) > elite_q:
            elite, elite_q = mutants[m].copy(), int(sq[m])
        history.append(elite_q)

    # 5. report
    anchors = _sort_anchors(elite)
    st = stats(anchors, thr_q, True)[0][0]
    assert int(st[:, 3].sum()) == elite_q
    table = [dict(anchor=[float(a[0]), float(a[1])], count=int(r[0]), mean_iou=(float(r[3]) / (float(r[0]) * Q_ONE) if r[0] else 0.0),
                  recall=(float(r[4]) / float(r[0]) if r[0] else 0.0)) for a, r in zip(anchors, st)]
    return dict(anchors=[[float(a[0]), float(a[1])] for a in anchors], fitness=elite_q / (n * float(Q_ONE)), recall=int(st[:, 4].sum()) / float(n),
                table=table, history=history, start_sum_q=[int(v) for v in start_q], lloyd_sum_q=lloyd_q, sum_q=elite_q, n=int(n), skipped=skipped,
                settings=dict(k=k, seed=int(seed), n_init=n_init, lloyd_iters=lloyd_iters, evolve=evolve, population=population,
                              mutation_prob=float(mutation_prob), sigma=float(sigma), thr=float(thr), scale=float(scale)))


# ---- sizes of a dataset ----------------------------------------------------------------------------------------------------------

def load_sizes_csv(csv_dirpath):
    """int64 [n, 2] = (w, h) of every box of every csv of the folder, files in sorted order."""
    from . import bbox_utils
    out = [np.zeros((0, 2), np.int64)]
    for fn in sorted(f for f in os.listdir(csv_dirpath) if f.endswith('.csv')):
        boxes = bbox_utils.load_boxes_to_xywhc(os.path.join(csv_dirpath, fn))
        out.append(np.asarray(boxes[:, 2:4], np.int64).reshape(-1, 2))
    return np.concatenate(out)


def load_sizes_lmdb(path):
    """int64 [n, 2] = (w, h) of every box of every record of an lmdb written by build_lmdb.py, in key order."""
    from . import lmdbio
    from .isg_ai_pb import ImageYoloBoxesPair
    out = [np.zeros((0, 2), np.int64)]
    with lmdbio.Environment(path) as env:
        for _, value in env.items():
            m = ImageYoloBoxesPair().ParseFromString(value)
            if m.box_count > 0:
                boxes = np.frombuffer(m.boxes, dtype=np.dtype(m.box_type)).reshape(m.box_count, 5)
                out.append(boxes[:, 2:4].astype(np.int64))
    return np.concatenate(out)


# ---- files and flags -------------------------------------------------------------------------------------------------------------

def save_anchors(path, fit, anchor_scale=None):
    """The dict fit_anchors returns, as JSON (settings and results only).  anchor_scale: an owner table to record beside it
    (find_anchor_sizes.py --output records default_anchor_scales of its anchors); load_anchor_scale reads it back."""
    if anchor_scale is not None:
        fit = dict(fit, anchor_scale=check_anchor_scales(anchor_scale, len(fit['anchors'])))
    with open(path, 'w') as f:
        json.dump(fit, f, indent=1, sort_keys=True)
        f.write('\n')


def load_anchors(path):
    """-> the dict save_anchors wrote; 'anchors' is checked like the --anchors flag."""
    with open(path) as f:
        fit = json.load(f)
    if not isinstance(fit, dict) or 'anchors' not in fit:
        raise ValueError('{}: not an anchors file (no "anchors" entry)'.format(path))
    fit['anchors'] = [list(a) for a in check_anchors(fit['anchors'])]
    if 'anchor_scale' in fit:      # a file with the table reads like one without it; load_anchor_scale hands the table out
        check_anchor_scales(fit.pop('anchor_scale'), len(fit['anchors']))
    return fit


def load_anchor_scale(path):
    """-> the owner table an anchors file records (checked against its anchors), or None for a file without one."""
    with open(path) as f:
        fit = json.load(f)
    if not isinstance(fit, dict) or 'anchors' not in fit:
        raise ValueError('{}: not an anchors file (no "anchors" entry)'.format(path))
    if 'anchor_scale' not in fit:
        return None
    return check_anchor_scales(fit['anchor_scale'], len(check_anchors(fit['anchors'])))


def check_anchors(anchors):
    """-> [(w, h)] of floats; refuses none, more than 16, and sizes that are not two positive finite numbers."""
    try:
        out = [(float(w), float(h)) for w, h in anchors]
    except (TypeError, ValueError):
        raise ValueError('anchors must be a list of (w, h) pairs of numbers, got {!r}'.format(anchors))
    if not 1 <= len(out) <= MAX_ANCHORS:
        raise ValueError('between 1 and {} anchors, got {}'.format(MAX_ANCHORS, len(out)))
    for w, h in out:
        if not (math.isfinite(w) and math.isfinite(h) and w > 0 and h > 0):
            raise ValueError('anchor sizes must be positive and finite, got {},{}'.format(w, h))
    return out


# ---- per-scale anchor assignment -----------------------------------------------------------------------------------
# An owner table anchor_scale[A] gives each anchor's scale: 0 = stride 32 (coarse), 1 = stride 16, 2 = stride 8 (fine).

def default_anchor_scales(anchors):
    """The owner table YOLOv3 / Darknet use: anchors ranked by area ascending (ties: the lower index first), the anchor of rank r
    goes to scale 2 - (3 r) // A, so the smallest third sits on the fine grid.  Nine anchors give 3 / 3 / 3.  A < 3 raises."""
    anchors = check_anchors(anchors)
    A = len(anchors)
    if A < 3:
        raise ValueError('per-scale anchor assignment needs at least 3 anchors (one per scale), got {}'.format(A))
    area = np.array([float(w) * float(h) for w, h in anchors], np.float64)
    order = np.argsort(area, kind='stable')
    table = [0] * A
    for r, a in enumerate(order):
        table[int(a)] = 2 - (3 * r) // A
    return table


def check_anchor_scales(table, A):
    """-> [scale of anchor a] as ints; refuses a table of another length, entries outside 0..2 and a scale that owns no anchor."""
    try:
        out = [int(s) for s in table]
        exact = all(float(s) == int(s) for s in table)
    except (TypeError, ValueError):
        raise ValueError('anchor_scale must be a list of integers, got {!r}'.format(table))
    if not exact:
        raise ValueError('anchor_scale must be a list of integers, got {!r}'.format(table))
    if not 3 <= int(A) <= MAX_ANCHORS:
        raise ValueError('per-scale anchor assignment needs 3..{} anchors, got {}'.format(MAX_ANCHORS, A))
    if len(out) != int(A):
        raise ValueError('anchor_scale has {} entries for {} anchors'.format(len(out), A))
    if any(s not in (0, 1, 2) for s in out):
        raise ValueError('anchor_scale entries must be 0 (stride 32), 1 (stride 16) or 2 (stride 8), got {!r}'.format(out))
    for s in range(3):
        if s not in out:
            raise ValueError('scale {} owns no anchor in anchor_scale {!r}: every scale needs at least one'.format(s, out))
    return out


def parse_anchor_masks(masks, A):
    """Explicit masks, coarse -> fine, e.g. [[6, 7, 8], [3, 4, 5], [0, 1, 2]] (or the flag's text '6,7,8 3,4,5 0,1,2') -> the owner
    table.  The masks must partition 0..A-1 with no empty part."""
    if isinstance(masks, str):
        masks = masks.split()
    masks = list(masks)
    if len(masks) != 3:
        raise ValueError('anchor masks are three index lists (stride 32, 16, 8), got {}'.format(len(masks)))
    A = int(A)
    table = [None] * A
    for s, m in enumerate(masks):
        if isinstance(m, str):
            m = m.split(',')
        try:
            idx = [int(str(i).strip()) for i in m]      # '1.5' and 1.5 are refused, 3 and numpy integers pass
        except (TypeError, ValueError):
            raise ValueError('an anchor mask is a list of anchor indices, got {!r}'.format(m))
        if not idx:
            raise ValueError('anchor mask {} is empty: every scale needs at least one anchor'.format(s))
        for i in idx:
            if not 0 <= i < A:
                raise ValueError('anchor index {} outside 0..{}'.format(i, A - 1))
            if table[i] is not None:
                raise ValueError('anchor {} appears in more than one mask'.format(i))
            table[i] = s
    missing = [i for i, s in enumerate(table) if s is None]
    if missing:
        raise ValueError('anchors {} appear in no mask'.format(missing))
    return check_anchor_scales(table, A)


def scale_masks(table):
    """Owner table -> the three masks, coarse -> fine, each in index (= slot) order."""
    return [[a for a, s in enumerate(table) if s == t] for t in range(3)]


def resolve_anchor_scales(spec, anchors):
    """What YoloV3(anchor_scales=...) and ImageReader(anchor_scale=...) accept -> owner table or None: None, 'auto' (the default
    table), an owner table [A], or three masks."""
    if spec is None:
        return None
    A = len(anchors)
    if isinstance(spec, str):
        if spec != 'auto':
            raise ValueError("anchor_scales must be None, 'auto', an owner table or three index lists, got {!r}".format(spec))
        return default_anchor_scales(anchors)
    spec = list(spec)
    if len(spec) == 3 and all(isinstance(m, (list, tuple, np.ndarray)) for m in spec):
        return parse_anchor_masks(spec, A)
    return check_anchor_scales(spec, A)


def parse_anchor_args(args):
    """['10,14', '23,27'] -> [(10, 14), (23, 27)] (ints where the text is an integer, else floats)."""
    out = []
    for s in args:
        parts = str(s).split(',')
        if len(parts) != 2:
            raise ValueError('an anchor is W,H, got {!r}'.format(s))
        try:
            pair = tuple(int(p) if p.strip().lstrip('+-').isdigit() else float(p) for p in parts)
        except ValueError:
            raise ValueError('an anchor is W,H with two numbers, got {!r}'.format(s))
        out.append(pair)
    check_anchors(out)
    return out


def format_number(v):
    """Shortest text that reads back as the same float32."""
    v = float(v)
    return str(int(v)) if v == int(v) else '%.9g' % v


def anchors_flag(anchors):
    """'--anchors W,H W,H ...' for a train.py command line."""
    return '--anchors ' + ' '.join('{},{}'.format(format_number(w), format_number(h)) for w, h in anchors)


def format_fit(fit):
    """The lines the command lines print about a fit: the per-anchor table, the totals and the flag."""
    lines = ['{:>11} x {:<11} {:>9}   mean IoU   recall@{:g}'.format('anchor w', 'h', 'boxes', fit['settings']['thr'])]
    for row in fit['table']:
        lines.append('{:>11} x {:<11} {:>9}   {:.4f}     {:.4f}'.format(format_number(row['anchor'][0]), format_number(row['anchor'][1]), row['count'],
                                                                   row['mean_iou'], row['recall']))
    lines.append('fitness (mean best IoU) = {:.6f}, recall@{:g} = {:.6f} over {} boxes ({} skipped); IoU k-means alone: {:.6f}'.format(
        fit['fitness'], fit['settings']['thr'], fit['recall'], fit['n'], fit['skipped'], fit['lloyd_sum_q'] / (fit['n'] * float(Q_ONE))))
    lines.append(anchors_flag(fit['anchors']))
    return lines
