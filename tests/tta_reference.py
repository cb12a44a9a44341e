"""NumPy restatements of the test-time augmentation kernels (yolo3hip.h: y3_tta_views_nhwc, y3_tta_unmap, y3_box_vote).

A view is a 3-bit code: 4 = transpose (applied first), 1 = flip x, 2 = flip y.  Everything the kernels do in fp32 is done here
in float32 in the same order; the vote's sums are float64 (any order: the kernel's differs by at most the final rounding)."""
import numpy as np

FLIP_X, FLIP_Y, TRANSPOSE = 1, 2, 4
f32 = np.float32


def view_of(img, code):
    """img [..., H, W] -> the view (a NumPy view, no arithmetic)."""
    out = img
    if code & TRANSPOSE:
        out = np.swapaxes(out, -1, -2)
    if code & FLIP_X:
        out = out[..., :, ::-1]
    if code & FLIP_Y:
        out = out[..., ::-1, :]
    return out


def views_nchw(src, codes):
    """src [N, C, H, W] -> [N * k, C, H, W], image-major and view-minor."""
    return np.stack([np.ascontiguousarray(view_of(src[i], c)) for i in range(src.shape[0]) for c in codes])


def views_nhwc(src, codes, dc=4):
    """src [N, C, H, W] of any 4-byte dtype -> [N * k, H, W, dc] with the channels beyond C zero (bits are kept: no cast)."""
    v = views_nchw(src, codes)
    out = np.zeros((v.shape[0], v.shape[2], v.shape[3], dc), src.dtype)
    out[..., :src.shape[1]] = v.transpose(0, 2, 3, 1)
    return out


def forward_boxes(boxes, code, h, w):
    """Corner boxes [M, 4] = x0, y0, x1, y1 of an H x W image -> the same boxes in the frame of view `code` (float32)."""
    b = np.array(boxes, f32).reshape(-1, 4).copy()
    if code & TRANSPOSE:
        b = b[:, [1, 0, 3, 2]]
        h, w = w, h
    if code & FLIP_X:
        b[:, 0], b[:, 2] = f32(w) - b[:, 2], f32(w) - b[:, 0]
    if code & FLIP_Y:
        b[:, 1], b[:, 3] = f32(h) - b[:, 3], f32(h) - b[:, 1]
    return b


def unmap_boxes(boxes, code, h, w):
    """Inverse of forward_boxes for a view whose own frame is H x W (square when it transposes): un-flip, then transpose."""
    b = np.array(boxes, f32).reshape(-1, 4).copy()
    if code & FLIP_X:
        b[:, 0], b[:, 2] = f32(w) - b[:, 2], f32(w) - b[:, 0]
    if code & FLIP_Y:
        b[:, 1], b[:, 3] = f32(h) - b[:, 3], f32(h) - b[:, 1]
    if code & TRANSPOSE:
        b = b[:, [1, 0, 3, 2]]
    return b


def unmap_rows(rows, codes, h, w):
    """rows float32 [N * k, Nb, D] -> a copy with the corners of view j % k mapped back; the other columns untouched."""
    out = np.array(rows, f32, copy=True)
    k = len(codes)
    for j in range(out.shape[0]):
        out[j, :, 0:4] = unmap_boxes(out[j, :, 0:4], codes[j % k], h, w)
    return out


def clip_boxes(b, clip_wh):
    b = np.array(b, f32).reshape(-1, 4).copy()
    if clip_wh is not None:
        b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], f32(0)), f32(clip_wh[0]))
        b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], f32(0)), f32(clip_wh[1]))
    return b


def iou_f32(k, b):
    """The NMS kernels' IoU of box k [4] against boxes b [M, 4], float32 in their order (0 / 0 -> NaN)."""
    k = np.asarray(k, f32)
    b = np.asarray(b, f32).reshape(-1, 4)
    karea = (k[2] - k[0]) * (k[3] - k[1])
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    xl, yt = np.maximum(k[0], b[:, 0]), np.maximum(k[1], b[:, 1])
    xr, yb = np.minimum(k[2], b[:, 2]), np.minimum(k[3], b[:, 3])
    inter = np.maximum(yb - yt, f32(0)) * np.maximum(xr - xl, f32(0))
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / ((karea + area) - inter)


def candidates(rows_img, cls, min_box, score_thr, clip_wh):
    """(row indices in row order, clipped boxes float32 [M, 4], scores float32 [M]) of the NMS candidates of class cls."""
    r = np.asarray(rows_img, f32)
    b = clip_boxes(r[:, 0:4], clip_wh)
    with np.errstate(invalid='ignore'):
        s = np.sqrt(r[:, 5 + cls] * r[:, 4])
        ok = ((b[:, 2] - b[:, 0]) > f32(min_box)) & ((b[:, 3] - b[:, 1]) > f32(min_box)) & (s >= f32(score_thr))
    idx = np.nonzero(ok)[0]
    return idx, b[idx], s[idx]


def vote(rows, keep_idx, keep_cnt, keep_score, min_box, score_thr, clip_wh, vote_iou, views, rows_per_view, consensus):
    """y3_box_vote.  Returns a dict: box64 [N, K, max_keep, 4] (float64, before the one rounding), score float32 [N, K, max_keep],
    members [N, K, max_keep] int (member count), valid bool [N, K, max_keep] (j < min(keep_cnt, max_keep)), margin = the
    smallest |iou - vote_iou| over every (keep, candidate) pair whose IoU is not exactly 1.0 between bit-identical boxes."""
    rows = np.asarray(rows, f32)
    n, nb, d = rows.shape
    K, max_keep = d - 5, keep_idx.shape[2]
    box64 = np.zeros((n, K, max_keep, 4))
    score = np.zeros((n, K, max_keep), f32)
    members = np.zeros((n, K, max_keep), np.int64)
    valid = np.zeros((n, K, max_keep), bool)
    margin = np.inf
    thr = f32(vote_iou)
    for i in range(n):
        own = clip_boxes(rows[i, :, 0:4], clip_wh)
        for c in range(K):
            idx, b, s = candidates(rows[i], c, min_box, score_thr, clip_wh)
            for j in range(min(int(keep_cnt[i, c]), max_keep)):
                valid[i, c, j] = True
                kb = own[keep_idx[i, c, j]]
                iou = iou_f32(kb, b) if idx.size else np.zeros(0, f32)
                same = np.all(b.view(np.uint32) == kb.view(np.uint32)[None, :], axis=1) & (iou == f32(1)) if idx.size else np.zeros(0, bool)
                dist = np.abs(iou.astype(np.float64) - float(thr))[~same & ~np.isnan(iou)]
                if dist.size:
                    margin = min(margin, float(dist.min()))
                with np.errstate(invalid='ignore'):
                    mem = iou >= thr
                members[i, c, j] = int(mem.sum())
                sm = s[mem].astype(np.float64)
                if mem.any() and sm.sum() > 0:
                    box64[i, c, j] = (sm[:, None] * b[mem].astype(np.float64)).sum(0) / sm.sum()
                else:
                    box64[i, c, j] = kb
                if consensus:
                    acc = f32(0)
                    for v in range(views):
                        sv = s[mem & (idx // rows_per_view == v)]
                        acc = f32(acc + (sv.max() if sv.size else f32(0)))
                    score[i, c, j] = acc / f32(views)
                else:
                    score[i, c, j] = keep_score[i, c, j]
    return {'box64': box64, 'score': score, 'members': members, 'valid': valid, 'margin': margin}


# ---- the synthetic scene of the box-vote tests --------------------------------------------------------------------------------
VOTE_CHUNK = 256                      # Y3_VOTE_CHUNK: candidates a workgroup stages in LDS per pass
SCENE = dict(n=2, K=3, views=4, slots=200, clip_wh=(970, 480), min_box=10.0, score_thr=0.1, iou_thr=0.3,
             # candidates per (image, class): none, one, one below / at / above the LDS chunk, more than two chunks
             counts=((0, 1, VOTE_CHUNK - 1), (VOTE_CHUNK, VOTE_CHUNK + 1, 600)),
             shared_slot=57)          # image 1: its view-0 row is the best candidate of classes 1 AND 2, alone in class 1, with all its views in class 2


def vote_scene(seed=11):
    """rows float32 [2, 4 * 200, 5 + 3] of known member sets.  Slot t of every view is object t: a 40 x 40 box on a 20 x 10 grid of
    pitch 50 that starts at -10 (the first row and column leave the image and are clipped; the last column too), moved by up to
    2 px per corner from view to view (IoU between views > 0.6), objects apart from each other (IoU 0).  Every 7th object
    is the same box, bit for bit, in all views; every 5th has its view-3 copy 24 px to the right (IoU about 0.25 with the
    others, and about as much with its right neighbour: no member at 0.5); every 17th is 8 x 8 and fails the small-box filter.  Which rows are candidates of which class
    is set through the class columns, to the exact counts of SCENE['counts']."""
    S = SCENE
    rng = np.random.default_rng(seed)
    n, K, k, nbv = S['n'], S['K'], S['views'], S['slots']
    nb = k * nbv
    rows = np.zeros((n, nb, 5 + K), f32)
    t = np.arange(nbv)
    base = np.stack([-10 + 50 * (t % 20), -10 + 50 * (t // 20)], 1).astype(np.float64)
    for i in range(n):
        frac = rng.uniform(0, 1, (nbv, 2))
        for v in range(k):
            jit = rng.uniform(-2, 2, (nbv, 4))
            jit[t % 7 == 0] = 0
            x0 = base[:, 0] + frac[:, 0] + jit[:, 0]
            y0 = base[:, 1] + frac[:, 1] + jit[:, 1]
            x1 = base[:, 0] + frac[:, 0] + 40 + jit[:, 2]
            y1 = base[:, 1] + frac[:, 1] + 40 + jit[:, 3]
            if v == 3:
                far = (t % 5 == 0) & (t % 7 != 0)
                x0, x1 = x0 + 24 * far, x1 + 24 * far
            small = t % 17 == 3
            x1 = np.where(small, x0 + 8, x1)
            y1 = np.where(small, y0 + 8, y1)
            rows[i, v * nbv:(v + 1) * nbv, 0:4] = np.stack([x0, y0, x1, y1], 1).astype(f32)
        rows[i, :, 4] = rng.uniform(0.5, 0.95, nb).astype(f32)
        rows[i, :, 5:] = f32(0.001)
        b = clip_boxes(rows[i, :, 0:4], S['clip_wh'])
        ok = ((b[:, 2] - b[:, 0]) > f32(S['min_box'])) & ((b[:, 3] - b[:, 1]) > f32(S['min_box']))
        shared = S['shared_slot'] + nbv * np.arange(k)               # the rows of one object, view by view
        for c in range(K):
            want = S['counts'][i][c]
            forced = np.zeros(0, np.int64)
            if i == 1 and c == 1:
                forced = shared[:1]
            if i == 1 and c == 2:
                forced = shared
            free = np.setdiff1d(np.nonzero(ok)[0], shared)
            pick = np.concatenate([forced, rng.permutation(free)[:want - forced.size]]) if want else forced[:0]
            rows[i, pick, 5 + c] = rng.uniform(0.3, 0.95, pick.size).astype(f32)
        if i == 1:
            rows[i, shared[0], 4:] = [1.0, 0.001, 1.0, 1.0]           # the top score of its cluster under both classes
    return rows


def scene_margin(rows, vote_iou):
    """The smallest |iou - vote_iou| over EVERY pair of candidates of one (image, class) -- a superset of the (keep, candidate)
    pairs a vote forms -- bit-identical boxes with IoU exactly 1 left out; and the candidate counts [n][K]."""
    S = SCENE
    margin, counts = np.inf, []
    for i in range(rows.shape[0]):
        counts.append([])
        for c in range(S['K']):
            idx, b, s = candidates(rows[i], c, S['min_box'], S['score_thr'], S['clip_wh'])
            counts[-1].append(int(idx.size))
            for q in range(idx.size):
                iou = iou_f32(b[q], b)
                same = np.all(b.view(np.uint32) == b[q].view(np.uint32)[None, :], axis=1) & (iou == f32(1))
                d = np.abs(iou.astype(np.float64) - float(f32(vote_iou)))[~same & ~np.isnan(iou)]
                if d.size:
                    margin = min(margin, float(d.min()))
    return margin, counts
