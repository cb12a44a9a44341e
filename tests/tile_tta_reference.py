"""NumPy restatements for tile test-time augmentation: the pool y3_tile_merge_voted builds, on top of the
tile-merge restatement of tests/tile_merge_reference.py, and the synthetic batches and tile tables the GPU tests use."""
import numpy as np

import inference_tiled as it
import tile_merge_reference as tm

F = np.float32
E = it.EDGE_EFFECT_RANGE
MARGINS = (0.0, 8.0)


def voted_detections(voted, keep_idx, keep_cnt, nb):
    """What the host merge would be handed for a batch whose kept boxes were voted: per tile (boxes [M,4] f32, scores [M] f32,
    labels [M] i32), class-major, keep order inside a class, entry j of (tile, class) read from voted[t, c, j, 0:5]; an entry
    whose keep_idx lies outside 0 .. nb-1 is skipped, a count is clamped to 0 .. max_keep; None for an empty tile."""
    n, K, max_keep = keep_idx.shape
    out = []
    for t in range(n):
        b, s, lab = [], [], []
        for c in range(K):
            m = min(max(int(keep_cnt[t, c]), 0), max_keep)
            ok = (keep_idx[t, c, :m] >= 0) & (keep_idx[t, c, :m] < nb)
            b.append(voted[t, c, :m, 0:4][ok].astype(np.float32))
            s.append(voted[t, c, :m, 4][ok].astype(np.float32))
            lab.append(np.full(int(ok.sum()), c, np.int32))
        b, s, lab = np.concatenate(b), np.concatenate(s), np.concatenate(lab)
        out.append((b, s, lab) if b.shape[0] else None)
    return out


def voted_pool(voted, keep_idx, keep_cnt, nb, xs, ys, tile_size, img_size, margin=0.0):
    """The pool float64 [M, 6] y3_tile_merge_voted leaves for one batch (tile_merge_reference.pool on the voted entries)."""
    return tm.pool(voted_detections(voted, keep_idx, keep_cnt, nb), xs, ys, tile_size, img_size, margin)


def voted_from_rows(rows, keep_idx, keep_cnt, keep_score):
    """voted [n, K, max_keep, 6] holding exactly what y3_tile_merge reads: rows[keep_idx] and keep_score (class in column 5)."""
    n, K, max_keep = keep_idx.shape
    nb = rows.shape[1]
    voted = np.full((n, K, max_keep, 6), -7, np.float32)
    for t in range(n):
        for c in range(K):
            m = min(max(int(keep_cnt[t, c]), 0), max_keep)
            idx = keep_idx[t, c, :m]
            ok = (idx >= 0) & (idx < nb)
            voted[t, c, :m, 0:4][ok] = rows[t, idx[ok].astype(np.int64), 0:4]
            voted[t, c, :m, 4] = keep_score[t, c, :m]
            voted[t, c, :m, 5] = c
    return voted


def _axis(rng, m, size, origin, img):
    """(lo, hi) of m boxes along one axis of a tile: centres mostly in the tile's zone, some anywhere, and at the front exactly on
    every comparison boundary of the ghost test and one ulp either side of it."""
    c = np.where(rng.random(m) < 0.7, rng.uniform(90, size - 90, m), rng.uniform(-40, size + 40, m)).astype(np.float32)
    specials = [E - mg for mg in MARGINS] + [size - E + mg for mg in MARGINS] + [E - origin, img - E - origin]
    k = 0
    for sv in specials:
        for d in (-1, 0, 1):
            v = F(sv)
            c[k] = v if d == 0 else np.nextafter(v, F(d * 1e9))
            k += 1
    h = rng.choice(np.array([4.0, 8.0, 16.0, 7.5, 12.25], np.float32), m)
    return (c - h).astype(np.float32), (c + h).astype(np.float32)


def voted_batch(seed, img, tile, K, nb=120):
    """(voted [n, K, nb, 6], keep_idx, keep_cnt, table, xs, ys) for every tile of an image: voted boxes around every boundary of
    the merge (ghost bands, halves on either side of even, far outside the image), counts from 0 to nb, a class without an entry
    when K == 3, a few keep_idx entries out of range, and in every tile one row kept under classes 0 and K-1 with different
    voted boxes.  Entries beyond a count hold -7."""
    rng = np.random.default_rng(seed)
    table, xs, ys = it.tile_table(img[0], img[1], tile)
    n = len(xs)
    voted = np.full((n, K, nb, 6), -7, np.float32)
    keep_idx = np.full((n, K, nb), -7, np.int32)
    keep_cnt = np.zeros((n, K), np.int32)
    for t in range(n):
        for c in range(K):
            m = int(rng.integers(24, nb + 1))
            if (t + c) % 5 == 4 or (K == 3 and c == 1):
                m = 0
            keep_cnt[t, c] = m
            if m == 0:
                continue
            x0, x1 = _axis(rng, m, tile[1], xs[t], img[1])
            y0, y1 = _axis(rng, m, tile[0], ys[t], img[0])
            x0[18:22] = np.array([10.5, 11.5, -2.5, 0.5], np.float32)          # halves: the tile origins are integers
            y1[18:22] = np.array([120.5, 121.5, 122.5, 123.5], np.float32)
            x1[22] += F(3000)                                                  # far outside: the rounded centre leaves the image
            x0[23], x1[23] = F(-20), F(60)                                     # negative: the clamp (where the tile starts at x = 0)
            voted[t, c, :m, 0], voted[t, c, :m, 1], voted[t, c, :m, 2], voted[t, c, :m, 3] = x0, y0, x1, y1
            voted[t, c, :m, 4] = np.sort(rng.uniform(0.1, 1, m).astype(np.float32))[::-1]
            voted[t, c, :m, 5] = c
            keep_idx[t, c, :m] = rng.permutation(nb)[:m]
            if m > 30 and t % 3 == 1:
                keep_idx[t, c, 25] = -1 if c == 0 else nb                      # never produced by the NMS: skipped, not read
        if keep_cnt[t, 0] and keep_cnt[t, K - 1] and K > 1:
            keep_idx[t, 0, 0] = keep_idx[t, K - 1, 0] = 5
            voted[t, 0, 0, 0:4] = [100, 100, 130, 140]
            voted[t, K - 1, 0, 0:4] = [104, 98, 131, 139]
    return voted, keep_idx, keep_cnt, table, xs, ys


def gather_tables(th, tw, height, width):
    """Tile table rows {y0, ny, pre_y, x0, nx, pre_x} for tiles of th x tw over a height x width image, as tile_table clamps them:
    an interior crop, a top-left tile with reflected rows and columns in front (non-zero pre_y / pre_x), a bottom-right tile cut by
    the image (reflected behind), one with both, and the whole image as one crop."""
    ny, nx = min(th, height), min(tw, width)
    rows = [[min(3, height - ny), ny, 0, min(5, width - nx), nx, 0],
            [0, max(1, min(th - 5, height)), 5, 0, max(1, min(tw - 7, width)), 7],
            [height - max(1, ny - 3), max(1, ny - 3), 0, width - max(1, nx - 2), max(1, nx - 2), 0],
            [0, max(2, ny // 3), 2, width - max(2, nx // 3), max(2, nx // 3), 3],
            [0, ny, 0, 0, nx, 0]]
    return np.asarray(rows, np.int32)
