"""CPU-only tests of opt-in mosaic augmentation: the counter-based record draw, the box remap against a pixel
oracle (one mask per box pushed through the NumPy restatement of the kernel), and the argument checks of Dataset.mosaic() and
train.py."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
sys.path.insert(0, PKG)

ANCHORS = [(64, 384), (384, 64)]


def _quadrants(cy, cx, h, w):
    return ((0, 0, cy, cx), (0, cx, cy, w - cx), (cy, 0, h - cy, cx), (cy, cx, h - cy, w - cx))


def _abi_errors(recs, n, h, w):
    """The validation rules of y3_mosaic_batch (include/yolo3hip.h), restated."""
    bad = []
    for i, r in enumerate(recs):
        if not (0 <= r['cy'] <= h and 0 <= r['cx'] <= w):
            bad.append((i, 'seam'))
            continue
        if r['reserved'].any():
            bad.append((i, 'reserved'))
        for q, (_, _, qh, qw) in enumerate(_quadrants(int(r['cy']), int(r['cx']), h, w)):
            if qh == 0 or qw == 0:
                continue
            if not 0 <= r['src'][q] < n:
                bad.append((i, q, 'source'))
            if r['oy'][q] < 0 or r['oy'][q] + qh > h or r['ox'][q] < 0 or r['ox'][q] + qw > w:
                bad.append((i, q, 'window'))
    return bad


def _is_identity(r, i, h, w):
    return r['cy'] == h and r['cx'] == w and r['src'][0] == i and r['oy'][0] == 0 and r['ox'][0] == 0


# ---- draw_mosaic ---------------------------------------------------------------------------------------------------------
def test_record_dtype_matches_the_header():
    from yolo3 import augment
    d = augment.MOSAIC_RECORD
    assert d.itemsize == 64 and d.names == ('cy', 'cx', 'src', 'oy', 'ox', 'reserved')
    assert [d.fields[k][1] for k in d.names] == [0, 4, 8, 24, 40, 56]
    hdr = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    assert ' y3_mosaic_batch(' in hdr and 'typedef struct y3_mosaic_record' in hdr
    from yolo3 import _hip
    assert 'y3_mosaic_batch' in _hip.SIGNATURES and hasattr(_hip.lib, 'y3_mosaic_batch')


def test_draw_is_a_pure_function_of_its_arguments():
    from yolo3 import augment
    a = augment.draw_mosaic(3, 1, 7, 8, (64, 64), 1.0)
    assert a.dtype == augment.MOSAIC_RECORD and a.shape == (8,)
    assert a.tobytes() == augment.draw_mosaic(3, 1, 7, 8, (64, 64), 1.0).tobytes()
    for other in ((3, 1, 8), (3, 0, 7), (4, 1, 7)):          # another batch index, shard, seed
        assert a.tobytes() != augment.draw_mosaic(other[0], other[1], other[2], 8, (64, 64), 1.0).tobytes(), other
    state = np.random.get_state()[1].copy()                  # no global np.random
    augment.draw_mosaic(0, 0, 0, 8, (64, 64), 0.5)
    assert np.array_equal(np.random.get_state()[1], state)


@pytest.mark.parametrize('size', [(64, 64), (96, 160), (32, 32)])
def test_every_drawn_record_is_valid_for_the_kernel(size):
    from yolo3 import augment
    h, w = size
    seen_cy, seen_cx = set(), set()
    for b in range(40):                                      # 40 batches x 8 images
        recs = augment.draw_mosaic(5, 0, b, 8, size, 1.0)
        assert _abi_errors(recs, 8, h, w) == []
        assert not any(_is_identity(r, i, h, w) for i, r in enumerate(recs))      # prob = 1: no identity record
        assert all(h // 4 <= r['cy'] <= h - h // 4 and w // 4 <= r['cx'] <= w - w // 4 for r in recs)
        seen_cy.update(recs['cy'].tolist())
        seen_cx.update(recs['cx'].tolist())
    assert min(seen_cy) <= h // 4 + 2 and max(seen_cy) >= h - h // 4 - 2 and len(seen_cy) > (h // 2) // 2      # the whole range is used
    assert min(seen_cx) <= w // 4 + 2 and max(seen_cx) >= w - w // 4 - 2


def test_sources_are_distinct_from_four_images_up_and_in_range_below():
    from yolo3 import augment
    for n in (4, 5, 8):
        partners = set()
        for b in range(60):
            for i, r in enumerate(augment.draw_mosaic(1, 0, b, n, (64, 64), 1.0)):
                s = r['src'].tolist()
                assert s[0] == i and len(set(s)) == 4 and all(0 <= v < n for v in s), (n, b, i, s)
                partners.update(s[1:])
        assert partners == set(range(n))
    for n in (1, 2, 3):
        for b in range(60):
            recs = augment.draw_mosaic(1, 0, b, n, (64, 64), 1.0)
            assert _abi_errors(recs, n, 64, 64) == []
            for i, r in enumerate(recs):
                s = r['src'].tolist()
                assert s[0] == i and all(0 <= v < n for v in s)
                assert n == 1 or all(v != i for v in s[1:])


def test_share_of_mosaics_follows_prob():
    from yolo3 import augment
    recs = np.concatenate([augment.draw_mosaic(11, 0, b, 8, (64, 64), 0.5) for b in range(250)])
    ident = np.array([_is_identity(r, i % 8, 64, 64) for i, r in enumerate(recs)])
    assert len(recs) == 2000 and abs((~ident).mean() - 0.5) <= 0.05, (~ident).mean()
    assert _abi_errors(recs[:8], 8, 64, 64) == []
    for r in recs[ident]:                                    # the identity record is the ABI's, nothing else set
        assert r['src'][1:].tolist() == [0, 0, 0] and not r['oy'].any() and not r['ox'].any()


# ---- mosaic_boxes against pixels ---------------------------------------------------------------------------------------------
def _rec(cy, cx, src, oy, ox):
    from yolo3 import augment
    r = np.zeros(1, augment.MOSAIC_RECORD)
    r[0] = (cy, cx, src, oy, ox, [0, 0])
    return r


def _pixel_oracle(box_lists, records, size, min_visible):
    """Every box painted alone into a mask of its image, the masks pushed through mosaic_reference: per output image, quadrants in
    order and boxes in source order, the bounding rectangle of the surviving pixels; the pixel count over the box's area decides
    the min_visible drop (in exact rational arithmetic)."""
    from yolo3 import augment
    h, w = size
    n = len(box_lists)
    out = [[] for _ in range(n)]
    pieces = {}
    for s, boxes in enumerate(box_lists):
        for k, (bx, by, bw, bh, cls) in enumerate([] if boxes is None else np.asarray(boxes).tolist()):
            mask = np.zeros((n, 1, h, w), np.uint8)
            mask[s, 0, by:by + bh, bx:bx + bw] = 1
            assert mask.sum() == bw * bh, 'test boxes lie inside their image'
            moved = augment.mosaic_reference(mask, records)
            for i, r in enumerate(records):
                for q, (qy, qx, qh, qw) in enumerate(_quadrants(int(r['cy']), int(r['cx']), h, w)):
                    if qh == 0 or qw == 0 or int(r['src'][q]) != s:
                        continue
                    ys, xs = np.nonzero(moved[i, 0, qy:qy + qh, qx:qx + qw])
                    if len(ys) and Fraction(len(ys)) >= Fraction(min_visible) * bw * bh:
                        rect = (qx + xs.min(), qy + ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1, cls)
                        assert rect[2] * rect[3] == len(ys)                      # the visible part of a box is a rectangle
                        pieces[(i, q, k)] = rect
    for (i, q, k) in sorted(pieces):
        out[i].append(pieces[(i, q, k)])
    return [np.array(o, np.int32).reshape(-1, 5) for o in out]


def test_boxes_follow_their_pixels_named_cases():
    """32 x 32, seam (16, 16); quadrant 0 of output 0 shows the window [4,20) x [4,20) of image 0."""
    from yolo3 import augment
    size = (32, 32)
    b0 = np.array([[10, 6, 14, 8, 0],       # cut by the seam column: 10 of 14 columns stay
                   [14, 14, 10, 10, 1],     # cut by both seams: 36 of 100 pixels
                   [12, 4, 8, 4, 0],        # ends exactly on the seam column, starts on the window's first row: whole
                   [20, 8, 6, 6, 1],        # starts exactly on the seam: fully outside the window
                   [16, 0, 8, 8, 0],        # 4 x 4 of 8 x 8 visible: exactly min_visible, kept
                   [17, 0, 8, 8, 1],        # 3 x 4 of 8 x 8 visible: below it, dropped
                   [24, 24, 6, 6, 0]], np.int32)      # nowhere near the window
    b1 = np.array([[0, 0, 32, 32, 1], [3, 5, 4, 4, 0]], np.int32)
    b2 = np.array([[8, 8, 16, 16, 0]], np.int32)
    lists = [b0, b1, b2, None]
    recs = np.concatenate([_rec(16, 16, [0, 1, 2, 3], [4, 0, 8, 16], [4, 16, 0, 16]),      # image 3 (quadrant 3) has no boxes
                           _rec(32, 32, [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]),         # identity
                           _rec(10, 32, [3, 9, 2, 9], [5, 0, 0, 0], [0, 0, 0, 0]),         # no right half: quadrants 1, 3 empty, their fields junk
                           _rec(16, 16, [0, 0, 0, 0], [0, 0, 16, 16], [0, 16, 0, 16])])    # image 0 put together again from its own quarters
    got = augment.mosaic_boxes(lists, recs, size)
    want = _pixel_oracle(lists, recs, size, 0.25)
    for i in range(4):
        assert got[i].dtype == np.int32 and got[i].shape[1] == 5 and np.array_equal(got[i], want[i]), (i, got[i], want[i])
    assert got[0].tolist()[:4] == [[6, 2, 10, 8, 0], [10, 10, 6, 6, 1], [8, 0, 8, 4, 0], [12, 0, 4, 4, 0]]
    assert [16, 0, 16, 16, 1] in got[0].tolist()                    # the whole-image box of image 1 fills quadrant 1
    assert np.array_equal(got[1], b1)                               # identity: the boxes as they came
    assert got[2].tolist() == [[8, 18, 16, 14, 0]]                  # rows [0, 22) of image 2 below the seam row 10: 14 of its 16 rows
    # a lower threshold keeps the 12 / 64 box, a higher one drops the 36 / 100 box; each as the pixels say
    for mv in (0.0, 0.1875, 0.375, 1.0):       # dyadic: min_visible * area is exact in float64
        got = augment.mosaic_boxes(lists, recs, size, min_visible=mv)
        want = _pixel_oracle(lists, recs, size, mv)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), mv
    assert augment.mosaic_boxes(lists, recs, size, 0.1875)[0].tolist()[4] == [13, 0, 3, 4, 1]


def test_boxes_follow_their_pixels_random_sweep():
    from yolo3 import augment
    rng = np.random.default_rng(7)
    size = (32, 32)
    total = 0
    for trial in range(12):
        n = int(rng.integers(1, 6))
        lists = []
        for _ in range(n):
            k = int(rng.integers(0, 4))
            wh = rng.integers(1, 20, (k, 2))
            xy = np.stack([rng.integers(0, 32 - wh[:, 0] + 1), rng.integers(0, 32 - wh[:, 1] + 1)], 1) if k else np.zeros((0, 2), int)
            lists.append(np.concatenate([xy, wh, rng.integers(0, 3, (k, 1))], 1).astype(np.int32) if k else None)
        recs = augment.draw_mosaic(trial, 0, 0, n, size, 0.8)
        got = augment.mosaic_boxes(lists, recs, size)
        want = _pixel_oracle(lists, recs, size, 0.25)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (trial, g, w)
            total += len(g)
    assert total > 20


def test_boxes_empty_inputs_and_identity():
    from yolo3 import augment
    recs = augment.draw_mosaic(0, 0, 0, 4, (32, 32), 1.0)
    for lists in ([None] * 4, [np.zeros((0, 5), np.int32)] * 4):
        out = augment.mosaic_boxes(lists, recs, (32, 32))
        assert len(out) == 4 and all(o.shape == (0, 5) and o.dtype == np.int32 for o in out)
    ident = np.zeros(3, augment.MOSAIC_RECORD)
    ident['cy'], ident['cx'] = 32, 32
    ident['src'][:, 0] = np.arange(3)
    boxes = [np.array([[5, 5, 10, 10, 1], [0, 0, 3, 3, 0], [5, 5, 10, 10, 1]], np.int32), None, np.array([[31, 31, 1, 1, 2]], np.int32)]
    out = augment.mosaic_boxes(boxes, ident, (32, 32))
    assert np.array_equal(out[0], boxes[0]) and out[1].shape == (0, 5) and np.array_equal(out[2], boxes[2])
    assert out[0] is not boxes[0]


def test_reference_identity_and_quadrants():
    from yolo3 import augment
    x = np.arange(2 * 3 * 4 * 6, dtype=np.float32).reshape(2, 3, 4, 6)
    ident = np.zeros(2, augment.MOSAIC_RECORD)
    ident['cy'], ident['cx'] = 4, 6
    ident['src'][:, 0] = [0, 1]
    assert np.array_equal(augment.mosaic_reference(x, ident), x)
    r = np.concatenate([_rec(1, 2, [0, 1, 1, 0], [3, 0, 1, 0], [4, 2, 0, 1]), _rec(4, 0, [5, 0, 5, 5], [9, 0, 9, 9], [9, 0, 9, 9])])
    y = augment.mosaic_reference(x, r)
    assert np.array_equal(y[0, :, :1, :2], x[0, :, 3:4, 4:6]) and np.array_equal(y[0, :, :1, 2:], x[1, :, 0:1, 2:6])
    assert np.array_equal(y[0, :, 1:, :2], x[1, :, 1:4, 0:2]) and np.array_equal(y[0, :, 1:, 2:], x[0, :, 0:3, 1:5])
    assert np.array_equal(y[1], x[0])                        # only quadrant 1 is non-empty; the junk in the others is ignored


# ---- Dataset.mosaic / train.py ---------------------------------------------------------------------------------------------
def _make_lmdb(path, n=4, size=(64, 64, 3)):
    import build_lmdb
    from yolo3 import lmdbio
    rng = np.random.default_rng(3)
    items = []
    for i in range(n):
        img = rng.integers(0, 256, size, dtype=np.uint8)
        boxes = np.array([[4 + i, 6, 20, 24, i % 2]], np.int32)
        items.append(build_lmdb.make_record(img, boxes, i, 'img%03d' % i))
    lmdbio.write_environment(path, items)


def test_dataset_mosaic_argument_checks(tmp_path):
    from yolo3.imagereader import ImageReader
    path = str(tmp_path / 'train-syn.lmdb')
    _make_lmdb(path)
    rd = ImageReader(path, ANCHORS, num_workers=1, augmentation_device='gpu', label_device='gpu')
    base = rd.get_tf_dataset()
    assert base.mosaic_cfg is None and base.batch(2).prefetch(2).mosaic_cfg is None
    a = base.batch(2).mosaic(0.5, seed=3).prefetch(2).multiscale([(64, 64), (96, 96)], 1)
    b = base.multiscale([(64, 64), (96, 96)], 1).mosaic(0.5, 3, min_visible=0.25).batch(2)
    assert a.mosaic_cfg == b.mosaic_cfg == (0.5, 3, 0.25) and a.multiscale_cfg == b.multiscale_cfg and a.prefetch_depth == 2
    assert base.mosaic(1).mosaic_cfg == (1.0, 0, 0.25)
    for bad in (0, -0.1, 1.5, True, float('nan')):
        with pytest.raises(ValueError, match='prob'):
            base.mosaic(bad)
    with pytest.raises(ValueError, match='min_visible'):
        base.mosaic(0.5, min_visible=2)
    for plain in (ImageReader(path, ANCHORS, num_workers=1, augmentation_device='gpu'), ImageReader(path, ANCHORS, num_workers=1)):
        with pytest.raises(ValueError, match='label_device'):
            plain.get_tf_dataset().mosaic(0.5)
    with pytest.raises(ValueError, match='batch'):           # a mosaic needs the other images of a batch
        next(iter(base.mosaic(0.5)))


def _parse(extra):
    import train
    return train.build_parser().parse_args(['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c'] + extra)


def test_train_parser_and_train_model_mosaic_flags(capsys):
    import train
    a = _parse([])
    assert (a.mosaic_prob, a.mosaic_seed, a.mosaic_min_visible) == (0.0, 0, 0.25)
    a = _parse(['--augmentation_device', 'gpu', '--mosaic_prob', '0.5', '--mosaic_seed', '9', '--mosaic_min_visible', '0.4',
                '--multiscale_min', '320', '--multiscale_max', '608'])
    assert (a.mosaic_prob, a.mosaic_seed, a.mosaic_min_visible, a.multiscale_min) == (0.5, 9, 0.4, 320)
    with pytest.raises(SystemExit):
        _parse(['--mosaic_prob', '0.5'])
    assert '--mosaic_prob needs --augmentation_device gpu' in capsys.readouterr().err
    for bad in (['--mosaic_prob', '1.5'], ['--mosaic_prob', '-0.5'], ['--mosaic_prob', '0.5', '--mosaic_min_visible', '3']):
        with pytest.raises(SystemExit):
            _parse(['--augmentation_device', 'gpu'] + bad)
    with pytest.raises(ValueError, match='augmentation_device'):      # checked before a reader or the device is touched
        train.train_model(2, 2, 'absent-a', 'absent-b', 'absent-c', 1, 1e-4, True, mosaic_prob=0.5)
    with pytest.raises(ValueError, match='mosaic_prob'):
        train.train_model(2, 2, 'absent-a', 'absent-b', 'absent-c', 1, 1e-4, True, augmentation_device='gpu', mosaic_prob=2.0)


def test_library_refuses_bad_records_without_a_device():
    """The host-side validation of y3_mosaic_batch needs no GPU: fake, disjoint addresses that nothing dereferences (every call
    here fails a check before the first launch)."""
    from yolo3 import augment
    from yolo3._hip import lib
    src, out = 1 << 20, 1 << 24
    n, c, h, w = 3, 3, 8, 12

    def call(recs, src=src, out=out, n=n, c=c, h=h, w=w):
        recs = np.ascontiguousarray(recs, dtype=augment.MOSAIC_RECORD)
        rc = lib.y3_mosaic_batch(src, n, c, h, w, recs.ctypes.data, out, None)
        return rc, lib.y3_last_error().decode()

    good = _rec(4, 6, [0, 1, 2, 0], [1, 2, 3, 4], [0, 1, 2, 6])
    cases = [(_rec(9, 6, [0] * 4, [0] * 4, [0] * 4), 'seam'), (_rec(4, -1, [0] * 4, [0] * 4, [0] * 4), 'seam'),
             (_rec(4, 6, [0, 3, 2, 0], [0] * 4, [0] * 4), 'source image'), (_rec(4, 6, [0, 1, -1, 0], [0] * 4, [0] * 4), 'source image'),
             (_rec(4, 6, [0, 1, 2, 0], [0, 0, 5, 0], [0] * 4), 'window'), (_rec(4, 6, [0, 1, 2, 0], [0] * 4, [0, 0, 0, 7]), 'window'),
             (_rec(4, 6, [0, 1, 2, 0], [-1, 0, 0, 0], [0] * 4), 'window')]
    for bad, what in cases:
        rc, msg = call(np.concatenate([good, bad, good]))
        assert rc == -1 and msg.startswith('mosaic_batch: record 1') and what in msg, (what, rc, msg)
    r = np.concatenate([good] * 3)
    r['reserved'][2, 0] = 7
    rc, msg = call(r)
    assert rc == -1 and 'record 2' in msg and 'reserved' in msg
    for kw, what in ((dict(c=2), 'channels'), (dict(n=0), 'dims'), (dict(h=0), 'dims'), (dict(w=-3), 'dims'), (dict(src=0), 'null'),
                     (dict(out=src), 'overlap'), (dict(out=src + 4 * (n * c * h * w - 1)), 'overlap'), (dict(src=src + 2), 'aligned'),
                     (dict(h=1 << 16, w=1 << 15), 'too large')):
        rc, msg = call(np.concatenate([good] * 3), **kw)
        assert rc == -1 and what in msg, (kw, rc, msg)
