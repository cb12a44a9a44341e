"""GPU tests of opt-in mosaic augmentation: y3_mosaic_batch against its NumPy restatement bit for bit (seams at
every edge, every source shift mod 4, unaligned destinations, the 32-image chunk boundary), its host-side refusals, the data
plane end to end (alone and with multi-scale, both prefetch settings), one training step on a mosaic batch, train.py, and the
unchanged default path."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
sys.path.insert(0, PKG)

ANCHORS = [(64, 384), (384, 64)]
CANARY = 0xCAFEF00D
GUARD = 1024                        # words before and after `out`
SPECIAL = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0x7f800001, 0xffc12345, 0x00000001, 0x00000000], np.uint32)


def _bits(rng, shape):
    """Random 32-bit patterns with -0.0, the infinities, quiet and signalling NaNs with payloads and a denormal sprinkled in."""
    x = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    flat = x.reshape(-1)
    idx = rng.integers(0, flat.size, max(1, flat.size // 5))
    flat[idx] = SPECIAL[rng.integers(0, len(SPECIAL), len(idx))]
    return x


def _to_dev(u32):
    return torch.from_numpy(np.ascontiguousarray(u32).view(np.int32)).cuda().view(torch.float32)


def _to_u32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _records(rows):
    from yolo3 import augment
    r = np.zeros(len(rows), augment.MOSAIC_RECORD)
    for i, (cy, cx, src, oy, ox) in enumerate(rows):
        r[i] = (cy, cx, src, oy, ox, [0, 0])
    return r


def _random_records(rng, n, h, w, cy, cx):
    """Seam (cy, cx) for every output image, random sources and random windows that fit; the fields of empty quadrants are junk."""
    rows = []
    for _ in range(n):
        src, oy, ox = [], [], []
        for qh, qw in ((cy, cx), (cy, w - cx), (h - cy, cx), (h - cy, w - cx)):
            if qh == 0 or qw == 0:
                src.append(int(rng.integers(-5, n + 5)))
                oy.append(int(rng.integers(-9, h + 9)))
                ox.append(int(rng.integers(-9, w + 9)))
            else:
                src.append(int(rng.integers(0, n)))
                oy.append(int(rng.integers(0, h - qh + 1)))
                ox.append(int(rng.integers(0, w - qw + 1)))
        rows.append((cy, cx, src, oy, ox))
    return _records(rows)


def _call(x_u32, records, shift=0, src_shift=0):
    """y3_mosaic_batch into a canary-filled buffer, `out` starting `shift` words past the front guard and `src` `src_shift` words
    into its allocation -> (rc, out words, whether the guards and the slack are untouched)."""
    from yolo3._hip import lib
    n, c, h, w = x_u32.shape
    total = x_u32.size
    src = torch.zeros(total + 4, dtype=torch.int32, device='cuda')
    src[src_shift:src_shift + total] = torch.from_numpy(np.ascontiguousarray(x_u32).reshape(-1).view(np.int32)).cuda()
    buf = torch.full((GUARD + total + 4 + GUARD,), CANARY - 2 ** 32, dtype=torch.int32, device='cuda')
    recs = np.ascontiguousarray(records)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.y3_mosaic_batch(src.data_ptr() + 4 * src_shift, n, c, h, w, recs.ctypes.data, buf.data_ptr() + 4 * (GUARD + shift), st)
    torch.cuda.synchronize()
    words = buf.cpu().numpy().view(np.uint32)
    lo, hi = GUARD + shift, GUARD + shift + total
    clean = bool((words[:lo] == CANARY).all() and (words[hi:] == CANARY).all())
    return rc, words[lo:hi].reshape(x_u32.shape), clean


def _check(x, records, **kw):
    from yolo3 import augment
    rc, got, clean = _call(x, records, **kw)
    assert rc == 0, rc
    want = augment.mosaic_reference(x, records)
    assert clean, 'words outside out were written'
    assert np.array_equal(got, want), '%d words differ' % int((got != want).sum())


SHAPES = [(1, 1, 1, 1), (1, 3, 7, 33), (2, 1, 3, 1100), (5, 3, 32, 64), (4, 3, 96, 96), (8, 3, 64, 64)]


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_every_seam_position(shape):
    """cx in {0, 1, 2, 3, w-1, w} x cy in {0, 1, h-1, h}: every combination of empty quadrants, spans shorter than one 16-byte
    group, random sources and windows; `out` at each of the four word offsets of a 16-byte group, `src` likewise."""
    n, c, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x = _bits(rng, shape)
    k = 0
    for cy in sorted({v for v in (0, 1, h - 1, h) if 0 <= v <= h}):
        for cx in sorted({v for v in (0, 1, 2, 3, w - 1, w) if 0 <= v <= w}):
            _check(x, _random_records(rng, n, h, w, cy, cx), shift=k % 4, src_shift=(k // 4) % 4)
            k += 1
    assert k >= (4 if h == 1 else 12)


def test_kernel_every_source_shift_mod_4():
    """(ox - qx) mod 4 takes all four values on both sides of the seam, with the destination 16-byte aligned."""
    n, c, h, w = 4, 3, 32, 64
    rng = np.random.default_rng(1)
    x = _bits(rng, (n, c, h, w))
    seen = set()
    for cx in (20, 21, 22, 23):
        for d in range(4):
            rows = [(13, cx, [(i + 1) % n, (i + 2) % n, (i + 3) % n, i], [3, 0, 7, 1], [d, (d + 1) % 4, (d + 2) % 4, (d + 3) % 4]) for i in range(n)]
            recs = _records(rows)
            seen.update(('left', (d + q) % 4) for q in (0, 2))
            seen.update(('right', ((d + q) % 4 - cx) % 4) for q in (1, 3))
            _check(x, recs)
    assert seen == {(side, r) for side in ('left', 'right') for r in range(4)}


def test_kernel_full_window_identity_and_aliased_sources():
    from yolo3 import augment
    n, c, h, w = 4, 3, 32, 64
    rng = np.random.default_rng(2)
    x = _bits(rng, (n, c, h, w))
    other = _records([(h, w, [(i + 1) % n, 0, 0, 0], [0] * 4, [0] * 4) for i in range(n)])          # cy = h: the whole of another image
    rc, got, clean = _call(x, other)
    assert rc == 0 and clean and np.array_equal(got, np.roll(x, -1, axis=0))
    ident = _records([(h, w, [i, 0, 0, 0], [0] * 4, [0] * 4) for i in range(n)])
    rc, got, clean = _call(x, ident)
    assert rc == 0 and clean and np.array_equal(got, x)                                              # an exact copy
    _check(x, _records([(h, 0, [0, (i + 2) % n, 0, 0], [0] * 4, [0] * 4) for i in range(n)]))         # cx = 0: quadrant 1 is everything
    _check(x, _records([(11, 27, [2, 2, 2, 2], [5, 21, 0, 3], [30, 1, 9, 27]) for i in range(n)]))   # all four quadrants read image 2
    # the wrapper: a new tensor on the current stream, the input untouched
    from yolo3.imagereader import mosaic_device
    recs = augment.draw_mosaic(3, 0, 0, n, (h, w), 1.0)
    xd = _to_dev(x)
    yd = mosaic_device(xd, recs)
    assert yd.data_ptr() != xd.data_ptr() and yd.shape == xd.shape and yd.dtype == torch.float32
    assert np.array_equal(_to_u32(yd), augment.mosaic_reference(x, recs)) and np.array_equal(_to_u32(xd), x)


def test_kernel_sources_across_the_chunk_boundary():
    """33 images of 1 x 8 x 8: the records travel 32 per launch; output 0 reads image 32 and output 32 reads image 0."""
    n = 33
    rng = np.random.default_rng(3)
    x = _bits(rng, (n, 1, 8, 8))
    rows = [(3, 5, [(i + 32) % n, (i + 1) % n, (32 - i) % n, i], [1, 2, 0, 3], [0, 4, 2, 1]) for i in range(n)]
    assert rows[0][2][0] == 32 and rows[32][2][2] == 0
    _check(x, _records(rows))
    _check(x, _records(rows), shift=3, src_shift=1)


def test_validation_refuses_before_any_launch():
    """Every rule of the header: Y3_EINVAL, a message, and the canary-filled out untouched."""
    from yolo3._hip import lib
    n, c, h, w = 3, 3, 8, 12
    rng = np.random.default_rng(4)
    x = _bits(rng, (n, c, h, w))
    good = (4, 6, [0, 1, 2, 0], [1, 2, 3, 4], [0, 1, 2, 6])
    _check(x, _records([good] * n))

    def refused(records, what, xs=x):
        rc, got, clean = _call(xs, records)
        msg = lib.y3_last_error().decode()
        assert rc == -1 and msg.startswith('mosaic_batch') and what in msg, (what, rc, msg)
        assert clean and (got == CANARY).all(), what

    def one_bad(rec):
        return _records([good, rec, good])

    for cy, cx in ((-1, 6), (9, 6), (4, -1), (4, 13)):
        refused(one_bad((cy, cx, [0, 1, 2, 0], [0] * 4, [0] * 4)), 'seam')
    for q in range(4):
        for bad in (-1, n):
            src = [0, 1, 2, 0]
            src[q] = bad
            refused(one_bad((4, 6, src, good[3], good[4])), 'source image')
        for field, v in ((3, -1), (3, 5), (4, -1), (4, 7)):          # oy < 0, oy + 4 > 8, ox < 0, ox + 6 > 12
            rec = [4, 6, [0, 1, 2, 0], list(good[3]), list(good[4])]
            rec[field][q] = v
            refused(one_bad(tuple(rec)), 'window')
    # an empty quadrant's fields are ignored, however wrong
    _check(x, one_bad((8, 12, [1, -7, 99, n], [0, -3, 50, 9], [0, 80, -1, 13])))
    r = one_bad(good)
    r['reserved'][1, 1] = 1
    refused(r, 'reserved')
    r = _records([good] * 2)
    refused(r, 'channels', xs=_bits(rng, (2, 2, 8, 12)))             # c = 2
    # bad n / h / w and null pointers: nothing to launch into, so straight at the entry point
    buf = torch.full((64,), CANARY - 2 ** 32, dtype=torch.int32, device='cuda')
    src = torch.zeros(64, dtype=torch.float32, device='cuda')
    rec1 = _records([(1, 1, [0] * 4, [0] * 4, [0] * 4)])
    st = torch.cuda.current_stream().cuda_stream
    for args in ((0, 1, 1, 1), (-1, 1, 1, 1), (1, 1, 0, 1), (1, 1, 1, -2), (1, 4, 1, 1)):
        assert lib.y3_mosaic_batch(src.data_ptr(), *args, rec1.ctypes.data, buf.data_ptr(), st) == -1 and lib.y3_last_error()
    assert lib.y3_mosaic_batch(None, 1, 1, 1, 1, rec1.ctypes.data, buf.data_ptr(), st) == -1 and b'null' in lib.y3_last_error()
    assert lib.y3_mosaic_batch(src.data_ptr(), 1, 1, 1, 1, None, buf.data_ptr(), st) == -1 and b'null' in lib.y3_last_error()
    # overlapping ranges: in place, out starting inside src, src starting inside out; adjacent ranges are fine
    both = torch.full((4 * 16,), CANARY - 2 ** 32, dtype=torch.int32, device='cuda')
    rec2 = _records([(2, 2, [0, 1, 1, 0], [0] * 4, [0] * 4)] * 2)
    p = both.data_ptr()
    for s_off, o_off in ((0, 0), (0, 31), (31, 0), (0, 1)):
        assert lib.y3_mosaic_batch(p + 4 * s_off, 2, 1, 4, 4, rec2.ctypes.data, p + 4 * o_off, st) == -1
        assert b'overlap' in lib.y3_last_error()
    torch.cuda.synchronize()
    assert (both.cpu().numpy().view(np.uint32) == CANARY).all() and (buf.cpu().numpy().view(np.uint32) == CANARY).all()
    assert lib.y3_mosaic_batch(p, 2, 1, 4, 4, rec2.ctypes.data, p + 4 * 32, st) == 0
    torch.cuda.synchronize()
    w32 = both.cpu().numpy().view(np.uint32)
    assert (w32[32:] == CANARY).all() and (w32[:32] == CANARY).all()       # a copy of canaries into canaries, and nothing else moved


# ---- data plane ------------------------------------------------------------------------------------------------------------
def _make_lmdb(path, n, size, seed=3, lo=12, hi=None):
    import build_lmdb
    from yolo3 import lmdbio
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n):
        img = rng.integers(0, 256, size, dtype=np.uint8)
        k = int(rng.integers(0 if i % 4 == 3 else 1, 4))
        wh = rng.integers(lo, hi or size[0] // 2, (k, 2))
        xy = np.stack([rng.integers(0, size[1] - wh[:, 0]), rng.integers(0, size[0] - wh[:, 1])], 1) if k else np.zeros((0, 2), int)
        boxes = np.concatenate([xy, wh, rng.integers(0, 2, (k, 1))], 1).astype(np.int32)
        items.append(build_lmdb.make_record(img, boxes, i, 'img%03d' % i))
    lmdbio.write_environment(path, items)


def _take(path, nb, prefetch, mosaic, multiscale):
    """nb batches of 4 off a fresh unshuffled one-worker reader (identity augmentation records) -> NumPy, plus the reader."""
    from yolo3.imagereader import ImageReader
    rd = ImageReader(path, ANCHORS, use_augmentation=False, shuffle=False, num_workers=1, augmentation_device='gpu', label_device='gpu')
    ds = rd.get_tf_dataset().batch(4)
    if mosaic is not None:
        ds = ds.mosaic(*mosaic)
    if multiscale is not None:
        ds = ds.multiscale(*multiscale)
    if prefetch:
        ds = ds.prefetch(2)
    rd.startup()
    try:
        it = iter(ds)
        out = [[t.cpu().numpy() for t in next(it)] for _ in range(nb)]
        it.close()
    finally:
        rd.shutdown()
    assert ds.batches >= nb
    return out, rd, ds


def _expected(path, rd, ds, nb, mosaic):
    """The same batches by hand: the examples loaded here in key order, augment_device -> (mosaic_reference on the host) ->
    zscore_normalize_device, and format_boxes of (mosaic_boxes of) the boxes."""
    from yolo3 import augment, lmdbio
    from yolo3.imagereader import augment_device, zscore_normalize_device, format_boxes
    crop = tuple(rd.image_size[:2])
    with lmdbio.Environment(path) as env:
        ex = [rd.load_example(rd.keys_flat[i % len(rd.keys_flat)], env) for i in range(4 * nb)]
    out = []
    for b in range(nb):
        e = ex[4 * b:4 * b + 4]
        size = ds.size_of_batch(b)
        recs = augment.rescale_record(np.concatenate([v[2] for v in e]), crop, size)
        boxes = [augment.scale_boxes(v[1], crop, size) for v in e]
        imgs = augment_device(torch.from_numpy(np.stack([v[0] for v in e])).cuda(), recs, size)
        if mosaic is not None:
            mrec = augment.draw_mosaic(mosaic[1], rd.shard_index, b, 4, size, mosaic[0])
            imgs = torch.from_numpy(augment.mosaic_reference(imgs.cpu().numpy(), mrec)).cuda()
            boxes = augment.mosaic_boxes(boxes, mrec, size, mosaic[2])
        labs = [format_boxes(bx if len(bx) else None, size + (3,), ANCHORS, rd.number_classes) for bx in boxes]
        out.append([zscore_normalize_device(imgs).cpu().numpy()] + [np.stack([l[s] for l in labs]) for s in range(3)])
    return out


def _same_batches(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 4
        for t, (a, e) in enumerate(zip(g, w)):
            assert a.shape == e.shape and a.dtype == e.dtype == np.float32, (b, t, a.shape, e.shape)
            assert np.array_equal(a.view(np.uint32), e.view(np.uint32)), 'batch %d tensor %d: %d words differ' % (
                b, t, int((a.view(np.uint32) != e.view(np.uint32)).sum()))


@pytest.fixture(scope='module')
def lmdb64(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('mosaic') / 'train-syn.lmdb')
    _make_lmdb(path, 12, (64, 64, 3))
    return path


@pytest.mark.parametrize('prefetch', [False, True])
@pytest.mark.parametrize('multi', [False, True])
def test_dataset_mosaic_end_to_end(lmdb64, prefetch, multi):
    """Dataset.mosaic(1.0, seed): images bit-identical to zscore(mosaic_reference(augment_device(...))), labels to
    format_boxes(mosaic_boxes(...)); with multiscale at both of its sizes."""
    from yolo3 import augment
    mosaic = (1.0, 5, 0.25)
    multiscale = ([(64, 64), (96, 96)], 1, 1) if multi else None
    got, rd, ds = _take(lmdb64, 2, prefetch, mosaic, multiscale)
    sizes = [tuple(g[0].shape[2:]) for g in got]
    assert sizes == ([(64, 64), (96, 96)] if multi else [(64, 64)] * 2)
    _same_batches(got, _expected(lmdb64, rd, ds, 2, mosaic))
    plain = _expected(lmdb64, rd, ds, 2, None)
    assert not np.array_equal(got[0][0], plain[0][0])                      # it is a mosaic, and boxes moved with it
    assert any(not np.array_equal(g[3], p[3]) for g, p in zip(got, plain)) and any(g[3].any() for g in got)
    assert all(not augment._is_identity(r, i, 64, 64) for i, r in enumerate(augment.draw_mosaic(5, 0, 0, 4, (64, 64), 1.0)))


def test_dataset_mosaic_repeats_and_defaults_are_untouched(lmdb64):
    """Two runs with one seed repeat bit for bit, another seed gives other batches; without .mosaic() the batches are those of
    the chain augment_device -> zscore_normalize_device (what this path launched before the option existed)."""
    a, rd, ds = _take(lmdb64, 2, True, (1.0, 5, 0.25), None)
    b, _, _ = _take(lmdb64, 2, False, (1.0, 5, 0.25), None)
    _same_batches(a, b)
    c, _, _ = _take(lmdb64, 1, False, (1.0, 6, 0.25), None)
    assert not np.array_equal(a[0][0], c[0][0])
    for prefetch in (False, True):
        got, rd, ds = _take(lmdb64, 2, prefetch, None, None)
        assert ds.mosaic_cfg is None
        _same_batches(got, _expected(lmdb64, rd, ds, 2, None))


def test_mosaic_grows_the_box_count_past_the_prefetch_buffer(lmdb64):
    """One output image takes the boxes of four inputs: more than the batch's own maximum, which sized the pinned buffer."""
    from yolo3 import augment
    from yolo3.imagereader import ImageReader, collate_boxes
    rd = ImageReader(lmdb64, ANCHORS, use_augmentation=False, shuffle=False, num_workers=1, augmentation_device='gpu', label_device='gpu')
    ds = rd.get_tf_dataset().batch(4).mosaic(1.0, 0, min_visible=0.0)
    size = (64, 64)
    big = [np.array([[0, 0, 64, 64, 0], [0, 0, 64, 64, 1]], np.int32)] * 4      # whole-image boxes: every quadrant keeps both
    boxes, counts = collate_boxes(big)
    pinned = (torch.from_numpy(boxes).pin_memory(), torch.from_numpy(counts).pin_memory())
    imgs = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (4, 64, 64, 3), dtype=np.uint8)).cuda()
    recs = np.concatenate([augment.identity_record((64, 64, 3), size) for _ in range(4)])
    out = ds._device_batch(torch.device('cuda', torch.cuda.current_device()), imgs, recs, *pinned)
    torch.cuda.synchronize()
    assert np.array_equal(pinned[0].numpy(), boxes) and np.array_equal(pinned[1].numpy(), counts)      # the inputs were not written
    mrec = augment.draw_mosaic(0, 0, 0, 4, size, 1.0)
    moved = augment.mosaic_boxes(big, mrec, size, 0.0)
    assert max(len(m) for m in moved) == 8 > boxes.shape[1]
    from yolo3.imagereader import format_boxes
    labs = [format_boxes(m, size + (3,), ANCHORS, rd.number_classes) for m in moved]
    for s in range(3):
        assert np.array_equal(out[1 + s].cpu().numpy(), np.stack([l[s] for l in labs]))


def test_training_step_on_a_mosaic_batch(lmdb64):
    from yolo3.model import YoloV3
    from yolo3.imagereader import ImageReader
    rd = ImageReader(lmdb64, ANCHORS, use_augmentation=True, shuffle=False, num_workers=1, augmentation_device='gpu', label_device='gpu')
    ds = rd.get_tf_dataset().batch(4).mosaic(1.0, 2)
    rd.startup()
    try:
        it = iter(ds)
        batch = next(it)
        it.close()
    finally:
        rd.shutdown()
    assert tuple(batch[0].shape) == (4, 3, 64, 64) and bool(torch.isfinite(batch[0]).all()) and float(batch[3][..., 4].sum()) > 0
    yolo = YoloV3(4, [64, 64, 3], rd.number_classes, ANCHORS, learning_rate=1e-4)
    loss = float(yolo.train_step((batch[0], list(batch[1:]))))
    torch.cuda.synchronize()
    assert np.isfinite(loss) and loss > 0
    assert bool(torch.isfinite(yolo.grads).all()) and float(yolo.grads.abs().sum()) > 0


def test_cli_mosaic_training(tmp_path):
    """train.py --augmentation_device gpu --mosaic_prob 1.0 for one epoch on a tiny database: the configuration line, finite
    losses, an export at the stored size."""
    tmp = str(tmp_path)
    for split, cnt, seed in (('train', 8, 5), ('test', 3, 6)):
        _make_lmdb(os.path.join(tmp, '%s-syn.lmdb' % split), cnt, (64, 64, 3), seed=seed, lo=16, hi=32)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = os.path.join(tmp, 'out')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--batch_size', '4', '--test_every_n_steps', '5', '--train_database',
                        os.path.join(tmp, 'train-syn.lmdb'), '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out,
                        '--early_stopping', '1', '--use_augmentation', '1', '--augmentation_device', 'gpu', '--max_epochs', '1', '--reader_count', '1',
                        '--mosaic_prob', '1.0', '--mosaic_seed', '3', '--learning_rate', '1e-4'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Mosaic augmentation: probability 1 per image, four images of the batch per mosaic (seed 3)' in r.stdout
    train = [ln.split(',') for ln in open(glob.glob(os.path.join(out, 'scalars-*', 'train.csv'))[0]).read().split()][1:]
    assert len(train) == 6 and all(np.isfinite(float(v)) for row in train for v in row[1:])
    losses = [float(v) for v in open(os.path.join(out, 'test_loss.csv')).read().split()]
    assert len(losses) == 1 and np.isfinite(losses[0])
    z = np.load(os.path.join(out, 'saved_model', 'yolov3.npz'))
    assert z['meta_img_size'].tolist() == [64, 64, 3]
