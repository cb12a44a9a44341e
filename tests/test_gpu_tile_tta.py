"""Tile test-time augmentation on the device: y3_tile_gather_zscore_views_nhwc against both compositions it
replaces, y3_tile_merge_voted against the NumPy restatement of tests/tile_tta_reference.py, YoloV3.predict_tiles_tta against
predict_tta, inference_image_tiled / evaluate_tiled under tile_tta end to end, and the command lines.  Every comparison is bit for
bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inference_tiled as it
import tile_merge_reference as tm
import tile_tta_reference as tt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
E = it.EDGE_EFFECT_RANGE
TILE = (256, 256)
D4_SHUFFLED = (6, 0, 3, 5, 1, 7, 2, 4)
CANARY = 0x7fc5a5a5          # a NaN with a payload: any arithmetic on it, or any store over it, shows
PAD = 64                     # canary words in front of and behind `out` (256 bytes: out stays 16-byte aligned)
CODES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the gather kernel ---------------------------------------------------------------------------------------------------
def _image(seed, h, w, c, dtype):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        return rng.uniform(-1e3, 1e3, (h, w, c)).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, (h, w, c)).astype(dtype)


def _dev_image(img):
    return torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img).cuda()


def _gather_views(img_dev, img, table_dev, n, th, tw, views, pitch):
    """One y3_tile_gather_zscore_views_nhwc launch between canaries -> int32 CUDA tensor [n * k, th, tw, pitch] of the raw bits."""
    from yolo3 import _hip
    h, w, c = img.shape
    k = len(views)
    words = n * k * th * tw * pitch
    buf = torch.from_numpy(np.full(words + 2 * PAD, CANARY, np.uint32).view(np.int32)).cuda()
    ws = torch.empty(int(_hip.lib.y3_zscore_workspace_bytes(n)) // 8 + 1, dtype=torch.float64, device='cuda')
    _hip.check(_hip.lib.y3_tile_gather_zscore_views_nhwc(img_dev.data_ptr(), CODES[img.dtype], h, w, c, table_dev.data_ptr(), n, th, tw,
                                                         _hip.int_array(views), k, buf.data_ptr() + 4 * PAD, pitch, ws.data_ptr(), _st()),
               'y3_tile_gather_zscore_views_nhwc')
    canary = torch.tensor(CANARY, dtype=torch.int32, device='cuda')
    assert bool((buf[:PAD] == canary).all()) and bool((buf[-PAD:] == canary).all()), 'a canary word was overwritten'
    return buf[PAD:-PAD].view(n * k, th, tw, pitch)


def _composition_a(img_dev, img, table_dev, n, th, tw, views, pitch):
    """y3_tile_gather_zscore_nhwc, permuted with torch: transpose first, then flip x, then flip y."""
    from yolo3 import _hip
    h, w, c = img.shape
    base = torch.empty(n, th, tw, pitch, dtype=torch.float32, device='cuda')
    ws = torch.empty(int(_hip.lib.y3_zscore_workspace_bytes(n)) // 8 + 1, dtype=torch.float64, device='cuda')
    _hip.check(_hip.lib.y3_tile_gather_zscore_nhwc(img_dev.data_ptr(), CODES[img.dtype], h, w, c, table_dev.data_ptr(), n, th, tw, base.data_ptr(),
                                                   pitch, ws.data_ptr(), _st()), 'y3_tile_gather_zscore_nhwc')
    base = base.view(torch.int32)
    out = []
    for t in range(n):
        for code in views:
            v = base[t]
            if code & 4:
                v = v.transpose(0, 1)
            if code & 1:
                v = v.flip(1)
            if code & 2:
                v = v.flip(0)
            out.append(v)
    return torch.stack(out).contiguous()


def _composition_b(img_dev, img, table_dev, n, th, tw, views, pitch):
    """y3_tile_gather -> y3_zscore -> y3_tta_views_nhwc."""
    from yolo3 import _hip, imagereader
    h, w, c = img.shape
    k = len(views)
    tiles = torch.empty(n, c, th, tw, dtype=torch.float32, device='cuda')
    _hip.check(_hip.lib.y3_tile_gather(img_dev.data_ptr(), CODES[img.dtype], h, w, c, table_dev.data_ptr(), n, th, tw, tiles.data_ptr(), _st()),
               'y3_tile_gather')
    z = imagereader.zscore_normalize_device(tiles)
    out = torch.full((n * k, th, tw, pitch), 7.0, dtype=torch.float32, device='cuda')
    _hip.check(_hip.lib.y3_tta_views_nhwc(z.data_ptr(), n, c, th, tw, _hip.int_array(views), k, _hip.Tensor(out.data_ptr(), n * k, th, tw, pitch, pitch),
                                          _st()), 'y3_tta_views_nhwc')
    return out.view(torch.int32)


def _check_gather(img, table, th, tw, views, pitch):
    h, w, _ = img.shape
    assert np.all(table[:, [0, 3]] >= 0) and np.all(table[:, [1, 4]] >= 1) and np.all(table[:, [2, 5]] >= 0)
    assert np.all(table[:, 0] + table[:, 1] <= h) and np.all(table[:, 3] + table[:, 4] <= w)          # every crop lies inside the image
    n = table.shape[0]
    img_dev, table_dev = _dev_image(img), torch.from_numpy(table).cuda()
    got = _gather_views(img_dev, img, table_dev, n, th, tw, views, pitch)
    a = _composition_a(img_dev, img, table_dev, n, th, tw, views, pitch)
    b = _composition_b(img_dev, img, table_dev, n, th, tw, views, pitch)
    assert got.shape == a.shape == b.shape
    assert torch.equal(got, a), ('composition a', th, tw, views, pitch, img.dtype)
    assert torch.equal(got, b), ('composition b', th, tw, views, pitch, img.dtype)
    again = _gather_views(img_dev, img, table_dev, n, th, tw, views, pitch)
    assert torch.equal(got, again)
    return got


SHAPES = [(32, 32, D4_SHUFFLED), (33, 33, D4_SHUFFLED), (40, 40, D4_SHUFFLED), (96, 96, D4_SHUFFLED), (40, 72, (0, 1, 2, 3)), (40, 72, (3, 0)),
          (40, 40, (0,)), (40, 72, (3,))]
PARAMS = [(np.uint8, 3, 4), (np.uint8, 1, 4), (np.uint8, 3, 8), (np.uint16, 3, 4), (np.float32, 3, 4), (np.float32, 1, 4)]


@pytest.mark.parametrize('th,tw,views', SHAPES)
def test_gather_views_equals_both_compositions(th, tw, views):
    """32 and 96: whole 32 x 32 blocks; 33: one pixel into a second block; 40 and 40 x 72: ragged last blocks in both directions,
    under straight and transposing views.  Tables with clamped edge tiles (reflected rows and columns in front and behind)."""
    for dtype, c, pitch in PARAMS:
        img = _image(th * 3 + tw + c + pitch, 100, 130, c, dtype)
        got = _check_gather(img, tt.gather_tables(th, tw, 100, 130), th, tw, views, pitch)
        body = got.view(torch.float32)
        assert not bool(body[..., c:].view(torch.int32).any())                     # the floats of a pixel beyond the channels are zero
        assert float(body[..., :c].abs().max()) > 0.5 and len(views) == got.shape[0] // 5
    if len(views) > 1:      # the views really differ: the comparison is not between copies of view 0
        assert not torch.equal(got[0], got[1])


@pytest.mark.parametrize('th,tw,views', [(96, 96, D4_SHUFFLED), (40, 72, (3, 0)), (33, 33, (5, 2))])
def test_gather_views_of_an_image_smaller_than_the_tile(th, tw, views):
    """20 x 25 under tiles of up to 96: the reflection wraps more than once, behind the crop and (pre 50 / 60) in front of it."""
    for dtype in (np.uint8, np.float32):
        img = _image(th + tw, 20, 25, 3, dtype)
        table = np.concatenate([tt.gather_tables(th, tw, 20, 25), np.array([[0, 20, 50, 0, 25, 60], [7, 1, 0, 3, 1, 0]], np.int32)])
        _check_gather(img, table, th, tw, views, 4)


def test_gather_views_of_a_constant_tile_subtracts_only():
    """std 0 (and std <= 1): the subtract-only branch; every value is exactly 0, or pixel - mean."""
    img = np.full((100, 130, 3), 7, np.uint8)
    got = _check_gather(img, tt.gather_tables(40, 40, 100, 130), 40, 40, D4_SHUFFLED, 4)
    assert not bool(got.any())
    img = (np.indices((100, 130)).sum(0) % 2).astype(np.uint8)[:, :, None].repeat(3, 2)       # a checkerboard of 0 / 1: std 0.5
    got = _check_gather(img, tt.gather_tables(40, 40, 100, 130), 40, 40, (0, 4, 1), 4).view(torch.float32)
    assert set(np.unique(got[..., :3].cpu().numpy()).tolist()) == {-0.5, 0.5}


# ---- 2. the voted merge -----------------------------------------------------------------------------------------------------
def _merge_voted(b, img, margin, cap=None, splits=None, voted=None):
    """A voted_batch through TilePool / merge_tiles_device(voted=...) in the given tile ranges -> (float64 [M, 6], pool)."""
    from yolo3 import bbox_utils
    v, keep_idx, keep_cnt, table = (torch.from_numpy(a).cuda() for a in b[:4])
    n, K, nb = keep_idx.shape
    rows = torch.zeros(n, nb, 5 + K, device='cuda')                      # never read on the voted path: only its shape is
    score = torch.zeros(n, K, nb, device='cuda')
    kw = {} if cap is None else {'cap': cap}
    pool = bbox_utils.TilePool(TILE, img, margin, E, **kw)
    for a, e in (splits or [(0, n)]):
        bbox_utils.merge_tiles_device(pool, rows[a:e].contiguous(), keep_idx[a:e].contiguous(), keep_cnt[a:e].contiguous(), score[a:e].contiguous(),
                                      table[a:e].contiguous(), voted=v[a:e].contiguous())
    out, m = pool.finish()
    assert out.shape == (m, 6)
    return out.cpu().numpy().astype(np.float64), pool


def _want_voted(b, img, margin, tiles=slice(None)):
    voted, keep_idx, keep_cnt, table, xs, ys = b
    return tt.voted_pool(voted[tiles], keep_idx[tiles], keep_cnt[tiles], keep_idx.shape[2], xs[tiles], ys[tiles], TILE, img, margin)


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('margin', tt.MARGINS)
def test_voted_pool_matches_restatement_bit_for_bit(K, margin):
    for img in ((200, 150), (150, 760), (300, 330)):          # one tile; 1 x 12 tiles; 5 x 6 tiles
        b = tt.voted_batch(10 * K + img[0], img, TILE, K)
        want = _want_voted(b, img, margin)
        got, _ = _merge_voted(b, img, margin)
        assert got.shape == want.shape and np.array_equal(got, want), (img, got.shape, want.shape)
        assert want.shape[0] > 0 and np.any(want[:, 0] == 0) and (K == 1 or not np.any(want[:, 5] == 1))
        # less than every listed entry survived: the ghost test, the centre test and the range check of keep_idx all decided
        assert want.shape[0] < int(b[2].sum())
    if K == 3:      # a row kept under two classes with different voted boxes gives two different pool rows
        one = tt.voted_batch(31, (200, 150), TILE, K)
        got, _ = _merge_voted(one, (200, 150), margin)
        assert one[1][0, 0, 0] == one[1][0, 2, 0] == 5
        assert [100, 100, 130, 140] in got[got[:, 5] == 0][:, 0:4].tolist() and [104, 98, 131, 139] in got[got[:, 5] == 2][:, 0:4].tolist()


def test_voted_batches_append_in_order_and_the_pool_retries():
    img = (300, 330)
    b = tt.voted_batch(11, img, TILE, 3)
    want = _want_voted(b, img, 8.0)
    for splits in ([(0, 13), (13, 30)], [(0, 1), (1, 2), (2, 30)]):
        got, _ = _merge_voted(b, img, 8.0, splits=splits)
        assert np.array_equal(got, want), splits
    got, _ = _merge_voted(b, img, 8.0, splits=[(13, 30), (0, 13)])
    assert np.array_equal(got, np.concatenate([_want_voted(b, img, 8.0, slice(13, 30)), _want_voted(b, img, 8.0, slice(0, 13))]))
    assert not np.array_equal(got, want)
    # a pool too small: nothing is written past cap, the counts are, and finish() merges the retained voted arrays again
    total = want.shape[0]
    for cap in (3, total - 1, total):
        got, pool = _merge_voted(b, img, 8.0, cap=cap, splits=[(0, 13), (13, 30)])
        assert np.array_equal(got, want) and pool.cap == max(cap, total), cap


def test_voted_filled_from_the_rows_is_tile_merge_byte_for_byte():
    from yolo3 import _hip
    rng = np.random.default_rng(3)
    img, K, nb = (300, 330), 3, 120
    b = tt.voted_batch(17, img, TILE, K, nb)
    keep_idx, keep_cnt, table = b[1], b[2], b[3]
    n = keep_idx.shape[0]
    rows = rng.uniform(-30, 290, (n, nb, 5 + K)).astype(np.float32)
    rows[:, :, 2:4] = rows[:, :, 0:2] + rng.choice(np.array([8.0, 16.5, 31.25], np.float32), (n, nb, 2))
    keep_score = rng.uniform(0.1, 1, (n, K, nb)).astype(np.float32)
    voted = tt.voted_from_rows(rows, keep_idx, keep_cnt, keep_score)
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(rows=rows, idx=keep_idx, cnt=keep_cnt, score=keep_score, table=table, voted=voted).items()}
    wsb = int(_hip.lib.y3_tile_merge_workspace_bytes(n, K))
    ws = torch.empty(wsb // 4, dtype=torch.int32, device='cuda')
    cap, pools = 4096, []
    for use_voted in (False, True):
        pool = torch.full((cap, 6), -7.0, dtype=torch.float32, device='cuda')
        count = torch.zeros(2, dtype=torch.int32, device='cuda')
        tail = (dev['table'].data_ptr(), TILE[0], TILE[1], img[0], img[1], E, 8.0, pool.data_ptr(), cap, count.data_ptr(), ws.data_ptr(),
                wsb, _st())
        if use_voted:
            _hip.check(_hip.lib.y3_tile_merge_voted(dev['voted'].data_ptr(), n, nb, K, dev['idx'].data_ptr(), dev['cnt'].data_ptr(), nb, *tail),
                       'y3_tile_merge_voted')
        else:
            _hip.check(_hip.lib.y3_tile_merge(dev['rows'].data_ptr(), n, nb, 5 + K, K, dev['idx'].data_ptr(), dev['cnt'].data_ptr(),
                                              dev['score'].data_ptr(), nb, *tail), 'y3_tile_merge')
        pools.append((pool.cpu().numpy(), count.cpu().tolist()))
    assert pools[0][1] == pools[1][1] and 0 < pools[0][1][0] == pools[0][1][1] < cap
    assert pools[0][0].tobytes() == pools[1][0].tobytes()
    assert np.array_equal(pools[1][0][:pools[1][1][0]].astype(np.float64), tt.voted_pool(voted, keep_idx, keep_cnt, nb, b[4], b[5], TILE, img, 8.0))


# ---- 3. predict_tiles_tta ---------------------------------------------------------------------------------------------------
ANCHORS = [(48, 48), (90, 60), (60, 90)]


@functools.lru_cache(maxsize=None)
def _yolo():
    from yolo3.model import YoloV3
    return YoloV3(4, [256, 256, 3], 2, ANCHORS, seed=7)


@functools.lru_cache(maxsize=None)
def _scene():
    """(image 500 x 700 x 3 uint8, its tile table, xs, ys)."""
    img = np.random.default_rng(1).integers(0, 256, (500, 700, 3), dtype=np.uint8)
    return (img,) + it.tile_table(500, 700, TILE)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('name,count', [('flips', 4), ('d4', 2)])
def test_predict_tiles_tta_is_predict_tta_on_the_gathered_tiles(name, count, precision):
    from yolo3 import bbox_utils, imagereader
    yolo = _yolo()
    img, table, xs, ys = _scene()
    views = bbox_utils.TTA_VIEWS[name]
    img_dev, table_dev = torch.from_numpy(img).cuda(), torch.from_numpy(table).cuda()
    t0 = 9                                                              # tiles of the second row: interior and right-edge ones
    got = yolo.predict_tiles_tta(img_dev, 0, img.shape, table_dev.data_ptr() + 24 * t0, count, views, tile_size=TILE, precision=precision).clone()
    x = imagereader.zscore_normalize_device(it.tiles_to_device(img_dev, 0, img.shape, table_dev, t0, count, TILE))
    want = yolo.predict_tta(x, views, precision=precision)
    assert got.shape == want.shape and got.shape[0] == count and got.shape[1] % len(views) == 0 and got.shape[2] == 7
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(got).all()) and not torch.equal(got[0], got[1])
    with pytest.raises(ValueError):
        yolo.predict_tiles_tta(img_dev, 0, img.shape, table_dev.data_ptr(), count, views, tile_size=(256, 320))


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model():
    return _yolo().get_keras_model()


def _oracle(nms, vote_iou, score, group=4, min_box=8):
    """The pipeline restated from its parts, the tiles grouped as the pipeline groups them (batch_size 16 / 4 views = 4 per call)."""
    from yolo3 import bbox_utils, imagereader
    yolo = _yolo()
    img, table, xs, ys = _scene()
    views = bbox_utils.TTA_VIEWS['flips']
    img_dev, table_dev = torch.from_numpy(img).cuda(), torch.from_numpy(table).cuda()
    bl, sl, ll = [], [], []
    for b0 in range(0, len(xs), group):
        nb = min(group, len(xs) - b0)
        x = imagereader.zscore_normalize_device(it.tiles_to_device(img_dev, 0, img.shape, table_dev, b0, nb, TILE))
        rows = yolo.predict_tta(x, views).clone()
        for k, (boxes, scores, labels, _) in enumerate(bbox_utils.detect_tta(rows, len(views), min_box, method=nms, vote_iou=vote_iou, score=score)):
            if boxes is None:
                continue
            r = it.merge_tile_detections(boxes, scores, labels, xs[b0 + k], ys[b0 + k], TILE, img.shape)
            if r is not None:
                bl.append(r[0])
                sl.append(r[1])
                ll.append(r[2])
    return it.finalize_predictions(bl, sl, ll, img.shape)


@functools.lru_cache(maxsize=None)
def _plain():
    """The image without tile TTA, at the parent's call signature."""
    return it.inference_image_tiled(_model(), _scene()[0], list(TILE), 8, 16)


@pytest.mark.parametrize('nms', ['hard', 'soft-linear'])
@pytest.mark.parametrize('vote', [False, True])
def test_inference_image_tiled_with_tile_tta_is_the_oracle(vote, nms):
    img = _scene()[0]
    kw = dict(tta_vote_iou=0.5, tta_score='consensus') if vote else {}
    want = _oracle(nms, 0.5 if vote else None, 'consensus' if vote else 'keep')
    host = it.inference_image_tiled(_model(), img, list(TILE), 8, batch_size=16, nms=nms, tile_tta='flips', **kw)
    assert host.dtype == want.dtype == np.float64 and want.shape[0] > 0
    assert host.shape == want.shape and np.array_equal(host, want)
    dev = it.inference_image_tiled(_model(), img, list(TILE), 8, batch_size=16, nms=nms, tile_tta='flips', merge_device='gpu', **kw)
    assert np.array_equal(dev, host)
    # not vacuous: the views add detections or move them, and voting changes boxes or scores once more
    plain = _plain() if nms == 'hard' else it.inference_image_tiled(_model(), img, list(TILE), 8, 16, nms)
    assert plain.shape[0] > 0 and not (host.shape == plain.shape and np.array_equal(host, plain))
    if vote:
        unvoted = it.inference_image_tiled(_model(), img, list(TILE), 8, batch_size=16, nms=nms, tile_tta='flips')
        assert not (unvoted.shape == host.shape and np.array_equal(unvoted, host))
    # the seam margin and the merge NMS work on top as they do on plain tiles
    seam = it.inference_image_tiled(_model(), img, list(TILE), 8, batch_size=16, nms=nms, tile_tta='flips', merge_device='gpu', seam_margin=8,
                                    merge_nms='hard', **kw)
    pool = it.tiled_pool_device(_model(), img, list(TILE), 8, 16, nms, 0.5, 8.0, 'flips', kw.get('tta_vote_iou'), kw.get('tta_score', 'keep'))
    p = pool[0].cpu().numpy()
    assert pool[1] == p.shape[0] >= dev.shape[0] and pool[2] == 2
    assert np.array_equal(seam, tm.gather_kept(p, tm.nms_labelled(p, 2, 'hard')).astype(np.float64)) and 0 < seam.shape[0] <= p.shape[0]


# ---- 5. defaults ------------------------------------------------------------------------------------------------------------
class _Recorder:
    """The model with every run_tiles call's keywords recorded."""
    supports_slots = True

    def __init__(self, model):
        self._m, self._y, self._fm, self.calls, self.counts = model, model._y, model._fm, [], []

    def __call__(self, *a, **kw):
        return self._m(*a, **kw)

    def run_tiles(self, *a, **kw):
        self.calls.append((len(a), sorted(kw)))
        self.counts.append(int(a[4]))
        return self._m.run_tiles(*a, **kw)


def test_defaults_launch_what_they_launched(monkeypatch):
    from yolo3 import _hip
    img = _scene()[0]
    seen = []
    for name in ('y3_tile_gather_zscore_views_nhwc', 'y3_tile_merge_voted'):
        real = getattr(_hip.lib, name)
        monkeypatch.setattr(_hip.lib, name, lambda *a, _n=name, _r=real: (seen.append(_n), _r(*a))[1])
    for dev in ('cpu', 'gpu'):
        old, new = _Recorder(_model()), _Recorder(_model())
        a = it.inference_image_tiled(old, img, list(TILE), 8, 16, 'hard', 0.5, dev, 0.0, 'none', 0.5)          # the parent's signature
        b = it.inference_image_tiled(new, img, list(TILE), 8, batch_size=16, merge_device=dev, tile_tta='none', tta_vote_iou=None, tta_score='keep')
        assert a.shape[0] > 0 and np.array_equal(a, b) and np.array_equal(a, _plain())
        assert old.calls == new.calls and len(old.calls) == 6 and all(kw == ['slot', 'tile_size'] for _, kw in new.calls)
    assert seen == []
    it.inference_image_tiled(_model(), img, list(TILE), 8, batch_size=16, merge_device='gpu', tile_tta='hflip', tta_vote_iou=0.5)
    assert set(seen) == {'y3_tile_gather_zscore_views_nhwc', 'y3_tile_merge_voted'}          # the spy does see the calls when they are made


@pytest.mark.parametrize('bs', [9, 3, None])
def test_other_schedules_keep_the_views_of_a_tile_in_one_call(bs):
    """batch_size 9 under 4 views is 2 tiles per call, 3 the one-tile minimum, None the default schedule (25 inputs on the fp32
    path: 6 tiles): every tile goes through once, in order, with its views."""
    model = _Recorder(_model())
    got = it.inference_image_tiled(model, _scene()[0], list(TILE), 8, batch_size=bs, tile_tta='flips', merge_device='gpu')
    counts = model.counts
    assert got.shape[0] > 0 and sum(counts) == 88 and all(kw == ['slot', 'tile_size', 'views'] for _, kw in model.calls)
    limit = it.BATCH_SIZE if bs is None else bs
    assert all(c * 4 <= limit or c == 1 for c in counts) and max(counts) == max(1, limit // 4)


# ---- 6. the evaluator and the command lines ---------------------------------------------------------------------------------
def _evaluator_state(ev):
    return [a for a in ev.matches()] + [ev.image_counts().cpu().numpy(), ev._npos.copy(), np.array([ev.num_images])]


def test_evaluate_tiled_and_the_command_lines(tmp_path):
    from PIL import Image
    import evaluate
    from yolo3 import bbox_utils, metrics
    tmp = str(tmp_path)
    model_file = os.path.join(tmp, 'model.npz')
    _yolo().save_weights(model_file)
    img_dir, csv_dir, out_dir = os.path.join(tmp, 'imgs'), os.path.join(tmp, 'gt'), os.path.join(tmp, 'out')
    os.makedirs(img_dir)
    os.makedirs(csv_dir)
    rng = np.random.default_rng(9)
    imgs = {'a': _scene()[0], 'b': rng.integers(0, 256, (300, 420, 3), dtype=np.uint8)}
    kw = dict(tile_tta='flips', tta_vote_iou=0.5)
    thr = [0.3, 0.5]
    ev = metrics.DetectionEvaluator(2, thr)
    examples, host = [], {}
    for name in sorted(imgs):
        Image.fromarray(imgs[name]).save(os.path.join(img_dir, name + '.png'))
        pred = it.inference_image_tiled(_model(), imgs[name], list(TILE), 8, merge_device='gpu', **kw)
        host[name] = it.inference_image_tiled(_model(), imgs[name], list(TILE), 8, **kw)
        assert pred.shape[0] > 0 and np.array_equal(pred, host[name])
        g = pred[::2]                                     # ground truth: every other detection (so there are TPs) and boxes of its own
        gt = np.stack([g[:, 0], g[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1], g[:, 5]], 1).astype(np.int64)
        gt = np.concatenate([gt, [[5, 5, 40, 40, 0], [100, 200, 30, 50, 1]]])
        bbox_utils.write_boxes_from_xywhc(gt, os.path.join(csv_dir, name + '.csv'))
        ev.add_detections([pred[:, 0:4]], [pred[:, 4]], [pred[:, 5]], [gt])
        examples.append((name, imgs[name], gt))
    # in process: the evaluator's state after add_pool on the device pools is the one add_detections leaves, and evaluate_tiled
    # (its own model, loaded from the file) gives that result
    pooled = metrics.DetectionEvaluator(2, thr)
    for name, img, gt in examples:
        pool, count, K = it.tiled_pool_device(_model(), img, list(TILE), 8, **kw)
        assert K == 2
        pooled.add_pool(pool, count, gt)
    for u, v in zip(_evaluator_state(pooled), _evaluator_state(ev)):
        assert u.dtype == v.dtype and np.array_equal(u, v)
    res, count, _ = evaluate.evaluate_tiled(examples, model_file, list(TILE), 8, iou_thresholds=thr, **kw)
    assert count == 2
    want = ev.result()
    for k in ('ap', 'recall', 'tp', 'fp', 'npos'):
        assert np.array_equal(res[k], want[k], equal_nan=True), k
    assert want['tp'].sum() > 0
    # the command lines reproduce both
    want_csv, got_csv = os.path.join(tmp, 'want.csv'), os.path.join(tmp, 'got.csv')
    evaluate.write_csv(want, want_csv)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    flags = ['--tile-height', '256', '--tile-width', '256', '--min-box-size', '8', '--image-format', 'png', '--tile-tta', 'flips',
             '--tile-tta-vote-iou', '0.5']
    r = subprocess.run([sys.executable, os.path.join(PKG, 'evaluate.py'), '--saved-model-filepath', model_file, '--image-folder', img_dir,
                        '--csv-folder', csv_dir, '--tiled', '--iou-thresholds'] + [str(t) for t in thr] + ['--output-file', got_csv] + flags,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'Evaluated 2 images' in r.stdout and 'Tile TTA: flips (4 views), vote IoU 0.5, score keep' in r.stdout
    assert open(got_csv, 'rb').read() == open(want_csv, 'rb').read()
    r = subprocess.run([sys.executable, os.path.join(PKG, 'inference_tiled.py'), '--saved-model-filepath', model_file, '--image-folder', img_dir,
                        '--output-folder', out_dir] + flags, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in sorted(imgs):
        bbox_utils.write_boxes_from_ltrbpc(host[name], os.path.join(tmp, name + '.want.csv'))
        assert open(os.path.join(out_dir, name + '.csv'), 'rb').read() == open(os.path.join(tmp, name + '.want.csv'), 'rb').read(), name


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
class _NoTiles:
    supports_slots = True

    def __call__(self, batch, training=False, slot=0):
        raise AssertionError('the model must not be called')


def test_tile_tta_needs_the_fused_path():
    img = _scene()[0]
    with pytest.raises(ValueError, match='run_tiles'):
        it.inference_image_tiled(_NoTiles(), img, list(TILE), 8, tile_tta='flips')
    with pytest.raises(ValueError, match='run_tiles'):
        it.tiled_pool_device(_NoTiles(), img, list(TILE), 8, tile_tta='hflip')
    with pytest.raises(ValueError, match='run_tiles'):
        it.inference_image_tiled(_yolo().get_keras_feature_map_model(), img, list(TILE), 8, tile_tta='flips')
