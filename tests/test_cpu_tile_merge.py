"""CPU-only checks of the device tile merge: the NumPy restatement the kernels are tested against equals the
host merge at margin 0, argument and CLI errors fire before any device work, the new entry points are declared."""
import ctypes
import os
import sys

import numpy as np
import pytest

import inference_tiled as it
import tile_merge_reference as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
F = np.float32


def _tiles(rng, tile, img, per_tile=60):
    """Per tile (boxes, scores, labels) with centres on the comparison boundaries, halves on both sides of even, boxes that
    leave the image; every fourth tile empty."""
    table, xs, ys = it.tile_table(img[0], img[1], tile)
    dets = []
    for k in range(len(xs)):
        if k % 4 == 3:
            dets.append(None)
            continue
        c = np.stack([rng.uniform(-30, tile[1] + 30, per_tile), rng.uniform(-30, tile[0] + 30, per_tile)], 1).astype(np.float32)
        special_x = [96, tile[1] - 96, 96 - xs[k], img[1] - 96 - xs[k]]
        special_y = [96, tile[0] - 96, 96 - ys[k], img[0] - 96 - ys[k]]
        for i, (sx, sy) in enumerate(zip(special_x, special_y)):
            for j, d in enumerate((-1, 0, 1)):
                vx, vy = F(sx), F(sy)
                if d:
                    vx, vy = np.nextafter(vx, F(d * 1e9)), np.nextafter(vy, F(d * 1e9))
                c[(i * 3 + j) * 2, 0] = vx
                c[(i * 3 + j) * 2 + 1, 1] = vy
        half = rng.choice([4.0, 8.0, 16.0, 7.5, 12.5], (per_tile, 2)).astype(np.float32)
        b = np.concatenate([c - half, c + half], 1).astype(np.float32)
        b[40:46, 0] = np.array([10.5, 11.5, 12.5, -3.5, -2.5, 0.5], np.float32)        # .5 on either side of even
        b[46:50] += F(400)                                                            # beyond the image
        b[50:53] -= F(500)
        dets.append((b, rng.uniform(0.1, 1, per_tile).astype(np.float32), rng.integers(0, 3, per_tile).astype(np.int32)))
    return dets, xs, ys


@pytest.mark.parametrize('tile,img', [((256, 256), (200, 150)), ((256, 256), (150, 760)), ((256, 256), (300, 330)), ((224, 256), (500, 300))])
def test_restatement_at_margin_zero_is_the_host_merge(tile, img):
    rng = np.random.default_rng(tile[0] + img[1])
    dets, xs, ys = _tiles(rng, tile, img)
    want = tm.pool(dets, xs, ys, tile, img, host=True)
    got = tm.pool(dets, xs, ys, tile, img, 0.0)
    assert want.dtype == got.dtype == np.float64 and want.shape == got.shape and want.shape[0] > 0
    assert np.array_equal(want, got)
    # per tile too, None included
    for k, d in enumerate(dets):
        if d is None:
            continue
        a = it.merge_tile_detections(d[0], d[1], d[2], xs[k], ys[k], tile, img)
        b = tm.merge_tile(d[0], d[1], d[2], xs[k], ys[k], tile, img, 0.0)
        assert (a is None) == (b is None)
        if a is not None:
            assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_margin_only_adds_detections_and_keeps_their_order():
    tile, img = (256, 256), (300, 330)
    dets, xs, ys = _tiles(np.random.default_rng(5), tile, img, 80)
    prev = tm.pool(dets, xs, ys, tile, img, 0.0)
    for margin in (7.5, 95.0):
        cur = tm.pool(dets, xs, ys, tile, img, margin)
        assert cur.shape[0] > prev.shape[0]
        rows = [tuple(r) for r in cur]
        pos = -1
        for r in prev:                        # prev is a subsequence of cur
            pos = rows.index(tuple(r), pos + 1)
        prev = cur


def test_labelled_nms_restatement_by_hand():
    # class 0: two overlapping boxes (IoU 0.5) and a distant one; class 1: one box; class 2 absent
    p = np.array([[0, 0, 10, 10, 0.9, 0], [0, 0, 10, 5, 0.8, 0], [50, 50, 60, 60, 0.7, 0], [0, 0, 10, 10, 0.6, 1]], np.float32)
    none = tm.nms_labelled(p, 3, 'none')
    assert [r.tolist() for r, _ in none] == [[0, 1, 2], [3], []]
    hard = tm.nms_labelled(p, 3, 'hard')
    assert [r.tolist() for r, _ in hard] == [[0, 2], [3], []]
    soft = tm.nms_labelled(p, 3, 'soft-linear')
    assert soft[0][0].tolist() == [0, 2, 1] and np.isclose(soft[0][1][2], 0.4)
    kept = tm.gather_kept(p, soft)
    assert kept.shape == (4, 6) and kept[:, 5].tolist() == [0, 0, 0, 1] and np.isclose(kept[2, 4], 0.4)
    # equal scores: the higher row first
    q = np.array([[0, 0, 1, 1, 0.5, 0], [5, 5, 6, 6, 0.5, 0]], np.float32)
    assert tm.nms_labelled(q, 1, 'none')[0][0].tolist() == [1, 0]


def test_argument_errors():
    from yolo3 import bbox_utils
    assert bbox_utils.MERGE_NMS_METHODS == ('none',) + bbox_utils.NMS_METHODS
    img = np.zeros((300, 300, 3), np.uint8)
    bad = ({'seam_margin': 8.0}, {'merge_nms': 'hard'}, {'merge_device': 'gpu', 'seam_margin': 96.0}, {'merge_device': 'gpu', 'seam_margin': -1.0},
           {'merge_device': 'gpu', 'seam_margin': float('nan')}, {'merge_device': 'gpu', 'merge_nms': 'greedy'},
           {'merge_device': 'gpu', 'merge_nms': 'soft-gaussian', 'merge_nms_sigma': 0.0}, {'merge_device': 'tpu'})
    for kw in bad:                                   # before the model or a device is touched
        with pytest.raises(ValueError):
            it.inference_image_tiled(None, img, [256, 256], 8, **kw)
        with pytest.raises(ValueError):
            it.inference_image_folder('/nonexistent', 'png', '/nonexistent', '/nonexistent', [256, 256], 8, **kw)
    bbox_utils.check_merge_args('gpu', 95.5, 'soft-gaussian', 0.5)
    bbox_utils.check_merge_args()


def test_library_rejects_bad_arguments_before_launch():
    from yolo3 import _hip
    lib = _hip.lib
    a = 1 << 20
    ok = dict(rows=a, n=2, nb=100, ld=7, K=2, idx=2 * a, cnt=3 * a, sc=4 * a, mk=100, table=5 * a, th=256, tw=256, H=500, W=700, edge=96, margin=0.0,
              pool=6 * a, cap=64, count=7 * a, ws=8 * a, wsb=1 << 10)

    def call(**kw):
        q = dict(ok, **kw)
        return lib.y3_tile_merge(q['rows'], q['n'], q['nb'], q['ld'], q['K'], q['idx'], q['cnt'], q['sc'], q['mk'], q['table'], q['th'], q['tw'],
                                 q['H'], q['W'], q['edge'], q['margin'], q['pool'], q['cap'], q['count'], q['ws'], q['wsb'], None)
    for name in ('rows', 'idx', 'cnt', 'sc', 'table', 'pool', 'count', 'ws'):
        assert call(**{name: None}) == -1 and b'null' in lib.y3_last_error(), name
    for kw in ({'n': 0}, {'nb': 0}, {'ld': 3}, {'K': 0}, {'mk': 0}, {'cap': 0}, {'H': 0}, {'W': (1 << 24) + 1}, {'H': (1 << 24) + 1}, {'th': 0},
               {'edge': -1}, {'wsb': 4}):
        assert call(**kw) == -1, kw
    assert call(n=40000, K=2) == -1 and b'segments' in lib.y3_last_error()          # Y3_TILE_MERGE_MAX_SEGMENTS
    for m in (-0.5, 96.0, 200.0, float('nan')):
        assert call(margin=m) == -1 and b'margin' in lib.y3_last_error(), m
    assert lib.y3_tile_merge_workspace_bytes(2, 2) == 20 and lib.y3_tile_merge_workspace_bytes(0, 2) == 0

    def nms(method, m=10, thr=0.1, sigma=0.5, pool=a):
        return lib.y3_nms_labelled(pool, m, 2, method, thr, 0.3, sigma, 2 * a, 3 * a, 4 * a, 10, 5 * a, 1 << 20, None)
    assert nms(5) == -1 and b'method' in lib.y3_last_error()
    assert nms(-1) == -1
    assert nms(0, pool=None) == -1 and b'null' in lib.y3_last_error()
    assert nms(0, m=0) == -1
    assert nms(2, thr=0.0) == -1 and nms(3, sigma=0.0) == -1


def test_entry_points_declared_exported_and_bound():
    from yolo3 import _hip
    hdr = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    so = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('y3_tile_merge', 'y3_tile_merge_workspace_bytes', 'y3_nms_labelled'):
        assert ' %s(' % name in hdr and name in _hip.SIGNATURES and hasattr(so, name), name
    assert '#define Y3_NMS_NONE 4' in hdr
    assert 'inference_tiled.py:230-301' in hdr


def _run(capsys, script, *args):
    """The script's __main__ block in this process (its parser exits before anything else happens): (exit code, stdout, stderr)."""
    import runpy
    argv, cols = sys.argv, os.environ.get('COLUMNS')
    sys.argv = [script] + list(args)
    os.environ['COLUMNS'] = '200'
    try:
        with pytest.raises(SystemExit) as e:
            runpy.run_path(os.path.join(PKG, script), run_name='__main__')
    finally:
        sys.argv = argv
        if cols is None:
            del os.environ['COLUMNS']
        else:
            os.environ['COLUMNS'] = cols
    cap = capsys.readouterr()
    return e.value.code, cap.out, cap.err


def test_cli_flags_and_errors(capsys):
    code, out, _ = _run(capsys, 'inference_tiled.py', '--help')
    out = ' '.join(out.split())
    assert code == 0
    for flag in ('--merge-device {cpu,gpu}', '--seam-margin PX', '--merge-nms {none,hard,diou,soft-linear,soft-gaussian}', '--merge-nms-sigma'):
        assert flag in out, flag
    base = ['--saved-model-filepath', '/nonexistent', '--output-folder', '/nonexistent', '--image-folder', '/nonexistent']
    for extra in (['--seam-margin', '8'], ['--merge-nms', 'hard'], ['--merge-device', 'gpu', '--seam-margin', '96'],
                  ['--merge-device', 'gpu', '--seam-margin', '-1'], ['--merge-device', 'gpu', '--merge-nms', 'soft-gaussian', '--merge-nms-sigma', '0']):
        code, _, err = _run(capsys, 'inference_tiled.py', *(base + extra))
        assert code == 2 and 'error:' in err, (extra, err[-500:])
    code, out, _ = _run(capsys, 'evaluate.py', '--help')
    out = ' '.join(out.split())
    assert code == 0
    for flag in ('--tiled', '--tile-height', '--tile-width', '--seam-margin PX', '--merge-nms {none,hard,diou,soft-linear,soft-gaussian}'):
        assert flag in out, flag
    ev = ['--saved-model-filepath', '/nonexistent']
    folders = ['--image-folder', '/nonexistent', '--csv-folder', '/nonexistent']
    for extra in (['--tiled', '--database', '/nonexistent', '--tile-height', '256', '--tile-width', '256'], folders + ['--tiled'],
                  folders + ['--tiled', '--tile-height', '256', '--tile-width', '256', '--seam-margin', '96'],
                  folders + ['--seam-margin', '8'], folders + ['--merge-nms', 'hard'], folders + ['--tile-height', '256']):
        code, _, err = _run(capsys, 'evaluate.py', *(ev + extra))
        assert code == 2 and 'error:' in err, (extra, err[-500:])
