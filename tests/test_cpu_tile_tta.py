"""CPU-only checks of tile test-time augmentation: the library refuses bad calls before any launch, the batching
rule that keeps all views of a tile in one network call, and the command lines of inference_tiled.py and evaluate.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
EINVAL = -1          # Y3_EINVAL


def _gather(views, th=64, tw=64, c=3, pitch=4, img=64, table=64, out=64, ws=64, k=None, dtype=0):
    """y3_tile_gather_zscore_views_nhwc on made-up (16-byte aligned, never dereferenced) pointers -> (return code, message)."""
    from yolo3 import _hip
    codes = None if views is None else _hip.int_array(views)
    rc = _hip.lib.y3_tile_gather_zscore_views_nhwc(img, dtype, 100, 130, c, table, 2, th, tw, codes, len(views) if k is None else k, out, pitch,
                                                   ws, None)
    return rc, _hip.lib.y3_last_error()


def test_library_refuses_bad_arguments_without_device():
    """Y3_EINVAL with a message before anything is launched (no GPU here: a launch would fail differently)."""
    rc, msg = _gather([0, 5], th=40, tw=72)
    assert rc == EINVAL and b'tile_gather_zscore_views_nhwc' in msg and b'square' in msg          # a transposing view, 40 x 72 tile
    rc, msg = _gather([1, 1])
    assert rc == EINVAL and b'twice' in msg
    rc, msg = _gather([0, 8])
    assert rc == EINVAL and b'outside 0 .. 7' in msg
    rc, msg = _gather([0] * 9)
    assert rc == EINVAL and b'views' in msg
    rc, msg = _gather([0, 1], c=5)
    assert rc == EINVAL and b'channels' in msg
    rc, msg = _gather([0, 1], pitch=6)
    assert rc == EINVAL and b'pitch' in msg
    for kw in ({'img': None}, {'table': None}, {'out': None}, {'ws': None}):
        rc, msg = _gather([0, 1], **kw)
        assert rc == EINVAL and b'null pointer' in msg, kw
    rc, msg = _gather(None, k=2)
    assert rc == EINVAL and b'null pointer' in msg
    assert _gather([0, 1], pitch=0)[0] == EINVAL and _gather([0, 1], out=72)[0] == EINVAL and _gather([0], dtype=3)[0] == EINVAL
    assert _gather([], k=0)[0] == EINVAL


def test_voted_merge_refuses_bad_arguments_without_device():
    from yolo3 import _hip
    lib = _hip.lib

    def merge(voted=64, n=2, nb=10, K=2, mk=10, margin=0.0, ws=1 << 10, cap=16):
        return lib.y3_tile_merge_voted(voted, n, nb, K, 64, 64, mk, 64, 256, 256, 500, 700, 96, margin, 64, cap, 64, 64, ws, None)
    assert merge(voted=None) == EINVAL and b'tile_merge_voted: null pointer' in lib.y3_last_error()
    assert merge(nb=0) == EINVAL and merge(cap=0) == EINVAL and merge(margin=96.0) == EINVAL
    assert merge(ws=4) == EINVAL and b'tile_merge_voted: workspace' in lib.y3_last_error()


def test_header_documents_the_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    from yolo3 import _hip
    for name in ('y3_tile_gather_zscore_views_nhwc', 'y3_tile_merge_voted'):
        assert name in hdr and name in _hip.SIGNATURES and hasattr(_hip.lib, name)
    assert 'DESIGN §3.26' in hdr


def test_batching_keeps_the_views_of_a_tile_together():
    import inference_tiled as it
    # the bf16 plan of 100 network inputs: 25 tiles x 4 views
    got = it.tta_tile_batches([45, 45, 10], 4, 25)
    assert got == [11, 11, 2, 1] and sum(got) == 25
    # never more inputs than scheduled, except the one-tile minimum; every tile exactly once
    for sizes, k, n in (([45, 45, 10], 4, 25), ([45, 45, 10], 8, 13), ([16] * 22, 4, 88), ([25, 25, 25, 5], 2, 40), ([3, 3, 2], 4, 2),
                        ([25], 8, 3), ([7, 7, 7, 3], 4, 6)):
        got = it.tta_tile_batches(sizes, k, n)
        assert sum(got) == n and all(t >= 1 for t in got), (sizes, k, n, got)
        for i, t in enumerate(got):
            b = sizes[i % len(sizes)]
            assert t * k <= b or t == 1, (sizes, k, n, got)
    assert it.tta_tile_batches([16] * 22, 4, 88) == [4] * 22
    # k = 1 is the identity
    for sizes in ([45, 45, 10], [25, 25, 25, 13], [7], [1, 1, 1]):
        assert it.tta_tile_batches(sizes, 1, sum(sizes)) == sizes
    assert it.tta_tile_batches([45, 45, 10], 4, 0) == []
    for bad in (([4], 0, 2), ([], 2, 2), ([0, 0], 2, 2)):
        with pytest.raises(ValueError):
            it.tta_tile_batches(*bad)


def _run(capsys, script, *args):
    """The script's __main__ block in this process: (SystemExit code or the exception, stdout, stderr)."""
    import runpy
    argv, cols = sys.argv, os.environ.get('COLUMNS')
    sys.argv = [script] + list(args)
    os.environ['COLUMNS'] = '200'
    try:
        with pytest.raises(BaseException) as e:
            runpy.run_path(os.path.join(PKG, script), run_name='__main__')
    finally:
        sys.argv = argv
        if cols is None:
            del os.environ['COLUMNS']
        else:
            os.environ['COLUMNS'] = cols
    cap = capsys.readouterr()
    return (e.value.code if isinstance(e.value, SystemExit) else e.value), cap.out, cap.err


def test_cli_flags_and_errors(capsys, tmp_path):
    missing = str(tmp_path / 'missing.npz')
    empty = tmp_path / 'images'
    empty.mkdir()
    tiles = ['--tile-height', '256', '--tile-width', '256']
    inf = ['--saved-model-filepath', missing, '--output-folder', str(tmp_path / 'out'), '--image-folder', str(empty)] + tiles
    ev = ['--saved-model-filepath', missing, '--image-folder', str(empty), '--csv-folder', str(empty), '--tiled'] + tiles
    full = ['--tile-tta', 'd4', '--tile-tta-vote-iou', '0.5', '--tile-tta-score', 'consensus']
    for script, base in (('inference_tiled.py', inf), ('evaluate.py', ev)):
        code, out, _ = _run(capsys, script, '--help')
        out = ' '.join(out.split())
        assert code == 0
        for flag in ('--tile-tta {none,hflip,flips,d4}', '--tile-tta-vote-iou T', '--tile-tta-score {keep,consensus}'):
            assert flag in out, (script, flag)
        # the flags parse: the run gets as far as the missing model file
        for extra in ([], full, ['--tile-tta', 'flips'], ['--tile-tta', 'hflip', '--tile-tta-vote-iou', '1']):
            code, out, err = _run(capsys, script, *(base + extra))
            assert not isinstance(code, int), (script, extra, code, err[-500:])
            assert 'missing' in str(code).lower() or isinstance(code, (RuntimeError, OSError)), (script, extra, code)
        for extra in (['--tile-tta', 'rot90'], ['--tile-tta', 'flips', '--tile-tta-vote-iou', '0'],
                      ['--tile-tta', 'flips', '--tile-tta-vote-iou', '1.5'], ['--tile-tta', 'flips', '--tile-tta-score', 'consensus'],
                      ['--tile-tta-vote-iou', '0.5'], ['--tile-tta', 'flips', '--tile-tta-score', 'mean']):
            code, _, err = _run(capsys, script, *(base + extra))
            assert code == 2 and 'error:' in err, (script, extra, err[-500:])
        # d4 transposes: a non-square tile is refused
        wide = [a if a != '256' or base[i - 1] != '--tile-width' else '320' for i, a in enumerate(base)]
        code, _, err = _run(capsys, script, *(wide + ['--tile-tta', 'd4']))
        assert code == 2 and 'square' in err, (script, err[-500:])
        code, _, err = _run(capsys, script, *(wide + ['--tile-tta', 'flips']))
        assert not isinstance(code, int), (script, err[-500:])
    # evaluate.py: the tile flags go with --tiled only, and --tta stays refused there
    plain = ['--saved-model-filepath', missing, '--image-folder', str(empty), '--csv-folder', str(empty)]
    for extra in (['--tile-tta', 'flips'], ['--tile-tta-vote-iou', '0.5'], ['--tile-tta-score', 'consensus']):
        code, _, err = _run(capsys, 'evaluate.py', *(plain + extra))
        assert code == 2 and 'go with --tiled' in err, (extra, err[-500:])
    code, _, err = _run(capsys, 'evaluate.py', *(ev + ['--tta', 'flips']))
    assert code == 2 and '--tta does not go with --tiled' in err
    code, out, _ = _run(capsys, 'evaluate.py', *(ev + full))
    assert 'tile_tta = d4' in out and 'tile_tta_vote_iou = 0.5' in out and 'tile_tta_score = consensus' in out and 'tta = none' in out


def test_python_entry_points_refuse_bad_options_before_any_device_work():
    import numpy as np
    import inference_tiled as it
    img = np.zeros((300, 300, 3), np.uint8)
    for kw in (dict(tile_tta='rot90'), dict(tile_tta='flips', tta_vote_iou=0.0), dict(tile_tta='flips', tta_score='consensus'),
               dict(tile_tta='d4')):
        with pytest.raises(ValueError):
            it.inference_image_tiled(None, img, [256, 320], 8, **kw)
        with pytest.raises(ValueError):
            it.tiled_pool_device(None, img, [256, 320], 8, **kw)
