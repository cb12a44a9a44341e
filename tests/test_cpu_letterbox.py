"""Letterbox front end without a GPU: the fp64 restatement against torch's antialiased bilinear, the record
geometry, every refusal of the three entry points (nothing is launched: there is no device here), and the command-line refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import letterbox_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
EINVAL = -1

# (in_h, in_w) -> (out_h, out_w): reductions, enlargements, the identity, 1000 -> 7 and 1 -> 4
TORCH_SHAPES = [((64, 96), (32, 48)), ((100, 37), (32, 12)), ((7, 5), (32, 23)), ((24, 24), (24, 24)), ((1000, 3), (7, 3)), ((1, 9), (4, 9)),
                ((3, 1000), (1, 96)), ((128, 192), (64, 96)), ((33, 65), (17, 64))]


@pytest.mark.parametrize('src,dst', TORCH_SHAPES)
def test_restatement_is_torchs_antialiased_bilinear(src, dst):
    x = np.random.default_rng(src[0] * 1000 + src[1]).uniform(-1, 1, (2,) + src)
    want = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=dst, mode='bilinear', antialias=True, align_corners=False)[0].numpy()
    got = lr.resize(x, *dst)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


def test_weights_of_the_special_cases():
    assert np.array_equal(lr.axis_weights(9, 9), np.eye(9))
    w = lr.axis_weights(16, 8)
    assert np.array_equal(w[3, 5:9], [0.125, 0.375, 0.375, 0.125]) and np.count_nonzero(w[3]) == 4
    assert np.allclose(lr.axis_weights(37, 12).sum(1), 1, rtol=0, atol=1e-15)


GEOMETRY = [((1, 5000), (416, 416)), ((5000, 1), (416, 416)), ((416, 416), (416, 416)), ((208, 208), (416, 416)), ((832, 416), (416, 416)),
            ((415, 416), (416, 416)), ((417, 416), (416, 416)), ((1080, 1920), (416, 416)), ((7, 5), (64, 96)), ((3, 1000), (64, 96)),
            ((100, 37), (32, 32)), ((4000, 3000), (608, 416)), ((2049, 3), (64, 96)), ((95, 64), (64, 96))]


@pytest.mark.parametrize('src,frame', GEOMETRY)
def test_record_geometry(src, frame):
    from yolo3 import letterbox
    (h, w), (H, W) = src, frame
    rec = letterbox.letterbox_record(h, w, H, W, 48)[0]
    ref = lr.record(h, w, H, W, 48)[0]
    assert letterbox.LETTERBOX_RECORD == lr.RECORD and rec.tobytes() == ref.tobytes()
    nh, nw, py, px = int(rec['new_h']), int(rec['new_w']), int(rec['pad_y']), int(rec['pad_x'])
    assert 1 <= nh <= H and 1 <= nw <= W and (nh == H or nw == W)                      # the limiting axis fills the frame
    assert py == (H - nh) // 2 and px == (W - nw) // 2
    bottom, right = H - nh - py, W - nw - px
    assert py + nh + bottom == H and px + nw + right == W and 0 <= bottom - py <= 1 and 0 <= right - px <= 1
    r = min(H / h, W / w)
    assert (nh == 1 or abs(nh - h * r) <= 0.5 + 1e-9) and (nw == 1 or abs(nw - w * r) <= 0.5 + 1e-9)
    assert int(rec['src_offset']) == 48 and (int(rec['src_h']), int(rec['src_w'])) == (h, w)


def test_record_cases_by_hand():
    from yolo3 import letterbox
    f = lambda *a: tuple(int(letterbox.letterbox_record(*a)[0][k]) for k in ('new_h', 'new_w', 'pad_y', 'pad_x'))
    assert f(1, 5000, 416, 416) == (1, 416, 207, 0)          # the remainder (one row more) below
    assert f(5000, 1, 416, 416) == (416, 1, 0, 207)
    assert f(416, 416, 416, 416) == (416, 416, 0, 0)
    assert f(208, 208, 416, 416) == (416, 416, 0, 0)         # smaller than the frame: enlarged
    assert f(1080, 1920, 416, 416) == (234, 416, 91, 0)
    assert f(415, 416, 416, 416) == (415, 416, 0, 0)         # a one-pixel remainder goes to the bottom
    with pytest.raises(ValueError):
        letterbox.letterbox_record(0, 5, 32, 32)
    recs, total = letterbox.pack_layout([(7, 5, 3), (2, 2, 3), (1, 1, 3)], 1, 32, 32)
    assert [int(o) for o in recs['src_offset']] == [0, 112, 128] and total == 144
    with pytest.raises(ValueError, match='image 1'):
        letterbox.pack_layout([(7, 5, 3), (1, 3000, 3)], 1, 32, 32)          # 3000 -> 32 columns reduces by more than 64


def _rec(**kw):
    r = lr.hand_record(64, 96, 32, 48, 0, 0)
    for k, v in kw.items():
        r[0][k] = v
    return r


def _msg():
    from yolo3 import _hip
    return _hip.lib.y3_last_error().decode()


BAD_RECORDS = [(dict(new_h=0), 'content'), (dict(new_w=-3), 'content'), (dict(pad_y=1, new_h=32), 'does not fit'), (dict(pad_x=17), 'does not fit'),
               (dict(src_offset=8), 'multiple of 16'), (dict(src_h=32769), 'source'), (dict(src_w=0), 'source'),
               (dict(src_h=2049, new_h=32), 'more than 64'), (dict(src_w=20000, new_w=48), 'more than 64'), (dict(pad_x=-1), 'padding')]


def test_every_refusal_comes_before_any_launch():
    """No device is needed: a refused call returns Y3_EINVAL with its message and launches nothing."""
    from yolo3 import _hip
    lib = _hip.lib
    src, out, ws = 4096, 8192, 16384           # never dereferenced
    good = _rec()
    batch = lambda rec=good, src=src, dtype=0, c=3, n=1, H=32, W=48, out=out: lib.y3_letterbox_batch(src, dtype, c, n, rec.ctypes.data if rec is not None
                                                                                                  else None, H, W, 0.0, out, None)
    dst = lambda **kw: _hip.Tensor(**dict(dict(ptr=out, n=1, h=32, w=48, c=4, ld=4), **kw))
    fused = lambda rec=good, src=src, dtype=0, c=3, n=1, d=None, ws=ws: lib.y3_letterbox_zscore_nhwc(
        src, dtype, c, n, rec.ctypes.data if rec is not None else None, d if d is not None else dst(), ws, None)
    unmap = lambda rec=good, rows=out, n=1, nb=10, ld=7, clip=1: lib.y3_letterbox_unmap(rows, n, nb, ld, rec.ctypes.data if rec is not None else None,
                                                                                     clip, None)
    for call in (batch, fused):
        for kw, word in ((dict(src=None), 'null'), (dict(rec=None), 'null'), (dict(dtype=3), 'dtype'), (dict(dtype=-1), 'dtype'), (dict(c=2), 'channels'),
                         (dict(c=4), 'channels'), (dict(n=0), '1 .. 16'), (dict(n=17), '1 .. 16'), (dict(src=4100), 'aligned')):
            assert call(**kw) == EINVAL and word in _msg(), (kw, _msg())
        for kw, word in BAD_RECORDS:
            assert call(rec=_rec(**kw)) == EINVAL and word in _msg(), (kw, _msg())
        two = np.concatenate([good, _rec(new_h=0)])
        assert call(rec=two, n=2, **({'d': dst(n=2)} if call is fused else {})) == EINVAL and 'record 1' in _msg()
    assert batch(out=None) == EINVAL and 'null' in _msg()
    assert batch(H=0) == EINVAL and 'frame' in _msg()
    assert batch(W=40000) == EINVAL and 'frame' in _msg()
    # a bad destination, as y3_tta_views_nhwc refuses it
    for kw in (dict(ptr=None), dict(n=2), dict(c=2), dict(c=6, ld=8), dict(ld=6), dict(c=8, ld=4), dict(ptr=out + 4)):
        assert fused(d=dst(**kw)) == EINVAL and _msg().startswith('letterbox_zscore_nhwc'), (kw, _msg())
    assert fused(ws=None) == EINVAL and 'null' in _msg()
    assert fused(ws=ws + 8) == EINVAL and 'workspace' in _msg()
    assert lib.y3_letterbox_zscore_nhwc(src, 0, 3, 1, good.ctypes.data, None, ws, None) == EINVAL and 'null' in _msg()
    # the unmap
    for kw, word in ((dict(rows=None), 'null'), (dict(rec=None), 'null'), (dict(n=0), '1 .. 16'), (dict(n=17), '1 .. 16'), (dict(nb=0), 'sizes'),
                     (dict(ld=3), 'sizes'), (dict(clip=2), 'clip'), (dict(rec=_rec(new_w=0)), 'content'), (dict(rec=_rec(src_h=0)), 'source'),
                     (dict(rec=_rec(pad_y=-2)), 'padding')):
        assert unmap(**kw) == EINVAL and word in _msg() and _msg().startswith('letterbox_unmap'), (kw, _msg())
    # pure host-side size query: partials and statistics, then the staged frames
    assert lib.y3_letterbox_workspace_bytes(2, 32, 48, 3) >= 2 * 3 * 32 * 48 * 4 + 2 * 128 * 16 + 16
    assert lib.y3_letterbox_workspace_bytes(2, 32, 48, 3) % 16 == 0 and lib.y3_letterbox_workspace_bytes(0, 32, 48, 3) == 0
    with pytest.raises(_hip.HipError, match='letterbox_unmap'):
        _hip.check(unmap(clip=2), 'y3_letterbox_unmap')


def test_header_and_binding_declare_the_entry_points():
    from yolo3 import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('y3_letterbox_batch', 'y3_letterbox_zscore_nhwc', 'y3_letterbox_workspace_bytes', 'y3_letterbox_unmap'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    text = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    assert 'typedef struct y3_letterbox_record' in text and '#define Y3_LETTERBOX_MAX_IMAGES 16' in text


def _cli(script, *args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + os.environ.get('PYTHONPATH', '').split(os.pathsep)))
    return subprocess.run([sys.executable, os.path.join(PKG, script)] + list(args), capture_output=True, text=True, env=env, timeout=300)


def test_command_lines_refuse_letterbox_with_tta_or_tiled(tmp_path):
    base = ['--saved-model-filepath', str(tmp_path / 'none.npz'), '--image-folder', str(tmp_path), '--letterbox']
    r = _cli('inference.py', *(base + ['--output-folder', str(tmp_path / 'o'), '--tta', 'hflip']))
    assert r.returncode == 2 and '--letterbox does not go with --tta' in r.stderr
    ev = base + ['--csv-folder', str(tmp_path)]
    r = _cli('evaluate.py', *(ev + ['--tta', 'flips']))
    assert r.returncode == 2 and '--letterbox does not go with --tta or --tiled' in r.stderr
    r = _cli('evaluate.py', *(ev + ['--tiled', '--tile-height', '96', '--tile-width', '96']))
    assert r.returncode == 2 and '--letterbox does not go with --tta or --tiled' in r.stderr
    assert not (tmp_path / 'o').exists()


def test_evaluate_examples_refuses_letterbox_with_tta():
    from yolo3 import metrics
    with pytest.raises(ValueError, match='letterbox does not go with tta'):
        metrics.evaluate_examples(None, [], None, 4, 8, tta='flips', letterbox=True)
