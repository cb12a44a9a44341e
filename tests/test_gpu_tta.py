"""Test-time augmentation on the device: y3_tta_views_nhwc, y3_tta_unmap and y3_box_vote against the NumPy
restatements of tests/tta_reference.py, YoloV3.predict_tta against predict on the stacked views, and the command lines."""
import functools
import os
import runpy
import sys

import numpy as np
import pytest
import torch

import tta_reference as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
D4 = tuple(range(8))
CANARY = 0x7fc5a5a5          # a NaN with a payload: any arithmetic on it, or any store over it, shows
EINVAL = -1


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(seed, shape):
    """Random 32-bit patterns (NaNs of both kinds, infinities and denormals among them) with a few NaN payloads planted."""
    a = np.random.default_rng(seed).integers(0, 2 ** 32, shape, dtype=np.uint32)
    flat = a.reshape(-1)
    flat[::97] = 0x7fc01234                # quiet NaN, payload
    flat[5::101] = 0xffa00001              # signalling NaN, sign set
    flat[7::103] = 0x7f800001
    return a


def _views_launch(src, codes, ld, prefill=CANARY, dc=4):
    """(return code, destination words [n * k * h * w * ld + 64] int64-safe uint32 array) of one y3_tta_views_nhwc call."""
    from yolo3 import _hip
    n, c, h, w = src.shape
    k = len(codes)
    words = n * k * h * w * ld
    buf = torch.from_numpy(np.full(words + 64, prefill, np.uint32).view(np.int32)).cuda()
    s = torch.from_numpy(src.view(np.int32)).cuda()
    rc = _hip.lib.y3_tta_views_nhwc(s.data_ptr(), n, c, h, w, _hip.int_array(codes), k, _hip.Tensor(buf.data_ptr(), n * k, h, w, dc, ld), _st())
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy().view(np.uint32)


# 32 x 32 and 96 x 96 are whole tiles of the kernel's 32-pixel tile; 24 x 24 is a single partial tile, 40 x 40 and 72 x 72 end in a
# ragged tile in both directions, so the guards of the load and of the TRANSPOSED store decide there; 40 x 72 is ragged and not square
@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('h,w,codes', [(32, 32, (0,)), (32, 32, (5,)), (32, 32, D4), (96, 96, (0,)), (96, 96, (5,)), (96, 96, D4),
                                       (24, 24, (0,)), (24, 24, (5,)), (24, 24, D4), (40, 40, (0,)), (40, 40, (5,)), (40, 40, D4),
                                       (72, 72, (6, 4, 7)), (64, 96, (0, 1, 2, 3)), (40, 72, (3, 0))])
def test_views_are_bit_exact(h, w, codes, c, n):
    """Whole tiles, one partial tile, ragged last tiles under straight and transposing views, a non-square image with the flips;
    pixel pitch 4 (n = 1) and 8."""
    from yolo3 import _hip
    ld = 4 if n == 1 else 8
    src = _bits(h * 7 + w + c + n, (n, c, h, w))
    rc, got = _views_launch(src, codes, ld)
    assert rc == 0, _hip.lib.y3_last_error()
    k = len(codes)
    body = got[:-64].reshape(n * k, h, w, ld)
    want = tr.views_nhwc(src, codes)
    assert np.array_equal(body[..., :4], want)                       # uint32 compare: NaN payloads included
    assert not body[..., c:4].any()                                  # pad channels are zero
    assert np.all(body[..., 4:] == CANARY) and np.all(got[-64:] == CANARY)      # nothing beyond the four channels, nothing after the tensor


@pytest.mark.parametrize('c,dc,ld', [(6, 8, 8), (5, 8, 12), (2, 8, 8), (8, 8, 8)])
def test_views_with_more_than_four_channels(c, dc, ld):
    """A destination of two groups of four channels: the second group partly, wholly or not at all padding."""
    from yolo3 import _hip
    src = _bits(c * 31 + ld, (2, c, 40, 40))
    rc, got = _views_launch(src, D4, ld, dc=dc)
    assert rc == 0, _hip.lib.y3_last_error()
    body = got[:-64].reshape(16, 40, 40, ld)
    assert np.array_equal(body[..., :dc], tr.views_nhwc(src, D4, dc))
    assert not body[..., c:dc].any() and np.all(body[..., dc:] == CANARY) and np.all(got[-64:] == CANARY)


def test_views_refuse_a_transpose_of_a_non_square_image():
    from yolo3 import _hip
    src = _bits(1, (1, 3, 64, 96))
    rc, got = _views_launch(src, (0, 5), 4)
    assert rc == EINVAL and b'square' in _hip.lib.y3_last_error()
    assert np.all(got == CANARY)
    rc, got = _views_launch(src, (1, 1), 4)
    assert rc == EINVAL and np.all(got == CANARY)
    rc, got = _views_launch(_bits(2, (1, 5, 64, 96)), (0, 1), 4)           # five channels into a destination of four
    assert rc == EINVAL and np.all(got == CANARY)


@pytest.mark.parametrize('h,w,codes,n', [(96, 96, D4, 2), (64, 96, (0, 1, 2, 3), 2), (96, 96, (6, 3, 5), 1)])
def test_unmap_is_the_float32_restatement(h, w, codes, n):
    from yolo3 import _hip
    rng = np.random.default_rng(h + len(codes))
    k, nb, d = len(codes), 301, 7                                    # more than one block of 256 rows, a ragged last one
    rows = rng.standard_normal((n * k, nb, d)).astype(np.float32)
    rows[:, :, 0:4] = rng.uniform(-60, 160, (n * k, nb, 4)).astype(np.float32)        # outside the image and negative too
    rows[:, ::9, 0:4] = rng.integers(-8, 120, (n * k, len(range(0, nb, 9)), 4)).astype(np.float32)
    rows[:, 5, 6] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    dev = torch.from_numpy(np.concatenate([rows.reshape(-1), np.full(16, 123.0, np.float32)])).cuda()
    rc = _hip.lib.y3_tta_unmap(dev.data_ptr(), n * k, nb, d, _hip.int_array(codes), k, h, w, _st())
    assert rc == 0, _hip.lib.y3_last_error()
    got = dev.cpu().numpy()
    want = tr.unmap_rows(rows, codes, h, w)
    assert np.array_equal(got[:-16].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.array_equal(got[:-16].reshape(rows.shape)[:, :, 4:].view(np.uint32), rows[:, :, 4:].view(np.uint32))
    assert np.all(got[-16:] == 123.0)
    if n * k > 1 and codes[0] != codes[-1]:
        assert not np.array_equal(got[:-16], rows.reshape(-1))


# ---- predict_tta ------------------------------------------------------------------------------------------------------------
ANCHORS = [(12, 12), (30, 20), (20, 30)]


@functools.lru_cache(maxsize=None)
def _model(use_graph):
    from yolo3.model import YoloV3
    return YoloV3(2, [96, 96, 3], 2, ANCHORS, seed=3, use_graph=use_graph)


def _images(seed, n):
    from yolo3 import imagereader
    x = torch.from_numpy(np.random.default_rng(seed).uniform(0, 255, (n, 3, 96, 96)).astype(np.float32)).cuda()
    return imagereader.zscore_normalize_device(x)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('use_graph', [False, True])
def test_predict_tta_is_predict_on_the_stacked_views(use_graph, precision):
    """Against the same batch of 16 (never a batch of 2, whose launch plan may differ); a second call reuses the plan."""
    yolo = _model(use_graph)
    plans = None
    for seed in (1, 2):
        x = _images(seed, 2)
        stacked = torch.from_numpy(tr.views_nchw(x.cpu().numpy(), D4)).cuda()
        want = tr.unmap_rows(yolo.predict(stacked, precision=precision).cpu().numpy(), D4, 96, 96)
        got = yolo.predict_tta(x, D4, precision=precision)
        assert got.shape == (2, 8 * want.shape[1], want.shape[2])
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.reshape(got.shape).view(np.uint32))
        assert np.isfinite(got).all() and not np.array_equal(got[0, :want.shape[1]], got[0, want.shape[1]:2 * want.shape[1]])
        if plans is None:
            plans = len(yolo._plans)
    assert len(yolo._plans) == plans


def test_predict_tta_refuses_more_than_16_network_inputs():
    yolo = _model(False)
    before = len(yolo._plans)
    with pytest.raises(ValueError, match='18 network inputs'):
        yolo.predict_tta(_images(3, 3), (0, 1, 2, 3, 4, 5))
    with pytest.raises(ValueError):
        yolo.predict_tta(_images(3, 1)[:, :, :64], (0, 1))
    assert len(yolo._plans) == before


# ---- box voting -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    """The scene's rows on the device with the device NMS's keep lists for them (computed once, never written again)."""
    from yolo3 import bbox_utils
    S = tr.SCENE
    rows = tr.vote_scene()
    dev = torch.from_numpy(rows).cuda()
    keep = bbox_utils.nms_device(dev, S['min_box'], S['iou_thr'], S['score_thr'], S['clip_wh'], private_outputs=True)
    torch.cuda.synchronize()
    return rows, dev, keep, tuple(t.cpu().numpy() for t in keep)


def _vote_launch(dev, keep, vote_iou, mode, max_keep=None):
    """One raw y3_box_vote call over the scene into a canary-filled out: [n, K, max_keep, 6] as uint32."""
    from yolo3 import _hip
    S = tr.SCENE
    n, nb, d = dev.shape
    K = d - 5
    idx, cnt, sc = keep
    if max_keep is not None:
        idx, sc = idx[:, :, :max_keep].contiguous(), sc[:, :, :max_keep].contiguous()
    mk = idx.shape[2]
    out = torch.from_numpy(np.full(n * K * mk * 6 + 32, CANARY, np.uint32).view(np.int32)).cuda()
    ws_bytes = int(_hip.lib.y3_box_vote_workspace_bytes(n, nb, K))
    ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.float32, device=dev.device)
    rc = _hip.lib.y3_box_vote(dev.data_ptr(), n, nb, K, idx.data_ptr(), cnt.data_ptr(), sc.data_ptr(), mk, S['min_box'], S['score_thr'],
                              float(S['clip_wh'][0]), float(S['clip_wh'][1]), vote_iou, S['views'], S['slots'], mode, out.data_ptr(),
                              ws.data_ptr(), ws_bytes, _st())
    assert rc == 0, _hip.lib.y3_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert np.all(got[-32:] == CANARY)
    return got[:-32].reshape(n, K, mk, 6)


@functools.lru_cache(maxsize=None)
def _vote_reference(vote_iou, consensus, max_keep=None):
    S = tr.SCENE
    rows, _, _, (idx, cnt, sc) = _scene()
    if max_keep is not None:
        idx, sc = idx[:, :, :max_keep], sc[:, :, :max_keep]
    return tr.vote(rows, idx, cnt, sc, S['min_box'], S['score_thr'], S['clip_wh'], vote_iou, S['views'], S['slots'], consensus)


def _check_vote(got, ref, rows, keep_np, clip_wh):
    valid = ref['valid']
    f = got.view(np.float32)
    assert np.all(got[~valid] == CANARY)                                      # nothing written beyond keep_cnt
    assert np.array_equal(f[..., 4][valid].view(np.uint32), ref['score'][valid].view(np.uint32))      # scores bit for bit
    cls = np.broadcast_to(np.arange(got.shape[1], dtype=np.float32)[None, :, None], valid.shape)
    assert np.array_equal(f[..., 5][valid], cls[valid])
    want32 = ref['box64'].astype(np.float32)
    # fp64 accumulation, one rounding: another summation order moves the result by at most one fp32 unit in the last place of it
    err = np.abs(f[..., 0:4].astype(np.float64) - want32.astype(np.float64))[valid]
    assert np.all(err <= np.spacing(np.abs(want32[valid]))), float(err.max())
    # a single member is the keep itself: its own clipped box, bit for bit
    single = valid & (ref['members'] == 1)
    assert single.any()
    idx = keep_np[0]
    for i, c, j in zip(*np.nonzero(single)):
        own = tr.clip_boxes(rows[i, idx[i, c, j], 0:4], clip_wh)[0]
        assert np.array_equal(got[i, c, j, 0:4], own.view(np.uint32)), (i, c, j)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('vote_iou', [0.5, 1.0])
def test_vote_matches_the_restatement(vote_iou, mode):
    S = tr.SCENE
    rows, dev, keep, keep_np = _scene()
    cnt = keep_np[1]
    ref = _vote_reference(vote_iou, bool(mode))
    assert ref['margin'] > 1e-4                                               # membership cannot hang on a rounding
    # the scene reaches what it is meant to reach
    assert cnt[0, 0] == 0 and cnt[0, 1] == 1 and cnt[1, 2] > 4 * 32           # a class without keeps; more keeps than one pass of the grid's waves
    a, b = set(keep_np[0][1, 1, :cnt[1, 1]]), set(keep_np[0][1, 2, :cnt[1, 2]])
    row = S['shared_slot']                                                    # kept under two classes, with different members
    assert row in a and row in b
    j1, j2 = list(keep_np[0][1, 1, :cnt[1, 1]]).index(row), list(keep_np[0][1, 2, :cnt[1, 2]]).index(row)
    assert ref['members'][1, 1, j1] == 1 and ref['members'][1, 2, j2] == (4 if vote_iou < 1 else 1)
    if vote_iou == 1.0:
        assert ref['members'][ref['valid']].max() > 1                         # identical boxes repeated in the views are members of each other
    else:
        assert ref['members'][ref['valid']].max() >= 4 and (ref['members'][ref['valid']] == 2).any()
    got = _vote_launch(dev, keep, vote_iou, mode)
    _check_vote(got, ref, rows, keep_np, S['clip_wh'])
    if mode == 1:
        s = got.view(np.float32)[..., 4][ref['valid']]
        assert s.min() > 0 and len(np.unique(s)) > 10
    else:
        # membership in keep mode, directly: the consensus launch, whose scores pin every member set bit for bit, adds the same
        # members in the same order, so the voted corners of the two modes are the same bits
        other = _vote_launch(dev, keep, vote_iou, 1)
        assert np.array_equal(other.view(np.float32)[..., 4][ref['valid']].view(np.uint32),
                              _vote_reference(vote_iou, True)['score'][ref['valid']].view(np.uint32))
        assert np.array_equal(got[..., 0:4][ref['valid']], other[..., 0:4][ref['valid']])
    again = _vote_launch(dev, keep, vote_iou, mode)
    assert np.array_equal(got, again)                                         # no atomics: the same bits on every run


def test_vote_with_max_keep_below_the_keep_count():
    S = tr.SCENE
    rows, dev, keep, keep_np = _scene()
    assert keep_np[1].max() > 3
    ref = _vote_reference(0.5, True, 3)
    assert ref['valid'].sum() == np.minimum(keep_np[1], 3).sum()
    got = _vote_launch(dev, keep, 0.5, 1, max_keep=3)
    _check_vote(got, ref, rows, (keep_np[0][:, :, :3], keep_np[1], keep_np[2][:, :, :3]), S['clip_wh'])
    full = _vote_launch(dev, keep, 0.5, 1)
    assert np.array_equal(got[ref['valid']], full[:, :, :3][ref['valid']])


def test_detect_tta_is_the_vote_and_without_a_vote_is_detect():
    from yolo3 import bbox_utils
    S = tr.SCENE
    rows, dev, keep, keep_np = _scene()
    kw = dict(iou_threshold=S['iou_thr'], score_threshold=S['score_thr'], clip_wh=S['clip_wh'])
    plain = bbox_utils.detect(dev, S['min_box'], **kw)
    pooled = bbox_utils.detect_tta(dev, S['views'], S['min_box'], **kw)
    for p, q in zip(plain, pooled):
        for u, v in zip(p, q):
            assert u.dtype == v.dtype and np.array_equal(u, v)
    voted = bbox_utils.detect_tta(dev, S['views'], S['min_box'], vote_iou=0.5, score='consensus', **kw)
    raw = _vote_launch(dev, keep, 0.5, 1).view(np.float32)
    for i in range(S['n']):
        want = np.concatenate([raw[i, c, :keep_np[1][i, c]] for c in range(S['K'])])
        b, s, lab, kept = voted[i]
        assert np.array_equal(b, want[:, 0:4]) and np.array_equal(s, want[:, 4]) and np.array_equal(lab, want[:, 5].astype(np.int32))
        assert np.array_equal(kept, plain[i][3]) and lab.dtype == np.int32
    pools = bbox_utils.detect_tta_pools(dev, S['views'], S['min_box'], vote_iou=0.5, score='consensus', **kw)
    assert all(p.is_cuda and p.shape == (m, 6) and np.array_equal(p[:, 0:4].cpu().numpy(), voted[i][0]) for i, (p, m) in enumerate(pools))


# ---- the command lines --------------------------------------------------------------------------------------------------------
def _main(script, *args):
    """The script's __main__ block in this process (no second interpreter, no second library load)."""
    argv = sys.argv
    sys.argv = [script] + list(args)
    try:
        runpy.run_path(os.path.join(PKG, script), run_name='__main__')
    finally:
        sys.argv = argv


@pytest.fixture(scope='module')
def cli_case(tmp_path_factory):
    from PIL import Image
    from yolo3.model import YoloV3
    tmp = str(tmp_path_factory.mktemp('tta_cli'))
    model_file = os.path.join(tmp, 'model.npz')
    YoloV3(2, [96, 96, 3], 2, ANCHORS, seed=7).save_weights(model_file)
    img_dir = os.path.join(tmp, 'imgs')
    os.makedirs(img_dir)
    rng = np.random.default_rng(5)
    imgs = {name: rng.integers(0, 256, (96, 96, 3), dtype=np.uint8) for name in ('a', 'b')}
    for name, im in imgs.items():
        Image.fromarray(im).save(os.path.join(img_dir, name + '.png'))
    return tmp, model_file, img_dir, imgs


def test_inference_cli(cli_case, capsys):
    tmp, model_file, img_dir, imgs = cli_case
    base = ['--saved-model-filepath', model_file, '--image-folder', img_dir, '--image-format', 'png', '--min-box-size', '4']
    outs = {}
    for name, extra in (('plain', []), ('none', ['--tta', 'none']), ('d4', ['--tta', 'd4', '--tta-vote-iou', '0.5', '--tta-score', 'consensus'])):
        outs[name] = os.path.join(tmp, 'out_' + name)
        _main('inference.py', *(base + ['--output-folder', outs[name]] + extra))
    capsys.readouterr()
    for name in imgs:
        plain = open(os.path.join(outs['plain'], name + '.csv'), 'rb').read()
        assert plain == open(os.path.join(outs['none'], name + '.csv'), 'rb').read()
        assert len(plain.splitlines()) > 1
        lines = open(os.path.join(outs['d4'], name + '.csv')).read().splitlines()
        assert lines[0] == 'X,Y,W,H,C' and len(lines) > 1
        b = np.array([[int(v) for v in ln.split(',')] for ln in lines[1:]])
        assert np.all(b[:, 0] >= 0) and np.all(b[:, 1] >= 0) and np.all(b[:, 0] + b[:, 2] <= 96) and np.all(b[:, 1] + b[:, 3] <= 96)
        assert np.all(b[:, 2] >= 4) and np.all(b[:, 3] >= 4) and set(b[:, 4]) <= {0, 1}
    assert sorted(os.listdir(outs['d4'])) == ['a.csv', 'b.csv']


def _evaluator_state(ev):
    return [a for a in ev.matches()] + [ev.image_counts().cpu().numpy(), ev._npos.copy(), np.array([ev.num_images])]


def test_evaluate_cli(cli_case, capsys):
    import evaluate
    from yolo3 import bbox_utils, imagereader, metrics
    from yolo3.model import YoloV3
    tmp, model_file, img_dir, imgs = cli_case
    csv_dir = os.path.join(tmp, 'gt')
    os.makedirs(csv_dir, exist_ok=True)
    yolo = YoloV3.from_file(model_file)
    views = bbox_utils.TTA_VIEWS['flips']
    thr = [0.3, 0.5]
    want_ev = metrics.DetectionEvaluator(2, thr)
    # both images in ONE network call of 2 x 4 views, as evaluate.py batches them: another batch size may take another launch plan
    names = sorted(imgs)
    x = torch.from_numpy(np.stack([np.ascontiguousarray(imgs[name].astype(np.float32).transpose(2, 0, 1)) for name in names])).cuda()
    rows = yolo.predict_tta(imagereader.zscore_normalize_device(x), views)
    dets = bbox_utils.detect_tta(rows, len(views), 4, clip_wh=(96, 96), vote_iou=0.5)
    gts = {}
    for name, (b, s, lab, _) in zip(names, dets):
        assert b.shape[0] > 2
        g = np.concatenate([np.round(b[::2]), lab[::2, None]], 1)          # every other detection as ground truth, so there are TPs
        gts[name] = np.concatenate([np.stack([g[:, 0], g[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1], g[:, 4]], 1),
                                    [[5, 5, 40, 40, 0]]]).astype(np.int64)
        bbox_utils.write_boxes_from_xywhc(gts[name], os.path.join(csv_dir, name + '.csv'))
        want_ev.add_detections([b], [s], [lab], [gts[name]])
    # the loop evaluate.py runs: the same evaluator state, bit for bit
    got_ev = metrics.DetectionEvaluator(2, thr)
    examples = [(name + '.png', imgs[name], gts[name]) for name in sorted(imgs)]
    assert metrics.evaluate_examples(yolo, examples, got_ev, 4, 8, tta='flips', tta_vote_iou=0.5) == 2
    for u, v in zip(_evaluator_state(got_ev), _evaluator_state(want_ev)):
        assert u.dtype == v.dtype and np.array_equal(u, v)
    assert want_ev.result()['tp'].sum() > 0
    # and the command line: the csv of that state
    want_csv, got_csv, none_csv, plain_csv = (os.path.join(tmp, n) for n in ('want.csv', 'got.csv', 'none.csv', 'plain.csv'))
    evaluate.write_csv(want_ev.result(), want_csv)
    base = ['--saved-model-filepath', model_file, '--image-folder', img_dir, '--csv-folder', csv_dir, '--image-format', 'png',
            '--min-box-size', '4', '--iou-thresholds'] + [str(t) for t in thr]
    capsys.readouterr()
    _main('evaluate.py', *(base + ['--output-file', got_csv, '--tta', 'flips', '--tta-vote-iou', '0.5']))
    out = capsys.readouterr().out
    assert 'Evaluated 2 images' in out and 'TTA: flips (4 views), vote IoU 0.5, score keep' in out
    assert open(got_csv, 'rb').read() == open(want_csv, 'rb').read()
    # --tta none prints the table, and writes the csv, of a run without the flag
    tables = []
    for path, extra in ((plain_csv, []), (none_csv, ['--tta', 'none'])):
        _main('evaluate.py', *(base + ['--output-file', path] + extra))
        out = capsys.readouterr().out
        assert 'TTA:' not in out
        tables.append(out[out.index('NMS: hard'):])
    assert tables[0] == tables[1] and 'mAP50' in tables[0]
    assert open(plain_csv, 'rb').read() == open(none_csv, 'rb').read()
