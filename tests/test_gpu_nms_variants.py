"""GPU tests of the opt-in NMS variants (y3_nms_per_class_ex) against the NumPy restatements of
tests/nms_variants_reference.py: diou and soft-linear bit for bit (keep_idx, keep_cnt, keep_score), soft-gaussian to
1e-5 relative on inputs whose scores stay well separated; 'hard' through _ex is y3_nms_per_class bit for bit."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nms_variants_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
CODES = {'hard': 0, 'diou': 1, 'soft-linear': 2, 'soft-gaussian': 3}


def _launch(rows, method, min_box, score_thr=0.1, iou_thr=0.3, sigma=0.5, clip=None, max_keep=None, legacy=False):
    """One launch on the current stream; rows: CUDA float32 [n, nb, 5+K].  Returns device (keep_idx, keep_cnt, keep_score)."""
    from yolo3 import _hip
    n, nb, d = rows.shape
    k = d - 5
    mk = nb if max_keep is None else max_keep
    idx = torch.full((n, k, mk), -7, dtype=torch.int32, device=rows.device)
    cnt = torch.full((n, k), -7, dtype=torch.int32, device=rows.device)
    sc = torch.full((n, k, mk), -7.0, dtype=torch.float32, device=rows.device)
    cw, ch = (float(clip[0]), float(clip[1])) if clip is not None else (-1.0, -1.0)
    st = torch.cuda.current_stream(rows.device).cuda_stream
    if legacy:
        wsb = int(_hip.lib.y3_nms_workspace_bytes(n, nb, k))
        ws = torch.empty(wsb // 4 + 4, dtype=torch.float32, device=rows.device)
        _hip.check(_hip.lib.y3_nms_per_class(rows.data_ptr(), n, nb, k, float(min_box), float(score_thr), float(iou_thr), cw, ch,
                                             idx.data_ptr(), cnt.data_ptr(), sc.data_ptr(), mk, ws.data_ptr(), wsb, st))
    else:
        wsb = int(_hip.lib.y3_nms_workspace_bytes_ex(n, nb, k, CODES[method]))
        ws = torch.empty(max(wsb, 4) // 4 + 4, dtype=torch.float32, device=rows.device)
        _hip.check(_hip.lib.y3_nms_per_class_ex(rows.data_ptr(), n, nb, k, CODES[method], float(min_box), float(score_thr), float(iou_thr),
                                                float(sigma), cw, ch, idx.data_ptr(), cnt.data_ptr(), sc.data_ptr(), mk, ws.data_ptr(), wsb,
                                                st), 'y3_nms_per_class_ex')
    return idx, cnt, sc, ws


def _host(out):
    idx, cnt, sc = (t.cpu().numpy() for t in out[:3])
    return idx, cnt, sc


def _segments(out):
    """-> per image, per class (rows, scores) of the valid entries."""
    idx, cnt, sc = _host(out)
    return [[(idx[i, c, :cnt[i, c]], sc[i, c, :cnt[i, c]]) for c in range(cnt.shape[1])] for i in range(cnt.shape[0])]


def _check_exact(out, rows_np, method, min_box, clip=None, score_thr=0.1, iou_thr=0.3, max_keep=None, what=''):
    got = _segments(out)
    for i, img in enumerate(rows_np):
        want = ref.per_class(img, method, min_box, score_thr, iou_thr, clip_wh=clip, max_keep=max_keep)
        for c, ((gr, gs), (wr, ws)) in enumerate(zip(got[i], want)):
            tag = (what, method, i, c, min_box, clip)
            assert gr.shape == wr.shape, (tag, gr.shape, wr.shape)
            assert np.array_equal(gr, wr), (tag, np.nonzero(gr != wr)[0][:5])
            assert np.array_equal(gs.view(np.uint32), ws.astype(np.float32).view(np.uint32)), tag


def _goldens(golden_dir):
    return [p for p in sorted(glob.glob(os.path.join(golden_dir, 'nms_*.npz'))) if 'rows' in np.load(p).files]


def test_hard_through_ex_is_nms_per_class(golden_dir):
    for path in _goldens(golden_dir):
        z = np.load(path)
        rows = torch.from_numpy(np.stack([z['rows'], z['rows'][::-1].copy()])).cuda()
        for mb, clip in ((float(z['min_box']), None), (0.0, (400.0, 380.0))):
            a = _host(_launch(rows, 'hard', mb, clip=clip))
            b = _host(_launch(rows, 'hard', mb, clip=clip, legacy=True))
            assert np.array_equal(a[1], b[1]), path
            for i in range(2):
                for c in range(a[1].shape[1]):
                    m = a[1][i, c]
                    assert np.array_equal(a[0][i, c, :m], b[0][i, c, :m]), path
                    assert np.array_equal(a[2][i, c, :m].view(np.uint32), b[2][i, c, :m].view(np.uint32)), path
        if 'keep' in z.files:
            got = _segments(_launch(rows[:1], 'hard', float(z['min_box'])))[0]
            assert np.array_equal(np.concatenate([g[0] for g in got]), z['keep']), path


@pytest.mark.parametrize('method', ['diou', 'soft-linear'])
def test_bit_exact_on_goldens(golden_dir, method):
    names = ['nms_small_k2', 'nms_sparse416_k2', 'nms_dense416_k1', 'nms_dense416_k2', 'nms_sparse608_k3']
    for name in names:
        z = np.load(os.path.join(golden_dir, name + '.npz'))
        rows_np = z['rows'][None]
        rows = torch.from_numpy(rows_np).cuda()
        for mb, clip in ((float(z['min_box']), None), (0.0, (400.0, 380.0)), (32.0, (300.0, 416.0)), (0.0, None)):
            _check_exact(_launch(rows, method, mb, clip=clip), rows_np, method, mb, clip, what=name)
    # several images of different kinds in one launch
    za, zb = np.load(os.path.join(golden_dir, 'nms_sparse416_k2.npz')), np.load(os.path.join(golden_dir, 'nms_dense416_k2.npz'))
    rows_np = np.stack([za['rows'], zb['rows'], za['rows'][::-1].copy()])
    _check_exact(_launch(torch.from_numpy(rows_np).cuda(), method, 32.0), rows_np, method, 32.0, what='batched')


def _large_rows(rng, nb, K, size=900):
    """nb rows (> 16384: the workspace paths of both kernels), about a third of them candidates per class."""
    rows = np.zeros((nb, 5 + K), np.float32)
    c = rng.uniform(0, size, (nb, 2))
    wh = rng.uniform(10, 80, (nb, 2))
    rows[:, 0:2] = c - wh / 2
    rows[:, 2:4] = c + wh / 2
    rows[:, 4] = rng.uniform(0.2, 1, nb)
    rows[:, 5:] = np.where(rng.random((nb, K)) < 0.35, rng.uniform(0.05, 1, (nb, K)), 0.001)
    return rows


@pytest.mark.parametrize('method', ['diou', 'soft-linear'])
def test_bit_exact_beyond_16384_rows(method):
    rng = np.random.default_rng(608)
    rows_np = np.stack([_large_rows(rng, 22743, 2), _large_rows(rng, 22743, 2)])       # a 608^2 tile's row count
    rows = torch.from_numpy(rows_np).cuda()
    for mb, clip in ((0.0, None), (32.0, (700.0, 650.0))):
        _check_exact(_launch(rows, method, mb, clip=clip), rows_np, method, mb, clip, what='22743')


def _separated_rows(seed, m=48, K=2, size=300):
    """Candidates whose soft-gaussian scores stay well separated (checked by the caller) from each other and from the
    threshold after every decay: scores on a grid of steps of 1/m, boxes that overlap in clusters."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((m, 5 + K), np.float32)
    c = rng.uniform(0, size, (m, 2))
    w = rng.uniform(30, 70, (m, 2))
    rows[:, 0:2] = c - w / 2
    rows[:, 2:4] = c + w / 2
    rows[:, 4] = 1
    for k in range(K):
        rows[:, 5 + k] = (0.15 + 0.85 * rng.permutation(m) / m) ** 2
    return rows


def test_soft_gaussian_matches_float64():
    """Same rows in the same order, scores within 1e-5 relative.  Not bit for bit: the device expf and NumPy's exp may differ
    in the last ulp, so the inputs are built (and checked) to keep every decision at least 1e-3 relative away from a tie."""
    imgs = [_separated_rows(s) for s in (5, 7, 8)]
    for img in imgs:
        assert ref.soft_gaussian_margins(img, 0, 0.1, 0.3, 0.5) > 1e-3
    for nb in (48, 9000):                    # 9000 rows: the same candidates padded with non-candidates (workspace path)
        rows_np = np.zeros((len(imgs), nb, imgs[0].shape[1]), np.float32)
        for i, img in enumerate(imgs):
            rows_np[i, :img.shape[0]] = img
        got = _segments(_launch(torch.from_numpy(rows_np).cuda(), 'soft-gaussian', 0.0))
        for i, img in enumerate(imgs):
            want = ref.per_class(img, 'soft-gaussian', 0.0)
            for c, ((gr, gs), (wr, ws)) in enumerate(zip(got[i], want)):
                assert len(wr) > 30 and np.array_equal(gr, wr), (nb, i, c)
                assert np.allclose(gs.astype(np.float64), ws, rtol=1e-5, atol=0), (nb, i, c, np.max(np.abs(gs / ws - 1)))


def test_edge_cases(golden_dir):
    # no candidates / one candidate
    for name, want in (('nms_empty', [0, 0]), ('nms_allsmall', [0, 0]), ('nms_single', [1, 0])):
        z = np.load(os.path.join(golden_dir, name + '.npz'))
        rows = torch.from_numpy(z['rows'][None]).cuda()
        for m in ref.METHODS:
            idx, cnt, sc = _host(_launch(rows, m, float(z['min_box'])))
            assert cnt[0].tolist() == want, (name, m)
            if want[0]:
                assert idx[0, 0, 0] == z['keep'][0] and sc[0, 0, 0] == z['scores'][0], (name, m)
    # 64 identical boxes, score 0.9 each: linear keeps the highest row; gaussian decays geometrically, highest rows first
    rows_np = np.zeros((1, 64, 6), np.float32)
    rows_np[0, :, 0:4] = [10, 20, 90, 70]
    rows_np[0, :, 4] = 1.0
    rows_np[0, :, 5] = 0.81
    rows = torch.from_numpy(rows_np).cuda()
    idx, cnt, sc = _host(_launch(rows, 'soft-linear', 0.0))
    assert cnt[0, 0] == 1 and idx[0, 0, 0] == 63
    idx, cnt, sc = _host(_launch(rows, 'soft-gaussian', 0.0, sigma=4.0))
    s0 = float(np.sqrt(np.float32(0.81)))
    f = np.exp(-1.0 / 4.0)
    k = int(np.floor(np.log(0.1 / s0) / np.log(f))) + 1          # s0 f^j >= 0.1 for j < k
    assert k == 9 and cnt[0, 0] == k
    assert idx[0, 0, :k].tolist() == list(range(63, 63 - k, -1))
    assert np.allclose(sc[0, 0, :k], s0 * f ** np.arange(k), rtol=1e-5, atol=0)
    idx, cnt, sc = _host(_launch(rows, 'diou', 0.0))
    assert cnt[0, 0] == 1 and idx[0, 0, 0] == 63
    # max_keep below the output count: the first max_keep entries, keep_cnt = max_keep, nothing written beyond
    z = np.load(os.path.join(golden_dir, 'nms_sparse416_k2.npz'))
    rows_np = np.stack([z['rows']] * 2)
    for m in ('diou', 'soft-linear'):
        out = _launch(torch.from_numpy(rows_np).cuda(), m, 32.0, max_keep=5)
        assert _host(out)[1].tolist() == [[5, 5], [5, 5]]
        _check_exact(out, rows_np, m, 32.0, max_keep=5, what='max_keep')
    out = _host(_launch(torch.from_numpy(rows_np).cuda(), 'soft-gaussian', 32.0, max_keep=5))
    full = _host(_launch(torch.from_numpy(rows_np).cuda(), 'soft-gaussian', 32.0))
    assert out[1].tolist() == [[5, 5], [5, 5]]
    assert np.array_equal(out[0], full[0][:, :, :5]) and np.array_equal(out[2], full[2][:, :, :5])


def test_deterministic_across_launches_and_streams(golden_dir):
    z = np.load(os.path.join(golden_dir, 'nms_dense416_k2.npz'))
    rows = torch.from_numpy(np.stack([z['rows']] * 8)).cuda()
    big = torch.from_numpy(np.stack([_large_rows(np.random.default_rng(3), 22743, 2)] * 2)).cuda()
    for r in (rows, big):
        for m in ('diou', 'soft-linear', 'soft-gaussian'):
            first = _host(_launch(r, m, 32.0))
            for _ in range(19):
                again = _host(_launch(r, m, 32.0))
                for a, b in zip(first, again):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), m
            # two streams at once, each with its own outputs and workspace
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            s1.wait_stream(torch.cuda.current_stream())
            s2.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s1):
                o1 = _launch(r, m, 32.0)
            with torch.cuda.stream(s2):
                o2 = _launch(r, m, 32.0)
            torch.cuda.synchronize()
            for o in (o1, o2):
                for a, b in zip(first, _host(o)):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), m


def _synthetic_scene(rng, n, nb, K, size):
    gts, rows = [], np.zeros((n, nb, 5 + K), np.float32)
    for i in range(n):
        g = int(rng.integers(2, 15))
        gt = np.concatenate([rng.integers(0, size - 50, (g, 2)), rng.integers(14, 50, (g, 2)), rng.integers(0, K, (g, 1))], 1)
        gts.append(gt)
        src = gt[rng.integers(0, g, nb)]
        xy = src[:, :2] + rng.normal(0, 4, (nb, 2))
        wh = src[:, 2:4] * rng.uniform(0.8, 1.25, (nb, 2))
        stray = rng.random(nb) < 0.3
        xy[stray] = rng.uniform(-10, size, (stray.sum(), 2))
        rows[i, :, 0:2] = xy
        rows[i, :, 2:4] = xy + wh
        rows[i, :, 4] = rng.uniform(0.05, 1, nb)
        rows[i, :, 5:] = rng.uniform(0, 0.3, (nb, K))
        rows[i, np.arange(nb), 5 + src[:, 4]] = np.where(stray, rows[i, np.arange(nb), 5 + src[:, 4]], rng.uniform(0.3, 1, nb))
    return rows, gts


@pytest.mark.parametrize('method', ['diou', 'soft-linear'])
def test_evaluator_add_batch_matches_restated_keep_lists(method):
    from yolo3 import metrics
    rng = np.random.default_rng(11)
    K, n, nb, size = 2, 5, 400, 256
    rows_np, gts = _synthetic_scene(rng, n, nb, K, size)
    clip = (size, size)
    dev = metrics.DetectionEvaluator(K)
    dev.add_batch(torch.from_numpy(rows_np[:3]).cuda(), gts[:3], 8, clip_wh=clip, nms=method)
    dev.add_batch(torch.from_numpy(rows_np[3:]).cuda(), gts[3:], 8, clip_wh=clip, nms=method)
    host = metrics.DetectionEvaluator(K)
    boxes, scores, labels, rids = [], [], [], []
    for i in range(n):
        per = ref.per_class(rows_np[i], method, 8, clip_wh=clip)
        r = np.concatenate([p[0] for p in per]).astype(np.int64)
        b = rows_np[i, r, 0:4].copy()
        b[:, 0::2] = np.clip(b[:, 0::2], 0, size)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, size)
        boxes.append(b)
        scores.append(np.concatenate([p[1] for p in per]).astype(np.float32))
        labels.append(np.concatenate([np.full(len(p[0]), c, np.int32) for c, p in enumerate(per)]))
        rids.append(r)
    host.add_detections(boxes, scores, labels, gts, rids)
    rd, rh = dev.result(), host.result()
    for a, b in zip(dev.matches(), host.matches()):
        assert np.array_equal(a, b)
    for k in ('ap', 'recall', 'tp', 'fp', 'npos'):
        assert np.array_equal(rd[k], rh[k], equal_nan=True), k
    assert rd['tp'].sum() > 0 and rd['fp'].sum() > 0


def _env():
    return dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))


def test_inference_tiled_cli_soft_gaussian_matches_in_process(tmp_path):
    from PIL import Image
    sys.path.insert(0, PKG)
    import inference_tiled
    from yolo3 import bbox_utils
    from yolo3.model import YoloV3
    tmp = str(tmp_path)
    model_file = os.path.join(tmp, 'model.npz')
    YoloV3(4, [256, 256, 3], 2, [(48, 48), (90, 60), (60, 90)], seed=7).save_weights(model_file)
    img_dir, out_dir = os.path.join(tmp, 'imgs'), os.path.join(tmp, 'dets')
    os.makedirs(img_dir)
    img = np.random.default_rng(9).integers(0, 256, (500, 700, 3), dtype=np.uint8)
    Image.fromarray(img).save(os.path.join(img_dir, 'b.png'))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'inference_tiled.py'), '--saved-model-filepath', model_file, '--output-folder', out_dir,
                        '--image-folder', img_dir, '--image-format', 'png', '--tile-height', '256', '--tile-width', '256', '--min-box-size', '8',
                        '--nms', 'soft-gaussian', '--nms-sigma', '0.4'], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    model = YoloV3.from_file(model_file).get_keras_model()
    pred = inference_tiled.inference_image_tiled(model, img, [256, 256], 8, nms='soft-gaussian', nms_sigma=0.4)
    hard = inference_tiled.inference_image_tiled(model, img, [256, 256], 8)
    want = os.path.join(tmp, 'want.csv')
    bbox_utils.write_boxes_from_ltrbpc(pred, want)
    got = open(os.path.join(out_dir, 'b.csv'), 'rb').read()
    assert got == open(want, 'rb').read()
    assert pred.shape[0] > 0 and not np.array_equal(pred, hard)     # the flag reaches the per-tile NMS


def test_evaluate_cli_diou_reports_in_process_ap(tmp_path):
    sys.path.insert(0, PKG)
    import build_lmdb
    import evaluate
    from yolo3 import lmdbio
    from yolo3.model import YoloV3
    tmp = str(tmp_path)
    size, K = (256, 256, 3), 2
    rng = np.random.default_rng(21)
    items = []
    for i in range(6):
        k = int(rng.integers(1, 4))
        wh = rng.integers(40, 120, (k, 2))
        xy = np.stack([rng.integers(0, size[1] - wh[:, 0]), rng.integers(0, size[0] - wh[:, 1])], 1)
        boxes = np.concatenate([xy, wh, rng.integers(0, K, (k, 1))], 1).astype(np.int32)
        items.append(build_lmdb.make_record(rng.integers(0, 256, size, dtype=np.uint8), boxes, i, 'img%03d' % i))
    db = os.path.join(tmp, 'test-syn.lmdb')
    lmdbio.write_environment(db, items)
    model_file = os.path.join(tmp, 'model.npz')
    YoloV3(4, list(size), K, [(48, 48), (90, 60), (60, 90)], seed=7).save_weights(model_file)
    thr = [0.1, 0.3, 0.5]
    out_csv = os.path.join(tmp, 'diou.csv')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'evaluate.py'), '--saved-model-filepath', model_file, '--database', db,
                        '--batch-size', '4', '--min-box-size', '8', '--iou-thresholds'] + [str(t) for t in thr] +
                       ['--nms', 'diou', '--output-file', out_csv], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'NMS: diou' in r.stdout and 'mAP50 = ' in r.stdout and 'mAP50:95 = ' in r.stdout
    res, count, _ = evaluate.evaluate(evaluate.database_examples(db), model_file, 8, batch_size=4, iou_thresholds=thr, nms='diou')
    assert count == 6
    lines = open(out_csv).read().splitlines()
    head = lines[0].split(',')
    for ln in lines[1:]:
        cells = dict(zip(head, ln.split(',')))
        got = np.array([float(cells['ap@%.2f' % t]) if cells['ap@%.2f' % t] else np.nan for t in thr])
        want = res['map'] if cells['class'] == 'mean' else res['ap'][int(cells['class'])]
        assert np.allclose(got, want, rtol=0, atol=1e-12, equal_nan=True), (cells['class'], got, want)
    assert 'mAP50 = {:.4f}'.format(res['map50']) in r.stdout
