"""CPU tests of the opt-in NMS variants (y3_nms_per_class_ex): properties of the NumPy restatements in
tests/nms_variants_reference.py, the C ABI and its host-side argument checks, and the CLI flags' defaults."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nms_variants_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')


def _random_rows(rng, nb, K, size=400, wh=(20, 90), score=(0.05, 1.0)):
    rows = np.zeros((nb, 5 + K), np.float32)
    c = rng.uniform(0, size, (nb, 2))
    w = rng.uniform(wh[0], wh[1], (nb, 2))
    rows[:, 0:2] = c - w / 2
    rows[:, 2:4] = c + w / 2
    rows[:, 4] = rng.uniform(score[0], score[1], nb)
    rows[:, 5:] = rng.uniform(score[0], score[1], (nb, K))
    return rows


def _keys_desc(rows_np, cls, min_box, score_thr, clip=None):
    idx, _, s = ref.candidates(rows_np, cls, min_box, score_thr, clip)
    order = np.argsort(ref.order_keys(s, idx), kind='stable')[::-1]
    return idx[order].astype(np.int32), s[order]


def test_soft_linear_above_one_emits_every_candidate_in_key_order():
    rng = np.random.default_rng(1)
    rows = _random_rows(rng, 600, 2)
    for clip in (None, (300, 350)):
        out = ref.per_class(rows, 'soft-linear', 16, 0.1, 1.0, clip_wh=clip)
        for c, (r, s) in enumerate(out):
            want_r, want_s = _keys_desc(rows, c, 16, 0.1, clip)
            assert len(r) > 100
            assert np.array_equal(r, want_r)
            assert np.array_equal(s.view(np.uint32), want_s.view(np.uint32))


def test_soft_gaussian_tiny_sigma_is_hard_nms_at_zero():
    rng = np.random.default_rng(2)
    rows = _random_rows(rng, 500, 2)
    soft = ref.per_class(rows, 'soft-gaussian', 8, 0.1, 0.3, sigma=1e-30)
    hard = ref.per_class(rows, 'hard', 8, 0.1, 0.0)
    for (rs, ss), (rh, sh) in zip(soft, hard):
        assert len(rh) > 10
        assert np.array_equal(rs, rh)
        assert np.array_equal(ss.astype(np.float32), sh)     # a survivor's factor is exp(-0) = 1: scores unchanged


def test_diou_on_disjoint_boxes_is_hard():
    # a grid of boxes that do not touch: every IoU is 0, so both keep everything, in key order
    g = np.arange(12, dtype=np.float32) * 50
    x, y = np.meshgrid(g, g)
    n = x.size
    rows = np.zeros((n, 7), np.float32)
    rows[:, 0], rows[:, 1] = x.ravel(), y.ravel()
    rows[:, 2], rows[:, 3] = x.ravel() + 40, y.ravel() + 40
    rng = np.random.default_rng(3)
    rows[:, 4:] = rng.uniform(0.2, 1, (n, 3))
    for thr in (0.0, 0.3):
        d = ref.per_class(rows, 'diou', 0, 0.1, thr)
        h = ref.per_class(rows, 'hard', 0, 0.1, thr)
        for (rd, sd), (rh, sh) in zip(d, h):
            assert len(rd) == n and np.array_equal(rd, rh) and np.array_equal(sd, sh)


def test_diou_keeps_distant_centres_hard_suppresses():
    # IoU 0.34 > 0.3: hard drops the second box; the centre penalty rho2 / c2 = 33^2 / 2e4 brings DIoU's value to 0.285
    rows = np.array([[0, 0, 100, 100, 1, 0.9], [0, 0, 100, 34, 1, 0.8]], np.float32)
    assert len(ref.per_class(rows, 'hard', 0, 0.1, 0.3)[0][0]) == 1
    assert ref.per_class(rows, 'diou', 0, 0.1, 0.3)[0][0].tolist() == [0, 1]


def test_soft_linear_decay_by_hand():
    rows = np.array([[0, 0, 10, 10, 1, 0.81], [0, 0, 10, 5, 1, 0.64], [50, 50, 60, 60, 1, 0.49]], np.float32)
    r, s = ref.per_class(rows, 'soft-linear', 0, 0.1, 0.3)[0]
    assert r.tolist() == [0, 2, 1]                   # box 1 (IoU 0.5 with box 0) decays to 0.8 * 0.5 = 0.4 < 0.7
    assert s[1] == np.sqrt(np.float32(0.49)) and s[2] == np.sqrt(np.float32(0.64)) * (np.float32(1) - np.float32(0.5))


def test_header_declares_and_library_exports_the_variant_entries():
    from yolo3 import _hip
    hdr = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    for name, code in (('Y3_NMS_HARD', 0), ('Y3_NMS_DIOU', 1), ('Y3_NMS_SOFT_LINEAR', 2), ('Y3_NMS_SOFT_GAUSSIAN', 3)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, code), hdr), name
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('y3_nms_per_class_ex', 'y3_nms_workspace_bytes_ex'):
        assert re.search(r'\b%s\(' % name, hdr) and hasattr(lib, name) and name in _hip.SIGNATURES, name
    # the workspace query: hard / diou take y3_nms_workspace_bytes; soft nothing up to 8192 rows, its SoA state above
    for nb in (300, 7098, 22743):
        for m in (0, 1):
            assert _hip.lib.y3_nms_workspace_bytes_ex(8, nb, 2, m) == _hip.lib.y3_nms_workspace_bytes(8, nb, 2)
    assert _hip.lib.y3_nms_workspace_bytes_ex(8, 7098, 2, 2) == 0
    assert _hip.lib.y3_nms_workspace_bytes_ex(8, 22743, 2, 3) >= 8 * 2 * 22743 * 24
    assert _hip.lib.y3_nms_workspace_bytes_ex(8, 22743, 2, 3) <= _hip.lib.y3_nms_workspace_bytes(8, 22743, 2)


def test_library_rejects_bad_variant_arguments_before_launch():
    from yolo3 import _hip
    lib = _hip.lib

    def call(method, score_thr=0.1, sigma=0.5):
        return lib.y3_nms_per_class_ex(64, 1, 100, 2, method, 0.0, score_thr, 0.3, sigma, -1.0, -1.0, 64, 64, 64, 100, 64, 1 << 20, None)
    assert call(4) == -1 and b'method' in lib.y3_last_error()
    assert call(-1) == -1
    assert call(2, score_thr=0.0) == -1 and b'score_thr' in lib.y3_last_error()
    assert call(3, score_thr=-1.0) == -1
    assert call(3, sigma=0.0) == -1 and b'sigma' in lib.y3_last_error()
    assert call(3, sigma=float('nan')) == -1


def test_host_argument_validation():
    import torch
    from yolo3 import bbox_utils, metrics
    assert bbox_utils.NMS_METHODS == ('hard', 'diou', 'soft-linear', 'soft-gaussian')
    rows = torch.zeros(1, 10, 7)          # a CPU tensor: the checks must fire before anything touches a device
    for kw in ({'method': 'soft'}, {'method': 'soft-gaussian', 'sigma': 0.0}, {'method': 'soft-gaussian', 'sigma': -1.0},
               {'method': 'soft-linear', 'score_threshold': 0.0}, {'method': 'soft-gaussian', 'score_threshold': -0.1}):
        with pytest.raises(ValueError):
            bbox_utils.nms_device(rows, **kw)
        with pytest.raises(ValueError):
            bbox_utils.detect(rows, 0, **kw)
    bbox_utils.check_nms_args('hard', sigma=0.0, score_threshold=0.0)       # hard / diou ignore sigma and allow a zero threshold
    bbox_utils.check_nms_args('diou', sigma=-1.0, score_threshold=0.0)
    # the evaluator checks before it looks at itself or the rows (constructing one needs a device)
    with pytest.raises(ValueError):
        metrics.DetectionEvaluator.add_batch(None, rows, [np.zeros((0, 5))], 0, nms='greedy')
    with pytest.raises(ValueError):
        metrics.evaluate_examples(None, [], None, 0, 1, nms='soft-gaussian', nms_sigma=0)


def _help(script):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''), COLUMNS='200')
    r = subprocess.run([sys.executable, os.path.join(PKG, script), '--help'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return ' '.join(r.stdout.split())


@pytest.mark.parametrize('script', ['inference.py', 'inference_tiled.py', 'evaluate.py'])
def test_cli_nms_flags_default_to_hard(script):
    out = _help(script)
    assert '--nms {hard,diou,soft-linear,soft-gaussian}' in out
    assert 'hard (the reference\'s greedy NMS, default)' in out and '--nms-sigma' in out


def test_train_parser_defaults_to_hard():
    sys.path.insert(0, PKG)
    import train
    from yolo3 import bbox_utils
    base = ['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c']
    a = train.build_parser().parse_args(base)
    assert a.test_map_nms == 'hard' and a.test_map_nms_sigma == 0.5
    assert train.TEST_MAP_NMS_METHODS == bbox_utils.NMS_METHODS
    assert train.build_parser().parse_args(base + ['--test_map_nms', 'diou']).test_map_nms == 'diou'
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(base + ['--test_map_nms', 'greedy'])
