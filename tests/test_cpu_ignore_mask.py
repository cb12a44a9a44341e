"""Opt-in ignore mask against each image's ground-truth boxes, the part that needs no GPU: the restatement
(tests/ignore_mask_reference.py) by hand and the band conditions of every input tests/test_gpu_ignore_mask.py compares gradients
on, the host-side validation, the CLI flags, and the C ABI with its argument checks."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import ignore_mask_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
F64 = torch.float64


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_truth_boxes_by_hand():
    gt = torch.zeros(2, 2, 2, 2, 7)
    gt[0, 0, 1, 1, 0:5] = torch.tensor([10., 20., 30., 40., 1.])
    gt[0, 1, 0, 0, 0:5] = torch.tensor([50., 60., 70., 80., 1.])
    gt[0, 0, 0, 1, 0:5] = torch.tensor([1., 2., 3., 4., 1.])
    lists = M.truth_boxes(gt)
    assert [tuple(l.shape) for l in lists] == [(3, 4), (0, 4)]
    assert lists[0].tolist() == [[1., 2., 3., 4.], [10., 20., 30., 40.], [50., 60., 70., 80.]]      # row, column, anchor order


def test_best_iou_by_hand():
    pred = torch.tensor([[100., 100., 40., 40.], [300., 300., 10., 10.]], dtype=F64).reshape(2, 1, 1, 1, 4)
    truth = [torch.tensor([[100., 100., 20., 20.], [120., 100., 40., 40.]], dtype=F64), torch.zeros(0, 4, dtype=F64)]
    best = M.best_iou(pred, truth)
    assert abs(float(best[0, 0, 0, 0]) - 800. / 2400.) < 1e-15            # the shifted box wins over the inner one (0.25)
    assert float(best[1, 0, 0, 0]) == float('-inf')                        # an empty list masks nothing
    # image 1's prediction is not compared with image 0's boxes, and a NaN IoU (0 / 0) is dropped
    truth = [torch.zeros(0, 4, dtype=F64), torch.tensor([[0., 0., 0., 0.], [300., 300., 10., 10.]], dtype=F64)]
    pred[0, 0, 0, 0] = torch.tensor([300., 300., 10., 10.], dtype=F64)
    best = M.best_iou(pred, truth)
    assert float(best[0, 0, 0, 0]) == float('-inf') and float(best[1, 0, 0, 0]) == 1.0
    pred[1, 0, 0, 0] = torch.tensor([0., 0., 0., 0.], dtype=F64)
    assert float(M.best_iou(pred, [truth[0], truth[1][:1]])[1, 0, 0, 0]) == float('-inf')


def test_only_the_objectness_term_departs_and_the_mask_is_constant():
    c = M.make_case('rect96x160')
    img = (c['hw'][0], c['hw'][1], 3)
    for kind in ('mse', 'ciou'):
        for fm, gt in zip(c['fms'], c['gts']):
            x = fm.double().requires_grad_(True)
            info = {}
            got = [p.detach() for p in M.loss_layer_truth(x, gt.double(), img, c['anchors'], c['K'], kind, 1.0, c['truth'], 0.5, info)]
            want = M.R.loss_layer_ex(fm.double(), gt.double(), img, c['anchors'], c['K'], kind, 1.0)
            assert float(got[0]) == float(want[0]) and float(got[1]) == float(want[1]) and float(got[3]) == float(want[3])
            assert not info['best'].requires_grad
            # a positive cell is never masked; an empty list leaves every negative valid
            assert not bool((info['ignored'] & info['positive']).any())
            e = {}
            none = M.loss_layer_truth(fm.double(), gt.double(), img, c['anchors'], c['K'], kind, 1.0, [t[:0] for t in c['truth']], 0.5, e)
            assert int(e['ignored'].sum()) == 0 and float(none[2]) >= float(got[2])
            # threshold 1: only an exact copy would be masked
            one = {}
            M.loss_layer_truth(fm.double(), gt.double(), img, c['anchors'], c['K'], kind, 1.0, c['truth'], 1.0, one)
            assert int(one['ignored'].sum()) == 0


@pytest.mark.parametrize('name', sorted(M.CASES))
def test_band_conditions_of_the_gpu_inputs(name):
    """The objectness-gradient comparisons of test_gpu_ignore_mask.py leave out the negatives within BAND of the threshold: on every
    input they use, those are at most 1 % of the ignored negatives, of which there are at least 20 -- in fp64 and in fp32 alike."""
    c = M.make_case(name)
    want = {'sq416': (27927, 804, 1), 'rect96x160': (3716, 22, 0)}[name]
    for dtype in (torch.float64, torch.float32):
        neg, ign, bnd = M.case_counts(c, 0.5, dtype)
        print(name, dtype, 'negatives', neg, 'ignored', ign, 'within %g of the threshold' % M.BAND, bnd)
        assert ign >= M.MIN_IGNORED and bnd <= M.MAX_BAND_SHARE * ign, (neg, ign, bnd)
        assert (neg, ign, bnd) == want
    assert M.BAND == 1e-4 and M.MIN_IGNORED == 20 and M.MAX_BAND_SHARE == 0.01
    assert sum(int(t.shape[0]) for t in c['truth']) > 0 and len(c['truth']) == c['n']
    assert all(int(t.shape[0]) == 0 for t in M.make_case(name, empty=True)['truth'])


def test_edge_case_builder():
    chunk = 256
    for n, grid in ((1, (1, 1)), (3, (2, 3)), (3, (13, 13))):
        c = M.make_edge_case(n, grid, chunk + 1, chunk, seed=7)
        img = (c['hw'][0], c['hw'][1], 3)
        info = {}
        M.loss_layer_truth(c['fm'].double(), c['gt'].double(), img, c['anchors'], c['K'], 'mse', 1.0, list(c['lists']), 0.5, info)
        for p in c['planted']:
            assert bool(info['ignored'][p]) and float(info['best'][p]) > 0.999999
        # the fillers alone decide nothing: with the deciding box past a capacity the planted prediction stays valid
        cut = {}
        M.loss_layer_truth(c['fm'].double(), c['gt'].double(), img, c['anchors'], c['K'], 'mse', 1.0, list(c['lists'][:, :chunk]), 0.5, cut)
        assert int(cut['ignored'].sum()) == 0 and float(cut['best'].max()) == 0.0


def test_step_labels_builder():
    gts = M.make_step_labels(3, 4, (96, 96), [(24, 24), (40, 40)], 2, [3, 0, 2, 1])
    assert [tuple(g.shape) for g in gts] == [(4, 3, 3, 2, 7), (4, 6, 6, 2, 7), (4, 12, 12, 2, 7)]
    lists = M.truth_boxes(torch.from_numpy(gts[2]))
    assert int(lists[1].shape[0]) == 0 and all(0 < int(lists[i].shape[0]) <= k for i, k in ((0, 3), (2, 2), (3, 1)))


# ---- host-side validation and the CLI -------------------------------------------------------------------------------------------
def test_host_argument_validation():
    from yolo3 import model
    assert model.IGNORE_MASKS == ('reference', 'truth')
    model.check_ignore_mask_args()
    model.check_ignore_mask_args('reference', 0.5, 1024)
    model.check_ignore_mask_args('truth', 0.5, 1024)
    model.check_ignore_mask_args('truth', 1.0, 1)
    model.check_ignore_mask_args('truth', 0.7, np.int64(4096))
    for bad in (('paper', 0.5, 1024), (None, 0.5, 1024), ('TRUTH', 0.5, 1024), ('truth', 0.0, 1024), ('truth', -0.1, 1024),
                ('truth', 1.0001, 1024), ('truth', float('nan'), 1024), ('truth', float('inf'), 1024), ('truth', None, 1024),
                ('truth', 'x', 1024), ('truth', True, 1024), ('truth', 0.5, 0), ('truth', 0.5, -3), ('truth', 0.5, 2.5),
                ('truth', 0.5, None), ('truth', 0.5, True), ('truth', 0.5, 2 ** 31),
                ('reference', 0.7, 1024), ('reference', 0.5, 512), ('reference', 0.7, 512)):
        with pytest.raises(ValueError):
            model.check_ignore_mask_args(*bad)
    # the constructor checks before it asks for a device (this machine may have none: a RuntimeError would mean it asked first)
    for kw in ({'ignore_mask': 'paper'}, {'ignore_mask': 'truth', 'ignore_thresh': 0.0}, {'ignore_thresh': 0.7}, {'max_truth_boxes': 16},
               {'ignore_mask': 'truth', 'max_truth_boxes': 0}):
        with pytest.raises(ValueError):
            model.YoloV3(4, [96, 96, 3], 2, **kw)


def test_train_cli_flags():
    sys.path.insert(0, PKG)
    import train
    from yolo3 import model
    assert train.IGNORE_MASKS == model.IGNORE_MASKS
    base = ['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c']
    parser = train.build_parser()
    text = ' '.join(parser.format_help().split())
    assert '--ignore_mask {reference,truth}' in text and '--ignore_thresh' in text and '--ignore_max_boxes' in text
    a = parser.parse_args(base)
    assert a.ignore_mask == 'reference' and a.ignore_thresh == 0.5 and a.ignore_max_boxes == 1024
    a = parser.parse_args(base + ['--ignore_mask', 'truth', '--ignore_thresh', '0.7', '--ignore_max_boxes', '64'])
    assert a.ignore_mask == 'truth' and a.ignore_thresh == 0.7 and a.ignore_max_boxes == 64
    for bad in (['--ignore_mask', 'paper'], ['--ignore_mask', 'truth', '--ignore_thresh', '0'], ['--ignore_mask', 'truth', '--ignore_thresh', '1.5'],
                ['--ignore_mask', 'truth', '--ignore_thresh', 'nan'], ['--ignore_mask', 'truth', '--ignore_max_boxes', '0'],
                ['--ignore_mask', 'truth', '--ignore_max_boxes', 'x'], ['--ignore_thresh', '0.7'], ['--ignore_max_boxes', '64']):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
    with pytest.raises(ValueError):      # checked before any reader or device is set up
        train.train_model(2, 3, 'a', 'b', 'c', 1, 1e-4, False, ignore_mask='reference', ignore_thresh=0.7)
    with pytest.raises(ValueError):
        train.train_model(2, 3, 'a', 'b', 'c', 1, 1e-4, False, ignore_mask='truth', ignore_thresh=0.0)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    from yolo3 import _hip
    text = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    m = re.search(r'#define\s+Y3_TRUTH_CHUNK\s+(\d+)\b', text)
    assert m and int(m.group(1)) >= 64
    assert 'model.py:250-282' in text
    m = re.search(r'int\s+y3_loss_fwd_bwd_truth\s*\(([^;]*)\)\s*;', text)
    assert m, 'y3_loss_fwd_bwd_truth is not declared'
    args = ' '.join(m.group(1).split())
    assert ('int box_loss, float box_weight, const float* truth_boxes, const int* truth_counts, int truth_cap, float ignore_thresh, '
            'float* loss4, float* ignored, const y3_tensor* dfm') in args
    assert re.search(r'int\s+y3_truth_boxes\s*\(\s*const float\*\s*gt,\s*int n,\s*long long cells_anchors,\s*int d,', text)
    for name in ('y3_truth_boxes', 'y3_loss_truth_workspace_bytes', 'y3_loss_fwd_bwd_truth'):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib, name), name
    assert len(_hip.SIGNATURES['y3_loss_fwd_bwd_truth'][1]) == len(_hip.SIGNATURES['y3_loss_fwd_bwd_ex'][1]) + 5
    for n in (1, 3, 8, 64):
        assert _hip.lib.y3_loss_truth_workspace_bytes(n) > 0
    assert _hip.lib.y3_loss_truth_workspace_bytes(8) >= 8 * 5 * 4
    assert _hip.lib.y3_loss_truth_workspace_bytes(0) == 0


def test_library_rejects_bad_arguments_before_launch():
    """Bad arguments are rejected on the host before any launch, with a message."""
    from yolo3 import _hip
    lib = _hip.lib
    anchors = _hip.float_array([64, 384, 384, 64])

    def loss(box_loss=0, box_weight=1.0, boxes=64, counts=64, cap=16, thr=0.5, ignored=64):
        # every pointer is a small integer: a launch would fault, so a clean return proves that the check came first
        t = _hip.Tensor(64, 1, 13, 13, 14, 16)
        return lib.y3_loss_fwd_bwd_truth(t, 64, anchors, 2, 2, 416, 416, 8.0, box_loss, box_weight, boxes, counts, cap, thr, 64, ignored, t, 64, None)
    for thr in (0.0, -0.5, 1.0001, 2.0, float('nan'), float('inf'), float('-inf')):
        assert loss(thr=thr) == -1 and b'ignore_thresh' in lib.y3_last_error(), thr
    for cap in (0, -1):
        assert loss(cap=cap) == -1 and b'truth_cap' in lib.y3_last_error(), cap
    assert loss(boxes=None) == -1 and b'null' in lib.y3_last_error()
    assert loss(counts=None) == -1 and b'null' in lib.y3_last_error()
    assert loss(box_loss=4) == -1 and b'box_loss' in lib.y3_last_error()
    assert loss(box_loss=-1) == -1 and b'box_loss' in lib.y3_last_error()
    assert loss(box_loss=0, box_weight=2.0) == -1 and b'box_weight' in lib.y3_last_error()
    for w in (0.0, -1.0, float('nan'), float('inf')):
        assert loss(box_loss=3, box_weight=w) == -1 and b'box_weight' in lib.y3_last_error(), w
    t = _hip.Tensor(0, 1, 13, 13, 14, 16)
    assert lib.y3_loss_fwd_bwd_truth(t, 64, anchors, 2, 2, 416, 416, 8.0, 0, 1.0, 64, 64, 16, 0.5, 64, None, t, 64, None) == -1
    assert b'null' in lib.y3_last_error()

    def gather(gt=64, n=3, ca=64, d=7, boxes=64, counts=64, cap=16):
        return lib.y3_truth_boxes(gt, n, ca, d, boxes, counts, cap, None)
    for kw in (dict(gt=None), dict(boxes=None), dict(counts=None)):
        assert gather(**kw) == -1 and b'null' in lib.y3_last_error(), kw
    for kw in (dict(n=0), dict(n=-1), dict(ca=0), dict(ca=-5), dict(ca=2 ** 31), dict(d=4), dict(cap=0), dict(cap=-1)):
        assert gather(**kw) == -1 and b'truth_boxes' in lib.y3_last_error(), kw
