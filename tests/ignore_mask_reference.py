"""Torch statement of the opt-in ignore mask against each image's ground-truth boxes: y3_truth_boxes and y3_loss_fwd_bwd_truth
(include/yolo3hip.h).

Decode, box, class terms and the form of the objectness term are oracle.model's / box_loss_reference's; only the mask is stated
here: a prediction without an object is left out of the objectness loss when its decoded box overlaps a ground-truth box OF ITS
OWN IMAGE with IoU >= thr.  Any dtype: the tests use float64 with autograd (the mask is a constant of the backward pass) and
float32.  The threshold is rounded to float32 first, the value the kernel is handed.

Band rule: float32 on the device and float64 here may put a prediction on different sides of the threshold.  Comparisons of the
objectness gradient leave out the negatives whose float64 `best` lies within BAND of the threshold, and nothing else.  1e-4 is
about a hundred times the error of an IoU near 0.5 computed with a few dozen float32 roundings.
"""
import numpy as np
import torch

import box_loss_reference as R
from oracle import model as om

BAND = 1e-4
MIN_IGNORED = 20        # a case of the gradient comparison has at least this many ignored negatives ...
MAX_BAND_SHARE = 0.01   # ... of which at most this share lies in the band
CASES = R.CASES         # the inputs of tests/test_gpu_box_loss.py, reused
MODEL_CASE = R.MODEL_CASE


def truth_boxes(gt):
    """gt [N, Gh, Gw, A, 5+K] -> list of N tensors [count_i, 4]: the (cx, cy, w, h) of the rows with gt[..., 4] != 0 in index order
    (row, column, anchor).  What y3_truth_boxes writes, without the capacity cut."""
    g = gt.reshape(gt.shape[0], -1, gt.shape[-1])
    return [g[i][g[i][:, 4] != 0][:, 0:4].clone() for i in range(g.shape[0])]


def best_iou(pred, truth):
    """pred [N, Gh, Gw, A, 4] (cx, cy, w, h); truth: list of N [count_i, 4] -> [N, Gh, Gw, A]: the best IoU of each prediction with
    the boxes of its own image, from corners c -+ s/2, a NaN IoU dropped, -inf for an empty list."""
    best = torch.full(pred.shape[:-1], float('-inf'), dtype=pred.dtype)
    for i, tb in enumerate(truth):
        if tb.shape[0] == 0:
            continue
        tb = tb.to(pred.dtype)
        p = pred[i].unsqueeze(-2)                                    # [Gh, Gw, A, 1, 4]
        px0, px1 = p[..., 0] - p[..., 2] / 2.0, p[..., 0] + p[..., 2] / 2.0
        py0, py1 = p[..., 1] - p[..., 3] / 2.0, p[..., 1] + p[..., 3] / 2.0
        tx0, tx1 = tb[:, 0] - tb[:, 2] / 2.0, tb[:, 0] + tb[:, 2] / 2.0
        ty0, ty1 = tb[:, 1] - tb[:, 3] / 2.0, tb[:, 1] + tb[:, 3] / 2.0
        ix = torch.clamp(torch.minimum(px1, tx1) - torch.maximum(px0, tx0), min=0.0)
        iy = torch.clamp(torch.minimum(py1, ty1) - torch.maximum(py0, ty0), min=0.0)
        inter = ix * iy
        iou = inter / (p[..., 2] * p[..., 3] + tb[:, 2] * tb[:, 3] - inter)
        iou = torch.where(torch.isnan(iou), torch.full_like(iou, float('-inf')), iou)
        best[i] = iou.max(dim=-1).values
    return best


def loss_layer_truth(fm, gt, img_size, anchors, num_classes, box_loss, box_weight, truth, thr, info=None):
    """(box, wh, obj, class), each / local batch, of one scale with the truth mask: fm NCHW [N, A*(5+K), Gh, Gw], gt
    [N, Gh, Gw, A, 5+K], truth as truth_boxes() gives it (already cut to the capacity, if any).  Box, wh and class are
    box_loss_reference.loss_layer_ex's.  ``info`` (optional dict) receives loss_layer_ex's entries and 'best' [N, Gh, Gw, A],
    'negative' and 'ignored' (bool: without an object and left out of the objectness loss)."""
    parts = R.loss_layer_ex(fm, gt, img_size, anchors, num_classes, box_loss, box_weight, info)
    _, pred, obj_logits, _ = om.reorg_layer(fm, img_size, anchors, num_classes)
    gt = gt.to(fm.dtype)
    gm = gt[..., 4:5]
    best = best_iou(pred.detach(), truth)
    thr = torch.tensor(float(np.float32(thr)), dtype=fm.dtype)
    ignore = (best < thr).to(fm.dtype).unsqueeze(-1)
    valid = (gm + (1 - gm) * ignore).detach()
    obj = (valid * om._sigmoid_ce(gm.detach(), obj_logits)).sum() / float(fm.shape[0])
    if info is not None:
        info['best'] = best
        info['negative'] = gt[..., 4] == 0
        info['ignored'] = info['negative'] & ~(best < thr)
    return parts[0], parts[1], obj, parts[3]


def band(info, thr):
    """The negatives whose `best` lies within BAND of the (float32-rounded) threshold: [N, Gh, Gw, A] bool."""
    return info['negative'] & ((info['best'].double() - float(np.float32(thr))).abs() < BAND)


def counts(info, thr):
    """(negatives, ignored negatives, negatives in the band) of one loss_layer_truth call's ``info``."""
    return int(info['negative'].sum()), int(info['ignored'].sum()), int(band(info, thr).sum())


# ---- inputs of tests/test_gpu_ignore_mask.py, built here so that tests/test_cpu_ignore_mask.py can assert their conditions without a GPU
def make_case(name, empty=False):
    """box_loss_reference.make_case plus 'truth': the per-image lists of the finest label tensor."""
    c = R.make_case(name, empty=empty)
    c['truth'] = truth_boxes(c['gts'][2])
    return c


def case_counts(c, thr=0.5, dtype=torch.float64):
    """(negatives, ignored, band members) summed over the three scales of a case."""
    tot = np.zeros(3, np.int64)
    img = (c['hw'][0], c['hw'][1], 3)
    for fm, gt in zip(c['fms'], c['gts']):
        info = {}
        loss_layer_truth(fm.to(dtype), gt.to(dtype), img, c['anchors'], c['K'], 'mse', 1.0, c['truth'], thr, info)
        tot += np.array(counts(info, thr))
    return tuple(int(v) for v in tot)


EDGE_ANCHORS = [(64, 384), (384, 64)]
EDGE_K = 2
FAR = -1.0e4        # centre of the filler boxes of an edge list: they overlap no prediction


def make_edge_case(n, grid, count, decide_at, seed):
    """One scale without objects, logits N(0, 1.2^2), and a synthetic list of ``count`` boxes per image fed directly.  Image i
    plants prediction (last cell, anchor i % A): the box at list index ``decide_at`` (None: nowhere) is that prediction's own
    decoded box (IoU 1 with it); every other entry is a 10 x 10 box centred at FAR.  With decide_at = count - 1 a dropped tail
    chunk shows; with decide_at at or past a capacity the planted prediction must stay valid.
    -> dict(n, hw, anchors, K, fm [n, A*(5+K), Gh, Gw] float32, gt (all zero), lists [n, count, 4] float32, planted [(i, gy, gx, a)])."""
    gh, gw = grid
    A, D = len(EDGE_ANCHORS), 5 + EDGE_K
    hw = (gh * 32, gw * 32)
    g = torch.Generator().manual_seed(seed)
    fm = torch.randn(n, A * D, gh, gw, generator=g) * 1.2
    gt = torch.zeros(n, gh, gw, A, D)
    _, pred, _, _ = om.reorg_layer(fm.double(), (hw[0], hw[1], 3), EDGE_ANCHORS, EDGE_K)
    lists = torch.zeros(n, count, 4)
    lists[..., 0:2] = FAR
    lists[..., 2:4] = 10.0
    planted = []
    for i in range(n):
        a = i % A
        planted.append((i, gh - 1, gw - 1, a))
        if decide_at is not None and count:
            lists[i, decide_at] = pred[i, gh - 1, gw - 1, a].float()
    return dict(n=n, hw=hw, anchors=EDGE_ANCHORS, K=EDGE_K, fm=fm, gt=gt, lists=lists, planted=planted)


def make_step_labels(seed, n, hw, anchors, num_classes, per_image):
    """Three label tensors of a batch whose image i has per_image[i] random boxes (0 = an image without boxes)."""
    rng = np.random.default_rng(seed)
    parts = [R.make_labels(rng, 1, hw, anchors, num_classes, int(k)) for k in per_image]
    assert len(parts) == n
    return [np.concatenate([p[s] for p in parts], 0) for s in range(3)]
