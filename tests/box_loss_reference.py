"""Torch statement of the opt-in IoU box-regression losses of y3_loss_fwd_bwd_ex (include/yolo3hip.h).

Decode, ignore mask, objectness and class terms are oracle.model's (reorg_layer, and loss_layer itself for 'mse'); only
the box term is stated here.  Any dtype: the tests use float64 and autograd, the kernel is float32 with a hand-derived
backward.  alpha of CIoU is detached (a constant of the backward pass), torch.minimum / maximum / clamp hand the gradient
to the selected operand.
"""
import math

import torch

from oracle import model as om

BOX_LOSSES = ('mse', 'giou', 'diou', 'ciou')
KINK_PX = 1e-3      # gradient comparisons leave out positives closer than this to a branch of min / max / clamp


def box_term(pred, true, kind, info=None):
    """1 - X per box.  pred, true: [..., 4] as (cx, cy, w, h) in pixels.  ``info`` (optional dict) receives 'iou' and
    'kink_margin': the smallest |.| among px0-gx0, px1-gx1, py0-gy0, py1-gy1 and the two overlap extents before the clamp."""
    if kind not in BOX_LOSSES[1:]:
        raise ValueError('box term of %r' % (kind,))
    bx, by, bw, bh = pred[..., 0], pred[..., 1], pred[..., 2], pred[..., 3]
    g0, g1, g2, g3 = true[..., 0], true[..., 1], true[..., 2], true[..., 3]
    px0, px1, py0, py1 = bx - bw / 2.0, bx + bw / 2.0, by - bh / 2.0, by + bh / 2.0
    gx0, gx1, gy0, gy1 = g0 - g2 / 2.0, g0 + g2 / 2.0, g1 - g3 / 2.0, g1 + g3 / 2.0
    ixr = torch.minimum(px1, gx1) - torch.maximum(px0, gx0)
    iyr = torch.minimum(py1, gy1) - torch.maximum(py0, gy0)
    inter = torch.clamp(ixr, min=0.0) * torch.clamp(iyr, min=0.0)
    union = bw * bh + g2 * g3 - inter
    iou = inter / union
    cw = torch.maximum(px1, gx1) - torch.minimum(px0, gx0)
    ch = torch.maximum(py1, gy1) - torch.minimum(py0, gy0)
    if kind == 'giou':
        c_area = cw * ch
        x = iou - (c_area - union) / c_area
    else:
        c2 = cw * cw + ch * ch
        rho2 = (bx - g0) ** 2 + (by - g1) ** 2
        x = iou - rho2 / c2
        if kind == 'ciou':
            v = (4.0 / math.pi ** 2) * (torch.atan(g2 / g3) - torch.atan(bw / bh)) ** 2
            alpha = (v / ((1.0 - iou) + v + 1e-7)).detach()
            x = x - alpha * v
    if info is not None:
        info['iou'] = iou.detach()
        info['kink_margin'] = torch.stack([px0 - gx0, px1 - gx1, py0 - gy0, py1 - gy1, ixr, iyr], -1).detach().abs().min(-1).values
    return 1.0 - x


def loss_layer_ex(fm, gt, img_size, anchors, num_classes, box_loss, box_weight, info=None):
    """(box, 0, obj, class), each / local batch, of one scale: fm NCHW [N, A*(5+K), Gh, Gw], gt [N, Gh, Gw, A, 5+K].
    'mse' (box_weight 1) is oracle.model.loss_layer itself, (xy, wh, obj, class).  ``info`` (optional dict) receives
    'positive' [N, Gh, Gw, A] bool and 'kink_margin' [N, Gh, Gw, A] (inf where there is no object)."""
    if box_loss not in BOX_LOSSES:
        raise ValueError('box_loss must be one of %s, got %r' % (', '.join(BOX_LOSSES), box_loss))
    if not (float(box_weight) > 0 and math.isfinite(float(box_weight))) or (box_loss == 'mse' and float(box_weight) != 1.0):
        raise ValueError('box_weight %r with %s' % (box_weight, box_loss))
    parts = om.loss_layer(fm, gt, img_size, anchors, num_classes)
    gt = gt.to(fm.dtype)
    sel = gt[..., 4] != 0
    if info is not None:
        info['positive'] = sel
        info['kink_margin'] = torch.full(sel.shape, float('inf'), dtype=fm.dtype)
    if box_loss == 'mse':
        return parts
    _, pred, _, _ = om.reorg_layer(fm, img_size, anchors, num_classes)
    zero = torch.zeros((), dtype=fm.dtype)
    if not bool(sel.any()):       # a branch, not a product: cells without an object never reach the box term
        return zero, zero, parts[2], parts[3]
    sub = {}
    term = box_term(pred[sel], gt[sel][:, 0:4], box_loss, sub)
    if info is not None:
        info['kink_margin'][sel] = sub['kink_margin']
    box = (gt[sel][:, 4] * float(box_weight) * term).sum() / float(fm.shape[0])
    return box, zero, parts[2], parts[3]


# ---- the inputs of tests/test_gpu_box_loss.py: built here so that tests/test_cpu_box_loss.py can assert, without a GPU, that the
# ---- reference alone meets the kink-share condition on every one of them
CASES = {
    # name: (n, (H, W), anchors, K, boxes per image, label seed, logit seed)
    'sq416': (4, (416, 416), [(64, 384), (384, 64)], 2, 40, 131, 137),          # test_loss_fwd_bwd_matches_oracle's geometry, more boxes
    'rect96x160': (4, (96, 160), [(32, 32), (128, 128), (256, 256)], 3, 6, 231, 237),
}
MODEL_CASE = dict(img=96, n=4, seed=17)     # the model-level step: test_gpu_model._setup(96, 4, 17, False)


def make_labels(rng, n, hw, anchors, num_classes, per_image):
    """Three label tensors [n, Gh, Gw, A, 5+K] of ``per_image`` random integer boxes per image (imagereader.format_boxes)."""
    import numpy as np
    from yolo3.imagereader import format_boxes
    H, W = hw
    labs = [[], [], []]
    for _ in range(n):
        wh = np.stack([rng.integers(20, W // 2, per_image), rng.integers(20, H // 2, per_image)], 1)
        xy = np.stack([rng.integers(0, W - wh[:, 0]), rng.integers(0, H - wh[:, 1])], 1) if per_image else np.zeros((0, 2), int)
        boxes = np.concatenate([xy, wh, rng.integers(0, num_classes, (per_image, 1))], 1).astype(np.int32)
        lab = format_boxes(boxes, (H, W, 3), anchors, num_classes)
        for i in range(3):
            labs[i].append(lab[i])
    return [np.stack(l) for l in labs]


def make_case(name, empty=False):
    """-> dict(n, hw, anchors, K, fms: three float32 NCHW logit tensors N(0, 1.2^2), gts: three float32 label tensors)."""
    import numpy as np
    n, hw, anchors, K, per_image, lseed, fseed = CASES[name]
    gts = make_labels(np.random.default_rng(lseed), n, hw, anchors, K, 0 if empty else per_image)
    g = torch.Generator().manual_seed(fseed)
    fms = [(torch.randn(n, len(anchors) * (5 + K), hw[0] // s, hw[1] // s, generator=g) * 1.2) for s in (32, 16, 8)]
    return dict(n=n, hw=hw, anchors=anchors, K=K, fms=fms, gts=[torch.from_numpy(x) for x in gts])


def kink_share(info):
    """(positives closer than KINK_PX to a branch, positives) of one loss_layer_ex call's ``info``."""
    pos = info['positive']
    return int((info['kink_margin'][pos] < KINK_PX).sum()), int(pos.sum())


def make_extreme_case():
    """'sq416' with extreme logits.  Every positive: each centre logit drawn from {-30, +30, as it was}, each size logit from
    {+30, as it was}.  A size logit of -30 makes a box of 1e-11 px whose overlap extent with the target is its own width, which the
    kink rule counts as a branch point, so only the first positive of each scale gets size logits of -30 (finiteness is checked on
    all of them, the gradient under the rule).  Next to the positives, a quarter of the cells without an object get size logits of
    100: float32 expf overflows there and the box term must not be evaluated.  -> (case, overflow masks [n, Gh, Gw, A] per scale)."""
    import numpy as np
    c = make_case('sq416')
    rng = np.random.default_rng(331)
    A, D = len(c['anchors']), 5 + c['K']
    masks = []
    for fm, gt in zip(c['fms'], c['gts']):
        n, _, Gh, Gw = fm.shape
        f = fm.permute(0, 2, 3, 1).reshape(n, Gh, Gw, A, D).clone()
        pos = gt[..., 4] != 0
        box = f[..., 0:4][pos]                                      # [P, 4]
        pick = torch.from_numpy(rng.integers(0, 3, tuple(box.shape)))
        pick[:, 2:4] = torch.clamp(pick[:, 2:4], min=1)
        box = torch.where(pick == 0, torch.full_like(box, -30.0), torch.where(pick == 1, torch.full_like(box, 30.0), box))
        box[0, 2:4] = -30.0
        over = torch.from_numpy(rng.random((n, Gh, Gw, A)) < 0.25) & ~pos
        f[..., 0:4][pos] = box
        f[..., 2:4][over] = 100.0
        fm.copy_(f.reshape(n, Gh, Gw, A * D).permute(0, 3, 1, 2))
        masks.append(over)
    return c, masks
