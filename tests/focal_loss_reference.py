"""Torch statement of the opt-in focal loss and class-label smoothing of y3_loss_fwd_bwd_focal (include/yolo3hip.h).

Decode is oracle.model.reorg_layer's, the box terms and the reference's ignore mask are box_loss_reference.loss_layer_ex's, the truth
mask is ignore_mask_reference.loss_layer_truth's; only the objectness and class terms are stated here.  For a label z in [0, 1], a
logit x and p = sigmoid(x):

    ce = max(x, 0) - x z + log1p(exp(-|x|))                         (oracle.model._sigmoid_ce)
    m  = z sigmoid(-x) + (1 - z) sigmoid(x)                          (1 - p_t, formed without that subtraction)
    w  = alpha z + (1 - alpha)(1 - z) for alpha != 0, else 1
    FL = w m^gamma ce
    dFL/dx = w [m^gamma (p - z) + gamma m^gamma r (1 - 2z) ce],  r = p (1 - p) / m, r = 0 where m = 0

focal_term is valid in any dtype and differentiable by autograd; focal_grad is the closed form of the last line, which stays finite
where autograd of m**gamma need not (m -> 0 with gamma < 1).  Class labels are smoothed as Keras BinaryCrossentropy(label_smoothing)
does: z' = g (1 - eps) + eps / 2.  A term with gamma = alpha = 0 (and eps = 0 for class) is `neutral`: it is the base layer's own.

Band rule.  Under the truth mask the comparisons of dfm[..., 4] leave out the negatives whose fp64 best IoU lies within
ignore_mask_reference.BAND of the threshold, at most MAX_BAND_SHARE of the ignored negatives (ignore_mask_reference's rule, used as
it is).  Under the reference's mask nothing is left out: tests/test_cpu_focal_loss.py asserts that no negative of any fixed input
lies in the band around 0.5.
"""
import functools

import numpy as np
import torch

import box_loss_reference as R
import ignore_mask_reference as M
import loss_edges as E
from oracle import model as om

BAND, MAX_BAND_SHARE = M.BAND, M.MAX_BAND_SHARE
CASES = R.CASES
MODEL_CASE = R.MODEL_CASE
MASK_CASE = 'rect_only1'            # the label set of loss_edges.MASK_CASES used here: the reference mask ignores dozens of negatives
MIN_MASK_IGNORED = 24               # "dozens"
SATURATED_LOGITS = (-100.0, -30.0, 30.0, 100.0)     # and "as drawn"
NEUTRAL = (0.0, 0.0, 0.0, 0.0, 0.0)
FOCAL_TERMS = ('obj', 'class', 'both')


def term_args(gamma, alpha, terms, eps):
    """(gamma_obj, alpha_obj, gamma_cls, alpha_cls, eps): the term that ``terms`` leaves out gets gamma = alpha = 0."""
    if terms not in FOCAL_TERMS:
        raise ValueError('terms %r' % (terms,))
    obj = (float(gamma), float(alpha)) if terms in ('obj', 'both') else (0.0, 0.0)
    cls = (float(gamma), float(alpha)) if terms in ('class', 'both') else (0.0, 0.0)
    return obj + cls + (float(eps),)


def check_args(gamma, alpha, eps=0.0):
    if not (gamma >= 0.0 and np.isfinite(gamma)) or not (alpha == 0.0 or 0.0 < alpha < 1.0) or not 0.0 <= eps < 1.0:
        raise ValueError('gamma %r alpha %r label smoothing %r' % (gamma, alpha, eps))


def smooth(g, eps):
    return g * (1.0 - eps) + 0.5 * eps


def _weight(z, alpha):
    return alpha * z + (1.0 - alpha) * (1.0 - z) if alpha != 0.0 else torch.ones_like(z)


def focal_term(z, x, gamma, alpha):
    """FL(z, x) elementwise, any dtype; autograd differentiates it as written."""
    ce = om._sigmoid_ce(z, x)
    m = z * torch.sigmoid(-x) + (1.0 - z) * torch.sigmoid(x)
    mg = m ** gamma if gamma != 0.0 else torch.ones_like(m)
    return _weight(z, alpha) * mg * ce


def focal_grad(z, x, gamma, alpha):
    """dFL/dx elementwise in closed form (no m^(gamma - 1)): finite for every gamma >= 0 and every logit."""
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    ce = om._sigmoid_ce(z, x)
    m = z * q + (1.0 - z) * p
    mg = m ** gamma if gamma != 0.0 else torch.ones_like(m)
    r = torch.where(m > 0, (p * q) / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m))
    return _weight(z, alpha) * (mg * (p - z) + gamma * mg * r * (1.0 - 2.0 * z) * ce)


def focal_grad_scale(z, x, gamma, alpha):
    """The sum of the magnitudes of the two addends of focal_grad, elementwise: what a per-element error bound is relative to (the
    addends have opposite signs where a smoothed label lies between p and 1 - p, and their sum may cancel)."""
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    ce = om._sigmoid_ce(z, x)
    m = z * q + (1.0 - z) * p
    mg = m ** gamma if gamma != 0.0 else torch.ones_like(m)
    r = torch.where(m > 0, (p * q) / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m))
    return _weight(z, alpha) * (mg * (p - z).abs() + gamma * mg * r * (1.0 - 2.0 * z).abs() * ce)


def focal_grad_floor(z, x, gamma, alpha):
    """What fp64 rounding alone can put between two evaluations of dFL/dx, elementwise.  p - z, and the 1 - z - exp(-x) / (1 + exp(-x))
    that autograd forms for the same quantity, are differences of numbers of magnitude 1, each rounded to half an ulp (2^-53): where
    they cancel (z = 1 at x = 20: p - z = -2e-9) the error stays a few 2^-53 in absolute terms.  It reaches the derivative multiplied
    by w m^gamma, and by gamma ce r <= gamma ce in the second addend.  Sixteen such half-ulps."""
    ce = om._sigmoid_ce(z, x)
    m = z * torch.sigmoid(-x) + (1.0 - z) * torch.sigmoid(x)
    mg = m ** gamma if gamma != 0.0 else torch.ones_like(m)
    return 16.0 * 2.0 ** -53 * _weight(z, alpha) * mg * (1.0 + gamma * ce)


def neutral(gamma, alpha, eps=0.0):
    return gamma == 0.0 and alpha == 0.0 and eps == 0.0


def valid_mask(fm, gt, img_size, anchors, num_classes, truth=None, thr=0.5, info=None):
    """The factor of the objectness term, [N, Gh, Gw, A, 1], a constant of the backward pass: gm + (1 - gm) [best < threshold] with
    `best` against the reference's mask boxes (Q7; truth None) or against the image's own ground-truth boxes.  ``info`` receives
    'best' (-inf where there is nothing to compare with), 'negative', 'ignored' and 'band' [N, Gh, Gw, A]."""
    gt = gt.to(fm.dtype)
    gm = gt[..., 4:5]
    if truth is None:
        oi = {}
        om.loss_layer(fm.detach(), gt, img_size, anchors, num_classes, oi)
        best = oi['best_iou'] if oi['best_iou'] is not None else torch.full(gt.shape[:-1], float('-inf'), dtype=fm.dtype)
        thr = 0.5
    else:
        _, pred, _, _ = om.reorg_layer(fm.detach(), img_size, anchors, num_classes)
        best = M.best_iou(pred, [t.to(fm.dtype) for t in truth])
        thr = float(np.float32(thr))
    ignore = (best < thr).to(fm.dtype).unsqueeze(-1)
    if info is not None:
        info['best'] = best
        info['negative'] = gt[..., 4] == 0
        info['ignored'] = info['negative'] & ~(best < thr)
        info['band'] = info['negative'] & ((best.double() - thr).abs() < BAND)
    return (gm + (1 - gm) * ignore).detach()


def loss_layer_focal(fm, gt, img_size, anchors, num_classes, box_loss, box_weight, args, truth=None, thr=0.5, info=None):
    """(box, wh, obj, class), each / local batch, of one scale: fm NCHW [N, A*(5+K), Gh, Gw], gt [N, Gh, Gw, A, 5+K]; args as
    term_args gives them.  truth None: box_loss_reference.loss_layer_ex (the reference's mask); else
    ignore_mask_reference.loss_layer_truth with these per-image lists and threshold.  A neutral term is the base layer's own value."""
    go, ao, gc, ac, eps = args
    check_args(go, ao)
    check_args(gc, ac, eps)
    base_info = {}
    if truth is None:
        parts = R.loss_layer_ex(fm, gt, img_size, anchors, num_classes, box_loss, box_weight, base_info)
    else:
        parts = M.loss_layer_truth(fm, gt, img_size, anchors, num_classes, box_loss, box_weight, truth, thr, base_info)
    if info is not None:
        info.update(base_info)
    _, _, obj_logits, cls_logits = om.reorg_layer(fm, img_size, anchors, num_classes)
    g = gt.to(fm.dtype)
    gm = g[..., 4:5]
    B = float(fm.shape[0])
    valid = valid_mask(fm, gt, img_size, anchors, num_classes, truth, thr, info)
    obj, cls = parts[2], parts[3]
    if not neutral(go, ao):
        obj = (valid * focal_term(gm, obj_logits, go, ao)).sum() / B
    if not neutral(gc, ac, eps):
        cls = (gm * focal_term(smooth(g[..., 5:], eps), cls_logits, gc, ac)).sum() / B
    return parts[0], parts[1], obj, cls


def closed_form_channels(fm, gt, img_size, anchors, num_classes, args, valid):
    """d(obj + class)/d(logits) in closed form, [N, Gh, Gw, A, 1 + K] (objectness, then the classes), each / local batch."""
    go, ao, gc, ac, eps = args
    _, _, obj_logits, cls_logits = om.reorg_layer(fm.detach(), img_size, anchors, num_classes)
    g = gt.to(fm.dtype)
    gm = g[..., 4:5]
    B = float(fm.shape[0])
    return torch.cat([valid * focal_grad(gm, obj_logits, go, ao), gm * focal_grad(smooth(g[..., 5:], eps), cls_logits, gc, ac)], -1) / B


class Scale:
    """The fp64 reference of one scale of a case under one box loss and one mask, computed once: decode, mask and the gradient of the
    box terms do not depend on the focal arguments.  reference(args) then costs one elementwise pass."""

    def __init__(self, case, si, box_loss='mse', truth=None, thr=0.5, gbs=16.0):
        self.case, self.si, self.gbs = case, si, float(gbs)
        self.img = (case['hw'][0], case['hw'][1], 3)
        self.anchors, self.K = case['anchors'], case['K']
        self.A = len(self.anchors)
        self.fm, self.gt = case['fms'][si].double(), case['gts'][si].double()
        self.n, _, self.Gh, self.Gw = self.fm.shape
        self.box_loss, self.truth, self.thr = box_loss, (None if truth is None else [t.double() for t in truth]), thr
        x = self.fm.clone().requires_grad_(True)
        self.info = {}
        if self.truth is None:
            parts = R.loss_layer_ex(x, self.gt, self.img, self.anchors, self.K, box_loss, 1.0, self.info)
        else:
            parts = M.loss_layer_truth(x, self.gt, self.img, self.anchors, self.K, box_loss, 1.0, self.truth, thr, self.info)
        self.base_parts = np.array([float(p.detach()) for p in parts])
        box = parts[0] + parts[1]
        self.box_grad = torch.zeros(self.n, self.Gh, self.Gw, self.A, 5 + self.K, dtype=torch.float64)
        if box.requires_grad:
            (box / self.gbs).backward()
            self.box_grad = self.cells(x.grad)
        self.valid = valid_mask(self.fm, self.gt, self.img, self.anchors, self.K, self.truth, thr, self.info)

    def cells(self, t):
        return t.permute(0, 2, 3, 1).reshape(self.n, self.Gh, self.Gw, self.A, 5 + self.K)

    def reference(self, args):
        """-> (parts [4] numpy, dfm [n, Gh, Gw, A, 5+K] of sum(parts) / gbs with the objectness and class channels in closed form)"""
        with torch.no_grad():
            parts = loss_layer_focal(self.fm, self.gt, self.img, self.anchors, self.K, self.box_loss, 1.0, args, self.truth, self.thr)
            g = self.box_grad.clone()
            g[..., 4:] = closed_form_channels(self.fm, self.gt, self.img, self.anchors, self.K, args, self.valid) / self.gbs
        return np.array([float(p) for p in parts]), g

    def autograd(self, args):
        """The same through autograd of the restatement as written."""
        x = self.fm.clone().requires_grad_(True)
        parts = loss_layer_focal(x, self.gt, self.img, self.anchors, self.K, self.box_loss, 1.0, args, self.truth, self.thr)
        (sum(parts) / self.gbs).backward()
        return np.array([float(p.detach()) for p in parts]), self.cells(x.grad)


# ---- inputs of tests/test_gpu_focal_loss.py, built here so that tests/test_cpu_focal_loss.py can assert their conditions without a GPU
def _with_truth(c):
    c['truth'] = M.truth_boxes(c['gts'][2])
    return c


@functools.lru_cache(maxsize=None)
def make_case(name, empty=False):
    """'sq416' / 'rect96x160' (box_loss_reference.CASES), 'mask' (loss_edges' MASK_CASE: logits planted so that the reference mask
    fires), 'saturated', 'k1'; each with 'truth', the per-image lists of its finest label tensor.  Cached: do not modify."""
    if name in CASES:
        return _with_truth(R.make_case(name, empty=empty))
    if name == 'mask':
        c = E.make_mask_case(MASK_CASE, empty)
        return _with_truth(dict(c, fms=[f.clone() for f in c['fms']], gts=[g.clone() for g in c['gts']]))
    if name == 'saturated':
        return _with_truth(make_saturated_case(empty))
    if name == 'k1':
        return _with_truth(make_k1_case(empty))
    raise KeyError(name)


KERNEL_CASES = ('sq416', 'rect96x160', 'mask', 'saturated')      # every comparison against fp64 runs on these


def make_saturated_case(empty=False):
    """'rect96x160' (3 anchors, 3 classes) with each objectness and each class logit of every (cell, anchor), positives and negatives
    alike, drawn from SATURATED_LOGITS or left as drawn, five choices equally likely.  The box logits stay N(0, 1.2^2)."""
    c = R.make_case('rect96x160', empty=empty)
    rng = np.random.default_rng(521)
    A = len(c['anchors'])
    table = torch.tensor(SATURATED_LOGITS)
    for fm in c['fms']:
        f = E.cells(fm, A)
        pick = torch.from_numpy(rng.integers(0, 5, tuple(f.shape)))
        pick[..., 0:4] = 4
        f = torch.where(pick < 4, table[torch.clamp(pick, max=3)], f)
        fm.copy_(E.nchw(f))
    return c


def saturated_counts(c):
    """{(logit, 'pos' | 'neg'): entries of the objectness and class channels holding that planted logit} over the three scales."""
    out = {}
    A = len(c['anchors'])
    for fm, gt in zip(c['fms'], c['gts']):
        f = E.cells(fm, A)[..., 4:]
        pos = (gt[..., 4] != 0).unsqueeze(-1).expand_as(f)
        for v in SATURATED_LOGITS:
            out[(v, 'pos')] = out.get((v, 'pos'), 0) + int(((f == v) & pos).sum())
            out[(v, 'neg')] = out.get((v, 'neg'), 0) + int(((f == v) & ~pos).sum())
    return out


def make_k1_case(empty=False):
    """One class: 2 images of 64 x 96, two anchors, three boxes per image, logits N(0, 1.2^2)."""
    n, hw, anchors, K = 2, (64, 96), [(24, 24), (40, 40)], 1
    gts = R.make_labels(np.random.default_rng(523), n, hw, anchors, K, 0 if empty else 3)
    g = torch.Generator().manual_seed(527)
    fms = [(torch.randn(n, len(anchors) * (5 + K), hw[0] // s, hw[1] // s, generator=g) * 1.2) for s in (32, 16, 8)]
    return dict(n=n, hw=hw, anchors=anchors, K=K, fms=fms, gts=[torch.from_numpy(x) for x in gts])


def mask_counts(c, truth=False, thr=0.5):
    """(negatives, ignored, band members) over the three scales of a case, fp64, under the reference mask or the truth mask."""
    tot = np.zeros(3, np.int64)
    img = (c['hw'][0], c['hw'][1], 3)
    for fm, gt in zip(c['fms'], c['gts']):
        info = {}
        valid_mask(fm.double(), gt.double(), img, c['anchors'], c['K'], c['truth'] if truth else None, thr, info)
        tot += np.array([int(info[k].sum()) for k in ('negative', 'ignored', 'band')])
    return tuple(int(v) for v in tot)


# (gamma, alpha, terms, eps) of the kernel comparison: {2, 0.5, 1.5} x {0, 0.25} x {obj, class, both} x {0, 0.1} is 36 combinations;
# these 24 keep every (gamma, alpha, terms) triple of gamma 2 and every value of every factor under the other two gammas.
COMBINATIONS = tuple(
    [(2.0, a, t, e) for a in (0.0, 0.25) for t in FOCAL_TERMS for e in (0.0, 0.1)]
    + [(0.5, 0.0, 'obj', 0.1), (0.5, 0.25, 'obj', 0.0), (0.5, 0.25, 'class', 0.1), (0.5, 0.0, 'class', 0.0), (0.5, 0.0, 'both', 0.0),
       (0.5, 0.25, 'both', 0.1)]
    + [(1.5, 0.25, 'obj', 0.1), (1.5, 0.0, 'obj', 0.0), (1.5, 0.0, 'class', 0.1), (1.5, 0.25, 'class', 0.0), (1.5, 0.25, 'both', 0.0),
       (1.5, 0.0, 'both', 0.1)])
