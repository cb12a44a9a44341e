"""Fixed inputs and rules for the branches of the default loss path (loss_kernel<Y3_BOX_LOSS_MSE, false> with loss_present /
loss_clear / loss_finalize) and of decode_kernel (csrc/detect.hip) that N(0, 1.2^2) logits never or almost never take.

Importable without a GPU: tests/test_cpu_loss_edges.py asserts every condition below on these inputs with the fp64 oracle alone
(oracle.model.loss_layer and its info['best_iou'], reorg_layer, decode); tests/test_gpu_loss_edges.py then runs the kernels on them.

  mask-dense cases   logits planted so that the ignore mask (quirk Q7) fires often, and four label sets that decide which anchors
                     are present: a kernel that ignored present[], or read a stale flag, would mask other negatives
  threshold case     a negative whose best IoU is exactly 0.5 in float32 and in float64: `best < 0.5` keeps it out of the loss
  gate cases         positives replanted on both sides of the prediction-side clip [0.01, 0.99] of the xy term and of the clamp
                     [1e-9, 1e9] of the wh term, next to negatives whose size logits overflow float32 expf
  underflow case     size logits of -110 on a few positives: float32 expf gives 0 and the reference's `== 0 -> 1` rule applies
  decode cases       1, 2 and 4 scales, K = 1, a non-square image, a batch that takes the grid-stride loop round twice, saturated
                     and overflowing logits

Band rules.  The ignore mask compares an IoU with 0.5: the objectness gradient of a negative whose fp64 best IoU lies within
ignore_mask_reference.BAND of 0.5 is left out of comparisons, and each mask-dense case has at least MIN_IGNORED ignored negatives of
which at most MAX_BAND_SHARE are in the band (the constants of ignore_mask_reference, used as they are).  The xy gate compares the
in-cell position with 0.01 / 0.99: see CLIP_BAND.
"""
import functools

import numpy as np
import torch

import box_loss_reference as R
from ignore_mask_reference import BAND, MAX_BAND_SHARE, MIN_IGNORED      # noqa: F401  (re-exported: the rule's constants)
from oracle import model as om

GBS = 16.0              # global batch of every loss comparison (test_gpu_box_loss.GBS)
MASK_R = 4              # the top-left MASK_R x MASK_R cells of every scale carry planted size logits
MASK_SIGMA = 0.25
MIN_ABSENT_ONLY = 10    # negatives per case that only a kernel ignoring present[] would mask

# The xy gate.  The reference computes the in-cell position as (sigmoid(t) + off) * stride / stride - off in float32 and passes the
# gradient where it lies in [0.01, 0.99].  Every stride used here is a power of two (asserted by reference()), so * stride / stride
# is exact; the last subtraction is exact as well (both operands are multiples of ulp(s + off) and the result is below 1).  What is
# left is the rounding of s + off, at most half an ulp of a number below off + 1, and the error of float32 sigmoid, a few 2^-24.
# The largest cell index used is 51 (the 52 x 52 scale of sq416), off + 1 <= 52 < 64, and float32 numbers in [32, 64) are 2^-18
# apart: the float32 position is within 2^-19 + a few 2^-24 < 2^-18 of the exact one.  Four such ulps:
CLIP_ULP = 2.0 ** -18
CLIP_BAND = 4 * CLIP_ULP            # 1.5e-5; sigmoid(+-4.5) and sigmoid(+-4.7) are about 1e-3 from the edges
MAX_CELL_INDEX = 51
CENTRE_LOGITS = (-6.0, -4.7, -4.5, 4.5, 4.7, 6.0)       # and "as drawn"
SIZE_LOGITS = (-21.0, -20.0, 20.0, 21.0, -30.0, 30.0)   # and "as drawn";  e^20 < 1e9 < e^21
OVERFLOW_LOGIT = 100.0              # float32 expf(100) = inf
UNDERFLOW_LOGIT = -110.0            # float32 expf(-110) = 0 exactly (the smallest denormal is e^-103.3); nothing is planted in
                                    # (-104, -87), where it is the implementation's business whether denormal results are flushed
MIN_PER_GATE = 5


# ---- layout -----------------------------------------------------------------------------------------------------------------------
def cells(fm, A):
    """NCHW [n, A*D, Gh, Gw] -> a copy as [n, Gh, Gw, A, D]."""
    n, c, Gh, Gw = fm.shape
    return fm.permute(0, 2, 3, 1).reshape(n, Gh, Gw, A, c // A).clone()


def nchw(f):
    """[n, Gh, Gw, A, D] -> NCHW [n, A*D, Gh, Gw] (a view where it can be)."""
    n, Gh, Gw, A, D = f.shape
    return f.reshape(n, Gh, Gw, A * D).permute(0, 3, 1, 2)


def present_anchors(gt):
    """The anchors with at least one object in the label tensor [n, Gh, Gw, A, 5+K] of one scale: what loss_present_kernel flags."""
    return [a for a in range(gt.shape[3]) if bool((gt[..., a, 4] != 0).any())]


def anchor_box_iou(pred, anchors):
    """pred [..., 4] (cx, cy, w, h) -> [..., Q]: the IoU with the origin-centred box of each of the Q anchors, in the operation
    order of oracle.model.loss_layer (broadcast_iou).  Quirk Q7: the mask boxes sit at the origin, not at the objects."""
    anc = torch.tensor(anchors, dtype=pred.dtype)
    pxy, pwh = pred[..., None, 0:2], pred[..., None, 2:4]
    imin = torch.maximum(pxy - pwh / 2.0, torch.zeros_like(anc) - anc / 2.0)
    imax = torch.minimum(pxy + pwh / 2.0, torch.zeros_like(anc) + anc / 2.0)
    iwh = torch.clamp(imax - imin, min=0.0)
    inter = iwh[..., 0] * iwh[..., 1]
    return inter / (pwh[..., 0] * pwh[..., 1] + anc[:, 0] * anc[:, 1] - inter)


# ---- the fp64 reference of one scale ----------------------------------------------------------------------------------------------
def reference(case, si, zero_size=None):
    """oracle.model.loss_layer with autograd in fp64 on scale ``si`` of a case.
    -> (parts [4] numpy, dfm [n, Gh, Gw, A, 5+K] of sum(parts) / GBS, info).  info: 'positive', 'negative', 'best' (the best IoU
    against the mask boxes, -inf where no anchor is present), 'ignored' and 'band' (negatives), 'obj_term' (the objectness term of a
    cell, counted as a valid negative, as it enters the objectness part), 'iou_q' [..., Q] against every anchor's box, 'present',
    'pr' [..., 2] the in-cell position the xy gate tests, 'pwh' [..., 2] the size ratio the wh clamp tests.
    zero_size: optional bool [n, Gh, Gw, A, 2]; those size logits are evaluated as 0 and get gradient 0 (underflow_rule)."""
    H, W = case['hw']
    anchors, K = case['anchors'], case['K']
    A = len(anchors)
    gt = case['gts'][si].double()
    xc = cells(case['fms'][si].double(), A)
    if zero_size is not None:
        xc[..., 2:4][zero_size] = 0.0
    xc.requires_grad_(True)
    fm = nchw(xc)
    n, _, Gh, Gw = fm.shape
    for s in (H // Gh, W // Gw):
        assert s & (s - 1) == 0, 'CLIP_BAND is derived for power-of-two strides'
    assert max(Gh, Gw) - 1 <= MAX_CELL_INDEX, 'CLIP_BAND is derived for cell indices up to %d' % MAX_CELL_INDEX
    oi = {}
    parts = om.loss_layer(fm, gt, (H, W, 3), anchors, K, oi)
    (sum(parts) / GBS).backward()
    grad = xc.grad.clone()
    if zero_size is not None:
        grad[..., 2:4][zero_size] = 0.0
    with torch.no_grad():
        off, pred, obj, _ = om.reorg_layer(fm, (H, W, 3), anchors, K)
        stride = torch.tensor([H // Gh, W // Gw], dtype=torch.float64)           # (s_y, s_x) applied to (x, y): Q6
        info = dict(positive=gt[..., 4] != 0, negative=gt[..., 4] == 0, present=present_anchors(gt))
        info['best'] = oi['best_iou'] if oi['best_iou'] is not None else torch.full(gt.shape[:-1], float('-inf'), dtype=torch.float64)
        info['ignored'] = info['negative'] & ~(info['best'] < 0.5)
        info['band'] = info['negative'] & ((info['best'] - 0.5).abs() < BAND)
        info['obj_term'] = om._sigmoid_ce(torch.zeros_like(obj), obj)[..., 0] / float(n)
        info['iou_q'] = anchor_box_iou(pred, anchors)
        info['pr'] = pred[..., 0:2] / stride - off
        info['pwh'] = pred[..., 2:4] / torch.tensor(anchors, dtype=torch.float64)
    return np.array([float(p.detach()) for p in parts]), grad, info


def absent_only(info):
    """Negatives that a kernel ignoring present[] would mask and a correct one does not: best IoU against the absent anchors' boxes
    >= 0.5 + BAND, best IoU against the present ones < 0.5 - BAND.  [n, Gh, Gw, A] bool."""
    Q = info['iou_q'].shape[-1]
    absent = [q for q in range(Q) if q not in info['present']]
    if not absent:
        return torch.zeros_like(info['negative'])
    away = info['iou_q'][..., absent].max(-1).values
    return info['negative'] & (away >= 0.5 + BAND) & (info['best'] < 0.5 - BAND)


def band_objectness_bound(info):
    """What band members can explain of a difference in the objectness part: float32 may put each of them on the other side of 0.5,
    which adds or removes its objectness term.  The sum of those terms."""
    return float(info['obj_term'][info['band']].sum())


def xy_gate(info):
    """[..., 2] int: -1 where the in-cell position is below 0.01, +1 above 0.99, 0 where the gate is open (0.01 <= p <= 0.99)."""
    p = info['pr']
    return (p > 0.99).to(torch.int64) - (p < 0.01).to(torch.int64)


def wh_gate(info):
    """[..., 2] int: -1 where size / anchor is below 1e-9, +1 above 1e9, 0 where the gate is open."""
    q = info['pwh']
    return (q > 1e9).to(torch.int64) - (q < 1e-9).to(torch.int64)


def clip_band(info):
    """Positives whose fp64 in-cell x or y lies within CLIP_BAND of 0.01 or 0.99: float32 may take the other side of the gate, so
    their xy gradient is left out of comparisons.  [n, Gh, Gw, A] bool."""
    p = info['pr']
    near = ((p - 0.01).abs() < CLIP_BAND) | ((p - 0.99).abs() < CLIP_BAND)
    return info['positive'] & near.any(-1)


# ---- mask-dense cases -------------------------------------------------------------------------------------------------------------
# name: (geometry of box_loss_reference.CASES, boxes per image, label seed, (w range, h range) per wanted anchor, wanted anchors)
MASK_CASES = {
    'sq416_both': ('sq416', 10, 431, {0: ((20, 60), (120, 200)), 1: ((120, 200), (20, 60))}, [0, 1]),
    'sq416_only0': ('sq416', 10, 433, {0: ((20, 60), (120, 200))}, [0]),
    'sq416_only1': ('sq416', 10, 439, {1: ((120, 200), (20, 60))}, [1]),
    'rect_only1': ('rect96x160', 6, 443, {1: ((80, 120), (60, 90))}, [1]),
}
MASK_LOGIT_SEED = 449


def make_shaped_labels(rng, n, hw, anchors, num_classes, per_image, shapes):
    """box_loss_reference.make_labels with the box sizes drawn from ``shapes`` ({anchor: ((w0, w1), (h0, h1))}, one entry picked per
    box), so that imagereader.format_boxes assigns the wanted anchors only."""
    from yolo3.imagereader import format_boxes
    H, W = hw
    keys = sorted(shapes)
    labs = [[], [], []]
    for _ in range(n):
        pick = rng.integers(0, len(keys), per_image)
        wh = np.array([[rng.integers(*shapes[keys[p]][0]), rng.integers(*shapes[keys[p]][1])] for p in pick]).reshape(per_image, 2)
        xy = np.stack([rng.integers(0, W - wh[:, 0]), rng.integers(0, H - wh[:, 1])], 1)
        boxes = np.concatenate([xy, wh, rng.integers(0, num_classes, (per_image, 1))], 1).astype(np.int32)
        lab = format_boxes(boxes, (H, W, 3), anchors, num_classes)
        for i in range(3):
            labs[i].append(lab[i])
    return [np.stack(l) for l in labs]


def plant_mask_logits(case, seed=MASK_LOGIT_SEED):
    """In the top-left MASK_R x MASK_R cells of every scale, every (image, cell, anchor a) gets size logits log(anchor_q / anchor_a) +
    N(0, MASK_SIGMA^2) for a random anchor q: a box about as large as the mask box of anchor q, close enough to the origin to overlap
    it by half.  Everything else stays N(0, 1.2^2)."""
    rng = np.random.default_rng(seed)
    anc = np.array(case['anchors'], np.float64)
    A = len(anc)
    for fm in case['fms']:
        f = cells(fm, A)
        n, Gh, Gw = f.shape[:3]
        rh, rw = min(MASK_R, Gh), min(MASK_R, Gw)
        q = rng.integers(0, A, (n, rh, rw, A))
        t = np.log(anc[q] / anc[None, None, None]) + rng.normal(0.0, MASK_SIGMA, (n, rh, rw, A, 2))
        f[:, :rh, :rw, :, 2:4] = torch.from_numpy(t).float()
        fm.copy_(nchw(f))


@functools.lru_cache(maxsize=None)
def make_mask_case(name, empty=False):
    """-> box_loss_reference.make_case's dict with planted logits and shaped labels (empty: no object anywhere).  Cached: do not
    modify what it returns."""
    geo, per_image, lseed, shapes, _ = MASK_CASES[name]
    c = R.make_case(geo, empty=True)
    plant_mask_logits(c)
    if not empty:
        n, hw, anchors, K = c['n'], c['hw'], c['anchors'], c['K']
        c['gts'] = [torch.from_numpy(x) for x in make_shaped_labels(np.random.default_rng(lseed), n, hw, anchors, K, per_image, shapes)]
    return c


@functools.lru_cache(maxsize=None)
def mask_reference(name, si, empty=False):
    """reference() of one scale of a mask-dense case, computed once."""
    return reference(make_mask_case(name, empty), si)


def mask_counts(name):
    """(positives, negatives, ignored, band members, absent-only negatives) summed over the three scales, and the per-scale ignored."""
    tot, per_scale = np.zeros(5, np.int64), []
    for si in range(3):
        _, _, info = mask_reference(name, si)
        row = [int(info[k].sum()) for k in ('positive', 'negative', 'ignored', 'band')] + [int(absent_only(info).sum())]
        tot += np.array(row)
        per_scale.append(row[2])
    return tuple(int(v) for v in tot), per_scale


# ---- the threshold itself ---------------------------------------------------------------------------------------------------------
THRESHOLD_CELL = (4, 0, 0)      # (gy, gx, anchor) on the 13 x 13 scale of sq416


@functools.lru_cache(maxsize=None)
def make_threshold_case():
    """The labels of 'sq416_only0' (anchor 0, 64 x 384, present) over logits N(0, 1.2^2), with one prediction per image planted on
    the coarse scale at cell (gy 4, gx 0), anchor 0: centre logits of -110 and size logits of 0.  float32 sigmoid(-110) is
    1 / (1 + inf) = 0 and expf(0) = 1, so the box is 64 x 384 at (0, 128) exactly; against the mask box 64 x 384 at the origin the
    overlap is 64 x 256 = 16384 = 2^14 of a union of 2 * 24576 - 16384 = 2^15: IoU = 0.5 with no rounding anywhere, in float64 as
    well (sigmoid(-110) = 2e-48 vanishes in every sum).  `best < 0.5` is false: the prediction is ignored.  `<=` would count it."""
    base = make_mask_case('sq416_only0')
    c = R.make_case('sq416', empty=True)
    c['gts'] = [g.clone() for g in base['gts']]
    gy, gx, a = THRESHOLD_CELL
    f = cells(c['fms'][0], 2)
    f[:, gy, gx, a, 0:2] = -110.0
    f[:, gy, gx, a, 2:4] = 0.0
    c['fms'][0].copy_(nchw(f))
    return c


# ---- gates of the MSE box terms ---------------------------------------------------------------------------------------------------
GATE_SEEDS = {'sq416': 461, 'rect96x160': 463}


@functools.lru_cache(maxsize=None)
def make_gate_case(name):
    """box_loss_reference.make_case(name) with its positives replanted: each centre logit drawn from CENTRE_LOGITS or left as drawn,
    each size logit from SIZE_LOGITS or left as drawn (seven choices each, equally likely).  A quarter of the cells without an object
    get size logits of OVERFLOW_LOGIT.  -> (case, overflow masks [n, Gh, Gw, A] per scale).  Cached: do not modify."""
    c = R.make_case(name)
    rng = np.random.default_rng(GATE_SEEDS[name])
    A = len(c['anchors'])
    masks = []
    for fm, gt in zip(c['fms'], c['gts']):
        f = cells(fm, A)
        pos = gt[..., 4] != 0
        box = f[..., 0:4][pos]                                       # [P, 4]
        pick = torch.from_numpy(rng.integers(0, 7, tuple(box.shape)))
        table = torch.tensor([CENTRE_LOGITS, CENTRE_LOGITS, SIZE_LOGITS, SIZE_LOGITS], dtype=box.dtype).t()       # [6, 4]
        planted = torch.gather(table, 0, torch.clamp(pick, max=5))
        box = torch.where(pick < 6, planted, box)
        over = torch.from_numpy(rng.random(tuple(pos.shape)) < 0.25) & ~pos
        f[..., 0:4][pos] = box
        f[..., 2:4][over] = OVERFLOW_LOGIT
        fm.copy_(nchw(f))
        masks.append(over)
    return c, masks


@functools.lru_cache(maxsize=None)
def gate_reference(name, si):
    return reference(make_gate_case(name)[0], si)


def gate_counts(name):
    """{'x': [below, inside, above], 'y': ..., 'w': ..., 'h': ..., 'edge': positives with an open xy gate and a centre logit of
    +-4.5, 'positives', 'clip_band', 'overflow'} over the three scales of a gate case."""
    case, masks = make_gate_case(name)
    out = dict(x=[0, 0, 0], y=[0, 0, 0], w=[0, 0, 0], h=[0, 0, 0], edge=0, positives=0, clip_band=0, overflow=0)
    for si in range(3):
        _, _, info = gate_reference(name, si)
        pos = info['positive']
        gx, gw = xy_gate(info)[pos], wh_gate(info)[pos]
        for key, col in (('x', gx[:, 0]), ('y', gx[:, 1]), ('w', gw[:, 0]), ('h', gw[:, 1])):
            for j, v in enumerate((-1, 0, 1)):
                out[key][j] += int((col == v).sum())
        t = cells(case['fms'][si], len(case['anchors']))[..., 0:2][pos]
        out['edge'] += int(((t.abs() == 4.5) & (gx == 0)).sum())
        out['positives'] += int(pos.sum())
        out['clip_band'] += int(clip_band(info).sum())
        out['overflow'] += int(masks[si].sum())
    return out


# ---- a size logit that underflows -------------------------------------------------------------------------------------------------
UNDERFLOW_PLANTS = ((True, False), (False, True), (True, True))      # (w, h) of the first three positives of each scale


@functools.lru_cache(maxsize=None)
def make_underflow_case():
    """'sq416' as drawn; the first three positives of each scale get UNDERFLOW_LOGIT as width logit, height logit and both.
    -> (case, planted masks [n, Gh, Gw, A, 2] per scale).  Cached: do not modify."""
    c = R.make_case('sq416')
    masks = []
    for fm, gt in zip(c['fms'], c['gts']):
        f = cells(fm, 2)
        idx = torch.nonzero(gt[..., 4] != 0)[:len(UNDERFLOW_PLANTS)]
        m = torch.zeros(tuple(gt.shape[:-1]) + (2,), dtype=torch.bool)
        for (i, gy, gx, a), wh in zip(idx.tolist(), UNDERFLOW_PLANTS):
            m[i, gy, gx, a] = torch.tensor(wh)
        f[..., 2:4][m] = UNDERFLOW_LOGIT
        fm.copy_(nchw(f))
        masks.append(m)
    return c, masks


def underflow_rule(case, si, planted):
    """The expected result where a size logit is UNDERFLOW_LOGIT.  In float32, which is what the reference's graph computes in,
    exp(-110) is exactly 0, so size / anchor is 0, `where(x == 0, 1, x)` replaces it by the constant 1 and the term is
    (log true_twh - log 1)^2 = (log true_twh - 0)^2.  The selected operand is a constant, so the gradient to the logit is exactly 0.
    float64 does not underflow (exp(-110) = 1.7e-48 is clamped to 1e-9 instead), so the oracle is evaluated with those logits set
    to 0 -- exp(0) = 1 gives the same log 1 = 0 -- and their gradient is set to 0.  -> reference()'s triple."""
    return reference(case, si, zero_size=planted)


def underflow_terms_by_hand(case, si, planted):
    """sum over the planted entries of (log(true size / anchor))^2 / n: their share of the wh part, from the labels alone."""
    gt = case['gts'][si].double()
    anc = torch.tensor(case['anchors'], dtype=torch.float64)
    ltw = torch.log(gt[..., 2:4] / anc)
    return float((ltw[planted] ** 2).sum()) / float(gt.shape[0])


# ---- decode -----------------------------------------------------------------------------------------------------------------------
# name: (n, (H, W), anchors, K, [(Gh, Gw, ld - D) per scale], seed)
DECODE_CASES = {
    'one_scale': (3, (64, 64), [(10, 14), (33, 23)], 2, [(2, 2, 0)], 471),
    'two_scales': (2, (64, 64), [(10, 14), (33, 23)], 2, [(2, 2, 2), (4, 4, 0)], 473),
    'four_scales_k1': (3, (64, 64), [(10, 14), (33, 23), (50, 40)], 1, [(2, 2, 0), (4, 4, 2), (8, 8, 5), (16, 16, 14)], 479),
    # Q6: x is multiplied by H // Gh and y by W // Gw.  With a 3 x 10 grid on 96 x 160 those are 32 and 16 the wrong way round
    'rect_q6': (2, (96, 160), [(32, 32), (128, 128), (256, 256)], 3, [(3, 10, 4), (6, 10, 0), (12, 20, 1)], 487),
    # 50 * (169 + 676 + 2704) * 3 = 532 350 rows of 8 floats > 2048 blocks * 256 threads: the grid-stride loop takes a second pass
    'second_pass': (50, (416, 416), [(32, 32), (128, 128), (256, 256)], 3, [(13, 13, 0), (26, 26, 4), (52, 52, 8)], 491),
}
DECODE_MAX_THREADS = 2048 * 256


@functools.lru_cache(maxsize=None)
def make_decode_case(name, extreme=False):
    """-> dict(n, hw, anchors, K, fms: float32 NCHW logits N(0, 1.5^2), lds, want: oracle.model.decode in fp64 [n, Nb, 5+K]).
    extreme: each centre / objectness / class logit becomes -30 or +30 with probability 1/6 each (saturated sigmoid), and a tenth of
    the rows gets OVERFLOW_LOGIT as width logit, height logit or both ('over' [n, Nb, 2] bool in row order)."""
    n, hw, anchors, K, grids, seed = DECODE_CASES[name]
    A, D = len(anchors), 5 + K
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    fms, over = [], []
    for Gh, Gw, _ in grids:
        fm = torch.randn(n, A * D, Gh, Gw, generator=g) * 1.5
        if extreme:
            f = cells(fm, A)
            pick = torch.from_numpy(rng.integers(0, 6, tuple(f.shape)))
            pick[..., 2:4] = 5
            f = torch.where(pick == 0, torch.full_like(f, -30.0), torch.where(pick == 1, torch.full_like(f, 30.0), f))
            kind = torch.from_numpy(rng.integers(0, 30, tuple(f.shape[:-1])))             # 0: w, 1: h, 2: both, else none
            m = torch.stack([(kind == 0) | (kind == 2), (kind == 1) | (kind == 2)], -1)
            f[..., 2:4][m] = OVERFLOW_LOGIT
            fm = nchw(f).contiguous()
            over.append(m.reshape(n, -1, 2))
        fms.append(fm)
    want = om.decode([f.double() for f in fms], (hw[0], hw[1], 3), anchors, K)
    c = dict(n=n, hw=hw, anchors=anchors, K=K, fms=fms, lds=[A * D + pad for _, _, pad in grids], want=want)
    if extreme:
        c['over'] = torch.cat(over, 1)
    return c
