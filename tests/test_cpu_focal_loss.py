"""Opt-in focal loss and class-label smoothing, the part that needs no GPU: the restatement
(tests/focal_loss_reference.py) and its closed-form gradient against fp64 autograd, the conditions of every input
tests/test_gpu_focal_loss.py compares on, the host-side validation, the CLI flags, and the C ABI with its argument checks."""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import focal_loss_reference as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
F64 = torch.float64
R, M = F.R, F.M


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_focal_term_by_hand():
    x = torch.tensor([0.0, 2.0, -3.0], dtype=F64)
    for z in (0.0, 1.0, 0.05, 0.95):
        zt = torch.full_like(x, z)
        p = torch.sigmoid(x)
        pt = z * p + (1 - z) * (1 - p)
        ce = -(z * torch.log(p) + (1 - z) * torch.log(1 - p))
        for gamma in (0.0, 0.5, 2.0):
            for alpha in (0.0, 0.25):
                w = alpha * z + (1 - alpha) * (1 - z) if alpha else 1.0
                want = w * (1 - pt) ** gamma * ce
                got = F.focal_term(zt, x, gamma, alpha)
                assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max()), (z, gamma, alpha)
    # hard labels: the focal loss of Lin et al., -alpha_t (1 - p_t)^gamma log p_t
    assert abs(float(F.focal_term(torch.ones(1, dtype=F64), torch.zeros(1, dtype=F64), 2.0, 0.25)) - 0.25 * 0.25 * math.log(2.0)) < 1e-15
    assert abs(float(F.focal_term(torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64), 2.0, 0.25)) - 0.75 * 0.25 * math.log(2.0)) < 1e-15
    # smoothing, the Keras form
    sm = F.smooth(torch.tensor([0.0, 1.0], dtype=F64), 0.1).tolist()
    assert sm[0] == 0.05 and abs(sm[1] - 0.95) < 1e-15 and F.smooth(torch.tensor([0.0, 1.0], dtype=F64), 0.0).tolist() == [0.0, 1.0]
    assert F.term_args(2.0, 0.25, 'obj', 0.1) == (2.0, 0.25, 0.0, 0.0, 0.1) and F.term_args(2.0, 0.25, 'class', 0.0) == (0.0, 0.0, 2.0, 0.25, 0.0)
    assert F.term_args(1.5, 0.0, 'both', 0.0) == (1.5, 0.0, 1.5, 0.0, 0.0)


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def test_closed_form_is_autograd_elementwise():
    """Per element, not per tensor: each derivative within 1e-12 of the sum of the magnitudes of its two addends plus the rounding
    floor of that element (focal_grad_floor: a few 2^-53 times w m^gamma), so the tail of well-classified logits (derivatives of
    1e-9 down to 1e-26 at |x| = 20) is held to its own size."""
    x = torch.linspace(-20.0, 20.0, 401, dtype=F64)
    smallest = 1.0
    for z in (0.0, 1.0, 0.05, 0.95, 0.5):
        for gamma in (0.0, 0.5, 1.5, 2.0):
            for alpha in (0.0, 0.25):
                zt = torch.full_like(x, z)
                xv = x.clone().requires_grad_(True)
                F.focal_term(zt, xv, gamma, alpha).sum().backward()
                got = F.focal_grad(zt, x, gamma, alpha)
                scale = F.focal_grad_scale(zt, x, gamma, alpha)
                over = (got - xv.grad).abs() > 1e-12 * scale + F.focal_grad_floor(zt, x, gamma, alpha)
                assert not bool(over.any()), (z, gamma, alpha, x[over].tolist())
                assert _rel(got, xv.grad) <= 1e-12
                smallest = min(smallest, float(scale[scale > 0].min()))
    assert smallest < 1e-20          # the tail was there to be checked
    # gamma = 0, alpha = 0: the plain sigmoid cross-entropy and its gradient p - z
    z = torch.full_like(x, 0.95)
    assert torch.equal(F.focal_term(z, x, 0.0, 0.0), F.om._sigmoid_ce(z, x))
    assert _rel(F.focal_grad(z, x, 0.0, 0.0), torch.sigmoid(x) - z) <= 1e-15


@pytest.mark.parametrize('name', ['sq416', 'rect96x160', 'mask', 'k1'])
def test_closed_form_is_autograd_on_the_gpu_inputs(name):
    """The reference test_gpu_focal_loss.py compares with (closed-form objectness and class channels next to the autograd gradient
    of the box terms) equals autograd of the restatement as written, to 1e-12 of each tensor's largest magnitude, on every
    unsaturated input; under both masks and with an IoU box loss."""
    c = F.make_case(name)
    combos = F.COMBINATIONS if name != 'sq416' else F.COMBINATIONS[::4]
    for si in range(3):
        for kw in (dict(), dict(box_loss='ciou'), dict(truth=c['truth'])):
            s = F.Scale(c, si, **kw)
            for combo in (combos if not kw else combos[:2]):
                args = F.term_args(*combo)
                p1, g1 = s.reference(args)
                p2, g2 = s.autograd(args)
                assert np.array_equal(p1, p2), (name, si, combo)
                worst = max(_rel(g1, g2), _rel(g1[..., 4], g2[..., 4]), _rel(g1[..., 5:], g2[..., 5:]))
                assert worst <= 1e-12, (name, si, kw.keys(), combo, worst)
                # the box channels do not depend on the focal arguments
                assert torch.equal(g1[..., 0:4], s.box_grad[..., 0:4])


def test_saturated_case_is_finite_in_closed_form():
    c = F.make_case('saturated')
    counts = F.saturated_counts(c)
    print(counts)
    for v in F.SATURATED_LOGITS:
        assert counts[(v, 'pos')] >= 20 and counts[(v, 'neg')] >= 1000, counts
    for si in range(3):
        s = F.Scale(c, si)
        for combo in F.COMBINATIONS:
            parts, g = s.reference(F.term_args(*combo))
            assert np.all(np.isfinite(parts)) and bool(torch.isfinite(g).all()), (si, combo)
    # the limits, by hand, in float64 and in float32 (where sigmoid(-100) is 0: m = 0, r = 0)
    for dt in (F64, torch.float32):
        one, zero = torch.ones(1, dtype=dt), torch.zeros(1, dtype=dt)
        for gamma in (0.5, 2.0):
            # a confident correct prediction: no loss, no gradient
            assert abs(float(F.focal_grad(one, 100 * one, gamma, 0.25))) < 1e-30 and abs(float(F.focal_grad(zero, -100 * one, gamma, 0.25))) < 1e-30
            # a confident wrong one: m = 1, ce = 100, gradient w (p - z) (+ gamma r ce with r -> 0)
            assert abs(float(F.focal_grad(zero, 100 * one, gamma, 0.25)) - 0.75) < 1e-6
            assert abs(float(F.focal_grad(one, -100 * one, gamma, 0.25)) + 0.25) < 1e-6
            assert abs(float(F.focal_term(zero, 100 * one, gamma, 0.25)) - 75.0) < 1e-4
        g = F.focal_grad(torch.tensor([0.0, 1.0, 0.05, 0.95], dtype=dt).repeat(4), torch.tensor(F.SATURATED_LOGITS, dtype=dt).repeat_interleave(4), 0.5, 0.0)
        assert bool(torch.isfinite(g).all())


def test_neutral_arguments_are_the_base_layers():
    for name in ('rect96x160', 'mask'):
        c = F.make_case(name)
        img = (c['hw'][0], c['hw'][1], 3)
        for fm, gt in zip(c['fms'], c['gts']):
            for kind in ('mse', 'ciou'):
                want = R.loss_layer_ex(fm.double(), gt.double(), img, c['anchors'], c['K'], kind, 1.0)
                got = F.loss_layer_focal(fm.double(), gt.double(), img, c['anchors'], c['K'], kind, 1.0, F.NEUTRAL)
                assert all(float(a) == float(b) for a, b in zip(got, want))
                wt = M.loss_layer_truth(fm.double(), gt.double(), img, c['anchors'], c['K'], kind, 1.0, c['truth'], 0.5)
                gt_ = F.loss_layer_focal(fm.double(), gt.double(), img, c['anchors'], c['K'], kind, 1.0, F.NEUTRAL, c['truth'], 0.5)
                assert all(float(a) == float(b) for a, b in zip(gt_, wt))
                # stated through focal_term with gamma = alpha = eps = 0, the terms are the base layer's too (another summation: 1e-14)
                info = {}
                valid = F.valid_mask(fm.double(), gt.double(), img, c['anchors'], c['K'], None, 0.5, info)
                _, _, ol, cl = F.om.reorg_layer(fm.double(), img, c['anchors'], c['K'])
                g = gt.double()
                obj = float((valid * F.focal_term(g[..., 4:5], ol, 0.0, 0.0)).sum()) / fm.shape[0]
                cls = float((g[..., 4:5] * F.focal_term(F.smooth(g[..., 5:], 0.0), cl, 0.0, 0.0)).sum()) / fm.shape[0]
                assert abs(obj - float(want[2])) <= 1e-13 * obj and abs(cls - float(want[3])) <= 1e-13 * max(cls, 1e-300)
            # a focal setting changes its own term only
            one = F.loss_layer_focal(fm.double(), gt.double(), img, c['anchors'], c['K'], 'mse', 1.0, F.term_args(2.0, 0.25, 'obj', 0.0))
            base = R.loss_layer_ex(fm.double(), gt.double(), img, c['anchors'], c['K'], 'mse', 1.0)
            assert float(one[0]) == float(base[0]) and float(one[1]) == float(base[1]) and float(one[3]) == float(base[3])
            assert 0.0 < float(one[2]) < float(base[2])
            two = F.loss_layer_focal(fm.double(), gt.double(), img, c['anchors'], c['K'], 'mse', 1.0, F.term_args(2.0, 0.0, 'class', 0.1))
            assert float(two[2]) == float(base[2]) and 0.0 < float(two[3]) != float(base[3])
    with pytest.raises(ValueError):
        F.loss_layer_focal(fm.double(), gt.double(), img, c['anchors'], c['K'], 'mse', 1.0, (-1.0, 0.0, 0.0, 0.0, 0.0))


def test_band_conditions_of_the_gpu_inputs():
    """Under the reference's mask no negative of any fixed input lies within BAND of 0.5 in fp64: nothing is left out of a
    comparison there.  Under the truth mask the band members are at most MAX_BAND_SHARE of the ignored negatives."""
    assert F.BAND == M.BAND == 1e-4 and F.MAX_BAND_SHARE == M.MAX_BAND_SHARE == 0.01
    for name in F.KERNEL_CASES + ('k1',):
        c = F.make_case(name)
        neg, ign, bnd = F.mask_counts(c)
        tneg, tign, tbnd = F.mask_counts(c, truth=True)
        print(name, 'reference mask: negatives', neg, 'ignored', ign, 'band', bnd, '; truth mask: ignored', tign, 'band', tbnd)
        assert bnd == 0, (name, bnd)
        assert tbnd <= F.MAX_BAND_SHARE * tign, (name, tign, tbnd)
        if name == 'mask':
            assert ign >= F.MIN_MASK_IGNORED, ign       # the reference mask does fire on this one
        empty = F.make_case(name, empty=True)
        assert F.mask_counts(empty)[1:] == (0, 0) and all(int(t.shape[0]) == 0 for t in empty['truth'])
    assert F.MASK_CASE in F.E.MASK_CASES and F.make_case('k1')['K'] == 1


def test_no_input_has_a_positive_near_a_branch_of_the_iou_losses():
    """test_gpu_focal_loss.py compares whole gradient tensors under box_loss='ciou' and leaves out nothing but band negatives: no
    positive of its inputs is within box_loss_reference.KINK_PX of a branch of min / max / clamp."""
    for name in F.KERNEL_CASES + ('k1',):
        c = F.make_case(name)
        for si in range(3):
            kinks, positives = R.kink_share(F.Scale(c, si, 'ciou').info)
            assert kinks == 0 and positives > 0, (name, si, kinks, positives)


def test_combinations_cover_every_value_and_term():
    assert 20 <= len(F.COMBINATIONS) <= 28 and len(set(F.COMBINATIONS)) == len(F.COMBINATIONS)
    full = {(g, a, t, e) for g in (2.0, 0.5, 1.5) for a in (0.0, 0.25) for t in F.FOCAL_TERMS for e in (0.0, 0.1)}
    assert set(F.COMBINATIONS) <= full
    for col, values in enumerate(((2.0, 0.5, 1.5), (0.0, 0.25), F.FOCAL_TERMS, (0.0, 0.1))):
        for g in (2.0, 0.5, 1.5):
            assert {c[col] for c in F.COMBINATIONS if c[0] == g} >= (set(values) if col else {g}), (col, g)


# ---- host-side validation and the CLI -------------------------------------------------------------------------------------------
def test_host_argument_validation():
    from yolo3 import model
    assert model.FOCAL_TERMS == F.FOCAL_TERMS == ('obj', 'class', 'both')
    model.check_focal_args()
    model.check_focal_args(2.0, 0.25, 'both', 0.1)
    model.check_focal_args(0.0, 0.0, 'obj', 0.0)
    model.check_focal_args(0.5, 0.999, 'class', 0.999)
    model.check_focal_args(2, 0, 'obj', 0)
    model.check_focal_args(np.float32(1.5), np.float64(0.25), 'both', np.float32(0.1))
    for bad in ((-0.5, 0.0, 'both', 0.0), (float('nan'), 0.0, 'both', 0.0), (float('inf'), 0.0, 'both', 0.0), (None, 0.0, 'both', 0.0),
                ('x', 0.0, 'both', 0.0), (True, 0.0, 'both', 0.0),
                (2.0, -0.25, 'both', 0.0), (2.0, 1.0, 'both', 0.0), (2.0, 1.5, 'both', 0.0), (2.0, float('nan'), 'both', 0.0), (2.0, None, 'both', 0.0),
                (2.0, 'x', 'both', 0.0), (2.0, True, 'both', 0.0),
                (2.0, 0.25, 'objectness', 0.0), (2.0, 0.25, None, 0.0), (2.0, 0.25, 'BOTH', 0.0), (2.0, 0.25, 2, 0.0),
                (2.0, 0.25, 'both', -0.1), (2.0, 0.25, 'both', 1.0), (2.0, 0.25, 'both', float('nan')), (2.0, 0.25, 'both', float('inf')),
                (2.0, 0.25, 'both', None), (2.0, 0.25, 'both', 'x'), (2.0, 0.25, 'both', True)):
        with pytest.raises(ValueError):
            model.check_focal_args(*bad)
    assert model.focal_term_args(2.0, 0.25, 'obj', 0.1) == F.term_args(2.0, 0.25, 'obj', 0.1) == (2.0, 0.25, 0.0, 0.0, 0.1)
    assert model.focal_term_args(2.0, 0.25, 'class', 0.0) == (0.0, 0.0, 2.0, 0.25, 0.0)
    assert model.focal_term_args(1.5, 0.0, 'both', 0.0) == (1.5, 0.0, 1.5, 0.0, 0.0)
    # the constructor checks before it asks for a device (this machine may have none: a RuntimeError would mean it asked first)
    for kw in ({'focal_gamma': -1.0}, {'focal_gamma': 2.0, 'focal_alpha': 1.0}, {'focal_terms': 'all'}, {'label_smoothing': 1.0},
               {'focal_gamma': float('nan')}, {'label_smoothing': -0.1}):
        with pytest.raises(ValueError):
            model.YoloV3(4, [96, 96, 3], 2, **kw)


def test_default_arguments_select_no_focal_launch():
    """A model built without the arguments hands its plans no focal setting: the plan builder then emits the launches it emitted
    before (test_gpu_focal_loss.py asserts on the plan's loss_calls, which needs a device)."""
    from yolo3 import model
    sig = inspect.signature(model.YoloV3.__init__).parameters
    assert [sig[k].default for k in ('focal_gamma', 'focal_alpha', 'focal_terms', 'label_smoothing')] == [0.0, 0.0, 'both', 0.0]
    y = object.__new__(model.YoloV3)
    y.focal_gamma, y.focal_alpha, y.focal_terms, y.label_smoothing = 0.0, 0.0, 'both', 0.0
    assert y.focal_args() is None
    for terms in F.FOCAL_TERMS:
        y.focal_terms = terms
        assert y.focal_args() is None
    y.focal_gamma, y.focal_alpha, y.focal_terms, y.label_smoothing = 2.0, 0.25, 'obj', 0.1
    assert y.focal_args() == (2.0, 0.25, 0.0, 0.0, 0.1)
    y.focal_gamma, y.focal_alpha, y.focal_terms, y.label_smoothing = 0.0, 0.0, 'both', 0.1
    assert y.focal_args() == (0.0, 0.0, 0.0, 0.0, 0.1)


def test_train_cli_flags():
    sys.path.insert(0, PKG)
    import train
    from yolo3 import model
    assert train.FOCAL_TERMS == model.FOCAL_TERMS
    base = ['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c']
    parser = train.build_parser()
    text = ' '.join(parser.format_help().split())
    assert '--focal_gamma' in text and '--focal_alpha' in text and '--focal_terms {obj,class,both}' in text and '--label_smoothing' in text
    assert '--model_selection loss' in text and 'not comparable' in text
    a = parser.parse_args(base)
    assert a.focal_gamma == 0.0 and a.focal_alpha == 0.0 and a.focal_terms is None and a.label_smoothing == 0.0
    a = parser.parse_args(base + ['--focal_gamma', '2', '--focal_alpha', '0.25', '--focal_terms', 'obj', '--label_smoothing', '0.1'])
    assert a.focal_gamma == 2.0 and a.focal_alpha == 0.25 and a.focal_terms == 'obj' and a.label_smoothing == 0.1
    a = parser.parse_args(base + ['--label_smoothing', '0.1'])           # smoothing alone needs no focal term
    assert a.focal_gamma == 0.0 and a.label_smoothing == 0.1
    for bad in (['--focal_gamma', '-1'], ['--focal_gamma', 'nan'], ['--focal_gamma', 'inf'], ['--focal_gamma', 'x'],
                ['--focal_gamma', '2', '--focal_alpha', '1'], ['--focal_gamma', '2', '--focal_alpha', '-0.1'], ['--focal_gamma', '2', '--focal_alpha', 'nan'],
                ['--focal_gamma', '2', '--focal_terms', 'all'], ['--label_smoothing', '1'], ['--label_smoothing', '-0.1'], ['--label_smoothing', 'nan'],
                ['--focal_alpha', '0.25'], ['--focal_terms', 'obj'], ['--focal_terms', 'both'], ['--focal_gamma', '0', '--focal_alpha', '0.25'],
                ['--focal_gamma', '0', '--focal_terms', 'class'], ['--label_smoothing', '0.1', '--focal_alpha', '0.25']):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
    for kw in (dict(focal_alpha=0.25), dict(focal_terms='obj'), dict(focal_gamma=-1.0), dict(focal_gamma=2.0, focal_alpha=1.0),
               dict(label_smoothing=1.0), dict(focal_gamma=2.0, focal_terms='all')):
        with pytest.raises(ValueError):      # checked before any reader or device is set up
            train.train_model(2, 3, 'a', 'b', 'c', 1, 1e-4, False, **kw)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry():
    from yolo3 import _hip
    text = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    m = re.search(r'int\s+y3_loss_fwd_bwd_focal\s*\(([^;]*)\)\s*;', text)
    assert m, 'y3_loss_fwd_bwd_focal is not declared'
    args = ' '.join(m.group(1).split())
    truth = ' '.join(re.search(r'int\s+y3_loss_fwd_bwd_truth\s*\(([^;]*)\)\s*;', text).group(1).split())
    head, tail = truth.rsplit(', ', 1)
    assert args == head + ', float gamma_obj, float alpha_obj, float gamma_cls, float alpha_cls, float label_smoothing, ' + tail
    assert 'model.py:286-287' in text and 'model.py:293-294' in text          # the reference lines the entry stands beside
    assert 'y3_loss_fwd_bwd_focal' in _hip.SIGNATURES and hasattr(_hip.lib, 'y3_loss_fwd_bwd_focal')
    sig, base = _hip.SIGNATURES['y3_loss_fwd_bwd_focal'][1], _hip.SIGNATURES['y3_loss_fwd_bwd_truth'][1]
    assert len(sig) == len(base) + 5 and sig[:len(base) - 1] == base[:-1] and sig[-1] == base[-1] and sig[-6:-1] == [_hip.f32] * 5
    readme = open(os.path.join(ROOT, 'README.md')).read()
    n = len(re.findall(r'^(?:int|size_t|const char\*)\s+y3_\w+\s*\(', text, re.M))
    assert n == len(_hip.SIGNATURES) and '(%d extern "C" entry points' % n in readme


def test_library_rejects_bad_arguments_before_launch():
    """Bad arguments are rejected on the host before any launch, with a message."""
    from yolo3 import _hip
    lib = _hip.lib
    anchors = _hip.float_array([64, 384, 384, 64])

    def loss(focal=(2.0, 0.25, 2.0, 0.25, 0.1), box_loss=0, box_weight=1.0, boxes=64, counts=64, cap=16, thr=0.5, fm=64, gt=64, loss4=64, ws=64,
             anc=anchors):
        # every pointer is a small integer: a launch would fault, so a clean return proves that the check came first
        t = _hip.Tensor(fm, 1, 13, 13, 14, 16)
        return lib.y3_loss_fwd_bwd_focal(t, gt, anc, 2, 2, 416, 416, 8.0, box_loss, box_weight, boxes, counts, cap, thr, loss4, 64, t, ws,
                                         *focal, None)
    nan, inf = float('nan'), float('inf')
    for g in (-1.0, -1e-6, nan, inf, -inf):
        assert loss((g, 0.25, 2.0, 0.25, 0.1)) == -1 and b'gamma' in lib.y3_last_error(), g
        assert loss((2.0, 0.25, g, 0.25, 0.1)) == -1 and b'gamma' in lib.y3_last_error(), g
    for a in (-0.25, 1.0, 1.5, nan, inf):
        assert loss((2.0, a, 2.0, 0.25, 0.1)) == -1 and b'alpha' in lib.y3_last_error(), a
        assert loss((2.0, 0.25, 2.0, a, 0.1)) == -1 and b'alpha' in lib.y3_last_error(), a
    for e in (-0.1, 1.0, 2.0, nan, inf):
        assert loss((2.0, 0.25, 2.0, 0.25, e)) == -1 and b'label_smoothing' in lib.y3_last_error(), e
    # neutral arguments do not switch the other checks off, nor do valid focal ones
    for focal in ((0.0, 0.0, 0.0, 0.0, 0.0), (2.0, 0.25, 2.0, 0.25, 0.1)):
        for kw in (dict(fm=None), dict(gt=None), dict(loss4=None), dict(ws=None), dict(anc=None)):
            assert loss(focal, **kw) == -1 and b'null' in lib.y3_last_error(), kw
        # one list without the other is not the reference mask
        assert loss(focal, boxes=None) == -1 and b'null' in lib.y3_last_error()
        assert loss(focal, counts=None) == -1 and b'null' in lib.y3_last_error()
        for thr in (0.0, 1.5, nan):
            assert loss(focal, thr=thr) == -1 and b'ignore_thresh' in lib.y3_last_error(), thr
        assert loss(focal, cap=0) == -1 and b'truth_cap' in lib.y3_last_error()
        assert loss(focal, box_loss=4) == -1 and b'box_loss' in lib.y3_last_error()
        assert loss(focal, box_loss=0, box_weight=2.0) == -1 and b'box_weight' in lib.y3_last_error()
        assert loss(focal, box_loss=3, box_weight=nan) == -1 and b'box_weight' in lib.y3_last_error()
        # the reference mask (both lists null) still checks the rest
        assert loss(focal, boxes=None, counts=None, box_loss=7) == -1 and b'box_loss' in lib.y3_last_error()
        assert loss(focal, boxes=None, counts=None, fm=None) == -1 and b'null' in lib.y3_last_error()
