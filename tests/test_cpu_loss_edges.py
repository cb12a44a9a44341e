"""The conditions of tests/test_gpu_loss_edges.py, asserted on its fixed inputs (tests/loss_edges.py) with the fp64 oracle alone: they
hold before a GPU is involved.  Every test prints the counts it asserts on."""
import math

import numpy as np
import pytest
import torch

import loss_edges as E
from oracle import model as om

F32 = torch.float32


def test_constants_are_the_projects():
    import ignore_mask_reference as M
    assert (E.BAND, E.MIN_IGNORED, E.MAX_BAND_SHARE) == (M.BAND, M.MIN_IGNORED, M.MAX_BAND_SHARE) == (1e-4, 20, 0.01)
    # the planted logits sit on the sides of the edges the helper says they do, about 1e-3 away
    sig = lambda t: 1.0 / (1.0 + math.exp(-t))
    assert 0.01 < sig(-4.5) < 0.012 and 0.988 < sig(4.5) < 0.99 and 0.008 < sig(-4.7) < 0.01 and 0.99 < sig(4.7) < 0.992
    assert min(abs(sig(t) - e) for t in (-4.7, -4.5) for e in (0.01,)) > 50 * E.CLIP_BAND
    assert math.exp(20) < 1e9 < math.exp(21) and math.exp(-21) < 1e-9 < math.exp(-20)
    # a few float32 ulps of off + 1 at the largest cell index
    ulp = float(np.spacing(np.float32(E.MAX_CELL_INDEX + 1)))
    assert ulp == E.CLIP_ULP and E.CLIP_BAND == 4 * ulp
    # float32 exp at the planted extremes
    assert float(torch.exp(torch.tensor(E.OVERFLOW_LOGIT, dtype=F32))) == float('inf')
    assert float(torch.exp(torch.tensor(E.UNDERFLOW_LOGIT, dtype=F32))) == 0.0 and math.exp(E.UNDERFLOW_LOGIT) > 0.0
    for t in E.CENTRE_LOGITS + E.SIZE_LOGITS + (E.OVERFLOW_LOGIT, E.UNDERFLOW_LOGIT):
        assert not -104.0 < t < -87.0


@pytest.mark.parametrize('name', sorted(E.MASK_CASES))
def test_mask_case_labels_assign_only_the_wanted_anchors(name):
    c = E.make_mask_case(name)
    wanted = E.MASK_CASES[name][4]
    for si in range(3):
        assert E.present_anchors(c['gts'][si]) == wanted, (name, si)
    assert all(E.present_anchors(g) == [] for g in E.make_mask_case(name, empty=True)['gts'])
    # the same planted logits under every label set of a geometry
    for other in E.MASK_CASES:
        if E.MASK_CASES[other][0] == E.MASK_CASES[name][0]:
            assert all(torch.equal(a, b) for a, b in zip(c['fms'], E.make_mask_case(other)['fms']))


@pytest.mark.parametrize('name', sorted(E.MASK_CASES))
def test_mask_case_conditions(name):
    """At least MIN_IGNORED ignored negatives per case, at most MAX_BAND_SHARE of them in the band, and for the cases with an absent
    anchor at least MIN_ABSENT_ONLY negatives that only a kernel ignoring present[] would mask."""
    (pos, neg, ign, bnd, absent), per_scale = E.mask_counts(name)
    print('%s: positives %d, negatives %d, ignored %d (%s per scale), band members %d, absent-only %d'
          % (name, pos, neg, ign, ' + '.join(str(v) for v in per_scale), bnd, absent))
    assert pos >= 20
    assert ign >= E.MIN_IGNORED and bnd <= E.MAX_BAND_SHARE * ign, (ign, bnd)
    if len(E.MASK_CASES[name][4]) < len(E.make_mask_case(name)['anchors']):
        assert absent >= E.MIN_ABSENT_ONLY, absent
    else:
        assert absent == 0
    for si in range(3):
        _, _, info = E.mask_reference(name, si)
        # the helper's per-anchor IoU is the oracle's: its best over the present anchors is info['best_iou'], bit for bit
        assert torch.equal(info['iou_q'][..., info['present']].max(-1).values, info['best'])
        assert not bool((info['ignored'] & info['positive']).any())
        # no anchor present: nothing is ignored
        _, _, none = E.mask_reference(name, si, True)
        assert int(none['ignored'].sum()) == 0 and bool((none['best'] == float('-inf')).all())


def test_the_mask_changes_the_loss_of_every_mask_case():
    """The ignored negatives carry a visible share of the objectness part: leaving the mask out would move it by more than ten times the 2e-5 the loss parts are compared at."""
    for name in sorted(E.MASK_CASES):
        for si in range(3):
            parts, _, info = E.mask_reference(name, si)
            dropped = float(info['obj_term'][info['ignored']].sum())
            print('%s scale %d: objectness part %.4f, terms of the ignored negatives %.4f' % (name, si, parts[2], dropped))
            assert dropped > 10 * 2e-5 * parts.max()


def test_threshold_case_is_exactly_on_the_threshold():
    c = E.make_threshold_case()
    gy, gx, a = E.THRESHOLD_CELL
    _, _, info = E.reference(c, 0)
    assert info['present'] == [0]
    assert bool(info['negative'][:, gy, gx, a].all())
    assert bool((info['best'][:, gy, gx, a] == 0.5).all()) and bool(info['ignored'][:, gy, gx, a].all())
    planted = torch.zeros_like(info['band'])
    planted[:, gy, gx, a] = True
    assert torch.equal(info['band'], planted)            # nothing else is within BAND of the threshold
    # float32, in the kernel's order of operations
    t = E.cells(c['fms'][0], 2)[:, gy, gx, a]
    one = torch.ones((), dtype=F32)
    s = one / (one + torch.exp(-t[:, 0:2]))
    assert bool((s == 0).all())
    bx, by = (s[:, 0] + gx) * 32.0, (s[:, 1] + gy) * 32.0
    bw, bh = torch.exp(t[:, 2]) * 64.0, torch.exp(t[:, 3]) * 384.0
    ix = torch.clamp(torch.minimum(bx + bw / 2, torch.tensor(32.0)) - torch.maximum(bx - bw / 2, torch.tensor(-32.0)), min=0)
    iy = torch.clamp(torch.minimum(by + bh / 2, torch.tensor(192.0)) - torch.maximum(by - bh / 2, torch.tensor(-192.0)), min=0)
    inter = ix * iy
    iou = inter / (bw * bh + 64.0 * 384.0 - inter)
    assert iou.dtype == F32 and bool((inter == 16384.0).all()) and bool((iou == 0.5).all())


@pytest.mark.parametrize('name', sorted(E.GATE_SEEDS))
def test_gate_case_conditions(name):
    """Every value of every gate is taken by at least MIN_PER_GATE positives, at most 1 % of the positives are in the clip band, no
    positive is near an edge of the wh clamp, and the overflowing negatives overlap no mask box."""
    k = E.gate_counts(name)
    print('%s: positives %d; [below, inside, above] x %s y %s w %s h %s; open xy gate at a logit of +-4.5: %d; clip band %d; '
          'overflowing negatives %d' % (name, k['positives'], k['x'], k['y'], k['w'], k['h'], k['edge'], k['clip_band'], k['overflow']))
    for key in 'xywh':
        assert min(k[key]) >= E.MIN_PER_GATE, (key, k[key])
    assert k['edge'] >= E.MIN_PER_GATE
    assert k['clip_band'] <= 0.01 * k['positives'] and k['clip_band'] == 0
    case, masks = E.make_gate_case(name)
    for si in range(3):
        parts, grad, info = E.gate_reference(name, si)
        pos, over = info['positive'], masks[si]
        assert int(over.sum()) > 10 and not bool((over & pos).any())
        assert bool((E.cells(case['fms'][si], len(case['anchors']))[..., 2:4][over] == E.OVERFLOW_LOGIT).all())
        # size / anchor of a positive is nowhere within a factor of e^0.2 of 1e-9 or 1e9 (21 - log 1e9 = 0.28): float32 takes the side fp64 takes
        lq = torch.log(info['pwh'][pos])
        assert float(torch.minimum((lq - math.log(1e9)).abs(), (lq + math.log(1e9)).abs()).min()) > 0.2
        # fp64: finite, and a closed gate is an exact zero of the gradient
        assert np.isfinite(parts).all() and bool(torch.isfinite(grad).all())
        assert bool((grad[..., 0:2][pos][E.xy_gate(info)[pos] != 0] == 0).all())
        assert bool((grad[..., 2:4][pos][E.wh_gate(info)[pos] != 0] == 0).all())
        assert bool((grad[..., 0:2][pos][E.xy_gate(info)[pos] == 0] != 0).all())
        # exp(100) fits a double: the IoU of an overflowing negative with every mask box is below 1e-30 (0 in float32: x / inf)
        assert float(info['iou_q'][over].max()) < 1e-30 and not bool(info['ignored'][over].any())
        assert bool((grad[..., 0:4][over] == 0).all())
        # float32: the size is inf, the overlap finite, the IoU with every mask box exactly 0
        _, pred32, _, _ = om.reorg_layer(case['fms'][si], (case['hw'][0], case['hw'][1], 3), case['anchors'], case['K'])
        assert pred32.dtype == F32 and bool(torch.isinf(pred32[..., 2:4][over]).all())
        assert bool((E.anchor_box_iou(pred32, case['anchors'])[over] == 0).all())


def test_underflow_case():
    case, plants = E.make_underflow_case()
    for si in range(3):
        m = plants[si]
        assert int(m.sum()) == 4 and int(m.any(-1).sum()) == 3
        pos = case['gts'][si][..., 4] != 0
        assert bool(pos[m.any(-1)].all())
        f = E.cells(case['fms'][si], 2)
        assert bool((f[..., 2:4][m] == E.UNDERFLOW_LOGIT).all()) and float(f[..., 2:4].max()) < 50.0       # never next to an overflow
        parts, grad, info = E.underflow_rule(case, si, m)
        assert bool((grad[..., 2:4][m] == 0).all())
        # the planted entries' share of the wh part is (log true_twh - 0)^2: take it away by evaluating them as log true_twh
        hand = E.underflow_terms_by_hand(case, si, m)
        c2 = dict(case, fms=[f_.clone() for f_ in case['fms']])
        anc = torch.tensor(case['anchors'])
        f2 = E.cells(c2['fms'][si], 2)
        f2[..., 2:4][m] = torch.log(case['gts'][si][..., 2:4] / anc)[m]
        c2['fms'][si].copy_(E.nchw(f2))
        without = E.reference(c2, si)[0]
        print('underflow scale %d: wh part %.6f, planted share %.6f by hand, %.6f by difference' % (si, parts[1], hand, parts[1] - without[1]))
        assert hand > 0.01 and abs((parts[1] - without[1]) - hand) <= 1e-6 * hand
        # the plain fp64 oracle, which does not underflow, says something else: log 1e-9 in place of log 1
        plain = E.reference(case, si)[0]
        assert plain[1] > parts[1] + 100.0


@pytest.mark.parametrize('name', sorted(E.DECODE_CASES))
def test_decode_cases(name):
    n, hw, anchors, K, grids, _ = E.DECODE_CASES[name]
    rows = n * sum(gh * gw for gh, gw, _ in grids) * len(anchors)
    c = E.make_decode_case(name)
    assert tuple(c['want'].shape) == (n, rows // n, 5 + K) and bool(torch.isfinite(c['want']).all())
    print('%s: %d scales, %d rows of %d floats, ld - D %s' % (name, len(grids), rows, 5 + K, [p for _, _, p in grids]))
    if name == 'second_pass':
        assert rows == 532350 and rows > E.DECODE_MAX_THREADS
    else:
        assert rows < 4096
    if name == 'rect_q6':
        assert (hw[0] // grids[0][0], hw[1] // grids[0][1]) == (32, 16)
    pads = [p for _, _, p in grids]
    assert 0 in pads and (len(grids) == 1 or (max(pads) > 0 and len(set(c['lds'])) == len(grids)))


def test_decode_extreme_case():
    for name in ('four_scales_k1', 'rect_q6'):
        c = E.make_decode_case(name, True)
        A, K = len(c['anchors']), c['K']
        sat = sum(int((E.cells(f, A)[..., [0, 1, 4]].abs() == 30.0).sum()) for f in c['fms'])
        over = c['over']
        print('%s extreme: rows %d, saturated centre / objectness logits %d, rows with an overflowing width %d, height %d, both %d'
              % (name, over.shape[0] * over.shape[1], sat, int(over[..., 0].sum()), int(over[..., 1].sum()), int(over.all(-1).sum())))
        assert sat > 50 and int(over[..., 0].sum()) >= 5 and int(over[..., 1].sum()) >= 5 and int(over.all(-1).sum()) >= 2
        want = c['want']
        assert bool(torch.isfinite(want).all()) and float(want[..., 4:].min()) >= 0.0 and float(want[..., 4:].max()) <= 1.0
        assert float(want[..., 2][over[..., 0]].min()) > 1e40
