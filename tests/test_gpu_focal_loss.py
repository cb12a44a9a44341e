"""y3_loss_fwd_bwd_focal (opt-in focal loss and class-label smoothing) on the GPU: bit for bit against
y3_loss_fwd_bwd_ex / y3_loss_fwd_bwd_truth wherever they must agree (both terms neutral: everything; otherwise the box channels,
loss4[0:2], the mask-only count and whatever belongs to a neutral term), against tests/focal_loss_reference.py in fp64 at the
tolerances of test_gpu_box_loss.py / test_gpu_ignore_mask.py (gradients 1e-4 of the largest reference magnitude of the tensor and of
the objectness / class channels alone, loss parts 2e-5 of the largest part and of the focal parts themselves), and through YoloV3 and
train.py.

The fp64 gradient is the closed form of focal_loss_reference.focal_grad (tests/test_cpu_focal_loss.py shows it equal to autograd of
the restatement to 1e-12 on every unsaturated input); it is what stays finite on the saturated case.  Band rule: under the truth
mask the negatives whose fp64 best IoU lies within 1e-4 of the threshold are left out of the objectness-gradient comparison, at most
1 % of the ignored negatives; under the reference's mask no input has such a negative (asserted here and, without a GPU, in
test_cpu_focal_loss.py) and nothing is left out.  Every comparison prints its figures before it asserts."""
import functools
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import focal_loss_reference as F
from test_gpu_box_loss import GBS, SENTINEL, _write_dataset
from test_gpu_ignore_mask import _TruthScale, _device_lists, _model, _model_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
R, M = F.R, F.M
CAP, THR = 1024, 0.5


@pytest.fixture(scope='module')
def hip():
    from yolo3 import _hip
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return _hip


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


class _FocalScale(_TruthScale):
    """test_gpu_ignore_mask._TruthScale plus the focal launch."""

    def launch_focal(self, kind, args, lists=None, with_ignored=True):
        """lists None: null truth lists = the reference's mask; else (boxes [n, CAP, 4], counts [n]) on the device.
        -> (loss4 [4], dfm buffer with its padding, ignored [1] or None)"""
        hip = self.hip
        buf, dv = self.nhwc_buf(self.n, self.Gh, self.Gw, self.D, ld=self.ld, fill=SENTINEL)
        loss4 = torch.zeros(4, device='cuda')
        ignored = torch.zeros(1, device='cuda') if lists is not None and with_ignored else None
        if lists is None:
            ws = torch.zeros(int(hip.lib.y3_loss_workspace_bytes()) // 4 + 4, device='cuda')
        else:
            ws = torch.full((int(hip.lib.y3_loss_truth_workspace_bytes(self.n)) // 4 + 4,), float('nan'), device='cuda')
        H, W = self.case['hw']
        tf_ = hip.Tensor(self.fv.data_ptr(), self.n, self.Gh, self.Gw, self.D, self.ld)
        td = hip.Tensor(dv.data_ptr(), self.n, self.Gh, self.Gw, self.D, self.ld)
        rc = hip.lib.y3_loss_fwd_bwd_focal(tf_, self.gd.data_ptr(), self.anc, self.A, self.K, H, W, GBS, R.BOX_LOSSES.index(kind), 1.0,
                                           None if lists is None else lists[0].data_ptr(), None if lists is None else lists[1].data_ptr(),
                                           CAP if lists is not None else 1, THR, loss4.data_ptr(),
                                           None if ignored is None else ignored.data_ptr(), td, ws.data_ptr(),
                                           *[float(v) for v in args], _stream())
        hip.check(rc, 'y3_loss_fwd_bwd_focal')
        self._keep = (ws, tf_, td, lists)
        return loss4, buf, ignored


# ---- shared, computed once: the device copy of each scale, its truth lists, the non-focal launches and the fp64 base ----------------
@functools.lru_cache(maxsize=None)
def _scale(name, si, empty=False):
    from yolo3 import _hip
    return _FocalScale(_hip, F.make_case(name, empty), si)


@functools.lru_cache(maxsize=None)
def _lists(name, empty=False):
    from yolo3 import _hip
    return _device_lists(_hip, F.make_case(name, empty)['gts'][2], CAP)


@functools.lru_cache(maxsize=None)
def _plain(name, si, kind, truth, empty=False):
    """The non-focal launch (y3_loss_fwd_bwd_ex, or y3_loss_fwd_bwd_truth) on the host: (loss4 [4], dfm buffer, ignored or None)"""
    s = _scale(name, si, empty)
    if truth:
        boxes, counts = _lists(name, empty)
        l, buf, ign = s.launch_truth(kind, boxes, counts, CAP, THR)
    else:
        (l, buf), ign = s.launch(kind), None
    torch.cuda.synchronize()
    return l.cpu(), buf.cpu(), None if ign is None else ign.cpu()


@functools.lru_cache(maxsize=None)
def _ref(name, si, kind, truth, empty=False):
    c = F.make_case(name, empty)
    return F.Scale(c, si, kind, c['truth'] if truth else None, THR, GBS)


def _check(name, si, kind, truth, args, empty=False):
    """One focal launch against the non-focal launch (bits) and against fp64 (tolerances).  -> band members left out"""
    what = '%s%s scale %d %s %s mask, args %s' % (name, ' (empty)' if empty else '', si, kind, 'truth' if truth else 'reference', (args,))
    s, ref = _scale(name, si, empty), _ref(name, si, kind, truth, empty)
    pl, pbuf, pign = _plain(name, si, kind, truth, empty)
    l, buf, ign = s.launch_focal(kind, args, _lists(name, empty) if truth else None)
    torch.cuda.synchronize()
    l, buf = l.cpu(), buf.cpu()
    got, plain = s.cells(buf), s.cells(pbuf)
    go, ao, gc, ac, eps = args
    # -- bits
    def differing(x, y):
        return int((_bits(x) != _bits(y)).sum())
    bits = {'padding': int((s.padding(buf) != SENTINEL).sum()), 'non-finite': int((~torch.isfinite(buf)).sum()) + int((~torch.isfinite(l)).sum()),
            'box channels': differing(got[..., 0:4], plain[..., 0:4]), 'loss4[0:2]': differing(l[0:2], pl[0:2])}
    if F.neutral(go, ao):
        bits['neutral objectness channel'], bits['neutral objectness part'] = differing(got[..., 4], plain[..., 4]), differing(l[2], pl[2])
    if F.neutral(gc, ac, eps):
        bits['neutral class channels'], bits['neutral class part'] = differing(got[..., 5:], plain[..., 5:]), differing(l[3], pl[3])
    if truth:
        bits['ignored'] = differing(ign.cpu(), pign)
    print('%s: floats whose bits differ from the non-focal launch / are out of place: %s' % (what, bits))
    assert not any(bits.values()), '%s: %s' % (what, bits)
    # -- fp64
    parts, gref = ref.reference(args)
    band = ref.info['band']
    n_band, n_ign = int(band.sum()), int(ref.info['ignored'].sum())
    g, w = got.double().clone(), gref.clone()
    if truth:
        g[..., 4][band] = 0.0
        w[..., 4][band] = 0.0
    scales = [float(w.abs().max()), float(w[..., 4].abs().max()), float(w[..., 5:].abs().max())]
    errs = [float((g - w).abs().max()), float((g[..., 4] - w[..., 4]).abs().max()), float((g[..., 5:] - w[..., 5:]).abs().max())]
    lp = l.double().numpy()
    print('%s: ignored %d, left out %d; dfm max err %.3e (scale %.3e), objectness %.3e (%.3e), class %.3e (%.3e); parts got %s want %s'
          % (what, n_ign, n_band if truth else 0, errs[0], scales[0], errs[1], scales[1], errs[2], scales[2], lp.tolist(), parts.tolist()))
    if truth:
        assert n_band <= F.MAX_BAND_SHARE * n_ign, '%s: %d of %d ignored negatives in the band' % (what, n_band, n_ign)
    else:
        assert n_band == 0, '%s: %d negatives within %g of 0.5 under the reference mask' % (what, n_band, F.BAND)
    for e, sc, which in zip(errs, scales, ('tensor', 'objectness channel', 'class channels')):
        assert e <= 1e-4 * sc, '%s: %s, max abs err %.3e > 1e-4 * %.3e' % (what, which, e, sc)
    top = float(np.abs(parts).max())
    for i, which in enumerate(('box', 'wh', 'objectness', 'class')):
        assert abs(lp[i] - parts[i]) <= 2e-5 * top, '%s: %s part %r vs %r (largest part %r)' % (what, which, lp[i], parts[i], top)
    for i, which in ((2, 'objectness'), (3, 'class')):
        assert abs(lp[i] - parts[i]) <= 2e-5 * abs(parts[i]), '%s: %s part %r vs %r' % (what, which, lp[i], parts[i])
    return n_band if truth else 0


# ---- 1. both terms neutral: the launch of y3_loss_fwd_bwd_ex / y3_loss_fwd_bwd_truth ------------------------------------------------
@pytest.mark.parametrize('kind', ['mse', 'ciou'])
@pytest.mark.parametrize('name', F.KERNEL_CASES)
def test_neutral_is_the_non_focal_entry(hip, name, kind):
    for si in range(3):
        s = _scale(name, si)
        for truth in (False, True):
            pl, pbuf, pign = _plain(name, si, kind, truth)
            l, buf, ign = s.launch_focal(kind, F.NEUTRAL, _lists(name) if truth else None)
            torch.cuda.synchronize()
            what = (name, kind, si, truth)
            assert _same_bits(l.cpu(), pl), (what, l.tolist(), pl.tolist())
            assert _same_bits(buf.cpu(), pbuf), what                       # every float of the buffer: the pitch padding too
            assert bool((s.padding(buf) == SENTINEL).all()), what
            if truth:
                assert _same_bits(ign.cpu(), pign), what
                # ignored == NULL is accepted, as by y3_loss_fwd_bwd_truth
                l2, buf2, none = s.launch_focal(kind, F.NEUTRAL, _lists(name), with_ignored=False)
                torch.cuda.synchronize()
                assert none is None and _same_bits(l2.cpu(), pl) and _same_bits(buf2.cpu(), pbuf), what
    if kind == 'mse':      # and the plain entry point itself
        l0, d0 = _scale(name, 0).launch(None)
        torch.cuda.synchronize()
        assert _same_bits(l0.cpu(), _plain(name, 0, 'mse', False)[0]) and _same_bits(d0.cpu(), _plain(name, 0, 'mse', False)[1])


# ---- 2. the combinations against fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('combo', F.COMBINATIONS, ids=lambda c: 'g%g-a%g-%s-e%g' % c)
def test_focal_matches_fp64(hip, combo):
    args = F.term_args(*combo)
    for name in F.KERNEL_CASES:
        for si in range(3):
            _check(name, si, 'mse', False, args)


# ---- 3. saturated logits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['mse', 'ciou'])
def test_saturated_logits_stay_finite(hip, kind):
    case = F.make_case('saturated')
    counts = F.saturated_counts(case)
    print(counts)
    assert all(counts[(v, side)] > 0 for v in F.SATURATED_LOGITS for side in ('pos', 'neg'))
    for combo in [c for c in F.COMBINATIONS if c[0] == 0.5] + [(2.0, 0.25, 'both', 0.1)]:
        assert combo[0] in (0.5, 2.0)
        for si in range(3):
            for truth in (False, True):
                _check('saturated', si, kind, truth, F.term_args(*combo))         # finite, and the fp64 closed form
                if kind == 'ciou':     # cells without an object: +0 in the box channels, whatever the logits
                    s = _scale('saturated', si)
                    buf = s.launch_focal(kind, F.term_args(*combo), _lists('saturated') if truth else None)[1]
                    torch.cuda.synchronize()
                    neg = case['gts'][si][..., 4] == 0
                    assert bool((_bits(s.cells(buf)[..., 0:4][neg]) == 0).all())


# ---- 4. empty labels, one class -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('combo', [(2.0, 0.25, 'both', 0.1), (0.5, 0.0, 'obj', 0.0), (1.5, 0.25, 'class', 0.1)], ids=lambda c: 'g%g-a%g-%s-e%g' % c)
def test_empty_labels_and_one_class(hip, combo):
    args = F.term_args(*combo)
    for name in ('sq416', 'rect96x160', 'k1'):
        for si in range(3):
            for truth in (False, True):
                _check(name, si, 'mse', truth, args, empty=True)
                s = _scale(name, si, True)
                l, buf, _ = s.launch_focal('ciou', args, _lists(name, True) if truth else None)
                torch.cuda.synchronize()
                got = s.cells(buf)
                # no object anywhere: exact zeros in the box and class channels and parts; every negative is valid
                assert bool((_bits(got[..., 0:4]) == 0).all()) and bool((got[..., 5:] == 0).all()) and l.cpu().tolist()[0:2] == [0.0, 0.0]
                assert float(l[3]) == 0.0 and float(l[2]) > 0.0
    assert F.make_case('k1')['K'] == 1
    for si in range(3):
        for truth in (False, True):
            _check('k1', si, 'mse', truth, args)
            _check('k1', si, 'ciou', truth, args)


# ---- 5. crossed with an IoU box loss and with the truth mask ----------------------------------------------------------------------
@pytest.mark.parametrize('kind,truth', [('ciou', False), ('mse', True), ('ciou', True)])
def test_crossed_with_box_loss_and_truth_mask(hip, kind, truth):
    args = F.term_args(2.0, 0.25, 'both', 0.1)
    ignored = 0
    for name in F.KERNEL_CASES:
        for si in range(3):
            if kind != 'mse':       # the kink rule of test_gpu_box_loss.py has nothing to leave out on these inputs (test_cpu_focal_loss.py)
                assert R.kink_share(_ref(name, si, kind, truth).info)[0] == 0
            _check(name, si, kind, truth, args)
            ignored += int(_ref(name, si, kind, truth).info['ignored'].sum())
            if truth:
                # the mask-only count, against the restatement as well
                ign = float(_scale(name, si).launch_focal(kind, args, _lists(name))[2])
                ref = _ref(name, si, kind, truth)
                assert abs(ign - int(ref.info['ignored'].sum())) <= int(ref.info['band'].sum()), (name, si, ign)
    assert ignored >= M.MIN_IGNORED


def test_rejected_call_leaves_the_outputs_alone(hip):
    s = _scale('rect96x160', 1)
    args = F.term_args(2.0, 0.25, 'both', 0.1)
    l, buf, _ = s.launch_focal('mse', args)
    torch.cuda.synchronize()
    keep = (l.clone(), buf.clone())
    ws, tf_, td = s._keep[0:3]
    H, W = s.case['hw']
    lib = hip.lib

    def call(a=args, box_loss=0):
        return lib.y3_loss_fwd_bwd_focal(tf_, s.gd.data_ptr(), s.anc, s.A, s.K, H, W, GBS, box_loss, 1.0, None, None, 1, THR, l.data_ptr(), None, td,
                                         ws.data_ptr(), *a, _stream())
    nan = float('nan')
    for a in ((-1.0, 0.0, 0.0, 0.0, 0.0), (nan, 0.0, 0.0, 0.0, 0.0), (2.0, 1.0, 0.0, 0.0, 0.0), (2.0, -0.5, 0.0, 0.0, 0.0), (0.0, 0.0, nan, 0.0, 0.0),
              (0.0, 0.0, 2.0, 1.5, 0.0), (0.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 0.0, -0.1), (0.0, 0.0, 0.0, 0.0, nan)):
        assert call(a) == -1 and lib.y3_last_error(), a
    assert call(box_loss=9) == -1
    torch.cuda.synchronize()
    assert _same_bits(l, keep[0]) and _same_bits(buf, keep[1])
    assert call() == 0
    torch.cuda.synchronize()
    assert not _same_bits(l, keep[0]) and _same_bits(buf, keep[1])          # accepted: loss4 accumulates, dfm is rewritten with the same bits


# ---- 6. model level ---------------------------------------------------------------------------------------------------------------
FOCAL_KW = dict(focal_gamma=2, focal_alpha=0.25, label_smoothing=0.1)


def test_model_step_matches_the_restatement():
    """A real train_step of YoloV3(focal_gamma=2, focal_alpha=0.25, label_smoothing=0.1) at MODEL_CASE: its own head feature maps go
    through the fp64 restatement."""
    import teacher_forced as tf
    from yolo3._hip import lib
    params, images, gts, anchors, K, img, n = _model_inputs()
    yolo = _model(params, anchors, K, img, n, **FOCAL_KW)
    assert (yolo.focal_gamma, yolo.focal_alpha, yolo.focal_terms, yolo.label_smoothing) == (2.0, 0.25, 'both', 0.1)
    cap = tf.capture_step(yolo, images, gts)
    plan = yolo._plan(n, True)
    assert [c[0] for c in plan.loss_calls] == [lib.y3_loss_fwd_bwd_focal] * 3
    args = F.term_args(2.0, 0.25, 'both', 0.1)
    assert all(tuple(c[1][-5:]) == args and c[1][10] is None and c[1][11] is None for c in plan.loss_calls)      # the reference mask
    want = np.zeros(4)
    for si, (fm, dfm, gt) in enumerate(zip(cap['fm'], cap['dfm'], cap['gts'])):
        ref = F.Scale(dict(hw=(img, img), anchors=anchors, K=K, fms=[fm.cpu()], gts=[gt]), 0, gbs=cap['gbs'])
        parts, gref = ref.reference(args)
        want += parts
        got = ref.cells(dfm.cpu()).double()
        n_band = int(ref.info['band'].sum())
        scales = [float(gref.abs().max()), float(gref[..., 4].abs().max()), float(gref[..., 5:].abs().max())]
        errs = [float((got - gref).abs().max()), float((got[..., 4] - gref[..., 4]).abs().max()), float((got[..., 5:] - gref[..., 5:]).abs().max())]
        print('model step scale %d: band %d; dfm max err %.3e (scale %.3e), objectness %.3e (%.3e), class %.3e (%.3e)'
              % (si, n_band, errs[0], scales[0], errs[1], scales[1], errs[2], scales[2]))
        assert n_band == 0, 'scale %d: %d negatives within %g of 0.5' % (si, n_band, F.BAND)
        for e, sc in zip(errs, scales):
            assert e <= 1e-4 * sc, (si, e, sc)
    got4 = cap['loss4'].cpu().double().numpy()
    print('model step loss4 got %s want %s' % (got4.tolist(), want.tolist()))
    for i in range(4):
        assert abs(got4[i] - want[i]) <= 2e-5 * float(np.abs(want).max())
    for i in (2, 3):
        assert abs(got4[i] - want[i]) <= 2e-5 * abs(want[i])
    # the focal terms took part: the plain model's step on the same inputs has the same box parts and other objectness / class parts
    plain = _model(params, anchors, K, img, n)
    cap0 = tf.capture_step(plain, images, gts)
    p4 = cap0['loss4'].cpu()
    assert _same_bits(p4[0:2], cap['loss4'].cpu()[0:2]) and float(p4[2]) > got4[2] and float(p4[3]) != got4[3]
    # test_step uses the same terms
    lt = float(yolo.test_step((images.cuda(), [torch.from_numpy(v).cuda() for v in gts])))
    assert np.isfinite(lt) and [c[0] for c in yolo._plan(n, False).loss_calls] == [lib.y3_loss_fwd_bwd_focal] * 3


def test_model_graph_replay_save_load_and_default(tmp_path):
    from yolo3._hip import lib
    from yolo3.model import YoloV3
    params, images, gts, anchors, K, img, n = _model_inputs()
    x, g = images.cuda(), [torch.from_numpy(v).cuda() for v in gts]
    eager = _model(params, anchors, K, img, n, **FOCAL_KW)
    graph = _model(params, anchors, K, img, n, use_graph=True, **FOCAL_KW)
    for step in range(3):                     # the graph model captures in its first step and replays in every step
        le, lg = eager.train_step((x, g)), graph.train_step((x, g))
        torch.cuda.synchronize()
        assert _same_bits(le.reshape(1), lg.reshape(1)), (step, float(le), float(lg))
        for name in ('grads', 'params', 'moving', 'adam_m', 'adam_v'):
            assert torch.equal(getattr(eager, name), getattr(graph, name)), (step, name)
    assert graph._plan(n, True).graph is not None
    # save / load: the file carries the settings, and the loaded model takes the next step with the same bits
    path = str(tmp_path / 'focal.npz')
    eager.save_weights(path)
    z = np.load(path)
    assert z['meta_focal'].tolist() == [2.0, 0.25, 0.1] and str(z['meta_focal_terms']) == 'both'
    back = YoloV3.from_file(path)
    assert (back.focal_gamma, back.focal_alpha, back.focal_terms, back.label_smoothing) == (2.0, 0.25, 'both', 0.1)
    assert [c[0] for c in back._plan(n, True).loss_calls] == [lib.y3_loss_fwd_bwd_focal] * 3
    back.load_weights(path, load_optimizer=True)
    le, lb = eager.train_step((x, g)), back.train_step((x, g))
    torch.cuda.synchronize()
    assert _same_bits(le.reshape(1), lb.reshape(1)), (float(le), float(lb))
    for name in ('grads', 'params', 'moving', 'adam_m', 'adam_v'):
        assert torch.equal(getattr(eager, name), getattr(back, name)), name
    # a model built without the arguments: the parent's kernel list and arguments, and a weight file without the entries
    plain = _model(params, anchors, K, img, n)
    zeros = _model(params, anchors, K, img, n, focal_gamma=0.0, focal_alpha=0.0, focal_terms='obj', label_smoothing=0.0)
    for m in (plain, zeros):
        calls = m._plan(n, True).loss_calls
        assert [c[0] for c in calls] == [lib.y3_loss_fwd_bwd] * 3 and all(len(c[1]) == 11 for c in calls)
    lp, lz = plain.train_step((x, g)), zeros.train_step((x, g))
    torch.cuda.synchronize()
    assert _same_bits(lp.reshape(1), lz.reshape(1)) and torch.equal(plain.params, zeros.params)
    p2 = str(tmp_path / 'plain.npz')
    plain.save_weights(p2)
    assert not [k for k in np.load(p2).files if 'focal' in k]
    assert YoloV3.from_file(p2).focal_args() is None
    # loading across settings takes the weights and says so
    with pytest.warns(UserWarning, match='focal setting'):
        plain.load_weights(path)
    with pytest.warns(UserWarning, match='focal setting'):
        eager.load_weights(p2)


def test_model_with_truth_mask_box_loss_accumulation_and_sizes():
    """The focal terms over ignore_mask='truth', box_loss='ciou', accumulate_steps=2 and train_sizes: the truth lists reach the focal
    entry, the mask-only count is the non-focal truth model's, and each size has its own plan."""
    from yolo3._hip import lib
    params, images, gts, anchors, K, img, n = _model_inputs()
    x, g = images.cuda(), [torch.from_numpy(v).cuda() for v in gts]
    kw = dict(ignore_mask='truth', box_loss='ciou', accumulate_steps=2, train_sizes=[(64, 64), (96, 96)])
    focal = _model(params, anchors, K, img, n, **kw, **FOCAL_KW)
    base = _model(params, anchors, K, img, n, **kw)
    calls = focal._plan(n, True).loss_calls
    assert [c[0] for c in calls] == [lib.y3_loss_fwd_bwd_focal] * 3 and all(c[1][10] is not None and c[1][11] is not None for c in calls)
    assert [c[0] for c in base._plan(n, True).loss_calls] == [lib.y3_loss_fwd_bwd_truth] * 3
    for step in range(2):
        lf, lb = float(focal.train_step((x, g))), float(base.train_step((x, g)))
        torch.cuda.synchronize()
        assert np.isfinite(lf) and np.isfinite(lb) and lf != lb, (step, lf, lb)
        assert float(focal.last_ignored) == float(base.last_ignored) and int(focal.last_truth_max) == int(base.last_truth_max)
    assert focal.iterations == base.iterations and bool(torch.isfinite(focal.params).all()) and not torch.equal(focal.params, base.params)
    p64 = focal._plan(n, True, size=(64, 64))
    assert [c[0] for c in p64.loss_calls] == [lib.y3_loss_fwd_bwd_focal] * 3 and p64 is not focal._plan(n, True)


# ---- 7. train.py ------------------------------------------------------------------------------------------------------------------
def test_cli_train_with_focal_loss(tmp_path):
    tmp = str(tmp_path)
    _write_dataset(tmp, 8, (256, 256, 3))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = os.path.join(tmp, 'out')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--batch_size', '2', '--test_every_n_steps', '3', '--train_database',
                        os.path.join(tmp, 'train-syn.lmdb'), '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out,
                        '--early_stopping', '1', '--use_augmentation', '1', '--max_epochs', '1', '--learning_rate', '1e-4',
                        '--focal_gamma', '2', '--focal_alpha', '0.25', '--focal_terms', 'both', '--label_smoothing', '0.1'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'focal_gamma = 2.0' in r.stdout and 'label_smoothing = 0.1' in r.stdout and 'Focal loss: gamma 2, alpha 0.25' in r.stdout
    saved = os.path.join(out, 'saved_model', 'yolov3.npz')
    assert os.path.exists(saved) and os.path.exists(os.path.join(out, 'checkpoint', 'ckpt.npz'))
    assert np.load(saved)['meta_focal'].tolist() == [2.0, 0.25, 0.1]
    dirs = glob.glob(os.path.join(out, 'scalars-*'))
    assert len(dirs) == 1
    for split in ('train', 'test'):
        lines = open(os.path.join(dirs[0], split + '.csv')).read().splitlines()
        assert lines[0] == 'step,loss,loss_xy,loss_wh,loss_obj,loss_class' and len(lines) >= 2, (split, lines)
        for ln in lines[1:]:
            vals = [float(v) for v in ln.split(',')]
            print(split, ln)
            assert all(np.isfinite(v) for v in vals) and vals[1] > 0 and vals[4] > 0 and vals[5] > 0, (split, ln)
