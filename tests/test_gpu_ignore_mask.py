"""y3_truth_boxes and y3_loss_fwd_bwd_truth (opt-in ignore mask against each image's ground-truth boxes) on the GPU:
the gather bit for bit against NumPy, the loss against tests/ignore_mask_reference.py in fp64 with autograd at the tolerances of
test_gpu_box_loss.py (gradients 1e-4 of the tensor's largest reference magnitude, loss parts 2e-5), bit for bit against
y3_loss_fwd_bwd_ex wherever the two must agree, the edges of the list, and through YoloV3 and train.py.

Band rule (ignore_mask_reference): comparisons of dfm[..., 4] leave out the negatives whose fp64 best IoU lies within 1e-4 of the
threshold -- float32 and float64 may decide differently there -- and nothing else; the two fixed cases assert that those are at
most 1 % of at least 20 ignored negatives (tests/test_cpu_ignore_mask.py asserts the same without a GPU).  Loss sums and the
ignored count are compared on all cells, the count to within the number of band members.  Every comparison prints its figures
before it asserts."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ignore_mask_reference as M
from test_gpu_box_loss import GBS, SENTINEL, _Scale, _write_dataset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
R = M.R


@pytest.fixture(scope='module')
def hip():
    from yolo3 import _hip
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return _hip


def _chunk():
    import re
    text = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    return int(re.search(r'#define\s+Y3_TRUTH_CHUNK\s+(\d+)\b', text).group(1))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. y3_truth_boxes ----------------------------------------------------------------------------------------------------------
def _gather(hip, gt, cap):
    """gt: host float32 [n, ca, d] -> (boxes [n, cap, 4] with NaN canaries where nothing was written, counts [n]) on the host"""
    n, ca, d = gt.shape
    boxes = torch.full((n, cap, 4), float('nan'), device='cuda')
    counts = torch.full((n,), -77, dtype=torch.int32, device='cuda')
    g = torch.from_numpy(gt).cuda()
    hip.check(hip.lib.y3_truth_boxes(g.data_ptr(), n, ca, d, boxes.data_ptr(), counts.data_ptr(), cap, _stream()), 'y3_truth_boxes')
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), counts.cpu().numpy()


def _gather_numpy(gt, cap):
    n = gt.shape[0]
    boxes = np.full((n, cap, 4), np.nan, np.float32)
    counts = np.zeros(n, np.int32)
    for i in range(n):
        rows = gt[i][gt[i][:, 4] != 0][:, 0:4]
        counts[i] = len(rows)
        m = min(len(rows), cap)
        boxes[i, :m] = rows[:m]
    return boxes, counts


@pytest.mark.parametrize('d', [6, 8])
@pytest.mark.parametrize('ca', [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_truth_boxes_bit_for_bit(hip, ca, d):
    n = 3
    rng = np.random.default_rng(1000 * d + ca)
    base = rng.standard_normal((n, ca, d)).astype(np.float32) * 100.0
    patterns = {
        'none': np.zeros((n, ca), bool),
        'all': np.ones((n, ca), bool),
        'every other': np.broadcast_to(np.arange(ca) % 2 == 0, (n, ca)).copy(),
        'last row': np.broadcast_to(np.arange(ca) == ca - 1, (n, ca)).copy(),
        'per image': np.stack([np.zeros(ca, bool), np.ones(ca, bool), rng.random(ca) < 0.3]),
    }
    for what, pos in patterns.items():
        gt = base.copy()
        # objectness labels: 1, another non-zero value now and then (any value != 0 counts), -0.0 and +0 where there is no object
        gt[..., 4] = np.where(pos, np.where(rng.random((n, ca)) < 0.1, np.float32(-0.25), np.float32(1.0)),
                              np.where(rng.random((n, ca)) < 0.5, np.float32(-0.0), np.float32(0.0)))
        top = int(pos.sum(1).max())
        for cap in sorted({max(1, top - 1), max(1, top), top + 3, max(1, top // 2)}):
            got_b, got_c = _gather(hip, gt, cap)
            want_b, want_c = _gather_numpy(gt, cap)
            assert np.array_equal(got_c, want_c) and np.array_equal(got_c, pos.sum(1)), (what, cap, got_c, want_c)
            assert np.array_equal(got_b.view(np.uint32), want_b.view(np.uint32)), (what, cap)       # canaries past min(count, cap) included
    # the same bits on every run
    gt = base.copy()
    gt[..., 4] = patterns['per image']
    first = _gather(hip, gt, 37)
    for _ in range(5):
        again = _gather(hip, gt, 37)
        assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32)) and np.array_equal(first[1], again[1])


# ---- 2. y3_loss_fwd_bwd_truth ---------------------------------------------------------------------------------------------------
class _TruthScale(_Scale):
    """test_gpu_box_loss._Scale plus the truth-mask launch."""

    def launch_truth(self, kind, boxes, counts, cap, thr, with_ignored=True, loss4=None, ignored=None):
        """boxes [n, cap, 4] / counts [n] int32 on the device -> (loss4 [4], dfm buffer with its padding, ignored [1] or None)"""
        hip = self.hip
        buf, dv = self.nhwc_buf(self.n, self.Gh, self.Gw, self.D, ld=self.ld, fill=SENTINEL)
        loss4 = torch.zeros(4, device='cuda') if loss4 is None else loss4
        if with_ignored and ignored is None:
            ignored = torch.zeros(1, device='cuda')
        ws = torch.full((int(hip.lib.y3_loss_truth_workspace_bytes(self.n)) // 4 + 4,), float('nan'), device='cuda')     # nothing needs zeroing
        H, W = self.case['hw']
        tf_ = hip.Tensor(self.fv.data_ptr(), self.n, self.Gh, self.Gw, self.D, self.ld)
        td = hip.Tensor(dv.data_ptr(), self.n, self.Gh, self.Gw, self.D, self.ld)
        rc = hip.lib.y3_loss_fwd_bwd_truth(tf_, self.gd.data_ptr(), self.anc, self.A, self.K, H, W, GBS, R.BOX_LOSSES.index(kind), 1.0,
                                           boxes.data_ptr(), counts.data_ptr(), cap, float(thr), loss4.data_ptr(),
                                           ignored.data_ptr() if with_ignored else None, td, ws.data_ptr(), _stream())
        hip.check(rc, 'y3_loss_fwd_bwd_truth')
        self._keep = (ws, tf_, td, boxes, counts)
        return loss4, buf, ignored

    def reference_truth(self, kind, truth, thr):
        """fp64 autograd -> (parts [4], dfm [n, Gh, Gw, A, 5+K], info)"""
        H, W = self.case['hw']
        x = self.fm.double().requires_grad_(True)
        info = {}
        parts = M.loss_layer_truth(x, self.gt.double(), (H, W, 3), self.case['anchors'], self.K, kind, 1.0, [t.double() for t in truth], thr, info)
        (sum(parts) / GBS).backward()
        g = x.grad.permute(0, 2, 3, 1).reshape(self.n, self.Gh, self.Gw, self.A, 5 + self.K)
        return np.array([float(p.detach()) for p in parts]), g, info


def _device_lists(hip, gt_fine, cap):
    """The lists of the finest label tensor [n, Gh, Gw, A, D] (host) gathered on the device -> (boxes, counts) device tensors"""
    n, D = gt_fine.shape[0], gt_fine.shape[-1]
    g = gt_fine.float().cuda().contiguous()
    boxes = torch.full((n, cap, 4), float('nan'), device='cuda')
    counts = torch.zeros(n, dtype=torch.int32, device='cuda')
    hip.check(hip.lib.y3_truth_boxes(g.data_ptr(), n, g.numel() // (n * D), D, boxes.data_ptr(), counts.data_ptr(), cap, _stream()), 'y3_truth_boxes')
    return boxes, counts


def _compare_gradient(got, want, info, thr, what):
    """got / want [n, Gh, Gw, A, 5+K]: band rule on the objectness channel, kink rule of test_gpu_box_loss on the box channels of
    the IoU losses, then 1e-4 of the largest reference magnitude of the whole tensor and, stricter, of the objectness channel.
    -> number of band members"""
    band = M.band(info, thr)
    kink = info['positive'] & (info['kink_margin'] < R.KINK_PX)
    got, want = got.double().clone(), want.clone()
    assert bool(torch.isfinite(got).all()), '%s: non-finite gradient' % what
    got[..., 4][band] = 0.0
    want[..., 4][band] = 0.0
    got[..., 0:4][kink] = 0.0
    want[..., 0:4][kink] = 0.0
    scale, obj_scale = float(want.abs().max()), float(want[..., 4].abs().max())
    err, obj_err = float((got - want).abs().max()), float((got[..., 4] - want[..., 4]).abs().max())
    print('%s: negatives %d, ignored %d, left out (best within %g of %g) %d; max err %.3e = %.2e of the tensor scale %.3e; objectness %.3e '
          '= %.2e of its scale %.3e' % (what, int(info['negative'].sum()), int(info['ignored'].sum()), M.BAND, thr, int(band.sum()), err,
                                        err / max(scale, 1e-30), scale, obj_err, obj_err / max(obj_scale, 1e-30), obj_scale))
    assert err <= 1e-4 * scale, '%s: max abs err %.3e > 1e-4 * %.3e' % (what, err, scale)
    assert obj_err <= 1e-4 * obj_scale, '%s: objectness, max abs err %.3e > 1e-4 * %.3e' % (what, obj_err, obj_scale)
    return int(band.sum())


def _compare_parts(got, want, what, obj=2):
    """Loss parts on all cells, 2e-5 of the largest part (the project's tolerance); obj: index of the objectness part, if it is there."""
    from util import assert_close
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print('%s: loss parts got %s want %s%s' % (what, got.tolist(), want.tolist(),
                                             '' if obj is None else '; objectness rel err %.2e' % (abs(got[obj] - want[obj]) / max(abs(want[obj]), 1e-30))))
    assert_close(got, want, rtol=2e-5, what=what)


@pytest.mark.parametrize('kind', ['mse', 'ciou'])
@pytest.mark.parametrize('name', sorted(M.CASES))
def test_truth_loss_matches_fp64_autograd(hip, name, kind):
    thr, cap = 0.5, 1024
    case = M.make_case(name)
    boxes, counts = _device_lists(hip, case['gts'][2], cap)
    torch.cuda.synchronize()
    for i, t in enumerate(case['truth']):           # the device lists are the restatement's
        assert int(counts[i]) == t.shape[0] and torch.equal(boxes[i, :t.shape[0]].cpu(), t.float())
    loss4, ignored = torch.zeros(4, device='cuda'), torch.zeros(1, device='cuda')
    want_parts, want_ignored, n_band = np.zeros(4), 0, 0
    for si in range(3):
        s = _TruthScale(hip, case, si)
        parts, gref, info = s.reference_truth(kind, case['truth'], thr)
        want_parts += parts
        want_ignored += int(info['ignored'].sum())
        _, buf, _ = s.launch_truth(kind, boxes, counts, cap, thr, loss4=loss4, ignored=ignored)
        le, de = s.launch(kind)                    # y3_loss_fwd_bwd_ex on the same inputs
        torch.cuda.synchronize()
        got, ex = s.cells(buf), s.cells(de)
        n_band += _compare_gradient(got, gref, info, thr, '%s %s scale %d dfm' % (name, kind, si))
        # the mask touches objectness only
        assert torch.equal(got[..., 0:4], ex[..., 0:4]) and torch.equal(got[..., 5:], ex[..., 5:])
        assert bool((s.padding(buf) == SENTINEL).all())
        lt = s.launch_truth(kind, boxes, counts, cap, thr)[0].cpu()       # this scale alone, from a zeroed loss4
        # box, wh and class sums: the same terms as the unmasked launch, added up over another block partition
        _compare_parts(lt.numpy()[[0, 1, 3]], le.cpu().numpy()[[0, 1, 3]], '%s %s scale %d box / wh / class against the unmasked launch' % (name, kind, si), obj=None)
        # a positive cell is never masked: its objectness gradient is the unmasked launch's
        pos = info['positive']
        assert torch.equal(got[..., 4][pos], ex[..., 4][pos])
    _compare_parts(loss4.cpu().numpy(), want_parts, '%s %s' % (name, kind))
    got_ignored = float(ignored)
    print('%s %s: ignored %r, restatement %d, band members %d' % (name, kind, got_ignored, want_ignored, n_band))
    assert want_ignored >= M.MIN_IGNORED and n_band <= M.MAX_BAND_SHARE * want_ignored, (want_ignored, n_band)
    assert got_ignored == int(got_ignored) and abs(got_ignored - want_ignored) <= n_band


@pytest.mark.parametrize('grid', [(1, 1), (2, 3), (13, 13)])
@pytest.mark.parametrize('n', [1, 3])
def test_edges_of_the_list(hip, n, grid):
    """Synthetic lists fed directly: counts of 0, 1, Y3_TRUTH_CHUNK, Y3_TRUTH_CHUNK + 1 and a count above truth_cap (only the first
    cap boxes act).  The one box that decides each image's planted prediction is the last of the list, so a dropped tail chunk
    shows; with the deciding box at or past the capacity the planted prediction stays valid.  (The grids hold 2 to 338 predictions
    per image: the band rule applies, its 20-ignored condition is for the fixed cases.)"""
    chunk, thr = _chunk(), 0.5
    #        count      deciding index  capacity
    rows = [(0, None, 4), (1, 0, 4), (chunk, chunk - 1, chunk), (chunk + 1, chunk, chunk + 8), (2 * chunk + 3, 2 * chunk + 2, 3 * chunk),
            (chunk + 1, chunk, chunk), (chunk + 40, chunk + 39, chunk + 39), (5, 4, 1)]
    for count, decide_at, cap in rows:
        c = M.make_edge_case(n, grid, count, decide_at, seed=100 * grid[0] + n)
        case = dict(n=n, hw=c['hw'], anchors=c['anchors'], K=c['K'], fms=[c['fm']], gts=[c['gt']])
        s = _TruthScale(hip, case, 0)
        # the buffer holds `cap` slots per image; what lies past min(count, cap) is NaN and must not be read into the mask
        boxes = torch.full((n, cap, 4), float('nan'))
        m = min(count, cap)
        boxes[:, :m] = c['lists'][:, :m]
        counts = torch.full((n,), count, dtype=torch.int32)
        acting = [c['lists'][i, :m] for i in range(n)]
        parts, gref, info = s.reference_truth('mse', acting, thr)
        l, buf, ign = s.launch_truth('mse', boxes.cuda(), counts.cuda(), cap, thr)
        torch.cuda.synchronize()
        got = s.cells(buf)
        what = 'n %d grid %s count %d cap %d' % (n, grid, count, cap)
        n_band = _compare_gradient(got, gref, info, thr, what)
        _compare_parts(l.cpu().numpy(), parts, what)
        assert abs(float(ign) - int(info['ignored'].sum())) <= n_band, (what, float(ign), int(info['ignored'].sum()))
        acts = decide_at is not None and decide_at < cap
        for p in c['planted']:
            assert bool(info['ignored'][p]) == acts, (what, p)
            assert (float(got[p][4]) == 0.0) == acts, (what, p, float(got[p][4]))       # sigmoid(t) / (n gbs) is never 0 when valid
        if count == 0:
            assert float(ign) == 0.0


def _two_image_case():
    """Two images with identical logits; objects (and hence truth) in image 1 only."""
    case = M.make_case('rect96x160')
    for fm in case['fms']:
        fm[0] = fm[1]
    for gt in case['gts']:
        gt[0] = 0.0
    keep = lambda t: t[:2].clone()
    return dict(n=2, hw=case['hw'], anchors=case['anchors'], K=case['K'], fms=[keep(f) for f in case['fms']], gts=[keep(g) for g in case['gts']])


def test_mask_is_per_image_and_empty_lists_mask_nothing(hip):
    thr, cap = 0.5, 64
    case = _two_image_case()
    boxes, counts = _device_lists(hip, case['gts'][2], cap)
    torch.cuda.synchronize()
    assert int(counts[0]) == 0 and int(counts[1]) > 0
    none = torch.zeros(2, dtype=torch.int32, device='cuda')
    total = 0.0
    for si in range(3):
        s = _TruthScale(hip, case, si)
        l, buf, ign = s.launch_truth('mse', boxes, counts, cap, thr)
        l0, buf0, ign0 = s.launch_truth('mse', boxes, none, cap, thr)         # empty lists: nothing is ignored
        lnull, bufnull, nothing = s.launch_truth('mse', boxes, counts, cap, thr, with_ignored=False)      # ignored == NULL is accepted
        torch.cuda.synchronize()
        got, got0 = s.cells(buf), s.cells(buf0)
        assert nothing is None and torch.equal(l, lnull) and torch.equal(buf, bufnull)
        assert float(ign0) == 0.0
        # image 0 has no truth of its own: all-valid, whatever image 1's boxes are (a batch-wide gather, as in Q7, would mask it like
        # image 1, whose logits it shares)
        f = s.fm.permute(0, 2, 3, 1).reshape(2, s.Gh, s.Gw, s.A, 5 + s.K)
        want0 = torch.sigmoid(f[0, ..., 4].double()) / (2 * GBS)
        assert torch.equal(got[0, ..., 4], got0[0, ..., 4])
        assert float((got[0, ..., 4].double() - want0).abs().max()) <= 1e-6 * float(want0.max())
        masked = (got[1, ..., 4] == 0) & (s.gt[1, ..., 4] == 0)
        assert float(ign) == float(masked.sum()), (si, float(ign), int(masked.sum()))
        total += float(ign)
        assert torch.equal(got[1, ..., 4][~masked], got0[1, ..., 4][~masked])
    assert total > 0        # image 1 did mask something, so image 0 had something to differ by


def test_overflowing_size_logits_stay_finite(hip):
    """Size logits of 100 in cells without an object: expf overflows, the IoU with every truth box is 0 or NaN, dfm[..., 4] is finite."""
    case, masks = R.make_extreme_case()
    lists = M.truth_boxes(case['gts'][2])
    cap = 1024
    boxes, counts = _device_lists(hip, case['gts'][2], cap)
    for si in range(3):
        s = _TruthScale(hip, case, si)
        assert float(torch.exp(s.fv[..., 2]).max()) == float('inf')
        for kind in ('mse', 'ciou'):
            l, buf, ign = s.launch_truth(kind, boxes, counts, cap, 0.5)
            torch.cuda.synchronize()
            got = s.cells(buf)
            assert bool(torch.isfinite(got[..., 4]).all()) and bool(torch.isfinite(ign).all()) and np.isfinite(float(l[2]))
            # an overflowed negative is never ignored: it keeps the unmasked objectness gradient
            ex = s.cells(s.launch(kind)[1])
            torch.cuda.synchronize()
            assert torch.equal(got[..., 4][masks[si]], ex[..., 4][masks[si]])
            if kind == 'ciou':
                assert bool(torch.isfinite(got).all())
    assert sum(int(t.shape[0]) for t in lists) > 0


def test_rejected_call_leaves_the_outputs_alone(hip):
    case = M.make_case('rect96x160')
    boxes, counts = _device_lists(hip, case['gts'][2], 64)
    s = _TruthScale(hip, case, 1)
    l, buf, ign = s.launch_truth('mse', boxes, counts, 64, 0.5)
    torch.cuda.synchronize()
    keep = (l.clone(), buf.clone(), ign.clone())
    ws, tf_, td = s._keep[0:3]
    H, W = case['hw']
    lib = hip.lib

    def call(box_loss=0, weight=1.0, b=boxes.data_ptr(), c=counts.data_ptr(), cap=64, thr=0.5):
        return lib.y3_loss_fwd_bwd_truth(tf_, s.gd.data_ptr(), s.anc, s.A, s.K, H, W, GBS, box_loss, weight, b, c, cap, thr, l.data_ptr(),
                                         ign.data_ptr(), td, ws.data_ptr(), _stream())
    for kw in (dict(thr=0.0), dict(thr=1.5), dict(thr=float('nan')), dict(cap=0), dict(b=None), dict(c=None), dict(box_loss=7),
               dict(box_loss=0, weight=2.0), dict(box_loss=3, weight=0.0)):
        assert call(**kw) == -1 and lib.y3_last_error(), kw
    torch.cuda.synchronize()
    # td views a fresh buffer of the last launch_truth: the rejected calls wrote neither it nor loss4 / ignored
    assert torch.equal(l, keep[0]) and torch.equal(buf, keep[1]) and torch.equal(ign, keep[2])
    assert call() == 0
    torch.cuda.synchronize()
    assert float(ign) == 2 * float(keep[2]) and not torch.equal(l, keep[0])        # accepted: both accumulate


# ---- 3. model level ---------------------------------------------------------------------------------------------------------------
def _model_inputs():
    from oracle import model as om
    from test_gpu_kernels import _labels
    from test_gpu_model import ANCHORS, K
    img, n, seed = M.MODEL_CASE['img'], M.MODEL_CASE['n'], M.MODEL_CASE['seed']
    params = om.init_params(3, len(ANCHORS), K, seed=seed)
    images = torch.randn(n, 3, img, img, generator=torch.Generator().manual_seed(seed))
    gts = _labels(np.random.default_rng(seed), n, img, ANCHORS, K, per_image=3)
    return params, images, gts, ANCHORS, K, img, n


def _model(params, anchors, K, img, n, **kw):
    from yolo3.model import YoloV3
    yolo = YoloV3(n, [img, img, 3], K, anchors, learning_rate=1e-3, **kw)
    yolo.set_weights(params)
    return yolo


def test_default_model_is_the_reference_mask():
    from yolo3._hip import lib
    params, images, gts, anchors, K, img, n = _model_inputs()
    x, g = images.cuda(), [torch.from_numpy(v).cuda() for v in gts]
    plain = _model(params, anchors, K, img, n)
    named = _model(params, anchors, K, img, n, ignore_mask='reference')
    plan = plain._plan(n, True)
    assert plain.ignore_mask == 'reference' and [c[0] for c in plan.loss_calls] == [lib.y3_loss_fwd_bwd] * 3
    assert plan.truth_call is None and plan.truth_boxes is None and plan.ignored is None
    assert [c[0] for c in named._plan(n, True).loss_calls] == [lib.y3_loss_fwd_bwd] * 3
    for step in range(3):
        lp, ln = plain.train_step((x, g)), named.train_step((x, g))
        torch.cuda.synchronize()
        assert torch.equal(lp, ln), step
    assert torch.equal(plain.params, named.params) and torch.equal(plain.grads, named.grads) and torch.equal(plain.moving, named.moving)
    assert plain.last_ignored is None and plain.last_truth_max is None


def test_model_step_matches_the_restatement():
    """A real train_step of YoloV3(ignore_mask='truth') at MODEL_CASE: its own head feature maps go through the fp64 restatement."""
    import teacher_forced as tf
    from yolo3._hip import lib
    params, images, gts, anchors, K, img, n = _model_inputs()
    thr = 0.5
    yolo = _model(params, anchors, K, img, n, ignore_mask='truth')
    assert yolo.ignore_mask == 'truth' and yolo.ignore_thresh == 0.5 and yolo.max_truth_boxes == 1024
    assert yolo.last_ignored is None and yolo.last_truth_max is None
    cap = tf.capture_step(yolo, images, gts)
    plan = yolo._plan(n, True)
    assert [c[0] for c in plan.loss_calls] == [lib.y3_loss_fwd_bwd_truth] * 3 and plan.truth_call[0] == lib.y3_truth_boxes
    assert tuple(plan.truth_boxes.shape) == (n, 1024, 4) and tuple(plan.truth_counts.shape) == (n,) and plan.ignored.numel() == 1
    truth = M.truth_boxes(cap['gts'][2])
    assert plan.truth_counts.cpu().tolist() == [t.shape[0] for t in truth]
    assert int(yolo.last_truth_max) == max(t.shape[0] for t in truth)
    want, want_ignored, n_band = np.zeros(4), 0, 0
    for si, (fm, dfm, gt) in enumerate(zip(cap['fm'], cap['dfm'], cap['gts'])):
        x = fm.cpu().double().requires_grad_(True)
        info = {}
        parts = M.loss_layer_truth(x, gt.double(), (img, img, 3), anchors, K, 'mse', 1.0, [t.double() for t in truth], thr, info)
        (sum(parts) / cap['gbs']).backward()
        want += np.array([float(p.detach()) for p in parts])
        want_ignored += int(info['ignored'].sum())
        shape = (n, fm.shape[2], fm.shape[3], len(anchors), 5 + K)
        n_band += _compare_gradient(dfm.cpu().permute(0, 2, 3, 1).reshape(shape), x.grad.permute(0, 2, 3, 1).reshape(shape), info, thr,
                                    'model step scale %d dfm' % si)
    _compare_parts(cap['loss4'].cpu().numpy(), want, 'model step loss4')
    got_ignored = float(yolo.last_ignored)
    print('model step: ignored %r, restatement %d, band members %d' % (got_ignored, want_ignored, n_band))
    assert abs(got_ignored - want_ignored) <= n_band
    # test_step uses the same mask
    lt = float(yolo.test_step((images.cuda(), [torch.from_numpy(v).cuda() for v in gts])))
    assert np.isfinite(lt) and [c[0] for c in yolo._plan(n, False).loss_calls] == [lib.y3_loss_fwd_bwd_truth] * 3
    assert int(yolo.last_truth_max) == max(t.shape[0] for t in truth)


SMALL_ANCHORS = [(24, 24), (40, 40)]      # close to the 20-48 px boxes of the labels below: the mask has something to ignore
LOW_THR = 0.3


def test_graph_replay_equals_eager_with_changing_labels():
    from oracle import model as om
    K, img, n = 2, 96, 4
    params = om.init_params(3, len(SMALL_ANCHORS), K, seed=23)
    images = torch.randn(n, 3, img, img, generator=torch.Generator().manual_seed(23)).cuda()
    per_step = [[3, 2, 4, 1], [2, 0, 3, 3], [1, 4, 2, 2]]          # step 1 has an image without boxes
    kw = dict(ignore_mask='truth', ignore_thresh=LOW_THR, max_truth_boxes=8)
    eager = _model(params, SMALL_ANCHORS, K, img, n, **kw)
    graph = _model(params, SMALL_ANCHORS, K, img, n, use_graph=True, **kw)
    seen = []
    for step, per_image in enumerate(per_step):
        gts = M.make_step_labels(50 + step, n, (img, img), SMALL_ANCHORS, K, per_image)
        g = [torch.from_numpy(v).cuda() for v in gts]
        le, lg = eager.train_step((images, g)), graph.train_step((images, g))
        torch.cuda.synchronize()
        assert torch.equal(le, lg), (step, float(le), float(lg))
        for name in ('grads', 'params', 'moving', 'adam_m', 'adam_v'):
            assert torch.equal(getattr(eager, name), getattr(graph, name)), (step, name)
        pe, pg = eager._plan(n, True), graph._plan(n, True)
        want_counts = [t.shape[0] for t in M.truth_boxes(torch.from_numpy(gts[2]))]
        assert pe.truth_counts.cpu().tolist() == want_counts == pg.truth_counts.cpu().tolist(), (step, want_counts)      # replayed with this step's labels
        assert float(eager.last_ignored) == float(graph.last_ignored) and int(eager.last_truth_max) == int(graph.last_truth_max) == max(want_counts)
        seen.append(float(eager.last_ignored))
    print('ignored per step', seen)
    assert per_step[1][1] == 0 and max(seen) > 0        # the mask acted
    assert graph._plan(n, True).graph is not None


def test_multiscale_chain():
    """One model with train_sizes stepping at 96, 64, 96 equals the chain of fixed-size models (tests/test_gpu_multiscale.py): the
    per-plan truth buffers keep the sizes apart."""
    import tempfile
    from oracle import model as om
    from yolo3.model import YoloV3
    K, n = 2, 2
    params = om.init_params(3, len(SMALL_ANCHORS), K, seed=11)
    kw = dict(learning_rate=1e-3, ignore_mask='truth', ignore_thresh=LOW_THR, max_truth_boxes=8)
    batches = {}
    for s in (96, 64):
        images = torch.randn(n, 3, s, s, generator=torch.Generator().manual_seed(100 + s)).cuda()
        gts = M.make_step_labels(100 + s, n, (s, s), SMALL_ANCHORS, K, [3, 2])
        batches[s] = (images, [torch.from_numpy(v).cuda() for v in gts])
    a = YoloV3(n, [96, 96, 3], K, SMALL_ANCHORS, train_sizes=[(64, 64), (96, 96)], **kw)
    a.set_weights(params)
    b = {s: YoloV3(n, [s, s, 3], K, SMALL_ANCHORS, **kw) for s in (96, 64)}
    b[96].set_weights(params)
    prev = None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'hand.npz')
        for i, s in enumerate([96, 64, 96]):
            la = float(a.train_step(batches[s]))
            m = b[s]
            if prev is not None and prev is not m:
                prev.save_weights(path)
                m.load_weights(path, load_optimizer=True)
            lb = float(m.train_step(batches[s]))
            torch.cuda.synchronize()
            prev = m
            assert la == lb and np.isfinite(la), (i, s, la, lb)
            assert float(a.last_ignored) == float(m.last_ignored) and int(a.last_truth_max) == int(m.last_truth_max)
    for name in ('params', 'adam_m', 'adam_v', 'moving', 'grads'):
        assert torch.equal(getattr(a, name), getattr(prev, name)), name
    p96, p64 = a._plan(n, True), a._plan(n, True, size=(64, 64))
    assert p96.truth_boxes is not p64.truth_boxes and p96.ignored is not p64.ignored and p96.truth_counts is not p64.truth_counts


# ---- 4. train.py ------------------------------------------------------------------------------------------------------------------
def test_cli_train_with_truth_mask(tmp_path):
    tmp = str(tmp_path)
    _write_dataset(tmp, 8, (256, 256, 3))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = os.path.join(tmp, 'out')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--batch_size', '2', '--test_every_n_steps', '3', '--train_database',
                        os.path.join(tmp, 'train-syn.lmdb'), '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out,
                        '--early_stopping', '1', '--use_augmentation', '1', '--max_epochs', '1', '--learning_rate', '1e-4',
                        '--ignore_mask', 'truth', '--ignore_thresh', '0.7'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'ignore_mask = truth' in r.stdout and 'ignore_thresh = 0.7' in r.stdout
    assert os.path.exists(os.path.join(out, 'saved_model', 'yolov3.npz'))
    dirs = glob.glob(os.path.join(out, 'scalars-*'))
    assert len(dirs) == 1
    lines = open(os.path.join(dirs[0], 'ignored.csv')).read().splitlines()
    assert lines[0] == 'step,ignored,truth_max' and len(lines) >= 2, lines
    for ln in lines[1:]:
        step, ignored, truth_max = (int(v) for v in ln.split(','))
        print(ln)
        assert ignored >= 0 and 0 <= truth_max <= 3, ln       # the synthetic records hold 1 to 3 boxes (augmentation may drop some)
    train = open(os.path.join(dirs[0], 'train.csv')).read().splitlines()
    assert len(train) == len(lines)                           # one row where train.csv gets its rows (no accumulation here)
