"""The default loss path (y3_loss_fwd_bwd: loss_kernel<Y3_BOX_LOSS_MSE, false> with loss_present / loss_clear / loss_finalize) and
y3_decode_fwd on the branches that N(0, 1.2^2) logits do not take, on the fixed inputs of tests/loss_edges.py, whose conditions
tests/test_cpu_loss_edges.py asserts without a GPU.

Tolerances are the project's for these kernels: gradients 1e-4 of the largest reference magnitude of the tensor and, stricter, of the
channels under test alone; loss parts 2e-5 (test_loss_fwd_bwd_matches_oracle, test_gpu_box_loss); decode rtol 1e-5 on boxes and
rtol 1e-5, atol 2e-6 on scores (test_decode_matches_oracle).  What is left out of a comparison is what a band rule of loss_edges
names -- the objectness gradient of negatives within BAND of the mask threshold, the xy gradient of positives within CLIP_BAND of
a clip edge -- and nothing else.  Every comparison prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import loss_edges as E
from test_gpu_box_loss import GBS, SENTINEL, _Scale

pytestmark = pytest.mark.gpu

assert GBS == E.GBS


@pytest.fixture(scope='module')
def hip():
    from yolo3 import _hip
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return _hip


class _WsScale(_Scale):
    """_Scale whose launch takes the caller's workspace (the flag-hygiene tests share one between launches)."""

    def fresh_workspace(self, fill=0.0):
        return torch.full((int(self.hip.lib.y3_loss_workspace_bytes()) // 4,), fill, device='cuda')       # exactly what the header promises

    def launch_on(self, ws):
        """y3_loss_fwd_bwd on the current stream -> (loss4 [4], dfm buffer with its padding)"""
        hip = self.hip
        buf, dv = self.nhwc_buf(self.n, self.Gh, self.Gw, self.D, ld=self.ld, fill=SENTINEL)
        loss4 = torch.zeros(4, device='cuda')
        H, W = self.case['hw']
        tf_ = hip.Tensor(self.fv.data_ptr(), self.n, self.Gh, self.Gw, self.D, self.ld)
        td = hip.Tensor(dv.data_ptr(), self.n, self.Gh, self.Gw, self.D, self.ld)
        hip.check(hip.lib.y3_loss_fwd_bwd(tf_, self.gd.data_ptr(), self.anc, self.A, self.K, H, W, GBS, loss4.data_ptr(), td, ws.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
        return loss4, buf


def _err(got, want):
    return float((got - want).abs().max()) if got.numel() else 0.0


def _compare_gradient(got, want, info, what, channels, skip_obj=None, skip_xy=None):
    """got / want [n, Gh, Gw, A, 5+K].  skip_obj / skip_xy: cells whose objectness / xy gradient a band rule leaves out.  1e-4 of the
    largest reference magnitude of the whole tensor and, stricter, of ``channels`` (a slice) alone."""
    got, want = got.double().clone(), want.clone()
    assert bool(torch.isfinite(got).all()), '%s: non-finite gradient' % what
    for skip, ch in ((skip_obj, slice(4, 5)), (skip_xy, slice(0, 2))):
        if skip is not None:
            got[..., ch][skip] = 0.0
            want[..., ch][skip] = 0.0
    scale, sub_scale = float(want.abs().max()), float(want[..., channels].abs().max())
    err, sub_err = _err(got, want), _err(got[..., channels], want[..., channels])
    print('%s: positives %d, ignored negatives %d, left out: objectness of %d band members, xy of %d in the clip band; max err %.3e = %.2e of '
          'the tensor scale %.3e; channels %s: %.3e = %.2e of their scale %.3e'
          % (what, int(info['positive'].sum()), int(info['ignored'].sum()), 0 if skip_obj is None else int(skip_obj.sum()),
             0 if skip_xy is None else int(skip_xy.sum()), err, err / max(scale, 1e-30), scale, (channels.start, channels.stop), sub_err,
             sub_err / max(sub_scale, 1e-30), sub_scale))
    assert err <= 1e-4 * scale, '%s: max abs err %.3e > 1e-4 * %.3e' % (what, err, scale)
    assert sub_err <= 1e-4 * sub_scale, '%s: channels %s, max abs err %.3e > 1e-4 * %.3e' % (what, channels, sub_err, sub_scale)


def _compare_parts(got, want, what, obj_slack=0.0):
    """Loss parts (xy, wh, obj, class) on all cells at 2e-5 of the largest part; the objectness part, stricter, at 2e-5 of itself plus
    ``obj_slack``, the objectness terms of the band members (loss_edges.band_objectness_bound)."""
    from util import assert_close
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print('%s: loss parts got %s want %s; rel err %s; objectness off by %.3e, bound %.3e (band members explain %.3e of it)'
          % (what, got.tolist(), want.tolist(), ['%.2e' % (abs(g - w) / max(abs(w), 1e-30)) for g, w in zip(got, want)],
             abs(got[2] - want[2]), 2e-5 * abs(want[2]) + obj_slack, obj_slack))
    assert_close(got, want, rtol=2e-5, what=what)
    assert abs(got[2] - want[2]) <= 2e-5 * abs(want[2]) + obj_slack, '%s: objectness part %r vs %r' % (what, got[2], want[2])


# ---- 1. the ignore mask and the anchor-present flags -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(E.MASK_CASES))
def test_mask_dense_case_matches_fp64_autograd(hip, name):
    """y3_loss_fwd_bwd on logits planted so that the mask fires often, under label sets that make both, one or the other anchor present.
    Measured on an MI355X: gradient errors at most 1.7e-5 of the tensor scale and 8.4e-8 of the objectness channel's (bound 1e-4),
    loss parts within 2.6e-7 (bound 2e-5); no input has a band member."""
    case = E.make_mask_case(name)
    (pos, neg, ign, bnd, absent), _ = E.mask_counts(name)
    print('%s: positives %d, negatives %d, ignored %d, band members %d, absent-only %d' % (name, pos, neg, ign, bnd, absent))
    assert ign >= E.MIN_IGNORED and bnd <= E.MAX_BAND_SHARE * ign
    assert absent >= E.MIN_ABSENT_ONLY or len(E.MASK_CASES[name][4]) == len(case['anchors'])
    loss4 = torch.zeros(4, device='cuda')
    want_parts, slack = np.zeros(4), 0.0
    for si in range(3):
        s = _Scale(hip, case, si)
        parts, gref, info = E.mask_reference(name, si)
        want_parts += parts
        slack += E.band_objectness_bound(info)
        _, buf = s.launch(None, loss4=loss4)
        torch.cuda.synchronize()
        got = s.cells(buf)
        _compare_gradient(got, gref, info, '%s scale %d dfm' % (name, si), slice(4, 5), skip_obj=info['band'])
        # an ignored negative outside the band gets exactly zero, one the flags keep out of the mask does not
        sure = info['ignored'] & ~info['band']
        assert bool((got[..., 4][sure] == 0).all())
        assert bool((got[..., 4][E.absent_only(info)] != 0).all())
        assert bool((s.padding(buf) == SENTINEL).all())
    _compare_parts(loss4.cpu().numpy(), want_parts, name, slack)


def test_threshold_is_part_of_the_mask(hip):
    """A negative whose best IoU is 0.5 exactly, in float32 and in float64, is ignored: `best < 0.5` is false."""
    case = E.make_threshold_case()
    gy, gx, a = E.THRESHOLD_CELL
    s = _Scale(hip, case, 0)
    parts, gref, info = E.reference(case, 0)
    l, buf = s.launch(None)
    torch.cuda.synchronize()
    got = s.cells(buf)
    print('threshold case: objectness gradient of the planted predictions %s (fp64 %s); of their other anchor %s'
          % (got[:, gy, gx, a, 4].tolist(), gref[:, gy, gx, a, 4].tolist(), got[:, gy, gx, 1 - a, 4].tolist()))
    assert bool((gref[:, gy, gx, a, 4] == 0).all())
    assert bool((got[:, gy, gx, a, 4] == 0).all())
    planted = torch.zeros_like(info['band'])
    planted[:, gy, gx, a] = True
    assert torch.equal(info['band'], planted)            # nothing but the planted predictions is near the threshold: compared in full
    _compare_gradient(got, gref, info, 'threshold case dfm', slice(4, 5))
    _compare_parts(l.cpu().numpy(), parts, 'threshold case')


def test_present_flags_do_not_outlive_a_call(hip):
    """One workspace, one stream: only anchor 1 present, then only anchor 0 -- the second result is that of a fresh zeroed workspace,
    bit for bit; so is the result on a workspace of y3_loss_workspace_bytes() filled with NaN bit patterns; and so is that of labels
    without an object after a call with both anchors present (no flag set: nothing is ignored)."""
    only0, only1, both = (E.make_mask_case(k) for k in ('sq416_only0', 'sq416_only1', 'sq416_both'))
    none = E.make_mask_case('sq416_both', True)
    for si in range(3):
        s0, s1, sb, sn = (_WsScale(hip, c, si) for c in (only0, only1, both, none))
        fresh = s0.launch_on(s0.fresh_workspace())
        ws = s0.fresh_workspace()
        s1.launch_on(ws)
        after = s0.launch_on(ws)
        dirty = s0.launch_on(s0.fresh_workspace(float('nan')))
        fresh_none = sn.launch_on(sn.fresh_workspace())
        ws2 = sn.fresh_workspace()
        sb.launch_on(ws2)
        after_none = sn.launch_on(ws2)
        torch.cuda.synchronize()
        for what, (l, d) in (('after the other anchor', after), ('NaN-filled workspace', dirty)):
            same = torch.equal(l, fresh[0]) and torch.equal(d, fresh[1])
            print('scale %d, %s: loss4 %s vs fresh %s, dfm equal: %s' % (si, what, l.tolist(), fresh[0].tolist(), torch.equal(d, fresh[1])))
            assert same, (si, what)
        print('scale %d, no object after both anchors: loss4 %s vs fresh %s' % (si, after_none[0].tolist(), fresh_none[0].tolist()))
        assert torch.equal(after_none[0], fresh_none[0]) and torch.equal(after_none[1], fresh_none[1])
        # and nothing is ignored there: every objectness gradient is sigmoid(logit) * gscale > 0 unless float32 rounds it to 0
        _, gref, info = E.mask_reference('sq416_both', si, True)
        assert int(info['ignored'].sum()) == 0
        _compare_gradient(sn.cells(after_none[1]), gref, info, 'no object, scale %d dfm' % si, slice(4, 5))


# ---- 2. gates of the MSE box terms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(E.GATE_SEEDS))
def test_gates_of_the_mse_box_terms(hip, name):
    """Positives on both sides of the xy clip and of the wh clamp, negatives whose size logits overflow expf.  Measured on an MI355X:
    gradient errors at most 2.5e-5 of the scale of the box channels (bound 1e-4; the largest belong to open xy gates next to a clip
    edge, whose in-cell position carries the float32 rounding of sigmoid + offset), loss parts within 2.1e-6 (bound 2e-5)."""
    case, masks = E.make_gate_case(name)
    k = E.gate_counts(name)
    print('%s: positives %d; [below, inside, above] x %s y %s w %s h %s; clip band %d; overflowing negatives %d'
          % (name, k['positives'], k['x'], k['y'], k['w'], k['h'], k['clip_band'], k['overflow']))
    assert all(min(k[key]) >= E.MIN_PER_GATE for key in 'xywh') and k['clip_band'] <= 0.01 * k['positives']
    loss4 = torch.zeros(4, device='cuda')
    want_parts = np.zeros(4)
    for si in range(3):
        s = _Scale(hip, case, si)
        assert float(torch.exp(s.fv[..., 2]).max()) == float('inf')          # the overflow is real in float32
        parts, gref, info = E.gate_reference(name, si)
        want_parts += parts
        l, buf = s.launch(None, loss4=loss4)
        torch.cuda.synchronize()
        got = s.cells(buf)
        assert bool(torch.isfinite(loss4).all()) and bool(torch.isfinite(buf).all())
        pos, over, cb = info['positive'], masks[si], E.clip_band(info)
        _compare_gradient(got, gref, info, '%s gates scale %d dfm' % (name, si), slice(0, 4), skip_obj=info['band'], skip_xy=cb)
        # a gate closed in fp64 (outside the clip band) is an exact zero of the kernel
        gxy, gwh = E.xy_gate(info), E.wh_gate(info)
        closed_xy = pos.unsqueeze(-1) & (gxy != 0) & ~cb.unsqueeze(-1)
        closed_wh = pos.unsqueeze(-1) & (gwh != 0)
        open_xy = pos.unsqueeze(-1) & (gxy == 0) & ~cb.unsqueeze(-1)
        print('%s gates scale %d: closed xy gates %d, closed wh gates %d, open xy gates %d'
              % (name, si, int(closed_xy.sum()), int(closed_wh.sum()), int(open_xy.sum())))
        assert bool((got[..., 0:2][closed_xy] == 0).all()) and bool((got[..., 2:4][closed_wh] == 0).all())
        assert bool((got[..., 0:2][open_xy] != 0).all())
        # negatives, the overflowing ones among them: zero in the box channels, the objectness gradient of fp64 (nothing is masked
        # there: x / inf = 0 in float32, below 1e-30 in fp64)
        assert bool((got[..., 0:4][~pos] == 0).all()) and bool((got[..., 0:4][over] == 0).all())
        assert not bool(info['ignored'][over].any()) and bool((got[..., 4][over] != 0).all())
        oerr, oscale = _err(got[..., 4][over].double(), gref[..., 4][over]), float(gref[..., 4].abs().max())
        print('%s gates scale %d: objectness gradient of %d overflowing negatives, max err %.3e = %.2e of the channel scale %.3e'
              % (name, si, int(over.sum()), oerr, oerr / oscale, oscale))
        assert oerr <= 1e-4 * oscale
        assert bool((s.padding(buf) == SENTINEL).all())
    _compare_parts(loss4.cpu().numpy(), want_parts, '%s gates' % name, 0.0)


def test_size_logit_that_underflows_takes_the_zero_rule(hip):
    """expf(-110) = 0 in float32: size / anchor == 0 becomes 1, the term is (log true_twh - 0)^2 and its gradient exactly 0
    (loss_edges.underflow_rule)."""
    case, plants = E.make_underflow_case()
    loss4 = torch.zeros(4, device='cuda')
    want_parts = np.zeros(4)
    for si in range(3):
        s = _Scale(hip, case, si)
        m = plants[si]
        assert float(torch.exp(s.fv[..., 2:4]).min()) == 0.0                  # the underflow is real in float32
        parts, gref, info = E.underflow_rule(case, si, m)
        want_parts += parts
        _, buf = s.launch(None, loss4=loss4)
        torch.cuda.synchronize()
        got = s.cells(buf)
        print('underflow scale %d: wh gradient of the planted entries %s' % (si, got[..., 2:4][m].tolist()))
        assert bool((got[..., 2:4][m] == 0).all())
        _compare_gradient(got, gref, info, 'underflow scale %d dfm' % si, slice(0, 4), skip_obj=info['band'], skip_xy=E.clip_band(info))
    _compare_parts(loss4.cpu().numpy(), want_parts, 'underflow', 0.0)


# ---- 3. decode ---------------------------------------------------------------------------------------------------------------------
def _decode(hip, c, out=None, nscales=None, tweak=None):
    """y3_decode_fwd on a loss_edges decode case -> (return code, out [n, Nb, 5+K])."""
    from util import nhwc_buf, stream
    A, K, n = len(c['anchors']), c['K'], c['n']
    D = A * (5 + K)
    arr = (hip.Tensor * max(len(c['fms']), 5))()
    views = []
    for i, (f, ld) in enumerate(zip(c['fms'], c['lds'])):
        _, v = nhwc_buf(n, f.shape[2], f.shape[3], D, ld=ld)           # padding NaN: reading it would show
        v.copy_(f.permute(0, 2, 3, 1))
        views.append(v)
        arr[i] = hip.Tensor(v.data_ptr(), n, f.shape[2], f.shape[3], D, ld)
    for i in range(len(c['fms']), 5):
        arr[i] = arr[0]
    if tweak is not None:
        tweak(arr)
    if out is None:
        out = torch.full((n, c['want'].shape[1], 5 + K), SENTINEL, device='cuda')
    rc = hip.lib.y3_decode_fwd(arr, len(c['fms']) if nscales is None else nscales, hip.float_array([v for a in c['anchors'] for v in a]), A, K,
                               c['hw'][0], c['hw'][1], out.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, out


def _compare_boxes(got, want, what):
    """Corner columns, rtol 1e-5 of the largest reference magnitude among them (test_decode_matches_oracle)."""
    from util import assert_close
    e, sc = _err(got.double(), want), float(want.abs().max())
    print('%s: %d values; max err %.3e = %.2e of the box scale %.3e (bound 1e-5)' % (what, got.numel(), e, e / sc, sc))
    assert_close(got, want, rtol=1e-5, what=what)


def _compare_scores(got, want, what):
    from util import assert_close
    print('%s: %d values; max err %.3e (bound 2e-6)' % (what, got.numel(), _err(got.double(), want)))
    assert_close(got, want, rtol=1e-5, atol=2e-6, what=what)


@pytest.mark.parametrize('name', sorted(E.DECODE_CASES))
def test_decode_shapes_match_oracle(hip, name):
    """1, 2 and 4 scales with their own ld each, K = 1, a grid on which the stride swap (Q6) shows, and 532 350 rows: more than the
    2048 blocks of 256 threads the launch is clamped to, so the grid-stride loop takes a second pass."""
    c = E.make_decode_case(name)
    rows = c['n'] * c['want'].shape[1]
    if name == 'second_pass':
        assert rows == 532350 and rows > E.DECODE_MAX_THREADS
    rc, out = _decode(hip, c)
    assert rc == 0, hip.lib.y3_last_error()
    got = out.cpu()
    _compare_boxes(got[..., :4], c['want'][..., :4], name + ' boxes')
    _compare_scores(got[..., 4:], c['want'][..., 4:], name + ' scores')


@pytest.mark.parametrize('name', ['four_scales_k1', 'rect_q6'])
def test_decode_saturated_and_overflowing_logits(hip, name):
    """Centre and score logits of +-30 against fp64; rows with a size logit of 100 hold the float32 evaluation, c -+ inf / 2."""
    c = E.make_decode_case(name, True)
    rc, out = _decode(hip, c)
    assert rc == 0, hip.lib.y3_last_error()
    got, want, over = out.cpu(), c['want'], c['over']
    assert not bool(torch.isnan(got).any())
    assert float(got[..., 4:].min()) >= 0.0 and float(got[..., 4:].max()) <= 1.0
    _compare_scores(got[..., 4:], want[..., 4:], name + ' extreme, scores of all rows')
    plain = ~over.any(-1)
    _compare_boxes(got[plain][:, :4], want[plain][:, :4], name + ' extreme, boxes of rows without overflow')
    inf = float('inf')
    ow, oh = over[..., 0], over[..., 1]
    print('%s extreme: rows with an overflowing width %d, height %d' % (name, int(ow.sum()), int(oh.sum())))
    assert bool((got[..., 0][ow] == -inf).all()) and bool((got[..., 2][ow] == inf).all())
    assert bool((got[..., 1][oh] == -inf).all()) and bool((got[..., 3][oh] == inf).all())
    # the axis that does not overflow is as everywhere
    _compare_boxes(got[ow & ~oh][:, [1, 3]], want[ow & ~oh][:, [1, 3]], name + ' extreme, y corners of rows with an overflowing width')
    _compare_boxes(got[oh & ~ow][:, [0, 2]], want[oh & ~ow][:, [0, 2]], name + ' extreme, x corners of rows with an overflowing height')


def test_refused_decode_leaves_out_untouched(hip):
    c = E.make_decode_case('four_scales_k1')

    def wrong_c(arr):
        arr[2].c += 1

    def wrong_n(arr):
        arr[1].n += 1

    for what, kw in (('nscales 0', dict(nscales=0)), ('nscales 5', dict(nscales=5)), ('c != A * (5 + K)', dict(tweak=wrong_c)),
                     ('mismatched n', dict(tweak=wrong_n))):
        rc, out = _decode(hip, c, **kw)
        print('%s: return code %d, %s' % (what, rc, hip.lib.y3_last_error().decode()))
        assert rc == -1, what
        assert bool((out == SENTINEL).all()), what
    rc, out = _decode(hip, c)
    assert rc == 0 and not bool((out == SENTINEL).any())
