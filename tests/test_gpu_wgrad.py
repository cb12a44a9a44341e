"""The kernel gradient (y3_conv2d_wgrad_x) at the sizes training runs it, against fp64, and its reduction contract.

conv_wgrad_x3_kernel is the largest line of the training profile; test_conv_wgrad covers it on small ad-hoc shapes only.  Here:
every Appendix-A shape at batch 8 (the training batch: up to 86 528 pixels summed per weight) and the 13^2 / 26^2 shapes at batch 1
(small-batch training), which between them reach all four reduction forms of plan_wgrad_x3 (conv_plan.cpp) -- one pixel run, the
in-kernel ticket reduction, the slab reduction with XCD-remapped items, the slab reduction with the XCD-strided padded grid.
test_wgrad_cases_cover_every_reduction_form reads the plans back, so the claim holds if the planner moves.  Inputs look like
activations (mostly positive, non-zero mean: a wrong tap offset at the SAME-pad border changes the sums), src is a channel slice
of a wider concat buffer and both operands have a pitch beyond their channels, with NaN in everything a kernel must not read."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import APP_A, _conv_ref, _pad_same, hip      # noqa: F401  (hip: the module fixture)

SRC_PAD, SRC_OFF = 16, 16          # src = channels [16, 16 + cin) of a buffer of cin + 16 + 16 channels per pixel
DD_PAD = 8                         # ddst pitch: Nout rounded up to 4, plus 8
ONE_RUN_FLOOR = 1e-6               # x3 error floor (of max|ref|) for plans with a single pixel run: see the fp64 test's docstring


def _cases():
    out = [(8,) + s for s in APP_A]
    out += [(1,) + s for s in APP_A if s[0] in (13, 26) and s[2] >= 128]      # batch 1: one pixel run, 4-split tickets
    return out


CASES = _cases()
# the four reduction forms of the x3 kernel gradient (include/yolo3hip.h: y3_conv2d_wgrad_plan_x)
FORMS = ('one pixel run', 'in-kernel tickets', 'slab, XCD-remapped items', 'slab, XCD-strided padded grid')


def _plan(hip, m, cin, k, cout, flags):
    o = (C.c_int * 8)()
    ws = int(hip.lib.y3_conv2d_wgrad_plan_x(m, cin, k, cout, flags, o))
    return list(o), ws


def _form(plan):
    splits, in_kernel = plan[2], plan[5]
    if splits == 1:
        return FORMS[0]
    if in_kernel:
        return FORMS[1]
    return FORMS[2] if splits < 32 else FORMS[3]


def _geom(case):
    n, hw, cin, cout, k, s = case
    oh = -(-hw // s)
    return n, hw, cin, cout, k, s, oh, n * oh * oh


def _activations(g, shape):
    """leaky-relu of a normal plus an offset: what a conv's input and (roughly) its output gradient look like after BN + lrelu"""
    return F.leaky_relu(torch.randn(shape, generator=g) + 0.5, 0.1)


def test_wgrad_cases_cover_every_reduction_form():
    """CASES reach all four plan forms of the x3 kernel gradient (host-only plan query: no GPU)."""
    from yolo3 import _hip
    seen = {}
    for case in CASES:
        n, hw, cin, cout, k, s, oh, m = _geom(case)
        if _hip.lib.y3_conv2d_wgrad_x3_ok(m, cin, k, cout):
            plan, _ = _plan(_hip, m, cin, k, cout, _hip.CONV_X3)
            seen.setdefault(_form(plan), []).append((case, plan[2]))
    assert set(seen) == set(FORMS), sorted(seen)
    # the multi-split slab forms are not a single shape each: the padded grid with few and with many tiles
    assert len(seen[FORMS[3]]) >= 2 and len(seen[FORMS[1]]) >= 2


def _operands(hip, case, seed):
    from util import nhwc_buf
    n, hw, cin, cout, k, s, oh, m = _geom(case)
    g = torch.Generator().manual_seed(seed)
    x = _activations(g, (n, cin, hw, hw))
    if cin == 4:
        x[:, 3] = 0                     # the RGB layer: channels padded 3 -> 4
    dy = _activations(g, (n, cout, oh, oh)) - 0.3
    sld = cin + SRC_PAD + SRC_OFF
    sbuf, sv = nhwc_buf(n, hw, hw, cin, ld=sld, off=SRC_OFF)
    sv.copy_(x.permute(0, 2, 3, 1))
    cld = (cout + 3) // 4 * 4 + DD_PAD
    _, ddv = nhwc_buf(n, oh, oh, cout, ld=cld)
    ddv.copy_(dy.permute(0, 2, 3, 1))
    src = hip.Tensor(sv.data_ptr(), n, hw, hw, cin, sld)
    dd = hip.Tensor(ddv.data_ptr(), n, oh, oh, cout, cld)
    return x, dy, (sbuf, ddv), src, dd


def _ref_dw(x, dy, k, s):
    """fp64 autograd of the TF-SAME conv: dw in the Keras layout [kh, kw, cin, cout]"""
    wk = torch.zeros(k, k, x.shape[1], dy.shape[1], dtype=torch.float64, requires_grad=True)
    y = _conv_ref(x, wk, None, k, s)
    y.backward(dy.double())
    return wk.grad


def _run(hip, src, dd, k, s, dw, flags, ws=None):
    from util import stream
    wsb = int(hip.lib.y3_conv2d_wgrad_workspace_x(src, dd, k, s, flags))
    if ws is None:
        ws = torch.zeros(wsb // 4 + 4, device='cuda')        # tickets in the head: zeroed once (yolo3hip.h)
    rc = hip.lib.y3_conv2d_wgrad_x(src, dd, k, s, dw.data_ptr(), flags, ws.data_ptr(), wsb, stream())
    return rc, ws


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n%d_%d_%d_%d_k%d_s%d' % c)
def test_conv_wgrad_x3_error_against_fp64_at_training_size(hip, case):
    """f32 (v_mfma_f32) kernel gradient within 5e-5 * max|ref| of fp64 (test_conv_wgrad's rule); the x3 kernel gradient on the SAME
    inputs at most 2x the f32 kernel's error (or 2e-7 * max|ref|), the rule the forward and data gradient keep
    (test_conv_x3_error_against_fp64_is_that_of_the_f32_instruction).  Shapes y3_conv2d_wgrad_x3_ok() refuses must be refused
    loudly, with dw left unwritten.
    One exception to the 2x rule, measured: where the x3 plan sums all pixels in ONE run (batch 1 at 13^2: 169 pixels) the f32 plan
    cuts them into two runs of <= 96 and adds the halves, so x3's accumulator chain is twice as long and its error 1.6-2.0x the f32
    kernel's (4.3e-7 .. 7.0e-7 of max|ref|; every multi-split plan: 0.6-1.3x).  There x3 is held to 2x f32 or ONE_RUN_FLOOR * max|ref|."""
    n, hw, cin, cout, k, s, oh, m = _geom(case)
    x, dy, keep, src, dd = _operands(hip, case, seed=hw * 7 + cin + cout + k + n)
    ref = _ref_dw(x, dy, k, s)
    scale = float(ref.abs().max())
    ok = bool(hip.lib.y3_conv2d_wgrad_x3_ok(m, cin, k, cout))
    err = {}
    for name, flags in (('f32', 0), ('x3', hip.CONV_X3)):
        dw = torch.full((k, k, cin, cout), float('nan'), device='cuda')
        rc, _ = _run(hip, src, dd, k, s, dw, flags)
        if flags and not ok:
            assert rc != 0, 'x3 kernel gradient accepted a shape y3_conv2d_wgrad_x3_ok() refuses'
            torch.cuda.synchronize()
            assert torch.isnan(dw).all(), 'a refused x3 kernel gradient wrote dw'
            continue
        hip.check(rc, 'conv wgrad ' + name)
        got = dw.cpu().double()
        assert torch.isfinite(got).all(), name + ': non-finite dw'
        err[name] = float((got - ref).abs().max())
    line = {'case': list(case), 'scale': scale, 'f32': err['f32'], 'x3': err.get('x3')}
    if ok:
        plan, _ = _plan(hip, m, cin, k, cout, hip.CONV_X3)
        line.update(form=_form(plan), splits=plan[2], ratio=err['x3'] / max(err['f32'], 1e-300))
    print('wgrad error', json.dumps(line))
    assert err['f32'] <= 5e-5 * scale, 'f32 kernel gradient: error %.3e > 5e-5 * %.3e' % (err['f32'], scale)
    if ok:
        floor = ONE_RUN_FLOOR if line['splits'] == 1 else 2e-7
        assert err['x3'] <= max(2.0 * err['f32'], floor * scale), 'x3 kernel gradient: error %.3e vs f32 %.3e' % (err['x3'], err['f32'])


# one training shape per multi-split form of the x3 plan (checked below)
REPRO_CASES = [((8, 13, 512, 1024, 3, 2), FORMS[1]),       # 3 splits over 288 tiles
               ((8, 26, 512, 256, 1, 1), FORMS[2]),        # 29 splits
               ((8, 104, 64, 128, 3, 1), FORMS[3])]        # 91 splits (grid padded to 96) over 5 tiles


@pytest.mark.gpu
@pytest.mark.parametrize('arith', ['f32', 'x3'])
@pytest.mark.parametrize('case,form', REPRO_CASES, ids=lambda c: str(c).replace(' ', ''))
def test_conv_wgrad_reduction_is_reproducible_and_ignores_the_slab_contents(hip, case, form, arith):
    """Two calls on one workspace give the same bits (every ticket came back to zero), and a third call after the slab area
    behind the 256 KiB ticket header was filled with NaN still gives those bits: the workspace contract (yolo3hip.h) zeroes the
    header only, so nothing may read a slab before this call wrote it."""
    n, hw, cin, cout, k, s, oh, m = _geom(case)
    flags = hip.CONV_X3 if arith == 'x3' else 0
    plan, wsb = _plan(hip, m, cin, k, cout, flags)
    assert plan[2] > 1 and wsb > 256 * 1024
    if arith == 'x3':
        assert _form(plan) == form
    _, _, keep, src, dd = _operands(hip, case, seed=3)
    outs = []
    ws = None
    for rnd in range(3):
        if rnd == 2:
            ws[256 * 1024 // 4:].fill_(float('nan'))
        dw = torch.full((k, k, cin, cout), float('nan'), device='cuda')
        rc, ws = _run(hip, src, dd, k, s, dw, flags, ws)
        hip.check(rc, 'conv wgrad')
        torch.cuda.synchronize()
        assert int(ws[:256 * 1024 // 4].view(torch.int32).abs().sum()) == 0, 'a ticket did not return to zero'
        outs.append(dw.cpu())
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), 'second call on the same workspace differs'
    assert torch.equal(outs[0], outs[2]), 'the result depends on what the slab area held before the call'


# the stride-2 data gradients of Appendix A that the x3 merged launch takes (y3_conv2d_dgrad_x3_ok), at the training batch
DGRAD_S2 = [s for s in APP_A if s[4] == 2 and s[1] >= 64]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', DGRAD_S2, ids=lambda c: '%d_%d_%d_k%d_s%d' % c)
def test_conv_dgrad_x3_stride2_error_against_fp64_at_batch_8(hip, shape):
    """The stride-2 data gradients at batch 8 (other K-slice plans than at batch 1-2): x3 error at most 2x the f32 kernel's on the
    same inputs (or 2e-7 * max|ref|), f32 within 2e-5 * max|ref|, as test_conv_x3_error_against_fp64_is_that_of_the_f32_instruction."""
    from util import nhwc_buf, stream, x3_planes
    hw, cin, cout, k, s = shape
    n, oh = 8, -(-hw // s)
    g = torch.Generator().manual_seed(hw * 5 + cin + cout)
    wk = torch.randn(k, k, cin, cout, generator=g) * (1.0 / (k * k * cin) ** 0.5)
    dy = torch.randn(n, cout, oh, oh, generator=g)
    cld = cout + DD_PAD
    _, dyv = nhwc_buf(n, oh, oh, cout, ld=cld)
    dyv.copy_(dy.permute(0, 2, 3, 1))
    DY = hip.Tensor(dyv.data_ptr(), n, oh, oh, cout, cld)
    xr = torch.zeros(n, cin, hw, hw, dtype=torch.float64, requires_grad=True)
    _conv_ref(xr, wk, None, k, s).backward(dy.double())
    refd = xr.grad.permute(0, 2, 3, 1)
    scale = float(refd.abs().max())
    dld = cin + 4
    assert hip.lib.y3_conv2d_dgrad_x3_ok(DY, k, s, hip.Tensor(0, n, hw, hw, cin, dld))
    w_keras = wk.contiguous().cuda()
    err = {}
    for name, flag, wt in (('f32', 0, wk.permute(0, 1, 3, 2).contiguous().cuda()), ('x3', hip.CONV_X3, x3_planes(hip, w_keras))):
        _, dxv = nhwc_buf(n, hw, hw, cin, ld=dld, fill=0.0)
        DX = hip.Tensor(dxv.data_ptr(), n, hw, hw, cin, dld)
        wsb = int(hip.lib.y3_conv2d_dgrad_workspace_x(DY, k, s, DX, flag))
        ws = torch.zeros(wsb // 4 + 4, device='cuda')
        hip.check(hip.lib.y3_conv2d_dgrad(DY, wt.data_ptr(), k, s, DX, flag, ws.data_ptr(), wsb, stream()), 'conv dgrad ' + name)
        got = dxv.cpu().double()
        assert torch.isfinite(got).all(), name
        err[name] = float((got - refd).abs().max())
    print('dgrad error', json.dumps({'shape': list(shape), 'scale': scale, 'f32': err['f32'], 'x3': err['x3'], 'ratio': err['x3'] / err['f32']}))
    assert err['f32'] <= 2e-5 * scale
    assert err['x3'] <= max(2.0 * err['f32'], 2e-7 * scale), 'data gradient: x3 error %.3e vs f32 %.3e' % (err['x3'], err['f32'])
