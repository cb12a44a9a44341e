"""The kernel gradient (y3_conv2d_wgrad_x) and the stride-2 data gradient (y3_conv2d_dgrad, y3_conv2d_dgrad_bn) under every plan form,
against fp64.

plan_wgrad / plan_wgrad_x3 choose tile, pixel runs and reduction form from (m, cin, ksize, cout), plan_dgrad_multi_* the tile and the
K slices of each parity class: another batch or image size is another code path.  tests/grad_forms.py classifies the launches of the
network at batch 1-16 x image side 320-608 (its docstring defines the signatures) and picks the cheapest real layer of every class,
plus the odd-sized stride-2 shapes; this file runs each of them (test id = class + layer shape):

* operands as the model lays them out: the source a channel slice at an offset of a wider buffer, pitches beyond the channels, NaN in
  everything a kernel must not read or write; activation-like data (leaky-relu of a normal plus an offset: a zero-mean input hides
  a wrong border tap or run boundary -- test_cpu_grad_forms.py shows that these data do not);
* references: ONE fp64 convolution on the CPU each (grad_forms.wgrad_reference / dgrad2_reference), shared by the two arithmetics;
* the tolerances are the ones the older tests keep: kernel gradient f32 5e-5 * max|ref|, x3 at most twice the f32 kernel's error on
  the same inputs or the floor of test_gpu_wgrad (2e-7, ONE_RUN_FLOOR for a single pixel run); data gradient 2e-5 * max|ref|
  (test_conv_dgrad), its BatchNorm-backward moments as test_gpu_plan_forms.  Next to every kernel check an fp32 evaluation of the
  same inputs on the CPU must stay within HALF the bound, so a failure says whether the data or the kernel is at fault.  For the
  kernel gradient that evaluation is one fp32 convolution per image and band of 32 output rows, the bands added in fp32 in order
  (grad_forms.wgrad_f32_banded: an order over the pixels of its own, whatever the library does inside a call; one call over all
  416^2 pixels of the first layer comes to 0.3 of the bound); it stays below 0.05 of the bound for every class, so it is asserted
  for all of them;
* the plan read back from the library is the class, the workspace queries give the plan's bytes;
* the workspace contract (include/yolo3hip.h) for every plan that splits: the first launch finds a zero ticket header and NaN in the
  whole slab area, the second the workspace as the first left it; both finite and bit-identical, the header zero afterwards.  One
  byte less than the plan's bytes: the kernel gradient refuses and leaves dw unwritten; the data gradient, given no workspace, runs
  its whole-tile fallback within the same bound.

With Y3_GRAD_FORMS_PROFILE=<file> the worst error / bound ratio of every class is written there (profiles/grad_forms.txt is such a
run); no tolerance here is derived from those figures."""
import os

import pytest
import torch

import grad_forms as gf
from test_gpu_kernels import hip      # noqa: F401  (the module fixture)
from test_gpu_plan_forms import BN_TOL, DBIAS_TOL, HDR, _bits_equal, _bn_reference, _header_is_zero, _ratio, _workspace
from test_gpu_wgrad import ONE_RUN_FLOOR

WGRAD_TOL, X3_FLOOR, DGRAD_TOL = 5e-5, 2e-7, 2e-5      # test_conv_wgrad / test_gpu_wgrad / test_conv_dgrad

CASES = sorted(gf.cases('wgrad') + gf.cases('dgrad2'), key=lambda r: (r[1].entry, r[1].shape(), r[1].arith))      # the arithmetics of a shape share a reference
ROWS = {}
COLS = ('wgrad', 'dgrad', 'dgrad_accum', 'dgrad_no_ws', 'bn_moments', 'cpu_fp32')


@pytest.fixture(scope='module', autouse=True)
def _profile():
    yield
    _CACHE.clear()       # the last shape's inputs and reference: not kept for the rest of the session
    path = os.environ.get('Y3_GRAD_FORMS_PROFILE')
    if path and ROWS:
        with open(path, 'w') as f:
            f.write('# worst error / bound per gradient form (tests/test_gpu_grad_forms.py; 1.0 = at the bound, - = not part of the class)\n')
            f.write('# bounds: wgrad f32 %g of max|ref|, x3 max(2 x the f32 kernel\'s error, %g (one run: %g) of max|ref|); dgrad %g of max|ref|;\n'
                    '# bn_moments %g (dbias %g); cpu_fp32: the fp32 evaluation on the CPU against the f32 bound (must stay <= 0.5)\n'
                    % (WGRAD_TOL, X3_FLOOR, ONE_RUN_FLOOR, DGRAD_TOL, BN_TOL, DBIAS_TOL))
            f.write('%-58s %-30s %s\n' % ('# class', 'n,h,w,cin,cout,k,s', ' '.join('%11s' % c for c in COLS)))
            for cid in sorted(ROWS):
                shape, r = ROWS[cid]
                f.write('%-58s %-30s %s\n' % (cid, ','.join(str(v) for v in shape), ' '.join('%11s' % ('%.4f' % r[c] if c in r else '-') for c in COLS)))


_CACHE = {}


def _cached(key, make):
    """the inputs and fp64 reference of a shape, kept until another shape asks"""
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def _wgrad_data(shape):
    n, h, w, cin, cout, k, s = shape
    x, dy = gf.wgrad_inputs(shape)
    ref = gf.wgrad_reference(x, dy, k, s)
    return dict(x=x, dy=dy, ref=ref, cpu32=_ratio(gf.wgrad_f32_banded(x, dy, k, s), ref, WGRAD_TOL), f32err=None)


def _dgrad2_data(shape):
    dy, wk, init, a = gf.dgrad2_inputs(shape)
    ref = gf.dgrad2_reference(shape, dy, wk)
    return dict(dy=dy, wk=wk, init=init, a=a, ref=ref, cpu32=_ratio(gf.dgrad2_reference(shape, dy, wk, dtype=torch.float32), ref, DGRAD_TOL))


def _wgrad_launches(hip, src, dd, k, s, shape, flags, wsb):
    """y3_conv2d_wgrad_x once, or twice on one workspace where the plan splits: the list of dw, each pre-filled with NaN"""
    from util import stream
    n, h, w, cin, cout = shape[:5]
    ws = _workspace(wsb)
    outs = []
    for launch in range(2 if wsb else 1):        # the second one finds the workspace as the first left it
        dw = torch.full((k, k, cin, cout), float('nan'), device='cuda')
        hip.check(hip.lib.y3_conv2d_wgrad_x(src, dd, k, s, dw.data_ptr(), flags, ws.data_ptr(), wsb, stream()), 'conv wgrad')
        torch.cuda.synchronize()
        assert _header_is_zero(ws), 'launch %d left a ticket behind' % launch
        outs.append(dw)
    return outs, ws


def _kernel_gradient(hip, sig, mb):
    from util import nhwc_buf, stream
    n, h, w, cin, cout, k, s = mb.shape()
    oh, ow, flags = mb.oh, mb.ow, mb.flags
    assert mb.signature() == sig, 'the representative is no longer what the library plans'
    plan, wsb = mb.plan()
    form = gf.wgrad_form(plan)
    assert (wsb > HDR * 4) == (form != 'onerun') and (wsb == 0) == (form == 'onerun'), plan
    c = _cached(('wgrad', mb.shape()), lambda: _wgrad_data(mb.shape()))
    row = {'cpu_fp32': c['cpu32']}
    print('%s plan %s: fp32 on the CPU at %.4f of the f32 bound' % (mb.id(), plan, c['cpu32']))
    assert c['cpu32'] <= 0.5, 'the DATA break the bound (fp32 per image and row band on the CPU: %.3f of it)' % c['cpu32']
    sld, cld = gf.src_ld(cin), gf.dst_ld(cout)
    sbuf, sv = nhwc_buf(n, h, w, cin, ld=sld, off=gf.SRC_OFF)
    sv.copy_(c['x'].permute(0, 2, 3, 1))
    dbuf, ddv = nhwc_buf(n, oh, ow, cout, ld=cld)
    ddv.copy_(c['dy'].permute(0, 2, 3, 1))
    src, dd = hip.Tensor(sv.data_ptr(), n, h, w, cin, sld), hip.Tensor(ddv.data_ptr(), n, oh, ow, cout, cld)
    assert int(hip.lib.y3_conv2d_wgrad_workspace_x(src, dd, k, s, flags)) == wsb
    ref = c['ref']
    scale = float(ref.abs().max())

    def error(dw):
        got = dw.cpu().double()
        assert torch.isfinite(got).all(), 'non-finite dw'
        return float((got - ref).abs().max())

    outs, ws = _wgrad_launches(hip, src, dd, k, s, mb.shape(), flags, wsb)
    err = error(outs[0])
    if mb.arith == 'f32':
        c['f32err'] = err
        bound = WGRAD_TOL * scale
    else:
        if c['f32err'] is None:          # the f32 kernel on the same inputs, under its own plan
            c['f32err'] = error(_wgrad_launches(hip, src, dd, k, s, mb.shape(), 0, gf.wgrad_plan(mb.m, cin, k, cout, 0)[1])[0][0])
        bound = max(2.0 * c['f32err'], (ONE_RUN_FLOOR if plan[2] == 1 else X3_FLOOR) * scale)
        assert c['f32err'] <= WGRAD_TOL * scale, 'the f32 kernel gradient on these inputs: error %.3e > 5e-5 * %.3e' % (c['f32err'], scale)
    row['wgrad'] = err / bound
    print('  wgrad error %.3e (f32 kernel %.3e, max|ref| %.3e): %.4f of the bound' % (err, c['f32err'], scale, row['wgrad']))
    ROWS[gf.sig_id(sig)] = (mb.shape(), row)
    assert row['wgrad'] <= 1.0, 'kernel gradient: %.3f of the bound (error %.3e, f32 kernel %.3e, max|ref| %.3e)' % (row['wgrad'], err, c['f32err'], scale)
    if wsb:
        assert _bits_equal(outs[0], outs[1]), 'the second launch on the same workspace gives other bits'
        # one byte less than the plan's bytes: refused, dw left unwritten
        dw = torch.full((k, k, cin, cout), float('nan'), device='cuda')
        rc = hip.lib.y3_conv2d_wgrad_x(src, dd, k, s, dw.data_ptr(), flags, ws.data_ptr(), wsb - 1, stream())
        torch.cuda.synchronize()
        assert rc != 0, 'a workspace one byte short was accepted'
        assert torch.isnan(dw).all() and _header_is_zero(ws), 'a refused kernel gradient wrote dw or a ticket'


def _data_gradient2(hip, sig, mb):
    from util import nhwc_buf, stream, x3_planes
    n, h, w, cin, cout, k, s = mb.shape()
    oh, ow, x3 = mb.oh, mb.ow, mb.flags
    assert mb.signature() == sig, 'the representative is no longer what the library plans'
    c = _cached(('dgrad2', mb.shape()), lambda: _dgrad2_data(mb.shape()))
    row = {'cpu_fp32': c['cpu32']}
    cld, dld = gf.src_ld(cout), gf.dst_ld(cin)
    _, ddv = nhwc_buf(n, oh, ow, cout, ld=cld, off=gf.SRC_OFF)
    ddv.copy_(c['dy'].permute(0, 2, 3, 1))
    dbuf, dsv = nhwc_buf(n, h, w, cin, ld=dld)
    DD, DS = hip.Tensor(ddv.data_ptr(), n, oh, ow, cout, cld), hip.Tensor(dsv.data_ptr(), n, h, w, cin, dld)
    how, rows, cls, exact = gf.dgrad_plan(mb.shape(), x3, DD, DS)
    assert (how, rows, cls, exact) == mb.plan(), 'the plan depends on the data pointers'
    print('%s %s, %d rows, %d bytes, classes %s: fp32 on the CPU at %.4f of the bound'
          % (mb.id(), how, rows, exact, [(q['taps'], q['m'], q['tiles'], q['s0'], q['chunk0'], q['nk']) for q in cls], c['cpu32']))
    assert c['cpu32'] <= 0.5, 'the DATA break the bound (fp32 conv2d_input on the CPU: %.3f of it)' % c['cpu32']
    cuts = any(q['s0'] > 1 or q['s1'] > 1 for q in cls)
    assert (exact > HDR * 4) == cuts and (exact == 0) == (not cuts)
    if x3:
        assert hip.lib.y3_conv2d_dgrad_x3_ok(DD, k, s, DS) and how == 'merged-x3'
        wop = x3_planes(hip, c['wk'].contiguous().cuda())                       # planes of the Keras layout [kh, kw, ci, co]
    else:
        wop = c['wk'].permute(0, 1, 3, 2).contiguous().cuda()                   # [kh, kw, co, ci]
    wsb = int(hip.lib.y3_conv2d_dgrad_workspace_x(DD, k, s, DS, x3))            # what the model allocates and passes
    assert wsb >= exact and (wsb == exact or how != 'merged-x3')
    ws = _workspace(wsb)
    ref = c['ref']
    outs = []
    for launch in range(2 if cuts else 1):       # the second one finds the workspace as the first left it
        dbuf.fill_(float('nan'))
        hip.check(hip.lib.y3_conv2d_dgrad(DD, wop.data_ptr(), k, s, DS, x3, ws.data_ptr(), wsb, stream()), 'conv dgrad')
        torch.cuda.synchronize()
        assert _header_is_zero(ws), 'launch %d left a ticket behind' % launch
        outs.append(dbuf.clone())
    got = outs[0].view(n, h, w, dld)
    row['dgrad'] = _ratio(got[..., :cin].cpu(), ref, DGRAD_TOL)
    # dsrc += v, on the workspace the launches above left
    dsv.copy_(c['init'])
    hip.check(hip.lib.y3_conv2d_dgrad(DD, wop.data_ptr(), k, s, DS, hip.EPI_ACCUM | x3, ws.data_ptr(), wsb, stream()), 'conv dgrad, accumulate')
    row['dgrad_accum'] = _ratio(dsv.cpu(), ref + c['init'].double(), DGRAD_TOL)
    pad_ok = bool(torch.isnan(got[..., cin:]).all() and torch.isnan(dbuf.view(n, h, w, dld)[..., cin:]).all()) and _header_is_zero(ws)
    print('  dgrad %.4f accumulate %.4f of the bound' % (row['dgrad'], row['dgrad_accum']))
    ROWS[gf.sig_id(sig)] = (mb.shape(), row)
    assert row['dgrad'] <= 1.0, 'conv dgrad: %.3f of the bound' % row['dgrad']
    assert row['dgrad_accum'] <= 1.0, 'conv dgrad with Y3_EPI_ACCUM: %.3f of the bound' % row['dgrad_accum']
    assert pad_ok, 'pitch padding overwritten, or a ticket left behind'
    if cuts:
        assert _bits_equal(outs[0], outs[1]), 'the second launch on the same workspace gives other bits'
        # workspace_bytes = 0 disables the split (yolo3hip.h): the whole-tile fallback of the merged launch
        dbuf.fill_(float('nan'))
        hip.check(hip.lib.y3_conv2d_dgrad(DD, wop.data_ptr(), k, s, DS, x3, ws.data_ptr(), 0, stream()), 'conv dgrad without a workspace')
        row['dgrad_no_ws'] = _ratio(dsv.cpu(), ref, DGRAD_TOL)
        print('  without a workspace %.4f of the bound' % row['dgrad_no_ws'])
        assert row['dgrad_no_ws'] <= 1.0, 'conv dgrad, whole-tile fallback: %.3f of the bound' % row['dgrad_no_ws']
        assert torch.isnan(dbuf.view(n, h, w, dld)[..., cin:]).all() and _header_is_zero(ws)
    tiles = int(hip.lib.y3_conv2d_dgrad_bn_tiles_x(DD, k, s, DS, x3))
    assert tiles == rows, 'the rows of partial statistics: %d, the plan says %d' % (tiles, rows)
    if not tiles:
        assert how == 'by-class', 'a merged data gradient without the BatchNorm-backward epilogue'
        return
    # y3_conv2d_dgrad_bn: the same gradient bits, and the partial moments of (gradient, bn_a) per row tile
    _, av = nhwc_buf(n, h, w, cin, ld=cin + 8)
    av.copy_(c['a'])
    A = hip.Tensor(av.data_ptr(), n, h, w, cin, cin + 8)
    part = torch.empty(tiles * 6 * cin, device='cuda')
    parts = []
    for launch in range(2 if cuts else 1):
        dbuf.fill_(float('nan'))
        part.fill_(float('nan'))
        hip.check(hip.lib.y3_conv2d_dgrad_bn(DD, wop.data_ptr(), k, s, DS, x3, A, part.data_ptr(), ws.data_ptr(), wsb, stream()), 'conv dgrad_bn')
        torch.cuda.synchronize()
        assert _header_is_zero(ws), 'dgrad_bn launch %d left a ticket behind' % launch
        assert _bits_equal(dbuf, outs[0]), 'y3_conv2d_dgrad_bn (launch %d) changed the data gradient' % launch
        parts.append(part.clone())
    assert torch.isfinite(parts[0]).all(), 'non-finite partial moments'
    if cuts:
        assert _bits_equal(parts[0], parts[1]), 'the second dgrad_bn launch on the same workspace gives other partial moments'
    g = torch.Generator().manual_seed(cin * 3 + cout + k)
    gamma, mean, rstd = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.1, torch.rand(cin, generator=g) + 0.5
    gd, md, rd = gamma.cuda(), mean.cuda(), rstd.cuda()
    res = [torch.empty(cin, device='cuda') for _ in range(3)] + [torch.empty(3 * cin, device='cuda')]
    hip.check(hip.lib.y3_bn_bwd_finalize_tiles(parts[0].data_ptr(), tiles, cin, n * h * w, gd.data_ptr(), md.data_ptr(), rd.data_ptr(), 0.2,
                                               res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr(), stream()), 'bn_bwd_finalize_tiles')
    want = _bn_reference(ref, c['a'], gamma, mean, rstd, 0.2)
    dbias_scale = float((want[3][:cin].abs() * ref.abs().sum(dim=(0, 1, 2))).max())      # |k1| sum |dy|: the sums dbias is a difference of
    worst = 0.0
    for name, r_, x_ in zip(('dgamma', 'dbeta', 'dbias', 'coef'), want, res):
        q = _ratio(x_.cpu(), r_, BN_TOL) if name != 'dbias' else _ratio(x_.cpu(), r_, 0, atol=DBIAS_TOL * dbias_scale)
        print('  bn %s %.4f of the bound' % (name, q))
        worst = max(worst, q)
    row['bn_moments'] = worst
    assert worst <= 1.0, 'BatchNorm-backward quantities from the epilogue moments: %.3f of the bound' % worst


@pytest.mark.gpu
@pytest.mark.parametrize('sig,mb', CASES, ids=[mb.id() for _, mb in CASES])
def test_grad_form(hip, sig, mb):
    """One launch form of y3_conv2d_wgrad_x / the stride-2 y3_conv2d_dgrad (see the module docstring) on a real layer, against fp64."""
    if mb.entry == 'wgrad':
        _kernel_gradient(hip, sig, mb)
    else:
        _data_gradient2(hip, sig, mb)
