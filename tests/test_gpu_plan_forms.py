"""y3_conv2d_fwd and the stride-1 y3_conv2d_dgrad under every split-K plan form, against fp64.

plan_conv / plan_conv_x3 choose kernel, tile, K slices and the reducing slice per launch from (m, cin, ksize, cout): another batch
or image size is another code path.  tests/plan_forms.py classifies the launches of the network at batch 1-16 x image side 320-608
by plan form and picks the cheapest real layer of every class; this file runs each of them (test id = class + layer shape):

* operands as the model lays them out: the source a channel slice of a wider buffer, the destination with a pitch beyond its
  channels, NaN in everything a kernel must not read or write; activation-like data (leaky-relu of a normal plus OFFSET: a
  zero-mean input hides a wrong border tap);
* the tolerances are the ones test_gpu_kernels.py keeps (test_conv_fwd, test_conv_dgrad, test_conv_dgrad_bn_epilogue_stats); next
  to every kernel check a plain fp32 evaluation of the same inputs on the CPU must stay within HALF the bound, so a failure says
  whether the data or the kernel is at fault;
* the workspace contract (include/yolo3hip.h) for every plan that splits: the first launch finds a zero ticket header and NaN in
  the whole slab area, the second the workspace as the first left it; both finite and bit-identical, statistics included, the
  header zero afterwards.

With Y3_PLAN_FORMS_PROFILE=<file> the worst error / bound ratio of every class is written there (profiles/plan_forms.txt is such
a run); no tolerance here is derived from those figures."""
import os

import pytest
import torch
import torch.nn.functional as F

import plan_forms as pf
from test_gpu_kernels import _conv_ref, hip      # noqa: F401  (hip: the module fixture)

OFFSET = 0.5             # of the normal under the leaky-relu that makes activations, gradients and residuals: one constant for all cases
SRC_OFF, SRC_PAD = 16, 16    # the source: channels [16, 16 + c) of a buffer of 16 + c (rounded up to 4) + 16 channels per pixel
DST_PAD = 8              # destination pitch: channels rounded up to 4, plus 8
HDR = 256 * 1024 // 4    # floats of ticket header in front of the slabs
FWD_TOL, STATS_TOL, DGRAD_TOL = 2e-5, 1e-4, 2e-5      # test_conv_fwd / test_conv_dgrad
BN_TOL, DBIAS_TOL = 2e-5, 1e-4                        # test_conv_dgrad_bn_epilogue_stats

REPS, LEFT_OUT = pf.representatives()
REPS = sorted(REPS, key=lambda r: (r[1].entry, r[1].shape(), r[1].arith))      # the two arithmetics of a shape share a reference


def _epilogue_classes():
    """the first two forward classes of every (arithmetic, split form): they also run the inference epilogue"""
    out, seen = set(), {}
    for sig, mb in sorted(REPS, key=lambda r: pf.sig_id(r[0])):
        if sig[0] == 'fwd' and seen.setdefault((sig[1], sig[5]), 0) < 2:
            seen[(sig[1], sig[5])] += 1
            out.add(sig)
    return out


EPILOGUE = _epilogue_classes()
ROWS = {}


@pytest.fixture(scope='module', autouse=True)
def _profile():
    yield
    path = os.environ.get('Y3_PLAN_FORMS_PROFILE')
    if path and ROWS:
        cols = ('fwd', 'stats', 'epilogue', 'dgrad', 'dgrad_accum', 'bn_moments')
        with open(path, 'w') as f:
            f.write('# worst error / bound per plan form (tests/test_gpu_plan_forms.py; 1.0 = at the bound, - = not part of the class)\n')
            f.write('# bounds: fwd %g, stats %g, dgrad %g of max|ref|; bn_moments %g (dbias %g)\n' % (FWD_TOL, STATS_TOL, DGRAD_TOL, BN_TOL, DBIAS_TOL))
            f.write('%-52s %-30s %s\n' % ('# class', 'n,h,w,cin,cout,k,s', ' '.join('%11s' % c for c in cols)))
            for cid in sorted(ROWS):
                shape, r = ROWS[cid]
                f.write('%-52s %-30s %s\n' % (cid, ','.join(str(v) for v in shape), ' '.join('%11s' % ('%.4f' % r[c] if c in r else '-') for c in cols)))


def _act(g, shape, alpha=0.1):
    return F.leaky_relu(torch.randn(shape, generator=g) + OFFSET, alpha)


def _ratio(got, ref, tol, atol=None):
    """max|got - ref| over the bound (tol * max|ref| unless given); got must be finite"""
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all(), 'non-finite output'
    bound = tol * max(float(ref.abs().max()), 1e-30) if atol is None else atol
    return float((got - ref).abs().max()) / bound


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _workspace(wsb):
    """a workspace as the contract wants it before the FIRST launch -- header zero -- with NaN in all of the slab area"""
    ws = torch.zeros(wsb // 4 + 4, device='cuda')
    ws[HDR:].fill_(float('nan'))
    return ws


def _header_is_zero(ws):
    return int(ws[:HDR].view(torch.int32).abs().sum()) == 0


_CACHE = {}


def _cached(key, make):
    """the inputs and fp64 reference of a shape, kept until another shape asks"""
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def _seed(shape):
    return sum(v * p for v, p in zip(shape, (7, 11, 13, 17, 19, 23, 29)))


def _fwd_reference(shape):
    n, h, w, cin, cout, k, s = shape
    g = torch.Generator().manual_seed(_seed(shape))
    x = _act(g, (n, cin, h, w))
    if cin == 4:
        x[:, 3] = 0                      # the RGB layer: channels padded 3 -> 4
    wk = torch.randn(k, k, cin, cout, generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    oh, ow = -(-h // s), -(-w // s)
    r = _act(g, (n, cout, oh, ow))
    ref = F.leaky_relu(_conv_ref(x, wk, b, k, s), 0.2)
    f32 = F.leaky_relu(_conv_ref(x, wk, b, k, s, dtype=torch.float32), 0.2)
    return dict(x=x, wk=wk, b=b, sc=sc, sh=sh, r=r, ref=ref, cpu32=_ratio(f32, ref, FWD_TOL))


def _dgrad_reference(shape):
    n, h, w, cin, cout, k, s = shape
    assert s == 1
    g = torch.Generator().manual_seed(_seed(shape) + 1)
    dy = _act(g, (n, cout, h, w))
    wk = torch.randn(k, k, cin, cout, generator=g) * 0.1
    init = torch.randn(n, h, w, cin, generator=g)
    a = _act(g, (n, h, w, cin), 0.2)     # activation of the layer that produced the conv's input (y3_conv2d_dgrad_bn)
    w_oihw = wk.permute(3, 2, 0, 1)
    # fp64 autograd's data gradient of the SAME-padded stride-1 conv (pad k // 2 on every side), without paying for its forward
    ref = torch.nn.grad.conv2d_input((n, cin, h, w), w_oihw.double(), dy.double(), stride=1, padding=k // 2).permute(0, 2, 3, 1)
    f32 = torch.nn.grad.conv2d_input((n, cin, h, w), w_oihw.contiguous(), dy, stride=1, padding=k // 2).permute(0, 2, 3, 1)
    return dict(dy=dy, wk=wk, init=init, a=a, ref=ref, cpu32=_ratio(f32, ref, DGRAD_TOL))


def _bn_reference(dz, a, gamma, mean, rstd, alpha):
    """dgamma, dbeta, dbias, coef[3][c] of y3_bn_bwd_stats / y3_bn_bwd_finalize_tiles from fp64 moments of (dz, a), both [n, h, w, c]"""
    dz, a = dz.double().reshape(-1, dz.shape[-1]), a.double().reshape(-1, a.shape[-1])
    ga, mu, rr = gamma.double(), mean.double(), rstd.double()
    count = dz.shape[0]
    pos = (a > 0).double()
    s0, s1, s2, s3, s4, s5 = dz.sum(0), (dz * a).sum(0), (dz * pos).sum(0), (a * pos).sum(0), pos.sum(0), a.sum(0)
    db = s0
    dg = rr * (s1 - mu * s0)                                                           # sum dz * xhat
    sdys = alpha * s0 + (1 - alpha) * s2                                               # sum dz * slope
    ss = alpha * count + (1 - alpha) * s4                                              # sum slope
    sxs = rr * ((1 - alpha) * (s3 - mu * s4) + alpha * (s5 - mu * count))              # sum xhat * slope
    dbias = ga * rr * (sdys - db / count * ss - dg / count * sxs)
    k1 = ga * rr
    k2 = -ga * rr * rr * dg / count
    k3 = -ga * rr * db / count - k2 * mu
    return dg, db, dbias, torch.cat([k1, k2, k3])


def _check_class(hip, sig, mb):
    """the representative is still what the library plans on this machine"""
    flags = hip.CONV_X3 if mb.arith == 'x3' else 0
    assert mb.signature() == sig
    p, wsb = pf.plan(*mb.gemm(), flags=flags)
    assert (wsb > HDR * 4) == (sig[5] != 'whole'), p
    return flags, p, wsb


def _forward(hip, sig, mb):
    from util import nhwc_buf, stream, x3_planes
    n, h, w, cin, cout, k, s = mb.shape()
    x3, plan, wsb = _check_class(hip, sig, mb)
    c = _cached(('fwd', mb.shape()), lambda: _fwd_reference(mb.shape()))
    row = {}
    print('%s plan %s: fp32 on the CPU at %.4f of the bound' % (mb.id(), plan, c['cpu32']))
    assert c['cpu32'] <= 0.5, 'the DATA break the bound (fp32 conv2d on the CPU: %.3f of it): lower OFFSET' % c['cpu32']
    oh, ow, m = mb.oh, mb.ow, n * mb.oh * mb.ow
    sld = SRC_OFF + cin + SRC_PAD
    sbuf, sv = nhwc_buf(n, h, w, cin, ld=sld, off=SRC_OFF)
    sv.copy_(c['x'].permute(0, 2, 3, 1))
    dld = (cout + 3) // 4 * 4 + DST_PAD
    dbuf, dv = nhwc_buf(n, oh, ow, cout, ld=dld)
    wd = c['wk'].contiguous().cuda()
    if x3:
        wd = x3_planes(hip, c['wk'].permute(0, 1, 3, 2).contiguous().cuda())
    bd = c['b'].cuda()
    src, dst = hip.Tensor(sv.data_ptr(), n, h, w, cin, sld), hip.Tensor(dv.data_ptr(), n, oh, ow, cout, dld)
    tiles = int(hip.lib.y3_conv2d_stats_tiles_x(m, cin, k, cout, x3))
    assert tiles == plan[10] and int(hip.lib.y3_conv2d_fwd_workspace_x(m, cin, k, cout, x3)) == wsb
    stats = torch.empty(tiles * 2 * cout, device='cuda')
    ws = _workspace(wsb)
    outs = []
    for launch in range(2 if wsb else 1):        # the second one finds the workspace as the first left it
        dbuf.fill_(float('nan'))
        stats.fill_(float('nan'))
        hip.check(hip.lib.y3_conv2d_fwd(src, wd.data_ptr(), bd.data_ptr(), k, s, dst, hip.EPI_LRELU | x3, 0.2, None, None, None, stats.data_ptr(),
                                        ws.data_ptr(), wsb, stream()), 'conv fwd')
        torch.cuda.synchronize()
        assert _header_is_zero(ws), 'launch %d left a ticket behind' % launch
        outs.append((dbuf.clone(), stats.clone()))
    ref = c['ref']
    got = outs[0][0].view(n, oh, ow, dld)
    row['fwd'] = _ratio(got[..., :cout].cpu().permute(0, 3, 1, 2), ref, FWD_TOL)
    st = outs[0][1].view(tiles, 2, cout).double().sum(0).cpu()
    assert torch.isfinite(outs[0][1]).all(), 'non-finite statistics'
    rs, rq = ref.sum(dim=(0, 2, 3)), (ref * ref).sum(dim=(0, 2, 3))
    row['stats'] = max(_ratio(st[0], rs, 0, atol=STATS_TOL * float(ref.abs().sum(dim=(0, 2, 3)).max())), _ratio(st[1], rq, STATS_TOL))
    print('  fwd %.4f stats %.4f of the bound' % (row['fwd'], row['stats']))
    ROWS[pf.sig_id(sig)] = (mb.shape(), row)
    assert row['fwd'] <= 1.0, 'conv fwd: %.3f of the bound' % row['fwd']
    assert row['stats'] <= 1.0, 'conv fwd statistics: %.3f of the bound' % row['stats']
    assert torch.isnan(got[..., cout:]).all(), 'pitch padding overwritten'
    if wsb:
        assert _bits_equal(outs[0][0], outs[1][0]), 'the second launch on the same workspace gives other output bits'
        assert _bits_equal(outs[0][1], outs[1][1]), 'the second launch on the same workspace gives other statistics'
    if sig in EPILOGUE:      # the inference epilogue: lrelu -> scale / shift -> + residual, no statistics
        scd, shd = c['sc'].cuda(), c['sh'].cuda()
        _, rv = nhwc_buf(n, oh, ow, cout, ld=dld)
        rv.copy_(c['r'].permute(0, 2, 3, 1))
        dbuf.fill_(float('nan'))
        hip.check(hip.lib.y3_conv2d_fwd(src, wd.data_ptr(), bd.data_ptr(), k, s, dst, hip.EPI_LRELU | x3, 0.2, scd.data_ptr(), shd.data_ptr(),
                                        hip.Tensor(rv.data_ptr(), n, oh, ow, cout, dld), None, ws.data_ptr(), wsb, stream()), 'conv fwd, inference epilogue')
        eref = ref * c['sc'].double()[None, :, None, None] + c['sh'].double()[None, :, None, None] + c['r'].double()
        row['epilogue'] = _ratio(dv.cpu().permute(0, 3, 1, 2), eref, FWD_TOL)
        print('  inference epilogue %.4f of the bound' % row['epilogue'])
        assert row['epilogue'] <= 1.0, 'fused inference epilogue: %.3f of the bound' % row['epilogue']
        assert torch.isnan(dbuf.view(n, oh, ow, dld)[..., cout:]).all() and _header_is_zero(ws)


def _data_gradient(hip, sig, mb):
    from util import nhwc_buf, stream, x3_planes
    n, h, w, cin, cout, k, s = mb.shape()
    x3, plan, wsb = _check_class(hip, sig, mb)
    c = _cached(('dgrad', mb.shape()), lambda: _dgrad_reference(mb.shape()))
    row = {}
    print('%s plan %s: fp32 on the CPU at %.4f of the bound' % (mb.id(), plan, c['cpu32']))
    assert c['cpu32'] <= 0.5, 'the DATA break the bound (fp32 conv2d_input on the CPU: %.3f of it): lower OFFSET' % c['cpu32']
    cld = SRC_OFF + (cout + 3) // 4 * 4 + SRC_PAD
    _, ddv = nhwc_buf(n, h, w, cout, ld=cld, off=SRC_OFF)
    ddv.copy_(c['dy'].permute(0, 2, 3, 1))
    dld = cin + DST_PAD
    dbuf, dsv = nhwc_buf(n, h, w, cin, ld=dld)
    DD, DS = hip.Tensor(ddv.data_ptr(), n, h, w, cout, cld), hip.Tensor(dsv.data_ptr(), n, h, w, cin, dld)
    if x3:
        assert hip.lib.y3_conv2d_dgrad_x3_ok(DD, k, 1, DS)
        wop = x3_planes(hip, c['wk'].contiguous().cuda())                       # planes of the Keras layout [kh, kw, ci, co]
    else:
        wop = c['wk'].permute(0, 1, 3, 2).contiguous().cuda()                   # [kh, kw, co, ci]
    assert int(hip.lib.y3_conv2d_dgrad_workspace_x(DD, k, 1, DS, x3)) == wsb
    ws = _workspace(wsb)
    ref = c['ref']
    outs = []
    for launch in range(2 if wsb else 1):
        dbuf.fill_(float('nan'))
        hip.check(hip.lib.y3_conv2d_dgrad(DD, wop.data_ptr(), k, 1, DS, x3, ws.data_ptr(), wsb, stream()), 'conv dgrad')
        torch.cuda.synchronize()
        assert _header_is_zero(ws), 'launch %d left a ticket behind' % launch
        outs.append(dbuf.clone())
    got = outs[0].view(n, h, w, dld)
    row['dgrad'] = _ratio(got[..., :cin].cpu(), ref, DGRAD_TOL)
    # dsrc += v, on the workspace the launches above left
    dsv.copy_(c['init'])
    hip.check(hip.lib.y3_conv2d_dgrad(DD, wop.data_ptr(), k, 1, DS, hip.EPI_ACCUM | x3, ws.data_ptr(), wsb, stream()), 'conv dgrad, accumulate')
    row['dgrad_accum'] = _ratio(dsv.cpu(), ref + c['init'].double(), DGRAD_TOL)
    pad_ok = bool(torch.isnan(got[..., cin:]).all() and torch.isnan(dbuf.view(n, h, w, dld)[..., cin:]).all()) and _header_is_zero(ws)
    print('  dgrad %.4f accumulate %.4f of the bound' % (row['dgrad'], row['dgrad_accum']))
    ROWS[pf.sig_id(sig)] = (mb.shape(), row)
    assert row['dgrad'] <= 1.0, 'conv dgrad: %.3f of the bound' % row['dgrad']
    assert row['dgrad_accum'] <= 1.0, 'conv dgrad with Y3_EPI_ACCUM: %.3f of the bound' % row['dgrad_accum']
    assert pad_ok, 'pitch padding overwritten, or a ticket left behind'
    if wsb:
        assert _bits_equal(outs[0], outs[1]), 'the second launch on the same workspace gives other bits'
    tiles = int(hip.lib.y3_conv2d_dgrad_bn_tiles_x(DD, k, 1, DS, x3))
    if not tiles:
        assert not sig[2] or os.environ.get('Y3_NO_FAST'), 'a fast-path data gradient without the BatchNorm-backward epilogue'
        return
    # y3_conv2d_dgrad_bn: the same gradient bits, and the partial moments of (gradient, bn_a) per row tile
    _, av = nhwc_buf(n, h, w, cin, ld=cin + 8)
    av.copy_(c['a'])
    A = hip.Tensor(av.data_ptr(), n, h, w, cin, cin + 8)
    part = torch.empty(tiles * 6 * cin, device='cuda')
    parts = []
    for launch in range(2 if wsb else 1):
        dbuf.fill_(float('nan'))
        part.fill_(float('nan'))
        hip.check(hip.lib.y3_conv2d_dgrad_bn(DD, wop.data_ptr(), k, 1, DS, x3, A, part.data_ptr(), ws.data_ptr(), wsb, stream()), 'conv dgrad_bn')
        torch.cuda.synchronize()
        assert _header_is_zero(ws), 'dgrad_bn launch %d left a ticket behind' % launch
        assert _bits_equal(dbuf, outs[0]), 'y3_conv2d_dgrad_bn (launch %d) changed the data gradient' % launch
        parts.append(part.clone())
    assert torch.isfinite(parts[0]).all(), 'non-finite partial moments'
    if wsb:
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
@pytest.mark.parametrize('sig,mb', REPS, ids=[mb.id() for _, mb in REPS])
def test_plan_form(hip, sig, mb):
    """One launch form of y3_conv2d_fwd / y3_conv2d_dgrad (see the module docstring) on a real layer of the network, against fp64."""
    if mb.entry == 'fwd':
        _forward(hip, sig, mb)
    else:
        _data_gradient(hip, sig, mb)
