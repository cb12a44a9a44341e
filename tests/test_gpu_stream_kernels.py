"""The streaming kernels of csrc/pointwise.hip and the bf16 helpers of csrc/conv_bf16.hip at their edges, through the C ABI as
yolo3/model.py calls it: every case of tests/stream_kernels.py against its fp64 reference, within the derived bound element by
element and channel by channel; NaN canaries around every written view; bits where the operation is exact.

Y3_STREAM_ERR=<file> writes the worst error / bound of every (entry point, case, output) of the run to <file>
(profiles/stream_kernels_err.txt is such a run)."""
import os

import numpy as np
import pytest
import torch

import stream_kernels as sk

pytestmark = pytest.mark.gpu
NAN = float('nan')


@pytest.fixture(scope='module')
def hip():
    from yolo3 import _hip
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    yield _hip
    path = os.environ.get('Y3_STREAM_ERR')
    if path:
        with open(path, 'w') as f:
            f.write('# worst |error| / bound per entry point and case, and the output that gave it (tests/test_gpu_stream_kernels.py)\n')
            worst = {}
            for (entry, cid, name), r in sk.RATIOS.items():
                if '(restated)' not in entry and r >= worst.get((entry, cid), (-1.0, ''))[0]:
                    worst[(entry, cid)] = (r, name)
            for (entry, cid), (r, name) in sorted(worst.items()):
                f.write('%-26s %-22s %.3f  %s\n' % (entry, cid, r, name))


def _ids(cases):
    return [c['id'] for c in cases]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _buf(M, c, pad=0, off=0, dtype=torch.float32, src=None):
    """NaN-filled flat CUDA buffer and the [M, c] view of pitch c + pad that starts `off` elements in"""
    ld = c + pad
    flat = torch.full((off + M * ld + 8,), NAN, dtype=dtype, device='cuda')
    view = torch.as_strided(flat, (M, c), (ld, 1), off)
    if src is not None:
        view.copy_(src.reshape(M, c))
    return flat, view, ld


def _canaries_alive(flat, view):
    """every element of the flat buffer outside the view is still NaN"""
    chk = flat.clone()
    torch.as_strided(chk, view.shape, view.stride(), view.storage_offset()).zero_()
    return int(torch.isnan(chk.float()).sum()) == flat.numel() - view.numel() and not bool(torch.isnan(view.float()).any())


def _outs(sizes):
    """per-channel outputs carved from one NaN buffer with 4-float gaps: {name: view}, flat"""
    total = 4 + sum(n + 4 for n in sizes.values())
    flat = torch.full((total,), NAN, device='cuda')
    views, o = {}, 4
    for k, n in sizes.items():
        views[k] = flat[o:o + n]
        o += n + 4
    return views, flat


def _gaps_alive(flat, views):
    return int(torch.isnan(flat).sum()) == flat.numel() - sum(v.numel() for v in views.values())


def _bnb_outs(c):
    return _outs(dict(dgamma=c, dbeta=c, dbias=c, coef=3 * c))


def _bnb_launch(hip, DY, A, DR, acc, d, o, ws, ws_bytes):
    g, m, r = d['gamma'].cuda(), d['mean'].cuda(), d['rstd'].cuda()
    rc = hip.lib.y3_bn_bwd_stats(DY, A, DR, acc, g.data_ptr(), m.data_ptr(), r.data_ptr(), sk.ALPHA, o['dgamma'].data_ptr(), o['dbeta'].data_ptr(),
                                 o['dbias'].data_ptr(), o['coef'].data_ptr(), ws.data_ptr(), ws_bytes, _st())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('case', sk.BNB_CASES + [sk.BNB_GRID_CASE], ids=_ids(sk.BNB_CASES + [sk.BNB_GRID_CASE]))
def test_bn_bwd_stats_and_apply(hip, case):
    d = sk.bnb_case(case)
    M, c, want, bound = case['M'], case['c'], d['want'], d['bound']
    plan = sk.plan_bnb(M, c)
    dyF, dyV, dy_ld = _buf(M, c, case['pad'][0], case['off'][0], src=d['dy'])
    aF, aV, a_ld = _buf(M, c, case['pad'][1], case['off'][1], src=d['a'])
    drF, drV, dr_ld = _buf(M, c, case['pad'][2], case['off'][2])
    DY, A, DR = hip.Tensor(dyV.data_ptr(), 1, 1, M, c, dy_ld), hip.Tensor(aV.data_ptr(), 1, 1, M, c, a_ld), hip.Tensor(drV.data_ptr(), 1, 1, M, c, dr_ld)
    ws_bytes = int(hip.lib.y3_bn_bwd_workspace(M, c))
    assert ws_bytes == plan['workspace']
    ws = torch.zeros(ws_bytes + 256, dtype=torch.uint8, device='cuda')
    ws[ws_bytes:] = 0xA5
    o, oF = _bnb_outs(c)
    # without dres; dres = dy into a NaN view; dres += dy onto known values: identical per-channel bits every time
    hip.check(_bnb_launch(hip, DY, A, None, 0, d, o, ws, ws_bytes), 'bn_bwd_stats')
    first = oF.clone()
    assert int(ws[:1024].view(torch.int32).abs().sum()) == 0, 'tickets not reset'
    hip.check(_bnb_launch(hip, DY, A, DR, 0, d, o, ws, ws_bytes), 'bn_bwd_stats dres')
    assert torch.equal(drV, dyV) and _canaries_alive(drF, drV), 'dres = dy'
    assert torch.equal(oF.view(torch.int32), first.view(torch.int32)), 'bn_bwd_stats is not reproducible'
    r0 = torch.from_numpy(np.random.default_rng(1).standard_normal((M, c)).astype(np.float32)).cuda()
    drV.copy_(r0)
    hip.check(_bnb_launch(hip, DY, A, DR, 1, d, o, ws, ws_bytes), 'bn_bwd_stats dres accumulate')
    assert torch.equal(drV, r0 + dyV) and _canaries_alive(drF, drV), 'dres += dy'
    assert torch.equal(oF.view(torch.int32), first.view(torch.int32)), 'bn_bwd_stats is not reproducible'
    assert int(ws[:1024].view(torch.int32).abs().sum()) == 0, 'tickets not reset'
    assert bool((ws[ws_bytes:] == 0xA5).all()), 'wrote past the workspace it asked for'
    assert _gaps_alive(oF, o) and _canaries_alive(dyF, dyV) and _canaries_alive(aF, aV)
    got = dict(dgamma=o['dgamma'], dbeta=o['dbeta'], dbias=o['dbias'], k1=o['coef'][:c], k2=o['coef'][c:2 * c], k3=o['coef'][2 * c:])
    fails = []
    for k in got:
        try:
            sk.check('bn_bwd_stats', case['id'], k, got[k], want[k], bound[k])
        except AssertionError as e:
            fails.append(str(e))
    # apply, and apply with the fan-in: the same dz bits, dres exactly dy / dres + dy
    dzF, dzV, dz_ld = _buf(M, c, 4, 4)
    DZ = hip.Tensor(dzV.data_ptr(), 1, 1, M, c, dz_ld)
    hip.check(hip.lib.y3_bn_bwd_apply(DY, A, o['coef'].data_ptr(), sk.ALPHA, DZ, _st()), 'bn_bwd_apply')
    torch.cuda.synchronize()
    assert _canaries_alive(dzF, dzV)
    try:
        sk.check('bn_bwd_apply', case['id'], 'dz', dzV, want['dz'], bound['dz'])
    except AssertionError as e:
        fails.append(str(e))
    dz2F, dz2V, _ = _buf(M, c, 4, 4)
    DZ2 = hip.Tensor(dz2V.data_ptr(), 1, 1, M, c, dz_ld)
    drF.fill_(NAN)
    hip.check(hip.lib.y3_bn_bwd_apply_fanin(DY, A, o['coef'].data_ptr(), sk.ALPHA, DZ2, DR, 0, _st()), 'bn_bwd_apply_fanin')
    torch.cuda.synchronize()
    assert torch.equal(dz2V.view(torch.int32), dzV.view(torch.int32)) and torch.equal(drV, dyV) and _canaries_alive(drF, drV)
    drV.copy_(r0)
    hip.check(hip.lib.y3_bn_bwd_apply_fanin(DY, A, o['coef'].data_ptr(), sk.ALPHA, DZ2, DR, 1, _st()), 'bn_bwd_apply_fanin accumulate')
    torch.cuda.synchronize()
    assert torch.equal(dz2V.view(torch.int32), dzV.view(torch.int32)) and torch.equal(drV, r0 + dyV) and _canaries_alive(drF, drV) and _canaries_alive(dz2F, dz2V)
    assert not fails, '\n'.join(fails)


def test_bn_bwd_finalize_tiles_agrees_with_bn_bwd_stats_on_the_same_data(hip):
    case = sk.BNB_GRID_CASE
    d = sk.bnb_case(case)
    M, c = case['M'], case['c']
    _, dyV, dy_ld = _buf(M, c, 0, 0, src=d['dy'])
    _, aV, a_ld = _buf(M, c, 0, 0, src=d['a'])
    ws_bytes = int(hip.lib.y3_bn_bwd_workspace(M, c))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device='cuda')
    o, _ = _bnb_outs(c)
    hip.check(_bnb_launch(hip, hip.Tensor(dyV.data_ptr(), 1, 1, M, c, dy_ld), hip.Tensor(aV.data_ptr(), 1, 1, M, c, a_ld), None, 0, d, o, ws, ws_bytes))
    partials = sk.tile_moments(d['a'], d['dy'], case['tile_rows'])
    _, fbound = sk.bwd_finalize_reference(partials, d['gamma'], d['mean'], d['rstd'], M)
    f, fF = _bnb_outs(c)
    pd, g, m, r = partials.cuda(), d['gamma'].cuda(), d['mean'].cuda(), d['rstd'].cuda()
    hip.check(hip.lib.y3_bn_bwd_finalize_tiles(pd.data_ptr(), partials.shape[0], c, M, g.data_ptr(), m.data_ptr(), r.data_ptr(), sk.ALPHA, f['dgamma'].data_ptr(),
                                               f['dbeta'].data_ptr(), f['dbias'].data_ptr(), f['coef'].data_ptr(), _st()), 'bn_bwd_finalize_tiles')
    torch.cuda.synchronize()
    assert _gaps_alive(fF, f)
    for k, sl in (('dgamma', None), ('dbeta', None), ('dbias', None), ('k1', slice(0, c)), ('k2', slice(c, 2 * c)), ('k3', slice(2 * c, 3 * c))):
        a_, b_ = (o[k], f[k]) if sl is None else (o['coef'][sl], f['coef'][sl])
        sk.check('finalize_tiles==stats', case['id'], k, b_, a_.double().cpu(), d['bound'][k] + fbound[k])


@pytest.mark.parametrize('case', sk.BWD_FINALIZE_CASES, ids=_ids(sk.BWD_FINALIZE_CASES))
def test_bn_bwd_finalize_tiles(hip, case):
    d = sk.bwd_finalize_case(case)
    c = case['c']
    f, fF = _bnb_outs(c)
    pd, g, m, r = d['partials'].cuda(), d['gamma'].cuda(), d['mean'].cuda(), d['rstd'].cuda()
    hip.check(hip.lib.y3_bn_bwd_finalize_tiles(pd.data_ptr(), case['tiles'], c, d['count'], g.data_ptr(), m.data_ptr(), r.data_ptr(), sk.ALPHA,
                                               f['dgamma'].data_ptr(), f['dbeta'].data_ptr(), f['dbias'].data_ptr(), f['coef'].data_ptr(), _st()), 'bn_bwd_finalize_tiles')
    torch.cuda.synchronize()
    assert _gaps_alive(fF, f)
    got = dict(dgamma=f['dgamma'], dbeta=f['dbeta'], dbias=f['dbias'], k1=f['coef'][:c], k2=f['coef'][c:2 * c], k3=f['coef'][2 * c:])
    for k in got:
        sk.check('bn_bwd_finalize_tiles', case['id'], k, got[k], d['want'][k], d['bound'][k])


@pytest.mark.parametrize('case', sk.STATS_FINALIZE_CASES, ids=_ids(sk.STATS_FINALIZE_CASES))
def test_bn_stats_finalize(hip, case):
    d = sk.stats_finalize_data(case)
    c = case['c']
    want, bound, _ = sk.stats_finalize_reference(d)
    o, oF = _outs(dict(save_mean=c, save_rstd=c, scale=c, shift=c, moving_mean=c, moving_var=c))
    o['moving_mean'].copy_(d['moving_mean'])
    o['moving_var'].copy_(d['moving_var'])
    before = oF.clone()
    st, g, b = d['stats'].cuda(), d['gamma'].cuda(), d['beta'].cuda()
    mm, mv = (o['moving_mean'].data_ptr(), o['moving_var'].data_ptr()) if case['moving'] else (None, None)
    hip.check(hip.lib.y3_bn_stats_finalize(st.data_ptr(), case['tiles'], c, d['count'], g.data_ptr(), b.data_ptr(), sk.EPS, sk.MOM, mm, mv, o['save_mean'].data_ptr(),
                                           o['save_rstd'].data_ptr(), o['scale'].data_ptr(), o['shift'].data_ptr(), _st()), 'bn_stats_finalize')
    torch.cuda.synchronize()
    assert _gaps_alive(oF, o)
    if not case['moving']:
        assert torch.equal(o['moving_mean'], before[o['moving_mean'].storage_offset():][:c]) and 'moving_mean' not in want
    for k in want:
        sk.check('bn_stats_finalize', case['id'], k, o[k], want[k], bound[k])


@pytest.mark.parametrize('case', sk.BN_APPLY_CASES, ids=_ids(sk.BN_APPLY_CASES))
def test_bn_apply(hip, case):
    d = sk.bn_apply_data(case)
    M, c = case['M'], case['c']
    want, bound = sk.bn_apply_reference(d)
    aF, aV, a_ld = _buf(M, c, case['pad'][0], case['off'][0], src=d['a'])
    yF, yV, y_ld = _buf(M, c, case['pad'][1], case['off'][1])
    R = None
    if case['resid']:
        rF, rV, r_ld = _buf(M, c, case['pad'][2], case['off'][2], src=d['resid'])
        R = hip.Tensor(rV.data_ptr(), 1, 1, M, c, r_ld)
    sc, sh = d['scale'].cuda(), d['shift'].cuda()
    hip.check(hip.lib.y3_bn_apply(hip.Tensor(aV.data_ptr(), 1, 1, M, c, a_ld), sc.data_ptr(), sh.data_ptr(), R, hip.Tensor(yV.data_ptr(), 1, 1, M, c, y_ld), _st()), 'bn_apply')
    torch.cuda.synchronize()
    assert _canaries_alive(yF, yV)
    sk.check('bn_apply', case['id'], 'y', yV, want, bound)


def test_bn_fold_inference_batched(hip):
    f = sk.fold_data()
    params, moving, table = f['params'].cuda(), f['moving'].cuda(), f['table'].cuda()
    chan = torch.full((f['chan_len'],), NAN, device='cuda')
    hip.check(hip.lib.y3_bn_fold_inference_batched(params.data_ptr(), moving.data_ptr(), chan.data_ptr(), table.data_ptr(), len(sk.FOLD_LAYERS), sk.EPS, _st()))
    torch.cuda.synchronize()
    assert int(torch.isnan(chan).sum()) == f['chan_len'] - 2 * sum(sk.FOLD_LAYERS), 'wrote between the segments (or left a NaN inside one)'
    for r in f['table'].tolist():
        C = r[6]
        o, oF = _outs(dict(scale=C, shift=C))
        hip.check(hip.lib.y3_bn_fold_inference(params.data_ptr() + 4 * r[0], params.data_ptr() + 4 * r[1], moving.data_ptr() + 4 * r[2], moving.data_ptr() + 4 * r[3],
                                               sk.EPS, C, o['scale'].data_ptr(), o['shift'].data_ptr(), _st()))
        torch.cuda.synchronize()
        assert _gaps_alive(oF, o)
        assert torch.equal(chan[r[4]:r[4] + C].view(torch.int32), o['scale'].view(torch.int32)) and torch.equal(chan[r[5]:r[5] + C].view(torch.int32), o['shift'].view(torch.int32))
        want, bound = sk.fold_reference(f['params'][r[0]:r[0] + C], f['params'][r[1]:r[1] + C], f['moving'][r[2]:r[2] + C], f['moving'][r[3]:r[3] + C])
        for k in want:
            sk.check('bn_fold_inference', 'C%d' % C, k, o[k], want[k], bound[k])


@pytest.mark.parametrize('case', sk.UPSAMPLE_CASES, ids=_ids(sk.UPSAMPLE_CASES))
def test_upsample_fp32(hip, case):
    n, h, w, ci, co = case['n'], case['h'], case['w'], case['cin'], case['cout']
    x, dout = sk.upsample_data(case)
    npix = n * h * w
    xF, xV, x_ld = _buf(npix, ci, 4, 4, src=x)
    oF, oV, o_ld = _buf(4 * npix, co, case['pad'], case['off'])
    X, O = hip.Tensor(xV.data_ptr(), n, h, w, ci, x_ld), hip.Tensor(oV.data_ptr(), n, 2 * h, 2 * w, co, o_ld)
    hip.check(hip.lib.y3_upsample_sum2x_fwd(X, O, _st()), 'upsample_fwd')
    torch.cuda.synchronize()
    assert _canaries_alive(oF, oV)
    want, bound = sk.upsample_fwd_reference(x, co)
    sk.check('upsample_sum2x_fwd', case['id'], 'y', oV, want.reshape(-1, co), bound.reshape(-1, co))
    oV.copy_(dout.reshape(-1, co))
    dF, dV, d_ld = _buf(npix, ci, 4, 4)
    hip.check(hip.lib.y3_upsample_sum2x_bwd(O, hip.Tensor(dV.data_ptr(), n, h, w, ci, d_ld), _st()), 'upsample_bwd')
    torch.cuda.synchronize()
    assert _canaries_alive(dF, dV) and _canaries_alive(oF, oV)
    want, bound = sk.upsample_bwd_reference(dout, ci)
    sk.check('upsample_sum2x_bwd', case['id'], 'dx', dV, want.reshape(-1, ci), bound.reshape(-1, ci))


@pytest.mark.parametrize('case', sk.UPSAMPLE_BF16_CASES, ids=_ids(sk.UPSAMPLE_BF16_CASES))
def test_upsample_bf16(hip, case):
    n, h, w, ci, co = case['n'], case['h'], case['w'], case['cin'], case['cout']
    x, _ = sk.upsample_data(case, bf16=True)
    npix = n * h * w
    xF, xV, x_ld = _buf(npix, ci, 3, 1, dtype=torch.bfloat16, src=x)
    oF, oV, o_ld = _buf(4 * npix, co, case['pad'], case['off'], dtype=torch.bfloat16)
    hip.check(hip.lib.y3_upsample_sum2x_fwd_bf16(hip.Tensor(xV.data_ptr(), n, h, w, ci, x_ld), hip.Tensor(oV.data_ptr(), n, 2 * h, 2 * w, co, o_ld), _st()), 'upsample_bf16')
    torch.cuda.synchronize()
    assert _canaries_alive(oF, oV)
    want, bound = sk.upsample_fwd_reference(x, co, bf16=True)
    sk.check('upsample_sum2x_fwd_bf16', case['id'], 'y', oV.float(), want.reshape(-1, co), bound.reshape(-1, co))


@pytest.mark.parametrize('case', sk.COPY_CASES, ids=_ids(sk.COPY_CASES))
def test_copy_and_add_inplace_are_exact(hip, case):
    M, c = case['M'], case['c']
    g = np.random.default_rng(sk.seed_of('cp' + case['id']))
    src = torch.from_numpy((g.standard_normal((M, c)) * 10.0 ** g.uniform(-3, 3, c)).astype(np.float32))
    r0 = torch.from_numpy(g.standard_normal((M, c)).astype(np.float32)).cuda()
    sF, sV, s_ld = _buf(M, c, case['spad'], 4, src=src)
    dF, dV, d_ld = _buf(M, c, case['dpad'], 8)
    S, D = hip.Tensor(sV.data_ptr(), 1, 1, M, c, s_ld), hip.Tensor(dV.data_ptr(), 1, 1, M, c, d_ld)
    hip.check(hip.lib.y3_copy(S, D, _st()), 'copy')
    torch.cuda.synchronize()
    assert torch.equal(dV.view(torch.int32), sV.view(torch.int32)) and _canaries_alive(dF, dV)
    dV.copy_(r0)
    hip.check(hip.lib.y3_add_inplace(S, D, _st()), 'add_inplace')
    torch.cuda.synchronize()
    assert torch.equal(dV, r0 + sV) and _canaries_alive(dF, dV) and _canaries_alive(sF, sV)


@pytest.mark.parametrize('case', sk.LAYOUT_CASES, ids=_ids(sk.LAYOUT_CASES))
def test_layout_changes_are_exact(hip, case):
    n, c, h, w, dc, ld = (case[k] for k in ('n', 'c', 'h', 'w', 'dc', 'ld'))
    g = torch.Generator().manual_seed(sk.seed_of(case['id']))
    x = torch.randn(n, c, h, w, generator=g).cuda()
    npix = n * h * w
    dF, dV, _ = _buf(npix, dc, ld - dc, 4)
    hip.check(hip.lib.y3_nchw_to_nhwc(x.data_ptr(), n, c, h, w, hip.Tensor(dV.data_ptr(), n, h, w, dc, ld), _st()), 'nchw_to_nhwc')
    torch.cuda.synchronize()
    assert _canaries_alive(dF, dV)
    assert torch.equal(dV[:, :c].reshape(n, h, w, c), x.permute(0, 2, 3, 1)) and bool((dV[:, c:] == 0).all())
    for cc in (dc, c):       # the whole padded pixel, and the first c channels of it (ld > c)
        back = torch.full((n * cc * h * w + 8,), NAN, device='cuda')
        hip.check(hip.lib.y3_nhwc_to_nchw(hip.Tensor(dV.data_ptr(), n, h, w, cc, ld), back.data_ptr(), _st()), 'nhwc_to_nchw')
        torch.cuda.synchronize()
        assert bool(torch.isnan(back[-8:]).all())
        b = back[:-8].view(n, cc, h, w)
        assert torch.equal(b[:, :c], x) and bool((b[:, c:] == 0).all())


@pytest.mark.parametrize('count', sk.FILL_COUNTS)
def test_fill_is_exact(hip, count):
    f = torch.full((count + 12,), NAN, device='cuda')
    hip.check(hip.lib.y3_fill(f.data_ptr() + 16, count, -2.5, _st()), 'fill')
    torch.cuda.synchronize()
    assert bool((f[4:4 + count] == -2.5).all()) and int(torch.isnan(f).sum()) == 12


@pytest.mark.parametrize('case', sk.COLSUM_CASES, ids=_ids(sk.COLSUM_CASES))
def test_colsum(hip, case):
    M, c, ld = case['M'], case['c'], case['ld']
    x = sk.colsum_data(case)
    xF, xV, _ = _buf(M, c, ld - c, 4, src=x)
    o, oF = _outs(dict(sum=c))
    hip.check(hip.lib.y3_colsum(hip.Tensor(xV.data_ptr(), 1, 1, M, c, ld), o['sum'].data_ptr(), _st()), 'colsum')
    torch.cuda.synchronize()
    assert _gaps_alive(oF, o)
    want, bound = sk.colsum_reference(x)
    sk.check('colsum', case['id'], 'sum', o['sum'], want, bound)


def _zscore(hip, x):
    n, count = x.shape
    xd = x.cuda().contiguous()
    out = torch.full((n * count + 8,), NAN, device='cuda')
    wb = int(hip.lib.y3_zscore_workspace_bytes(n))
    ws = torch.full((wb + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    hip.check(hip.lib.y3_zscore(xd.data_ptr(), out.data_ptr(), n, count, ws.data_ptr(), _st()), 'zscore')
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[-8:]).all()) and bool((ws[wb:] == 0xA5).all())
    return out[:-8].view(n, count)


@pytest.mark.parametrize('count', (sk.ZSCORE_BRANCH_COUNT,) + sk.ZSCORE_COUNTS)
def test_zscore(hip, count):
    """the images of one launch take different branches; the subtract-only branch is exact"""
    x = sk.zscore_branch_images() if count == sk.ZSCORE_BRANCH_COUNT else sk.zscore_count_images(count)
    want, bound, divide, sd, exact = sk.zscore_reference(x)
    got = _zscore(hip, x).cpu()
    assert torch.equal(got[~divide].view(torch.int32), exact[~divide].view(torch.int32)), 'subtract-only branch'
    sk.check('zscore', 'n%d' % count, 'out', got, want, bound)
    if count == sk.ZSCORE_BRANCH_COUNT:
        assert torch.equal(got[1], x[1]) and bool((got[0] == 0).all())
        assert torch.equal(got[2], x[1]), 'the checkerboard x 4 divided by its sd of exactly 4'


def test_f32_to_bf16_is_round_to_nearest_even_at_every_edge(hip):
    bits = np.array([b for b, _ in sk.BF16_TABLE], np.uint32)
    want, nan = sk.bf16_bits_rne(bits)
    src = torch.from_numpy(bits.view(np.float32).copy()).cuda()
    dst = torch.full((len(bits) + 8,), NAN, dtype=torch.bfloat16, device='cuda')
    hip.check(hip.lib.y3_f32_to_bf16(src.data_ptr(), dst.data_ptr(), len(bits), _st()), 'f32_to_bf16')
    torch.cuda.synchronize()
    got = dst[:len(bits)].view(torch.int16).cpu().numpy().view(np.uint16)
    bad = [(hex(int(b)), why, hex(int(g)), hex(int(w_))) for (b, why), g, w_, isn in zip(sk.BF16_TABLE, got, want, nan) if not isn and g != w_]
    assert not bad, bad
    assert bool(torch.isnan(dst[:len(bits)].float().cpu()[torch.from_numpy(nan)]).all()), 'NaN must stay NaN'
    assert bool(torch.isnan(dst[len(bits):].float()).all())
    x = sk.f32_to_bf16_random()
    dst = torch.full((x.numel() + 8,), NAN, dtype=torch.bfloat16, device='cuda')
    hip.check(hip.lib.y3_f32_to_bf16(x.cuda().data_ptr(), dst.data_ptr(), x.numel(), _st()), 'f32_to_bf16')
    torch.cuda.synchronize()
    assert torch.equal(dst[:-8].cpu().view(torch.int16), x.to(torch.bfloat16).view(torch.int16)) and bool(torch.isnan(dst[-8:].float()).all())


def test_refused_shapes_return_an_error_and_launch_nothing(hip):
    d = sk.bnb_case(sk.BNB_CASES[0])
    o, oF = _bnb_outs(1056)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')

    def refused(rc, word):
        msg = hip.lib.y3_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)
        torch.cuda.synchronize()
        assert bool(torch.isnan(oF).all()) and int(ws.sum()) == 0, 'something was launched'

    for c in sk.BNB_REFUSED_C:
        assert int(hip.lib.y3_bn_bwd_workspace(64, c)) == 0
        flat = torch.zeros(64 * c, device='cuda')
        T = hip.Tensor(flat.data_ptr(), 1, 1, 64, c, c)
        dd = dict(gamma=torch.ones(c), mean=torch.zeros(c), rstd=torch.ones(c))
        refused(_bnb_launch(hip, T, T, None, 0, dd, o, ws, ws.numel()), '4 / 8 / 16, or a multiple of 32 up to 1024')
    c, M = 32, 64
    flat = torch.zeros(M * (c + 4) + 8, device='cuda')
    dd = dict(gamma=torch.ones(c), mean=torch.zeros(c), rstd=torch.ones(c))
    good = hip.Tensor(flat.data_ptr(), 1, 1, M, c, c)
    need = int(hip.lib.y3_bn_bwd_workspace(M, c))
    refused(_bnb_launch(hip, good, good, None, 0, dd, o, ws, need - 1), 'workspace')
    refused(_bnb_launch(hip, good, good, None, 0, dd, o, ws[4:], need), 'workspace')                       # workspace not 16-byte aligned
    for bad in (hip.Tensor(flat.data_ptr() + 4, 1, 1, M, c, c), hip.Tensor(flat.data_ptr(), 1, 1, M, c, c + 2), hip.Tensor(flat.data_ptr(), 1, 1, M, c - 2, c)):
        refused(_bnb_launch(hip, bad, good, None, 0, dd, o, ws, need), 'alignment')
        refused(_bnb_launch(hip, good, good, bad, 0, dd, o, ws, need), 'alignment')
        y = hip.Tensor(flat.data_ptr(), 1, 1, M, bad.c, bad.ld) if bad.c != c else good
        assert hip.lib.y3_copy(bad, y, _st()) == -1 and hip.lib.y3_upsample_sum2x_fwd(bad, good, _st()) == -1
        assert hip.lib.y3_bn_apply(bad, o['dgamma'].data_ptr(), o['dbeta'].data_ptr(), None, y, _st()) == -1
    assert hip.lib.y3_bn_stats_finalize(flat.data_ptr(), 1, 6, 4, flat.data_ptr(), flat.data_ptr(), sk.EPS, sk.MOM, None, None, o['dgamma'].data_ptr(), o['dbeta'].data_ptr(),
                                        o['dbias'].data_ptr(), o['coef'].data_ptr(), _st()) == -1
    assert hip.lib.y3_bn_stats_finalize(flat.data_ptr(), 1, 8, 4, flat.data_ptr(), flat.data_ptr(), sk.EPS, sk.MOM, flat.data_ptr(), None, o['dgamma'].data_ptr(),
                                        o['dbeta'].data_ptr(), o['dbias'].data_ptr(), o['coef'].data_ptr(), _st()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(oF).all()) and float(flat.abs().sum()) == 0
