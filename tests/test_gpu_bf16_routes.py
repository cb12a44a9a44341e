"""y3_conv2d_fwd_bf16_ws on every kernel route of the inference plan, against fp64.

describe_bf16 (csrc/conv_bf16.hip) picks one of nine launch routes per call (tests/bf16_routes.py says how, and which launches of the network
fall into which class).  This file runs

* the cheapest real layer of every class (test_route: id = class + layer shape), with the epilogue the model passes -- bias,
  leaky-relu 0.2 and the folded BatchNorm scale / shift for conv layers, linear fp32 for heads, the residual where the layer has one;
* the two patch instantiations no layer of the network launches (bf16_routes.extra_members), the same way;
* small shapes that enter the epilogue and fallback branches no layer of the network enters (test_variant): element-by-element
  stores for rows that are not 16-byte aligned, a ragged last 8-channel group, a linear epilogue, no scale / shift, no bias, alpha
  outside [0, 1], no workspace or one a byte too short;
* the largest launch under the 2 GiB limit on both of its routes, and the refusal one tile above it.

Every case asks y3_conv2d_fwd_bf16_plan, with the very arguments of the launch, which kernel it takes, and asserts that this is the
route its name says.  Operands: inputs, residual and weights rounded to bf16 (the weights through y3_transpose_weights +
y3_f32_to_bf16), so products are exact in fp32 and only the order of fp32 accumulation and one rounding on store differ from
the reference; every pitch and pad holds NaN.  Bounds (none is new: test_gpu_kernels.test_conv_fwd_bf16 and the race tests):

    bf16 output   |got - ref| <= |ref| * 2^-8 + 2e-5 * max|ref|      (half a bf16 ulp is up to 2^-8 of the value; + accumulation order)
    fp32 output   |got - ref| <= 2e-5 * max|ref|

against an fp64 convolution of the same operands for up to four images of the batch (first, adjacent middle pair, last), and for
the WHOLE batch, where it is larger, |ref| * 2^-8 + 2e-5 * max|ref| against y3_conv2d_fwd (the fp32 MFMA kernel, itself held to
fp64 by test_gpu_plan_forms.py) on the same operands plus the residual, so that no image of a 45-tile launch goes unchecked.

With Y3_BF16_ROUTES_PROFILE=<file> one JSON line per case is written there (profiles/bf16_routes.txt is such a run); no tolerance
here is derived from those figures."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import bf16_routes as br
from test_gpu_kernels import _conv_ref, hip      # noqa: F401  (hip: the module fixture)

OFFSET = 0.5             # of the normal under the leaky-relu that makes inputs and residuals (a zero-mean input hides a wrong border tap)
HDR = 256 * 1024 // 4    # floats of ticket header in front of the split-K slabs
BF16_REL, TOL = 2.0 ** -8, 2e-5
REF_CHUNK_BYTES = 1 << 30    # the fp32 kernel that checks a whole batch runs on this much input or output at a time

REPS, LEFT_OUT = br.representatives()
EXTRA = br.extra_members()
ROWS = []


@pytest.fixture(scope='module', autouse=True)
def _profile():
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    yield
    torch.set_num_threads(threads)
    path = os.environ.get('Y3_BF16_ROUTES_PROFILE')
    if path and ROWS:
        with open(path, 'w') as f:
            f.write('# tests/test_gpu_bf16_routes.py: one line per case; plan = y3_conv2d_fwd_bf16_plan of the launch; worst_err / ratio against fp64 on\n'
                    '# the checked images (ratio = worst error / bound, 1.0 = at the bound: a bf16 output just above a power of two that is rounded half an ulp\n'
                    '# sits at 0.98), not_nearest: share of bf16 outputs that are not the nearest bf16 of the fp64 value; batch_ratio: the whole batch\n'
                    '# against the fp32 MFMA kernel\n')
            for row in ROWS:
                f.write(json.dumps(row) + '\n')


def _act(shape, g, dtype=torch.bfloat16):
    return F.leaky_relu(torch.randn(shape, generator=g, device='cuda') + OFFSET, 0.1).to(dtype)


def _strided(buf, n, h, w, c, ld, off):
    return torch.as_strided(buf, (n, h, w, c), (h * w * ld, w * ld, ld, 1), off)


def _nan_buf(n, h, w, ld, off, dtype):
    return torch.full((n * h * w * ld + off + 8,), float('nan'), dtype=dtype, device='cuda')


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _excess(got, ref, out_f32, scale=None):
    """(worst |got - ref|, worst error / bound) under the bound of the output type; got must be finite"""
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), 'non-finite output'
    scale = float(ref.abs().max()) if scale is None else scale
    bound = TOL * max(scale, 1e-30) + (0.0 if out_f32 else BF16_REL) * ref.abs()
    err = (got - ref).abs()
    return float(err.max()), float((err / bound).max())


class Case(object):
    """One launch: geometry, epilogue, pitches and pointer offsets (in elements), how it is given a workspace."""

    def __init__(self, name, shape, resid=False, out_f32=False, flags=None, alpha=br.LRELU_ALPHA, affine=True, bias=True, src_ld=None, dst_ld=None,
                 resid_ld=None, dst_off=0, resid_off=0, ws='query', expect=None, subset=None, whole_batch=True, seed=0):
        self.name, self.shape, self.resid, self.out_f32, self.flags, self.alpha, self.affine, self.bias = name, shape, resid, out_f32, flags, alpha, affine, bias
        n, h, w, cin, cout, k, s = shape
        self.src_ld = src_ld or cin + 8
        self.dst_ld = dst_ld or ((cout + 3) // 4 * 4 + 4 if out_f32 else (cout + 7) // 8 * 8 + 8)
        self.resid_ld = resid_ld or cout
        self.dst_off, self.resid_off, self.ws, self.expect, self.subset, self.whole_batch, self.seed = dst_off, resid_off, ws, expect, subset, whole_batch, seed


def _member_case(mb):
    """a Member of the envelope as a Case: the model's pitches where a concat buffer gives one, else 16 bytes of NaN pad per row"""
    n, h, w, cin, cout, k, s = mb.shape()
    return Case(mb.id(), mb.shape(), resid=mb.resid, out_f32=mb.out_f32, flags=mb.flags, alpha=mb.alpha, affine=not mb.head,
                src_ld=mb.src_ld if mb.src_ld != cin else None, dst_ld=mb.dst_ld if mb.dst_ld != cout and not mb.head else None,
                subset=mb.subset(), seed=sum(v * p for v, p in zip(mb.shape(), (7, 11, 13, 17, 19, 23, 29))))


def host_plan(c):
    """the query for a Case with made-up pointers of the case's alignment: what test_cpu_bf16_routes.py checks the table below with"""
    hip = br._lib()
    n, h, w, cin, cout, k, s = c.shape
    need = int(hip.lib.y3_conv2d_fwd_bf16_workspace(n * -(-h // s) * -(-w // s), cin, k, cout))
    eb = 4 if c.out_f32 else 2
    return br.plan(n, h, w, cin, cout, k, s, resid=c.resid, out_f32=c.out_f32, flags=hip.EPI_LRELU if c.flags is None else c.flags, alpha=c.alpha,
                   affine=c.affine, bias=c.bias, src_ld=c.src_ld, dst_ld=c.dst_ld, resid_ld=c.resid_ld, dst_ptr=br.FAKE + eb * c.dst_off,
                   resid_ptr=br.FAKE + 2 * c.resid_off, ws_bytes={'query': need, 'none': 0, 'short': need - 1, 'plain': 0}[c.ws])


def variant_case(name, shape, kw):
    return Case(name, shape, seed=len(name) + sum(shape), **kw)


def _run(hip, c):
    """Launch the case (twice on one workspace), check it as the module docstring says; returns (plan, bytes of workspace used)."""
    from util import stream
    n, h, w, cin, cout, k, s = c.shape
    oh, ow, m = -(-h // s), -(-w // s), n * (-(-h // s)) * (-(-w // s))
    flags = hip.EPI_LRELU if c.flags is None else c.flags
    g = torch.Generator(device='cuda').manual_seed(1000 + c.seed)
    # operands on the device; the reference reads back what the kernel is given
    sbuf = _nan_buf(n, h, w, c.src_ld, 8, torch.bfloat16)
    sv = _strided(sbuf, n, h, w, cin, c.src_ld, 8)
    for i in range(n):
        sv[i].copy_(_act((h, w, cin), g))
    wk = (torch.randn(k, k, cin, cout, generator=g, device='cuda') * 0.1).to(torch.bfloat16)
    wf = wk.float().contiguous()
    wt = torch.empty(k * k * cout * cin, device='cuda')
    hip.check(hip.lib.y3_transpose_weights(wf.data_ptr(), wt.data_ptr(), k * k, cin, cout, stream()))
    wtb = torch.empty(k * k * cout * cin, dtype=torch.bfloat16, device='cuda')
    hip.check(hip.lib.y3_f32_to_bf16(wt.data_ptr(), wtb.data_ptr(), wt.numel(), stream()))
    assert torch.equal(wtb.view(k, k, cout, cin), wk.permute(0, 1, 3, 2))
    b = torch.randn(cout, generator=g, device='cuda') if c.bias else None
    sc = torch.rand(cout, generator=g, device='cuda') + 0.5 if c.affine else None
    sh = torch.randn(cout, generator=g, device='cuda') if c.affine else None
    rv = None
    if c.resid:
        rbuf = _nan_buf(n, oh, ow, c.resid_ld, c.resid_off, torch.bfloat16)
        rv = _strided(rbuf, n, oh, ow, cout, c.resid_ld, c.resid_off)
        for i in range(n):
            rv[i].copy_(_act((oh, ow, cout), g))
    ddt = torch.float32 if c.out_f32 else torch.bfloat16
    dbuf = _nan_buf(n, oh, ow, c.dst_ld, c.dst_off, ddt)
    dv = _strided(dbuf, n, oh, ow, cout, c.dst_ld, c.dst_off)
    ptr = lambda t: None if t is None else t.data_ptr()
    need = int(hip.lib.y3_conv2d_fwd_bf16_workspace(m, cin, k, cout))
    wsb = {'query': need, 'none': 0, 'short': need - 1, 'plain': 0}[c.ws]
    assert c.ws not in ('short',) or need > HDR * 4
    ws = torch.zeros(max(need, 16) // 4 + 4, device='cuda')
    ws[HDR:].fill_(float('nan'))          # the contract: a zero ticket header; the slabs may hold anything
    args = (hip.Tensor(sv.data_ptr(), n, h, w, cin, c.src_ld), wtb.data_ptr(), ptr(b), k, s, hip.Tensor(dv.data_ptr(), n, oh, ow, cout, c.dst_ld),
            int(c.out_f32), flags, c.alpha, ptr(sc), ptr(sh), hip.Tensor(rv.data_ptr(), n, oh, ow, cout, c.resid_ld) if c.resid else None)
    wargs = (ws.data_ptr() if wsb else None, wsb)
    out = (br.C.c_int * 12)()
    used = int(hip.lib.y3_conv2d_fwd_bf16_plan(*(args + wargs + (out,))))
    p = list(out)
    plan = dict(zip(br.OUT_NAMES, p))
    assert p[0] != 0, hip.lib.y3_last_error()
    sig = br.signature(p, m, cout, c.out_f32)
    print('%s: plan %s, %d bytes of workspace' % (c.name, plan, used))
    if c.expect is not None:
        assert sig == c.expect, 'the launch is planned as %s, the case is for %s' % (br.sig_id(sig), br.sig_id(c.expect))
    # grid / splits describe a split launch exactly when workspace bytes are used
    tiles = -(-m // p[1]) * -(-cout // p[2])
    assert (used > 0) == (p[6] > 1) and used in (0, need) and (used == 0 or wsb >= need)
    if p[0] == hip.BF16_ROUTE_RING or p[0] == hip.BF16_ROUTE_PP:
        assert p[4] == tiles * p[6], (plan, tiles)
    outs = []
    for launch in range(2):
        dbuf.fill_(float('nan'))
        if c.ws == 'plain':
            hip.check(hip.lib.y3_conv2d_fwd_bf16(*(args + (stream(),))), 'conv2d_fwd_bf16')
        else:
            hip.check(hip.lib.y3_conv2d_fwd_bf16_ws(*(args + wargs + (stream(),))), 'conv2d_fwd_bf16_ws')
        torch.cuda.synchronize()
        assert int(ws[:HDR].view(torch.int32).abs().sum()) == 0, 'launch %d left a ticket behind' % launch
        outs.append(dbuf.clone())
    if not used:
        assert bool(torch.isnan(ws[HDR:]).all()), 'a launch that the query says does not split wrote to the workspace'
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), 'the second launch on the same workspace gives other bits'
    pads = outs[0].clone()
    _strided(pads, n, oh, ow, cout, c.dst_ld, c.dst_off).fill_(float('nan'))
    pads_ok = bool(torch.isnan(pads).all())
    del pads, outs
    # fp64 on the checked images
    subset = list(range(n)) if c.subset is None else c.subset
    idx = torch.tensor(subset, device='cuda')
    nchw = lambda t: t.index_select(0, idx).float().permute(0, 3, 1, 2).cpu()
    x64 = nchw(sv)
    ref = _conv_ref(x64, wk.float().cpu(), None if b is None else b.cpu(), k, s)
    if flags & hip.EPI_LRELU:
        ref = torch.where(ref > 0, ref, ref * float(torch.tensor(c.alpha, dtype=torch.float32)))
    if c.affine:
        ref = ref * sc.cpu().double()[None, :, None, None] + sh.cpu().double()[None, :, None, None]
    if c.resid:
        ref = ref + nchw(rv).double()
    got = nchw(dv)
    err, ratio = _excess(got, ref, c.out_f32)
    # reported, not asserted: the share of elements that are not the round-to-nearest of the fp64 value (accumulation order flips them)
    flips = None if c.out_f32 else float((got != ref.to(torch.float32).to(torch.bfloat16).float()).double().mean())
    row = {'id': c.name, 'route': br.sig_id(sig), 'plan': plan, 'ws_bytes': used, 'images': len(subset), 'worst_err': err, 'max_ref': float(ref.abs().max()), 'ratio': ratio}
    if flips is not None:
        row['not_nearest'] = flips
    del ref, x64, got
    # the whole batch against the fp32 MFMA kernel on the same operands (+ the residual)
    if n > len(subset) and c.whole_batch:
        fld = (cout + 3) // 4 * 4
        per = max(1, REF_CHUNK_BYTES // (4 * max(h * w * cin, oh * ow * fld)))
        y32 = torch.empty(n, oh, ow, fld, device='cuda')
        for i0 in range(0, n, per):
            i1 = min(n, i0 + per)
            x32 = sv[i0:i1].float().contiguous()
            fws_b = int(hip.lib.y3_conv2d_fwd_workspace((i1 - i0) * oh * ow, cin, k, cout))
            fws = torch.zeros(fws_b // 4 + 4, device='cuda')
            hip.check(hip.lib.y3_conv2d_fwd(hip.Tensor(x32.data_ptr(), i1 - i0, h, w, cin, cin), wf.data_ptr(), ptr(b), k, s,
                                            hip.Tensor(y32[i0:i1].data_ptr(), i1 - i0, oh, ow, cout, fld), flags & hip.EPI_LRELU, c.alpha, ptr(sc), ptr(sh), None, None,
                                            fws.data_ptr(), fws_b, stream()), 'conv2d_fwd (fp32 reference of the whole batch)')
            torch.cuda.synchronize()
            del x32, fws
        worst, scale = 0.0, float(y32[..., :cout].abs().max())
        for i in range(n):
            r_i = y32[i, ..., :cout].double() + (rv[i].double() if c.resid else 0.0)
            worst = max(worst, _excess(dv[i], r_i, False, scale=max(scale, float(r_i.abs().max())))[1])
        row['batch_ratio'] = worst
        del y32
    ROWS.append(row)
    print(json.dumps(row))
    assert ratio <= 1.0, '%s against fp64: %.3f of the bound (worst error %.3e)' % (c.name, ratio, err)
    assert row.get('batch_ratio', 0.0) <= 1.0, '%s, whole batch against the fp32 kernel: %.3f of the bound' % (c.name, row['batch_ratio'])
    assert pads_ok, 'pitch padding (or memory around the destination) overwritten'
    return p, used


@pytest.mark.gpu
@pytest.mark.parametrize('sig,mb', REPS + EXTRA, ids=[mb.id() for _, mb in REPS + EXTRA])
def test_route(hip, sig, mb):
    """One route class of y3_conv2d_fwd_bf16_ws (tests/bf16_routes.py) on a real layer of the network, against fp64."""
    assert not LEFT_OUT and mb.signature() == sig
    c = _member_case(mb)
    c.expect = sig
    p, used = _run(hip, c)
    assert (p, used) == mb.plan(), 'the launch with real pointers is planned differently from the envelope member: %s / %s' % (p, mb.plan()[0])


def _variants():
    """(name, shape, expected (route name, bm, bn, vec_ok, splits > 1), Case arguments); flags None = Y3_EPI_LRELU"""
    NP = 8       # Y3_BF16_NO_PATCH
    t64, t128, t256 = (2, 13, 13, 128, 256, 3, 1), (4, 128, 128, 32, 128, 1, 1), (4, 80, 80, 64, 256, 1, 1)
    c32, c64 = (2, 40, 45, 32, 64, 3, 1), (2, 40, 45, 64, 128, 3, 1)
    c32s2, c64s2 = (2, 67, 131, 32, 64, 3, 2), (2, 67, 131, 64, 128, 3, 2)
    out = []
    # rows that are not 16-byte aligned: vec_ok == 0, the element-by-element epilogue -- a pitch of cout + 2 elements, plain and with
    # the pointer one element (2 bytes) further; t256 is a ping-pong shape with aligned rows, c32 / c64 are patch shapes
    out.append(('aligned-pingpong', t256, ('pp', 256, 256, 1, False), dict()))
    for name, shape, tile in (('64x64', t64, (64, 64)), ('128x128', t128, (128, 128)), ('256x128', t256, (256, 128))):
        for resid in (False, True):
            for off in (0, 1):
                # (the 64 x 64 shape is split along K, so the reducing slice runs the element-by-element epilogue; novec-c64-shape is whole)
                out.append(('novec-%s%s%s' % (name, '-resid' if resid else '', '-offset' if off else ''), shape, ('ring',) + tile + (0, name == '64x64'),
                            dict(resid=resid, dst_ld=shape[4] + 2, dst_off=off)))
    out.append(('novec-resid-pitch-only', t128, ('ring', 128, 128, 0, False), dict(resid=True, resid_ld=t128[4] + 2)))
    out.append(('novec-resid-offset-only', t64, ('ring', 64, 64, 0, True), dict(resid=True, resid_ld=t64[4] + 2, resid_off=1)))
    out.append(('novec-c32-shape', c32, ('ring', 128, 64, 0, False), dict(resid=True, dst_ld=66)))
    out.append(('novec-c64-shape', c64, ('ring', 64, 64, 0, False), dict(resid=True, dst_ld=130, dst_off=1)))
    out.append(('novec-f32-out', (2, 20, 20, 64, 14, 1, 1), ('ring', 128, 32, 0, False), dict(out_f32=True, flags=0, affine=False, dst_ld=15)))
    # a ragged last 8-channel group with bf16 output and a residual (aligned rows: the other groups take the 16-byte path)
    out.append(('ragged-group-resid', (2, 20, 20, 64, 100, 1, 1), ('ring', 64, 64, 1, False), dict(resid=True, resid_ld=104)))
    out.append(('ragged-group-resid-128x128', (4, 128, 128, 32, 132, 1, 1), ('ring', 128, 128, 1, False), dict(resid=True, resid_ld=136)))
    # a linear epilogue, no scale / shift, no bias
    out.append(('linear-bf16', (2, 20, 20, 64, 128, 1, 1), ('ring', 64, 64, 1, False), dict(flags=0)))
    out.append(('linear-f32', (2, 20, 20, 64, 128, 1, 1), ('ring', 64, 64, 1, False), dict(flags=0, out_f32=True)))
    out.append(('linear-bf16-c32', c32, ('c32', 256, 64, 1, False), dict(flags=0, resid=True)))
    out.append(('no-affine-resid', (2, 20, 20, 64, 128, 1, 1), ('ring', 64, 64, 1, False), dict(affine=False, resid=True)))
    out.append(('no-affine-resid-pingpong', t256, ('pp', 256, 256, 1, False), dict(affine=False, resid=True)))
    out.append(('no-bias-ring', (2, 20, 20, 64, 128, 1, 1), ('ring', 64, 64, 1, False), dict(bias=False)))
    out.append(('no-bias-c32', c32, ('c32', 256, 64, 1, False), dict(bias=False)))
    out.append(('no-bias-c64', c64s2, ('c64', 64, 128, 1, False), dict(bias=False)))
    # alpha outside [0, 1] keeps a launch off the patch kernels (their leaky-relu is max(v, alpha v)); 0.2 takes them
    for name, shape, patch, ring in (('c32', c32, ('c32', 256, 64), (128, 64)), ('c64', c64, ('c64', 128, 128), (64, 64)),
                                     ('c32s2', c32s2, ('c32', 128, 64), (128, 64)), ('c64s2', c64s2, ('c64', 64, 128), (64, 64))):
        res = name in ('c32', 'c64')
        out.append(('alpha0.2-%s' % name, shape, patch + (1, False), dict(resid=res)))
        if name in ('c32', 'c64'):
            out.append(('alpha1.5-%s' % name, shape, ('ring',) + ring + (1, False), dict(resid=res, alpha=1.5)))
            out.append(('alpha-0.1-%s' % name, shape, ('ring',) + ring + (1, False), dict(resid=res, alpha=-0.1)))
    out.append(('no-patch-flag-c32', c32, ('ring', 128, 64, 1, False), dict(resid=True, flags=1 | NP)))
    # a shape whose plan splits K: with the workspace, through the entry without one, with a workspace one byte short
    sk = (1, 16, 16, 1024, 512, 1, 1)
    out.append(('split-k', sk, ('ring', 64, 64, 1, True), dict()))
    out.append(('split-k-no-workspace-entry', sk, ('ring', 64, 64, 1, False), dict(ws='plain')))
    out.append(('split-k-null-workspace', sk, ('ring', 64, 64, 1, False), dict(ws='none')))
    out.append(('split-k-workspace-a-byte-short', sk, ('ring', 64, 64, 1, False), dict(ws='short', resid=True)))
    return out


VARIANTS = _variants()


@pytest.mark.gpu
@pytest.mark.parametrize('name,shape,expect,kw', VARIANTS, ids=[v[0] for v in VARIANTS])
def test_variant(hip, name, shape, expect, kw):
    """An epilogue or fallback branch of y3_conv2d_fwd_bf16(_ws) that no layer of the network enters, on a small shape with a full
    fp64 reference; the query must say that the launch takes the kernel, tile and epilogue path the case is named after."""
    assert hip.EPI_LRELU == 1 and hip.BF16_NO_PATCH == 8
    p, used = _run(hip, variant_case(name, shape, kw))
    route, bm, bn, vec_ok, split = expect
    assert (br.route_names()[p[0]], p[1], p[2], p[8], p[6] > 1) == (route, bm, bn, vec_ok, split), (name, dict(zip(br.OUT_NAMES, p)))


LIMIT_SHAPE = (608, 608, 32, 64, 3, 2)       # the 32 -> 64 stride-2 layer of 608^2 tiles


@pytest.mark.gpu
def test_refusal_above_2_gib(hip):
    """91 tiles of 608^2 into the 32 -> 64 stride-2 layer: a source of 2.15 GB.  Y3_EINVAL with the '2 GiB' message (byte offsets
    inside the kernels are 32-bit), from the query as well, and the destination is not touched."""
    from util import stream
    h, w, cin, cout, k, s = LIMIT_SHAPE
    n, oh, ow = 91, h // s, w // s
    assert n * h * w * cin * 2 > 2 ** 31
    src = torch.empty(n * h * w * cin, dtype=torch.bfloat16, device='cuda')
    dst = torch.full((n * oh * ow * cout,), float('nan'), dtype=torch.bfloat16, device='cuda')
    wtb = torch.zeros(k * k * cout * cin, dtype=torch.bfloat16, device='cuda')
    b = torch.zeros(cout, device='cuda')
    args = (hip.Tensor(src.data_ptr(), n, h, w, cin, cin), wtb.data_ptr(), b.data_ptr(), k, s, hip.Tensor(dst.data_ptr(), n, oh, ow, cout, cout), 0,
            hip.EPI_LRELU, 0.2, None, None, None)
    out = (br.C.c_int * 12)()
    assert int(hip.lib.y3_conv2d_fwd_bf16_plan(*(args + (None, 0, out)))) == 0 and list(out) == [0] * 12 and b'2 GiB' in hip.lib.y3_last_error()
    for flags in (hip.EPI_LRELU, hip.EPI_LRELU | hip.BF16_NO_PATCH):
        a = args[:7] + (flags,) + args[8:]
        assert hip.lib.y3_conv2d_fwd_bf16_ws(*(a + (None, 0, stream()))) == -1 and b'2 GiB' in hip.lib.y3_last_error()
        assert hip.lib.y3_conv2d_fwd_bf16(*(a + (stream(),))) == -1 and b'2 GiB' in hip.lib.y3_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()), 'a refused launch wrote to its destination'


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['patch', 'ring'])
def test_largest_launch_under_2_gib(hip, route):
    """The same layer at 90 tiles: a source of 2 129 264 640 bytes, under 2^31 - 1 by less than a tile, so 32-bit byte offsets come
    within a tile of the limit.  Once on the patch kernel and once, with Y3_BF16_NO_PATCH, on the ring kernel: images 0, 44, 45 and
    89 against fp64, all 90 against the fp32 kernel.  One launch pair per route (the two-launch reproducibility check)."""
    h, w, cin, cout, k, s = LIMIT_SHAPE
    n = 90
    assert 2 ** 31 - 1 - n * h * w * cin * 2 < h * w * cin * 2 and n * h * w * cin * 2 == 2129264640
    flags = hip.EPI_LRELU | (hip.BF16_NO_PATCH if route == 'ring' else 0)
    p, used = _run(hip, Case('limit-90-tiles-%s' % route, (n,) + LIMIT_SHAPE, flags=flags, src_ld=cin, dst_ld=cout, subset=[0, 44, 45, 89], seed=90))
    assert (br.route_names()[p[0]], p[1], p[2]) == (('c32', 128, 64) if route == 'patch' else ('ring', 128, 64))
