"""YOLOv3-SPP on the GPU: the pooling kernels bit for bit against the restatement of tests/spp_reference.py, their
gradient against fp64 autograd, the new 2048 -> 512 1x1 layer under every launch plan it gets, the model with spp=True against the
oracle network with the block, and the wiring of the option through graphs, multi-scale plans, accumulation and weight files.

* forward: exact (max does not round; -0 == +0), NaN exactly where the restatement has it, in two layouts: separate buffers with
  pitches beyond the channels and NaN canaries in the gaps, and the model's -- one 4C-wide buffer, source = slice 0;
* backward: integer data -> every sum exact -> bit-equal to fp64 autograd; normal data within the per-element bound of
  spp_reference.backward_bound (additions x 2^-24 x sum of absolute terms); two launches give the same bits; with
  Y3_SPP_PROFILE=<file> the worst error / bound ratio per case is written there (profiles/spp_err.txt is such a run);
* the new GEMM shape: one representative per plan signature of spp_reference.gemm_representatives(), run by the checks of
  test_gpu_plan_forms / test_gpu_grad_forms / test_gpu_bf16_routes themselves -- their data, references and tolerances;
* model: the rule of test_gpu_model (error <= 6 x the oracle's own fp32-vs-fp64 distance + its floors, imported)."""
import os

import numpy as np
import pytest
import torch

import spp_reference as sr
from test_gpu_kernels import hip      # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

LAYOUTS = ('separate', 'model')
RATIOS = {}


@pytest.fixture(scope='module', autouse=True)
def _profile():
    yield
    path = os.environ.get('Y3_SPP_PROFILE')
    if path and RATIOS:
        with open(path, 'w') as f:
            f.write('# y3_spp_bwd on normal data: worst |error| / bound per case (tests/test_gpu_spp.py; 1.0 = at the bound)\n')
            f.write('# bound per element: (terms + accumulate) x 2^-24 x (sum |terms| + |old|), tests/spp_reference.py\n')
            f.write('%-22s %-10s %12s %12s\n' % ('# case', 'layout', 'overwrite', 'accumulate'))
            for (cid, layout) in sorted(RATIOS):
                r = RATIOS[(cid, layout)]
                f.write('%-22s %-10s %12.4f %12.4f\n' % (cid, layout, r[0], r[1]))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _view(buf, n, h, w, c, ld, off):
    return torch.as_strided(buf, (n, h, w, c), (h * w * ld, w * ld, ld, 1), off)


def _tensor(hip, buf, n, h, w, c, ld, off):
    return hip.Tensor(buf.data_ptr() + buf.element_size() * off, n, h, w, c, ld)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_values(got, want):
    """bit-exact up to the sign of zero, NaN exactly where `want` has it"""
    got, want = got.float().cpu(), want.float()
    return bool(torch.equal(torch.isnan(got), torch.isnan(want))) and bool(((got == want) | torch.isnan(want)).all())


def _forward_buffers(case, layout, dtype):
    """(source buffer, ld, offset), (pooled buffer, ld, offset): NaN everywhere"""
    n, h, w, c = case
    nan = lambda numel: torch.full((numel,), float('nan'), dtype=dtype, device='cuda')
    if layout == 'model':
        buf = nan(n * h * w * 4 * c)
        return (buf, 4 * c, 0), (buf, 4 * c, c)
    sld, dld = c + sr.SRC_PAD, 3 * c + sr.DST_PAD
    return (nan(n * h * w * sld + 8), sld, 8), (nan(n * h * w * dld + 4), dld, 4)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', sr.KERNEL_CASES, ids=[sr.case_id(c) for c in sr.KERNEL_CASES])
def test_forward_kernel_is_exact(hip, case, dtype, layout):
    n, h, w, c = case
    fn = hip.lib.y3_spp_fwd if dtype == torch.float32 else hip.lib.y3_spp_fwd_bf16
    for kind in sr.DATA_KINDS:
        x = sr.make_input(case, kind).to(dtype)
        want = sr.spp_forward(x)
        (sbuf, sld, soff), (dbuf, dld, doff) = _forward_buffers(case, layout, dtype)
        sv, dv = _view(sbuf, n, h, w, c, sld, soff), _view(dbuf, n, h, w, 3 * c, dld, doff)
        sv.copy_(x)
        before = _bits(sbuf).clone()
        hip.check(fn(_tensor(hip, sbuf, n, h, w, c, sld, soff), _tensor(hip, dbuf, n, h, w, 3 * c, dld, doff), _st()), 'spp_fwd')
        torch.cuda.synchronize()
        assert _same_values(dv, want), (kind, 'values')
        assert torch.equal(_bits(sv), _bits(x.cuda())), (kind, 'the source changed')
        if kind == 'nan':
            assert int(torch.isnan(want).sum()) >= 3 * n and bool(torch.equal(torch.isnan(dv).cpu(), torch.isnan(want)))
        # everything but the pooled channels is what it was: canaries in the gaps, the source slice in the model's layout
        after = _bits(dbuf).clone()
        _view(after, n, h, w, 3 * c, dld, doff).zero_()
        ref = (before if layout == 'model' else _bits(torch.full_like(dbuf, float('nan')))).clone()
        _view(ref, n, h, w, 3 * c, dld, doff).zero_()
        assert torch.equal(after, ref), (kind, 'a byte outside the pooled channels changed')


def test_refused_planes_launch_nothing(hip):
    for n, h, w, c in sr.REFUSED_CASES:
        src = torch.zeros(n * h * w * c, device='cuda')
        dst = torch.full((n * h * w * 3 * c,), float('nan'), device='cuda')
        S, D = hip.Tensor(src.data_ptr(), n, h, w, c, c), hip.Tensor(dst.data_ptr(), n, h, w, 3 * c, 3 * c)
        assert hip.lib.y3_spp_fwd(S, D, _st()) == -1 and b'4096' in hip.lib.y3_last_error()
        assert hip.lib.y3_spp_bwd(S, D, S, 0, _st()) == -1
        torch.cuda.synchronize()
        assert bool(torch.isnan(dst).all()) and float(src.abs().sum()) == 0.0


def _backward_run(hip, case, layout, x, dd, old, accumulate):
    """y3_spp_bwd twice; returns dsrc of the first launch and checks repeatability and canaries"""
    n, h, w, c = case
    nan = lambda numel: torch.full((numel,), float('nan'), device='cuda')
    if layout == 'model':
        abuf, gbuf = nan(n * h * w * 4 * c), nan(n * h * w * 4 * c)
        S = (abuf, 4 * c, 0)
        DD, DS = (gbuf, 4 * c, c), (gbuf, 4 * c, 0)
    else:
        sld, dld, gld = c + sr.SRC_PAD, 3 * c + sr.DST_PAD, c + 12
        S, DD, DS = (nan(n * h * w * sld + 8), sld, 8), (nan(n * h * w * dld + 4), dld, 4), (nan(n * h * w * gld + 16), gld, 16)
    sv, ddv, dsv = _view(S[0], n, h, w, c, S[1], S[2]), _view(DD[0], n, h, w, 3 * c, DD[1], DD[2]), _view(DS[0], n, h, w, c, DS[1], DS[2])
    sv.copy_(x)
    ddv.copy_(dd)
    outs = []
    for launch in range(2):
        if accumulate:
            dsv.copy_(old)
        else:
            dsv.fill_(float('nan'))
        hip.check(hip.lib.y3_spp_bwd(_tensor(hip, S[0], n, h, w, c, S[1], S[2]), _tensor(hip, DD[0], n, h, w, 3 * c, DD[1], DD[2]),
                                     _tensor(hip, DS[0], n, h, w, c, DS[1], DS[2]), accumulate, _st()), 'spp_bwd')
        torch.cuda.synchronize()
        outs.append(dsv.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), 'two launches give other bits'
    assert torch.equal(_bits(sv), _bits(x.cuda())) and torch.equal(_bits(ddv), _bits(dd.cuda())), 'an input changed'
    rest = DS[0].clone()
    _view(rest, n, h, w, c, DS[1], DS[2]).fill_(float('nan'))
    if layout == 'model':
        _view(rest, n, h, w, 3 * c, DD[1], DD[2]).fill_(float('nan'))
    assert bool(torch.isnan(rest).all()), 'a canary changed'
    return outs[0].cpu()


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('case', sr.KERNEL_CASES, ids=[sr.case_id(c) for c in sr.KERNEL_CASES])
def test_backward_kernel(hip, case, layout):
    n, h, w, c = case
    g = torch.Generator().manual_seed(5 + sum(case))
    # integer data: every partial sum is an integer far below 2^24, so fp32 is exact
    x = sr.make_input(case, 'tied')
    dd = torch.randint(-3, 4, (n, h, w, 3 * c), generator=g).float()
    old = torch.randint(-5, 6, (n, h, w, c), generator=g).float()
    want, terms, _ = sr.spp_backward(x, dd)
    assert float(terms.sum()) == 3.0 * n * h * w * c
    for acc in (0, 1):
        got = _backward_run(hip, case, layout, x, dd, old, acc)
        ref = (want + old.double() if acc else want).float()
        assert torch.equal(got, ref), 'integer data, accumulate=%d: not the bits of fp64 autograd' % acc
    # normal data: the per-element bound
    x = sr.make_input(case, 'normal')
    dd = torch.randn(n, h, w, 3 * c, generator=g)
    old = torch.randn(n, h, w, c, generator=g)
    want, terms, mag = sr.spp_backward(x, dd)
    ratios = []
    for acc in (0, 1):
        got = _backward_run(hip, case, layout, x, dd, old, acc).double()
        assert bool(torch.isfinite(got).all())
        ref = want + old.double() if acc else want
        bound = sr.backward_bound(terms, mag, old if acc else None)
        err = (got - ref).abs()
        ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
        print('%s %s accumulate=%d: worst error / bound %.4f (most terms into one element: %d)' % (sr.case_id(case), layout, acc, ratio, int(terms.max())))
        ratios.append(ratio)
    RATIOS[(sr.case_id(case), layout)] = ratios
    assert max(ratios) <= 1.0, ratios


# ---- the 2048 -> 512 1x1 layer under every plan it gets --------------------------------------------------------------
_REPS = sr.gemm_representatives()


def _ids(entry, ident):
    return ['%s-n%d_g%d' % (ident(sig), mb.n, mb.h) for sig, mb in _REPS[entry]]


def _pf_id(sig):
    import plan_forms as pf
    return pf.sig_id(sig)


def _gf_id(sig):
    import grad_forms as gf
    return gf.sig_id(sig)


def _br_id(sig):
    import bf16_routes as br
    return br.sig_id(sig)


@pytest.mark.parametrize('sig,mb', _REPS['fwd'], ids=_ids('fwd', _pf_id))
def test_new_layer_forward(hip, sig, mb):
    import test_gpu_plan_forms as t
    t._forward(hip, sig, mb)


@pytest.mark.parametrize('sig,mb', _REPS['dgrad'], ids=_ids('dgrad', _pf_id))
def test_new_layer_data_gradient(hip, sig, mb):
    import test_gpu_plan_forms as t
    t._data_gradient(hip, sig, mb)


@pytest.mark.parametrize('sig,mb', _REPS['wgrad'], ids=_ids('wgrad', _gf_id))
def test_new_layer_kernel_gradient(hip, sig, mb):
    import test_gpu_grad_forms as t
    t._kernel_gradient(hip, sig, mb)


@pytest.mark.parametrize('sig,mb', _REPS['bf16'], ids=_ids('bf16', _br_id))
def test_new_layer_bf16_forward(hip, sig, mb):
    import test_gpu_bf16_routes as t
    assert mb.signature() == sig
    c = t._member_case(mb)
    c.expect = sig
    p, used = t._run(hip, c)
    assert (p, used) == mb.plan()


# ---- the model ---------------------------------------------------------------------------------------------------------
def _setup(img, n, seed, randomize_bn, **kw):
    from test_gpu_kernels import _labels
    from test_gpu_model import ANCHORS, K
    from yolo3.model import YoloV3
    params = sr.init_params(3, len(ANCHORS), K, seed=seed, randomize_bn=randomize_bn)
    if randomize_bn:      # as test_gpu_model._setup: keep the head logits O(1)
        for p in params:
            if 'gamma' not in p:
                p['W'] *= 0.02
    yolo = YoloV3(n, [img, img, 3], K, ANCHORS, learning_rate=1e-3, spp=True, **kw)
    yolo.set_weights(params)
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(n, 3, img, img, generator=g)
    gts = _labels(np.random.default_rng(seed), n, img, ANCHORS, K, per_image=3)
    return params, yolo, images, gts


def test_counts_of_the_model():
    params, yolo, _, _ = _setup(64, 1, 3, True)
    assert len(yolo.specs) == 76 and len(yolo.trainable_weights()) == 298
    assert sum(int(np.prod(w.shape)) for w in yolo.trainable_weights()) == 62839882
    for a, b in zip(params, yolo.get_weights()):
        for k in a:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('img,n', [(320, 1), (96, 3)])
def test_inference_matches_spp_oracle(img, n):
    from oracle import model as om
    from test_gpu_model import ANCHORS, K, _check
    params, yolo, images, _ = _setup(img, n, 7, True)
    out = yolo.predict(images.cuda()).cpu().numpy()
    refs = {}
    for dt in (torch.float32, torch.float64):
        net = sr.SppNet(params, 3, len(ANCHORS), K, dtype=dt)
        with torch.no_grad():
            fms = net.feature_maps(images.to(dt), training=False)
            refs[dt] = (om.decode(fms, (img, img, 3), ANCHORS, K).numpy(), [f.numpy() for f in fms])
    fm_gpu = [f.cpu().numpy() for f in yolo.feature_maps(images.cuda(), training=False)]
    for i in range(3):
        _check(fm_gpu[i], refs[torch.float32][1][i], refs[torch.float64][1][i], 'feature_map_%d' % (i + 1))
    _check(out[..., 4:], refs[torch.float32][0][..., 4:], refs[torch.float64][0][..., 4:], 'scores')
    b32, b64 = refs[torch.float32][0][..., :4], refs[torch.float64][0][..., :4]
    den = np.abs(b64) + 1.0
    _check(out[..., :4] / den, b32 / den, b64 / den, 'boxes', mult=10.0)
    # the block is in the graph: the plain network on the same remaining weights gives another coarsest map
    at = sr.spp_layer_index(om.layer_specs(3, len(ANCHORS), K))
    plain = om.Net(params[:at] + params[at + 1:], 3, len(ANCHORS), K, dtype=torch.float64)
    with torch.no_grad():
        other = plain.feature_maps(images.double(), training=False)[0].numpy()
    assert np.abs(other - refs[torch.float64][1][0]).max() > 1e-3 * np.abs(other).max()


def test_bf16_inference_matches_bf16_spp_oracle():
    """the yardstick of test_gpu_model.test_bf16_inference_matches_bf16_oracle: no farther from the emulation with the same rounding
    points than twice the emulation's own distance to the fp32 network"""
    from oracle import model as om
    from test_gpu_model import ANCHORS, K, _rel_l2
    img, n = 96, 3
    params, yolo, images, _ = _setup(img, n, 7, True)
    out16 = yolo.predict(images.cuda(), precision='bf16').cpu().numpy()
    fm16 = [f.cpu().numpy() for f in yolo.feature_maps(images.cuda(), precision='bf16')]
    net = sr.SppNet(params, 3, len(ANCHORS), K, dtype=torch.float32)
    with torch.no_grad():
        f32 = net.feature_maps(images, training=False)
        dec32 = om.decode(f32, (img, img, 3), ANCHORS, K).numpy()
        net.bf16 = True
        fe = net.feature_maps(images, training=False)
        dece = om.decode(fe, (img, img, 3), ANCHORS, K).numpy()
    assert np.isfinite(out16).all()
    for i in range(3):
        d_emul, d_prec = _rel_l2(fm16[i], fe[i].numpy()), _rel_l2(fe[i].numpy(), f32[i].numpy())
        print('fm%d  bf16-kernel vs bf16-oracle %.3e   bf16-oracle vs fp32-oracle %.3e' % (i + 1, d_emul, d_prec))
        assert d_emul <= 2.0 * d_prec + 1e-4 and d_prec < 0.05, (i, d_emul, d_prec)
    d_emul, d_prec = _rel_l2(out16, dece), _rel_l2(dece, dec32)
    assert d_emul <= 2.0 * d_prec + 1e-4 and d_emul <= 4e-2, (d_emul, d_prec)


_ORACLE_STEPS = {}


@pytest.mark.parametrize('img,n,arith', [(224, 2, 'x3'), (224, 2, 'f32'), (96, 4, 'x3')])
def test_train_step_matches_spp_oracle(img, n, arith):
    from oracle import model as om
    from test_gpu_model import ANCHORS, GRAD_FLOOR, GRAD_FLOOR_X3, K, _check
    from yolo3.model import Mean
    params, yolo, images, gts = _setup(img, n, 11, False, conv_arithmetic=arith)
    floor = GRAD_FLOOR_X3 if arith == 'x3' else GRAD_FLOOR
    res = _ORACLE_STEPS.get((img, n))
    if res is None:
        res = {}
        for dt in (torch.float32, torch.float64):
            net = sr.SppNet(params, 3, len(ANCHORS), K, dtype=dt, requires_grad=True)
            adam = om.AdamState(net.trainable(), 1e-3)
            step = om.train_step(net, adam, images.to(dt), [torch.from_numpy(g) for g in gts], (img, img, 3), ANCHORS, K, n)
            res[dt] = (step, [(q['mean'].numpy().copy(), q['var'].numpy().copy()) for q in net.p if 'mean' in q])
        _ORACLE_STEPS.clear()
        _ORACLE_STEPS[(img, n)] = res
    (r32, mov32), (r64, mov64) = res[torch.float32], res[torch.float64]
    assert len(r64['grads']) == 298
    mets = [Mean() for _ in range(5)]
    loss = yolo.train_step((images.cuda(), [torch.from_numpy(g).cuda() for g in gts], *mets))
    assert abs(float(loss) - r64['loss']) <= 6 * abs(r32['loss'] - r64['loss']) + 1e-5 * abs(r64['loss']), (float(loss), r64['loss'])
    np.testing.assert_allclose([m.result() for m in mets], [r64['loss']] + r64['parts'], rtol=1e-4)
    flat = []
    for sp, d in zip(yolo.specs, yolo.get_gradients()):
        flat += [d['W'], d['b']] + ([d['gamma'], d['beta']] if sp.bn else [])
    assert len(flat) == 298
    for i, (g, a, b) in enumerate(zip(flat, r32['grads'], r64['grads'])):
        a, b, g = a.numpy().astype(np.float64), b.numpy(), np.asarray(g, np.float64)
        nb = np.linalg.norm(b) + 1e-30
        noise, err = np.linalg.norm(a - b) / nb, np.linalg.norm(g - b) / nb
        assert np.isfinite(g).all() and err <= 6.0 * noise + floor, 'grad tensor %d: rel L2 err %.3e (oracle fp32 noise %.3e)' % (i, err, noise)
    mov = [(d['mean'], d['var']) for d in yolo.get_weights() if 'mean' in d]
    for i, ((m, v), (m32, v32), (m64, v64)) in enumerate(zip(mov, mov32, mov64)):
        _check(m, m32, m64, 'moving mean %d' % i, rel=1e-4)
        _check(v, v32, v64, 'moving var %d' % i, rel=1e-4)


# ---- wiring ----------------------------------------------------------------------------------------------------------
def _norm_arg(a):
    from yolo3 import _hip
    if isinstance(a, _hip.Tensor):
        return ('tensor', a.n, a.h, a.w, a.c, a.ld)
    if isinstance(a, bool) or a is None or isinstance(a, (float, str)):
        return a
    if isinstance(a, int):
        return 'address' if a >= (1 << 32) else a
    if isinstance(a, (tuple, list)):
        return tuple(_norm_arg(v) for v in a)
    if callable(a):
        return a.__name__
    return type(a).__name__


def _launches(plan):
    return [(_norm_arg(fn), _norm_arg(args)) for lst in (plan.fwd, plan.bwd) for fn, args in lst]


def test_spp_off_builds_the_launch_list_of_a_model_without_the_keyword():
    from test_gpu_model import ANCHORS, K
    from yolo3.model import YoloV3
    base = YoloV3(2, [64, 64, 3], K, ANCHORS)
    off = YoloV3(2, [64, 64, 3], K, ANCHORS, spp=False)
    on = YoloV3(2, [64, 64, 3], K, ANCHORS, spp=True)
    assert base.spp is False and base.arena_floats == off.arena_floats < on.arena_floats
    for training, bf16 in ((True, False), (False, False), (False, True)):
        a, b, c = (_launches(m._plan(2, training, bf16)) for m in (base, off, on))
        assert a == b and len(a) > (150 if training else 70)
        names = lambda l: [fn for fn, _ in l]
        assert not any('spp' in str(fn) for fn in names(a))
        assert sum('spp' in str(fn) for fn in names(c)) == (2 if training else 1)
        assert ('y3_spp_fwd_bf16' in names(c)) == bf16 and ('y3_spp_bwd' in names(c)) == training


def test_graph_captured_step_equals_the_eager_step():
    from test_gpu_model import ANCHORS, K
    from yolo3.model import YoloV3
    params, a, images, gts = _setup(64, 2, 13, True)
    b = YoloV3(2, [64, 64, 3], K, ANCHORS, learning_rate=1e-3, spp=True, use_graph=True)
    b.set_weights(params)
    gt_dev = [torch.from_numpy(g).cuda() for g in gts]
    for step in range(3):
        la, lb = float(a.train_step((images.cuda(), gt_dev))), float(b.train_step((images.cuda(), gt_dev)))
        torch.cuda.synchronize()
        assert la == lb and np.isfinite(la), step
        assert torch.equal(a.grads, b.grads) and torch.equal(a.params, b.params) and torch.equal(a.moving, b.moving), step
    for prec in ('fp32', 'bf16'):
        assert torch.equal(a.predict(images.cuda(), precision=prec), b.predict(images.cuda(), precision=prec)), prec


def test_tta_identity_view_is_predict():
    """predict_tta writes the views straight into the plan's input and runs the same plan: with the identity view alone its rows are
    predict's, bit for bit, in both precisions; with two views the first block of rows has predict's shape and finite values"""
    params, yolo, images, _ = _setup(96, 2, 7, True)
    dev = images.cuda()
    for prec in ('fp32', 'bf16'):
        rows = yolo.predict(dev, precision=prec).clone()
        assert torch.equal(yolo.predict_tta(dev, (0,), precision=prec), rows), prec
        two = yolo.predict_tta(dev, (0, 1), precision=prec)
        assert two.shape == (2, 2 * rows.shape[1], rows.shape[2]) and bool(torch.isfinite(two).all())


def test_plans_per_size_equal_a_chain_of_fixed_size_models(tmp_path):
    from test_gpu_model import ANCHORS, K
    from test_gpu_multiscale import STATE, _batch_at, _dev
    from yolo3.model import YoloV3
    n, kw = 2, dict(learning_rate=1e-3, spp=True)
    params = sr.init_params(3, len(ANCHORS), K, seed=11)
    batches = {s: _batch_at((s, s), n, 100 + s) for s in (96, 64)}
    a = YoloV3(n, [96, 96, 3], K, ANCHORS, train_sizes=[(64, 64), (96, 96)], **kw)
    a.set_weights(params)
    b = {s: YoloV3(n, [s, s, 3], K, ANCHORS, **kw) for s in (96, 64)}
    b[96].set_weights(params)
    path = os.path.join(str(tmp_path), 'hand.npz')
    prev = None
    for i, s in enumerate([96, 64, 96]):
        la = float(a.train_step(_dev(batches[s])))
        m = b[s]
        if prev is not None and prev is not m:
            prev.save_weights(path)
            m.load_weights(path, load_optimizer=True)
        lb = float(m.train_step(_dev(batches[s])))
        torch.cuda.synchronize()
        prev = m
        assert la == lb and np.isfinite(la), (i, s, la, lb)
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(prev, name)), name
    assert {k[4] for k in a._plans if k[1]} == {(96, 96), (64, 64)}


def test_accumulation_over_two_batches_is_restated_in_numpy():
    from test_gpu_grad_accum import F32, NORM_RTOL, STATE, _norm64, _np, _numpy_adam
    from test_gpu_model import ANCHORS, K
    from yolo3.model import YoloV3, clip_scale
    params, _, images, gts = _setup(96, 4, 7, False)
    y = YoloV3(2, [96, 96, 3], K, ANCHORS, learning_rate=1e-3, spp=True, accumulate_steps=2)
    y.set_weights(params)
    gt_dev = [torch.from_numpy(g).cuda() for g in gts]
    batch = lambda j: (images[2 * j:2 * j + 2].cuda(), [g[2 * j:2 * j + 2] for g in gt_dev])
    y.train_step(batch(0)), y.train_step(batch(1))
    torch.cuda.synchronize()
    assert y.iterations == 1 and y.micro_step == 0
    before = [_np(getattr(y, name)) for name in STATE]
    gs = []
    for j in (1, 0):
        y.train_step(batch(j))
        torch.cuda.synchronize()
        gs.append(_np(y.grads))
    assert y.iterations == 2 and not np.array_equal(gs[0], gs[1])
    a2 = (gs[0] + gs[1]).astype(np.float32)
    assert np.array_equal(_np(y.grad_acc), a2)
    n64 = _norm64(a2, 2)
    assert abs(float(y.last_grad_norm) - n64) <= NORM_RTOL * n64
    s = clip_scale(n64, None, 2)
    want = _numpy_adam(*before, a2, F32(y._lr_t()), s)
    for name, w in zip(STATE, want):
        assert np.array_equal(_np(getattr(y, name)), w), name
    new = y.specs[55]
    assert float(np.abs(a2[new.w_off:new.w_off + 2048 * 512]).sum()) > 0      # the new layer takes part


def test_weight_files(tmp_path, capsys):
    from oracle import model as om
    from test_gpu_model import ANCHORS, K
    from yolo3.model import YoloV3, spp_transfer_map
    params, yolo, images, gts = _setup(64, 2, 5, True)
    yolo.train_step((images.cuda(), [torch.from_numpy(g).cuda() for g in gts]))
    rows = yolo.predict(images.cuda()).clone()
    path = str(tmp_path / 'spp.npz')
    yolo.save_weights(path)
    back = YoloV3.from_file(path)
    assert back.spp is True and len(back.specs) == 76
    assert torch.equal(back.predict(images.cuda()), rows)
    # a plain model's file: from_file gives a plain model; loading it into the SPP model, or the SPP file into a plain one, raises
    plain = YoloV3(2, [64, 64, 3], K, ANCHORS)
    pparams = om.init_params(3, len(ANCHORS), K, seed=9, randomize_bn=True)
    for p in pparams:      # as _setup: keep the head logits O(1)
        if 'gamma' not in p:
            p['W'] *= 0.02
    plain.set_weights(pparams)
    ppath = str(tmp_path / 'plain.npz')
    plain.save_weights(ppath)
    assert 'meta_spp' not in np.load(ppath) and YoloV3.from_file(ppath).spp is False
    for m, p in ((yolo, ppath), (plain, path)):
        with pytest.raises(ValueError) as e:
            m.load_weights(p)
        assert 'spp=True' in str(e.value) and 'spp=False' in str(e.value)
    # transfer: every layer by role, the layer behind the pools keeps what it had, the optimiser state is not loaded
    mine = yolo.get_weights()
    yolo.adam_m.fill_(3.0)
    capsys.readouterr()
    yolo.load_weights(ppath, transfer=True)
    said = capsys.readouterr().out.strip().splitlines()
    assert len(said) == 1 and 'layer 55' in said[0] and '2048 -> 512' in said[0]
    got, src = yolo.get_weights(), plain.get_weights()
    for i, j in enumerate(spp_transfer_map(yolo.specs)):
        want = mine[i] if j is None else src[j]
        assert sorted(got[i]) == sorted(want)
        for k in want:
            assert np.array_equal(got[i][k], want[k]), (i, j, k)
    assert float(yolo.adam_m.min()) == 3.0 and bool(torch.isfinite(yolo.predict(images.cuda())).all())
