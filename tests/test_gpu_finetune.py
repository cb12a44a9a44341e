"""Fine-tuning on the device: y3_bn_frozen_bwd against its restatements (tests/finetune_reference.py), and a model
with a frozen layer prefix / frozen BatchNorm statistics / pretrained initialisation, eagerly and as a captured graph.  With
Y3_FINETUNE_ERR=<file> the worst error / bound ratio of every quantity of the kernel cases is written there
(profiles/finetune_err.txt is such a run)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import finetune_reference as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
EINVAL = -1

# (n, h, w) x c: every m of {1, 63, 64, 65, 257, 2 * 13 * 13} and every c of {4, 8, 16, 32, 96, 1024} twice
SHAPES = [((1, 1, 1), 4), ((1, 7, 9), 8), ((1, 8, 8), 16), ((1, 5, 13), 32), ((1, 1, 257), 96), ((2, 13, 13), 1024),
          ((1, 1, 1), 1024), ((1, 9, 7), 96), ((1, 4, 16), 4), ((1, 13, 5), 8), ((1, 257, 1), 16), ((2, 13, 13), 32)]
DRES = ['none', 'overwrite', 'accumulate']


class _View:
    """An [n, h, w, c] view with pitch ld > c inside a NaN-filled buffer, one guard row before and after."""

    def __init__(self, geom, c, data, pad, off):
        from yolo3 import _hip
        n, h, w = geom
        self.m, self.c, self.ld, self.off = n * h * w, c, c + pad, off
        host = np.full((self.m + 2, self.ld), np.nan, np.float32)
        if data is not None:
            host[1:-1, off:off + c] = data
        self.start = host.copy()
        self.buf = torch.from_numpy(host).cuda()
        self.v = _hip.view(self.buf, n, h, w, c, self.ld, self.ld + off)

    def read(self):
        return self.buf.cpu().numpy()

    def data(self):
        return self.read()[1:-1, self.off:self.off + self.c]

    def canaries_untouched(self, written):
        """Everything but the view (or, written=False, the whole buffer) holds the bits it started with."""
        now, was = self.read().view(np.uint32).copy(), self.start.view(np.uint32).copy()
        if written:
            now[1:-1, self.off:self.off + self.c] = was[1:-1, self.off:self.off + self.c] = 0
        return np.array_equal(now, was)


def _case(geom, c, seed):
    rng = np.random.default_rng(seed)
    m = geom[0] * geom[1] * geom[2]
    dy = rng.standard_normal((m, c)).astype(np.float32)
    a = rng.standard_normal((m, c)).astype(np.float32)
    a = np.where(a < 0, a * np.float32(0.2), a).astype(np.float32)
    z = rng.random((m, c))
    a[z < 0.05] = 0.0
    a[(z >= 0.05) & (z < 0.10)] = -0.0
    scale = (rng.standard_normal(c) * 1.5).astype(np.float32)
    mean = rng.standard_normal(c).astype(np.float32)
    var = (rng.random(c) * 2 + 0.01).astype(np.float32)
    dres0 = rng.standard_normal((m, c)).astype(np.float32)
    return dy, a, scale, mean, var, dres0


def _launch(geom, c, dy, a, scale, mean, var, dres0, mode, alpha, vec, ws=None):
    from yolo3._hip import lib
    pad, off = ((8, 4) if vec else (7, 3))         # ld and offset multiples of 4 (16-byte accesses), or neither (element-wise)
    V = dict(dy=_View(geom, c, dy, pad, off), a=_View(geom, c, a, pad + 4, off), dz=_View(geom, c, None, pad, off),
             dres=_View(geom, c, dres0, pad + 8, off) if mode != 'none' else None)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    sc, mu, va = dev(scale), dev(mean), dev(var)
    out = torch.full((3, c + 2), float('nan'), dtype=torch.float32, device='cuda')          # dgamma | dbeta | dbias, a guard each side
    m = geom[0] * geom[1] * geom[2]
    need = int(lib.y3_bn_frozen_bwd_workspace(m, c))
    assert need > 1024
    if ws is None:
        ws = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
        ws[need:] = 0xAB
    ptr = lambda r: out.data_ptr() + 4 * (r * (c + 2) + 1)
    rc = lib.y3_bn_frozen_bwd(V['dy'].v, V['a'].v, V['dres'].v if V['dres'] else None, 1 if mode == 'accumulate' else 0, sc.data_ptr(),
                              mu.data_ptr(), va.data_ptr(), float(fr.EPS), float(alpha), V['dz'].v, ptr(0), ptr(1), ptr(2), ws.data_ptr(),
                              need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, V, out.cpu().numpy(), ws, need


@functools.lru_cache(maxsize=None)
def _run_case(idx, vec):
    """One kernel case with all its assertions; returns the worst err / bound ratio per quantity."""
    geom, c = SHAPES[idx]
    mode, alpha = DRES[idx % 3], np.float32(0.1 if idx % 2 else 0.2)
    dy, a, scale, mean, var, dres0 = _case(geom, c, 100 + idx)
    rc, V, out, ws, need = _launch(geom, c, dy, a, scale, mean, var, dres0, mode, alpha, vec)
    assert rc == 0
    want_dz = fr.frozen_dz_f32(dy, a, scale, alpha)
    assert np.array_equal(V['dz'].data().view(np.uint32), want_dz.view(np.uint32))
    assert V['dz'].canaries_untouched(True) and V['dy'].canaries_untouched(False) and V['a'].canaries_untouched(False)
    if mode != 'none':
        want_dres = fr.frozen_dres_f32(dy, dres0, mode == 'accumulate')
        assert np.array_equal(V['dres'].data().view(np.uint32), want_dres.view(np.uint32))
        assert V['dres'].canaries_untouched(True)
    assert np.isnan(out[:, 0]).all() and np.isnan(out[:, -1]).all()
    wsh = ws.cpu().numpy()
    assert not wsh[:1024].any() and (wsh[need:] == 0xAB).all()
    S1, S2, S3 = fr.frozen_sums_f64(dy, a, want_dz)
    want = fr.frozen_results_f64(S1, S2, S3, mean, var)
    bounds = fr.frozen_bounds(dy, a, want_dz, mean, var)
    ratios = {}
    for name, got, w, b in zip(('dgamma', 'dbeta', 'dbias'), out[:, 1:-1], want, bounds):
        err = np.abs(got.astype(np.float64) - w)
        ratios[name] = float((err / b).max()) if np.isfinite(got).all() else float('inf')
        print('%s m=%d c=%d: worst err / bound %.3g' % (name, dy.shape[0], c, ratios[name]))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    # the same launch again, on the workspace the first one left behind
    rc2, V2, out2, _, _ = _launch(geom, c, dy, a, scale, mean, var, dres0, mode, alpha, vec, ws=ws)
    assert rc2 == 0
    assert np.array_equal(out2.view(np.uint32), out.view(np.uint32))
    assert np.array_equal(V2['dz'].data().view(np.uint32), V['dz'].data().view(np.uint32))
    return ratios


@pytest.mark.parametrize('vec', [True, False], ids=['vec16', 'elementwise'])
@pytest.mark.parametrize('idx', range(len(SHAPES)))
def test_bn_frozen_bwd_against_the_restatements(idx, vec):
    """dz / dres bit-equal to the float32 restatement, the per-channel results within the bound derived from the roundings
    (finetune_reference.frozen_bounds), NaN canaries around every view untouched, the ticket header left zero, two launches
    bit-equal."""
    _run_case(idx, vec)


def test_bn_frozen_bwd_error_profile():
    """All cases above (cached): the worst err / bound ratio per quantity, written to the file Y3_FINETUNE_ERR names."""
    _worst = {}
    for idx in range(len(SHAPES)):
        for vec in (True, False):
            for k, v in _run_case(idx, vec).items():
                _worst[k] = max(_worst.get(k, 0.0), v)
    lines = ['y3_bn_frozen_bwd against the exact fp64 sums: worst |err| / bound over %d shapes x (16-byte, element-wise) views;' % len(SHAPES),
             'bound = one fp32 rounding + m * 2^-53 * sum|term| (+ the cancellation term of dgamma), tests/finetune_reference.py']
    lines += ['%-7s %.4g' % (k, _worst[k]) for k in ('dgamma', 'dbeta', 'dbias')]
    print('\n'.join(lines))
    if os.environ.get('Y3_FINETUNE_ERR'):
        with open(os.environ['Y3_FINETUNE_ERR'], 'w') as f:
            f.write('\n'.join(lines) + '\n')
    assert all(v <= 1.0 for v in _worst.values())


def test_bn_frozen_bwd_refuses_bad_calls():
    from yolo3 import _hip
    from yolo3._hip import lib
    geom, c = (1, 4, 4), 32
    dy, a, scale, mean, var, dres0 = _case(geom, c, 7)
    V = dict(dy=_View(geom, c, dy, 8, 4), a=_View(geom, c, a, 8, 4), dz=_View(geom, c, None, 8, 4), dres=_View(geom, c, dres0, 8, 4))
    dev = lambda x: torch.from_numpy(x).cuda()
    sc, mu, va = dev(scale), dev(mean), dev(var)
    out = torch.zeros(3, c, dtype=torch.float32, device='cuda')
    need = int(lib.y3_bn_frozen_bwd_workspace(16, c))
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    good = dict(dy=V['dy'].v, a=V['a'].v, dres=V['dres'].v, acc=0, scale=sc.data_ptr(), mean=mu.data_ptr(), var=va.data_ptr(), eps=1e-3,
                alpha=0.2, dz=V['dz'].v, dg=out[0].data_ptr(), db=out[1].data_ptr(), dbi=out[2].data_ptr(), ws=ws.data_ptr(), wsb=need)

    def call(**kw):
        k = dict(good, **kw)
        return lib.y3_bn_frozen_bwd(k['dy'], k['a'], k['dres'], k['acc'], k['scale'], k['mean'], k['var'], k['eps'], k['alpha'], k['dz'],
                                    k['dg'], k['db'], k['dbi'], k['ws'], k['wsb'], st)

    assert call() == 0
    for name in ('dy', 'a', 'dz', 'scale', 'mean', 'var', 'dg', 'db', 'dbi', 'ws'):
        assert call(**{name: None}) == EINVAL, name
        assert b'bn_frozen_bwd' in lib.y3_last_error()
    for bad_c in (12, 36, 2048, 6):
        bv = lambda: _View(geom, bad_c, None, 8, 4).v
        assert call(dy=bv(), a=bv(), dz=bv(), dres=None) == EINVAL, bad_c
        assert lib.y3_bn_frozen_bwd_workspace(16, bad_c) == 0
    other = _View((1, 4, 5), c, None, 8, 4)
    assert call(a=other.v) == EINVAL and call(dz=other.v) == EINVAL and call(dres=other.v) == EINVAL
    assert call(dz=V['dy'].v) == EINVAL and call(dz=V['a'].v) == EINVAL and call(dz=V['dres'].v) == EINVAL
    shifted = _hip.view(V['dy'].buf, 1, 4, 4, c, V['dy'].ld, V['dy'].ld + 8)          # overlaps dy without being equal to it
    assert call(dz=shifted) == EINVAL
    assert call(wsb=need - 8) == EINVAL and call(ws=ws.data_ptr() + 4) == EINVAL
    for eps in (float('nan'), float('inf'), -float('inf')):
        assert call(eps=eps) == EINVAL
    torch.cuda.synchronize()
    assert not ws.cpu().numpy()[:1024].any()


def test_bn_frozen_bwd_dz_equals_the_apply_kernel_with_scale_as_coefficients():
    """y3_bn_bwd_apply with coef = (scale, 0, 0) computes (scale * dy + 0 * a + 0) * slope: the additions of the two zeros leave
    every non-zero product as it is but turn a product of -0 into +0, so the comparison is of VALUES (-0 == +0), exact, not of bits."""
    from yolo3._hip import lib
    geom, c = (2, 13, 13), 96
    dy, a, scale, mean, var, dres0 = _case(geom, c, 31)
    rc, V, _, _, _ = _launch(geom, c, dy, a, scale, mean, var, dres0, 'none', fr.ALPHA, True)
    assert rc == 0
    coef = torch.zeros(3 * c, dtype=torch.float32, device='cuda')
    coef[:c] = torch.from_numpy(scale).cuda()
    dz2 = _View(geom, c, None, 8, 4)
    assert lib.y3_bn_bwd_apply(V['dy'].v, V['a'].v, coef.data_ptr(), float(fr.ALPHA), dz2.v, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got, want = V['dz'].data(), dz2.data()
    assert np.array_equal(got, want) and not np.isnan(got).any()


# ---- the model -------------------------------------------------------------------------------------------------------------------------
ANCHORS, K, IMG, N = [(64, 384), (384, 64)], 2, 64, 2


def _model(seed=5, classes=K, randomize_bn=True, **kw):
    from oracle import model as om
    from yolo3.model import YoloV3
    params = om.init_params(3, len(ANCHORS), classes, seed=seed, randomize_bn=randomize_bn)
    if randomize_bn:
        for p in params:           # (test_gpu_model._setup: keep the head logits O(1) under randomised BatchNorm)
            if 'gamma' not in p:
                p['W'] *= 0.02
    yolo = YoloV3(N, [IMG, IMG, 3], classes, ANCHORS, learning_rate=1e-3, **kw)
    yolo.set_weights(params)
    return yolo


def _batch(seed=5, classes=K):
    from test_gpu_kernels import _labels
    images = torch.randn(N, 3, IMG, IMG, generator=torch.Generator().manual_seed(seed))
    return images, _labels(np.random.default_rng(seed), N, IMG, ANCHORS, classes, per_image=3)


def _steps(yolo, images, gts, k):
    for _ in range(k):
        loss = yolo.train_step((images.cuda(), [torch.from_numpy(g).cuda() for g in gts]))
    torch.cuda.synchronize()
    return float(loss)


def _layer_bits(yolo, arena, moving):
    """Per layer: the bits of its segment of a parameter-shaped arena and of its moving statistics."""
    p, mv = arena.cpu().numpy().view(np.uint32), moving.cpu().numpy().view(np.uint32)
    out = []
    for sp in yolo.specs:
        seg = [p[sp.w_off:sp.end_off]]
        if sp.bn:
            seg += [mv[sp.mv_off:sp.mv_off + sp.cout], mv[yolo.moving_stride + sp.mv_off:yolo.moving_stride + sp.mv_off + sp.cout]]
        out.append([s.copy() for s in seg])
    return out


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('nfrozen', [2, 52])
def test_frozen_prefix_keeps_its_bits(nfrozen, use_graph):
    """AdamW with weight decay, EMA and clipping for three steps: parameters, moving statistics and EMA copies of every frozen layer
    keep their bits, those of every trainable layer change, and the gradient arena in front of the trainable suffix is never written."""
    yolo = _model(freeze_layers=nfrozen, optimizer='adamw', weight_decay=0.05, ema_decay=0.9, ema_warmup=1.0, grad_clip_norm=1.0,
                  use_graph=use_graph)
    images, gts = _batch()
    off = yolo.specs[nfrozen].w_off
    yolo.grads[:off].fill_(float('nan'))      # (canaries: they would poison the norm if any pass read the frozen prefix)
    g0 = yolo.grads.cpu().numpy().view(np.uint32).copy()
    before = (_layer_bits(yolo, yolo.params, yolo.moving), _layer_bits(yolo, yolo.ema_params, yolo.ema_moving))
    loss = _steps(yolo, images, gts, 3)
    assert np.isfinite(loss) and np.isfinite(float(yolo.last_grad_norm))
    after = (_layer_bits(yolo, yolo.params, yolo.moving), _layer_bits(yolo, yolo.ema_params, yolo.ema_moving))
    for what, b, a in zip(('live', 'ema'), before, after):
        for i, (lb, la) in enumerate(zip(b, a)):
            same = [np.array_equal(x, y) for x, y in zip(lb, la)]
            if i < nfrozen:
                assert all(same), (what, i, same)
            else:
                assert not any(same), (what, i, same)
    g1 = yolo.grads.cpu().numpy().view(np.uint32)
    assert np.array_equal(g1[:off], g0[:off]) and np.isfinite(yolo.grads[off:].cpu().numpy()).all()
    # grad_norm is the norm over the trainable parameters only, before the clip
    plain = _model(freeze_layers=nfrozen, grad_clip_norm=1.0, use_graph=use_graph)
    _steps(plain, images, gts, 1)
    want = float((plain.grads[off:].double() ** 2).sum().sqrt())
    assert abs(float(plain.last_grad_norm) - want) <= 1e-5 * want


def _check(rep):
    rep.print()
    assert not rep.failures, '%d failures, first: %s' % (len(rep.failures), rep.failures[:8])


@pytest.mark.parametrize('nfrozen,freeze_bn', [(52, False), (10, False), (0, True), (52, True)])
def test_finetune_step_against_fp64_teacher_forced(nfrozen, freeze_bn):
    """One step against the fp64 restatement (finetune_reference.check_step): loss parts, every trainable parameter gradient and
    activation gradient, the trainable layers' forward and the frozen layers' inference form, at teacher_forced.BOUNDS.  10 cuts
    inside a residual stage: a frozen block input is the residual of trainable layers."""
    yolo = _model(seed=11, freeze_layers=nfrozen, freeze_bn=freeze_bn)
    images, gts = _batch(11)
    cap = fr.capture_step(yolo, images, gts)
    _check(fr.check_step(cap, tag='freeze %d bn %d' % (nfrozen, freeze_bn)))
    plan = yolo._plan(N, True)
    names = [e[0].__name__ for e in plan.fwd + plan.bwd if not isinstance(e[0], str)]
    assert names.count('y3_bn_stats_finalize') == (0 if freeze_bn else sum(1 for sp in yolo.specs[nfrozen:] if sp.bn))
    assert names.count('y3_bn_frozen_bwd') == (sum(1 for sp in yolo.specs[nfrozen:] if sp.bn) if freeze_bn else 0)
    assert names.count('y3_bn_fold_inference_batched') == 1 and names.count('y3_conv2d_dgrad_bn') * freeze_bn == 0


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('nfrozen', [0, 52])
def test_frozen_statistics_stay_and_gamma_beta_train(nfrozen, use_graph):
    yolo = _model(freeze_layers=nfrozen, freeze_bn=True, use_graph=use_graph)
    images, gts = _batch()
    mv0 = yolo.moving.cpu().numpy().view(np.uint32).copy()
    w0 = yolo.get_weights()
    loss = _steps(yolo, images, gts, 3)
    assert np.isfinite(loss)
    assert np.array_equal(yolo.moving.cpu().numpy().view(np.uint32), mv0)
    for i, (b, a) in enumerate(zip(w0, yolo.get_weights())):
        if 'gamma' in b:
            changed = [not np.array_equal(b[k], a[k]) for k in ('gamma', 'beta')]
            assert all(changed) == (i >= nfrozen) and any(changed) == (i >= nfrozen), (i, changed)
    # the captured step computes what the eager one does
    if use_graph:
        eager = _model(freeze_layers=nfrozen, freeze_bn=True)
        _steps(eager, images, gts, 3)
        np.testing.assert_allclose(yolo.params.cpu().numpy(), eager.params.cpu().numpy(), rtol=0, atol=1e-6)


@pytest.mark.parametrize('case', ['sgd-accumulate-graph', 'spp-frozen-bn', 'multiscale', 'last-head-only'])
def test_finetune_composes(case):
    """The settings beside the other options of training: SGD with decay under accumulation in captured graphs, the SPP network
    with frozen statistics, two input sizes (one plan each), and everything frozen but the last head.  Two optimiser steps each:
    finite losses, the frozen layers' bits as they were, the last head changed."""
    kw, sizes, nfrozen = dict(freeze_layers=52), [IMG], 52
    if case == 'sgd-accumulate-graph':
        kw.update(optimizer='sgd', weight_decay=5e-4, accumulate_steps=2, grad_clip_norm=10.0, use_graph=True)
    elif case == 'spp-frozen-bn':
        kw.update(spp=True, freeze_bn=True, ema_decay=0.9)
    elif case == 'multiscale':
        kw.update(train_sizes=[(IMG, IMG), (96, 96)], freeze_bn=True)
        sizes = [IMG, 96]
    else:
        nfrozen = 74
        kw.update(freeze_layers=nfrozen)
    from yolo3.model import YoloV3
    from test_gpu_kernels import _labels
    yolo = YoloV3(N, [IMG, IMG, 3], K, ANCHORS, learning_rate=1e-3, seed=3, **kw)
    assert yolo.freeze_layers == nfrozen and len(yolo.specs) == (76 if kw.get('spp') else 75)
    before = _layer_bits(yolo, yolo.params, yolo.moving)
    rng = np.random.default_rng(8)
    for step in range(2 * yolo.accumulate_steps):
        s = sizes[step % len(sizes)]
        images = torch.randn(N, 3, s, s, generator=torch.Generator().manual_seed(step))
        gts = _labels(rng, N, s, ANCHORS, K, per_image=3)
        loss = float(yolo.train_step((images.cuda(), [torch.from_numpy(g).cuda() for g in gts])))
        assert np.isfinite(loss)
    torch.cuda.synchronize()
    assert yolo.iterations == 2
    after = _layer_bits(yolo, yolo.params, yolo.moving)
    for i, (lb, la) in enumerate(zip(before, after)):
        same = [np.array_equal(x, y) for x, y in zip(lb, la)]
        assert all(same) if i < nfrozen else not same[0], (i, same)
    if yolo.freeze_bn:
        assert all(np.array_equal(x, y) for lb, la in zip(before, after) for x, y in zip(lb[1:], la[1:]))
    assert np.isfinite(yolo.params.cpu().numpy()).all()


def test_load_pretrained_into_another_class_count(tmp_path, capsys):
    src = _model(seed=3)
    path = str(tmp_path / 'two.npz')
    src.save_weights(path)
    dst = _model(seed=9, classes=3, randomize_bn=False)
    init = dst.get_weights()
    kept = dst.load_pretrained(path)
    heads = [i for i, sp in enumerate(dst.specs) if not sp.bn]
    assert kept == heads and dst.iterations == 0
    printed = capsys.readouterr().out
    assert all('layer %d ' % i in printed for i in heads)
    file, now = src.get_weights(), dst.get_weights()
    for i in range(len(dst.specs)):
        ref = init[i] if i in heads else file[i]
        assert sorted(now[i]) == sorted(ref)
        for k in ref:
            assert np.array_equal(now[i][k].view(np.uint32), ref[k].view(np.uint32)), (i, k)
    assert not dst.adam_m.any() and not dst.adam_v.any()
    images, gts = _batch(4, classes=3)
    assert np.isfinite(_steps(dst, images, gts, 1)) and dst.iterations == 1
    # heads of equal shape load; an SPP file does not go into a plain model
    same = _model(seed=9)
    assert same.load_pretrained(path) == []
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(same.get_weights(), file) for k in b)


def _normalised(plan):
    """The launch lists up to addresses: function names, and of the arguments the geometry of every view and every plain number."""
    from yolo3._hip import Tensor
    out = []
    for e in plan.fwd + [('|', ())] + plan.bwd:
        fn, args = e[0], e[1]
        if isinstance(fn, str):
            out.append((fn, args if not isinstance(args, tuple) else len(args)))
            continue
        norm = []
        for v in args:
            if isinstance(v, Tensor):
                norm.append((v.n, v.h, v.w, v.c, v.ld))
            elif isinstance(v, float) or v is None or (isinstance(v, int) and abs(v) < 2 ** 24):
                norm.append(v)
            else:
                norm.append('addr')
        out.append((fn.__name__, tuple(norm)))
    return out


def test_default_call_lists_unchanged():
    """A model built without the arguments emits the call lists of freeze_layers=0, freeze_bn=False -- the comparison the issue
    allows where lists recorded from the parent commit are impractical (they hold ~700 launches with their argument tuples) -- and
    those lists hold none of the launches fine-tuning adds: no fold in the training plan, no y3_bn_frozen_bwd, one statistics pass
    and one y3_bn_apply per BatchNorm layer."""
    a = _model(randomize_bn=False)
    b = _model(randomize_bn=False, freeze_layers=0, freeze_bn=False)
    la, lb = _normalised(a._plan(N, True)), _normalised(b._plan(N, True))
    assert la == lb
    names = [n for n, _ in la]
    nbn = sum(1 for sp in a.specs if sp.bn)
    assert 'y3_bn_fold_inference_batched' not in names and 'y3_bn_frozen_bwd' not in names
    assert names.count('y3_bn_stats_finalize') == nbn == names.count('y3_bn_apply')
    assert names.count('y3_conv2d_fwd') == len(a.specs) and a.train_off == 0 and a.train_floats == a.arena_floats
    assert a._adam_call[1][0] == a.params.data_ptr() and a._adam_call[1][4] == a.arena_floats


def test_cli_finetune_from_a_pretrained_file(tmp_path):
    """train.py --init_weights ... --freeze backbone --freeze_bn 1 for two batches: exit 0, and the exported model's backbone
    layers hold the bits of the init file."""
    from test_gpu_cli import _write_dataset
    from yolo3.model import YoloV3
    tmp = str(tmp_path)
    size = (256, 256, 3)
    _write_dataset(tmp, 4, size)              # two classes
    init = os.path.join(tmp, 'init.npz')
    src = YoloV3(2, list(size), 3, ANCHORS)     # another class count than the dataset's two
    src.save_weights(init)
    want = src.get_weights()
    out = os.path.join(tmp, 'out')
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--batch_size', '2', '--test_every_n_steps', '1', '--train_database',
                        os.path.join(tmp, 'train-syn.lmdb'), '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out,
                        '--early_stopping', '1', '--use_augmentation', '0', '--max_epochs', '1', '--reader_count', '1', '--init_weights', init,
                        '--freeze', 'backbone', '--freeze_bn', '1'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Fine-tuning: 52 of 75 layers frozen' in r.stdout and 'keep their initialisation' in r.stdout
    assert r.stdout.count('Train Epoch 0: Batch') == 2
    got = YoloV3.from_file(os.path.join(out, 'saved_model', 'yolov3.npz')).get_weights()
    for i in range(52):
        for k in want[i]:
            assert np.array_equal(got[i][k].view(np.uint32), want[i][k].view(np.uint32)), (i, k)
    assert any(not np.array_equal(got[i]['W'], want[i]['W']) for i in range(52, 58))
