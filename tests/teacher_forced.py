"""Teacher-forced, layer-by-layer check of the training step and of the fp32 inference plan against fp64 (test helper).

capture_step() runs one ordinary YoloV3.train_step and reads back everything the plan leaves in its buffers: per BatchNorm layer
the post-leaky-relu tensor `a`, the output `y`, its final gradient, the saved batch mean / rstd; per upsample its output and
gradient; per head the feature map and its gradient; the loss parts; the arenas before and after the step.  check_step() then
recomputes every launch of the plan in fp64 from the GPU's OWN inputs to it (oracle.model.Net with `force` + `teacher`), so
nothing compounds and no leaky-relu slope can flip: each layer is held to roughly the per-kernel tolerance of the launches
between its forced inputs and the checked output (BOUNDS).  One backward pass of the surrogate
    sum_j <y_ref_j, dy_gpu_j> + sum_j <up_ref_j, dup_gpu_j> + sum_h <fm_ref_h, dfm_gpu_h>
gives every parameter gradient and, for every forced tensor, the sum of its consumers' vector-Jacobian products, which the
GPU's final gradient of that tensor must equal (residual fan-in, EPI_ACCUM, concat slices and upsample backward together).
The loss is checked on its own (oracle loss_layer on the GPU's feature maps); ignore-mask decisions within IGNORE_MARGIN of the
threshold are excluded from the objectness gradient and counted.

Bounds are relative to max|ref| of each tensor, as in util.assert_close.  check_step / check_inference return a Report whose
failures name the quantity and the layer; Report.lines() gives the worst err / bound ratio of every quantity kind.
"""
import math

import numpy as np
import torch

from oracle import model as om

BOUNDS = {
    'a': 2e-5,              # conv + bias + leaky relu (test_conv_fwd)
    'mean': 1e-5,           # saved batch statistics (test_batchnorm_train_fwd_bwd)
    'rstd': 1e-5,
    'moving': 1e-5,         # moving mean / variance after the step
    'y': 1e-5,              # BatchNorm apply (+ residual)
    'up': 1e-5,             # upsample forward (test_upsample_sum2x)
    'dgamma': 1e-4,         # BatchNorm backward (test_batchnorm_train_fwd_bwd)
    'dbeta': 1e-4,
    'dbias': 1e-4,          # ... with the floor 1e-4 x max_c sum |dz| of that test
    'dW': 1e-4 + 5e-5,      # BatchNorm backward + kernel gradient (test_conv_wgrad; x3 held to the same rule)
    'dact': 1e-4 + 2e-5,    # every activation gradient: BatchNorm backward + data gradient (test_conv_dgrad)
    'fm': 2e-5,             # heads (test_conv_fwd_detection_head)
    'head_dW': 5e-5,        # head kernel gradient (test_conv_wgrad)
    'head_db': 5e-5,        # head bias gradient (column sum), floor 5e-5 x max_c sum |dfm|
    'dfm': 1e-4,            # loss gradient (test_loss_fwd_bwd_matches_oracle)
    'loss4': 2e-5,
    'adam': 1e-6,           # parameters, m, v after the step (test_adam_matches_oracle)
    'infer': 2e-5,          # fp32 inference plan: conv + leaky relu + folded BatchNorm + residual (test_conv_fwd_fused_inference_epilogue)
}
IGNORE_MARGIN = 1e-5        # |best IoU - 0.5| below this: the ignore decision is rounding noise, the objectness gradient is not compared
F64 = torch.float64


class Report:
    def __init__(self, tag):
        self.tag = tag
        self.worst = {}       # kind -> (ratio, layer)
        self.failures = []

    def add(self, kind, layer, got, ref, rtol=None, atol=None, mask=None):
        """max |got - ref| against rtol x max|ref| (or atol); mask: elements to compare (True = compare)."""
        rtol = BOUNDS[kind] if rtol is None else rtol
        ref = ref.detach().to(F64)
        got = got.detach().to(device=ref.device, dtype=F64)
        if got.shape != ref.shape:
            self._note(kind, layer, math.inf, 'shape %s vs %s' % (tuple(got.shape), tuple(ref.shape)))
            return
        scale = float(ref.abs().max()) if ref.numel() else 1.0
        bound = rtol * max(scale, 1e-30) if atol is None else atol
        diff = (got - ref).abs()
        if mask is not None:
            diff = torch.where(mask, diff, torch.zeros_like(diff))
        finite = bool(torch.isfinite(got if mask is None else torch.where(mask, got, torch.zeros_like(got))).all())
        err = float(diff.max()) if diff.numel() else 0.0
        ratio = err / bound if finite else math.inf
        self._note(kind, layer, ratio, 'max err %.3e > bound %.3e (scale %.3e)' % (err, bound, scale))

    def exact(self, kind, layer, ok, what=''):
        self._note(kind, layer, 0.0 if ok else math.inf, 'not bit-identical %s' % what)

    def _note(self, kind, layer, ratio, msg):
        if kind not in self.worst or ratio > self.worst[kind][0]:
            self.worst[kind] = (ratio, layer)
        if not ratio <= 1.0:
            self.failures.append('%s layer %s: %s' % (kind, layer, msg))

    def lines(self):
        return ['%s %-8s worst err/bound %.3g at layer %s' % (self.tag, k, r, l) for k, (r, l) in sorted(self.worst.items())]

    def print(self):
        for ln in self.lines():
            print(ln)


# ---- arenas <-> per-layer tensors (layout: yolo3.model.build_layer_specs) ----------------------------------------------------------
def unpack(arena, specs, padded=False):
    """Arena -> per-layer dicts W [k, k, cin(_pad), cout], b, gamma, beta (views of the arena)."""
    out = []
    for sp in specs:
        W = arena[sp.w_off:sp.w_off + sp.k * sp.k * sp.cin_pad * sp.cout].view(sp.k, sp.k, sp.cin_pad, sp.cout)
        d = dict(W=W if padded else W[:, :, :sp.cin], b=arena[sp.b_off:sp.b_off + sp.cout])
        if sp.bn:
            d['gamma'] = arena[sp.g_off:sp.g_off + sp.cout]
            d['beta'] = arena[sp.be_off:sp.be_off + sp.cout]
        out.append(d)
    return out


def unpack_moving(moving, specs, stride):
    return [(moving[sp.mv_off:sp.mv_off + sp.cout], moving[stride + sp.mv_off:stride + sp.mv_off + sp.cout]) for sp in specs if sp.bn]


def transposed(params, specs):
    """CPU restatement of the transposed copy (params_t): [tap][Cout][Cin] of every kernel after the first, -> {layer: tensor}."""
    return {i: unpack(params, [sp], padded=True)[0]['W'].reshape(sp.k * sp.k, sp.cin_pad, sp.cout).transpose(1, 2)
            for i, sp in enumerate(specs) if i > 0}


def split_planes(w):
    """The x3 weight planes (include/yolo3hip.h, y3_x3_split_weights) of w [taps, rows, kpr] fp32: each piece the round-to-nearest
    bf16 of what the earlier ones leave; layout planes[(((tap * kpr/16 + c/16) * rows + row) * 3 + piece) * 16 + c % 16]."""
    taps, rows, kpr = w.shape
    pieces, r = [], w.float()
    for _ in range(3):
        p = r.to(torch.bfloat16)
        pieces.append(p)
        r = r - p.float()             # exact in fp32
    P = torch.stack(pieces).view(3, taps, rows, kpr // 16, 16)
    return P.permute(1, 3, 2, 0, 4).reshape(-1)


def planes_of(params, specs):
    """-> ({layer: planes of the Keras copy}, {layer: planes of the transposed copy}) for the layers whose K per row is a
    multiple of 16 (what y3_x3_prepare_weights_batched writes)."""
    keras, trans = {}, {}
    for i, sp in enumerate(specs):
        if i == 0:
            continue
        W = unpack(params, [sp], padded=True)[0]['W'].reshape(sp.k * sp.k, sp.cin_pad, sp.cout)
        if sp.cout % 16 == 0:
            keras[i] = split_planes(W)
        if sp.cin_pad % 16 == 0:
            trans[i] = split_planes(W.transpose(1, 2).contiguous())
    return keras, trans


def _bn_indices(specs):
    return [i for i, sp in enumerate(specs) if sp.bn]


def _head_indices(specs):
    return [i for i, sp in enumerate(specs) if not sp.bn]


# ---- capture of the real step ---------------------------------------------------------------------------------------------------
def _nchw(t):
    return t.torch_view().permute(0, 3, 1, 2).clone()


def capture_step(yolo, images, gts):
    """One ordinary yolo.train_step (eager, kernel gradients on the side stream by default) plus what its plan leaves behind."""
    pre = dict(params=yolo.params.clone(), moving=yolo.moving.clone(), m=yolo.adam_m.clone(), v=yolo.adam_v.clone())
    yolo.train_step((images.cuda(), [torch.as_tensor(g).cuda() for g in gts]))
    torch.cuda.synchronize()
    n = int(images.shape[0])
    plan = yolo._plan(n, True)
    cap = dict(specs=yolo.specs, moving_stride=yolo.moving_stride, in_channels=yolo.img_size[2], anchors=list(yolo.anchors),
               K=yolo.number_classes, img_size=tuple(yolo.img_size), gbs=float(yolo.global_batch_size),
               images=images.float().cuda(), gts=[torch.as_tensor(g).float() for g in gts], pre=pre,
               a=[], y=[], dy=[], mean=[], rstd=[], up=[], dup=[], fm=[], dfm=[], slices=[])
    for op in plan.ops:
        if op[0] == 'conv_layer':
            _, i, src, a, y, resid, _ = op
            sp = yolo.specs[i]
            c0 = sp.ch_off + 2 * sp.cout
            cap['a'].append(_nchw(a))
            cap['y'].append(_nchw(y))
            cap['dy'].append(_nchw(y.grad))
            cap['mean'].append(yolo.chan[c0:c0 + sp.cout].clone())
            cap['rstd'].append(yolo.chan[c0 + sp.cout:c0 + 2 * sp.cout].clone())
            if y.parent is not None:
                cap['slices'].append(len(cap['y']) - 1)
        elif op[0] == 'head':
            cap['fm'].append(_nchw(op[3]))
            cap['dfm'].append(_nchw(op[3].grad))
        else:
            cap['up'].append(_nchw(op[2]))
            cap['dup'].append(_nchw(op[2].grad))
    cap['loss4'] = plan.loss4.clone()
    cap['grads'] = yolo.grads.clone()
    cap['lr_t'] = float(yolo.lr_t_dev[0])
    cap['post'] = dict(params=yolo.params.clone(), moving=yolo.moving.clone(), m=yolo.adam_m.clone(), v=yolo.adam_v.clone(),
                       params_t=yolo.params_t.clone(),
                       planes=None if yolo.planes is None else yolo.planes.clone(),
                       planes_t=None if yolo.planes_t is None else yolo.planes_t.clone())
    return cap


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def _ref_params(cap, device):
    P = [{k: v.to(device=device, dtype=F64) for k, v in d.items()} for d in unpack(cap['pre']['params'], cap['specs'])]
    for d, (m, v) in zip([d for d, sp in zip(P, cap['specs']) if sp.bn], unpack_moving(cap['pre']['moving'], cap['specs'], cap['moving_stride'])):
        d['mean'], d['var'] = m.to(device, F64), v.to(device, F64)
    return P


def check_step(cap, device=None, forward_only=False, tag='step'):
    """Every launch of the captured step against fp64, teacher-forced.  device: where the fp64 reference runs (default: the
    capture's device).  forward_only: the forward checks (a, statistics, y, upsample, feature maps, moving statistics) only."""
    specs = cap['specs']
    device = cap['images'].device if device is None else device
    rep = Report(tag)
    bn_i, head_i = _bn_indices(specs), _head_indices(specs)
    P = _ref_params(cap, device)
    A, K = len(cap['anchors']), cap['K']
    net = om.Net(P, cap['in_channels'], A, K, dtype=F64, requires_grad=not forward_only, device=device)
    leaves_y = [t.to(device, F64).requires_grad_(not forward_only) for t in cap['y']]
    leaves_up = [t.to(device, F64).requires_grad_(not forward_only) for t in cap['up']]
    net.force = {'layers': leaves_y, 'up': leaves_up}
    net.teacher = {'a': [t.to(device, F64) for t in cap['a']]}
    x = cap['images'].to(device, F64)
    with torch.set_grad_enabled(not forward_only):
        fms = net.feature_maps(x, training=True)
    T = net.teacher
    assert len(T['y']) == len(bn_i) == len(cap['y']) and len(T['up']) == len(cap['up']) == 2 and len(fms) == len(cap['fm']) == 3
    moving = unpack_moving(cap['pre']['moving'], specs, cap['moving_stride'])
    moving_post = unpack_moving(cap['post']['moving'], specs, cap['moving_stride'])
    for j, i in enumerate(bn_i):
        rep.add('a', i, cap['a'][j], T['act'][j])
        mean, var, cnt = net.batch_stats[j]
        rep.add('mean', i, cap['mean'][j], mean)
        rep.add('rstd', i, cap['rstd'][j], torch.rsqrt(var + om.BN_EPS))
        (m0, v0), (m1, v1) = moving[j], moving_post[j]
        rep.add('moving', i, m1, m0.to(device, F64) * om.BN_MOMENTUM + mean * (1 - om.BN_MOMENTUM))
        rep.add('moving', i, v1, v0.to(device, F64) * om.BN_MOMENTUM + var * (cnt / max(cnt - 1.0, 1.0)) * (1 - om.BN_MOMENTUM))
        rep.add('y', i, cap['y'][j], T['y'][j])
    for j in range(2):
        rep.add('up', 'up%d' % j, cap['up'][j], T['up'][j])
    for h, i in enumerate(head_i):
        rep.add('fm', i, cap['fm'][h], fms[h])
    if forward_only:
        return rep

    # surrogate backward: every output seeded with the implementation's own gradient of it
    dev = lambda t: t.to(device, F64)
    S = sum((y * dev(g)).sum() for y, g in zip(T['y'], cap['dy']))
    S = S + sum((u * dev(g)).sum() for u, g in zip(T['up'], cap['dup']))
    S = S + sum((f * dev(g)).sum() for f, g in zip(fms, cap['dfm']))
    params = net.trainable()
    grads = torch.autograd.grad(S, params + leaves_y + leaves_up, allow_unused=True)
    zeros = lambda t: torch.zeros_like(t)
    grads = [g if g is not None else zeros(t) for g, t in zip(grads, params + leaves_y + leaves_up)]
    gp, gy, gu = grads[:len(params)], grads[len(params):len(params) + len(leaves_y)], grads[len(params) + len(leaves_y):]
    G = unpack(cap['grads'], specs)
    k = 0
    for i, sp in enumerate(specs):
        dW, db = gp[k], gp[k + 1]
        if sp.bn:
            dg, dbe = gp[k + 2], gp[k + 3]
            k += 4
            rep.add('dW', i, G[i]['W'], dW)
            rep.add('dgamma', i, G[i]['gamma'], dg)
            rep.add('dbeta', i, G[i]['beta'], dbe)
            dz_abs = _dz_abs_sum(net, cap, bn_i.index(i), i, device)
            rep.add('dbias', i, G[i]['b'], db, atol=BOUNDS['dbias'] * max(float(dz_abs.max()), 1e-30))
        else:
            k += 2
            h = head_i.index(i)
            rep.add('head_dW', i, G[i]['W'], dW)
            rep.add('head_db', i, G[i]['b'], db, atol=BOUNDS['head_db'] * max(float(dev(cap['dfm'][h]).abs().sum(dim=(0, 2, 3)).max()), 1e-30))
    for j, i in enumerate(bn_i):
        rep.add('dact', i, cap['dy'][j], gy[j])
    for j in range(2):
        rep.add('dact', 'up%d' % j, cap['dup'][j], gu[j])
    # padded input channels of the first layer: exactly zero gradient, exactly zero after the step
    sp0 = specs[0]
    for name, arena in (('grads', cap['grads']), ('params', cap['post']['params']), ('m', cap['post']['m']), ('v', cap['post']['v'])):
        pad = unpack(arena, [sp0], padded=True)[0]['W'][:, :, sp0.cin:, :]
        rep.exact('pad', 0, bool((pad == 0).all()), '(padded input channels of %s)' % name)
    _check_loss(rep, cap)
    _check_adam(rep, cap)
    _check_derived(rep, cap)
    return rep


def _dz_abs_sum(net, cap, j, i, device):
    """Per channel sum over pixels of |dz| of BatchNorm layer j (layer i) in fp64, from the forced a, the GPU's dy and the
    reference statistics (the BatchNorm + leaky-relu backward written out): the floor of the dbias comparison."""
    a = cap['a'][j].to(device, F64)
    dy = cap['dy'][j].to(device, F64)
    mean, var, _ = net.batch_stats[j]
    rstd = torch.rsqrt(var + om.BN_EPS)[None, :, None, None]
    xhat = (a - mean[None, :, None, None]) * rstd
    gamma = net.p[i]['gamma'].detach()[None, :, None, None]
    g = dy * gamma
    da = rstd * (g - g.mean(dim=(0, 2, 3), keepdim=True) - xhat * (g * xhat).mean(dim=(0, 2, 3), keepdim=True))
    dz = da * torch.where(a > 0, 1.0, om.LRELU_ALPHA)
    return dz.abs().sum(dim=(0, 2, 3))


def _check_loss(rep, cap):
    """loss4 and every fm.grad against oracle loss_layer in fp64 on the GPU's own feature maps."""
    H, W, C = cap['img_size']
    A, K = len(cap['anchors']), cap['K']
    parts = torch.zeros(4, dtype=F64)
    slack = torch.zeros(4, dtype=F64)
    near_total = 0
    for h in range(3):
        fm = cap['fm'][h].detach().cpu().to(F64).requires_grad_(True)
        gt = cap['gts'][h].cpu().to(F64)
        info = {}
        p = om.loss_layer(fm, gt, (H, W, C), cap['anchors'], K, info=info)
        (sum(p) / cap['gbs']).backward()
        parts += torch.stack([q.detach() for q in p])
        mask = torch.ones_like(fm, dtype=torch.bool)
        if info['best_iou'] is not None:
            near = ((info['best_iou'] - 0.5).abs() < IGNORE_MARGIN) & (gt[..., 4] == 0)       # [N, G, G, A]
            near_total += int(near.sum())
            if bool(near.any()):
                N, _, Gh, Gw = fm.shape
                obj = fm.detach().permute(0, 2, 3, 1).reshape(N, Gh, Gw, A, 5 + K)[..., 4]
                slack[2] += float((torch.clamp(obj, min=0) + torch.log1p(torch.exp(-obj.abs())))[near].sum()) / N
                m = mask.permute(0, 2, 3, 1).reshape(N, Gh, Gw, A, 5 + K).clone()
                m[..., 4] &= ~near
                mask = m.reshape(N, Gh, Gw, A * (5 + K)).permute(0, 3, 1, 2)
        rep.add('dfm', 'head%d' % h, cap['dfm'][h].cpu(), fm.grad, mask=mask)
    # the excluded predictions must stay few: at most 0.1 % of them (and at least one is allowed)
    n_pred = sum(int(np.prod(f.shape)) // (5 + K) for f in cap['fm'])
    rep._note('ignore', '-', near_total / max(1.0, 1e-3 * n_pred), '%d predictions within %.0e of the ignore threshold' % (near_total, IGNORE_MARGIN))
    got = cap['loss4'].cpu().to(F64)
    bound = BOUNDS['loss4'] * float(parts.abs().max())
    err = ((got - parts).abs() - slack).clamp_min(0)
    rep._note('loss4', '-', float(err.max()) / bound, 'loss parts %s vs %s' % (got.tolist(), parts.tolist()))


def _check_adam(rep, cap):
    """The arena after the step against Keras Adam in fp64 applied to (pre-step params, GPU grads, m, v), with the fp32
    hyper-parameters the kernel is given (1 - fp32(0.999) is 1.3e-5 away from 1e-3)."""
    f32 = lambda v: float(np.float32(v))
    b1, b2, eps, lr = f32(0.9), f32(0.999), f32(1e-7), cap['lr_t']
    specs = cap['specs']
    d = lambda t: t.to(F64)
    g, p0, m0, v0 = d(cap['grads']), d(cap['pre']['params']), d(cap['pre']['m']), d(cap['pre']['v'])
    m = m0 + (g - m0) * (1 - b1)
    v = v0 + (g * g - v0) * (1 - b2)
    p = p0 - (m * lr) / (torch.sqrt(v) + eps)
    for name, got, want in (('params', cap['post']['params'], p), ('m', cap['post']['m'], m), ('v', cap['post']['v'], v)):
        for i, (dg, dw) in enumerate(zip(unpack(got, specs), unpack(want, specs))):
            for key in dg:
                rep.add('adam', '%d.%s.%s' % (i, key, name), dg[key], dw[key])


def _check_derived(rep, cap):
    """params_t, planes, planes_t after the step equal, bit for bit, the CPU restatement of the transpose and of the three-piece
    split of the GPU's new params (include/yolo3hip.h)."""
    specs = cap['specs']
    post = cap['post']
    pt = post['params_t']
    for i, want in transposed(post['params'], specs).items():
        sp = specs[i]
        got = pt[sp.w_off:sp.w_off + want.numel()]
        rep.exact('params_t', i, torch.equal(got, want.reshape(-1)))
    if post['planes'] is None:
        return
    keras, trans = planes_of(post['params'], specs)
    for name, arena, want in (('planes', post['planes'], keras), ('planes_t', post['planes_t'], trans)):
        for i, w in want.items():
            got = arena[3 * specs[i].w_off:3 * specs[i].w_off + w.numel()]
            rep.exact(name, i, torch.equal(got.view(torch.int16), w.view(torch.int16)))


# ---- the fp32 inference plan ------------------------------------------------------------------------------------------------------
def check_inference(yolo, images, params, device=None, tag='infer'):
    """predict() on the fp32 plan, then every conv layer, upsample and head of it recomputed in fp64 from the plan's own inputs
    (plan.layer_out / the upsample outputs forced, moving statistics of `params`): folded BatchNorm, the fused epilogue with the
    residual, the x3 forward."""
    n = int(images.shape[0])
    yolo.predict(images.cuda(), precision='fp32')
    plan = yolo._plan(n, False, False)
    torch.cuda.synchronize()
    layers = [_nchw(t) for t in plan.layer_out]
    ups = [_nchw(op[2]) for op in plan.ops if op[0] == 'upsample']
    fms = [_nchw(f) for f in plan.fms]
    device = layers[0].device if device is None else device
    net = om.Net(params, yolo.img_size[2], len(yolo.anchors), yolo.number_classes, dtype=F64, device=device)
    net.trace_exact, net.up_trace = [], []
    net.force = {'layers': [t.to(device, F64) for t in layers], 'up': [t.to(device, F64) for t in ups]}
    with torch.no_grad():
        ref_fms = net.feature_maps(images.to(device, F64), training=False)
    rep = Report(tag)
    bn_i, head_i = _bn_indices(yolo.specs), _head_indices(yolo.specs)
    assert len(layers) == len(net.trace_exact) == len(bn_i)
    for j, i in enumerate(bn_i):
        rep.add('infer', i, layers[j], net.trace_exact[j])
    for j, (g, r) in enumerate(zip(ups, net.up_trace)):
        rep.add('up', 'up%d' % j, g, r)
    for h, i in enumerate(head_i):
        rep.add('fm', i, fms[h], ref_fms[h])
    return rep
