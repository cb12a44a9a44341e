"""References for fine-tuning (test helper): y3_bn_frozen_bwd restated in NumPy float32 (dz, dres) and in fp64 (the
three sums, dgamma / dbeta / dbias and the bound they are held to), and one training step with a frozen layer prefix and / or
frozen BatchNorm statistics restated in fp64 torch autograd from oracle.model's layer functions, teacher-forced per layer in the
manner of tests/teacher_forced.py.

The bound of the per-channel results is derived from the roundings alone, nothing of it is fitted to the kernel:
  * the kernel's value is one fp32 rounding of an fp64 number: |value| * 2^-24 (+ the smallest fp32 subnormal);
  * an fp64 sum of m terms, in any order, is within m * 2^-53 * sum|term| of the exact sum (each of the < m additions rounds a
    partial sum that is at most sum|term| in magnitude);
  * dgamma = (S2 - mean * S1) / sqrt(var + eps): the absolute errors of S2 and of mean * S1 go through the subtraction unchanged,
    however small the difference is (the cancellation term), so they are divided by sqrt(var + eps) and not scaled by the result;
    the product, the difference, the square root and the division round once each in fp64.
The reference sums are exact (math.fsum) and their formula runs in fp64 too; the fp64 roundings counted below cover it as well.
"""
import math

import numpy as np
import torch

from oracle import model as om
import teacher_forced as tf

ALPHA = np.float32(0.2)
EPS = np.float32(1e-3)
U32 = 2.0 ** -24
U64 = 2.0 ** -53
F64 = torch.float64


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def frozen_dz_f32(dy, a, scale, alpha=ALPHA):
    """dz = (dy * scale_c) * (a > 0 ? 1 : alpha) with two fp32 roundings in this order; dy, a [m, c] float32, scale [c]."""
    dy, a, scale = np.asarray(dy, np.float32), np.asarray(a, np.float32), np.asarray(scale, np.float32)
    t = (dy * scale[None, :]).astype(np.float32)
    slope = np.where(a > 0, np.float32(1.0), np.float32(alpha)).astype(np.float32)
    return (t * slope).astype(np.float32)


def frozen_dres_f32(dy, dres0, accumulate):
    """dres = dy, or dres0 + dy (one fp32 rounding) with accumulate."""
    dy = np.asarray(dy, np.float32)
    return (np.asarray(dres0, np.float32) + dy).astype(np.float32) if accumulate else dy.copy()


def frozen_dz_f64(dy, a, scale, alpha=ALPHA):
    """The same expression without the roundings."""
    return np.asarray(dy, np.float64) * np.asarray(scale, np.float64)[None, :] * np.where(np.asarray(a) > 0, 1.0, float(alpha))


def _fsum_cols(x):
    return np.array([math.fsum(col) for col in np.asarray(x, np.float64).T], np.float64)


def frozen_sums_f64(dy, a, dz):
    """(S1, S2, S3) = (sum dy, sum dy * a, sum dz) per channel, exact sums of the fp64 terms (dy * a of two fp32 values is exact
    in fp64), rounded once."""
    dy64, a64 = np.asarray(dy, np.float64), np.asarray(a, np.float64)
    return _fsum_cols(dy64), _fsum_cols(dy64 * a64), _fsum_cols(dz)


def frozen_results_f64(S1, S2, S3, mean, var, eps=EPS):
    """(dgamma, dbeta, dbias) in fp64; var + eps with eps the fp32 value the kernel is given."""
    sd = np.sqrt(np.asarray(var, np.float64) + float(np.float32(eps)))
    return (S2 - np.asarray(mean, np.float64) * S1) / sd, S1.copy(), S3.copy()


def frozen_bounds(dy, a, dz, mean, var, eps=EPS):
    """Per-channel bounds (dgamma, dbeta, dbias) on |kernel - frozen_results_f64|, from the roundings (module docstring)."""
    dy64, a64, dz64 = np.asarray(dy, np.float64), np.asarray(a, np.float64), np.asarray(dz, np.float64)
    m = dy64.shape[0]
    S1, S2, S3 = frozen_sums_f64(dy, a, dz)
    mean64 = np.asarray(mean, np.float64)
    sd = np.sqrt(np.asarray(var, np.float64) + float(np.float32(eps)))
    acc1 = m * U64 * np.abs(dy64).sum(0)
    acc2 = m * U64 * np.abs(dy64 * a64).sum(0)
    acc3 = m * U64 * np.abs(dz64).sum(0)
    tiny = 2.0 ** -149
    g = (S2 - mean64 * S1) / sd
    b_dbeta = np.abs(S1) * U32 + acc1 + tiny
    b_dbias = np.abs(S3) * U32 + acc3 + tiny
    cancel = (acc2 + np.abs(mean64) * acc1 + 2 * U64 * (np.abs(S2) + np.abs(mean64 * S1))) / sd
    b_dgamma = np.abs(g) * U32 + cancel + 4 * U64 * np.abs(g) + tiny
    return b_dgamma, b_dbeta, b_dbias


# ---- the training step -------------------------------------------------------------------------------------------------------------
class FineTuneNet(om.Net):
    """oracle.model.Net with the BatchNorm mode chosen per layer (Net has one mode for the whole network): layers below
    freeze_layers run as in inference (training=False: moving statistics, no teacher forcing, nothing recorded); a trainable
    layer normalises with its batch statistics, or with freeze_bn with the moving statistics while gamma / beta stay live.  The
    layer body restates Net._conv_layer with that one decision added; the walk (feature_maps) is Net's own."""

    def __init__(self, *args, freeze_layers=0, freeze_bn=False, **kw):
        super().__init__(*args, **kw)
        self.freeze_layers, self.freeze_bn = int(freeze_layers), bool(freeze_bn)
        self._nt = 0
        for i, q in enumerate(self.p):
            if i < self.freeze_layers:
                for t in q.values():
                    t.requires_grad_(False)

    def feature_maps(self, x, training):
        self._nt = 0
        return super().feature_maps(x, training)

    def _conv_layer(self, x, i, training):
        import torch.nn.functional as F
        sp, q = self.specs[i], self.p[i]
        k, s = sp['k'], sp['s']
        ph, pw = om.same_pad(x.shape[2], k, s), om.same_pad(x.shape[3], k, s)
        x = F.pad(x, (pw[0], pw[1], ph[0], ph[1]))
        z = F.conv2d(x, q['W'].permute(3, 2, 0, 1), q['b'], stride=s)
        if not sp['bn']:
            return z
        a = F.leaky_relu(z, om.LRELU_ALPHA)
        train = training and i >= self.freeze_layers
        if train:
            if self.teacher is not None:
                self.teacher['act'].append(a.detach())
                if 'a' in self.teacher:
                    a = om._ForcedLeakyRelu.apply(z, self.teacher['a'][self._nt])
            self._nt += 1
        if train and not self.freeze_bn:
            mean = a.mean(dim=(0, 2, 3))
            var = a.var(dim=(0, 2, 3), unbiased=False)
            self.batch_stats.append((mean.detach(), var.detach(), a.numel() // a.shape[1]))
        else:
            mean, var = q['mean'], q['var']
        y = (a - mean[None, :, None, None]) * torch.rsqrt(var[None, :, None, None] + om.BN_EPS)
        return y * q['gamma'][None, :, None, None] + q['beta'][None, :, None, None]


def capture_step(yolo, images, gts):
    """One yolo.train_step of a model with freeze_layers / freeze_bn, plus what its plan leaves behind: the output of EVERY conv
    layer (frozen ones included: the reference consumes them), and per trainable BatchNorm layer `a` and the gradient of its output."""
    pre = dict(params=yolo.params.clone(), moving=yolo.moving.clone())
    yolo.train_step((images.cuda(), [torch.as_tensor(g).cuda() for g in gts]))
    torch.cuda.synchronize()
    plan = yolo._plan(int(images.shape[0]), True)
    cap = dict(specs=yolo.specs, moving_stride=yolo.moving_stride, in_channels=yolo.img_size[2], anchors=list(yolo.anchors),
               K=yolo.number_classes, img_size=tuple(yolo.img_size), gbs=float(yolo.global_batch_size), images=images.float().cuda(),
               gts=[torch.as_tensor(g).float() for g in gts], pre=pre, freeze_layers=yolo.freeze_layers, freeze_bn=yolo.freeze_bn,
               layers=[tf._nchw(t) for t in plan.layer_out], a={}, dy={}, up=[], dup=[], fm=[tf._nchw(f) for f in plan.fms],
               dfm=[tf._nchw(f.grad) for f in plan.fms], op_layers=[op[1] for op in plan.ops if op[0] in ('conv_layer', 'head')])
    for op in plan.ops:
        if op[0] == 'conv_layer':
            cap['a'][op[1]] = tf._nchw(op[3])
            cap['dy'][op[1]] = tf._nchw(op[4].grad)
        elif op[0] == 'upsample':
            cap['up'].append(tf._nchw(op[2]))
            cap['dup'].append(tf._nchw(op[2].grad))
    cap['loss4'] = plan.loss4.clone()
    cap['grads'] = yolo.grads.clone()
    cap['post'] = dict(params=yolo.params.clone(), moving=yolo.moving.clone())
    return cap


def check_step(cap, tag='finetune'):
    """The captured step against FineTuneNet in fp64, teacher-forced: every trainable layer's forward from the GPU's own inputs
    to it, every frozen layer's inference form, the loss parts, and every trainable parameter gradient and activation gradient
    from one backward pass of the surrogate of tests/teacher_forced.py.  Tolerances: teacher_forced.BOUNDS."""
    specs, N, fbn = cap['specs'], cap['freeze_layers'], cap['freeze_bn']
    device = cap['images'].device
    rep = tf.Report(tag)
    bn_i, head_i = tf._bn_indices(specs), tf._head_indices(specs)
    tr_bn = [i for i in bn_i if i >= N]
    assert sorted(cap['a']) == tr_bn and all(i >= N for i in head_i), 'the plan records exactly the trainable layers'
    assert cap['op_layers'] == [i for i in range(len(specs)) if i >= N]
    P = tf._ref_params(cap, device)
    net = FineTuneNet(P, cap['in_channels'], len(cap['anchors']), cap['K'], dtype=F64, requires_grad=True, device=device,
                      freeze_layers=N, freeze_bn=fbn)
    leaves_y = [t.to(device, F64).requires_grad_(i >= N) for i, t in zip(bn_i, cap['layers'])]
    leaves_up = [t.to(device, F64).requires_grad_(True) for t in cap['up']]
    net.force = {'layers': leaves_y, 'up': leaves_up}
    net.teacher = {'a': [cap['a'][i].to(device, F64) for i in tr_bn]}
    fms = net.feature_maps(cap['images'].to(device, F64), training=True)
    T = net.teacher
    assert len(T['y']) == len(bn_i) and len(T['act']) == len(tr_bn) and len(T['up']) == len(cap['up']) == 2
    for j, i in enumerate(bn_i):
        if i < N:
            rep.add('infer', i, cap['layers'][j], T['y'][j])
        else:
            rep.add('a', i, cap['a'][i], T['act'][tr_bn.index(i)])
            rep.add('y', i, cap['layers'][j], T['y'][j])
    for j in range(2):
        rep.add('up', 'up%d' % j, cap['up'][j], T['up'][j])
    for h, i in enumerate(head_i):
        rep.add('fm', i, cap['fm'][h], fms[h])

    dev = lambda t: t.to(device, F64)
    S = sum((T['y'][bn_i.index(i)] * dev(cap['dy'][i])).sum() for i in tr_bn)
    S = S + sum((u * dev(g)).sum() for u, g in zip(T['up'], cap['dup']))
    S = S + sum((f * dev(g)).sum() for f, g in zip(fms, cap['dfm']))
    params = [t for t in net.trainable() if t.requires_grad]
    ly = [leaves_y[bn_i.index(i)] for i in tr_bn]
    wrt = params + ly + leaves_up
    grads = [g if g is not None else torch.zeros_like(t) for g, t in zip(torch.autograd.grad(S, wrt, allow_unused=True), wrt)]
    gp, gy, gu = grads[:len(params)], grads[len(params):len(params) + len(ly)], grads[len(params) + len(ly):]
    G = tf.unpack(cap['grads'], specs)
    k = nb = 0
    for i, sp in enumerate(specs):
        if i < N:
            continue
        dW, db = gp[k], gp[k + 1]
        if sp.bn:
            dg, dbe = gp[k + 2], gp[k + 3]
            k += 4
            rep.add('dW', i, G[i]['W'], dW)
            rep.add('dgamma', i, G[i]['gamma'], dg)
            rep.add('dbeta', i, G[i]['beta'], dbe)
            stats = None if fbn else net.batch_stats[nb]
            nb += 1
            dz_abs = _dz_abs_sum(net, cap, i, stats, device)
            rep.add('dbias', i, G[i]['b'], db, atol=tf.BOUNDS['dbias'] * max(float(dz_abs.max()), 1e-30))
        else:
            k += 2
            h = head_i.index(i)
            rep.add('head_dW', i, G[i]['W'], dW)
            rep.add('head_db', i, G[i]['b'], db, atol=tf.BOUNDS['head_db'] * max(float(dev(cap['dfm'][h]).abs().sum(dim=(0, 2, 3)).max()), 1e-30))
    for j, i in enumerate(tr_bn):
        rep.add('dact', i, cap['dy'][i], gy[j])
    for j in range(2):
        rep.add('dact', 'up%d' % j, cap['dup'][j], gu[j])
    tf._check_loss(rep, cap)
    return rep


def _dz_abs_sum(net, cap, i, stats, device):
    """Per channel sum of |dz| of trainable BatchNorm layer i in fp64: the floor of the dbias comparison (teacher_forced._dz_abs_sum;
    stats None: frozen statistics, where dz = dy * gamma * rsqrt(moving var + eps) * slope)."""
    a, dy = cap['a'][i].to(device, F64), cap['dy'][i].to(device, F64)
    gamma = net.p[i]['gamma'].detach()[None, :, None, None]
    slope = torch.where(a > 0, 1.0, om.LRELU_ALPHA)
    if stats is None:
        rstd = torch.rsqrt(net.p[i]['var'].detach() + om.BN_EPS)[None, :, None, None]
        return (dy * gamma * rstd * slope).abs().sum(dim=(0, 2, 3))
    mean, var, _ = stats
    rstd = torch.rsqrt(var + om.BN_EPS)[None, :, None, None]
    xhat = (a - mean[None, :, None, None]) * rstd
    g = dy * gamma
    da = rstd * (g - g.mean(dim=(0, 2, 3), keepdim=True) - xhat * (g * xhat).mean(dim=(0, 2, 3), keepdim=True))
    return (da * slope).abs().sum(dim=(0, 2, 3))
