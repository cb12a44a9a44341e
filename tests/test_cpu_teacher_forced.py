"""The teacher-forced checker of the training step (tests/teacher_forced.py) on the CPU: a capture built from the fp32 oracle, in
the format capture_step() reads from the GPU, passes it; four targeted corruptions of that capture each fail it.  This is what
shows that its bounds are sharp enough to see a 1e-3 error in one tensor, a concat slice off by one channel, a stale weight copy."""
import copy

import numpy as np
import pytest
import torch

from oracle import model as om
import teacher_forced as tf

IMG, N, LR = 64, 2, 1e-3
ANCHORS = [(64, 384), (384, 64)]
K = 2
W_LAYER = 20          # a 3x3 layer of the 256-channel feature block
STALE_LAYER = 30      # a 3x3 layer of the 512-channel feature block (K per row a multiple of 16 in both copies)


def _specs():
    from yolo3.model import build_layer_specs
    return build_layer_specs(3, len(ANCHORS), K)


def _pack(layers, specs, floats):
    arena = torch.zeros(floats, dtype=torch.float32)
    for sp, d in zip(specs, layers):
        dst = tf.unpack(arena, [sp], padded=True)[0]
        dst['W'][:, :, :sp.cin] = torch.as_tensor(np.asarray(d['W'])).float()
        for k in ('b', 'gamma', 'beta'):
            if k in dst:
                dst[k].copy_(torch.as_tensor(np.asarray(d[k])).float())
    return arena


def _pack_moving(layers, specs, stride):
    mov = torch.zeros(2 * stride, dtype=torch.float32)
    for (m, v), d in zip(tf.unpack_moving(mov, specs, stride), [d for d, sp in zip(layers, specs) if sp.bn]):
        m.copy_(torch.as_tensor(np.asarray(d['mean'])).float())
        v.copy_(torch.as_tensor(np.asarray(d['var'])).float())
    return mov


def _layers(arena, moving, specs, stride):
    out = [{k: v.clone() for k, v in d.items()} for d in tf.unpack(arena, specs)]
    for d, (m, v) in zip([d for d, sp in zip(out, specs) if sp.bn], tf.unpack_moving(moving, specs, stride)):
        d['mean'], d['var'] = m.clone(), v.clone()
    return out


def _forward(layers, images, gts, specs, backward):
    """fp32 oracle step with autograd: the tensors capture_step() reads from the plan's buffers."""
    net = om.Net(layers, 3, len(ANCHORS), K, dtype=torch.float32, requires_grad=backward)
    net.teacher = {}                  # record only
    with torch.set_grad_enabled(backward):
        fms = net.feature_maps(images, training=True)
    T = net.teacher
    cap = dict(a=[t.clone() for t in T['act']], y=[t.detach().clone() for t in T['y']], up=[t.detach().clone() for t in T['up']],
               fm=[f.detach().clone() for f in fms],
               mean=[m.clone() for m, _, _ in net.batch_stats], rstd=[torch.rsqrt(v + om.BN_EPS) for _, v, _ in net.batch_stats])
    if backward:
        for t in T['y'] + T['up'] + list(fms):
            t.retain_grad()
        parts = [0.0] * 4
        for fm, gt in zip(fms, gts):
            parts = [p + q for p, q in zip(parts, om.loss_layer(fm, gt, (IMG, IMG, 3), ANCHORS, K))]
        (sum(parts) / float(N)).backward()
        cap.update(dy=[t.grad.clone() for t in T['y']], dup=[t.grad.clone() for t in T['up']], dfm=[f.grad.clone() for f in fms],
                   loss4=torch.stack([p.detach() for p in parts]), grads=[p.grad.clone() for p in net.trainable()])
    return net, cap


def _moving_after(moving, net, specs, stride):
    out = moving.clone()
    for (m, v), (mean, var, cnt) in zip(tf.unpack_moving(out, specs, stride), net.batch_stats):
        m.mul_(om.BN_MOMENTUM).add_(mean * (1 - om.BN_MOMENTUM))
        v.mul_(om.BN_MOMENTUM).add_(var * (cnt / max(cnt - 1.0, 1.0)) * (1 - om.BN_MOMENTUM))
    return out


def _adam32(p, g, m, v, lr_t):
    """The arithmetic of y3_adam_step in fp32 (fp32 hyper-parameters, 1 - b computed in fp32)."""
    f = np.float32
    o1, o2, eps = float(f(1) - f(0.9)), float(f(1) - f(0.999)), float(f(1e-7))
    m = m + (g - m) * o1
    v = v + (g * g - v) * o2
    return p - (m * lr_t) / (torch.sqrt(v) + eps), m, v


def _derived(params, specs):
    pt = torch.zeros_like(params)
    for i, w in tf.transposed(params, specs).items():
        pt[specs[i].w_off:specs[i].w_off + w.numel()] = w.reshape(-1)
    planes = torch.zeros(3 * params.numel(), dtype=torch.bfloat16)
    planes_t = torch.zeros_like(planes)
    keras, trans = tf.planes_of(params, specs)
    for arena, d in ((planes, keras), (planes_t, trans)):
        for i, w in d.items():
            arena[3 * specs[i].w_off:3 * specs[i].w_off + w.numel()] = w
    return pt, planes, planes_t


@pytest.fixture(scope='module')
def fake():
    """Two steps of the fp32 oracle at 64 x 2, as capture_step() would record them from the GPU."""
    from test_gpu_kernels import _labels
    specs, floats, _, stride = _specs()
    params = om.init_params(3, len(ANCHORS), K, seed=11)
    g = torch.Generator().manual_seed(11)
    images = torch.randn(N, 3, IMG, IMG, generator=g)
    gts = [torch.from_numpy(x).float() for x in _labels(np.random.default_rng(11), N, IMG, ANCHORS, K, per_image=3)]
    p0, mv0 = _pack(params, specs, floats), _pack_moving(params, specs, stride)
    net, c = _forward(_layers(p0, mv0, specs, stride), images, gts, specs, True)
    grads = _pack([dict(W=c['grads'][k], b=c['grads'][k + 1], **(dict(gamma=c['grads'][k + 2], beta=c['grads'][k + 3]) if sp.bn else {}))
                   for sp, k in zip(specs, np.cumsum([0] + [4 if sp.bn else 2 for sp in specs])[:-1])], specs, floats)
    lr_t = float(np.float32(LR * np.sqrt(1 - 0.999) / (1 - 0.9)))
    zeros = torch.zeros(floats)
    p1, m1, v1 = _adam32(p0, grads, zeros, zeros, lr_t)
    mv1 = _moving_after(mv0, net, specs, stride)
    pt, planes, planes_t = _derived(p1, specs)
    base = dict(specs=specs, moving_stride=stride, in_channels=3, anchors=ANCHORS, K=K, img_size=(IMG, IMG, 3), gbs=float(N),
                images=images, gts=gts, slices=[25, 42])
    cap1 = dict(base, pre=dict(params=p0, moving=mv0, m=zeros, v=zeros), grads=grads, lr_t=lr_t,
                post=dict(params=p1, moving=mv1, m=m1, v=v1, params_t=pt, planes=planes, planes_t=planes_t),
                **{k: c[k] for k in ('a', 'y', 'dy', 'mean', 'rstd', 'up', 'dup', 'fm', 'dfm', 'loss4')})

    def step2(stale_layer=None):
        layers = _layers(p1, mv1, specs, stride)
        if stale_layer is not None:       # this layer's forward reads the weights from before the Adam step
            layers[stale_layer]['W'] = tf.unpack(p0, specs)[stale_layer]['W'].clone()
        net2, c2 = _forward(layers, images, gts, specs, False)
        return dict(base, pre=dict(params=p1, moving=mv1, m=m1, v=v1), post=dict(moving=_moving_after(mv1, net2, specs, stride)), **c2)
    return cap1, step2, p0


def _kinds(rep):
    return {f.split(' layer ')[0] + ' ' + f.split(' layer ')[1].split(':')[0] for f in rep.failures}


def test_checker_passes_the_fp32_oracle(fake):
    cap1, step2, _ = fake
    rep = tf.check_step(cap1, tag='cpu-fake step 1')
    rep.print()
    assert not rep.failures, rep.failures[:10]
    expected = {'a', 'mean', 'rstd', 'moving', 'y', 'up', 'fm', 'dW', 'dgamma', 'dbeta', 'dbias', 'dact', 'head_dW', 'head_db', 'dfm',
                'loss4', 'adam', 'pad', 'params_t', 'planes', 'planes_t', 'ignore'}
    assert expected <= set(rep.worst), expected - set(rep.worst)
    rep2 = tf.check_step(step2(), forward_only=True, tag='cpu-fake step 2')
    rep2.print()
    assert not rep2.failures, rep2.failures[:10]


def test_checker_sees_one_kernel_gradient_off_by_1e_3(fake):
    cap = copy.copy(fake[0])
    cap['grads'] = cap['grads'].clone()
    tf.unpack(cap['grads'], cap['specs'])[W_LAYER]['W'].mul_(1 + 1e-3)
    rep = tf.check_step(cap, tag='dW x (1 + 1e-3)')
    assert 'dW %d' % W_LAYER in _kinds(rep), rep.failures[:10]


def test_checker_sees_a_concat_slice_gradient_shifted_by_one_channel(fake):
    cap = copy.copy(fake[0])
    j = cap['slices'][1]                          # route2: the second half of the 1024-channel concat
    assert cap['y'][j].shape[1] == 512
    cap['dy'] = list(cap['dy'])
    cap['dy'][j] = torch.roll(cap['dy'][j], 1, dims=1)
    rep = tf.check_step(cap, tag='concat slice shifted')
    layer = [i for i, sp in enumerate(cap['specs']) if sp.bn][j]
    assert 'dact %d' % layer in _kinds(rep), rep.failures[:10]


def test_checker_sees_a_forward_with_the_weights_from_before_the_step(fake):
    rep = tf.check_step(fake[1](stale_layer=STALE_LAYER), forward_only=True, tag='stale forward at step 2')
    assert 'a %d' % STALE_LAYER in _kinds(rep), rep.failures[:10]


def test_checker_sees_stale_planes_of_one_layer(fake):
    cap, _, p0 = fake
    cap = copy.copy(cap)
    post = dict(cap['post'])
    post['planes_t'] = post['planes_t'].clone()
    sp = cap['specs'][STALE_LAYER]
    w = tf.planes_of(p0, cap['specs'])[1][STALE_LAYER]
    post['planes_t'][3 * sp.w_off:3 * sp.w_off + w.numel()] = w
    cap['post'] = post
    rep = tf.check_step(cap, tag='stale planes_t')
    assert _kinds(rep) == {'planes_t %d' % STALE_LAYER}, rep.failures[:10]
