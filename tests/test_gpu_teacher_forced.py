"""Every launch of the real training step and of the fp32 inference plan against fp64, teacher-forced (tests/teacher_forced.py):
each layer's reference is computed from the GPU's own inputs to that layer, so errors do not compound and every tensor is held to
roughly its per-kernel tolerance -- where test_train_step_matches_oracle can only make a 1e-2-class statement about the wiring.
The fp64 reference runs on the GPU (torch, fp64 convolutions), over the whole batch.  Each case prints the worst err / bound
ratio of every quantity kind and the layer it occurs in."""
import numpy as np
import pytest
import torch

import teacher_forced as tf

pytestmark = pytest.mark.gpu


def _check(rep):
    rep.print()
    assert not rep.failures, '%d failures, first: %s' % (len(rep.failures), rep.failures[:8])


def _two_steps(yolo, images, gts, tag):
    cap = tf.capture_step(yolo, images, gts)
    assert cap['slices'] == [25, 42]          # route1 / route2 are written into the concat buffers (test_cpu_teacher_forced: 'slices')
    _check(tf.check_step(cap, tag=tag + ' step 1'))
    del cap
    # step 2: the forward reads the weights the Adam step wrote (params_t / planes_t / params refreshed by _refresh_transposed)
    cap = tf.capture_step(yolo, images, gts)
    _check(tf.check_step(cap, forward_only=True, tag=tag + ' step 2'))


# (320, 8): of the (image side, batch) pairs of the plan-form envelope (tests/plan_forms.py) whose oracle costs no more than (416, 8)'s,
# the one whose step runs the most forward / data-gradient plan forms that no other shape list of the suite reaches but
# test_gpu_plan_forms.py (plan_forms.step_classes; test_cpu_plan_forms.py prints the table: 9 at (320, 8), 6 at (320, 4) and (512, 4),
# 3 at (416, 2) / (416, 4)).  It is also the second training geometry of the stride-2 merged data gradient, the BatchNorm-backward
# plan and the kernel gradient, which have no plan query to enumerate their forms with.
@pytest.mark.parametrize('img,n,arith', [(96, 4, 'f32'), (96, 4, 'x3'), (96, 4, 'x3-all'), (416, 8, 'f32'), (416, 8, 'x3'), (320, 8, 'f32'), (320, 8, 'x3')])
def test_train_step_layers_teacher_forced(img, n, arith):
    """(416, 8) is the benchmarked step; 'x3-all' also puts the x3 kernels on the 1x1 layers and the 64-channel stride-2 data gradient."""
    from test_gpu_model import _setup
    om, params, yolo, images, gts = _setup(img, n, 11, False, conv_arithmetic=arith)
    plan = yolo._plan(n, True)
    if arith == 'f32':
        assert not (plan.x3_fwd or plan.x3_dgrad or plan.x3_wgrad) and yolo.planes is None
    else:
        assert plan.x3_fwd and plan.x3_dgrad and plan.x3_wgrad
        if arith == 'x3-all':
            assert any(yolo.specs[i].k == 1 for i in plan.x3_fwd) and any(yolo.specs[i].s == 2 and yolo.specs[i].cin_pad == 64 for i in plan.x3_dgrad)
    _two_steps(yolo, images, gts, '%dx%d %s' % (img, n, arith))


def test_train_step_layers_teacher_forced_nonsquare_grayscale_three_anchors():
    """The model of test_nonsquare_grayscale_three_anchors: 96 x 160, one input channel (padded to 4), three anchors and classes."""
    from oracle import model as om
    from yolo3.model import YoloV3
    from yolo3.imagereader import format_boxes
    anchors, K3, H, W, n = [(32, 32), (128, 128), (256, 256)], 3, 96, 160, 2
    yolo = YoloV3(n, [H, W, 1], K3, conv_arithmetic='x3')
    yolo.set_weights(om.init_params(1, 3, K3, seed=22))
    g = torch.Generator().manual_seed(21)
    images = torch.randn(n, 1, H, W, generator=g)
    rng = np.random.default_rng(22)
    labs = []
    for _ in range(n):
        wh = rng.integers(20, 60, (2, 2))
        xy = np.stack([rng.integers(0, W - wh[:, 0]), rng.integers(0, H - wh[:, 1])], 1)
        labs.append(format_boxes(np.concatenate([xy, wh, rng.integers(0, K3, (2, 1))], 1).astype(np.int32), (H, W, 1), anchors, K3))
    gts = [np.stack([l[s] for l in labs]) for s in range(3)]
    _two_steps(yolo, images, gts, '96x160 C1 x3')


@pytest.mark.parametrize('arith', ['f32', 'x3'])
@pytest.mark.parametrize('img,n', [(416, 8), (608, 2), (512, 4)])      # (512, 4): more otherwise-unreached forward plan forms than (608, 4) (2 against 1)
def test_inference_layers_teacher_forced(img, n, arith):
    """predict() on the fp32 plan: folded BatchNorm, the fused epilogue with the residual, the x3 forward; randomised BatchNorm."""
    from test_gpu_model import _setup
    om, params, yolo, images, _ = _setup(img, n, 7, True, conv_arithmetic=arith)
    _check(tf.check_inference(yolo, images, params, tag='infer %dx%d %s' % (img, n, arith)))
