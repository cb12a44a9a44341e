"""Cost of fine-tuning.

    python tools/finetune_cost.py kernels [launches]    y3_bn_frozen_bwd beside y3_bn_bwd_stats + y3_bn_bwd_apply on the same tensors, the
                                                        8 x 52^2 x 256 and 8 x 13^2 x 1024 layers of the 416^2 step; run it under
                                                        `rocprofv3 --kernel-trace --stats --` for the times
    python tools/finetune_cost.py steps [steps] [rounds]    train_step at 8 x 416^2 for default / freeze_bn / freeze_layers 52 / both,
                                                            alternated in one process
"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + '/object-detection-yolov3_amd')
import numpy as np   # noqa: E402
import torch         # noqa: E402
import bench         # noqa: E402
from yolo3 import _hip   # noqa: E402
from yolo3._hip import lib, check   # noqa: E402
from yolo3.model import YoloV3, BACKBONE_LAYERS   # noqa: E402


def kernels(launches):
    st = torch.cuda.current_stream().cuda_stream
    for n, hw, c in ((8, 52, 256), (8, 13, 1024)):
        m = n * hw * hw
        dy, a, dz = (torch.randn(m * c, device='cuda') for _ in range(3))
        per = lambda: torch.rand(c, device='cuda') + 0.5
        gamma, mean, rstd, scale, var = per(), per(), per(), per(), per()
        out = torch.zeros(3, c, device='cuda')
        coef = torch.zeros(3 * c, device='cuda')
        ws = torch.zeros(max(int(lib.y3_bn_bwd_workspace(m, c)), int(lib.y3_bn_frozen_bwd_workspace(m, c))), dtype=torch.uint8, device='cuda')
        v = lambda t: _hip.view(t, n, hw, hw, c)
        print('%d x %d^2 x %d: %.1f MB per tensor; pair reads 4 and writes 1, frozen reads 2 and writes 1' % (n, hw, c, m * c * 4 / 1e6))
        for _ in range(launches):
            check(lib.y3_bn_bwd_stats(v(dy), v(a), None, 0, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), 0.2, out[0].data_ptr(), out[1].data_ptr(),
                                      out[2].data_ptr(), coef.data_ptr(), ws.data_ptr(), ws.numel(), st), 'bn_bwd_stats')
            check(lib.y3_bn_bwd_apply(v(dy), v(a), coef.data_ptr(), 0.2, v(dz), st), 'bn_bwd_apply')
            check(lib.y3_bn_frozen_bwd(v(dy), v(a), None, 0, scale.data_ptr(), mean.data_ptr(), var.data_ptr(), 1e-3, 0.2, v(dz), out[0].data_ptr(),
                                       out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel(), st), 'bn_frozen_bwd')
        torch.cuda.synchronize()


def steps(n, rounds):
    images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    gts = [torch.from_numpy(x).cuda() for x in bench.synth_labels(np.random.default_rng(3), 8)]
    models = {name: YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1, **kw)
              for name, kw in (('default', {}), ('freeze_bn', dict(freeze_bn=True)), ('freeze52', dict(freeze_layers=BACKBONE_LAYERS)),
                               ('both', dict(freeze_layers=BACKBONE_LAYERS, freeze_bn=True)))}
    for name, y in models.items():
        for _ in range(5):
            y.train_step((images, gts))
        plan = y._plan(8, True)
        print('%-9s: %d forward + %d backward launches' % (name, len(plan.fwd), sum(1 for e in plan.bwd if not isinstance(e[0], str) or e[0] == 'side_call')))
    for r in range(rounds):
        for name, y in models.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                loss = y.train_step((images, gts))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / n
            print('round %d %-9s: %.3f ms per step, %.1f images/s over %d steps, loss %.6f' % (r, name, dt * 1e3, 8 / dt, n, float(loss)), flush=True)


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'steps'
    if mode == 'kernels':
        kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
    else:
        steps(int(sys.argv[2]) if len(sys.argv) > 2 else 40, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
