"""Cost of the opt-in optimisers.

    python tools/optimizer_cost.py kernels [launches]    every y3_optim_step instantiation at the real arena sizes (plain and SPP) with
                                                         the model's 75 / 76 decay ranges, beside y3_adam_step / y3_adam_step_ema on the
                                                         same arenas (optim_kernel<3, false, false> and <3, true, false>: Adam is the
                                                         fourth kind of the same template, with the decay machinery compiled out); run
                                                         it under `rocprofv3 --kernel-trace --stats --` for the times
    python tools/optimizer_cost.py steps [steps] [rounds]    train_step at 8 x 416^2 for adam, adamw and sgd, alternated in one process
"""
import ctypes
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
from yolo3.model import YoloV3, build_layer_specs, decay_ranges   # noqa: E402


def kernels(launches):
    st = torch.cuda.current_stream().cuda_stream
    for spp in (False, True):
        specs, count, _, mstride = build_layer_specs(3, len(bench.ANCHORS), 2, spp)
        ranges = decay_ranges(specs)
        table = (ctypes.c_longlong * (2 * len(ranges)))(*[v for r in ranges for v in r])
        z = lambda n: torch.zeros(n, device='cuda')
        p, g, m, v, e, mv, emv = z(count), z(count), z(count), z(count), z(count), z(2 * mstride), z(2 * mstride)
        g.normal_()
        hyper, omd, s = torch.tensor([1e-4, 5e-8], device='cuda'), torch.tensor([1e-4], device='cuda'), torch.tensor([0.5], device='cuda')
        print('spp %d: arena %d floats (%.1f MB per stream), %d decay ranges, moving %d floats' % (spp, count, count * 4 / 1e6, len(ranges), 2 * mstride))
        for _ in range(launches):
            check(lib.y3_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), count, hyper.data_ptr(), 0.9, 0.999, 1e-7, st), 'adam')
            check(lib.y3_adam_step_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), count, hyper.data_ptr(), 0.9, 0.999, 1e-7, e.data_ptr(),
                                       mv.data_ptr(), emv.data_ptr(), 2 * mstride, omd.data_ptr(), st), 'adam_ema')
            for kind in (_hip.OPT_SGD, _hip.OPT_SGD_NESTEROV, _hip.OPT_ADAMW):
                for ema in (False, True):
                    for scaled in (False, True):
                        d = _hip.OptimDesc()
                        d.kind, d.param, d.grad, d.m, d.count, d.hyper_dev = kind, p.data_ptr(), g.data_ptr(), m.data_ptr(), count, hyper.data_ptr()
                        d.v = v.data_ptr() if kind == _hip.OPT_ADAMW else None
                        d.momentum, d.weight_decay, d.beta1, d.beta2, d.eps = 0.9, 5e-4, 0.9, 0.999, 1e-7
                        d.decay_ranges_host, d.n_ranges = table, len(ranges)
                        if ema:
                            d.ema_param, d.moving, d.ema_moving, d.moving_count, d.omd_dev = e.data_ptr(), mv.data_ptr(), emv.data_ptr(), 2 * mstride, omd.data_ptr()
                        if scaled:
                            d.scale_dev = s.data_ptr()
                        check(lib.y3_optim_step(ctypes.byref(d), st), 'optim')
        torch.cuda.synchronize()


def steps(n, rounds):
    images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
    gts = [torch.from_numpy(x).cuda() for x in bench.synth_labels(np.random.default_rng(3), 8)]
    models = {name: YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1, **kw)
              for name, kw in (('adam', {}), ('adamw', dict(optimizer='adamw', weight_decay=5e-4)), ('sgd', dict(optimizer='sgd', weight_decay=5e-4)))}
    for y in models.values():
        for _ in range(5):
            y.train_step((images, gts))
    for r in range(rounds):
        for name, y in models.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                loss = y.train_step((images, gts))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / n
            print('round %d %-5s: %.3f ms per step, %.1f images/s over %d steps, loss %.6f' % (r, name, dt * 1e3, 8 / dt, n, float(loss)), flush=True)


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'steps'
    if mode == 'kernels':
        kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
    else:
        steps(int(sys.argv[2]) if len(sys.argv) > 2 else 40, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
