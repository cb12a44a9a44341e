"""Cost of the weight EMA: the bench.py training step at batch 8 x 416^2, host-launched, with and without
ema_decay.  python tools/ema_cost.py [ema_decay (0 = off)] [steps]
Under `rocprofv3 --kernel-trace --stats -- python tools/ema_cost.py ...` the stats file gives y3_adam_step's kernel against y3_adam_step_ema's
(optim_kernel<3, false, false> against optim_kernel<3, true, false>, csrc/optim.hip)."""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + '/object-detection-yolov3_amd')
import numpy as np   # noqa: E402
import torch         # noqa: E402
import bench         # noqa: E402
from yolo3.model import YoloV3   # noqa: E402

decay = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
yolo = YoloV3(8, [416, 416, 3], 2, bench.ANCHORS, learning_rate=1e-4, seed=1, ema_decay=decay or None)
images = torch.randn(8, 3, 416, 416, generator=torch.Generator().manual_seed(100)).cuda()
gts = [torch.from_numpy(x).cuda() for x in bench.synth_labels(np.random.default_rng(3), 8)]
for _ in range(5):
    loss = yolo.train_step((images, gts))
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(steps):
    loss = yolo.train_step((images, gts))
torch.cuda.synchronize()
dt = (time.perf_counter() - t) / steps
print('ema_decay %g: %.3f ms per step, %.1f images/s over %d steps, loss %.6f, arena %d floats, moving %d floats'
      % (decay, dt * 1e3, 8 / dt, steps, float(loss), yolo.arena_floats, yolo.moving.numel()))
