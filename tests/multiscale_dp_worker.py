"""Rank process of tests/test_gpu_multiscale.py: two data-parallel training steps of a multi-scale model (train_sizes), the
first at IMG, the second at IMG2, on the gloo backend so that two ranks can share cuda:0, and a dump of what each step left behind.
usage: multiscale_dp_worker.py OUT_DIR IMG IMG2 N_PER_RANK SEED   (RANK / WORLD_SIZE / MASTER_* in the environment)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'object-detection-yolov3_amd'), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                      # noqa: E402
import torch                            # noqa: E402
import torch.distributed as dist       # noqa: E402


def make_cases(sizes, n_total, seed):
    """The full global batch at every size (every rank builds the same ones and takes its slice)."""
    from dp_worker import make_case
    cases = [make_case(s, n_total, seed + i) for i, s in enumerate(sizes)]
    anchors, K, params = cases[0][:3]
    return anchors, K, params, [(c[3], c[4]) for c in cases]


def main():
    out_dir, img, img2, n, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    from yolo3 import streams
    streams.reserve()
    dist.init_process_group('gloo')
    from yolo3.model import YoloV3
    from yolo3.parallel import DataParallel
    anchors, K, params, batches = make_cases((img, img2), n * world, seed)
    yolo = YoloV3(n * world, [img, img, 3], K, anchors, learning_rate=1e-3, train_sizes=[(img2, img2)])
    if rank == 0:
        yolo.set_weights(params)        # the other ranks keep their own random init until the broadcast
    strategy = DataParallel(bucket_mb=8.0)
    strategy.attach(yolo)
    strategy.broadcast_parameters(yolo.params, yolo.moving)
    yolo._refresh_transposed()
    sl = slice(rank * n, (rank + 1) * n)
    out = dict(buckets=len(strategy.buckets))
    for i, (images, gts) in enumerate(batches):
        loss = yolo.dist_train_step(strategy, (images[sl].cuda(), [torch.from_numpy(x[sl]).cuda() for x in gts]))
        torch.cuda.synchronize()
        out['grads%d' % i] = yolo.grads.cpu().numpy()
        out['params%d' % i] = yolo.params.cpu().numpy()
        out['loss%d' % i] = float(loss)
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), **out)
    strategy.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
