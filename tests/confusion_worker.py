"""Rank process of tests/test_gpu_confusion.py: every rank builds the same shared detection set, feeds its [rank::world] share to
a DetectionEvaluator with class score thresholds and the confusion matrix and merges with metrics.all_gather_evaluator (gloo, so
two ranks can share cuda:0).  Then rank 1 does the same with other thresholds: every rank must get the ValueError.
usage: confusion_worker.py OUT_DIR SEED N K   (RANK / WORLD_SIZE / MASTER_* in the environment)
Writes OUT_DIR/rank<r>.npz, the merged evaluator's matches and result arrays, and OUT_DIR/raised<r>.txt, the error's text."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'object-detection-yolov3_amd'), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                      # noqa: E402
import torch                            # noqa: E402
import torch.distributed as dist       # noqa: E402

THRESHOLDS = [0.5, 0.75]
CUTS = [0.3, 0.45, 0.15]


def feed(ev, dets, gts, batch):
    for b0 in range(0, len(dets), batch):
        d = dets[b0:b0 + batch]
        ev.add_detections([x[0] for x in d], [x[1] for x in d], [x[2] for x in d], gts[b0:b0 + batch], [x[3] for x in d])
    return ev


def main():
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo')
    out_dir, seed, n, K = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    from yolo3 import metrics
    import confusion_reference as cr
    dets, gts = cr.seeded_set(seed, n, K)
    ev = feed(metrics.DetectionEvaluator(K, THRESHOLDS, class_score_thresholds=CUTS[:K], confusion=True), dets[rank::world], gts[rank::world], 3)
    merged = metrics.all_gather_evaluator(ev)
    res = merged.result()
    cls, score, tp = merged.matches()
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), cls=cls, score=score, tp_masks=tp, num_images=merged.num_images,
             counts=merged.image_counts().cpu().numpy(), confusion=res['confusion'], confusion_op=res['confusion_op'],
             cuts=res['class_score_thresholds'], ap=res['ap'], tp=res['tp'], fp=res['fp'], npos=res['npos'])
    other = CUTS[:K] if rank == 0 else [c + 0.01 for c in CUTS[:K]]
    ev = feed(metrics.DetectionEvaluator(K, THRESHOLDS, class_score_thresholds=other, confusion=True), dets[rank:rank + 1], gts[rank:rank + 1], 1)
    try:
        metrics.all_gather_evaluator(ev)
    except ValueError as e:
        open(os.path.join(out_dir, 'raised%d.txt' % rank), 'w').write(str(e))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
