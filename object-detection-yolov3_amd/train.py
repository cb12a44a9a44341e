#!/usr/bin/env python3
"""train.py -- YOLOv3 training loop on MI355X.  Reference: train.py:28-267 (same flags and semantics).

    python train.py --train_database D/train-x.lmdb --test_database D/test-x.lmdb --output_dir OUT
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...   # 8 GPUs

Kept from the reference: anchors [(64,384),(384,64)] (train.py:33), READER_COUNT = 3 reader processes per GPU (:16),
global batch = batch_size x replicas (:41), Adam warm-up at lr/10 for min(1000, N) steps of epoch 0 (:107-113), the
"step > N: break" loop bound (N+1 steps, Q16), NaN-loss abort (:124-125), per-step metric print, test loop of
image_count/batch_size(+1) batches (:76,:144), test_loss.csv (:170-173), best checkpoint on a new minimum (:178-182),
early stopping with CONVERGENCE_TOLERANCE 1e-4 (:185-197), final export of the best checkpoint (:208-221).
Added (opt-in, off by default): --test_map 1 runs a test-set mAP pass after every test epoch (<out>/test_map.csv), and
--model_selection map50 / map50_95 checkpoints and stops early on that mAP instead of the test loss, and
--ema_decay D keeps an exponential moving average of the weights whose copy the test loss, the mAP pass and the checkpoint
(hence the export) use, and --box_loss giou / diou / ciou (with --box_loss_weight W) trains and tests with an
IoU-family box-regression loss in place of the reference's xy + wh terms.  The scalar CSVs keep their columns:
with an IoU loss `loss_xy` carries the box term and `loss_wh` is 0.  The weight files do not record the choice.
--accumulate_steps N sums the gradients of N consecutive batches into one optimiser step (effective batch = batch_size x
replicas x N; a "step" of the loop, of --test_every_n_steps and of train.csv stays one batch) and --grad_clip_norm X bounds the
global L2 norm of the (averaged) gradient at X; with either, <scalars>/grad_norm.csv gets one row per optimiser
step: the train.csv step that completed it, the norm before clipping and the factor applied to the summed gradient.
--multiscale_min A --multiscale_max B (with --augmentation_device gpu) trains at a changing square input size: every
--multiscale_period batches (default 10) a side is drawn from the multiples of 32 in [A, B] as a pure function of
--multiscale_seed and the batch count, the same on every rank; the batch is augmented straight to that size and its labels are
built on the device at it.  <scalars>/train_size.csv gets one row per step.  The test reader, the test loss, the
mAP pass, model selection, the checkpoint and the export stay at the size the images are stored at.
--mosaic_prob P (with --augmentation_device gpu; 0 = off) turns each training image, with probability P, into a mosaic of itself
and three other images of its batch, composed on the device after the augmentation; the draws are a pure function
of --mosaic_seed, the rank and the batch count, and a box stays when at least --mosaic_min_visible of its area is still visible.
Composes with the --multiscale_* flags; the test reader, the mAP pass, the checkpoint and the export are untouched.
--affine_prob P (with --augmentation_device gpu; 0 = off) warps each training image, with probability P, through a random rotation
(+-affine_degrees), shear (+-affine_shear degrees per axis), gain (1 +- affine_scale) and translation (+-affine_translate of the
side) on the device, after the augmentation and the mosaic; pixels from outside the image get --affine_fill, the
draws are a pure function of --affine_seed, the rank, the batch count and the image, and a box stays when at least
--affine_min_visible of its transformed area is inside the image.  Composes with --multiscale_* and --mosaic_prob.
--photo_prob P (with --augmentation_device gpu; 0 = off) sends each training image, with probability P, through a random colour
matrix (hue rotation by +-photo_hue turns and saturation gain 1 +- photo_saturation of the YIQ chroma plane, value gain 1 +-
photo_value), a clamp to [0, photo_white] and a tone curve with exponent 2^(+-photo_gamma); --mixup_prob P (0 = off) blends each
image, with probability P, with another image of its batch, lambda uniform in 0.5 +- mixup_spread, and gives it the boxes of both.
Both are one elementwise pass on the device after the warp, right before the z-score; the draws are pure functions
of --photo_seed / --mixup_seed, the rank, the batch count and the image.  A brightness gain alone would be cancelled by the
per-image z-score; that is why there is no such flag.
--ignore_mask truth (with --ignore_thresh T, default 0.5, and --ignore_max_boxes N, default 1024) leaves a prediction without an
object out of the objectness loss when it overlaps a ground-truth box of its own image with IoU >= T, the rule of the paper, in
place of the reference's mask; training and test loss use the same mask.  <scalars>/ignored.csv gets one row per
optimiser step: the predictions left out in that batch and the longest per-image box list (a warning once if it exceeds N).
--focal_gamma G (with --focal_alpha A, default 0 = no balancing factor, and --focal_terms obj / class / both, default both) gives the
objectness and / or class term the focal form w m^G ce of Lin et al., and --label_smoothing E trains the class term against the
labels g (1 - E) + E / 2; training and test loss use the same terms, the scalar CSVs keep their columns, and the
weight files record the setting.  Test losses of runs with different settings are not comparable.
--spp 1 trains the YOLOv3-SPP variant of the network: a 5 / 9 / 13 max-pool pyramid and one more 1x1 layer in the block of the
coarsest scale.  Checkpoint, EMA export and model selection carry it; the weight files record it, and inference.py,
inference_tiled.py and evaluate.py take it from there.
--optimizer sgd (with --momentum M, default 0.9, and --nesterov 1) or adamw trains with SGD-momentum or AdamW in place of the
reference's Adam, and --weight_decay WD decays the convolution kernels only: coupled L2 for sgd, decoupled for adamw (DESIGN
§3.19).  --lr_schedule constant / cosine / step (with --lr_warmup_steps W, --lr_warmup_start_factor S, --lr_total_steps T,
--lr_final_factor F, --lr_milestones A B ..., --lr_gamma G) replaces the epoch-0 rule by learning_rate x a factor of the optimiser
step: epoch 0 then has the full size, and <scalars>/lr.csv gets one row per optimiser step.  The weight files record the optimiser.
--anchors W,H [W,H ...], --anchors_file FILE (written by find_anchor_sizes.py --metric iou --output) or --auto_anchors K replace the
reference's pair of anchors; at most one of the three.  --auto_anchors K fits K anchors to the boxes of the training
database before the readers start (yolo3.anchors.fit_anchors; --auto_anchors_evolve, --auto_anchors_seed), on the host or, with
--auto_anchors_device gpu, in a child process that runs find_anchor_sizes.py --device gpu (this process must not touch the GPU before
its readers are forked); every rank computes the same anchors, rank 0 writes <out>/anchors.json.  The weight files carry the anchors.
--anchor_assignment scale, or --anchor_masks "6,7,8 3,4,5 0,1,2" (the anchors of stride 32, 16, 8; implies scale), gives each anchor
to ONE scale as YOLOv3 / Darknet do: a box is a positive only on the scale that owns its best anchor and head s has
A_s (5 + K) channels; needs at least 3 anchors; rank 0 writes <out>/anchor_scales.json, the weight files carry the table.  The default
(all) is the reference's network, every anchor on every scale.
Changed: MirroredStrategy -> one process per GPU + RCCL (yolo3.parallel); TF checkpoint / SavedModel -> .npz weight
files (<out>/checkpoint/ckpt.npz, <out>/saved_model/yolov3.npz); TensorBoard event files -> <out>/scalars-<ts>/{train,test}.csv.
"""
import argparse
import contextlib
import datetime
import os
import time

import numpy as np

READER_COUNT = 3  # per gpu (train.py:16)
CONVERGENCE_TOLERANCE = 1e-4  # train.py:185


def best_epoch_of(test_loss, tolerance=CONVERGENCE_TOLERANCE):
    """train.py:185-192: the FIRST epoch whose test loss is within `tolerance` of the minimum."""
    error_from_best = np.abs(np.asarray(test_loss) - np.min(test_loss))
    error_from_best[error_from_best < tolerance] = 0
    return int(np.where(error_from_best == 0)[0][0])


def should_stop(test_loss, early_stopping_count, tolerance=CONVERGENCE_TOLERANCE):
    """train.py:193-197: stop once more than `early_stopping_count` epochs have passed since the best one."""
    return len(test_loss) - best_epoch_of(test_loss, tolerance) > early_stopping_count


def is_new_minimum(test_loss):
    """train.py:178: checkpoint when the newest test loss is the (first) minimum of the series."""
    return (len(test_loss) - 1) == int(np.argmin(test_loss))


def best_epoch_of_max(scores, tolerance=CONVERGENCE_TOLERANCE):
    """best_epoch_of for a score where higher is better (mAP): the FIRST epoch within `tolerance` of the maximum.  NaN
    epochs (no ground truth) never count."""
    v = np.asarray(scores, np.float64)
    if np.all(np.isnan(v)):
        raise ValueError('no epoch has a finite score')
    with np.errstate(invalid='ignore'):
        error_from_best = np.abs(v - np.nanmax(v))
        error_from_best[error_from_best < tolerance] = 0
    return int(np.where(error_from_best == 0)[0][0])


def should_stop_max(scores, early_stopping_count, tolerance=CONVERGENCE_TOLERANCE):
    """should_stop for a higher-is-better score: more than `early_stopping_count` epochs since the best one."""
    return len(scores) - best_epoch_of_max(scores, tolerance) > early_stopping_count


def is_new_maximum(scores):
    """is_new_minimum for a higher-is-better score: the newest value is the (first) maximum; a NaN never is."""
    v = np.asarray(scores, np.float64)
    return not np.isnan(v[-1]) and (len(v) - 1) == int(np.argmax(np.where(np.isnan(v), -np.inf, v)))


MODEL_SELECTIONS = ('loss', 'map50', 'map50_95')
# = yolo3.bbox_utils.NMS_METHODS, spelled out so that building the parser does not load the HIP library
TEST_MAP_NMS_METHODS = ('hard', 'diou', 'soft-linear', 'soft-gaussian')
# yolo3.model.BOX_LOSSES, restated so that --help needs no device library
BOX_LOSSES = ('mse', 'giou', 'diou', 'ciou')
IGNORE_MASKS = ('reference', 'truth')
FOCAL_TERMS = ('obj', 'class', 'both')
OPTIMIZERS = ('adam', 'adamw', 'sgd')
LR_SCHEDULES = ('reference', 'constant', 'cosine', 'step')      # 'reference' = the epoch-0 rule of the reference's loop


def effective_test_map(test_map, model_selection):
    """--test_map as it takes effect: a mAP model selection needs the mAP pass, so it implies --test_map 1."""
    if model_selection not in MODEL_SELECTIONS:
        raise ValueError('model_selection must be one of {}, got {!r}'.format(MODEL_SELECTIONS, model_selection))
    return bool(test_map) or model_selection != 'loss'


def evaluate_test_map(yolo, strategy, database, batch_size, min_box_size, world, rank, nms='hard', nms_sigma=0.5):
    """One mAP pass over the test lmdb (COCO thresholds): this rank reads its keys[rank::world] share in this process and runs
    it through the live model's fp32 predict plan (the plan test_step uses), then the ranks' evaluators are merged.  With
    world > 1 the model evaluated is the one a checkpoint would save: the MEAN of the replicas' BN moving statistics
    (App. C4) is swapped in for the pass and every replica's own values are put back after.  A collective: every rank
    calls it.  nms / nms_sigma: the NMS method of the pass (bbox_utils.NMS_METHODS) and its Gaussian parameter.  Returns
    (DetectionEvaluator.result() over the whole test set, images, seconds)."""
    from yolo3 import metrics
    t0 = time.time()
    own = None
    if strategy is not None:
        mean = strategy.mean_moving_stats(yolo.moving)
        own = yolo.moving.clone()
        yolo.moving.copy_(mean)
    try:
        ev = metrics.DetectionEvaluator(yolo.number_classes)
        metrics.evaluate_examples(yolo, metrics.database_examples(database, world, rank), ev, min_box_size, batch_size, precision='fp32',
                                  nms=nms, nms_sigma=nms_sigma)
    finally:
        if own is not None:
            yolo.moving.copy_(own)
    if world > 1:
        ev = metrics.all_gather_evaluator(ev)
    res = ev.result()
    return res, ev.num_images, time.time() - t0


def multiscale_sizes(multiscale_min, multiscale_max):
    """The square sizes of --multiscale_min / --multiscale_max: every multiple of 32 in [min, max]; None when both are None (off).
    ValueError when only one is given, either is no positive multiple of 32, or min > max."""
    if multiscale_min is None and multiscale_max is None:
        return None
    if multiscale_min is None or multiscale_max is None:
        raise ValueError('--multiscale_min and --multiscale_max go together')
    lo, hi = int(multiscale_min), int(multiscale_max)
    if lo < 32 or hi < 32 or lo % 32 or hi % 32:
        raise ValueError('--multiscale_min / --multiscale_max must be positive multiples of 32, got {} / {}'.format(lo, hi))
    if lo > hi:
        raise ValueError('--multiscale_min {} is larger than --multiscale_max {}'.format(lo, hi))
    return [(v, v) for v in range(lo, hi + 1, 32)]


def abort_on_nan(loss_value, message):
    """train.py:124-125,151-152."""
    if np.isnan(float(loss_value)):
        raise RuntimeError(message)


def effective_reader_count(requested, cpus, local_world):
    """Reader processes per GPU.  The reference starts READER_COUNT = 3 per GPU (train.py:16) for a TensorFlow step; a ~17 ms
    step with augmentation on (~20 ms of CPU per image) wants about 12 (tools/train_throughput.py).  Two readers (train, test)
    run per rank and every rank of the node shares the host, so both the default and an explicit --reader_count are capped by
    the cores one rank may use: cpus // local_world minus one for the rank's own main + prefetch threads, never below 1."""
    share = max(1, (cpus or 1) // max(local_world, 1) - 1)
    if requested is None:
        requested = max(READER_COUNT, min(12, share - 1))
    return max(1, min(int(requested), share))


def check_mosaic_args(mosaic_prob, mosaic_min_visible):
    """--mosaic_prob / --mosaic_min_visible -> the probability as a float (0.0 = off).  ValueError outside [0, 1]."""
    p = float(mosaic_prob or 0.0)
    if not 0.0 <= p <= 1.0:
        raise ValueError('--mosaic_prob must be in [0, 1], got {!r}'.format(mosaic_prob))
    if not 0.0 <= float(mosaic_min_visible) <= 1.0:
        raise ValueError('--mosaic_min_visible must be in [0, 1], got {!r}'.format(mosaic_min_visible))
    return p


def check_affine_args(affine_prob, affine_degrees=10.0, affine_shear=2.0, affine_scale=0.1, affine_translate=0.1, affine_fill=0.0,
                      affine_min_visible=0.25):
    """--affine_prob and its magnitudes -> the probability as a float (0.0 = off).  ValueError outside the ranges of
    Dataset.affine: prob in [0, 1], degrees in [0, 180], shear in [0, 45), scale in [0, 1), translate in [0, 1], a finite fill,
    min_visible in [0, 1]."""
    p = float(affine_prob or 0.0)
    if not 0.0 <= p <= 1.0:
        raise ValueError('--affine_prob must be in [0, 1], got {!r}'.format(affine_prob))
    if not 0.0 <= float(affine_degrees) <= 180.0:
        raise ValueError('--affine_degrees must be in [0, 180], got {!r}'.format(affine_degrees))
    if not 0.0 <= float(affine_shear) < 45.0:
        raise ValueError('--affine_shear must be in [0, 45), got {!r}'.format(affine_shear))
    if not 0.0 <= float(affine_scale) < 1.0:
        raise ValueError('--affine_scale must be in [0, 1), got {!r}'.format(affine_scale))
    if not 0.0 <= float(affine_translate) <= 1.0:
        raise ValueError('--affine_translate must be in [0, 1], got {!r}'.format(affine_translate))
    if not abs(float(affine_fill)) < float('inf'):
        raise ValueError('--affine_fill must be finite, got {!r}'.format(affine_fill))
    if not 0.0 <= float(affine_min_visible) <= 1.0:
        raise ValueError('--affine_min_visible must be in [0, 1], got {!r}'.format(affine_min_visible))
    return p


def check_photo_args(photo_prob, photo_hue=0.015, photo_saturation=0.7, photo_value=0.4, photo_gamma=0.0, photo_white=None):
    """--photo_prob and its magnitudes -> the probability as a float (0.0 = off).  ValueError outside the ranges of
    Dataset.photometric: prob in [0, 1], hue in [0, 0.5], saturation and value in [0, 1], gamma in [0, 4], white finite and > 0
    (or not given: the top of the stored pixel range)."""
    p = float(photo_prob or 0.0)
    if not 0.0 <= p <= 1.0:
        raise ValueError('--photo_prob must be in [0, 1], got {!r}'.format(photo_prob))
    if not 0.0 <= float(photo_hue) <= 0.5:
        raise ValueError('--photo_hue must be in [0, 0.5], got {!r}'.format(photo_hue))
    if not 0.0 <= float(photo_saturation) <= 1.0:
        raise ValueError('--photo_saturation must be in [0, 1], got {!r}'.format(photo_saturation))
    if not 0.0 <= float(photo_value) <= 1.0:
        raise ValueError('--photo_value must be in [0, 1], got {!r}'.format(photo_value))
    if not 0.0 <= float(photo_gamma) <= 4.0:
        raise ValueError('--photo_gamma must be in [0, 4], got {!r}'.format(photo_gamma))
    if photo_white is not None and not 0.0 < float(photo_white) < float('inf'):
        raise ValueError('--photo_white must be finite and > 0, got {!r}'.format(photo_white))
    return p


def check_mixup_args(mixup_prob, mixup_spread=0.1):
    """--mixup_prob and --mixup_spread -> the probability as a float (0.0 = off).  ValueError outside prob in [0, 1], spread in
    [0, 0.5]."""
    p = float(mixup_prob or 0.0)
    if not 0.0 <= p <= 1.0:
        raise ValueError('--mixup_prob must be in [0, 1], got {!r}'.format(mixup_prob))
    if not 0.0 <= float(mixup_spread) <= 0.5:
        raise ValueError('--mixup_spread must be in [0, 0.5], got {!r}'.format(mixup_spread))
    return p


def build_lr_schedule(lr_schedule='reference', warmup_steps=0, warmup_start_factor=0.0, total_steps=None, final_factor=0.01, milestones=(),
                      gamma=0.1):
    """--lr_schedule and its flags -> a yolo3.schedule.LrSchedule, or None for 'reference' (the loop's own epoch-0 rule, which
    takes none of the other flags).  ValueError on a bad combination."""
    if lr_schedule not in LR_SCHEDULES:
        raise ValueError('lr_schedule must be one of {}, got {!r}'.format(', '.join(LR_SCHEDULES), lr_schedule))
    if lr_schedule == 'reference':
        if warmup_steps or warmup_start_factor or total_steps is not None or final_factor != 0.01 or tuple(milestones) or gamma != 0.1:
            raise ValueError('--lr_warmup_* / --lr_total_steps / --lr_final_factor / --lr_milestones / --lr_gamma need --lr_schedule '
                             "constant, cosine or step: 'reference' is the reference's rule, learning_rate / 10 during epoch 0")
        return None
    from yolo3.schedule import LrSchedule
    return LrSchedule(lr_schedule, warmup_steps, warmup_start_factor, total_steps, final_factor, tuple(milestones), gamma)


REFERENCE_ANCHORS = [(64, 384), (384, 64)]      # train.py:33


def check_anchor_flags(anchors, anchors_file, auto_anchors):
    """At most one of --anchors, --anchors_file and --auto_anchors; -> the checked --anchors list, or None without that flag."""
    given = [name for name, v in (('--anchors', anchors), ('--anchors_file', anchors_file), ('--auto_anchors', auto_anchors)) if v is not None]
    if len(given) > 1:
        raise ValueError('{} and {} exclude each other: give at most one source of anchors'.format(given[0], given[1]))
    if auto_anchors is not None and not 1 <= int(auto_anchors) <= 16:
        raise ValueError('--auto_anchors K: K in 1..16, got {!r}'.format(auto_anchors))
    if anchors is None:
        return None
    from yolo3.anchors import check_anchors, parse_anchor_args
    if all(isinstance(a, str) for a in anchors):
        return parse_anchor_args(anchors)
    check_anchors(anchors)
    return [tuple(a) for a in anchors]


def resolve_anchors(anchors, anchors_file, auto_anchors, train_database_filepath, output_folder, rank=0, evolve=1000, seed=0, device='cpu'):
    """The anchors of a run: the flag's, a file's, a fit to the boxes of the training database, or the reference's pair.  Runs before
    the readers are created and never touches the GPU in this process: the device fit is a fresh child process."""
    parsed = check_anchor_flags(anchors, anchors_file, auto_anchors)
    if parsed is not None:
        return parsed
    if anchors_file is None and auto_anchors is None:
        return list(REFERENCE_ANCHORS)
    from yolo3 import anchors as fitting
    if anchors_file is not None:
        return [tuple(a) for a in fitting.load_anchors(anchors_file)['anchors']]
    if device == 'gpu':
        import subprocess
        import sys
        import tempfile
        here = os.path.dirname(os.path.abspath(__file__))
        with tempfile.TemporaryDirectory(prefix='anchors-rank{}-'.format(rank)) as tmp:
            path = os.path.join(tmp, 'anchors.json')
            env = dict(os.environ, PYTHONPATH=here + os.pathsep + os.environ.get('PYTHONPATH', ''))
            r = subprocess.run([sys.executable, os.path.join(here, 'find_anchor_sizes.py'), '--metric', 'iou', '--database', train_database_filepath,
                                '--k', str(int(auto_anchors)), '--evolve', str(int(evolve)), '--seed', str(int(seed)), '--device', 'gpu',
                                '--output', path], env=env, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError('--auto_anchors_device gpu: find_anchor_sizes.py failed ({}):\n{}'.format(r.returncode, r.stderr[-2000:]))
            fit = fitting.load_anchors(path)
    else:
        wh = fitting.load_sizes_lmdb(train_database_filepath)
        if wh.shape[0] == 0:
            raise ValueError('--auto_anchors: {} holds no boxes'.format(train_database_filepath))
        fit = fitting.fit_anchors(wh, int(auto_anchors), seed=int(seed), evolve=int(evolve), device='cpu')
    if rank == 0:
        print('Anchors fitted to the {} boxes of {} (scored on the {}):'.format(fit['n'], train_database_filepath, device))
        for line in fitting.format_fit(fit):
            print(line)
        fitting.save_anchors(os.path.join(output_folder, 'anchors.json'), fit)
    return [tuple(a) for a in fit['anchors']]


def check_anchor_assignment(anchor_assignment, anchor_masks):
    """--anchor_assignment {all, scale} and --anchor_masks "6,7,8 3,4,5 0,1,2"  -> 'all' or 'scale'.  Masks imply
    'scale' and contradict an explicit 'all'; the masks themselves are checked once the anchors are known (resolve_anchor_scale)."""
    if anchor_assignment not in (None, 'all', 'scale'):
        raise ValueError("--anchor_assignment must be 'all' or 'scale', got {!r}".format(anchor_assignment))
    if anchor_masks is not None:
        if anchor_assignment == 'all':
            raise ValueError('--anchor_masks gives every anchor to one scale: it contradicts --anchor_assignment all')
        masks = anchor_masks.split() if isinstance(anchor_masks, str) else list(anchor_masks)
        if len(masks) != 3:
            raise ValueError('--anchor_masks takes three comma-separated index lists (stride 32, 16, 8), e.g. "6,7,8 3,4,5 0,1,2"; got {!r}'
                             .format(anchor_masks))
        return 'scale'
    return anchor_assignment or 'all'


def resolve_anchor_scale(anchor_assignment, anchor_masks, anchors, output_folder=None, rank=0, anchors_file=None):
    """The owner table of a run (one scale per anchor), or None for the reference's assignment of every anchor to every scale:
    --anchor_masks, else the table an --anchors_file records, else yolo3.anchors.default_anchor_scales of the anchors.
    With an output folder, rank 0 writes <out>/anchor_scales.json next to anchors.json."""
    if check_anchor_assignment(anchor_assignment, anchor_masks) == 'all':
        return None
    from yolo3 import anchors as fitting
    table = None
    if anchor_masks is not None:
        table = fitting.parse_anchor_masks(anchor_masks, len(anchors))
    elif anchors_file is not None:
        table = fitting.load_anchor_scale(anchors_file)
    if table is None:
        table = fitting.default_anchor_scales(anchors)
    if output_folder is not None and rank == 0:
        import json
        with open(os.path.join(output_folder, 'anchor_scales.json'), 'w') as f:
            json.dump(dict(anchors=[[float(w), float(h)] for w, h in anchors], anchor_scale=table, anchor_masks=fitting.scale_masks(table)), f,
                      indent=1, sort_keys=True)
            f.write('\n')
    return table


def describe_freeze(specs, freeze_layers, freeze_bn):
    """The line train_model prints about a fine-tuning run: how many layers and parameters are frozen and how many train."""
    count = lambda sp: sp.k * sp.k * sp.cin * sp.cout + sp.cout * (3 if sp.bn else 1)
    frozen = sum(count(sp) for sp in specs[:freeze_layers])
    total = sum(count(sp) for sp in specs)
    return ('Fine-tuning: {} of {} layers frozen ({} parameters, BatchNorm on the stored statistics), {} layers train ({} parameters); '
            'BatchNorm of the trainable layers uses {}'.format(freeze_layers, len(specs), frozen, len(specs) - freeze_layers, total - frozen,
                                                                'the stored statistics, which stay (gamma and beta train)' if freeze_bn
                                                                else 'batch statistics'))


def train_model(batch_size, test_every_n_steps, train_database_filepath, test_database_filepath, output_folder, early_stopping_count,
                learning_rate, use_augmentation, max_epochs=None, reader_count=None, backend='nccl', augmentation_device='cpu',
                test_map=False, model_selection='loss', test_map_min_box_size=32, ema_decay=0.0, test_map_nms='hard', test_map_nms_sigma=0.5,
                box_loss='mse', box_loss_weight=1.0, accumulate_steps=1, grad_clip_norm=None, multiscale_min=None, multiscale_max=None,
                multiscale_period=10, multiscale_seed=0, mosaic_prob=0.0, mosaic_seed=0, mosaic_min_visible=0.25,
                ignore_mask='reference', ignore_thresh=0.5, ignore_max_boxes=1024, focal_gamma=0.0, focal_alpha=0.0, focal_terms=None,
                label_smoothing=0.0, spp=False, optimizer='adam', momentum=0.9, nesterov=False, weight_decay=0.0, lr_schedule='reference',
                lr_warmup_steps=0, lr_warmup_start_factor=0.0, lr_total_steps=None, lr_final_factor=0.01, lr_milestones=(), lr_gamma=0.1,
                affine_prob=0.0, affine_degrees=10.0, affine_shear=2.0, affine_scale=0.1, affine_translate=0.1, affine_fill=0.0, affine_seed=0,
                affine_min_visible=0.25, init_weights=None, init_optimizer=False, freeze_layers=0, freeze_bn=False, anchors=None, anchors_file=None,
                auto_anchors=None, auto_anchors_evolve=1000, auto_anchors_seed=0, auto_anchors_device='cpu', photo_prob=0.0, photo_hue=0.015,
                photo_saturation=0.7, photo_value=0.4, photo_gamma=0.0, photo_white=None, photo_seed=0, mixup_prob=0.0, mixup_spread=0.1,
                mixup_seed=0, anchor_assignment=None, anchor_masks=None):
    check_anchor_flags(anchors, anchors_file, auto_anchors)
    check_anchor_assignment(anchor_assignment, anchor_masks)
    spp_kw = dict(spp=True) if spp else {}
    from yolo3.model import check_freeze_args
    check_freeze_args(freeze_layers, freeze_bn)
    if init_optimizer and not init_weights:
        raise ValueError('init_optimizer needs init_weights: there is no file to take the optimiser state from')
    # fine-tuning: settings of this run, not of the network -- the export below is built without them
    freeze_kw = dict(freeze_layers=int(freeze_layers), freeze_bn=bool(freeze_bn)) if freeze_layers or freeze_bn else {}
    schedule = build_lr_schedule(lr_schedule, lr_warmup_steps, lr_warmup_start_factor, lr_total_steps, lr_final_factor, lr_milestones, lr_gamma)
    from yolo3.model import check_optimizer_args
    check_optimizer_args(optimizer, momentum, nesterov, weight_decay, schedule)
    optim_kw = dict(optimizer=optimizer, momentum=momentum, nesterov=bool(nesterov), weight_decay=weight_decay) if optimizer != 'adam' else {}
    test_map = effective_test_map(test_map, model_selection)
    mosaic_prob = check_mosaic_args(mosaic_prob, mosaic_min_visible)
    if mosaic_prob and augmentation_device != 'gpu':
        raise ValueError('mosaic augmentation needs augmentation_device gpu: the batches are composed and labelled on the device')
    affine_prob = check_affine_args(affine_prob, affine_degrees, affine_shear, affine_scale, affine_translate, affine_fill, affine_min_visible)
    if affine_prob and augmentation_device != 'gpu':
        raise ValueError('affine augmentation needs augmentation_device gpu: the batches are warped and labelled on the device')
    photo_prob = check_photo_args(photo_prob, photo_hue, photo_saturation, photo_value, photo_gamma, photo_white)
    if photo_prob and augmentation_device != 'gpu':
        raise ValueError('photometric augmentation needs augmentation_device gpu: the pass runs on the device, after the augmentation')
    mixup_prob = check_mixup_args(mixup_prob, mixup_spread)
    if mixup_prob and augmentation_device != 'gpu':
        raise ValueError('mixup needs augmentation_device gpu: the batches are blended and labelled on the device')
    train_sizes = multiscale_sizes(multiscale_min, multiscale_max)
    if train_sizes is not None and augmentation_device != 'gpu':
        raise ValueError('multi-scale training needs augmentation_device gpu: the batches are resampled and labelled on the device')
    if train_sizes is not None and int(multiscale_period) < 1:
        raise ValueError('multiscale_period must be >= 1, got {!r}'.format(multiscale_period))
    from yolo3.model import check_box_loss_args, check_focal_args, check_grad_args, check_ignore_mask_args
    check_box_loss_args(box_loss, box_loss_weight)
    check_focal_flags(focal_gamma, focal_alpha, focal_terms)
    focal_terms = 'both' if focal_terms is None else focal_terms
    check_focal_args(focal_gamma, focal_alpha, focal_terms, label_smoothing)
    focal_on = bool(focal_gamma or focal_alpha or label_smoothing)
    focal_kw = dict(focal_gamma=focal_gamma, focal_alpha=focal_alpha, focal_terms=focal_terms, label_smoothing=label_smoothing) if focal_on else {}
    check_ignore_mask_args(ignore_mask, ignore_thresh, ignore_max_boxes)
    mask_args = dict(ignore_mask=ignore_mask, ignore_thresh=ignore_thresh, max_truth_boxes=ignore_max_boxes) if ignore_mask != 'reference' else {}
    check_grad_args(accumulate_steps, grad_clip_norm)
    if test_map:
        from yolo3 import bbox_utils
        bbox_utils.check_nms_args(test_map_nms, test_map_nms_sigma)
    ema_decay = float(ema_decay) if ema_decay else None
    os.makedirs(output_folder, exist_ok=True)

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    # the reference's pair unless a flag says otherwise; before the readers, which take the anchors and fork
    anchors = resolve_anchors(anchors, anchors_file, auto_anchors, train_database_filepath, output_folder, rank, auto_anchors_evolve,
                              auto_anchors_seed, auto_anchors_device)
    # every anchor on every scale unless a flag gives each to one; the readers and the model take the same table
    anchor_scale = resolve_anchor_scale(anchor_assignment, anchor_masks, anchors, output_folder, rank, anchors_file)
    scale_reader_kw = dict(anchor_scale=anchor_scale) if anchor_scale is not None else {}
    scale_model_kw = dict(anchor_scales=anchor_scale) if anchor_scale is not None else {}
    if anchor_scale is not None and rank == 0:
        print('Per-scale anchor assignment: anchors of stride 32 / 16 / 8 = {} (anchor_scales.json)'.format(
            ' / '.join(','.join(str(i) for i, s in enumerate(anchor_scale) if s == t) for t in range(3))))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    global_batch_size = batch_size * world
    local_world = int(os.environ.get('LOCAL_WORLD_SIZE', str(world)))
    asked = reader_count
    reader_count = effective_reader_count(reader_count, os.cpu_count() or 8, local_world)
    if asked is not None and reader_count != asked:
        print('reader_count {} capped to {} ({} cpus / {} ranks on this node)'.format(asked, reader_count, os.cpu_count(), local_world))

    # readers first: their worker processes are forked before this process touches the GPU
    from yolo3 import imagereader
    print('Setting up test image reader')
    # one reader per rank: the unshuffled test reader takes this rank's stride of the key list (the reference splits one
    # global test batch over its replicas, train.py:64-66)
    test_reader = imagereader.ImageReader(test_database_filepath, anchors, use_augmentation=False, shuffle=False, num_workers=reader_count,
                                          num_shards=world, shard_index=rank, augmentation_device=augmentation_device, **scale_reader_kw)
    print('Test Reader has {} images'.format(test_reader.get_image_count()))
    print('Setting up training image reader')
    train_reader = imagereader.ImageReader(train_database_filepath, anchors, use_augmentation=use_augmentation, shuffle=True,
                                           num_workers=reader_count, balance_classes=True, augmentation_device=augmentation_device,
                                           **scale_reader_kw,
                                           **(dict(label_device='gpu') if train_sizes is not None or mosaic_prob or affine_prob or mixup_prob else {}),
                                           # (a shuffled reader ignores its shard when it picks keys; the mosaic, affine, photometric and
                                           # mixup draws are keyed by it)
                                           **(dict(num_shards=world, shard_index=rank) if mosaic_prob or affine_prob or photo_prob or mixup_prob else {}))
    print('Train Reader has {} images'.format(train_reader.get_image_count()))
    training_checkpoint_filepath = None
    try:
        print('Starting Readers')
        train_reader.startup()
        test_reader.startup()

        import torch
        import torch.distributed as dist
        from yolo3 import model
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
        from yolo3 import streams
        streams.reserve()      # side / comm streams bind to hardware queues before a communicator creates its own (yolo3/streams.py)
        strategy = None
        if world > 1:
            os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
            if backend == 'nccl':                  # = RCCL over xGMI, one GPU per rank
                # a launcher that hands every rank its OWN device through *_VISIBLE_DEVICES shows exactly one device per rank: fine.
                # A mask that shows several devices but fewer than the ranks would put two nccl ranks on one device.
                isolated = any(os.environ.get(k) for k in ('HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES'))
                ndev = torch.cuda.device_count()
                if ndev < int(os.environ.get('LOCAL_WORLD_SIZE', str(world))) and not (isolated and ndev == 1):
                    raise RuntimeError('backend nccl (RCCL) needs one GPU per rank: %d visible for %s ranks; use --backend gloo to rehearse on fewer'
                                       % (ndev, os.environ.get('LOCAL_WORLD_SIZE', str(world))))
                dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank % torch.cuda.device_count()))
            else:
                dist.init_process_group(backend)
            from yolo3.parallel import DataParallel
            strategy = DataParallel()

        train_dataset = train_reader.get_tf_dataset().batch(batch_size).prefetch(reader_count)
        test_dataset = test_reader.get_tf_dataset().batch(batch_size).prefetch(reader_count)
        if train_sizes is not None:
            train_dataset = train_dataset.multiscale(train_sizes, multiscale_period, multiscale_seed)
            print('Multi-scale training: sizes {} drawn every {} batches (seed {}); testing, checkpoint and export stay at {}'.format(
                [s[0] for s in train_sizes], multiscale_period, multiscale_seed, train_reader.get_image_size()[:2]))
        if mosaic_prob:
            train_dataset = train_dataset.mosaic(mosaic_prob, mosaic_seed, mosaic_min_visible)
            print('Mosaic augmentation: probability {:g} per image, four images of the batch per mosaic (seed {}); boxes with less than '
                  '{:g} of their area visible are dropped; the test reader is untouched'.format(mosaic_prob, mosaic_seed, mosaic_min_visible))
        if affine_prob:
            train_dataset = train_dataset.affine(affine_prob, affine_degrees, affine_shear, affine_scale, affine_translate, affine_fill, affine_seed,
                                                 affine_min_visible)
            print('Affine augmentation: probability {:g} per image, rotation +-{:g} deg, shear +-{:g} deg, gain 1 +- {:g}, translation +-{:g} of '
                  'the side, fill {:g} (seed {}); boxes with less than {:g} of their area inside the image are dropped; the test reader is '
                  'untouched'.format(affine_prob, affine_degrees, affine_shear, affine_scale, affine_translate, affine_fill, affine_seed,
                                     affine_min_visible))
        if photo_prob:
            train_dataset = train_dataset.photometric(photo_prob, photo_hue, photo_saturation, photo_value, photo_gamma, photo_seed, photo_white)
            print('Photometric augmentation: probability {:g} per image, hue +-{:g} turns, saturation 1 +- {:g}, value 1 +- {:g}, tone exponent '
                  '2^+-{:g}, white {:g} (seed {}); the test reader is untouched'.format(photo_prob, photo_hue, photo_saturation, photo_value, photo_gamma,
                                                                                       train_dataset.photo_cfg[6], photo_seed))
        if mixup_prob:
            train_dataset = train_dataset.mixup(mixup_prob, mixup_spread, mixup_seed)
            print('MixUp: probability {:g} per image, lambda uniform in 0.5 +- {:g} (seed {}), partner from the same batch, boxes of both '
                  'images kept; the test reader is untouched'.format(mixup_prob, mixup_spread, mixup_seed))

        print('Creating model')
        number_classes = train_reader.get_number_classes()
        yolo = model.YoloV3(global_batch_size, train_reader.get_image_size(), number_classes, anchors, learning_rate, ema_decay=ema_decay,
                            box_loss=box_loss, box_loss_weight=box_loss_weight, accumulate_steps=accumulate_steps,
                            grad_clip_norm=grad_clip_norm, **(dict(train_sizes=train_sizes) if train_sizes is not None else {}), **mask_args,
                            **focal_kw, **spp_kw, **optim_kw, **(dict(lr_schedule=schedule) if schedule is not None else {}), **freeze_kw, **scale_model_kw)
        if init_weights:
            # every rank reads the same file, so the replicas start equal (the broadcast below then changes nothing)
            if init_optimizer:
                yolo.load_weights(init_weights, load_optimizer=True)      # (refuses another network or optimiser)
                print('Initial weights, optimiser moments and step count ({}) from {}; the epoch counter, the early-stopping history and '
                      'the EMA start fresh'.format(yolo.iterations, init_weights))
            else:
                kept = yolo.load_pretrained(init_weights)
                print('Initial weights from {}: {} of {} layers loaded, {} keep their initialisation; optimiser state and step count start '
                      'fresh'.format(init_weights, len(yolo.specs) - len(kept), len(yolo.specs), kept if kept else 'none'))
        if freeze_kw:
            print(describe_freeze(yolo.specs, yolo.freeze_layers, yolo.freeze_bn))
        if optimizer != 'adam' or schedule is not None:
            print('Optimizer: {}{}, weight decay {:g} on the convolution kernels; learning-rate schedule: {}'.format(
                optimizer, ' (momentum {:g}{})'.format(momentum, ', Nesterov' if nesterov else '') if optimizer == 'sgd' else '', weight_decay,
                lr_schedule))
        if spp:
            print('Network: YOLOv3-SPP (5 / 9 / 13 max-pool pyramid in the block of the coarsest scale, {} conv layers)'.format(len(yolo.specs)))
        if strategy is not None:
            strategy.attach(yolo)
            strategy.broadcast_parameters(yolo.params, yolo.moving)
            yolo._refresh_transposed()
            yolo.reset_ema()            # every replica starts the average from rank 0's weights
        if ema_decay is not None:
            print('Using an exponential moving average of the weights (decay {}, warm-up {:g} steps) for the test loss, the mAP pass '
                  'and the checkpoint'.format(ema_decay, yolo.ema_warmup))

        log_grad_norm = accumulate_steps > 1 or grad_clip_norm is not None
        if log_grad_norm:
            print('Effective batch size {} = batch_size {} x {} replicas x {} accumulated steps; gradient norm {}'.format(
                batch_size * world * accumulate_steps, batch_size, world, accumulate_steps,
                'clipped at {}'.format(grad_clip_norm) if grad_clip_norm is not None else 'not clipped'))

        if focal_on:
            print('Focal loss: gamma {:g}, alpha {:g} on the {} term{}; class-label smoothing {:g} (training and test loss){}'.format(
                focal_gamma, focal_alpha, {'obj': 'objectness', 'class': 'class', 'both': 'objectness and class'}[focal_terms],
                '' if focal_terms != 'both' else 's', label_smoothing,
                '; the test loss that selects the model is not comparable with that of another setting' if model_selection == 'loss' else ''))

        log_ignored = ignore_mask == 'truth'
        warned_truth_cap = False
        if log_ignored:
            print('Ignore mask: predictions without an object that overlap a ground-truth box of their image with IoU >= {:g} are left out '
                  'of the objectness loss (training and test loss; at most {} boxes per image)'.format(ignore_thresh, ignore_max_boxes))

        def averaged():
            """The model the loop judges and keeps: the EMA copy when there is one (each replica's own EMA moving statistics,
            which evaluate_test_map and the checkpoint replace by their mean over the replicas), else the live weights."""
            return yolo.ema_weights() if ema_decay is not None else contextlib.nullcontext()

        train_epoch_size = test_every_n_steps
        test_epoch_size = test_reader.get_image_count() / batch_size
        test_loss = list()
        map_rows = list()          # test_map.csv: epoch, map50, map50_95, tp50, fp50, npos
        map_scores = list()        # the --model_selection mAP per epoch
        names = ['loss', 'loss_xy', 'loss_wh', 'loss_obj', 'loss_class']
        train_metrics = [model.Mean('train_' + n) for n in names]
        test_metrics = [model.Mean('test_' + n) for n in names]

        current_time = datetime.datetime.now().strftime("%Y%m%dT%H%M%S")
        log_dir = os.path.join(output_folder, 'scalars-' + current_time)
        if rank == 0:
            os.makedirs(log_dir, exist_ok=True)
            for split in ('train', 'test'):
                with open(os.path.join(log_dir, split + '.csv'), 'w') as fh:
                    fh.write('step,' + ','.join(names) + '\n')
            if log_grad_norm:
                with open(os.path.join(log_dir, 'grad_norm.csv'), 'w') as fh:
                    fh.write('step,grad_norm,scale\n')
            if train_sizes is not None:
                with open(os.path.join(log_dir, 'train_size.csv'), 'w') as fh:
                    fh.write('step,height,width\n')
            if log_ignored:
                with open(os.path.join(log_dir, 'ignored.csv'), 'w') as fh:
                    fh.write('step,ignored,truth_max\n')
            if schedule is not None:
                with open(os.path.join(log_dir, 'lr.csv'), 'w') as fh:
                    fh.write('step,lr\n')

        def log_scalars(split, step, metrics):
            if rank == 0:
                with open(os.path.join(log_dir, split + '.csv'), 'a') as fh:
                    fh.write('{},{}\n'.format(step, ','.join(repr(m.result()) for m in metrics)))

        epoch = 0
        print('Running Network')
        while True:  # loop until early stopping
            print('---- Epoch: {} ----'.format(epoch))
            if schedule is not None:
                # the schedule owns the rate: the full epoch size from epoch 0 on, no per-epoch set_learning_rate
                cur_train_epoch_size = train_epoch_size
            elif epoch == 0:
                cur_train_epoch_size = min(1000, train_epoch_size)
                print('Performing Adam Optimizer learning rate warmup for {} steps'.format(cur_train_epoch_size))
                yolo.set_learning_rate(learning_rate / 10)
            else:
                cur_train_epoch_size = train_epoch_size
                yolo.set_learning_rate(learning_rate)

            start_time = time.time()
            for step, (batch_images, l1, l2, l3) in enumerate(train_dataset):
                if step > cur_train_epoch_size:
                    break
                inputs = (batch_images, (l1, l2, l3), *train_metrics)
                loss_value = yolo.dist_train_step(strategy, inputs)
                abort_on_nan(loss_value, 'Training Loss went to NaN, try a lower learning rate')
                print('Train Epoch {}: Batch {}/{}: Loss {}'.format(epoch, step, train_epoch_size, train_metrics[0].result()))
                log_scalars('train', int(epoch * train_epoch_size + step), train_metrics)
                if train_sizes is not None and rank == 0:
                    with open(os.path.join(log_dir, 'train_size.csv'), 'a') as fh:
                        fh.write('{},{},{}\n'.format(int(epoch * train_epoch_size + step), int(batch_images.shape[2]), int(batch_images.shape[3])))
                if log_grad_norm and rank == 0 and yolo.micro_step == 0:      # this batch completed an optimiser step
                    with open(os.path.join(log_dir, 'grad_norm.csv'), 'a') as fh:
                        fh.write('{},{!r},{!r}\n'.format(int(epoch * train_epoch_size + step), float(yolo.last_grad_norm),
                                                        float(yolo.grad_scale_dev)))
                if schedule is not None and rank == 0 and yolo.micro_step == 0:      # one row per optimiser step: its number and rate
                    with open(os.path.join(log_dir, 'lr.csv'), 'a') as fh:
                        fh.write('{},{!r}\n'.format(yolo.iterations, yolo.current_learning_rate()))
                if log_ignored and rank == 0 and yolo.micro_step == 0:       # (of the batch that completed the optimiser step)
                    truth_max = int(yolo.last_truth_max)
                    with open(os.path.join(log_dir, 'ignored.csv'), 'a') as fh:
                        fh.write('{},{},{}\n'.format(int(epoch * train_epoch_size + step), int(yolo.last_ignored), truth_max))
                    if truth_max > ignore_max_boxes and not warned_truth_cap:
                        warned_truth_cap = True
                        print('WARNING: an image has {} ground-truth boxes, --ignore_max_boxes is {}: the ignore mask sees only the first '
                              '{} of them (warned once)'.format(truth_max, ignore_max_boxes, ignore_max_boxes))
                for m in train_metrics:
                    m.reset_states()

            epoch_test_loss = list()
            with averaged():
                for step, (batch_images, l1, l2, l3) in enumerate(test_dataset):
                    if step > test_epoch_size:
                        break
                    inputs = (batch_images, (l1, l2, l3), *test_metrics)
                    loss_value = yolo.dist_test_step(strategy, inputs)
                    abort_on_nan(loss_value, 'Test Loss went to NaN')
                    epoch_test_loss.append(float(loss_value))
            test_loss.append(np.mean(epoch_test_loss))
            print('Test Epoch: {}: Loss = {}'.format(epoch, test_metrics[0].result()))
            log_scalars('test', int((epoch + 1) * train_epoch_size), test_metrics)
            for m in test_metrics:
                m.reset_states()

            if test_map:
                with averaged():
                    res, map_images, map_secs = evaluate_test_map(yolo, strategy, test_database_filepath, batch_size, test_map_min_box_size, world, rank,
                                                                     test_map_nms, test_map_nms_sigma)
                print('Test Epoch: {}: mAP50 = {}, mAP50:95 = {} ({} images, mAP pass took {:.3f} s)'.format(
                    epoch, res['map50'], res['map50_95'], map_images, map_secs))
                if model_selection != 'loss':
                    if not map_scores and int(res['npos'].sum()) == 0:
                        raise RuntimeError('--model_selection {}: the test set holds no ground-truth boxes, so its mAP is undefined'.format(model_selection))
                    map_scores.append(res[model_selection])
                map_rows.append((epoch, res['map50'], res['map50_95'], int(res['tp50'].sum()), int(res['fp50'].sum()), int(res['npos'].sum())))
                if rank == 0:
                    with open(os.path.join(output_folder, 'test_map.csv'), 'w') as csvfile:
                        csvfile.write('epoch,map50,map50_95,tp50,fp50,npos\n')
                        for row in map_rows:
                            csvfile.write('{},{!r},{!r},{},{},{}\n'.format(*row))

            if rank == 0:
                with open(os.path.join(output_folder, 'test_loss.csv'), 'w') as csvfile:
                    for v in test_loss:
                        csvfile.write(str(v))
                        csvfile.write('\n')
            print('Epoch took: {} s'.format(time.time() - start_time))

            if model_selection == 'loss':
                improved = is_new_minimum(test_loss)
                if improved:
                    print('Test loss improved: {}, saving checkpoint'.format(np.min(test_loss)))
            else:
                improved = is_new_maximum(map_scores)
                if improved:
                    print('Test {} improved: {}, saving checkpoint'.format(model_selection, map_scores[-1]))
            if improved:
                # BN moving statistics are sync-on-read: the checkpoint stores their MEAN over the replicas (App. C4); every
                # replica keeps its own running values (a collective: all ranks take part, rank 0 writes)
                with averaged():
                    saved_moving = strategy.mean_moving_stats(yolo.moving) if strategy is not None else None
                    training_checkpoint_filepath = os.path.join(output_folder, 'checkpoint', 'ckpt.npz')
                    if rank == 0:
                        os.makedirs(os.path.dirname(training_checkpoint_filepath), exist_ok=True)
                        yolo.save_weights(training_checkpoint_filepath, moving=saved_moving)

            print('Best Current Epoch Selection:')
            if model_selection == 'loss':
                print('Test Loss:')
                print(test_loss)
                print('Best epoch: {}'.format(best_epoch_of(test_loss)))
                if should_stop(test_loss, early_stopping_count):
                    break
            else:
                print('Test {}:'.format(model_selection))
                print(map_scores)
                print('Best epoch: {}'.format(best_epoch_of_max(map_scores)))
                if should_stop_max(map_scores, early_stopping_count):
                    break
            epoch = epoch + 1
            if max_epochs is not None and epoch >= max_epochs:
                break
    finally:
        print('Shutting down train_reader')
        train_reader.shutdown()
        print('Shutting down test_reader')
        test_reader.shutdown()

    if training_checkpoint_filepath is not None and rank == 0:
        print('Converting checkpoint into Saved_Model')
        from yolo3 import model
        best = model.YoloV3(global_batch_size, train_reader.get_image_size(), number_classes, anchors, learning_rate,
                            box_loss=box_loss, box_loss_weight=box_loss_weight, **mask_args, **focal_kw, **spp_kw, **optim_kw, **scale_model_kw)
        best.load_weights(training_checkpoint_filepath)
        os.makedirs(os.path.join(output_folder, 'saved_model'), exist_ok=True)
        best.save_weights(os.path.join(output_folder, 'saved_model', 'yolov3.npz'))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def _accumulate_steps_arg(text):
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('an integer >= 1, got {!r}'.format(text))
    if k < 1:
        raise argparse.ArgumentTypeError('an integer >= 1, got {!r}'.format(text))
    return k


def _grad_clip_norm_arg(text):
    try:
        c = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a finite number > 0, got {!r}'.format(text))
    if not (c > 0.0 and c != float('inf')):
        raise argparse.ArgumentTypeError('a finite number > 0, got {!r}'.format(text))
    return c


def _ignore_thresh_arg(text):
    try:
        t = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a number in (0, 1], got {!r}'.format(text))
    if not (0.0 < t <= 1.0):
        raise argparse.ArgumentTypeError('a number in (0, 1], got {!r}'.format(text))
    return t


def _focal_gamma_arg(text):
    try:
        g = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a finite number >= 0, got {!r}'.format(text))
    if not (g >= 0.0 and g != float('inf')):
        raise argparse.ArgumentTypeError('a finite number >= 0, got {!r}'.format(text))
    return g


def _focal_alpha_arg(text):
    try:
        a = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('0 or a number in (0, 1), got {!r}'.format(text))
    if not (a == 0.0 or 0.0 < a < 1.0):
        raise argparse.ArgumentTypeError('0 or a number in (0, 1), got {!r}'.format(text))
    return a


def _label_smoothing_arg(text):
    try:
        e = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a number in [0, 1), got {!r}'.format(text))
    if not (0.0 <= e < 1.0):
        raise argparse.ArgumentTypeError('a number in [0, 1), got {!r}'.format(text))
    return e


def _momentum_arg(text):
    try:
        m = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a number in [0, 1), got {!r}'.format(text))
    if not (0.0 <= m < 1.0):
        raise argparse.ArgumentTypeError('a number in [0, 1), got {!r}'.format(text))
    return m


def _weight_decay_arg(text):
    try:
        w = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a finite number >= 0, got {!r}'.format(text))
    if not (w >= 0.0 and w != float('inf')):
        raise argparse.ArgumentTypeError('a finite number >= 0, got {!r}'.format(text))
    return w


def _unit_factor_arg(text):
    try:
        f = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a number in [0, 1], got {!r}'.format(text))
    if not (0.0 <= f <= 1.0):
        raise argparse.ArgumentTypeError('a number in [0, 1], got {!r}'.format(text))
    return f


def _lr_gamma_arg(text):
    try:
        g = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a finite number > 0, got {!r}'.format(text))
    if not (g > 0.0 and g != float('inf')):
        raise argparse.ArgumentTypeError('a finite number > 0, got {!r}'.format(text))
    return g


def _step_count_arg(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('an integer >= 0, got {!r}'.format(text))
    if v < 0:
        raise argparse.ArgumentTypeError('an integer >= 0, got {!r}'.format(text))
    return v


def _step_number_arg(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('an integer >= 1, got {!r}'.format(text))
    if v < 1:
        raise argparse.ArgumentTypeError('an integer >= 1, got {!r}'.format(text))
    return v


def check_focal_flags(focal_gamma, focal_alpha, focal_terms):
    """--focal_alpha / --focal_terms say how the focal form is applied: without --focal_gamma > 0 there is none.  focal_terms None =
    the flag was not given."""
    if (focal_alpha or focal_terms is not None) and not focal_gamma > 0:
        raise ValueError('--focal_alpha / --focal_terms need --focal_gamma > 0: without it no term has the focal form')


def _ignore_max_boxes_arg(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('an integer >= 1, got {!r}'.format(text))
    if v < 1 or v >= 2 ** 31:
        raise argparse.ArgumentTypeError('an integer >= 1, got {!r}'.format(text))
    return v


def _multiscale_side_arg(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('a positive multiple of 32, got {!r}'.format(text))
    if v < 32 or v % 32:
        raise argparse.ArgumentTypeError('a positive multiple of 32, got {!r}'.format(text))
    return v


def _multiscale_period_arg(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('an integer >= 1, got {!r}'.format(text))
    if v < 1:
        raise argparse.ArgumentTypeError('an integer >= 1, got {!r}'.format(text))
    return v


def _freeze_layers_arg(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('an integer >= 0, got {!r}'.format(text))
    if v < 0:
        raise argparse.ArgumentTypeError('an integer >= 0, got {!r}'.format(text))
    return v


FREEZE_NAMES = {'backbone': 52}      # yolo3.model.BACKBONE_LAYERS restated: parsing loads no device library


class _Parser(argparse.ArgumentParser):
    """The checks that span several flags: an argparse error like any other."""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        try:
            sizes = multiscale_sizes(a.multiscale_min, a.multiscale_max)
        except ValueError as e:
            self.error(str(e))
        if sizes is not None and a.augmentation_device != 'gpu':
            self.error('--multiscale_min / --multiscale_max need --augmentation_device gpu')
        try:
            prob = check_mosaic_args(a.mosaic_prob, a.mosaic_min_visible)
        except ValueError as e:
            self.error(str(e))
        if prob and a.augmentation_device != 'gpu':
            self.error('--mosaic_prob needs --augmentation_device gpu')
        try:
            prob = check_affine_args(a.affine_prob, a.affine_degrees, a.affine_shear, a.affine_scale, a.affine_translate, a.affine_fill,
                                     a.affine_min_visible)
        except ValueError as e:
            self.error(str(e))
        if prob and a.augmentation_device != 'gpu':
            self.error('--affine_prob needs --augmentation_device gpu')
        try:
            prob = check_photo_args(a.photo_prob, a.photo_hue, a.photo_saturation, a.photo_value, a.photo_gamma, a.photo_white)
        except ValueError as e:
            self.error(str(e))
        if prob and a.augmentation_device != 'gpu':
            self.error('--photo_prob needs --augmentation_device gpu')
        try:
            prob = check_mixup_args(a.mixup_prob, a.mixup_spread)
        except ValueError as e:
            self.error(str(e))
        if prob and a.augmentation_device != 'gpu':
            self.error('--mixup_prob needs --augmentation_device gpu')
        # (yolo3.model.check_ignore_mask_args, which train_model calls, restated: parsing loads no device library)
        if a.ignore_mask == 'reference' and (a.ignore_thresh != 0.5 or a.ignore_max_boxes != 1024):
            self.error("--ignore_thresh / --ignore_max_boxes need --ignore_mask truth: the reference's mask has no such parameters")
        try:
            check_focal_flags(a.focal_gamma, a.focal_alpha, a.focal_terms)
        except ValueError as e:
            self.error(str(e))
        # (yolo3.model.check_optimizer_args restated, as above)
        if a.optimizer == 'adam' and a.weight_decay > 0:
            self.error("--weight_decay needs --optimizer adamw or sgd: adam is the reference's Keras Adam, which has none")
        if a.freeze is not None:
            if a.freeze_layers not in (0, FREEZE_NAMES[a.freeze]):
                self.error('--freeze {} means --freeze_layers {}, got --freeze_layers {}'.format(a.freeze, FREEZE_NAMES[a.freeze], a.freeze_layers))
            a.freeze_layers = FREEZE_NAMES[a.freeze]
        if a.init_optimizer and not a.init_weights:
            self.error('--init_optimizer 1 needs --init_weights')
        try:
            check_anchor_flags(a.anchors, a.anchors_file, a.auto_anchors)
        except ValueError as e:
            self.error(str(e))
        try:
            check_anchor_assignment(a.anchor_assignment, a.anchor_masks)
        except ValueError as e:
            self.error(str(e))
        if a.auto_anchors is None and (a.auto_anchors_evolve != 1000 or a.auto_anchors_seed != 0 or a.auto_anchors_device != 'cpu'):
            self.error('--auto_anchors_evolve / --auto_anchors_seed / --auto_anchors_device need --auto_anchors K')
        try:
            build_lr_schedule(a.lr_schedule, a.lr_warmup_steps, a.lr_warmup_start_factor, a.lr_total_steps, a.lr_final_factor, a.lr_milestones,
                              a.lr_gamma)
        except ValueError as e:
            self.error(str(e))
        return a


def build_parser():
    parser = _Parser(prog='train_yolo', description='Script which trains a yolo_v3 model')
    parser.add_argument('--batch_size', dest='batch_size', type=int, help='training batch size', default=8)
    parser.add_argument('--learning_rate', dest='learning_rate', type=float, default=1e-4)
    parser.add_argument('--test_every_n_steps', dest='test_every_n_steps', type=int, help='number of gradient update steps to take between test epochs', default=1000)
    parser.add_argument('--train_database', dest='train_database_filepath', type=str, help='lmdb database to use for (Required)', required=True)
    parser.add_argument('--test_database', dest='test_database_filepath', type=str, help='lmdb database to use for testing (Required)', required=True)
    parser.add_argument('--output_dir', dest='output_folder', type=str, help='Folder where outputs will be saved (Required)', required=True)
    parser.add_argument('--early_stopping', dest='terminate_after_num_epochs_without_test_loss_improvement', type=int, default=10)
    parser.add_argument('--use_augmentation', dest='use_augmentation', type=int, default=1)
    parser.add_argument('--reader_count', dest='reader_count', type=int, default=None, help='(addition) reader processes per GPU; default: 3 (as the reference) up to 12 when the host has the cores')
    parser.add_argument('--max_epochs', dest='max_epochs', type=int, default=None, help='(addition) stop after this many epochs')
    parser.add_argument('--backend', dest='backend', type=str, default='nccl', help='(addition) torch.distributed backend under torch.distributed.run: nccl (= RCCL, one GPU per rank) or gloo (rehearsal; ranks may share a GPU)')
    parser.add_argument('--augmentation_device', dest='augmentation_device', choices=('cpu', 'gpu'), default='cpu',
                        help='(addition) where the readers\' images are augmented: cpu = in the reader processes (as the reference), gpu = drawn '
                             'there, applied to each batch by HIP kernels; the test reader (no augmentation) uploads its pixels unconverted either way round')
    parser.add_argument('--test_map', dest='test_map', type=int, choices=(0, 1), default=0,
                        help='(addition) 1: after every test epoch, one mAP pass over the test lmdb (COCO thresholds), printed and written to <output_dir>/test_map.csv')
    parser.add_argument('--test_map_min_box_size', dest='test_map_min_box_size', type=int, default=32,
                        help='(addition) smallest detection the mAP pass considers (as evaluate.py --min-box-size)')
    parser.add_argument('--test_map_nms', dest='test_map_nms', choices=TEST_MAP_NMS_METHODS, default='hard',
                        help='(addition) NMS method of the mAP pass (as evaluate.py --nms): hard (default), diou, soft-linear or soft-gaussian')
    parser.add_argument('--test_map_nms_sigma', dest='test_map_nms_sigma', type=float, default=0.5,
                        help='(addition) sigma of --test_map_nms soft-gaussian (> 0)')
    parser.add_argument('--model_selection', dest='model_selection', choices=MODEL_SELECTIONS, default='loss',
                        help='(addition) what picks the checkpoint and drives early stopping: the test loss (first minimum, as the reference) '
                             'or the test-set mAP50 / mAP50:95 (first maximum; implies --test_map 1)')
    parser.add_argument('--ema_decay', dest='ema_decay', type=float, default=0.0,
                        help='(addition) 0 (default): off; in (0, 1): keep an exponential moving average of the weights (decay ramped up '
                             'over the first few thousand steps) and use it for the test loss, the mAP pass, the checkpoint and the export')
    parser.add_argument('--box_loss', dest='box_loss', choices=BOX_LOSSES, default='mse',
                        help='(addition) box-regression term of the training and test loss: mse (default) = the reference\'s xy + wh terms; '
                             'giou, diou or ciou = 1 - that IoU measure per labelled cell.  With an IoU loss the loss_xy column of the scalar '
                             'CSVs carries the box term and loss_wh is 0')
    parser.add_argument('--box_loss_weight', dest='box_loss_weight', type=float, default=1.0,
                        help='(addition) factor of the box term of --box_loss giou / diou / ciou (finite, > 0; mse takes 1)')
    parser.add_argument('--accumulate_steps', dest='accumulate_steps', type=_accumulate_steps_arg, default=1,
                        help='(addition) 1 (default): off; N > 1: sum the gradients of N consecutive batches into one optimiser step '
                             '(effective batch = batch_size x replicas x N at the activation memory of one batch)')
    parser.add_argument('--grad_clip_norm', dest='grad_clip_norm', type=_grad_clip_norm_arg, default=None,
                        help='(addition) off by default; X > 0: scale the gradient of an optimiser step so that its global L2 norm is at '
                             'most X (as Keras Adam(global_clipnorm=X))')
    parser.add_argument('--multiscale_min', dest='multiscale_min', type=_multiscale_side_arg, default=None,
                        help='(addition) with --multiscale_max: train at a changing square input size, every multiple of 32 from this side ... '
                             '(needs --augmentation_device gpu; testing, checkpoint and export stay at the stored size)')
    parser.add_argument('--multiscale_max', dest='multiscale_max', type=_multiscale_side_arg, default=None,
                        help='(addition) ... to this side (a multiple of 32, >= --multiscale_min)')
    parser.add_argument('--multiscale_period', dest='multiscale_period', type=_multiscale_period_arg, default=10,
                        help='(addition) batches between two draws of the multi-scale size (default 10)')
    parser.add_argument('--multiscale_seed', dest='multiscale_seed', type=int, default=0,
                        help='(addition) seed of the multi-scale size schedule: the size of batch i is a pure function of (seed, i // period)')
    parser.add_argument('--mosaic_prob', dest='mosaic_prob', type=float, default=0.0,
                        help='(addition) off by default; P in (0, 1]: each training image becomes, with probability P, a mosaic of itself and '
                             'three other images of its batch (needs --augmentation_device gpu; composes with --multiscale_*; the test reader is untouched)')
    parser.add_argument('--mosaic_seed', dest='mosaic_seed', type=int, default=0,
                        help='(addition) seed of the mosaic draws: a pure function of (seed, rank, batch count, image)')
    parser.add_argument('--mosaic_min_visible', dest='mosaic_min_visible', type=float, default=0.25,
                        help='(addition) a box of a mosaic stays when at least this share of its area lies in the window taken from its image (default 0.25)')
    parser.add_argument('--affine_prob', dest='affine_prob', type=float, default=0.0,
                        help='(addition) off by default; P in (0, 1]: each training image is warped, with probability P, through a random '
                             'rotation, shear, gain and translation on the device (needs --augmentation_device gpu; composes with '
                             '--multiscale_* and --mosaic_prob; the test reader is untouched)')
    parser.add_argument('--affine_degrees', dest='affine_degrees', type=float, default=10.0,
                        help='(addition) the rotation is drawn in +- this many degrees, in [0, 180] (default 10)')
    parser.add_argument('--affine_shear', dest='affine_shear', type=float, default=2.0,
                        help='(addition) the x and y shear angles are each drawn in +- this many degrees, in [0, 45) (default 2)')
    parser.add_argument('--affine_scale', dest='affine_scale', type=float, default=0.1,
                        help='(addition) the isotropic gain is drawn in 1 +- this, in [0, 1) (default 0.1)')
    parser.add_argument('--affine_translate', dest='affine_translate', type=float, default=0.1,
                        help='(addition) the translation is drawn in +- this share of the image side per axis, in [0, 1] (default 0.1)')
    parser.add_argument('--affine_fill', dest='affine_fill', type=float, default=0.0,
                        help='(addition) value of the pixels a warp brings in from outside the image, in stored-pixel units (default 0)')
    parser.add_argument('--affine_seed', dest='affine_seed', type=int, default=0,
                        help='(addition) seed of the affine draws: a pure function of (seed, rank, batch count, image)')
    parser.add_argument('--affine_min_visible', dest='affine_min_visible', type=float, default=0.25,
                        help='(addition) a warped box stays when at least this share of its transformed area lies inside the image (default 0.25)')
    parser.add_argument('--photo_prob', dest='photo_prob', type=float, default=0.0,
                        help='(addition) off by default; P in (0, 1]: each training image goes, with probability P, through a random colour '
                             'matrix, clamp and tone curve on the device (needs --augmentation_device gpu; the test reader is untouched)')
    parser.add_argument('--photo_hue', dest='photo_hue', type=float, default=0.015,
                        help='(addition) the YIQ chroma plane is rotated by +- this many turns, in [0, 0.5] (default 0.015)')
    parser.add_argument('--photo_saturation', dest='photo_saturation', type=float, default=0.7,
                        help='(addition) the chroma gain is drawn in 1 +- this, in [0, 1] (default 0.7)')
    parser.add_argument('--photo_value', dest='photo_value', type=float, default=0.4,
                        help='(addition) the value gain is drawn in 1 +- this, in [0, 1] (default 0.4); alone it is cancelled by the z-score '
                             'up to the clamp at --photo_white')
    parser.add_argument('--photo_gamma', dest='photo_gamma', type=float, default=0.0,
                        help='(addition) the tone exponent is 2^e, e drawn in +- this, in [0, 4] (default 0: no tone curve)')
    parser.add_argument('--photo_white', dest='photo_white', type=float, default=None,
                        help='(addition) top of the pixel range: the clamp and the scale of the tone curve (default: 255 for a uint8, 65535 '
                             'for a uint16 database; a float32 database must give it)')
    parser.add_argument('--photo_seed', dest='photo_seed', type=int, default=0,
                        help='(addition) seed of the photometric draws: a pure function of (seed, rank, batch count, image)')
    parser.add_argument('--mixup_prob', dest='mixup_prob', type=float, default=0.0,
                        help='(addition) off by default; P in (0, 1]: each training image is blended, with probability P, with another image '
                             'of its batch and gets the boxes of both (needs --augmentation_device gpu; the test reader is untouched)')
    parser.add_argument('--mixup_spread', dest='mixup_spread', type=float, default=0.1,
                        help='(addition) lambda is uniform in 0.5 +- this, in [0, 0.5] (default 0.1); a uniform window, not a Beta draw')
    parser.add_argument('--mixup_seed', dest='mixup_seed', type=int, default=0,
                        help='(addition) seed of the MixUp draws: a pure function of (seed, rank, batch count, image)')
    parser.add_argument('--ignore_mask', dest='ignore_mask', choices=IGNORE_MASKS, default='reference',
                        help='(addition) ignore mask of the objectness loss: reference (default) = the reference\'s; truth = a prediction '
                             'without an object is left out when it overlaps a ground-truth box of its own image with IoU >= --ignore_thresh')
    parser.add_argument('--ignore_thresh', dest='ignore_thresh', type=_ignore_thresh_arg, default=0.5,
                        help='(addition) IoU threshold of --ignore_mask truth, in (0, 1] (default 0.5, the paper\'s; reference takes no other)')
    parser.add_argument('--ignore_max_boxes', dest='ignore_max_boxes', type=_ignore_max_boxes_arg, default=1024,
                        help='(addition) ground-truth boxes per image that --ignore_mask truth keeps (default 1024; reference takes no other)')
    parser.add_argument('--focal_gamma', dest='focal_gamma', type=_focal_gamma_arg, default=0.0,
                        help='(addition) 0 (default): off; G > 0: the objectness and / or class term (--focal_terms) becomes the focal loss '
                             'w m^G ce, m = 1 - p_t (training and test loss).  With --model_selection loss: test losses of runs with different '
                             'focal / label-smoothing settings are not comparable')
    parser.add_argument('--focal_alpha', dest='focal_alpha', type=_focal_alpha_arg, default=0.0,
                        help='(addition) balancing factor of --focal_gamma: 0 (default) = none, A in (0, 1) weighs a label z by A z + (1 - A)(1 - z)')
    parser.add_argument('--focal_terms', dest='focal_terms', choices=FOCAL_TERMS, default=None,
                        help='(addition) the terms --focal_gamma applies to: obj, class or both (default both)')
    parser.add_argument('--label_smoothing', dest='label_smoothing', type=_label_smoothing_arg, default=0.0,
                        help='(addition) 0 (default): off; E in (0, 1): the class term is trained against the labels g (1 - E) + E / 2 '
                             '(as Keras BinaryCrossentropy(label_smoothing=E))')
    parser.add_argument('--spp', dest='spp', type=int, choices=(0, 1), default=0,
                        help='(addition) 0 (default): the reference\'s network; 1: YOLOv3-SPP, a 5 / 9 / 13 max-pool pyramid and one more 1x1 '
                             'layer in the block of the coarsest scale (the weight files record it)')
    parser.add_argument('--optimizer', dest='optimizer', choices=OPTIMIZERS, default='adam',
                        help='(addition) adam (default) = the reference\'s Keras Adam; adamw = the same step with decoupled weight decay; '
                             'sgd = SGD with momentum and L2 decay (the weight files record it)')
    parser.add_argument('--momentum', dest='momentum', type=_momentum_arg, default=0.9,
                        help='(addition) momentum of --optimizer sgd, in [0, 1) (default 0.9)')
    parser.add_argument('--nesterov', dest='nesterov', type=int, choices=(0, 1), default=0,
                        help='(addition) 1: Nesterov form of --optimizer sgd')
    parser.add_argument('--weight_decay', dest='weight_decay', type=_weight_decay_arg, default=0.0,
                        help='(addition) 0 (default): none; WD > 0: weight decay on the convolution kernels only, never on biases, gamma or '
                             'beta (needs --optimizer adamw or sgd)')
    parser.add_argument('--lr_schedule', dest='lr_schedule', choices=LR_SCHEDULES, default='reference',
                        help='(addition) reference (default) = learning_rate / 10 during the shortened epoch 0, as the reference; constant, '
                             'cosine or step = learning_rate x a factor of the optimiser step, after a linear warm-up (<scalars>/lr.csv)')
    parser.add_argument('--lr_warmup_steps', dest='lr_warmup_steps', type=_step_count_arg, default=0,
                        help='(addition) optimiser steps of the linear warm-up from --lr_warmup_start_factor to 1 (default 0)')
    parser.add_argument('--lr_warmup_start_factor', dest='lr_warmup_start_factor', type=_unit_factor_arg, default=0.0,
                        help='(addition) factor the warm-up starts from, in [0, 1] (default 0)')
    parser.add_argument('--lr_total_steps', dest='lr_total_steps', type=_step_number_arg, default=None,
                        help='(addition) optimiser step at which --lr_schedule cosine reaches --lr_final_factor (required for cosine, > warm-up)')
    parser.add_argument('--lr_final_factor', dest='lr_final_factor', type=_unit_factor_arg, default=0.01,
                        help='(addition) factor --lr_schedule cosine ends at and holds, in [0, 1] (default 0.01)')
    parser.add_argument('--lr_milestones', dest='lr_milestones', type=_step_number_arg, nargs='*', default=[],
                        help='(addition) optimiser steps, strictly increasing, at each of which --lr_schedule step multiplies the rate by --lr_gamma')
    parser.add_argument('--lr_gamma', dest='lr_gamma', type=_lr_gamma_arg, default=0.1,
                        help='(addition) factor of --lr_schedule step per milestone (default 0.1)')
    parser.add_argument('--init_weights', dest='init_weights', type=str, default=None,
                        help='(addition) start from this weight file (written by a training run or save_weights) instead of random weights: '
                             'layers are matched by role, the class count, anchors, batch size, learning rate and optimiser may differ, a '
                             'detection head of another shape keeps its initialisation; every rank reads the file')
    parser.add_argument('--init_optimizer', dest='init_optimizer', type=int, choices=(0, 1), default=0,
                        help='(addition) 1: with --init_weights, also restore the optimiser moments and step count, so that a learning-rate '
                             'schedule continues (the file must hold the same network and optimiser); the epoch counter, the early-stopping '
                             'history and the EMA start fresh all the same')
    parser.add_argument('--freeze_layers', dest='freeze_layers', type=_freeze_layers_arg, default=0,
                        help='(addition) 0 (default): every layer trains; N: the first N conv layers are not trainable, their BatchNorm '
                             'included (as Keras layer.trainable = False): no gradients, no optimiser step, no weight decay for them')
    parser.add_argument('--freeze', dest='freeze', choices=tuple(FREEZE_NAMES), default=None,
                        help='(addition) backbone: the same as --freeze_layers 52, the Darknet-53 layers in front of the first yolo block')
    parser.add_argument('--freeze_bn', dest='freeze_bn', type=int, choices=(0, 1), default=0,
                        help='(addition) 1: the BatchNorm of the trainable layers normalises with the stored moving statistics, which are '
                             'not updated; gamma and beta keep training (for batches too small to estimate statistics from)')
    parser.add_argument('--anchors', dest='anchors', type=str, nargs='+', default=None, metavar='W,H',
                        help='(addition) the anchors, as W,H pairs in pixels (at most 16), in place of the reference\'s 64,384 384,64; the '
                             'weight files carry them, so inference.py, inference_tiled.py and evaluate.py need no flag')
    parser.add_argument('--anchors_file', dest='anchors_file', type=str, default=None,
                        help='(addition) take the anchors from this JSON file (find_anchor_sizes.py --metric iou --output)')
    parser.add_argument('--auto_anchors', dest='auto_anchors', type=int, default=None, metavar='K',
                        help='(addition) fit K anchors (1..16) to the boxes of the training database before training starts (IoU k-means and a '
                             'mutation search); <output_dir>/anchors.json records them')
    parser.add_argument('--auto_anchors_evolve', dest='auto_anchors_evolve', type=_step_count_arg, default=1000,
                        help='(addition) mutants tried by the search of --auto_anchors (default 1000; 0: IoU k-means alone)')
    parser.add_argument('--auto_anchors_seed', dest='auto_anchors_seed', type=int, default=0, help='(addition) seed of --auto_anchors')
    parser.add_argument('--auto_anchors_device', dest='auto_anchors_device', choices=('cpu', 'gpu'), default='cpu',
                        help='(addition) where --auto_anchors scores its candidates: cpu (in this process) or gpu (a child process running the '
                             'HIP kernel); the same anchors either way')
    parser.add_argument('--anchor_assignment', dest='anchor_assignment', choices=('all', 'scale'), default=None,
                        help='(addition) all (default): every anchor on every scale, the reference\'s network; scale: each anchor is owned by '
                             'one scale as in YOLOv3 / Darknet (by area: the largest third on stride 32, the smallest on stride 8), a box is a '
                             'positive only on the scale of its best anchor, and head s has A_s (5 + K) channels; needs at least 3 anchors; '
                             'the weight files carry the table, <output_dir>/anchor_scales.json records it')
    parser.add_argument('--anchor_masks', dest='anchor_masks', type=str, default=None, metavar='"I,.. I,.. I,.."',
                        help='(addition) the anchors of stride 32, 16 and 8 as three comma-separated index lists, e.g. "6,7,8 3,4,5 0,1,2": a '
                             'partition of the anchors with no empty part; implies --anchor_assignment scale')
    return parser


if __name__ == "__main__":
    a = build_parser().parse_args()
    print('Arguments:')
    for k, v in vars(a).items():
        print('{} = {}'.format(k, v))
    train_model(a.batch_size, a.test_every_n_steps, a.train_database_filepath, a.test_database_filepath, a.output_folder,
                a.terminate_after_num_epochs_without_test_loss_improvement, a.learning_rate, bool(a.use_augmentation), a.max_epochs, a.reader_count, a.backend,
                a.augmentation_device, bool(a.test_map), a.model_selection, a.test_map_min_box_size, a.ema_decay, a.test_map_nms,
                a.test_map_nms_sigma, a.box_loss, a.box_loss_weight, a.accumulate_steps, a.grad_clip_norm, a.multiscale_min, a.multiscale_max,
                a.multiscale_period, a.multiscale_seed, a.mosaic_prob, a.mosaic_seed, a.mosaic_min_visible, a.ignore_mask, a.ignore_thresh,
                a.ignore_max_boxes, a.focal_gamma, a.focal_alpha, a.focal_terms, a.label_smoothing, bool(a.spp), a.optimizer, a.momentum, bool(a.nesterov),
                a.weight_decay, a.lr_schedule, a.lr_warmup_steps, a.lr_warmup_start_factor, a.lr_total_steps, a.lr_final_factor,
                tuple(a.lr_milestones), a.lr_gamma, a.affine_prob, a.affine_degrees, a.affine_shear, a.affine_scale, a.affine_translate,
                a.affine_fill, a.affine_seed, a.affine_min_visible, a.init_weights, bool(a.init_optimizer), a.freeze_layers, bool(a.freeze_bn),
                a.anchors, a.anchors_file, a.auto_anchors, a.auto_anchors_evolve, a.auto_anchors_seed, a.auto_anchors_device,
                photo_prob=a.photo_prob, photo_hue=a.photo_hue, photo_saturation=a.photo_saturation, photo_value=a.photo_value,
                photo_gamma=a.photo_gamma, photo_white=a.photo_white, photo_seed=a.photo_seed, mixup_prob=a.mixup_prob,
                mixup_spread=a.mixup_spread, mixup_seed=a.mixup_seed, anchor_assignment=a.anchor_assignment, anchor_masks=a.anchor_masks)
