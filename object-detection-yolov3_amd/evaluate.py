#!/usr/bin/env python3
"""evaluate.py -- detection accuracy of a saved model: AP per class and IoU threshold, mAP@0.5 and mAP@0.5:0.95.

Not in the reference.  The images go through inference.py's path (per-image z-score -> network -> clip -> small-box
filter -> class-wise NMS, same defaults) and the NMS keep lists are matched against the ground truth on the GPU
(yolo3.metrics.DetectionEvaluator; the metric is defined in DESIGN §3.6).  Ground truth comes from either
  --database      an lmdb written by build_lmdb.py (the records as stored: no augmentation), or
  --image-folder + --csv-folder   images and X,Y,W,H,C csv files of the same basename (build_lmdb.py's input).
Under `python -m torch.distributed.run --nproc-per-node N` every rank evaluates every N-th example (keys[rank::N]) and
the ranks' evaluators are merged (yolo3.metrics.all_gather_evaluator, a collective); rank 0 prints and writes the csv.
--area-ranges scores every class once per range of box area (COCO's AP small / medium / large with its ignore rule),
--operating-points and --pr-curves write the best-F1 score threshold and the PR curve per class, range and IoU threshold
(DESIGN §3.16); they go with every other flag.  --score-thresholds cuts every class's detections at its own score threshold
(a number, or the csv --operating-points wrote) and --confusion-matrix writes the class-agnostic confusion matrix of the
detections that are left; they too go with every other flag.
"""
import argparse
import math
import os
import time

import numpy as np
import torch

from yolo3 import bbox_utils, imagereader, metrics
from yolo3.model import YoloV3


def load_model(path):
    if os.path.isdir(path):
        path = os.path.join(path, 'yolov3.npz')
    return YoloV3.from_file(path)


def database_examples(path, num_shards=1, shard_index=0):
    """(name, HWC uint8 image, [G,5] X,Y,W,H,C) of every num_shards-th record from shard_index on, in key order."""
    return metrics.database_examples(path, num_shards, shard_index)


def folder_examples(image_folder, csv_folder, image_format, num_shards=1, shard_index=0):
    """(name, HWC image, [G,5] X,Y,W,H,C) of every image of the folder, sorted by file name (every num_shards-th from
    shard_index on); the csv of image a.tif is <csv_folder>/a.csv (build_lmdb.py); a missing csv means no ground truth."""
    ext = '.' + image_format.lstrip('.')
    for fn in sorted(f for f in os.listdir(image_folder) if f.endswith(ext))[shard_index::num_shards]:
        img = imagereader.imread(os.path.join(image_folder, fn))
        stem = fn[:-len(ext)]
        yield fn, (img[:, :, None] if img.ndim == 2 else img), bbox_utils.load_boxes_to_xywhc(os.path.join(csv_folder, stem + '.csv'))


def evaluate(examples, saved_model_filepath, min_box_size, precision='fp32', batch_size=8, iou_thresholds=metrics.COCO_IOU_THRESHOLDS,
             max_detections=None, distributed=False, nms='hard', nms_sigma=0.5, tta='none', tta_vote_iou=None, tta_score='keep',
             area_ranges=None, area_names=None, curves=False, letterbox=False, class_score_thresholds=None, confusion=False):
    """Runs the model over ``examples`` and returns (DetectionEvaluator.result() dict, number of images, seconds).
    distributed: a collective over the default process group; every rank passes its keys[rank::world] share of the
    examples and gets the result over all of them.  nms / nms_sigma: the NMS method (bbox_utils.NMS_METHODS) and its
    Gaussian parameter.  tta / tta_vote_iou / tta_score: test-time augmentation (metrics.evaluate_examples).  area_ranges /
    area_names / curves / class_score_thresholds / confusion: DetectionEvaluator's.  letterbox: images of any size, each
    letterboxed into the model input (not with tta; metrics.evaluate_examples)."""
    bbox_utils.check_nms_args(nms, nms_sigma)
    bbox_utils.check_tta_args(tta, tta_vote_iou, tta_score)
    yolo = load_model(saved_model_filepath)
    yolo.inference_precision = precision
    ev = metrics.DetectionEvaluator(yolo.number_classes, iou_thresholds, max_detections, area_ranges=area_ranges, area_names=area_names,
                                    curves=curves, class_score_thresholds=_resolve_cuts(class_score_thresholds, yolo.number_classes),
                                    confusion=confusion)
    t0 = time.perf_counter()
    metrics.evaluate_examples(yolo, examples, ev, min_box_size, batch_size, nms=nms, nms_sigma=nms_sigma, tta=tta, tta_vote_iou=tta_vote_iou,
                              tta_score=tta_score, letterbox=letterbox)
    if distributed:
        ev = metrics.all_gather_evaluator(ev)
    res = ev.result()
    torch.cuda.synchronize()
    return res, ev.num_images, time.perf_counter() - t0


def evaluate_tiled(examples, saved_model_filepath, tile_size, min_box_size, precision='fp32', batch_size=None,
                   iou_thresholds=metrics.COCO_IOU_THRESHOLDS, max_detections=None, distributed=False, nms='hard', nms_sigma=0.5,
                   seam_margin=0.0, merge_nms='none', merge_nms_sigma=0.5, area_ranges=None, area_names=None, curves=False,
                   class_score_thresholds=None, confusion=False, tile_tta='none', tta_vote_iou=None, tta_score='keep'):
    """``evaluate`` for the tiled pipeline (inference_tiled.py with --merge-device gpu): every image, of any size, is cut
    into tiles, the tiles' detections are merged on the device (seam_margin) and the pool is matched against the
    whole-image ground truth there (DetectionEvaluator.add_pool with nms=merge_nms).  batch_size: tiles per network launch
    (None: inference_tiled's default).  area_ranges / area_names / curves / class_score_thresholds / confusion:
    DetectionEvaluator's.  tile_tta / tta_vote_iou / tta_score: test-time augmentation of every tile
    (inference_tiled.inference_image_tiled).  Returns (result dict, number of images, seconds)."""
    import inference_tiled
    bbox_utils.check_nms_args(nms, nms_sigma)
    bbox_utils.check_merge_args('gpu', seam_margin, merge_nms, merge_nms_sigma, inference_tiled.EDGE_EFFECT_RANGE)
    bbox_utils.check_tta_args(tile_tta, tta_vote_iou, tta_score, tile_size)
    yolo = load_model(saved_model_filepath)
    yolo.inference_precision = precision
    if list(tile_size) != list(yolo.img_size[:2]):
        raise RuntimeError('tile size {} must equal the size the model was trained at {} (Q18)'.format(list(tile_size), yolo.img_size[:2]))
    model = yolo.get_keras_model()
    ev = metrics.DetectionEvaluator(yolo.number_classes, iou_thresholds, max_detections, area_ranges=area_ranges, area_names=area_names,
                                    curves=curves, class_score_thresholds=_resolve_cuts(class_score_thresholds, yolo.number_classes),
                                    confusion=confusion)
    t0 = time.perf_counter()
    for _, img, gt in examples:
        pool, count, _ = inference_tiled.tiled_pool_device(model, img, tile_size, min_box_size, batch_size, nms, nms_sigma, seam_margin,
                                                           tile_tta, tta_vote_iou, tta_score)
        ev.add_pool(pool, count, gt, nms=merge_nms, nms_sigma=merge_nms_sigma)
    if distributed:
        ev = metrics.all_gather_evaluator(ev)
    res = ev.result()
    torch.cuda.synchronize()
    return res, ev.num_images, time.perf_counter() - t0


def _resolve_cuts(spec, num_classes):
    """class_score_thresholds of evaluate / evaluate_tiled: None, values, or a callable of the model's class count (the command
    line's: the csv can only be checked once the model is loaded)."""
    return spec(num_classes) if callable(spec) else spec


def _fmt(v):
    return '' if isinstance(v, float) and math.isnan(v) else repr(float(v))


def parse_area_ranges(values):
    """--area-ranges: ['coco'], or LO:HI strings and 'all' (every area: a leading '-inf' would read as an option) ->
    (area_ranges, area_names) of DetectionEvaluator; a range is named by its text (raises ValueError)."""
    if len(values) == 1 and values[0] == 'coco':
        return metrics.check_area_ranges('coco')
    out = []
    for v in values:
        lo, sep, hi = ('-inf', ':', 'inf') if v == 'all' else v.partition(':')
        if not sep:
            raise ValueError("--area-ranges: 'coco', or 'all' and LO:HI pairs, got {!r}".format(v))
        out.append((float(lo), float(hi)))
    return metrics.check_area_ranges(out, values)


def write_operating_points(res, path):
    """One row per class, range and IoU threshold: the best-F1 score cut (keep score >= score_threshold) and what it yields."""
    with open(path, 'w') as fh:
        fh.write('class,range,iou_threshold,score_threshold,precision,recall,f1,tp,fp,npos\n')
        for c in range(res['ap'].shape[0]):
            for a, name in enumerate(res['area_names']):
                for t, thr in enumerate(res['iou_thresholds']):
                    fh.write(','.join([str(c), name, repr(float(thr)), _fmt(float(res['best_score'][a, c, t])),
                                       _fmt(float(res['best_precision'][a, c, t])), _fmt(float(res['best_recall'][a, c, t])),
                                       _fmt(float(res['best_f1'][a, c, t])), str(int(res['best_tp'][a, c, t])),
                                       str(int(res['best_fp'][a, c, t])), str(int(res['npos_area'][c, a]))]) + '\n')


def write_pr_curves(res, path):
    """One row per class, range, IoU threshold and recall point j / 100: the envelope precision there and the score at which
    that recall is first reached (empty where it never is)."""
    with open(path, 'w') as fh:
        fh.write('class,range,iou_threshold,recall,precision,score\n')
        for c in range(res['ap'].shape[0]):
            for a, name in enumerate(res['area_names']):
                for t, thr in enumerate(res['iou_thresholds']):
                    for j in range(101):
                        fh.write(','.join([str(c), name, repr(float(thr)), repr(j / 100), _fmt(float(res['pr_precision'][a, c, t, j])),
                                           _fmt(float(res['pr_score'][a, c, t, j]))]) + '\n')


def write_confusion_matrix(res, path):
    """One row per IoU threshold and true class, then a 'background' row (the unmatched detections per predicted class); the last
    column counts the missed ground-truth boxes of the row's class."""
    K = res['confusion'].shape[1] - 1
    with open(path, 'w') as fh:
        fh.write(','.join(['iou_threshold', 'true'] + ['pred_%d' % c for c in range(K)] + ['missed']) + '\n')
        for t, thr in enumerate(res['iou_thresholds']):
            for g in range(K + 1):
                fh.write(','.join([repr(float(thr)), str(g) if g < K else 'background'] + [str(int(v)) for v in res['confusion'][t, g]]) + '\n')


def write_csv(res, path, area_columns=False):
    """One row per class, then a 'mean' row (mean over the classes with ground truth; NaN cells are empty).  area_columns:
    append one ap_<range name> column per area range (the class's mean AP over the thresholds in that range)."""
    thr = res['iou_thresholds']
    names = res['area_names'] if area_columns else []
    with open(path, 'w') as fh:
        fh.write(','.join(['class', 'npos', 'tp', 'fp', 'precision', 'recall', 'f1', 'ap'] + ['ap@%.2f' % t for t in thr] +
                          ['ap_' + n for n in names]) + '\n')
        valid = res['npos'] > 0
        for c in range(res['ap'].shape[0]):
            ap_mean = float(res['ap'][c].mean()) if valid[c] else float('nan')
            cells = [str(c), str(int(res['npos'][c])), str(int(res['tp50'][c])), str(int(res['fp50'][c])), _fmt(res['precision50'][c]),
                     _fmt(res['recall50'][c]), _fmt(res['f1_50'][c]), _fmt(ap_mean)] + [_fmt(v) for v in res['ap'][c]]
            cells += [_fmt(float(res['ap_area'][a, c].mean())) for a in range(len(names))]         # NaN where the range holds no GT of c
            fh.write(','.join(cells) + '\n')
        fh.write(','.join(['mean', str(int(res['npos'].sum())), '', '', '', '', '', _fmt(res['map_all'])] + [_fmt(v) for v in res['map']] +
                          [_fmt(float(np.mean(res['map_area'][a]))) for a in range(len(names))]) + '\n')


def print_table(res):
    thr = res['iou_thresholds']
    op = res['op_threshold']
    print('{:>6} {:>7} {:>7} {:>7} {:>9} {:>9} {:>9} {:>9} {:>9}'.format('class', 'npos', 'tp', 'fp', 'precision', 'recall', 'f1',
                                                                          'AP@%.2f' % op, 'AP'))
    col = int(np.nonzero(thr == np.float32(op))[0][0])
    for c in range(res['ap'].shape[0]):
        print('{:>6} {:>7d} {:>7d} {:>7d} {:>9.4f} {:>9.4f} {:>9.4f} {:>9.4f} {:>9.4f}'.format(
            c, int(res['npos'][c]), int(res['tp50'][c]), int(res['fp50'][c]), res['precision50'][c], res['recall50'][c], res['f1_50'][c],
            res['ap'][c, col], float(np.mean(res['ap'][c]))))
    print('tp / fp / precision / recall / f1 at IoU {:.2f}; AP = mean over IoU {}'.format(op, ', '.join('%.2f' % t for t in thr)))
    print('mAP50 = {:.4f}  mAP50:95 = {:.4f}  mAP (all thresholds) = {:.4f}'.format(res['map50'], res['map50_95'], res['map_all']))
    for a, name in enumerate(res.get('area_names', [])):
        lo, hi = res['area_ranges'][a]
        print('area {:>8} [{:g}, {:g}]: npos {:d}  AP = {:.4f}  AP50 = {:.4f}  AR = {:.4f}'.format(
            name, lo, hi, int(res['npos_area'][:, a].sum()), float(np.mean(res['map_area'][a])), res['map50_area'][a], res['ar_area'][a]))
    if 'class_score_thresholds' in res:
        print('score thresholds per class: {}'.format(', '.join(repr(float(v)) for v in res['class_score_thresholds'])))
    if 'confusion_op' in res:
        cm = res['confusion_op']
        K = cm.shape[0] - 1
        print('confusion matrix at IoU {:.2f} (rows: true class, columns: predicted class; class-agnostic matching):'.format(op))
        print('{:>10} '.format('true') + ' '.join('{:>7}'.format('pred %d' % c) for c in range(K)) + ' {:>7}'.format('missed'))
        for g in range(K + 1):
            print('{:>10} '.format(g if g < K else 'background') + ' '.join('{:>7d}'.format(int(v)) for v in cm[g]))


if __name__ == '__main__':
    parser = argparse.ArgumentParser(prog='evaluate', description='Script to measure the detection accuracy (AP / mAP) of the selected model')
    parser.add_argument('--saved-model-filepath', type=str, help='Filepath to the saved model to use', required=True)
    parser.add_argument('--database', type=str, default=None, help='lmdb written by build_lmdb.py (e.g. test-<name>.lmdb)')
    parser.add_argument('--image-folder', dest='image_folder', type=str, default=None)
    parser.add_argument('--csv-folder', dest='csv_folder', type=str, default=None, help='X,Y,W,H,C csv per image, same basename')
    parser.add_argument('--image-format', dest='image_format', type=str, default='tif')
    parser.add_argument('--min-box-size', type=int, default=32, help='Smallest detection to consider. Default (32, 32).')
    parser.add_argument('--precision', choices=['fp32', 'bf16'], default='fp32', help='conv arithmetic')
    parser.add_argument('--batch-size', type=int, default=None, help='images per model call (default 8); with --tiled: tiles per network '
                        'launch (default: inference_tiled.py\'s)')
    parser.add_argument('--iou-thresholds', type=float, nargs='+', default=None,
                        help='IoU thresholds (1..32 values in (0, 1]); default 0.50:0.05:0.95')
    parser.add_argument('--max-detections', type=int, default=None, help='detections kept per image and class (default: all NMS keeps)')
    parser.add_argument('--output-file', type=str, default=None, help='per-class csv')
    parser.add_argument('--nms', choices=list(bbox_utils.NMS_METHODS), default='hard',
                        help='NMS method (extension): hard (the reference\'s greedy NMS, default), diou, soft-linear or soft-gaussian')
    parser.add_argument('--nms-sigma', dest='nms_sigma', type=float, default=0.5, help='sigma of --nms soft-gaussian (> 0)')
    parser.add_argument('--tiled', action='store_true', help='score the tiled pipeline (inference_tiled.py --merge-device gpu) on images of any '
                        'size from --image-folder / --csv-folder; needs --tile-height and --tile-width (the size the model was trained at)')
    parser.add_argument('--tile-height', type=int, default=None)
    parser.add_argument('--tile-width', type=int, default=None)
    parser.add_argument('--seam-margin', dest='seam_margin', type=float, default=0.0, metavar='PX',
                        help='--tiled: a tile also keeps centres up to PX inside its ghost band (0 <= PX < 96)')
    parser.add_argument('--merge-nms', dest='merge_nms', choices=list(bbox_utils.MERGE_NMS_METHODS), default='none',
                        help='--tiled: class-wise NMS over the merged detections of the whole image')
    parser.add_argument('--merge-nms-sigma', dest='merge_nms_sigma', type=float, default=0.5, help='sigma of --merge-nms soft-gaussian (> 0)')
    parser.add_argument('--tta', choices=list(bbox_utils.TTA_VIEWS), default='none',
                        help='test-time augmentation (not with --tiled): also run the flipped (hflip, flips) and transposed (d4: square '
                        'inputs) views of every image and pool their detections before --nms; none (default) runs each image once')
    parser.add_argument('--tta-vote-iou', dest='tta_vote_iou', type=float, default=None, metavar='T',
                        help='--tta: replace every kept box by the score-weighted mean of the pooled candidates with IoU >= T (0 < T <= 1)')
    parser.add_argument('--tta-score', dest='tta_score', choices=list(bbox_utils.TTA_SCORES), default='keep',
                        help='--tta with --tta-vote-iou: keep the NMS score (default) or the mean over the views of the best member score')
    parser.add_argument('--tile-tta', dest='tile_tta', choices=list(bbox_utils.TTA_VIEWS), default='none',
                        help='--tiled: test-time augmentation of every tile: also run its flipped (hflip, flips) and transposed (d4: square '
                        'tiles) views and pool their detections before --nms; --batch-size then counts network inputs')
    parser.add_argument('--tile-tta-vote-iou', dest='tile_tta_vote_iou', type=float, default=None, metavar='T',
                        help='--tile-tta: replace every kept box by the score-weighted mean of the pooled candidates with IoU >= T (0 < T <= 1)')
    parser.add_argument('--tile-tta-score', dest='tile_tta_score', choices=list(bbox_utils.TTA_SCORES), default='keep',
                        help='--tile-tta with --tile-tta-vote-iou: keep the NMS score (default) or the mean over the views of the best member score')
    parser.add_argument('--letterbox', action='store_true',
                        help='images of any size (not with --tta or --tiled): rescale each with its aspect ratio kept and pad it to the model '
                        'input on the device; detections are matched in the image\'s own pixels')
    parser.add_argument('--area-ranges', dest='area_ranges', type=str, nargs='+', default=None, metavar='LO:HI',
                        help="also score per range of box area in px^2, both ends closed: 'coco' (all, small <= 32^2, medium, large > 96^2) "
                        "or up to 8 of LO:HI (inf allowed) and 'all'; detections and ground truth outside a range are ignored there, not counted")
    parser.add_argument('--operating-points', dest='operating_points', type=str, default=None, metavar='FILE',
                        help='csv of the score threshold of best F1 per class, area range and IoU threshold')
    parser.add_argument('--pr-curves', dest='pr_curves', type=str, default=None, metavar='FILE',
                        help='csv of the 101-point precision/recall curve per class, area range and IoU threshold')
    parser.add_argument('--score-thresholds', dest='score_thresholds', type=str, default=None, metavar='S|FILE',
                        help='keep a detection only if its score >= the threshold of its class: one number for every class, or the csv '
                        '--operating-points wrote (an empty cell: no cut for that class).  The cut is applied after the NMS: for --nms hard '
                        'and diou, with every cut at or above the base score threshold 0.1, that equals cutting before the NMS (a dropped box '
                        'could only have suppressed boxes scoring below it); for the soft methods it applies to the decayed scores')
    parser.add_argument('--score-thresholds-range', dest='score_thresholds_range', type=str, default='all', metavar='NAME',
                        help='--score-thresholds FILE: the area range whose rows to take (default all)')
    parser.add_argument('--score-thresholds-iou', dest='score_thresholds_iou', type=float, default=0.5, metavar='T',
                        help='--score-thresholds FILE: the IoU threshold whose rows to take (default 0.5)')
    parser.add_argument('--confusion-matrix', dest='confusion_matrix', type=str, default=None, metavar='FILE',
                        help='csv of the confusion matrix per IoU threshold: every detection left after --score-thresholds is matched to '
                        'the ground truth of ANY class; rows true class (+ background), columns predicted class (+ missed)')
    parser.add_argument('--backend', type=str, default='nccl', help='torch.distributed backend under torch.distributed.run: nccl (= RCCL, '
                        'one GPU per rank) or gloo (rehearsal; ranks may share a GPU)')
    a = parser.parse_args()
    if (a.database is None) == (a.image_folder is None and a.csv_folder is None):
        parser.error('give exactly one data source: --database, or --image-folder with --csv-folder')
    if a.database is None and (a.image_folder is None or a.csv_folder is None):
        parser.error('--image-folder and --csv-folder go together')
    if a.tiled:
        if a.database is not None:
            parser.error('--tiled reads whole images: give --image-folder with --csv-folder, not --database')
        if a.tile_height is None or a.tile_width is None:
            parser.error('--tiled needs --tile-height and --tile-width')
        try:
            bbox_utils.check_merge_args('gpu', a.seam_margin, a.merge_nms, a.merge_nms_sigma)
        except ValueError as e:
            parser.error(str(e))
    elif a.tile_height is not None or a.tile_width is not None or a.seam_margin != 0 or a.merge_nms != 'none':
        parser.error('--tile-height, --tile-width, --seam-margin and --merge-nms go with --tiled')
    try:
        bbox_utils.check_tta_args(a.tta, a.tta_vote_iou, a.tta_score)
    except ValueError as e:
        parser.error(str(e))
    if a.tta == 'none' and a.tta_vote_iou is not None:
        parser.error('--tta-vote-iou and --tta-score go with --tta')
    if a.tiled and a.tta != 'none':
        parser.error('--tta does not go with --tiled')
    if not a.tiled and (a.tile_tta != 'none' or a.tile_tta_vote_iou is not None or a.tile_tta_score != 'keep'):
        parser.error('--tile-tta, --tile-tta-vote-iou and --tile-tta-score go with --tiled')
    try:
        bbox_utils.check_tta_args(a.tile_tta, a.tile_tta_vote_iou, a.tile_tta_score, (a.tile_height, a.tile_width) if a.tiled else None)
    except ValueError as e:
        parser.error(str(e))
    if a.tile_tta == 'none' and a.tile_tta_vote_iou is not None:
        parser.error('--tile-tta-vote-iou and --tile-tta-score go with --tile-tta')
    if a.letterbox and (a.tiled or a.tta != 'none'):
        parser.error('--letterbox does not go with --tta or --tiled')
    if a.batch_size is None and not a.tiled:
        a.batch_size = 8
    if a.batch_size is not None and a.batch_size < 1:
        parser.error('--batch-size must be >= 1')
    if a.nms == 'soft-gaussian' and not a.nms_sigma > 0:
        parser.error('--nms-sigma must be > 0')
    if a.max_detections is not None and a.max_detections < 1:
        parser.error('--max-detections must be >= 1')
    thresholds = metrics.COCO_IOU_THRESHOLDS if a.iou_thresholds is None else a.iou_thresholds
    if not 1 <= len(thresholds) <= 32 or not all(0 < t <= 1 for t in thresholds):
        parser.error('--iou-thresholds: 1..32 values in (0, 1]')
    area_ranges = area_names = None
    if a.area_ranges is not None:
        try:
            area_ranges, area_names = parse_area_ranges(a.area_ranges)
        except ValueError as e:
            parser.error(str(e))
    curves = a.operating_points is not None or a.pr_curves is not None
    cuts = None
    if a.score_thresholds is not None:
        def cuts(num_classes):
            return metrics.load_score_thresholds(a.score_thresholds, num_classes, a.score_thresholds_range, a.score_thresholds_iou)
    elif a.score_thresholds_range != 'all' or a.score_thresholds_iou != 0.5:
        parser.error('--score-thresholds-range and --score-thresholds-iou go with --score-thresholds')
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    if world > 1:
        import torch.distributed as dist
        device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count())
        torch.cuda.set_device(device)
        if a.backend == 'nccl':
            dist.init_process_group('nccl', device_id=device)
        else:
            dist.init_process_group(a.backend)
    if rank == 0:
        print('Arguments:')
        for k, v in vars(a).items():
            print('{} = {}'.format(k, v))
    if a.database is not None:
        examples = database_examples(a.database, world, rank)
    else:
        examples = folder_examples(a.image_folder, a.csv_folder, a.image_format, world, rank)
    if a.tiled:
        res, count, secs = evaluate_tiled(examples, a.saved_model_filepath, [a.tile_height, a.tile_width], a.min_box_size, a.precision,
                                          a.batch_size, thresholds, a.max_detections, distributed=world > 1, nms=a.nms, nms_sigma=a.nms_sigma,
                                          seam_margin=a.seam_margin, merge_nms=a.merge_nms, merge_nms_sigma=a.merge_nms_sigma,
                                          area_ranges=area_ranges, area_names=area_names, curves=curves, class_score_thresholds=cuts,
                                          confusion=a.confusion_matrix is not None, tile_tta=a.tile_tta, tta_vote_iou=a.tile_tta_vote_iou,
                                          tta_score=a.tile_tta_score)
    else:
        res, count, secs = evaluate(examples, a.saved_model_filepath, a.min_box_size, a.precision, a.batch_size, thresholds, a.max_detections,
                                    distributed=world > 1, nms=a.nms, nms_sigma=a.nms_sigma, tta=a.tta, tta_vote_iou=a.tta_vote_iou,
                                    tta_score=a.tta_score, area_ranges=area_ranges, area_names=area_names, curves=curves,
                                    letterbox=a.letterbox, class_score_thresholds=cuts, confusion=a.confusion_matrix is not None)
    if rank == 0:
        print('Evaluated {} images in {:.2f} s ({:.1f} images/s)'.format(count, secs, count / secs if secs > 0 else float('nan')))
        print('NMS: {}'.format(a.nms + (' (sigma {:g})'.format(a.nms_sigma) if a.nms == 'soft-gaussian' else '')))
        if a.tta != 'none':
            print('TTA: {} ({} views), {}'.format(a.tta, len(bbox_utils.TTA_VIEWS[a.tta]), 'no voting' if a.tta_vote_iou is None else
                                                  'vote IoU {:g}, score {}'.format(a.tta_vote_iou, a.tta_score)))
        if a.letterbox:
            print('Letterbox: images of any size into the model input, boxes in their own pixels')
        if a.tiled:
            print('Tiled: {} x {} tiles, seam margin {:g}, merge NMS {}'.format(a.tile_height, a.tile_width, a.seam_margin, a.merge_nms))
            if a.tile_tta != 'none':
                print('Tile TTA: {} ({} views), {}'.format(a.tile_tta, len(bbox_utils.TTA_VIEWS[a.tile_tta]), 'no voting' if a.tile_tta_vote_iou is None
                                                           else 'vote IoU {:g}, score {}'.format(a.tile_tta_vote_iou, a.tile_tta_score)))
        print_table(res)
        if a.output_file:
            write_csv(res, a.output_file, area_columns=area_ranges is not None)
        if a.operating_points:
            write_operating_points(res, a.operating_points)
        if a.pr_curves:
            write_pr_curves(res, a.pr_curves)
        if a.confusion_matrix:
            write_confusion_matrix(res, a.confusion_matrix)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
