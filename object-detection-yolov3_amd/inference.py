#!/usr/bin/env python3
"""inference.py -- per image: z-score -> network -> clip -> small-box filter -> class-wise NMS -> X,Y,W,H,C csv.
Reference: inference.py:24-135 (same flags).  --saved-model-filepath points at the weight file written by train.py
(<output_dir>/saved_model/yolov3.npz) instead of a TF SavedModel.  Everything between reading the image and writing
the csv runs on the GPU."""
import argparse
import os

import numpy as np
import torch

from yolo3 import bbox_utils, imagereader, metrics
from yolo3.model import YoloV3


def load_model(path):
    if os.path.isdir(path):
        path = os.path.join(path, 'yolov3.npz')
    return YoloV3.from_file(path)


def write_detections(group, dets, output_folder, image_format):
    """One X,Y,W,H,C csv per image of the group."""
    for img_filepath, (boxes, scores, class_label, _) in zip(group, dets):
        file_name = os.path.split(img_filepath)[1]
        if boxes is None:                                             # the reference would crash here (Q11); write an empty csv
            out = np.zeros((0, 5), np.int32)
        else:
            boxes[:, 2] = boxes[:, 2] - boxes[:, 0]
            boxes[:, 3] = boxes[:, 3] - boxes[:, 1]
            out = np.concatenate((boxes, class_label.reshape(-1, 1)), axis=-1).astype(np.int32)    # truncation (Q20)
        print('Found: {} rois'.format(out.shape[0]))
        bbox_utils.write_boxes_from_xywhc(out, os.path.join(output_folder, file_name.replace(image_format, 'csv')))


def inference(image_folder, image_format, saved_model_filepath, output_folder, min_box_size, precision='fp32', batch_size=8, nms='hard',
              nms_sigma=0.5, tta='none', tta_vote_iou=None, tta_score='keep', letterbox=False, score_thresholds=None, score_thresholds_range='all',
              score_thresholds_iou=0.5):
    """score_thresholds: a number, or the csv evaluate.py --operating-points wrote (its rows of range score_thresholds_range and IoU
    threshold score_thresholds_iou; metrics.load_score_thresholds): a detection is kept only if its score >= the threshold of its
    class, cut on the device behind the NMS (bbox_utils.cut_keep_lists; with tta: on the pooled arrays, filter_class_scores).
    letterbox: the images of the folder may differ in size; each is rescaled with its aspect ratio kept and padded to the model's
    input on the device, and its boxes come back in its own pixels (YoloV3.predict_letterbox); not with tta.
    tta: a view set of bbox_utils.TTA_VIEWS; every image also goes through the network flipped / transposed and the views'
    detections are pooled before the NMS.  tta_vote_iou: box voting over the pool at this IoU (None: the NMS
    alone); tta_score: 'keep' or 'consensus'.  'none' is the path without any of it."""
    bbox_utils.check_nms_args(nms, nms_sigma)
    views = bbox_utils.check_tta_args(tta, tta_vote_iou, tta_score)
    if letterbox and tta != 'none':
        raise ValueError('letterbox does not go with tta')
    os.makedirs(output_folder, exist_ok=True)
    if image_format.startswith('.'):
        image_format = image_format[1:]
    img_filepath_list = [os.path.join(image_folder, fn) for fn in os.listdir(image_folder) if fn.endswith('.{}'.format(image_format))]
    # replicas only (no collective): under `python -m torch.distributed.run --nproc-per-node N` every rank takes every N-th image
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    if world > 1:
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count())
        img_filepath_list = sorted(img_filepath_list)[rank::world]
    yolo = load_model(saved_model_filepath)
    yolo.inference_precision = precision          # 'bf16': bf16 MFMA convs, fp32 heads / decode / NMS (not in the reference)
    yolo_model = yolo.get_keras_model()
    cuts = None if score_thresholds is None else metrics.load_score_thresholds(score_thresholds, yolo.number_classes, score_thresholds_range,
                                                                              score_thresholds_iou)
    print('Starting inference of file list')
    # The reference runs one image per model call (inference.py:40-101).  Here up to `batch_size` images go through the
    # network together; each is still z-scored with its own statistics and clipped / filtered / NMS'ed on its own.
    for g0 in range(0, len(img_filepath_list), batch_size):
        group = img_filepath_list[g0:g0 + batch_size]
        imgs = []
        for i, img_filepath in enumerate(group):
            print('{}/{} : {}'.format(g0 + i, len(img_filepath_list), os.path.split(img_filepath)[1]))
            img = imagereader.imread(img_filepath)
            imgs.append(img[:, :, None] if img.ndim == 2 else img)
        if letterbox:
            # --letterbox (extension): any sizes; the kernel has clipped the boxes to each image, --min-box-size is in its own pixels
            dets, step = [], yolo.LETTERBOX_MAX_BATCH
            for s0 in range(0, len(group), step):
                rows, _ = yolo.predict_letterbox(imgs[s0:s0 + step])
                dets += bbox_utils.detect(rows, min_box_size, clip_wh=None, method=nms, sigma=nms_sigma, class_score_thresholds=cuts)
            write_detections(group, dets, output_folder, image_format)
            continue
        height, width, channels = imgs[0].shape
        if any(im.shape != imgs[0].shape for im in imgs):
            raise RuntimeError('images of one folder must share one size (the model input is fixed, Q18): {}'.format({im.shape for im in imgs}))
        x = torch.from_numpy(np.stack([np.ascontiguousarray(im.astype(np.float32).transpose((2, 0, 1))) for im in imgs])).cuda()
        x = imagereader.zscore_normalize_device(x)                       # per-image statistics (inference.py:49)
        if tta == 'none':
            rows = yolo_model(x, training=False)                              # [B, Nb, 5+K]
            # clip to the image (the intent of inference.py:62-65, Q11), small-box filter (:72), class-wise NMS (:79)
            dets = bbox_utils.detect(rows, min_box_size, clip_wh=(width, height), method=nms, sigma=nms_sigma,   # --nms: extension
                                     class_score_thresholds=cuts)
        else:
            # --tta (extension): the views of a few images per network call, pooled per image, then the same clip / filter / NMS
            bbox_utils.check_tta_args(tta, tta_vote_iou, tta_score, (height, width))
            dets, step = [], bbox_utils.tta_group_size(views)
            for s0 in range(0, len(group), step):
                rows = yolo.predict_tta(x[s0:s0 + step], views)              # [b, k * Nb, 5+K], boxes in the image's frame
                dets += bbox_utils.detect_tta(rows, len(views), min_box_size, clip_wh=(width, height), method=nms, sigma=nms_sigma,
                                              vote_iou=tta_vote_iou, score=tta_score)
            if cuts is not None:
                dets = bbox_utils.filter_class_scores(dets, cuts)
        write_detections(group, dets, output_folder, image_format)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(prog='inference', description='Script to detect stars with the selected model')
    parser.add_argument('--saved-model-filepath', type=str, help='Filepath to the saved model to use', required=True)
    parser.add_argument('--output-folder', type=str, required=True)
    parser.add_argument('--image-folder', dest='image_folder', type=str, required=True)
    parser.add_argument('--image-format', dest='image_format', type=str, default='tif')
    parser.add_argument('--min-box-size', type=int, default=32, help='Smallest detection to consider. Default (32, 32).')
    parser.add_argument('--precision', choices=['fp32', 'bf16'], default='fp32', help='conv arithmetic (extension; the reference is fp32)')
    parser.add_argument('--batch-size', type=int, default=8, help='images per model call (extension; the reference runs one)')
    parser.add_argument('--nms', choices=list(bbox_utils.NMS_METHODS), default='hard',
                        help='NMS method (extension): hard (the reference\'s greedy NMS, default), diou, soft-linear or soft-gaussian')
    parser.add_argument('--nms-sigma', dest='nms_sigma', type=float, default=0.5, help='sigma of --nms soft-gaussian (> 0)')
    parser.add_argument('--tta', choices=list(bbox_utils.TTA_VIEWS), default='none',
                        help='test-time augmentation (extension): also run the flipped (hflip, flips) and transposed (d4: square inputs) '
                        'views of every image and pool their detections before --nms; none (default) runs each image once')
    parser.add_argument('--tta-vote-iou', dest='tta_vote_iou', type=float, default=None, metavar='T',
                        help='--tta: replace every kept box by the score-weighted mean of the pooled candidates with IoU >= T (0 < T <= 1)')
    parser.add_argument('--tta-score', dest='tta_score', choices=list(bbox_utils.TTA_SCORES), default='keep',
                        help='--tta with --tta-vote-iou: keep the NMS score (default) or the mean over the views of the best member score')
    parser.add_argument('--letterbox', action='store_true',
                        help='images of any size (extension): rescale each with its aspect ratio kept and pad it to the model input on '
                        'the device; boxes and --min-box-size are in the image\'s own pixels (not with --tta)')
    parser.add_argument('--score-thresholds', dest='score_thresholds', type=str, default=None, metavar='S|FILE',
                        help='keep a detection only if its score >= the threshold of its class (extension): one number for every class, or '
                        'the csv evaluate.py --operating-points wrote (an empty cell: no cut for that class).  The cut is applied after the '
                        'NMS: for --nms hard and diou, with every cut at or above the base score threshold 0.1, that equals cutting before the '
                        'NMS (a dropped box could only have suppressed boxes scoring below it); for the soft methods it applies to the '
                        'decayed scores')
    parser.add_argument('--score-thresholds-range', dest='score_thresholds_range', type=str, default='all', metavar='NAME',
                        help='--score-thresholds FILE: the area range whose rows to take (default all)')
    parser.add_argument('--score-thresholds-iou', dest='score_thresholds_iou', type=float, default=0.5, metavar='T',
                        help='--score-thresholds FILE: the IoU threshold whose rows to take (default 0.5)')
    a = parser.parse_args()
    if a.score_thresholds is None and (a.score_thresholds_range != 'all' or a.score_thresholds_iou != 0.5):
        parser.error('--score-thresholds-range and --score-thresholds-iou go with --score-thresholds')
    if a.letterbox and a.tta != 'none':
        parser.error('--letterbox does not go with --tta')
    if a.nms == 'soft-gaussian' and not a.nms_sigma > 0:
        parser.error('--nms-sigma must be > 0')
    try:
        bbox_utils.check_tta_args(a.tta, a.tta_vote_iou, a.tta_score)
    except ValueError as e:
        parser.error(str(e))
    if a.tta == 'none' and a.tta_vote_iou is not None:
        parser.error('--tta-vote-iou and --tta-score go with --tta')
    print('Arguments:')
    for k, v in vars(a).items():
        print('{} = {}'.format(k, v))
    inference(a.image_folder, a.image_format, a.saved_model_filepath, a.output_folder, a.min_box_size, a.precision, a.batch_size, a.nms, a.nms_sigma,
              a.tta, a.tta_vote_iou, a.tta_score, a.letterbox, a.score_thresholds, a.score_thresholds_range, a.score_thresholds_iou)
