"""Host mirror of the reference's imagereader.py pieces that sit on the hot-path
contract: z-score normalisation (GPU kernel), HWC->CHW formatting and the
ground-truth label layout the loss consumes.

ImageReader       imagereader.py:79-460  (lmdb + protobuf datasets, worker processes, bounded queue)
zscore_normalize  imagereader.py:34-46   (csrc/pointwise.hip, fp64 partial sums)
augment_device    augment.py:30-125 on the device (csrc/augment.hip) for ImageReader(..., augmentation_device='gpu')
format_image      imagereader.py:57-60
format_boxes      ImageReader.__format_boxes, imagereader.py:252-324 (host NumPy,
                  as in the reference: it runs in the reader processes)
mosaic_device     y3_mosaic_batch (csrc/augment.hip): the augmented batch recombined, four windows per output image, for
                  Dataset.mosaic() (not in the reference)
affine_device     y3_affine_batch (csrc/augment.hip): every image of the batch warped through an affine map, bilinear, for
                  Dataset.affine() (not in the reference)
photometric_device  y3_photometric_batch (csrc/augment.hip): colour matrix, clamp, tone curve and MixUp of the batch in one
                  elementwise pass, for Dataset.photometric() / Dataset.mixup() (not in the reference)
format_labels_device  the same three label tensors built on the device from the boxes of a batch (y3_format_labels,
                  csrc/detect.hip) for ImageReader(..., label_device='gpu') and Dataset.multiscale()
"""
import multiprocessing
import os
import queue
import random
import traceback

import numpy as np
import torch

from ._hip import lib, check, float_array, int_array
from .anchors import check_anchor_scales
from . import augment
from . import lmdbio
from .isg_ai_pb import ImageYoloBoxesPair

NETWORK_DOWNSAMPLE_FACTOR = 32   # model.YoloV3.NETWORK_DOWNSAMPLE_FACTOR (model.py:25)
# augment_image_box_pair's arguments in the training reader (imagereader.py:369-391)
TRAIN_AUGMENTATION = dict(reflection_flag=True, rotation_flag=False, noise_augmentation_severity=0.03, scale_augmentation_severity=0.1,
                          blur_augmentation_max_sigma=2, box_size_augmentation_severity=0.03, box_location_jitter_severity=0.03)
_AUG_DTYPES = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}


def zscore_normalize_device(x):
    """x: CUDA float32 tensor [B, ...]; each x[b] is normalised with its own
    whole-tensor mean / population std (imagereader.py:34-46)."""
    assert x.is_cuda and x.dtype == torch.float32
    x = x.contiguous()
    b = x.shape[0]
    count = x[0].numel()
    out = torch.empty_like(x)
    ws = torch.empty(int(lib.y3_zscore_workspace_bytes(b)) // 8 + 1, dtype=torch.float64, device=x.device)
    st = torch.cuda.current_stream(x.device).cuda_stream
    check(lib.y3_zscore(x.data_ptr(), out.data_ptr(), b, count, ws.data_ptr(), st), 'y3_zscore')
    return out


def augment_device(src, records, crop_to, ranges=False):
    """y3_augment_batch: src CUDA [B, H, W, C] (uint8, uint16 or float32, HWC as stored), records AUG_RECORD [B] (host; see
    augment.draw_augmentation) -> float32 [B, C, crop_h, crop_w], resampled / cropped / flipped / noised / blurred, NOT z-scored.
    Enqueued on the current stream.  ranges=True also returns the per-image (min, max) of the resampled crop the noise was
    scaled by (CUDA float32 [B] each)."""
    assert src.is_cuda and src.dim() == 4 and src.dtype in _AUG_DTYPES, (src.dtype, tuple(src.shape))
    src = src.contiguous()
    records = np.ascontiguousarray(records, dtype=augment.AUG_RECORD)
    b, h, w, c = src.shape
    assert records.shape == (b,)
    ho, wo = int(crop_to[0]), int(crop_to[1])
    out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=src.device)
    ws = torch.empty(int(lib.y3_augment_workspace_bytes(b, ho, wo, c)), dtype=torch.uint8, device=src.device)
    st = torch.cuda.current_stream(src.device).cuda_stream
    check(lib.y3_augment_batch(src.data_ptr(), _AUG_DTYPES[src.dtype], b, h, w, c, records.ctypes.data, ho, wo, out.data_ptr(),
                               ws.data_ptr(), st), 'y3_augment_batch')
    if not ranges:
        return out
    enc = ws[:8 * b].view(torch.int32).view(b, 2).to(torch.int64) & 0xffffffff      # yolo3hip.h: encoded max, encoded -min
    bits = torch.where(enc >= 2**31, enc - 2**31, 2**32 - 1 - enc)
    bits = torch.where(bits >= 2**31, bits - 2**32, bits).to(torch.int32)
    val = bits.view(torch.float32)
    return out, -val[:, 1], val[:, 0]


def mosaic_device(x, records):
    """y3_mosaic_batch: x CUDA float32 [B, C, H, W] (C = 1 or 3), records MOSAIC_RECORD [B] (host; see augment.draw_mosaic) -> a new
    tensor of the same shape, every output image copied together from windows of up to four images of x.  Enqueued on the current
    stream."""
    assert x.is_cuda and x.dim() == 4 and x.dtype == torch.float32, (x.dtype, tuple(x.shape))
    x = x.contiguous()
    records = np.ascontiguousarray(records, dtype=augment.MOSAIC_RECORD)
    b, c, h, w = x.shape
    assert records.shape == (b,)
    out = torch.empty_like(x)
    st = torch.cuda.current_stream(x.device).cuda_stream
    check(lib.y3_mosaic_batch(x.data_ptr(), b, c, h, w, records.ctypes.data, out.data_ptr(), st), 'y3_mosaic_batch')
    return out


def affine_device(x, records):
    """y3_affine_batch: x CUDA float32 [B, C, H, W] (C = 1 or 3), records AFFINE_RECORD [B] (host; see augment.draw_affine) -> a new
    tensor of the same shape, every image warped through its record's inverse map (bilinear, `fill` outside).  Enqueued on the
    current stream."""
    assert x.is_cuda and x.dim() == 4 and x.dtype == torch.float32, (x.dtype, tuple(x.shape))
    x = x.contiguous()
    records = np.ascontiguousarray(records, dtype=augment.AFFINE_RECORD)
    b, c, h, w = x.shape
    assert records.shape == (b,)
    out = torch.empty_like(x)
    st = torch.cuda.current_stream(x.device).cuda_stream
    check(lib.y3_affine_batch(x.data_ptr(), b, c, h, w, records.ctypes.data, out.data_ptr(), st), 'y3_affine_batch')
    return out


def photometric_device(x, records):
    """y3_photometric_batch: x CUDA float32 [B, C, H, W] (C = 1 or 3), records PHOTO_RECORD [B] (host; see augment.draw_photometric
    and augment.draw_mixup) -> a new tensor of the same shape: every image through its record's colour matrix, clamp and tone
    curve, then blended with its partner's finished image where lambda < 1.  Enqueued on the current stream."""
    assert x.is_cuda and x.dim() == 4 and x.dtype == torch.float32, (x.dtype, tuple(x.shape))
    x = x.contiguous()
    records = np.ascontiguousarray(records, dtype=augment.PHOTO_RECORD)
    b, c, h, w = x.shape
    assert records.shape == (b,)
    out = torch.empty_like(x)
    st = torch.cuda.current_stream(x.device).cuda_stream
    check(lib.y3_photometric_batch(x.data_ptr(), b, c, h, w, records.ctypes.data, out.data_ptr(), st), 'y3_photometric_batch')
    return out


def format_labels_device(boxes, counts, image_size, anchors, number_classes, anchor_scale=None):
    """y3_format_labels: boxes CUDA int32 [B, M, 5] (x, y, w, h, class; top-left corner; M may be 0), counts CUDA int32 [B] ->
    the three float32 label tensors [B, G, G, A, 5+K] of format_boxes (bit-identical per image), written completely by one
    launch on the current stream.  anchor_scale (an owner table [A]): y3_format_labels_scales, [B, G, G, A_s, 5+K]."""
    assert boxes.is_cuda and boxes.dtype == torch.int32 and boxes.dim() == 3 and boxes.shape[2] == 5, (boxes.dtype, tuple(boxes.shape))
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.shape == (boxes.shape[0],), (counts.dtype, tuple(counts.shape))
    boxes, counts = boxes.contiguous(), counts.contiguous()
    b, m = int(boxes.shape[0]), int(boxes.shape[1])
    h, w = int(image_size[0]), int(image_size[1])
    a, k = len(anchors), int(number_classes)
    f = NETWORK_DOWNSAMPLE_FACTOR
    anchors_c = float_array([float(v) for an in anchors for v in an])
    st = torch.cuda.current_stream(boxes.device).cuda_stream
    if anchor_scale is not None:
        owner = check_anchor_scales(anchor_scale, a)
        out = [torch.empty((b, h // (f >> s), w // (f >> s), owner.count(s), 5 + k), dtype=torch.float32, device=boxes.device) for s in range(3)]
        check(lib.y3_format_labels_scales(boxes.data_ptr() if m else None, counts.data_ptr(), b, m, anchors_c, int_array(owner), a, k, h, w,
                                          out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), st), 'y3_format_labels_scales')
        return out
    out = [torch.empty((b, h // (f >> s), w // (f >> s), a, 5 + k), dtype=torch.float32, device=boxes.device) for s in range(3)]
    check(lib.y3_format_labels(boxes.data_ptr() if m else None, counts.data_ptr(), b, m, anchors_c, a, k, h, w,
                               out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), st), 'y3_format_labels')
    return out


def collate_boxes(box_lists, out=None):
    """Boxes of a batch, [k_i, 5] each (None = none) -> (boxes int32 [B, M, 5] zero-padded, counts int32 [B]) with M the batch
    maximum (at least 1): nothing is dropped.  out: optional (boxes, counts) arrays to fill, boxes with room for M."""
    counts = np.array([0 if b is None else len(b) for b in box_lists], np.int32)
    m = max(1, int(counts.max()) if len(counts) else 1)
    if out is None:
        boxes = np.zeros((len(box_lists), m, 5), np.int32)
    else:
        boxes, cdst = out
        assert boxes.shape[1] >= m
        boxes[...] = 0
        cdst[...] = counts
        counts = cdst
    for i, b in enumerate(box_lists):
        if counts[i]:
            boxes[i, :counts[i]] = b
    return boxes, counts


def zscore_normalize(image_data):
    """imagereader.py:34-46 on one image (any layout / dtype) -> float32 ndarray."""
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(image_data).astype(np.float32))).cuda()
    return zscore_normalize_device(x[None])[0].cpu().numpy()


def format_image(image_data):
    """imagereader.py:57-60: HWC -> CHW."""
    return np.transpose(image_data, [2, 0, 1])


def format_boxes(boxes, image_size, anchors, number_classes, anchor_scale=None):
    """ImageReader.__format_boxes (imagereader.py:252-324).

    boxes [n,5] = [x, y, w, h, class] with (x, y) the top-left corner.  Returns
    three float32 label tensors [G, G, A, 5+K] (G = size/32, /16, /8).  The box
    centre is floor(xy + (wh-1)/2); the best anchor (IoU of co-centred w,h) is
    written at the SAME anchor slot of all three scales (Q5).

    anchor_scale (addition): an owner table [A] of scales 0..2 gives [G, G, A_s, 5+K] instead: the box goes only to
    the scale that owns its best anchor (still the best of ALL anchors), at that anchor's slot (its rank among the scale's
    anchors).  None runs the reference's code."""
    if anchor_scale is not None:
        return _format_boxes_scales(boxes, image_size, anchors, number_classes, anchor_scale)
    anchors = np.asarray(anchors, dtype=np.float32)
    num_anchors = len(anchors)
    f = NETWORK_DOWNSAMPLE_FACTOR
    grid_sizes = [(int(image_size[0] / f), int(image_size[1] / f)),
                  (int(image_size[0] / (f / 2)), int(image_size[1] / (f / 2))),
                  (int(image_size[0] / (f / 4)), int(image_size[1] / (f / 4)))]
    label = [np.zeros((g[0], g[1], num_anchors, 5 + number_classes), dtype=np.float32) for g in grid_sizes]
    if boxes is None or boxes.shape[0] == 0:
        return label
    boxes = boxes.astype(np.float32)
    box_wh = boxes[:, 2:4]
    boxes[:, 0:2] = np.floor(boxes[:, 0:2] + ((box_wh - 1) / 2.0))
    wh = np.expand_dims(box_wh, -2)
    inter_wh = np.maximum(np.minimum(wh / 2.0, anchors / 2.0) - np.maximum(-wh / 2.0, -anchors / 2.0), 0.0)
    inter = inter_wh[..., 0] * inter_wh[..., 1]
    iou = inter / (wh[..., 0] * wh[..., 1] + anchors[:, 0] * anchors[:, 1] - inter)
    best_anchor = np.argmax(iou, axis=-1)
    for t, n in enumerate(best_anchor):
        for l, g in enumerate(grid_sizes):
            i = np.floor(boxes[t, 1] / image_size[0] * g[0]).astype('int32')
            j = np.floor(boxes[t, 0] / image_size[1] * g[1]).astype('int32')
            c = boxes[t, 4].astype('int32')
            label[l][i, j, n, 0:4] = boxes[t, 0:4]
            label[l][i, j, n, 4] = 1.0
            label[l][i, j, n, 5 + c] = 1.0
    return label


def _format_boxes_scales(boxes, image_size, anchors, number_classes, anchor_scale):
    """format_boxes with every anchor owned by one scale: the same float32 arithmetic, line for line; only the scale loop and the
    slot differ."""
    anchors = np.asarray(anchors, dtype=np.float32)
    owner = check_anchor_scales(anchor_scale, len(anchors))
    slot = [owner[:a].count(owner[a]) for a in range(len(owner))]
    f = NETWORK_DOWNSAMPLE_FACTOR
    grid_sizes = [(int(image_size[0] / f), int(image_size[1] / f)),
                  (int(image_size[0] / (f / 2)), int(image_size[1] / (f / 2))),
                  (int(image_size[0] / (f / 4)), int(image_size[1] / (f / 4)))]
    label = [np.zeros((g[0], g[1], owner.count(l), 5 + number_classes), dtype=np.float32) for l, g in enumerate(grid_sizes)]
    if boxes is None or boxes.shape[0] == 0:
        return label
    boxes = boxes.astype(np.float32)
    box_wh = boxes[:, 2:4]
    boxes[:, 0:2] = np.floor(boxes[:, 0:2] + ((box_wh - 1) / 2.0))
    wh = np.expand_dims(box_wh, -2)
    inter_wh = np.maximum(np.minimum(wh / 2.0, anchors / 2.0) - np.maximum(-wh / 2.0, -anchors / 2.0), 0.0)
    inter = inter_wh[..., 0] * inter_wh[..., 1]
    iou = inter / (wh[..., 0] * wh[..., 1] + anchors[:, 0] * anchors[:, 1] - inter)
    best_anchor = np.argmax(iou, axis=-1)
    for t, n in enumerate(best_anchor):
        l = owner[n]
        g = grid_sizes[l]
        i = np.floor(boxes[t, 1] / image_size[0] * g[0]).astype('int32')
        j = np.floor(boxes[t, 0] / image_size[1] * g[1]).astype('int32')
        c = boxes[t, 4].astype('int32')
        label[l][i, j, slot[n], 0:4] = boxes[t, 0:4]
        label[l][i, j, slot[n], 4] = 1.0
        label[l][i, j, slot[n], 5 + c] = 1.0
    return label


def inverse_format_boxes(label, batch_id):
    """imagereader.py:63-76: boxes [n,4] = x, y, w, h (top-left) back from a label tensor [B,G,G,A,5+K], anchor 0 only,
    in np.nonzero order; modifies the label rows in place like the reference does."""
    boxes = []
    ii, jj = np.nonzero(label[batch_id, :, :, 0, 4])
    for k in range(len(ii)):
        bb = label[batch_id, ii[k], jj[k], 0, 0:4]
        bb[0] = bb[0] - int(bb[2] / 2)
        bb[1] = bb[1] - int(bb[3] / 2)
        boxes.append(bb)
    return np.vstack(boxes)


def imread(fp):
    """imagereader.py:49-50 (skimage.io.imread there; PIL here).  Returns HWC or HW ndarray."""
    from PIL import Image
    return np.asarray(Image.open(fp))


def imwrite(img, fp):
    from PIL import Image
    Image.fromarray(np.asarray(img)).save(fp)


def _loader_process(reader, worker_id):
    reader._image_loader(worker_id)


class Dataset:
    """What get_tf_dataset() hands out: an iterable of (image[C,H,W], label_1, label_2, label_3); ``batch(n)`` stacks
    n examples and moves them to the GPU, where the images are z-scored by the HIP kernel (the reference z-scores in
    the reader processes on the CPU, imagereader.py:398); ``prefetch(d)`` assembles up to d batches ahead in pinned host
    memory on a background thread (tf.data's prefetch, train.py:61), so that taking examples off the worker queue and
    stacking them overlaps the GPU step instead of preceding it.
    With a label_device='gpu' reader the examples carry their boxes; a batch pads them to its own maximum (with counts) and
    y3_format_labels builds the label tensors on the device.  ``multiscale(sizes, period, seed)`` (such a reader only, DESIGN
    §3.11) gives batch i -- counted over the life of this object, not per epoch -- the size sizes[j], j a pure function of
    (seed, i // period): the batch is augmented straight to that size and its labels are built at it.
    ``mosaic(prob, seed, min_visible)`` (such a reader only) turns each image of a batch, with probability prob, into a
    mosaic of itself and three other images of the same batch: drawn as a pure function of (seed, the reader's shard, i), composed
    on the device after the augmentation at the batch's size, the boxes remapped on the host before they are uploaded.
    ``affine(prob, degrees, shear, scale, translate, fill, seed, min_visible)`` (such a reader only) warps each image
    of a batch, with probability prob, through a random rotation, shear, gain and translation: drawn as a pure function of (seed,
    the reader's shard, i, image), applied on the device after the augmentation and the mosaic and before the z-score, at the
    batch's own size; the boxes are remapped on the host (augment.affine_boxes) after the mosaic's.
    ``photometric(prob, hue, saturation, value, gamma, seed, white)`` (a reader with augmentation_device='gpu') sends
    each image of a batch, with probability prob, through a random colour matrix (hue rotation and saturation gain of the YIQ
    chroma plane, value gain), a clamp to [0, white] and a tone curve; ``mixup(prob, spread, seed)`` (label_device='gpu' as well)
    blends each image, with probability prob, with another finished image of its batch and gives it the boxes of both
    (augment.mixup_boxes, after the affine's).  Both are one device pass, y3_photometric_batch, after the warp and right before the
    z-score, at the batch's own size; a fill region left by the warp goes through the colour transform like any other pixel."""

    def __init__(self, reader, batch_size=None, device=None, prefetch_depth=0, multiscale=None, mosaic=None, affine=None, photometric=None,
                 mixup=None):
        self.reader, self.batch_size, self.device, self.prefetch_depth = reader, batch_size, device, prefetch_depth
        self.multiscale_cfg = multiscale       # None or (sizes [(h, w)], period, seed)
        self.mosaic_cfg = mosaic               # None or (prob, seed, min_visible)
        self.affine_cfg = affine               # None or (prob, degrees, shear, scale, translate, fill, seed, min_visible)
        self.photo_cfg = photometric           # None or (prob, hue, saturation, value, gamma, seed, white)
        self.mixup_cfg = mixup                 # None or (prob, spread, seed)
        self.batches = 0                       # batches handed out so far, over every iteration of this object

    def _with(self, **changes):
        """A Dataset on the same reader with every setting of this one but `changes`."""
        cfg = dict(batch_size=self.batch_size, device=self.device, prefetch_depth=self.prefetch_depth, multiscale=self.multiscale_cfg,
                   mosaic=self.mosaic_cfg, affine=self.affine_cfg, photometric=self.photo_cfg, mixup=self.mixup_cfg)
        cfg.update(changes)
        return Dataset(self.reader, **cfg)

    def batch(self, n):
        return self._with(batch_size=int(n))

    def prefetch(self, n):
        return self._with(prefetch_depth=max(1, min(int(n), 4)))     # batches, not examples: 4 is plenty

    def multiscale(self, sizes, period, seed=0):
        """Multi-scale training: see the class docstring.  sizes: (h, w) pairs, multiples of 32; period: batches per draw."""
        if getattr(self.reader, 'label_device', 'cpu') != 'gpu':
            raise ValueError("multiscale() needs a reader with label_device='gpu': the labels are built at the drawn size")
        sizes = [(int(s[0]), int(s[1])) for s in sizes]
        if not sizes or any(h < 32 or w < 32 or h % 32 or w % 32 for h, w in sizes):
            raise ValueError('multiscale sizes must be (h, w) multiples of {}, got {!r}'.format(NETWORK_DOWNSAMPLE_FACTOR, sizes))
        if isinstance(period, bool) or int(period) != period or int(period) < 1:
            raise ValueError('multiscale period must be an integer >= 1, got {!r}'.format(period))
        return self._with(multiscale=(sizes, int(period), int(seed)))

    def mosaic(self, prob, seed=0, min_visible=0.25):
        """Mosaic augmentation: see the class docstring.  prob: share of mosaic images, 0 < prob <= 1; min_visible: a box stays when
        at least this share of its area lies in the window taken from its image (augment.mosaic_boxes)."""
        if getattr(self.reader, 'label_device', 'cpu') != 'gpu':
            raise ValueError("mosaic() needs a reader with label_device='gpu': label tensors built in the workers cannot be remapped")
        if isinstance(prob, bool) or not 0 < float(prob) <= 1:
            raise ValueError('mosaic prob must be in (0, 1], got {!r}'.format(prob))
        if isinstance(min_visible, bool) or not 0 <= float(min_visible) <= 1:
            raise ValueError('mosaic min_visible must be in [0, 1], got {!r}'.format(min_visible))
        return self._with(mosaic=(float(prob), int(seed), float(min_visible)))

    def affine(self, prob, degrees=10.0, shear=2.0, scale=0.1, translate=0.1, fill=0.0, seed=0, min_visible=0.25):
        """Random affine warp: see the class docstring.  prob: share of warped images, 0 < prob <= 1; degrees in [0, 180]: rotation
        drawn in +-degrees; shear in [0, 45): x and y shear angles in +-shear degrees; scale in [0, 1): gain in 1 +- scale;
        translate in [0, 1]: shift in +-translate of the image side; fill: finite value of the pixels from outside the image (in
        the units of the stored pixels, before the z-score); min_visible: a box stays when at least this share of its transformed
        area lies inside the image (augment.affine_boxes).  The magnitudes are defaults, not tuned values."""
        if getattr(self.reader, 'label_device', 'cpu') != 'gpu':
            raise ValueError("affine() needs a reader with label_device='gpu': label tensors built in the workers cannot be remapped")
        if isinstance(prob, bool) or not 0 < float(prob) <= 1:
            raise ValueError('affine prob must be in (0, 1], got {!r}'.format(prob))
        for name, v, ok in (('degrees', degrees, lambda v: 0 <= v <= 180), ('shear', shear, lambda v: 0 <= v < 45),
                            ('scale', scale, lambda v: 0 <= v < 1), ('translate', translate, lambda v: 0 <= v <= 1),
                            ('fill', fill, np.isfinite), ('min_visible', min_visible, lambda v: 0 <= v <= 1)):
            if isinstance(v, bool) or not ok(float(v)):
                raise ValueError('affine {} out of range, got {!r}'.format(name, v))
        return self._with(affine=(float(prob), float(degrees), float(shear), float(scale), float(translate), float(fill), int(seed), float(min_visible)))

    def photometric(self, prob, hue=0.015, saturation=0.7, value=0.4, gamma=0.0, seed=0, white=None):
        """Colour / tone jitter: see the class docstring.  prob: share of changed images, 0 < prob <= 1; hue in [0, 0.5]: rotation of
        the YIQ chroma plane drawn in +-hue turns; saturation, value in [0, 1]: gains drawn in 1 +- saturation, 1 +- value; gamma in
        [0, 4]: tone exponent 2^(+-gamma) on t / white; white: the top of the stored pixel range (the clamp and the scale of the tone
        curve), by default 255 for a uint8 and 65535 for a uint16 database -- a float32 database must pass it.  A one-channel
        database ignores hue and saturation.  The magnitudes are the common recipe's defaults, not tuned values."""
        if getattr(self.reader, 'augmentation_device', 'cpu') != 'gpu':
            raise ValueError("photometric() needs a reader with augmentation_device='gpu': the pass runs on the device, after the augmentation")
        if isinstance(prob, bool) or not 0 < float(prob) <= 1:
            raise ValueError('photometric prob must be in (0, 1], got {!r}'.format(prob))
        for name, v, ok in (('hue', hue, lambda v: 0 <= v <= 0.5), ('saturation', saturation, lambda v: 0 <= v <= 1),
                            ('value', value, lambda v: 0 <= v <= 1), ('gamma', gamma, lambda v: 0 <= v <= 4)):
            if isinstance(v, bool) or not ok(float(v)):
                raise ValueError('photometric {} out of range, got {!r}'.format(name, v))
        if white is None:
            stored = getattr(self.reader, 'image_dtype', None)
            white = {'uint8': 255.0, 'uint16': 65535.0}.get(str(stored))
            if white is None:
                raise ValueError('photometric() on a {} database needs white: the top of its pixel range is not known'.format(stored))
        if isinstance(white, bool) or not (np.isfinite(float(white)) and float(white) > 0):
            raise ValueError('photometric white must be finite and > 0, got {!r}'.format(white))
        return self._with(photometric=(float(prob), float(hue), float(saturation), float(value), float(gamma), int(seed), float(white)))

    def mixup(self, prob, spread=0.1, seed=0):
        """MixUp: see the class docstring.  prob: share of mixed images, 0 < prob <= 1; spread in [0, 0.5]: lambda uniform in
        0.5 +- spread (a uniform window, not the papers' Beta draw: augment.draw_mixup)."""
        if getattr(self.reader, 'augmentation_device', 'cpu') != 'gpu':
            raise ValueError("mixup() needs a reader with augmentation_device='gpu': the images are blended on the device, after the augmentation")
        if getattr(self.reader, 'label_device', 'cpu') != 'gpu':
            raise ValueError("mixup() needs a reader with label_device='gpu': label tensors built in the workers cannot be merged")
        if isinstance(prob, bool) or not 0 < float(prob) <= 1:
            raise ValueError('mixup prob must be in (0, 1], got {!r}'.format(prob))
        if isinstance(spread, bool) or not 0 <= float(spread) <= 0.5:
            raise ValueError('mixup spread must be in [0, 0.5], got {!r}'.format(spread))
        return self._with(mixup=(float(prob), float(spread), int(seed)))

    def _photo_records(self, index, n):
        """The PHOTO_RECORD [n] of batch `index` (photometric() and / or mixup() on), drawn after the affine's records."""
        if self.photo_cfg is not None:
            prob, hue, saturation, value, gamma, seed, white = self.photo_cfg
            rec = augment.draw_photometric(seed, self.reader.shard_index, index, n, self.reader.image_size[2], prob, hue, saturation, value, gamma, white)
        else:
            rec = augment.photo_identity_records(n)
        if self.mixup_cfg is not None:
            prob, spread, seed = self.mixup_cfg
            rec = augment.draw_mixup(rec, seed, self.reader.shard_index, index, prob, spread)
        return rec

    def size_of_batch(self, i):
        """(h, w) of batch i of this dataset: the reader's stored size unless multiscale() is on."""
        if self.multiscale_cfg is None:
            return tuple(self.reader.image_size[:2])
        sizes, period, seed = self.multiscale_cfg
        return sizes[augment.multiscale_choice(seed, int(i) // period, len(sizes))]

    def _device_batch(self, dev, imgs, records, boxes, counts):
        """A label_device='gpu' batch on the device: imgs the raw pixels (already there), records host AUG_RECORD [B], boxes /
        counts host int32 (NumPy arrays or pinned tensors).  Augments to this batch's size, z-scores, builds the labels; with
        mosaic() on, the records of this batch are drawn here, the boxes remapped on the host and the augmented images recombined
        before the z-score; with affine() on, its records are drawn here too, the boxes go through affine_boxes after mosaic_boxes
        and the images through y3_affine_batch after the mosaic.  Without affine() no call is added.  With photometric() or
        mixup() on, their records are drawn after the affine's, mixup_boxes runs after affine_boxes, and y3_photometric_batch runs
        after the warp, right before the z-score (a fill region left by the warp goes through the colour transform like any other
        pixel).  With neither, no call and no allocation is added."""
        crop = tuple(self.reader.image_size[:2])
        index = self.batches
        size = self.size_of_batch(index)
        self.batches += 1
        if size != crop:
            records = augment.rescale_record(records, crop, size)
            b = boxes.numpy() if torch.is_tensor(boxes) else boxes
            boxes = augment.scale_boxes(b.reshape(-1, 5), crop, size).reshape(b.shape)      # (padding rows are never read)
        mosaic = None
        if self.mosaic_cfg is not None:
            prob, seed, min_visible = self.mosaic_cfg
            mosaic = augment.draw_mosaic(seed, self.reader.shard_index, index, len(records), size, prob)
            b, c = (x.numpy() if torch.is_tensor(x) else x for x in (boxes, counts))
            # an output image can hold the boxes of four inputs: collated afresh (never into the pinned prefetch buffer)
            boxes, counts = collate_boxes(augment.mosaic_boxes([b[i, :c[i]] for i in range(len(c))], mosaic, size, min_visible))
        affine = None
        if self.affine_cfg is not None:
            prob, degrees, shear, scale, translate, fill, seed, min_visible = self.affine_cfg
            affine, forward = augment.draw_affine(seed, self.reader.shard_index, index, len(records), size, prob, degrees, shear, scale, translate, fill)
            b, c = (x.numpy() if torch.is_tensor(x) else x for x in (boxes, counts))
            boxes, counts = collate_boxes(augment.affine_boxes([b[i, :c[i]] for i in range(len(c))], forward, size, min_visible))
        photo = None
        if self.photo_cfg is not None or self.mixup_cfg is not None:
            photo = self._photo_records(index, len(records))
            if self.mixup_cfg is not None:
                b, c = (x.numpy() if torch.is_tensor(x) else x for x in (boxes, counts))
                boxes, counts = collate_boxes(augment.mixup_boxes([b[i, :c[i]] for i in range(len(c))], photo))
        as_t =lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev, non_blocking=True)
        labels = format_labels_device(as_t(boxes), as_t(counts), (size[0], size[1], self.reader.image_size[2]), self.reader.anchors,
                                      self.reader.number_classes, **getattr(self.reader, '_label_kw', {}))
        imgs = augment_device(imgs, records, size)
        if mosaic is not None:
            imgs = mosaic_device(imgs, mosaic)
        if affine is not None:
            imgs = affine_device(imgs, affine)
        if photo is not None:
            imgs = photometric_device(imgs, photo)
        return (zscore_normalize_device(imgs), *labels)

    def _host_label_photometric(self, imgs):
        """photometric() on a label_device='cpu' reader (labels built in the workers; no mixup() there): the pass on the augmented
        batch, records keyed by this object's batch count as _device_batch keys them."""
        index = self.batches
        self.batches += 1
        return photometric_device(imgs, self._photo_records(index, imgs.shape[0]))

    def shard(self, num_shards, index):
        """experimental_distribute_dataset (train.py:62,66): every replica reads its own examples.  The reader's
        workers are forked at startup(), so the shard must be fixed before that (ImageReader(..., num_shards, shard_index));
        on a started reader this only checks that the request matches."""
        self.reader.set_shard(num_shards, index)
        return self

    def _examples(self):
        """Lists of batch_size examples off the worker queue; a short tail is dropped like tf.data drop_remainder."""
        gen = self.reader.raw_generator()
        while True:
            ex = []
            for e in gen:
                ex.append(e)
                if len(ex) == self.batch_size:
                    break
            if len(ex) < self.batch_size:
                return
            yield ex

    def __iter__(self):
        if self.batch_size is None:
            if self.mosaic_cfg is not None:
                raise ValueError('mosaic() combines the images of a batch: call batch(n) before iterating')
            if self.affine_cfg is not None:
                raise ValueError('affine() warps the images of a batch on the device: call batch(n) before iterating')
            if self.photo_cfg is not None:
                raise ValueError('photometric() changes the images of a batch on the device: call batch(n) before iterating')
            if self.mixup_cfg is not None:
                raise ValueError('mixup() blends the images of a batch: call batch(n) before iterating')
            yield from self.reader.generator()           # z-scored examples, as the reference's unbatched dataset yields them
            return
        dev = self.device or torch.device('cuda', torch.cuda.current_device())
        on_gpu = self.reader.augmentation_device == 'gpu'     # examples carry raw HWC pixels + an AUG_RECORD (ImageReader)
        lab_gpu = getattr(self.reader, 'label_device', 'cpu') == 'gpu'     # examples are (pixels, boxes, AUG_RECORD): labels built here
        crop = self.reader.image_size[:2]
        if not self.prefetch_depth:
            for ex in self._examples():
                imgs = torch.from_numpy(np.stack([e[0] for e in ex])).to(dev, non_blocking=True)
                if lab_gpu:
                    yield self._device_batch(dev, imgs, np.concatenate([e[2] for e in ex]), *collate_boxes([e[1] for e in ex]))
                    continue
                labels = [torch.from_numpy(np.stack([e[i] for e in ex])).to(dev, non_blocking=True) for i in (1, 2, 3)]
                if on_gpu:
                    imgs = augment_device(imgs, np.concatenate([e[4] for e in ex]), crop)
                    if self.photo_cfg is not None:
                        imgs = self._host_label_photometric(imgs)
                yield (zscore_normalize_device(imgs), *labels)
            return
        import queue
        import threading
        ready = queue.Queue(maxsize=self.prefetch_depth)
        ring = [dict(bufs=None, event=None) for _ in range(self.prefetch_depth + 2)]
        stop = threading.Event()

        def hand_over(item):
            while not stop.is_set():
                try:
                    ready.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def producer():
            try:
                for i, ex in enumerate(self._examples()):
                    if stop.is_set():
                        return
                    slot = ring[i % len(ring)]
                    if slot['event'] is not None:
                        slot['event'].synchronize()          # the upload that last used these pinned buffers has finished
                    if lab_gpu:
                        if slot['bufs'] is None:
                            slot['bufs'] = [torch.empty((len(ex),) + ex[0][0].shape, dtype=torch.from_numpy(ex[0][0]).dtype, pin_memory=True),
                                            None, torch.empty(len(ex), dtype=torch.int32, pin_memory=True)]
                        np.stack([e[0] for e in ex], out=slot['bufs'][0].numpy())
                        need = max([1] + [len(e[1]) for e in ex])
                        if slot['bufs'][1] is None or slot['bufs'][1].shape[1] < need:       # the box buffer grows: no fixed cap, nothing dropped
                            cap = 1 << (need - 1).bit_length()
                            slot['bufs'][1] = torch.empty((len(ex), cap, 5), dtype=torch.int32, pin_memory=True)
                        collate_boxes([e[1] for e in ex], out=(slot['bufs'][1].numpy(), slot['bufs'][2].numpy()))
                        slot['records'] = np.concatenate([e[2] for e in ex])
                        if not hand_over(slot):
                            return
                        continue
                    if slot['bufs'] is None:
                        slot['bufs'] = [torch.empty((len(ex),) + ex[0][j].shape, dtype=torch.from_numpy(ex[0][j]).dtype, pin_memory=True)
                                        for j in range(4)]
                    for j in range(4):
                        np.stack([e[j] for e in ex], out=slot['bufs'][j].numpy())
                    if on_gpu:
                        slot['records'] = np.concatenate([e[4] for e in ex])   # host side: read by the y3_augment_batch call
                    if not hand_over(slot):
                        return
            finally:
                hand_over(None)

        threading.Thread(target=producer, name='yolo3-prefetch', daemon=True).start()
        try:
            while True:
                slot = ready.get()
                if slot is None:
                    return
                if lab_gpu:
                    out = self._device_batch(dev, slot['bufs'][0].to(dev, non_blocking=True), slot['records'], slot['bufs'][1], slot['bufs'][2])
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(dev))      # behind the uploads from the pinned buffers
                    slot['event'] = ev
                    yield out
                    continue
                dev_t = [b.to(dev, non_blocking=True) for b in slot['bufs']]
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                slot['event'] = ev
                imgs = augment_device(dev_t[0], slot['records'], crop) if on_gpu else dev_t[0]
                if on_gpu and self.photo_cfg is not None:
                    imgs = self._host_label_photometric(imgs)
                yield (zscore_normalize_device(imgs), dev_t[1], dev_t[2], dev_t[3])
        finally:
            stop.set()          # the consumer walked away (epoch boundary): the producer exits at its next hand-over


class ImageReader:
    """imagereader.ImageReader (imagereader.py:79-460): same constructor, startup / shutdown / get_image_size /
    get_number_classes / get_image_count / get_example / generator; get_tf_dataset() returns a ``Dataset``."""

    def __init__(self, img_db, anchors, use_augmentation=True, balance_classes=False, shuffle=True, num_workers=1, num_shards=1, shard_index=0,
                 augmentation_device='cpu', label_device='cpu', anchor_scale=None):
        """num_shards / shard_index (addition): with one process per GPU every rank owns a reader; an unshuffled reader
        (the test set) then serves every num_shards-th stride of the key list, so the ranks evaluate disjoint images like
        the replicas of the reference's one distributed test batch.
        augmentation_device (addition): 'cpu' augments in the worker processes (augment.augment_image_box_pair, the
        reference's design); 'gpu' has the workers draw only the random decisions (augment.draw_augmentation) and hand out
        the stored pixels, which the batches then augment on the device (augment_device, csrc/augment.hip).
        label_device (addition): 'cpu' builds the three label tensors in the worker processes (format_boxes, the reference's
        design); 'gpu' (needs augmentation_device='gpu') has the workers hand out the transformed boxes, [k, 5] int32, and the
        batches build the labels on the device (format_labels_device): the same tensors, a few dozen boxes over PCIe instead.
        anchor_scale (addition): an owner table [A] (yolo3.anchors.default_anchor_scales / parse_anchor_masks); the
        label builder in use, host or device, then writes [G, G, A_s, 5+K] tensors.  None: the reference's labels."""
        assert augmentation_device in ('cpu', 'gpu'), augmentation_device
        if label_device not in ('cpu', 'gpu'):
            raise ValueError("label_device must be 'cpu' or 'gpu', got {!r}".format(label_device))
        if label_device == 'gpu' and augmentation_device != 'gpu':
            raise ValueError("label_device='gpu' needs augmentation_device='gpu': the workers then hand out boxes and records, not tensors")
        self.augmentation_device = augmentation_device
        self.label_device = label_device
        self.num_shards, self.shard_index = int(num_shards), int(shard_index)
        assert 0 <= self.shard_index < self.num_shards
        self.image_db = img_db
        self.use_augmentation = use_augmentation
        self.queue_starvation = False
        self.balance_classes = balance_classes
        self.anchors = anchors
        self.number_anchors = len(anchors)
        self.anchor_scale = None if anchor_scale is None else check_anchor_scales(anchor_scale, len(anchors))
        self._label_kw = {} if self.anchor_scale is None else {'anchor_scale': self.anchor_scale}
        if not os.path.exists(self.image_db):
            print('Could not load database file: ')
            print(self.image_db)
            raise Exception("Missing Database")
        self.shuffle = shuffle
        random.seed()
        self.keys_flat = []
        self.keys = [[]]
        env = lmdbio.Environment(self.image_db)
        all_keys = list(env.keys())
        empty_images_flag = False
        highest = 0
        for key in all_keys:                                      # key = "<n>_<name>:<c0,c1,...>" (build_lmdb.py:90-96)
            for k in key.decode('ascii').split(':')[1].split(','):
                if len(k) == 0:
                    empty_images_flag = True
                else:
                    highest = max(highest, int(k))
        for _ in range(highest):
            self.keys.append([])
        if empty_images_flag:
            self.keys.append([])
        for key in all_keys:
            self.keys_flat.append(key)
            for k in key.decode('ascii').split(':')[1].split(','):
                idx = 0 if len(k) == 0 else (int(k) + 1 if empty_images_flag else int(k))
                self.keys[idx].append(key)
        datum = ImageYoloBoxesPair().ParseFromString(env.get(self.keys_flat[0]))
        self.image_size = [datum.img_height, datum.img_width, datum.channels]
        self.image_dtype = np.dtype(datum.img_type) if datum.img_type else np.dtype(np.uint8)      # of the first record: Dataset.photometric's default white
        env.close()
        self.number_classes = len(self.keys) - 1 if empty_images_flag else len(self.keys)
        print('Found images of shape: {}'.format(self.image_size))
        print('Dataset has {} examples'.format(len(self.keys_flat)))
        self.nb_workers = num_workers
        self.maxOutQSize = num_workers * 10
        ctx = multiprocessing.get_context('fork')
        self._ctx = ctx
        self.terminateQ = ctx.Queue(maxsize=self.nb_workers)
        self.outQ = ctx.Queue(maxsize=self.maxOutQSize)
        self.workers = None
        self.done = False

    def get_image_size(self):
        return self.image_size

    def get_number_classes(self):
        return self.number_classes

    def get_image_count(self):
        return int(len(self.keys_flat))

    def set_shard(self, num_shards, index):
        if self.workers:
            if (int(num_shards), int(index)) != (self.num_shards, self.shard_index):
                raise RuntimeError('reader already started as shard {}/{}; pass num_shards / shard_index to ImageReader()'.format(
                    self.shard_index, self.num_shards))
            return
        assert 0 <= int(index) < int(num_shards)
        self.num_shards, self.shard_index = int(num_shards), int(index)

    def startup(self):
        self.done = False
        self.workers = [self._ctx.Process(target=_loader_process, args=(self, i), daemon=True) for i in range(self.nb_workers)]
        for w in self.workers:
            w.start()

    def shutdown(self):
        if not self.workers:
            return
        for _ in self.workers:
            self.terminateQ.put(None)
        got = 0
        while got < len(self.workers):                      # drain so blocked workers can finish (imagereader.py:203-222)
            try:
                while True:
                    if self.outQ.get(timeout=0.2) is None:
                        got += 1
            except queue.Empty:
                if not any(w.is_alive() for w in self.workers):
                    break
        for w in self.workers:
            w.join(5)
        self.workers = None

    def _next_key(self, state):
        if self.shuffle:
            if self.balance_classes:                            # imagereader.py:226-240
                while True:
                    label_idx = random.randint(0, len(self.keys) - 1)
                    if len(self.keys[label_idx]) > 0:
                        break
                return self.keys[label_idx][random.randint(0, len(self.keys[label_idx]) - 1)]
            return self.keys_flat[random.randint(0, len(self.keys_flat) - 1)]
        # no shuffle: stride the flat key list by worker id (Q17).  The reference indexes keys_flat[worker id] unguarded and
        # raises IndexError when a database has fewer images than reader processes; wrap instead.
        # With several shards (one reader per rank) worker w of shard s starts at s * nb_workers + w and strides by
        # num_shards * nb_workers: together the ranks walk the key list exactly like one reader with all the workers.
        state['idx'] %= len(self.keys_flat)
        fn = self.keys_flat[state['idx']]
        state['idx'] = (state['idx'] + self.nb_workers * self.num_shards) % len(self.keys_flat)
        return fn

    def load_example(self, key, env):
        """One example as the workers produce it: (image[C,H,W] float32 NOT yet z-scored, label_1, label_2, label_3); with
        augmentation_device='gpu': (image[H,W,C] as stored, label_1, label_2, label_3, AUG_RECORD [1]); with label_device='gpu'
        as well: (image[H,W,C] as stored, boxes [k,5] int32 -- what format_boxes would have been given -- , AUG_RECORD [1])."""
        datum = ImageYoloBoxesPair().ParseFromString(env.get(key))
        img, boxes = datum.to_arrays()
        if list(img.shape) != list(self.image_size):
            raise RuntimeError("Encountered unexpected image shape from database. Expected {}. Found {}.".format(self.image_size, img.shape))
        boxes = boxes.copy()
        crop_to = [self.image_size[0], self.image_size[1]]
        if self.augmentation_device == 'gpu':
            if self.use_augmentation:
                rec, boxes = augment.draw_augmentation(img.shape, boxes, crop_to=crop_to, **TRAIN_AUGMENTATION)
            else:
                rec = augment.identity_record(img.shape, crop_to)
            if self.label_device == 'gpu':
                boxes = np.zeros((0, 5), np.int32) if boxes is None else np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 5)
                return (np.ascontiguousarray(img), boxes, rec)
            labels = format_boxes(boxes, self.image_size, self.anchors, self.number_classes, **self._label_kw)
            return (np.ascontiguousarray(img), labels[0], labels[1], labels[2], rec)
        if self.use_augmentation:                               # severities of imagereader.py:369-391
            img, boxes = augment.augment_image_box_pair(img.astype(np.float32), boxes, crop_to=crop_to, **TRAIN_AUGMENTATION)
        if img.shape[0] != self.image_size[0] or img.shape[1] != self.image_size[1]:
            img, boxes = augment.crop_to_size(img, boxes, crop_to)
        img = np.ascontiguousarray(format_image(img)).astype(np.float32)
        labels = format_boxes(boxes, self.image_size, self.anchors, self.number_classes, **self._label_kw)
        return (img, labels[0], labels[1], labels[2])

    def _image_loader(self, worker_id):
        state = {'idx': self.shard_index * self.nb_workers + worker_id}
        try:
            random.seed()
            np.random.seed((os.getpid() * 2654435761) % (2 ** 32))
            env = lmdbio.Environment(self.image_db)
            while True:
                try:
                    if self.terminateQ.get_nowait() is None:
                        break
                except queue.Empty:
                    pass
                self.outQ.put(self.load_example(self._next_key(state), env))
        except Exception as e:                                  # imagereader.py:413-417
            print('***************** Reader Error *****************')
            print(e)
            traceback.print_exc()
            print('***************** Reader Error *****************')
        finally:
            self.outQ.put(None)

    def _get_raw(self):
        if self.outQ.qsize() < int(0.1 * self.maxOutQSize):     # imagereader.py:424-430
            if not self.queue_starvation:
                print('Input Queue Starvation !!!!')
            self.queue_starvation = True
        if self.queue_starvation and self.outQ.qsize() > int(0.5 * self.maxOutQSize):
            print('Input Queue Starvation Over')
            self.queue_starvation = False
        return self.outQ.get()

    def get_example(self):
        """imagereader.py:420-436: one (image, label_1, label_2, label_3) with the image z-scored (imagereader.py:398 does it
        in the worker; here the workers hand out raw pixels because the batched path z-scores whole batches on the GPU, so the
        single-example accessors normalise on the way out -- on the GPU as well, there is no host z-score in this package)."""
        example = self._get_raw()
        if example is None:
            return None
        if self.label_device == 'gpu':                         # a batch of one through the device path, labels included
            src = torch.from_numpy(example[0][None]).cuda()
            img = zscore_normalize_device(augment_device(src, example[2], self.image_size[:2]))[0].cpu().numpy()
            boxes, counts = collate_boxes([example[1]])
            labels = format_labels_device(torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda(), self.image_size, self.anchors,
                                          self.number_classes, **self._label_kw)
            return (img,) + tuple(l[0].cpu().numpy() for l in labels)
        if self.augmentation_device == 'gpu':                  # a batch of one through the device path
            src = torch.from_numpy(example[0][None]).cuda()
            img = zscore_normalize_device(augment_device(src, example[4], self.image_size[:2]))[0].cpu().numpy()
            return (img,) + tuple(example[1:4])
        return (zscore_normalize(example[0]),) + tuple(example[1:])

    def generator(self):
        while True:
            example = self.get_example()
            if example is None:
                return
            yield example

    def raw_generator(self):
        """Examples as the workers produce them (image NOT z-scored): what Dataset.batch() stacks and normalises on the GPU."""
        while True:
            example = self._get_raw()
            if example is None:
                return
            yield example

    def get_queue_size(self):
        return self.outQ.qsize()

    def get_tf_dataset(self):
        """imagereader.py:443-460 (a torch-side iterable instead of tf.data)."""
        return Dataset(self)

    get_dataset = get_tf_dataset
