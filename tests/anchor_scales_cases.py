"""Inputs shared by tests/test_cpu_anchor_scales.py and tests/test_gpu_anchor_scales.py (per-scale anchor assignment).
Host only: nothing here needs a device, and nothing here uses the feature's own code to build an expectation."""
import numpy as np

SIX = [(5, 6), (9, 9), (14, 20), (20, 12), (30, 30), (60, 50)]
NINE = [(3, 4), (5, 9), (9, 7), (9, 17), (17, 13), (16, 31), (30, 24), (40, 50), (80, 70)]      # Darknet's nine, about a quarter size

# name -> (anchors, owner table): the scale (0 = stride 32 .. 2 = stride 8) of every anchor.  Names count coarse / middle / fine.
PARTITIONS = {
    '1/1/1': ([(40, 36), (18, 14), (6, 7)], [0, 1, 2]),
    '2/1/1': ([(6, 7), (14, 18), (30, 26), (50, 44)], [2, 1, 0, 0]),
    '3/3/3': (NINE, [2, 2, 2, 1, 1, 1, 0, 0, 0]),
    '1/2/3': (SIX, [2, 2, 2, 1, 1, 0]),
    'shuffled': (SIX, [1, 2, 0, 2, 1, 2]),          # the widths of 1/2/3, slots that do not follow the index order of the sizes
}


def masks_of(table):
    """Owner table -> the anchors of scale 0, 1, 2, each in index order (the slot order)."""
    return [[a for a, s in enumerate(table) if s == t] for t in range(3)]


def random_boxes(rng, count, size, K, lo=2, hi=None):
    """[count, 5] int32 = x, y, w, h, class with the box inside a size x size image."""
    hi = int(size * 0.9) if hi is None else hi
    wh = rng.integers(lo, hi + 1, (count, 2))
    xy = np.stack([rng.integers(0, size - wh[:, 0] + 1), rng.integers(0, size - wh[:, 1] + 1)], 1) if count else np.zeros((0, 2), np.int64)
    return np.concatenate([xy, wh, rng.integers(0, K, (count, 1))], 1).astype(np.int32)


def box_batch(size, K, seed, per_image=(300, 0)):
    """Boxes of a batch, zero-padded to the longest list -> (boxes int32 [B, M, 5], counts int32 [B]).  The default is an image with
    300 boxes (two passes of the 256-box chunk, many cell collisions) and an image with none."""
    rng = np.random.default_rng(seed)
    m = max(max(per_image), 1)
    boxes = np.zeros((len(per_image), m, 5), np.int32)
    for i, k in enumerate(per_image):
        boxes[i, :k] = random_boxes(rng, k, size, K)
    return boxes, np.array(per_image, np.int32)


def collision_same_anchor(anchors):
    """Two boxes of SIX's anchor 2, centres (16, 19) and (17, 20): one stride-8 cell, one anchor, other coordinates and classes."""
    assert anchors == SIX
    return np.array([[10, 10, 14, 20, 0], [11, 10, 14, 21, 1]], np.int32)


def collision_other_scale(anchors, table):
    """Two boxes centred at (16, 19), one of anchor 2 and one of anchor 4, which another scale owns: the same cell of every grid,
    and in scale mode each on its own scale."""
    assert anchors == SIX and table[2] != table[4]
    return np.array([[10, 10, 14, 20, 0], [2, 5, 30, 30, 1]], np.int32)


def label_batch(size, K, anchors, table, seed, per_image):
    """Three scale-mode label tensors [B, G, G, A_s, 5+K] of random boxes (imagereader.format_boxes)."""
    from yolo3.imagereader import format_boxes
    rng = np.random.default_rng(seed)
    per = [format_boxes(random_boxes(rng, int(k), size, K, lo=4, hi=50), (size, size, 3), anchors, K, anchor_scale=table) for k in per_image]
    return [np.stack([p[s] for p in per]) for s in range(3)]


def default_call_lists(YoloV3, imagereader, calls):
    """What a model and a label build WITHOUT the feature's arguments launch: the entry-point names `calls` collects (the caller
    wraps every symbol of the library before this runs), keyed by phase.  Uses nothing the parent commit lacks."""
    import torch
    out = {}
    anchors, K, img, n = [(64, 384), (384, 64)], 2, 64, 2
    images = torch.randn(n, 3, img, img, generator=torch.Generator().manual_seed(1)).cuda()
    boxes = np.array([[[5, 8, 40, 30, 1], [20, 10, 30, 50, 0]]] * n, np.int32)
    labs = [imagereader.format_boxes(boxes[i].copy(), (img, img, 3), anchors, K) for i in range(n)]
    gts = [torch.from_numpy(np.stack([l[s] for l in labs])).cuda() for s in range(3)]
    del calls[:]
    yolo = YoloV3(n, [img, img, 3], K, anchors, learning_rate=1e-4, seed=3)
    out['construct'] = list(calls)
    for phase, run in (('train_step', lambda: yolo.train_step((images, gts))), ('train_step_2', lambda: yolo.train_step((images, gts))),
                       ('test_step', lambda: yolo.test_step((images, gts))), ('predict', lambda: yolo.predict(images)),
                       ('labels', lambda: imagereader.format_labels_device(torch.from_numpy(boxes).cuda(), torch.full((n,), 2, dtype=torch.int32).cuda(),
                                                                           (img, img, 3), anchors, K))):
        del calls[:]
        run()
        torch.cuda.synchronize()
        out[phase] = list(calls)
    truth = YoloV3(n, [img, img, 3], K, anchors, learning_rate=1e-4, seed=3, ignore_mask='truth')
    del calls[:]
    truth.train_step((images, gts))
    torch.cuda.synchronize()
    out['train_step_truth'] = list(calls)
    return out
