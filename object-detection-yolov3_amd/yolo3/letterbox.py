"""Letterbox geometry: an image of any size -> the network frame with the aspect ratio kept, and the records
y3_letterbox_batch / y3_letterbox_zscore_nhwc / y3_letterbox_unmap take (include/yolo3hip.h).  Host arithmetic only: Python
integers and fp64."""
import math

import numpy as np

LETTERBOX_RECORD = np.dtype([('src_offset', '<u8'), ('src_h', '<i4'), ('src_w', '<i4'), ('new_h', '<i4'), ('new_w', '<i4'),
                             ('pad_y', '<i4'), ('pad_x', '<i4')])
assert LETTERBOX_RECORD.itemsize == 32
MAX_IMAGES = 16          # Y3_LETTERBOX_MAX_IMAGES: images per call
MAX_SIDE = 32768         # source and frame sides
MAX_SCALE = 64           # src / new on each axis
DTYPE_CODES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}      # as y3_tile_gather


def letterbox_record(h, w, H, W, src_offset=0):
    """One LETTERBOX_RECORD (shape (1,)) for a source of h x w in a frame of H x W: r = min(H / h, W / w), the content
    new = min(frame, max(1, floor(src * r + 0.5))) per axis, centred, the odd pixel of padding at the bottom / right.  Images
    smaller than the frame are enlarged."""
    h, w, H, W = int(h), int(w), int(H), int(W)
    if min(h, w, H, W) < 1:
        raise ValueError('letterbox_record: sizes must be >= 1 (got {} x {} into {} x {})'.format(h, w, H, W))
    r = min(H / h, W / w)
    new_h = min(H, max(1, int(math.floor(h * r + 0.5))))
    new_w = min(W, max(1, int(math.floor(w * r + 0.5))))
    rec = np.zeros(1, LETTERBOX_RECORD)
    rec['src_offset'], rec['src_h'], rec['src_w'] = int(src_offset), h, w
    rec['new_h'], rec['new_w'] = new_h, new_w
    rec['pad_y'], rec['pad_x'] = (H - new_h) // 2, (W - new_w) // 2
    return rec


def check_record(rec, index=0):
    """The limits of the kernels, as a ValueError that names the image (the library would refuse the call as well)."""
    for ax, s, n in (('height', int(rec['src_h']), int(rec['new_h'])), ('width', int(rec['src_w']), int(rec['new_w']))):
        if s > MAX_SIDE:
            raise ValueError('letterbox: image {}: {} {} above {}'.format(index, ax, s, MAX_SIDE))
        if s > MAX_SCALE * n:
            raise ValueError('letterbox: image {}: {} {} -> {} is a reduction by more than {} (too thin for this frame)'.format(
                index, ax, s, n, MAX_SCALE))


def pack_layout(shapes, itemsize, H, W):
    """(records [n], total bytes) for images of `shapes` (h, w, c) packed one after the other at 16-byte aligned offsets."""
    recs, off = [], 0
    for i, (h, w, c) in enumerate(shapes):
        rec = letterbox_record(h, w, H, W, off)
        check_record(rec[0], i)
        recs.append(rec)
        off += (int(h) * int(w) * int(c) * int(itemsize) + 15) & ~15
    return np.concatenate(recs), off
