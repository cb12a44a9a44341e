"""Host-side augmentation of (image, boxes) pairs, mirroring the reference's augment.py
(augment_image_box_pair :30-125, augment_boxes :128-189, apply_affine_transformation_boxes :192-272,
apply_affine_transformation :275-297, crop_to_size :20-27).

CPU pre-processing in the reader processes, as in the reference; it is stochastic (draws from the global np.random in
the reference's order) and outside the measured path.  scikit-image is not available in this image, so
the rescale of augment.py:277-280 is restated on scipy.ndimage.map_coordinates (rescale_bilinear).  Pinned by
tests/golden/augment.npz, produced by running the reference's augment.py under seeded np.random: boxes and crop
offsets identical, pixels to 1e-4 of the 8-bit range.  Boxes are [n,5] = x, y, w, h, class (top-left corner).

draw_augmentation is the device path's half of augment_image_box_pair: the same random decisions, boxes transformed here,
the pixels left to y3_augment_batch (csrc/augment.hip) through one AUG_RECORD per image.

Not in the reference, device path only: draw_mosaic / mosaic_boxes / mosaic_reference, draw_affine / affine_boxes /
affine_reference (the rotation the reference's rotation_flag names and asserts away, with shear, gain and translation)
and colour_matrix / draw_photometric / draw_mixup / mixup_boxes / photometric_reference (colour matrix, clamp, tone
curve and MixUp, one elementwise pass).
"""
import numpy as np
import scipy.ndimage

MIN_VISIBLE = 12      # boxes with less than 12 px inside the crop are dropped (augment.py:228-237)

# y3_aug_record (include/yolo3hip.h), one per image of a y3_augment_batch call
AUG_RECORD = np.dtype([('src_h', '<i4'), ('src_w', '<i4'), ('rows', '<i4'), ('cols', '<i4'), ('dy', '<i4'), ('dx', '<i4'),
                       ('reflect_x', '<i4'), ('reflect_y', '<i4'), ('noise_severity', '<f4'), ('u_noise', '<f4'),
                       ('blur_sigma', '<f4'), ('reserved', '<i4'), ('seed', '<u8')])
assert AUG_RECORD.itemsize == 56


def jitter_boxes(boxes, location_jitter, size_jitter, img_shape):
    """augment.py:128-189.  Returns None for an empty input (Q14)."""
    if boxes is None or boxes.shape[0] == 0:
        return None
    b = boxes.astype(np.int64).copy()
    x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    for i in range(len(x)):
        x[i] += int(location_jitter * w[i] * np.random.randn())
        y[i] += int(location_jitter * h[i] * np.random.randn())
    for i in range(len(x)):
        d = int(size_jitter * w[i] * np.random.randn())
        x[i] -= int(d / 2)
        w[i] += d
        d = int(size_jitter * h[i] * np.random.randn())
        y[i] -= int(d / 2)
        h[i] += d
    x1 = np.minimum(x + w - 1, img_shape[1] - 1)
    y1 = np.minimum(y + h - 1, img_shape[0] - 1)
    x0, y0 = np.maximum(x, 0), np.maximum(y, 0)
    ww, hh = x1 - x0 + 1, y1 - y0 + 1
    assert np.all(hh > 0) and np.all(ww > 0), 'box with zero or negative size'      # augment.py:180, same failure mode
    return np.stack([x0, y0, ww, hh, b[:, 4]], 1).astype(np.int32)


def transform_boxes(boxes, crop_size, reflect_x, reflect_y, scale_x, scale_y, dx, dy):
    """augment.py:192-272: scale, shift by the crop origin, drop boxes that left the crop, clamp, reflect."""
    if boxes is None or boxes.shape[0] == 0:
        return None
    cls = boxes[:, 4]
    x0 = boxes[:, 0] * scale_x - dx
    x1 = (boxes[:, 0] + boxes[:, 2] - 1) * scale_x - dx
    y0 = boxes[:, 1] * scale_y - dy
    y1 = (boxes[:, 1] + boxes[:, 3] - 1) * scale_y - dy
    h, w = crop_size[0], crop_size[1]
    keep = ~((x0 >= w) | (y0 >= h) | (x1 < 0) | (y1 < 0))
    keep &= ~((x0 >= w - MIN_VISIBLE) | (y0 >= h - MIN_VISIBLE) | (x1 < MIN_VISIBLE) | (y1 < MIN_VISIBLE))
    if not keep.any():
        return None
    x0, y0, x1, y1, cls = x0[keep], y0[keep], x1[keep], y1[keep], cls[keep]
    x0, y0 = np.maximum(x0, 0), np.maximum(y0, 0)
    x1, y1 = np.minimum(x1, w - 1), np.minimum(y1, h - 1)
    if reflect_x:
        x0, x1 = w - x1, w - x0
    if reflect_y:
        y0, y1 = h - y1, h - y0
    return np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1, cls], 1).astype(np.int32)


def rescale_bilinear(img, scale_y, scale_x):
    """skimage.transform.rescale(img, [scale_y, scale_x(, 1)], mode='reflect', preserve_range=True) as used at
    augment.py:277-280 (scikit-image is not in this image): output shape round(shape * scale); output pixel centres map to
    input coordinates (r + 0.5) * in_rows / out_rows - 0.5 (likewise for columns); bilinear; out-of-range samples reflect
    without repeating the edge (numpy.pad 'reflect' = scipy 'mirror').  Returns float64 like skimage does."""
    img = np.asarray(img, dtype=np.float64)
    rows = int(np.round(scale_y * img.shape[0]))
    cols = int(np.round(scale_x * img.shape[1]))
    r = (np.arange(rows) + 0.5) * (img.shape[0] / rows) - 0.5
    c = (np.arange(cols) + 0.5) * (img.shape[1] / cols) - 0.5
    grid = np.meshgrid(r, c, indexing='ij')
    if img.ndim == 2:
        return scipy.ndimage.map_coordinates(img, grid, order=1, mode='mirror')
    return np.stack([scipy.ndimage.map_coordinates(img[:, :, ch], grid, order=1, mode='mirror') for ch in range(img.shape[2])], axis=2)


def transform_image(img, reflect_x, reflect_y, scale_x, scale_y, crop_to):
    """augment.py:275-297: rescale, random crop to crop_to, flips.  Returns (img float64, dx, dy)."""
    if scale_x != 1 or scale_y != 1:
        img = rescale_bilinear(img, scale_y, scale_x)
    else:
        img = np.asarray(img, dtype=np.float64)      # skimage's identity rescale also returns float64 (values unchanged to 1e-12)
    dy = dx = 0
    if img.shape[0] - crop_to[0] > 0:
        dy = int(np.random.randint(0, img.shape[0] - crop_to[0]))
    if img.shape[1] - crop_to[1] > 0:
        dx = int(np.random.randint(0, img.shape[1] - crop_to[1]))
    img = img[dy:dy + crop_to[0], dx:dx + crop_to[1]]
    if reflect_x:
        img = np.fliplr(img)
    if reflect_y:
        img = np.flipud(img)
    return img, dx, dy


def crop_to_size(img, boxes, crop_to):
    """augment.py:20-27."""
    img, dx, dy = transform_image(img, False, False, 1.0, 1.0, crop_to)
    return img, transform_boxes(boxes, crop_to, False, False, 1.0, 1.0, dx, dy)


def augment_image_box_pair(img, boxes, rotation_flag=False, reflection_flag=False, crop_to=None, noise_augmentation_severity=0,
                           scale_augmentation_severity=0, blur_augmentation_max_sigma=0, box_size_augmentation_severity=0,
                           box_location_jitter_severity=0):
    """augment.py:30-125 (same parameter names and ranges)."""
    assert not rotation_flag, 'Rotation not implemented for image and boxes pair'
    img = np.asarray(img, dtype=np.float32)
    assert img.ndim in (2, 3)
    noise = noise_augmentation_severity or 0
    scale = scale_augmentation_severity or 0
    blur = blur_augmentation_max_sigma or 0
    assert 0 <= noise < 1 and 0 <= scale < 1 and 0 <= (box_size_augmentation_severity or 0) < 1 and 0 <= (box_location_jitter_severity or 0) < 1
    if crop_to is None:
        crop_to = img.shape[:2]
    reflect_x = reflect_y = False
    scale_x = scale_y = 1
    if reflection_flag:
        reflect_x = np.random.rand() > 0.5
        reflect_y = np.random.rand() > 0.5
    if scale > 0:
        hi = 1.0 + scale
        lo = max(max(crop_to[0] / img.shape[0], crop_to[1] / img.shape[1]), 1.0 - scale)
        scale_x = lo + (hi - lo) * np.random.rand()
        scale_y = lo + (hi - lo) * np.random.rand()
    boxes = jitter_boxes(boxes, box_location_jitter_severity or 0, box_size_augmentation_severity or 0, img.shape)
    img, dx, dy = transform_image(img, reflect_x, reflect_y, scale_x, scale_y, crop_to)
    boxes = transform_boxes(boxes, crop_to, reflect_x, reflect_y, scale_x, scale_y, dx, dy)
    if noise > 0:
        smax = noise * (np.max(img) - np.min(img))
        sigma = -smax + 2 * smax * np.random.rand()
        img = img + np.random.standard_normal(img.shape) * sigma
    if blur > 0:
        sigma = -blur + 2 * blur * np.random.rand()
        if sigma > 0:
            img = scipy.ndimage.gaussian_filter(img, sigma, mode='reflect')
    return np.asarray(img, dtype=np.float32), boxes


def identity_record(img_shape, crop_to=None):
    """The record of crop_to_size (augment.py:20-27): scale 1, no flips, no noise, no blur.  Draws the crop offsets from
    np.random exactly as crop_to_size does (none when the image already has the crop's size)."""
    rec, _ = draw_augmentation(img_shape, None, crop_to=crop_to)
    return rec


def draw_augmentation(img_shape, boxes, rotation_flag=False, reflection_flag=False, crop_to=None, noise_augmentation_severity=0,
                      scale_augmentation_severity=0, blur_augmentation_max_sigma=0, box_size_augmentation_severity=0,
                      box_location_jitter_severity=0):
    """The random decisions of augment_image_box_pair (same keyword arguments) without touching pixels -> (record, boxes).

    Draws from the global np.random in augment_image_box_pair's order: reflect_x, reflect_y, scale_x, scale_y, the box
    jitter normals, dy, dx, the noise uniform; everything up to there -- boxes, flips, rescaled size, crop offsets -- is
    what augment_image_box_pair gives under the same seed.  Then, where the host path spends H*W*C normals on the noise
    (which the device draws from its own counter-based stream keyed by `seed`), this draws the blur uniform and the 64-bit
    noise seed: the blur sigma has the host path's distribution but not its seed-for-seed value.  record: AUG_RECORD
    array of shape [1]; boxes: transformed on the host (None when none survive), as augment_image_box_pair returns them."""
    assert not rotation_flag, 'Rotation not implemented for image and boxes pair'
    assert len(img_shape) in (2, 3)
    noise = noise_augmentation_severity or 0
    scale = scale_augmentation_severity or 0
    blur = blur_augmentation_max_sigma or 0
    assert 0 <= noise < 1 and 0 <= scale < 1 and 0 <= (box_size_augmentation_severity or 0) < 1 and 0 <= (box_location_jitter_severity or 0) < 1
    H, W = int(img_shape[0]), int(img_shape[1])
    if crop_to is None:
        crop_to = (H, W)
    reflect_x = reflect_y = False
    scale_x = scale_y = 1
    if reflection_flag:
        reflect_x = np.random.rand() > 0.5
        reflect_y = np.random.rand() > 0.5
    if scale > 0:
        hi = 1.0 + scale
        lo = max(max(crop_to[0] / H, crop_to[1] / W), 1.0 - scale)
        scale_x = lo + (hi - lo) * np.random.rand()
        scale_y = lo + (hi - lo) * np.random.rand()
    boxes = jitter_boxes(boxes, box_location_jitter_severity or 0, box_size_augmentation_severity or 0, img_shape)
    rows, cols = H, W
    if scale_x != 1 or scale_y != 1:                     # rescale_bilinear's output size
        rows, cols = int(np.round(scale_y * H)), int(np.round(scale_x * W))
    dy = dx = 0                                          # transform_image's crop offsets
    if rows - crop_to[0] > 0:
        dy = int(np.random.randint(0, rows - crop_to[0]))
    if cols - crop_to[1] > 0:
        dx = int(np.random.randint(0, cols - crop_to[1]))
    boxes = transform_boxes(boxes, crop_to, reflect_x, reflect_y, scale_x, scale_y, dx, dy)
    u_noise = np.random.rand() if noise > 0 else 0.0
    sigma = (-blur + 2 * blur * np.random.rand()) if blur > 0 else 0.0
    seed = np.random.randint(0, 2**64, dtype=np.uint64) if noise > 0 else 0
    rec = np.zeros(1, AUG_RECORD)
    rec[0] = (H, W, rows, cols, dy, dx, int(reflect_x), int(reflect_y), noise, u_noise, sigma, 0, seed)
    return rec, boxes


# ---- multi-scale training: the same augmented crop, resampled to another network input size ----------------
def rescale_record(rec, crop_from, size):
    """The record that makes y3_augment_batch(..., h_out=size[0], w_out=size[1]) produce the crop `rec` describes at
    crop_from = (h, w), resampled to `size`: rows, cols, dy, dx scaled by size / crop_from and rounded to nearest (half up, in
    exact integer arithmetic), rows' / cols' at least the new crop, dy' / dx' clamped so that the crop fits (dy' + size[0] <=
    rows').  Flips, noise and the blur sigma are unchanged: sigma stays in OUTPUT pixels, so the kernel's radius limit holds.
    rec: AUG_RECORD array of any shape; returns a new array, equal to rec when size == crop_from."""
    out = np.array(rec, dtype=AUG_RECORD, copy=True)
    for full, off, c, s in (('rows', 'dy', int(crop_from[0]), int(size[0])), ('cols', 'dx', int(crop_from[1]), int(size[1]))):
        if s == c:
            continue
        n = np.maximum((2 * out[full].astype(np.int64) * s + c) // (2 * c), s)
        o = np.minimum((2 * out[off].astype(np.int64) * s + c) // (2 * c), n - s)
        out[full], out[off] = n, o
    return out


def scale_boxes(boxes, crop_from, size):
    """The box side of rescale_record: [n,5] integer boxes (x, y, w, h, class; top-left corner) of a crop_from = (h, w) image
    mapped into a `size` image.  Corner based and rounded OUTWARDS in exact integer arithmetic: the left / top edge x becomes
    floor(x * s / c), the exclusive right / bottom edge x + w becomes ceil((x + w) * s / c); then the near edge is clamped to
    [0, s - 1] and the far edge to [near + 1, s], so every box stays inside the new image with w, h >= 1, and a box covering the
    whole crop covers the whole target.  An axis whose size does not change is returned as it came (the identity at equal
    sizes, whatever the boxes).  None / empty input comes back unchanged."""
    if boxes is None or boxes.shape[0] == 0:
        return boxes
    out = np.array(boxes, copy=True)
    b = out.astype(np.int64)
    for lo, ext, c, s in ((0, 2, int(crop_from[1]), int(size[1])), (1, 3, int(crop_from[0]), int(size[0]))):
        if s == c:
            continue
        near = np.clip((b[:, lo] * s) // c, 0, s - 1)
        far = np.clip(-((-(b[:, lo] + b[:, ext]) * s) // c), near + 1, s)
        out[:, lo], out[:, ext] = near, far - near
    return out


def multiscale_choice(seed, block, count):
    """Index in 0 .. count-1 of the size multi-scale training uses for the block-th run of `period` batches: a pure function of
    (seed, block) -- splitmix64 of seed * 2^32 + block, reduced modulo count -- so every rank draws the same size and a run can
    be repeated."""
    m = (1 << 64) - 1
    z = ((int(seed) << 32) + int(block) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return int(z % int(count))


# ---- mosaic (not in the reference): every output image put together from four images of its own batch -------
# y3_mosaic_record (include/yolo3hip.h), one per OUTPUT image of a y3_mosaic_batch call
MOSAIC_RECORD = np.dtype([('cy', '<i4'), ('cx', '<i4'), ('src', '<i4', (4,)), ('oy', '<i4', (4,)), ('ox', '<i4', (4,)), ('reserved', '<i4', (2,))])
assert MOSAIC_RECORD.itemsize == 64

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix64(z):
    """splitmix64's output function (the one multiscale_choice uses)."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _quadrants(cy, cx, h, w):
    """(qy, qx, qh, qw) of quadrants 0..3 around the seam (cy, cx) of an h x w image."""
    return ((0, 0, cy, cx), (0, cx, cy, w - cx), (cy, 0, h - cy, cx), (cy, cx, h - cy, w - cx))


def draw_mosaic(seed, shard, batch_index, n, size, prob):
    """MOSAIC_RECORD [n] for the batch_index-th batch of n images of size = (h, w) on reader shard `shard`: a pure function of its
    arguments (no global np.random: the prefetch thread and a rerun draw the same batch; another shard, batch or seed another).

    Draws are counter based.  Output image i owns the stream key_i = the splitmix64 output function folded over (seed, shard,
    batch_index, i) -- k = 0; for v in those four: k = mix((k ^ v) + 0x9E3779B97F4A7C15) -- and its j-th draw is the 64-bit word
    u_j = mix(key_i + (j + 1) * 0x9E3779B97F4A7C15), i.e. splitmix64 seeded with key_i.  A uniform integer in [lo, hi] is
    lo + u % (hi - lo + 1) (the modulo bias is below 2^-50 for any image size).  Exact draw order per image:
      u_0        the image is a mosaic when (u_0 >> 11) * 2^-53 < prob; otherwise the identity record (cy = h, cx = w, src[0] = i,
                 windows at 0) is emitted and the remaining words are not used
      u_1, u_2   cy in [h//4, h - h//4], cx in [w//4, w - w//4]
      u_3..u_5   src[1], src[2], src[3] (src[0] = i).  n >= 4: without replacement from the other n - 1 images in ascending
                 order -- u_j % (number left) indexes the list of images not yet taken --, so the four are distinct.  n = 2, 3:
                 each from the other n - 1 images, repetition allowed.  n = 1: image 0
      u_6..u_13  oy[0], ox[0], oy[1], ox[1], ..., oy[3], ox[3]: oy[q] in [0, h - qh], ox[q] in [0, w - qw], the positions where
                 the quadrant's qh x qw window fits into its source."""
    h, w = int(size[0]), int(size[1])
    n = int(n)
    if n < 1 or h < 1 or w < 1:
        raise ValueError('draw_mosaic: n, h, w must be >= 1, got {} {} {}'.format(n, h, w))
    rec = np.zeros(n, MOSAIC_RECORD)
    for i in range(n):
        key = 0
        for v in (seed, shard, batch_index, i):
            key = _mix64((key ^ (int(v) & _M64)) + _GOLDEN)
        u = lambda j: _mix64(key + (j + 1) * _GOLDEN)
        r = rec[i]
        if not (u(0) >> 11) * 2.0 ** -53 < prob:
            r['cy'], r['cx'], r['src'][0] = h, w, i
            continue
        cy = h // 4 + u(1) % (h - 2 * (h // 4) + 1)
        cx = w // 4 + u(2) % (w - 2 * (w // 4) + 1)
        r['cy'], r['cx'], r['src'][0] = cy, cx, i
        others = [k for k in range(n) if k != i]
        for q in (1, 2, 3):
            if n >= 4:
                r['src'][q] = others.pop(u(2 + q) % len(others))
            elif n >= 2:
                r['src'][q] = others[u(2 + q) % len(others)]
        for q, (_, _, qh, qw) in enumerate(_quadrants(cy, cx, h, w)):
            r['oy'][q] = u(6 + 2 * q) % (h - qh + 1)
            r['ox'][q] = u(7 + 2 * q) % (w - qw + 1)
    return rec


def _is_identity(r, i, h, w):
    return r['cy'] == h and r['cx'] == w and r['src'][0] == i and r['oy'][0] == 0 and r['ox'][0] == 0


def mosaic_boxes(box_lists, records, size, min_visible=0.25):
    """The boxes of the output images of y3_mosaic_batch(records) from the boxes of its input images.  box_lists: one int32 [k, 5]
    array per input image (x, y, w, h, class; top-left corner; the box covers [x, x+w) x [y, y+h)), None or empty = no boxes.
    Returns one int32 [k', 5] array per output image ([0, 5] when empty).

    Per output image, quadrants 0..3 in order and within a quadrant the boxes of its source in their order: the box is
    intersected with the source window [ox, ox+qw) x [oy, oy+qh); dropped when the clipped w' < 1 or h' < 1; dropped when
    w' * h' < min_visible * (w * h) (exact integer products, compared in float64: a visible fraction of exactly min_visible
    stays); otherwise shifted by (qx - ox, qy - oy).  The class is unchanged.  An image with the identity record keeps its
    boxes exactly as they came, order included (no clipping is applied to it).  min_visible = 0.25 is a default, not a tuned
    value."""
    h, w = int(size[0]), int(size[1])
    empty = np.zeros((0, 5), np.int32)
    src = [empty if b is None or len(b) == 0 else np.asarray(b, np.int32).reshape(-1, 5) for b in box_lists]
    assert len(records) == len(src), (len(records), len(src))
    out = []
    for i, r in enumerate(records):
        if _is_identity(r, i, h, w):
            out.append(src[i].copy())
            continue
        kept = []
        for q, (qy, qx, qh, qw) in enumerate(_quadrants(int(r['cy']), int(r['cx']), h, w)):
            if qh == 0 or qw == 0:
                continue
            oy, ox = int(r['oy'][q]), int(r['ox'][q])
            for bx, by, bw, bh, cls in src[int(r['src'][q])].tolist():
                x0, y0 = max(bx, ox), max(by, oy)
                x1, y1 = min(bx + bw, ox + qw), min(by + bh, oy + qh)
                if x1 - x0 < 1 or y1 - y0 < 1:
                    continue
                if float((x1 - x0) * (y1 - y0)) < np.float64(min_visible) * float(bw * bh):
                    continue
                kept.append((x0 + qx - ox, y0 + qy - oy, x1 - x0, y1 - y0, cls))
        out.append(np.array(kept, np.int32).reshape(-1, 5))
    return out


def mosaic_reference(batch, records):
    """y3_mosaic_batch restated in NumPy slices (the oracle of the GPU tests): batch [n, c, h, w] of any dtype -> a new array."""
    batch = np.asarray(batch)
    n, _, h, w = batch.shape
    assert len(records) == n
    out = np.empty_like(batch)
    for i, r in enumerate(records):
        for q, (qy, qx, qh, qw) in enumerate(_quadrants(int(r['cy']), int(r['cx']), h, w)):
            if qh == 0 or qw == 0:
                continue
            oy, ox = int(r['oy'][q]), int(r['ox'][q])
            out[i, :, qy:qy + qh, qx:qx + qw] = batch[int(r['src'][q]), :, oy:oy + qh, ox:ox + qw]
    return out


# ---- random affine warp (not in the reference): rotation, shear, isotropic gain and translation ---------------
# y3_affine_record (include/yolo3hip.h), one per image of a y3_affine_batch call
AFFINE_RECORD = np.dtype([('m', '<f4', (6,)), ('fill', '<f4'), ('reserved', '<i4')])
assert AFFINE_RECORD.itemsize == 32
AFFINE_MAX_COORD = 2.0 ** 30      # y3_affine_batch refuses |m0| (w-1) + |m1| (h-1) + |m2| (and the y row alike) above this
_AFFINE_STREAM = 0xAFF1E          # folded into the key after (seed, shard, batch, image): not the mosaic's stream of the same seed


def affine_identity_records(n, fill=0.0):
    """n records of the identity map (an exact copy of the image)."""
    rec = np.zeros(int(n), AFFINE_RECORD)
    rec['m'] = (1, 0, 0, 0, 1, 0)
    rec['fill'] = fill
    return rec


def affine_record(forward, fill=0.0):
    """One AFFINE_RECORD from a FORWARD 3 x 3 matrix (source pixel -> output pixel, last row 0 0 1): inverted in float64, the six
    coefficients rounded once to float32."""
    inv = np.linalg.inv(np.asarray(forward, np.float64))
    rec = np.zeros(1, AFFINE_RECORD)
    rec['m'][0] = inv[:2].reshape(6).astype(np.float32)
    rec['fill'] = fill
    return rec


def draw_affine_parameters(seed, shard, batch_index, image, prob, degrees=0.0, shear=0.0, scale=0.0, translate=0.0):
    """The draw of one image (draw_affine's docstring has the stream and the order): None when the image is not warped, else
    (rotation degrees, x shear degrees, y shear degrees, gain, x translation, y translation as shares of the side)."""
    key = 0
    for v in (seed, shard, batch_index, image, _AFFINE_STREAM):
        key = _mix64((key ^ (int(v) & _M64)) + _GOLDEN)
    u = lambda j: (_mix64(key + (j + 1) * _GOLDEN) >> 11) * 2.0 ** -53
    if not u(0) < prob:
        return None
    between = lambda j, mag: -float(mag) + 2.0 * float(mag) * u(j)
    return (between(1, degrees), between(2, shear), between(3, shear), 1.0 + between(4, scale), between(5, translate), between(6, translate))


def draw_affine(seed, shard, batch_index, n, size, prob, degrees=0.0, shear=0.0, scale=0.0, translate=0.0, fill=0.0):
    """(AFFINE_RECORD [n], forward matrices float64 [n, 3, 3]) for the batch_index-th batch of n images of size = (h, w) on reader
    shard `shard`: a pure function of its arguments, counter based exactly as draw_mosaic is (no global np.random).  Image i owns
    the key folded over (seed, shard, batch_index, i, 0xAFF1E) -- k = 0; for v in those five: k = mix((k ^ v) + 0x9E3779B97F4A7C15)
    -- so its draw does not depend on n; its j-th word is u_j = mix(key + (j + 1) * 0x9E3779B97F4A7C15), the uniform U_j =
    (u_j >> 11) * 2^-53 in [0, 1), and a value in [lo, hi] is lo + (hi - lo) * U_j.  Draw order per image:
      U_0       the image is warped when U_0 < prob; otherwise it gets the identity record and matrix, the other words unused
      U_1       rotation angle a in [-degrees, degrees]: Rot = [[cos a, -sin a], [sin a, cos a]] on (x, y), x to the right, y down
      U_2, U_3  x and y shear angles in [-shear, shear] degrees: Shear = [[1, tan sx], [tan sy, 1]]
      U_4       gain in [1 - scale, 1 + scale]
      U_5, U_6  translation in [-translate, translate] * w along x, * h along y
    forward = T . Shear . (gain Rot) . C in float64, C moving the image centre ((w-1)/2, (h-1)/2) to the origin and T moving it back
    plus the drawn translation; the record holds its float64 inverse rounded once to float32.  A draw with every magnitude zero is
    the identity record exactly."""
    h, w = int(size[0]), int(size[1])
    n = int(n)
    if n < 1 or h < 1 or w < 1:
        raise ValueError('draw_affine: n, h, w must be >= 1, got {} {} {}'.format(n, h, w))
    rec = affine_identity_records(n, fill)
    mats = np.tile(np.eye(3), (n, 1, 1))
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    for i in range(n):
        par = draw_affine_parameters(seed, shard, batch_index, i, prob, degrees, shear, scale, translate)
        if par is None or par == (0.0, 0.0, 0.0, 1.0, 0.0, 0.0):
            continue
        rot, shx, shy = np.deg2rad(par[0]), np.deg2rad(par[1]), np.deg2rad(par[2])
        gain, tx, ty = par[3], par[4] * w, par[5] * h
        c = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1]], np.float64)
        r = np.array([[gain * np.cos(rot), -gain * np.sin(rot), 0], [gain * np.sin(rot), gain * np.cos(rot), 0], [0, 0, 1]], np.float64)
        s = np.array([[1, np.tan(shx), 0], [np.tan(shy), 1, 0], [0, 0, 1]], np.float64)
        t = np.array([[1, 0, cx + tx], [0, 1, cy + ty], [0, 0, 1]], np.float64)
        mats[i] = t @ s @ r @ c
        rec[i] = affine_record(mats[i], fill)[0]
    return rec, mats


def affine_boxes(box_lists, matrices, size, min_visible=0.25):
    """The boxes of the output images of y3_affine_batch from the boxes of its input images and the FORWARD matrices (float64
    [n, 3, 3], source pixel -> output pixel; draw_affine's second result).  box_lists: one int32 [k, 5] array per image (x, y, w, h,
    class; top-left corner; the box covers the pixel centres x .. x+w-1, y .. y+h-1), None or empty = no boxes.  Returns one int32
    [k', 5] array per image ([0, 5] when empty), order kept.

    Per box: its four pixel-centre corners (x, y), (x+w-1, y), (x, y+h-1), (x+w-1, y+h-1) go through the matrix in float64; the
    axis-aligned bounds of the four are rounded to the nearest pixel centre, halves up (floor(v + 0.5)), which gives the
    unclipped box x0..x1, y0..y1 (inclusive) of area (x1-x0+1)(y1-y0+1); it is clipped to [0, w-1] x [0, h-1]; dropped when a
    clipped side is below 2 px; dropped when the clipped area < min_visible * the unclipped area (exact integer products compared
    in float64: a share of exactly min_visible stays).  The class is unchanged.  An image whose matrix is exactly the identity
    keeps its boxes as they came (no clipping, no 2 px rule).  Integer matrices (flips, quarter turns, integer shifts) move the
    corners exactly, so the boxes are the permuted boxes of the permuted pixels: a flip sends x to w-1-x -- one pixel left of
    transform_boxes' reflection, which is the reference's w - x.  Under a rotation the bounds are those of the rotated rectangle,
    so they grow; the min_visible share is taken of that grown box.  min_visible = 0.25 is a default, not a tuned value."""
    h, w = int(size[0]), int(size[1])
    empty = np.zeros((0, 5), np.int32)
    src = [empty if b is None or len(b) == 0 else np.asarray(b, np.int32).reshape(-1, 5) for b in box_lists]
    matrices = np.asarray(matrices, np.float64)
    assert matrices.shape == (len(src), 3, 3), (matrices.shape, len(src))
    out = []
    for b, m in zip(src, matrices):
        if np.array_equal(m, np.eye(3)) or len(b) == 0:
            out.append(b.copy())
            continue
        bx = b.astype(np.float64)
        xa, ya, xb, yb = bx[:, 0], bx[:, 1], bx[:, 0] + bx[:, 2] - 1, bx[:, 1] + bx[:, 3] - 1
        px = np.stack([xa, xb, xa, xb], 1)
        py = np.stack([ya, ya, yb, yb], 1)
        qx = (m[0, 0] * px + m[0, 1] * py) + m[0, 2]
        qy = (m[1, 0] * px + m[1, 1] * py) + m[1, 2]
        x0, x1 = np.floor(qx.min(1) + 0.5).astype(np.int64), np.floor(qx.max(1) + 0.5).astype(np.int64)
        y0, y1 = np.floor(qy.min(1) + 0.5).astype(np.int64), np.floor(qy.max(1) + 0.5).astype(np.int64)
        full = (x1 - x0 + 1) * (y1 - y0 + 1)
        cx0, cy0, cx1, cy1 = np.maximum(x0, 0), np.maximum(y0, 0), np.minimum(x1, w - 1), np.minimum(y1, h - 1)
        cw, ch = cx1 - cx0 + 1, cy1 - cy0 + 1
        keep = (cw >= 2) & (ch >= 2)
        keep &= ~((cw * ch).astype(np.float64) < np.float64(min_visible) * full.astype(np.float64))
        out.append(np.stack([cx0, cy0, cw, ch, b[:, 4].astype(np.int64)], 1)[keep].astype(np.int32).reshape(-1, 5))
    return out


def affine_coords(records, size, dtype=np.float32):
    """The source coordinates y3_affine_batch evaluates, restated: (sx, sy) of shape [n, h, w] each, in `dtype` arithmetic with the
    kernel's order of unfused operations, sx = (m0 * x + m1 * y) + m2 and sy = (m3 * x + m4 * y) + m5, x and y the output pixel's
    column and row converted to `dtype`.  dtype float32 reproduces the kernel bit for bit; float64 (the float32 coefficients
    widened) is the exact-coordinate mode the comparison with scipy uses."""
    h, w = int(size[0]), int(size[1])
    m = np.asarray(records['m']).astype(dtype).reshape(-1, 6)
    x = np.arange(w).astype(dtype)[None, None, :]
    y = np.arange(h).astype(dtype)[None, :, None]
    c = lambda k: m[:, k][:, None, None]
    sx = (c(0) * x + c(1) * y) + c(2)
    sy = (c(3) * x + c(4) * y) + c(5)
    assert sx.dtype == dtype and sy.dtype == dtype
    return sx, sy


def affine_reference(batch, records, coords=np.float32, detail=False):
    """y3_affine_batch restated in NumPy (the oracle of the tests): batch [n, c, h, w] float32 -> float64 [n, c, h, w].

    Coordinates as affine_coords(records, (h, w), coords); x0 = floor(sx), fx = sx - x0 in that dtype (y alike).  The four taps
    (y0 + {0, 1}, x0 + {0, 1}) carry the weights (1 - fy | fy) * (1 - fx | fx), formed in float64; a tap outside the image has the
    value `fill`; a tap whose weight is exactly zero contributes nothing, whatever it holds (NaN and Inf included).  A pixel with
    exactly one non-zero weight is that tap itself.  detail=True returns (values, magnitude, single, bits): magnitude = the
    float64 sum of |weight * tap| the error bound of the tests scales with, single = the pixels with one non-zero weight, and
    bits = uint32, for those pixels the tap's own bit pattern (NaN payload and -0.0 kept), elsewhere the float32 rounding of the
    value."""
    batch = np.ascontiguousarray(batch, dtype=np.float32)
    n, ch, h, w = batch.shape
    records = np.asarray(records, dtype=AFFINE_RECORD)
    assert records.shape == (n,)
    sx, sy = affine_coords(records, (h, w), coords)
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f).astype(np.float64), (sy - y0f).astype(np.float64)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    val = np.zeros((n, ch, h, w), np.float64)
    mag = np.zeros((n, ch, h, w), np.float64)
    bits = np.zeros((n, ch, h, w), np.uint32)
    count = np.zeros((n, h, w), np.int64)
    words = batch.view(np.uint32)
    img = np.arange(n)[:, None, None]
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            wgt = wy * wx
            live = wgt != 0
            yy, xx = y0 + dy, x0 + dx
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
            count += live
            for k in range(ch):
                fill = np.broadcast_to(records['fill'][:, None, None], (n, h, w))
                tap32 = np.where(inside, batch[img, k, yc, xc], fill).astype(np.float32)
                with np.errstate(invalid='ignore', over='ignore'):
                    tap = tap32.astype(np.float64)              # (a signalling NaN raises 'invalid' when it is widened)
                    term = np.where(live, wgt * np.where(live, tap, 0.0), 0.0)
                val[:, k] += term
                mag[:, k] += np.abs(term)
                tapbits = np.where(inside, words[img, k, yc, xc], np.ascontiguousarray(fill.astype(np.float32)).view(np.uint32))
                bits[:, k] = np.where(live, tapbits, bits[:, k])
    single = np.broadcast_to((count == 1)[:, None], val.shape)
    with np.errstate(invalid='ignore', over='ignore'):
        rounded = val.astype(np.float32).view(np.uint32)
    bits = np.where(single, bits, rounded)
    if detail:
        return val, mag, single, bits
    return val


# ---- colour / tone jitter and MixUp (not in the reference) -----------------------------------------------------
# y3_photo_record (include/yolo3hip.h), one per OUTPUT image of a y3_photometric_batch call
PHOTO_RECORD = np.dtype([('m', '<f4', (9,)), ('bias', '<f4', (3,)), ('gamma', '<f4'), ('white', '<f4'), ('partner', '<i4'), ('lambda', '<f4')])
assert PHOTO_RECORD.itemsize == 64
_PHOTO_STREAM = 0xC0105           # folded into the key after (seed, shard, batch, image): apart from the mosaic's and the affine's words
_MIXUP_STREAM = 0x313C5           # MixUp's own stream, so that --photo_seed == --mixup_seed does not couple the two draws
# RGB -> YIQ (NTSC).  The rows of I and Q sum to zero and the row of Y to one, so grey (r = g = b) has no chroma and its own luma.
_YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]], np.float64)
_YIQ_INV = np.linalg.inv(_YIQ)


def photo_identity_records(n):
    """n records that leave their image alone: identity matrix, no bias, gamma 1, white 0 (no clamp), lambda 1, partner = itself."""
    rec = np.zeros(int(n), PHOTO_RECORD)
    rec['m'] = np.eye(3, dtype=np.float32).reshape(9)
    rec['gamma'] = 1
    rec['lambda'] = 1
    rec['partner'] = np.arange(int(n))
    return rec


def colour_matrix(hue_turns=0.0, saturation=1.0, value=1.0):
    """float64 3 x 3 matrix on (r, g, b): the chroma plane (I, Q) of YIQ rotated by 2 pi hue_turns and scaled by `saturation`, the
    luma Y scaled by `value`, converted back to RGB -- the linear hue-rotate and saturate operators, not a piecewise HSV round trip:
    continuous in all three arguments, M(h1) M(h2) = M(h1 + h2), grey maps to value * grey, saturation 0 sends a pixel to its luma
    grey.  hue_turns == 0 and saturation == 1 return value * I exactly (built directly, not as a rounded product)."""
    hue_turns, saturation, value = float(hue_turns), float(saturation), float(value)
    if hue_turns == 0.0 and saturation == 1.0:
        return value * np.eye(3)
    a = 2.0 * np.pi * hue_turns
    mid = np.array([[value, 0, 0], [0, saturation * np.cos(a), -saturation * np.sin(a)], [0, saturation * np.sin(a), saturation * np.cos(a)]], np.float64)
    return _YIQ_INV @ mid @ _YIQ


def _stream(seed, shard, batch_index, image, stream):
    """The counter-based stream of one image (draw_affine's construction): j -> the 64-bit word u_j."""
    key = 0
    for v in (seed, shard, batch_index, image, stream):
        key = _mix64((key ^ (int(v) & _M64)) + _GOLDEN)
    return lambda j: _mix64(key + (j + 1) * _GOLDEN)


def draw_photometric(seed, shard, batch_index, n, channels, prob, hue=0.0, saturation=0.0, value=0.0, gamma=0.0, white=255.0):
    """PHOTO_RECORD [n] (lambda 1: no MixUp) for the batch_index-th batch of n images on reader shard `shard`: a pure function of
    its arguments, counter based exactly as draw_affine is.  Image i owns the key folded over (seed, shard, batch_index, i, 0xC0105)
    -- k = 0; for v in those five: k = mix((k ^ v) + 0x9E3779B97F4A7C15) --, so its draw does not depend on n; its j-th word is
    u_j = mix(key + (j + 1) * 0x9E3779B97F4A7C15), the uniform U_j = (u_j >> 11) * 2^-53 in [0, 1), and a value in [lo, hi] is
    lo + (hi - lo) * U_j.  Draw order per image:
      U_0   the image is changed when U_0 < prob; otherwise it gets the identity record, the other words unused
      U_1   hue rotation in [-hue, hue] turns           (channels == 3 only; the word is skipped, not reused, when channels == 1)
      U_2   saturation gain in [1 - saturation, 1 + saturation]     (channels == 3 only, likewise)
      U_3   value gain in [1 - value, 1 + value]
      U_4   tone exponent e in [-gamma, gamma]; the record's gamma is 2^e, uniform in the exponent
    m = colour_matrix(hue, saturation, value) rounded once to float32 (channels == 1: m[0] = the value gain), bias 0, the clamp
    to [0, white] on.  A changed image whose draw is neutral (every magnitude zero) gets the identity record exactly, clamp off.
    Note that a value gain alone is cancelled by the z-score that follows, up to the clamp at `white`: it matters through the
    clamp and in a mixed image only."""
    n, channels = int(n), int(channels)
    if n < 1 or channels not in (1, 3):
        raise ValueError('draw_photometric: n >= 1 and channels 1 or 3, got {} {}'.format(n, channels))
    if not float(white) > 0:
        raise ValueError('draw_photometric: white must be > 0, got {!r}'.format(white))
    rec = photo_identity_records(n)
    for i in range(n):
        word = _stream(seed, shard, batch_index, i, _PHOTO_STREAM)
        u = lambda j: (word(j) >> 11) * 2.0 ** -53
        if not u(0) < prob:
            continue
        between = lambda j, mag: -float(mag) + 2.0 * float(mag) * u(j)
        h, s = (between(1, hue), 1.0 + between(2, saturation)) if channels == 3 else (0.0, 1.0)
        v, e = 1.0 + between(3, value), between(4, gamma)
        if (h, s, v, e) == (0.0, 1.0, 1.0, 0.0):
            continue
        m = colour_matrix(h, s, v)
        rec['m'][i] = m.reshape(9).astype(np.float32) if channels == 3 else np.array([v, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
        rec['gamma'][i] = 2.0 ** e
        rec['white'][i] = white
    return rec


def draw_mixup(records, seed, shard, batch_index, prob, spread=0.1):
    """A copy of PHOTO_RECORD [n] `records` with `partner` and `lambda` set for MixUp (Zhang et al., "mixup"; as used for detection
    in "Bag of Freebies for Training Object Detection Neural Networks"): image i owns the key folded over (seed, shard,
    batch_index, i, 0x313C5), words and uniforms as in draw_photometric.  Draw order per image:
      U_0   the image is mixed when U_0 < prob and n > 1; otherwise lambda = 1 and partner = i, the other words unused
      u_1   partner: j = u_1 % (n - 1) over the other n - 1 images in ascending order, partner = j + (j >= i)
      U_2   lambda = (0.5 - spread) + 2 spread U_2, rounded once to float32: uniform in [0.5 - spread, 0.5 + spread]
    The papers draw lambda from Beta(a, a) (a = 1.5 for detection; 32 in other recipes): mass around 0.5.  A uniform window
    around 0.5 stands in for it here because it keeps the draw a closed-form function of one word (no rejection loop, so the
    number of words per image is fixed); it is not a Beta draw and is not claimed to be one.  out_i = lambda * image_i + (1 -
    lambda) * image_partner, each image finished under its own record."""
    rec = np.array(records, dtype=PHOTO_RECORD, copy=True)
    n = len(rec)
    if not 0.0 <= float(spread) <= 0.5:
        raise ValueError('draw_mixup: spread must be in [0, 0.5], got {!r}'.format(spread))
    for i in range(n):
        rec['partner'][i], rec['lambda'][i] = i, 1.0
        if n < 2:
            continue
        word = _stream(seed, shard, batch_index, i, _MIXUP_STREAM)
        if not (word(0) >> 11) * 2.0 ** -53 < prob:
            continue
        j = word(1) % (n - 1)
        rec['partner'][i] = j + (j >= i)
        rec['lambda'][i] = (0.5 - float(spread)) + 2.0 * float(spread) * ((word(2) >> 11) * 2.0 ** -53)
    return rec


def mixup_boxes(box_lists, records):
    """The boxes of the output images of y3_photometric_batch: image i keeps its own boxes, followed by its partner's where
    records['lambda'][i] < 1 (a mixed image shows the objects of both).  box_lists: one int32 [k, 5] array per image, None or empty
    = no boxes.  Returns one fresh int32 [k', 5] array per image ([0, 5] when empty): order kept, nothing dropped or clipped, no
    result shares memory with an input."""
    empty = np.zeros((0, 5), np.int32)
    src = [empty if b is None or len(b) == 0 else np.asarray(b, np.int32).reshape(-1, 5) for b in box_lists]
    records = np.asarray(records, dtype=PHOTO_RECORD)
    assert records.shape == (len(src),), (records.shape, len(src))
    out = []
    for i, b in enumerate(src):
        if records['lambda'][i] < 1:
            out.append(np.concatenate([b, src[int(records['partner'][i])]]).astype(np.int32).reshape(-1, 5))
        else:
            out.append(b.copy())
    return out


def _photo_finish(img, r, dtype):
    """Stages 1-3 of y3_photometric_batch on one image [c, h, w] float32 under record r -> (the finished image in `dtype`, the
    float32 value t after the clamp).  Stages 1 and 2 are float32 in the kernel's order whatever `dtype` is."""
    c = img.shape[0]
    m = np.asarray(r['m'], np.float32).reshape(3, 3)
    rows = []
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for k in range(c):
            acc = None
            for j in range(c):
                if m[k, j] == 0:
                    continue
                t = img[j] if m[k, j] == 1 else m[k, j] * img[j]
                acc = t if acc is None else acc + t
            b = np.float32(r['bias'][k])
            if b != 0:
                acc = np.full(img.shape[1:], b, np.float32) if acc is None else acc + b
            rows.append(np.zeros(img.shape[1:], np.float32) if acc is None else acc)
        t = np.stack(rows)
        assert t.dtype == np.float32
        white, gamma = np.float32(r['white']), np.float32(r['gamma'])
        if white > 0:
            t = np.where(t < 0, np.float32(0), np.where(t > white, white, t))
        if gamma == 1:
            return t.astype(dtype), t
        s = t / white                      # float32 in both modes: an IEEE division, the same word as the kernel's
        assert s.dtype == np.float32
        if dtype == np.float32:
            y = white * np.where(s == 0, np.float32(0), np.exp2(gamma * np.log2(s)))
            assert y.dtype == np.float32
        else:
            s = s.astype(np.float64)
            y = np.float64(white) * np.where(s == 0, 0.0, np.power(np.where(s == 0, 1.0, s), np.float64(gamma)))
    return y, t


def photometric_reference(batch, records, dtype=np.float32, detail=False):
    """y3_photometric_batch restated in NumPy (the oracle of the tests): batch [n, c, h, w] float32 -> `dtype` [n, c, h, w].

    dtype float32 follows the kernel operation by operation -- the matrix with its skipped zero terms, unmultiplied ones and
    skipped zero bias, the clamp as selects, the curve as white * exp2(gamma * log2(t / white)), the blend (lambda * a) + ((1 -
    lambda) * b) -- and is bit-exact for every record without a tone curve (NumPy's exp2 / log2 are not the device's).  dtype
    float64 is the exact-curve mode of the error bound: stages 1 and 2 and the quotient s = t / white stay float32 (they are
    exact restatements: the division is IEEE on both sides, so a t below white * 2^-149 gives s = 0 and y = 0 here as there), the
    power s^gamma and its product with white are evaluated in float64 on that s, and the blend in float64 with the float32 lambda
    and the float32 1 - lambda.  detail=True returns (out, finished, t): `finished` the images after stage 3 in `dtype` (the blend mixes
    finished[i] and finished[partner]), t the float32 values after the clamp."""
    batch = np.ascontiguousarray(batch, dtype=np.float32)
    n = batch.shape[0]
    records = np.asarray(records, dtype=PHOTO_RECORD)
    assert batch.ndim == 4 and batch.shape[1] in (1, 3) and records.shape == (n,)
    done = [_photo_finish(batch[i], records[i], dtype) for i in range(n)]
    finished = np.stack([d[0] for d in done])
    t = np.stack([d[1] for d in done])
    out = finished.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            lam = np.float32(records['lambda'][i])
            if lam != 1:
                rest = np.float32(1) - lam
                out[i] = (lam.astype(dtype) * finished[i]) + (rest.astype(dtype) * finished[int(records['partner'][i])])
    assert out.dtype == dtype
    if detail:
        return out, finished, t
    return out
