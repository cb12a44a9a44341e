"""Host half of the device augmentation path (ImageReader(..., augmentation_device='gpu')): augment.draw_augmentation draws
augment_image_box_pair's random decisions in the same order, and y3_augment_batch validates its records on the host."""
import itertools

import numpy as np
import pytest

from yolo3 import augment


def _apply_record_on_host(img, rec, crop_to):
    """The pixels of one record with the host helpers: rescale to (rows, cols), crop at (dy, dx), flips."""
    img = np.asarray(img, dtype=np.float32)
    H, W = img.shape[:2]
    if (rec['rows'], rec['cols']) != (H, W):
        img = augment.rescale_bilinear(img, rec['rows'] / H, rec['cols'] / W)
    else:
        img = np.asarray(img, dtype=np.float64)
    dy, dx = int(rec['dy']), int(rec['dx'])
    img = img[dy:dy + crop_to[0], dx:dx + crop_to[1]]
    if rec['reflect_x']:
        img = np.fliplr(img)
    if rec['reflect_y']:
        img = np.flipud(img)
    return np.asarray(img, dtype=np.float32)


def _boxes(rng, shape, k):
    wh = rng.integers(14, max(15, min(shape[:2]) // 2), (k, 2))
    xy = np.stack([rng.integers(0, shape[1] - wh[:, 0]), rng.integers(0, shape[0] - wh[:, 1])], 1)
    return np.concatenate([xy, wh, rng.integers(0, 3, (k, 1))], 1).astype(np.int32)


def _same_boxes(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


CASES = [((90, 120, 3), None), ((90, 120, 3), (64, 96)), ((70, 100), (60, 90)), ((64, 64, 1), None), ((48, 80, 3), (40, 40)),
         ((128, 96, 3), (128, 96))]


@pytest.mark.parametrize('shape,crop', CASES)
def test_draw_matches_host_path_without_noise_and_blur(shape, crop):
    """Boxes identical and the record's flips / rescaled size / crop offsets reproduce augment_image_box_pair's image exactly."""
    rng = np.random.default_rng(len(shape) * 100 + shape[0])
    img = rng.integers(0, 256, shape).astype(np.float32)
    crop_to = crop or shape[:2]
    for seed, (scale, refl, jit) in itertools.product(range(6), [(0, False, 0), (0.1, True, 0.03), (0.3, True, 0.08), (0.05, False, 0)]):
        boxes = _boxes(rng, shape, 3)
        kw = dict(reflection_flag=refl, crop_to=crop, scale_augmentation_severity=scale, box_size_augmentation_severity=jit,
                  box_location_jitter_severity=jit)
        np.random.seed(seed)
        want_img, want_boxes = augment.augment_image_box_pair(img.copy(), boxes.copy(), **kw)
        after_host = np.random.rand()
        np.random.seed(seed)
        rec, got_boxes = augment.draw_augmentation(img.shape, boxes.copy(), **kw)
        assert np.random.rand() == after_host                 # no noise / blur: the two paths consume the same draws
        assert rec.dtype == augment.AUG_RECORD and rec.shape == (1,)
        r = rec[0]
        assert (r['src_h'], r['src_w']) == shape[:2] and r['noise_severity'] == 0 and r['blur_sigma'] == 0 and r['seed'] == 0
        assert r['dy'] + crop_to[0] <= r['rows'] and r['dx'] + crop_to[1] <= r['cols']
        assert _same_boxes(got_boxes, want_boxes), (seed, scale)
        assert np.array_equal(_apply_record_on_host(img, r, crop_to), want_img), (seed, scale)


@pytest.mark.parametrize('noise,blur', [(0.03, 0), (0.03, 2), (0.5, 1.5), (0, 2)])
def test_draw_keeps_boxes_and_geometry_with_noise_and_blur(noise, blur):
    """With noise / blur on, everything up to the noise uniform is still the host path's: boxes, flips, sizes, offsets; the
    blur sigma lies in the host path's range; the noise seed is drawn only when there is noise."""
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (96, 112, 3)).astype(np.float32)
    for seed in range(8):
        boxes = _boxes(rng, img.shape, 4)
        kw = dict(reflection_flag=True, crop_to=(80, 96), noise_augmentation_severity=noise, scale_augmentation_severity=0.1,
                  blur_augmentation_max_sigma=blur, box_size_augmentation_severity=0.03, box_location_jitter_severity=0.03)
        np.random.seed(seed)
        _, want_boxes = augment.augment_image_box_pair(img.copy(), boxes.copy(), **kw)
        np.random.seed(seed)
        rec, got_boxes = augment.draw_augmentation(img.shape, boxes.copy(), **kw)
        assert _same_boxes(got_boxes, want_boxes), seed
        kw0 = dict(kw, noise_augmentation_severity=0, blur_augmentation_max_sigma=0)
        np.random.seed(seed)
        rec0, _ = augment.draw_augmentation(img.shape, boxes.copy(), **kw0)
        geometry = ['src_h', 'src_w', 'rows', 'cols', 'dy', 'dx', 'reflect_x', 'reflect_y']
        assert all(rec[0][f] == rec0[0][f] for f in geometry), seed
        r = rec[0]
        assert np.isclose(r['noise_severity'], noise) and 0 <= r['u_noise'] <= 1
        assert -blur <= r['blur_sigma'] <= blur
        assert (r['seed'] != 0) == (noise > 0)


def test_identity_record_is_crop_to_size():
    src = np.arange(50 * 60 * 3, dtype=np.float32).reshape(50, 60, 3)
    np.random.seed(3)
    want, _ = augment.crop_to_size(src, None, (40, 48))
    after = np.random.rand()
    np.random.seed(3)
    rec = augment.identity_record(src.shape, (40, 48))
    assert np.random.rand() == after
    assert np.array_equal(_apply_record_on_host(src, rec[0], (40, 48)), want)
    r = augment.identity_record((64, 64, 1))[0]
    assert (r['rows'], r['cols'], r['dy'], r['dx'], r['reflect_x'], r['reflect_y']) == (64, 64, 0, 0, 0, 0)


def _valid_record(h=32, w=40):
    rec = np.zeros(1, augment.AUG_RECORD)
    rec[0] = (h, w, h + 4, w + 6, 2, 3, 1, 0, 0.03, 0.7, 1.5, 0, 12345)
    return rec


def test_augment_batch_rejects_bad_records_without_device():
    """Every record is validated on the host before any launch: rejected with Y3_EINVAL and a message (the pointers are
    fake; nothing reaches a device)."""
    from yolo3 import _hip
    lib = _hip.lib
    fake = 1 << 20
    assert lib.y3_augment_workspace_bytes(8, 416, 416, 3) >= 8 * 3 * 416 * 416 * 4
    assert lib.y3_augment_workspace_bytes(0, 416, 416, 3) == 0

    def call(rec, dtype=0, c=3, h_out=32, w_out=40, h_in=32, w_in=40, src=fake):
        rec = np.ascontiguousarray(rec)
        return lib.y3_augment_batch(src, dtype, len(rec), h_in, w_in, c, rec.ctypes.data, h_out, w_out, fake, fake, None)

    def bad(field, value, word):
        rec = _valid_record()
        rec[0][field] = value
        assert call(rec) == -1, (field, value)
        assert word in lib.y3_last_error(), (field, value, lib.y3_last_error())

    bad('rows', 0, b'rescaled size')
    bad('cols', -3, b'rescaled size')
    bad('dy', 5, b'crop')              # dy + h_out = 37 > rows 36
    bad('dx', 7, b'crop')              # dx + w_out = 47 > cols 46
    bad('dy', -1, b'crop')
    bad('src_h', 33, b'source')
    bad('reflect_x', 2, b'reflect')
    bad('noise_severity', np.nan, b'noise')
    bad('noise_severity', np.inf, b'noise')
    bad('noise_severity', -0.1, b'noise')
    bad('u_noise', 1.5, b'noise')
    bad('blur_sigma', np.nan, b'blur')
    bad('blur_sigma', np.inf, b'blur')
    bad('blur_sigma', 2.2, b'blur')    # radius int(4 * 2.2 + 0.5) = 9 > 8
    # the bad record may be any one of the batch
    recs = np.concatenate([_valid_record(), _valid_record(), _valid_record()])
    recs[2]['rows'] = 10
    assert call(recs) == -1 and b'record 2' in lib.y3_last_error()
    assert call(_valid_record(), dtype=3) == -1 and b'dtype' in lib.y3_last_error()
    assert call(_valid_record(), c=2) == -1 and b'channels' in lib.y3_last_error()
    assert call(_valid_record(), c=4) == -1 and b'channels' in lib.y3_last_error()
    assert call(_valid_record(), src=None) == -1 and b'null' in lib.y3_last_error()
    with pytest.raises(_hip.HipError):
        _hip.check(call(_valid_record(), dtype=-1), 'y3_augment_batch')


def test_augment_batch_rejects_the_first_width_and_sigma_past_its_limits_without_device():
    """One pixel past the widest row the LDS stage takes (float32, C = 3: 2560 pixels = 30720 bytes) and the first sigma of
    radius 9 (int(4 * 2.125 + 0.5)): Y3_EINVAL and a message; the last accepted values are run by tests/test_gpu_augment_edges.py."""
    from yolo3 import _hip
    lib = _hip.lib
    fake = 1 << 20

    def call(rec, dtype, c, h_in, w_in, h_out, w_out):
        rec = np.ascontiguousarray(rec)
        return lib.y3_augment_batch(fake, dtype, 1, h_in, w_in, c, rec.ctypes.data, h_out, w_out, fake, fake, None)

    rec = np.zeros(1, augment.AUG_RECORD)
    rec[0] = (3, 2561, 3, 2561, 0, 0, 0, 0, 0, 0.5, 0, 0, 0)
    assert call(rec, 2, 3, 3, 2561, 3, 300) == -1 and b'exceed the LDS row stage' in lib.y3_last_error()
    rec[0] = (3, 5121, 3, 5121, 0, 0, 0, 0, 0, 0.5, 0, 0, 0)                # uint16, C = 3: 5120 pixels are the same 30720 bytes
    assert call(rec, 1, 3, 3, 5121, 3, 300) == -1 and b'exceed the LDS row stage' in lib.y3_last_error()
    rec = _valid_record()
    rec[0]['blur_sigma'] = 2.125
    assert call(rec, 0, 3, 32, 40, 32, 40) == -1 and b'blur sigma 2.125' in lib.y3_last_error()
    rec[0]['blur_sigma'] = np.nextafter(np.float32(2.125), np.float32(3))
    assert call(rec, 0, 3, 32, 40, 32, 40) == -1 and b'blur' in lib.y3_last_error()


def test_reader_gpu_mode_hands_out_raw_pixels_and_records(tmp_path):
    """augmentation_device='gpu' workers: stored pixels (HWC, stored dtype), labels of the draw's boxes, one record."""
    import build_lmdb
    from yolo3 import lmdbio
    from yolo3.imagereader import ImageReader, format_boxes, TRAIN_AUGMENTATION
    rng = np.random.default_rng(8)
    items, truth = [], {}
    for i in range(4):
        img = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
        boxes = _boxes(rng, img.shape, 2)
        key, val = build_lmdb.make_record(img, boxes, i, 'img%03d' % i)
        items.append((key, val))
        truth[key] = (img, boxes)
    path = str(tmp_path / 'train-g.lmdb')
    lmdbio.write_environment(path, items)
    anchors = [(64, 384), (384, 64)]
    with pytest.raises(AssertionError):
        ImageReader(path, anchors, augmentation_device='tpu')
    plain_cpu = ImageReader(path, anchors, use_augmentation=False, shuffle=False)
    plain_gpu = ImageReader(path, anchors, use_augmentation=False, shuffle=False, augmentation_device='gpu')
    aug_gpu = ImageReader(path, anchors, use_augmentation=True, shuffle=False, augmentation_device='gpu')
    with lmdbio.Environment(path) as env:
        for key in plain_cpu.keys_flat:
            img, boxes = truth[key]
            c = plain_cpu.load_example(key, env)
            g = plain_gpu.load_example(key, env)
            assert len(g) == 5 and g[0].dtype == np.uint8 and np.array_equal(g[0], img)
            assert all(np.array_equal(a, b) for a, b in zip(c[1:4], g[1:4]))
            r = g[4][0]
            assert (r['rows'], r['cols'], r['dy'], r['dx'], r['noise_severity'], r['blur_sigma']) == (96, 96, 0, 0, 0, 0)
            np.random.seed(11)
            a = aug_gpu.load_example(key, env)
            np.random.seed(11)
            rec, want_boxes = augment.draw_augmentation(img.shape, boxes.copy(), crop_to=[96, 96], **TRAIN_AUGMENTATION)
            assert a[4] == rec
            want = format_boxes(want_boxes, (96, 96, 3), anchors, aug_gpu.get_number_classes())
            assert all(np.array_equal(x, y) for x, y in zip(a[1:4], want))
