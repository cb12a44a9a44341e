"""y3_augment_batch (csrc/augment.hip) against the host augmentation (yolo3/augment.py, scipy) and the reference's goldens,
and the reader / dataset / CLI path that uses it (ImageReader(..., augmentation_device='gpu'))."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage

from augment_edges import philox_normals as _philox_normals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _record(H, W, rows, cols, dy=0, dx=0, rx=0, ry=0, noise=0.0, u=0.5, blur=0.0, seed=0):
    from yolo3 import augment
    rec = np.zeros(1, augment.AUG_RECORD)
    rec[0] = (H, W, rows, cols, dy, dx, int(rx), int(ry), noise, u, blur, 0, seed)
    return rec


def _run(imgs, records, crop, ranges=False):
    """imgs: [B, H, W(, C)] ndarray (uint8 / uint16 / float32) -> device augment -> numpy [B, C, h, w] (and min / max)."""
    torch = _torch()
    from yolo3.imagereader import augment_device
    imgs = np.asarray(imgs)
    if imgs.ndim == 3:
        imgs = imgs[..., None]
    src = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    r = augment_device(src, np.concatenate(records) if isinstance(records, list) else records, crop, ranges=ranges)
    torch.cuda.synchronize()
    if ranges:
        return r[0].cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy()
    return r.cpu().numpy()


def _host_crop(img, rec, crop):
    """float64 HWC (or HW) crop of one record with the host path's helpers (augment.transform_image's arithmetic)."""
    from yolo3 import augment
    img = np.asarray(img, dtype=np.float32)
    H, W = img.shape[:2]
    r = rec[0] if rec.shape else rec
    if (r['rows'], r['cols']) != (H, W):
        img = augment.rescale_bilinear(img, r['rows'] / H, r['cols'] / W)
    img = np.asarray(img, dtype=np.float64)[r['dy']:r['dy'] + crop[0], r['dx']:r['dx'] + crop[1]]
    if r['reflect_x']:
        img = np.fliplr(img)
    if r['reflect_y']:
        img = np.flipud(img)
    return img


def _chw(img):
    return img[None] if img.ndim == 2 else np.transpose(img, (2, 0, 1))


def test_resample_matches_reference_goldens(golden_dir):
    """Resample + crop + flips against the reference's own pixels (augment.npz affine_img_* / affine_img2, produced by the
    reference's augment.py with skimage's rescale): 5e-3 on the 0..255 range, identity scale to 1e-6."""
    z = np.load(os.path.join(golden_dir, 'augment.npz'))
    img = z['img']
    for i, (c, crop) in enumerate(zip(z['affine_img_cases'], z['affine_img_crops'])):
        rx, ry, sx, sy = c
        dx, dy = z['affine_img_%d_dxdy' % i].tolist()
        rows = int(np.round(sy * img.shape[0])) if (sx, sy) != (1, 1) else img.shape[0]
        cols = int(np.round(sx * img.shape[1])) if (sx, sy) != (1, 1) else img.shape[1]
        out = _run(img[None], _record(90, 120, rows, cols, dy, dx, rx, ry), tuple(crop))[0]
        err = np.abs(out - _chw(z['affine_img_%d' % i])).max()
        assert err <= (1e-6 if sx == 1 and sy == 1 else 5e-3), (i, err)
    img2 = z['img2']                                                   # 2-D image: C = 1
    dx, dy = z['affine_img2_dxdy'].tolist()
    rec = _record(70, 100, int(np.round(0.95 * 70)), int(np.round(1.2 * 100)), dy, dx, True, False)
    out = _run(img2[None], rec, (60, 90))[0]
    assert out.shape == (1, 60, 90) and np.abs(out[0] - z['affine_img2']).max() <= 5e-3


@pytest.mark.parametrize('dtype,C', [(np.uint8, 3), (np.uint16, 3), (np.float32, 3), (np.uint8, 1), (np.float32, 1)])
def test_resample_matches_host_transform_sweep(dtype, C):
    """Against augment.transform_image's arithmetic (float64) over scales 0.85-1.3 per axis (incl. the training range and
    exactly 1), every flip combination, crop offsets 0 and maximal, in one batch of mixed rescaled sizes (> one launch chunk):
    <= 1e-3 on 0..255 (scale 1: exact), and the device's min / max of each crop equal the host crop's to the same bound."""
    rng = np.random.default_rng(7)
    H, W, crop = 90, 120, (64, 96)
    shape = (H, W, C) if C > 1 else (H, W)
    img = rng.integers(0, 256, shape).astype(dtype)
    if dtype == np.uint16:
        img = (img.astype(np.uint32) * 257).astype(np.uint16)         # full 16-bit range
    if dtype == np.float32:
        img = img + rng.random(shape).astype(np.float32)
    scale = 1.0 / 257 if dtype == np.uint16 else 1.0                  # compare on the 0..255 range
    recs, wants = [], []
    for (sy, sx), rx, ry, far in itertools.product([(0.85, 1.3), (1.0, 1.1), (1.05, 1.0), (1.3, 0.85), (1.1, 1.07), (1, 1)],
                                                   (0, 1), (0, 1), (False, True)):
        rows, cols = int(np.round(sy * H)), int(np.round(sx * W))
        rows, cols = max(rows, crop[0]), max(cols, crop[1])
        dy, dx = (rows - crop[0], cols - crop[1]) if far else (0, 0)
        rec = _record(H, W, rows, cols, dy, dx, rx, ry)
        recs.append(rec)
        wants.append(_host_crop(img, rec, crop))
    out, mn, mx = _run(np.stack([img] * len(recs)), recs, crop, ranges=True)
    for i, (rec, want) in enumerate(zip(recs, wants)):
        err = np.abs(out[i] - _chw(want)).max() * scale
        exact = rec[0]['rows'] == H and rec[0]['cols'] == W
        assert err <= (0.0 if exact else 1e-3), (i, rec, err)
        assert abs(mn[i] - want.min()) * scale <= 1e-3 and abs(mx[i] - want.max()) * scale <= 1e-3, (i, mn[i], want.min(), mx[i], want.max())
    full = _run(img[None], _record(H, W, H, W), (H, W))[0]                           # scale 1, no crop: an exact copy
    assert np.array_equal(full, _chw(img.astype(np.float32)))


@pytest.mark.parametrize('C', [3, 1])
def test_blur_matches_scipy_gaussian_filter(C):
    """Blur alone (noise 0) against scipy.ndimage.gaussian_filter(host crop, sigma, mode='reflect') on every axis, the channel
    axis included (C = 3: radius up to 8 > 3 channels, the reflections wrap), <= 1e-3 on 0..255."""
    rng = np.random.default_rng(11)
    H, W, crop = 72, 88, (64, 80)
    shape = (H, W, C) if C > 1 else (H, W)
    img = rng.integers(0, 256, shape).astype(np.uint8)
    sigmas = [0.05, 0.3, 0.7, 1.0, 1.5, 1.99, 2.0]
    recs = [_record(H, W, 79, 95, 5 + i, 2 * i, i % 2, (i // 2) % 2, blur=s) for i, s in enumerate(sigmas)]
    recs.append(_record(H, W, 79, 95, 2, 2, blur=-1.0))                   # sigma <= 0: no blur
    out = _run(np.stack([img] * len(recs)), recs, crop)
    for i, rec in enumerate(recs):
        base = _host_crop(img, rec, crop)
        s = rec[0]['blur_sigma']
        want = scipy.ndimage.gaussian_filter(base, float(s), mode='reflect') if s > 0 else base
        err = np.abs(out[i] - _chw(want)).max()
        assert err <= 1e-3, (C, float(s), err)
    # a blurred image that mixes channels really differs from the unmixed per-channel blur (the fold is exercised)
    if C == 3:
        per_channel = scipy.ndimage.gaussian_filter(_host_crop(img, recs[5], crop), (1.99, 1.99, 0), mode='reflect')
        assert np.abs(out[5] - _chw(per_channel)).max() > 1.0


def test_noise_statistics_and_stream():
    """Batch with noise minus the same batch without: per image mean ~ 0 and std ~ |sigma_i| (sigma_i from the host crop's range
    and u_noise) within 4 standard errors, 68.27 % +- 0.5 % inside +-1 sigma, lag-1 correlations along W, H, C < 0.01, images
    with different seeds uncorrelated; the draws are the documented Philox stream, and the same records give the same bits."""
    rng = np.random.default_rng(5)
    H, W, C, crop = 256, 256, 3, (240, 240)
    img = rng.integers(0, 256, (H, W, C)).astype(np.uint8)
    us = [0.02, 0.98, 0.3, 0.75, 0.1, 0.6]
    recs = [_record(H, W, 270, 262, 5 * i, 3 * i, i % 2, 0, noise=0.03, u=u, seed=int(rng.integers(1, 2**63))) for i, u in enumerate(us)]
    clean = [r.copy() for r in recs]
    for r in clean:
        r[0]['noise_severity'] = 0
    noisy = _run(np.stack([img] * len(recs)), recs, crop)
    base = _run(np.stack([img] * len(recs)), clean, crop)
    again = _run(np.stack([img] * len(recs)), recs, crop)
    assert np.array_equal(noisy, again)
    zs = []
    for i, rec in enumerate(recs):
        host = _host_crop(img, rec, crop)
        sigma = 0.03 * (2 * us[i] - 1) * (host.max() - host.min())
        d = (noisy[i].astype(np.float64) - base[i]).ravel()
        N = d.size
        assert abs(d.mean()) <= 4 * abs(sigma) / np.sqrt(N), (i, d.mean(), sigma)
        assert abs(d.std() - abs(sigma)) <= 4 * abs(sigma) / np.sqrt(2 * N), (i, d.std(), sigma)
        z = d / sigma
        assert abs(np.mean(np.abs(z) <= 1) - 0.6827) <= 0.005, i
        zc = z.reshape(C, crop[0], crop[1])
        for a, b in ((zc[:, :, 1:], zc[:, :, :-1]), (zc[:, 1:], zc[:, :-1]), (zc[1:], zc[:-1])):
            assert abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]) < 0.01, i
        assert np.abs(z - _philox_normals(int(rec[0]['seed']), N)).max() <= 1e-3, i     # the header's stream, element order CHW
        zs.append(z)
    for a, b in itertools.combinations(zs, 2):
        assert abs(np.corrcoef(a, b)[0, 1]) < 0.01


def test_training_chain_repeats_bit_for_bit():
    """The full chain at the training severities (imagereader.TRAIN_AUGMENTATION): the same bits over 20 launches at
    8 x 416^2 x 3 and 8 x 608^2 x 3."""
    torch = _torch()
    from yolo3 import augment
    from yolo3.imagereader import TRAIN_AUGMENTATION, augment_device
    rng = np.random.default_rng(2)
    for S in (416, 608):
        imgs = rng.integers(0, 256, (8, S, S, 3), dtype=np.uint8)
        np.random.seed(S)
        recs = np.concatenate([augment.draw_augmentation((S, S, 3), None, crop_to=(S, S), **TRAIN_AUGMENTATION)[0] for _ in range(8)])
        recs[0]['blur_sigma'] = 1.9                                     # at least one image takes every pass
        src = torch.from_numpy(imgs).cuda()
        first = augment_device(src, recs, (S, S)).clone()
        for _ in range(19):
            assert torch.equal(augment_device(src, recs, (S, S)), first), S
        assert bool(torch.isfinite(first).all())


def _make_lmdb(path, n, size, seed=3):
    import build_lmdb
    from yolo3 import lmdbio
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n):
        img = rng.integers(0, 256, size, dtype=np.uint8)
        k = int(rng.integers(1, 4))
        wh = rng.integers(20, size[0] // 2, (k, 2))
        xy = np.stack([rng.integers(0, size[1] - wh[:, 0]), rng.integers(0, size[0] - wh[:, 1])], 1)
        boxes = np.concatenate([xy, wh, rng.integers(0, 2, (k, 1))], 1).astype(np.int32)
        items.append(build_lmdb.make_record(img, boxes, i, 'img%03d' % i))
    lmdbio.write_environment(path, items)


def _batches(reader, nb, prefetch):
    ds = reader.get_tf_dataset().batch(4)
    if prefetch:
        ds = ds.prefetch(2)
    it = iter(ds)
    out = [[t.cpu().numpy() for t in next(it)] for _ in range(nb)]
    it.close()
    return out


@pytest.mark.parametrize('prefetch', [False, True])
def test_dataset_identity_records_bit_identical_to_cpu_mode(tmp_path, prefetch):
    """use_augmentation=False: the GPU mode uploads the stored uint8 pixels and converts them on the device; batches after the
    z-score and all three label tensors are the CPU mode's bits, and so is get_example()."""
    from yolo3.imagereader import ImageReader
    path = str(tmp_path / 'train-syn.lmdb')
    _make_lmdb(path, 10, (96, 96, 3))
    anchors = [(64, 384), (384, 64)]
    got = {}
    for mode in ('cpu', 'gpu'):
        rd = ImageReader(path, anchors, use_augmentation=False, shuffle=False, num_workers=1, augmentation_device=mode)
        rd.startup()
        try:
            got[mode + '_example'] = rd.get_example()          # first: the prefetch thread takes a varying number of examples ahead
            got[mode] = _batches(rd, 3, prefetch)
        finally:
            rd.shutdown()
    for bc, bg in zip(got['cpu'], got['gpu']):
        assert bg[0].shape == (4, 3, 96, 96) and bg[0].dtype == np.float32
        assert all(np.array_equal(a, b) for a, b in zip(bc, bg))
    ec, eg = got['cpu_example'], got['gpu_example']
    assert len(eg) == 4 and eg[0].shape == (3, 96, 96) and all(np.array_equal(a, b) for a, b in zip(ec, eg))


def test_dataset_with_augmentation_on_gpu(tmp_path):
    """use_augmentation=True in GPU mode: batches of the right shape / dtype / device, finite; the worker's labels are
    format_boxes of draw_augmentation's boxes, and its record really changes the pixels."""
    torch = _torch()
    from yolo3 import augment, lmdbio
    from yolo3.imagereader import ImageReader, TRAIN_AUGMENTATION, augment_device, format_boxes
    from yolo3.isg_ai_pb import ImageYoloBoxesPair
    path = str(tmp_path / 'train-syn.lmdb')
    _make_lmdb(path, 8, (128, 128, 3), seed=4)
    anchors = [(64, 384), (384, 64)]
    rd = ImageReader(path, anchors, use_augmentation=True, shuffle=True, num_workers=2, balance_classes=True, augmentation_device='gpu')
    with lmdbio.Environment(path) as env:
        for j, key in enumerate(rd.keys_flat):
            np.random.seed(j)
            img, l1, l2, l3, rec = rd.load_example(key, env)
            _, boxes = ImageYoloBoxesPair().ParseFromString(env.get(key)).to_arrays()
            np.random.seed(j)
            want_rec, want_boxes = augment.draw_augmentation(img.shape, boxes.copy(), crop_to=[128, 128], **TRAIN_AUGMENTATION)
            assert rec == want_rec
            want = format_boxes(want_boxes, (128, 128, 3), anchors, rd.get_number_classes())
            assert all(np.array_equal(a, b) for a, b in zip((l1, l2, l3), want))
            out = augment_device(torch.from_numpy(img[None].copy()).cuda(), rec, (128, 128))
            assert bool(torch.isfinite(out).all())
            if rec[0]['noise_severity'] > 0 and rec[0]['u_noise'] != 0.5:
                assert not torch.equal(out[0], torch.from_numpy(img).cuda().permute(2, 0, 1).float())
    rd.startup()
    try:
        for prefetch in (False, True):
            for b in _batches(rd, 2, prefetch):
                assert b[0].shape == (4, 3, 128, 128) and b[0].dtype == np.float32 and np.isfinite(b[0]).all()
                assert b[1].shape == (4, 4, 4, 2, 7) and b[3].shape == (4, 16, 16, 2, 7)
        ds = iter(rd.get_tf_dataset().batch(4).prefetch(2))
        x = next(ds)
        ds.close()
        assert x[0].is_cuda and x[0].dtype == torch.float32 and all(t.is_cuda for t in x[1:])
    finally:
        rd.shutdown()


def test_cli_train_with_gpu_augmentation(tmp_path):
    """train.py --augmentation_device gpu runs to completion on a tiny database and writes its checkpoint and test_loss.csv."""
    from test_gpu_cli import _write_dataset
    tmp = str(tmp_path)
    _write_dataset(tmp, 8, (256, 256, 3))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = os.path.join(tmp, 'out')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--batch_size', '2', '--test_every_n_steps', '3', '--train_database',
                        os.path.join(tmp, 'train-syn.lmdb'), '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out,
                        '--early_stopping', '1', '--use_augmentation', '1', '--augmentation_device', 'gpu', '--max_epochs', '2',
                        '--learning_rate', '1e-4'], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'augmentation_device = gpu' in r.stdout
    losses = [float(v) for v in open(os.path.join(out, 'test_loss.csv')).read().split()]
    assert len(losses) >= 1 and all(np.isfinite(losses))
    assert os.path.exists(os.path.join(out, 'saved_model', 'yolov3.npz')) and os.path.exists(os.path.join(out, 'checkpoint', 'ckpt.npz'))
