"""CPU-only tests of the opt-in colour / tone jitter and MixUp: the record layout, the counter-based draws, the
properties of colour_matrix, mixup_boxes, the NumPy restatement's own rules, the argument checks of Dataset.photometric() /
Dataset.mixup() and train.py, the host-side refusals of y3_photometric_batch, and the untouched default path."""
import os
import sys

import numpy as np
import pytest

import photometric_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
sys.path.insert(0, PKG)

ANCHORS = [(64, 384), (384, 64)]
LUMA = np.array([0.299, 0.587, 0.114])


# ---- the record ------------------------------------------------------------------------------------------------------------
def test_record_dtype_matches_the_header():
    from yolo3 import augment, _hip
    d = augment.PHOTO_RECORD
    assert d.itemsize == 64 and d.names == ('m', 'bias', 'gamma', 'white', 'partner', 'lambda')
    assert [d.fields[k][1] for k in d.names] == [0, 36, 48, 52, 56, 60]
    assert d['m'].shape == (9,) and d['bias'].shape == (3,) and d['partner'].base == np.dtype('<i4') and d['lambda'] == np.dtype('<f4')
    hdr = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    assert ' y3_photometric_batch(' in hdr and 'typedef struct y3_photo_record' in hdr
    assert 'y3_photometric_batch' in _hip.SIGNATURES and hasattr(_hip.lib, 'y3_photometric_batch')
    r = augment.photo_identity_records(5)
    assert r.dtype == d and np.array_equal(r['m'], np.tile(np.eye(3, dtype=np.float32).reshape(9), (5, 1))) and not r['bias'].any()
    assert (r['gamma'] == 1).all() and (r['white'] == 0).all() and (r['lambda'] == 1).all() and np.array_equal(r['partner'], np.arange(5))


# ---- the draws -------------------------------------------------------------------------------------------------------------
def test_draws_are_pure_functions_of_their_arguments():
    from yolo3 import augment
    args = (3, 1, 7, 8, 3, 1.0, 0.05, 0.7, 0.4, 0.5, 255.0)
    a = augment.draw_photometric(*args)
    assert a.dtype == augment.PHOTO_RECORD and a.shape == (8,)
    assert a.tobytes() == augment.draw_photometric(*args).tobytes()
    for other in ((3, 1, 8), (3, 0, 7), (4, 1, 7)):          # another batch index, shard, seed
        assert a.tobytes() != augment.draw_photometric(*other, *args[3:]).tobytes(), other
    assert len({a[i]['m'].tobytes() for i in range(8)}) == 8  # another image, other words
    state = np.random.get_state()[1].copy()                  # no global np.random
    augment.draw_mixup(augment.draw_photometric(0, 0, 0, 8, 3, 0.5, 0.1), 0, 0, 0, 0.5)
    assert np.array_equal(np.random.get_state()[1], state)
    # image i does not depend on n
    assert augment.draw_photometric(3, 1, 7, 40, *args[4:])[:8].tobytes() == a.tobytes()
    assert augment.draw_photometric(3, 1, 7, 3, *args[4:]).tobytes() == a[:3].tobytes()
    assert (a['white'] == 255).all() and (a['lambda'] == 1).all() and not a['bias'].any()
    # MixUp likewise; its lambda and whether image i is mixed do not depend on n (the partner is drawn among n - 1)
    m = augment.draw_mixup(a, 3, 1, 7, 1.0, 0.2)
    assert m.tobytes() == augment.draw_mixup(a, 3, 1, 7, 1.0, 0.2).tobytes() and a['lambda'].max() == 1      # a copy: `a` is untouched
    for other in ((3, 1, 8), (3, 0, 7), (4, 1, 7)):
        assert m.tobytes() != augment.draw_mixup(a, *other, 1.0, 0.2).tobytes(), other
    big = augment.draw_mixup(augment.photo_identity_records(40), 3, 1, 7, 0.5, 0.2)
    small = augment.draw_mixup(augment.photo_identity_records(8), 3, 1, 7, 0.5, 0.2)
    assert np.array_equal(big['lambda'][:8], small['lambda']) and 0 < (small['lambda'] < 1).sum() < 8
    for f in ('m', 'bias', 'gamma', 'white'):
        assert np.array_equal(m[f], a[f])


def test_word_streams_differ_from_mosaic_and_affine_for_equal_seeds():
    """The first uniform of image 0 under (seed, shard, batch) = (5, 0, 2): the mosaic's, the affine's, the photometric and the
    MixUp stream give four different words, so equal seeds do not couple the four draws."""
    from yolo3 import augment
    key = 0
    for v in (5, 0, 2, 0):
        key = augment._mix64((key ^ v) + augment._GOLDEN)
    mosaic = augment._mix64(key + augment._GOLDEN)
    words = {mosaic, augment._stream(5, 0, 2, 0, augment._AFFINE_STREAM)(0), augment._stream(5, 0, 2, 0, augment._PHOTO_STREAM)(0),
             augment._stream(5, 0, 2, 0, augment._MIXUP_STREAM)(0)}
    assert len(words) == 4
    # _stream is draw_affine's construction: the affine's first uniform decides `warped` as its U_0 does
    u0 = (augment._stream(5, 0, 2, 0, augment._AFFINE_STREAM)(0) >> 11) * 2.0 ** -53
    assert (augment.draw_affine_parameters(5, 0, 2, 0, u0 + 1e-9, 10.0) is not None) and augment.draw_affine_parameters(5, 0, 2, 0, u0, 10.0) is None
    # and a photometric draw decides by its own word
    p0 = (augment._stream(5, 0, 2, 0, augment._PHOTO_STREAM)(0) >> 11) * 2.0 ** -53
    ident = augment.photo_identity_records(1).tobytes()
    assert augment.draw_photometric(5, 0, 2, 1, 3, p0, 0.1, 0.5, 0.5).tobytes() == ident
    assert augment.draw_photometric(5, 0, 2, 1, 3, p0 + 1e-9, 0.1, 0.5, 0.5).tobytes() != ident


def test_zero_magnitudes_prob_zero_and_one_channel():
    from yolo3 import augment
    ident = augment.photo_identity_records(6)
    assert augment.draw_photometric(1, 0, 0, 6, 3, 1.0).tobytes() == ident.tobytes()                       # every magnitude zero
    assert augment.draw_photometric(1, 0, 0, 6, 3, 0.0, 0.1, 0.7, 0.4, 1.0).tobytes() == ident.tobytes()   # nobody drawn
    assert augment.draw_photometric(1, 0, 0, 6, 1, 1.0, 0.1, 0.7).tobytes() == ident.tobytes()             # one channel ignores hue / saturation
    assert augment.draw_mixup(ident, 1, 0, 0, 0.0).tobytes() == ident.tobytes()
    one = augment.draw_photometric(1, 0, 0, 6, 1, 1.0, 0.1, 0.7, 0.4, 0.5, 65535.0)
    three = augment.draw_photometric(1, 0, 0, 6, 3, 1.0, 0.0, 0.0, 0.4, 0.5, 65535.0)
    assert np.array_equal(one['m'][:, 0], three['m'][:, 0]) and np.array_equal(one['gamma'], three['gamma'])      # the same words for value and gamma
    assert np.array_equal(one['m'][:, 1:], ident['m'][:, 1:]) and (one['white'] == 65535).all()
    # a pure value draw is value * I exactly
    assert np.array_equal(three['m'], three['m'][:, :1] * np.eye(3, dtype=np.float32).reshape(9))
    with pytest.raises(ValueError):
        augment.draw_photometric(0, 0, 0, 0, 3, 1.0)
    with pytest.raises(ValueError):
        augment.draw_photometric(0, 0, 0, 4, 2, 1.0)
    with pytest.raises(ValueError):
        augment.draw_photometric(0, 0, 0, 4, 3, 1.0, white=0.0)
    with pytest.raises(ValueError):
        augment.draw_mixup(ident, 0, 0, 0, 1.0, 0.6)


def test_draw_ranges_and_shares():
    from yolo3 import augment
    hue, sat, val, gam = 0.1, 0.6, 0.3, 1.5
    n = 4000
    rec = np.concatenate([augment.draw_photometric(11, 2, b, 8, 3, 0.3, hue, sat, val, gam) for b in range(n // 8)])
    changed = rec['white'] > 0
    assert abs(changed.mean() - 0.3) < 4 * np.sqrt(0.3 * 0.7 / n)                  # four standard deviations of the binomial share
    g = np.log2(rec['gamma'][changed].astype(np.float64))
    assert g.min() >= -gam - 1e-6 and g.max() <= gam + 1e-6 and g.min() < -0.9 * gam and g.max() > 0.9 * gam
    # value = the gain of grey, saturation = the gain of the chroma, hue = its angle: read back from the matrices
    m = rec['m'][changed].astype(np.float64).reshape(-1, 3, 3)
    v = (m @ np.ones(3))[:, 0]
    assert v.min() >= 1 - val - 1e-6 and v.max() <= 1 + val + 1e-6 and v.min() < 1 - 0.9 * val and v.max() > 1 + 0.9 * val
    yiq = augment._YIQ @ m @ augment._YIQ_INV
    s = np.hypot(yiq[:, 1, 1], yiq[:, 2, 1])
    a = np.arctan2(yiq[:, 2, 1], yiq[:, 1, 1]) / (2 * np.pi)
    assert s.min() >= 1 - sat - 1e-6 and s.max() <= 1 + sat + 1e-6 and s.min() < 1 - 0.9 * sat and s.max() > 1 + 0.9 * sat
    assert a.min() >= -hue - 1e-6 and a.max() <= hue + 1e-6 and a.min() < -0.9 * hue and a.max() > 0.9 * hue
    # the record is the float64 matrix of its parameters rounded once
    i = int(np.nonzero(changed)[0][0])
    want = augment.colour_matrix(a[0], s[0], v[0])
    assert np.abs(want - m[0]).max() < 1e-6 and rec['m'][i].dtype == np.float32
    # MixUp: share, partner never the image itself and uniform over the others, lambda in the window
    mix = np.concatenate([augment.draw_mixup(augment.photo_identity_records(4), 7, 0, b, 0.4, 0.15) for b in range(n // 4)])
    mixed = mix['lambda'] < 1
    assert abs(mixed.mean() - 0.4) < 4 * np.sqrt(0.4 * 0.6 / n)
    own = np.tile(np.arange(4), n // 4)
    assert (mix['partner'][mixed] != own[mixed]).all() and np.array_equal(mix['partner'][~mixed], own[~mixed])
    assert ((mix['partner'] >= 0) & (mix['partner'] < 4)).all()
    lam = mix['lambda'][mixed]
    assert lam.min() >= np.float32(0.35) and lam.max() <= np.float32(0.65) and lam.min() < 0.36 and lam.max() > 0.64
    for i in range(4):
        seen = np.bincount(mix['partner'][mixed & (own == i)], minlength=4)
        assert seen[i] == 0 and (seen[np.arange(4) != i] > 0.25 * seen.sum()).all(), (i, seen)
    assert (augment.draw_mixup(augment.photo_identity_records(1), 7, 0, 0, 1.0)['lambda'] == 1).all()      # n == 1 is never mixed
    two = augment.draw_mixup(augment.photo_identity_records(2), 7, 0, 0, 1.0)
    assert np.array_equal(two['partner'], [1, 0]) and (two['lambda'] < 1).all()


# ---- colour_matrix ---------------------------------------------------------------------------------------------------------
def test_colour_matrix_properties():
    from yolo3 import augment
    cm = augment.colour_matrix
    assert cm().dtype == np.float64 and np.array_equal(cm(), np.eye(3)) and np.array_equal(cm(0, 1, 0.75), 0.75 * np.eye(3))
    rng = np.random.default_rng(0)
    for _ in range(20):
        h, s, v = rng.uniform(-0.5, 0.5), rng.uniform(0, 2), rng.uniform(0.2, 2)
        m = cm(h, s, v)
        assert np.allclose(m @ np.ones(3), v * np.ones(3), rtol=0, atol=1e-12)                 # the grey axis maps to value * itself
        assert np.allclose(LUMA @ cm(h, s, 1.0), LUMA, rtol=0, atol=1e-12)                     # luma is preserved at value 1
        h2 = rng.uniform(-0.5, 0.5)
        assert np.allclose(cm(h) @ cm(h2), cm(h + h2), rtol=0, atol=1e-12)                     # M(a) M(b) = M(a + b)
        assert np.allclose(cm(h, s) @ cm(0, 0.5), cm(h, 0.5 * s), rtol=0, atol=1e-12)
        px = rng.uniform(0, 255, 3)
        assert np.allclose(cm(h, 0.0, 1.0) @ px, (LUMA @ px) * np.ones(3), rtol=0, atol=1e-10)     # saturation 0: the luma grey
    assert np.allclose(cm(1.0), np.eye(3), rtol=0, atol=1e-12) and np.allclose(cm(0.5) @ cm(0.5), np.eye(3), rtol=0, atol=1e-12)
    # a third of a turn is NOT a channel permutation: this operator turns the chroma plane of YIQ, not the RGB cube
    third = cm(1.0 / 3.0)
    for p in pr.PERMUTATIONS:
        assert np.abs(third - pr.permutation_matrix(p).reshape(3, 3)).max() > 0.2, p
    assert np.abs(third).min() > 0.01                                                          # no zero entry at all
    # continuous across what would be a hue sector boundary of a piecewise HSV round trip
    px = np.array([200.0, 200.0, 30.0])                                                        # r == g: on the boundary
    assert np.abs(cm(1e-7) @ px - cm(-1e-7) @ px).max() < 1e-3


# ---- mixup_boxes -----------------------------------------------------------------------------------------------------------
def test_mixup_boxes_union_order_empty_lists_and_aliasing():
    from yolo3 import augment
    a = np.array([[1, 2, 3, 4, 0], [5, 6, 7, 8, 1]], np.int32)
    b = np.array([[9, 9, 9, 9, 1]], np.int32)
    lists = [a, b, None, np.zeros((0, 5), np.int32)]
    rec = pr.records(4, partner=[1, 2, 0, 3], **{'lambda': [0.5, 0.25, 0.0, 1.0]})
    out = augment.mixup_boxes(lists, rec)
    assert all(o.dtype == np.int32 and o.ndim == 2 and o.shape[1] == 5 for o in out)
    assert np.array_equal(out[0], np.concatenate([a, b])) and np.array_equal(out[1], b) and np.array_equal(out[2], a) and out[3].shape == (0, 5)
    assert not any(np.shares_memory(o, x) for o in out for x in (a, b))
    out[0][:] = -1
    assert a[0, 0] == 1 and b[0, 0] == 9
    # lambda == 1: untouched whatever the partner field says; partner == itself doubles its list; n == 1
    rec = pr.records(2, partner=[1, 1], **{'lambda': [1.0, 0.5]})
    out = augment.mixup_boxes([a, b], rec)
    assert np.array_equal(out[0], a) and np.array_equal(out[1], np.concatenate([b, b])) and not np.shares_memory(out[0], a)
    one = augment.mixup_boxes([a], augment.draw_mixup(augment.photo_identity_records(1), 0, 0, 0, 1.0))
    assert len(one) == 1 and np.array_equal(one[0], a)
    with pytest.raises(AssertionError):
        augment.mixup_boxes([a, b], pr.records(3))


# ---- the restatement's own rules -------------------------------------------------------------------------------------------
def test_reference_rules_on_the_host():
    """What the GPU tests compare against, checked for the rules it must itself obey: copies keep their words, skipped terms do
    not leak, the clamp keeps NaN, the curve's ends are exact, the float64 mode agrees with the float32 mode to float32 accuracy,
    and a mixed image uses the partner's own record."""
    from yolo3 import augment
    rng = np.random.default_rng(3)
    words = pr.special_bits(rng, (7, 3, 5, 7))
    x = words.view(np.float32)
    recs = pr.records(7, m=np.stack([pr.permutation_matrix(p) for p in pr.PERMUTATIONS] + [pr.permutation_matrix((0, 1, 2))]))
    out = augment.photometric_reference(x, recs)
    assert out.dtype == np.float32
    for i, p in enumerate(pr.PERMUTATIONS):
        assert np.array_equal(out[i].view(np.uint32), words[i][list(p)])
    clamped = augment.photometric_reference(x, pr.records(7, white=10.0))
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(clamped), nan) and np.array_equal(clamped.view(np.uint32)[nan], words[nan])
    assert (clamped[~nan] >= 0).all() and (clamped[~nan] <= 10).all()
    # a zero coefficient hides its channel
    y = rng.uniform(0, 255, (1, 3, 4, 4)).astype(np.float32)
    y[0, 1] = np.nan
    r = pr.records(1, m=[[0.5, 0, 0.5, 0, 1, 0, 0.25, 0, 2]], bias=[[1, 0, 0]])
    o = augment.photometric_reference(y, r)
    assert np.isfinite(o[0, 0]).all() and np.isnan(o[0, 1]).all() and np.isfinite(o[0, 2]).all()
    assert np.array_equal(o[0, 0], (np.float32(0.5) * y[0, 0] + np.float32(0.5) * y[0, 2]) + np.float32(1))
    # the curve: ends exact, both modes close, gamma 1 a copy
    t = pr.tone_sweep(255.0)
    z = np.tile(t, (4, 1, 1, 1))
    r = pr.records(4, gamma=pr.TONE_GAMMAS, white=255.0)
    f32, f64 = augment.photometric_reference(z, r), augment.photometric_reference(z, r, np.float64)
    assert f64.dtype == np.float64 and (f32[z == 0] == 0).all() and (f64[z == 0] == 0).all() and (f32[z == 255] == 255).all() and (f64[z == 255] == 255).all()
    s = (t / np.float32(255)).astype(np.float64)
    assert np.array_equal(f64[2, 0, 0], 255.0 * np.where(s == 0, 0.0, s ** 1.25))
    assert (np.abs(f32 - f64) <= pr.tone_bound(f64, s, np.float64(r['gamma'])[:, None, None, None], 255.0, 64.0) + 1e-300).all()
    # MixUp under the partner's own record
    img = rng.uniform(0, 255, (2, 3, 4, 4)).astype(np.float32)
    r = pr.records(2, m=[pr.permutation_matrix((0, 1, 2)), pr.permutation_matrix((2, 0, 1)) * 0.5], partner=[1, 0], **{'lambda': [0.25, 1.0]})
    o, fin, _ = augment.photometric_reference(img, r, detail=True)
    assert np.array_equal(fin[1], np.float32(0.5) * img[1][[2, 0, 1]]) and np.array_equal(o[1], fin[1])
    assert np.array_equal(o[0], (np.float32(0.25) * img[0]) + (np.float32(0.75) * fin[1]))


# ---- Dataset.photometric / Dataset.mixup, train.py ---------------------------------------------------------------------------
def _make_lmdb(path, n=6, size=(64, 64, 3), dtype=np.uint8):
    import build_lmdb
    from yolo3 import lmdbio
    rng = np.random.default_rng(1)
    items = []
    for i in range(n):
        img = rng.integers(0, 256, size).astype(dtype)
        boxes = np.array([[4 + i, 6, 20, 24, i % 2]], np.int32)
        if dtype == np.uint8:
            items.append(build_lmdb.make_record(img, boxes, i, 'img%03d' % i))
        else:                                                  # (make_record stores uint8; the record format itself carries the dtype)
            from yolo3.isg_ai_pb import ImageYoloBoxesPair
            items.append((build_lmdb.record_key(boxes, i, 'img%03d' % i), ImageYoloBoxesPair.from_arrays(img, boxes).SerializeToString()))
    lmdbio.write_environment(path, items)


def test_dataset_argument_checks(tmp_path):
    from yolo3.imagereader import ImageReader
    path = str(tmp_path / 'train-syn.lmdb')
    _make_lmdb(path)
    rd = ImageReader(path, ANCHORS, num_workers=1, augmentation_device='gpu', label_device='gpu')
    base = rd.get_tf_dataset()
    assert base.photo_cfg is None and base.mixup_cfg is None and base.batch(2).prefetch(2).photo_cfg is None
    assert base.photometric(1).photo_cfg == (1.0, 0.015, 0.7, 0.4, 0.0, 0, 255.0) and base.mixup(1).mixup_cfg == (1.0, 0.1, 0)
    pcfg, mcfg = (0.5, 0.1, 0.5, 0.3, 1.0, 9, 200.0), (0.25, 0.3, 4)
    a = base.batch(2).photometric(0.5, hue=0.1, saturation=0.5, value=0.3, gamma=1, seed=9, white=200).mixup(0.25, 0.3, 4).prefetch(2)
    a = a.multiscale([(64, 64), (96, 96)], 1).mosaic(0.5, 3).affine(0.5)
    b = base.affine(0.5).mosaic(0.5, 3).multiscale([(64, 64), (96, 96)], 1).mixup(*mcfg).photometric(*pcfg[:5], pcfg[5], pcfg[6]).batch(2).shard(1, 0)
    assert a.photo_cfg == b.photo_cfg == pcfg and a.mixup_cfg == b.mixup_cfg == mcfg and a.mosaic_cfg == b.mosaic_cfg == (0.5, 3, 0.25)
    assert a.affine_cfg == b.affine_cfg and a.affine_cfg is not None and a.multiscale_cfg == b.multiscale_cfg and a.prefetch_depth == 2
    assert a.batch_size == b.batch_size == 2
    for bad in (0, -0.1, 1.5, True, float('nan')):
        with pytest.raises(ValueError, match='prob'):
            base.photometric(bad)
        with pytest.raises(ValueError, match='prob'):
            base.mixup(bad)
    for kw, what in ((dict(hue=-0.1), 'hue'), (dict(hue=0.6), 'hue'), (dict(saturation=1.5), 'saturation'), (dict(saturation=-1), 'saturation'),
                     (dict(value=2), 'value'), (dict(value=True), 'value'), (dict(gamma=-1), 'gamma'), (dict(gamma=5), 'gamma'),
                     (dict(gamma=float('nan')), 'gamma'), (dict(white=0), 'white'), (dict(white=-5), 'white'), (dict(white=float('inf')), 'white')):
        with pytest.raises(ValueError, match=what):
            base.photometric(0.5, **kw)
    for bad in (-0.1, 0.6, True, float('nan')):
        with pytest.raises(ValueError, match='spread'):
            base.mixup(0.5, bad)
    # photometric() needs the device augmentation only; mixup() the device labels too
    half = ImageReader(path, ANCHORS, num_workers=1, augmentation_device='gpu')
    assert half.get_tf_dataset().photometric(0.5).photo_cfg[6] == 255.0
    with pytest.raises(ValueError, match='label_device'):
        half.get_tf_dataset().mixup(0.5)
    plain = ImageReader(path, ANCHORS, num_workers=1)
    with pytest.raises(ValueError, match='augmentation_device'):
        plain.get_tf_dataset().photometric(0.5)
    with pytest.raises(ValueError, match='augmentation_device'):
        plain.get_tf_dataset().mixup(0.5)
    with pytest.raises(ValueError, match='batch'):
        next(iter(base.photometric(0.5)))
    with pytest.raises(ValueError, match='batch'):
        next(iter(base.mixup(0.5)))


@pytest.mark.parametrize('dtype,white', [(np.uint16, 65535.0), (np.float32, None)])
def test_default_white_follows_the_stored_dtype(tmp_path, dtype, white):
    from yolo3.imagereader import ImageReader
    path = str(tmp_path / 'train-syn.lmdb')
    _make_lmdb(path, 2, (32, 32, 3), dtype)
    ds = ImageReader(path, ANCHORS, num_workers=1, augmentation_device='gpu').get_tf_dataset()
    if white is None:
        with pytest.raises(ValueError, match='white'):
            ds.photometric(0.5)
        assert ds.photometric(0.5, white=1.0).photo_cfg[6] == 1.0
    else:
        assert ds.photometric(0.5).photo_cfg[6] == white


def _parse(extra):
    import train
    return train.build_parser().parse_args(['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c'] + extra)


def test_train_parser_and_train_model_flags(capsys):
    import train
    a = _parse([])
    assert (a.photo_prob, a.photo_hue, a.photo_saturation, a.photo_value, a.photo_gamma, a.photo_white, a.photo_seed) == (0.0, 0.015, 0.7, 0.4, 0.0, None, 0)
    assert (a.mixup_prob, a.mixup_spread, a.mixup_seed) == (0.0, 0.1, 0)
    a = _parse(['--augmentation_device', 'gpu', '--photo_prob', '0.5', '--photo_hue', '0.1', '--photo_saturation', '0.5', '--photo_value', '0.3',
                '--photo_gamma', '1', '--photo_white', '4095', '--photo_seed', '9', '--mixup_prob', '0.25', '--mixup_spread', '0.3', '--mixup_seed', '4',
                '--mosaic_prob', '0.5', '--affine_prob', '0.5', '--multiscale_min', '320', '--multiscale_max', '608'])
    assert (a.photo_prob, a.photo_hue, a.photo_saturation, a.photo_value, a.photo_gamma, a.photo_white, a.photo_seed, a.mixup_prob, a.mixup_spread,
            a.mixup_seed) == (0.5, 0.1, 0.5, 0.3, 1.0, 4095.0, 9, 0.25, 0.3, 4)
    for flag in ('--photo_prob', '--mixup_prob'):
        with pytest.raises(SystemExit):
            _parse([flag, '0.5'])
        assert flag + ' needs --augmentation_device gpu' in capsys.readouterr().err
    for bad in (['--photo_prob', '1.5'], ['--photo_prob', '-0.5'], ['--photo_hue', '0.6'], ['--photo_saturation', '2'], ['--photo_value', '-1'],
                ['--photo_gamma', '5'], ['--photo_white', '0'], ['--photo_white', 'inf'], ['--photo_white', 'nan'], ['--mixup_prob', '2'],
                ['--mixup_spread', '0.6'], ['--mixup_spread', '-0.1']):
        with pytest.raises(SystemExit):
            _parse(['--augmentation_device', 'gpu', '--photo_prob', '0.5', '--mixup_prob', '0.5'] + bad)
    assert train.check_photo_args(0) == 0.0 and train.check_photo_args(None) == 0.0 and train.check_photo_args(0.25, 0.5, 1, 1, 4, 1.0) == 0.25
    assert train.check_mixup_args(0) == 0.0 and train.check_mixup_args(None) == 0.0 and train.check_mixup_args(1, 0.5) == 1.0
    for args, what in (((2.0,), 'photo_prob'), ((0.5, -1), 'photo_hue'), ((0.5, 0.1, 1.5), 'photo_saturation'), ((0.5, 0.1, 0.5, 1.5), 'photo_value'),
                       ((0.5, 0.1, 0.5, 0.5, -1), 'photo_gamma'), ((0.5, 0.1, 0.5, 0.5, 0, float('nan')), 'photo_white')):
        with pytest.raises(ValueError, match=what):
            train.check_photo_args(*args)
    for args, what in (((2.0,), 'mixup_prob'), ((0.5, 0.75), 'mixup_spread')):
        with pytest.raises(ValueError, match=what):
            train.check_mixup_args(*args)
    for kw in (dict(photo_prob=0.5), dict(mixup_prob=0.5)):      # checked before a reader or the device is touched
        with pytest.raises(ValueError, match='augmentation_device'):
            train.train_model(2, 2, 'absent-a', 'absent-b', 'absent-c', 1, 1e-4, True, **kw)
    with pytest.raises(ValueError, match='photo_gamma'):
        train.train_model(2, 2, 'absent-a', 'absent-b', 'absent-c', 1, 1e-4, True, augmentation_device='gpu', photo_prob=0.5, photo_gamma=9)
    with pytest.raises(ValueError, match='mixup_spread'):
        train.train_model(2, 2, 'absent-a', 'absent-b', 'absent-c', 1, 1e-4, True, augmentation_device='gpu', mixup_prob=0.5, mixup_spread=1)


def test_default_dataset_never_calls_the_binding(tmp_path, monkeypatch):
    """_device_batch with a counting stand-in for every entry point of the library: without photometric() / mixup() the plain, the
    mosaic and the affine dataset make exactly the calls they made (the lists of tests/test_cpu_affine.py), y3_photometric_batch
    not among them; with either option it is called once, after the affine warp and right before the z-score, and with mixup()
    the labels are built from the union lists.  No GPU: the stand-ins return Y3_OK and the tensors stay on the CPU."""
    import torch
    from yolo3 import augment, imagereader, _hip
    calls, seen = [], {}

    class Counting:
        def __getattr__(self, name):
            real = getattr(_hip.lib, name)
            if name.endswith('_bytes'):
                return real

            def entry(*a):
                calls.append(name)
                seen[name] = a
                return 0
            return entry
    monkeypatch.setattr(imagereader, 'lib', Counting())
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev=None: type('S', (), {'cuda_stream': 0})())
    path = str(tmp_path / 'train-syn.lmdb')
    _make_lmdb(path)
    rd = imagereader.ImageReader(path, ANCHORS, use_augmentation=False, num_workers=1, augmentation_device='gpu', label_device='gpu')
    base = rd.get_tf_dataset().batch(4)
    imgs = torch.zeros((4, 64, 64, 3), dtype=torch.uint8)
    recs = np.concatenate([augment.identity_record((64, 64, 3), (64, 64)) for _ in range(4)])
    boxes, counts = imagereader.collate_boxes([np.array([[4, 6, 20, 24, 0]], np.int32)] * 4)
    plain = ['y3_format_labels', 'y3_augment_batch', 'y3_zscore']
    photo = ['y3_photometric_batch', 'y3_zscore']
    for ds, want in ((base, plain), (base.mosaic(1.0), plain[:2] + ['y3_mosaic_batch', 'y3_zscore']),
                     (base.multiscale([(64, 64), (96, 96)], 1), plain),
                     (base.affine(1.0), plain[:2] + ['y3_affine_batch', 'y3_zscore']),
                     (base.mosaic(1.0).affine(1.0, seed=4), plain[:2] + ['y3_mosaic_batch', 'y3_affine_batch', 'y3_zscore']),
                     (base.photometric(1.0), plain[:2] + photo), (base.mixup(1.0), plain[:2] + photo),
                     (base.photometric(0.5).mixup(0.5), plain[:2] + photo),
                     (base.mixup(1.0).mosaic(1.0).photometric(1.0).affine(1.0, seed=4).multiscale([(64, 64), (64, 96)], 1),
                      plain[:2] + ['y3_mosaic_batch', 'y3_affine_batch'] + photo)):
        del calls[:]
        out = ds._device_batch(torch.device('cpu'), imgs, recs, boxes.copy(), counts.copy())
        assert calls == want, (calls, want)
        assert len(out) == 4 and tuple(out[0].shape) == (4, 3) + ds.size_of_batch(0)
        if ds.mixup_cfg is not None and ds.mosaic_cfg is None:
            assert seen['y3_format_labels'][2:4] == (4, 2)          # n = 4 images, 2 boxes each: its own and its partner's


# ---- the library's refusals ------------------------------------------------------------------------------------------------
def test_library_refuses_bad_arguments_without_a_device():
    """The host-side validation of y3_photometric_batch needs no GPU: fake, disjoint addresses that nothing dereferences (every
    call here fails a check before the first launch)."""
    from yolo3 import augment
    from yolo3._hip import lib
    src, out = 1 << 20, 1 << 24
    n, c, h, w = 3, 3, 8, 12

    def call(recs, src=src, out=out, n=n, c=c, h=h, w=w):
        recs = None if recs is None else np.ascontiguousarray(recs, dtype=augment.PHOTO_RECORD)
        rc = lib.y3_photometric_batch(src, n, c, h, w, None if recs is None else recs.ctypes.data, out, None)
        return rc, lib.y3_last_error().decode()

    good = pr.records(3, white=255.0, partner=[1, 2, 0], **{'lambda': 0.5})
    for field, idxs in (('m', [(1, k) for k in range(9)]), ('bias', [(1, k) for k in range(3)]), ('gamma', [1]), ('white', [1]), ('lambda', [1])):
        for idx in idxs:
            for v in (np.nan, np.inf, -np.inf):
                r = good.copy()
                r[field][idx] = v
                rc, msg = call(r)
                assert rc == -1 and msg.startswith('photometric_batch: record 1') and 'non-finite' in msg, (field, idx, v, rc, msg)
    for field, idx, v, what in (('gamma', 0, 0.0, 'gamma 0'), ('gamma', 2, -1.5, 'gamma -1.5'), ('white', 2, -1.0, 'white -1'),
                                ('lambda', 0, -0.5, 'lambda -0.5'), ('lambda', 0, 1.25, 'lambda 1.25'), ('partner', 2, 3, 'partner image 3 of 3'),
                                ('partner', 2, -1, 'partner image -1 of 3')):
        r = good.copy()
        r[field][idx] = v
        rc, msg = call(r)
        assert rc == -1 and msg.startswith('photometric_batch: record %d' % idx) and what in msg, (field, v, rc, msg)
    r = good.copy()
    r['white'][0], r['gamma'][0] = 0.0, 0.5
    rc, msg = call(r)
    assert rc == -1 and 'record 0' in msg and 'needs white > 0' in msg, msg
    for kw, what in ((dict(recs=None), 'null'), (dict(src=0), 'null'), (dict(out=0), 'null'), (dict(c=2), 'channels 2'), (dict(c=4), 'channels 4'),
                     (dict(n=0), 'bad dims'), (dict(h=0), 'bad dims'), (dict(w=-3), 'bad dims'), (dict(h=1 << 16, w=1 << 15), 'too large'),
                     (dict(src=src + 2), 'aligned'), (dict(out=out + 1), 'aligned'), (dict(out=src), 'overlap'),
                     (dict(out=src + 4 * (n * c * h * w - 1)), 'overlap'), (dict(src=out + 4), 'overlap')):
        rc, msg = call(kw.pop('recs', good), **kw)
        assert rc == -1 and msg.startswith('photometric_batch:') and what in msg, (kw, rc, msg)
