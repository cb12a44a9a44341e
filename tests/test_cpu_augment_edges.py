"""tests/augment_edges.py held to what it claims, without a GPU: the fp64 restatement against the host augmentation
(yolo3/augment.py), the reference's goldens and an index-by-index blur; every case table against the property it is named
for; the bounds against 1e-3 on 0..255, against an fp32 evaluation of step 1, and against a wrong outermost tap."""
import os

import numpy as np
import pytest
import scipy.ndimage

import augment_edges as ae
from yolo3 import augment


def _ids(cases):
    return [c['id'] for c in cases]


def _host_crop(img, rec, crop):
    """float64 HWC crop of one record with the host path's helpers (augment.transform_image's arithmetic)"""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[:2]
    if (rec['rows'], rec['cols']) != (H, W):
        img = augment.rescale_bilinear(img, rec['rows'] / H, rec['cols'] / W)
        assert img.shape[:2] == (rec['rows'], rec['cols'])
    img = img[rec['dy']:rec['dy'] + crop[0], rec['dx']:rec['dx'] + crop[1]]
    if rec['reflect_x']:
        img = np.fliplr(img)
    if rec['reflect_y']:
        img = np.flipud(img)
    return img


def _scale(case):
    """the size of the case's values against 0..255"""
    return 257.0 if case['dtype'] == 'uint16' else 1.0


# ---- 1. the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('table', sorted(ae.TABLES))
def test_resample_is_the_host_path_arithmetic_on_every_case(table):
    """fp64 against fp64: the host path forms the coordinate (q + 0.5) n_in / n_res - 0.5 in floating point (a few 1e-14 px off the
    exact one), so 1e-9 of the range"""
    for case in ae.TABLES[table]:
        imgs = ae.case_images(case)
        for i, rec in enumerate(case['records']):
            got = ae.resample(imgs[i], rec, case['crop'])
            want = _host_crop(imgs[i], rec, case['crop'])
            assert got.shape == case['crop'] + (case['C'],)
            assert np.abs(got - want).max() <= 1e-9 * 255 * _scale(case), (case['id'], i)
            if case['flags'][i].get('exact_copy'):
                assert (rec['rows'], rec['cols']) == (case['h_in'], case['w_in'])
                assert np.array_equal(np.transpose(got, (2, 0, 1)), ae.exact_copy_bits(case, i).astype(np.float64)), (case['id'], i)


def test_resample_matches_the_reference_goldens(golden_dir):
    """tests/golden/augment.npz at the tolerances of the existing golden tests: 5e-3 on 0..255, identity scale 1e-6"""
    z = np.load(os.path.join(golden_dir, 'augment.npz'))
    img = z['img']
    for i, (c, crop) in enumerate(zip(z['affine_img_cases'], z['affine_img_crops'])):
        rx, ry, sx, sy = c
        dx, dy = z['affine_img_%d_dxdy' % i].tolist()
        same = sx == 1 and sy == 1
        rows = img.shape[0] if same else int(np.round(sy * img.shape[0]))
        cols = img.shape[1] if same else int(np.round(sx * img.shape[1]))
        got = ae.resample(img, ae.record(img.shape[0], img.shape[1], rows, cols, dy, dx, rx, ry), tuple(crop))
        assert np.abs(got - z['affine_img_%d' % i]).max() <= (1e-6 if same else 5e-3), i
    img2 = z['img2']
    dx, dy = z['affine_img2_dxdy'].tolist()
    got = ae.resample(img2, ae.record(70, 100, int(np.round(0.95 * 70)), int(np.round(1.2 * 100)), dy, dx, True, False), (60, 90))
    assert np.abs(got[..., 0] - z['affine_img2']).max() <= 5e-3


@pytest.mark.parametrize('shape', [(1, 1, 3), (1, 7, 3), (7, 1, 1), (3, 5, 3), (2, 2, 1), (8, 8, 3), (33, 9, 3)])
def test_blur_is_the_index_by_index_period_2n_reflection(shape):
    x = np.random.default_rng(shape[0] * 100 + shape[1]).uniform(0, 255, shape)
    for sigma in (0.1249, 0.125, 0.3749, 0.375, 1.0, 2.0, 2.124):
        got, want = ae.blur(x, sigma), ae.blur_indexwise(x, sigma)
        assert np.abs(got - want).max() <= 1e-12 * 255, (shape, sigma)
        if ae.radius_of(sigma) == 0:
            assert got is x or np.array_equal(got, x)
    assert np.abs(ae.blur(x, 1.0) - scipy.ndimage.gaussian_filter(x, float(np.float32(1.0)), mode='reflect')).max() == 0
    w = ae.gauss_weights(2.0)
    assert abs(w[0] + 2 * w[1:].sum() - 1) < 1e-15 and abs(w[8] - 6.7e-5) < 1e-6


def test_chain_is_noise_then_blur_of_the_resampled_crop_in_chw_order():
    case = [c for c in ae.SEAM_CASES if c['id'] == 'seam-5x257-c3'][0]
    i = 5                                                                   # sigma 2.0, noise + blur
    rec, img = case['records'][i], ae.case_images(case)[i]
    assert rec['noise_severity'] > 0 and ae.radius_of(rec['blur_sigma']) == 8
    want, (mn, mx) = ae.chain(img, rec, case['crop'])
    x = ae.resample(img, rec, case['crop'])
    assert (mn, mx) == (x.min(), x.max()) and np.abs(x - _host_crop(img, rec, case['crop'])).max() <= 1e-9 * 255
    s = float(np.float32(float(rec['noise_severity']) * (2 * float(rec['u_noise']) - 1))) * (mx - mn)
    z = ae.philox_normals(int(rec['seed']), x.size).reshape(3, 5, 257)       # element (ch * H + y) * W + x
    lit = scipy.ndimage.gaussian_filter(x + s * np.transpose(z, (1, 2, 0)), float(rec['blur_sigma']), mode='reflect')
    assert want.shape == (3, 5, 257) and np.abs(want - np.transpose(lit, (2, 0, 1))).max() <= 1e-9
    assert s != 0 and abs(ae.philox_normals(2 ** 63 + 12345, 4096).std() - 1) < 0.05
    assert not np.array_equal(ae.philox_normals(0, 64), ae.philox_normals(2 ** 32, 64))      # the high key word matters


# ---- 2. the tables ---------------------------------------------------------------------------------------------------
def _kinds(case):
    return [ae.case_full(case, i)['kind'] for i in range(len(case['records']))]


def test_every_record_is_one_the_library_accepts():
    for case in ae.ALL_CASES:
        H, W = case['crop']
        assert ae.stage_bytes(case['w_in'], case['C'], case['dtype']) <= ae.STAGE_BYTES, case['id']
        assert case['C'] in (1, 3) and case['dtype'] in ae.DTYPE_CODE
        for rec in case['records']:
            assert rec['dy'] >= 0 and rec['dx'] >= 0 and rec['dy'] + H <= rec['rows'] and rec['dx'] + W <= rec['cols'], case['id']
            assert 0 <= rec['u_noise'] <= 1 and rec['noise_severity'] >= 0 and ae.radius_of(rec['blur_sigma']) <= ae.MAX_RADIUS
        assert len(case['records']) * case['C'] * H * W <= 400_000, case['id']          # a few seconds per case at the most


def test_seam_cases_span_the_segments_they_claim():
    assert {c['crop'] for c in ae.SEAM_CASES} == {(5, 255), (5, 256), (5, 257), (5, 264), (3, 513), (33, 257)}
    assert {c['crop'][1] for c in ae.SEAM_CASES} >= {255, 256, 257, 264}
    assert sum(c['crop'][1] > ae.SEGMENT for c in ae.SEAM_CASES) >= 4 and any(c['crop'][1] > 2 * ae.SEGMENT for c in ae.SEAM_CASES)
    assert any(0 < c['crop'][1] - ae.SEGMENT < ae.MAX_RADIUS for c in ae.SEAM_CASES)       # segment 1 shorter than its halo
    assert any(c['crop'][0] > ae.COL_TILE[0] for c in ae.SEAM_CASES)
    for size in ae.SEAM_SIZES:
        assert {c['C'] for c in ae.SEAM_CASES if c['crop'] == size} == {1, 3}
    for case in ae.SEAM_CASES:
        assert case['dtype'] == 'uint8' and case['source'] == 'u255'
        kinds = _kinds(case)
        for kind in ('blur', 'noise+blur'):
            recs = [r for r, k in zip(case['records'], kinds) if k == kind]
            assert sorted(ae.radius_of(r['blur_sigma']) for r in recs) == [1, 4, 8, 8]
            assert {float(r['blur_sigma']) for r in recs} == {float(np.float32(s)) for s in ae.SIGMAS}
            assert {(int(r['reflect_x']), int(r['reflect_y'])) for r in recs} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_column_and_tiny_cases_sit_on_the_tile_edges_and_below_the_radius():
    th, tw = ae.COL_TILE
    assert {c['crop'] for c in ae.COLUMN_CASES} == {(H, W) for H in (31, 32, 33, 40, 65) for W in (63, 64, 65)}
    assert {c['crop'][0] for c in ae.COLUMN_CASES} >= {th - 1, th, th + 1, 2 * th + 1} and {c['crop'][1] for c in ae.COLUMN_CASES} == {tw - 1, tw, tw + 1}
    assert {c['C'] for c in ae.COLUMN_CASES} == {1, 3}
    assert {c['crop'] for c in ae.TINY_CASES} == {(1, 1), (1, 7), (7, 1), (3, 5), (2, 2), (8, 8)}
    for case in ae.COLUMN_CASES + ae.TINY_CASES:
        kinds = _kinds(case)
        assert kinds.count('blur') == 4 and kinds.count('noise+blur') == 4
        assert max(ae.radius_of(r['blur_sigma']) for r in case['records']) == 8
        assert float(np.float32(2.124)) in {float(r['blur_sigma']) for r in case['records']}
    for size in ae.TINY_SIZES:
        assert {c['C'] for c in ae.TINY_CASES if c['crop'] == size} == {1, 3}
    assert all(min(c['crop']) <= ae.MAX_RADIUS for c in ae.TINY_CASES) and any(4 * max(c['crop']) <= ae.MAX_RADIUS for c in ae.TINY_CASES)


def test_source_cases_are_tiny_unaligned_and_far_outside_the_training_scales():
    by_id = {c['id']: c for c in ae.SOURCE_CASES}

    def row_bytes(c):
        return c['w_in'] * c['C'] * np.dtype(c['dtype']).itemsize

    assert all(row_bytes(by_id[i]) % 4 != 0 for i in ae.UNALIGNED_IDS)
    assert {row_bytes(by_id[i]) for i in ae.UNALIGNED_IDS} >= {273, 37, 30, 66}
    assert row_bytes(by_id[ae.ALIGNED_CONTROL_ID]) == 276
    assert by_id[ae.ALIGNED_CONTROL_ID]['crop'] == by_id['source-rows13x91-uint8-c3']['crop']
    tiny = [c for c in ae.SOURCE_CASES if 'tiny' in c['id']]
    assert {(c['h_in'], c['w_in']) for c in tiny} == {(1, 1), (1, 9), (9, 1), (2, 2), (2, 3)}
    for c in tiny:
        H, W = c['crop']
        offs = {(int(r['dy']), int(r['dx'])) for r in c['records']}
        assert all(r['rows'] >= 4 * c['h_in'] and r['cols'] >= 4 * c['w_in'] for r in c['records'])
        assert (0, 0) in offs and (int(c['records'][0]['rows']) - H, int(c['records'][0]['cols']) - W) in offs
    assert any(r['rows'] == 80 and r['cols'] == 112 for r in by_id['source-up2-float32-c3']['records'])
    assert any(r['rows'] == int(np.round(0.3 * 40)) and r['cols'] == int(np.round(0.3 * 56)) for r in by_id['source-down0.3-float32-c1']['records'])
    # each dtype with each C, with and without a rescale
    seen = set()
    for c in ae.SOURCE_CASES:
        for r in c['records']:
            seen.add((c['dtype'], c['C'], (r['rows'], r['cols']) == (c['h_in'], c['w_in'])))
    assert {(d, C, e) for d in ae.DTYPE_CODE for C in (1, 3) for e in (False, True)} <= seen


def test_wide_case_is_exactly_at_the_stage_limit():
    c = ae.WIDE_CASE
    assert (c['dtype'], c['C'], c['h_in'], c['w_in'], c['crop']) == ('float32', 3, 3, 2560, (3, 300))
    assert c['w_in'] * 3 * 4 == 30720 and ae.stage_bytes(c['w_in'], 3, 'float32') == ae.STAGE_BYTES
    assert ae.stage_bytes(ae.WIDE_REFUSED_W, 3, 'float32') > ae.STAGE_BYTES and ae.WIDE_REFUSED_W == c['w_in'] + 1
    a, b = c['records']
    assert a['cols'] == 2560 and a['rows'] == 3 and c['flags'][0].get('exact_copy') and b['cols'] == 2600
    assert a['dx'] + 300 == a['cols'] and b['dx'] + 300 == b['cols']                      # the far end of the staged rows


def test_signed_and_noise_cases_hold_the_values_and_the_records_they_claim():
    by_src = {c['source']: c for c in ae.SIGNED_CASES}
    assert set(by_src) == {'signed', 'negative', 'const+', 'const-'}
    sg, ng = ae.case_images(by_src['signed'])[0], ae.case_images(by_src['negative'])[0]
    assert sg.dtype == np.float32 and (sg < 0).any() and (sg > 0).any() and abs(sg.std() - 50) < 5
    assert ng.max() <= -1 and ng.min() >= -200 and ng.min() < -150
    assert np.unique(ae.case_images(by_src['const+'])).tolist() == [37.5] and np.unique(ae.case_images(by_src['const-'])).tolist() == [-37.5]
    for c in ae.SIGNED_CASES:
        noisy = [r for r in c['records'] if r['noise_severity'] == np.float32(0.03)]
        assert {float(r['u_noise']) for r in noisy} == {0.0, 0.25, 1.0} and len(noisy) == 6
        if c['source'].startswith('const'):
            same = [i for i, f in enumerate(c['flags']) if f.get('same_bits_as') is not None]
            assert len(same) == 3 and all(ae.case_full(c, i)['s'] == 0 and c['records'][i]['noise_severity'] > 0 for i in same)
    assert {(c['dtype'], c['C']) for c in ae.NOISE_CASES} == {('uint8', 1), ('uint16', 3), ('float32', 1), ('float32', 3)}
    for c in ae.NOISE_CASES:
        assert c['crop'] == (24, 40)
        noisy = [(r, f) for r, f in zip(c['records'], c['flags']) if r['noise_severity'] > 0]
        combos = {(int(r['reflect_x']), int(r['reflect_y']), round(float(r['u_noise']), 3)) for r, _ in noisy}
        assert combos == {(x, y, u) for x in (0, 1) for y in (0, 1) for u in (0.0, 0.3, 0.5, 1.0)}
        assert {int(r['seed']) for r, _ in noisy} == set(ae.SEEDS) and ae.SEEDS[:3] == (0, 2 ** 32, 2 ** 63 + 12345)
        for r, f in noisy:
            p = c['records'][f['plain']]
            assert p['noise_severity'] == 0 and all(p[k] == r[k] for k in ('rows', 'cols', 'dy', 'dx', 'reflect_x', 'reflect_y'))
            assert (f['same_bits_as'] == f['plain']) == (r['u_noise'] == 0.5) and (ae.noise_factor(r) == 0) == (r['u_noise'] == 0.5)


def test_radius_cases_give_the_radii_claimed():
    assert [ae.radius_of(s) for s in (0.1249, 0.125, 0.3749, 0.375, 2.124, 2.125)] == [0, 1, 1, 2, 8, 9]
    assert tuple(ae.radius_of(s) for s in ae.RADIUS_SIGMAS) == ae.RADIUS_EXPECTED and len(ae.RADIUS_SIGMAS) == 17
    assert set(ae.RADIUS_EXPECTED) == set(range(9)) and ae.radius_of(ae.RADIUS_REFUSED_SIGMA) == ae.MAX_RADIUS + 1
    assert {c['C'] for c in ae.RADIUS_CASES} == {1, 3}
    for c in ae.RADIUS_CASES:
        assert [ae.radius_of(r['blur_sigma']) for r in c['records'][1:]] == list(ae.RADIUS_EXPECTED)
        assert [f.get('same_bits_as') for f in c['flags'][1:]] == [0] + [None] * 16 and ae.case_full(c, 1)['kind'] == 'resample'


def test_mixed_batch_orderings_have_the_chunk_composition_claimed():
    assert len(ae.MIXED_BATCH) == 3
    comp = {}
    for c in ae.MIXED_BATCH:
        assert len(c['records']) == 40 > ae.CHUNK and c['crop'] == (24, 40) and not c['shared']
        kinds = _kinds(c)
        want = {'neither': 'resample', 'noise': 'noise', 'blur': 'blur', 'both': 'noise+blur'}
        assert kinds == [want[f['kind']] for f in c['flags']]
        comp[c['id']] = (set(kinds[:ae.CHUNK]), set(kinds[ae.CHUNK:]))
        assert len({(int(r['rows']), int(r['cols'])) for r in c['records']}) == 40                 # a rescaled size of its own per image
        imgs = ae.case_images(c)
        assert not np.array_equal(imgs[0], imgs[ae.CHUNK])
        mm = [(ae.case_full(c, i)['mn'], ae.case_full(c, i)['mx']) for i in (0, ae.CHUNK, ae.CHUNK + 1)]
        assert len(set(mm)) == 3 or mm[0][1] - mm[0][0] != mm[1][1] - mm[1][0]
    every = {'resample', 'noise', 'blur', 'noise+blur'}
    assert comp['mixed-chunk1-mixed'] == ({'resample'}, every) and comp['mixed-chunk0-mixed'] == (every, {'resample'})
    assert comp['mixed-interleaved'] == (every, every)
    inter = _kinds(ae.MIXED_BATCH[2])
    assert all(inter[i] != inter[i + 1] for i in range(39))


# ---- 3. the bounds ---------------------------------------------------------------------------------------------------
def _resample_fp32(img, rec, crop):
    """step 1 as the header states it for the device: exact integer floor, fp32 fraction of the remainder, fp32 lerps"""
    img = np.asarray(img, np.float32)
    f32 = np.float32

    def axis(n_in, n_res, start, count):
        q = np.arange(start, start + count, dtype=np.int64)
        num, den = (2 * q + 1) * n_in - n_res, 2 * n_res
        i0 = num // den
        f = (num - i0 * den).astype(f32) / f32(den)
        return ae.mirror(i0, n_in), ae.mirror(i0 + 1, n_in), f

    def lerp(a, b, f):
        return np.where(f == 0, a, (f32(1) - f) * a + f * b).astype(f32)

    H, W = crop
    ya, yb, fy = axis(img.shape[0], int(rec['rows']), int(rec['dy']), H)
    xa, xb, fx = axis(img.shape[1], int(rec['cols']), int(rec['dx']), W)
    fxb, fyb = fx[None, :, None], fy[:, None, None]
    v = lerp(lerp(img[ya][:, xa], img[ya][:, xb], fxb), lerp(img[yb][:, xa], img[yb][:, xb], fxb), fyb)
    v = v[:, ::-1] if rec['reflect_x'] else v
    return v[::-1] if rec['reflect_y'] else v


@pytest.mark.parametrize('table', sorted(ae.TABLES))
def test_bounds_hold_for_an_fp32_evaluation_and_stay_below_1e_3_on_0_255(table):
    """Worst fp32-restated step 1 error / bound per table: 0.25 - 0.64 (three roundings allowed per lerp term, the restatement makes
    them with mixed signs); the kernel on an MI355X gave the same figures.  Every bound without the noise term, and every noise + blur bound on uint8 sources, is <= 1e-3 on
    0..255 -- what tests/test_gpu_augment.py allows for resample and for blur."""
    worst = 0.0
    for case in ae.TABLES[table]:
        imgs = ae.case_images(case)
        for i, rec in enumerate(case['records']):
            full = ae.case_full(case, i)
            got = np.transpose(_resample_fp32(imgs[i], rec, case['crop']), (2, 0, 1))
            r, where = ae.worst_ratio(got, full['base'], full['base_bound'])
            worst = max(worst, r)
            assert r <= 1.0, (case['id'], i, r, where)
            assert np.isfinite(full['bound']).all() and (full['bound'] >= full['base_bound'] * (full['radius'] == 0)).all()
            if case['source'] == 'u255' and (full['kind'] in ('resample', 'blur') or (full['kind'] == 'noise+blur' and case['dtype'] == 'uint8')):
                assert full['bound'].max() <= 1e-3 * _scale(case), (case['id'], i, full['kind'], full['bound'].max())
                assert full['mx_iv'][1] - full['mx_iv'][0] <= 1e-3 * _scale(case) and full['mn_iv'][1] - full['mn_iv'][0] <= 1e-3 * _scale(case)
            if full['kind'] == 'noise+blur' and case['dtype'] == 'uint8':
                assert abs(full['s']) <= 0.13
    print('\n%s: worst fp32-restated resample error / bound %.3f' % (table, worst))


def _chain_fp32(img, rec, crop, z):
    """steps 1-3 in fp32 in the order the header's passes give: noise, blur along W, channel mix, blur along H (HWC in, CHW out)"""
    f32 = np.float32
    x = _resample_fp32(img, rec, crop)
    nf = f32(ae.noise_factor(rec))
    if nf != 0:
        x = (x + (nf * (x.max() + -x.min())) * np.transpose(z, (1, 2, 0)).astype(f32)).astype(f32)
    R = ae.radius_of(rec['blur_sigma'])
    if R > 0:
        w64 = ae.gauss_weights(rec['blur_sigma'])
        w = w64.astype(f32)

        def axis_blur(v, axis):
            i = np.arange(v.shape[axis])
            acc = w[0] * v
            for k in range(1, R + 1):
                acc = acc + w[k] * (np.take(v, ae.reflect(i - k, len(i)), axis=axis) + np.take(v, ae.reflect(i + k, len(i)), axis=axis))
            return acc.astype(f32)

        x = axis_blur(x, 1)
        C = x.shape[2]
        if C > 1:
            mix = np.zeros((C, C))
            for co in range(C):
                for k in range(-R, R + 1):
                    mix[co, int(ae.reflect(co + k, C))] += w64[abs(k)]
            mix = mix.astype(f32)
            v = np.zeros_like(x)
            for ci in range(C):
                v = v + mix[None, None, :, ci] * x[:, :, ci:ci + 1]
            x = v.astype(f32)
        x = axis_blur(x, 0)
    return np.transpose(x, (2, 0, 1))


@pytest.mark.parametrize('table', ['seam', 'column', 'tiny', 'signed', 'radius', 'mixed'])
def test_bounds_hold_for_an_fp32_evaluation_of_noise_and_blur(table):
    """The passes restated in fp32 NumPy with the fp64 twin's normals rounded to fp32 (so without the NORMAL_TOL the bound grants the
    device's logf / cosf).  Worst error / bound per table: blur 0.14 - 0.29, noise + blur 0.07 - 0.17, noise 0.005 - 0.22; the kernels on
    an MI355X gave the same figures to three digits (profiles/augment_edges_err.txt)."""
    worst = {}
    for case in ae.TABLES[table]:
        imgs = ae.case_images(case)
        for i, rec in enumerate(case['records']):
            full = ae.case_full(case, i)
            if full['kind'] == 'resample':
                continue
            r, where = ae.worst_ratio(_chain_fp32(imgs[i], rec, case['crop'], full['z']), full['want'], full['bound'])
            worst[full['kind']] = max(worst.get(full['kind'], 0.0), r)
            assert r <= 1.0, (case['id'], i, full['kind'], r, where)
    print('\n%s: worst fp32-restated error / bound %s' % (table, {k: round(v, 3) for k, v in worst.items()}))


@pytest.mark.parametrize('table', sorted(ae.TABLES))
def test_a_wrong_outermost_tap_stays_above_the_bound_of_every_noise_and_blur_record(table):
    n, lowest = 0, np.inf
    for case in ae.TABLES[table]:
        for i, rec in enumerate(case['records']):
            full = ae.case_full(case, i)
            if full['kind'] != 'noise+blur':
                continue
            d = ae.discrimination(full, rec)
            if d is None:
                assert case['crop'] == (1, 1) and case['C'] == 1
                continue
            n += 1
            lowest = min(lowest, d)
            assert d > 1.0, (case['id'], i, float(rec['blur_sigma']), d)
    print('\n%s: %d noise + blur records, lowest wrong-tap change / bound %.3g' % (table, n, lowest))
    assert n > 0 or table in ('source', 'wide', 'noise', 'radius')


def test_a_wrong_kernel_would_leave_the_bounds():
    """single slips in the fp64 restatement -- never an address -- leave the bound of the case that is there for them"""
    # the halo of segment 1 starts one column late
    case = ae.CASES_BY_ID['seam-5x257-c1']
    i = 4                                                                   # sigma 2.0, blur alone
    full, rec = ae.case_full(case, i), case['records'][i]
    x = np.transpose(full['base'], (1, 2, 0))
    padded = x[:, ae.reflect(np.arange(-8, 257 + 8), 257)]
    padded[:, 256:264] = padded[:, 257:265]                                 # what segment 1 sees as its left halo
    w = ae.gauss_weights(rec['blur_sigma'])
    row = sum(w[abs(k)] * padded[:, 8 + k:8 + k + 257] for k in range(-8, 9))
    good = sum(w[abs(k)] * x[:, ae.reflect(np.arange(257) + k, 257)] for k in range(-8, 9))
    bad = np.where(np.arange(257)[None, :, None] >= 256, row, good)
    out = scipy.ndimage.gaussian_filter1d(bad, float(rec['blur_sigma']), axis=0, mode='reflect')
    assert ae.worst_ratio(np.transpose(out, (2, 0, 1)), full['want'], full['bound'])[0] > 1
    # the column pass reflecting with period 2 (n - 1)
    case = ae.CASES_BY_ID['tiny-3x5-c1']
    full, rec = ae.case_full(case, 2), case['records'][2]                   # sigma 1.0, blur alone
    x = np.transpose(full['base'], (1, 2, 0))
    rowpass = scipy.ndimage.gaussian_filter1d(x, float(rec['blur_sigma']), axis=1, mode='reflect')
    bad = scipy.ndimage.gaussian_filter1d(rowpass, float(rec['blur_sigma']), axis=0, mode='mirror')
    assert ae.worst_ratio(np.transpose(bad, (2, 0, 1)), full['want'], full['bound'])[0] > 1e3
    # the noise index without the channel term
    case = ae.NOISE_CASES[1]
    i = [k for k, r in enumerate(case['records']) if r['noise_severity'] > 0 and r['u_noise'] == 1.0][0]
    full = ae.case_full(case, i)
    z_bad = np.broadcast_to(full['z'][:1], full['z'].shape)
    assert ae.worst_ratio(full['base'] + full['s'] * z_bad, full['want'], full['bound'])[0] > 1e2
