"""GPU tests of the opt-in colour / tone jitter and MixUp pass: y3_photometric_batch through the C ABI on buffers the
test owns -- `out` pre-filled with NaN between two 256-byte canaries, `src` unchanged --, bit for bit against
augment.photometric_reference(float32) for every record without a tone curve, the tone curve against the float64 mode within the
bound of tests/photometric_reference.py, every refusal, then the data plane end to end and train.py.

Which path of csrc/augment.hip a shape reaches (P = h * w elements per plane, 256 threads per workgroup):
  1 x 1, 5 x 7, 33 x 67   P no multiple of 4: photometric_kernel<C, 1>, one pixel per thread; 33 x 67 = 2211 pixels is 9 workgroups,
                          the last one partial
  8 x 12                  P = 96: photometric_kernel<C, 4>, 24 groups of four pixels in one workgroup.  `out` 16-byte aligned: every
                          group whole (16-byte loads and stores); `out` shifted by 4 bytes: 25 groups per plane, the first and the
                          last partial (float by float), the others whole at a source alignment of 4 or 8 bytes; `src` shifted
                          alone: whole groups, 16-byte loads at 4-byte alignment
  33 x 68                 P = 2244 = 4 * 561: three workgroups, the last one partial
  96 x 128                P = 12288: 12 full workgroups per image (the non-square case of the data plane's sizes)
  n = 1, 2, 3, 17         17 = Y3_PHO_CHUNK + 1: two launches, the second with one image whose partner lies in the first chunk

Y3_PHOTO_ERR=<file> writes the worst |error| / bound of every tone-curve case of the run to <file>, with the bound's constant set
to one, i.e. the measured figure behind TONE_K (profiles/photometric_err.txt is such a run)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import photometric_reference as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
ANCHORS = [(64, 384), (384, 64)]
SHAPES = [(1, 1), (5, 7), (33, 67), (8, 12), (33, 68)]


@pytest.fixture(scope='module', autouse=True)
def report():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    yield
    path = os.environ.get('Y3_PHOTO_ERR')
    if path:
        with open(path, 'w') as f:
            f.write('# worst |error| / ((1 + gamma |log2 s|) 2^-24 |y| + floor) per tone-curve case, i.e. the bound of\n'
                    '# tests/photometric_reference.py with its constant set to 1, and the element that gave it (tests/test_gpu_photometric.py).\n'
                    '# TONE_K = 4 x the worst of the sweep cases.\n')
            for cid, (r, where) in sorted(pr.RATIOS.items()):
                f.write('%-44s %.3f  %s\n' % (cid, r, where))
            if pr.RATIOS:
                f.write('%-44s %.3f\n' % ('all', max(v[0] for v in pr.RATIOS.values())))


def _call(words, recs, expect_rc=0, src_shift=0, out_shift=0):
    """One y3_photometric_batch call: words uint32 [n, c, h, w] (the source bits) at `src_shift` floats past a 16-byte boundary,
    `out` at `out_shift` floats past one, pre-filled with NaN between two 256-byte canaries of 0xA5 -> the output words.  The
    canaries must survive and `src` must come back unchanged."""
    from yolo3._hip import lib
    n, c, h, w = words.shape
    total = words.size
    sbuf = torch.zeros(total + 4, dtype=torch.int32, device='cuda')
    src = sbuf[src_shift:src_shift + total]
    src.copy_(torch.from_numpy(np.ascontiguousarray(words).reshape(-1).view(np.int32)))
    lead = pr.CANARY_BYTES + 4 * out_shift
    buf = torch.full((lead + 4 * total + pr.CANARY_BYTES,), 0xA5, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    body = buf[lead:lead + 4 * total]
    nan_word = 0x7fc00000
    body.copy_(torch.from_numpy(np.full(total, nan_word, np.uint32).view(np.uint8)))
    recs = np.ascontiguousarray(recs)
    assert recs.shape == (n,) and recs.dtype.itemsize == 64
    rc = lib.y3_photometric_batch(src.data_ptr(), n, c, h, w, recs.ctypes.data, body.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.y3_last_error())
    assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + 4 * total:] == 0xA5).all()), 'wrote outside out'
    assert np.array_equal(src.cpu().numpy().view(np.uint32).reshape(words.shape), words), 'src was written'
    out = body.cpu().numpy().view(np.uint32).reshape(words.shape)
    if rc != 0:
        assert (out == nan_word).all(), 'a refused call wrote'
    return out


def _check_exact(words, recs, what, **shifts):
    """The device against photometric_reference(float32), word for word (a NaN out of arithmetic: a NaN)."""
    from yolo3 import augment
    assert (recs['gamma'] == 1).all()
    want = augment.photometric_reference(words.view(np.float32), recs).view(np.uint32)
    got = _call(words, recs, **shifts)
    ok = pr.same_words(got, want)
    assert ok.all(), '%s: %d words differ, first at %r' % (what, int((~ok).sum()), tuple(int(v[0]) for v in np.nonzero(~ok)))
    return got


def _finite(rng, shape, scale=60.0, shift=100.0):
    return (rng.standard_normal(shape) * scale + shift).astype(np.float32).view(np.uint32)


# ---- exact stages ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('size', SHAPES)
def test_identity_and_permutations_copy_the_bits(size, c):
    """The identity and (c = 3) the six channel permutations, one record per image of one call, on sources seeded with NaN
    payloads, -0.0, the infinities and denormals: the output is the permuted source, word for word."""
    h, w = size
    perms = pr.PERMUTATIONS if c == 3 else [(0, 1, 2)]
    n = len(perms) + 1
    words = pr.special_bits(np.random.default_rng(100 * h + w + c), (n, c, h, w))
    recs = pr.records(n, m=np.stack([pr.permutation_matrix(p) for p in perms] + [pr.permutation_matrix((0, 1, 2))]))
    got = _call(words, recs)
    for i, p in enumerate(perms):
        assert np.array_equal(got[i], words[i][list(p[:c])]), (size, c, p)
    assert np.array_equal(got[n - 1], words[n - 1])
    from yolo3 import augment
    assert np.array_equal(augment.photometric_reference(words.view(np.float32), recs).view(np.uint32), got)


def test_unused_channel_never_leaks():
    """Inf and NaN fill one channel; rows that do not use it stay finite and equal the restatement, the row that uses it is NaN /
    Inf.  A clamp is on for half of the images."""
    n, c, h, w = 6, 3, 8, 12
    rng = np.random.default_rng(7)
    words = _finite(rng, (n, c, h, w))
    m = np.zeros((n, 9), np.float32)
    for i in range(n):
        bad = i % 3
        words[i, bad] = np.where(rng.random((h, w)) < 0.5, np.uint32(0x7f800000), np.uint32(0x7fc00055))
        for k in range(3):
            if k == bad:
                m[i, 3 * k:3 * k + 3] = (0.5, 0.25, 2.0)
            else:
                m[i, 3 * k:3 * k + 3] = [0 if j == bad else 0.75 - 0.5 * j for j in range(3)]
    recs = pr.records(n, m=m, bias=np.tile(np.float32([0, 3.5, -2]), (n, 1)), white=[0, 255] * 3)
    got = _check_exact(words, recs, 'unused channel').view(np.float32)
    for i in range(n):
        for k in range(3):
            assert np.isfinite(got[i, k]).all() == (k != i % 3), (i, k)


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('size', SHAPES + [(96, 128)])
def test_random_matrices_bias_and_clamp_match_the_restatement(size, c):
    """Random matrices with bias (some coefficients exactly 0 and exactly 1, some bias 0), without and with the clamp -- data on
    both sides of [0, white], NaN, -0.0 and Inf among it: NaN stays NaN through the clamp, Inf becomes white."""
    h, w = size
    n = 2 if size == (96, 128) else 5
    rng = np.random.default_rng(h * 1000 + w + c)
    words = _finite(rng, (n, c, h, w), 120.0, 100.0)
    flat = words.reshape(-1)
    idx = rng.integers(0, flat.size, max(1, flat.size // 16))
    flat[idx] = pr.SPECIAL[rng.integers(0, len(pr.SPECIAL), len(idx))]
    m = rng.uniform(-1.5, 1.5, (n, 9)).astype(np.float32)
    m[rng.random((n, 9)) < 0.25] = 0
    m[rng.random((n, 9)) < 0.15] = 1
    bias = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
    bias[rng.random((n, 3)) < 0.4] = 0
    for white in (0.0, 255.0):
        recs = pr.records(n, m=m, bias=bias, white=white)
        got = _check_exact(words, recs, 'matrix %dx%d c=%d white=%g' % (h, w, c, white)).view(np.float32)
        if white:
            fin = ~np.isnan(got)
            assert (got[fin] >= 0).all() and (got[fin] <= white).all()
            assert got.size < 200 or ((got[fin] == 0).any() and (got[fin] == white).any())      # the clamp acted on both sides
    # NaN stays NaN through the clamp: the identity with the clamp on keeps every NaN of the source a NaN, clamps the rest
    ident = pr.records(n, white=255.0)
    got = _check_exact(words, ident, 'clamp only')
    src_nan = np.isnan(words.view(np.float32))
    assert src_nan.any() or words.size < 200
    assert np.array_equal(np.isnan(got.view(np.float32)), src_nan) and np.array_equal(got[src_nan], words[src_nan])


@pytest.mark.parametrize('shifts', [(0, 0), (1, 0), (0, 1), (1, 1), (3, 2)])
@pytest.mark.parametrize('c', [1, 3])
def test_shifted_views_give_the_same_words(shifts, c):
    """8 x 12 (a width that is a multiple of 4) with `src` / `out` on a 16-byte boundary and 4, 8 or 12 bytes past one: the vector
    path with whole groups, and the partial first / last group of every plane; the same words either way, between the canaries."""
    n, h, w = 3, 8, 12
    rng = np.random.default_rng(11 + c)
    words = _finite(rng, (n, c, h, w))
    m = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    recs = pr.records(n, m=m, bias=np.float32([[1, 0, -1]] * n), white=255.0, partner=[1, 2, 2], **{'lambda': [0.25, 1.0, 0.75]})
    base = _check_exact(words, recs, 'aligned')
    got = _check_exact(words, recs, 'shifted %r' % (shifts,), src_shift=shifts[0], out_shift=shifts[1])
    assert np.array_equal(got, base)


# ---- MixUp -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('size', [(5, 7), (33, 68)])
def test_mixup_blends_two_finished_images(size, c):
    """lambda in {0, 0.5, 1, one drawn value}, partner == i, mutual partners, a partner with another record (matrix, bias, clamp):
    word for word; the blend takes the PARTNER's record for the partner (checked against a blend by hand)."""
    from yolo3 import augment
    h, w = size
    n = 6
    rng = np.random.default_rng(h + w + c)
    words = _finite(rng, (n, c, h, w))
    m = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    m[0] = pr.permutation_matrix((0, 1, 2))
    drawn = augment.draw_mixup(augment.photo_identity_records(8), 3, 0, 0, 1.0, 0.3)['lambda'][5]
    assert 0.2 <= drawn <= 0.8 and drawn != 0.5
    recs = pr.records(n, m=m, bias=rng.uniform(-5, 5, (n, 3)).astype(np.float32), white=[0, 255, 200, 0, 255, 255],
                      partner=[1, 0, 2, 5, 0, 3], **{'lambda': [0.5, 0.0, drawn, 1.0, drawn, 0.5]})
    got = _check_exact(words, recs, 'mixup %dx%d c=%d' % (h, w, c)).view(np.float32)
    alone = recs.copy()
    alone['lambda'] = 1
    fin = _check_exact(words, alone, 'finished').view(np.float32)
    for i in range(n):
        lam, p = np.float32(recs['lambda'][i]), int(recs['partner'][i])
        want = fin[i] if lam == 1 else (lam * fin[i]) + ((np.float32(1) - lam) * fin[p])
        assert np.array_equal(got[i], want), i
    assert np.array_equal(got[1].view(np.uint32), ((np.float32(0) * fin[1]) + fin[0]).view(np.uint32))     # lambda 0: 0 * a + 1 * b


def test_nan_reaches_exactly_the_outputs_that_read_its_image():
    """Image 2 is all NaN: it is read by output 2 (its own) and by the outputs whose lambda < 1 names it as partner; an output
    with lambda == 1 ignores its partner field.  Every other output is finite."""
    n, c, h, w = 5, 3, 8, 12
    words = _finite(np.random.default_rng(2), (n, c, h, w))
    words[2] = 0x7fc00000
    recs = pr.records(n, white=255.0, partner=[2, 2, 0, 4, 2], **{'lambda': [0.5, 1.0, 1.0, 0.5, 0.0]})
    got = _check_exact(words, recs, 'nan image').view(np.float32)
    reads = [True, False, True, False, True]
    for i in range(n):
        assert np.isnan(got[i]).all() if reads[i] else np.isfinite(got[i]).all(), i


@pytest.mark.parametrize('n', [1, 2, 3, pr.CHUNK + 1])
def test_batch_sizes_two_launches_and_a_second_call(n):
    """n = 1 (never mixed by a draw; partner 0 is itself), 2, 3 and one image more than a launch takes: every image mixed with a
    partner that lies in the other launch where there is one; a second call returns the same words."""
    c, h, w = 3, 5, 8
    rng = np.random.default_rng(n)
    words = _finite(rng, (n, c, h, w))
    m = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    recs = pr.records(n, m=m, white=255.0, partner=[(n - 1 - i) for i in range(n)], **{'lambda': [0.25 + 0.5 * (i % 2) for i in range(n)]})
    got = _check_exact(words, recs, 'n = %d' % n)
    assert np.array_equal(_call(words, recs), got)
    one = np.concatenate([_call(np.stack([words[i], words[n - 1 - i]]), pr.records(2, m=m[[i, n - 1 - i]], white=255.0, partner=[1, 0],
                                                                                  **{'lambda': [recs['lambda'][i], 1.0]}))[:1] for i in range(n)])
    assert np.array_equal(one, got)


# ---- the tone curve ----------------------------------------------------------------------------------------------------------
def _check_tone(x, recs, cid):
    """Every element against photometric_reference(float64) within tone_bound / blend_bound; the worst ratio with the constant
    set to one is recorded under `cid`."""
    from yolo3 import augment
    want, fin, t = augment.photometric_reference(x, recs, np.float64, detail=True)
    got = _call(x.view(np.uint32), recs).view(np.float32).astype(np.float64)
    n = len(recs)
    white = recs['white'].astype(np.float64)[:, None, None, None]
    gamma = recs['gamma'].astype(np.float64)[:, None, None, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(white > 0, (t / recs['white'][:, None, None, None]).astype(np.float32), np.float32(1)).astype(np.float64)
    worst = (0.0, None)
    for k in (pr.TONE_K, 1.0):
        fb = np.where(gamma == 1, 0.0, pr.tone_bound(fin, s, gamma, white, k))
        lim = fb.copy()
        for i in range(n):
            if recs['lambda'][i] != 1:
                p = int(recs['partner'][i])
                lim[i] = pr.blend_bound(recs['lambda'][i], fin[i], fb[i], fin[p], fb[p])
        err = np.abs(got - want)
        if k == pr.TONE_K:
            bad = ~(err <= lim)
            ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1), np.where(err > 0, np.inf, 0.0))
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            print('%s: worst |error| / bound %.3f at %r' % (cid, ratio[i], tuple(int(v) for v in i)))
            failed = int(bad.sum()), float(ratio[i])
        else:
            ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0.0)
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            worst = (float(ratio[i]), 'image %d element %r gamma %.4g white %g t %.9g' % (
                i[0], tuple(int(v) for v in i[1:]), recs['gamma'][i[0]], recs['white'][i[0]], t[i]))
            print('%s: with the constant at 1: worst ratio %.3f, %s' % (cid, worst[0], worst[1]))
    if worst[0] >= pr.RATIOS.get(cid, (-1.0,))[0]:
        pr.RATIOS[cid] = worst
    assert failed[0] == 0, '%s: %d elements outside the bound, worst error / bound %.3f' % (cid, failed[0], failed[1])
    return got, want


@pytest.mark.parametrize('white', pr.TONE_WHITES)
def test_tone_curve_sweep_within_the_measured_bound(white):
    """The sweep the bound's constant was measured on: gamma in {0.5, 0.8, 1.25, 2} (one image each), t over [0, white] with both
    ends and the smallest positive values; t = 0 and t = white exact."""
    t = pr.tone_sweep(white)
    w = 4 * ((len(t) + 3) // 4)
    x = np.full((len(pr.TONE_GAMMAS), 1, 1, w), np.float32(white), np.float32)
    x[:, 0, 0, :len(t)] = t
    recs = pr.records(len(pr.TONE_GAMMAS), gamma=pr.TONE_GAMMAS, white=white)
    got, want = _check_tone(x, recs, 'sweep white=%g' % white)
    assert (got[x == 0] == 0).all() and (got[x == np.float32(white)] == white).all() and (x == 0).any()


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('size', [(5, 7), (33, 68), (96, 128)])
def test_tone_curve_with_matrix_clamp_and_mixup(size, c):
    """Drawn records (hue, saturation, value, gamma, every image changed) with MixUp on every image, on data that leaves [0, white]
    on both sides: matrix and clamp exact, the curve and the blend within the bound."""
    from yolo3 import augment
    h, w = size
    n = 2 if size == (96, 128) else 4
    rng = np.random.default_rng(h * w + c)
    x = (rng.random((n, c, h, w)) * 330 - 30).astype(np.float32)
    recs = augment.draw_mixup(augment.draw_photometric(5, 0, 0, n, c, 1.0, 0.1, 0.7, 0.4, 1.0, 255.0), 5, 0, 0, 1.0, 0.3)
    assert (recs['gamma'] != 1).all() and (recs['lambda'] < 1).all()
    got, _ = _check_tone(x, recs, 'drawn %dx%d c=%d' % (h, w, c))
    assert np.isfinite(got).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched():
    """Every Y3_EINVAL of yolo3hip.h with its message, before any launch: `out` keeps its NaN pre-fill between the canaries."""
    from yolo3._hip import lib
    words = _finite(np.random.default_rng(1), (3, 3, 8, 12))
    good = pr.records(3, white=255.0, partner=[1, 2, 0], **{'lambda': 0.5})
    _call(words, good)
    cases = []
    for v in (np.nan, np.inf, -np.inf):
        cases += [('m', (1, 4), v, 'non-finite'), ('bias', (0, 2), v, 'non-finite'), ('gamma', 2, v, 'non-finite'), ('white', 1, v, 'non-finite'),
                  ('lambda', 0, v, 'non-finite')]
    cases += [('gamma', 1, 0.0, 'gamma'), ('gamma', 1, -2.0, 'gamma'), ('white', 2, -1.0, 'white'), ('lambda', 0, -0.25, 'lambda'),
              ('lambda', 2, 1.5, 'lambda'), ('partner', 1, 3, 'partner'), ('partner', 1, -1, 'partner')]
    for field, idx, v, what in cases:
        r = good.copy()
        r[field][idx] = v
        _call(words, r, expect_rc=-1)
        msg = lib.y3_last_error().decode()
        assert msg.startswith('photometric_batch: record %d' % (idx[0] if isinstance(idx, tuple) else idx)) and what in msg, msg
    r = good.copy()
    r['white'][1], r['gamma'][1] = 0.0, 2.0
    _call(words, r, expect_rc=-1)
    assert 'needs white > 0' in lib.y3_last_error().decode()
    r = good.copy()
    r['lambda'][1], r['partner'][1] = 1.0, 99           # ignored when lambda == 1
    _call(words, r)
    _call(_finite(np.random.default_rng(2), (3, 2, 8, 12)), good, expect_rc=-1)
    assert 'channels' in lib.y3_last_error().decode()
    # null pointers, bad dims, misaligned and overlapping ranges; adjacent ranges are fine
    both = torch.full((4 * 16,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    rec2 = pr.records(2)
    p, st = both.data_ptr(), torch.cuda.current_stream().cuda_stream
    for args, what in (((None, 2, 1, 4, 4, rec2.ctypes.data, p), b'null'), ((p, 2, 1, 4, 4, None, p + 128), b'null'), ((p, 2, 1, 4, 4, rec2.ctypes.data, None), b'null'),
                       ((p, 0, 1, 4, 4, rec2.ctypes.data, p + 128), b'bad dims'), ((p, 2, 1, 0, 4, rec2.ctypes.data, p + 128), b'bad dims'),
                       ((p, 2, 1, 4, -1, rec2.ctypes.data, p + 128), b'bad dims'), ((p, 2, 1, 1 << 16, 1 << 15, rec2.ctypes.data, p + 128), b'too large')):
        assert lib.y3_photometric_batch(*args, st) == -1 and what in lib.y3_last_error(), (args, lib.y3_last_error())
    for s_off, o_off in ((0, 0), (0, 31), (31, 0), (0, 1)):
        assert lib.y3_photometric_batch(p + 4 * s_off, 2, 1, 4, 4, rec2.ctypes.data, p + 4 * o_off, st) == -1 and b'overlap' in lib.y3_last_error()
    assert lib.y3_photometric_batch(p + 2, 2, 1, 4, 4, rec2.ctypes.data, p + 4 * 32, st) == -1 and b'aligned' in lib.y3_last_error()
    assert lib.y3_photometric_batch(p, 2, 1, 4, 4, rec2.ctypes.data, p + 4 * 32, st) == 0
    torch.cuda.synchronize()
    assert bool((both == 0x5A5A5A5A).all())


def test_wrapper_returns_a_new_tensor():
    from yolo3 import augment
    from yolo3.imagereader import photometric_device
    n, c, h, w = 2, 3, 96, 128
    x = (np.random.default_rng(3).random((n, c, h, w)) * 255).astype(np.float32)
    recs = augment.draw_mixup(augment.draw_photometric(3, 0, 0, n, c, 1.0, 0.05, 0.5, 0.3, 0.0, 255.0), 3, 0, 0, 1.0, 0.2)
    xd = torch.from_numpy(x).cuda()
    yd = photometric_device(xd, recs)
    assert yd.data_ptr() != xd.data_ptr() and yd.shape == xd.shape and yd.dtype == torch.float32
    assert np.array_equal(yd.cpu().numpy().view(np.uint32), augment.photometric_reference(x, recs).view(np.uint32)) and np.array_equal(xd.cpu().numpy(), x)


# ---- data plane --------------------------------------------------------------------------------------------------------------
PHOTO = (1.0, 0.05, 0.7, 0.4, 0.0, 7, None)      # prob, hue, saturation, value, gamma (0: every stage exact), seed, white
MIXUP = (1.0, 0.2, 9)                             # prob, spread, seed
AFFINE = (1.0, 30.0, 5.0, 0.3, 0.1, 0.0, 7, 0.25)


@pytest.fixture(scope='module')
def lmdb64(tmp_path_factory):
    from test_gpu_mosaic import _make_lmdb
    path = str(tmp_path_factory.mktemp('photometric') / 'train-syn.lmdb')
    _make_lmdb(path, 12, (64, 64, 3))
    return path


def _take(path, nb, prefetch, photo=None, mixup=None, mosaic=None, affine=None, multiscale=None):
    """nb batches of 4 off a fresh unshuffled one-worker reader (identity augmentation records) -> NumPy, plus reader and dataset."""
    from yolo3.imagereader import ImageReader
    rd = ImageReader(path, ANCHORS, use_augmentation=False, shuffle=False, num_workers=1, augmentation_device='gpu', label_device='gpu')
    ds = rd.get_tf_dataset().batch(4)
    if photo is not None:
        ds = ds.photometric(*photo)
    if mosaic is not None:
        ds = ds.mosaic(*mosaic)
    if mixup is not None:
        ds = ds.mixup(*mixup)
    if affine is not None:
        ds = ds.affine(*affine)
    if multiscale is not None:
        ds = ds.multiscale(*multiscale)
    if prefetch:
        ds = ds.prefetch(2)
    rd.startup()
    try:
        it = iter(ds)
        out = [[t.cpu().numpy() for t in next(it)] for _ in range(nb)]
        it.close()
    finally:
        rd.shutdown()
    return out, rd, ds


def _expected(path, rd, ds, nb, photo, mixup, mosaic=None, affine=None):
    """The same batches by hand: "the same dataset without them" -- augment_device -> (mosaic_device) -> (affine_device), the
    passes that were there -- then photometric_reference(float32) on the host -> zscore_normalize_device; labels = format_boxes of
    mixup_boxes of (affine_boxes of (mosaic_boxes of)) the boxes."""
    from yolo3 import augment, lmdbio
    from yolo3.imagereader import augment_device, mosaic_device, affine_device, zscore_normalize_device, format_boxes
    crop = tuple(rd.image_size[:2])
    with lmdbio.Environment(path) as env:
        ex = [rd.load_example(rd.keys_flat[i % len(rd.keys_flat)], env) for i in range(4 * nb)]
    out = []
    for b in range(nb):
        e = ex[4 * b:4 * b + 4]
        size = ds.size_of_batch(b)
        recs = augment.rescale_record(np.concatenate([v[2] for v in e]), crop, size)
        boxes = [augment.scale_boxes(v[1], crop, size) for v in e]
        imgs = augment_device(torch.from_numpy(np.stack([v[0] for v in e])).cuda(), recs, size)
        if mosaic is not None:
            mrec = augment.draw_mosaic(mosaic[1], rd.shard_index, b, 4, size, mosaic[0])
            imgs = mosaic_device(imgs, mrec)
            boxes = augment.mosaic_boxes(boxes, mrec, size, mosaic[2])
        if affine is not None:
            arec, fwd = augment.draw_affine(affine[6], rd.shard_index, b, 4, size, *affine[:6])
            imgs = affine_device(imgs, arec)
            boxes = augment.affine_boxes(boxes, fwd, size, affine[7])
        imgs = imgs.cpu().numpy()
        prec = augment.photo_identity_records(4)
        if photo is not None:
            prec = augment.draw_photometric(photo[5], rd.shard_index, b, 4, 3, photo[0], photo[1], photo[2], photo[3], photo[4], 255.0)
        if mixup is not None:
            prec = augment.draw_mixup(prec, mixup[2], rd.shard_index, b, mixup[0], mixup[1])
            boxes = augment.mixup_boxes(boxes, prec)
        if photo is not None or mixup is not None:
            imgs = augment.photometric_reference(imgs, prec)
        labs = [format_boxes(bx if len(bx) else None, size + (3,), ANCHORS, rd.number_classes) for bx in boxes]
        z = zscore_normalize_device(torch.from_numpy(imgs).cuda()).cpu().numpy()
        out.append([z] + [np.stack([l[s] for l in labs]) for s in range(3)])
    return out


def _same_batches(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 4
        for t, (a, e) in enumerate(zip(g, w)):
            assert a.shape == e.shape and a.dtype == e.dtype == np.float32, (b, t, a.shape, e.shape)
            assert np.array_equal(a.view(np.uint32), e.view(np.uint32)), 'batch %d tensor %d: %d words differ' % (
                b, t, int((a.view(np.uint32) != e.view(np.uint32)).sum()))


@pytest.mark.parametrize('prefetch', [False, True])
@pytest.mark.parametrize('chain', ['alone', 'mosaic+affine+multiscale'])
def test_dataset_photometric_and_mixup_end_to_end(lmdb64, prefetch, chain):
    """photometric(1.0) + mixup(1.0) without a tone curve, so every stage is exact: batches bit-equal to the dataset without them
    -> photometric_reference -> z-score, labels bit-equal to format_boxes of the mixup_boxes lists; once alone, once behind
    mosaic + affine at both sizes of multiscale (the order mosaic -> affine -> this pass); the prefetch path draws the same."""
    full = chain != 'alone'
    mosaic = (1.0, 5, 0.25) if full else None
    affine = AFFINE if full else None
    multiscale = ([(64, 64), (64, 96)], 1, 1) if full else None
    got, rd, ds = _take(lmdb64, 2, prefetch, PHOTO, MIXUP, mosaic, affine, multiscale)
    assert ds.photo_cfg == PHOTO[:6] + (255.0,) and ds.mixup_cfg == MIXUP
    if full:
        assert sorted(tuple(g[0].shape[2:]) for g in got) == [(64, 64), (64, 96)]
    _same_batches(got, _expected(lmdb64, rd, ds, 2, PHOTO, MIXUP, mosaic, affine))
    plain = _expected(lmdb64, rd, ds, 2, None, None, mosaic, affine)
    assert not np.allclose(got[0][0], plain[0][0], atol=1e-3)
    assert sum(int(g[3][..., 4].sum()) for g in got) > sum(int(p[3][..., 4].sum()) for p in plain)      # the partners' boxes are there


def test_dataset_rerun_tone_curve_and_defaults_are_untouched(lmdb64):
    """Two runs with one seed repeat bit for bit, another seed gives other batches; with a tone curve the batch stays finite; with
    neither option the batches are those of the chain augment_device -> zscore_normalize_device, which is what this path launched
    before the options existed."""
    a, _, _ = _take(lmdb64, 2, True, PHOTO, MIXUP)
    b, _, _ = _take(lmdb64, 2, False, PHOTO, MIXUP)
    _same_batches(a, b)
    c, _, _ = _take(lmdb64, 1, False, PHOTO[:5] + (8, None), MIXUP)
    d, _, _ = _take(lmdb64, 1, False, PHOTO, (1.0, 0.2, 10))
    assert not np.array_equal(a[0][0], c[0][0]) and not np.array_equal(a[0][0], d[0][0])
    e, _, _ = _take(lmdb64, 1, False, (1.0, 0.05, 0.7, 0.4, 1.0, 7, None), None)
    assert np.isfinite(e[0][0]).all() and not np.array_equal(e[0][0], a[0][0])
    for prefetch in (False, True):
        p, rd, ds0 = _take(lmdb64, 2, prefetch)
        assert ds0.photo_cfg is None and ds0.mixup_cfg is None
        _same_batches(p, _expected(lmdb64, rd, ds0, 2, None, None))


def test_photometric_on_a_reader_with_host_labels(lmdb64):
    """photometric() needs only augmentation_device='gpu': on a reader whose labels are built in the workers the pass runs behind
    augment_device, in both the plain and the prefetch loop."""
    from yolo3 import augment, lmdbio
    from yolo3.imagereader import ImageReader, augment_device, zscore_normalize_device
    res = []
    for prefetch in (False, True):
        rd = ImageReader(lmdb64, ANCHORS, use_augmentation=False, shuffle=False, num_workers=1, augmentation_device='gpu')
        ds = rd.get_tf_dataset().batch(4).photometric(*PHOTO)
        ds = ds.prefetch(2) if prefetch else ds
        rd.startup()
        try:
            it = iter(ds)
            res.append([[t.cpu().numpy() for t in next(it)] for _ in range(2)])
            it.close()
        finally:
            rd.shutdown()
    _same_batches(res[0], res[1])
    rd2 = ImageReader(lmdb64, ANCHORS, use_augmentation=False, shuffle=False, num_workers=1, augmentation_device='gpu', label_device='gpu')
    with lmdbio.Environment(lmdb64) as env:
        ex = [rd2.load_example(rd2.keys_flat[i], env) for i in range(4, 8)]      # batch 1
    imgs = augment_device(torch.from_numpy(np.stack([v[0] for v in ex])).cuda(), np.concatenate([v[2] for v in ex]), (64, 64)).cpu().numpy()
    prec = augment.draw_photometric(PHOTO[5], 0, 1, 4, 3, *PHOTO[:5], 255.0)
    want = zscore_normalize_device(torch.from_numpy(augment.photometric_reference(imgs, prec)).cuda()).cpu().numpy()
    assert np.array_equal(res[0][1][0].view(np.uint32), want.view(np.uint32))


def test_training_step_on_a_jittered_mixed_batch(lmdb64):
    from yolo3.model import YoloV3
    from yolo3.imagereader import ImageReader
    rd = ImageReader(lmdb64, ANCHORS, use_augmentation=True, shuffle=False, num_workers=1, augmentation_device='gpu', label_device='gpu')
    ds = rd.get_tf_dataset().batch(4).photometric(1.0, gamma=0.5, seed=2).mixup(1.0, seed=2)
    rd.startup()
    try:
        it = iter(ds)
        batch = next(it)
        it.close()
    finally:
        rd.shutdown()
    assert tuple(batch[0].shape) == (4, 3, 64, 64) and bool(torch.isfinite(batch[0]).all()) and float(batch[3][..., 4].sum()) > 0
    yolo = YoloV3(4, [64, 64, 3], rd.number_classes, ANCHORS, learning_rate=1e-4)
    loss = float(yolo.train_step((batch[0], list(batch[1:]))))
    torch.cuda.synchronize()
    assert np.isfinite(loss) and loss > 0
    assert bool(torch.isfinite(yolo.grads).all()) and float(yolo.grads.abs().sum()) > 0


def test_cli_photometric_mixup_training(tmp_path):
    """train.py --augmentation_device gpu --photo_prob 1 --mixup_prob 1 for two steps on a tiny database: the configuration
    lines, finite losses, an export at the stored size."""
    from test_gpu_mosaic import _make_lmdb
    tmp = str(tmp_path)
    for split, cnt, seed in (('train', 8, 5), ('test', 3, 6)):
        _make_lmdb(os.path.join(tmp, '%s-syn.lmdb' % split), cnt, (64, 64, 3), seed=seed, lo=16, hi=32)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = os.path.join(tmp, 'out')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--batch_size', '4', '--test_every_n_steps', '2', '--train_database',
                        os.path.join(tmp, 'train-syn.lmdb'), '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out,
                        '--early_stopping', '1', '--use_augmentation', '1', '--augmentation_device', 'gpu', '--max_epochs', '1', '--reader_count', '1',
                        '--photo_prob', '1.0', '--photo_hue', '0.05', '--photo_gamma', '0.5', '--photo_seed', '3', '--mixup_prob', '1.0',
                        '--mixup_spread', '0.2', '--mixup_seed', '4', '--learning_rate', '1e-4'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Photometric augmentation: probability 1 per image, hue +-0.05 turns, saturation 1 +- 0.7, value 1 +- 0.4, tone exponent 2^+-0.5, white 255 (seed 3)' in r.stdout
    assert 'MixUp: probability 1 per image, lambda uniform in 0.5 +- 0.2 (seed 4)' in r.stdout
    train = [ln.split(',') for ln in open(glob.glob(os.path.join(out, 'scalars-*', 'train.csv'))[0]).read().split()][1:]
    assert len(train) >= 2 and all(np.isfinite(float(v)) for row in train for v in row[1:])
    losses = [float(v) for v in open(os.path.join(out, 'test_loss.csv')).read().split()]
    assert len(losses) == 1 and np.isfinite(losses[0])
    z = np.load(os.path.join(out, 'saved_model', 'yolov3.npz'))
    assert z['meta_img_size'].tolist() == [64, 64, 3]
