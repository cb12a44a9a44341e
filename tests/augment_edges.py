"""The pixel kernels of y3_augment_batch (csrc/augment.hip) at their edges: a float64 restatement of the contract in
include/yolo3hip.h (steps 1-4 above y3_aug_record), case tables and per-element error bounds.  Host only: this module imports
no GPU code.  test_cpu_augment_edges.py holds the restatement, the tables and the bounds to what they claim;
test_gpu_augment_edges.py runs them.

WHAT THE TABLES ARE FOR.  The kernels work in 256-column segments with a reflect halo (row pass), 64 x 32 tiles with a row halo
(column pass), launch chunks of 32 images, a 4-byte or an element-wise staging copy of the two source rows, and keep the crop's
min / max as order-preserving keys.  Every table below sits on one of these boundaries; the CPU test asserts that it does.

ERROR BOUNDS.  Sources are exact fp32 numbers (uint8, uint16, float32); the restatement works in fp64.  U = 2^-24 is the unit
roundoff of fp32 and a chain of k roundings costs ku(k) = k U (1 + 2^-20), as in stream_kernels.py.  The library is built with
-ffp-contract=off, so every product and sum below is rounded.  Every bound is per element and relative to the sum of the
ABSOLUTE addends that enter that element, never to a tensor-wide maximum; errors of an earlier step pass through the later,
linear steps with the same non-negative weights.  All of it times (1 + 2^-10) for the second-order terms, plus SLACK = 1e-12 of
the absolute sum for the fp64 side.
  resample   the fraction f = fl(fl(rem) / fl(den)) carries k = 3 roundings: |f^ - f| <= ku(3) f.  lerp(a, b, f) = (1 - f) a + f b
             makes 3 roundings on the a term (1 - f, product, sum) and 2 on the b term, and moves by |f^ - f| (|a| + |b|):
                 L(a, b, f) = ku(3) (f (|a| + |b|) + (1 - f) |a| + f |b|),   0 when f == 0 (the kernel returns a).
             Three lerps: e = L(top, bot, fy) + (1 - fy) L(a00, a01, fx) + fy L(a10, a11, fx).  On 0..255 at most 2.8e-4.
  min / max  max is monotone: the device's max lies in [max(x - e), max(x + e)], its min in [min(x - e), min(x + e)].
  noise      s^ = fl(noise fl(max^ + (-min^))) (2 roundings, and the two intervals above), fl(s^ z^) (1), fl(x + s z) (1):
                 e += |s| NORMAL_TOL + |z| |noise| (Emax + Emin) + ku(3) |s z| + ku(1) (|x| + |s z|).
             NORMAL_TOL = 1e-3 is not derived (logf, cosf): it is the figure tests/test_gpu_augment.py already allows between the
             device's N(0,1) and the fp64 twin; the GPU test reports what it measures.
  blur       per axis acc = w0 p0 + sum_k wk (p-k + p+k): a term passes the fp32 rounding of its weight, the pair sum, the
             product and at most R further sums, k = R + 3, of blur(|x|).  The channel mix is a 3-term dot product from 0 with
             fp32 coefficients: k = 4 of mix(|x|).  On 0..255 at radius 8 at most 2 ku(11) 255 + ku(4) 255 = 4e-4.
Together below the 1e-3 on 0..255 that tests/test_gpu_augment.py allows for resample and for blur (asserted on the CPU).

DISCRIMINATION.  In a noise + blur record the noise term |s| NORMAL_TOL must not hide a wrong outermost tap, w[R] times the
difference of two neighbours: discrimination() moves the outermost tap of the first axis longer than 1 by one element, passes the
change through the remaining axes in fp64 and returns the largest change / bound near the segment seam.  The tables keep
severity * 255 at 0.13 so that it stays above 1 (asserted on the CPU for every such record).
"""
import functools
import zlib

import numpy as np
import scipy.ndimage

from yolo3.augment import AUG_RECORD

U = 2.0 ** -24
SLACK = 1e-12
SECOND_ORDER = 1.0 + 2.0 ** -10
NORMAL_TOL = 1e-3
CHUNK = 32                      # images per launch
SEGMENT = 256                   # columns per workgroup of the row pass
COL_TILE = (32, 64)             # rows x columns per workgroup of the column pass
MAX_RADIUS = 8
STAGE_BYTES = 61440             # two source rows, each rounded up to 16 bytes
DTYPE_CODE = {'uint8': 0, 'uint16': 1, 'float32': 2}
SIGMAS = (0.3749, 1.0, 2.0, 2.124)
SMALL_NOISE = 0.0005            # severity of the noise + blur records: |s| = 0.13 on 0..255
SEEDS = (0, 2 ** 32, 2 ** 63 + 12345, 0x5DEECE66D1234567)


def ku(k):
    return k * U * (1.0 + 2.0 ** -20)


def seed_of(name):
    return zlib.crc32(name.encode())


def radius_of(sigma):
    """int(4 sigma + 0.5) of the fp32 sigma the record carries; 0 for sigma <= 0"""
    s = float(np.float32(sigma))
    return int(4.0 * s + 0.5) if s > 0 else 0


def stage_bytes(w_in, c, dtype):
    row = w_in * c * np.dtype(dtype).itemsize
    return 2 * ((row + 15) // 16 * 16)


def record(h_in, w_in, rows, cols, dy=0, dx=0, rx=0, ry=0, noise=0.0, u=0.5, blur=0.0, seed=0):
    rec = np.zeros(1, AUG_RECORD)
    rec[0] = (h_in, w_in, rows, cols, dy, dx, int(rx), int(ry), noise, u, blur, 0, seed)
    return rec[0]


# ------------------------------------------------------------------------------------------------------------------
# the contract in fp64
# ------------------------------------------------------------------------------------------------------------------
def mirror(p, n):
    """whole-sample symmetric, period 2 (n - 1), the edge is not repeated (scipy 'mirror')"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    q = p % period
    return np.where(q < n, q, period - q)


def reflect(p, n):
    """half-sample symmetric, period 2 n, the edge repeats (scipy 'reflect')"""
    q = np.asarray(p, np.int64) % (2 * n)
    return np.where(q < n, q, 2 * n - 1 - q)


def source_coords(n_in, n_res, start, count):
    """rescaled indices start .. start + count - 1: the two (mirrored) source indices and the fp64 fraction of
    ((2q + 1) n_in - n_res) / (2 n_res), floor and remainder in exact integers"""
    q = np.arange(start, start + count, dtype=np.int64)
    num, den = (2 * q + 1) * n_in - n_res, 2 * n_res
    i0 = num // den
    f = (num - i0 * den).astype(np.float64) / den
    return mirror(i0, n_in), mirror(i0 + 1, n_in), f


def _lerp_bound(a, b, f):
    return np.where(f > 0, ku(3) * (f * (a + b) + (1 - f) * a + f * b), 0.0)


def resample(img, rec, crop, with_bound=False):
    """step 1: float64 [H, W, C] of one record (bilinear, mirror, crop, then the flips); with_bound: also its error bound"""
    img = np.asarray(img, np.float64)
    if img.ndim == 2:
        img = img[..., None]
    H, W = crop
    ya, yb, fy = source_coords(img.shape[0], int(rec['rows']), int(rec['dy']), H)
    xa, xb, fx = source_coords(img.shape[1], int(rec['cols']), int(rec['dx']), W)
    fxb, fyb = fx[None, :, None], fy[:, None, None]
    a00, a01, a10, a11 = img[ya][:, xa], img[ya][:, xb], img[yb][:, xa], img[yb][:, xb]
    top, bot = (1 - fxb) * a00 + fxb * a01, (1 - fxb) * a10 + fxb * a11
    v = (1 - fyb) * top + fyb * bot
    mt, mb = (1 - fxb) * np.abs(a00) + fxb * np.abs(a01), (1 - fxb) * np.abs(a10) + fxb * np.abs(a11)
    e = _lerp_bound(mt, mb, fyb) + (1 - fyb) * _lerp_bound(np.abs(a00), np.abs(a01), fxb) + fyb * _lerp_bound(np.abs(a10), np.abs(a11), fxb)
    e = e * SECOND_ORDER + SLACK * ((1 - fyb) * mt + fyb * mb)
    if rec['reflect_x']:
        v, e = v[:, ::-1], e[:, ::-1]
    if rec['reflect_y']:
        v, e = v[::-1], e[::-1]
    return (v, e) if with_bound else v


def philox_normals(seed, n):
    """Host twin of the device stream (yolo3hip.h): Philox4x32-10, key = seed halves, counter (e, 0, 0, 0); Box-Muller."""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    c0 = np.arange(n, dtype=np.uint32)
    c1 = np.zeros(n, np.uint32)
    c2 = np.zeros(n, np.uint32)
    c3 = np.zeros(n, np.uint32)
    k0, k1 = seed & 0xffffffff, seed >> 32
    for _ in range(10):
        p0 = c0.astype(np.uint64) * M0
        p1 = c2.astype(np.uint64) * M1
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint32(k0), lo1, hi0 ^ c3 ^ np.uint32(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    u1 = ((c0 >> 8).astype(np.float64) + 1) * 2.0**-24
    u2 = (c1 >> 8).astype(np.float64) * 2.0**-24
    return np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)


def noise_factor(rec):
    """float32(severity * (2 u - 1)), formed in double from the record's fp32 fields"""
    return float(np.float32(float(rec['noise_severity']) * (2.0 * float(rec['u_noise']) - 1.0)))


def noise(x_chw, rec):
    """step 2: x + s N(0,1), s = float32(severity (2u - 1)) (max - min) of x, element order CHW.  Returns (noisy, s, normals)."""
    x = np.asarray(x_chw, np.float64)
    s = noise_factor(rec) * (x.max() - x.min())
    z = philox_normals(int(rec['seed']), x.size).reshape(x.shape)
    return x + s * z, s, z


def blur(x_hwc, sigma):
    """step 3: scipy's gaussian_filter with the record's fp32 sigma on all three axes; the identity for radius 0"""
    x = np.asarray(x_hwc, np.float64)
    if radius_of(sigma) == 0:
        return x
    return scipy.ndimage.gaussian_filter(x, float(np.float32(sigma)), mode='reflect')


def gauss_weights(sigma):
    """w[0 .. R] of the fp32 sigma, normalised over -R .. R"""
    s, R = float(np.float32(sigma)), radius_of(sigma)
    phi = np.exp(-0.5 / (s * s) * np.arange(R + 1, dtype=np.float64) ** 2)
    return phi / (phi[0] + 2 * phi[1:].sum())


def blur_indexwise(x_hwc, sigma):
    """the same blur index by index: period-2n reflection on each axis in turn, weights normalised over -R .. R"""
    x = np.asarray(x_hwc, np.float64)
    R = radius_of(sigma)
    if R == 0:
        return x
    w = gauss_weights(sigma)
    for axis in range(3):
        n = x.shape[axis]
        out = np.zeros_like(x)
        for i in range(n):
            acc = 0.0
            for k in range(-R, R + 1):
                acc = acc + w[abs(k)] * np.take(x, int(reflect(i + k, n)), axis=axis)
            idx = [slice(None)] * 3
            idx[axis] = i
            out[tuple(idx)] = acc
        x = out
    return x


def _blur1(x, sigma, axis):
    return scipy.ndimage.gaussian_filter1d(x, float(np.float32(sigma)), axis=axis, mode='reflect')


def chain_full(img, rec, crop):
    """Steps 1-4 of one record in fp64 with everything the tests compare against: want / bound [C, H, W], base / base_bound (step
    1 alone, CHW), mn / mx and the intervals mn_iv / mx_iv the device's keys must fall in, s, the normals z (CHW) or None, the
    noisy image before the blur (HWC), kind in {'resample', 'noise', 'blur', 'noise+blur'}."""
    x, e = resample(img, rec, crop, with_bound=True)
    base, base_bound = np.transpose(x, (2, 0, 1)).copy(), np.transpose(e, (2, 0, 1)).copy()
    mn, mx = float(x.min()), float(x.max())
    mn_iv, mx_iv = (float((x - e).min()), float((x + e).min())), (float((x - e).max()), float((x + e).max()))
    R = radius_of(rec['blur_sigma'])
    nf = noise_factor(rec)
    s, z, n = 0.0, None, x
    if nf != 0.0:
        noisy, s, z = noise(base, rec)
        zh = np.transpose(z, (1, 2, 0))
        n = np.transpose(noisy, (1, 2, 0))
        emx, emn = max(mx_iv[1] - mx, mx - mx_iv[0]), max(mn_iv[1] - mn, mn - mn_iv[0])
        sz = np.abs(s * zh)
        e = e + abs(s) * NORMAL_TOL + np.abs(zh) * abs(nf) * (emx + emn) + ku(3) * sz + ku(1) * (np.abs(x) + sz)
    want = n
    if R > 0:
        sig = rec['blur_sigma']
        C = x.shape[2]
        A = _blur1(np.abs(n), sig, 1)
        e = _blur1(e, sig, 1) + ku(R + 3) * A
        if C > 1:
            A = _blur1(A, sig, 2)
            e = _blur1(e, sig, 2) + ku(4) * A
        A = _blur1(A, sig, 0)
        e = (_blur1(e, sig, 0) + ku(R + 3) * A) * SECOND_ORDER + SLACK * A
        want = blur(n, sig)
    kind = ('noise+blur' if R > 0 else 'noise') if nf != 0.0 else ('blur' if R > 0 else 'resample')
    return dict(want=np.transpose(want, (2, 0, 1)).copy(), bound=np.transpose(e, (2, 0, 1)).copy(), base=base, base_bound=base_bound, mn=mn, mx=mx,
                mn_iv=mn_iv, mx_iv=mx_iv, s=s, z=z, noisy_hwc=n, kind=kind, radius=R)


def chain(img, rec, crop):
    """the float64 [C, H, W] result of one record and the (min, max) of its step 1"""
    f = chain_full(img, rec, crop)
    return f['want'], (f['mn'], f['mx'])


def discrimination(full, rec):
    """A noise + blur record: the outermost tap (weight w[R]) of the first axis longer than 1 -- W, else H, else C -- reads the
    element one further out; the change of the output through the remaining axes, in fp64, over the bound.  Returns the largest
    ratio over the columns within R of a segment seam (all columns of an image of one segment), or None when every axis has
    length 1 (every tap reads the one element: nothing to tell apart)."""
    n, R, sig = full['noisy_hwc'], full['radius'], rec['blur_sigma']
    H, W, C = n.shape
    axis = 1 if W > 1 else 0 if H > 1 else 2 if C > 1 else None
    if axis is None:
        return None
    L = n.shape[axis]
    i = np.arange(L)
    d = gauss_weights(sig)[R] * (np.take(n, reflect(i + R + 1, L), axis=axis) - np.take(n, reflect(i + R, L), axis=axis))
    for other in (0, 1, 2):
        if other != axis:
            d = _blur1(d, sig, other)
    ratio = np.abs(np.transpose(d, (2, 0, 1))) / full['bound']
    if W > SEGMENT:
        cols = np.concatenate([np.arange(s0 - R, s0 + R) for s0 in range(SEGMENT, W, SEGMENT)])
        ratio = ratio[:, :, cols[(cols >= 0) & (cols < W)]]
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------
# case tables: a case is one y3_augment_batch call
# ------------------------------------------------------------------------------------------------------------------
def _case(table, cid, dtype, C, h_in, w_in, crop, records, source='u255', shared=True, **extra):
    """records: list of (record, flags) -- flags: same_bits_as = index of the record of this batch whose output bits it must
    equal, exact_copy = the output is the source's values, plain = index of the same geometry without noise and blur"""
    recs = [r for r, _ in records]
    assert all(int(r['src_h']) == h_in and int(r['src_w']) == w_in for r in recs)
    return dict(table=table, id='%s-%s' % (table, cid), dtype=dtype, C=C, h_in=h_in, w_in=w_in, crop=tuple(crop), records=recs,
                flags=[dict(f) for _, f in records], source=source, shared=shared, **extra)


def case_images(case):
    """[n, h_in, w_in, C] of the case's dtype; one image repeated when the case shares it.  Sources: u255 = random 0..255 (uint16:
    times 257, float32: plus a random fraction), signed = N(0, 50^2), negative = -200 .. -1, const+ / const- = +-37.5"""
    return _images_cached(case['id'])


@functools.lru_cache(maxsize=None)
def _images_cached(cid):
    case = CASES_BY_ID[cid]
    g = np.random.default_rng(seed_of(cid))
    n, shape = len(case['records']), (case['h_in'], case['w_in'], case['C'])
    count = 1 if case['shared'] else n
    src, dt = case['source'], np.dtype(case['dtype'])
    if src == 'u255':
        a = g.integers(0, 256, (count,) + shape)
        if dt == np.uint16:
            a = a * 257
        a = a.astype(dt)
        if dt == np.float32:
            a = a + g.random((count,) + shape).astype(np.float32)
    elif src == 'signed':
        a = (50.0 * g.standard_normal((count,) + shape)).astype(np.float32)
    elif src == 'negative':
        a = -g.uniform(1.0, 200.0, (count,) + shape).astype(np.float32)
    else:
        a = np.full((count,) + shape, 37.5 if src == 'const+' else -37.5, np.float32)
    a = np.ascontiguousarray(np.broadcast_to(a, (n,) + shape) if case['shared'] else a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _full_cached(cid, i):
    case = CASES_BY_ID[cid]
    return chain_full(case_images(case)[i], case['records'][i], case['crop'])


def case_full(case, i):
    """chain_full of record i of a case: computed once, shared, never modified by a test"""
    return _full_cached(case['id'], i)


def _flips(j):
    return j & 1, (j >> 1) & 1


def _blur_pairs(h_in, w_in, rows, cols, dy, dx, sigmas, tag):
    """per sigma a blur-alone record and a noise + blur record with the opposite flips: both kinds meet all four flip pairs"""
    out = []
    for j, s in enumerate(sigmas):
        rx, ry = _flips(j)
        out.append((record(h_in, w_in, rows, cols, dy, dx, rx, ry, blur=s), {}))
        out.append((record(h_in, w_in, rows, cols, dy, dx, 1 - rx, 1 - ry, noise=SMALL_NOISE, u=float(j % 2), blur=s,
                           seed=seed_of('%s%d' % (tag, j)) | (j << 40)), {}))
    return out


# the row pass: widths either side of one segment, 8 past it (the halo of segment 1 is the whole segment), a third segment
SEAM_SIZES = ((5, 255), (5, 256), (5, 257), (5, 264), (3, 513), (33, 257))
SEAM_CASES = [_case('seam', '%dx%d-c%d' % (H, W, C), 'uint8', C, H + 3, W + 5, (H, W), _blur_pairs(H + 3, W + 5, H + 4, W + 7, 1, 2, SIGMAS, 'seam'))
              for H, W in SEAM_SIZES for C in (1, 3)]

# the column pass: 32-row x 64-column tiles, one short / exact / one past in both directions, a third row tile
COLUMN_SIZES = tuple((H, W) for H in (31, 32, 33, 40, 65) for W in (63, 64, 65))
COLUMN_CASES = [_case('column', '%dx%d-c%d' % (H, W, 1 + 2 * (k % 2)), 'uint8', 1 + 2 * (k % 2), H + 2, W + 2, (H, W),
                      _blur_pairs(H + 2, W + 2, H + 3, W + 3, 1, 1, SIGMAS, 'col')) for k, (H, W) in enumerate(COLUMN_SIZES)]

# axes shorter than the radius: the reflection wraps several times
TINY_SIZES = ((1, 1), (1, 7), (7, 1), (3, 5), (2, 2), (8, 8))
TINY_CASES = [_case('tiny', '%dx%d-c%d' % (H, W, C), 'uint8', C, H + 2, W + 3, (H, W), _blur_pairs(H + 2, W + 3, H + 3, W + 4, 1, 1, SIGMAS, 'tiny'))
              for H, W in TINY_SIZES for C in (1, 3)]


def _source_cases():
    out = []
    # tiny sources, upscaled >= 4 x: n == 1 and period 2 of the mirror; crop at offset 0 and at the maximal offset, every flip
    for (h, w), dtype, C in (((1, 1), 'uint8', 3), ((1, 9), 'float32', 1), ((9, 1), 'uint16', 3), ((2, 2), 'float32', 3), ((2, 3), 'uint8', 1)):
        rows, cols = 4 * h + 3, 4 * w + 2
        crop = (min(rows - 1, 6), min(cols - 1, 10))
        recs = [(record(h, w, rows, cols, 0, 0, 0, 0), {}), (record(h, w, rows, cols, rows - crop[0], cols - crop[1], 1, 0), {}),
                (record(h, w, rows, cols, 0, cols - crop[1], 0, 1), {}), (record(h, w, rows, cols, rows - crop[0], 0, 1, 1), {})]
        out.append(_case('source', 'tiny%dx%d-%s-c%d' % (h, w, dtype, C), dtype, C, h, w, crop, recs))
    # 2.0 x up and 0.3 x down, well outside the training range 0.85 - 1.3; each with an exact copy beside it
    out.append(_case('source', 'up2-float32-c3', 'float32', 3, 40, 56, (30, 40),
                     [(record(40, 56, 80, 112, 0, 0), {}), (record(40, 56, 80, 112, 50, 72, 1, 1), {}), (record(40, 56, 40, 56, 10, 16, 0, 1), dict(exact_copy=True))]))
    out.append(_case('source', 'down0.3-float32-c1', 'float32', 1, 40, 56, (10, 14),
                     [(record(40, 56, 12, 17, 0, 0), {}), (record(40, 56, 12, 17, 2, 3, 1, 0), {}), (record(40, 56, 40, 56, 30, 42, 1, 1), dict(exact_copy=True))]))
    # rows of 273, 37, 30 and 66 bytes take the element-wise staging copy (and their images start at any address); 276 is the control
    for (h, w), dtype, C in (((13, 91), 'uint8', 3), ((13, 37), 'uint8', 1), ((13, 5), 'uint16', 3), ((13, 33), 'uint16', 1), ((13, 92), 'uint8', 3)):
        crop = (9, min(w, 20) - 1)
        recs = [(record(h, w, h, w, 0, 0), dict(exact_copy=True)), (record(h, w, h, w, h - crop[0], w - crop[1], 1, 1), dict(exact_copy=True)),
                (record(h, w, 15, w + 4, 0, 0, 1, 0), {}), (record(h, w, 15, w + 4, 15 - crop[0], w + 4 - crop[1], 0, 1), {}),
                (record(h, w, 11, w + 1, 1, 1, 0, 0, blur=1.0), {})]
        out.append(_case('source', 'rows%dx%d-%s-c%d' % (h, w, dtype, C), dtype, C, h, w, crop, recs))
    return out


SOURCE_CASES = _source_cases()
UNALIGNED_IDS = ('source-rows13x91-uint8-c3', 'source-rows13x37-uint8-c1', 'source-rows13x5-uint16-c3', 'source-rows13x33-uint16-c1', 'source-tiny2x3-uint8-c1')
ALIGNED_CONTROL_ID = 'source-rows13x92-uint8-c3'

# the largest accepted source row: 2560 x 3 x 4 = 30720 bytes, 61440 bytes of dynamic LDS
WIDE_CASE = _case('wide', '3x2560-float32-c3', 'float32', 3, 3, 2560, (3, 300),
                  [(record(3, 2560, 3, 2560, 0, 2260, 0, 1), dict(exact_copy=True)), (record(3, 2560, 3, 2600, 0, 2300, 1, 0), {})])
WIDE_REFUSED_W = 2561


def _signed_cases():
    out = []
    for src in ('signed', 'negative', 'const+', 'const-'):
        recs = [(record(20, 28, 20, 28, 2, 3, 1, 0), dict(exact_copy=True)), (record(20, 28, 23, 31, 3, 4, 0, 1), {})]
        for j, u in enumerate((0.0, 0.25, 1.0)):
            recs.append((record(20, 28, 20, 28, 2, 3, 1, 0, noise=0.03, u=u, seed=SEEDS[j + 1]), dict(plain=0, same_bits_as=0 if src.startswith('const') else None)))
            recs.append((record(20, 28, 23, 31, 3, 4, 0, 1, noise=0.03, u=u, seed=SEEDS[j]), dict(plain=1)))
        recs.append((record(20, 28, 23, 31, 3, 4, 0, 1, blur=1.0), dict(plain=1)))
        if not src.startswith('const'):                                    # nothing tells two taps of a constant image apart
            recs.append((record(20, 28, 23, 31, 3, 4, 1, 1, noise=SMALL_NOISE, u=1.0, blur=2.0, seed=77), {}))
        out.append(_case('signed', src, 'float32', 3, 20, 28, (16, 24), recs, source=src))
    return out


SIGNED_CASES = _signed_cases()


def _noise_cases():
    out = []
    for dtype, C in (('uint8', 1), ('uint16', 3), ('float32', 1), ('float32', 3)):
        recs = [(record(28, 46, 30, 48, 3, 5, *_flips(j)), {}) for j in range(4)]
        for j in range(4):
            for k, u in enumerate((0.0, 0.3, 0.5, 1.0)):
                recs.append((record(28, 46, 30, 48, 3, 5, *_flips(j), noise=0.03, u=u, seed=SEEDS[(j + k) % 4]), dict(plain=j, same_bits_as=j if u == 0.5 else None)))
        out.append(_case('noise', '%s-c%d' % (dtype, C), dtype, C, 28, 46, (24, 40), recs))
    return out


NOISE_CASES = _noise_cases()

# fp32 sigmas at and just below every step of int(4 sigma + 0.5), and the last accepted one
RADIUS_SIGMAS = tuple(v for r in range(1, 9) for v in ((2 * r - 1) / 8 - 0.0001, (2 * r - 1) / 8)) + (2.124,)
RADIUS_EXPECTED = tuple(v for r in range(1, 9) for v in (r - 1, r)) + (8,)
RADIUS_REFUSED_SIGMA = 2.125
RADIUS_CASES = [_case('radius', 'c%d' % C, 'float32', C, 15, 24, (12, 20),
                      [(record(15, 24, 16, 26, 2, 3, 1, 0), {})] + [(record(15, 24, 16, 26, 2, 3, 1, 0, blur=s), dict(plain=0, same_bits_as=0 if radius_of(s) == 0 else None))
                                                                   for s in RADIUS_SIGMAS]) for C in (1, 3)]

MIXED_KINDS = ('neither', 'noise', 'blur', 'both')
MIXED_ORDERS = {'chunk1-mixed': ['neither'] * 32 + [MIXED_KINDS[i % 4] for i in range(8)],
                'chunk0-mixed': [MIXED_KINDS[i % 4] for i in range(32)] + ['neither'] * 8,
                'interleaved': [MIXED_KINDS[i % 4] for i in range(40)]}


def _mixed_record(i, kind):
    sev = {'neither': 0.0, 'noise': 0.03, 'blur': 0.0, 'both': SMALL_NOISE}[kind]
    sig = SIGMAS[(i // 4) % 4] if kind in ('blur', 'both') else 0.0
    rows, cols = 30 + i % 7, 50 + (3 * i) % 11                     # a rescaled size of its own per image
    return record(30, 50, rows, cols, i % (rows - 23), (2 * i) % (cols - 39), *_flips(i // 2), noise=sev, u=float(i % 3 == 0), blur=sig, seed=seed_of('mixed%d' % i) << 7)


MIXED_BATCH = [_case('mixed', name, 'uint8', 3, 30, 50, (24, 40), [(_mixed_record(i, k), dict(kind=k)) for i, k in enumerate(kinds)], shared=False)
               for name, kinds in MIXED_ORDERS.items()]

TABLES = dict(seam=SEAM_CASES, column=COLUMN_CASES, tiny=TINY_CASES, source=SOURCE_CASES, wide=[WIDE_CASE], signed=SIGNED_CASES, noise=NOISE_CASES,
              radius=RADIUS_CASES, mixed=MIXED_BATCH)
ALL_CASES = [c for t in TABLES.values() for c in t]
CASES_BY_ID = {c['id']: c for c in ALL_CASES}
assert len(CASES_BY_ID) == len(ALL_CASES)


def exact_copy_bits(case, i):
    """float32 [C, H, W] of an exact-copy record: the source's values, cropped, flipped"""
    rec, (H, W) = case['records'][i], case['crop']
    v = case_images(case)[i][int(rec['dy']):int(rec['dy']) + H, int(rec['dx']):int(rec['dx']) + W].astype(np.float32)
    if rec['reflect_x']:
        v = v[:, ::-1]
    if rec['reflect_y']:
        v = v[::-1]
    return np.ascontiguousarray(np.transpose(v, (2, 0, 1)))


def decode_key(u):
    """the float of an order-preserving key (yolo3hip.h: key = sign ? ~bits : bits | 2^31)"""
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
RATIOS = {}          # (table, pass) -> (worst |error| / bound, case id, record, element (ch, y, x))
NORMAL_DEV = {}      # case id -> (worst |device normal - fp64 twin|, its resolution)


def worst_ratio(got, want, bound):
    """(max over elements of |got - want| / bound, its index); 0 / 0 = 0, x / 0 = inf; got must be finite"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), 'non-finite output'
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)
    k = int(np.argmax(ratio)) if ratio.size else 0
    return (float(ratio.flat[k]) if ratio.size else 0.0), tuple(int(v) for v in np.unravel_index(k, ratio.shape)) if ratio.size else ()


def check(table, name, case_id, rec_i, got, want, bound, fails=None):
    """|got - want| <= bound element by element; remembers the worst ratio per (table, pass).  With `fails` a miss is appended
    there (the caller asserts once, after every record of the batch has been looked at) instead of raised."""
    r, where = worst_ratio(got, want, bound)
    if r >= RATIOS.get((table, name), (-1.0,))[0]:
        RATIOS[(table, name)] = (r, case_id, rec_i, where)
    if r > 1.0:
        msg = '%s record %d %s: error / bound = %.3g at %s' % (case_id, rec_i, name, r, where)
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)
    return r
