"""Case tables, comparison rules and the error bound of the photometric tests (tests/test_cpu_photometric.py,
tests/test_gpu_photometric.py); the oracle itself is yolo3.augment.photometric_reference, the NumPy restatement of
include/yolo3hip.h's y3_photometric_batch.

Exact stages.  The colour matrix, the clamp and the blend are fp32 operations in a stated order, which NumPy float32 repeats: the
device must return the restatement's words.  One freedom is left by IEEE 754: the payload (and sign) of a NaN that comes OUT of an
arithmetic operation.  same_words() therefore asks for equal words, or a NaN on both sides; the tests of pure copies (identity,
permutations) compare against the source words themselves, where a NaN must keep its payload.

The tone curve.  The kernel evaluates y = white * exp2f(g * log2f(s)), s = t / white (an IEEE division, which the float64 mode of
the restatement repeats in float32: s is the same word on both sides), s == 0 -> 0.  With relative errors e1 (log2f), e2 (the
product), e3 (exp2f) and e4 (the last product), each a few u = 2^-24,
    y_device = white * s^g * 2^(g log2(s) (e1 + e2)) * (1 + e3) (1 + e4)
so |y_device - y| <= (e3 + e4 + ln 2 * g |log2 s| (e1 + e2)) |y| to first order: the form (A + B g |log2 s|) u |y|.  A and B would
follow from the documented accuracy of exp2f / log2f; no such document for this target is at hand, so they are not invented: the
worst ratio |error| / ((1 + g |log2 s|) u |y|) was MEASURED on an MI355X over the sweep below (g in {0.5, 0.8, 1.25, 2}, t over
[0, white] with both ends, the smallest denormals and normals, a logarithmic and a linear ladder; white 255, 65535 and 1) and
A = B = TONE_K is four times that worst ratio (profiles/photometric_err.txt has both figures and the element).  The margin covers
inputs the sweep did not visit; the three kernel mutants of that file miss by orders of magnitude more.
Below the normal range fp32 has no relative accuracy: where exp2f's result is denormal its error is TONE_K denormal steps at
most by the same measure, which the product with white scales, and the product rounds once more, hence the floor
(TONE_K * white + 1) * 2^-149 added to the bound.  t = 0 and t = white are exact: s = 0 is answered 0 and log2f(1) = 0,
exp2f(0) = 1.
A mixed element is out = fl(fl(lambda a) + fl(rest b)): the bounds of a and b weighted by lambda and rest, plus one rounding of
each product and one of the sum, at most 2 u (|lambda a| + |rest b|).  The whole bound carries the factor (1 + 2^-20) for the
second-order terms dropped above."""
import itertools

import numpy as np

U = 2.0 ** -24
CHUNK = 16                    # Y3_PHO_CHUNK of csrc/augment.hip: output images per launch
CANARY_BYTES = 256
SPECIAL = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0x7f800001, 0xffc12345, 0x00000001, 0x00000000], np.uint32)
PERMUTATIONS = list(itertools.permutations(range(3)))
# A = B of the tone bound: four times the worst measured ratio, 1.72 (profiles/photometric_err.txt: gamma 1.25 deep in the
# logarithmic ladder, the same figure at all three whites).
TONE_MEASURED_WORST = 1.72
TONE_K = 4 * TONE_MEASURED_WORST
TONE_GAMMAS = (0.5, 0.8, 1.25, 2.0)
TONE_WHITES = (255.0, 65535.0, 1.0)

RATIOS = {}                   # case id -> (worst |error| / bound with K = 1, where): filled by the GPU tests, written under Y3_PHOTO_ERR


def special_bits(rng, shape):
    """Random 32-bit patterns with -0.0, the infinities, quiet and signalling NaNs with payloads and a denormal sprinkled in."""
    x = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    flat = x.reshape(-1)
    idx = rng.integers(0, flat.size, max(1, flat.size // 5))
    flat[idx] = SPECIAL[rng.integers(0, len(SPECIAL), len(idx))]
    return x


def records(n, **fields):
    """n identity records with the given fields overwritten (a scalar or one value per record)."""
    from yolo3 import augment
    r = augment.photo_identity_records(n)
    for k, v in fields.items():
        r[k] = np.asarray(v, r.dtype[k].base).reshape((-1,) + r.dtype[k].shape) if np.ndim(v) else v
    return r


def permutation_matrix(p):
    """Row k of the matrix takes channel p[k]: out[k] = in[p[k]]."""
    m = np.zeros((3, 3), np.float32)
    for k, j in enumerate(p):
        m[k, j] = 1
    return m.reshape(9)


def same_words(got, want):
    """uint32 arrays: equal words, or a NaN on both sides (the payload of an arithmetic NaN is the hardware's)."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    nan = lambda a: (a & 0x7fffffff) > 0x7f800000
    return (got == want) | (nan(got) & nan(want))


def tone_sweep(white):
    """float32 values t over [0, white]: both ends, the smallest denormals, the first normals, the values just inside the ends, a
    logarithmic ladder over the whole fp32 range below white and a linear one."""
    w = np.float32(white)
    tiny = np.array([0, 1, 2, 3, 7, 1 << 22, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, 1 << 24], np.uint32).view(np.float32)
    log = (w * np.exp2(-np.linspace(0, 160, 1500))).astype(np.float32)
    lin = (w * np.linspace(0, 1, 1500)).astype(np.float32)
    ends = np.array([np.nextafter(w, np.float32(0)), w, np.nextafter(np.float32(0), w)], np.float32)
    t = np.concatenate([tiny, log, lin, ends])
    return np.unique(t[t <= w])


def tone_bound(y, s, gamma, white, k=TONE_K):
    """Per-element bound of a finished tone-curve value: y float64 (exact), s the float32 quotient t / white, gamma and white
    broadcastable.  Elements with s == 0 or s == 1 have bound 0: they must be exact."""
    s = np.asarray(s, np.float64)
    with np.errstate(divide='ignore'):
        span = np.where(s > 0, np.abs(np.log2(np.where(s > 0, s, 1.0))), 0.0)
    rel = k * (1.0 + gamma * span) * U * np.abs(y)
    floor = (k * white + 1.0) * 2.0 ** -149
    return np.where((s == 0) | (s == 1), 0.0, (rel + floor) * (1 + 2.0 ** -20))


def blend_bound(lam, a, bound_a, b, bound_b):
    """Bound of fl(fl(lam a) + fl(rest b)), rest = fl(1 - lam), against lam a + rest b in float64."""
    lam = np.float32(lam)
    rest = np.float64(np.float32(1) - lam)
    lam = np.float64(lam)
    return (lam * bound_a + rest * bound_b + 2 * U * (np.abs(lam * a) + np.abs(rest * b))) * (1 + 2.0 ** -20)
