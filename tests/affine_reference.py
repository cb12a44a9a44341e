"""Case tables and the error bound of the affine warp tests (tests/test_cpu_affine.py, tests/test_gpu_affine.py); the oracle itself
is yolo3.augment.affine_reference, the NumPy restatement of include/yolo3hip.h's y3_affine_batch.

The bound.  The kernel evaluates lerp(lerp(t00, t01, fx), lerp(t10, t11, fx), fy) with lerp(a, b, f) = (1 - f) * a + f * b in fp32,
every operation rounded on its own (csrc/augment.hip aff_lerp states the count): 1 - f (1 rounding), (1 - f) * a (1), f * b (1) and
the sum (1), so `a` goes through 3 roundings of one lerp and `b` through 2; the outer lerp adds 3 or 2 more.  The worst tap, t00,
carries K = 6 roundings, each a relative error of at most u = 2^-24 (round to nearest; the products of the cases below are far
from the subnormal range), so with the coordinates, floors and fractions reproduced bit for bit and the exact weights w_i formed
from those fractions,
    |out - sum_i w_i tap_i| <= ((1 + u)^6 - 1) sum_i |w_i tap_i| = 6 u (1 + O(u)) sum_i |w_i tap_i|.
The tests hold every element to K * 2^-24 * sum |w_i tap_i|: the first-order bound, the second-order term being 2.5 u = 1.5e-7 of
it.  A tap with weight exactly zero is not part of the sum and is never read; an element with one non-zero weight is compared as
bits.  Nothing here is tuned to what the kernel returns."""
import numpy as np

K_ROUNDINGS = 6
TILE = 32                     # Y3_AFF_TILE of csrc/augment.hip: the sizes below straddle it
CANARY_BYTES = 256
SPECIAL = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0x7f800001, 0xffc12345, 0x00000001, 0x00000000], np.uint32)

RATIOS = {}                   # case id -> (worst |error| / bound, where): filled by the GPU tests, written out under Y3_AFFINE_ERR


def bound(magnitude):
    """Per-element bound from affine_reference's magnitude = sum |w_i tap_i| (float64)."""
    return K_ROUNDINGS * 2.0 ** -24 * magnitude


def special_bits(rng, shape):
    """Random 32-bit patterns with -0.0, the infinities, quiet and signalling NaNs with payloads and a denormal sprinkled in."""
    x = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    flat = x.reshape(-1)
    idx = rng.integers(0, flat.size, max(1, flat.size // 5))
    flat[idx] = SPECIAL[rng.integers(0, len(SPECIAL), len(idx))]
    return x


def records(rows, fill=0.0):
    from yolo3 import augment
    r = np.zeros(len(rows), augment.AFFINE_RECORD)
    for i, row in enumerate(rows):
        r[i] = (np.asarray(row[:6], np.float32), row[6] if len(row) > 6 else fill, 0)
    return r


def exact_maps(h, w):
    """(name, six integer coefficients) of the maps that must be exact copies / permutations on an h x w image: the identity,
    integer shifts of both signs (one moves the whole image out), the two flips, the turns by 90, 180 and 270 degrees about the
    corner pixel grid (on a non-square image part of a quarter turn reads outside: `fill` there)."""
    return [('identity', (1, 0, 0, 0, 1, 0)),
            ('shift +3 +2', (1, 0, 3, 0, 1, 2)),
            ('shift -2 -5', (1, 0, -2, 0, 1, -5)),
            ('shift +1 -1', (1, 0, 1, 0, 1, -1)),
            ('shift out', (1, 0, w, 0, 1, -h)),
            ('flip x', (-1, 0, w - 1, 0, 1, 0)),
            ('flip y', (1, 0, 0, 0, -1, h - 1)),
            ('turn 90', (0, -1, w - 1, 1, 0, 0)),
            ('turn 180', (-1, 0, w - 1, 0, -1, h - 1)),
            ('turn 270', (0, 1, 0, -1, 0, h - 1))]


EXACT_SIZES = [(33, 33), (1, 1), (1, 40), (40, 1)]
GENERAL_SIZES = [(TILE - 1, TILE - 1), (TILE, TILE), (TILE + 1, TILE + 1), (2 * TILE + 1, 2 * TILE + 1), (TILE - 1, 2 * TILE + 1), (40, 72)]


def general_forward(h, w):
    """Forward matrices of the general cases on an h x w image: rotations up to 45 degrees, shear, gains 0.5 .. 1.5, sub-pixel
    translations, alone and combined."""
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0

    def make(deg=0.0, shx=0.0, shy=0.0, gain=1.0, tx=0.0, ty=0.0):
        a = np.deg2rad(deg)
        c = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1]], np.float64)
        r = gain * np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 0]]) + np.diag([0, 0, 1.0])
        s = np.array([[1, np.tan(np.deg2rad(shx)), 0], [np.tan(np.deg2rad(shy)), 1, 0], [0, 0, 1]], np.float64)
        t = np.array([[1, 0, cx + tx], [0, 1, cy + ty], [0, 0, 1]], np.float64)
        return t @ s @ r @ c
    return [make(deg=45), make(deg=-30, gain=0.5), make(deg=17, gain=1.5, tx=0.25, ty=-0.75), make(shx=12, shy=-7),
            make(tx=0.5, ty=0.5), make(tx=-3.125, ty=7.0625), make(deg=-45, shx=5, shy=5, gain=1.25, tx=-2.3, ty=1.7),
            make(gain=0.5, tx=1e-3), make(deg=3, shx=-2, gain=0.9, tx=0.1 * w, ty=-0.1 * h)]


def general_records(h, w, fill):
    from yolo3 import augment
    return np.concatenate([augment.affine_record(m, fill) for m in general_forward(h, w)])


def boundary_records(w):
    """Records whose sx is exactly -1, 0, w-1 and w for whole columns (the four fill boundaries in x), with sy at a half pixel so
    that two rows mix: sx = x + d for d in {-1 - 0, 0, ...} written as integer shifts, and the same with fx = 0.5 one column on."""
    rows = []
    for d in (-1.0, 0.0, float(w - 1), float(w), -0.5, w - 0.5):
        rows.append((1, 0, d, 0, 1, 0.5))            # column 0 reads sx = d
        rows.append((1, 0, d - (w - 1), 0, 1, -0.25))  # the last column reads sx = d
    return rows
