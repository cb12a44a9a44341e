"""The streaming kernels around the convolutions (csrc/pointwise.hip, and the two bf16 helpers at the end of csrc/conv_bf16.hip):
case tables, fp64 references and per-element error bounds.  Host only: this module imports no GPU code.
test_cpu_stream_kernels.py holds the tables and the bounds to what they claim; test_gpu_stream_kernels.py runs them.

WORKGROUP LAYOUT OF y3_bn_bwd_stats -- plan_bnb() below restates plan_bnb of pointwise.hip.  From (M, c):
    lc = min(c / 4, 8) float4 lanes per row (a power of two), sw = 4 lc channels per slice, slices = c / sw,
    rgn = 256 / lc row groups, trip = 4 rgn rows per trip, parts = min(cdiv(M, trip), max(1, 256 / slices)),
    rows_per_block = cdiv(M, parts); band p = rows [p rpb, min((p + 1) rpb, M)), possibly empty or starting past M.
Row group g of a band of L rows makes cdiv(L - g, trip) trips (0 if g >= L); the double-buffered loop leaves through a
different exit for 1, 2, odd >= 3 and even >= 4 trips.  Accepted channel counts: 4 / 8 / 16, or a multiple of 32 up to 1024.

ERROR BOUNDS.  Inputs are exact fp32 numbers, sums are formed in fp64, every output is rounded to fp32 once or a stated number
of times k.  U = 2^-24 is the unit roundoff of fp32 (U16 = 2^-8 of bf16); a chain of k roundings costs (1 + U)^k - 1 <
k U (1 + 2^-20) for k <= 32: ku(k).  SLACK = 1e-12 times the sum of ABSOLUTE addends of a channel covers the fp64 sums (their
order differs between kernel, reference and restatement) -- 1e-12 of the absolute sum is four orders below one fp32 rounding
of it, so it is what makes a bound on a cancelling quantity such as dbias mean something.  Nothing is measured against a
tensor-wide maximum: bounds are per channel for per-channel outputs, per element for tensors.  The count k stands next to
each bound with the roundings that give it.
"""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
U16 = 2.0 ** -8
SLACK = 1e-12
ALPHA = float(np.float32(0.1))       # the kernels take fp32 scalars: references use the same numbers
EPS = float(np.float32(1e-3))
MOM = float(np.float32(0.99))
GRID_CAP = 2048 * 256                # stream_blocks(): 2048 blocks of 256 threads, then a grid-stride loop
MAX_FLOATS = 6_000_000


def ku(k):
    return k * U * (1.0 + 2.0 ** -20)


def cdiv(a, b):
    return -(-a // b)


def seed_of(name):
    return zlib.crc32(name.encode())


# ------------------------------------------------------------------------------------------------------------------
# plan_bnb
# ------------------------------------------------------------------------------------------------------------------
def plan_bnb(M, c):
    """None if y3_bn_bwd_stats refuses c; else the layout (see the module docstring).  'ntrips' is per band that of row group
    0 (the most trips of the band), 'thread_ntrips' the set over all row groups of all bands."""
    if c < 4 or c > 1024 or c % 4:
        return None
    lc = min(c // 4, 8)
    if lc & (lc - 1):
        return None
    sw = 4 * lc
    if c % sw:
        return None
    slices = c // sw
    rgn = 256 // lc
    trip = 4 * rgn
    cap = max(1, 256 // slices)
    want_parts = cdiv(M, trip)
    parts = max(1, min(want_parts, cap))
    rpb = cdiv(M, parts)
    ntrips, threads, empty_last = [], set(), False
    for p in range(parts):
        r0 = p * rpb
        r1 = min(r0 + rpb, M)
        L = max(r1 - r0, 0)
        ntrips.append(cdiv(L, trip) if L > 0 else 0)
        for g in range(rgn):
            threads.add(cdiv(L - g, trip) if g < L else 0)
        if p == parts - 1:
            empty_last = r1 <= r0
    return dict(lc=lc, sw=sw, slices=slices, rgn=rgn, trip=trip, cap=cap, parts=parts, rows_per_block=rpb, ntrips=ntrips,
                thread_ntrips=threads, empty_last_band=empty_last, last_band_starts_past=(parts - 1) * rpb > M,
                parts_class='parts=1' if parts == 1 else ('parts=cap' if parts == cap and want_parts >= cap else 'parts<cap'),
                workspace=1024 + parts * c * 48)


def _nt_class(t):
    return 'ntrips>=5' if t >= 5 else 'ntrips=%d' % t


def bnb_classes(case):
    """every class a bn_bwd_stats case belongs to, computed from the plan (the case's own 'why' must be among them)"""
    M, c = case['M'], case['c']
    p = plan_bnb(M, c)
    out = {'lc=%d' % p['lc'], 'slices=%d' % p['slices'], p['parts_class']}
    out |= {'c%d:band-%s' % (c, _nt_class(t)) for t in p['ntrips'] if t > 0}
    out |= {'thread-%s' % _nt_class(t) for t in p['thread_ntrips']}
    if p['empty_last_band']:
        out.add('empty-last-band')
    if M == 1:
        out.add('M=1')
    if M == p['trip'] - 1:
        out.add('lc%d:M=trip-1' % p['lc'])
    if M == p['trip'] + 1:
        out.add('lc%d:M=trip+1' % p['lc'])
    pads, offs = case['pad'], case['off']
    out.add('view:sliced' if all(pads) and all(o and o % 4 == 0 for o in offs) else 'view:packed' if not any(pads) and not any(offs) else 'view:mixed')
    return out


def _bnb(M, c, why, pad=(8, 4, 12), off=(4, 8, 4)):
    """pad: ld - c of (dy, a, dres); off: start offset in floats of each view inside its buffer (a channel slice of a concat
    buffer starts inside a pixel)"""
    return dict(id='M%d-c%d' % (M, c), M=M, c=c, why=tuple(why), pad=tuple(pad), off=tuple(off))


# c = 32: trip 128, cap 256.  40000 rows: 254 bands of 157 (2 trips), one of 122 (1 trip), one EMPTY that starts past M.
# 65800: bands of 258 (3) and one of 10 (1).  132730: bands of 519 (5; row groups >= 7 make 4) and one of 385 (4).
# c = 1024: trip 128, cap 8.  1033: bands of 130 (2) and 123 (1).  2057: 258 (3) and 251 (2).  4105: 514 (5) and 507 (4).
BNB_CASES = [
    _bnb(1, 32, ['M=1', 'parts=1', 'lc=8', 'slices=1', 'view:sliced']),
    _bnb(1, 4, ['M=1', 'lc=1', 'view:packed'], pad=(0, 0, 0), off=(0, 0, 0)),
    _bnb(1023, 4, ['lc1:M=trip-1', 'lc=1', 'parts=1']),
    _bnb(1025, 4, ['lc1:M=trip+1', 'parts<cap']),
    _bnb(777, 8, ['lc=2']),
    _bnb(1500, 16, ['lc=4'], pad=(0, 0, 0), off=(0, 0, 0)),
    _bnb(127, 32, ['lc8:M=trip-1', 'c32:band-ntrips=1', 'thread-ntrips=1']),
    _bnb(129, 32, ['lc8:M=trip+1', 'parts<cap']),
    _bnb(40000, 32, ['empty-last-band', 'parts=cap', 'c32:band-ntrips=2', 'c32:band-ntrips=1', 'thread-ntrips=0', 'thread-ntrips=2']),
    _bnb(65800, 32, ['c32:band-ntrips=3', 'thread-ntrips=3']),
    _bnb(132730, 32, ['c32:band-ntrips>=5', 'c32:band-ntrips=4', 'thread-ntrips=4', 'thread-ntrips>=5']),
    _bnb(200, 96, ['slices=3', 'parts<cap']),
    _bnb(11000, 96, ['slices=3', 'parts=cap']),
    _bnb(9, 1024, ['slices=32', 'parts=1']),
    _bnb(1033, 1024, ['c1024:band-ntrips=2', 'c1024:band-ntrips=1', 'parts=cap']),
    _bnb(2057, 1024, ['c1024:band-ntrips=3'], pad=(0, 0, 0), off=(0, 0, 0)),
    _bnb(4105, 1024, ['c1024:band-ntrips>=5', 'c1024:band-ntrips=4']),
]
BNB_REQUIRED = (['lc=%d' % v for v in (1, 2, 4, 8)] + ['slices=%d' % v for v in (1, 3, 32)] + ['parts=1', 'parts<cap', 'parts=cap']
                + ['c%d:band-%s' % (c, t) for c in (32, 1024) for t in ('ntrips=1', 'ntrips=2', 'ntrips=3', 'ntrips=4', 'ntrips>=5')]
                + ['thread-ntrips=%d' % v for v in (0, 1, 2, 3, 4)] + ['thread-ntrips>=5']
                + ['empty-last-band', 'M=1', 'lc1:M=trip-1', 'lc1:M=trip+1', 'lc8:M=trip-1', 'lc8:M=trip+1', 'view:sliced', 'view:packed'])
BNB_DRES_MODES = ('none', 'overwrite', 'accumulate')        # every case runs all three on the GPU
BNB_REFUSED_C = (12, 20, 24, 40, 1056)

# rows 64 per tile (the last of 7): y3_bn_bwd_finalize_tiles is fed the moments of the SAME data as y3_bn_bwd_stats.  The data
# lie on a 1/64 grid inside [-4, 4): every 64-row moment is then exact in fp32 (products are multiples of 2^-12 below 16, 64
# of them below 2^10: 22 bits), so both kernels sum the same numbers and must agree within the sum of their bounds.
BNB_GRID_CASE = dict(id='grid-M327-c96', M=327, c=96, tile_rows=64, why=('finalize_tiles == stats',), pad=(8, 4, 12), off=(4, 8, 4))

BN_APPLY_CASES = [dict(id='M1-c4', M=1, c=4, pad=(0, 0, 0), off=(0, 0, 0), resid=False, why=('tiny',)),
                  dict(id='M333-c36', M=333, c=36, pad=(4, 8, 12), off=(4, 8, 12), resid=True, why=('sliced views', 'c % 32 != 0')),
                  dict(id='M66000-c32', M=66000, c=32, pad=(0, 8, 0), off=(0, 4, 0), resid=True, why=('second grid-stride trip',))]

# (tiles, c, rows per tile, moving statistics given); count = tiles * rows
STATS_FINALIZE_CASES = [dict(id='t%d-c%d-r%d-%s' % (t, c, r, 'mov' if mv else 'nomov'), tiles=t, c=c, rows=r, moving=mv, why=tuple(why))
                        for t, c, r, mv, why in [(1, 4, 1, True, ['tiles=1', 'c=4', 'count=1', 'moving']),
                                                 (2, 36, 5, True, ['tiles=2', 'c=36', 'constant-channel']),
                                                 (511, 4, 2, False, ['tiles=511', 'no-moving']),
                                                 (512, 36, 3, True, ['tiles=512']),
                                                 (513, 1024, 2, True, ['tiles=513', 'c=1024']),
                                                 (1025, 36, 2, False, ['tiles=1025', 'no-moving'])]]
STATS_FINALIZE_REQUIRED = ['tiles=%d' % t for t in (1, 2, 511, 512, 513, 1025)] + ['c=4', 'c=36', 'c=1024', 'count=1', 'moving', 'no-moving', 'constant-channel']
BWD_FINALIZE_CASES = [dict(id='t%d-c%d' % (t, c), tiles=t, c=c, rows=r, why=('tiles=%d' % t, 'c=%d' % c))
                      for t, c, r in [(1, 4, 3), (63, 36, 2), (64, 1024, 2), (65, 4, 2), (200, 36, 2), (200, 1024, 2)]]
BWD_FINALIZE_REQUIRED = ['tiles=%d' % t for t in (1, 63, 64, 65, 200)] + ['c=4', 'c=36', 'c=1024']

FOLD_LAYERS = (1, 3, 255, 256, 257, 1024)      # one table; the segments are scattered with NaN gaps between them

# (in c, out c, n, h, w, ld - out c of the output, start offset of the output view)
UPSAMPLE_CASES = [dict(id='%d-%d-n%d-%dx%d' % (ci, co, n, h, w), cin=ci, cout=co, n=n, h=h, w=w, pad=pad, off=off)
                  for ci, co, n, h, w, pad, off in [(4, 4, 1, 1, 1, 0, 0), (64, 128, 3, 3, 5, 128, 64), (256, 256, 1, 3, 5, 0, 0), (260, 8, 3, 1, 1, 8, 4),
                                                    (512, 512, 3, 3, 5, 4, 0), (1024, 4, 1, 3, 5, 12, 8)]]
UPSAMPLE_BF16_CASES = UPSAMPLE_CASES + [dict(id='%d-%d-n%d-%dx%d' % (ci, co, n, h, w), cin=ci, cout=co, n=n, h=h, w=w, pad=pad, off=off)
                                        for ci, co, n, h, w, pad, off in [(1, 1, 3, 3, 5, 0, 0), (65, 3, 1, 1, 1, 5, 3), (64, 64, 3, 3, 5, 64, 64)]]

# (pixels, c, ld - c of the source, of the destination)
COPY_CASES = [dict(id='M%d-c%d' % (m, c), M=m, c=c, spad=sp, dpad=dp, why=why)
              for m, c, sp, dp, why in [(3, 4, 0, 4, 'tiny'), (66000, 32, 0, 8, 'second grid-stride trip, pitches differ'), (515, 12, 4, 0, 'pitches differ')]]
# (n, c, h, w, channels of the NHWC side, its ld)
LAYOUT_CASES = [dict(id='n%d-c%d-%dx%d-to%d-ld%d' % (n, c, h, w, dc, ld), n=n, c=c, h=h, w=w, dc=dc, ld=ld, why=why)
                for n, c, h, w, dc, ld, why in [(2, 3, 6, 5, 4, 4, '3 into 4'), (3, 3, 5, 7, 8, 12, '3 into 8, ld > c'), (1, 3, 725, 725, 4, 4, 'past 524 288 pixels')]]
FILL_COUNTS = (0, 1, 255, 257, GRID_CAP + 3)
COLSUM_CASES = [dict(id='M%d-c%d-ld%d' % (m, c, ld), M=m, c=c, ld=ld) for m, c, ld in
                [(1, 1, 1), (1, 14, 16), (1023, 14, 16), (1024, 1, 1), (1024, 14, 14), (1025, 14, 16), (5000, 1, 4), (5000, 14, 16)]]
ZSCORE_COUNTS = (1, 255, 128 * 256 + 1)
ZSCORE_BRANCH_COUNT = 4096
F32_TO_BF16_RANDOM = 4096 * 256 + 77


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm + leaky-relu backward
# ------------------------------------------------------------------------------------------------------------------
_CENTRES = (0.0, 30.0, -3.0, 0.5, -30.0, 3.0, -1.0, 0.0)      # channel means of z in standard deviations
_DY_OFFS = (0.0, 2.0, -0.5, 0.0, 5.0)


def batch_stats(a32):
    """fp32 save_mean / save_rstd of an activation [M, c], as y3_bn_stats_finalize leaves them (fp64, rounded once)"""
    x = a32.double()
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean.float(), (1.0 / torch.sqrt(var + EPS)).float()


def bnb_data(M, c, seed, grid=False):
    """a = leaky_relu(z) and dy [M, c] fp32, gamma, save_mean, save_rstd [c] fp32.  Per channel: the scale of a is log-uniform
    over 1e-2 .. 1e2, its mean up to 30 standard deviations either side (all positive / all negative channels included), dy
    has a scale of its own (1e-3 .. 10) and a mean of up to 5 of its standard deviations (so dbias cancels), gamma is
    log-uniform over 1e-3 .. 1e3.  Some a are exactly +0.0 and some exactly -0.0 (the slope boundary)."""
    g = np.random.default_rng(seed)
    ch = np.arange(c)
    if grid:
        a = np.round(g.uniform(-4, 4, (M, c)) * 64) / 64
        a = np.clip(a, -4, 4 - 1 / 64).astype(np.float32)
        dy = np.clip(np.round(g.uniform(-4, 4, (M, c)) * 64) / 64, -4, 4 - 1 / 64).astype(np.float32)
    else:
        sig = 10.0 ** g.uniform(-2, 2, c)
        ctr = np.asarray(_CENTRES)[ch % len(_CENTRES)]
        z = sig * (g.standard_normal((M, c)) + ctr)
        a = np.where(z > 0, z, ALPHA * z).astype(np.float32)
        tsc = 10.0 ** g.uniform(-3, 1, c)
        dy = (tsc * (g.standard_normal((M, c)) + np.asarray(_DY_OFFS)[ch % len(_DY_OFFS)])).astype(np.float32)
    # the zeros go into the channels centred within 3 standard deviations (a zero in a channel 30 away would BE its variance)
    near = ch[np.abs(np.asarray(_CENTRES)[ch % len(_CENTRES)]) <= 3]
    k = max(1, (M * c) // 97)
    a[g.integers(0, M, k), g.choice(near, k)] = 0.0
    a[g.integers(0, M, k), g.choice(near, k)] = -0.0
    a[0, 0] = 0.0
    a[-1, -1] = -0.0
    gamma = (10.0 ** g.uniform(-3, 3, c)).astype(np.float32)
    a, dy, gamma = torch.from_numpy(a), torch.from_numpy(dy), torch.from_numpy(gamma)
    mu, r = batch_stats(a)
    return dict(a=a, dy=dy, gamma=gamma, mean=mu, rstd=r, M=M, c=c)


def bn_lrelu_autograd(a, dy, gamma, mean, rstd, alpha=ALPHA, resid=False):
    """fp64 torch autograd of y = BN(leaky_relu(z)) (+ resid) with the batch statistics the kernel is GIVEN: `mean` and `rstd`
    enter by value (they are fp32 numbers in the tests) while the gradient flows through them as through the batch mean and
    rsqrt(batch variance + eps) -- d mean / d a_i = 1 / M, d var / d a_i = 2 (a_i - mean) / M, d rstd / d var = -rstd^3 / 2.
    With the exact fp64 statistics this IS the literal layer (test_cpu_stream_kernels checks that).  z is recovered from a
    (a > 0 ? a : a / alpha), so dz goes through a = leaky_relu(z); torch gives the slope alpha at z = 0 and z = -0.
    Returns dz [M, c], dgamma, dbeta, dbias = sum dz [c] and dresid (or None), all fp64."""
    x = a.double()
    z = torch.where(x > 0, x, x / alpha).requires_grad_(True)
    ga = gamma.double().clone().requires_grad_(True)
    be = torch.zeros_like(ga).requires_grad_(True)
    res = torch.zeros_like(x).requires_grad_(True) if resid else None
    act = F.leaky_relu(z, alpha)
    m_ag = act.mean(0)
    mu = m_ag + (mean.double() - m_ag).detach()
    ve_ag = (act * act).mean(0) - mu * mu
    ve = ve_ag + (rstd.double() ** -2 - ve_ag).detach()
    y = (act - mu) * torch.rsqrt(ve) * ga + be
    if resid:
        y = y + res
    y.backward(dy.double())
    return z.grad, ga.grad, be.grad, z.grad.sum(0), (res.grad if resid else None)


def raw_moments(a, dy):
    """S [6, c] (the kernel's S0 .. S5: sum dy, dy a, dy [a > 0], a [a > 0], #[a > 0], a) and the same of absolute addends, fp64"""
    x, d = a.double(), dy.double()
    pos = (a > 0).double()
    S = torch.stack([d.sum(0), (d * x).sum(0), (d * pos).sum(0), (x * pos).sum(0), pos.sum(0), x.sum(0)])
    T = torch.stack([d.abs().sum(0), (d * x).abs().sum(0), (d.abs() * pos).sum(0), (x.abs() * pos).sum(0), pos.sum(0), x.abs().sum(0)])
    return S, T


def bnb_formula(S, T, gamma, mean, rstd, count, alpha=ALPHA):
    """dgamma, dbeta, dbias and k1, k2, k3 from the six sums, in fp64, and the per-channel bound of each:
    ku(1) |want| (ONE rounding: every one of them is formed in fp64 and stored as fp32) + SLACK * sum of absolute addends."""
    ga, mu, r, M = gamma.double(), mean.double(), rstd.double(), float(count)
    db = S[0]
    dg = r * (S[1] - mu * S[0])
    sdys = alpha * S[0] + (1 - alpha) * S[2]
    ss = alpha * M + (1 - alpha) * S[4]
    sxs = r * ((1 - alpha) * (S[3] - mu * S[4]) + alpha * (S[5] - mu * M))
    dbias = ga * r * (sdys - db / M * ss - dg / M * sxs)
    k1 = ga * r
    k2 = -ga * r * r * dg / M
    k3 = -ga * r * db / M - k2 * mu
    amu = mu.abs()
    t_db = T[0]
    t_dg = r * (T[1] + amu * T[0])
    t_sxs = r * ((1 - alpha) * (T[3] + amu * S[4]) + alpha * (T[5] + amu * M))
    t_dbias = ga.abs() * r * (alpha * T[0] + (1 - alpha) * T[2] + (db.abs() + t_db) / M * ss + (dg.abs() + t_dg) / M * t_sxs)
    t_k2 = ga.abs() * r * r * t_dg / M
    t_k3 = ga.abs() * r * t_db / M + amu * t_k2
    want = dict(dgamma=dg, dbeta=db, dbias=dbias, k1=k1, k2=k2, k3=k3)
    slack = dict(dgamma=t_dg, dbeta=t_db, dbias=t_dbias, k1=torch.zeros_like(k1), k2=t_k2, k3=t_k3)
    bound = {k: ku(1) * want[k].abs() + SLACK * slack[k] for k in want}
    return want, bound, slack


def dz_bound(a, dy, want, slack, alpha=ALPHA):
    """|dz error| per element.  The apply kernel forms ((k1 dy + k2 a) + k3) slope in fp32 from fp32 coefficients: the k1 dy
    term passes k = 5 roundings (coefficient, product, two adds, the multiply by the slope), the k2 a term the same five, k3
    three; 5 covers all (fused multiply-adds only remove roundings).  The slope scales what was rounded before it."""
    x, d = a.double(), dy.double()
    s = torch.where(a > 0, torch.ones_like(x), torch.full_like(x, alpha))
    return s * (ku(5) * ((want['k1'] * d).abs() + (want['k2'] * x).abs() + want['k3'].abs()) + SLACK * (x.abs() * slack['k2'] + slack['k3']))


@functools.lru_cache(maxsize=None)
def _bnb_case_cached(cid):
    case = {c['id']: c for c in BNB_CASES + [BNB_GRID_CASE]}[cid]
    d = bnb_data(case['M'], case['c'], seed_of(cid), grid=case is BNB_GRID_CASE)
    dz, dg, db, dbias, _ = bn_lrelu_autograd(d['a'], d['dy'], d['gamma'], d['mean'], d['rstd'])
    S, T = raw_moments(d['a'], d['dy'])
    fw, fb, slack = bnb_formula(S, T, d['gamma'], d['mean'], d['rstd'], case['M'])
    want = dict(fw, dgamma=dg, dbeta=db, dbias=dbias, dz=dz)        # the gradients from autograd, the coefficients from the formula
    bound = dict(fb)
    for k in ('dgamma', 'dbeta', 'dbias'):
        bound[k] = ku(1) * want[k].abs() + SLACK * slack[k]
    bound['dz'] = dz_bound(d['a'], d['dy'], fw, slack)
    return dict(d, want=want, bound=bound, formula=fw, S=S, T=T)


def bnb_case(case):
    """data, want and bound of a bn_bwd_stats case: computed once, shared, never modified by a test"""
    return _bnb_case_cached(case['id'])


def bnb_restate(d, alpha=ALPHA):
    """the kernels' arithmetic in numpy at the kernels' precision: fp64 sums and last-arrival formula, fp32 coefficients, fp32
    apply without fused multiply-adds"""
    S, T = raw_moments(d['a'], d['dy'])
    w, _, _ = bnb_formula(S, T, d['gamma'], d['mean'], d['rstd'], d['M'], alpha)
    out = {k: v.float() for k, v in w.items()}
    a, dy = d['a'], d['dy']
    s = torch.where(a > 0, torch.ones_like(a), torch.full_like(a, np.float32(alpha)))
    out['dz'] = ((out['k1'] * dy + out['k2'] * a) + out['k3']) * s
    return out


def tile_moments(a, dy, rows):
    """[tiles][6][c] fp32 partial moments of <= `rows` rows each, as the data-gradient epilogue leaves them"""
    parts = []
    for r0 in range(0, a.shape[0], rows):
        S, _ = raw_moments(a[r0:r0 + rows], dy[r0:r0 + rows])
        parts.append(S)
    return torch.stack(parts).float().contiguous()


def bwd_finalize_reference(partials, gamma, mean, rstd, count, alpha=ALPHA):
    """the formulas in fp64 over the fp32 partials the kernel reads"""
    P = partials.double()
    want, bound, _ = bnb_formula(P.sum(0), P.abs().sum(0), gamma, mean, rstd, count, alpha)
    return want, bound


@functools.lru_cache(maxsize=None)
def _bwd_finalize_cached(cid):
    case = {c['id']: c for c in BWD_FINALIZE_CASES}[cid]
    M = case['tiles'] * case['rows']
    d = bnb_data(M, case['c'], seed_of('bf' + cid))
    partials = tile_moments(d['a'], d['dy'], case['rows'])
    want, bound = bwd_finalize_reference(partials, d['gamma'], d['mean'], d['rstd'], M)
    return dict(partials=partials, gamma=d['gamma'], mean=d['mean'], rstd=d['rstd'], count=M, want=want, bound=bound)


def bwd_finalize_case(case):
    return _bwd_finalize_cached(case['id'])


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm training statistics, apply, inference fold
# ------------------------------------------------------------------------------------------------------------------
def stats_finalize_data(case):
    """[tiles][2][c] fp32 partials {sum a, sum a^2} of `rows` rows each, gamma / beta / moving statistics.  Channel 1 is
    CONSTANT (value 1.5) with sums of squares that came out 2^-18 low, as fp32 tile sums may: its variance is negative before
    the clamp.  With count = 1 every channel has variance 0 up to the rounding of a^2."""
    g = np.random.default_rng(seed_of('sf' + case['id']))
    t, c, r = case['tiles'], case['c'], case['rows']
    sig = 10.0 ** g.uniform(-2, 2, c)
    ctr = np.asarray(_CENTRES)[np.arange(c) % len(_CENTRES)] * sig
    m_t = ctr + sig * g.standard_normal((t, c)) / math.sqrt(r)
    q_t = sig ** 2 * g.uniform(0.5, 1.5, (t, c)) * (r > 1) + m_t ** 2
    S, Q = r * m_t, r * q_t
    if c > 1 and t * r > 1:
        S[:, 1] = r * 1.5
        Q[:, 1] = r * 2.25 * (1 - 2.0 ** -18)
    stats = torch.from_numpy(np.stack([S, Q], 1).astype(np.float32)).contiguous()
    gamma = torch.from_numpy((10.0 ** g.uniform(-3, 3, c)).astype(np.float32))
    beta = torch.from_numpy((g.standard_normal(c) * 10.0 ** g.uniform(-2, 2, c)).astype(np.float32))
    mm = torch.from_numpy((ctr * g.uniform(0.5, 1.5, c)).astype(np.float32))
    mv = torch.from_numpy((sig ** 2 * g.uniform(0.5, 1.5, c)).astype(np.float32))
    return dict(stats=stats, gamma=gamma, beta=beta, moving_mean=mm, moving_var=mv, count=t * r, use_moving=case['moving'])


def stats_finalize_reference(d, eps=EPS, mom=MOM):
    """mean, clamped biased variance, rstd, scale, shift and the moving statistics in fp64 over the fp32 partials, with bounds.
    The kernel sums in fp64 and then works in fp32:
      save_mean  k = 1 (the fp64 mean rounded)                                            + SLACK sum|partials| / count
      save_rstd  k = 1 (1 / sqrt(var + eps) in fp64, rounded); var = E2 - mean^2 cancels: + rstd^3 / 2 * SLACK (E|2| + mean^2)
      scale      k = 2 (rstd, gamma * rstd)
      shift      beta - fmean * scale: the product term passes k = 5 (fmean 1, scale 2, product 1, subtraction 1), beta k = 1
      moving_mean  mm * mom + fmean * (1 - mom): k = 4 on the second term (fmean, 1 - mom, product, add), 2 on the first
      moving_var   mv * mom + (float)(var * bessel) * (1 - mom): the same count; var carries its SLACK term"""
    P = d['stats'].double()
    n = float(d['count'])
    s, q = P[:, 0].sum(0), P[:, 1].sum(0)
    sa, qa = P[:, 0].abs().sum(0), P[:, 1].abs().sum(0)
    mean = s / n
    var = torch.clamp(q / n - mean * mean, min=0.0)
    t_mean = SLACK * sa / n
    t_var = SLACK * (qa / n + mean * mean) + 2 * mean.abs() * t_mean
    rstd = 1.0 / torch.sqrt(var + eps)
    t_rstd = 0.5 * rstd ** 3 * t_var
    ga, be = d['gamma'].double(), d['beta'].double()
    scale = ga * rstd
    shift = be - mean * scale
    bessel = n / (n - 1) if n > 1 else 1.0
    want = dict(save_mean=mean, save_rstd=rstd, scale=scale, shift=shift)
    bound = dict(save_mean=ku(1) * mean.abs() + t_mean, save_rstd=ku(1) * rstd + t_rstd, scale=ku(2) * scale.abs() + ga.abs() * t_rstd,
                 shift=ku(5) * (mean * scale).abs() + ku(1) * be.abs() + scale.abs() * t_mean + (mean * ga).abs() * t_rstd)
    if d.get('use_moving', True):
        mm, mv = d['moving_mean'].double(), d['moving_var'].double()
        want['moving_mean'] = mm * mom + mean * (1 - mom)
        want['moving_var'] = mv * mom + var * bessel * (1 - mom)
        bound['moving_mean'] = ku(2) * (mm * mom).abs() + ku(4) * (mean * (1 - mom)).abs() + (1 - mom) * t_mean
        bound['moving_var'] = ku(2) * (mv * mom).abs() + ku(4) * (var * bessel * (1 - mom)).abs() + (1 - mom) * bessel * t_var
    return want, bound, var


def stats_finalize_restate(d, eps=EPS, mom=MOM):
    """the kernel's arithmetic: fp64 sums, mean, variance and rstd; fp32 from there on"""
    P = d['stats'].double()
    n = float(d['count'])
    mean = P[:, 0].sum(0) / n
    var = torch.clamp(P[:, 1].sum(0) / n - mean * mean, min=0.0)
    rstd = (1.0 / torch.sqrt(var + eps)).float()
    fmean = mean.float()
    sc = d['gamma'] * rstd
    out = dict(save_mean=fmean, save_rstd=rstd, scale=sc, shift=d['beta'] - fmean * sc)
    bessel = n / (n - 1) if n > 1 else 1.0
    m32, om = torch.tensor(mom, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32) - torch.tensor(mom, dtype=torch.float32)
    out['moving_mean'] = d['moving_mean'] * m32 + fmean * om
    out['moving_var'] = d['moving_var'] * m32 + (var * bessel).float() * om
    return out


def bn_apply_data(case):
    g = np.random.default_rng(seed_of('ap' + case['id']))
    M, c = case['M'], case['c']
    sig = 10.0 ** g.uniform(-2, 2, c)
    ctr = np.asarray(_CENTRES)[np.arange(c) % len(_CENTRES)] * sig
    a = torch.from_numpy((ctr + sig * g.standard_normal((M, c))).astype(np.float32))
    scale = (10.0 ** g.uniform(-3, 3, c)) / sig * g.choice([-1.0, 1.0], c)
    shift = torch.from_numpy((-ctr * scale + g.standard_normal(c)).astype(np.float32))       # beta - mean * scale cancels
    resid = torch.from_numpy((g.standard_normal((M, c)) * 10.0 ** g.uniform(-2, 2, c)).astype(np.float32)) if case['resid'] else None
    return dict(a=a, scale=torch.from_numpy(scale.astype(np.float32)), shift=shift, resid=resid)


def bn_apply_reference(d):
    """y = a scale + shift (+ resid) in fp64; k = 3 roundings (product, add, residual add) of at most the sum of the absolute operands"""
    p = d['a'].double() * d['scale'].double()
    want = p + d['shift'].double()
    mag = p.abs() + d['shift'].double().abs()
    if d['resid'] is not None:
        want = want + d['resid'].double()
        mag = mag + d['resid'].double().abs()
    return want, ku(3) * mag


def bn_apply_restate(d):
    y = d['a'] * d['scale'] + d['shift']
    return y + d['resid'] if d['resid'] is not None else y


def fold_data():
    """one arena each for {gamma, beta}, {moving mean, moving var} and {scale, shift} with NaN between the layers' segments; the
    table rows {gamma, beta, mean, var, scale, shift (float offsets), C}"""
    g = np.random.default_rng(seed_of('fold'))
    rows, po, mo, co = [], 3, 5, 7
    for C in FOLD_LAYERS:
        rows.append([po, po + C + 2, mo + C + 1, mo, co + C + 3, co, C])      # beta behind gamma, mean behind var, shift before scale
        po, mo, co = po + 2 * C + 9, mo + 2 * C + 6, co + 2 * C + 11
    params, moving = np.full(po, np.nan, np.float32), np.full(mo, np.nan, np.float32)
    for r in rows:
        C = r[6]
        params[r[0]:r[0] + C] = 10.0 ** g.uniform(-3, 3, C) * g.choice([-1.0, 1.0], C)
        params[r[1]:r[1] + C] = g.standard_normal(C) * 10.0 ** g.uniform(-2, 2, C)
        moving[r[2]:r[2] + C] = g.standard_normal(C) * 10.0 ** g.uniform(-2, 2, C)
        v = 10.0 ** g.uniform(-4, 3, C)
        v[0] = 0.0
        moving[r[3]:r[3] + C] = v
    return dict(params=torch.from_numpy(params), moving=torch.from_numpy(moving), chan_len=co, table=torch.tensor(rows, dtype=torch.int32))


def fold_reference(gamma, beta, mean, var, eps=EPS):
    """scale = gamma / sqrt(var + eps), shift = beta - mean scale in fp64.  The kernel works in fp32 throughout:
    scale k = 4 (var + eps, sqrt, reciprocal, product); shift: the product term 4 + 1 (product) + 1 (subtraction) = 6, beta 1."""
    ga, be, mu, va = gamma.double(), beta.double(), mean.double(), var.double()
    sc = ga / torch.sqrt(va + eps)
    sh = be - mu * sc
    return dict(scale=sc, shift=sh), dict(scale=ku(4) * sc.abs(), shift=ku(6) * (mu * sc).abs() + ku(1) * be.abs())


def fold_restate(gamma, beta, mean, var, eps=EPS):
    sc = gamma * (torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32)))
    return dict(scale=sc, shift=beta - mean * sc)


# ------------------------------------------------------------------------------------------------------------------
# upsample
# ------------------------------------------------------------------------------------------------------------------
def upsample_data(case, bf16=False):
    """x [n, h, w, cin] and dout [n, 2h, 2w, cout]: per-channel scales 1e-2 .. 1e2 and both signs, so that a pixel's sum is
    small against the sum of its absolute addends"""
    g = np.random.default_rng(seed_of('up' + case['id']))
    n, h, w, ci, co = case['n'], case['h'], case['w'], case['cin'], case['cout']
    x = torch.from_numpy((g.standard_normal((n, h, w, ci)) * 10.0 ** g.uniform(-2, 2, ci)).astype(np.float32))
    dout = torch.from_numpy((g.standard_normal((n, 2 * h, 2 * w, co)) * 10.0 ** g.uniform(-2, 2, co)).astype(np.float32))
    if bf16:
        x = x.to(torch.bfloat16)
    return x, dout


def upsample_fwd_reference(x, cout, lanes_step=256, bf16=False):
    """conv_transpose2d with an all-ones [cin, cout, 2, 2] kernel, stride 2, fp64 -> [n, 2h, 2w, cout], and the bound per output.
    fp32 kernel: a value passes 2 adds inside its float4, ceil(C / 256) accumulations of its lane and the 6 levels of the wave sum:
    k = 6 + ceil(C / 256) + 2 roundings of at most sum|x| of the pixel.  bf16 kernel: one value per lane and trip, k = 6 +
    ceil(C / 64), then ONE bf16 rounding of the sum."""
    xd = x.double()
    ci = x.shape[-1]
    y = F.conv_transpose2d(xd.permute(0, 3, 1, 2), torch.ones(ci, cout, 2, 2, dtype=torch.float64), stride=2).permute(0, 2, 3, 1)
    mag = F.conv_transpose2d(xd.abs().permute(0, 3, 1, 2), torch.ones(ci, cout, 2, 2, dtype=torch.float64), stride=2).permute(0, 2, 3, 1)
    if bf16:
        b32 = ku(6 + cdiv(ci, 64)) * mag
        return y, b32 + U16 * (y.abs() + b32)
    return y, ku(6 + cdiv(ci, lanes_step) + 2) * mag


def upsample_bwd_reference(dout, cin):
    """the gradient of the same conv_transpose2d w.r.t. its input (torch autograd, fp64) -> [n, h, w, cin].  A lane adds
    4 * ceil(outC / 256) float4 sums (four output pixels): k = 6 + 4 ceil(outC / 256) + 2 roundings of at most sum|dout| of
    the four pixels."""
    n, h2, w2, co = dout.shape
    x = torch.zeros(n, cin, h2 // 2, w2 // 2, dtype=torch.float64, requires_grad=True)
    ones = torch.ones(cin, co, 2, 2, dtype=torch.float64)
    F.conv_transpose2d(x, ones, stride=2).backward(dout.double().permute(0, 3, 1, 2))
    mag = F.conv2d(dout.double().abs().permute(0, 3, 1, 2), torch.ones(cin, co, 2, 2, dtype=torch.float64), stride=2)
    return x.grad.permute(0, 2, 3, 1), ku(6 + 4 * cdiv(co, 256) + 2) * mag.permute(0, 2, 3, 1)


def _wave_tree(s):
    for k in (32, 16, 8, 4, 2, 1):
        s = s[..., :k] + s[..., k:2 * k]
    return s[..., 0]


def _lane_sums(v, width):
    """v [pix, C] fp32 -> [pix, 64]: the kernel's per-lane running sums (float4 lanes of 256 channels a trip, or single bf16
    values of 64 a trip), in fp32, in the kernel's order"""
    pix, C = v.shape
    step = 64 * width
    pad = cdiv(C, step) * step - C
    v = torch.cat([v, torch.zeros(pix, pad)], 1).view(pix, -1, 64, width)
    q = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3]) if width == 4 else v[..., 0]
    s = torch.zeros(pix, 64)
    for t in range(q.shape[1]):
        s = s + q[:, t]
    return s


def upsample_fwd_restate(x, cout, bf16=False):
    n, h, w, ci = x.shape
    s = _wave_tree(_lane_sums(x.float().reshape(-1, ci), 1 if bf16 else 4)).view(n, h, w)
    if bf16:
        s = s.to(torch.bfloat16)
    return s.repeat_interleave(2, 1).repeat_interleave(2, 2)[..., None].expand(-1, -1, -1, cout)


def upsample_bwd_restate(dout, cin):
    n, h2, w2, co = dout.shape
    s = torch.zeros(n * (h2 // 2) * (w2 // 2), 64)
    for a in range(2):
        for b in range(2):
            v = dout[:, a::2, b::2].reshape(-1, co)
            pad = cdiv(co, 256) * 256 - co
            v = torch.cat([v, torch.zeros(v.shape[0], pad)], 1).view(v.shape[0], -1, 64, 4)
            q = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
            for t in range(q.shape[1]):
                s = s + q[:, t]
    return _wave_tree(s).view(n, h2 // 2, w2 // 2, 1).expand(-1, -1, -1, cin)


# ------------------------------------------------------------------------------------------------------------------
# column sum, z-score, fp32 -> bf16
# ------------------------------------------------------------------------------------------------------------------
def colsum_data(case):
    g = np.random.default_rng(seed_of('cs' + case['id']))
    M, c = case['M'], case['c']
    return torch.from_numpy(((g.standard_normal((M, c)) + np.asarray(_DY_OFFS)[np.arange(c) % 5]) * 10.0 ** g.uniform(-2, 2, c)).astype(np.float32))


def colsum_reference(x):
    """k = 1: an fp64 sum rounded once"""
    want = x.double().sum(0)
    return want, ku(1) * want.abs() + SLACK * x.double().abs().sum(0)


def zscore_branch_images(count=ZSCORE_BRANCH_COUNT):
    """the five images of one launch, in this order: constant; +-1 checkerboard (mean 0, sd exactly 1: subtract only); the
    same x 4 (sd 4: divide); 16-bit range, mean ~ 60 000, sd ~ 3; sd ~ 0.25.  All values lie on a grid (integers, or multiples
    of 2^-10) on which the fp64 sums of x and x^2 are EXACT in any order, so mean and sd do not depend on the order of summation."""
    assert count % 2 == 0
    g = np.random.default_rng(seed_of('zs%d' % count))
    board = np.where(np.arange(count) % 2 == 0, 1.0, -1.0)
    imgs = [np.full(count, 7.25), board, 4 * board, np.round(60000 + 3 * g.standard_normal(count)), np.round(0.25 * g.standard_normal(count) * 1024) / 1024]
    return torch.from_numpy(np.stack(imgs).astype(np.float32))


def zscore_count_images(count):
    """three images of `count` values for the block-count edges: sd ~ 3 (divide), sd ~ 0.25 (subtract), constant"""
    g = np.random.default_rng(seed_of('zc%d' % count))
    if count == 1:
        return torch.tensor([[5.0], [-0.75], [0.0]])
    imgs = [np.round((10 + 3 * g.standard_normal(count)) * 64) / 64, np.round(0.25 * g.standard_normal(count) * 1024) / 1024, np.full(count, -3.5)]
    return torch.from_numpy(np.stack(imgs).astype(np.float32))


def zscore_reference(x):
    """The rule of imagereader.zscore_normalize_device: each image minus its whole-image mean, divided by its population
    standard deviation unless that is <= 1.  x [n, count] fp32 on a grid with exact fp64 sums (see zscore_branch_images).
    Returns want (fp64), bound, divide [n] (bool), sd (fp64) and `exact`: the fp32 bits of the subtract-only branch
    (x - (float)mean, one fp32 subtraction -- there is nothing else to round).
    Divide branch: mean and sd are rounded to fp32 (k = 1 each); the kernel forms the variance as E2 - mean^2 in fp64 from exact sums
    through 4 fp64 roundings of at most E2 + mean^2 (two quotients, the square, the difference): rel(sd) = U + 2^-53 * 4 (E2 +
    mean^2) / (2 var).  Then one subtraction and one division in fp32:
        |err| <= (U |mean| + U |x - mean|) / sd + |want| (U + rel(sd)),  all times (1 + 2^-10) for the second-order terms."""
    xd = x.double()
    n = xd.shape[1]
    mean = xd.sum(1) / n
    e2 = (xd * xd).sum(1) / n
    var = ((xd - mean[:, None]) ** 2).sum(1) / n          # centred: the reference itself does not cancel
    sd = torch.sqrt(var)
    divide = sd > 1.0
    div = torch.where(divide, sd, torch.ones_like(sd))
    want = (xd - mean[:, None]) / div[:, None]
    rel_sd = U + torch.where(divide, 2.0 ** -53 * 4 * (e2 + mean * mean) / (2 * var.clamp(min=1e-300)), torch.zeros_like(sd))
    bound = ((U * mean.abs())[:, None] + U * (xd - mean[:, None]).abs()) / div[:, None] + want.abs() * (U + rel_sd)[:, None]
    exact = x - mean.float()[:, None]
    return want, bound * (1 + 2.0 ** -10), divide, sd, exact


def zscore_restate(x):
    xd = x.double()
    n = xd.shape[1]
    mean = xd.sum(1) / n
    var = torch.clamp((xd * xd).sum(1) / n - mean * mean, min=0.0)
    mv, sd = mean.float(), torch.sqrt(var).float()
    sub = x - mv[:, None]
    return torch.where((sd <= 1.0)[:, None], sub, sub / sd[:, None])


# fp32 bit patterns for y3_f32_to_bf16, with what each is there for
BF16_TABLE = [(0x3f808000, 'tie, even below: down'), (0x3f818000, 'tie, odd below: up'), (0xbf808000, 'negative tie down'), (0xbf818000, 'negative tie up'),
              (0x3f807fff, 'just below a tie'), (0x3f808001, 'just above a tie'), (0x3f80ffff, 'rounds up across the fraction'), (0x3fffffff, 'carry into the exponent'),
              (0x00000000, '+0'), (0x80000000, '-0'), (0x7f800000, '+inf'), (0xff800000, '-inf'), (0x7fc00000, 'quiet NaN'), (0xffc00001, 'negative NaN'),
              (0x7f800001, 'signalling NaN with a low payload: must not become inf'), (0x00000001, 'smallest denormal'), (0x00008000, 'denormal tie to zero'),
              (0x00018000, 'denormal tie up'), (0x007fffff, 'largest denormal: rounds to the smallest normal'), (0x80008001, 'negative denormal just above a tie'),
              (0x7f7fffff, 'largest finite: rounds to +inf'), (0xff7fffff, 'most negative finite: rounds to -inf'), (0x7f7f7fff, 'largest that stays finite'),
              (0x7f7f8000, 'tie at the top: odd below, up to inf')]


def bf16_bits_rne(bits):
    """round-to-nearest-even of fp32 bit patterns (uint32 array) to bf16 bit patterns; NaN -> the quiet NaN 0x7fc0 | sign"""
    b = np.asarray(bits, np.uint64)
    nan = ((b & 0x7f800000) == 0x7f800000) & ((b & 0x007fffff) != 0)
    r = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    return np.where(nan, ((b >> 16) & 0x8000) | 0x7fc0, r).astype(np.uint16), nan


def f32_to_bf16_random():
    """4096 * 256 + 77 values (a second trip past the 4096-block cap): normal numbers of every magnitude, and every 16th a tie"""
    g = np.random.default_rng(seed_of('bf16'))
    x = (g.standard_normal(F32_TO_BF16_RANDOM) * 10.0 ** g.uniform(-30, 30, F32_TO_BF16_RANDOM)).astype(np.float32)
    b = x.view(np.uint32)
    b[::16] = (b[::16] & 0xffff0000) | 0x8000
    return torch.from_numpy(b.view(np.float32).copy())


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, want, bound):
    """max over elements of |got - want| / bound (0 / 0 = 0, x / 0 = inf); got must be finite"""
    got, want, bound = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double(), torch.as_tensor(bound).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), 'non-finite output'
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err))      # x / 0 = inf
    return float(ratio.max())


RATIOS = {}


def check(entry, case_id, name, got, want, bound):
    """assert |got - want| <= bound element by element; remember the worst ratio per (entry, case, output)"""
    r = worst_ratio(got, want, bound)
    RATIOS[(entry, case_id, name)] = max(r, RATIOS.get((entry, case_id, name), 0.0))
    assert r <= 1.0, '%s %s %s: error / bound = %.3g' % (entry, case_id, name, r)
    return r
