"""The plan forms of the kernel gradient (y3_conv2d_wgrad_x) and of the stride-2 data gradient (y3_conv2d_dgrad), one real layer per
form, and the inputs and fp64 references their tests share (host only: no GPU).  The companion of plan_forms.py, whose layer table,
envelope (batch 1-16 x image side 320-608), cost cap and tie-breaking order it imports.

ENTRY 'wgrad'.  plan_wgrad / plan_wgrad_x3 (csrc/conv_plan.cpp) choose from (m, cin, ksize, cout) the tile bkr x bn of the [K][cout] gradient
and cut the m = N*OH*OW pixels into `splits` runs of `chunk`; y3_conv2d_wgrad_plan_x reports {bkr, bn, splits, chunk, tiles, in_kernel,
grid, pixel_table}.  THE SIGNATURE of a kernel-gradient launch is

    ('wgrad', arithmetic, bkr, bn, reduction form, ksize, stride, K % bkr != 0, cout % bn != 0, m % chunk != 0, padded XCD grid)

arithmetic 'f32' / 'x3'; the reduction form one of test_gpu_wgrad.FORMS, here by short name:
    onerun      one pixel run (splits == 1), written straight to dw
    tickets     2 .. 8 runs, the last one of a tile to finish reduces inside the kernel
    slab-remap  more runs, < 32: natural-layout slabs + slab_reduce_kernel, work items remapped over the XCDs
    slab-xcd    >= 32 runs: the same on the XCD-strided grid; `padded XCD grid` = splits % 8 != 0, the grid is rounded up to a multiple
                of 8 runs and the blocks whose run index is >= splits return early
ksize and stride shape the tap-validity masks and the pixel table; the three ragged bits are a last K tile, column tile and pixel
run that are not full.  Members: all 23 layers, in both arithmetics where y3_conv2d_wgrad_x3_ok takes the shape.

Which tile / form combinations the planner cannot produce in the envelope (from plan_wgrad's text).  The f32 dispatch of
y3_conv2d_wgrad_x has six instantiations; plan_wgrad asks for 4096 waves, i.e. about 1024 / tiles runs of at least 128 pixels:
    64x32    K <= 64 and cout <= 32: the first layer (K = 36) and the 1x1 layer 64 -> 32.  One tile, and never fewer than 25 600
             pixels: always >= 200 runs, 'slab-xcd' only
    64x128   3x3 with 64 < K <= 576 and cout > 64: the layer 64 -> 128 alone; 9 tiles and >= 6400 pixels: 'slab-xcd' only
    128x128  what the measured overrides leave of it: the 3x3 layer 128 -> 256 (18 tiles: wants 57 runs) with >= 1600 pixels, so
             >= 13 runs: the two slab forms only, never 'onerun' or 'tickets'
    128x32 (the 14-channel heads), 64x64 (the other 1x1 layers), 128x64 (cout <= 64, or 3x3 with K * cout >= 2^20): all four forms
plan_wgrad_x3 has the 128x128 tile only, with all four forms.  test_cpu_grad_forms.py asserts that every tile, every form and every
(tile, form) pair that occurs in the envelope occurs among the representatives, per arithmetic, and prints the pairs.

ENTRY 'dgrad2'.  The stride-2 3x3 data gradient is cut into the four output-parity classes (4, 2, 2, 1 taps); describe_dgrad sends
them out as one merged launch (plan_dgrad_multi_f32: whole tiles; plan_dgrad_multi_x3: every class cut along K on its own) or, off
the fast path, one launch per class.  y3_conv2d_dgrad_plan_x reports it.  THE SIGNATURE is

    ('dgrad2', arithmetic, how, bm, bn, cut, short last slice, any class m % bm != 0, cin % bn != 0, per-class forms, unequal classes)

how = 'merged-f32' / 'merged-x3' / 'by-class'; cut = the tap counts of the classes that are cut along K, in launch order: () / (4,) /
(4, 2, 2) / (4, 2, 2, 1); short last slice = some cut class whose last slice is shorter than the others; per-class forms = the
plan_forms.split_form of every class for a 'by-class' launch (else ()); unequal classes = the parity classes differ in pixel count.
Members: the five stride-2 layers, with x3 where y3_conv2d_dgrad_x3_ok takes the shape.  Every envelope size is even, so there the
four classes are equal and SAME pad_before is 0; odd sizes are the only way to unequal classes and pad_before = 1.  The two
OFF_NETWORK shapes (from test_gpu_kernels.DGRAD_CASES) bring those in: classified by the same signature and listed NEXT TO the
envelope's representatives (off_network(), cases()), never instead of one.

representatives(entry) keeps, per signature, the member with the fewest multiply-adds whose fp64 reference fits the cost cap
(plan_forms.CAP_FLOP / CAP_BYTES; ties as plan_forms breaks them).  `python tests/grad_forms.py` prints the lists.
"""
import ctypes as C
import sys

import torch
import torch.nn.functional as F

import plan_forms as pf
from plan_forms import APP_A, BATCHES, SIDES, CAP_FLOP, CAP_BYTES, MAX_LEFT_OUT      # noqa: F401  (one definition for both modules)

if pf.ROOT not in sys.path:
    sys.path.insert(0, pf.ROOT)      # oracle.model.same_pad

ENTRIES = ('wgrad', 'dgrad2')
ARITHS = pf.ARITHS
WG_FORMS = ('onerun', 'tickets', 'slab-remap', 'slab-xcd')          # test_gpu_wgrad.FORMS, in that order
F32_WG_TILES = ((64, 32), (64, 64), (64, 128), (128, 32), (128, 64), (128, 128))      # the dispatch of y3_conv2d_wgrad_x
HOWS = ('single', 'merged-f32', 'merged-x3', 'by-class')            # out51[0] of y3_conv2d_dgrad_plan_x
OFF_NETWORK = [(1, 27, 31, 64, 64, 3, 2), (3, 30, 26, 128, 256, 3, 2)]      # from test_gpu_kernels.DGRAD_CASES: odd sizes

# operand layout of the tests (floats): the source a channel slice at an offset of a wider buffer, pitches beyond the channels
SRC_OFF, SRC_PAD, DST_PAD = 16, 16, 8
OFFSET = 0.5             # of the normal under the leaky-relu that makes the data


def src_ld(c):
    return SRC_OFF + (c + 3) // 4 * 4 + SRC_PAD


def dst_ld(c):
    return (c + 3) // 4 * 4 + DST_PAD


def _lib():
    from yolo3 import _hip
    return _hip


def wgrad_plan(m, cin, k, cout, flags):
    """y3_conv2d_wgrad_plan_x's eight numbers and the workspace bytes"""
    o = (C.c_int * 8)()
    ws = int(_lib().lib.y3_conv2d_wgrad_plan_x(m, cin, k, cout, flags, o))
    return list(o), ws


def wgrad_form(p):
    splits, in_kernel = p[2], p[5]
    if splits == 1:
        return WG_FORMS[0]
    if in_kernel:
        return WG_FORMS[1]
    return WG_FORMS[2] if splits < 32 else WG_FORMS[3]


def dgrad_plan(shape, flags, dd=None, ds=None):
    """y3_conv2d_dgrad_plan_x for the layer (n, h, w, cin, cout, k, s): (how, rows, per-class dicts, workspace bytes).  dd / ds: the
    tensors of a test (the pitches of its operands); by default the pitches the GPU test uses, with null data pointers."""
    hip = _lib()
    n, h, w, cin, cout, k, s = shape
    oh, ow = -(-h // s), -(-w // s)
    dd = dd or hip.Tensor(0, n, oh, ow, cout, src_ld(cout))
    ds = ds or hip.Tensor(0, n, h, w, cin, dst_ld(cin))
    o = (C.c_int * 51)()
    ws = int(hip.lib.y3_conv2d_dgrad_plan_x(dd, k, s, ds, flags, o))
    assert o[0] >= 0, 'y3_conv2d_dgrad_plan_x refuses %r' % (shape,)
    names = ('taps', 'm', 'bm', 'bn', 'tiles', 'f', 's0', 's1', 'chunk0', 'chunk1', 'nk', 'fast')
    cls = [dict(zip(names, o[3 + 12 * c:15 + 12 * c])) for c in range(o[1])]
    return HOWS[o[0]], o[2], cls, ws


def _class_plan13(c):
    """a class of y3_conv2d_dgrad_plan_x as the thirteen numbers plan_forms.split_form reads"""
    return [c['bm'], c['bn'], 16, c['tiles'], c['f'], c['s0'], c['s1'], c['chunk0'], c['chunk1'], 0, 0, c['fast'], c['nk']]


class Member(object):
    """One launch of the envelope with its layer: (n, h, w, cin) -> (n, oh, ow, cout)."""
    __slots__ = ('entry', 'arith', 'n', 'h', 'w', 'cin', 'cout', 'k', 's')

    def __init__(self, entry, arith, n, h, w, cin, cout, k, s):
        self.entry, self.arith, self.n, self.h, self.w, self.cin, self.cout, self.k, self.s = entry, arith, n, h, w, cin, cout, k, s

    @property
    def oh(self):
        return -(-self.h // self.s)

    @property
    def ow(self):
        return -(-self.w // self.s)

    @property
    def m(self):
        return self.n * self.oh * self.ow

    @property
    def flags(self):
        return _lib().CONV_X3 if self.arith == 'x3' else 0

    def shape(self):
        return (self.n, self.h, self.w, self.cin, self.cout, self.k, self.s)

    def macs(self):
        """multiply-adds of the one convolution the fp64 reference is"""
        return self.m * self.cin * self.k * self.k * self.cout

    def ref_flop(self):
        return 2.0 * self.macs()

    def ref_bytes(self):
        return 8 * self.n * max((self.h + 2) * (self.w + 2) * self.cin, self.oh * self.ow * self.cout)

    def within_cap(self):
        return self.ref_flop() <= CAP_FLOP and self.ref_bytes() <= CAP_BYTES

    def taken(self):
        """False where the x3 kernels refuse the shape"""
        if self.arith != 'x3':
            return True
        hip = _lib()
        if self.entry == 'wgrad':
            return bool(hip.lib.y3_conv2d_wgrad_x3_ok(self.m, self.cin, self.k, self.cout))
        return bool(hip.lib.y3_conv2d_dgrad_x3_ok(hip.Tensor(0, self.n, self.oh, self.ow, self.cout, src_ld(self.cout)), self.k, self.s,
                                                  hip.Tensor(0, self.n, self.h, self.w, self.cin, dst_ld(self.cin))))

    def plan(self):
        if self.entry == 'wgrad':
            return wgrad_plan(self.m, self.cin, self.k, self.cout, self.flags)
        return dgrad_plan(self.shape(), self.flags)

    def signature(self):
        if self.entry == 'wgrad':
            p, _ = self.plan()
            bkr, bn, splits, chunk = p[:4]
            K = self.k * self.k * self.cin
            return ('wgrad', self.arith, bkr, bn, wgrad_form(p), self.k, self.s, K % bkr != 0, self.cout % bn != 0, self.m % chunk != 0,
                    splits >= 32 and splits % 8 != 0)
        how, rows, cls, _ = self.plan()
        cut = tuple(c['taps'] for c in cls if c['s0'] > 1 or c['s1'] > 1)
        short = any(c['s0'] > 1 and c['nk'] - (c['s0'] - 1) * c['chunk0'] < c['chunk0'] for c in cls) if how != 'by-class' else False
        forms = tuple(pf.split_form(_class_plan13(c)) for c in cls) if how == 'by-class' else ()
        return ('dgrad2', self.arith, how, cls[0]['bm'], cls[0]['bn'], cut, short, any(c['m'] % c['bm'] != 0 for c in cls),
                self.cin % cls[0]['bn'] != 0, forms, len(set(c['m'] for c in cls)) > 1)

    def key(self):
        """the fixed order that breaks ties (plan_forms.Member.key)"""
        return (self.macs(), self.shape(), self.entry, self.arith)

    def id(self):
        return '%s-n%d_%dx%d_%d_%d_k%d_s%d' % ((sig_id(self.signature()),) + self.shape())

    def __repr__(self):
        return 'Member(%r, %r, %s)' % (self.entry, self.arith, ', '.join(str(v) for v in self.shape()))


def sig_id(sig):
    if sig[0] == 'wgrad':
        _, arith, bkr, bn, form, k, s, rk, rn, rm, pad = sig
        return 'wgrad-%s-%dx%d-%s-k%ds%d%s%s%s%s' % (arith, bkr, bn, form, k, s, '-raggedK' if rk else '', '-raggedN' if rn else '',
                                                     '-shortrun' if rm else '', '-padgrid' if pad else '')
    _, arith, how, bm, bn, cut, short, rm, rn, forms, uneq = sig
    return 'dgrad2-%s-%s-%dx%d-cut%s%s%s%s%s%s' % (arith, how.replace('-' + arith, ''), bm, bn, ''.join(str(t) for t in cut) or '0', '-shortK' if short else '',
                                                   '-raggedM' if rm else '', '-raggedN' if rn else '', ''.join('-' + f for f in forms),
                                                   '-unequal' if uneq else '')


def members_of(shapes, entry):
    """the launches `entry` makes for a list of layer shapes (n, h, w, cin, cout, k, s), in both arithmetics (x3 where it is taken)"""
    out = []
    for shape in shapes:
        if entry == 'dgrad2' and (shape[6] != 2 or shape[5] != 3):
            continue
        for arith in ARITHS:
            mb = Member(entry, arith, *shape)
            if mb.taken():
                out.append(mb)
    return out


_MEMO = {}


def envelope(entry):
    if entry not in _MEMO:
        _MEMO[entry] = members_of(pf.layer_shapes(), entry)
    return _MEMO[entry]


def off_network(entry):
    """the members outside the envelope that are listed next to its representatives, each under its own signature"""
    return [(mb.signature(), mb) for mb in members_of(OFF_NETWORK, entry)] if entry == 'dgrad2' else []


def classes(entry, members=None):
    """signature -> members, each list in the tie-breaking order"""
    by = {}
    for mb in envelope(entry) if members is None else members:
        by.setdefault(mb.signature(), []).append(mb)
    for v in by.values():
        v.sort(key=Member.key)
    return by


def representatives(entry):
    """(list of (signature, Member), list of left-out signatures): per class of the envelope the cheapest member within the cost cap.
    A class none of whose members fits the cap is left out BY NAME (the caller bounds how many).  cases(entry) adds off_network()."""
    reps, left = [], []
    for sig, mbs in sorted(classes(entry).items(), key=lambda kv: sig_id(kv[0])):
        fit = [mb for mb in mbs if mb.within_cap()]
        if fit:
            reps.append((sig, fit[0]))
        else:
            left.append(sig)
    return reps, left


def cases(entry):
    """what test_gpu_grad_forms.py runs: the representatives, then the off-network members"""
    return representatives(entry)[0] + off_network(entry)


def covered_by(shapes, entry):
    return set(mb.signature() for mb in members_of(shapes, entry))


def step_classes(side, n, entry):
    """the classes one training step of the network runs at this image side and batch"""
    return covered_by(pf.layer_shapes((n,), (side,)), entry)


# ---- the data and the fp64 references (CPU; shared by test_gpu_grad_forms.py and the sensitivity test) ----------------------------
def act(g, shape, alpha=0.1):
    """activation-like: leaky-relu of a normal plus OFFSET (a zero-mean input hides a wrong border tap or run boundary)"""
    return F.leaky_relu(torch.randn(shape, generator=g) + OFFSET, alpha)


def seed(shape):
    return sum(v * p for v, p in zip(shape, (7, 11, 13, 17, 19, 23, 29)))


def pad_same(x, k, s):
    from oracle.model import same_pad
    ph, pw = same_pad(x.shape[2], k, s), same_pad(x.shape[3], k, s)
    return F.pad(x, (pw[0], pw[1], ph[0], ph[1])), ph, pw


def wgrad_inputs(shape):
    """x [n, cin, h, w] and dy [n, cout, oh, ow] as test_gpu_wgrad._operands makes them"""
    n, h, w, cin, cout, k, s = shape
    g = torch.Generator().manual_seed(seed(shape) + 2)
    x = act(g, (n, cin, h, w))
    if cin == 4:
        x[:, 3] = 0                      # the RGB layer: channels padded 3 -> 4
    dy = act(g, (n, cout, -(-h // s), -(-w // s))) - 0.3
    return x, dy


def wgrad_reference(x, dy, k, s, dtype=torch.float64):
    """dw in the Keras layout [kh, kw, cin, cout]: ONE convolution, torch.nn.grad.conv2d_weight on the explicitly SAME-padded input"""
    xp, _, _ = pad_same(x.to(dtype), k, s)
    dw = torch.nn.grad.conv2d_weight(xp, (dy.shape[1], x.shape[1], k, k), dy.to(dtype), stride=s, padding=0)
    return dw.permute(2, 3, 1, 0).contiguous()


def wgrad_f32_banded(x, dy, k, s, rows=32):
    """The same in fp32 with an order of summation of its own over the pixels, whatever the library does inside a call: one fp32
    convolution per image and band of `rows` output rows, the bands added in fp32 in order."""
    xp, _, _ = pad_same(x, k, s)
    out = None
    for i in range(x.shape[0]):
        for r0 in range(0, dy.shape[2], rows):
            r1 = min(r0 + rows, dy.shape[2])
            d = torch.nn.grad.conv2d_weight(xp[i:i + 1, :, r0 * s:(r1 - 1) * s + k].contiguous(), (dy.shape[1], x.shape[1], k, k),
                                            dy[i:i + 1, :, r0:r1].contiguous(), stride=s, padding=0)
            out = d if out is None else out + d
    return out.permute(2, 3, 1, 0).contiguous()


def dgrad2_inputs(shape):
    """dy [n, cout, oh, ow], the Keras kernel [k, k, cin, cout], the destination's content for Y3_EPI_ACCUM, bn_a [n, h, w, cin]"""
    n, h, w, cin, cout, k, s = shape
    g = torch.Generator().manual_seed(seed(shape) + 3)
    dy = act(g, (n, cout, -(-h // s), -(-w // s)))
    wk = torch.randn(k, k, cin, cout, generator=g) * 0.1
    init = torch.randn(n, h, w, cin, generator=g)
    a = act(g, (n, h, w, cin), 0.2)
    return dy, wk, init, a


def dgrad2_reference(shape, dy, wk, dtype=torch.float64, drop_tap=None):
    """The data gradient [n, h, w, cin]: ONE convolution, torch.nn.grad.conv2d_input for the SAME-padded size with padding 0, the pad
    cropped.  drop_tap = (kh, kw): that tap's weights zeroed (the sensitivity test)."""
    n, h, w, cin, cout, k, s = shape
    from oracle.model import same_pad
    ph, pw = same_pad(h, k, s), same_pad(w, k, s)
    wo = wk.to(dtype).permute(3, 2, 0, 1).contiguous()
    if drop_tap is not None:
        wo[:, :, drop_tap[0], drop_tap[1]] = 0
    full = torch.nn.grad.conv2d_input((n, cin, h + ph[0] + ph[1], w + pw[0] + pw[1]), wo, dy.to(dtype), stride=s, padding=0)
    return full[:, :, ph[0]:ph[0] + h, pw[0]:pw[0] + w].permute(0, 2, 3, 1).contiguous()


if __name__ == '__main__':
    for entry in ENTRIES:
        reps, left = representatives(entry)
        for sig, mb in reps + off_network(entry):
            print('%-62s %-34s %6.1f GFLOP  plan %s' % (sig_id(sig), mb.shape(), mb.ref_flop() / 1e9, mb.plan()))
        print('%s: %d envelope launches, %d classes, %d representatives, left out: %s'
              % (entry, len(envelope(entry)), len(classes(entry)), len(reps), [sig_id(s) for s in left]))
