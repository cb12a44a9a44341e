"""The plan forms of y3_conv2d_fwd and the stride-1 y3_conv2d_dgrad, and one real layer per form (host only: no GPU).

plan_conv / plan_conv_x3 (csrc/conv_plan.cpp) decide per launch, from m = N*OH*OW, cin, ksize and cout, which kernel runs, on which
tile, and how the tiles are cut along K.  y3_conv2d_plan_x reports the decision as thirteen numbers
    {bm, bn, bk, tiles, f, s0, s1, chunk0, chunk1, grid, stats_tiles, fast, nk}
(include/yolo3hip.h): tiles [0, f) run s0 K slices of chunk0 steps, tiles [f, tiles) s1 slices of chunk1, nk steps in all.

THE SIGNATURE of a launch -- the one definition every user of this module shares -- is the tuple

    (entry, arithmetic, fast bit 0, bm, bn, split form, m % bm != 0, cout % bn != 0)

entry 'fwd' / 'dgrad', arithmetic 'f32' / 'x3', fast bit 0 = the MFMA kernel with split-K (0: the generic kernel), the last two:
a ragged last row tile / column tile (cout = the GEMM's output columns: the layer's cin for a data gradient).  Split form, with
`last` = nk - (s - 1) * chunk the length of the last slice of a tile cut into s slices of `chunk` steps:

    whole            no tile is cut (s0 == s1 == 1)
    uniform          every tile cut into the same s > 1 slices, last == chunk
    uniform-short    ... chunk / 3 < last < chunk
    uniform-third    ... last <= chunk / 3, dealt like any other slice (both planners produce them)
    overflow         ... last <= chunk / 3 and fast bit 1 set: the x3 "short-last overflow" plan, a few blocks more than workgroup
                     slots, the short slices dealt to the blocks dispatched last (conv_fast_decode<SHORTLAST>)
    mixed            two slice counts in one launch: 0 < f < tiles, s0 > 1
    remainder        whole rounds of 256 tiles stay whole, the remainder round is cut: s0 == 1, s1 > 1, last == chunk1
    remainder-short  ... last < chunk1

Which arithmetic can produce what (from the planners' text): plan_conv_x3 cuts a remainder round into EQUAL slices only
(`ch * S != nk` is skipped), so 'remainder-short' is f32-only; plan_conv gives one slice count to all tiles or cuts the remainder
round, never two counts, so 'mixed' is x3-only, and so is 'overflow' (short_last is set by plan_conv_x3 alone); the generic
kernel (fast bit 0 clear) and the 64-row and 32-column tiles (pick_tile) are f32-only: plan_conv_x3 has 128 x 128 and 128 x 64.

THE ENVELOPE: the 23 convolution shapes of the network (APP_A below: SURVEY.md Appendix A, sizes at 416 x 416) scaled to image
sides 320 / 416 / 512 / 608, at batch 1 / 2 / 4 / 8 / 16: the forward GEMM of every layer and the data-gradient GEMM of every
stride-1 layer but the first (nobody asks for the gradient of the image), in both arithmetics where y3_conv2d_x3_ok takes the
shape.  representatives() keeps, per signature, the member with the fewest multiply-adds whose fp64 reference fits the cost cap.
The list follows the planner: regenerate by calling representatives(); `python tests/plan_forms.py` prints it.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'object-detection-yolov3_amd') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))

# SURVEY.md Appendix A (hw at 416 x 416, cin as the kernels see it, cout, ksize, stride); the same table as test_gpu_kernels.APP_A,
# repeated so that this helper imports no test module (test_cpu_plan_forms.py asserts that the two tables are equal)
APP_A = [(416, 4, 32, 3, 1), (416, 32, 64, 3, 2), (208, 64, 32, 1, 1), (208, 32, 64, 3, 1), (208, 64, 128, 3, 2), (104, 128, 64, 1, 1),
         (104, 64, 128, 3, 1), (104, 128, 256, 3, 2), (52, 256, 128, 1, 1), (52, 128, 256, 3, 1), (52, 256, 512, 3, 2), (26, 512, 256, 1, 1),
         (26, 256, 512, 3, 1), (26, 512, 1024, 3, 2), (13, 1024, 512, 1, 1), (13, 512, 1024, 3, 1), (13, 512, 512, 1, 1), (26, 1024, 256, 1, 1),
         (26, 256, 256, 1, 1), (52, 512, 128, 1, 1), (13, 1024, 14, 1, 1), (26, 512, 14, 1, 1), (52, 256, 14, 1, 1)]
BATCHES = (1, 2, 4, 8, 16)
SIDES = (320, 416, 512, 608)
ARITHS = ('f32', 'x3')
ENTRIES = ('fwd', 'dgrad')
FORMS = ('whole', 'uniform', 'uniform-short', 'uniform-third', 'overflow', 'mixed', 'remainder', 'remainder-short')
F32_ONLY_FORMS = ('remainder-short',)
X3_ONLY_FORMS = ('mixed', 'overflow')
F32_TILES = ((64, 64), (64, 128), (128, 32), (128, 64), (128, 128))      # pick_tile
X3_TILES = ((128, 64), (128, 128))                                        # plan_conv_x3

# Cost cap of ONE case's fp64 CPU reference (a condition, not a measurement): 60 GFLOP (2 x multiply-adds of the convolution; the
# data gradient's reference is autograd's backward alone, torch.nn.grad.conv2d_input: one convolution) and 1 GiB for its largest
# fp64 tensor.
CAP_FLOP = 60e9
CAP_BYTES = 1 << 30
MAX_LEFT_OUT = 0.05       # at most this share of the classes may be left out, each by name, and only if no member fits the cap


def _lib():
    from yolo3 import _hip
    return _hip


def plan(m, cin, k, cout, flags):
    """y3_conv2d_plan_x's thirteen numbers and the workspace bytes"""
    o = (C.c_int * 13)()
    ws = int(_lib().lib.y3_conv2d_plan_x(m, cin, k, cout, flags, o))
    return list(o), ws


def split_form(p):
    bm, bn, bk, tiles, f, s0, s1, c0, c1, grid, stats, fast, nk = p
    if s0 > 1:
        if 0 < f < tiles and (s1 != s0 or c1 != c0):
            return 'mixed'
        last = nk - (s0 - 1) * c0
        assert 0 < last <= c0, p
        if fast & 2:
            assert 3 * last <= c0 and f == tiles, p
            return 'overflow'
        return 'uniform' if last == c0 else ('uniform-third' if 3 * last <= c0 else 'uniform-short')
    if s1 > 1 and f < tiles:
        last = nk - (s1 - 1) * c1
        assert 0 < last <= c1, p
        return 'remainder' if last == c1 else 'remainder-short'
    return 'whole'


def signature(entry, m, cin, k, cout, flags):
    """The class of the launch `entry` makes for an implicit GEMM of m rows, k*k*cin contracted, cout columns (a data gradient
    passes the layer's cout as cin and its cin as cout, as the entry point does).  None where y3_conv2d_x3_ok refuses x3."""
    hip = _lib()
    x3 = bool(flags & hip.CONV_X3)
    if x3 and not hip.lib.y3_conv2d_x3_ok(m, cin, k * k, cout):
        return None
    p, _ = plan(m, cin, k, cout, flags)
    return (entry, 'x3' if x3 else 'f32', p[11] & 1, p[0], p[1], split_form(p), m % p[0] != 0, cout % p[1] != 0)


def sig_id(sig):
    entry, arith, fast, bm, bn, form, rm, rn = sig
    return '%s-%s-%s%dx%d-%s%s%s' % (entry, arith, '' if fast else 'generic', bm, bn, form, '-raggedM' if rm else '', '-raggedN' if rn else '')


class Member(object):
    """One launch of the envelope with the layer geometry it came from: the layer maps (n, h, w, cin) -> (n, oh, ow, cout)."""
    __slots__ = ('entry', 'arith', 'n', 'h', 'w', 'cin', 'cout', 'k', 's')

    def __init__(self, entry, arith, n, h, w, cin, cout, k, s):
        self.entry, self.arith, self.n, self.h, self.w, self.cin, self.cout, self.k, self.s = entry, arith, n, h, w, cin, cout, k, s

    @property
    def oh(self):
        return -(-self.h // self.s)

    @property
    def ow(self):
        return -(-self.w // self.s)

    def gemm(self):
        """(m, cin, k, cout) as y3_conv2d_plan_x takes them"""
        if self.entry == 'fwd':
            return self.n * self.oh * self.ow, self.cin, self.k, self.cout
        return self.n * self.h * self.w, self.cout, self.k, self.cin

    def shape(self):
        return (self.n, self.h, self.w, self.cin, self.cout, self.k, self.s)

    def macs(self):
        m, c, k, nout = self.gemm()
        return m * c * k * k * nout

    def ref_flop(self):
        return 2.0 * self.macs()

    def ref_bytes(self):
        return 8 * self.n * max(self.h * self.w * self.cin, self.oh * self.ow * self.cout)

    def within_cap(self):
        return self.ref_flop() <= CAP_FLOP and self.ref_bytes() <= CAP_BYTES

    def signature(self):
        hip = _lib()
        return signature(self.entry, *self.gemm(), flags=hip.CONV_X3 if self.arith == 'x3' else 0)

    def key(self):
        """the fixed order that breaks ties"""
        return (self.macs(), self.shape(), self.entry, self.arith)

    def id(self):
        return '%s-n%d_%dx%d_%d_%d_k%d_s%d' % ((sig_id(self.signature()),) + self.shape())

    def __repr__(self):
        return 'Member(%r, %r, %s)' % (self.entry, self.arith, ', '.join(str(v) for v in self.shape()))


def layer_shapes(batches=BATCHES, sides=SIDES):
    """(n, h, w, cin, cout, k, s) of every layer shape at every batch / image side of the envelope"""
    out = []
    for side in sides:
        for n in batches:
            for hw, cin, cout, k, s in APP_A:
                assert hw * side % 416 == 0
                out.append((n, hw * side // 416, hw * side // 416, cin, cout, k, s))
    return out


def members_of(shapes, entries=ENTRIES):
    """the forward / stride-1 data-gradient launches of a list of layer shapes, in both arithmetics (x3 where it is taken)"""
    out = []
    for n, h, w, cin, cout, k, s in shapes:
        for entry in entries:
            if entry == 'dgrad' and (s != 1 or cin == 4):
                continue
            for arith in ARITHS:
                mb = Member(entry, arith, n, h, w, cin, cout, k, s)
                if mb.signature() is not None:
                    out.append(mb)
    return out


def envelope():
    return members_of(layer_shapes())


def classes(members=None):
    """signature -> members, each list in the tie-breaking order"""
    by = {}
    for mb in envelope() if members is None else members:
        by.setdefault(mb.signature(), []).append(mb)
    for v in by.values():
        v.sort(key=Member.key)
    return by


def representatives():
    """(list of (signature, Member), list of left-out signatures): per class the cheapest member within the cost cap.  A class
    none of whose envelope members fits the cap is left out BY NAME (the caller bounds how many)."""
    reps, left = [], []
    for sig, mbs in sorted(classes().items(), key=lambda kv: sig_id(kv[0])):
        fit = [mb for mb in mbs if mb.within_cap()]
        if fit:
            reps.append((sig, fit[0]))
        else:
            left.append(sig)
    return reps, left


def covered_by(shapes, entries=ENTRIES):
    """the classes a list of layer shapes (n, h, w, cin, cout, k, s) reaches through the given entry points"""
    return set(mb.signature() for mb in members_of(shapes, entries))


def step_classes(side, n, entries=ENTRIES):
    """the classes one step of the network (forward, and data gradient of every stride-1 layer) runs at this image side and batch"""
    return covered_by(layer_shapes((n,), (side,)), entries)


if __name__ == '__main__':
    reps, left = representatives()
    for sig, mb in reps:
        print('%-58s %-34s %6.1f GFLOP  plan %s' % (sig_id(sig), mb.shape(), mb.ref_flop() / 1e9, plan(*mb.gemm(), flags=4 if mb.arith == 'x3' else 0)[0]))
    print('%d envelope launches, %d classes, %d representatives, left out: %s' % (len(envelope()), len(classes()), len(reps), [sig_id(s) for s in left]))
