"""The kernel routes of y3_conv2d_fwd_bf16_ws, and one real layer of the inference plan per route class (host only: no GPU).

describe_bf16 (csrc/conv_bf16.hip) ends in an if-chain that picks, per launch, one of nine routes -- the 256 x 256
ping-pong kernel, the 32 -> 64 patch kernel (stride x residual: four instantiations), the 64 -> 128 patch kernel (stride: two), the
LDS-DMA ring kernel on five tiles, split along K on the 64 x 64 one -- from the shape, the flags (Y3_BF16_NO_PATCH, which
yolo3/model.py sets from its 300 MB traffic rule), alpha and the alignment of its operands.  y3_conv2d_fwd_bf16_plan reports
the description the entry point launches from as twelve numbers
    {route, bm, bn, bk, grid, threads, splits, chunk, vec_ok, patch stride, patch residual, nk}
(include/yolo3hip.h).

THE SIGNATURE of a launch, taken from the query alone (and from m, cout, the output type it was asked with):

    (route, bm, bn, bk, patch instantiation (stride, residual) or None, split form, m % bm != 0, cout % bn != 0, fp32 out, vec_ok)

split form: 'whole' (one K slice per tile), 'uniform' (splits > 1, every slice `chunk` steps), 'short-last' (the last slice,
nk - (splits - 1) * chunk steps, is shorter).

THE ENVELOPE: every bf16 conv launch of the inference plan -- layers 2..75 of the network and its three heads, with the arguments
yolo3/model.py passes: the residual of the layer, the pitches of the two concat buffers, fp32 output for the heads, the
Y3_BF16_NO_PATCH flag of the 300 MB rule (restated in `no_patch`; test_gpu_model.py holds the restatement to the model's own
launch list), a workspace of y3_conv2d_fwd_bf16_workspace bytes -- at the image sides and batches of plan_forms and at 10 / 25 / 45
tiles of 608^2 (the batches the tiled path plans), with heads of 14 and of 255 channels.  representatives() keeps, per signature,
the member with the fewest multiply-adds.

THE REFERENCE of a member is an fp64 convolution of at most four of its images (convolution is independent per image): the
first, the last and an adjacent middle pair, so that a row tile that straddles two images is always among them.  plan_forms' cost
cap applies to that subset, and no class may be left out (MAX_LEFT_OUT = 0: the costliest single image of any layer at side 608
is about 3.5 GFLOP).  `python tests/bf16_routes.py` prints the list.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'object-detection-yolov3_amd') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))

from plan_forms import BATCHES, CAP_BYTES, CAP_FLOP, SIDES      # noqa: E402  (the envelope's sizes and the cost cap are plan_forms')

TILE_BATCHES = (10, 25, 45)        # tiles of 608^2 per launch of the tiled path (4096^2 image: 100 tiles as [45, 45, 10]; 25: a 2 x 2 split)
TILE_SIDE = 608
HEADS = (14, 255)                  # 2 anchors x (5 + 2) as in APP_A, and 3 x 85 (the COCO head)
MAX_LEFT_OUT = 0                   # a condition: every class has a member whose subset reference fits the cap
SUBSET = 4                         # images of a member that get an fp64 reference
FILTERS = 1024                     # YoloV3.FILTER_COUNT
BLOCKS = 8                         # YoloV3.BLOCK_COUNT
LRELU_ALPHA = 0.2
SPLIT_FORMS = ('whole', 'uniform', 'short-last')
RING_TILES = ((128, 32), (128, 64), (256, 128), (128, 128), (64, 64))
BIG_TILES = ((256, 256), (256, 128), (128, 128))
FAKE = 0x10000                     # a 16-byte aligned address for the query (never dereferenced)
OUT_NAMES = ('route', 'bm', 'bn', 'bk', 'grid', 'threads', 'splits', 'chunk', 'vec_ok', 'patch_stride', 'patch_resid', 'nk')


def _lib():
    from yolo3 import _hip
    return _hip


def route_names():
    hip = _lib()
    return {hip.BF16_ROUTE_PP: 'pp', hip.BF16_ROUTE_C32: 'c32', hip.BF16_ROUTE_C64: 'c64', hip.BF16_ROUTE_RING: 'ring'}


def no_patch(m, cin, cout, s, resid):
    """yolo3/model.py's rule, restated: a conv layer that moves less than BF16_PATCH_MIN_BYTES (input + residual + output, bf16)
    stays off the patch kernels.  m = n * oh * ow output pixels, each reading s * s input pixels' worth of the source."""
    from yolo3.model import BF16_PATCH_MIN_BYTES
    moved = 2 * m * (s * s * cin + cout * (2 if resid else 1))
    return moved < BF16_PATCH_MIN_BYTES


def network(head):
    """The bf16 conv launches of one forward pass in emission order, as
    (down, cin, cout, k, s, resid, src_ld, dst_ld, head): the input is side / down pixels square, `resid` says whether the layer
    adds the input of its feature block, src_ld / dst_ld are the pitches (the last layer of the 256- and 512-channel stages
    writes, and the layers after them read, one half of a concat buffer), head: a detection head (linear, no BatchNorm, fp32
    output with a pitch rounded up to 4).  The RGB layer (y3_conv2d_first_bf16) is not among them."""
    out = []

    def conv(t, cout, k, s=1, resid=False, dst_ld=None):
        down, c, ld = t
        out.append((down, c, cout, k, s, resid, ld, dst_ld or cout, False))
        return (down * s, cout, dst_ld or cout)

    def feature_block(t, reps, last_ld=None):
        c = t[1]
        x = t
        for r in range(reps):
            x = conv(x, c // 2, 1)
            x = conv(x, c, 3, resid=True, dst_ld=last_ld if r == reps - 1 else None)
        return x

    def yolo_block(t, fc):
        for i in range(5):
            t = conv(t, fc if i % 2 else fc // 2, 3 if i % 2 else 1)
        x = conv(t, fc, 3)
        out.append((x[0], fc, head, 1, 1, False, fc, (head + 3) // 4 * 4, True))
        return t

    FC = FILTERS
    x = (1, FC // 32, FC // 32)                 # what the RGB layer leaves
    x = conv(x, FC // 16, 3, 2)
    x = feature_block(x, 1)
    x = conv(x, FC // 8, 3, 2)
    x = feature_block(x, 2)
    x = conv(x, FC // 4, 3, 2)
    x = feature_block(x, BLOCKS, last_ld=FC // 2)       # into the second half of cat3
    x = conv(x, FC // 2, 3, 2)
    x = feature_block(x, BLOCKS, last_ld=FC)            # into the second half of cat2
    x = conv(x, FC, 3, 2)
    x = feature_block(x, BLOCKS // 2)
    route = yolo_block(x, FC)
    conv(route, FC // 2, 1)                             # (its upsampled copy is the first half of cat2)
    route = yolo_block((16, FC, FC), FC // 2)
    conv(route, FC // 4, 1)
    yolo_block((8, FC // 2, FC // 2), FC // 4)
    return out


class Member(object):
    """One bf16 conv launch of the envelope: (n, h, w, cin) -> (n, oh, ow, cout) with the arguments the model passes."""
    __slots__ = ('n', 'h', 'w', 'cin', 'cout', 'k', 's', 'resid', 'head', 'src_ld', 'dst_ld', 'flags', '_plan')

    def __init__(self, n, h, w, cin, cout, k, s, resid, head, src_ld=None, dst_ld=None, flags=None):
        hip = _lib()
        self.n, self.h, self.w, self.cin, self.cout, self.k, self.s, self.resid, self.head = n, h, w, cin, cout, k, s, bool(resid), bool(head)
        self.src_ld = src_ld or cin
        self.dst_ld = dst_ld or ((cout + 3) // 4 * 4 if head else cout)
        if flags is None:
            flags = 0 if head else hip.EPI_LRELU | (hip.BF16_NO_PATCH if no_patch(self.m, cin, cout, s, resid) else 0)
        self.flags = flags
        self._plan = None

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
    def out_f32(self):
        return self.head

    @property
    def alpha(self):
        return 0.0 if self.head else LRELU_ALPHA

    def shape(self):
        return (self.n, self.h, self.w, self.cin, self.cout, self.k, self.s)

    def args(self):
        return self.shape() + (self.resid, self.head, self.src_ld, self.dst_ld, self.flags)

    def workspace_bytes(self):
        return int(_lib().lib.y3_conv2d_fwd_bf16_workspace(self.m, self.cin, self.k, self.cout))

    def plan(self):
        """(the query's twelve numbers, the workspace bytes the launch would use), with pointers that are aligned as the
        model's are"""
        if self._plan is None:
            self._plan = plan(self.n, self.h, self.w, self.cin, self.cout, self.k, self.s, resid=self.resid, out_f32=self.out_f32, flags=self.flags,
                              alpha=self.alpha, affine=not self.head, src_ld=self.src_ld, dst_ld=self.dst_ld, ws_bytes=self.workspace_bytes())
        return self._plan

    def signature(self):
        return signature(self.plan()[0], self.m, self.cout, self.out_f32)

    def macs(self):
        return self.m * self.cin * self.k * self.k * self.cout

    def subset(self):
        """the images that get an fp64 reference: all of up to SUBSET, else the first, an adjacent middle pair, the last"""
        if self.n <= SUBSET:
            return list(range(self.n))
        return [0, self.n // 2 - 1, self.n // 2, self.n - 1]

    def ref_flop(self):
        return 2.0 * self.macs() / self.n * len(self.subset())

    def ref_bytes(self):
        return 8 * len(self.subset()) * max(self.h * self.w * self.cin, self.oh * self.ow * self.cout)

    def within_cap(self):
        return self.ref_flop() <= CAP_FLOP and self.ref_bytes() <= CAP_BYTES

    def key(self):
        """the fixed order that breaks ties"""
        return (self.macs(),) + self.args()

    def id(self):
        return '%s-n%d_%dx%d_%d_%d_k%d_s%d' % ((sig_id(self.signature()),) + self.shape())

    def __repr__(self):
        return 'Member(%s)' % ', '.join(str(v) for v in self.args())


def plan(n, h, w, cin, cout, k, s, resid=False, out_f32=False, flags=0, alpha=LRELU_ALPHA, affine=True, bias=True, src_ld=None, dst_ld=None,
         resid_ld=None, ws_bytes=0, dst_ptr=FAKE, resid_ptr=FAKE, wt_ptr=FAKE):
    """y3_conv2d_fwd_bf16_plan for a launch described by its geometry; pointers are made-up addresses (the query reads their
    alignment and null-ness only).  Returns (the twelve numbers, workspace bytes used); a refused launch has route 0."""
    hip = _lib()
    oh, ow = -(-h // s), -(-w // s)
    src = hip.Tensor(FAKE, n, h, w, cin, src_ld or cin)
    dst = hip.Tensor(dst_ptr, n, oh, ow, cout, dst_ld or cout)
    res = hip.Tensor(resid_ptr, n, oh, ow, cout, resid_ld or cout) if resid else None
    o = (C.c_int * 12)()
    used = int(hip.lib.y3_conv2d_fwd_bf16_plan(src, wt_ptr, FAKE if bias else None, k, s, dst, int(out_f32), flags, alpha, FAKE if affine else None,
                                               FAKE if affine else None, res, FAKE if ws_bytes else None, ws_bytes, o))
    return list(o), used


def split_form(p):
    splits, chunk, nk = p[6], p[7], p[11]
    if splits == 1:
        return 'whole'
    last = nk - (splits - 1) * chunk
    assert 0 < last <= chunk, p
    return 'uniform' if last == chunk else 'short-last'


def signature(p, m, cout, out_f32):
    hip = _lib()
    assert p[0] in route_names(), 'the entry point refuses this launch: %s' % hip.lib.y3_last_error()
    patch = (p[9], p[10]) if p[0] in (hip.BF16_ROUTE_C32, hip.BF16_ROUTE_C64) else None
    return (p[0], p[1], p[2], p[3], patch, split_form(p), m % p[1] != 0, cout % p[2] != 0, bool(out_f32), p[8])


def sig_id(sig):
    route, bm, bn, bk, patch, form, rm, rn, f32, vec = sig
    return '%s%dx%dk%d%s-%s%s%s%s%s' % (route_names()[route], bm, bn, bk, '-s%d%s' % (patch[0], 'r' if patch[1] else '') if patch else '', form,
                                      '-raggedM' if rm else '', '-raggedN' if rn else '', '-f32' if f32 else '', '' if vec else '-novec')


def launches(side, n, head):
    """the Members of one forward pass at this image side and batch, in emission order"""
    out = []
    for down, cin, cout, k, s, resid, src_ld, dst_ld, is_head in network(head):
        assert side % 32 == 0
        out.append(Member(n, side // down, side // down, cin, cout, k, s, resid, is_head, src_ld, dst_ld))
    return out


def sizes():
    return [(side, n) for side in SIDES for n in BATCHES] + [(TILE_SIDE, n) for n in TILE_BATCHES]


_ENVELOPE = []


def envelope():
    if not _ENVELOPE:
        seen = {}
        for side, n in sizes():
            for head in HEADS:
                for mb in launches(side, n, head):
                    seen.setdefault(mb.args(), mb)
        _ENVELOPE.extend(seen.values())
    return list(_ENVELOPE)


def classes(members=None):
    """signature -> members, each list in the tie-breaking order"""
    by = {}
    for mb in envelope() if members is None else members:
        by.setdefault(mb.signature(), []).append(mb)
    for v in by.values():
        v.sort(key=Member.key)
    return by


def representatives():
    """(list of (signature, Member), list of left-out signatures): per class the member with the fewest multiply-adds; a class
    whose cheapest member's subset reference does not fit the cap is left out by name (MAX_LEFT_OUT: none may be)."""
    reps, left = [], []
    for sig, mbs in sorted(classes().items(), key=lambda kv: sig_id(kv[0])):
        if mbs[0].within_cap():
            reps.append((sig, mbs[0]))
        else:
            left.append(sig)
    return reps, left


def extra_members():
    """The two 32 -> 64 patch instantiations NO layer of the network launches -- its stride-1 32 -> 64 layer always adds a residual,
    its stride-2 one never does -- at the geometry of those two layers (10 tiles of 608^2), so that all six instantiations the
    library compiles are held to fp64: (signature, Member) like representatives()."""
    hip = _lib()
    out = []
    for h, s, resid in ((304, 1, False), (608, 2, True)):
        mb = Member(10, h, h, 32, 64, 3, s, resid, False, flags=hip.EPI_LRELU)
        out.append((mb.signature(), mb))
    return out


def covered_by(cases):
    """the classes a list of (n, h, w, cin, cout, k, s, resid, out_f32) launches reaches when it is launched the way
    test_gpu_kernels.test_conv_fwd_bf16 launches it (leaky-relu, bias, scale / shift, aligned rows, never Y3_BF16_NO_PATCH)"""
    hip = _lib()
    out = set()
    for n, h, w, cin, cout, k, s, resid, f32 in cases:
        oh, ow = -(-h // s), -(-w // s)
        wsb = int(hip.lib.y3_conv2d_fwd_bf16_workspace(n * oh * ow, cin, k, cout))
        p, _ = plan(n, h, w, cin, cout, k, s, resid=resid, out_f32=f32, flags=hip.EPI_LRELU, src_ld=cin + 8, dst_ld=(cout + 7) // 8 * 8 + 8, ws_bytes=wsb)
        out.add(signature(p, n * oh * ow, cout, f32))
    return out


def forward_classes(side, n, head=HEADS[0]):
    return set(mb.signature() for mb in launches(side, n, head))


def predicted_routes(side, n, head):
    """[(route, flags)] of the bf16 conv launches of one forward pass, in emission order"""
    return [(mb.plan()[0][0], mb.flags) for mb in launches(side, n, head)]


if __name__ == '__main__':
    reps, left = representatives()
    for sig, mb in reps:
        print('%-44s %-34s sub %4.1f GFLOP  plan %s' % (sig_id(sig), mb.shape(), mb.ref_flop() / 1e9, mb.plan()[0]))
    print('%d envelope launches, %d classes, %d representatives, left out: %s' % (len(envelope()), len(classes()), len(reps), [sig_id(s) for s in left]))
