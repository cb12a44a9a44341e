"""YOLOv3-SPP: a restatement of the spatial pyramid pooling block, the case lists of its kernels and an oracle
network with the block.  Host only: this module imports no GPU code.  test_cpu_spp.py holds the restatement to brute-force
window loops; test_gpu_spp.py runs the kernels and the model against it.

THE BLOCK.  SPP(x) = concat over channels of [x, pool5(x), pool9(x), pool13(x)]; pool k is a stride-1 max pool with SAME
padding whose padded positions never win: torch.nn.functional.max_pool2d(x, k, 1, k // 2) (implicit -inf padding).  Forward
values are exact in any dtype (max does not round; a NaN in a window gives NaN).  Backward: autograd through the same call in
fp64 -- the gradient of a window goes to its FIRST maximum in row-major order.

ERROR BOUND OF THE BACKWARD KERNEL.  dsrc[p] is a sum of t terms (the ddst of the windows that name p) formed in fp32 in a
fixed order from 0, plus what dsrc held with accumulate: t (+ 1) additions, each rounding a partial sum of at most S = sum of
the absolute terms.  |error| <= additions * 2^-24 * S (stream_kernels.ku), per element; with integer data every partial sum is
exact and the result is bit-equal to fp64."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import model as om
from stream_kernels import ku

POOLS = (5, 9, 13)

# (n, h, w, c) of the kernel tests.  The forward kernel has ONE path.  The backward kernel has two instantiations: a thread keeps
# the sums of up to 2 pixels (planes of up to SMALL_PLANE pixels) or of up to 16.  The host side of every launch has two paths:
# planes of more than 2048 pixels (64 KiB of LDS) raise the kernel's dynamic LDS limit first, and planes of more than MAX_PLANE
# pixels are refused.
MAX_PLANE = 4096
LDS_DEFAULT_PIXELS = 2048
SMALL_PLANE = 512
KERNEL_CASES = [(1, 1, 1, 4), (1, 2, 3, 4), (3, 7, 7, 36), (2, 10, 10, 512), (1, 13, 13, 512), (2, 19, 19, 512), (1, 20, 17, 8), (1, 33, 40, 8),
                (1, 16, 32, 4),      # SMALL_PLANE pixels: the largest plane of the backward kernel's 2-pixels-per-thread instantiation
                (1, 19, 27, 4),      # 513: the smallest of the other one
                (1, 32, 64, 4),      # 2048 pixels: the largest plane within the default LDS limit
                (1, 33, 64, 4),      # the first row beyond it
                (1, 64, 64, 4)]      # MAX_PLANE
REFUSED_CASES = [(1, 65, 64, 4), (1, 1, 4097, 4)]      # beyond MAX_PLANE: refused through the error channel, nothing launched
DATA_KINDS = ('normal', 'tied', 'inf', 'nan')
SRC_PAD, DST_PAD = 8, 4      # channels of NaN canary behind the source / pooled channels of the separate-buffer layout

# the 2048 -> 512 1x1 layer behind the pools: the GEMM shapes the planners are asked about
GEMM_BATCHES = (1, 2, 4, 8, 16)
GEMM_GRIDS = (10, 13, 16, 19)
GEMM_CIN, GEMM_COUT = 2048, 512


def gemm_representatives():
    """The distinct plan signatures of the four conv entry points for the new layer over GEMM_BATCHES x GEMM_GRIDS, in the words
    of the modules that pin the network's own (plan_forms / grad_forms / bf16_routes .signature), each with the first (batch, grid)
    that has it: {'fwd' | 'dgrad' | 'wgrad' | 'bf16': [(signature, member)]}.  Asks the library's host-side plan queries only."""
    import bf16_routes as br
    import grad_forms as gf
    import plan_forms as pf
    out = {'fwd': {}, 'dgrad': {}, 'wgrad': {}, 'bf16': {}}
    for n in GEMM_BATCHES:
        for g in GEMM_GRIDS:
            for arith in pf.ARITHS:
                for entry in ('fwd', 'dgrad'):
                    mb = pf.Member(entry, arith, n, g, g, GEMM_CIN, GEMM_COUT, 1, 1)
                    sig = mb.signature()
                    assert sig is not None or arith == 'x3', mb
                    if sig is not None:
                        out[entry].setdefault(sig, mb)
                mb = gf.Member('wgrad', arith, n, g, g, GEMM_CIN, GEMM_COUT, 1, 1)
                if mb.taken():
                    out['wgrad'].setdefault(mb.signature(), mb)
            mb = br.Member(n, g, g, GEMM_CIN, GEMM_COUT, 1, 1, False, False)
            out['bf16'].setdefault(mb.signature(), mb)
    return {k: list(v.items()) for k, v in out.items()}


def case_id(case):
    return 'n%d_%dx%d_c%d' % tuple(case)


def make_input(case, kind, seed=0):
    """[n, h, w, c] fp32 whose values are bf16 numbers (so that the same data serve both storage types).  normal: N(0, 1);
    tied: values from {-1, 0, 2}; inf: normal with a tenth of the elements +inf or -inf (and image 0, channel 0 all -inf); nan:
    normal with ONE NaN per image."""
    n, h, w, c = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + 11 * h + 13 * w + c + DATA_KINDS.index(kind))
    if kind == 'tied':
        return torch.tensor([-1.0, 0.0, 2.0])[torch.randint(0, 3, (n, h, w, c), generator=g)]
    x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16).float()
    if kind == 'inf':
        r = torch.rand(n, h, w, c, generator=g)
        x = torch.where(r < 0.05, torch.full_like(x, math.inf), x)
        x = torch.where(r > 0.95, torch.full_like(x, -math.inf), x)
        x[0, :, :, 0] = -math.inf
    if kind == 'nan':
        for i in range(n):
            p = int(torch.randint(0, h * w * c, (1,), generator=g))
            x[i].view(-1)[p] = math.nan
    return x


def pools_nchw(x):
    """[pool5, pool9, pool13] of an NCHW tensor, in its dtype"""
    return [F.max_pool2d(x, k, 1, k // 2) for k in POOLS]


def spp_forward(x):
    """x [n, h, w, c] (fp32, fp64 or bf16) -> [n, h, w, 3c] = [pool5 | pool9 | pool13], same dtype, exact"""
    t = x.permute(0, 3, 1, 2)
    work = t.float() if x.dtype == torch.bfloat16 else t
    return torch.cat(pools_nchw(work), dim=1).permute(0, 2, 3, 1).to(x.dtype).contiguous()


def spp_backward(x, ddst):
    """fp64 autograd: (dsrc [n, h, w, c], number of terms per element, sum of their absolute values)"""
    outs = []
    for g in (ddst.double(), torch.ones_like(ddst, dtype=torch.float64), ddst.double().abs()):
        t = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        torch.cat(pools_nchw(t), dim=1).backward(g.permute(0, 3, 1, 2))
        outs.append(t.grad.permute(0, 2, 3, 1).contiguous())
    return outs


def backward_bound(terms, mag, old=None):
    """per-element bound of the fp32 gather (module docstring); old: what dsrc held with accumulate"""
    adds = terms + (1.0 if old is not None else 0.0)
    return ku(1) * adds * (mag + (old.double().abs() if old is not None else 0.0))


def brute_force(x):
    """Window loops over a [h, w] fp64 array: (values [3, h, w], flat argmax [3, h, w]) with the first maximum in row-major order;
    a NaN anywhere in the window gives NaN (argmax then -1)."""
    h, w = x.shape
    val = np.empty((3, h, w))
    arg = np.empty((3, h, w), np.int64)
    for b, k in enumerate(POOLS):
        r = k // 2
        for i in range(h):
            for j in range(w):
                best, where, bad = None, -1, False
                for ii in range(max(i - r, 0), min(i + r, h - 1) + 1):
                    for jj in range(max(j - r, 0), min(j + r, w - 1) + 1):
                        v = x[ii, jj]
                        if v != v:
                            bad = True
                        elif best is None or v > best:
                            best, where = v, ii * w + jj
                val[b, i, j] = math.nan if bad else best
                arg[b, i, j] = -1 if bad else where
    return val, arg


# ----------------------------------------------------------------------------------------------------------------------
# the oracle network with the block
# ----------------------------------------------------------------------------------------------------------------------
def spp_layer_specs(in_channels, num_anchors, num_classes):
    """oracle.model.layer_specs with the 4 * 512 -> 512 1x1 layer behind the third layer of the coarsest block"""
    L = om.layer_specs(in_channels, num_anchors, num_classes)
    at = spp_layer_index(L)
    return L[:at] + [dict(cin=4 * L[at - 1]['cout'], cout=L[at - 1]['cout'], k=1, s=1, bn=True)] + L[at:]


def spp_layer_index(plain_specs):
    """index of the new layer in the SPP list: behind the third of the six layers in front of the first head"""
    first_head = next(i for i, sp in enumerate(plain_specs) if not sp['bn'])
    return first_head - 3


def init_params(in_channels, num_anchors, num_classes, seed=1, randomize_bn=False, dtype=np.float32):
    """oracle.model.init_params for the 76-layer list (the same draws in the same order: its own stream of random numbers)"""
    rng = np.random.default_rng(seed)
    P = []
    for sp in spp_layer_specs(in_channels, num_anchors, num_classes):
        k, cin, cout = sp['k'], sp['cin'], sp['cout']
        limit = math.sqrt(6.0 / (k * k * cin + k * k * cout))
        p = dict(W=rng.uniform(-limit, limit, (k, k, cin, cout)).astype(dtype), b=np.zeros(cout, dtype))
        if sp['bn']:
            if randomize_bn:
                p.update(gamma=rng.uniform(0.5, 1.5, cout).astype(dtype), beta=rng.normal(0, 0.1, cout).astype(dtype),
                         mean=rng.normal(0, 0.1, cout).astype(dtype), var=rng.uniform(0.5, 1.5, cout).astype(dtype))
                p['b'] = rng.normal(0, 0.1, cout).astype(dtype)
            else:
                p.update(gamma=np.ones(cout, dtype), beta=np.zeros(cout, dtype), mean=np.zeros(cout, dtype), var=np.ones(cout, dtype))
        P.append(p)
    return P


class SppNet(om.Net):
    """oracle.model.Net with the SPP spec list and the block in feature_maps; _conv_layer, the rounding points of the bf16
    emulation, decode, compute_loss, AdamState and train_step are the oracle's, unchanged.  `pools`: x (NCHW) -> the three
    pooled tensors (a test replaces it)."""

    def __init__(self, params, in_channels, num_anchors, num_classes, dtype=torch.float32, requires_grad=False, device=None):
        plain = om.layer_specs(in_channels, num_anchors, num_classes)
        at = spp_layer_index(plain)
        super().__init__(params[:at] + params[at + 1:], in_channels, num_anchors, num_classes, dtype=dtype, requires_grad=requires_grad, device=device)
        extra = om.Net([params[at]], in_channels, num_anchors, num_classes, dtype=dtype, requires_grad=requires_grad, device=device)
        self.specs = spp_layer_specs(in_channels, num_anchors, num_classes)
        self.p = self.p[:at] + extra.p + self.p[at:]
        self.spp_at = at
        self.pools = pools_nchw

    def feature_maps(self, x, training):
        self.batch_stats = []
        it = iter(range(len(self.specs)))
        raw = lambda t: self._conv_layer(t, next(it), training)

        def cl(t):
            i = next(it)
            y = self._conv_layer(t, i, training)
            return self._r(y) if self.specs[i]['bn'] else y      # heads stay fp32

        def feature_block(inp, reps):
            layer = inp
            for _ in range(reps):
                layer = cl(layer)
                layer = self._r(inp + raw(layer))
            return layer

        def yolo_block(inp, spp=False):
            if spp:
                inp = cl(cl(cl(inp)))
                inp = cl(torch.cat([inp] + list(self.pools(inp)), dim=1))      # pooling bf16 values is exact: no rounding point
            for _ in range(2 if spp else 5):
                inp = cl(inp)
            return inp, cl(inp)

        B = om.BLOCK_COUNT
        x = cl(cl(x))
        x = feature_block(x, 1)
        x = feature_block(cl(x), 2)
        route1 = x = feature_block(cl(x), B)
        route2 = x = feature_block(cl(x), B)
        route3 = feature_block(cl(x), B // 2)
        route, x = yolo_block(route3, True)
        fm1 = cl(x)
        x = cl(route)
        route, x = yolo_block(torch.cat([self._r(self._upsample_2x(x)), route2], dim=1))
        fm2 = cl(x)
        x = cl(route)
        route, x = yolo_block(torch.cat([self._r(self._upsample_2x(x)), route1], dim=1))
        fm3 = cl(x)
        return fm1, fm2, fm3
