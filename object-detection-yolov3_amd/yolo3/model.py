"""YoloV3 on MI355X: host-side mirror of the reference's ``model.YoloV3``
(/root/reference/model.py:19-540) driving hand-written HIP kernels through the
C ABI in include/yolo3hip.h.

Same constructor, methods and tensor contracts as the reference class
(model.py:423-540): NCHW z-scored images in, ``[N, Nb, 5+K]`` detections out,
three ``[N, G, G, A, 5+K]`` label tensors for the loss.  Internally everything
is NHWC fp32 in HBM (channel-contiguous = GEMM-K-contiguous), parameters /
gradients / Adam moments live in flat arenas in Keras ``trainable_weights``
order, and each step is a static list of kernel launches (replayable as one
HIP graph).  torch is used for device memory, streams and the RCCL all-reduce
only; there is no torch.nn / autograd / CPU fallback on this path.
"""
import collections
import contextlib
import ctypes
import functools
import math
import os
import warnings

import numpy as np
import torch

from . import _hip
from . import letterbox
from . import streams
from .anchors import resolve_anchor_scales, scale_masks
from ._hip import lib, check, view, int_array, EPI_LRELU, EPI_ACCUM, CONV_X3, BF16_NO_PATCH

BN_EPS = 1e-3          # Keras BatchNormalization defaults
BN_MOMENTUM = 0.99
LRELU_ALPHA = 0.2      # tf.nn.leaky_relu default (App. C3)
BF16_PATCH_MIN_BYTES = 300e6   # bf16 path: a 3x3 layer that moves less (input + residual + output) stays off the patch kernels
ALIGN = 64             # arena alignment in floats (256 B)


def ema_one_minus_decay(ema_decay, ema_warmup, t):
    """1 - d_t of the weight average after step t (1-based), with the warm-up ramp of the common YOLO trainers:
    d_t = ema_decay * (1 - exp(-t / ema_warmup)).  Computed in fp64 and rounded once to fp32, the value the fused Adam + EMA
    kernel reads (y3_adam_step_ema)."""
    d = float(ema_decay) * (1.0 - math.exp(-float(t) / float(ema_warmup)))
    return np.float32(1.0 - d)


BOX_LOSSES = ('mse', 'giou', 'diou', 'ciou')     # index = Y3_BOX_LOSS_* of y3_loss_fwd_bwd_ex


def check_box_loss_args(box_loss, box_loss_weight=1.0):
    """Host-side validation of a box-regression loss and its weight (the library checks them again): ValueError on an unknown
    kind, a weight that is not a finite number > 0, or a weight other than 1 with 'mse' (the reference's loss has no such factor)."""
    if box_loss not in BOX_LOSSES:
        raise ValueError('box_loss must be one of {}, got {!r}'.format(', '.join(BOX_LOSSES), box_loss))
    try:
        w = float(box_loss_weight)
    except (TypeError, ValueError):
        raise ValueError('box_loss_weight must be a number, got {!r}'.format(box_loss_weight))
    if not (w > 0.0 and math.isfinite(w)):
        raise ValueError('box_loss_weight must be finite and > 0, got {!r}'.format(box_loss_weight))
    if box_loss == 'mse' and w != 1.0:
        raise ValueError("box_loss_weight {!r} needs an IoU box_loss (giou, diou, ciou): 'mse' is the reference's loss, unweighted"
                         .format(box_loss_weight))


IGNORE_MASKS = ('reference', 'truth')
DEFAULT_IGNORE_THRESH = 0.5
DEFAULT_MAX_TRUTH_BOXES = 1024


def check_ignore_mask_args(ignore_mask='reference', ignore_thresh=DEFAULT_IGNORE_THRESH, max_truth_boxes=DEFAULT_MAX_TRUTH_BOXES):
    """Host-side validation of the ignore mask of the objectness loss (the library checks the numbers again):
    ValueError on an unknown mask, a threshold that is not a finite number in (0, 1], a capacity that is not an integer >= 1, or
    a threshold / capacity other than the defaults with 'reference' (the reference's mask has no such parameters)."""
    if ignore_mask not in IGNORE_MASKS:
        raise ValueError('ignore_mask must be one of {}, got {!r}'.format(', '.join(IGNORE_MASKS), ignore_mask))
    try:
        t = float(ignore_thresh)
    except (TypeError, ValueError):
        raise ValueError('ignore_thresh must be a number, got {!r}'.format(ignore_thresh))
    if isinstance(ignore_thresh, bool) or not (0.0 < t <= 1.0):
        raise ValueError('ignore_thresh must be finite and in (0, 1], got {!r}'.format(ignore_thresh))
    cap = max_truth_boxes
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 1 or cap >= 2 ** 31:
        raise ValueError('max_truth_boxes must be an integer >= 1, got {!r}'.format(max_truth_boxes))
    if ignore_mask == 'reference' and (t != DEFAULT_IGNORE_THRESH or cap != DEFAULT_MAX_TRUTH_BOXES):
        raise ValueError("ignore_thresh {!r} / max_truth_boxes {!r} need ignore_mask 'truth': the reference's mask has no such parameters"
                         .format(ignore_thresh, max_truth_boxes))


FOCAL_TERMS = ('obj', 'class', 'both')


def check_focal_args(focal_gamma=0.0, focal_alpha=0.0, focal_terms='both', label_smoothing=0.0):
    """Host-side validation of the focal form of the objectness / class loss and of class-label smoothing (the
    library checks the numbers again): ValueError unless focal_gamma is a finite number >= 0, focal_alpha is 0 (no balancing
    factor) or in (0, 1), focal_terms is one of obj, class, both, and label_smoothing is in [0, 1)."""
    vals = []
    for name, v in (('focal_gamma', focal_gamma), ('focal_alpha', focal_alpha), ('label_smoothing', label_smoothing)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError('{} must be a number, got {!r}'.format(name, v))
        if isinstance(v, bool):
            raise ValueError('{} must be a number, got {!r}'.format(name, v))
        vals.append(f)
    g, a, e = vals
    if not (g >= 0.0 and math.isfinite(g)):
        raise ValueError('focal_gamma must be finite and >= 0, got {!r}'.format(focal_gamma))
    if not (a == 0.0 or 0.0 < a < 1.0):
        raise ValueError('focal_alpha must be 0 (no balancing factor) or in (0, 1), got {!r}'.format(focal_alpha))
    if focal_terms not in FOCAL_TERMS:
        raise ValueError('focal_terms must be one of {}, got {!r}'.format(', '.join(FOCAL_TERMS), focal_terms))
    if not 0.0 <= e < 1.0:
        raise ValueError('label_smoothing must be in [0, 1), got {!r}'.format(label_smoothing))


def focal_term_args(focal_gamma=0.0, focal_alpha=0.0, focal_terms='both', label_smoothing=0.0):
    """(gamma_obj, alpha_obj, gamma_cls, alpha_cls, label_smoothing) as y3_loss_fwd_bwd_focal takes them: the term that
    focal_terms leaves out gets gamma = alpha = 0; label smoothing belongs to the class term whatever focal_terms says."""
    g, a = float(focal_gamma), float(focal_alpha)
    obj = (g, a) if focal_terms in ('obj', 'both') else (0.0, 0.0)
    cls = (g, a) if focal_terms in ('class', 'both') else (0.0, 0.0)
    return obj + cls + (float(label_smoothing),)


def check_grad_args(accumulate_steps=1, grad_clip_norm=None):
    """Host-side validation of the gradient accumulation count and the global-norm clip (the library checks them
    again): ValueError unless accumulate_steps is an integer >= 1 and grad_clip_norm is None (off) or a finite number > 0."""
    k = accumulate_steps
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError('accumulate_steps must be an integer >= 1, got {!r}'.format(accumulate_steps))
    if grad_clip_norm is None:
        return
    try:
        c = float(grad_clip_norm)
    except (TypeError, ValueError):
        raise ValueError('grad_clip_norm must be None (off) or a number, got {!r}'.format(grad_clip_norm))
    if isinstance(grad_clip_norm, bool) or not (c > 0.0 and math.isfinite(c)):
        raise ValueError('grad_clip_norm must be None (off) or finite and > 0, got {!r}'.format(grad_clip_norm))


def clip_scale(norm, clip, k):
    """The factor the scaled Adam kernel multiplies the accumulated gradient with (y3_grad_clip_scale, restated on the host for
    tests and logs): (1/k) * (clip / max(norm, clip)) for the pre-clip global norm `norm` of the averaged gradient, 1/k with
    clip None.  fp64, rounded once to fp32."""
    s = 1.0 / float(k)
    if clip is not None:
        s = s * (float(clip) / max(float(norm), float(clip)))
    return np.float32(s)


OPTIMIZERS = ('adam', 'adamw', 'sgd')


def check_optimizer_args(optimizer='adam', momentum=0.9, nesterov=False, weight_decay=0.0, lr_schedule=None):
    """Host-side validation of the optimiser setting (the library checks the numbers again): ValueError on an
    unknown optimiser, a momentum outside [0, 1), a nesterov that is not a boolean, a weight decay that is not a finite number
    >= 0, a weight decay with 'adam' (Keras Adam has none: 'adamw' is the decayed form), or a schedule without factor(t)."""
    if optimizer not in OPTIMIZERS:
        raise ValueError('optimizer must be one of {}, got {!r}'.format(', '.join(OPTIMIZERS), optimizer))
    vals = []
    for name, v in (('momentum', momentum), ('weight_decay', weight_decay)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError('{} must be a number, got {!r}'.format(name, v))
        if isinstance(v, bool):
            raise ValueError('{} must be a number, got {!r}'.format(name, v))
        vals.append(f)
    mu, wd = vals
    if not 0.0 <= mu < 1.0:
        raise ValueError('momentum must be in [0, 1), got {!r}'.format(momentum))
    if not (isinstance(nesterov, (bool, np.bool_)) or (isinstance(nesterov, (int, np.integer)) and nesterov in (0, 1))):
        raise ValueError('nesterov must be False or True, got {!r}'.format(nesterov))
    if not (wd >= 0.0 and math.isfinite(wd)):
        raise ValueError('weight_decay must be finite and >= 0, got {!r}'.format(weight_decay))
    if optimizer == 'adam' and wd > 0.0:
        raise ValueError("weight_decay {!r} needs optimizer 'adamw' (decoupled decay) or 'sgd': 'adam' is the reference's Keras Adam, "
                         'which has none'.format(weight_decay))
    if lr_schedule is not None and not callable(getattr(lr_schedule, 'factor', None)):
        raise ValueError('lr_schedule must be None or have a factor(t) method (yolo3.schedule.LrSchedule), got {!r}'.format(lr_schedule))


def decay_ranges(specs):
    """The segments of the parameter arena that weight decay applies to: the kernel W of every layer,
    [w_off, w_off + k*k*cin_pad*cout) in floats, in arena order.  Biases, gamma and beta are never decayed.  Segments start on
    multiples of 64 floats and cin_pad is a multiple of 4, so every begin and end is a multiple of 4 (y3_optim_step's rule)."""
    return [(sp.w_off, sp.w_off + sp.k * sp.k * sp.cin_pad * sp.cout) for sp in specs]


BACKBONE_LAYERS = 52      # the conv layers of Darknet-53 in front of the first yolo block: what `--freeze backbone` names


def check_freeze_args(freeze_layers=0, freeze_bn=False, n_layers=None):
    """Host-side validation of the fine-tuning settings: ValueError unless freeze_layers is an integer with
    0 <= freeze_layers < n_layers (n_layers None: the upper end is not checked) and freeze_bn is a boolean."""
    n = freeze_layers
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise ValueError('freeze_layers must be an integer, got {!r}'.format(freeze_layers))
    if n < 0 or (n_layers is not None and n >= n_layers):
        raise ValueError('freeze_layers must be in [0, {}): at least the last layer trains, got {!r}'.format(
            n_layers if n_layers is not None else 'number of layers', freeze_layers))
    if not (isinstance(freeze_bn, (bool, np.bool_)) or (isinstance(freeze_bn, (int, np.integer)) and freeze_bn in (0, 1))):
        raise ValueError('freeze_bn must be False or True, got {!r}'.format(freeze_bn))


def trainable_suffix(specs, arena_floats, freeze_layers=0):
    """(offset, count) in floats of the part of the parameter arena that trains with layers 0 .. freeze_layers - 1 frozen: the
    arena is in creation order, so it is the suffix from specs[freeze_layers].w_off on.  Every per-arena pass of a step (the
    optimiser, accumulation, norm, weight refresh, all-reduce) runs over it; the offset is a multiple of ALIGN floats."""
    off = specs[freeze_layers].w_off
    return off, arena_floats - off


def suffix_decay_ranges(specs, freeze_layers=0):
    """decay_ranges of the trainable layers, relative to the start of the trainable suffix (trainable_suffix): the table
    y3_optim_step gets when its arenas are passed from that offset on.  Frozen kernels are in no range: decay cannot shrink them."""
    off = specs[freeze_layers].w_off
    return [(lo - off, hi - off) for lo, hi in decay_ranges(specs[freeze_layers:])]


def check_train_sizes(img_size, train_sizes):
    """Host-side validation of the network input sizes train_step / test_step accept (multi-scale training).  None:
    the constructed size only, returned as [(H, W)].  Otherwise a list of (H, W), each a positive multiple of 32; the constructed
    img_size is always included (first).  ValueError otherwise."""
    own = (int(img_size[0]), int(img_size[1]))
    if train_sizes is None:
        return [own]
    out = [own]
    try:
        pairs = [(s[0], s[1], len(s)) for s in train_sizes]
    except (TypeError, IndexError):
        raise ValueError('train_sizes must be None or a list of (H, W) pairs, got {!r}'.format(train_sizes))
    for h, w, n in pairs:
        ok = n == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (h, w))
        if not ok or h < 32 or w < 32 or h % 32 or w % 32:
            raise ValueError('train_sizes must hold (H, W) pairs of positive multiples of 32, got {!r}'.format((h, w) if n == 2 else train_sizes))
        if (int(h), int(w)) not in out:
            out.append((int(h), int(w)))
    return out


def _round_up(v, a):
    return (v + a - 1) // a * a


class LayerSpec:
    __slots__ = ('cin', 'cin_pad', 'cout', 'k', 's', 'bn', 'w_off', 'b_off', 'g_off', 'be_off', 'end_off', 'bn_idx', 'ch_off', 'mv_off')


def build_layer_specs(in_channels, num_anchors, num_classes, spp=False, head_anchors=None):
    """Conv layers in Keras creation order (model.py:356-421); see the walk in
    ``_Plan._build`` which consumes them in the same order.  spp: the YOLOv3-SPP variant, one more 1x1 layer
    (4 * 512 -> 512) behind the third layer of the coarsest scale's block; everything else, and with spp off every offset, is
    the reference's network.  head_anchors: the anchors per head, coarse -> fine (per-scale anchor assignment):
    head s has A_s * (5 + K) output channels; None gives every head all num_anchors, and every offset is the reference's."""
    L = []

    def conv(cin, cout, k, s=1, bn=True):
        sp = LayerSpec()
        sp.cin, sp.cout, sp.k, sp.s, sp.bn = cin, cout, k, s, bn
        sp.cin_pad = _round_up(cin, 4)
        L.append(sp)
        return cout

    def feature_block(c, reps):
        for _ in range(reps):
            conv(c, c // 2, 1)
            conv(c // 2, c, 3)
        return c

    FC = YoloV3.FILTER_COUNT
    c = conv(in_channels, FC // 32, 3)
    c = conv(c, FC // 16, 3, 2)
    c = feature_block(c, 1)
    c = conv(c, FC // 8, 3, 2)
    c = feature_block(c, 2)
    c = conv(c, FC // 4, 3, 2)
    c = feature_block(c, YoloV3.BLOCK_COUNT)
    c = conv(c, FC // 2, 3, 2)
    c = feature_block(c, YoloV3.BLOCK_COUNT)
    c = conv(c, FC, 3, 2)
    c = feature_block(c, YoloV3.BLOCK_COUNT // 2)
    if head_anchors is None:
        head_anchors = [num_anchors] * 3
    if len(head_anchors) != 3 or any(int(a) < 1 for a in head_anchors):
        raise ValueError('head_anchors must be three counts >= 1 (coarse -> fine), got {!r}'.format(head_anchors))
    D = [int(a) * (5 + num_classes) for a in head_anchors]

    def yolo_block(cin, fc, spp=False):
        for i in range(3):
            conv(cin if i == 0 else fc, fc // 2, 1)
            if spp and i == 1:
                conv(4 * (fc // 2), fc // 2, 1)      # reads concat [x, pool5, pool9, pool13]
            conv(fc // 2, fc, 3)

    yolo_block(FC, FC, spp)
    conv(FC, D[0], 1, 1, bn=False)
    conv(FC // 2, FC // 2, 1)
    yolo_block(FC, FC // 2)
    conv(FC // 2, D[1], 1, 1, bn=False)
    conv(FC // 4, FC // 4, 1)
    yolo_block(FC // 2, FC // 4)
    conv(FC // 4, D[2], 1, 1, bn=False)
    # arena offsets (floats)
    off = 0
    bn_idx = 0
    ch = 0
    mv = 0
    for sp in L:
        sp.w_off = off
        off = _round_up(off + sp.k * sp.k * sp.cin_pad * sp.cout, ALIGN)
        sp.b_off = off
        off = _round_up(off + sp.cout, ALIGN)
        if sp.bn:
            sp.g_off = off
            off = _round_up(off + sp.cout, ALIGN)
            sp.be_off = off
            off = _round_up(off + sp.cout, ALIGN)
            sp.bn_idx = bn_idx
            bn_idx += 1
            sp.ch_off = ch                  # per-layer block [scale|shift|save_mean|save_rstd|k1|k2|k3], each cout floats
            ch = _round_up(ch + 7 * sp.cout, ALIGN)
            sp.mv_off = mv                  # offset into the moving mean / variance arrays
            mv = _round_up(mv + sp.cout, ALIGN)
        else:
            sp.g_off = sp.be_off = -1
            sp.bn_idx = -1
            sp.ch_off = sp.mv_off = -1
        sp.end_off = off
    return L, off, ch, mv


def spp_transfer_map(specs):
    """For the spec list of an SPP model: per layer the index of the plain network's layer with the same role, None for the
    layer only the SPP network has (the 1x1 layer whose input is 4x the width of the 1x1 conv_layer before it)."""
    fresh = [i for i in range(1, len(specs))
             if specs[i].k == 1 and specs[i - 1].k == 1 and specs[i - 1].bn and specs[i].cin == 4 * specs[i - 1].cout]
    if len(fresh) != 1:
        raise ValueError('spp_transfer_map: not the spec list of an SPP model')
    return [None if i == fresh[0] else i - (i > fresh[0]) for i in range(len(specs))]


def pretrained_map(specs, spp, file_shapes, file_spp):
    """How load_pretrained fills a model (spec list `specs`, SPP or not) from a weight file whose layers have the kernel shapes
    `file_shapes` ((k, k, Cin, Cout) each, creation order) and which holds the SPP network or not.  Returns (mapping, kept):
    mapping[i] = the file's layer with the role of model layer i, or None where the layer keeps its initialisation; kept = those i.
    Layers are matched by role: the same index, or spp_transfer_map for a plain file and an SPP model.  A detection head (bn=False)
    whose shape differs -- another class count or anchor count -- keeps its initialisation; any other difference is refused:
    ValueError for an SPP file and a plain model, another input channel count, another layer count or body shape."""
    if file_spp and not spp:
        raise ValueError('load_pretrained: the file holds the SPP network and this model is plain (spp=False): the layer behind the '
                         'pools has no place to go')
    mapping = spp_transfer_map(specs) if spp and not file_spp else list(range(len(specs)))
    if len(file_shapes) != 1 + max(j for j in mapping if j is not None):
        raise ValueError('load_pretrained: the file has {} layers, this model needs {}'.format(len(file_shapes), 1 + max(j for j in mapping if j is not None)))
    if tuple(file_shapes[0])[2] != specs[0].cin:
        raise ValueError('load_pretrained: the file was trained on {} input channels, this model reads {}'.format(tuple(file_shapes[0])[2], specs[0].cin))
    kept = []
    for i, sp in enumerate(specs):
        j = mapping[i]
        if j is None:
            kept.append(i)
        elif tuple(int(v) for v in file_shapes[j]) != (sp.k, sp.k, sp.cin, sp.cout):
            if sp.bn:
                raise ValueError('load_pretrained: layer {} is {} in the file and {} in this model'.format(i, tuple(file_shapes[j]), (sp.k, sp.k, sp.cin, sp.cout)))
            mapping[i] = None
            kept.append(i)
    return mapping, kept


class _T:
    """An NHWC activation (or a channel slice of one) plus its gradient twin."""

    def __init__(self, buf, n, h, w, c, ld=None, off=0):
        self.buf, self.n, self.h, self.w, self.c = buf, n, h, w, c
        self.ld = c if ld is None else ld
        self.off = off
        self.v = view(buf, n, h, w, c, self.ld, off)
        self.grad = None
        self.gw = False           # gradient already holds a contribution (next writer accumulates)
        self.children = []
        self.parent = None
        self.frozen = False       # written by a frozen layer (or the image): it gets no gradient

    @property
    def no_grad(self):
        """No gradient is wanted for this activation: its producer is frozen, or it is a concat whose producers all are."""
        return self.frozen or (bool(self.children) and all(ch.frozen for ch in self.children))

    @property
    def m(self):
        return self.n * self.h * self.w

    def slice(self, c0, c):
        t = _T(self.buf, self.n, self.h, self.w, c, self.ld, self.off + c0)
        t.parent = self
        self.children.append(t)
        return t

    def mark_written(self):
        self.gw = True
        for ch in self.children:
            ch.gw = True

    def torch_view(self):
        """[N,H,W,C] strided torch view (debug / export)."""
        flat = self.buf.view(-1)
        return torch.as_strided(flat, (self.n, self.h, self.w, self.c), (self.h * self.w * self.ld, self.w * self.ld, self.ld, 1), self.off)


class Mean:
    """Minimal stand-in for tf.keras.metrics.Mean (train.py:80-90)."""

    def __init__(self, name='mean', dtype=None):
        self.name = name
        self.reset_states()

    def update_state(self, value):
        self.total = self.total + (value.detach() if torch.is_tensor(value) else float(value))
        self.count += 1

    def result(self):
        if self.count == 0:
            return 0.0
        t = self.total / self.count
        return float(t.item()) if torch.is_tensor(t) else float(t)

    def reset_states(self):
        self.total = 0.0
        self.count = 0


def _pixels(v):
    return v.n * v.h * v.w


# ticketed conv launch -> the library's workspace query, fed with the launch's own arguments (those before the workspace)
_WS_QUERY = {
    'y3_conv2d_fwd': lambda src, wt, bias, k, s, dst, flags, *_: lib.y3_conv2d_fwd_workspace_x(_pixels(dst), src.c, k, dst.c, flags),
    'y3_conv2d_fwd_bf16_ws': lambda src, wt, bias, k, s, dst, *_: lib.y3_conv2d_fwd_bf16_workspace(_pixels(dst), src.c, k, dst.c),
    'y3_conv2d_dgrad': lambda ddst, wt, k, s, dsrc, flags: lib.y3_conv2d_dgrad_workspace_x(ddst, k, s, dsrc, flags),
    'y3_conv2d_dgrad_bn': lambda ddst, wt, k, s, dsrc, flags, *_: lib.y3_conv2d_dgrad_workspace_x(ddst, k, s, dsrc, flags),
}

# What the forward walk decides once for a layer and keeps as the last element of its op.  fwd / dgrad / wgrad: whether that launch
# runs the x3 kernels, CONV_X3 or 0 each; everything sized or emitted for the layer reads it from there.  bn: the addresses
# (save_mean, save_rstd, coef) of a BatchNorm layer's per-channel block, None for a head.
_Layer = collections.namedtuple('_Layer', 'fwd dgrad wgrad bn')


class _Plan:
    """Static launch list for one (batch size, mode, input size).  A plan owns everything whose shape follows the input: activations
    and their gradients, the label tensors, BatchNorm partial rows, the conv / kernel-gradient workspaces, its captured graphs.
    What depends on the weights alone (arenas, transposed and split copies, per-channel BatchNorm blocks) stays on the model."""

    def __init__(self, model, n, training, bf16, size):
        self.model = model
        self.size = size             # (H, W), as YoloV3._plan normalised it
        self.n = n
        self.training = training
        self.bf16 = bool(bf16) and not training     # reduced-precision conv path: inference only (BASELINE config 5)
        self.fwd = []      # [(cfunc, args)]   stream appended at run time
        self.bwd = []
        self.keep = []     # ctypes objects / tensors that must outlive the lists
        self.tensors = []
        self.graph = None
        self.graph_micro = None      # gradient accumulation: the captured micro-step that ends in the accumulator (YoloV3._capture)
        self.infer_graph = None
        self.infer_graph_tiles = None     # forward (without the input transpose) + decode, for predict_tiles
        self.zs_ws = None
        self.lb_ws = None            # workspace of y3_letterbox_zscore_nhwc (predict_letterbox)
        self._build()

    # -- allocation helpers -------------------------------------------------
    def _new(self, n, h, w, c, ld=None, zero=False, dtype=torch.float32):
        ld = c if ld is None else ld
        numel = n * h * w * ld
        buf = (torch.zeros if zero else torch.empty)(numel, dtype=dtype, device=self.model.device)
        t = _T(buf, n, h, w, c, ld)
        self.tensors.append(t)      # the launch lists hold raw pointers only: keep every buffer alive with the plan
        return t

    def _emit(self, lst, fn, *args):
        self.keep.append(args)
        lst.append((fn, args))

    def _at(self, arena, off):
        """Device address of float offset `off` (LayerSpec.*_off and their like) in one of the model's or the plan's flat buffers:
        an fp32 arena, the bf16 copy of one, or the piece planes (three bf16 planes per kernel, y3_x3_split_weights)."""
        pieces = 3 if arena is self.model.planes or arena is self.model.planes_t else 1
        return arena.data_ptr() + arena.element_size() * pieces * off

    def _conv_call(self, lst, fn, *args):
        """Emit a conv launch that may use the shared split-K workspace (allocated after the walk).  Its need is asked with the
        launch's own arguments, flags included (Y3_CONV_X3 changes the tile and the split-K plan): with fewer bytes than that
        the library quietly drops the split (yolo3hip.h)."""
        self.conv_ws_bytes = max(self.conv_ws_bytes, int(_WS_QUERY[fn.__name__](*args)))
        entry = [fn, args]
        self._conv_ws_users.append(entry)
        lst.append(entry)

    def _bind_conv_workspace(self):
        # zeroed once: the head of a conv workspace holds per-tile tickets that every launch leaves at zero (yolo3hip.h)
        self.conv_ws = torch.zeros(max(self.conv_ws_bytes // 4, 4), dtype=torch.float32, device=self.model.device)
        for lst in (self.fwd, self.bwd):
            for i, e in enumerate(lst):
                if isinstance(e, list):
                    fn, args = e
                    lst[i] = (fn, tuple(args) + (self.conv_ws.data_ptr(), self.conv_ws_bytes))
        self.keep.append(self._conv_ws_users)

    # -- network walk (model.py:356-421) ---------------------------------------
    def _build(self):
        mdl = self.model
        dev = mdl.device
        N = self.n
        (H, W), C = self.size, mdl.img_size[2]
        A, K = mdl.number_anchors, mdl.number_classes
        # anchors per scale: all of them on every scale unless the model has an owner table
        As = mdl.scale_anchor_counts
        Ds = [a * (5 + K) for a in As]
        Dlds = [_round_up(d, 4) for d in Ds]
        specs = mdl.specs
        P = mdl.params
        tr = self.training
        bf = self.bf16
        act = torch.bfloat16 if bf else torch.float32      # activation storage type after the first layer
        self.in_nchw = torch.zeros(N, C, H, W, dtype=torch.float32, device=dev)
        self.ops = []      # high-level records for the backward emission
        self.x3_fwd, self.x3_dgrad, self.x3_wgrad = [], [], []     # layers whose forward / data gradient / kernel gradient runs the x3 kernels (bench.py: work per arithmetic)
        self.layer_out = []  # output activation of every conv_layer, creation order (debug / tests)
        li = [0]

        x0 = self._new(N, H, W, specs[0].cin_pad, zero=True)
        x0.frozen = True
        self.x0 = x0                      # the network's NHWC input (channels padded to 4): predict_tiles writes it directly
        # fine-tuning, training plans only: layers 0 .. nfrozen - 1 run as in inference and leave nothing for
        # backward; fbn: the BatchNorm of the trainable layers normalises with the moving statistics
        nfrozen = mdl.freeze_layers if tr else 0
        fbn = tr and mdl.freeze_bn
        self._emit(self.fwd, lib.y3_nchw_to_nhwc, self.in_nchw.data_ptr(), N, C, H, W, x0.v)

        # shared workspaces.  The largest M*Cout of the net is conv1's (full resolution, FILTER_COUNT/32
        # channels); BN partial statistics need <= 2*Cout floats per row tile of >= 64 rows.
        max_mc = N * H * W * max(YoloV3.FILTER_COUNT // 32, max(Dlds))
        self.stats_ws = torch.empty(max_mc // 16 + 8192, dtype=torch.float32, device=dev)
        # split-K slabs of the small-spatial layers (y3_conv2d_fwd_workspace / _dgrad_workspace); 64 MiB covers every layer
        # of the 416 / 608 configurations, the exact need is checked per layer below
        self.conv_ws_bytes = 0
        self._conv_ws_users = []
        if not tr:
            # inference-mode BatchNorm (training=False, model.py:38): moving statistics folded into scale / shift, all layers at once
            self._emit(self.fwd, lib.y3_bn_fold_inference_batched, P.data_ptr(), mdl.moving.data_ptr(), mdl.chan.data_ptr(),
                       mdl.fold_table().data_ptr(), mdl.fold_layers, BN_EPS)
        if nfrozen or fbn:
            # scale / shift of the layers that normalise with the moving statistics, folded once per step so that they follow
            # set_weights / load_pretrained and, with freeze_bn, the gamma / beta of the step before.  The table is in creation
            # order: the frozen prefix is its first rows, freeze_bn takes all of them.
            rows = sum(1 for sp in specs if sp.bn) if fbn else sum(1 for sp in specs[:nfrozen] if sp.bn)
            self._emit(self.fwd, lib.y3_bn_fold_inference_batched, P.data_ptr(), mdl.moving.data_ptr(), mdl.chan.data_ptr(),
                       mdl.fold_table().data_ptr(), rows, BN_EPS)
        if tr:
            self.dz = torch.empty(max_mc, dtype=torch.float32, device=dev)
            # y3_bn_bwd_workspace(): 1 KiB of tickets (zero before the first launch) + <= 512 x 6 x 64 fp64 partials
            self.bnb_ws = torch.zeros(1024 + 512 * 6 * 64 * 8, dtype=torch.uint8, device=dev)
        ptr = functools.partial(self._at, P)

        def conv_layer(src, out=None, resid=None):
            """model.py:29-39 (+ the tf.add of model.py:47 when resid is given)."""
            i = li[0]
            li[0] += 1
            sp = specs[i]
            oh, ow = -(-src.h // sp.s), -(-src.w // sp.s)
            y = out if out is not None else self._new(N, oh, ow, sp.cout, dtype=act)
            frozen = i < nfrozen                                   # runs as in inference: no `a`, no statistics, no record for backward
            y.frozen = frozen
            train = tr and not frozen
            a = self._new(N, oh, ow, sp.cout) if train else None   # the convolution's own output: BatchNorm reads it again in backward
            rv = resid.v if resid is not None else None
            ch = self._at(mdl.chan, sp.ch_off)       # per-layer [scale|shift|mean|rstd|coef(3)] block
            cs = sp.cout * 4
            scale, shift, smean, srstd, coef = ch, ch + cs, ch + 2 * cs, ch + 3 * cs, ch + 4 * cs
            # fp32 arithmetic as three bf16 pieces per operand (conv_x3.hip) for the launches the model's policy names.  The gradients
            # have their activations' geometry, which is all the data-gradient query reads; the first layer has no data gradient.
            x3 = _Layer(CONV_X3 if not bf and mdl.x3_forward(sp, N * oh * ow) else 0,
                        CONV_X3 if train and not src.no_grad and mdl.x3_dgrad(a.v, sp.k, sp.s, src.v) else 0,
                        CONV_X3 if train and mdl.x3_wgrad(sp, N * oh * ow) else 0, (smean, srstd, coef))
            if x3.fwd:
                self.x3_fwd.append(i)
            # the x3 kernel wants the copy of the weights with K contiguous per output column, i.e. the three bf16 planes of the
            # TRANSPOSED kernel in the forward pass
            wfwd = self._at(mdl.planes_t, sp.w_off) if x3.fwd else ptr(sp.w_off)
            if train and fbn:
                # frozen statistics: the batch's are not collected; scale / shift come from the fold at the head of the list
                self._conv_call(self.fwd, lib.y3_conv2d_fwd, src.v, wfwd, ptr(sp.b_off), sp.k, sp.s, a.v, EPI_LRELU | x3.fwd,
                                LRELU_ALPHA, None, None, None, None)
                self._emit(self.fwd, lib.y3_bn_apply, a.v, scale, shift, rv, y.v)
                self.ops.append(('conv_layer', i, src, a, y, resid, x3))
            elif train:
                tiles = lib.y3_conv2d_stats_tiles_x(a.m, sp.cin_pad, sp.k, sp.cout, x3.fwd)
                assert tiles * 2 * sp.cout <= self.stats_ws.numel()
                self._conv_call(self.fwd, lib.y3_conv2d_fwd, src.v, wfwd, ptr(sp.b_off), sp.k, sp.s, a.v, EPI_LRELU | x3.fwd,
                                LRELU_ALPHA, None, None, None, self.stats_ws.data_ptr())
                self._emit(self.fwd, lib.y3_bn_stats_finalize, self.stats_ws.data_ptr(), tiles, sp.cout, a.m, ptr(sp.g_off), ptr(sp.be_off),
                           BN_EPS, BN_MOMENTUM, self._at(mdl.moving, sp.mv_off), self._at(mdl.moving, mdl.moving_stride + sp.mv_off),
                           smean, srstd, scale, shift)
                self._emit(self.fwd, lib.y3_bn_apply, a.v, scale, shift, rv, y.v)
                self.ops.append(('conv_layer', i, src, a, y, resid, x3))
            elif bf and i > 0:
                # (the shared conv workspace: small-M layers are split along K, y3_conv2d_fwd_bf16_workspace)
                # the patch kernels of the early 3x3 layers only where the layer streams from HBM (yolo3hip.h, Y3_BF16_NO_PATCH;
                # same box, graph replay: 25 x 608^2 6.54 -> 6.25 ms with them, 8 x 608^2 2.56 -> 2.61, 8 x 416^2 1.74 -> 1.78)
                moved = 2 * y.m * (sp.s * sp.s * sp.cin_pad + sp.cout * (2 if resid is not None else 1))
                self._conv_call(self.fwd, lib.y3_conv2d_fwd_bf16_ws, src.v, self._at(mdl.params_t_bf16, sp.w_off), ptr(sp.b_off), sp.k, sp.s, y.v, 0,
                                EPI_LRELU | (0 if moved >= BF16_PATCH_MIN_BYTES else BF16_NO_PATCH), LRELU_ALPHA, scale, shift, rv)
            elif bf and sp.cin_pad == 4 and sp.cout == 32 and sp.k == 3 and sp.s == 1:
                # the RGB layer: fp32 direct convolution, one rounding on the bf16 store
                self._emit(self.fwd, lib.y3_conv2d_first_bf16, src.v, ptr(sp.w_off), ptr(sp.b_off), y.v, EPI_LRELU, LRELU_ALPHA, scale, shift)
            elif bf:
                # (other first-layer shapes) fp32 MFMA kernel, output rounded to bf16 once
                y32 = self._new(N, oh, ow, sp.cout)
                self._conv_call(self.fwd, lib.y3_conv2d_fwd, src.v, ptr(sp.w_off), ptr(sp.b_off), sp.k, sp.s, y32.v, EPI_LRELU,
                                LRELU_ALPHA, scale, shift, None, None)
                self._emit(self.fwd, lib.y3_f32_to_bf16, y32.buf.data_ptr(), y.buf.data_ptr(), y.buf.numel())
            else:
                self._conv_call(self.fwd, lib.y3_conv2d_fwd, src.v, wfwd, ptr(sp.b_off), sp.k, sp.s, y.v, EPI_LRELU | x3.fwd,
                                LRELU_ALPHA, scale, shift, rv, None)
            self.layer_out.append(y)
            return y

        def feature_block(inp, reps, out_last=None):
            """model.py:42-48: every repetition adds the BLOCK input (Q2)."""
            layer = inp
            for r in range(reps):
                layer = conv_layer(layer)
                layer = conv_layer(layer, out=out_last if r == reps - 1 else None, resid=inp)
            return layer

        def spp_block(inp):
            """YOLOv3-SPP: the block's third layer writes channel slice 0 of a 4x wide buffer, one launch fills the
            other three slices with its 5 / 9 / 13 max pools, and the 1x1 layer that follows reads the whole buffer."""
            inp = conv_layer(conv_layer(inp))
            c = specs[li[0]].cout
            cat = self._new(N, inp.h, inp.w, 4 * c, dtype=act)      # concat([x, pool5(x), pool9(x), pool13(x)])
            x = conv_layer(inp, out=cat.slice(0, c))
            pools = cat.slice(c, 3 * c)
            self._emit(self.fwd, lib.y3_spp_fwd_bf16 if bf else lib.y3_spp_fwd, x.v, pools.v)
            pools.frozen = x.frozen
            if not x.frozen:
                self.ops.append(('spp', x, cat, pools))
            return conv_layer(cat)

        def yolo_block(inp, spp=False):
            if spp:
                inp = spp_block(inp)
            for _ in range(2 if spp else 5):
                inp = conv_layer(inp)
            return inp, conv_layer(inp)

        def head(src, g):
            """detection_layer (model.py:108-120): linear 1x1 conv, bias."""
            i = li[0]
            li[0] += 1
            sp = specs[i]
            fm = self._new(N, src.h, src.w, Ds[g], Dlds[g], zero=True)
            if bf:      # bf16 operands, fp32 feature map: decode / loss / NMS stay fp32
                self._conv_call(self.fwd, lib.y3_conv2d_fwd_bf16_ws, src.v, self._at(mdl.params_t_bf16, sp.w_off), ptr(sp.b_off), 1, 1, fm.v, 1, 0, 0.0,
                                None, None, None)
                return fm
            self._conv_call(self.fwd, lib.y3_conv2d_fwd, src.v, ptr(sp.w_off), ptr(sp.b_off), 1, 1, fm.v, 0, 0.0, None, None, None, None)
            if i >= nfrozen:
                self.ops.append(('head', i, src, fm, _Layer(0, 0, 0, None)))      # the heads stay on the fp32 kernels
            return fm

        def upsample_into(src, dst):
            self._emit(self.fwd, lib.y3_upsample_sum2x_fwd_bf16 if bf else lib.y3_upsample_sum2x_fwd, src.v, dst.v)
            dst.frozen = src.no_grad      # (no parameters of its own: frozen with its producer)
            if not dst.frozen:
                self.ops.append(('upsample', src, dst))

        FC = YoloV3.FILTER_COUNT
        g1h, g1w = H // 32, W // 32
        cat2 = self._new(N, g1h * 2, g1w * 2, FC, dtype=act)         # tf.concat([up(512), route2(512)])  model.py:368
        cat3 = self._new(N, g1h * 4, g1w * 4, FC // 2, dtype=act)    # tf.concat([up(256), route1(256)])  model.py:375
        cat2_up, cat2_rt = cat2.slice(0, FC // 2), cat2.slice(FC // 2, FC // 2)
        cat3_up, cat3_rt = cat3.slice(0, FC // 4), cat3.slice(FC // 4, FC // 4)

        x = conv_layer(x0)
        x = conv_layer(x)
        x = feature_block(x, 1)
        x = conv_layer(x)
        x = feature_block(x, 2)
        x = conv_layer(x)
        route1 = x = feature_block(x, YoloV3.BLOCK_COUNT, out_last=cat3_rt)
        x = conv_layer(x)
        route2 = x = feature_block(x, YoloV3.BLOCK_COUNT, out_last=cat2_rt)
        x = conv_layer(x)
        route3 = feature_block(x, YoloV3.BLOCK_COUNT // 2)

        route, x = yolo_block(route3, mdl.spp)
        fm1 = head(x, 0)
        x = conv_layer(route)
        upsample_into(x, cat2_up)
        route, x = yolo_block(cat2)
        fm2 = head(x, 1)
        x = conv_layer(route)
        upsample_into(x, cat3_up)
        route, x = yolo_block(cat3)
        fm3 = head(x, 2)
        assert li[0] == len(specs)
        self.fms = [fm1, fm2, fm3]

        # decode (model.py:169-212)
        self.nb = sum(f.h * f.w * a for f, a in zip(self.fms, As))
        self.boxes = torch.empty(N, self.nb, 5 + K, dtype=torch.float32, device=dev)
        self.fm_arr = (_hip.Tensor * 3)(*[f.v for f in self.fms])
        if mdl.anchor_scale is None:
            self.decode_call = (lib.y3_decode_fwd, (self.fm_arr, 3, mdl.anchors_c, A, K, H, W, self.boxes.data_ptr()))
        else:      # rows coarse -> fine, then row, column, slot; each with its own anchor
            self.decode_call = (lib.y3_decode_fwd_scales, (self.fm_arr, mdl.anchors_c, mdl.anchor_scale_c, A, K, H, W, self.boxes.data_ptr()))

        # loss (model.py:214-354): always available (test_step needs it in inference mode too)
        self.gt = [torch.zeros(N, f.h, f.w, a, 5 + K, dtype=torch.float32, device=dev) for f, a in zip(self.fms, As)]
        self.loss4 = torch.zeros(4, dtype=torch.float32, device=dev)
        # one workspace PER SCALE (anchor-present flags + block partials): the three calls of a step then share no word that one
        # clears while another has set or reads it (round 3: a shared flag array cleared by a memset node was mis-ordered in a replayed graph)
        ws_floats = (int(lib.y3_loss_workspace_bytes()) // 4 + 4 + 63) // 64 * 64
        self.loss_ws = torch.zeros(3 * ws_floats, dtype=torch.float32, device=dev)
        self.loss_calls = []
        self.truth_call = self.truth_boxes = self.truth_counts = self.ignored = None
        if mdl.ignore_mask == 'truth':
            # the paper's ignore mask: per-image box lists gathered from the finest label tensor -- format_boxes
            # writes every box at all three scales (Q5) and the finest has the fewest cell collisions -- then the truth variant of
            # the loss at every scale.  All pointers are static: a captured step replays the gather with each step's labels.
            cap = mdl.max_truth_boxes
            self.truth_boxes = torch.zeros(N, cap, 4, dtype=torch.float32, device=dev)
            self.truth_counts = torch.zeros(N, dtype=torch.int32, device=dev)
            self.ignored = torch.zeros(1, dtype=torch.float32, device=dev)
            fine, gfine = self.fms[-1], self.gt[-1]
            if mdl.anchor_scale is None:
                self.truth_call = (lib.y3_truth_boxes, (gfine.data_ptr(), N, fine.h * fine.w * A, 5 + K, self.truth_boxes.data_ptr(),
                                                        self.truth_counts.data_ptr(), cap))
            else:      # a box lives on one scale only: the list is gathered from all three label tensors, coarse -> fine
                self.truth_call = (lib.y3_truth_boxes_scales, tuple(g.data_ptr() for g in self.gt) + (N,) +
                                   tuple(f.h * f.w * a for f, a in zip(self.fms, As)) +
                                   (5 + K, self.truth_boxes.data_ptr(), self.truth_counts.data_ptr(), cap))
            ws_floats = (int(lib.y3_loss_truth_workspace_bytes(N)) // 4 + 63) // 64 * 64
            self.loss_ws = torch.zeros(3 * ws_floats, dtype=torch.float32, device=dev)
        focal = mdl.focal_args()                 # None: no focal setting, the call list of a model built without one
        for si, (f, g) in enumerate(zip(self.fms, self.gt)):
            f.grad = self._new(N, f.h, f.w, Ds[si], Dlds[si], zero=True)
            anc, As_i = mdl.scale_anchors_c[si], As[si]      # this scale's anchors in slot order (all of them without a table)
            ws = self._at(self.loss_ws, si * ws_floats)
            if focal is not None:
                # focal objectness / class terms and label smoothing over either mask: null lists select the reference's
                truth = mdl.ignore_mask == 'truth'
                self.loss_calls.append((lib.y3_loss_fwd_bwd_focal, (f.v, g.data_ptr(), anc, As_i, K, H, W, float(mdl.global_batch_size),
                                                                    BOX_LOSSES.index(mdl.box_loss), mdl.box_loss_weight,
                                                                    self.truth_boxes.data_ptr() if truth else None,
                                                                    self.truth_counts.data_ptr() if truth else None,
                                                                    cap if truth else 1, mdl.ignore_thresh, self.loss4.data_ptr(),
                                                                    self.ignored.data_ptr() if truth else None, f.grad.v, ws) + focal))
            elif mdl.ignore_mask == 'truth':
                self.loss_calls.append((lib.y3_loss_fwd_bwd_truth, (f.v, g.data_ptr(), anc, As_i, K, H, W, float(mdl.global_batch_size),
                                                                    BOX_LOSSES.index(mdl.box_loss), mdl.box_loss_weight,
                                                                    self.truth_boxes.data_ptr(), self.truth_counts.data_ptr(), cap,
                                                                    mdl.ignore_thresh, self.loss4.data_ptr(), self.ignored.data_ptr(),
                                                                    f.grad.v, ws)))
            elif mdl.box_loss == 'mse':    # the reference's loss: the call list of a model built without box-loss arguments
                self.loss_calls.append((lib.y3_loss_fwd_bwd, (f.v, g.data_ptr(), anc, As_i, K, H, W, float(mdl.global_batch_size),
                                                              self.loss4.data_ptr(), f.grad.v, ws)))
            else:                        # IoU box term in loss4[0], loss4[1] stays 0
                self.loss_calls.append((lib.y3_loss_fwd_bwd_ex, (f.v, g.data_ptr(), anc, As_i, K, H, W, float(mdl.global_batch_size),
                                                                 BOX_LOSSES.index(mdl.box_loss), mdl.box_loss_weight,
                                                                 self.loss4.data_ptr(), f.grad.v, ws)))
            f.gw = True
        if tr:
            self._build_backward()
        self._bind_conv_workspace()

    # -- backward emission -------------------------------------------------------
    def _grad_of(self, t):
        """Gradient twin of activation t (allocated on first use; slices of a
        concat buffer get slices of the concat's gradient)."""
        if t.grad is None:
            if t.parent is not None:
                self._grad_of(t.parent)
                return t.grad
            t.grad = self._new(t.n, t.h, t.w, t.c, t.ld)
            for ch in t.children:
                ch.grad = _T(t.grad.buf, ch.n, ch.h, ch.w, ch.c, ch.ld, ch.off)
        return t.grad

    def _kernel_grad(self, fn, *args):
        """Emit a kernel gradient (args up to the workspace): on the main stream, or with a side stream there, between an event the
        main stream records now (the operands are complete) and one the side stream records behind the launch.  Every kernel
        gradient goes the same way: they share one slab workspace, in stream order.  Returns the index of that second event (None
        on the main stream): whoever overwrites an operand, or reads the result, waits for it."""
        args += (self.wg_ws.data_ptr(), self.wg_ws_bytes)
        if self.side is None:
            self._emit(self.bwd, fn, *args)
            return None
        self.events += [torch.cuda.Event(), torch.cuda.Event()]
        e_go, e_wg = len(self.events) - 2, len(self.events) - 1
        self.bwd.append(('record', e_go))
        self.keep.append(args)
        self.bwd.append(('side_call', (fn, args, e_go, e_wg)))
        return e_wg

    def _main_wait(self, e):
        if e is not None:
            self.bwd.append(('main_wait', e))

    def _build_backward(self):
        mdl = self.model
        specs = mdl.specs
        gptr = functools.partial(self._at, mdl.grads)

        wg_need = 0
        for op in self.ops:
            if op[0] in ('conv_layer', 'head'):
                sp = specs[op[1]]
                wg_need = max(wg_need, int(lib.y3_conv2d_wgrad_workspace_x(op[2].v, op[3].v, sp.k, sp.s, op[-1].wgrad)))     # (dz has op[3]'s geometry)
        self.wg_ws = torch.zeros(max(wg_need // 4, 4), dtype=torch.float32, device=mdl.device)      # tickets + slabs, zeroed once
        self.wg_ws_bytes = wg_need

        # BatchNorm-backward statistics without a pass of their own: the gradient dy of a layer's output is complete when the
        # data gradient of its FIRST consumer in forward order has run (later consumers -- residual adds, routes -- are
        # visited earlier by the reversed walk).  If that consumer is a convolution reading exactly this tensor and the
        # shape qualifies (y3_conv2d_dgrad_bn_tiles; stride 2: the merged launch), its data gradient sums the raw moments in its epilogue and
        # the producer only needs y3_bn_bwd_finalize_tiles; every other layer keeps y3_bn_bwd_stats.
        epi_of = {}            # id(consumer op) -> (producer activation a, partial buffer, tiles)
        epi_for = {}           # id(producer op) -> (partial buffer, tiles)
        first_consumer = {}
        for op in self.ops:
            reads = []
            if op[0] == 'conv_layer':
                reads = [op[2]] + ([op[5]] if op[5] is not None else [])
            elif op[0] == 'head':
                reads = [op[2]]
            elif op[0] in ('upsample', 'spp'):
                reads = [op[1]]
            for t in reads:
                first_consumer.setdefault(id(t), op)
                if t.parent is not None:
                    first_consumer.setdefault(id(t.parent), op)
                for ch in t.children:
                    first_consumer.setdefault(id(ch), op)
        for op in self.ops:
            if op[0] != 'conv_layer' or mdl.freeze_bn:      # (frozen statistics need no moments of dy: y3_bn_frozen_bwd, below)
                continue
            a, y = op[3], op[4]
            cons = first_consumer.get(id(y))
            if cons is None or cons[0] != 'conv_layer' or cons[2] is not y or y.children or y is self.x0:
                continue      # (a concat SLICE qualifies: later readers of the whole concat are visited earlier by the reversed walk)
            csp = specs[cons[1]]
            tiles = int(lib.y3_conv2d_dgrad_bn_tiles_x(cons[3].v, csp.k, csp.s, y.v, cons[-1].dgrad))      # (geometry only, as in conv_layer)
            if tiles <= 0:
                continue
            part = torch.empty(tiles * 6 * y.c, dtype=torch.float32, device=mdl.device)
            epi_of[id(cons)] = (a, part, tiles)
            epi_for[id(op)] = (part, tiles)
        self.epilogue_stats_layers = len(epi_for)
        # The kernel gradient of a layer and its data gradient both start from dz and are independent.  Each is a single
        # round of workgroups with ~8 us of prologue + epilogue in which the matrix pipe idles, so the kernel gradients go to
        # a second stream and fill those bubbles: 23.3 -> 21.4 ms per step with host launches.  (Replayed as a HIP graph
        # the two branches gained nothing -- 23.8 ms -- so a graph-captured step keeps one stream.)  dz is double-buffered:
        # bn_bwd_apply of layer i-2 waits for the kernel gradient of layer i that still reads the buffer.
        two = (not mdl.use_graph) and os.environ.get('Y3_WGRAD_STREAM', '1') != '0'
        self.side = streams.reserve(mdl.device)[0] if two else None      # one per device, bound to its hardware queue early (streams.py)
        self.events = []
        dz_bufs = [self.dz, torch.empty_like(self.dz)] if two else [self.dz]
        dz_busy = [None, None]          # event index of the wgrad still reading each dz buffer
        head_wg = None                  # ... of the newest head's
        nconv = 0
        for op in reversed(self.ops):
            kind = op[0]
            if kind == 'head':
                _, i, src, fm, _ = op
                sp = specs[i]
                dfm = fm.grad
                self._emit(self.bwd, lib.y3_colsum, dfm.v, gptr(sp.b_off))
                head_wg = self._kernel_grad(lib.y3_conv2d_wgrad, src.v, dfm.v, 1, 1, gptr(sp.w_off))
                if not src.no_grad:
                    ds = self._grad_of(src)
                    self._conv_call(self.bwd, lib.y3_conv2d_dgrad, dfm.v, self._at(mdl.params_t, sp.w_off), 1, 1, ds.v, EPI_ACCUM if src.gw else 0)
                    src.mark_written()
                self.bwd.append(('layer_done', i))
            elif kind == 'upsample':
                _, src, dst = op
                assert dst.gw and not src.gw
                ds = self._grad_of(src)
                self._emit(self.bwd, lib.y3_upsample_sum2x_bwd, dst.grad.v, ds.v)
                src.mark_written()
            elif kind == 'spp':
                # the data gradient of the layer behind the pools has written the whole concat gradient, slice 0 (the identity
                # branch) included: the pools' share is added to it, on the main stream, before the producer's BatchNorm backward
                _, src, cat, pools = op
                assert cat.gw and src.gw
                self._emit(self.bwd, lib.y3_spp_bwd, src.v, pools.grad.v, src.grad.v, 1)
            else:
                _, i, src, a, y, resid, x3 = op
                smean, srstd, coef = x3.bn
                sp = specs[i]
                assert y.gw, 'gradient of layer %d output never produced' % i
                dy = y.grad
                dr = None
                dr_acc = 0
                if resid is not None and not resid.no_grad:     # out = resid + y  ->  d resid += d out, fused into the pass that reads dy anyway
                    dr = self._grad_of(resid)
                    dr_acc = 1 if resid.gw else 0
                    resid.mark_written()
                slot = nconv % len(dz_bufs)
                nconv += 1
                dz = _T(dz_bufs[slot], a.n, a.h, a.w, sp.cout)
                self.keep.append(dz)
                epi = epi_for.get(id(op))
                if mdl.freeze_bn:
                    # frozen statistics: dz, the residual fan-in, dgamma / dbeta / dbias in ONE pass over dy and a (it writes dz: the
                    # kernel gradient of two layers ago must have left the buffer)
                    assert int(lib.y3_bn_frozen_bwd_workspace(a.m, sp.cout)) <= self.bnb_ws.numel()
                    self._main_wait(dz_busy[slot])
                    self._emit(self.bwd, lib.y3_bn_frozen_bwd, dy.v, a.v, dr.v if dr is not None else None, dr_acc,
                               self._at(mdl.chan, sp.ch_off), self._at(mdl.moving, sp.mv_off), self._at(mdl.moving, mdl.moving_stride + sp.mv_off),
                               BN_EPS, LRELU_ALPHA, dz.v, gptr(sp.g_off), gptr(sp.be_off), gptr(sp.b_off), self.bnb_ws.data_ptr(), self.bnb_ws.numel())
                elif epi is not None:
                    # the statistics were summed by the data gradient that completed dy: finalize, then apply (+ residual fan-in)
                    part, tiles = epi
                    self._emit(self.bwd, lib.y3_bn_bwd_finalize_tiles, part.data_ptr(), tiles, sp.cout, a.m, self._at(mdl.params, sp.g_off),
                               smean, srstd, LRELU_ALPHA, gptr(sp.g_off), gptr(sp.be_off), gptr(sp.b_off), coef)
                else:
                    assert int(lib.y3_bn_bwd_workspace(a.m, sp.cout)) <= self.bnb_ws.numel()
                    self._emit(self.bwd, lib.y3_bn_bwd_stats, dy.v, a.v, dr.v if dr is not None else None, dr_acc,
                               self._at(mdl.params, sp.g_off), smean, srstd, LRELU_ALPHA, gptr(sp.g_off), gptr(sp.be_off), gptr(sp.b_off), coef,
                               self.bnb_ws.data_ptr(), self.bnb_ws.numel())
                if not mdl.freeze_bn:
                    self._main_wait(dz_busy[slot])      # the kernel gradient of two layers ago still reads this dz buffer
                    if epi is not None and dr is not None:
                        self._emit(self.bwd, lib.y3_bn_bwd_apply_fanin, dy.v, a.v, coef, LRELU_ALPHA, dz.v, dr.v, dr_acc)
                    else:
                        self._emit(self.bwd, lib.y3_bn_bwd_apply, dy.v, a.v, coef, LRELU_ALPHA, dz.v)
                # (kernel gradient on the x3 arithmetic: both operands are activations, no weight copy involved)
                dz_busy[slot] = self._kernel_grad(lib.y3_conv2d_wgrad_x, src.v, dz.v, sp.k, sp.s, gptr(sp.w_off), x3.wgrad)
                if x3.wgrad:
                    self.x3_wgrad.append(i)
                if not src.no_grad:
                    ds = self._grad_of(src)
                    # x3 data gradient: the kernel wants K (= this layer's output channels) contiguous per column: the planes of the Keras arena
                    wdg = self._at(mdl.planes, sp.w_off) if x3.dgrad else self._at(mdl.params_t, sp.w_off)
                    dflags = (EPI_ACCUM if src.gw else 0) | x3.dgrad
                    if x3.dgrad:
                        self.x3_dgrad.append(i)
                    if id(op) in epi_of:      # this launch completes d(src): it also sums the BatchNorm-backward moments of the producer
                        pa, part, _ = epi_of[id(op)]
                        self._conv_call(self.bwd, lib.y3_conv2d_dgrad_bn, dz.v, wdg, sp.k, sp.s, ds.v, dflags, pa.v, part.data_ptr())
                        self.keep.append(part)
                    else:
                        self._conv_call(self.bwd, lib.y3_conv2d_dgrad, dz.v, wdg, sp.k, sp.s, ds.v, dflags)
                    src.mark_written()
                self.bwd.append(('layer_done', i))
        for e in dz_busy + [head_wg]:
            self._main_wait(e)

    # -- execution -------------------------------------------------------------------
    def _run(self, lst, stream, dist=None):
        main = None
        pending = []                   # kernel gradients in flight on the side stream (event indices)
        for fn, args in lst:
            if fn == 'layer_done':
                if dist is not None:
                    if pending and dist.ends_bucket(args):
                        for e in pending:          # a gradient bucket is about to be all-reduced: its kernel gradients must be in
                            main.wait_event(self.events[e])
                        pending = []
                    dist.on_layer_done(args)
                continue
            if fn in ('record', 'main_wait', 'side_call'):
                if main is None:
                    main = torch.cuda.current_stream(self.model.device)
                if fn == 'record':
                    self.events[args].record(main)
                elif fn == 'main_wait':
                    main.wait_event(self.events[args])
                else:
                    f2, a2, e_wait, e_done = args
                    self.side.wait_event(self.events[e_wait])
                    rc = f2(*a2, self.side.cuda_stream)
                    if rc != 0:
                        check(rc, f2.__name__)
                    self.events[e_done].record(self.side)
                    pending.append(e_done)
                continue
            rc = fn(*args, stream)
            if rc != 0:
                check(rc, fn.__name__)

    def run_forward(self, stream, skip_input=False):
        self._run(self.fwd[1:] if skip_input else self.fwd, stream)      # fwd[0] is the NCHW -> NHWC transpose of the input

    def run_decode(self, stream):
        fn, args = self.decode_call
        check(fn(*args, stream), fn.__name__)

    def run_inference(self, stream, skip_input=False):
        self.run_forward(stream, skip_input)
        self.run_decode(stream)

    def run_loss(self, stream):
        # (a kernel launch, not tensor.zero_(): inside a captured step nothing may turn into a memset node -- DESIGN 9)
        check(lib.y3_fill(self.loss4.data_ptr(), 4, 0.0, stream), 'y3_fill')
        if self.truth_call is not None:
            check(lib.y3_fill(self.ignored.data_ptr(), 1, 0.0, stream), 'y3_fill')
            fn, args = self.truth_call
            check(fn(*args, stream), fn.__name__)
        for fn, args in self.loss_calls:
            check(fn(*args, stream), fn.__name__)

    def run_backward(self, stream, dist=None):
        """dist: the model's DataParallel (all-reduces each gradient bucket as its last layer completes), or None."""
        self._run(self.bwd, stream, dist)


class _CallableModel:
    """What get_keras_model()/get_keras_feature_map_model() hand out: callable
    like a Keras model, ``m(batch, training=False)`` (inference.py:58)."""

    def __init__(self, yolo, feature_maps):
        self._y = yolo
        self._fm = feature_maps

    supports_slots = True      # __call__(..., slot=k): k-th independent set of activation buffers (concurrent streams)

    def __call__(self, batch, training=False, slot=0):
        if self._fm:
            return self._y.feature_maps(batch, training=training)
        return self._y.predict(batch, slot=slot)

    def run_tiles(self, img_dev, dtype_code, img_shape, table_ptr, count, tile_size=None, slot=0, views=None):
        """inference_tiled's fast path: gather + z-score + forward + decode of `count` tiles (YoloV3.predict_tiles).  views: the
        test-time augmentation view codes; the rows of all views of a tile then come back pooled (YoloV3.predict_tiles_tta)."""
        if views is not None:
            return self._y.predict_tiles_tta(img_dev, dtype_code, img_shape, table_ptr, count, views, tile_size=tile_size, slot=slot)
        return self._y.predict_tiles(img_dev, dtype_code, img_shape, table_ptr, count, tile_size=tile_size, slot=slot)

    @property
    def trainable_weights(self):
        return self._y.trainable_weights()


class YoloV3:
    # Constants controlling the network (model.py:22-26)
    BLOCK_COUNT = 8
    FILTER_COUNT = 1024
    KERNEL_SIZE = 3
    NETWORK_DOWNSAMPLE_FACTOR = 32
    WEIGHT_DECAY = 5e-4      # declared by the reference but never applied (Q9)

    def __init__(self, global_batch_size, img_size, number_classes, anchors=None, learning_rate=1e-4, device=None, seed=None,
                 use_graph=False, inference_precision='fp32', conv_arithmetic=None, ema_decay=None, ema_warmup=2000,
                 box_loss='mse', box_loss_weight=1.0, accumulate_steps=1, grad_clip_norm=None, train_sizes=None,
                 ignore_mask='reference', ignore_thresh=DEFAULT_IGNORE_THRESH, max_truth_boxes=DEFAULT_MAX_TRUTH_BOXES,
                 focal_gamma=0.0, focal_alpha=0.0, focal_terms='both', label_smoothing=0.0, spp=False, optimizer='adam', momentum=0.9,
                 nesterov=False, weight_decay=0.0, lr_schedule=None, freeze_layers=0, freeze_bn=False, anchor_scales=None):
        """freeze_layers / freeze_bn are settings of a training run, not of the network: save_weights does not
        record them (inference does not care), from_file builds a model without them, and every run names them again.
        anchor_scales: None = every anchor on every scale, the reference's network; 'auto'
        (anchors.default_anchor_scales), an owner table [A] or three index lists coarse -> fine give each anchor to one scale:
        head s has A_s (5 + K) channels and the labels are [N, G, G, A_s, 5+K].  Part of the network: weight files record it."""
        # per-scale anchor assignment: checked before the device is needed
        given = [(32, 32), (128, 128), (256, 256)] if anchors is None else [tuple(a) for a in anchors]
        self.anchor_scale = resolve_anchor_scales(anchor_scales, given)
        # the optimiser: 'adam' without decay = the reference's Keras Adam and its launches; 'adamw' / 'sgd' run
        # y3_optim_step; lr_schedule: None or an object with factor(t) (schedule.LrSchedule); checked before the device is needed
        check_optimizer_args(optimizer, momentum, nesterov, weight_decay, lr_schedule)
        self.optimizer_kind = optimizer
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        self.weight_decay = float(weight_decay)
        self.lr_schedule = lr_schedule
        # the YOLOv3-SPP variant of the network: False = the reference's Darknet-53 with three plain heads
        if not (isinstance(spp, (bool, np.bool_)) or (isinstance(spp, (int, np.integer)) and spp in (0, 1))):
            raise ValueError('spp must be False or True, got {!r}'.format(spp))
        self.spp = bool(spp)
        # fine-tuning: layers 0 .. freeze_layers - 1 are not trainable (Keras layer.trainable = False, BatchNorm
        # included: they run as in inference); freeze_bn: the BatchNorm of the trainable layers normalises with the moving
        # statistics, which then stay.  0 / False = every layer trains, today's launches; checked before the device is needed
        check_freeze_args(freeze_layers, freeze_bn, len(build_layer_specs(int(img_size[2]), len(given), int(number_classes), self.spp)[0]))
        self.freeze_layers = int(freeze_layers)
        self.freeze_bn = bool(freeze_bn)
        # input sizes train_step / test_step accept: None = img_size only; checked before the device is needed
        self.train_sizes = check_train_sizes(img_size, train_sizes)
        # gradient accumulation and global-norm clipping: 1 / None = off; checked before the device is needed
        check_grad_args(accumulate_steps, grad_clip_norm)
        self.accumulate_steps = int(accumulate_steps)
        self.grad_clip_norm = float(grad_clip_norm) if grad_clip_norm is not None else None
        self.micro_step = 0                       # micro-steps of the pending optimiser step already taken: 0 .. accumulate_steps - 1
        # box-regression term of the loss: 'mse' = the reference's xy + wh terms; checked before the device is needed
        check_box_loss_args(box_loss, box_loss_weight)
        self.box_loss = box_loss
        self.box_loss_weight = float(box_loss_weight)
        # ignore mask of the objectness loss: 'reference' = the reference's (Q7), 'truth' = the paper's, against each
        # image's own ground-truth boxes; checked before the device is needed
        check_ignore_mask_args(ignore_mask, ignore_thresh, max_truth_boxes)
        self.ignore_mask = ignore_mask
        self.ignore_thresh = float(ignore_thresh)
        self.max_truth_boxes = int(max_truth_boxes)
        # focal form of the objectness / class terms and class-label smoothing: all 0 = the reference's plain sigmoid
        # cross-entropy and its launches; checked before the device is needed
        check_focal_args(focal_gamma, focal_alpha, focal_terms, label_smoothing)
        self.focal_gamma = float(focal_gamma)
        self.focal_alpha = float(focal_alpha)
        self.focal_terms = focal_terms
        self.label_smoothing = float(label_smoothing)
        self._loss_plan = None                    # the plan whose loss ran last: what last_ignored / last_truth_max read
        # exponential moving average of the weights: None / 0 = off; checked before the device is needed
        if ema_decay is not None and ema_decay != 0 and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError('ema_decay must be None (off) or in (0, 1), got %r' % (ema_decay,))
        if ema_decay and not float(ema_warmup) > 0.0:
            raise ValueError('ema_warmup must be > 0, got %r' % (ema_warmup,))
        if not torch.cuda.is_available():
            raise RuntimeError('yolo3.model.YoloV3 needs an MI355X (HIP) device: there is no CPU path')
        self.device = torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())
        self.number_classes = int(number_classes)
        self.learning_rate = float(learning_rate)
        self.global_batch_size = global_batch_size
        self.img_size = [int(v) for v in img_size]           # [H, W, C]  (model.py:428,440)
        if self.img_size[0] % 32 or self.img_size[1] % 32:
            raise ValueError('image size must be a multiple of %d' % YoloV3.NETWORK_DOWNSAMPLE_FACTOR)
        self.score_threshold = 0.1                           # dead attributes kept (Q10)
        self.iou_threshold = 0.5
        self.anchors = [(32, 32), (128, 128), (256, 256)] if anchors is None else [tuple(a) for a in anchors]
        self.number_anchors = len(self.anchors)
        self.anchors_c = _hip.float_array([v for a in self.anchors for v in a])
        # what each scale's loss call and head see: all anchors, or with an owner table the anchors the scale owns, in slot order
        if self.anchor_scale is None:
            self.anchor_scale_c = None
            self.scale_anchor_counts = [self.number_anchors] * 3
            self.scale_anchors_c = [self.anchors_c] * 3
        else:
            self.anchor_scale_c = _hip.int_array(self.anchor_scale)
            masks = scale_masks(self.anchor_scale)
            self.scale_anchor_counts = [len(m) for m in masks]
            self.scale_anchors_c = [_hip.float_array([v for a in m for v in self.anchors[a]]) for m in masks]
        H, W, C = self.img_size
        f = YoloV3.NETWORK_DOWNSAMPLE_FACTOR
        self.box_count_fm1 = (H / f) * (W / f)
        self.box_count_fm2 = (H / (f / 2)) * (W / (f / 2))
        self.box_count_fm3 = (H / (f / 4)) * (W / (f / 4))
        self.number_output_boxes = self.number_anchors * (self.box_count_fm1 + self.box_count_fm2 + self.box_count_fm3)
        if self.anchor_scale is not None:
            self.number_output_boxes = sum(a * c for a, c in zip(self.scale_anchor_counts, (self.box_count_fm1, self.box_count_fm2, self.box_count_fm3)))
        self.output_shape = [self.number_output_boxes, 5 + self.number_classes]

        self.specs, self.arena_floats, chan_floats, self.moving_stride = build_layer_specs(
            C, self.number_anchors, self.number_classes, self.spp, None if self.anchor_scale is None else self.scale_anchor_counts)
        # the part of the arenas a step touches: everything with no layer frozen (trainable_suffix)
        self.train_off, self.train_floats = trainable_suffix(self.specs, self.arena_floats, self.freeze_layers)
        dev = self.device
        z = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
        self.params = z(self.arena_floats)        # trainable arena: [W | b | gamma | beta] per layer
        self.params_t = z(self.arena_floats)      # kernels with channel axes swapped (dgrad operand)
        self.grads = z(self.arena_floats)
        self.adam_m = z(self.arena_floats)        # first moment; the momentum buffer of 'sgd'
        self.adam_v = z(self.arena_floats) if self.optimizer_kind != 'sgd' else None      # 'sgd' has no second moment
        self.moving = z(2 * self.moving_stride)   # [moving_mean | moving_var]
        self.chan = z(chan_floats)                # per BN layer: scale | shift | save_mean | save_rstd | k1 | k2 | k3
        # what the optimiser kernel reads per step: lr_t for 'adam'; {lr, 0} for 'sgd', {lr_t, lr * weight_decay} for 'adamw'
        self.hyper_dev = z(2)
        self.lr_t_dev = self.hyper_dev[0:1]
        self.beta1, self.beta2, self.adam_eps = 0.9, 0.999, 1e-7   # Keras Adam defaults (App. C5)
        self.iterations = 0
        # the average (ema_params, ema_moving) and the stash ema_weights() parks the live arenas in; None when off
        self.ema_decay = float(ema_decay) if ema_decay else None
        self.ema_warmup = float(ema_warmup)
        self.ema_params = self.ema_moving = self.ema_omd_dev = None
        self._ema_stash = None
        self._ema_swapped = False
        if self.ema_decay is not None:
            self.ema_params = z(self.arena_floats)
            self.ema_moving = z(2 * self.moving_stride)
            self.ema_omd_dev = z(1)
            self._ema_stash = (z(self.arena_floats), z(2 * self.moving_stride))
        # accumulator (only with accumulate_steps > 1), the fp64 per-block partial sums of squares, and the scalars the kernels
        # hand each other in device memory: `first` of the accumulate pass, the pre-clip norm, the scale of the Adam pass
        self.grad_acc = self.last_grad_norm = self.grad_scale_dev = self._grad_ws = self._acc_first_dev = self._grad_scalars = None
        if self.accumulate_steps > 1 or self.grad_clip_norm is not None:
            if self.accumulate_steps > 1:
                self.grad_acc = z(self.arena_floats)
                self._acc_first_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self._grad_ws = torch.zeros(int(lib.y3_grad_norm_workspace_bytes(self.arena_floats)) // 8, dtype=torch.float64, device=dev)
            self._grad_scalars = z(2)
            self.last_grad_norm = self._grad_scalars[0]      # 0-d views: the values of the last optimiser step, read when used
            self.grad_scale_dev = self._grad_scalars[1]
        self.use_graph = bool(use_graph)
        if inference_precision not in ('fp32', 'bf16'):
            raise ValueError("inference_precision must be 'fp32' or 'bf16'")
        self.inference_precision = inference_precision   # predict() default; training is always fp32
        # fp32 convolutions: 'f32' = v_mfma_f32_32x32x2_f32 everywhere; 'x3' = the layers named by x3_forward / x3_dgrad run their
        # fp32 arithmetic as three bf16 pieces per operand on the bf16 matrix pipe (Y3_CONV_X3, conv_x3.hip: fp32-class results,
        # 2.67x fewer matrix-pipe cycles).  Default 'x3'; environment Y3_CONV_X3=0 / 1 / all overrides the default.
        if conv_arithmetic is None:
            conv_arithmetic = {'0': 'f32', '1': 'x3', 'all': 'x3-all'}.get(os.environ.get('Y3_CONV_X3', '1'), 'x3')
        if conv_arithmetic not in ('f32', 'x3', 'x3-all'):
            raise ValueError("conv_arithmetic must be 'f32' or 'x3'")
        self.conv_arithmetic = conv_arithmetic
        # the x3 kernels read their weights as three bf16 piece planes (y3_x3_split_weights) of the copy with K contiguous per output
        # column: of params_t in the forward pass, of params in the data gradient; refreshed with params_t after every optimiser step
        self.planes = self.planes_t = None
        if conv_arithmetic != 'f32':
            self.planes = torch.zeros(3 * self.arena_floats, dtype=torch.bfloat16, device=dev)
            self.planes_t = torch.zeros(3 * self.arena_floats, dtype=torch.bfloat16, device=dev)
        self._x3_table = None
        self.params_t_bf16 = None                 # bf16 copy of params_t, made on first bf16 predict
        self._bf16_stale = True
        self.dist = None                          # set by parallel.DataParallel.attach()
        self._plans = {}
        self._lb_staging = {}        # slot -> pinned and device byte buffers of predict_letterbox
        self._tr_table = None
        self._tr_suffix = None
        self._fold_table = None
        self._adam_call = self._adam_launch()
        self._init_weights(seed)
        if self.freeze_layers:
            self._refresh_transposed_from(self.freeze_layers, launch=False)      # the tables of the optimiser step's refresh
        self.model = _CallableModel(self, False)
        self.model_feature_maps = _CallableModel(self, True)
        self.optimizer = self

    # ---- which launches run the x3 kernels ---------------------------------------
    def x3_forward(self, sp, m_out):
        if self.conv_arithmetic == 'f32' or not lib.y3_conv2d_x3_ok(m_out, sp.cin_pad, sp.k * sp.k, sp.cout):
            return False
        # measured (tools/x3_check.py --all, tools/layer_times.py; batch 8 at 416^2, launch by launch and inside the step): the 3x3
        # layers gain -- every one the kernels take (>= 32 input channels): 208^2 32->64 140 -> 116 us, the others 1.5-1.8x; the 1x1
        # layers (4-64 K steps: prologue + epilogue bound) do not
        return self.conv_arithmetic == 'x3-all' or sp.k == 3

    def x3_dgrad(self, ddst, k, s, dsrc):
        """ddst, dsrc: views with the geometry of the gradients of the layer's output (its channels are contracted) and input.  The
        shapes the kernels take are the library's to say, for both strides; the policy below is measured."""
        if self.conv_arithmetic == 'f32' or not lib.y3_conv2d_dgrad_x3_ok(ddst, k, s, dsrc):
            return False
        if self.conv_arithmetic == 'x3-all':
            return True
        if k != 3:
            return False      # the 1x1 layers do not gain (x3_forward)
        if s == 2:
            # the merged launch of the four parity classes; measured (tools/layer_times.py): 163 -> 125, 151 -> 124, 142 -> 103 us at
            # 13^2 / 26^2 / 52^2 output; 152 -> 151 for the 64-channel layer
            return dsrc.c >= 128
        # measured (as x3_forward): stride-1 data gradients 1.1-1.7x with >= 128 contracted channels and >= 64 outputs (0.79x for the
        # 64 -> 32 one)
        return ddst.c >= 128 and dsrc.c >= 64

    def x3_wgrad(self, sp, m_out):
        if self.conv_arithmetic == 'f32' or not lib.y3_conv2d_wgrad_x3_ok(m_out, sp.cin_pad, sp.k, sp.cout):
            return False
        # measured (tools/x3_check.py --wgrad): every 3x3 layer with >= 128 output channels 1.3-1.7x, stride 2 included; the 1x1
        # layers 1.1-1.2x at 52^2 / 26^2 and slower at 13^2
        return self.conv_arithmetic == 'x3-all' or sp.k == 3 or m_out >= 5000

    # ---- construction helpers --------------------------------------------------
    def _init_weights(self, seed):
        """Keras defaults: Glorot-uniform kernels, zero bias, gamma 1, beta 0,
        moving mean 0 / variance 1 (App. C2, C4)."""
        rng = np.random.default_rng(seed)
        layers = []
        for sp in self.specs:
            limit = math.sqrt(6.0 / (sp.k * sp.k * sp.cin + sp.k * sp.k * sp.cout))
            d = dict(W=rng.uniform(-limit, limit, (sp.k, sp.k, sp.cin, sp.cout)).astype(np.float32), b=np.zeros(sp.cout, np.float32))
            if sp.bn:
                d.update(gamma=np.ones(sp.cout, np.float32), beta=np.zeros(sp.cout, np.float32), mean=np.zeros(sp.cout, np.float32),
                         var=np.ones(sp.cout, np.float32))
            layers.append(d)
        self.set_weights(layers)

    # ---- weights in / out (Keras shapes, true Cin) --------------------------------------
    def set_weights(self, layers):
        """layers: list (creation order) of dicts W[kh,kw,Cin,Cout], b, and for
        conv_layers gamma, beta, mean, var."""
        assert len(layers) == len(self.specs)
        host = np.zeros(self.arena_floats, np.float32)
        mov = np.zeros(2 * self.moving_stride, np.float32)
        mov[self.moving_stride:] = 1.0
        for sp, d in zip(self.specs, layers):
            Wk = np.asarray(d['W'], np.float32)
            assert Wk.shape == (sp.k, sp.k, sp.cin, sp.cout), (Wk.shape, (sp.k, sp.k, sp.cin, sp.cout))
            Wp = np.zeros((sp.k, sp.k, sp.cin_pad, sp.cout), np.float32)
            Wp[:, :, :sp.cin, :] = Wk
            host[sp.w_off:sp.w_off + Wp.size] = Wp.ravel()
            host[sp.b_off:sp.b_off + sp.cout] = np.asarray(d['b'], np.float32)
            if sp.bn:
                host[sp.g_off:sp.g_off + sp.cout] = np.asarray(d['gamma'], np.float32)
                host[sp.be_off:sp.be_off + sp.cout] = np.asarray(d['beta'], np.float32)
                mov[sp.mv_off:sp.mv_off + sp.cout] = np.asarray(d['mean'], np.float32)
                mov[self.moving_stride + sp.mv_off:self.moving_stride + sp.mv_off + sp.cout] = np.asarray(d['var'], np.float32)
        self.params.copy_(torch.from_numpy(host))
        self.moving.copy_(torch.from_numpy(mov))
        self._refresh_transposed()
        self.reset_ema()

    # ---- exponential moving average of the weights ---------------------------
    def reset_ema(self):
        """Restart the average from the current weights and moving statistics (no-op when the EMA is off).  set_weights does
        it; a data-parallel trainer calls it again after broadcasting rank 0's weights.  Either way a half-accumulated optimiser
        step is dropped (micro_step back to 0: its gradients belong to other weights)."""
        self.micro_step = 0
        if self.ema_decay is None:
            return
        if self._ema_swapped:
            raise RuntimeError('reset_ema inside ema_weights()')
        self.ema_params.copy_(self.params)
        self.ema_moving.copy_(self.moving)

    def _ema_omd(self):
        return ema_one_minus_decay(self.ema_decay, self.ema_warmup, self.iterations)

    @contextlib.contextmanager
    def ema_weights(self, moving=None):
        """Within the block the model IS the average: ema_params in params, ema_moving (or `moving`, e.g. the cross-replica
        mean) in moving, derived weight copies refreshed; predict / predict_tiles / test_step / get_weights / save_weights
        all see it.  The arenas are copied in place (plans and captured graphs hold their raw pointers) and restored on
        exit, with the derived copies rebuilt from the restored weights (the same bits as before).  No training inside."""
        if self.ema_decay is None:
            raise RuntimeError('ema_weights(): this model keeps no average (ema_decay=None)')
        if self._ema_swapped:
            raise RuntimeError('ema_weights() does not nest')
        sp, sm = self._ema_stash
        sp.copy_(self.params)
        sm.copy_(self.moving)
        self.params.copy_(self.ema_params)
        self.moving.copy_(self.ema_moving if moving is None else moving)
        self._refresh_transposed()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self.params.copy_(sp)
            self.moving.copy_(sm)
            self._refresh_transposed()
            self._ema_swapped = False

    def _unpack(self, arena):
        host = arena.detach().cpu().numpy()
        out = []
        for sp in self.specs:
            Wp = host[sp.w_off:sp.w_off + sp.k * sp.k * sp.cin_pad * sp.cout].reshape(sp.k, sp.k, sp.cin_pad, sp.cout)
            d = dict(W=Wp[:, :, :sp.cin, :].copy(), b=host[sp.b_off:sp.b_off + sp.cout].copy())
            if sp.bn:
                d['gamma'] = host[sp.g_off:sp.g_off + sp.cout].copy()
                d['beta'] = host[sp.be_off:sp.be_off + sp.cout].copy()
            out.append(d)
        return out

    def get_weights(self, moving=None):
        """moving: optional replacement for self.moving (the cross-replica MEAN a checkpoint stores, parallel.mean_moving_stats)."""
        out = self._unpack(self.params)
        mov = (self.moving if moving is None else moving).detach().cpu().numpy()
        for sp, d in zip(self.specs, out):
            if sp.bn:
                d['mean'] = mov[sp.mv_off:sp.mv_off + sp.cout].copy()
                d['var'] = mov[self.moving_stride + sp.mv_off:self.moving_stride + sp.mv_off + sp.cout].copy()
        return out

    def get_gradients(self):
        """Last step's gradients, same structure as get_weights() (W, b, gamma, beta)."""
        return self._unpack(self.grads)

    def trainable_weights(self):
        """Flat list of arrays in Keras trainable_weights order (model.py:496)."""
        out = []
        for sp, d in zip(self.specs, self._unpack(self.params)):
            out += [d['W'], d['b']] + ([d['gamma'], d['beta']] if sp.bn else [])
        return out

    def focal_args(self):
        """The five trailing arguments of y3_loss_fwd_bwd_focal, or None when no focal setting is on (gamma, alpha and label
        smoothing all 0): the plans then emit the launches they emitted before the setting existed."""
        if self.focal_gamma == 0.0 and self.focal_alpha == 0.0 and self.label_smoothing == 0.0:
            return None
        return focal_term_args(self.focal_gamma, self.focal_alpha, self.focal_terms, self.label_smoothing)

    def save_weights(self, path, moving=None):
        """Own weight file (the reference's TF checkpoint / SavedModel formats need TF)."""
        flat = {}
        for i, d in enumerate(self.get_weights(moving)):
            for k, v in d.items():
                flat['l%03d_%s' % (i, k)] = v
        flat['meta_img_size'] = np.asarray(self.img_size, np.int64)
        flat['meta_number_classes'] = np.asarray(self.number_classes, np.int64)
        flat['meta_anchors'] = np.asarray(self.anchors, np.float32)
        flat['meta_global_batch_size'] = np.asarray(self.global_batch_size, np.int64)
        flat['meta_learning_rate'] = np.asarray(self.learning_rate, np.float64)
        if self.focal_args() is not None:         # a file written without a focal setting keeps the entries it had
            flat['meta_focal'] = np.asarray([self.focal_gamma, self.focal_alpha, self.label_smoothing], np.float64)
            flat['meta_focal_terms'] = np.asarray(self.focal_terms)
        if self.spp:                              # likewise: a file of the reference's network has no such entry
            flat['meta_spp'] = np.asarray(1, np.int64)
        if getattr(self, 'anchor_scale', None) is not None:       # likewise: the owner table, one scale per anchor
            flat['meta_anchor_scale'] = np.asarray(self.anchor_scale, np.int64)
        if getattr(self, 'optimizer_kind', 'adam') != 'adam':       # likewise: a file of the reference's Adam has no such entry
            flat['meta_optimizer'] = np.asarray(self.optimizer_kind)
            flat['meta_optimizer_args'] = np.asarray([self.momentum, float(self.nesterov), self.weight_decay], np.float64)
        flat['opt_iterations'] = np.asarray(self.iterations, np.int64)
        flat['opt_m'] = self.adam_m.detach().cpu().numpy()
        if self.adam_v is not None:               # 'sgd' has no second moment
            flat['opt_v'] = self.adam_v.detach().cpu().numpy()
        np.savez(path, **flat)

    @staticmethod
    def _optimizer_meta(z):
        """The optimiser setting a weight file carries (save_weights), as constructor arguments; none for a file without it."""
        if 'meta_optimizer' not in z:
            return {}
        mu, nes, wd = (float(v) for v in z['meta_optimizer_args'])
        return dict(optimizer=str(z['meta_optimizer']), momentum=mu, nesterov=bool(nes), weight_decay=wd)

    def load_weights(self, path, load_optimizer=False, transfer=False):
        """transfer=True: a file of the plain network into an SPP model -- every layer by role, the 4 * 512 -> 512 layer behind
        the pools keeps its initialisation, no optimiser state (spp_transfer_map)."""
        z = np.load(path, allow_pickle=False)
        theirs = YoloV3._spp_meta(z)
        if transfer:
            if load_optimizer:
                raise ValueError('load_weights: transfer=True loads no optimiser state')
            if theirs or not self.spp:
                raise ValueError('load_weights: transfer=True loads a file written with spp=False into a model with spp=True; {} has spp={}, '
                                 'this model has spp={}'.format(path, theirs, self.spp))
            mapping = spp_transfer_map(self.specs)
        elif theirs != self.spp:
            raise ValueError('load_weights: {} was written with spp={}, this model has spp={} (the two networks differ by one layer; '
                             'transfer=True loads a plain file into an SPP model)'.format(path, theirs, self.spp))
        else:
            mapping = list(range(len(self.specs)))
        mine_scale = getattr(self, 'anchor_scale', None)
        if YoloV3._anchor_scale_meta(z) != mine_scale:
            raise ValueError('load_weights: {} was written with anchor_scale {}, this model has {} (None: every anchor on every scale); '
                             'the heads differ'.format(path, YoloV3._anchor_scale_meta(z), mine_scale))
        mine = dict(focal_gamma=self.focal_gamma, focal_alpha=self.focal_alpha, focal_terms=self.focal_terms,
                    label_smoothing=self.label_smoothing) if self.focal_args() is not None else {}
        if YoloV3._focal_meta(z) != mine:          # the weights load all the same; the losses of the two settings are not comparable
            warnings.warn('load_weights: {} was written with focal setting {}, this model has {}'.format(path, YoloV3._focal_meta(z) or 'none',
                                                                                                         mine or 'none'))
        if load_optimizer and 'opt_m' in z:
            # the moments of one optimiser mean nothing to another (the momentum buffer of 'sgd' is no first moment)
            theirs_opt = YoloV3._optimizer_meta(z).get('optimizer', 'adam')
            if theirs_opt != self.optimizer_kind:
                raise ValueError("load_weights: load_optimizer=True, but {} holds the state of optimizer '{}' and this model has '{}'"
                                 .format(path, theirs_opt, self.optimizer_kind))
        layers = []
        own = self.get_weights() if transfer else None
        for (i, sp), j in zip(enumerate(self.specs), mapping):
            if j is None:
                print('load_weights: layer %d (1x1 %d -> %d behind the pools) is not in %s and keeps its initialisation' % (i, sp.cin, sp.cout, path))
                layers.append(own[i])
                continue
            d = {k: z['l%03d_%s' % (j, k)] for k in (['W', 'b', 'gamma', 'beta', 'mean', 'var'] if sp.bn else ['W', 'b'])}
            layers.append(d)
        self.set_weights(layers)
        if load_optimizer and 'opt_m' in z:
            self.adam_m.copy_(torch.from_numpy(z['opt_m']))
            if self.adam_v is not None:
                self.adam_v.copy_(torch.from_numpy(z['opt_v']))
            self.iterations = int(z['opt_iterations'])

    def load_pretrained(self, path):
        """Start fine-tuning from a file written by save_weights.  The model may differ from the file's in
        number_classes, anchors (values or count per scale), global_batch_size, learning rate and optimiser: layers are matched by
        role (pretrained_map; a plain file into an SPP model goes through spp_transfer_map), heads of equal shape load, and a
        detection head of another shape keeps its initialisation and is named in a printed line.  No optimiser state is loaded and
        `iterations` stays as it is (0 in a fresh model); the EMA restarts from the loaded weights (set_weights).  Raises ValueError
        for an SPP file into a plain model and for another input channel count.  Returns the indices of the layers that kept their
        initialisation."""
        z = np.load(path, allow_pickle=False)
        n_file = 0
        while 'l%03d_W' % n_file in z:
            n_file += 1
        mapping, kept = pretrained_map(self.specs, self.spp, [z['l%03d_W' % j].shape for j in range(n_file)], YoloV3._spp_meta(z))
        own = self.get_weights()
        layers = []
        for (i, sp), j in zip(enumerate(self.specs), mapping):
            if j is None:
                print('load_pretrained: layer %d (%s %dx%d %d -> %d) is not in %s with this shape and keeps its initialisation'
                      % (i, 'conv' if sp.bn else 'detection head', sp.k, sp.k, sp.cin, sp.cout, path))
                layers.append(own[i])
                continue
            layers.append({k: z['l%03d_%s' % (j, k)] for k in (['W', 'b', 'gamma', 'beta', 'mean', 'var'] if sp.bn else ['W', 'b'])})
        self.set_weights(layers)
        return kept

    @staticmethod
    def _focal_meta(z):
        """The focal settings a weight file carries (save_weights), as constructor arguments; none for a file without them."""
        if 'meta_focal' not in z:
            return {}
        g, a, e = (float(v) for v in z['meta_focal'])
        return dict(focal_gamma=g, focal_alpha=a, focal_terms=str(z['meta_focal_terms']), label_smoothing=e)

    @staticmethod
    def _spp_meta(z):
        """Whether a weight file holds the SPP network (save_weights); a file without the entry holds the plain one."""
        return bool(int(z['meta_spp'])) if 'meta_spp' in z else False

    @staticmethod
    def _anchor_scale_meta(z):
        """The owner table a weight file carries (save_weights); None for a file without one: every anchor on every scale."""
        return [int(v) for v in z['meta_anchor_scale']] if 'meta_anchor_scale' in z else None

    @staticmethod
    def from_file(path, device=None, lr_schedule=None):
        """The model a weight file describes, with its weights.  The file records the network, the focal setting and the optimiser;
        the learning-rate schedule is the caller's to pass, like box_loss to the constructor."""
        z = np.load(path, allow_pickle=False)
        y = YoloV3(int(z['meta_global_batch_size']), [int(v) for v in z['meta_img_size']], int(z['meta_number_classes']),
                   [tuple(float(v) for v in a) for a in z['meta_anchors']], float(z['meta_learning_rate']), device=device, spp=YoloV3._spp_meta(z), **YoloV3._focal_meta(z),
                   **YoloV3._optimizer_meta(z), lr_schedule=lr_schedule, anchor_scales=YoloV3._anchor_scale_meta(z))
        y.load_weights(path)
        return y

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _refresh_transposed(self, first=0):
        """params_t <- kernels with the channel axes swapped (operand of the data gradient), all layers in one launch.
        first: refresh layers `first` on only (the optimiser step with a frozen prefix: the copies of the frozen layers are
        current, and a table of fewer rows is the whole difference); 0: every layer, as set_weights needs."""
        if first:
            return self._refresh_transposed_from(first)
        if self._tr_table is None:
            rows, start = [], 0
            for sp in self.specs[1:]:          # the first layer has no data gradient
                rows.append([sp.w_off, sp.k * sp.k, sp.cin_pad, sp.cout, start])
                start += sp.k * sp.k * (-(-sp.cin_pad // 32)) * (-(-sp.cout // 32))
            self._tr_table = torch.tensor(rows, dtype=torch.int32, device=self.device)
            self._tr_tiles = start
        if self.planes is not None and os.environ.get('Y3_PREP_FUSED', '1') != '0':
            # one pass over the arena: transposed copy + the piece planes of both copies (bit-identical to the three launches below)
            check(lib.y3_x3_prepare_weights_batched(self.params.data_ptr(), self.params_t.data_ptr(), self.planes.data_ptr(), self.planes_t.data_ptr(),
                                                    self._tr_table.data_ptr(), len(self.specs) - 1, self._tr_tiles, self._stream()), 'y3_x3_prepare_weights_batched')
            self._bf16_stale = True
            return
        check(lib.y3_transpose_weights_batched(self.params.data_ptr(), self.params_t.data_ptr(), self._tr_table.data_ptr(), len(self.specs) - 1,
                                               self._tr_tiles, self._stream()), 'y3_transpose_weights_batched')
        if self.planes is not None:
            if self._x3_table is None:
                # the layers whose channel counts the x3 kernels take (K per row a multiple of 16), per copy: {offset, taps, rows, K per row, first block}
                tabs = []
                for fwd_copy in (False, True):
                    rows, start = [], 0
                    for sp in self.specs[1:]:
                        nrows, kpr = (sp.cout, sp.cin_pad) if fwd_copy else (sp.cin_pad, sp.cout)      # params_t: [tap][Cout][Cin]; params: [tap][Cin][Cout]
                        if kpr % 16:
                            continue
                        rows.append([sp.w_off, sp.k * sp.k, nrows, kpr, start])
                        start += -(-(sp.k * sp.k * nrows * kpr) // 1024)
                    tabs.append((torch.tensor(rows, dtype=torch.int32, device=self.device), len(rows), start))
                self._x3_table = tabs
            for (arena, planes), (tab, nl, blocks) in zip(((self.params, self.planes), (self.params_t, self.planes_t)), self._x3_table):
                check(lib.y3_x3_split_weights_batched(arena.data_ptr(), planes.data_ptr(), tab.data_ptr(), nl, blocks, self._stream()), 'y3_x3_split_weights_batched')
        self._bf16_stale = True

    def _refresh_transposed_from(self, first, launch=True):
        """_refresh_transposed for layers `first` >= 1 on: the same launches over tables that start at that layer.  The tables
        are device tensors: the constructor makes them (launch=False), never a captured step."""
        if self._tr_suffix is None or self._tr_suffix[0] != first:
            specs = self.specs[first:]
            rows, start = [], 0
            for sp in specs:
                rows.append([sp.w_off, sp.k * sp.k, sp.cin_pad, sp.cout, start])
                start += sp.k * sp.k * (-(-sp.cin_pad // 32)) * (-(-sp.cout // 32))
            tabs = []
            for fwd_copy in (False, True):
                xrows, xstart = [], 0
                for sp in specs:
                    nrows, kpr = (sp.cout, sp.cin_pad) if fwd_copy else (sp.cin_pad, sp.cout)
                    if kpr % 16:
                        continue
                    xrows.append([sp.w_off, sp.k * sp.k, nrows, kpr, xstart])
                    xstart += -(-(sp.k * sp.k * nrows * kpr) // 1024)
                tabs.append((torch.tensor(xrows, dtype=torch.int32, device=self.device), len(xrows), xstart))
            self._tr_suffix = (first, torch.tensor(rows, dtype=torch.int32, device=self.device), len(rows), start, tabs)
        if not launch:
            return
        _, table, nl, tiles, tabs = self._tr_suffix
        self._bf16_stale = True
        if self.planes is not None and os.environ.get('Y3_PREP_FUSED', '1') != '0':
            check(lib.y3_x3_prepare_weights_batched(self.params.data_ptr(), self.params_t.data_ptr(), self.planes.data_ptr(), self.planes_t.data_ptr(),
                                                    table.data_ptr(), nl, tiles, self._stream()), 'y3_x3_prepare_weights_batched')
            return
        check(lib.y3_transpose_weights_batched(self.params.data_ptr(), self.params_t.data_ptr(), table.data_ptr(), nl, tiles, self._stream()),
              'y3_transpose_weights_batched')
        if self.planes is not None:
            for (arena, planes), (tab, xl, blocks) in zip(((self.params, self.planes), (self.params_t, self.planes_t)), tabs):
                check(lib.y3_x3_split_weights_batched(arena.data_ptr(), planes.data_ptr(), tab.data_ptr(), xl, blocks, self._stream()), 'y3_x3_split_weights_batched')

    def fold_table(self):
        """Device table for y3_bn_fold_inference_batched (one row per BatchNorm layer)."""
        if self._fold_table is None:
            rows = [[sp.g_off, sp.be_off, sp.mv_off, self.moving_stride + sp.mv_off, sp.ch_off, sp.ch_off + sp.cout, sp.cout]
                    for sp in self.specs if sp.bn]
            self.fold_layers = len(rows)
            self._fold_table = torch.tensor(rows, dtype=torch.int32, device=self.device)
        return self._fold_table

    def _refresh_bf16(self):
        """params_t_bf16 <- round-to-nearest-even of params_t (the [tap][Cout][Cin] operand of y3_conv2d_fwd_bf16)."""
        if self.params_t_bf16 is None:
            self.params_t_bf16 = torch.zeros(self.arena_floats, dtype=torch.bfloat16, device=self.device)
        if self._bf16_stale:
            check(lib.y3_f32_to_bf16(self.params_t.data_ptr(), self.params_t_bf16.data_ptr(), self.arena_floats, self._stream()), 'y3_f32_to_bf16')
            torch.cuda.current_stream(self.device).synchronize()     # rare (weights changed); other streams may read the copy next
            self._bf16_stale = False

    # ---- reference API (model.py:466-479) ---------------------------------------------
    def get_keras_model(self):
        return self.model

    def get_keras_feature_map_model(self):
        return self.model_feature_maps

    def get_optimizer(self):
        return self.optimizer

    def set_learning_rate(self, learning_rate):
        self.learning_rate = float(learning_rate)

    def get_learning_rate(self):
        return self.learning_rate

    def _lr(self, t):
        """lr(t) of optimiser step t = 1, 2, ...: the base rate times the schedule's factor (fp64)."""
        return self.learning_rate * float(self.lr_schedule.factor(t)) if self.lr_schedule is not None else self.learning_rate

    def current_learning_rate(self):
        """The rate the last optimiser step ran with, lr(iterations); the base rate before the first step."""
        return self._lr(self.iterations) if self.iterations >= 1 else self.learning_rate

    # ---- execution -------------------------------------------------------------------------
    def _plan(self, n, training, bf16=False, slot=0, size=None):
        bf16 = bool(bf16) and not training
        size = (int(size[0]), int(size[1])) if size is not None else self.train_sizes[0]      # (the constructed size)
        key = (int(n), bool(training), bf16, int(slot), size)
        if bf16:
            self._refresh_bf16()
        if key not in self._plans:
            self._plans[key] = _Plan(self, int(n), bool(training), bf16, size)
        return self._plans[key]

    def _input_size(self, images, sizes=None):
        """(H, W) of an NCHW batch, which must be one of `sizes`: train_sizes for train_step / test_step, by default the constructed
        size alone.  Checked before a plan is looked up, so a refused batch leaves none behind."""
        sizes = self.train_sizes[:1] if sizes is None else sizes
        shape = tuple(images.shape)
        if len(shape) == 4 and shape[1] == self.img_size[2] and (int(shape[2]), int(shape[3])) in sizes:
            return (int(shape[2]), int(shape[3]))
        raise ValueError('input shape %s does not match the model input (C,H,W)=%s (Q18: fixed at construction)%s'
                         % (shape, (self.img_size[2], self.img_size[0], self.img_size[1]),
                            '' if len(sizes) == 1 else ' or another of its train_sizes %s' % (sizes,)))

    def _load_inputs(self, plan, images, gt_data=None):
        plan.in_nchw.copy_(torch.as_tensor(images).to(torch.float32), non_blocking=True)
        if gt_data is not None:
            for dst, src in zip(plan.gt, gt_data):
                dst.copy_(torch.as_tensor(src).to(torch.float32).reshape(dst.shape), non_blocking=True)

    def _graph_of(self, body, warm=None):
        """body(stream) as a HIP graph (the launch lists are static and read no host state).  A warm-up call -- `warm`, by default
        body itself -- runs first, so that lazy initialisation happens outside the capture."""
        (warm or body)(self._stream())
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode='thread_local'):      # the prefetch thread may allocate pinned memory meanwhile
            body(self._stream())
        return g

    def predict(self, images, precision=None, slot=0):
        """The saved 'yolov3' model (model.py:463): NCHW in -> [N, Nb, 5+K].  precision 'bf16' runs every conv after
        the RGB layer on the bf16 MFMA path (fp32 accumulate, fp32 heads / decode); default self.inference_precision.
        Calls with different ``slot`` use separate activation / output buffers and may run concurrently on different
        streams (inference_tiled does that); calls with the same slot must be stream-ordered."""
        self._input_size(images)
        plan = self._plan(int(images.shape[0]), False, (precision or self.inference_precision) == 'bf16', slot)
        self._load_inputs(plan, images)
        if self.use_graph:
            if plan.infer_graph is None:
                plan.infer_graph = self._graph_of(plan.run_inference)
            plan.infer_graph.replay()
        else:
            plan.run_inference(self._stream())
        return plan.boxes

    def predict_tiles(self, img_dev, dtype_code, img_shape, table_ptr, count, tile_size=None, precision=None, slot=0):
        """One batch of inference_tiled: tiles `table_ptr[0:count]` (device rows of tile_table) of the device-resident HWC image
        -> z-scored NHWC network input in two passes over the image (y3_tile_gather_zscore_nhwc; the same bits as
        tiles_to_device -> zscore_normalize_device -> the input transpose), then forward + decode.  Returns [count, Nb, 5+K]."""
        h, w, c = (int(v) for v in img_shape)
        if c != self.img_size[2] or (tile_size is not None and [int(tile_size[0]), int(tile_size[1])] != self.img_size[:2]):
            raise ValueError('tiles %s x %d channels do not match the model input (H,W,C)=%s (Q18: fixed at construction)' % (tile_size, c, self.img_size))
        count = int(count)
        plan = self._plan(count, False, (precision or self.inference_precision) == 'bf16', slot)
        st = self._stream()
        if plan.zs_ws is None:
            plan.zs_ws = torch.empty(int(lib.y3_zscore_workspace_bytes(count)) // 8 + 1, dtype=torch.float64, device=self.device)
        check(lib.y3_tile_gather_zscore_nhwc(img_dev.data_ptr(), int(dtype_code), h, w, c, table_ptr, count, self.img_size[0], self.img_size[1],
                                             plan.x0.buf.data_ptr(), plan.x0.ld, plan.zs_ws.data_ptr(), st), 'y3_tile_gather_zscore_nhwc')
        if self.use_graph:
            if plan.infer_graph_tiles is None:      # forward without the input transpose: the gather above wrote x0
                plan.infer_graph_tiles = self._graph_of(functools.partial(plan.run_inference, skip_input=True))
            plan.infer_graph_tiles.replay()
        else:
            plan.run_inference(st, skip_input=True)
        return plan.boxes

    def predict_tiles_tta(self, img_dev, dtype_code, img_shape, table_ptr, count, views, tile_size=None, precision=None, slot=0):
        """predict_tiles under test-time augmentation: the views (distinct 3-bit codes, bbox_utils.TTA_VIEWS) of tiles
        `table_ptr[0:count]` are gathered, z-scored per tile and written straight into the NHWC input of a plan of count * k network
        inputs, tile-major and view-minor (y3_tile_gather_zscore_views_nhwc; the same bits as tiles_to_device ->
        zscore_normalize_device -> predict_tta's views), go through the network as one batch, and every view's decode rows are mapped
        back to the tile's frame in place (y3_tta_unmap).  Returns [count, k * Nb, 5+K]: view v of a tile in rows v * Nb ..
        (v + 1) * Nb - 1, as predict_tta returns them for images."""
        h, w, c = (int(v) for v in img_shape)
        if c != self.img_size[2] or (tile_size is not None and [int(tile_size[0]), int(tile_size[1])] != self.img_size[:2]):
            raise ValueError('tiles %s x %d channels do not match the model input (H,W,C)=%s (Q18: fixed at construction)' % (tile_size, c, self.img_size))
        views = [int(v) for v in views]
        count, k = int(count), len(views)
        if count < 1 or k < 1:
            raise ValueError('predict_tiles_tta: {} tiles x {} views (at least one of each)'.format(count, k))
        plan = self._plan(count * k, False, (precision or self.inference_precision) == 'bf16', slot)
        st = self._stream()
        if plan.zs_ws is None:      # sized for the plan's count * k inputs, so predict_tiles can share it
            plan.zs_ws = torch.empty(int(lib.y3_zscore_workspace_bytes(count * k)) // 8 + 1, dtype=torch.float64, device=self.device)
        codes = int_array(views)
        th, tw = self.img_size[0], self.img_size[1]
        check(lib.y3_tile_gather_zscore_views_nhwc(img_dev.data_ptr(), int(dtype_code), h, w, c, table_ptr, count, th, tw, codes, k,
                                                   plan.x0.buf.data_ptr(), plan.x0.ld, plan.zs_ws.data_ptr(), st), 'y3_tile_gather_zscore_views_nhwc')
        if self.use_graph:
            if plan.infer_graph_tiles is None:      # forward without the input transpose: the gather above wrote x0
                plan.infer_graph_tiles = self._graph_of(functools.partial(plan.run_inference, skip_input=True))
            plan.infer_graph_tiles.replay()
        else:
            plan.run_inference(st, skip_input=True)
        check(lib.y3_tta_unmap(plan.boxes.data_ptr(), count * k, plan.nb, plan.boxes.shape[2], codes, k, th, tw, st), 'y3_tta_unmap')
        return plan.boxes.view(count, k * plan.nb, plan.boxes.shape[2])

    TTA_MAX_BATCH = 16     # images x views per network call: the conv routes are tested for batches 1..16

    def predict_tta(self, images, views, precision=None, slot=0):
        """Test-time augmentation: images CUDA float32 [N, C, H, W], z-scored already; views: distinct 3-bit
        codes (bbox_utils.TTA_VIEWS).  The N * k views are written straight into the plan's NHWC input (y3_tta_views_nhwc,
        image-major and view-minor), go through the network as one batch of N * k, and every view's decode rows are mapped
        back to the image's frame in place (y3_tta_unmap).  Returns [N, k * Nb, 5+K]: view v of an image in rows v * Nb ..
        (v + 1) * Nb - 1.  N * k <= TTA_MAX_BATCH."""
        if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.float32):
            raise ValueError('predict_tta: images must be a CUDA float32 tensor')
        h, w = self._input_size(images)
        views = [int(v) for v in views]
        n, k = int(images.shape[0]), len(views)
        if k < 1 or n * k > self.TTA_MAX_BATCH:
            raise ValueError('predict_tta: {} images x {} views = {} network inputs (1 .. {} per call)'.format(n, k, n * k, self.TTA_MAX_BATCH))
        images = images.contiguous()
        plan = self._plan(n * k, False, (precision or self.inference_precision) == 'bf16', slot)
        st = self._stream()
        codes = int_array(views)
        check(lib.y3_tta_views_nhwc(images.data_ptr(), n, int(images.shape[1]), h, w, codes, k, plan.x0.v, st), 'y3_tta_views_nhwc')
        if self.use_graph:
            if plan.infer_graph_tiles is None:      # forward without the input transpose: the launch above wrote x0
                plan.infer_graph_tiles = self._graph_of(functools.partial(plan.run_inference, skip_input=True))
            plan.infer_graph_tiles.replay()
        else:
            plan.run_inference(st, skip_input=True)
        check(lib.y3_tta_unmap(plan.boxes.data_ptr(), n * k, plan.nb, plan.boxes.shape[2], codes, k, h, w, st), 'y3_tta_unmap')
        return plan.boxes.view(n, k * plan.nb, plan.boxes.shape[2])

    LETTERBOX_MAX_BATCH = letterbox.MAX_IMAGES     # images per call: Y3_LETTERBOX_MAX_IMAGES, and the batches the conv routes are tested for

    def _letterbox_upload(self, images, slot):
        """HWC NumPy images of any sizes, one dtype, the model's channel count -> (device byte buffer, dtype code, records): the images
        packed at 16-byte aligned offsets into pinned staging and copied in one transfer; both buffers grow and are kept per slot."""
        images = [np.ascontiguousarray(im[:, :, None] if im.ndim == 2 else im) for im in images]
        if not 1 <= len(images) <= self.LETTERBOX_MAX_BATCH:
            raise ValueError('predict_letterbox: {} images (1 .. {} per call)'.format(len(images), self.LETTERBOX_MAX_BATCH))
        dt = images[0].dtype
        if dt not in letterbox.DTYPE_CODES or any(im.dtype != dt for im in images):
            raise ValueError('predict_letterbox: images must share one dtype of uint8, uint16, float32 (got {})'.format({str(im.dtype) for im in images}))
        if any(im.ndim != 3 or im.shape[2] != self.img_size[2] for im in images):
            raise ValueError('predict_letterbox: images must be HWC with the model\'s {} channels (got {})'.format(
                self.img_size[2], [tuple(im.shape) for im in images]))
        records, total = letterbox.pack_layout([im.shape for im in images], dt.itemsize, self.img_size[0], self.img_size[1])
        st = self._lb_staging.setdefault(int(slot), {'dev': None, 'pin': None, 'done': None})
        if st['done'] is not None:
            st['done'].synchronize()          # the copy of the call before this one has left the pinned staging
        if st['pin'] is None or st['pin'].numel() < total:
            cap = max(total, 2 * (st['pin'].numel() if st['pin'] is not None else 0))
            st['pin'] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            st['dev'] = torch.empty(cap, dtype=torch.uint8, device=self.device)
        host = st['pin'].numpy()
        for im, rec in zip(images, records):
            off = int(rec['src_offset'])
            host[off:off + im.nbytes] = im.reshape(-1).view(np.uint8)
        st['dev'][:total].copy_(st['pin'][:total], non_blocking=True)
        st['done'] = torch.cuda.Event()
        st['done'].record(torch.cuda.current_stream(self.device))
        return st['dev'], letterbox.DTYPE_CODES[dt], records

    def predict_letterbox(self, images, precision=None, slot=0):
        """Letterbox inference: images: 1 .. 16 HWC NumPy arrays of ANY sizes, one dtype (uint8 / uint16 / float32) and
        the model's channel count.  They are packed into one device byte buffer, resampled (antialiased, aspect ratio kept), padded
        and z-scored on their own content straight into the plan's NHWC input (y3_letterbox_zscore_nhwc), go through the network as
        one batch, and the decode rows are mapped back to each image's own pixels and clipped to it, in place
        (y3_letterbox_unmap).  Returns (rows [n, Nb, 5+K], records): letterbox.LETTERBOX_RECORD of every image."""
        src, code, records = self._letterbox_upload(images, slot)
        n, c = len(records), self.img_size[2]
        plan = self._plan(n, False, (precision or self.inference_precision) == 'bf16', slot)
        st = self._stream()
        if plan.lb_ws is None:
            plan.lb_ws = torch.empty(int(lib.y3_letterbox_workspace_bytes(n, self.img_size[0], self.img_size[1], c)) // 8 + 2, dtype=torch.float64,
                                     device=self.device)
        check(lib.y3_letterbox_zscore_nhwc(src.data_ptr(), code, c, n, records.ctypes.data, plan.x0.v, plan.lb_ws.data_ptr(), st),
              'y3_letterbox_zscore_nhwc')
        if self.use_graph:
            if plan.infer_graph_tiles is None:      # forward without the input transpose: the launches above wrote x0
                plan.infer_graph_tiles = self._graph_of(functools.partial(plan.run_inference, skip_input=True))
            plan.infer_graph_tiles.replay()
        else:
            plan.run_inference(st, skip_input=True)
        check(lib.y3_letterbox_unmap(plan.boxes.data_ptr(), n, plan.nb, plan.boxes.shape[2], records.ctypes.data, 1, st), 'y3_letterbox_unmap')
        return plan.boxes, records

    def feature_maps(self, images, training=False, precision=None):
        """The 'yolov3_fm' model (model.py:462): three NCHW feature maps (fp32 unless precision='bf16' is asked for)."""
        self._input_size(images)
        plan = self._plan(int(images.shape[0]), training, precision == 'bf16')
        self._load_inputs(plan, images)
        st = self._stream()
        plan.run_forward(st)
        return self._export_fms(plan, st)

    def _export_fms(self, plan, st):
        out = []
        for f in plan.fms:
            t = torch.empty(f.n, f.c, f.h, f.w, dtype=torch.float32, device=self.device)
            check(lib.y3_nhwc_to_nchw(f.v, t.data_ptr(), st), 'y3_nhwc_to_nchw')
            out.append(t)
        return out

    def _lr_t(self):
        t = self.iterations
        return self._lr(t) * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)

    def _fill_hyper(self):
        """The device scalars of optimiser step `iterations`, computed in fp64 and rounded once to fp32: lr_t for 'adam' and
        'adamw', lr for 'sgd'; 'adamw' also lr * weight_decay."""
        if self.optimizer_kind == 'sgd':
            self.lr_t_dev.fill_(float(np.float32(self._lr(self.iterations))))
            return
        self.lr_t_dev.fill_(self._lr_t())
        if self.optimizer_kind == 'adamw':
            self.hyper_dev[1:2].fill_(float(np.float32(self._lr(self.iterations) * self.weight_decay)))

    def _fwd_bwd(self, plan, st):
        plan.run_forward(st)
        plan.run_loss(st)
        if self.dist is not None:
            self.dist.begin_step()
        plan.run_backward(st, self.dist)

    def _grad_passes(self, st, last):
        """After the backward pass of a micro-step (kernel gradients joined into `st` by run_backward, all-reduce by finish_step):
        fold grads into the accumulator, and on the last micro-step leave the norm and the Adam scale in device memory."""
        n = self.train_floats                 # the trainable suffix of the arenas: all of them with no layer frozen
        if self.grad_acc is not None:
            check(lib.y3_grad_accumulate(self._tp(self.grad_acc), self._tp(self.grads), n, self._acc_first_dev.data_ptr(),
                                         self._grad_ws.data_ptr(), st), 'y3_grad_accumulate')
        elif last:
            check(lib.y3_grad_sumsq(self._tp(self.grads), n, self._grad_ws.data_ptr(), st), 'y3_grad_sumsq')
        if last:
            clip = self.grad_clip_norm if self.grad_clip_norm is not None else math.inf        # Y3_GRAD_CLIP_OFF
            check(lib.y3_grad_clip_scale(self._grad_ws.data_ptr(), n, self.accumulate_steps, clip, self.last_grad_norm.data_ptr(),
                                         self.grad_scale_dev.data_ptr(), st), 'y3_grad_clip_scale')

    def _tp(self, arena):
        """Device address of the trainable suffix of a parameter-shaped arena (its start with no layer frozen)."""
        return arena.data_ptr() + 4 * self.train_off

    def _adam_launch(self):
        """(entry point, arguments up to the stream) of the optimiser step: y3_adam_step* for the default 'adam', y3_optim_step for
        'adamw' / 'sgd' (the one place that chooses).  Every buffer it names is allocated by the constructor and only ever written
        in place, so the constructor calls this once; what changes per step (lr or lr_t, lr * weight decay, the EMA factor, the
        gradient scale) is read from device memory.  With frozen layers every arena is passed from the trainable suffix on
        (trainable_suffix: a pointer and a count), the decay ranges relative to it: frozen parameters, their moments and their EMA
        copies are never read or written."""
        g = self.grad_acc if self.grad_acc is not None else self.grads
        tp = self._tp
        if self.optimizer_kind != 'adam':
            # SGD with momentum / AdamW, decay on the kernels only: one descriptor, built once like the tuple below.
            # The range table is host memory the descriptor points into; both live as long as the model.
            ranges = self.decay_ranges = suffix_decay_ranges(self.specs, self.freeze_layers)
            self._decay_table = (ctypes.c_longlong * (2 * len(ranges)))(*[v for r in ranges for v in r])
            d = self._optim_desc = _hip.OptimDesc()
            d.kind = _hip.OPT_ADAMW if self.optimizer_kind == 'adamw' else _hip.OPT_SGD_NESTEROV if self.nesterov else _hip.OPT_SGD
            d.param, d.grad, d.m, d.count = tp(self.params), tp(g), tp(self.adam_m), self.train_floats
            d.v = tp(self.adam_v) if self.adam_v is not None else None
            d.hyper_dev = self.hyper_dev.data_ptr()
            d.momentum, d.weight_decay = self.momentum, self.weight_decay
            d.beta1, d.beta2, d.eps = self.beta1, self.beta2, self.adam_eps
            d.decay_ranges_host, d.n_ranges = self._decay_table, len(ranges)
            if self.ema_decay is not None:
                d.ema_param, d.moving, d.ema_moving = tp(self.ema_params), self.moving.data_ptr(), self.ema_moving.data_ptr()
                d.moving_count, d.omd_dev = self.moving.numel(), self.ema_omd_dev.data_ptr()
            if self._grad_ws is not None:
                d.scale_dev = self.grad_scale_dev.data_ptr()
            return lib.y3_optim_step, (ctypes.byref(d),)
        name = 'y3_adam_step'
        args = [tp(self.params), tp(g), tp(self.adam_m), tp(self.adam_v), self.train_floats,
                self.lr_t_dev.data_ptr(), self.beta1, self.beta2, self.adam_eps]
        if self.ema_decay is not None:
            # the same Adam step + the weight / moving-statistics average in the same pass
            name += '_ema'
            args += [tp(self.ema_params), self.moving.data_ptr(), self.ema_moving.data_ptr(), self.moving.numel(), self.ema_omd_dev.data_ptr()]
        if self._grad_ws is not None:
            # accumulation / clipping on: the same update on (accumulated gradient) * scale
            name += '_scaled'
            args += [self.grad_scale_dev.data_ptr()]
        return getattr(lib, name), tuple(args)

    def _adam(self, st):
        fn, args = self._adam_call
        check(fn(*args, st), fn.__name__)
        self._refresh_transposed(self.freeze_layers)

    @property
    def last_ignored(self):
        """ignore_mask='truth': the number of predictions without an object that the last train_step / test_step left out of the
        objectness loss, summed over the three scales (0-d device tensor, read when used); None before the first step and with
        'reference'."""
        plan = self._loss_plan
        return plan.ignored[0] if plan is not None and plan.ignored is not None else None

    @property
    def last_truth_max(self):
        """ignore_mask='truth': the longest per-image ground-truth list of the last train_step / test_step, before the cut at
        max_truth_boxes (0-d device tensor, computed when asked for); None before the first step and with 'reference'."""
        plan = self._loss_plan
        return plan.truth_counts.max() if plan is not None and plan.truth_counts is not None else None

    def _loss_out(self, plan, metrics):
        """plan.loss4 of the step just enqueued -> the loss the step returns (0-d device tensor), fed with its four parts to the
        metrics (loss, xy, wh, obj, class; fewer or None = not wanted)."""
        self._loss_plan = plan
        parts = plan.loss4.clone()
        loss_value = parts.sum() / float(self.global_batch_size)
        for mtr, val in zip(metrics, [loss_value, parts[0], parts[1], parts[2], parts[3]]):
            if mtr is not None:
                mtr.update_state(val)
        return loss_value

    def train_step(self, inputs):
        """model.py:481-508 for this replica.  inputs = (images, (gt1, gt2, gt3),
        loss_metric, loss_xy_metric, loss_wh_metric, loss_obj_metric, loss_class_metric);
        metrics may be None.  Returns the loss value as a 0-d device tensor.
        With accumulate_steps = k > 1 this is one MICRO-step: forward, loss, backward (and all-reduce) as ever, grads folded into
        the accumulator; only the k-th call in a row advances `iterations` and updates weights, moments and EMA.
        With train_sizes the images may have any listed (H, W), the labels the matching grids: every size has its own plan (and
        captured graphs), the weights, moments, accumulator and BatchNorm statistics are the model's."""
        images, gt_data = inputs[0], inputs[1]
        if self._ema_swapped:
            raise RuntimeError('train_step inside ema_weights(): the live weights are parked')
        plan = self._plan(int(images.shape[0]), True, size=self._input_size(images, self.train_sizes))
        self._load_inputs(plan, images, gt_data)
        last = self.micro_step == self.accumulate_steps - 1          # always, without accumulation
        if last:
            self.iterations += 1
            self._bf16_stale = True
            self._fill_hyper()
            if self.ema_decay is not None:
                self.ema_omd_dev.fill_(float(self._ema_omd()))
        if self.grad_acc is not None:
            self._acc_first_dev.fill_(1 if self.micro_step == 0 else 0)
        st = self._stream()
        if self.use_graph and self.dist is None:
            which = 'graph' if last else 'graph_micro'
            if getattr(plan, which) is None:
                self._capture(plan, last)
            getattr(plan, which).replay()
        else:
            self._fwd_bwd(plan, st)
            if self.dist is not None:
                self.dist.finish_step()
            if self._grad_ws is not None:
                self._grad_passes(st, last)
            if last:
                self._adam(st)
        self.micro_step = 0 if last else self.micro_step + 1
        return self._loss_out(plan, inputs[2:])

    def _capture(self, plan, last=True):
        """Capture forward + loss + backward + Adam of one step into a HIP graph.
        A warm-up pass (no Adam) runs first so lazy initialisation happens
        outside the capture; it only touches scratch state plus the BN moving
        statistics, which are restored before capturing.
        With gradient accumulation there are two graphs per plan: last=False is a
        micro-step that only folds its gradients into the accumulator (`first`
        comes from device memory, so one graph serves micro-steps 1 .. k-1),
        last=True adds the norm, the scale and the scaled Adam step."""
        def fwd_bwd(st):      # (a captured step has no data parallelism: train_step)
            plan.run_forward(st)
            plan.run_loss(st)
            plan.run_backward(st)

        def warm(st):
            moving = self.moving.clone()
            fwd_bwd(st)
            self.moving.copy_(moving)

        def step(st):
            fwd_bwd(st)
            if self._grad_ws is not None:
                self._grad_passes(st, last)
            if last:
                self._adam(st)

        setattr(plan, 'graph' if last else 'graph_micro', self._graph_of(step, warm))

    def dist_train_step(self, dist_strategy, inputs):
        """model.py:510-515: per-replica step + SUM of the per-replica losses."""
        if dist_strategy is not None and self.dist is None:
            dist_strategy.attach(self)
        loss = self.train_step(inputs)
        return dist_strategy.reduce_sum(loss) if dist_strategy is not None else loss

    def test_step(self, inputs):
        """model.py:517-534: BN in inference mode, loss + metrics, no update."""
        images, gt_data = inputs[0], inputs[1]
        plan = self._plan(int(images.shape[0]), False, size=self._input_size(images, self.train_sizes))
        self._load_inputs(plan, images, gt_data)
        st = self._stream()
        plan.run_forward(st)
        plan.run_loss(st)
        return self._loss_out(plan, inputs[2:])

    def dist_test_step(self, dist_strategy, inputs):
        """model.py:536-540."""
        loss = self.test_step(inputs)
        return dist_strategy.reduce_sum(loss) if dist_strategy is not None else loss
