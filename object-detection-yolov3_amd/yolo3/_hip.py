"""ctypes binding of libyolo3hip.so (C ABI: include/yolo3hip.h).

There is no CPU fallback: importing this module without the built library, or
calling an entry point that fails, raises.  Build with
``make -C object-detection-yolov3_amd/csrc`` (or ``__graft_entry__.build()``).
"""
import ctypes as C
import os

# torch's HIP runtime first, always: torch ships its own libamdhip64 / libhsa-runtime64, and the library below links the system
# ROCm's.  Loaded in the other order (`python __graft_entry__.py smoke`: build() imports this module before anything imports
# torch) the library's first launch failed with "no ROCm-capable device is detected" while torch itself ran.
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('Y3_LIB') or os.path.join(_HERE, '_lib', 'libyolo3hip.so')     # Y3_LIB: A/B two builds (tools/)


class HipLibraryMissing(ImportError):
    pass


class HipError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise HipLibraryMissing(
        'libyolo3hip.so not found at %s: build it with `make -C object-detection-yolov3_amd/csrc` '
        '(hipcc --offload-arch=gfx950).  There is no CPU fallback.' % LIB_PATH)

lib = C.CDLL(LIB_PATH)


class Tensor(C.Structure):
    """y3_tensor: NHWC view with pixel pitch ld (floats)."""
    _fields_ = [('ptr', C.c_void_p), ('n', C.c_int), ('h', C.c_int), ('w', C.c_int), ('c', C.c_int), ('ld', C.c_int)]


class OptimDesc(C.Structure):
    """y3_optim_desc: one SGD-momentum / AdamW step over a flat arena (y3_optim_step).  decay_ranges_host is a HOST array of
    n_ranges [begin, end) pairs; the holder keeps it alive."""
    _fields_ = [('kind', C.c_int), ('param', C.c_void_p), ('grad', C.c_void_p), ('m', C.c_void_p), ('v', C.c_void_p), ('count', C.c_size_t),
                ('hyper_dev', C.c_void_p), ('momentum', C.c_float), ('weight_decay', C.c_float), ('beta1', C.c_float), ('beta2', C.c_float),
                ('eps', C.c_float), ('decay_ranges_host', C.POINTER(C.c_longlong)), ('n_ranges', C.c_int), ('ema_param', C.c_void_p),
                ('moving', C.c_void_p), ('ema_moving', C.c_void_p), ('moving_count', C.c_size_t), ('omd_dev', C.c_void_p),
                ('scale_dev', C.c_void_p)]


TP = C.POINTER(Tensor)
vp, fp, ip = C.c_void_p, C.c_void_p, C.c_void_p     # device pointers travel as integers
i32, u32, f32, sz = C.c_int, C.c_uint, C.c_float, C.c_size_t

# name -> (restype, argtypes); every symbol declared in include/yolo3hip.h
SIGNATURES = {
    'y3_last_error': (C.c_char_p, []),
    'y3_debug_div': (i32, [i32, i32]),
    'y3_version': (i32, []),
    'y3_conv2d_fwd': (i32, [TP, fp, fp, i32, i32, TP, u32, f32, fp, fp, TP, fp, vp, sz, vp]),
    'y3_conv2d_stats_tiles': (i32, [i32, i32, i32, i32]),
    'y3_conv2d_fwd_workspace': (sz, [i32, i32, i32, i32]),
    'y3_conv2d_dgrad': (i32, [TP, fp, i32, i32, TP, u32, vp, sz, vp]),
    'y3_conv2d_stats_tiles_x': (i32, [i32, i32, i32, i32, u32]),
    'y3_conv2d_fwd_workspace_x': (sz, [i32, i32, i32, i32, u32]),
    'y3_conv2d_x3_ok': (i32, [i32, i32, i32, i32]),
    'y3_conv2d_dgrad_x3_ok': (i32, [TP, i32, i32, TP]),
    'y3_x3_split_weights': (i32, [fp, vp, i32, i32, i32, vp]),
    'y3_x3_split_weights_batched': (i32, [fp, vp, ip, i32, i32, vp]),
    'y3_x3_prepare_weights_batched': (i32, [fp, fp, vp, vp, ip, i32, i32, vp]),
    'y3_conv2d_dgrad_workspace_x': (sz, [TP, i32, i32, TP, u32]),
    'y3_conv2d_dgrad_bn_tiles_x': (i32, [TP, i32, i32, TP, u32]),
    'y3_conv2d_dgrad_workspace': (sz, [TP, i32, i32, TP]),
    'y3_conv2d_dgrad_bn': (i32, [TP, fp, i32, i32, TP, u32, TP, fp, vp, sz, vp]),
    'y3_conv2d_dgrad_bn_tiles': (i32, [TP, i32, i32, TP]),
    'y3_conv2d_wgrad': (i32, [TP, TP, i32, i32, fp, vp, sz, vp]),
    'y3_conv2d_wgrad_workspace': (sz, [TP, TP, i32, i32]),
    'y3_conv2d_wgrad_x': (i32, [TP, TP, i32, i32, fp, u32, vp, sz, vp]),
    'y3_conv2d_wgrad_workspace_x': (sz, [TP, TP, i32, i32, u32]),
    'y3_conv2d_wgrad_x3_ok': (i32, [i32, i32, i32, i32]),
    'y3_transpose_weights': (i32, [fp, fp, i32, i32, i32, vp]),
    'y3_transpose_weights_batched': (i32, [fp, fp, ip, i32, i32, vp]),
    'y3_bn_stats_finalize': (i32, [fp, i32, i32, i32, fp, fp, f32, f32, fp, fp, fp, fp, fp, fp, vp]),
    'y3_bn_fold_inference': (i32, [fp, fp, fp, fp, f32, i32, fp, fp, vp]),
    'y3_bn_fold_inference_batched': (i32, [fp, fp, fp, ip, i32, f32, vp]),
    'y3_bn_apply': (i32, [TP, fp, fp, TP, TP, vp]),
    'y3_bn_bwd_stats': (i32, [TP, TP, TP, i32, fp, fp, fp, f32, fp, fp, fp, fp, vp, sz, vp]),
    'y3_bn_bwd_workspace': (sz, [i32, i32]),
    'y3_bn_bwd_apply': (i32, [TP, TP, fp, f32, TP, vp]),
    'y3_bn_bwd_apply_fanin': (i32, [TP, TP, fp, f32, TP, TP, i32, vp]),
    'y3_bn_bwd_finalize_tiles': (i32, [fp, i32, i32, i32, fp, fp, fp, f32, fp, fp, fp, fp, vp]),
    'y3_bn_frozen_bwd': (i32, [TP, TP, TP, i32, fp, fp, fp, f32, f32, TP, fp, fp, fp, vp, sz, vp]),
    'y3_bn_frozen_bwd_workspace': (sz, [i32, i32]),
    'y3_upsample_sum2x_fwd': (i32, [TP, TP, vp]),
    'y3_upsample_sum2x_bwd': (i32, [TP, TP, vp]),
    'y3_spp_fwd': (i32, [TP, TP, vp]),
    'y3_spp_fwd_bf16': (i32, [TP, TP, vp]),
    'y3_spp_bwd': (i32, [TP, TP, TP, i32, vp]),
    'y3_copy': (i32, [TP, TP, vp]),
    'y3_conv2d_fwd_bf16': (i32, [TP, vp, fp, i32, i32, TP, i32, u32, f32, fp, fp, TP, vp]),
    'y3_conv2d_fwd_bf16_ws': (i32, [TP, vp, fp, i32, i32, TP, i32, u32, f32, fp, fp, TP, vp, sz, vp]),
    'y3_conv2d_fwd_bf16_workspace': (sz, [i32, i32, i32, i32]),
    'y3_conv2d_fwd_bf16_plan': (sz, [TP, vp, fp, i32, i32, TP, i32, u32, f32, fp, fp, TP, vp, sz, ip]),
    'y3_f32_to_bf16': (i32, [fp, vp, sz, vp]),
    'y3_conv2d_first_bf16': (i32, [TP, fp, fp, TP, u32, f32, fp, fp, vp]),
    'y3_tile_gather': (i32, [vp, i32, i32, i32, i32, ip, i32, i32, i32, fp, vp]),
    'y3_tile_gather_zscore_nhwc': (i32, [vp, i32, i32, i32, i32, ip, i32, i32, i32, fp, i32, vp, vp]),
    'y3_tile_gather_zscore_views_nhwc': (i32, [vp, i32, i32, i32, i32, ip, i32, i32, i32, C.POINTER(C.c_int), i32, fp, i32, vp, vp]),     # views: HOST array
    'y3_upsample_sum2x_fwd_bf16': (i32, [TP, TP, vp]),
    'y3_add_inplace': (i32, [TP, TP, vp]),
    'y3_fill': (i32, [fp, sz, f32, vp]),
    'y3_nchw_to_nhwc': (i32, [fp, i32, i32, i32, i32, TP, vp]),
    'y3_nhwc_to_nchw': (i32, [TP, fp, vp]),
    'y3_colsum': (i32, [TP, fp, vp]),
    'y3_decode_fwd': (i32, [TP, i32, C.POINTER(C.c_float), i32, i32, i32, i32, fp, vp]),
    'y3_loss_fwd_bwd': (i32, [TP, fp, C.POINTER(C.c_float), i32, i32, i32, i32, f32, fp, TP, vp, vp]),
    'y3_loss_fwd_bwd_ex': (i32, [TP, fp, C.POINTER(C.c_float), i32, i32, i32, i32, f32, i32, f32, fp, TP, vp, vp]),
    'y3_loss_workspace_bytes': (sz, []),
    'y3_truth_boxes': (i32, [fp, i32, C.c_longlong, i32, fp, ip, i32, vp]),
    'y3_loss_truth_workspace_bytes': (sz, [i32]),
    'y3_loss_fwd_bwd_truth': (i32, [TP, fp, C.POINTER(C.c_float), i32, i32, i32, i32, f32, i32, f32, fp, ip, i32, f32, fp, fp, TP, vp, vp]),
    'y3_loss_fwd_bwd_focal': (i32, [TP, fp, C.POINTER(C.c_float), i32, i32, i32, i32, f32, i32, f32, fp, ip, i32, f32, fp, fp, TP, vp, f32, f32, f32,
                                    f32, f32, vp]),
    'y3_adam_step': (i32, [fp, fp, fp, fp, sz, fp, f32, f32, f32, vp]),
    'y3_adam_step_ema': (i32, [fp, fp, fp, fp, sz, fp, f32, f32, f32, fp, fp, fp, sz, fp, vp]),
    'y3_grad_norm_workspace_bytes': (sz, [sz]),
    'y3_grad_accumulate': (i32, [fp, fp, sz, ip, vp, vp]),
    'y3_grad_sumsq': (i32, [fp, sz, vp, vp]),
    'y3_grad_clip_scale': (i32, [vp, sz, i32, C.c_double, fp, fp, vp]),
    'y3_adam_step_scaled': (i32, [fp, fp, fp, fp, sz, fp, f32, f32, f32, fp, vp]),
    'y3_adam_step_ema_scaled': (i32, [fp, fp, fp, fp, sz, fp, f32, f32, f32, fp, fp, fp, sz, fp, fp, vp]),
    'y3_optim_step': (i32, [C.POINTER(OptimDesc), vp]),
    'y3_nms_per_class': (i32, [fp, i32, i32, i32, f32, f32, f32, f32, f32, ip, ip, fp, i32, vp, sz, vp]),
    'y3_nms_workspace_bytes': (sz, [i32, i32, i32]),
    'y3_nms_single_class': (i32, [fp, i32, f32, ip, ip, fp, vp, sz, vp]),
    'y3_nms_per_class_ex': (i32, [fp, i32, i32, i32, i32, f32, f32, f32, f32, f32, f32, ip, ip, fp, i32, vp, sz, vp]),
    'y3_nms_workspace_bytes_ex': (sz, [i32, i32, i32, i32]),
    'y3_nms_labelled': (i32, [fp, i32, i32, i32, f32, f32, f32, ip, ip, fp, i32, vp, sz, vp]),
    'y3_tile_merge': (i32, [fp, i32, i32, i32, i32, ip, ip, fp, i32, ip, i32, i32, i32, i32, i32, f32, fp, i32, ip, vp, sz, vp]),
    'y3_tile_merge_workspace_bytes': (sz, [i32, i32]),
    'y3_tile_merge_voted': (i32, [fp, i32, i32, i32, ip, ip, i32, ip, i32, i32, i32, i32, i32, f32, fp, i32, ip, vp, sz, vp]),
    'y3_tta_views_nhwc': (i32, [fp, i32, i32, i32, i32, C.POINTER(C.c_int), i32, TP, vp]),     # views: HOST array
    'y3_tta_unmap': (i32, [fp, i32, i32, i32, C.POINTER(C.c_int), i32, i32, i32, vp]),
    'y3_box_vote': (i32, [fp, i32, i32, i32, ip, ip, fp, i32, f32, f32, f32, f32, f32, i32, i32, i32, fp, vp, sz, vp]),
    'y3_box_vote_workspace_bytes': (sz, [i32, i32, i32]),
    'y3_filter_small_boxes': (i32, [fp, i32, i32, f32, ip, ip, vp]),
    'y3_compute_iou': (i32, [fp, fp, i32, i32, fp, vp]),
    'y3_comm_unique_id': (i32, [vp]),
    'y3_comm_init': (i32, [vp, i32, i32, C.POINTER(C.c_void_p)]),
    'y3_allreduce_sum_f32': (i32, [vp, fp, sz, vp]),
    'y3_conv2d_plan': (sz, [i32, i32, i32, i32, C.POINTER(C.c_int)]),
    'y3_conv2d_wgrad_plan': (sz, [i32, i32, i32, i32, C.POINTER(C.c_int)]),
    'y3_conv2d_plan_x': (sz, [i32, i32, i32, i32, u32, C.POINTER(C.c_int)]),
    'y3_conv2d_wgrad_plan_x': (sz, [i32, i32, i32, i32, u32, C.POINTER(C.c_int)]),
    'y3_conv2d_dgrad_plan_x': (sz, [TP, i32, i32, TP, u32, C.POINTER(C.c_int)]),
    'y3_comm_info': (i32, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'y3_comm_destroy': (i32, [vp]),
    'y3_zscore': (i32, [fp, fp, i32, sz, vp, vp]),
    'y3_zscore_workspace_bytes': (sz, [i32]),
    'y3_augment_batch': (i32, [vp, i32, i32, i32, i32, i32, vp, i32, i32, fp, vp, vp]),     # records: HOST pointer (augment.AUG_RECORD)
    'y3_augment_workspace_bytes': (sz, [i32, i32, i32, i32]),
    'y3_mosaic_batch': (i32, [fp, i32, i32, i32, i32, vp, fp, vp]),     # records: HOST pointer (augment.MOSAIC_RECORD)
    'y3_affine_batch': (i32, [fp, i32, i32, i32, i32, vp, fp, vp]),     # records: HOST pointer (augment.AFFINE_RECORD)
    'y3_letterbox_batch': (i32, [vp, i32, i32, i32, vp, i32, i32, f32, fp, vp]),     # records: HOST pointer (letterbox.LETTERBOX_RECORD)
    'y3_letterbox_zscore_nhwc': (i32, [vp, i32, i32, i32, vp, TP, vp, vp]),
    'y3_letterbox_workspace_bytes': (sz, [i32, i32, i32, i32]),
    'y3_letterbox_unmap': (i32, [fp, i32, i32, i32, vp, i32, vp]),
    'y3_photometric_batch': (i32, [fp, i32, i32, i32, i32, vp, fp, vp]),     # records: HOST pointer (augment.PHOTO_RECORD)
    'y3_format_labels': (i32, [ip, ip, i32, i32, C.POINTER(C.c_float), i32, i32, i32, i32, fp, fp, fp, vp]),
    'y3_format_labels_scales': (i32, [ip, ip, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_int), i32, i32, i32, i32, fp, fp, fp, vp]),   # table: HOST
    'y3_decode_fwd_scales': (i32, [TP, C.POINTER(C.c_float), C.POINTER(C.c_int), i32, i32, i32, i32, fp, vp]),
    'y3_truth_boxes_scales': (i32, [fp, fp, fp, i32, C.c_longlong, C.c_longlong, C.c_longlong, i32, fp, ip, i32, vp]),
    'y3_anchor_stats_workspace_bytes': (sz, [i32, i32]),
    'y3_anchor_stats': (i32, [ip, C.c_longlong, fp, i32, i32, i32, i32, vp, vp, vp, vp]),
    'y3_eval_offsets':(i32, [ip, i32, i32, i32, ip, vp]),
    'y3_eval_match': (i32, [fp, i32, i32, i32, i32, f32, f32, ip, ip, fp, i32, i32, fp, ip, i32, i32, C.POINTER(C.c_float), i32, ip,
                            vp, vp, C.c_longlong, vp]),     # iou_thr: HOST array
    'y3_eval_ap': (i32, [vp, vp, C.c_longlong, i32, i32, ip, vp, sz, fp, fp, ip, ip, vp]),
    'y3_eval_ap_workspace_bytes': (sz, [C.c_longlong, i32]),
    'y3_eval_match_ranges': (i32, [fp, i32, i32, i32, i32, f32, f32, ip, ip, fp, i32, i32, fp, ip, i32, i32, C.POINTER(C.c_float), i32,
                                   C.POINTER(C.c_float), C.POINTER(C.c_float), i32, ip, vp, vp, vp, C.c_longlong, vp]),   # thr, lo, hi: HOST
    'y3_eval_ap_ranges': (i32, [vp, vp, vp, C.c_longlong, i32, i32, i32, ip, vp, sz, fp, fp, ip, ip, ip, ip, ip, fp, fp, fp, vp]),
    'y3_eval_ap_ranges_workspace_bytes': (sz, [C.c_longlong, i32, i32]),
    'y3_keep_cut': (i32, [fp, ip, i32, i32, i32, fp, vp]),
    'y3_eval_confusion': (i32, [fp, i32, i32, i32, i32, f32, f32, ip, ip, fp, i32, i32, fp, ip, i32, i32, C.POINTER(C.c_float), i32, ip,
                                C.c_longlong, vp, sz, vp, vp]),     # iou_thr: HOST array
    'y3_eval_confusion_workspace_bytes': (sz, [C.c_longlong]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _f = getattr(lib, _name)          # AttributeError if the library lacks a declared symbol
    _f.restype = _res
    _f.argtypes = _args

EPI_LRELU = 1
EPI_ACCUM = 2
BF16_ROUTE_PP, BF16_ROUTE_C32, BF16_ROUTE_C64, BF16_ROUTE_RING = 1, 2, 3, 4   # Y3_BF16_ROUTE_*: out12[0] of y3_conv2d_fwd_bf16_plan
BF16_NO_PATCH = 8   # Y3_BF16_NO_PATCH: keep a y3_conv2d_fwd_bf16 launch off the patch kernels (small batches, yolo3hip.h)
OPT_SGD, OPT_SGD_NESTEROV, OPT_ADAMW, OPT_MAX_RANGES = 0, 1, 2, 128   # Y3_OPT_*: y3_optim_desc.kind, and the longest range table
CONV_X3 = 4      # Y3_CONV_X3: fp32 arithmetic as three bf16 pieces per operand (conv_x3.hip); the weight operand changes layout


def check(rc, what=''):
    if rc != 0:
        raise HipError('%s failed (%d): %s' % (what or 'libyolo3hip call', rc, lib.y3_last_error().decode()))


def view(t, n, h, w, c, ld=None, offset=0):
    """Tensor struct over a torch CUDA tensor's storage (offset and ld in elements of t's dtype)."""
    return Tensor(t.data_ptr() + t.element_size() * offset, n, h, w, c, c if ld is None else ld)


def float_array(vals):
    arr = (C.c_float * len(vals))(*[float(v) for v in vals])
    return arr


def int_array(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])
