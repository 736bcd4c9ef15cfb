"""ctypes binding of the C ABI in ``include/mpnhip.h`` (``mpntrackseg_amd/csrc/libmpnhip.so``).

This is the only place the Python host code touches native code.  PyTorch is used for device
memory (``tensor.data_ptr()``) and the current HIP stream -- plumbing; every numeric op of the hot
path runs in the hand-written HIP kernels behind these entry points.  There is NO CPU fallback:
if the library cannot be loaded, or a tensor is not on a HIP device, the call raises.
"""
import ctypes as C
import functools
import os

import torch

MAX_LAYERS = 8
AGG_CODE = {"sum": 0, "mean": 1, "max": 2}

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libmpnhip.so")
_lib = None


class MpnhipError(RuntimeError):
    pass


# mpnhip_model.precision (include/mpnhip.h)
PRECISIONS = {'fp32': 0, 'bf16': 1, 'fp32_split': 2, 'fp32_wgsplit': 3}


class Mlp(C.Structure):
    _fields_ = [
        ("n_layers", C.c_int),
        ("in_dim", C.c_int),
        ("out_dims", C.c_int * MAX_LAYERS),
        ("weight", C.c_void_p * MAX_LAYERS),
        ("bias", C.c_void_p * MAX_LAYERS),
        ("grad_weight", C.c_void_p * MAX_LAYERS),
        ("grad_bias", C.c_void_p * MAX_LAYERS),
    ]


class Model(C.Structure):
    _fields_ = [
        ("dn", C.c_int), ("de", C.c_int), ("reattach_nodes", C.c_int), ("reattach_edges", C.c_int),
        ("agg", C.c_int), ("num_enc_steps", C.c_int),
        ("enc_node", Mlp), ("enc_edge", Mlp), ("edge", Mlp), ("flow_in", Mlp), ("flow_out", Mlp),
        ("node", Mlp), ("classifier", Mlp), ("precision", C.c_int), ("weights_prepacked", C.c_int),
    ]


class LinearBf16Args(C.Structure):
    """``mpnhip_linear_bf16_args`` (include/mpnhip.h)."""
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int64), ("x2", C.c_void_p), ("ldx2", C.c_int64), ("w", C.c_void_p), ("ldw", C.c_int64),
        ("b", C.c_void_p), ("c_in", C.c_void_p), ("ldc_in", C.c_int64), ("mask", C.c_void_p), ("ldmask", C.c_int64),
        ("y", C.c_void_p), ("ldy", C.c_int64), ("y16", C.c_void_p), ("ldy16", C.c_int64), ("m", C.c_int64),
        ("n", C.c_int), ("k", C.c_int), ("ksplit", C.c_int), ("x_bf16", C.c_int), ("w_bf16", C.c_int), ("relu", C.c_int),
        ("accumulate", C.c_int),
    ]


class SegJob(C.Structure):
    """``mpnhip_seg_job`` (include/mpnhip.h): one segmented sum of ``mpnhip_debug_segment_reduce3``."""
    _fields_ = [
        ("src", C.c_void_p), ("lds", C.c_int64), ("list", C.c_void_p), ("ptr", C.c_void_p), ("nseg", C.c_int), ("dim", C.c_int),
        ("out", C.c_void_p), ("ldo", C.c_int64), ("nmod", C.c_int), ("off0", C.c_int), ("off1", C.c_int), ("runs", C.c_int),
        ("run_stride", C.c_int), ("out16", C.c_void_p), ("ldo16", C.c_int64),
    ]


class DebugGemmGroup(C.Structure):
    """``mpnhip_debug_gemm_group`` (include/mpnhip.h): one row group of ``mpnhip_debug_gemm``."""
    _fields_ = [(n, C.c_void_p) for n in ("A", "A2", "a_idx", "B", "bias", "G1", "g1_idx", "G2", "g2_idx", "mask", "C", "c_idx",
                                          "row_begin", "row_end")] + \
               [(n, C.c_int64) for n in ("lda", "lda2", "ldb", "ldg1", "ldg2", "ldmask", "ldc", "m_static")]


class DebugGemmArgs(C.Structure):
    """``mpnhip_debug_gemm_args`` (include/mpnhip.h)."""
    _fields_ = [
        ("g", DebugGemmGroup * 2), ("ngroups", C.c_int), ("N", C.c_int), ("K", C.c_int), ("ksplit", C.c_int), ("relu", C.c_int),
        ("accumulate", C.c_int), ("m_upper", C.c_int64), ("small_tiles", C.c_int), ("b_layout", C.c_int), ("precision", C.c_int),
    ]


class WgradGroup(C.Structure):
    """``mpnhip_wgrad_group`` (include/mpnhip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("grad_w", "grad_b", "row_begin", "row_end")]


class WgradProduct(C.Structure):
    """``mpnhip_wgrad_product`` (include/mpnhip.h): one product of ``mpnhip_debug_weight_grad_batch``."""
    _fields_ = [
        ("dZ", C.c_void_p), ("ldz", C.c_int64), ("z_bstride", C.c_int64), ("dz_idx", C.c_void_p),
        ("H", C.c_void_p), ("ldh", C.c_int64), ("h_bstride", C.c_int64), ("h_idx", C.c_void_p),
        ("H2", C.c_void_p), ("ldh2", C.c_int64), ("h2_bstride", C.c_int64),
        ("ldw", C.c_int64), ("rows", C.c_int64), ("csplit", C.c_int), ("n_out", C.c_int), ("k_in", C.c_int), ("nbatch", C.c_int),
        ("src16", C.c_int), ("g", WgradGroup * 2),
    ]


CONV_MAX_SEGMENTS = 4


class ConvArgs(C.Structure):
    """``mpnhip_conv_args`` (include/mpnhip.h): one convolution / transposed convolution of ``mpnhip_conv2d_forward``."""
    _fields_ = [
        ("seg_data", C.c_void_p * CONV_MAX_SEGMENTS), ("seg_stride", C.c_int64 * CONV_MAX_SEGMENTS),
        ("seg_channels", C.c_int * CONV_MAX_SEGMENTS), ("n_segments", C.c_int), ("H", C.c_int), ("W", C.c_int), ("cout", C.c_int),
        ("ksize", C.c_int), ("transposed", C.c_int), ("relu", C.c_int), ("n_images", C.c_int64), ("weight", C.c_void_p),
        ("bias", C.c_void_p), ("out", C.c_void_p), ("out_stride", C.c_int64),
    ]


FPN_LEVELS = 4


class FpnLevels(C.Structure):
    """``mpnhip_fpn_levels`` (include/mpnhip.h): the four levels of one feature pyramid."""
    _fields_ = [("data", C.c_void_p * FPN_LEVELS), ("h", C.c_int * FPN_LEVELS), ("w", C.c_int * FPN_LEVELS), ("scale", C.c_float * FPN_LEVELS)]


class DebugEdgeChainFwd(C.Structure):
    """``mpnhip_debug_edge_chain_fwd`` (include/mpnhip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("P", "e0", "e_prev", "e_new", "msg", "logits", "h1", "hc", "hf", "mask")] + \
               [("save", C.c_int), ("hoist_e0", C.c_int)]


class DebugEdgeChainBf16Fwd(C.Structure):
    """``mpnhip_debug_edge_chain_bf16_fwd`` (include/mpnhip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("P", "e0", "e_prev", "e_new", "msg", "agg_out", "logits", "e16", "h1", "hc", "hf", "dec_h1", "dec_e",
                                          "dec_hc", "dec_hf", "dec_m", "mask")] + \
               [(n, C.c_int) for n in ("save", "rows16", "fused_agg", "plain_barriers")]


class DebugEdgeChainBwd(C.Structure):
    """``mpnhip_debug_edge_chain_bwd`` (include/mpnhip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("dAGG", "ARG", "dlog", "mask", "dE_io", "dZM", "dZF", "dZc", "dZ1", "dE0", "dEprev", "dZ2")] + \
               [("first_step", C.c_int), ("skip_e0", C.c_int), ("plain_barriers", C.c_int)]


# name -> (restype, argtypes); mirrors include/mpnhip.h one to one (tests/test_capi_symbols.py
# checks that every function the header declares is listed here and exported by the library)
class ConvBwdArgs(C.Structure):
    """``mpnhip_conv_bwd_args`` (include/mpnhip.h): the backward of one Conv2d (+ fused ReLU) of ``mpnhip_conv2d_backward``."""
    _fields_ = [
        ("seg_data", C.c_void_p * CONV_MAX_SEGMENTS), ("seg_stride", C.c_int64 * CONV_MAX_SEGMENTS),
        ("seg_channels", C.c_int * CONV_MAX_SEGMENTS), ("n_segments", C.c_int), ("H", C.c_int), ("W", C.c_int), ("cout", C.c_int),
        ("ksize", C.c_int), ("transposed", C.c_int), ("relu", C.c_int), ("n_images", C.c_int64), ("weight", C.c_void_p),
        ("y", C.c_void_p), ("y_stride", C.c_int64), ("grad_out", C.c_void_p), ("grad_out_stride", C.c_int64),
        ("grad_in", C.c_void_p), ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p),
    ]


class ConvAffineArgs(C.Structure):
    """``mpnhip_conv_affine_args`` (include/mpnhip.h): one Conv2d + folded BatchNorm + residual + ReLU of
    ``mpnhip_conv2d_affine_forward``."""
    _fields_ = [
        ("x", C.c_void_p), ("x_stride", C.c_int64), ("weight", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
        ("residual", C.c_void_p), ("residual_stride", C.c_int64), ("relu", C.c_int), ("out", C.c_void_p), ("out_stride", C.c_int64),
        ("n_images", C.c_int64), ("cin", C.c_int), ("cout", C.c_int), ("H", C.c_int), ("W", C.c_int), ("ksize", C.c_int),
        ("stride", C.c_int),
    ]


class ConvAffineUpArgs(C.Structure):
    """``mpnhip_conv_affine_up_args`` (include/mpnhip.h): ``ConvAffineArgs`` whose residual is a coarser map of
    ``residual_H x residual_W``, read at the nearest-neighbour source cell (``mpnhip_conv2d_affine_up_forward``)."""
    _fields_ = ConvAffineArgs._fields_ + [("residual_H", C.c_int), ("residual_W", C.c_int)]


_P, _I, _L, _Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
SIGNATURES = {
    "mpnhip_version": (C.c_char_p, []),
    "mpnhip_last_error": (C.c_char_p, []),
    "mpnhip_debug_counters": (_I, [C.POINTER(C.c_int64), _I, _I]),
    "mpnhip_debug_counter_name": (C.c_char_p, [_I]),
    "mpnhip_debug_saved": (_I, [C.POINTER(Model), _P, _I, _L, _P, _Z, _I, _I, _I, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int), _P]),
    "mpnhip_debug_backward_saved": (_I, [C.POINTER(Model), _I, _L, _P, _Z, _I, _I, _I, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int), _P]),
    "mpnhip_debug_aggregate": (_I, [_P, _I, _L, _P, _I, _I, _P, _P, _P]),
    "mpnhip_debug_segment_reduce3": (_I, [C.POINTER(SegJob), _L, _I, _P]),
    "mpnhip_debug_gemm": (_I, [C.POINTER(DebugGemmArgs), C.POINTER(C.c_int32), _P]),
    "mpnhip_debug_linear_splitk_scratch_floats": (_Z, [_L, _I, _I]),
    "mpnhip_debug_linear_splitk": (_I, [_P, _L, _P, _P, _P, _L, _L, _I, _I, _I, _I, _P, _P, _I, _I, _P, _L, _P, _Z, C.POINTER(C.c_int32),
                                        _P]),
    "mpnhip_debug_weight_grad_batch_workspace_bytes": (_Z, [C.POINTER(WgradProduct), _I, _I, _I, _L]),
    "mpnhip_debug_weight_grad_batch": (_I, [C.POINTER(WgradProduct), _I, _I, _I, _I, _L, _P, _Z, C.POINTER(C.c_int32), _P]),
    "mpnhip_debug_edge_chain_mask_ints": (_Z, [C.POINTER(Model), _L]),
    "mpnhip_debug_edge_chain_forward_workspace_bytes": (_Z, [C.POINTER(Model), _L]),
    "mpnhip_debug_edge_chain_forward": (_I, [C.POINTER(Model), _P, _I, _L, C.POINTER(DebugEdgeChainFwd), _P, _Z, _P]),
    "mpnhip_debug_edge_chain_backward_workspace_bytes": (_Z, [C.POINTER(Model)]),
    "mpnhip_debug_edge_chain_backward": (_I, [C.POINTER(Model), _P, _I, _L, C.POINTER(DebugEdgeChainBwd), _P, _Z, _P]),
    "mpnhip_debug_edge_chain_bf16_mask_ints": (_Z, [C.POINTER(Model), _L]),
    "mpnhip_debug_edge_chain_bf16_forward_workspace_bytes": (_Z, [C.POINTER(Model), _L]),
    "mpnhip_debug_edge_chain_bf16_geometry": (None, [C.POINTER(Model), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mpnhip_debug_edge_chain_bf16_forward": (_I, [C.POINTER(Model), _P, _I, _L, C.POINTER(DebugEdgeChainBf16Fwd), _P, _Z, _P]),
    "mpnhip_debug_node_chain_workspace_bytes": (_Z, [_I, _I]),
    "mpnhip_debug_node_chain": (_I, [_P, _I, _L, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_debug_node_chain_backward_workspace_bytes": (_Z, [_I, _I]),
    "mpnhip_debug_node_chain_backward": (_I, [_I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_graph_bytes": (_Z, [_I, _L]),
    "mpnhip_graph_prep_workspace_bytes": (_Z, [_I, _L]),
    "mpnhip_graph_prep": (_I, [_P, _I, _L, _P, _Z, _P, _Z, _P]),
    "mpnhip_graph_prep_forward": (_I, [_P, _I, _L, _P, _Z, _P, _Z, _P]),
    "mpnhip_graph_status": (_I, [_P, _I, _L, C.POINTER(C.c_int32), _P]),
    "mpnhip_forward_workspace_bytes": (_Z, [C.POINTER(Model), _I, _L, _I]),
    "mpnhip_forward": (_I, [C.POINTER(Model), _P, _I, _L, _P, _P, _P, _P, _P, _P, _Z, _I, _P]),
    "mpnhip_backward_workspace_bytes": (_Z, [C.POINTER(Model), _I, _L]),
    "mpnhip_backward": (_I, [C.POINTER(Model), _P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _P]),
    "mpnhip_backward_flags": (_I, [C.POINTER(Model), _P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _I, _P]),
    "mpnhip_backward_uses_side_stream": (_I, [C.POINTER(Model)]),
    "mpnhip_side_stream": (_P, []),
    "mpnhip_side_stream_join": (_I, [_P]),
    "mpnhip_meta_layer_workspace_bytes": (_Z, [C.POINTER(Model), _I, _L]),
    "mpnhip_meta_layer_forward": (_I, [C.POINTER(Model), _P, _I, _L, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_segment_reduce_workspace_bytes": (_Z, [_L, _I]),
    "mpnhip_segment_reduce": (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "mpnhip_segment_reduce_backward": (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _P, _P]),
    "mpnhip_bn_dropout_workspace_bytes": (_Z, [_L, _I]),
    "mpnhip_bn_relu_dropout_forward": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, C.c_float, C.c_float, _I, C.c_float, C.c_uint64, _P, _P, _P,
                                            _P, _Z, _P]),
    "mpnhip_bn_relu_dropout_backward": (_I, [_P, _P, _L, _I, _I, _P, _P, _P, _P, _I, C.c_float, C.c_uint64, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_linear": (_I, [_P, _L, _P, _P, _P, _L, _L, _I, _I, _I, _P]),
    "mpnhip_linear_bf16": (_I, [_P, _P]),
    "mpnhip_to_bf16": (_I, [_P, _P, _L, _P]),
    "mpnhip_time_linear_bf16": (_I, [_P, _I, C.POINTER(C.c_float), _P]),
    "mpnhip_weight_grad_workspace_bytes": (_Z, [_I, _I, _L, _I]),
    "mpnhip_weight_grad": (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "mpnhip_time_weight_grad": (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P, _Z, _I, C.POINTER(C.c_float), _P]),
    "mpnhip_weight_grad_prec": (_I, [_P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "mpnhip_weight_grad_bf16_rows_workspace_bytes": (_Z, [_I, _I, _L, _I]),
    "mpnhip_weight_grad_bf16_rows": (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "mpnhip_time_weight_grad_prec": (_I, [_P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _Z, _I, C.POINTER(C.c_float), _P]),
    "mpnhip_mlp_workspace_bytes": (_Z, [C.POINTER(Mlp), _L]),
    "mpnhip_mlp_forward": (_I, [C.POINTER(Mlp), _P, _P, _L, _P, _Z, _P]),
    "mpnhip_tracking_loss_workspace_bytes": (_Z, [_I, _L]),
    "mpnhip_tracking_loss": (_I, [_P, _P, _I, _L, _I, C.c_float, _P, _P, _P, _Z, _P]),
    "mpnhip_tracking_loss_graphs_workspace_bytes": (_Z, [_I, _L, _I]),
    "mpnhip_tracking_loss_graphs": (_I, [_P, _P, _P, _I, _I, _L, _I, C.c_float, _P, _P, _P, _Z, _P]),
    "mpnhip_step_metrics": (_I, [_P, _I, _L, _P, _P, _P, _P]),
    "mpnhip_step_metrics_graphs": (_I, [_P, _I, _L, _P, _P, _P, _P, _I, _P, _P]),
    "mpnhip_edge_labels_workspace_bytes": (_Z, [_L]),
    "mpnhip_edge_labels": (_I, [_P, _L, _P, _L, _I, _P, _P, _P, _Z, _P]),
    "mpnhip_mask_loss_workspace_bytes": (_Z, [_I, _L, _L, _I]),
    "mpnhip_mask_loss": (_I, [_P, _I, _P, _P, _P, _I, _L, _L, C.c_float, _P, _P, _P, _Z, _P]),
    "mpnhip_attention_aggregate": (_I, [_P, _I, _L, _P, _L, _P, _P, _P, _P, _P]),
    "mpnhip_attention_aggregate_backward": (_I, [_P, _I, _L, _P, _L, _P, _P, _P, _P, _I, _P, _P, _P]),
    "mpnhip_avgpool": (_I, [_P, _L, _I, _P, _P]),
    "mpnhip_conv2d_forward": (_I, [C.POINTER(ConvArgs), _P]),
    "mpnhip_conv2d_backward_workspace_bytes": (_Z, [C.POINTER(ConvBwdArgs)]),
    "mpnhip_conv2d_backward": (_I, [C.POINTER(ConvBwdArgs), _P, _Z, _P]),
    "mpnhip_layer_norm_forward": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int), _I, _L, _L, _P, _P, C.c_float,
                                       _P, _L, _P]),
    "mpnhip_conv_transpose2d_backward_workspace_bytes": (_Z, [C.POINTER(ConvBwdArgs)]),
    "mpnhip_conv_transpose2d_backward": (_I, [C.POINTER(ConvBwdArgs), _P, _Z, _P]),
    "mpnhip_layer_norm_backward_workspace_bytes": (_Z, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int), _I, _L, _L, _P,
                                                        C.c_float, _P, _L, _P, _P, _P]),
    "mpnhip_layer_norm_backward": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int), _I, _L, _L, _P, C.c_float, _P,
                                        _L, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_conv2d_affine_forward": (_I, [C.POINTER(ConvAffineArgs), _P]),
    "mpnhip_conv2d_affine_up_forward": (_I, [C.POINTER(ConvAffineUpArgs), _P]),
    "mpnhip_maxpool2d_forward": (_I, [_P, _L, _L, _I, _I, _I, _P, _L, _P]),
    "mpnhip_adam_step": (_I, [_P, _P, _P, _P, _L, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _I, _P]),
    "mpnhip_adam_step_guarded": (_I, [_P, _P, _P, _P, _L, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _I, _P, _P]),
    "mpnhip_adam_step_counted": (_I, [_P, _P, _P, _P, _L, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _I, _P, _P, _P]),
    "mpnhip_time_valid_conn_workspace_bytes": (_Z, [_I]),
    "mpnhip_time_valid_conn_count": (_I, [_P, _I, _L, _P, _P, _Z, _P]),
    "mpnhip_time_valid_conn_fill": (_I, [_P, _I, _L, _P, _L, _P, _P]),
    "mpnhip_time_valid_conn_directed_count": (_I, [_P, _I, _L, _P, _P, _Z, _P]),
    "mpnhip_time_valid_conn_directed_fill": (_I, [_P, _I, _L, _P, _L, _P, _P]),
    "mpnhip_edge_features": (_I, [_P, _L, _I, _P, C.c_float, _P, _P, _P, _P, _P, _P]),
    "mpnhip_pairwise_distance": (_I, [_P, _L, _I, _P, _L, C.c_float, _P, _P]),
    "mpnhip_embedding_keep": (_I, [_P, _L, _L, _P, _L, _P, _P]),
    "mpnhip_embedding_check": (_I, [_P, _L, _P, _L, _P, _P, _P]),
    "mpnhip_knn_mask_workspace_bytes": (_Z, [_L, _I]),
    "mpnhip_knn_mask": (_I, [_P, _P, _I, _L, _I, _I, _I, _P, _P, _Z, _P]),
    "mpnhip_window_flags": (_I, [_P, _L, _L, _L, _P, _P]),
    "mpnhip_compact_workspace_bytes": (_Z, [_L]),
    "mpnhip_compact": (_I, [_P, _L, _P, _P, _P, _Z, _P]),
    "mpnhip_gather_rows": (_I, [_P, _L, _P, _L, _I, _P, _P]),
    "mpnhip_gather_edges": (_I, [_P, _L, _P, _L, _L, _P, _P]),
    "mpnhip_window_accumulate": (_I, [_P, _P, _L, _P, _L, _I, _P, _P, _P]),
    "mpnhip_average_preds": (_I, [_P, _P, _L, _P, _P]),
    "mpnhip_node_mask_accumulate": (_I, [_P, _L, _L, _L, _L, _P, _P, _P]),
    "mpnhip_node_mask_average": (_I, [_P, _P, _L, _L, _P, _P]),
    "mpnhip_undirected_merge_workspace_bytes": (_Z, [_L]),
    "mpnhip_undirected_merge_sort": (_I, [_P, _L, _L, _P, _P, _P, _Z, _P]),
    "mpnhip_undirected_merge_fill": (_I, [_L, _L, _P, _Z, _P, _P, _P, _P]),
    "mpnhip_threshold_flags": (_I, [_P, _L, C.c_float, _P, _P]),
    "mpnhip_project_round_count_workspace_bytes": (_Z, [_L]),
    "mpnhip_project_round_count": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_project_greedy_workspace_bytes": (_Z, [_L]),
    "mpnhip_project_greedy": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_project_violated_masks": (_I, [_P, _L, _L, _P, _P, _P, _P, _P]),
    "mpnhip_connected_components_workspace_bytes": (_Z, [_L]),
    "mpnhip_connected_components": (_I, [_P, _L, _L, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_track_lengths": (_I, [_P, _L, _L, _P, _P, _P]),
    "mpnhip_project_exact_workspace_bytes": (_Z, [_L, _L]),
    "mpnhip_project_exact_plan": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_project_exact_fill": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _P, _L, _P, _Z, _P]),
    "mpnhip_project_exact_apply": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _L, _P, _P, _Z, _P]),
    "mpnhip_full_masks_workspace_bytes": (_Z, [_L, _L, _L, _L]),
    "mpnhip_paste_unique_masks": (_I, [_P, _L, _I, _I, _P, _P, _L, _P, _L, _I, _I, C.c_float, _P, _P, _P, _Z, _P]),
    "mpnhip_mask_run_events_count": (_I, [_P, _L, _L, _L, _P, _P, _P, _Z, _P]),
    "mpnhip_mask_run_events": (_I, [_P, _L, _L, _L, _L, _P, _P, _Z, _P]),
    "mpnhip_rle_encode_workspace_bytes": (_Z, [_L, _L]),
    "mpnhip_rle_encode": (_I, [_P, _P, _L, _L, _L, _P, _L, _P, _P, _Z, _P]),
    "mpnhip_rle_decode_workspace_bytes": (_Z, [_L]),
    "mpnhip_rle_decode_scan": (_I, [_P, _L, _P, _P, _L, _P, _P, _P, _P, _P]),
    "mpnhip_rle_decode_runs": (_I, [_P, _L, _P, _P, _L, _P, _P, _L, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_mots_workspace_bytes": (_Z, [_L, _L, _L, _L, _L]),
    "mpnhip_paint_label_runs": (_I, [_P, _P, _P, _L, _P, _L, _L, _L, _P, _P, _Z, _P]),
    "mpnhip_label_overlap": (_I, [_P, _P, _P, _L, _P, _L, _P, _P, _L, _L, _P, _L, _P]),
    "mpnhip_mots_frame_match": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_hota_workspace_bytes": (_Z, [_L, _L, _L, _L, _L]),
    "mpnhip_hota_frame_similarity": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _L, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_hota_accumulate_alignment": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _P, _P, _L, _L, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_hota_frame_scores": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _L, _L, _P, _P, _P, _P, _P]),
    "mpnhip_hota_alpha_accumulate": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _P, _P, _L, _L, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_hota_association": (_I, [_P, _P, _P, _L, _L, _P, _P, _Z, _P]),
    "mpnhip_clear_identity_workspace_bytes": (_Z, [_L, _L, _L, _L, _L]),
    "mpnhip_identity_accumulate": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _L, _L, _P, _P]),
    "mpnhip_identity_sums": (_I, [_P, _P, _L, _L, _P, _P]),
    "mpnhip_clear_frame_candidates": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _L, _L, _P, _P, _P, _P]),
    "mpnhip_clear_sequence_scan": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _P, _P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                        _Z, _P]),
    "mpnhip_clear_track_summary": (_I, [_P, _P, _P, _L, _P, _P]),
    "mpnhip_lsa_workspace_bytes": (_Z, [_L, _L, _L]),
    "mpnhip_lsa_batched": (_I, [_P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _I, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_box_iou_costs": (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _L, C.c_double, _P, _P, _P, _P]),
    "mpnhip_overlap_iou_costs": (_I, [_P, _L, _P, _P, _L, _P, _L, _P, _L, _L, C.c_double, _P, _P, _P, _P]),
    "mpnhip_gt_assign_finish": (_I, [_P, _P, _L, _P, _P, _L, _P, _L, _L, _P, _P, _P, _L, _P, _P, _P]),
    "mpnhip_roi_align_labels": (_I, [_P, _L, _I, _I, _P, _P, _P, _L, _P, _P, _L, _P, _P, _L, _P, _I, _I, _I, _P, _P, _P]),
    "mpnhip_reid_crops_workspace_bytes": (_Z, [_L, _I, _I, _I, _I]),
    "mpnhip_reid_crops": (_I, [_P, _L, _I, _I, _P, _P, _L, _I, _I, _I, _I, C.POINTER(C.c_float), _P, _P, _P, _Z, _P]),
    "mpnhip_rcnn_transform": (_I, [_P, _L, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_float), _P, _P]),
    "mpnhip_fpn_roi_align": (_I, [C.POINTER(FpnLevels), _L, _I, _P, _P, _P, _L, _I, _I, _P, _P, _P]),
    "mpnhip_box_predict": (_I, [_P, _L, _P, _P, _P, _P, _P, _L, _I, _I, _I, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, _P, _P, _P,
                                _P, _P]),
    "mpnhip_nms_batched_workspace_bytes": (_Z, [_L, _I]),
    "mpnhip_nms_batched": (_I, [_P, _P, _P, _L, _L, _I, C.c_float, C.c_float, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_roi_mask_finish": (_I, [_P, _L, _L, _I, _I, _I, _I, _P, _P]),
    "mpnhip_augment_boxes_workspace_bytes": (_Z, []),
    "mpnhip_augment_boxes": (_I, [_P, _P, _P, _L, _P, _P, _L, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_batch_pairs_workspace_bytes": (_Z, [_L]),
    "mpnhip_batch_pairs_count": (_I, [_P, _P, _P, _L, _L, _L, _P, _P, _Z, _P]),
    "mpnhip_batch_pairs_fill": (_I, [_P, _P, _P, _L, _L, _L, _P, _L, _P, _P]),
    "mpnhip_batch_edge_features": (_I, [_P, _L, _L, _P, _P, _P, _L, _P, _P, _L, _I, C.c_float, _P, _P, _P]),
    "mpnhip_batch_edge_layout_workspace_bytes": (_Z, [_L]),
    "mpnhip_batch_edge_layout": (_I, [_P, _L, _P, _L, _P, _L, _L, _P, _P, _P, _I, _P, _P, _P, _P, _Z, _P]),
    "mpnhip_profile_enable": (_I, [_I]),
    "mpnhip_edge_chain_active": (_I, [C.POINTER(Model)]),
    "mpnhip_profile_read": (_I, [C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int),
                                 C.POINTER(C.c_float)]),
    "mpnhip_profile_read_kind": (_I, [_I, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "mpnhip_time_aggregate": (_I, [_P, _I, _L, _P, _I, _I, _P, _I, C.POINTER(C.c_float), _P]),
    "mpnhip_time_linear": (_I, [_P, _P, _P, _P, _L, _I, _I, _I, C.POINTER(C.c_float), _P]),
}


def lib_path():
    return _LIB_PATH


def load():
    """Load libmpnhip.so (built by ``make`` / ``__graft_entry__.build()``); raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise MpnhipError(
                f"{_LIB_PATH} is missing: build it with `make` (or `python -c 'import __graft_entry__ as g; "
                "g.build()'`). mpntrackseg_amd has no CPU fallback.")
        lib = C.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def path_counters(reset=False):
    """{kernel-variant name: launches since the last reset} (``mpnhip_debug_counters``): which code paths the calls took."""
    lib = load()
    n = lib.mpnhip_debug_counters(None, 0, 0)
    arr = (C.c_int64 * n)()
    lib.mpnhip_debug_counters(arr, n, 1 if reset else 0)
    return {lib.mpnhip_debug_counter_name(i).decode(): int(arr[i]) for i in range(n)}


SAVED = {"enc_node": 0, "enc_edge": 1, "x": 2, "e": 3, "edge_hidden": 4, "cls_hidden": 5, "flow_hidden": 6, "msg": 7, "agg": 8,
         "argmax": 9}


def saved_activation(model, graph, fwd_ws, what, step=0, layer=0):
    """One activation a training forward (``autograd.native_forward_saved``) left in ``fwd_ws``, in original node / edge order
    (``mpnhip_debug_saved``); test instrumentation."""
    lib = load()
    m = model.c_model([])
    rows, width = C.c_int64(0), C.c_int(0)
    with torch.cuda.device(graph.device):
        check(lib.mpnhip_debug_saved(m, ptr(graph.buf), graph.N, graph.E, ptr(fwd_ws), fwd_ws.numel(), SAVED[what], int(step), int(layer),
                                     None, C.byref(rows), C.byref(width), stream_ptr()), "mpnhip_debug_saved")
        out = torch.empty((rows.value, width.value), dtype=torch.float32, device=graph.device)
        check(lib.mpnhip_debug_saved(m, ptr(graph.buf), graph.N, graph.E, ptr(fwd_ws), fwd_ws.numel(), SAVED[what], int(step), int(layer),
                                     ptr(out), C.byref(rows), C.byref(width), stream_ptr()), "mpnhip_debug_saved")
    return out


WG_PATHS = {-1: None, 0: "panel", 1: "rows16", 2: "tn_mfma", 3: "tn_narrowk", 4: "tn_small", 5: "tn_generic"}
WG_CHOSEN_FIELDS = ("path", "variant", "tiles_o", "tiles_c", "chunk", "nsplit", "narrow", "rolled", "xcd_map", "red_ny")


def debug_weight_grad_batch(products, precision, batched=False, one_launch=False, batch_slab_floats=0, fill=None):
    """The backward's weight-gradient routing over a list of ``WgradProduct`` (``mpnhip_debug_weight_grad_batch``); test
    instrumentation.  ``fill``: byte pattern the workspace is prefilled with.  Returns ``(rc, chosen)``: the status code (not
    raised: refusals are part of what the tests check) and per product a list of two dicts (``WG_CHOSEN_FIELDS``, ``path`` as a
    name of ``WG_PATHS``)."""
    lib = load()
    n = len(products)
    arr = (WgradProduct * n)(*products)
    prec = PRECISIONS[precision]
    need = lib.mpnhip_debug_weight_grad_batch_workspace_bytes(arr, n, prec, int(batched), int(batch_slab_floats))
    ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    out = (C.c_int32 * (n * 2 * len(WG_CHOSEN_FIELDS)))()
    rc = lib.mpnhip_debug_weight_grad_batch(arr, n, prec, int(batched), int(one_launch), int(batch_slab_floats), ptr(ws), ws.numel(), out,
                                            stream_ptr())
    torch.cuda.synchronize()
    nf = len(WG_CHOSEN_FIELDS)
    chosen = []
    for i in range(n):
        pair = []
        for q in range(2):
            d = dict(zip(WG_CHOSEN_FIELDS, out[(i * 2 + q) * nf:(i * 2 + q + 1) * nf]))
            d["path"] = WG_PATHS[d["path"]]
            pair.append(d)
        chosen.append(pair)
    return rc, chosen


BWD_SAVED = {"dz_node": 0, "dp": 1, "dz_flow": 2, "dz_edge": 3, "dz_cls": 4}


def backward_saved(model, graph, bwd_ws, what, step, layer=0):
    """One block of pre-activation gradients ``mpnhip_backward`` left in its workspace (``mpnhip_debug_backward_saved``);
    edges in sorted order.  Test / diagnosis instrumentation."""
    lib = load()
    m = model.c_model([])
    rows, width = C.c_int64(0), C.c_int(0)
    with torch.cuda.device(graph.device):
        check(lib.mpnhip_debug_backward_saved(m, graph.N, graph.E, ptr(bwd_ws), bwd_ws.numel(), BWD_SAVED[what], int(step), int(layer), None,
                                              C.byref(rows), C.byref(width), stream_ptr()), "mpnhip_debug_backward_saved")
        out = torch.empty((rows.value, width.value), dtype=torch.float32, device=graph.device)
        check(lib.mpnhip_debug_backward_saved(m, graph.N, graph.E, ptr(bwd_ws), bwd_ws.numel(), BWD_SAVED[what], int(step), int(layer), ptr(out),
                                              C.byref(rows), C.byref(width), stream_ptr()), "mpnhip_debug_backward_saved")
    return out


def check(rc, what):
    if rc != 0:
        msg = load().mpnhip_last_error().decode("utf-8", "replace")
        raise MpnhipError(f"{what} failed (code {rc}): {msg}")


def require_device(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise MpnhipError("mpntrackseg_amd runs on a HIP device only (tensor on %s); there is no CPU fallback"
                              % t.device)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_tensor_device(fn):
    """Decorator: run ``fn`` with the HIP device of its first device-tensor argument current, so that ``stream_ptr()`` and
    ``workspace()`` inside refer to THAT device's current stream (one process may hold several GPUs; launching on the
    current device's stream with another device's pointers is an invalid access)."""
    @functools.wraps(fn)
    def wrapper(*args, **kw):
        for a in list(args) + list(kw.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                with torch.cuda.device(a.device):
                    return fn(*args, **kw)
        return fn(*args, **kw)
    return wrapper


def f32c(t):
    """contiguous float32 view/copy of a tensor (no-op for the expected layout)"""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


_ws_cache = {}
# weight images left at the head of a forward workspace: buffer address -> (model id, weight key); see MOTMPNet.hot_path
_packed_state = {}
# bumped by every native in-place parameter update (train.FlatAdam writes through raw pointers: no torch version bump)
_weights_epoch = [0]
_model_uid = [0]  # source of MOTMPNet._mpnhip_uid tokens


def workspace(nbytes, device, tag="ws"):
    """Grow-only scratch buffer from torch's caching allocator, one per (device, tag, current stream of that device): two
    streams of one device never share scratch memory, so calls issued on different streams cannot race on it."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), tag, int(torch.cuda.current_stream(device).cuda_stream))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
        _packed_state.clear()  # a new buffer (possibly at a recycled address) holds no weight images
    return buf


def fill_mlp(dst, linears, with_grads=False, keep=None):
    """Fill an ``Mlp`` struct from a list of nn.Linear-like (weight [out,in], bias [out])."""
    assert 1 <= len(linears) <= MAX_LAYERS, "MLP depth not supported"
    dst.n_layers = len(linears)
    dst.in_dim = int(linears[0][0].shape[1])
    for i, (w, b) in enumerate(linears):
        assert w.dtype == torch.float32 and w.is_contiguous() and b.is_contiguous()
        dst.out_dims[i] = int(w.shape[0])
        dst.weight[i] = w.data_ptr()
        dst.bias[i] = b.data_ptr()
        dst.grad_weight[i] = None
        dst.grad_bias[i] = None
        if keep is not None:
            keep.extend([w, b])
    return dst


def fill_mlp_dims(dst, in_dim, dims, pointer=None):
    """Fill an ``Mlp`` struct with dims only; ``pointer``: an address for every weight, bias and gradient field."""
    dst.n_layers, dst.in_dim = len(dims), int(in_dim)
    for i, w in enumerate(dims):
        dst.out_dims[i] = int(w)
        dst.weight[i] = dst.bias[i] = dst.grad_weight[i] = dst.grad_bias[i] = pointer
    return dst


def dims_model(p, precision="fp32", pointer=None):
    """``Model`` of the ``graph_model_params`` dict ``p`` with dims only -- all the size queries read; ``pointer``: an address to put
    into every weight, bias and gradient field (argument checks that must pass without the pointers ever being followed)."""
    enc, cls = p["encoder_feats_dict"], p["classifier_feats_dict"]
    dn, de = enc["node_out_dim"], enc["edge_out_dim"]
    nf, ef = (2 if p["reattach_initial_nodes"] else 1), (2 if p["reattach_initial_edges"] else 1)
    m = Model()
    m.dn, m.de, m.reattach_nodes, m.reattach_edges = dn, de, nf - 1, ef - 1
    m.agg, m.num_enc_steps, m.precision = AGG_CODE[p["node_agg_fn"]], p["num_enc_steps"], PRECISIONS[precision]
    fill_mlp_dims(m.enc_node, enc["node_in_dim"], list(enc["node_dims"]) + [dn], pointer)
    fill_mlp_dims(m.enc_edge, enc["edge_in_dim"], list(enc["edge_dims"]) + [de], pointer)
    fill_mlp_dims(m.edge, nf * 2 * dn + ef * de, p["edge_model_feats_dict"]["dims"], pointer)
    fill_mlp_dims(m.flow_in, nf * dn + de, p["node_model_feats_dict"]["dims"], pointer)
    fill_mlp_dims(m.flow_out, nf * dn + de, p["node_model_feats_dict"]["dims"], pointer)
    fill_mlp_dims(m.node, 2 * dn, [dn], pointer)
    fill_mlp_dims(m.classifier, cls["edge_in_dim"], list(cls["edge_dims"]) + [cls["edge_out_dim"]], pointer)
    return m


class _StatusRing:
    """Pinned host slots for the asynchronous read-back of graph-prep error flags (a pinned allocation per graph would cost
    more than the prep).  A slot that was recycled before its graph looked at it falls back to the synchronous status()."""

    SLOTS = 512

    def __init__(self):
        self.host = None
        self.owner = [None] * self.SLOTS
        self.events = [None] * self.SLOTS
        self.next = 0

    def post(self, graph):
        if self.host is None:
            self.host = torch.empty((self.SLOTS, 4), dtype=torch.int32, pin_memory=True)
        i = self.next
        self.next = (i + 1) % self.SLOTS
        self.owner[i] = id(graph)
        with torch.cuda.device(graph.device):
            self.host[i].copy_(graph.buf[:16].view(torch.int32), non_blocking=True)
            ev = self.events[i]
            if ev is None:
                ev = self.events[i] = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
        return i

    def read(self, i, graph):
        if self.owner[i] != id(graph):
            return None
        self.events[i].synchronize()
        if self.owner[i] != id(graph):
            return None
        return int(self.host[i, 0])


_status_ring = _StatusRing()


class PreparedGraph:
    """Device-side sort of an edge_index (see ``mpnhip_graph_prep``)."""

    def __init__(self, edge_index, n_nodes, validate=False, full=True):
        """``full=False``: the primary order only (inference forward); anything that differentiates or evaluates the step
        metrics needs ``full=True`` (``self.full`` records which one this is)."""
        require_device(edge_index)
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise MpnhipError("edge_index must be int64 [2, E] (reference data/mot_graph.py:312)")
        lib = load()
        ei = edge_index.contiguous()
        self.N = int(n_nodes)
        self.E = int(ei.shape[1])
        self.device = ei.device
        self.full = bool(full)
        nb = lib.mpnhip_graph_bytes(self.N, self.E)
        self.buf = torch.empty(max(nb, 256), dtype=torch.uint8, device=ei.device)
        wsb = lib.mpnhip_graph_prep_workspace_bytes(self.N, self.E)
        ws = workspace(wsb, ei.device, "prep")
        with torch.cuda.device(ei.device):
            fn = lib.mpnhip_graph_prep if full else lib.mpnhip_graph_prep_forward
            check(fn(ptr(ei), self.N, self.E, ptr(self.buf), self.buf.numel(), ptr(ws), ws.numel(), stream_ptr()),
                  "mpnhip_graph_prep")
        # the error flag travels to the host asynchronously (pinned slot + event on the launch stream); the first consumer
        # that cares reads it with raise_if_invalid() AFTER it has enqueued its own work -- by then the prep is long done
        self._status_slot = None
        self._validated = False
        self._invalid = False
        if validate:
            st = self.status()
            self._validated = True
            if st[0] != 0:
                raise MpnhipError("edge_index has entries outside [0, N)")
        else:
            self._status_slot = _status_ring.post(self)

    def raise_if_invalid(self):
        """The reference raises IndexError from its ``x[row]`` / ``x[col]`` gathers when edge_index leaves [0, N) (mpn.py:69)
        -- on EVERY call; graph prep clamps such entries and sets a flag.  The flag is read once per prepared graph (the read
        waits for the prep kernels only, never for work enqueued after them) and its value kept: every later call on the same
        prepared graph raises again."""
        if not self._validated:
            flag = _status_ring.read(self._status_slot, self) if self._status_slot is not None else None
            if flag is None:
                flag = self.status()[0]
            self._validated = True
            self._status_slot = None
            self._invalid = flag != 0
        if self._invalid:
            raise IndexError("index out of range in edge_index: entries must lie in [0, %d) (reference mpn.py:69 gathers "
                             "x[row], x[col])" % self.N)

    def status(self):
        arr = (C.c_int32 * 4)()
        with torch.cuda.device(self.device):
            check(load().mpnhip_graph_status(ptr(self.buf), self.N, self.E, arr, stream_ptr()), "mpnhip_graph_status")
        return list(arr)
