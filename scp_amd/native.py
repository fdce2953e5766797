"""ctypes binding of libscp_hip.so (include/scp.h).

PyTorch appears here only as the owner of device memory and of the HIP stream; every call below goes
through the C ABI with raw device pointers.  There is NO fallback: if the library is missing or a
call fails, an exception is raised.
"""
import ctypes as C
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libscp_hip.so")
MAX_DEPTH = 21

CART, SPHER, CYLIN = 0, 1, 2
POS_MINMAX, POS_MINMAX_MUL, POS_POW2 = 0, 1, 2
_ERR = {-1: "SCP_EINVAL", -2: "SCP_ENOMEM", -3: "SCP_ESMALL", -4: "SCP_EHIP", -5: "SCP_ESTATE"}


class ScpError(RuntimeError):
    pass


class QuantInfo(C.Structure):
    _fields_ = [("bin_num", C.c_double), ("qs", C.c_double * 3), ("offset", C.c_double * 3),
                ("max_coord", C.c_int32), ("min_coord", C.c_int32)]


class Segment(C.Structure):
    _fields_ = [("point_begin", C.c_int64), ("point_count", C.c_int64), ("path_len", C.c_int32),
                ("path_bits", C.c_int32), ("drop_last", C.c_int32), ("reserved", C.c_int32)]


class SegmentInfo(C.Structure):
    _fields_ = [("depth", C.c_int32), ("max_coord", C.c_int32), ("n_leaves", C.c_int64), ("n_nodes", C.c_int64),
                ("node_base", C.c_int64), ("level_count", C.c_int64 * (MAX_DEPTH + 1))]


_lib = None
_vp = C.c_void_p


ABI_VERSION = 220      # include/scp.h: SCP_ABI_VERSION


def lib():
    """Load libscp_hip.so; raises if it has not been built (python -m scp_amd.build / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScpError(f"{LIB_PATH} is missing: run `python scp_amd/build.py` (hipcc, gfx950). "
                       "The SCP hot path has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    i32, i64 = C.c_int32, C.c_int64
    sig = {
        "scp_version": (C.c_int, []),
        "scp_geo_edge_mlps": (C.c_int, [_vp, i64, _vp, i64, _vp, i64, _vp, _vp, _vp, i64, i32, _vp]),
        "scp_mlp3_rows": (C.c_int, [_vp, i64, i64, _vp, _vp, _vp, _vp, i64, _vp, i32, i32, _vp]),
        "scp_swin_merge": (C.c_int, [_vp, i64, i64, _vp, _vp, _vp, _vp, C.c_float, _vp, i64, i32, _vp]),
        "scp_swin_ln_qkv": (C.c_int, [_vp, i64, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, i64, _vp, i64, i32, i32, _vp]),
        "scp_swin_kv_planes": (C.c_int, [_vp, _vp, i64, i64, _vp, _vp, _vp, _vp, _vp]),
        "scp_swin_attention_packed_planes": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, i32, i32, i32, _vp, _vp, _vp, i64, _vp, _vp]),
        "scp_split_rows_f16": (C.c_int, [_vp, i64, i32, i32, _vp, _vp, i64, _vp, _vp, _vp]),
        "scp_linear_split_f16": (C.c_int, [_vp, _vp, i64, _vp, _vp, _vp, _vp, i32, i32, _vp, _vp, i64, _vp, i64, i32, i32, i32, i32, i32, _vp]),
        "scp_last_hip_error": (C.c_int, []),
        "scp_device_count": (C.c_int, []),
        "scp_device_name": (C.c_int, [C.c_char_p, C.c_int]),
        "scp_quantize": (C.c_int, [_vp, i64, i32, C.c_double, C.c_double, _vp, _vp, C.POINTER(QuantInfo), _vp]),
        "scp_geom_create": (C.c_int, [C.POINTER(_vp)]),
        "scp_geom_destroy": (C.c_int, [_vp]),
        "scp_geom_build": (C.c_int, [_vp, _vp, i64, C.POINTER(Segment), i32, C.POINTER(SegmentInfo), _vp]),
        "scp_geom_build_xyz": (C.c_int, [_vp, _vp, _vp, i32, i32, _vp, i32, C.c_double, C.POINTER(Segment), _vp, C.POINTER(QuantInfo),
                                         C.POINTER(SegmentInfo), _vp]),
        "scp_geom_context_ehem_all": (C.c_int, [_vp, i32, i32, i32, _vp, _vp, _vp, _vp, _vp]),
        "scp_geom_emit_nodes": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "scp_geom_emit_leaves": (C.c_int, [_vp, i32, _vp, _vp]),
        "scp_geom_krecords_i64": (C.c_int, [_vp, i32, _vp, _vp]),
        "scp_geom_context_ehem": (C.c_int, [_vp, i32, i32, i32, _vp, _vp, _vp, _vp, _vp]),
        "scp_geom_context_octattn": (C.c_int, [_vp, i32, _vp, _vp, _vp, _vp]),
        "scp_knn_topk": (C.c_int, [_vp, i32, i32, i32, i32, _vp, _vp]),
        "scp_knn_topk_packed": (C.c_int, [_vp, _vp, i32, i32, _vp, _vp]),
        "scp_knn_topk_packed_bounded": (C.c_int, [_vp, _vp, i32, i32, _vp, _vp, _vp]),
        "scp_swin_attention_packed": (C.c_int, [_vp, _vp, _vp, _vp, _vp, i32, i32, i32, i32, _vp, _vp]),
        "scp_swin_attention_packed_split": (C.c_int, [_vp, _vp, _vp, _vp, _vp, i32, i32, i32, i32, _vp, _vp, i64, _vp]),
        "scp_set_attention_mode": (C.c_int, [i32]),
        "scp_set_attention_variant": (C.c_int, [i32]),
        "scp_get_attention_variant": (C.c_int, []),
        "scp_ctx_create": (C.c_int, [C.POINTER(_vp)]),
        "scp_ctx_destroy": (C.c_int, [_vp]),
        "scp_ctx_set": (C.c_int, [_vp, i32, i32]),
        "scp_ctx_get": (C.c_int, [_vp, i32]),
        "scp_ctx_make_current": (C.c_int, [_vp]),
        "scp_rc_debug_buffer": (C.c_int, [_vp]),
        "scp_rc_set_wide": (C.c_int, [i32]),
        "scp_prof_enable": (C.c_int, [i32]),
        "scp_prof_count": (C.c_int, []),
        "scp_prof_read": (C.c_int, [i32, _vp, _vp, _vp]),
        "scp_set_knn_mode": (C.c_int, [i32]),
        "scp_row_scale_f16": (C.c_int, [_vp, i64, i32, i32, _vp, _vp, _vp]),
        "scp_row_scale_from_max": (C.c_int, [_vp, i32, _vp, _vp, _vp]),
        "scp_linear_split_f16_max": (C.c_int, [_vp, _vp, i64, _vp, _vp, _vp, _vp, i32, i32, _vp, _vp, i64, _vp, i64, i32, i32, i32, i32, i32, _vp, _vp, i32, i32, i32, _vp]),
        "scp_octattn_attention_f16x3_vmax": (C.c_int, [_vp, _vp, _vp, _vp, _vp, i64, i32, i32, i32, i32, _vp, _vp, _vp, i64, _vp, _vp]),
        "scp_linear_f16x3_scaled": (C.c_int, [_vp, i64, _vp, _vp, _vp, i32, _vp, _vp, i64, _vp, i64, i32, i32, i32, i32, _vp, _vp, _vp]),
        "scp_layernorm_add": (C.c_int, [_vp, _vp, i64, i32, _vp, _vp, C.c_float, _vp, _vp]),
        "scp_layernorm_add_split_f16": (C.c_int, [_vp, _vp, i64, i32, _vp, _vp, C.c_float, _vp, _vp, _vp, i64, _vp, _vp, _vp]),
        "scp_set_knn_workgroup": (C.c_int, [i32]),
        "scp_knn_debug_buffer": (C.c_int, [_vp]),
        "scp_nn_sqdist_f64": (C.c_int, [_vp, i64, _vp, i64, _vp, _vp]),
        "scp_estimate_normals_f64": (C.c_int, [_vp, i64, C.c_double, i32, _vp, _vp, _vp, _vp, _vp]),
        "scp_nn_tieset_f64": (C.c_int, [i32, _vp, i64, _vp, i64, _vp, _vp, _vp, _vp]),
        "scp_edge_gather_max_ld": (C.c_int, [_vp, i64, _vp, i64, _vp, _vp, _vp, i32, i32, i32, i32, _vp, i32, _vp]),
        "scp_embed_gather": (C.c_int, [_vp, _vp, _vp, i64, _vp, _vp, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_packed_plan_sizes": (C.c_int, [_vp, i32, _vp]),
        "scp_packed_plan": (C.c_int, [_vp, i32, _vp, _vp, i32, _vp]),
        "scp_decode_expand": (C.c_int, [_vp, _vp, _vp, _vp, _vp, i64, i32, i32, i32, i32, i32, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "scp_edge_gather_max": (C.c_int, [_vp, _vp, _vp, _vp, _vp, i32, i32, i32, i32, _vp, i32, _vp]),
        "scp_swin_attention": (C.c_int, [_vp, _vp, _vp, _vp, i32, i32, i32, i32, i32, _vp, _vp]),
        "scp_octattn_attention": (C.c_int, [_vp, _vp, _vp, _vp, _vp, i32, i32, i32, i32, _vp, _vp, _vp]),
        "scp_octattn_f16x3_ws_bytes": (C.c_int64, [i32, i32, i32]),
        "scp_octattn_embed": (C.c_int, [_vp, _vp, i64, i32, _vp, i32, _vp, i32, i32, _vp, i32, _vp, _vp, i32, _vp, i32, _vp, _vp, _vp, i64, _vp, _vp, _vp]),
        "scp_octattn_attention_f16x3": (C.c_int, [_vp, _vp, _vp, _vp, _vp, i64, i32, i32, i32, i32, _vp, _vp, _vp, i64, _vp]),
        "scp_octattn_attention_rowinv": (C.c_int, [_vp, i64, i64, _vp, _vp, i64, i64, _vp, _vp, i64, i64, _vp, _vp, i64, i64, i32, i32, i32, i32, i32,
                                                   i32, _vp]),
        "scp_octattn_attention_rowinv_step": (C.c_int, [_vp, i64, _vp, _vp, i64, i64, i32, i32, _vp, _vp, i64, _vp, _vp, i64, _vp, _vp, i32, i32, i32,
                                                        _vp]),
        "scp_decode_expand_octattn": (C.c_int, [_vp, _vp, _vp, _vp, i64, i32, i32, i32, _vp, _vp, _vp, _vp, _vp]),
        "scp_decode_expand_batch": (C.c_int, [_vp, _vp, _vp, _vp, _vp, i64, _vp, i32, i32, _vp, i32, i64, i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "scp_split_weight_bf16": (C.c_int, [_vp, i32, i32, i32, i32, _vp, _vp, _vp]),
        "scp_linear_bf16x3": (C.c_int, [_vp, i64, _vp, _vp, i32, _vp, _vp, i64, _vp, i64, i32, i32, i32, i32, _vp]),
        "scp_split_weight_f16": (C.c_int, [_vp, i32, i32, i32, i32, _vp, _vp, _vp, _vp]),
        "scp_linear_f16x3": (C.c_int, [_vp, i64, _vp, _vp, _vp, i32, _vp, _vp, i64, _vp, i64, i32, i32, i32, i32, _vp, _vp]),
        "scp_linear_split": (C.c_int, [_vp, _vp, i64, _vp, _vp, i32, i32, _vp, _vp, i64, _vp, i64, _vp, _vp, i64, i32, i32, i32, i32, i32, _vp]),
        "scp_tile_weight_bf16": (C.c_int, [_vp, i32, i32, _vp, _vp]),
        "scp_swin_ln_linear": (C.c_int, [_vp, i64, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, i64, i32, i32, _vp]),
        "scp_swin_post_attn": (C.c_int, [_vp, _vp, i64, _vp, i64, _vp, _vp, _vp, _vp, C.c_float, _vp, i64, i32, _vp, i32, _vp]),
        "scp_swin_post_attn_weight_bytes": (C.c_int64, []),
        "scp_gelu_prescale": (C.c_double, []),
        "scp_split_rows": (C.c_int, [_vp, i64, i64, _vp, i32, _vp, _vp, i64, i64, _vp]),
        "scp_linear_split_scatter": (C.c_int, [_vp, _vp, i64, _vp, _vp, i32, i32, _vp, _vp, _vp, i64, i32, i32, i32, i32, i32, _vp]),
        "scp_linear_split_gather": (C.c_int, [_vp, _vp, i64, _vp, _vp, i32, i32, _vp, _vp, i64, _vp, _vp, i64, _vp, _vp, i64, i32, i32, i32, i32, i32, _vp]),
        "scp_linear_split_hier2": (C.c_int, [_vp, _vp, i64, i32, _vp, _vp, i64, i64, _vp, _vp, _vp, _vp, i32, _vp, _vp, _vp, i64, _vp, _vp, _vp, i64, i32, i32, i32, _vp]),
        "scp_layernorm_rows": (C.c_int, [_vp, i64, i64, _vp, _vp, i32, _vp, _vp, _vp, C.c_float, _vp, i64, i64, _vp]),
        "scp_layernorm_rows_split": (C.c_int, [_vp, i64, i64, _vp, _vp, i32, _vp, _vp, _vp, C.c_float, _vp, _vp, i64, i64, _vp]),
        "scp_gather_rows": (C.c_int, [_vp, i64, _vp, i32, _vp, i64, i64, _vp]),
        "scp_linear_f32": (C.c_int, [_vp, i64, _vp, _vp, _vp, i64, i32, i32, i32, i32, _vp]),
        "scp_softmax_cdf": (C.c_int, [_vp, i64, i64, i32, _vp, _vp, _vp, _vp, _vp]),
        "scp_pmf_cdf": (C.c_int, [_vp, i64, i32, _vp, _vp, _vp, _vp]),
        "scp_rate_workspace_bytes": (C.c_int64, [i64, i32]),
        "scp_rate_segments": (C.c_int, [_vp, i64, i64, i32, _vp, _vp, _vp, i32, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_temper_workspace_bytes": (C.c_int64, [i64, i32, i32]),
        "scp_temper_sweep": (C.c_int, [_vp, i64, i64, i32, _vp, _vp, i32, _vp, i32, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_temper_choose": (C.c_int, [_vp, _vp, _vp, i64, _vp, i32, i32, _vp, i32, i32, C.c_double, _vp, _vp, _vp, _vp]),
        "scp_scale_rows": (C.c_int, [_vp, i64, _vp, i64, i64, i32, _vp, _vp, i32, _vp]),
        "scp_ringlod_workspace_bytes": (C.c_int64, [i32, i32]),
        "scp_ringlod_cells": (C.c_int, [_vp, i64, i32, _vp, _vp, i32, _vp, _vp, i32, i32, _vp, _vp, _vp, i64, _vp]),
        "scp_force_rows": (C.c_int, [_vp, i64, i64, i32, _vp, _vp, _vp, _vp]),
        "scp_nn_error_split_f64": (C.c_int, [_vp, i64, _vp, i64, _vp, _vp, i32, _vp, i32, _vp, _vp, _vp, _vp, _vp, _vp]),
        "scp_dist_segments_f64": (C.c_int, [_vp, _vp, _vp, _vp, i64, _vp, i32, _vp, _vp]),
        "scp_rate_leaf_share_workspace_bytes": (C.c_int64, [i64, i32]),
        "scp_rate_leaf_share": (C.c_int, [_vp, _vp, _vp, i64, _vp, _vp, _vp, i32, i64, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_ring_bins_f64": (C.c_int, [_vp, i64, _vp, _vp, i32, _vp, i32, _vp, _vp, _vp]),
        "scp_share_segments_f64": (C.c_int, [_vp, _vp, _vp, i64, _vp, i32, _vp, _vp]),
        "scp_rate_depth_share_workspace_bytes": (C.c_int64, [i64, i32]),
        "scp_rate_depth_share": (C.c_int, [_vp, _vp, _vp, i64, _vp, _vp, _vp, i32, i64, i32, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_share_segments_depth_f64": (C.c_int, [_vp, _vp, _vp, i64, _vp, i32, i32, i64, _vp, _vp]),
        "scp_ac_encode_cdf": (C.c_int, [_vp, _vp, i64, i32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "scp_ac_encode_lohi": (C.c_int, [_vp, i64, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "scp_ac_dec_new": (C.c_int, [C.POINTER(_vp), _vp, C.c_size_t, i32]),
        "scp_ac_dec_next": (C.c_int, [_vp, _vp]),
        "scp_ac_dec_run": (C.c_int, [_vp, _vp, i64, _vp]),
        "scp_ac_dec_free": (C.c_int, [_vp]),
        "scp_ac_dec_run_ctx": (C.c_int, [_vp, _vp, i32, _vp, i64, _vp]),
        "scp_attr_leaf_values_workspace_bytes": (C.c_int64, [i64]),
        "scp_attr_forward_workspace_bytes": (C.c_int64, [i64, i32]),
        "scp_attr_inverse_workspace_bytes": (C.c_int64, [i64, i32]),
        "scp_attr_leaf_values": (C.c_int, [_vp, _vp, i64, _vp, i64, i32, i32, _vp, _vp, _vp, i64, _vp]),
        "scp_attr_forward": (C.c_int, [_vp, _vp, i64, i32, i32, _vp, _vp, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_attr_inverse": (C.c_int, [_vp, i64, i32, i32, i32, _vp, _vp, _vp, i64, _vp]),
        "scp_attr_level_counts": (C.c_int, [_vp, i64, i32, _vp, _vp, i64, _vp]),
        "scp_attr_pairs": (C.c_int, [_vp, _vp, i64, _vp, i32, _vp, _vp]),
        "scp_color_leaf_values_workspace_bytes": (C.c_int64, [i64]),
        "scp_color_forward_workspace_bytes": (C.c_int64, [i64, i32]),
        "scp_color_inverse_workspace_bytes": (C.c_int64, [i64, i32]),
        "scp_color_leaf_values": (C.c_int, [_vp, _vp, i64, _vp, i64, i32, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_color_forward": (C.c_int, [_vp, _vp, i64, i32, i32, _vp, _vp, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_color_inverse": (C.c_int, [_vp, i64, i32, i32, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_color_pairs": (C.c_int, [_vp, _vp, i64, _vp, i32, _vp, _vp]),
        "scp_attr_sweep_workspace_bytes": (C.c_int64, [i64, i32, i32]),
        "scp_color_sweep_workspace_bytes": (C.c_int64, [i64, i32, i32]),
        "scp_attr_sweep": (C.c_int, [_vp, _vp, i64, i32, _vp, i32, _vp, _vp, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_color_sweep": (C.c_int, [_vp, _vp, _vp, i64, i32, _vp, i32, _vp, _vp, _vp, _vp, _vp, _vp, i64, _vp]),
        "scp_ac_chunks_workspace_bytes": (C.c_int64, [i64, i64]),
        "scp_ac_chunks_encode_lohi": (C.c_int, [_vp, i64, i64, _vp, _vp, i64, _vp, _vp, i64, _vp]),
        "scp_ac_chunks_decode_ctx": (C.c_int, [_vp, _vp, i64, i64, _vp, i32, i32, _vp, i32, _vp, _vp, _vp]),
    }
    for name, (res, args) in sig.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
    if L.scp_version() != ABI_VERSION:
        raise ScpError(f"{LIB_PATH} implements ABI {L.scp_version()}, this binding is written for {ABI_VERSION} (include/scp.h: "
                       "SCP_ABI_VERSION; the weight-plane layout differs between versions): rebuild with `python scp_amd/build.py`")
    _lib = L
    return L


def _check(rc, what):
    if rc < 0:
        extra = f" (hipError {lib().scp_last_hip_error()})" if rc == -4 else ""
        raise ScpError(f"{what} failed: {_ERR.get(rc, rc)}{extra}")
    return rc


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The calling thread's current HIP stream as an integer handle.  torch.cuda.current_stream() builds a Stream object through four
    Python frames - 8 us per call, 71 ms per decoded frame (8 900 launches); the raw accessor takes 0.3 us."""
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return _RAW_STREAM(_RAW_DEVICE())
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype=None):
    if not t.is_cuda:
        raise ScpError("device tensor expected (the SCP hot path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise ScpError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ScpError("contiguous tensor expected")
    return t.data_ptr()


def _opt(t):
    return None if t is None else _dev(t)


# ------------------------------------------------------------------------------------------------- launch brackets (scp_debug.h)
PROF_TAGS = {1: "post_attn", 2: "ln_linear", 3: "attention", 4: "knn_feat", 5: "knn_pos", 6: "gemm_split", 7: "edge_mlp", 8: "merge",
             9: "edge_gather", 10: "cdf", 11: "gemm_f32", 12: "gemm_rows", 13: "split_rows", 14: "layernorm", 15: "oa_attention", 16: "geom",
             17: "other", 18: "mlp3", 19: "rate"}


class launch_profile:
    """`with native.launch_profile() as p: ...` - while inside, every bracketed C-ABI launch records a hipEvent pair around its kernel
    (include/scp_debug.h: scp_prof_*; the events are recorded in C next to the launch, no Python between them).  `p.records()` waits for
    the launches and returns [(tag name, milliseconds, algorithmic work)] in launch order.  A measurement hook, not a product path."""

    def __enter__(self):
        _check(lib().scp_prof_enable(1), "scp_prof_enable")
        return self

    def __exit__(self, *exc):
        lib().scp_prof_enable(0)
        return False

    def records(self):
        n = _check(lib().scp_prof_count(), "scp_prof_count")
        tags, ms, work = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float64)
        if n:
            n = _check(lib().scp_prof_read(n, tags.ctypes.data, ms.ctypes.data, work.ctypes.data), "scp_prof_read")
        return [(PROF_TAGS.get(int(t), str(int(t))), float(m), float(w)) for t, m, w in zip(tags[:n], ms[:n], work[:n])]


# ------------------------------------------------------------------------------------------------- stage G1
def quantize(xyz, mode, qs, cart_offset=-200.0, want_transformed=False):
    """xyz cuda float32 [n,3] -> (q cuda int32 [n,3], QuantInfo, transformed or None)."""
    n = xyz.shape[0]
    q = torch.empty((n, 3), dtype=torch.int32, device=xyz.device)
    tr = torch.empty((n, 3), dtype=torch.float32, device=xyz.device) if want_transformed else None
    info = QuantInfo()
    rc = lib().scp_quantize(_dev(xyz, torch.float32), n, mode, float(qs), float(cart_offset), _dev(q), _opt(tr),
                            C.byref(info), _stream())
    _check(rc, "scp_quantize")
    return q, info, tr


# ------------------------------------------------------------------------------------------------- stage G2/G3
class Geom:
    """Owns one scp_geom workspace (reusable across frames)."""

    def __init__(self):
        self._h = _vp()
        _check(lib().scp_geom_create(C.byref(self._h)), "scp_geom_create")
        self.info = []
        self.device = None

    def close(self):
        if self._h:
            lib().scp_geom_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build(self, q, segments):
        """q cuda int32 [n,3]; segments: list of (begin, count, path(list of bits) or None, drop_last)."""
        nseg = len(segments)
        segs = (Segment * nseg)()
        for i, (b, c, path, drop) in enumerate(segments):
            path = list(path or [])
            bits = 0
            for p in path:
                bits = (bits << 1) | int(p)
            segs[i] = Segment(int(b), int(c), len(path), bits, int(bool(drop)), 0)
        infos = (SegmentInfo * nseg)()
        rc = lib().scp_geom_build(self._h, _dev(q, torch.int32), q.shape[0], segs, nseg, infos, _stream())
        _check(rc, "scp_geom_build")
        self.info = list(infos)
        self.segments = segments
        self.device = q.device
        self.total_nodes = sum(i.n_nodes for i in self.info)
        return self.info

    def build_xyz(self, frames, mode, qs_list, cart_offset, shells, want_q=False):
        """Stage G1 + G2 in one launch sequence (scp_geom_build_xyz): frames = list of cuda float32 [n,3] tensors, shells = list of
        (path bits or None, drop_last) - one tree per (frame, shell), segment index = frame * len(shells) + shell.  Every point is
        transformed once; -> list of QuantInfo per segment (and the int32 [sum n, 3] integers of all segments when want_q)."""
        nf, ns = len(frames), len(shells)
        if len(qs_list) != ns or nf == 0:
            raise ScpError("build_xyz: one step per shell expected")
        ptrs = (C.c_void_p * nf)(*[_dev(f, torch.float32) for f in frames])
        cnt = (C.c_int64 * nf)(*[int(f.shape[0]) for f in frames])
        qs = (C.c_double * ns)(*[float(q) for q in qs_list])
        segs = (Segment * ns)()
        for i, (path, drop) in enumerate(shells):
            path = list(path or [])
            bits = 0
            for p in path:
                bits = (bits << 1) | int(p)
            segs[i] = Segment(0, 0, len(path), bits, int(bool(drop)), 0)
        nseg = nf * ns
        qinfo, infos = (QuantInfo * nseg)(), (SegmentInfo * nseg)()
        q = torch.empty((sum(int(f.shape[0]) for f in frames) * ns, 3), dtype=torch.int32, device=frames[0].device) if want_q else None
        rc = lib().scp_geom_build_xyz(self._h, ptrs, cnt, nf, mode, qs, ns, float(cart_offset), segs, _opt(q), qinfo, infos, _stream())
        _check(rc, "scp_geom_build_xyz")
        self.info = list(infos)
        self.segments = [(0, int(f.shape[0]), path, drop) for f in frames for (path, drop) in shells]
        self.device = frames[0].device
        self.total_nodes = sum(i.n_nodes for i in self.info)
        return (list(qinfo), q) if want_q else list(qinfo)

    def context_ehem_all(self, pos_mode, lidar_level, context_size):
        """Context tables of EVERY segment of the last build in one launch, rows back to back: -> (ctx u8 [R,12], pos f32 [R,3], the coded
        symbols IN CODING ORDER u8 [R], (min, max) per level int64 [sum of depths, 2])."""
        R = sum(self.rows(s) for s in range(len(self.info)))
        dev = self.device
        ctx = torch.empty((R, 12), dtype=torch.uint8, device=dev)
        pos = torch.empty((R, 3), dtype=torch.float32, device=dev)
        sym = torch.empty(R, dtype=torch.uint8, device=dev)
        mm = torch.empty((sum(i.depth for i in self.info), 2), dtype=torch.int64, device=dev)
        _check(lib().scp_geom_context_ehem_all(self._h, pos_mode, lidar_level, context_size, _dev(ctx), _dev(pos), _dev(sym), _dev(mm), _stream()),
               "scp_geom_context_ehem_all")
        return ctx, pos, sym, mm

    def level_counts(self, seg):
        i = self.info[seg]
        return [int(i.level_count[l]) for l in range(i.depth)]

    def nodes(self, want=("occ", "level", "octant", "parent", "pos")):
        N, dev = self.total_nodes, self.device
        out = {}
        if "occ" in want:
            out["occ"] = torch.empty(N, dtype=torch.uint8, device=dev)
        if "level" in want:
            out["level"] = torch.empty(N, dtype=torch.uint8, device=dev)
        if "octant" in want:
            out["octant"] = torch.empty(N, dtype=torch.uint8, device=dev)
        if "parent" in want:
            out["parent"] = torch.empty(N, dtype=torch.int32, device=dev)
        if "pos" in want:
            out["pos"] = torch.empty((N, 3), dtype=torch.int32, device=dev)
        rc = lib().scp_geom_emit_nodes(self._h, _opt(out.get("occ")), _opt(out.get("level")), _opt(out.get("octant")),
                                       _opt(out.get("parent")), _opt(out.get("pos")), _stream())
        _check(rc, "scp_geom_emit_nodes")
        return out

    def leaves(self, seg):
        pts = torch.empty((self.info[seg].n_leaves, 3), dtype=torch.int32, device=self.device)
        _check(lib().scp_geom_emit_leaves(self._h, seg, _dev(pts), _stream()), "scp_geom_emit_leaves")
        return pts

    def rows(self, seg):
        return int(self.info[seg].n_nodes) - int(bool(self.segments[seg][3]))

    def krecords(self, seg):
        out = torch.empty((self.rows(seg), 4, 6), dtype=torch.int64, device=self.device)
        _check(lib().scp_geom_krecords_i64(self._h, seg, _dev(out), _stream()), "scp_geom_krecords_i64")
        return out

    def context_ehem(self, seg, pos_mode, lidar_level):
        r, dev = self.rows(seg), self.device
        ctx = torch.empty((r, 12), dtype=torch.uint8, device=dev)
        pos = torch.empty((r, 3), dtype=torch.float32, device=dev)
        sym = torch.empty(r, dtype=torch.uint8, device=dev)
        mm = torch.empty((self.info[seg].depth, 2), dtype=torch.int64, device=dev)
        rc = lib().scp_geom_context_ehem(self._h, seg, pos_mode, lidar_level, _dev(ctx), _dev(pos), _dev(sym), _dev(mm),
                                         _stream())
        _check(rc, "scp_geom_context_ehem")
        return ctx, pos, sym, mm

    def context_octattn(self, seg):
        r, dev = self.rows(seg), self.device
        ctx = torch.empty((r, 12), dtype=torch.uint8, device=dev)
        pos = torch.empty((r, 4, 3), dtype=torch.float32, device=dev)
        sym = torch.empty(r, dtype=torch.uint8, device=dev)
        _check(lib().scp_geom_context_octattn(self._h, seg, _dev(ctx), _dev(pos), _dev(sym), _stream()),
               "scp_geom_context_octattn")
        return ctx, pos, sym


# ------------------------------------------------------------------------------------------------- stage M
def knn_topk(x, k):
    """x cuda f32 [B,n,C] -> idx int32 [B,n,k]."""
    B, n, Cc = x.shape
    idx = torch.empty((B, n, k), dtype=torch.int32, device=x.device)
    _check(lib().scp_knn_topk(_dev(x, torch.float32), B, n, Cc, k, _dev(idx), _stream()), "scp_knn_topk")
    return idx


def knn_topk_packed(x, ctab, thr0=None):
    """x cuda f32 [T,C] (T % 512 == 0), ctab cuda int32 [T/512, 2] = (sequence base row, real length) -> idx int32 [T,20] global.
    thr0: optional f32 [T] a-priori pruning bound per row (a value of 2 x.y - |x|^2 - |y|^2 that >= 20 candidates reach)."""
    T, Cc = x.shape
    idx = torch.zeros((T, 20), dtype=torch.int32, device=x.device)
    if thr0 is None:
        _check(lib().scp_knn_topk_packed(_dev(x, torch.float32), _dev(ctab, torch.int32), T, Cc, _dev(idx), _stream()), "scp_knn_topk_packed")
    else:
        _check(lib().scp_knn_topk_packed_bounded(_dev(x, torch.float32), _dev(ctab, torch.int32), T, Cc, _dev(thr0, torch.float32), _dev(idx),
                                                 _stream()), "scp_knn_topk_packed_bounded")
    return idx


def swin_attention_packed(q, k, v, bias_table, wtab, shift, split=False):
    """q,k,v cuda f32 [T,256] views (unit channel stride), wtab int32 [T/512, 2] = (sequence base row, padded length).
    split=True returns the output as a SplitAct (operand of linear_split) instead of fp32."""
    T = q.shape[0]
    if split:
        o = SplitAct.empty(T, 256, q.device)
        rc = lib().scp_swin_attention_packed_split(q.data_ptr(), k.data_ptr(), v.data_ptr(), _dev(bias_table, torch.float32),
                                                   _dev(wtab, torch.int32), T // 512, shift, q.stride(0), k.stride(0), o.t[0].data_ptr(),
                                                   o.t[1].data_ptr(), o.t.stride(1), _stream())
        _check(rc, "scp_swin_attention_packed_split")
        return o
    out = torch.empty((T, 256), dtype=torch.float32, device=q.device)
    rc = lib().scp_swin_attention_packed(q.data_ptr(), k.data_ptr(), v.data_ptr(), _dev(bias_table, torch.float32),
                                         _dev(wtab, torch.int32), T // 512, shift, q.stride(0), k.stride(0), _dev(out), _stream())
    _check(rc, "scp_swin_attention_packed")
    return out


class KvPlanes:
    """k, v fp32 [T, 256] views (T % 512 == 0 rows of the packed layout) as the bf16 hi / lo planes of the plane-fed window attention
    (csrc/attn.hip: swin_attn_planes_kernel): K [T, 256] with swizzled 16-byte chunks, V^T per (32-token block, head) as the linear image
    of the kernel's LDS tile.  `t`: bfloat16 [4, T, 256] = K hi, K lo, V^T hi, V^T lo."""

    __slots__ = ("t",)

    def __init__(self, k=None, v=None, t=None):
        if t is None:
            T = k.shape[0]
            t = torch.empty((4, T, 256), dtype=torch.bfloat16, device=k.device)
            _check(lib().scp_swin_kv_planes(k.data_ptr(), v.data_ptr(), k.stride(0), T, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                            t[3].data_ptr(), _stream()), "scp_swin_kv_planes")
        self.t = t


# How the attention output travels to swin_post_attn: "frag" (default) = planes in the fragment order of the post-attention kernels
# (include/scp.h: SCP_LDO_FRAG), "rows" = row-major planes (SCP_ATTN_O=rows; tests and A/B measurements - identical bits either way).
_ATTN_O = "rows" if os.environ.get("SCP_ATTN_O", "")[:1] == "r" else "frag"
LDO_FRAG = 0


def set_attn_o(mode):
    """Select the hand-over of the attention output ("frag" / "rows"); returns the previous mode (tests, A/B)."""
    global _ATTN_O
    if mode not in ("frag", "rows"):
        raise ScpError("attention output hand-over: 'frag' or 'rows'")
    prev, _ATTN_O = _ATTN_O, mode
    return prev


def attn_o_split():
    """The `split` argument of swin_attention_packed_planes for the hand-over in force: "frag", or True (rows)."""
    return "frag" if _ATTN_O == "frag" else True


class FragAct:
    """The attention output [M, 256] as bf16 hi / lo planes in the FRAGMENT ORDER of the post-attention kernels (csrc/rowchain.hip): per
    128-row tile and plane [32 chunks of 8 channels][128 rows][8].  `t`: bfloat16 [2, ceil(M / 128), 32, 128, 8]."""

    __slots__ = ("t", "M", "K")

    def __init__(self, t, M):
        self.t, self.M, self.K = t, M, 256

    @staticmethod
    def empty(M, device):
        return FragAct(torch.empty((2, -(-M // 128), 32, 128, 8), dtype=torch.bfloat16, device=device), M)

    @staticmethod
    def from_rows(a):
        """SplitAct [M, 256] -> the same values in fragment order (rows behind M in the last tile: zero)."""
        M = a.M
        nt = -(-M // 128)
        r = torch.zeros((2, nt * 128, 256), dtype=torch.bfloat16, device=a.t.device)
        r[:, :M] = a.t[:, :, :256]
        return FragAct(r.view(2, nt, 128, 32, 8).permute(0, 1, 3, 2, 4).contiguous(), M)

    def rows(self):
        """-> SplitAct [M, 256]: the planes un-permuted (element for element)."""
        nt = self.t.shape[1]
        return SplitAct(self.t.permute(0, 1, 3, 2, 4).reshape(2, nt * 128, 256)[:, :self.M].contiguous(), 256)

    def float(self):
        return self.rows().float()


def swin_attention_packed_planes(q, kv, bias_table, wtab, shift, split=False, valid=None):
    """swin_attention_packed with K / V as KvPlanes: operands staged by LDS-DMA, no conversion in the kernel; identical bits.
    valid (fp32 [T] / [T, 1], optional): query tiles of nothing but window padding are skipped, their output rows stay unwritten.
    split=True: the output as a SplitAct (row-major planes); split="frag": as a FragAct - the hand-over to swin_post_attn (the same values)."""
    T = q.shape[0]
    p = kv.t
    vp = None if valid is None else _dev(valid, torch.float32)
    if isinstance(split, str):
        if split != "frag":
            raise ScpError("swin_attention_packed_planes: split is False, True or 'frag'")
        o = FragAct.empty(T, q.device)
        rc = lib().scp_swin_attention_packed_planes(q.data_ptr(), p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(),
                                                    _dev(bias_table, torch.float32), _dev(wtab, torch.int32), T // 512, shift, q.stride(0), None,
                                                    o.t[0].data_ptr(), o.t[1].data_ptr(), LDO_FRAG, vp, _stream())
        _check(rc, "scp_swin_attention_packed_planes")
        return o
    if split:
        o = SplitAct.empty(T, 256, q.device)
        rc = lib().scp_swin_attention_packed_planes(q.data_ptr(), p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(),
                                                    _dev(bias_table, torch.float32), _dev(wtab, torch.int32), T // 512, shift, q.stride(0), None,
                                                    o.t[0].data_ptr(), o.t[1].data_ptr(), o.t.stride(1), vp, _stream())
        _check(rc, "scp_swin_attention_packed_planes")
        return o
    out = torch.empty((T, 256), dtype=torch.float32, device=q.device)
    rc = lib().scp_swin_attention_packed_planes(q.data_ptr(), p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(),
                                                _dev(bias_table, torch.float32), _dev(wtab, torch.int32), T // 512, shift, q.stride(0), _dev(out), None,
                                                None, 0, vp, _stream())
    _check(rc, "scp_swin_attention_packed_planes")
    return out


def nn_sqdist(a, b):
    """a [na,3], b [nb,3] float64 device tensors -> float64 [na]: squared distance of every a to its nearest b (exhaustive)."""
    a = _dev_f64(a)
    b = _dev_f64(b)
    out = torch.empty((a.shape[0],), dtype=torch.float64, device=a.device)
    _check(lib().scp_nn_sqdist_f64(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], out.data_ptr(), _stream()), "scp_nn_sqdist_f64")
    return out


def _dev_f64(t):
    if not t.is_cuda:
        raise ScpError("device tensor required (there is no CPU path in the product)")
    return t.to(torch.float64).contiguous()


TIE_MEAN_NORMAL, TIE_PLANE_ERROR = 0, 1     # include/scp.h: SCP_TIE_*


def estimate_normals(xyz, radius=1.0, max_nn=30, view=(0.0, 0.0, 0.0), want_idx=False):
    """xyz [n,3] device tensor -> (normals float64 [n,3], count int32 [n], idx int32 [n,max_nn] or None): scp_estimate_normals_f64."""
    x = _dev_f64(xyz)
    n = x.shape[0]
    normals = torch.empty((n, 3), dtype=torch.float64, device=x.device)
    count = torch.empty((n,), dtype=torch.int32, device=x.device)
    idx = torch.empty((n, int(max_nn)), dtype=torch.int32, device=x.device) if want_idx else None
    v = (C.c_double * 3)(*[float(c) for c in view])
    _check(lib().scp_estimate_normals_f64(x.data_ptr(), n, float(radius), int(max_nn), C.cast(v, _vp), normals.data_ptr(), count.data_ptr(),
                                          None if idx is None else idx.data_ptr(), _stream()), "scp_estimate_normals_f64")
    return normals, count, idx


def nn_tieset(mode, q, p, dmin, nrm):
    """scp_nn_tieset_f64 on float64 device tensors.  TIE_MEAN_NORMAL: dmin [np], nrm [np,3] of the streamed cloud p -> [nq,3];
    TIE_PLANE_ERROR: dmin [nq] of the queries, nrm [np,3] of p -> [nq]."""
    q, p, dmin, nrm = _dev_f64(q), _dev_f64(p), _dev_f64(dmin), _dev_f64(nrm)
    nq, np_ = q.shape[0], p.shape[0]
    if nrm.shape != (np_, 3) or dmin.shape != ((np_,) if mode == TIE_MEAN_NORMAL else (nq,)):
        raise ScpError(f"nn_tieset: dmin {tuple(dmin.shape)} / normals {tuple(nrm.shape)} do not fit {nq} queries against {np_} points")
    out = torch.empty((nq, 3) if mode == TIE_MEAN_NORMAL else (nq,), dtype=torch.float64, device=q.device)
    _check(lib().scp_nn_tieset_f64(int(mode), q.data_ptr(), nq, p.data_ptr(), np_, dmin.data_ptr(), nrm.data_ptr(), out.data_ptr(), _stream()),
           "scp_nn_tieset_f64")
    return out


def embed_gather(ctx, pos, inmap, occ_enc, level_enc, octant_enc):
    """ctx uint8 [T,12], pos f32 [T,3], inmap int64 [rows] -> (x f32 [rows,80], pos f32 [rows,3], occ_self int64 [rows])."""
    rows = inmap.shape[0]
    dev = ctx.device
    x = torch.empty((rows, 80), dtype=torch.float32, device=dev)
    p = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    o = torch.empty((rows,), dtype=torch.int64, device=dev)
    _check(lib().scp_embed_gather(_dev(ctx, torch.uint8), _dev(pos, torch.float32), _dev(inmap, torch.int64), ctx.shape[0], _dev(occ_enc),
                                  _dev(level_enc), _dev(octant_enc), x.data_ptr(), p.data_ptr(), o.data_ptr(), rows, _stream()),
           "scp_embed_gather")
    return x, p, o


_POPC = {}


def decode_expand(sym, pos, anc, octant, L, shift, lv_next, lv_clamp, polar, mn, den):
    """Decoder: children of one decoded level + the next level's model inputs, one launch (csrc/plan.hip: scp_decode_expand).
    sym int64 [n] (-1 = unknown), pos int32 [n,3], anc uint8 [n,9], octant uint8 [n] ->
    (occ8 uint8 [n], cpos int32 [m,3], canc uint8 [m,9], coct uint8 [m], cctx uint8 [m,12], cposn float32 [m,3]); one host sync (m)."""
    dev, n = sym.device, sym.shape[0]
    tab = popcount_table(dev)
    cum = torch.cumsum(tab[sym + 1], 0)
    m = int(cum[-1])
    occ8 = torch.empty(n, dtype=torch.uint8, device=dev)
    cpos = torch.empty((m, 3), dtype=torch.int32, device=dev)
    canc = torch.empty((m, 9), dtype=torch.uint8, device=dev)
    coct = torch.empty(m, dtype=torch.uint8, device=dev)
    cctx = torch.empty((m, 12), dtype=torch.uint8, device=dev)
    cposn = torch.empty((m, 3), dtype=torch.float32, device=dev)
    if m == 0:
        # no parent has a child (a multi-level shell whose last level holds only the dropped node): the C entry rejects the null
        # pointers of empty outputs, and there is nothing to launch - the occupancy bytes of unknown symbols are 0
        return (sym + 1).clamp_(min=0).to(torch.uint8), cpos, canc, coct, cctx, cposn
    _check(lib().scp_decode_expand(_dev(sym, torch.int64), cum.data_ptr(), _dev(pos, torch.int32), _dev(anc, torch.uint8), _dev(octant, torch.uint8), n,
                                   int(L), int(shift), int(lv_next), int(lv_clamp), 1 if polar else 0, float(mn), float(den), cpos.data_ptr(), canc.data_ptr(),
                                   coct.data_ptr(), cctx.data_ptr(), cposn.data_ptr(), occ8.data_ptr(), _stream()), "scp_decode_expand")
    return occ8, cpos, canc, coct, cctx, cposn


# include/scp.h: scp_expand_seg, as a numpy record (one row per segment of scp_decode_expand_batch)
EXPAND_SEG = np.dtype([("first", np.int64), ("count", np.int64), ("cfirst", np.int64), ("coded", np.int64), ("L", np.int32), ("shift", np.int32),
                       ("lv_next", np.int32), ("lv_clamp", np.int32), ("polar", np.int32), ("reserved", np.int32), ("mn", np.float64),
                       ("den", np.float64)])


def popcount_table(dev):
    """int64 [256] on `dev`: the set bits of every occupancy code (cached)."""
    tab = _POPC.get(dev)
    if tab is None:
        tab = _POPC[dev] = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device=dev)
    return tab


def decode_expand_batch(sym, pos, anc, octant, cum, seg, cs, wbase, M, T):
    """Lockstep decoder: the decoded levels of S <= 64 streams expanded in ONE launch (csrc/plan.hip: scp_decode_expand_batch).  The
    parents of the streams lie segment after segment in sym int64 [n] (-1 = unknown), pos int32 [n,3], anc uint8 [n,9], octant uint8 [n];
    cum int64 [n] = the inclusive scan of popcount(sym + 1) over the whole array; seg: EXPAND_SEG records [S] (host); wbase int64 [K,S]
    (host): first input row of window k of segment s, -1 = none; M = children in all, T = input rows in all.  ->
    (occ8 uint8 [n], cpos int32 [M,3], canc uint8 [M,9], coct uint8 [M] with segment s at rows cfirst[s].., cctx uint8 [T,12],
    cposn float32 [T,3] with child c < coded[s] of segment s at row wbase[c // cs, s] + c % cs).  Asynchronous: the tables go up in one
    copy out of pinned memory on the current stream, nothing is awaited."""
    dev, n = sym.device, sym.shape[0]
    seg = np.ascontiguousarray(seg, EXPAND_SEG)
    wbase = np.ascontiguousarray(wbase, np.int64)
    if wbase.ndim != 2 or wbase.shape[1] != seg.shape[0]:
        raise ScpError("decode_expand_batch: wbase must be [K, S]")
    S, K, M, T = int(seg.shape[0]), int(wbase.shape[0]), int(M), int(T)
    if cum.shape[0] != n or cum.dtype != torch.int64:
        raise ScpError("decode_expand_batch: cum must be the int64 scan of the parents")
    cpos = torch.empty((M, 3), dtype=torch.int32, device=dev)
    canc = torch.empty((M, 9), dtype=torch.uint8, device=dev)
    coct = torch.empty(M, dtype=torch.uint8, device=dev)
    cctx = torch.empty((T, 12), dtype=torch.uint8, device=dev)
    cposn = torch.empty((T, 3), dtype=torch.float32, device=dev)
    if M == 0 and n > 0:
        # no parent has a child (every stream sits on a last level that holds only the dropped node): nothing to launch, as in decode_expand
        return (sym + 1).clamp_(min=0).to(torch.uint8), cpos, canc, coct, cctx, cposn
    occ8 = torch.empty(n, dtype=torch.uint8, device=dev)
    host = torch.zeros((64 * EXPAND_SEG.itemsize + 8 * max(K * S, 1),), dtype=torch.uint8, pin_memory=True)
    host[:seg.nbytes] = torch.from_numpy(seg.view(np.uint8))
    host[64 * EXPAND_SEG.itemsize:64 * EXPAND_SEG.itemsize + wbase.nbytes] = torch.from_numpy(wbase.reshape(-1).view(np.uint8))
    scratch = host.to(dev, non_blocking=True)           # (torch keeps the pinned block until the copy has run)
    _check(lib().scp_decode_expand_batch(_dev(sym, torch.int64), cum.data_ptr(), _dev(pos, torch.int32), _dev(anc, torch.uint8), _dev(octant, torch.uint8),
                                         n, seg.ctypes.data, S, int(cs), wbase.ctypes.data, K, M, T, scratch.data_ptr(), cpos.data_ptr(),
                                         canc.data_ptr(), coct.data_ptr(), cctx.data_ptr(), cposn.data_ptr(), occ8.data_ptr(), _stream()),
           "scp_decode_expand_batch")
    return occ8, cpos, canc, coct, cctx, cposn


def packed_plan(lengths, device):
    """All index maps of the packed forward for one list of window lengths, ONE kernel launch (csrc/plan.hip).
    Returns (rows[11], dict of device tensors keyed like models/packed.py: PackedPlan.d)."""
    import numpy as np
    c = np.ascontiguousarray(np.asarray(lengths, np.int64))
    W = int(c.shape[0])
    rows = np.zeros(11, np.int64)
    _check(lib().scp_packed_plan_sizes(c.ctypes.data, W, rows.ctypes.data), "scp_packed_plan_sizes")
    r = [int(x) for x in rows]
    i64, i32, f32 = torch.int64, torch.int32, torch.float32
    spec = [("inmap", i64, (r[0],)), ("a1map", i64, (r[5],)), ("a2map", i64, (r[5],)), ("even_rows", i64, (r[9],)), ("odd_rows", i64, (r[10],)),
            ("even_dst", i64, (r[9],)), ("odd_dst", i64, (r[10],))]
    for s_ in range(4):
        spec += [(f"sme{s_}", i64, (r[s_ + 1],)), (f"smo{s_}", i64, (r[s_ + 1],))]
    for s_ in range(3):
        spec += [(f"cme{s_}", i64, (r[6 + s_],)), (f"cmo{s_}", i64, (r[6 + s_],))]
    spec += [(f"sc{s_}", i64, (r[0],)) for s_ in range(1, 5)] + [(f"cc{s_}", i64, (r[5],)) for s_ in range(1, 4)]
    spec += [(f"tab{l}", i32, (r[l] // 512, 2)) for l in range(9)] + [("knn_tab", i32, (r[0] // 512, 2))]
    spec += [(f"valid{l}", f32, (r[l], 1)) for l in range(9)]
    spec += [(f"sp{s_}", i64, (r[s_],)) for s_ in range(4)] + [(f"cp{s_}", i64, (r[5 + s_],)) for s_ in range(3)]
    spec += [("even_out", i64, (r[5],)), ("odd_out", i64, (r[5],))]
    t = {name: torch.empty(shape, dtype=dt, device=device) for name, dt, shape in spec}
    ptrs = (C.c_void_p * len(spec))(*[t[name].data_ptr() for name, _, _ in spec])
    scratch = torch.empty((36 * W,), dtype=torch.int64, device=device)
    _check(lib().scp_packed_plan(c.ctypes.data, W, scratch.data_ptr(), ptrs, len(spec), _stream()), "scp_packed_plan")
    d = dict(inmap=t["inmap"], a1map=t["a1map"], a2map=t["a2map"], even_rows=t["even_rows"], odd_rows=t["odd_rows"],
             even_dst=t["even_dst"], odd_dst=t["odd_dst"],
             self_merge=[(t[f"sme{s_}"], t[f"smo{s_}"]) for s_ in range(4)], cross_merge=[(t[f"cme{s_}"], t[f"cmo{s_}"]) for s_ in range(3)],
             self_concat=[t[f"sc{s_}"] for s_ in range(1, 5)], cross_concat=[t[f"cc{s_}"] for s_ in range(1, 4)],
             self_tab=[t[f"tab{l}"] for l in range(5)], cross_tab=[t[f"tab{l}"] for l in range(5, 9)], knn_tab=t["knn_tab"],
             self_valid=[t[f"valid{l}"] for l in range(5)], cross_valid=[t[f"valid{l}"] for l in range(5, 9)],
             self_parent=[t[f"sp{s_}"] for s_ in range(4)], cross_parent=[t[f"cp{s_}"] for s_ in range(3)],
             even_out=t["even_out"], odd_out=t["odd_out"])
    d["self_tiles"], d["cross_tiles"] = real_tiles(c, device)
    return r, d


def real_tiles(lengths, device, n_self=5, n_cross=4):
    """Per Swin stage of the packed layout the 128-row tiles that hold at least one real row (int32 device tensors, ascending): host
    arithmetic on the list of window lengths (a window's real rows are a prefix of its 512-aligned run), ONE host -> device copy.  The
    row-chain block kernel walks this list instead of every tile; tiles of nothing but window padding are 4.7 % of an L16-m frame."""
    import numpy as np
    c = np.asarray(lengths, np.int64)
    e = c + (c & 1)

    def lists(L, n):
        out = []
        for _ in range(n):
            Lp = -(-L // 512) * 512
            base = np.cumsum(Lp) - Lp
            nt = -(-L // 128)
            first = np.repeat(base // 128, nt)
            within = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
            out.append((first + within).astype(np.int32))
            L = (L + 1) // 2
        return out
    parts = lists(e, n_self) + lists(e // 2, n_cross)
    flat = torch.from_numpy(np.concatenate(parts)).to(device, non_blocking=True)
    cuts = np.cumsum([0] + [len(p) for p in parts])
    views = [flat[cuts[i]:cuts[i + 1]] for i in range(len(parts))]
    return views[:n_self], views[n_self:]


def edge_gather_max_rows(u, v, idx, scale, shift, out=None):
    """packed form: u, v f32 [n, C'] VIEWS with unit channel stride (any row stride), idx int32 [n, k] -> out f32 [n, C'] (`out`: an [n, C'] view with
    unit channel stride, e.g. the leading columns of the next search's feature buffer: no concatenation afterwards)."""
    n, Co = u.shape
    if out is None:
        out = torch.empty((n, Co), dtype=torch.float32, device=u.device)
    elif out.shape != (n, Co) or out.stride(1) != 1 or out.dtype != torch.float32 or out.stride(0) % 4 or out.data_ptr() % 16:
        raise ScpError("edge_gather_max_rows: out must be a float32 [n, C'] view with unit channel stride and 16-byte aligned rows")
    _check(lib().scp_edge_gather_max_ld(u.data_ptr(), u.stride(0), v.data_ptr(), v.stride(0), _dev(idx, torch.int32), _dev(scale), _dev(shift),
                                        1, n, Co, idx.shape[1], out.data_ptr(), out.stride(0), _stream()), "scp_edge_gather_max_ld")
    return out


_MODES = {"knn": "f32" if os.environ.get("SCP_KNN", "")[:1] == "f" else "f16x3",
          "attn": "f32" if os.environ.get("SCP_ATTN", "")[:1] == "f" else "bf16x3"}


def set_knn_mode(f16x3):
    """PROCESS default (test hook, include/scp_debug.h; an encoder uses a NumericProfile): True = f16x3 distances for the 144-/192-feature
    searches, False = exact fp32 MFMA chain."""
    _check(lib().scp_set_knn_mode(1 if f16x3 else 0), "scp_set_knn_mode")
    _MODES["knn"] = "f16x3" if f16x3 else "f32"


def set_knn_workgroup(shape):
    """256 (default): 256-query workgroups on the XCD-affine schedule, a barrier per group of tiles; 257 / 258: smaller groups; +16: outward
    sweep; 128: the 128-query kernel.  Same results."""
    _check(lib().scp_set_knn_workgroup(int(shape)), "scp_set_knn_workgroup")


class NumericProfile:
    """The numeric profile of ONE encoder / decoder (an scp_ctx of include/scp.h): which arithmetic the kernels with a choice use -
    feature kNN searches f16x3 (default) or the exact fp32 chain, window attention bf16x3 (default) or fp32 MFMA.  It belongs to the
    handle, not to the process: FrameEncoder / FrameDecoder make theirs current (for the calling thread) around their launches, so two
    encoders with different profiles in one process, or in different threads, each get their own arithmetic and their own streams."""

    def __init__(self, knn_f16x3=True, attention_bf16x3=True):
        self._h = _vp()
        _check(lib().scp_ctx_create(C.byref(self._h)), "scp_ctx_create")
        self.knn_f16x3, self.attention_bf16x3 = bool(knn_f16x3), bool(attention_bf16x3)
        _check(lib().scp_ctx_set(self._h, 1, int(self.knn_f16x3)), "scp_ctx_set")
        _check(lib().scp_ctx_set(self._h, 2, int(self.attention_bf16x3)), "scp_ctx_set")

    def describe(self, model_name):
        return numeric_profile(model_name, self)

    def __del__(self):
        # a profile that is current somewhere is referenced by that `use_profile` object, so this only runs for profiles nobody uses
        try:
            if self._h:
                lib().scp_ctx_destroy(self._h)
        except Exception:
            pass


_TLS = __import__("threading").local()


def current_profile():
    """The NumericProfile current for this thread (None = the process default)."""
    return getattr(_TLS, "profile", None)


class use_profile:
    """`with native.use_profile(p):` - p (a NumericProfile or None) is the calling thread's current profile inside the block."""

    def __init__(self, profile):
        self.profile = profile

    def __enter__(self):
        self.prev = current_profile()
        _check(lib().scp_ctx_make_current(self.profile._h if self.profile is not None else None), "scp_ctx_make_current")
        _TLS.profile = self.profile           # only once the C side has switched: the two thread-local views never disagree
        return self.profile

    def __exit__(self, *exc):
        lib().scp_ctx_make_current(self.prev._h if self.prev is not None else None)
        _TLS.profile = self.prev
        return False


def attention_bf16x3():
    """Whether the window attention of the calling thread runs its bf16x3 form (its current profile, or the process default)."""
    p = current_profile()
    return (_MODES["attn"] == "bf16x3") if p is None else p.attention_bf16x3


def numeric_profile(model_name, profile="current", decodable=False):
    """The arithmetic variants that decide the logits' last bits - hence the integer CDFs a decoder must reproduce - as a string.  The
    encoder writes it into its side-info file and the decoder refuses a stream coded under another profile.  `profile`: a
    NumericProfile, None (process default) or "current" (this thread's).  The remaining fields are constants since round 4 (the
    superseded launch forms they once named are gone).  The generation prefix (ehem/N) moves whenever a kernel's last bits do, and the
    decoder compares the whole string: streams of an older generation are refused by design, not decoded to garbage."""
    from . import ops
    from .models import packed
    if model_name == "OctAttention":
        if decodable:
            # octattn/1d: the decodable profile (models/oct_attention.py, decodable=True) - every logits row a function of its own window's
            # rows 0..t only: the row-invariant fp32 attention (csrc/octattn_rowinv.hip), no launch-global V scale
            return f"octattn/1d:gemm={ops.MODE},attn=rowinv32"
        return f"octattn/1:gemm={ops.MODE},attn={OCTATTN_MODE}"
    if profile == "current":
        profile = current_profile()
    knn = _MODES["knn"] if profile is None else ("f16x3" if profile.knn_f16x3 else "f32")
    attn = _MODES["attn"] if profile is None else ("bf16x3" if profile.attention_bf16x3 else "f32")
    # ehem/3: patch merging and the geometry generator's edge MLPs on row-chain kernels (other last bits than ehem/2)
    # ehem/4: the bf16x3 attention sweeps against the fixed reference 0 with the bias as the products' start value (csrc/attn.hip: attn_tile)
    # ehem/5: GELU as max(y, 0) - |y| exp(-beta y^2) / P4(|y|) (csrc/scp_internal.h) instead of the degree-12 erf polynomial
    # ehem/6: stages 0 and 1 of the layers over concat_states in one launch (the stage-1 product starts the accumulators: gemm_hier2_kernel), the two
    #         256-wide heads as one row-chain launch each (bias as the accumulators' start value: rc_mlp3_kernel)
    L = lib()
    attnv = "" if L.scp_get_attention_variant() == 1 else f",attnv={L.scp_get_attention_variant()}"     # process-wide test bracket (scp_debug.h)
    concat = ("hier2" if packed.FUSE2 else "hier") if packed.HIER else "direct"
    heads = "" if packed.CHAIN_HEADS else ",heads=split"
    return f"ehem/6:gemm={ops.MODE},knn={knn},attn={attn},concat={concat},swin=rowchain{heads}{attnv}"


def edge_gather_max(u, v, idx, scale, shift, out=None):
    """u,v [B,n,C'] f32, idx [B,n,k] i32, scale/shift [C'] -> out [B,n,C'] (may be a column slice of a wider tensor)."""
    B, n, Co = u.shape
    k = idx.shape[2]
    if out is None:
        out = torch.empty((B, n, Co), dtype=torch.float32, device=u.device)
    stride = out.stride(1)
    if out.stride(2) != 1 or out.stride(0) != n * stride:
        raise ScpError("edge_gather_max: out must be row-major with unit channel stride")
    rc = lib().scp_edge_gather_max(_dev(u, torch.float32), _dev(v, torch.float32), _dev(idx, torch.int32), _dev(scale),
                                   _dev(shift), B, n, Co, k, out.data_ptr(), stride, _stream())
    _check(rc, "scp_edge_gather_max")
    return out


def set_attention_mode(bf16x3=True):
    """PROCESS default (test hook, include/scp_debug.h; an encoder uses a NumericProfile): True = QK^T / PV as bf16x3 splits on bf16 MFMA,
    False = plain fp32 MFMA."""
    _check(lib().scp_set_attention_mode(1 if bf16x3 else 0), "scp_set_attention_mode")
    _MODES["attn"] = "bf16x3" if bf16x3 else "f32"


def swin_attention(q, k, v, bias_table, shift):
    """q,k,v cuda f32 [B,Lp,256] views (unit channel stride, Lp % 512 == 0), bias_table [1023,4] -> out [B,Lp,256]."""
    B, Lp, _ = q.shape
    for t in (q, k, v):
        if t.stride(2) != 1 or t.stride(0) != Lp * t.stride(1) or not t.is_cuda or t.dtype != torch.float32:
            raise ScpError("swin_attention: operands must be [B,Lp,256] views with unit channel stride")
    if k.stride(1) != v.stride(1):
        raise ScpError("swin_attention: k and v must share a row stride")
    out = torch.empty((B, Lp, 256), dtype=torch.float32, device=q.device)
    rc = lib().scp_swin_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), _dev(bias_table, torch.float32), B, Lp, shift,
                                  q.stride(1), k.stride(1), _dev(out), _stream())
    _check(rc, "scp_swin_attention")
    return out


ACT_NONE, ACT_LEAKY, ACT_GELU, ACT_RELU = 0, 1, 2, 3

# Lazily built device-side caches (split weights, fused parameter tensors) are created on whatever stream is current.  Every
# creation site bumps this counter; FrameEncoder.encode_async synchronises once after a call during which it moved, so that a
# frame enqueued later on ANOTHER stream (lane) never reads a cache entry whose creating kernels are still in flight.
CACHE_FILLS = 0


def note_cache_fill():
    global CACHE_FILLS
    CACHE_FILLS += 1



# SCP_WTILE=0: the dense kernels take row-major weight planes (A/B bracket).  Read ONCE, here - csrc/gemm.hip and gemm_split.hip read
# it once too (a static), so a value changed after the first launch could only make the two sides disagree.
WTILE = os.environ.get("SCP_WTILE", "1")[:1] != "0"


def _tile_in_place_of(hi, lo, Npad, Kpad):
    """The tiled images (scp_tile_weight_bf16) of two row-major 16-bit planes, on the current stream."""
    th, tl = torch.empty_like(hi), torch.empty_like(lo)
    for src, dst in ((hi, th), (lo, tl)):
        _check(lib().scp_tile_weight_bf16(src.data_ptr(), Npad, Kpad, dst.data_ptr(), _stream()), "scp_tile_weight_bf16")
    return th, tl


class SplitWeight:
    """bf16 hi/lo planes of a Linear weight [N,K], zero-padded to [Npad,Kpad], in the layout the dense kernels stream (built once per
    weight, split AND tiled in the constructor - one cache fill, on one stream; the row-major intermediate is not kept).
    `.hi / .lo`: the planes; `.tiled_layout`: whether they are tiled (always, unless SCP_WTILE=0)."""

    def __init__(self, w, tiled=None):
        N, K = w.shape
        self.N, self.K = N, K
        self.Npad, self.Kpad = -(-N // 256) * 256, -(-K // 32) * 32
        self.hi = torch.empty((self.Npad, self.Kpad), dtype=torch.bfloat16, device=w.device)
        self.lo = torch.empty_like(self.hi)
        wc = w.detach().contiguous().float()
        _check(lib().scp_split_weight_bf16(_dev(wc), N, K, self.Npad, self.Kpad, _dev(self.hi), _dev(self.lo), _stream()),
               "scp_split_weight_bf16")
        self.tiled_layout = WTILE if tiled is None else bool(tiled)
        if self.tiled_layout:
            self.hi, self.lo = _tile_in_place_of(self.hi, self.lo, self.Npad, self.Kpad)
        note_cache_fill()

    def tiled(self):
        """(hi, lo) as the dense kernels stream them: tiled (_tile_planes) by default, row-major under SCP_WTILE=0.  A weight built with
        the other layout than the library reads (the `tiled=` override exists for the layout tests) is refused, not multiplied."""
        if self.tiled_layout != WTILE:
            raise ScpError("SplitWeight: planes are %s but the library reads %s planes (SCP_WTILE)" % (
                "tiled" if self.tiled_layout else "row-major", "tiled" if WTILE else "row-major"))
        return (self.hi, self.lo)


def linear_bf16x3(x, sw, bias=None, act=ACT_NONE, residual=None, out=None):
    """x [..., K] fp32 (unit last stride, uniform row stride) -> [..., N]; out may be a column slice of a wider buffer."""
    K, N = sw.K, sw.N
    lead = x.shape[:-1]
    x2 = x.reshape(-1, K) if x.is_contiguous() else x
    if x2.dim() != 2:
        x2 = x.contiguous().reshape(-1, K)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
        o2 = out
    else:
        o2 = out.reshape(-1, N) if out.is_contiguous() else out
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, N) if residual.is_contiguous() else residual.contiguous().reshape(-1, N)
    wt = _tiled_pair(sw)
    rc = lib().scp_linear_bf16x3(x2.data_ptr(), x2.stride(0), wt[0].data_ptr(), wt[1].data_ptr(), sw.Kpad, _opt(bias),
                                 None if r2 is None else r2.data_ptr(), 0 if r2 is None else r2.stride(0), o2.data_ptr(),
                                 o2.stride(0), M, N, K, act, _stream())
    _check(rc, "scp_linear_bf16x3")
    return out.reshape(*lead, N) if out.dim() == 2 and len(lead) != 1 else out


def _tiled_pair(sw):
    if sw.tiled_layout != WTILE:
        raise ScpError("weight planes are not in the layout the library reads (SCP_WTILE)")
    return (sw.hi, sw.lo)


def _tiled_planes_always(sw):
    """(hi, lo) of a SplitWeight in the tiled layout whatever SCP_WTILE says (the row-chain kernels have no row-major mode)."""
    if sw.tiled_layout:
        return sw.hi, sw.lo
    return _tile_in_place_of(sw.hi, sw.lo, sw.Npad, sw.Kpad)


def _tile_planes(t):
    """bf16 plane [Npad, Kpad] -> the tiled layout the LDS-DMA kernels read: block (16-row group rb, 32-element k-slab ks) = 1 KiB =
    the LDS image of one DMA instruction, [r][p][8] with the logical 16-byte chunk p ^ ((r >> 2) & 3) of row r at position p (the
    read swizzle of csrc/gemm_split.hip), blocks ordered [rb][ks]."""
    N, K = t.shape
    v = t.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 1, 3, 4)                    # [rb, ks, r, q, e]
    r = torch.arange(16, device=t.device)
    q = (torch.arange(4, device=t.device)[None, :] ^ ((r[:, None] >> 2) & 3))        # [r, p] -> source chunk
    idx = q[None, None, :, :, None].expand(N // 16, K // 32, 16, 4, 8)
    return torch.gather(v, 3, idx).contiguous()


class SplitWeightF16:
    """Row-scaled f16 hi/lo planes of a Linear weight [N,K] (scp_split_weight_f16), zero-padded to [Npad,Kpad]."""

    def __init__(self, w):
        N, K = w.shape
        self.N, self.K = N, K
        self.Npad, self.Kpad = -(-N // 256) * 256, -(-K // 32) * 32      # 256: the row tile of scp_linear_split_f16 (128 suffices for scp_linear_f16x3)
        self.hi = torch.empty((self.Npad, self.Kpad), dtype=torch.float16, device=w.device)
        self.lo = torch.empty_like(self.hi)
        self.inv_scale = torch.empty((self.Npad,), dtype=torch.float32, device=w.device)
        wc = w.detach().contiguous().float()
        _check(lib().scp_split_weight_f16(_dev(wc), N, K, self.Npad, self.Kpad, _dev(self.hi), _dev(self.lo), _dev(self.inv_scale),
                                          _stream()), "scp_split_weight_f16")
        self.tiled_layout = WTILE
        if self.tiled_layout:       # the tiling is a permutation of 16-bit elements: the same kernel serves f16 planes
            self.hi, self.lo = _tile_in_place_of(self.hi, self.lo, self.Npad, self.Kpad)
        note_cache_fill()


class RowScales:
    """Power-of-two row scales of an fp32 activation [M, K] (scale, 1 / scale) for the f16x3 layers: computed once, shared by every
    layer that reads these rows (`rows(a, b)` = the scales of the row range [a, b))."""

    __slots__ = ("sc", "isc", "x")

    def __init__(self, x2=None, sc=None, isc=None):
        if x2 is not None:
            M, K = x2.shape
            ws = torch.empty((2, M), dtype=torch.float32, device=x2.device)
            _check(lib().scp_row_scale_f16(x2.data_ptr(), x2.stride(0), M, K, ws[0].data_ptr(), ws[1].data_ptr(), _stream()), "scp_row_scale_f16")
            sc, isc = ws[0], ws[1]
        self.sc, self.isc, self.x = sc, isc, x2

    def rows(self, a, b):
        return RowScales(None, self.sc[a:b], self.isc[a:b])

    @staticmethod
    def from_max(row_max):
        """The scales of rows whose maxima a producing kernel's epilogue took (linear_split_f16(..., row_max=...)): int32 [M] bit patterns of max |row|."""
        M = row_max.shape[0]
        ws = torch.empty((2, M), dtype=torch.float32, device=row_max.device)
        _check(lib().scp_row_scale_from_max(_dev(row_max, torch.int32), M, ws[0].data_ptr(), ws[1].data_ptr(), _stream()), "scp_row_scale_from_max")
        return RowScales(None, ws[0], ws[1])


class SplitActF16:
    """An fp32 activation [M, K] as the f16x3 kernels' operand, made ONCE (scp_split_rows_f16): power-of-two row scales (sc, isc) and
    the IEEE-half planes hi / lo [M, ld] of the scaled rows (ld = K rounded up to 32, padding zero).  `rows(a, b)`: the same for the row
    range [a, b) (views)."""

    __slots__ = ("hi", "lo", "sc", "isc", "K")

    def __init__(self, x2=None, parts=None):
        if x2 is not None:
            M, K = x2.shape
            ld = -(-K // 32) * 32
            pl = torch.empty((2, M, ld), dtype=torch.float16, device=x2.device)
            ws = torch.empty((2, M), dtype=torch.float32, device=x2.device)
            _check(lib().scp_split_rows_f16(x2.data_ptr(), x2.stride(0), M, K, pl[0].data_ptr(), pl[1].data_ptr(), ld, ws[0].data_ptr(), ws[1].data_ptr(),
                                            _stream()), "scp_split_rows_f16")
            parts = (pl[0], pl[1], ws[0], ws[1], K)
        self.hi, self.lo, self.sc, self.isc, self.K = parts

    @property
    def M(self):
        return self.hi.shape[0]

    def rows(self, a, b):
        return SplitActF16(parts=(self.hi[a:b], self.lo[a:b], self.sc[a:b], self.isc[a:b], self.K))


def linear_split_f16(a, sw, bias=None, act=ACT_NONE, residual=None, cfg=0, out=None, row_max=None, col_max=None):
    """act(A W^T + bias) + residual on pre-split f16 planes (SplitActF16 x SplitWeightF16) -> fp32 [M, N]; bit-identical to linear_f16x3
    on the fp32 rows the planes were made from (csrc/gemm_split.hip, F16 instantiation: operands by LDS-DMA, no conversion in the tile).
    row_max: ZEROED int32 [M], receives the bit patterns of max |out[m, :]|; col_max = (ZEROED int32 [1], col_lo, col_hi, rows): max |out[:rows,
    col_lo:col_hi]| - taken in the epilogue (scp_linear_split_f16_max), the scales of the next f16x3 layer without a pass over `out`."""
    if not sw.tiled_layout and WTILE:
        raise ScpError("linear_split_f16: weight planes are not tiled")
    M, N = a.M, sw.N
    if a.K != sw.K:
        raise ScpError("linear_split_f16: K mismatch")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.hi.device)
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, N)
        if r2.stride(1) != 1:
            r2 = r2.contiguous()
    if row_max is not None or col_max is not None:
        if row_max is not None and (row_max.dtype != torch.int32 or row_max.shape[0] != M or not row_max.is_contiguous()):
            raise ScpError("linear_split_f16: row_max must be a contiguous int32 [M]")
        cm, lo, hi, rows = col_max if col_max is not None else (None, 0, 0, 0)
        rc = lib().scp_linear_split_f16_max(a.hi.data_ptr(), a.lo.data_ptr(), a.hi.stride(0), a.isc.data_ptr(), sw.hi.data_ptr(), sw.lo.data_ptr(),
                                            sw.inv_scale.data_ptr(), sw.Npad, sw.Kpad, _opt(bias), None if r2 is None else r2.data_ptr(),
                                            0 if r2 is None else r2.stride(0), out.data_ptr(), out.stride(0), M, N, sw.K, act, cfg,
                                            None if row_max is None else row_max.data_ptr(), None if cm is None else _dev(cm, torch.int32), int(lo), int(hi), int(rows),
                                            _stream())
        _check(rc, "scp_linear_split_f16_max")
        return out
    rc = lib().scp_linear_split_f16(a.hi.data_ptr(), a.lo.data_ptr(), a.hi.stride(0), a.isc.data_ptr(), sw.hi.data_ptr(), sw.lo.data_ptr(),
                                    sw.inv_scale.data_ptr(), sw.Npad, sw.Kpad, _opt(bias), None if r2 is None else r2.data_ptr(),
                                    0 if r2 is None else r2.stride(0), out.data_ptr(), out.stride(0), M, N, sw.K, act, cfg, _stream())
    _check(rc, "scp_linear_split_f16")
    return out


def _rows_f16x3(x, K):
    x2 = x.reshape(-1, K)
    if x2.stride(1) != 1 or (x2.stride(0) & 3) or (x2.data_ptr() & 15):
        x2 = x2.contiguous()
    return x2


def linear_f16x3(x, sw, bias=None, act=ACT_NONE, residual=None, scales=None):
    """x [..., K] fp32 -> act(x @ W.T + bias) + residual, [..., N] fp32, on the f16x3 kernel (22-bit operands, row scaled).
    scales: RowScales of exactly these rows (else they are computed here)."""
    K, N = sw.K, sw.N
    lead = x.shape[:-1]
    x2 = _rows_f16x3(x, K)
    M = x2.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, N)
        if r2.stride(1) != 1:
            r2 = r2.contiguous()
    if scales is not None:
        if scales.sc.shape[0] != M:
            raise ScpError("linear_f16x3: row scales of another row count")
        rc = lib().scp_linear_f16x3_scaled(x2.data_ptr(), x2.stride(0), _tiled_pair(sw)[0].data_ptr(), _tiled_pair(sw)[1].data_ptr(), sw.inv_scale.data_ptr(), sw.Kpad,
                                           _opt(bias), None if r2 is None else r2.data_ptr(), 0 if r2 is None else r2.stride(0), out.data_ptr(),
                                           out.stride(0), M, N, K, act, scales.sc.data_ptr(), scales.isc.data_ptr(), _stream())
        _check(rc, "scp_linear_f16x3_scaled")
        return out.reshape(*lead, N)
    ws = torch.empty((2 * M,), dtype=torch.float32, device=x.device)
    rc = lib().scp_linear_f16x3(x2.data_ptr(), x2.stride(0), _tiled_pair(sw)[0].data_ptr(), _tiled_pair(sw)[1].data_ptr(), sw.inv_scale.data_ptr(), sw.Kpad,
                                _opt(bias), None if r2 is None else r2.data_ptr(), 0 if r2 is None else r2.stride(0), out.data_ptr(),
                                out.stride(0), M, N, K, act, ws.data_ptr(), _stream())
    _check(rc, "scp_linear_f16x3")
    return out.reshape(*lead, N)


class SplitAct:
    """An activation [M, K] as bf16 planes hi = bf16(x), lo = bf16(x - hi): t is bfloat16 [2, M, ld] (ld = K rounded up to 32,
    padding columns zero) or a column slice of such a buffer.  This is the operand format of scp_linear_split."""

    __slots__ = ("t", "K")

    def __init__(self, t, K):
        self.t, self.K = t, K

    @staticmethod
    def empty(M, K, device):
        return SplitAct(torch.empty((2, M, -(-K // 32) * 32), dtype=torch.bfloat16, device=device), K)

    @property
    def M(self):
        return self.t.shape[1]

    def cols(self, c0, c1):
        """view of columns [c0, c1) (c0 % 8 == 0)"""
        return SplitAct(self.t[:, :, c0:c1], c1 - c0)

    def float(self):
        return self.t[0, :, :self.K].float() + self.t[1, :, :self.K].float()


def linear_split_scatter(a, sw, bias, out_map, table, act=ACT_NONE, cfg=0):
    """table[out_map[m], :N] = act(a[m] . W^T + bias) for out_map[m] >= 0: fp32 rows written straight to their final positions.
    table: fp32 [rows, ld >= N] with unit column stride (a row-offset view selects the chunk)."""
    t = a.t
    N = sw.N
    if N % 4 and table.stride(0) >= -(-N // 4) * 4 and act == ACT_NONE:
        # ragged width (255 symbols): write the padding columns of the table row as well (zero weights -> just the padded bias) so
        # that every wave takes the 16-byte store path instead of the element-wise edge path
        Np = -(-N // 4) * 4
        if bias is not None:
            pb = getattr(sw, "_bias_pad", None)
            ver = (bias._version, bias.data_ptr())
            if pb is None or pb[0] is not bias or pb[2] != ver:
                pb = (bias, torch.cat((bias.detach().float(), torch.zeros(Np - N, dtype=torch.float32, device=bias.device))).contiguous(), ver)
                sw._bias_pad = pb
                note_cache_fill()
            bias = pb[1]
        N = Np
    _check(lib().scp_linear_split_scatter(t[0].data_ptr(), t[1].data_ptr(), t.stride(1), sw.tiled()[0].data_ptr(), sw.tiled()[1].data_ptr(), sw.Npad, sw.Kpad,
                                          _opt(bias), _dev(out_map, torch.int64), table.data_ptr(), table.stride(0), a.M, N, sw.K, act, cfg,
                                          _stream()), "scp_linear_split_scatter")


def split_rows(x, idx=None, out=None):
    """fp32 rows [n, C] -> SplitAct; idx int64 [rows] gathers rows (idx == n -> zero row)."""
    Cc = x.shape[1]
    rows = x.shape[0] if idx is None else idx.shape[0]
    if out is None:
        out = SplitAct.empty(rows, Cc, x.device)
    if x.stride(1) != 1:
        x = x.contiguous()
    t = out.t
    _check(lib().scp_split_rows(x.data_ptr(), x.stride(0), x.shape[0], _opt(idx), Cc, t[0].data_ptr(), t[1].data_ptr(), t.stride(1), rows,
                                _stream()), "scp_split_rows")
    return out


def linear_split(a, sw, bias=None, act=ACT_NONE, residual=None, out=None, out_split=None, want="f32", cfg=0, res_map=None, res_first=False):
    """a SplitAct [M, K] -> act(a @ W.T + bias) + residual as fp32 [M, N] (want "f32"), as SplitAct (want "split") or both
    (want "both": returns (fp32, SplitAct)).  out / out_split may be column slices of wider buffers."""
    M, N, K = a.M, sw.N, sw.K
    if a.K != K:
        raise ScpError("linear_split: K mismatch %d vs %d" % (a.K, K))
    t = a.t
    c = o = None
    if want in ("f32", "both"):
        c = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=t.device)
    if want in ("split", "both"):
        o = out_split if out_split is not None else SplitAct.empty(M, N, t.device)
    r2 = residual
    if res_map is not None or res_first:
        # out[m] = act(a[m] . W^T + bias + residual[res_map[m]]): gathered residual, added before the activation
        rc = lib().scp_linear_split_gather(t[0].data_ptr(), t[1].data_ptr(), t.stride(1), sw.tiled()[0].data_ptr(), sw.tiled()[1].data_ptr(), sw.Npad, sw.Kpad,
                                           _opt(bias), None if r2 is None else r2.data_ptr(), 0 if r2 is None else r2.stride(0),
                                           None if res_map is None else _dev(res_map, torch.int64),
                                           None if c is None else c.data_ptr(), 0 if c is None else c.stride(0),
                                           None if o is None else o.t[0].data_ptr(), None if o is None else o.t[1].data_ptr(),
                                           0 if o is None else o.t.stride(1), M, N, K, act, cfg, _stream())
        _check(rc, "scp_linear_split_gather")
        return c if want == "f32" else (o if want == "split" else (c, o))
    rc = lib().scp_linear_split(t[0].data_ptr(), t[1].data_ptr(), t.stride(1), sw.tiled()[0].data_ptr(), sw.tiled()[1].data_ptr(), sw.Npad, sw.Kpad, _opt(bias),
                                None if r2 is None else r2.data_ptr(), 0 if r2 is None else r2.stride(0),
                                None if c is None else c.data_ptr(), 0 if c is None else c.stride(0),
                                None if o is None else o.t[0].data_ptr(), None if o is None else o.t[1].data_ptr(),
                                0 if o is None else o.t.stride(1), M, N, K, act, cfg, _stream())
    _check(rc, "scp_linear_split")
    return c if want == "f32" else (o if want == "split" else (c, o))


def linear_split_hier2(a0, sw0, a1, sw1, parent, bias=None, act=ACT_NONE, residual=None, res_map=None, out_split=None):
    """act(a0 . W0^T + a1[parent] . W1^T + bias + residual[res_map]) -> SplitAct [M, N]: the two finest stages of a layer over concat_states
    (ehem.py:75-86) in ONE launch (csrc/gemm_split.hip: gemm_hier2_kernel) - the stage-1 product is computed for the tile's own parents and
    stays in the accumulators, no fp32 partial sum of it exists.  a0: SplitAct [M, K0] (stage-0 rows, M % 256 == 0), a1: SplitAct [M1, 256]
    (stage-1 rows), parent: int64 [M] (stage-1 row of every stage-0 row; consecutive token pairs of a window share consecutive parents),
    residual: fp32 [*, N] rows gathered through res_map (int64 [M]) - the coarser stages' partial sum."""
    if not WTILE:
        raise ScpError("linear_split_hier2 reads tiled weight planes (SCP_WTILE=0 is not supported by it)")
    M, N = a0.M, sw0.N
    if a0.K != sw0.K or a1.K != sw1.K or sw1.K != 256 or sw1.N != N or sw1.Npad != sw0.Npad or parent.shape[0] != M:
        raise ScpError("linear_split_hier2: operand shapes do not match")
    o = out_split if out_split is not None else SplitAct.empty(M, N, a0.t.device)
    t0, t1 = a0.t, a1.t
    rc = lib().scp_linear_split_hier2(t0[0].data_ptr(), t0[1].data_ptr(), t0.stride(1), sw0.Kpad, t1[0].data_ptr(), t1[1].data_ptr(), t1.stride(1), a1.M,
                                      sw0.tiled()[0].data_ptr(), sw0.tiled()[1].data_ptr(), sw1.tiled()[0].data_ptr(), sw1.tiled()[1].data_ptr(), sw0.Npad,
                                      _dev(parent, torch.int64), _opt(bias), None if residual is None else residual.data_ptr(),
                                      0 if residual is None else residual.stride(0), None if (residual is None or res_map is None) else _dev(res_map, torch.int64),
                                      o.t[0].data_ptr(), o.t[1].data_ptr(), o.t.stride(1), M, N, act, _stream())
    _check(rc, "scp_linear_split_hier2")
    return o


class LnFoldedWeight:
    """A Linear that follows a LayerNorm, with the LayerNorm's affine folded in (built once per weight):
    LN(x) . W^T + b = n(x) . (W diag(gamma))^T + (b + W beta), n = the normalised row.  `sw` = split + tiled planes of W diag(gamma),
    `wbeta` = W beta (kept apart from b: rows a window pads AFTER LayerNorm get b alone, swin_transformer.py:638-641)."""

    def __init__(self, w, gamma, beta):
        w64 = w.detach().double()
        self.sw = SplitWeight((w64 * gamma.detach().double()[None, :]).float())
        self.planes = _tiled_planes_always(self.sw)
        self.wbeta = (w64 @ beta.detach().double()).float().contiguous()
        self.N, self.K = self.sw.N, self.sw.K
        note_cache_fill()


def swin_ln_linear(x, fw, bias, eps=1e-5, valid=None, out=None):
    """out = valid * LayerNorm(x) . W^T + bias in one launch (csrc/rowchain.hip): x fp32 [M, 256] rows (unit channel stride),
    fw = LnFoldedWeight, valid fp32 [M] / [M, 1] or None.  -> fp32 [M, N]."""
    M = x.shape[0]
    if x.shape[1] != 256 or fw.K != 256 or x.stride(1) != 1:
        raise ScpError("swin_ln_linear: 256-channel rows expected")
    if out is None:
        out = torch.empty((M, fw.N), dtype=torch.float32, device=x.device)
    t = fw.planes
    rc = lib().scp_swin_ln_linear(x.data_ptr(), x.stride(0), None if valid is None else _dev(valid, torch.float32), t[0].data_ptr(), t[1].data_ptr(),
                                  _opt(bias), _dev(fw.wbeta), float(eps), out.data_ptr(), out.stride(0), M, fw.N, _stream())
    _check(rc, "scp_swin_ln_linear")
    return out


def swin_ln_qkv(x, fw, bias, eps=1e-5, valid=None):
    """swin_ln_linear for a query | key | value (fw.N = 768) or key | value (512) projection whose keys and values leave as the planes of the
    plane-fed window attention: -> (q fp32 [M, 256] or None, KvPlanes).  M % 512 == 0 (rows of the packed layout)."""
    M = x.shape[0]
    if x.shape[1] != 256 or fw.K != 256 or x.stride(1) != 1 or fw.N not in (512, 768) or (M & 127):
        raise ScpError("swin_ln_qkv: 256-channel rows in multiples of 128, N = 768 or 512 expected")
    q = torch.empty((M, 256), dtype=torch.float32, device=x.device) if fw.N == 768 else None
    pl = torch.empty((4, M, 256), dtype=torch.bfloat16, device=x.device)
    t = fw.planes
    rc = lib().scp_swin_ln_qkv(x.data_ptr(), x.stride(0), None if valid is None else _dev(valid, torch.float32), t[0].data_ptr(), t[1].data_ptr(),
                               _opt(bias), _dev(fw.wbeta), float(eps), None if q is None else q.data_ptr(), 256, pl.data_ptr(), M, M, fw.N, _stream())
    _check(rc, "scp_swin_ln_qkv")
    return q, KvPlanes(t=pl)


class EdgeMlpWeights:
    """The two edge MLPs of the geometry feature generator (Sequential(Linear, LeakyReLU, Linear, LeakyReLU, Linear) each: 448 -> 256 -> 256
    -> 256 and 512 -> 256 -> 256 -> 128) in the form scp_geo_edge_mlps streams: eight tiled [256, 256] matrices in a
    scp_swin_post_attn_weight_bytes() buffer (see csrc/rowchain.hip: rc_edge_mlp_kernel) and the six biases back to back."""

    def __init__(self, mlp1, mlp2):
        w11, w12, w13 = (mlp1[i].weight.detach().float() for i in (0, 2, 4))
        w21, w22, w23 = (mlp2[i].weight.detach().float() for i in (0, 2, 4))
        if tuple(w11.shape) != (256, 448) or tuple(w12.shape) != (256, 256) or tuple(w13.shape) != (256, 256) or tuple(w21.shape) != (256, 512) or \
                tuple(w22.shape) != (256, 256) or tuple(w23.shape) != (128, 256):
            raise ScpError("EdgeMlpWeights: unexpected layer shapes")
        dev = w11.device
        P = rc_perm16(256, dev)
        z = torch.zeros((256, 64), dtype=torch.float32, device=dev)
        mats = [w11[:, :256], torch.cat((w11[:, 256:], z), 1), w12[:, P], w13[:, P], w21[:, 256:][:, P], w21[:, :256], w22[:, P],
                torch.cat((w23[:, P], torch.zeros((128, 256), dtype=torch.float32, device=dev)), 0)]
        nbytes = lib().scp_swin_post_attn_weight_bytes()
        buf = torch.zeros((nbytes // 2,), dtype=torch.bfloat16, device=dev)
        half = nbytes // 4
        for m, w in enumerate(mats):
            hi, lo = _tiled_planes_always(SplitWeight(w.contiguous()))
            buf[m * 65536:(m + 1) * 65536] = hi.reshape(-1)[:65536]
            buf[half + m * 65536:half + (m + 1) * 65536] = lo.reshape(-1)[:65536]
        self.packed = buf
        self.bias = torch.cat([mlp1[i].bias.detach().float() for i in (0, 2, 4)] + [mlp2[i].bias.detach().float() for i in (0, 2, 4)]).contiguous()
        note_cache_fill()


def geo_edge_mlps(pos1, pos2, pos3, ew, out):
    """out[:, :128] = edge_mlp2(cat(pos3, edge_mlp1(cat(pos1, pos2, pos3)))) in one launch; pos1 / pos2 / pos3 fp32 [M, 64 | 128 | 256] (unit channel
    stride), out fp32 [M, >= 128] (may be a column slice of a wider buffer)."""
    M = pos1.shape[0]
    if pos1.shape[1] != 64 or pos2.shape[1] != 128 or pos3.shape[1] != 256 or pos1.stride(1) != 1 or pos2.stride(1) != 1 or pos3.stride(1) != 1 or out.stride(1) != 1:
        raise ScpError("geo_edge_mlps: [M, 64], [M, 128], [M, 256] rows expected")
    rc = lib().scp_geo_edge_mlps(pos1.data_ptr(), pos1.stride(0), pos2.data_ptr(), pos2.stride(0), pos3.data_ptr(), pos3.stride(0), ew.packed.data_ptr(),
                                 ew.bias.data_ptr(), out.data_ptr(), out.stride(0), M, _stream())
    _check(rc, "scp_geo_edge_mlps")
    return out


class Mlp3Weights:
    """A three-layer head Sequential(Linear, LeakyReLU, Linear, LeakyReLU, Linear) with 256 inputs and layers of <= 256 outputs in the form
    scp_mlp3_rows streams (csrc/rowchain.hip: rc_mlp3_kernel): three tiled [256, 256] matrices (unused rows / columns zero; layers 2, 3 with their
    columns in accumulator order) in a scp_swin_post_attn_weight_bytes() buffer, the three biases zero padded to 256 back to back."""

    def __init__(self, seq):
        ws = [seq[i].weight.detach().float() for i in (0, 2, 4)]
        bs = [seq[i].bias.detach().float() for i in (0, 2, 4)]
        if ws[0].shape[1] != 256 or any(w.shape[0] > 256 or w.shape[1] > 256 for w in ws) or ws[1].shape[1] != ws[0].shape[0] or ws[2].shape[1] != ws[1].shape[0]:
            raise ScpError("Mlp3Weights: a 256 -> (<= 256) -> (<= 256) -> (<= 256) head expected")
        dev = ws[0].device
        P = rc_perm16(256, dev)
        nbytes = lib().scp_swin_post_attn_weight_bytes()
        buf = torch.zeros((nbytes // 2,), dtype=torch.bfloat16, device=dev)
        half = nbytes // 4
        bias = torch.zeros((3, 256), dtype=torch.float32, device=dev)
        for m, (w, b) in enumerate(zip(ws, bs)):
            full = torch.zeros((256, 256), dtype=torch.float32, device=dev)
            full[:w.shape[0], :w.shape[1]] = w
            if m:
                full = full[:, P]
            hi, lo = _tiled_planes_always(SplitWeight(full.contiguous()))
            buf[m * 65536:(m + 1) * 65536] = hi.reshape(-1)[:65536]
            buf[half + m * 65536:half + (m + 1) * 65536] = lo.reshape(-1)[:65536]
            bias[m, :b.shape[0]] = b
        self.packed, self.bias, self.N = buf, bias.reshape(-1).contiguous(), int(ws[2].shape[0])
        note_cache_fill()


def mlp3_rows(x, mw, out, in_map=None, out_map=None, ncols=None):
    """out[out_map[m] or m, :ncols] = head(x[in_map[m] or m]) in one launch (scp_mlp3_rows): x fp32 [n, 256] rows (unit channel stride), mw = Mlp3Weights,
    out fp32 rows with unit column stride and 16-byte aligned rows (a column-offset view of a wider buffer is fine); in_map / out_map int64 (rows with
    out_map < 0 are dropped); ncols = columns written (default: the head's outputs rounded up to a multiple of 4 - padding columns receive 0)."""
    M = x.shape[0] if in_map is None else in_map.shape[0]
    if out_map is not None and out_map.shape[0] != M:
        raise ScpError("mlp3_rows: out_map must have one entry per row")
    if x.shape[1] != 256 or x.stride(1) != 1 or out.stride(1) != 1:
        raise ScpError("mlp3_rows: [n, 256] rows with unit channel stride expected")
    N = -(-mw.N // 4) * 4 if ncols is None else int(ncols)
    if out_map is None and out.shape[0] < M:
        raise ScpError("mlp3_rows: output has too few rows")
    _check(lib().scp_mlp3_rows(x.data_ptr(), x.stride(0), x.shape[0], None if in_map is None else _dev(in_map, torch.int64), mw.packed.data_ptr(), mw.bias.data_ptr(),
                               out.data_ptr(), out.stride(0), None if out_map is None else _dev(out_map, torch.int64), M, N, _stream()), "scp_mlp3_rows")
    return out


class MergeWeights:
    """SwinPatchMerging's LayerNorm(512) + reduction [256, 512] in the form scp_swin_merge streams (built once per layer): W' = W
    diag(gamma) as two [256, 256] halves, tiled planes at bytes 0 / 131072 of a scp_swin_post_attn_weight_bytes() buffer (lo planes behind
    its first half), and wbeta = W beta."""

    def __init__(self, w, gamma, beta):
        w64 = w.detach().double()
        wf = (w64 * gamma.detach().double()[None, :]).float()
        self.wbeta = (w64 @ beta.detach().double()).float().contiguous()
        nbytes = lib().scp_swin_post_attn_weight_bytes()
        buf = torch.zeros((nbytes // 2,), dtype=torch.bfloat16, device=w.device)
        half = nbytes // 4                                           # bf16 elements per plane region
        for kh in range(2):
            hi, lo = _tiled_planes_always(SplitWeight(wf[:, 256 * kh:256 * (kh + 1)].contiguous()))
            buf[kh * 65536:(kh + 1) * 65536] = hi.reshape(-1)[:65536]
            buf[half + kh * 65536:half + (kh + 1) * 65536] = lo.reshape(-1)[:65536]
        self.packed = buf
        note_cache_fill()


def swin_merge(x, ia, ib, mw, eps=1e-5):
    """LayerNorm(cat(x[ia], x[ib])) . W^T for the M = len(ia) merged rows of a patch-merging layer in one launch (csrc/rowchain.hip);
    an index equal to x.shape[0] stands for a row of zeros.  x fp32 [n, 256] rows (unit channel stride) -> fp32 [M, 256]."""
    M = ia.shape[0]
    if x.shape[1] != 256 or x.stride(1) != 1:
        raise ScpError("swin_merge: 256-channel rows expected")
    out = torch.empty((M, 256), dtype=torch.float32, device=x.device)
    rc = lib().scp_swin_merge(x.data_ptr(), x.stride(0), x.shape[0], _dev(ia, torch.int64), _dev(ib, torch.int64), mw.packed.data_ptr(), _dev(mw.wbeta),
                              float(eps), out.data_ptr(), out.stride(0), M, _stream())
    _check(rc, "scp_swin_merge")
    return out


def rc_perm16(n, device):
    """Column permutation of the row-chain kernels' chained operands (csrc/rowchain.hip): inside every group of 16, columns 4-7 and
    8-11 change places - the order in which an MFMA accumulator holds a row's channels, read as the next product's B fragment."""
    p = torch.arange(n, device=device)
    q = p & 15
    return (p & ~15) | (q & 3) | ((q & 4) << 1) | ((q & 8) >> 1)


class PostAttnWeights:
    """Weights of a Swin block's post-attention half in the form scp_swin_post_attn streams (built once per block): proj as it is;
    fc1 with layernorm_after's affine folded in (W1 diag(gamma), b1 + W1 beta) and its K axis in accumulator order; fc2 with its
    hidden axis in accumulator order.  The kernel evaluates GELU in the variable s y (s = scp_gelu_prescale(), csrc/scp_internal.h): fc1
    (weight and bias) carries the factor s, fc2's weight 1 / s."""

    def __init__(self, wp, bp, gamma, beta, w1, b1, w2, b2):
        dev = wp.device
        perm_k, perm_h = rc_perm16(256, dev), rc_perm16(w1.shape[0], dev)
        w1d = w1.detach().double()
        s = float(lib().scp_gelu_prescale())
        swp = SplitWeight(wp.detach().float().contiguous())
        sw1 = SplitWeight((w1d * gamma.detach().double()[None, :] * s).float()[:, perm_k].contiguous())
        sw2 = SplitWeight((w2.detach().double() / s).float()[:, perm_h].contiguous())
        # one buffer for the kernel's single buffer resource: the tiled planes proj hi | fc1 hi | fc2 hi | proj lo | fc1 lo | fc2 lo
        tiles = [_tiled_planes_always(w) for w in (swp, sw1, sw2)]
        self.packed = torch.cat([t[0].reshape(-1) for t in tiles] + [t[1].reshape(-1) for t in tiles]).contiguous()
        if self.packed.numel() * 2 != lib().scp_swin_post_attn_weight_bytes():
            raise ScpError("swin_post_attn: 256 -> 1024 -> 256 blocks only")
        self.bp = bp.detach().float().contiguous()
        self.b1 = ((b1.detach().double() + w1d @ beta.detach().double()) * s).float().contiguous()
        self.b2 = b2.detach().float().contiguous()
        note_cache_fill()


def swin_post_attn(o, x, pw, eps=1e-5, out=None, tiles=None):
    """x + proj(o) -> LayerNorm -> fc1 -> GELU -> fc2 -> + residual, one launch (csrc/rowchain.hip).  o: FragAct or SplitAct [M, 256] (the
    attention output planes, in fragment order or as rows), x: fp32 [M, 256] residual stream, pw: PostAttnWeights.  -> fp32 [M, 256] (`out` may be x itself).
    tiles (int32 device tensor, optional): the 128-row tiles to process (ascending); the others keep what `out` held (use out=x)."""
    M = x.shape[0]
    if o.K != 256 or o.M != M or x.shape[1] != 256 or x.stride(1) != 1:
        raise ScpError("swin_post_attn: [M, 256] operands expected")
    if out is None:
        out = torch.empty((M, 256), dtype=torch.float32, device=x.device)
    t = o.t
    ldo = LDO_FRAG if isinstance(o, FragAct) else t.stride(1)       # planes in fragment order / as rows
    rc = lib().scp_swin_post_attn(t[0].data_ptr(), t[1].data_ptr(), ldo, x.data_ptr(), x.stride(0), pw.packed.data_ptr(), _dev(pw.bp),
                                  _dev(pw.b1), _dev(pw.b2), float(eps), out.data_ptr(), out.stride(0), M,
                                  None if tiles is None else _dev(tiles, torch.int32), 0 if tiles is None else int(tiles.shape[0]), _stream())
    _check(rc, "scp_swin_post_attn")
    return out


def layernorm_rows(x, gamma, beta, eps=1e-5, valid=None, ia=None, ib=None, out=None, split=False):
    """x [n,256|512...] fp32 rows (unit channel stride).  Plain LN (ia None), LN of gathered rows (ia, C = 256) or of
    cat(x[ia], x[ib]) (C = 512).  valid: fp32 [rows] or [rows,1] multiplier.  Returns [rows, C] fp32, or a SplitAct (split=True)."""
    Cc = gamma.shape[0]
    rows = x.shape[0] if ia is None else ia.shape[0]
    if split:
        o = SplitAct.empty(rows, Cc, x.device)
        rc = lib().scp_layernorm_rows_split(x.data_ptr(), x.stride(0), x.shape[0], None if ia is None else _dev(ia, torch.int64),
                                            None if ib is None else _dev(ib, torch.int64), Cc, _dev(gamma), _dev(beta),
                                            None if valid is None else _dev(valid, torch.float32), float(eps), o.t[0].data_ptr(),
                                            o.t[1].data_ptr(), o.t.stride(1), rows, _stream())
        _check(rc, "scp_layernorm_rows_split")
        return o
    if out is None:
        out = torch.empty((rows, Cc), dtype=torch.float32, device=x.device)
    rc = lib().scp_layernorm_rows(x.data_ptr(), x.stride(0), x.shape[0], None if ia is None else _dev(ia, torch.int64),
                                  None if ib is None else _dev(ib, torch.int64), Cc, _dev(gamma), _dev(beta),
                                  None if valid is None else _dev(valid, torch.float32), float(eps), out.data_ptr(), out.stride(0),
                                  rows, _stream())
    _check(rc, "scp_layernorm_rows")
    return out


def layernorm_add(a, b, gamma, beta, eps=1e-5, planes=False):
    """LayerNorm(a + b) over the last axis (contiguous fp32 tensors of one shape; b may be None) in one kernel.  planes=True: returns
    (out, SplitActF16 of out's rows) - the f16x3 operand of the dense layers that read `out`, written in the same pass."""
    Cc = a.shape[-1]
    if not a.is_contiguous() or (b is not None and (not b.is_contiguous() or b.shape != a.shape)):
        raise ScpError("layernorm_add: contiguous operands of one shape expected")
    out = torch.empty_like(a)
    if planes:
        M, ld = a.numel() // Cc, -(-Cc // 32) * 32
        pl = torch.empty((2, M, ld), dtype=torch.float16, device=a.device)
        ws = torch.empty((2, M), dtype=torch.float32, device=a.device)
        _check(lib().scp_layernorm_add_split_f16(_dev(a, torch.float32), None if b is None else _dev(b, torch.float32), M, Cc, _dev(gamma), _dev(beta),
                                                 float(eps), out.data_ptr(), pl[0].data_ptr(), pl[1].data_ptr(), ld, ws[0].data_ptr(), ws[1].data_ptr(),
                                                 _stream()), "scp_layernorm_add_split_f16")
        return out, SplitActF16(parts=(pl[0], pl[1], ws[0], ws[1], Cc))
    _check(lib().scp_layernorm_add(_dev(a, torch.float32), None if b is None else _dev(b, torch.float32), a.numel() // Cc, Cc, _dev(gamma), _dev(beta),
                                   float(eps), out.data_ptr(), _stream()), "scp_layernorm_add")
    return out


def gather_rows(src, idx, out):
    """out[r, :C] = src[idx[r], :C]; `out` may be a column slice of a wider buffer (C = out.shape[1])."""
    Cc = out.shape[1]
    rc = lib().scp_gather_rows(src.data_ptr(), src.stride(0), _dev(idx, torch.int64), Cc, out.data_ptr(), out.stride(0), idx.shape[0],
                               _stream())
    _check(rc, "scp_gather_rows")
    return out


def linear_f32(x, w, bias=None, act=ACT_NONE):
    """exact fp32, batch-invariant dense layer: x [..., K] (unit last stride) @ w[N,K]^T (+bias, act) -> [..., N]."""
    K = w.shape[1]
    N = w.shape[0]
    lead = x.shape[:-1]
    x2 = x.reshape(-1, K) if x.is_contiguous() else x.contiguous().reshape(-1, K)
    M = x2.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    wc = w if w.is_contiguous() else w.contiguous()
    rc = lib().scp_linear_f32(x2.data_ptr(), x2.stride(0), _dev(wc.detach(), torch.float32), _opt(bias), out.data_ptr(), N, M, N, K, act,
                              _stream())
    _check(rc, "scp_linear_f32")
    return out.reshape(*lead, N)


OCTATTN_MODE = os.environ.get("SCP_OCTATTN", "f16x3")   # "f32": the fp32 MFMA kernel for head width 150 as well


def octattn_attention(q_u, k, k_u, v, v_u, heads, out=None, out_u=None, vmax=None):
    """Dual-stream causal attention (models/attention_model.py:58-95).  Head width 150 (the reference configuration) runs on the
    f16x3 kernel (22-bit operands on f16 MFMA, csrc/octattn_f16.hip); SCP_OCTATTN=f32 or any other width: the fp32 kernels.
    k, k_u, v, v_u may be column slices of one key | value projection output (unit channel stride, one common row stride)."""
    B, c, D = q_u.shape
    if out is None:
        out, out_u = torch.empty_like(q_u), torch.empty_like(q_u)
    elif not (out.is_contiguous() and out_u.is_contiguous() and out.shape == q_u.shape and out_u.shape == q_u.shape):
        raise ScpError("octattn_attention: out / out_u must be contiguous [B, c, D] float32")
    hd = D // heads
    ld = k.stride(-2)
    strided_ok = all(t.is_cuda and t.dtype == torch.float32 and t.stride(-1) == 1 and t.stride(-2) == ld and (t.dim() == 2 or t.stride(0) == c * ld)
                     for t in (k, k_u, v, v_u))
    if OCTATTN_MODE == "f16x3" and hd == 150 and (D & 3) == 0 and strided_ok:
        nb = lib().scp_octattn_f16x3_ws_bytes(B, c, heads)
        ws = torch.empty((nb + 1024,), dtype=torch.uint8, device=q_u.device)
        off = (-ws.data_ptr()) % 1024
        if vmax is not None:    # max |v| taken by the epilogue of the projection that wrote v (int32 [1]: the bit pattern of the float)
            rc = lib().scp_octattn_attention_f16x3_vmax(_dev(q_u), k.data_ptr(), k_u.data_ptr(), v.data_ptr(), v_u.data_ptr(), ld, B, c, heads, hd, _dev(out),
                                                        _dev(out_u), ws.data_ptr() + off, nb, _dev(vmax, torch.int32), _stream())
            _check(rc, "scp_octattn_attention_f16x3_vmax")
            return out, out_u
        rc = lib().scp_octattn_attention_f16x3(_dev(q_u), k.data_ptr(), k_u.data_ptr(), v.data_ptr(), v_u.data_ptr(), ld, B, c, heads, hd, _dev(out),
                                               _dev(out_u), ws.data_ptr() + off, nb, _stream())
        _check(rc, "scp_octattn_attention_f16x3")
        return out, out_u
    k, k_u, v, v_u = (t.contiguous() for t in (k, k_u, v, v_u))
    rc = lib().scp_octattn_attention(_dev(q_u), _dev(k), _dev(k_u), _dev(v), _dev(v_u), B, c, heads, hd,
                                     _dev(out), _dev(out_u), _stream())
    _check(rc, "scp_octattn_attention")
    return out, out_u


def _win_strides(t):
    """(window stride, row stride) in floats of a [B, c, X] or [c, X] float32 device tensor with unit channel stride."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.stride(-1) == 1):
        raise ScpError("octattn_attention_rowinv: float32 device tensors with unit channel stride expected")
    return (t.stride(0) if t.dim() == 3 else 0), t.stride(-2)


def octattn_attention_rowinv(q_u, k, v, heads, k_u=None, v_u=None, out=None, out_u=None, q0=0, q1=None, qoff=0):
    """The decodable profile's dual-stream causal attention (csrc/octattn_rowinv.hip): query rows [q0, q1) of every window, each row
    bit-identical whatever range or batch it is launched with.  k, v [B, >= q1, D] (or [>= q1, D]): the known stream's keys / values of
    rows 0 .. q1 - 1 (a column slice of the key | value projection, or a decoder's cache); q_u, k_u, v_u, out, out_u: row r at index
    r - qoff.  out / out_u: written in place when given (one of them may be None: that stream is skipped)."""
    D = q_u.shape[-1]
    B = q_u.shape[0] if q_u.dim() == 3 else 1
    q1 = (q_u.shape[-2] + qoff) if q1 is None else q1
    if out is None and out_u is None:
        raise ScpError("octattn_attention_rowinv: nothing to compute (out and out_u are None)")
    if q1 > k.shape[-2] or q1 - qoff > q_u.shape[-2]:
        raise ScpError("octattn_attention_rowinv: query range beyond the key rows")
    for t in (out, out_u, k_u, v_u):
        if t is not None and t.shape[-2] < q1 - qoff:
            raise ScpError("octattn_attention_rowinv: operand shorter than the query range")
    qw, qr = _win_strides(q_u)
    kw, kr = _win_strides(k)
    if _win_strides(v) != (kw, kr):
        raise ScpError("octattn_attention_rowinv: k and v must share their strides")
    uw = ur = 0
    if out_u is not None:
        uw, ur = _win_strides(k_u)
        if _win_strides(v_u) != (uw, ur):
            raise ScpError("octattn_attention_rowinv: k_u and v_u must share their strides")
    ow, orr = _win_strides(out if out is not None else out_u)
    if out is not None and out_u is not None and _win_strides(out_u) != (ow, orr):
        raise ScpError("octattn_attention_rowinv: out and out_u must share their strides")
    ptr = lambda t: None if t is None else t.data_ptr()        # strided views: the strides above describe them
    rc = lib().scp_octattn_attention_rowinv(q_u.data_ptr(), qw, qr, k.data_ptr(), v.data_ptr(), kw, kr, ptr(k_u), ptr(v_u), uw, ur, ptr(out),
                                            ptr(out_u), ow, orr, B, int(q0), int(q1), int(qoff), int(heads), D // heads, _stream())
    _check(rc, "scp_octattn_attention_rowinv")
    return out, out_u


def octattn_attention_rowinv_step(q_u, k, v, t, slot, heads, k_u=None, v_u=None, out=None, out_u=None):
    """The decodable profile's attention for ONE query row per stream (csrc/octattn_rowinv.hip: scp_octattn_attention_rowinv_step).
    q_u [S, D]: launch row s is the row stream slot[s] is decoding, row t[slot[s]] of its window; k, v [slots, rows, D]: the known
    stream's cache (column slices allowed: slot and row strides are passed); t int32 [slots], slot int32 [S]: device tensors, read by
    the kernel (no position is a launch argument, nothing synchronises).  k_u, v_u, out, out_u [S, D]; out / out_u are written in
    place, one of them may be None.  Row s has the bits of octattn_attention_rowinv(q0=t, q1=t + 1) on that slot's cache."""
    if out is None and out_u is None:
        raise ScpError("octattn_attention_rowinv_step: nothing to compute (out and out_u are None)")
    if q_u.dim() != 2 or k.dim() != 3 or v.shape != k.shape or k.shape[-1] != q_u.shape[-1]:
        raise ScpError("octattn_attention_rowinv_step: q_u [S, D] and k, v [slots, rows, D] expected")
    S, D = q_u.shape
    for x in (t, slot):
        if not (x.is_cuda and x.dtype == torch.int32 and x.dim() == 1 and x.is_contiguous()):
            raise ScpError("octattn_attention_rowinv_step: t and slot are contiguous int32 device tensors")
    if t.shape[0] != k.shape[0] or slot.shape[0] != S:
        raise ScpError("octattn_attention_rowinv_step: t has one entry per cache slot, slot one per launch row")
    if out_u is not None and (k_u is None or v_u is None):
        raise ScpError("octattn_attention_rowinv_step: out_u needs k_u and v_u")
    for x in (out, out_u) + ((k_u, v_u) if out_u is not None else ()):
        if x is not None and (x.dim() != 2 or x.shape[0] < S or x.shape[1] != D):
            raise ScpError("octattn_attention_rowinv_step: k_u, v_u, out, out_u are [S, D]")
    _, qr = _win_strides(q_u)
    kw, kr = _win_strides(k)
    if _win_strides(v) != (kw, kr):
        raise ScpError("octattn_attention_rowinv_step: k and v must share their strides")
    ur = 0
    if out_u is not None:
        _, ur = _win_strides(k_u)
        if _win_strides(v_u)[1] != ur:
            raise ScpError("octattn_attention_rowinv_step: k_u and v_u must share their row stride")
    _, orr = _win_strides(out if out is not None else out_u)
    if out is not None and out_u is not None and _win_strides(out_u)[1] != orr:
        raise ScpError("octattn_attention_rowinv_step: out and out_u must share their row stride")
    ptr = lambda x: None if x is None else x.data_ptr()        # strided views: the strides above describe them
    rc = lib().scp_octattn_attention_rowinv_step(q_u.data_ptr(), qr, k.data_ptr(), v.data_ptr(), kw, kr, k.shape[0], k.shape[1], ptr(k_u), ptr(v_u),
                                                 ur, ptr(out), ptr(out_u), orr, t.data_ptr(), slot.data_ptr(), S, int(heads), D // heads, _stream())
    _check(rc, "scp_octattn_attention_rowinv_step")
    return out, out_u


def decode_expand_octattn(sym, ctx, apos, L, depth):
    """Decoder, OctAttention layout: children of one decoded level + their model inputs, one launch (csrc/plan.hip:
    scp_decode_expand_octattn).  sym int64 [n] (-1 = no children), ctx uint8 [n,12], apos int32 [n,4,3] (the parents' context rows and
    their four integer origins) -> (occ8 uint8 [n], cctx uint8 [m,12], capos int32 [m,4,3], cpos float32 [m,4,3]); one host sync (m)."""
    dev, n = sym.device, sym.shape[0]
    tab = popcount_table(dev)
    cum = torch.cumsum(tab[sym + 1], 0)
    m = int(cum[-1])
    occ8 = torch.empty(n, dtype=torch.uint8, device=dev)
    cctx = torch.empty((m, 12), dtype=torch.uint8, device=dev)
    capos = torch.empty((m, 4, 3), dtype=torch.int32, device=dev)
    cpos = torch.empty((m, 4, 3), dtype=torch.float32, device=dev)
    if m == 0:
        return (sym + 1).clamp_(min=0).to(torch.uint8), cctx, capos, cpos
    _check(lib().scp_decode_expand_octattn(_dev(sym, torch.int64), cum.data_ptr(), _dev(ctx, torch.uint8), _dev(apos, torch.int32), n, int(L),
                                           int(depth - L), int(depth), cctx.data_ptr(), capos.data_ptr(), cpos.data_ptr(), occ8.data_ptr(), _stream()),
           "scp_decode_expand_octattn")
    return occ8, cctx, capos, cpos


def octattn_embed(ctx, pos, c, occ_enc, level_enc, octant_enc, pos_w, pos_b, pe, level_cap, max_level):
    """OctAttention's input stage in one launch (csrc/octattn_embed.hip): ctx uint8 [n,12], pos f32 [n,4,3] (n = B * c rows) ->
    (E f32 [2, n, D] both streams, SplitActF16 of E's 2 n rows)."""
    n = ctx.shape[0]
    d_occ, d_lvl, d_oct = occ_enc.shape[1], level_enc.shape[1], octant_enc.shape[1]
    d_pos = 0 if pos_w is None else pos_w.shape[0]
    D = 4 * (d_occ + d_lvl + d_oct + d_pos)
    ld = -(-D // 32) * 32
    dev = ctx.device
    E = torch.empty((2, n, D), dtype=torch.float32, device=dev)
    pl = torch.empty((2, 2 * n, ld), dtype=torch.float16, device=dev)
    ws = torch.empty((2, 2 * n), dtype=torch.float32, device=dev)
    rc = lib().scp_octattn_embed(_dev(ctx, torch.uint8), _dev(pos, torch.float32), n, c, _dev(occ_enc, torch.float32), d_occ, _dev(level_enc, torch.float32),
                                 d_lvl, max_level, _dev(octant_enc, torch.float32), d_oct, _opt(pos_w), _opt(pos_b), d_pos, _dev(pe, torch.float32),
                                 level_cap, E.data_ptr(), pl[0].data_ptr(), pl[1].data_ptr(), ld, ws[0].data_ptr(), ws[1].data_ptr(), _stream())
    _check(rc, "scp_octattn_embed")
    return E, SplitActF16(parts=(pl[0], pl[1], ws[0], ws[1], D))


# ------------------------------------------------------------------------------------------------- stage C
def softmax_cdf(logits, sym=None, want_pmf=False, want_lohi=True, want_cdf=False):
    """logits cuda f32 [n,nsym] (row stride allowed) -> dict(pmf, lohi, cdf)."""
    n, nsym = logits.shape
    if logits.stride(1) != 1:
        raise ScpError("softmax_cdf: unit column stride expected")
    dev = logits.device
    pmf = torch.empty((n, nsym), dtype=torch.float32, device=dev) if want_pmf else None
    lohi = torch.empty(n, dtype=torch.int32, device=dev) if (want_lohi and sym is not None) else None
    cdf = torch.empty((n, nsym + 1), dtype=torch.int16, device=dev) if want_cdf else None
    rc = lib().scp_softmax_cdf(logits.data_ptr(), logits.stride(0), n, nsym, _opt(sym), _opt(pmf), _opt(lohi), _opt(cdf),
                               _stream())
    _check(rc, "scp_softmax_cdf")
    return dict(pmf=pmf, lohi=lohi, cdf=cdf)


def pmf_cdf(pmf, sym=None, want_cdf=False):
    n, nsym = pmf.shape
    dev = pmf.device
    lohi = torch.empty(n, dtype=torch.int32, device=dev) if sym is not None else None
    cdf = torch.empty((n, nsym + 1), dtype=torch.int16, device=dev) if want_cdf else None
    rc = lib().scp_pmf_cdf(_dev(pmf, torch.float32), n, nsym, _opt(sym), _opt(lohi), _opt(cdf), _stream())
    _check(rc, "scp_pmf_cdf")
    return dict(lohi=lohi, cdf=cdf)


RATE_FIELDS = ("rows", "ideal_bits", "table_bits", "top1", "bad_rows")     # include/scp.h: scp_rate_seg, five 8-byte fields


def rate_segments(logits, sym, lohi, seg_off, want_rows=False):
    """Rate report of a coding-order logits table (csrc/rate.hip: scp_rate_segments).  logits cuda f32 [n,nsym] (row stride allowed), sym
    uint8 [n], lohi int32 [n] as softmax_cdf returns it; seg_off: the n_seg + 1 row offsets of the segments - a device int64 tensor, or a
    host sequence (then uploaded out of pinned memory on the current stream: nothing is awaited).  -> dict of device tensors per segment:
    rows, top1, bad_rows int64 [S], ideal_bits, table_bits float64 [S] (views of `raw` int64 [S,5], the scp_rate_seg records: one copy
    brings them all to the host); with want_rows also row_ideal, row_table float64 [n]; `keep`: what the launches use (workspace,
    offsets) - hold it until they have run."""
    n, nsym = logits.shape
    if logits.stride(1) != 1:
        raise ScpError("rate_segments: unit column stride expected")
    dev = logits.device
    if not isinstance(seg_off, torch.Tensor):
        host = torch.from_numpy(np.ascontiguousarray(seg_off, np.int64))
        seg_off = (host.pin_memory() if torch.cuda.is_available() else host).to(dev, non_blocking=True)
    S = int(seg_off.shape[0]) - 1
    if S < 0 or sym.shape[0] != n or lohi.shape[0] != n:
        raise ScpError("rate_segments: one symbol and one pair per row, and at least one offset, expected")
    raw = torch.empty((S, len(RATE_FIELDS)), dtype=torch.int64, device=dev)
    ws_bytes = int(lib().scp_rate_workspace_bytes(n, S))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    ri = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
    rt = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
    ld = int(logits.stride(0)) if n > 1 else max(int(logits.stride(0)), nsym)      # (the stride of a single row says nothing)
    rc = lib().scp_rate_segments(logits.data_ptr(), ld, n, nsym, _dev(sym, torch.uint8),
                                 _dev(lohi), _dev(seg_off, torch.int64), S, raw.data_ptr(), _opt(ri), _opt(rt), ws.data_ptr(), ws_bytes, _stream())
    _check(rc, "scp_rate_segments")
    out = dict(raw=raw, keep=(ws, seg_off), row_ideal=ri, row_table=rt)
    for k, name in enumerate(RATE_FIELDS):
        out[name] = raw[:, k].view(torch.float64) if name.endswith("_bits") else raw[:, k]
    return out


# ------------------------------------------------------------------------------------------------- temperature (csrc/temper.hip)
TEMPER_MAX_NT = 32                                                         # include/scp.h: SCP_TEMPER_MAX_NT
TEMPER_MIN_GAIN_BITS = 8.0                                                 # the byte a group's index costs as side information


def temper_grid(grid=None):
    """The grid of inverse temperatures as (numpy float32 [nt], index of its 1.0f).  None: float32(2 ** (j / 8)) for j = -12 .. 12, 25
    values from 0.354 to 2.83.  A grid holds 1 .. TEMPER_MAX_NT finite positive values, exactly one of them 1.0f."""
    g = np.array([2.0 ** (j / 8) for j in range(-12, 13)] if grid is None else grid, dtype=np.float64).astype(np.float32).reshape(-1)
    if not 1 <= g.shape[0] <= TEMPER_MAX_NT:
        raise ScpError(f"temper grid: {g.shape[0]} values, 1 .. {TEMPER_MAX_NT} expected")
    if not (np.isfinite(g).all() and (g > 0).all()):
        raise ScpError("temper grid: every inverse temperature is finite and positive")
    ones = np.flatnonzero(g == np.float32(1.0))
    if ones.shape[0] != 1:
        raise ScpError(f"temper grid: exactly one value is 1.0 (the stream as it is without the option), found {ones.shape[0]}")
    return np.ascontiguousarray(g), int(ones[0])


def _seg_off_dev(seg_off, dev):
    if isinstance(seg_off, torch.Tensor):
        return seg_off
    host = torch.from_numpy(np.ascontiguousarray(seg_off, np.int64))
    return (host.pin_memory() if torch.cuda.is_available() else host).to(dev, non_blocking=True)


def _row_stride(t):
    n, nsym = t.shape
    return int(t.stride(0)) if n > 1 else max(int(t.stride(0)), nsym)      # (the stride of a single row says nothing)


def temper_sweep(logits, sym, seg_off, betas, want_rows=False, out=None):
    """scp_temper_sweep: the ideal bits of every segment of a coding-order logits table at every inverse temperature of `betas` (float32
    values, at most TEMPER_MAX_NT, finite and positive).  logits / sym / seg_off as for rate_segments.  -> dict of device tensors: seg_bits
    float64 [S,nt], seg_bad int32 [S,nt] (column j = rate_segments' ideal_bits / bad_rows on the table scaled by betas[j], bit for bit),
    with want_rows row_bits float64 [n,nt]; seg_off (on the device); `keep`: what the launches use.  out: (seg_bits, seg_bad) to write into."""
    n, nsym = logits.shape
    if logits.stride(1) != 1:
        raise ScpError("temper_sweep: unit column stride expected")
    dev = logits.device
    seg_off = _seg_off_dev(seg_off, dev)
    betas = np.ascontiguousarray(betas, np.float32).reshape(-1)
    S, nt = int(seg_off.shape[0]) - 1, int(betas.shape[0])
    if S < 0 or sym.shape[0] != n:
        raise ScpError("temper_sweep: one symbol per row, and at least one offset, expected")
    ws_bytes = int(lib().scp_temper_workspace_bytes(n, S, nt))
    if ws_bytes < 0:
        raise ScpError(f"temper_sweep: a grid of {nt} values: 1 .. {TEMPER_MAX_NT} expected")
    seg_bits, seg_bad = out if out is not None else (torch.empty((S, nt), dtype=torch.float64, device=dev),
                                                     torch.empty((S, nt), dtype=torch.int32, device=dev))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    rows = torch.empty((n, nt), dtype=torch.float64, device=dev) if want_rows else None
    rc = lib().scp_temper_sweep(logits.data_ptr(), _row_stride(logits), n, nsym, _dev(sym, torch.uint8), _dev(seg_off, torch.int64), S,
                                betas.ctypes.data, nt, _dev(seg_bits, torch.float64), _dev(seg_bad, torch.int32), _opt(rows), ws.data_ptr(),
                                ws_bytes, _stream())
    _check(rc, "scp_temper_sweep")
    return dict(seg_bits=seg_bits, seg_bad=seg_bad, row_bits=rows, seg_off=seg_off, keep=(ws, seg_off))


def temper_choose(seg_bits, seg_bad, seg_off, n, group, ngroup, betas, unit, min_gain_bits=TEMPER_MIN_GAIN_BITS, out=None):
    """scp_temper_choose: one grid index per group of segments from a sweep's seg_bits / seg_bad (include/scp.h states the rule).  group:
    int32 [S], the group of every segment (device tensor, or a host sequence - uploaded out of pinned memory, nothing awaited); seg_off: the
    sweep's device offsets; n: the table's rows.  -> dict of device tensors: choice int32 [G], group_bits float64 [G,2] (at unit, at the
    choice), seg_beta float32 [S]; `keep`.  out: (choice, group_bits) to write into."""
    dev = seg_bits.device
    betas = np.ascontiguousarray(betas, np.float32).reshape(-1)
    S, nt = seg_bits.shape
    if not isinstance(group, torch.Tensor):
        host = torch.from_numpy(np.ascontiguousarray(group, np.int32))
        group = (host.pin_memory() if torch.cuda.is_available() else host).to(dev, non_blocking=True)
    if nt != betas.shape[0] or group.shape[0] != S or seg_bad.shape != seg_bits.shape or seg_off.shape[0] != S + 1:
        raise ScpError("temper_choose: seg_bits / seg_bad [S,nt] of a sweep over this grid, S + 1 offsets and one group per segment expected")
    choice, group_bits = out if out is not None else (torch.empty(ngroup, dtype=torch.int32, device=dev),
                                                      torch.empty((ngroup, 2), dtype=torch.float64, device=dev))
    seg_beta = torch.empty(S, dtype=torch.float32, device=dev)
    rc = lib().scp_temper_choose(_dev(seg_bits, torch.float64), _dev(seg_bad, torch.int32), _dev(seg_off, torch.int64), n, _dev(group, torch.int32),
                                 S, ngroup, betas.ctypes.data, nt, unit, float(min_gain_bits), _dev(choice, torch.int32),
                                 _dev(group_bits, torch.float64), seg_beta.data_ptr(), _stream())
    _check(rc, "scp_temper_choose")
    return dict(choice=choice, group_bits=group_bits, seg_beta=seg_beta, keep=(group, seg_off))


def scale_rows(table, seg_off, seg_beta, out=None):
    """scp_scale_rows: out[r, c] = float32(seg_beta[s] * table[r, c]) for the segment s of seg_off that holds row r - one float32 multiply,
    the arithmetic the encoder and the decoder of a tempered stream share.  table cuda f32 [n,nsym] (row stride allowed); seg_off: S + 1
    offsets (device int64, or a host sequence), seg_beta float32 [S] (device, or a host sequence).  out None: in place (columns beyond
    nsym of a strided table are left alone) -> table; else a f32 [n,nsym] tensor that does not overlap it -> out."""
    n, nsym = table.shape
    dev = table.device
    dst = table if out is None else out
    if table.stride(1) != 1 or dst.stride(1) != 1 or dst.shape != table.shape or dst.dtype != torch.float32 or table.dtype != torch.float32:
        raise ScpError("scale_rows: float32 tables of one shape with unit column stride expected")
    seg_off = _seg_off_dev(seg_off, dev)
    if not isinstance(seg_beta, torch.Tensor):
        host = torch.from_numpy(np.ascontiguousarray(seg_beta, np.float32))
        seg_beta = (host.pin_memory() if torch.cuda.is_available() else host).to(dev, non_blocking=True)
    S = int(seg_off.shape[0]) - 1
    if S < 0 or seg_beta.shape[0] != S:
        raise ScpError("scale_rows: S + 1 offsets and S inverse temperatures expected")
    rc = lib().scp_scale_rows(table.data_ptr(), _row_stride(table), dst.data_ptr(), _row_stride(dst), n, nsym, _dev(seg_off, torch.int64),
                              _dev(seg_beta, torch.float32), S, _stream())
    _check(rc, "scp_scale_rows")
    return dst


# ------------------------------------------------------------------------------------------------- ring LOD (csrc/ringlod.hip)
RINGLOD_MAX, RINGLOD_MAX_RINGS, RINGLOD_MAX_TABLES = 8, 32, 64             # include/scp.h: SCP_RINGLOD_MAX*
RINGLOD_SEG = np.dtype([("first", np.int64), ("count", np.int64), ("depth", np.int32), ("table", np.int32)])      # scp_ringlod_seg
# what a forced row costs under the coder's 16-bit tables: its one-hot CDF row is (c_low, c_high) = (0, 65282) - DESIGN.md 6, "Ring LOD"
FORCED_ROW_TABLE_BITS = 16.0 - float(np.log2(65282.0))


def ringlod_thresholds(edges, qs0, offset0):
    """Ring edges (dist_edges form: 0 = E_0 < E_1 < ...) -> the integer thresholds of E_1 .. on the radial axis of a shell quantised with
    step qs0 and offset offset0: t_i = clamp(ceil((E_i - offset0) / qs0), 0, 2^31 - 1), in float64 on the host.  A point of quantised
    radius q lies at q * qs0 + offset0, so q >= t_i says that it lies at or beyond E_i."""
    import math
    out = []
    for e in list(edges)[1:]:
        v = (float(e) - float(offset0)) / float(qs0)
        out.append(int(min(max(math.ceil(v), 0), 2 ** 31 - 1)) if v == v and abs(v) != float("inf") else (0 if v < 0 else 2 ** 31 - 1))
    return out


def _ringlod_tables(thresholds, drops):
    """One table (a flat list of thresholds) or several (a list of lists), one list of drops for all or one per table -> (int64 [T,R-1],
    uint8 [T,R]).  Shapes only: the library checks the values."""
    drops = np.asarray(drops)
    thr = np.asarray(thresholds, dtype=np.int64)
    if drops.ndim == 1:
        thr = thr.reshape(1, -1) if thr.ndim <= 1 else thr
        drops = np.broadcast_to(drops, (thr.shape[0], drops.shape[0]))
    if thr.ndim == 1:
        thr = thr.reshape(drops.shape[0], -1)
    if drops.ndim != 2 or thr.ndim != 2 or drops.shape[0] != thr.shape[0] or drops.shape[1] != thr.shape[1] + 1:
        raise ScpError(f"ring LOD: {tuple(drops.shape)} drops for {tuple(thr.shape)} thresholds: one more drop than thresholds per table expected")
    if drops.size and (not np.issubdtype(drops.dtype, np.integer) or drops.min() < 0 or drops.max() > 255):
        raise ScpError(f"ring LOD: drops are integers 0 .. {RINGLOD_MAX}")
    return np.ascontiguousarray(thr), np.ascontiguousarray(drops.astype(np.uint8))


def ringlod_cells(origins, thresholds, drops, start=0, level=None, segs=None, snapped=None):
    """scp_ringlod_cells: j = J(origin, s) per row of origins (cuda int32 [n,3]) under the integer rule of include/scp.h.  thresholds /
    drops: one table, or one per entry of a list (host integers); segs: None (every row table 0, s = start) or [(first row, count, depth,
    table)] - with level (cuda uint8 [n]: the rows' octree levels) s = depth - level + 1 per row.  snapped: None, True (a new tensor) or a
    cuda int32 [n,3] tensor (origins itself allowed) that receives (x >> j) << j.  -> j cuda uint8 [n], or (j, snapped)."""
    thr, dr = _ringlod_tables(thresholds, drops)
    n, dev = int(origins.shape[0]), origins.device
    if origins.dim() != 2 or origins.shape[1] != 3:
        raise ScpError(f"ringlod_cells: int32 [n,3] origins expected, got {tuple(origins.shape)}")
    seg = np.zeros(0, RINGLOD_SEG)
    if segs is not None:
        seg = np.zeros(len(segs), RINGLOD_SEG)
        for k, s in enumerate(segs):
            seg[k] = tuple(int(v) for v in s)
    if level is not None and tuple(level.shape) != (n,):
        raise ScpError("ringlod_cells: one level per row expected")
    ws_bytes = int(lib().scp_ringlod_workspace_bytes(thr.shape[0], seg.shape[0]))
    if ws_bytes < 0:
        raise ScpError(f"ringlod_cells: {thr.shape[0]} tables and {seg.shape[0]} segments: 1 .. {RINGLOD_MAX_TABLES} tables and at most "
                       f"{RINGLOD_MAX_TABLES} segments expected")
    j = torch.empty(n, dtype=torch.uint8, device=dev)
    out = torch.empty_like(origins) if snapped is True else snapped
    if out is not None and (out.shape != origins.shape or out.dtype != torch.int32):
        raise ScpError("ringlod_cells: snapped is an int32 tensor of the origins' shape")
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    rc = lib().scp_ringlod_cells(_dev(origins, torch.int32), n, int(start), None if level is None else _dev(level, torch.uint8),
                                 seg.ctypes.data if seg.shape[0] else None, seg.shape[0], thr.ctypes.data if thr.size else None,
                                 dr.ctypes.data, thr.shape[0], dr.shape[1], _dev(j), None if out is None else _dev(out), ws.data_ptr(),
                                 ws_bytes, _stream())
    _check(rc, "scp_ringlod_cells")
    return j if out is None else (j, out)


def force_rows(table, mask, sym=None, mismatch=None):
    """scp_force_rows: the rows of table (cuda f32 [n,nsym], row stride allowed) whose mask (cuda uint8 [n]) is set become (0, -1000,
    -1000, ...), in place.  sym (cuda uint8 [n]) with mismatch (cuda int64 [1], zeroed by the caller): the counter grows by the masked rows
    whose symbol is not 0.  -> table."""
    n, nsym = table.shape
    if not table.is_cuda or table.dtype != torch.float32 or table.stride(1) != 1 or tuple(mask.shape) != (n,):
        raise ScpError("force_rows: a device float32 table with unit column stride and one mask byte per row expected")
    if (sym is None) != (mismatch is None) or (sym is not None and (tuple(sym.shape) != (n,) or mismatch.numel() != 1)):
        raise ScpError("force_rows: symbols (one per row) and the mismatch counter (int64 [1]) go together")
    rc = lib().scp_force_rows(table.data_ptr(), _row_stride(table), n, nsym, _dev(mask, torch.uint8),
                              None if sym is None else _dev(sym, torch.uint8), None if mismatch is None else _dev(mismatch, torch.int64),
                              _stream())
    _check(rc, "scp_force_rows")
    return table


DIST_MAX_RINGS, DIST_MAX_BINS = 64, 4096                                   # include/scp.h: SCP_DIST_MAX_*
DIST_FLAG_AXIS, DIST_FLAG_GROUP_CLAMPED, DIST_FLAG_NO_NEIGHBOUR = 1, 2, 4  # include/scp.h: SCP_DIST_FLAG_*
# include/scp.h: scp_dist_seg, eight 8-byte fields and the 64 buckets of the histogram
DIST_FIELDS = ("rows", "axis_rows", "sum_sq", "sum_r2", "sum_phi2", "sum_theta2", "sum_r", "max_sq")
DIST_HIST = 64


def dist_edges(edges):
    """The ring edges of a distortion report as a tuple of floats: 0 = E_0 < E_1 < ..., finite, at most DIST_MAX_RINGS.  Host only."""
    try:
        e = tuple(float(v) for v in edges)
    except (TypeError, ValueError):
        raise ScpError(f"distortion report: ring edges are a list of numbers, got {edges!r}")
    if not e or e[0] != 0.0 or len(e) > DIST_MAX_RINGS or any(not (b > a) for a, b in zip(e, e[1:])) or not all(v * v < float("inf") for v in e):
        raise ScpError(f"distortion report: ring edges must start at 0, increase strictly, be finite and number at most {DIST_MAX_RINGS}, got {e}")
    return e


def _ring_args(fn, clouds, edges, group, n_groups, view):
    """The ring arguments of `fn` (nn_error_split, ring_bins), checked: the clouds, of which the first one is binned; the edges and the
    groups; the group of every point of the first cloud and its extremes (one read-back); the view.  -> (the clouds in float64, the
    arguments view, edges_sq, n_rings of the C entry point, the contiguous group tensor or None, n_groups)."""
    e = dist_edges(edges)
    n_groups = int(n_groups)
    if n_groups < 1 or n_groups * len(e) > DIST_MAX_BINS:
        raise ScpError(f"{fn}: {n_groups} groups x {len(e)} rings: between 1 and {DIST_MAX_BINS} bins expected")
    clouds = [_dev_f64(c) for c in clouds]
    if any(c.dim() != 2 or c.shape[1] != 3 or c.shape[0] < 1 for c in clouds):
        raise ScpError(f"{fn}: clouds of shape [n,3] with n >= 1 expected, got " + " and ".join(str(tuple(c.shape)) for c in clouds))
    n = clouds[0].shape[0]
    if group is not None:
        if not group.is_cuda or group.dtype != torch.int32 or tuple(group.shape) != (n,):
            raise ScpError(f"{fn}: group is a device int32 tensor with one entry per binned point ({n})")
        group = group.contiguous()
        lo, hi = int(group.min().item()), int(group.max().item())
        if lo < 0 or hi >= n_groups:
            raise ScpError(f"{fn}: group values {lo} .. {hi} outside 0 .. {n_groups - 1}")
    view = tuple(float(c) for c in view)
    if len(view) != 3 or not all(abs(c) < float("inf") for c in view):
        raise ScpError(f"{fn}: view is the sensor position, three finite numbers, got {view}")
    v = (C.c_double * 3)(*view)
    esq = (C.c_double * len(e))(*[c * c for c in e])
    return clouds, (C.cast(v, _vp), C.cast(esq, _vp), len(e)), group, n_groups


def nn_error_split(a, b, edges, group=None, n_groups=1, view=(0.0, 0.0, 0.0)):
    """scp_nn_error_split_f64 (csrc/distreport.hip).  a [na,3], b [nb,3] device tensors (compared in float64); edges: host list 0 = E_0 <
    E_1 < ..; group int32 [na] device tensor with 0 <= group < n_groups (None: all 0); view: the sensor, three host numbers.  -> dict of
    device tensors: idx int32 [na] (the LOWEST index among the nearest points of b), d2 float64 [na], comp float64 [na,3] (e_r, e_phi,
    e_theta of e = b[idx] - a), bin int32 [na] (group * len(edges) + ring), axis bool [na] (no local frame: on the sensor's axis), flag
    uint8 [na] (the DIST_FLAG_* bits).  Everything is checked before the launch; a group value out of range is refused here (one read-back
    of the group's extremes), and the kernel would clamp and flag it."""
    (a, b), ring, group, n_groups = _ring_args("nn_error_split", (a, b), edges, group, n_groups, view)
    na, dev = a.shape[0], a.device
    idx = torch.empty((na,), dtype=torch.int32, device=dev)
    d2 = torch.empty((na,), dtype=torch.float64, device=dev)
    comp = torch.empty((na, 3), dtype=torch.float64, device=dev)
    bin_ = torch.empty((na,), dtype=torch.int32, device=dev)
    flag = torch.empty((na,), dtype=torch.uint8, device=dev)
    _check(lib().scp_nn_error_split_f64(a.data_ptr(), na, b.data_ptr(), b.shape[0], *ring, None if group is None else group.data_ptr(), n_groups,
                                        idx.data_ptr(), d2.data_ptr(), comp.data_ptr(), bin_.data_ptr(), flag.data_ptr(), _stream()),
           "scp_nn_error_split_f64")
    return dict(idx=idx, d2=d2, comp=comp, bin=bin_, axis=(flag & DIST_FLAG_AXIS) != 0, flag=flag)


def _bin_order(bins, n_bins):
    """int32 bins [n] in any order -> (order int64 [n], seg_off int64 [n_bins + 1]): a stable sort brings every bin's rows together in
    index order, which the summation order contract needs; bin b owns order[seg_off[b] : seg_off[b + 1]]."""
    ordered, order = torch.sort(bins, stable=True)
    seg_off = torch.searchsorted(ordered, torch.arange(n_bins + 1, dtype=torch.int32, device=bins.device)).to(torch.int64).contiguous()
    return order, seg_off


def dist_segments(d2, comp, flag, bins, n_bins):
    """scp_dist_segments_f64: one record per bin 0 .. n_bins - 1 from the per-query tensors of nn_error_split (`flag`: its uint8 flags;
    `bins`: its int32 bins, in any order - a stable sort brings every bin's rows together in index order, which the summation order
    contract needs).  -> dict of device tensors, all views of `raw` int64 [n_bins, 72] (the scp_dist_seg records: one copy brings them all
    to the host): rows, axis_rows int64 [n_bins]; sum_sq, sum_r2, sum_phi2, sum_theta2, sum_r, max_sq float64 [n_bins]; hist int64
    [n_bins, 64].  A bin without rows is all zeros; a row whose bin lies outside 0 .. n_bins - 1 belongs to no record."""
    n_bins = int(n_bins)
    if n_bins < 1 or n_bins > DIST_MAX_BINS:
        raise ScpError(f"dist_segments: between 1 and {DIST_MAX_BINS} bins expected, got {n_bins}")
    for t, dt, name in ((d2, torch.float64, "d2"), (comp, torch.float64, "comp"), (flag, torch.uint8, "flag"), (bins, torch.int32, "bins")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
            raise ScpError(f"dist_segments: {name} is a device tensor of {dt} (there is no CPU path in the product)")
    n = d2.shape[0]
    if n < 1 or tuple(d2.shape) != (n,) or tuple(comp.shape) != (n, 3) or tuple(flag.shape) != (n,) or tuple(bins.shape) != (n,):
        raise ScpError(f"dist_segments: d2 [n], comp [n,3], flag [n], bins [n] with n >= 1 expected, got {tuple(d2.shape)}, {tuple(comp.shape)}, "
                       f"{tuple(flag.shape)}, {tuple(bins.shape)}")
    d2, comp, flag = d2.contiguous(), comp.contiguous(), flag.contiguous()
    order, seg_off = _bin_order(bins, n_bins)
    raw = torch.empty((n_bins, len(DIST_FIELDS) + DIST_HIST), dtype=torch.int64, device=d2.device)
    _check(lib().scp_dist_segments_f64(d2.data_ptr(), comp.data_ptr(), flag.data_ptr(), order.data_ptr(), n, seg_off.data_ptr(), n_bins,
                                       raw.data_ptr(), _stream()), "scp_dist_segments_f64")
    return dict(dist_record_views(raw), raw=raw)


def dist_record_views(raw):
    """The fields of scp_dist_seg records held as int64 [n_bins, 72] (a torch tensor or a numpy array, device or host) -> dict of views."""
    f64 = (lambda c: c.view(torch.float64)) if isinstance(raw, torch.Tensor) else (lambda c: c.view(np.float64))
    out = {}
    for k, name in enumerate(DIST_FIELDS):
        col = raw[:, k]
        out[name] = col if name in ("rows", "axis_rows") else f64(col)
    out["hist"] = raw[:, len(DIST_FIELDS):]
    return out


# ------------------------------------------------------------------------------------------------- rate per ring, depth report (csrc/ringrate.hip)
SHARE_FIELDS = ("leaves", "ideal_bits", "table_bits", "max_ideal_bits")     # include/scp.h: scp_share_seg, four 8-byte fields
MAX_SEGMENTS = 62                                                           # include/scp.h: SCP_MAX_SEGMENTS


def share_table(infos):
    """The per-segment table of rate_leaf_share from the SegmentInfo list of a Geom build (`Geom.info`): numpy int64 [S,4] = (node_base,
    n_nodes, depth, leaf_base), the leaves of the segments back to back in segment order.  Host only."""
    tab, leaf = np.zeros((len(infos), 4), np.int64), 0
    for s, i in enumerate(infos):
        tab[s] = (int(i.node_base), int(i.n_nodes), int(i.depth), leaf)
        leaf += int(i.n_leaves)
    return tab


def node_bits(order, node_of_row, row_ideal, row_table, total_nodes):
    """Per-row bits in CODING order -> per-node bits (index plumbing, torch): order int64 [R] = the frame-order row of every coded
    position (EncodePlan.coding_order_device), node_of_row int64 [R] = the node of every frame-order row (a drop_last segment's last
    node has no row), row_ideal / row_table float64 [R] (rate_segments(..., want_rows=True)).  -> (ideal, table) float64 [total_nodes],
    0 for a node without a row."""
    R = int(order.shape[0])
    if tuple(node_of_row.shape) != (R,) or tuple(row_ideal.shape) != (R,) or tuple(row_table.shape) != (R,):
        raise ScpError(f"node_bits: {R} coded positions, but {tuple(node_of_row.shape)} rows and {tuple(row_ideal.shape)} / {tuple(row_table.shape)} bits")
    node = node_of_row[order]
    ideal = torch.zeros(total_nodes, dtype=torch.float64, device=row_ideal.device)
    table = torch.zeros(total_nodes, dtype=torch.float64, device=row_ideal.device)
    ideal[node] = row_ideal
    table[node] = row_table
    return ideal, table


def _tree_pass(fn, occ, level, parent, bits_ideal, bits_table, segs, total_leaves, max_drop=None):
    """The tree pass of rate_leaf_share (max_drop None: scp_rate_leaf_share, costs [total_leaves]) and of rate_depth_share
    (scp_rate_depth_share, costs [max_drop + 1, total_leaves]): the five node columns and the [S,4] table checked, the workspace and the
    outputs made, the entry point called.  `fn` names the caller in messages and, behind `scp_`, its C entry point."""
    N = int(occ.shape[0])
    for t, dt, name in ((occ, torch.uint8, "occ"), (level, torch.uint8, "level"), (parent, torch.int32, "parent"),
                        (bits_ideal, torch.float64, "bits_ideal"), (bits_table, torch.float64, "bits_table")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != (N,):
            raise ScpError(f"{fn}: {name} is a device tensor of {dt} with one entry per node ({N})")
    segs = np.ascontiguousarray(segs, np.int64)
    if segs.ndim != 2 or segs.shape[1] != 4:
        raise ScpError(f"{fn}: the segment table is int64 [S,4] (node_base, n_nodes, depth, leaf_base), got {segs.shape}")
    planes = ()
    if max_drop is not None:
        max_drop = int(max_drop)
        if max_drop < 0 or max_drop > MAX_DEPTH:
            raise ScpError(f"{fn}: max_drop {max_drop} outside 0 .. {MAX_DEPTH}")
        planes = (max_drop + 1,)
    S, total_leaves = int(segs.shape[0]), int(total_leaves)
    ws_bytes = int(getattr(lib(), f"scp_{fn}_workspace_bytes")(N, S))
    if ws_bytes < 0:
        raise ScpError(f"{fn}: {N} nodes in {S} segments: 1 .. 2^30 nodes in 1 .. {MAX_SEGMENTS} segments expected")
    dev = occ.device
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    leaves = torch.empty(N, dtype=torch.int64, device=dev)
    ci = torch.empty(planes + (max(total_leaves, 0),), dtype=torch.float64, device=dev)
    ct = torch.empty(planes + (max(total_leaves, 0),), dtype=torch.float64, device=dev)
    rc = getattr(lib(), f"scp_{fn}")(_dev(occ), _dev(level), _dev(parent), N, _dev(bits_ideal), _dev(bits_table), segs.ctypes.data, S, total_leaves,
                                     *(() if max_drop is None else (max_drop,)), leaves.data_ptr(), ci.data_ptr(), ct.data_ptr(), ws.data_ptr(),
                                     ws_bytes, _stream())
    _check(rc, f"scp_{fn}")
    return dict(leaves=leaves, cost_ideal=ci, cost_table=ct)


def rate_leaf_share(occ, level, parent, bits_ideal, bits_table, segs, total_leaves):
    """scp_rate_leaf_share: every leaf's share of its ancestors' bits (include/scp.h states the definition).  occ / level uint8, parent
    int32, bits_ideal / bits_table float64: device tensors [N], the node columns of all segments of a build (Geom.nodes) and what every
    node cost; segs: host int64 [S,4] (node_base, n_nodes, depth, leaf_base) - share_table(geom.info).  -> dict of device tensors: leaves
    int64 [N], cost_ideal / cost_table float64 [total_leaves] (segment-major, the order of Geom.leaves inside a segment).  A table the
    library's validation pass objects to raises ScpError (SCP_EINVAL); the call waits for the stream once."""
    return _tree_pass("rate_leaf_share", occ, level, parent, bits_ideal, bits_table, segs, total_leaves)


def rate_depth_share(occ, level, parent, bits_ideal, bits_table, segs, total_leaves, max_drop):
    """scp_rate_depth_share: every leaf's share of the bits of levels 1 .. D - k for k = 0 .. max_drop (include/scp.h states the
    definition); the arguments of rate_leaf_share plus max_drop (0 .. MAX_DEPTH).  -> dict of device tensors: leaves int64 [N],
    cost_ideal / cost_table float64 [max_drop + 1, total_leaves] (plane k = cost_k; plane 0 = rate_leaf_share's costs bit for bit; a plane
    with k >= a segment's depth holds +0.0 there).  A table the library's validation pass objects to raises ScpError (SCP_EINVAL)."""
    return _tree_pass("rate_depth_share", occ, level, parent, bits_ideal, bits_table, segs, total_leaves, max_drop)


def ring_bins(xyz, edges, group=None, n_groups=1, view=(0.0, 0.0, 0.0)):
    """scp_ring_bins_f64: the (group, ring) bin of every point of a cloud [n,3] (device, compared in float64) - the bins nn_error_split
    gives its queries, integer for integer; edges / group / n_groups / view as there.  -> device int32 [n]."""
    (a,), ring, group, n_groups = _ring_args("ring_bins", (xyz,), edges, group, n_groups, view)
    n = a.shape[0]
    bin_ = torch.empty((n,), dtype=torch.int32, device=a.device)
    _check(lib().scp_ring_bins_f64(a.data_ptr(), n, *ring, None if group is None else group.data_ptr(), n_groups, bin_.data_ptr(), None, _stream()),
           "scp_ring_bins_f64")
    return bin_


def _share_segments(fn, cost_ideal, cost_table, bins, n_bins, planes):
    """share_segments (planes False: costs [n], scp_share_segments_f64) and share_segments_depth (costs [K, n], one launch of
    scp_share_segments_depth_f64) -> dict of views of `raw` int64 [n_bins, 4] / [K, n_bins, 4], and raw."""
    n_bins = int(n_bins)
    if n_bins < 1 or n_bins > DIST_MAX_BINS:
        raise ScpError(f"{fn}: between 1 and {DIST_MAX_BINS} bins expected, got {n_bins}")
    for t, dt, name in ((cost_ideal, torch.float64, "cost_ideal"), (cost_table, torch.float64, "cost_table"), (bins, torch.int32, "bins")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
            raise ScpError(f"{fn}: {name} is a device tensor of {dt} (there is no CPU path in the product)")
    want = "[K, n]" if planes else "[n]"
    if cost_ideal.dim() != 1 + planes or cost_ideal.shape[-1] < 1 or cost_table.shape != cost_ideal.shape or tuple(bins.shape) != (cost_ideal.shape[-1],):
        raise ScpError(f"{fn}: cost_ideal {want}, cost_table {want}, bins [n] with n >= 1 expected, got {tuple(cost_ideal.shape)}, "
                       f"{tuple(cost_table.shape)}, {tuple(bins.shape)}")
    n = int(cost_ideal.shape[-1])
    if planes and not 1 <= cost_ideal.shape[0] <= MAX_DEPTH + 1:
        raise ScpError(f"{fn}: between 1 and {MAX_DEPTH + 1} planes expected, got {cost_ideal.shape[0]}")
    cost_ideal, cost_table = cost_ideal.contiguous(), cost_table.contiguous()
    order, seg_off = _bin_order(bins, n_bins)
    raw = torch.empty(tuple(cost_ideal.shape[:-1]) + (n_bins, len(SHARE_FIELDS)), dtype=torch.int64, device=cost_ideal.device)
    args = (cost_ideal.data_ptr(), cost_table.data_ptr(), order.data_ptr(), n, seg_off.data_ptr(), n_bins)
    if planes:
        _check(lib().scp_share_segments_depth_f64(*args, int(cost_ideal.shape[0]), n, raw.data_ptr(), _stream()), "scp_share_segments_depth_f64")
    else:
        _check(lib().scp_share_segments_f64(*args, raw.data_ptr(), _stream()), "scp_share_segments_f64")
    return dict(share_record_views(raw), raw=raw)


def share_segments(cost_ideal, cost_table, bins, n_bins):
    """scp_share_segments_f64: one record per bin 0 .. n_bins - 1 from the leaf costs of rate_leaf_share and the leaves' bins (int32, any
    order: a stable sort brings every bin's rows together in index order, which the summation contract needs).  -> dict of device tensors,
    views of `raw` int64 [n_bins, 4] (the scp_share_seg records: one copy brings them all to the host): leaves int64, ideal_bits,
    table_bits, max_ideal_bits float64 [n_bins].  A bin without rows is all zeros; a row whose bin lies outside 0 .. n_bins - 1 belongs to
    no record."""
    return _share_segments("share_segments", cost_ideal, cost_table, bins, n_bins, False)


def share_record_views(raw):
    """The fields of scp_share_seg records held as int64 [.., n_bins, 4] (a torch tensor or a numpy array, device or host) -> dict of views."""
    f64 = (lambda c: c.view(torch.float64)) if isinstance(raw, torch.Tensor) else (lambda c: c.view(np.float64))
    return {name: (raw[..., k] if name == "leaves" else f64(raw[..., k])) for k, name in enumerate(SHARE_FIELDS)}


def share_segments_depth(cost_ideal, cost_table, bins, n_bins):
    """scp_share_segments_depth_f64: share_segments on every plane of cost_ideal / cost_table [K, n] (rate_depth_share) in one launch; the
    leaves' bins (int32 [n]) are the same for every plane.  -> dict of device tensors, views of `raw` int64 [K, n_bins, 4]: leaves int64,
    ideal_bits, table_bits, max_ideal_bits float64 [K, n_bins]; raw[0] is share_segments' raw on plane 0, field for field."""
    return _share_segments("share_segments_depth", cost_ideal, cost_table, bins, n_bins, True)


# ------------------------------------------------------------------------------------------------- reflectance layer (csrc/attr.hip)
ATTR_ALPHABET = 511                                                        # z = 2 |k| - (k > 0), |k| <= 255


def _attr_workspace(fn, dev, *args):
    n = _check(getattr(lib(), fn)(*args), fn)
    return torch.empty(max(int(n), 8) // 8 + 1, dtype=torch.int64, device=dev), int(n)


def _attr_leaves(leaves, who):
    if leaves.dim() != 2 or leaves.shape[1] != 3:
        raise ScpError(f"{who}: leaves of shape [U,3] expected, got {tuple(leaves.shape)}")
    _dev(leaves, torch.int32)
    return leaves


def attr_leaf_values(q, refl, leaves, depth, scale):
    """scp_attr_leaf_values: q device int32 [P,3] (the quantised points of the shell), refl device float32 [P], leaves device int32 [U,3]
    in the order of Geom.leaves -> (a uint8 [U], cnt int32 [U]): the rounded mean of the 8-bit point values that fall on every leaf."""
    leaves = _attr_leaves(leaves, "attr_leaf_values")
    if q.dim() != 2 or q.shape[1] != 3 or refl.dim() != 1 or refl.shape[0] != q.shape[0]:
        raise ScpError(f"attr_leaf_values: q [P,3] and refl [P] expected, got {tuple(q.shape)} and {tuple(refl.shape)}")
    U, dev = leaves.shape[0], leaves.device
    a = torch.empty(U, dtype=torch.uint8, device=dev)
    cnt = torch.empty(U, dtype=torch.int32, device=dev)
    ws, nb = _attr_workspace("scp_attr_leaf_values_workspace_bytes", dev, U)
    _check(lib().scp_attr_leaf_values(_dev(q, torch.int32), _dev(refl, torch.float32), q.shape[0], leaves.data_ptr(), U, int(depth), int(scale),
                                      a.data_ptr(), cnt.data_ptr(), ws.data_ptr(), nb, _stream()), "scp_attr_leaf_values")
    return a, cnt


def attr_forward(leaves, a, depth, Q):
    """scp_attr_forward: leaves device int32 [U,3], a device uint8 [U] -> dict of device tensors: k int16 [U - 1] and ctx uint8 [U - 1] in
    coding order (ctx = level - 1), root int32 [1], hist int32 [depth, 511], level_counts int64 [depth + 1]."""
    leaves = _attr_leaves(leaves, "attr_forward")
    U, dev, depth = leaves.shape[0], leaves.device, int(depth)
    if a.shape != (U,):
        raise ScpError(f"attr_forward: one value per leaf expected, got {tuple(a.shape)} for {U} leaves")
    if not 1 <= depth <= MAX_DEPTH:
        raise ScpError(f"attr_forward: depth {depth} outside 1 .. {MAX_DEPTH}")
    k = torch.empty(max(U - 1, 0), dtype=torch.int16, device=dev)
    ctx = torch.empty(max(U - 1, 0), dtype=torch.uint8, device=dev)
    root = torch.empty(1, dtype=torch.int32, device=dev)
    hist = torch.empty((depth, ATTR_ALPHABET), dtype=torch.int32, device=dev)
    counts = torch.empty(depth + 1, dtype=torch.int64, device=dev)
    ws, nb = _attr_workspace("scp_attr_forward_workspace_bytes", dev, U, depth)
    _check(lib().scp_attr_forward(leaves.data_ptr(), _dev(a, torch.uint8), U, depth, int(Q), k.data_ptr(), ctx.data_ptr(), root.data_ptr(),
                                  hist.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb, _stream()), "scp_attr_forward")
    return dict(k=k, ctx=ctx, root=root, hist=hist, level_counts=counts)


def attr_pairs(k, ctx, tables):
    """scp_attr_pairs: k int16 [n], ctx uint8 [n], tables uint16 [depth, 512] (all device; torch has the rows as int16) -> lohi int32 [n],
    the (c_low, c_high) pairs ac_encode_lohi takes."""
    if tables.dim() != 2 or tables.shape[1] != ATTR_ALPHABET + 1 or not 1 <= tables.shape[0] <= MAX_DEPTH:
        raise ScpError(f"attr_pairs: tables of shape [depth, {ATTR_ALPHABET + 1}] expected, got {tuple(tables.shape)}")
    if k.shape != ctx.shape or k.dim() != 1:
        raise ScpError("attr_pairs: one context per coefficient expected")
    lohi = torch.empty(k.shape[0], dtype=torch.int32, device=k.device)
    _check(lib().scp_attr_pairs(_dev(k, torch.int16), _dev(ctx, torch.uint8), k.shape[0], _dev(tables, torch.int16), tables.shape[0],
                                lohi.data_ptr(), _stream()), "scp_attr_pairs")
    return lohi


def attr_level_counts(leaves, depth):
    """scp_attr_level_counts: leaves device int32 [U,3] -> level_counts device int64 [depth + 1] (n_0 = U .. n_depth = 1)."""
    leaves = _attr_leaves(leaves, "attr_level_counts")
    U, dev, depth = leaves.shape[0], leaves.device, int(depth)
    counts = torch.empty(max(depth, 0) + 1, dtype=torch.int64, device=dev)
    ws, nb = _attr_workspace("scp_attr_inverse_workspace_bytes", dev, U, depth)
    _check(lib().scp_attr_level_counts(leaves.data_ptr(), U, depth, counts.data_ptr(), ws.data_ptr(), nb, _stream()), "scp_attr_level_counts")
    return counts


def attr_inverse(leaves, depth, Q, root, k):
    """scp_attr_inverse: leaves device int32 [U,3], the root value (host int) and k device int16 [U - 1] in coding order -> a uint8 [U]."""
    leaves = _attr_leaves(leaves, "attr_inverse")
    U, dev, depth = leaves.shape[0], leaves.device, int(depth)
    if k.shape != (max(U - 1, 0),):
        raise ScpError(f"attr_inverse: {max(U - 1, 0)} coefficients expected for {U} leaves, got {tuple(k.shape)}")
    a = torch.empty(U, dtype=torch.uint8, device=dev)
    ws, nb = _attr_workspace("scp_attr_inverse_workspace_bytes", dev, U, depth)
    _check(lib().scp_attr_inverse(leaves.data_ptr(), U, depth, int(Q), int(root), _dev(k, torch.int16), a.data_ptr(), ws.data_ptr(), nb, _stream()),
           "scp_attr_inverse")
    return a


# ------------------------------------------------------------------------------------------------- colour layer (csrc/color.hip)
COLOR_ALPHABET = 1021                                                      # z = 2 |k| - (k > 0), |k| <= 510 (Co / Cg differences)


def color_leaf_values(q, rgb, leaves, depth):
    """scp_color_leaf_values: q device int32 [P,3], rgb device uint8 [P,3], leaves device int32 [U,3] in the order of Geom.leaves ->
    (rgb_mean uint8 [U,3], ycc int16 [3,U] - the YCoCg-R image of the means, planar -, cnt int32 [U])."""
    leaves = _attr_leaves(leaves, "color_leaf_values")
    if q.dim() != 2 or q.shape[1] != 3 or rgb.shape != q.shape:
        raise ScpError(f"color_leaf_values: q [P,3] and rgb [P,3] expected, got {tuple(q.shape)} and {tuple(rgb.shape)}")
    U, dev = leaves.shape[0], leaves.device
    mean = torch.empty((U, 3), dtype=torch.uint8, device=dev)
    ycc = torch.empty((3, U), dtype=torch.int16, device=dev)
    cnt = torch.empty(U, dtype=torch.int32, device=dev)
    ws, nb = _attr_workspace("scp_color_leaf_values_workspace_bytes", dev, U)
    _check(lib().scp_color_leaf_values(_dev(q, torch.int32), _dev(rgb, torch.uint8), q.shape[0], leaves.data_ptr(), U, int(depth), mean.data_ptr(),
                                       ycc.data_ptr(), cnt.data_ptr(), ws.data_ptr(), nb, _stream()), "scp_color_leaf_values")
    return mean, ycc, cnt


def color_forward(leaves, ycc, depth, Q):
    """scp_color_forward: leaves device int32 [U,3], ycc device int16 [3,U] -> dict of device tensors: k int16 [3, U - 1] (every plane in
    coding order), ctx uint8 [U - 1] (level - 1, shared by the planes), root int32 [3], hist int32 [3 depth, 1021] (row channel * depth +
    level - 1), level_counts int64 [depth + 1]."""
    leaves = _attr_leaves(leaves, "color_forward")
    U, dev, depth = leaves.shape[0], leaves.device, int(depth)
    if ycc.shape != (3, U):
        raise ScpError(f"color_forward: ycc [3,{U}] expected for {U} leaves, got {tuple(ycc.shape)}")
    if not 1 <= depth <= MAX_DEPTH:
        raise ScpError(f"color_forward: depth {depth} outside 1 .. {MAX_DEPTH}")
    k = torch.empty((3, max(U - 1, 0)), dtype=torch.int16, device=dev)
    ctx = torch.empty(max(U - 1, 0), dtype=torch.uint8, device=dev)
    root = torch.empty(3, dtype=torch.int32, device=dev)
    hist = torch.empty((3 * depth, COLOR_ALPHABET), dtype=torch.int32, device=dev)
    counts = torch.empty(depth + 1, dtype=torch.int64, device=dev)
    ws, nb = _attr_workspace("scp_color_forward_workspace_bytes", dev, U, depth)
    _check(lib().scp_color_forward(leaves.data_ptr(), _dev(ycc, torch.int16), U, depth, int(Q), k.data_ptr(), ctx.data_ptr(), root.data_ptr(),
                                   hist.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb, _stream()), "scp_color_forward")
    return dict(k=k, ctx=ctx, root=root, hist=hist, level_counts=counts)


def color_pairs(k, ctx, tables):
    """scp_color_pairs: k int16 [3,n], ctx uint8 [n], tables uint16 [3 depth, 1022] (all device; torch has the rows as int16) -> lohi int32
    [3 n] in payload order (Y, Co, Cg), the (c_low, c_high) pairs ac_encode_lohi takes."""
    if tables.dim() != 2 or tables.shape[1] != COLOR_ALPHABET + 1 or tables.shape[0] % 3 or not 1 <= tables.shape[0] // 3 <= MAX_DEPTH:
        raise ScpError(f"color_pairs: tables of shape [3 depth, {COLOR_ALPHABET + 1}] expected, got {tuple(tables.shape)}")
    if k.dim() != 2 or ctx.dim() != 1 or k.shape != (3, ctx.shape[0]):
        raise ScpError("color_pairs: k [3,n] and one context per coefficient of a plane expected")
    lohi = torch.empty(3 * ctx.shape[0], dtype=torch.int32, device=k.device)
    _check(lib().scp_color_pairs(_dev(k, torch.int16), _dev(ctx, torch.uint8), ctx.shape[0], _dev(tables, torch.int16), tables.shape[0] // 3,
                                 lohi.data_ptr(), _stream()), "scp_color_pairs")
    return lohi


def color_inverse(leaves, depth, Q, root, k):
    """scp_color_inverse: leaves device int32 [U,3], the roots (three host ints: Y, Co, Cg) and k device int16 [3, U - 1] -> rgb uint8 [U,3]."""
    leaves = _attr_leaves(leaves, "color_inverse")
    U, dev, depth = leaves.shape[0], leaves.device, int(depth)
    if k.shape != (3, max(U - 1, 0)):
        raise ScpError(f"color_inverse: coefficients [3,{max(U - 1, 0)}] expected for {U} leaves, got {tuple(k.shape)}")
    r = (C.c_int32 * 3)(*[int(v) for v in root])
    rgb = torch.empty((U, 3), dtype=torch.uint8, device=dev)
    ws, nb = _attr_workspace("scp_color_inverse_workspace_bytes", dev, U, depth)
    _check(lib().scp_color_inverse(leaves.data_ptr(), U, depth, int(Q), C.cast(r, _vp), _dev(k, torch.int16), rgb.data_ptr(), ws.data_ptr(), nb, _stream()),
           "scp_color_inverse")
    return rgb


# ------------------------------------------------------------------------------------------------- step sweep (csrc/lift.h)
SWEEP_MAX_STEPS = 16                                                       # include/scp.h: SCP_SWEEP_MAX_STEPS
SWEEP_STEPS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 255)


def sweep_steps(steps=None):
    """The grid of steps of a sweep as numpy int32 [G].  None: SWEEP_STEPS.  A grid holds 1 .. SWEEP_MAX_STEPS integers in 1 .. 255,
    strictly ascending."""
    raw = list(SWEEP_STEPS if steps is None else steps)
    if not 1 <= len(raw) <= SWEEP_MAX_STEPS:
        raise ScpError(f"sweep steps: {len(raw)} steps, 1 .. {SWEEP_MAX_STEPS} expected")
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in raw):
        raise ScpError(f"sweep steps: integers expected, got {raw}")
    g = np.array([int(v) for v in raw], np.int64)
    if (g < 1).any() or (g > 255).any():
        raise ScpError(f"sweep steps: every step is 1 .. 255, got {g.tolist()}")
    if (np.diff(g) <= 0).any():
        raise ScpError(f"sweep steps: strictly ascending steps expected, got {g.tolist()}")
    return np.ascontiguousarray(g.astype(np.int32))


def _sweep(fn, channels, outs, alphabet, leaves, depth, steps, *values):
    U, dev, depth = leaves.shape[0], leaves.device, int(depth)
    if not 1 <= depth <= MAX_DEPTH:
        raise ScpError(f"{fn}: depth {depth} outside 1 .. {MAX_DEPTH}")
    g = sweep_steps(steps)
    G = int(g.shape[0])
    hist = torch.empty((G, channels * depth, alphabet), dtype=torch.int32, device=dev)
    sse = torch.empty((G, outs), dtype=torch.int64, device=dev)             # uint64 on the device; a sum stays far below 2^63
    linf = torch.empty((G, outs), dtype=torch.int32, device=dev)
    root = torch.empty(channels, dtype=torch.int32, device=dev)
    counts = torch.empty(depth + 1, dtype=torch.int64, device=dev)
    ws, nb = _attr_workspace(f"scp_{fn}_workspace_bytes", dev, U, depth, G)
    _check(getattr(lib(), f"scp_{fn}")(leaves.data_ptr(), *values, U, depth, g.ctypes.data, G, hist.data_ptr(), sse.data_ptr(), linf.data_ptr(),
                                       root.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb, _stream()), f"scp_{fn}")
    return dict(steps=g, hist=hist, sse=sse, linf=linf, root=root, level_counts=counts)


def attr_sweep(leaves, a, depth, steps=None):
    """scp_attr_sweep: leaves device int32 [U,3], a device uint8 [U], steps (sweep_steps) -> dict: steps numpy int32 [G] and the device
    tensors hist int32 [G, depth, 511] (row g: attr_forward's hist at Q = steps[g]), sse int64 [G, 1] and linf int32 [G, 1] (the squared
    and the largest error of attr_inverse's leaf values at that step against a), root int32 [1], level_counts int64 [depth + 1]."""
    leaves = _attr_leaves(leaves, "attr_sweep")
    if a.shape != (leaves.shape[0],):
        raise ScpError(f"attr_sweep: one value per leaf expected, got {tuple(a.shape)} for {leaves.shape[0]} leaves")
    return _sweep("attr_sweep", 1, 1, ATTR_ALPHABET, leaves, depth, steps, _dev(a, torch.uint8))


def color_sweep(leaves, ycc, rgb_mean, depth, steps=None):
    """scp_color_sweep: leaves device int32 [U,3], ycc int16 [3,U] and rgb_mean uint8 [U,3] as color_leaf_values returns them, steps
    (sweep_steps) -> dict: steps numpy int32 [G] and the device tensors hist int32 [G, 3 depth, 1021] (row g: color_forward's hist at
    Q = steps[g]), sse int64 [G, 3] and linf int32 [G, 3] (R, G, B: color_inverse's leaf colours at that step against rgb_mean), root
    int32 [3], level_counts int64 [depth + 1]."""
    leaves = _attr_leaves(leaves, "color_sweep")
    U = leaves.shape[0]
    if ycc.shape != (3, U) or rgb_mean.shape != (U, 3):
        raise ScpError(f"color_sweep: ycc [3,{U}] and rgb_mean [{U},3] expected, got {tuple(ycc.shape)} and {tuple(rgb_mean.shape)}")
    return _sweep("color_sweep", 3, 3, COLOR_ALPHABET, leaves, depth, steps, _dev(ycc, torch.int16), _dev(rgb_mean, torch.uint8))


# ------------------------------------------------------------------------------------------------- range coder (host)
def ac_encode_cdf(cdf, sym):
    """cdf uint16/int16 numpy [n,Lp], sym int16 numpy [n] -> bytes."""
    cdf = np.ascontiguousarray(cdf).view(np.uint16)
    sym = np.ascontiguousarray(sym, np.int16)
    cap = len(sym) * 4 + 64
    while True:
        out = np.empty(cap, np.uint8)
        n = C.c_size_t(0)
        rc = lib().scp_ac_encode_cdf(cdf.ctypes.data, sym.ctypes.data, len(sym), cdf.shape[1], out.ctypes.data, cap,
                                     C.byref(n))
        if rc == -3:
            cap *= 4
            continue
        _check(rc, "scp_ac_encode_cdf")
        return out[: n.value].tobytes()


def ac_encode_lohi(lohi):
    """lohi uint32/int32 numpy [n] (low 16 = c_low, high 16 = c_high, 0 => 65536) -> bytes."""
    lohi = np.ascontiguousarray(lohi).view(np.uint32)
    cap = len(lohi) * 4 + 64
    while True:
        out = np.empty(cap, np.uint8)
        n = C.c_size_t(0)
        rc = lib().scp_ac_encode_lohi(lohi.ctypes.data, len(lohi), out.ctypes.data, cap, C.byref(n))
        if rc == -3:
            cap *= 4
            continue
        _check(rc, "scp_ac_encode_lohi")
        return out[: n.value].tobytes()


# ------------------------------------------------------------------------------------------------- chunk-parallel range coder (csrc/ac_chunks.hip)
CHUNK_MIN, CHUNK_MAX, CHUNK_DEFAULT = 64, 1 << 20, 4096


def check_chunk(N, who="chunk size"):
    """The chunk size of a chunked payload as an int; outside 64 .. 2^20 symbols it is refused."""
    if isinstance(N, bool) or int(N) != N or not CHUNK_MIN <= int(N) <= CHUNK_MAX:
        raise ScpError(f"{who} {N}: {CHUNK_MIN} .. 2^20 symbols per chunk expected")
    return int(N)


def ac_chunks_encode(lohi_dev, N, cap=None):
    """scp_ac_chunks_encode_lohi: lohi device int32 [n] (the pairs ac_encode_lohi takes), N symbols per chunk -> (lengths numpy uint32 [C],
    the C chunks back to back as bytes): chunk c is ac_encode_lohi(lohi[c N:(c + 1) N]), byte for byte, all chunks coded at once on the
    device.  One wait (the lengths), then exactly the packed bytes cross; the pairs stay on the device.  cap: the size of the device
    buffer the chunks are packed into (default: the slots' bound, which cannot be too small); SCP_ESMALL when they do not fit."""
    N = check_chunk(N)
    if lohi_dev.dim() != 1 or lohi_dev.dtype != torch.int32:
        raise ScpError(f"ac_chunks_encode: pairs int32 [n] expected, got {lohi_dev.dtype} {tuple(lohi_dev.shape)}")
    n, dev = lohi_dev.shape[0], lohi_dev.device
    nchunks = -(-n // N)
    nb = _check(lib().scp_ac_chunks_workspace_bytes(n, N), "scp_ac_chunks_workspace_bytes")
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=dev)
    cap = nb if cap is None else int(cap)
    out = torch.empty(cap // 4 + 1, dtype=torch.int32, device=dev)
    head = torch.empty(nchunks + 1, dtype=torch.int32, device=dev)          # the lengths, then the status word
    _check(lib().scp_ac_chunks_encode_lohi(_dev(lohi_dev), n, N, head.data_ptr(), out.data_ptr(), cap, head.data_ptr() + 4 * nchunks, ws.data_ptr(), nb,
                                           _stream()), "scp_ac_chunks_encode_lohi")
    h = head.cpu().numpy()
    _check(int(h[nchunks]), "scp_ac_chunks_encode_lohi")
    lengths = h[:nchunks].view(np.uint32).copy()
    total = int(lengths.sum(dtype=np.int64))
    return lengths, out.view(torch.uint8)[:total].cpu().numpy().tobytes()


def ac_chunks_decode(payload_bytes, lengths, N, tables, table_of, ctx_dev, Lp):
    """scp_ac_chunks_decode_ctx: the chunk bytes back to back, their lengths (C integers), N symbols per chunk, tables uint16 / int16 numpy
    [ntab, Lp], table_of (nctx table indices), ctx device uint8 [n] -> device int16 [n]: symbol i decoded against row table_of[ctx[i]],
    chunk c being what AcDecoder(chunk c, Lp).run_ctx returns on its contexts; all chunks at once on the device.  A length table that
    does not have ceil(n / N) entries or does not add up to the bytes, a context >= nctx and a table index >= ntab are refused."""
    N = check_chunk(N)
    tables = np.ascontiguousarray(tables).view(np.uint16)
    table_of = np.ascontiguousarray(table_of, np.int64).reshape(-1)
    if tables.ndim != 2 or tables.shape[1] != int(Lp) or tables.shape[0] < 1:
        raise ScpError(f"ac_chunks_decode: tables of shape [ntab, {Lp}] expected, got {tables.shape}")
    if ctx_dev.dim() != 1 or ctx_dev.dtype != torch.uint8:
        raise ScpError(f"ac_chunks_decode: contexts uint8 [n] expected, got {ctx_dev.dtype} {tuple(ctx_dev.shape)}")
    n, dev = ctx_dev.shape[0], ctx_dev.device
    nchunks = -(-n // N)
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    data = np.frombuffer(bytes(payload_bytes), np.uint8)
    if lengths.shape[0] != nchunks:
        raise ScpError(f"ac_chunks_decode: {lengths.shape[0]} chunk lengths for {n} symbols in chunks of {N}: {nchunks} expected")
    if (lengths < 0).any() or int(lengths.sum()) != data.shape[0]:
        raise ScpError(f"ac_chunks_decode: the chunk lengths add up to {int(lengths.sum())}, the chunks hold {data.shape[0]} bytes")
    nctx, ntab = table_of.shape[0], tables.shape[0]
    if not 1 <= nctx <= 256 or (table_of < 0).any() or (table_of >= ntab).any():
        raise ScpError(f"ac_chunks_decode: 1 .. 256 contexts with a table index below {ntab} each expected, got {table_of.tolist()}")
    sym = torch.empty(n, dtype=torch.int16, device=dev)
    if n == 0:
        return sym
    top = int(ctx_dev.max().item())
    if top >= nctx:
        raise ScpError(f"ac_chunks_decode: context {top} of {nctx}")
    offsets = np.zeros(nchunks + 1, np.int64)
    np.cumsum(lengths, out=offsets[1:])
    d_bytes = torch.from_numpy(data.copy()).to(dev)
    d_off = torch.from_numpy(offsets).to(dev)
    d_tab = torch.from_numpy(tables.view(np.int16).copy()).to(dev)
    d_map = torch.from_numpy(table_of.astype(np.uint8)).to(dev)
    _check(lib().scp_ac_chunks_decode_ctx(d_bytes.data_ptr(), d_off.data_ptr(), n, N, d_tab.data_ptr(), ntab, int(Lp), d_map.data_ptr(), nctx,
                                          _dev(ctx_dev), sym.data_ptr(), _stream()), "scp_ac_chunks_decode_ctx")
    return sym


class AcDecoder:
    def __init__(self, byte_stream, Lp=256):
        self.Lp = Lp
        self._buf = np.frombuffer(byte_stream, np.uint8).copy()
        self._h = _vp()
        _check(lib().scp_ac_dec_new(C.byref(self._h), self._buf.ctypes.data, len(self._buf), Lp), "scp_ac_dec_new")

    def next(self, cdf_row):
        row = np.ascontiguousarray(cdf_row).view(np.uint16)
        return _check(lib().scp_ac_dec_next(self._h, row.ctypes.data), "scp_ac_dec_next")

    def run(self, cdf):
        """cdf uint16/int16 numpy [n,Lp] -> int16 numpy [n] (n consecutive symbols)."""
        cdf = np.ascontiguousarray(cdf).view(np.uint16)
        out = np.empty(cdf.shape[0], np.int16)
        _check(lib().scp_ac_dec_run(self._h, cdf.ctypes.data, cdf.shape[0], out.ctypes.data), "scp_ac_dec_run")
        return out

    def run_ctx(self, tables, ctx):
        """tables uint16/int16 numpy [nctx,Lp], ctx uint8 numpy [n] -> int16 numpy [n]: symbol i decoded against row ctx[i]."""
        tables = np.ascontiguousarray(tables).view(np.uint16)
        ctx = np.ascontiguousarray(ctx, np.uint8)
        if tables.ndim != 2 or tables.shape[1] != self.Lp:
            raise ScpError(f"run_ctx: tables of shape [nctx, {self.Lp}] expected, got {tables.shape}")
        out = np.empty(ctx.shape[0], np.int16)
        _check(lib().scp_ac_dec_run_ctx(self._h, tables.ctypes.data, tables.shape[0], ctx.ctypes.data, ctx.shape[0], out.ctypes.data),
               "scp_ac_dec_run_ctx")
        return out

    def __del__(self):
        try:
            if self._h:
                lib().scp_ac_dec_free(self._h)
        except Exception:
            pass
