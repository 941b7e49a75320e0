"""ctypes binding of ``libendodav_hip.so`` (C ABI: ``include/endodav_hip.h``).

The library is built in-tree by ``make`` / ``__graft_entry__.build()``.  There is no fallback:
if the shared object is missing or a symbol is absent, importing the binding raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EDV_LIB_PATH") or os.path.join(_HERE, "lib", "libendodav_hip.so")  # override: experiments only
ABI_VERSION = 15

LORA_TYPES = {"none": 0, "lora": 1, "dvlora": 2, "ssb": 3, "dash": 4}
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SIGMOID, ACT_SIGMOID_NEG = 0, 1, 2, 3, 4


class EdvConfig(C.Structure):
    """``struct edv_config`` — field order must match the header."""

    _fields_ = [
        ("abi_version", C.c_int32),
        ("embed_dim", C.c_int32),
        ("depth", C.c_int32),
        ("num_heads", C.c_int32),
        ("taps", C.c_int32 * 4),
        ("features", C.c_int32),
        ("out_channels", C.c_int32 * 4),
        ("image_h", C.c_int32),
        ("image_w", C.c_int32),
        ("num_frames", C.c_int32),
        ("pos_tokens", C.c_int32),
        ("lora_type", C.c_int32),
        ("lora_rank", C.c_int32),
        ("include_cls_token", C.c_int32),
        ("conv_head", C.c_int32),
        ("inv_sigmoid", C.c_int32),
        ("out_sigmoid", C.c_int32),
        ("temporal_lora", C.c_int32),
        ("dash_active", C.c_int32),
        ("use_clstoken", C.c_int32),
        ("residual_mask", C.c_uint32),
        ("use_bn", C.c_int32),
        ("pe_rope", C.c_int32),
    ]


_fp = C.c_void_p  # device pointers travel as integers
_i32, _i64, _f32, _f64 = C.c_int32, C.c_int64, C.c_float, C.c_double

# name -> (restype, argtypes); every symbol declared in include/endodav_hip.h
SIGNATURES = {
    "edv_abi_version": (C.c_int, []),
    "edv_last_error": (C.c_char_p, []),
    "edv_create": (C.c_int, [C.POINTER(EdvConfig), C.POINTER(C.c_void_p)]),
    "edv_destroy": (C.c_int, [C.c_void_p]),
    "edv_bind_param": (C.c_int, [C.c_void_p, C.c_char_p, _fp, C.POINTER(_i64), _i32]),
    "edv_prepare": (C.c_int, [C.c_void_p, C.c_void_p]),
    "edv_refresh_lora": (C.c_int, [C.c_void_p, C.c_void_p]),
    "edv_forward": (C.c_int, [C.c_void_p, _fp, _i32, _i32, _i32, _i32, C.POINTER(C.c_void_p), C.c_void_p]),
    "edv_output_shape": (C.c_int, [C.c_void_p, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "edv_stage_copy": (C.c_int, [C.c_void_p, C.c_char_p, _fp, C.POINTER(C.c_size_t), C.c_void_p]),
    "edv_set_capture": (C.c_int, [C.c_void_p, C.c_int]),
    "edv_profile_enable": (C.c_int, [C.c_void_p, C.c_uint32]),
    "edv_set_encoder_streams": (C.c_int, [C.c_void_p, _i32]),
    "edv_set_products": (C.c_int, [C.c_void_p, _i32, C.c_void_p]),
    "edv_get_products": (C.c_int, [C.c_void_p]),
    "edv_profile_set_mask": (C.c_int, [C.c_void_p, C.c_uint32]),
    "edv_profile_work": (C.c_int, [C.c_void_p, _i32, C.POINTER(_f64), C.POINTER(_f64)]),
    "edv_profile_read": (C.c_int, [C.c_void_p, _i32, C.POINTER(_i32), C.POINTER(_f64)]),
    "edv_device_bytes": (C.c_size_t, [C.c_void_p]),
    "edv_last_launch_count": (C.c_int, [C.c_void_p]),
    "edv_layernorm": (C.c_int, [_fp, _fp, _fp, _fp, _i64, _i32, _f32, _fp, _i32, _i32, C.c_void_p]),
    "edv_gemm_workspace": (C.c_size_t, []),
    "edv_gemm_x6_planes_bytes": (C.c_size_t, [_i32, _i32]),
    "edv_gemm_x6_split": (C.c_int, [_fp, C.c_void_p, _i32, _i32, C.c_void_p]),
    "edv_gemm_x6": (C.c_int, [_fp, C.c_void_p, _fp, _i64, _i32, _i32, _fp, _i32, _fp, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_gemm": (C.c_int, [_fp, _fp, _fp, _i64, _i32, _i32, _fp, _i32, _fp, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_pack_geglu": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, C.c_void_p]),
    "edv_gemm_geglu": (C.c_int, [_fp, _fp, _fp, _fp, _i64, _i32, _i32, C.c_void_p]),
    "edv_conv3x3": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _fp, _fp, C.c_void_p]),
    "edv_conv3x3_ws": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _fp, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_set_conv_impl": (C.c_int, [_i32]),
    "edv_set_x6_remainder": (C.c_int, [_i32, _i32]),
    "edv_conv3x3_dot": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _fp, _fp, _i32, C.c_void_p]),
    "edv_pack_conv3x3": (C.c_int, [_fp, _fp, _i32, _i32, C.c_void_p]),
    "edv_conv_transpose": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_attn_spatial_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_attn_spatial": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _fp, C.c_size_t, _fp, C.c_void_p]),
    "edv_set_train": (C.c_int, [C.c_void_p, _i32]),
    "edv_set_grad_scope": (C.c_int, [C.c_void_p, _i32, _i32, _i32, _i32]),
    "edv_set_bias_grads": (C.c_int, [C.c_void_p, _i32, _i32]),
    "edv_generation": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "edv_backward": (C.c_int, [C.c_void_p, C.c_uint64, _fp, C.POINTER(C.c_void_p), C.c_void_p]),
    "edv_grad_bind_flat": (C.c_int, [C.c_void_p, _i32, C.POINTER(C.c_char_p), C.POINTER(_i64), _fp, _i64, C.POINTER(_i64)]),
    "edv_grad": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(_i64)]),
    "edv_grad_copy": (C.c_int, [C.c_void_p, C.c_char_p, _fp, _i64, C.c_void_p]),
    "edv_attn_spatial_x6_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_attn_spatial_x6": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _fp, C.c_size_t, C.c_void_p]),
    "edv_attn_spatial_bwd_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_attn_spatial_bwd": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _i32, _i32, _i32, _fp, C.c_size_t, C.c_void_p]),
    "edv_layernorm_bwd": (C.c_int, [_fp, _fp, _fp, _fp, _i64, _i32, C.c_float, _i32, C.c_void_p]),
    "edv_ew_bwd": (C.c_int, [_fp, _fp, _fp, _fp, _i64, _i32, C.c_void_p]),
    "edv_geglu_bwd": (C.c_int, [_fp, _fp, _fp, _i64, _i32, C.c_void_p]),
    "edv_transpose_scale": (C.c_int, [_fp, _fp, _fp, _i32, _i32, C.c_void_p]),
    "edv_lora_grads_workspace": (C.c_size_t, [_i64, _i32, _i32, _i32]),
    "edv_lora_grads": (C.c_int, [_fp, _fp, _i64, _i32, _i32, _i32, _fp, _fp, _fp, _fp, C.c_float, _fp, _fp, C.c_size_t, _fp, _fp, _fp, _fp, C.c_void_p]),
    "edv_bilinear_bwd": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_dot_channels_bwd": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _i64, _i32, _i32, C.c_void_p]),
    "edv_conv3x3_wgrad_workspace": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32]),
    "edv_conv3x3_wgrad": (C.c_int, [_fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, _fp, C.c_size_t, _i32, C.c_void_p]),
    "edv_colsum_workspace": (C.c_size_t, [_i32]),
    "edv_colsum_rows": (C.c_int, [_fp, _fp, _i64, _i32, _fp, C.c_size_t, _fp, _i32, C.c_void_p]),
    "edv_colsum_batch_workspace": (C.c_size_t, [_i32, C.POINTER(_i64), C.POINTER(_i32)]),
    "edv_colsum_batch": (C.c_int, [_i32, C.POINTER(C.c_void_p), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_void_p), C.POINTER(_i32), _fp, C.c_size_t, C.c_void_p]),
    "edv_groupnorm_bwd": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_attn_temporal_bwd": (C.c_int, [_fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_pack_conv3x3_bwd": (C.c_int, [_fp, _fp, _i32, _i32, C.c_void_p]),
    "edv_conv3x3_s2_bwd": (C.c_int, [_fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_dilate2": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_pixel_unshuffle": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_attn_temporal": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_groupnorm_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_groupnorm": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _f32, _fp, C.c_size_t, C.c_void_p]),
    "edv_geglu": (C.c_int, [_fp, _fp, _i64, _i32, C.c_void_p]),
    "edv_rope_qk": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_trainer_loss_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_trainer_loss": (C.c_int, [C.c_void_p, _i32, _i32, _i32, C.c_void_p, _fp, C.c_void_p, _fp, C.c_size_t, C.c_void_p]),
    "edv_debug_fill_lds": (C.c_int, [C.c_float, C.c_void_p]),
    "edv_bilinear": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_dot_channels": (C.c_int, [_fp, _fp, _fp, _fp, _i64, _i32, _i32, C.c_void_p]),
    "edv_patchify": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_bicubic_pos": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, _f64, _f64, C.c_void_p]),
    "edv_resize_bicubic": (C.c_int, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    # additive entry point (ABI stays 15): uint8 frames -> the network's input; the slots are host memory, NULL = identity
    "edv_ingest_u8": (C.c_int, [_fp, _i32, C.POINTER(_i32), _i32, _fp, _i32, _i32, _i32, _i32, C.c_void_p]),
    # colour-mapped depth (additive, ABI stays 15): range [n][2] fp32 on the device, LUT [256][3] uint8, out uint8
    "edv_render_workspace": (C.c_size_t, [_i64]),
    "edv_render_range": (C.c_int, [_fp, _i64, _i32, _i32, _i32, _i64, _i64, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_render_colorize": (C.c_int, [_fp, _i64, _i32, _i32, _fp, _i32, _f32, _i32, _fp, _fp, _fp, C.c_void_p]),
    # point clouds on the device (additive, ABI stays 15): both calls take one CloudSelection
    "edv_cloud_tile_pixels": (_i32, []),
    "edv_cloud_workspace": (C.c_size_t, [_i64, _i32, _i32, _i32]),
    "edv_cloud_count": (C.c_int, [C.c_void_p, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_cloud_scatter": (C.c_int, [C.c_void_p, _fp, _i32, _fp, _fp, _fp, C.c_size_t, _fp, _fp, _i64, C.c_void_p]),
    # surface fusion on the device (additive, ABI stays 15): a TsdfVolume, and for integrate the cloud's CloudSelection
    "edv_tsdf_integrate": (C.c_int, [C.c_void_p, C.c_void_p, _fp, _i32, _fp, C.c_void_p]),
    "edv_tsdf_tile_voxels": (_i32, []),
    "edv_tsdf_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_tsdf_count": (C.c_int, [C.c_void_p, _f32, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_tsdf_extract": (C.c_int, [C.c_void_p, _f32, _fp, C.c_size_t, _fp, _fp, _i64, C.c_void_p]),
    # triangle meshes from the volume (additive, ABI stays 15)
    "edv_tsdf_mesh_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_tsdf_mesh_count": (C.c_int, [C.c_void_p, _f32, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_tsdf_mesh_extract": (C.c_int, [C.c_void_p, _f32, _fp, C.c_size_t, _fp, _fp, _fp, _i64, _fp, _i64, C.c_void_p]),
    # views of the volume (additive, ABI stays 15): cams [views][21] doubles on the device; normals and colours may be NULL
    "edv_tsdf_raycast": (C.c_int, [C.c_void_p, _fp, _i32, _i32, _i32, _f64, _f64, _i32, _f32, _fp, _fp, _fp, C.c_void_p]),
    # camera tracking against the volume (additive, ABI stays 15): a CloudSelection, the two cameras as host doubles (21 and 39), one raycast view
    "edv_icp_tile_pixels": (_i32, []),
    "edv_icp_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_icp_sums": (C.c_int, [C.c_void_p, _i64, C.POINTER(_f64), C.POINTER(_f64), _fp, _fp, _i32, _i32, _f64, _fp, _fp, C.c_size_t, C.c_void_p]),
    # the same with the frame's depth scale as a seventh unknown: 37 sums (additive, ABI stays 15)
    "edv_icp_scaled_workspace": (C.c_size_t, [_i32, _i32, _i32]),
    "edv_icp_scaled_sums": (C.c_int, [C.c_void_p, _i64, C.POINTER(_f64), C.POINTER(_f64), _fp, _fp, _i32, _i32, _f64, _fp, _fp, C.c_size_t, C.c_void_p]),
    # both with a colour block behind the geometric one: the frames and the view's colours (uint8), cols = 6 or 7, 2 * 29 or 2 * 37 sums (additive, ABI stays 15)
    "edv_icp_colour_workspace": (C.c_size_t, [_i32, _i32, _i32, _i32]),
    "edv_icp_colour_sums": (C.c_int, [C.c_void_p, _i64, _fp, C.POINTER(_f64), C.POINTER(_f64), _fp, _fp, _fp, _i32, _i32, _f64, _i32, _fp, _fp, C.c_size_t, C.c_void_p]),
    # robust tracking (additive, ABI stays 15): the live frame's normal map for frames first .. first + count - 1 (cams on the device, stride 0 or 21), and any
    # of the sums above with a normal test (live normals, min_cos) and Huber weights (huber, huber_colour); frames and colours may be NULL: no colour block
    "edv_frame_normals": (C.c_int, [C.c_void_p, _fp, _i32, _i64, _i64, _fp, C.c_void_p]),
    "edv_icp_robust_workspace": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32]),
    "edv_icp_robust_sums": (C.c_int, [C.c_void_p, _i64, _fp, C.POINTER(_f64), C.POINTER(_f64), _fp, _fp, _fp, _i32, _i32, _f64, _i32, _fp, _f64, _f64, _f64, _fp, _fp,
                                      C.c_size_t, C.c_void_p]),
    # coarse-to-fine tracking (additive, ABI stays 15): levels 1 .. L of one frame in one launch, float32 depth through a CloudSelection or uint8 RGB; the
    # levels lie one behind the other at the pixel offsets edv_pyramid_pixels states (host int64 [L])
    "edv_pyramid_max_levels": (_i32, []),
    "edv_pyramid_pixels": (C.c_size_t, [_i32, _i32, _i32, C.POINTER(_i64)]),
    "edv_depth_pyramid": (C.c_int, [C.c_void_p, _i64, _i32, _f32, _fp, C.c_void_p]),
    "edv_rgb_pyramid": (C.c_int, [_fp, _i64, _i32, _i32, _i64, _i32, _fp, C.c_void_p]),
    "edv_stitch_workspace": (C.c_size_t, []),
    "edv_stitch_fit": (C.c_int, [_fp, _i32, _i32, _fp, _i32, _i32, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_stitch_apply": (C.c_int, [_fp, _i32, _i32, _fp, _fp, _fp, _i32, _i32, C.c_void_p]),
    # evaluation on the device (ABI 14); results and scalars are doubles in device memory
    "edv_metrics_workspace": (C.c_size_t, [_i64, _i32, _i32]),
    "edv_masked_median": (C.c_int, [_fp, _fp, _i64, _f32, _f32, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_metrics_pred": (C.c_int, [_fp, _fp, _fp, _i64, _i32, _i32, _f64, _f64, _i32, _f32, _f32, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_metrics_errors": (C.c_int, [_fp, _fp, _i64, _i32, _i32, _f32, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_metrics_temporal": (C.c_int, [_fp, _fp, _i64, _i32, _i32, _f32, _fp, _fp, _fp, _fp, C.c_size_t, C.c_void_p]),
    "edv_photometric_loss_workspace": (C.c_size_t, [_i32, _i32, _i32, _i32]),
    "edv_photometric_loss": (C.c_int, [_fp, C.POINTER(C.c_void_p), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _i32, _i32, _fp, _fp, _fp, _fp, _f32, _f32, _f32,
                                       _fp, C.POINTER(C.c_void_p), _fp, C.c_size_t, C.c_void_p]),
    "edv_fold_lora": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _f32, _fp, _i32, _i32, _i32, C.c_void_p]),
    # test entry points (ABI 13); a row map is int32[4] = (period, stride, offset, inner), NULL = identity
    "edv_gemm_desc": (C.c_int, [C.c_void_p, C.c_void_p]),
    "edv_layernorm_mapped": (C.c_int, [_fp, C.POINTER(_i32), _fp, _fp, _fp, C.POINTER(_i32), _i64, _i32, _f32, _fp, _i32, _i32, _i32, _i32, C.c_void_p]),
    "edv_layernorm_bwd_mapped": (C.c_int, [_fp, C.POINTER(_i32), _fp, _fp, C.POINTER(_i32), _fp, C.POINTER(_i32), _i64, _i32, _f32, _i32, C.c_void_p]),
    "edv_fold_ssb": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, C.c_void_p]),
    "edv_fold_bn": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _f32, _fp, _i32, _i32, C.c_void_p]),
    "edv_fold_dash": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, C.c_void_p]),
    "edv_col_dot": (C.c_int, [_fp, _fp, _i64, _i32, _fp, _fp, _fp, C.c_void_p]),
    "edv_ssb_prep": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _i32, _i32, C.c_void_p]),
    "edv_sigmoid_bwd": (C.c_int, [_fp, _fp, _fp, _i64, C.c_void_p]),
    "edv_bilinear_add": (C.c_int, [_fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, _i32, C.c_void_p]),
    # test entry point (ABI 15): the stream-K planners on a given slot count, no device
    "edv_split_plan": (C.c_int, [_i32, _i64, _i32, _i32, C.POINTER(_i64)]),
}


# "linear_encoder" (the F.linear launches of the encoder blocks) is recorded whenever "linear" is enabled and read separately;
# "linear" then holds the remaining F.linear / 1x1-conv launches (patch embed, DPT head)
KERNEL_CLASSES = {"linear": 0, "conv3x3": 1, "attn_spatial": 2, "attn_temporal": 3, "layernorm": 4, "other": 5, "linear_encoder": 6,
                  "groupnorm": 7, "bilinear": 8, "geglu": 9, "dot_channels": 10, "patchify": 11, "attn_spatial_bwd": 12}
HBM_CLASSES = ("layernorm", "groupnorm", "bilinear", "geglu", "dot_channels", "patchify")  # bandwidth-bound kernels (bench.py roofline_hbm)


class EdvError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library once and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EdvError(
            f"{LIB_PATH} is missing: build it with `make` (hipcc --offload-arch=gfx950) or "
            "`python -c 'import __graft_entry__ as g; g.build()'`.  There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is absent
        fn.restype = res
        fn.argtypes = args
    got = lib.edv_abi_version()
    if got != ABI_VERSION:
        raise EdvError(f"libendodav_hip ABI {got} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load().edv_last_error()
        raise EdvError(f"{what}: {msg.decode() if msg else 'unknown error'}")


def ptr(t) -> int:
    """Device pointer of a torch tensor (0 for None)."""
    return 0 if t is None else t.data_ptr()


class TrainerLossInputs(C.Structure):
    """edv_trainer_loss_inputs (include/endodav_hip.h)."""
    _fields_ = [("color", C.c_void_p * 4), ("color_nb", C.c_void_p * 2), ("K", C.c_void_p), ("invK", C.c_void_p), ("T", C.c_void_p * 2),
                ("refined", (C.c_void_p * 2) * 4), ("registration", (C.c_void_p * 2) * 4), ("transform", (C.c_void_p * 2) * 4), ("mask", C.c_void_p * 2),
                ("position", (C.c_void_p * 2) * 4), ("disp", C.c_void_p * 4), ("disp_h", C.c_int32 * 4), ("disp_w", C.c_int32 * 4)]


class TrainerLossWeights(C.Structure):
    _fields_ = [("disparity_smoothness", C.c_float), ("transform_constraint", C.c_float), ("transform_smoothness", C.c_float), ("depth_reproj", C.c_float),
                ("depth_flow", C.c_float), ("tune_temporal", C.c_int32), ("min_depth", C.c_float), ("max_depth", C.c_float)]


class TrainerLossGrads(C.Structure):
    _fields_ = [("disp", C.c_void_p * 4), ("refined", (C.c_void_p * 2) * 4), ("transform", (C.c_void_p * 2) * 4), ("K", C.c_void_p), ("invK", C.c_void_p),
                ("T", C.c_void_p * 2)]


class CloudSelection(C.Structure):
    """edv_cloud_selection (include/endodav_hip.h): which pixels of a clip are kept and at what depth."""
    _fields_ = [("x_dev", C.c_void_p), ("n", _i64), ("h", _i32), ("w", _i32), ("step", _i32), ("mode", _i32), ("lo", _f32), ("span", _f32), ("gain", _f32),
                ("near_z", _f32), ("far_z", _f32), ("mask_dev", C.c_void_p), ("mask_stride", _i64)]


class TsdfVolume(C.Structure):
    """edv_tsdf_volume (include/endodav_hip.h): the device arrays and the geometry of a TSDF volume."""
    _fields_ = [("tsdf_dev", C.c_void_p), ("weight_dev", C.c_void_p), ("color_dev", C.c_void_p), ("nx", _i32), ("ny", _i32), ("nz", _i32),
                ("origin", _f64 * 3), ("voxel", _f64), ("trunc", _f64), ("max_weight", _f32)]


class GemmDescC(C.Structure):
    """edv_gemm_desc_t (include/endodav_hip.h): the GEMM descriptor of the test entry point edv_gemm_desc."""
    _fields_ = [("A", C.c_void_p), ("lda", _i32), ("a_map", _i32 * 4), ("W", C.c_void_p), ("ldw", _i32), ("C", C.c_void_p), ("ldc", _i32), ("c_map", _i32 * 4),
                ("M", _i64), ("N", _i32), ("K", _i32), ("bias", C.c_void_p), ("act", _i32), ("gamma", C.c_void_p), ("R1", C.c_void_p), ("ldr1", _i32),
                ("r1_map", _i32 * 4), ("R2", C.c_void_p), ("ldr2", _i32), ("P1", C.c_void_p), ("ldp1", _i32), ("p1_map", _i32 * 4), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("x6_planes", C.c_void_p)]


def stream_ptr(device=None) -> int:
    import torch

    return torch.cuda.current_stream(device).cuda_stream
