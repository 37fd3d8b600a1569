"""ctypes binding of ``libcar_hip.so`` (C ABI declared in ``include/car_hip.h`` and, for the matcher, in ``include/car_match.h`` and, for the encoder, in ``include/car_encoder.h``, ``include/car_trunk.h`` and ``include/car_decoder.h``, which it includes).

The library is built in-tree by ``__graft_entry__.build()``.  There is no fallback: if it cannot be loaded,
``load()`` raises.  Two handles on the one library: ``api()``, which the package calls — every entry that returns a status checks itself
and raises ``CarError(car_last_error())`` on a negative code — and ``load()``, the raw one, for tests and tools that assert on the codes.
ctypes releases the GIL around each call; all work is enqueued on the stream the caller passes.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p
from typing import Optional

# torch comes first: its wheel bundles its own libamdhip64.so, and the process must end up with ONE HIP runtime (the one that owns
# torch's device context and streams) — loading ours first binds /opt/rocm's copy.
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcar_hip.so")

_P = c_void_p
CAR_E_ARG, CAR_E_LAUNCH = -1, -2          # include/car_hip.h


class CarDims(ctypes.Structure):          # struct car_dims
    _fields_ = [("b", c_int), ("V", c_int), ("R", c_int), ("P", c_int), ("H", c_int), ("W", c_int), ("n_levels", c_int),
                ("level_h", c_int * 4), ("level_w", c_int * 4), ("level_c", c_int * 4), ("repeat_attention", c_int), ("no_sample", c_int)]


# struct car_weights: device pointers in declaration order (attribute path on the module, flattened to [out, in])
WEIGHT_FIELDS = (
    ["query_encode_latent", "query_encode_latent_2", "latent_value", "key_map", "key_map_2", "query_embed", "query_embed_2",
     "query_repeat_embed", "query_repeat_embed_2", "encode_latent", "phi.lin_in", "phi.lin_out"],
    ["phi.lin_z", "phi.blocks.fc_0", "phi.blocks.fc_1"])


class CarWeights(ctypes.Structure):
    _fields_ = ([(f"{n.replace('.', '_')}_{k}", _P) for n in WEIGHT_FIELDS[0] for k in ("w", "b")]
                + [("phi_lin_z_w", _P * 3), ("phi_lin_z_b", _P * 3), ("phi_fc_0_w", _P * 3), ("phi_fc_0_b", _P * 3),
                   ("phi_fc_1_w", _P * 3), ("phi_fc_1_b", _P * 3)])


class CarInputs(ctypes.Structure):
    _fields_ = [("poses", _P), ("uv", _P), ("lattice", _P), ("gmeta", _P), ("steps", _P)]


class CarOutputs(ctypes.Structure):
    _fields_ = [("rgb", _P), ("valid_mask", _P), ("depth_ray", _P), ("at_wt", _P), ("at_wt_max", _P), ("coords", _P),
                ("pixel_val", _P)]


# name -> (restype, argtypes); mirrors include/car_hip.h line by line
SIGNATURES = {
    "car_version": (c_int, []),
    "car_last_error": (c_char_p, []),
    "car_device_cu_count": (c_int, []),
    "car_pose_setup": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P]),
    "car_ray_setup": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P]),
    "car_sample_setup": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P,
                                 c_int, c_int, _P, _P]),
    "car_gather_encode_rows": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, _P, c_int, c_long, _P, c_int, _P]),
    "car_merge_lattice": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "car_merge_lattice_max": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P]),
    "car_lattice_encode_rows": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_long, _P, c_int, _P]),
    "car_lattice_encode_linear": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_long, _P, _P, c_int, c_int, _P, c_int, c_int, _P]),
    "car_project_points": (c_int, [_P, _P, c_int, c_long, c_int, c_int, c_int, c_int, _P, _P]),
    "car_gather_bilinear": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, c_long, c_int, c_int, c_int, c_int, _P, c_int, c_int, _P]),
    "car_gather_encode": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, _P, c_int, c_int, c_long, _P, c_int, _P]),
    "car_fused_blob_floats": (c_size_t, []),
    "car_fused_bias_floats": (c_size_t, []),
    "car_fused_samples": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                  _P, _P, _P, _P, _P, _P]),
    "car_exchange_rows": (c_int, [_P, _P, _P, _P, c_int, c_int, c_long, c_int, c_int, _P, _P, _P, _P]),
    "car_fused_pack_rows": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "car_fused_rows": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "car_fused_tile_steps": (c_int, []),
    "car_fused_samples_parts": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        _P, _P, _P, _P, _P, _P, _P]),
    "car_linear_packed_floats": (c_size_t, [c_int, c_int]),
    "car_linear_pack": (c_int, [_P, c_int, _P, c_int, c_int, _P, _P]),
    "car_linear": (c_int, [_P, c_int, _P, c_int, c_int, _P, c_int, c_long, c_int, _P]),
    "car_kq_tail_floats": (c_size_t, []),
    "car_kq_bias_floats": (c_size_t, []),
    "car_kq_pack": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "car_key_query_logits": (c_int, [_P, c_int, _P, _P, c_int, _P, _P, _P, c_long, _P, _P, _P]),
    "car_attend": (c_int, [_P, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, c_float, _P, _P, c_int, c_int,
                           _P, _P, _P, _P, _P]),
    "car_attend_parts": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "car_round2_packed_floats": (c_size_t, []),
    "car_round2_bias_floats": (c_size_t, []),
    "car_round2_logits": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "car_round2q_packed_floats": (c_size_t, []),
    "car_round2q_bias_floats": (c_size_t, []),
    "car_round2_logits_from_g": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "car_attend_round2": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, _P]),
    "car_round2q_pack": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "car_fused_pack": (c_int, [ctypes.POINTER(CarWeights), _P, _P, _P, _P]),
    "car_round2_pack": (c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "car_add_ray_bias_relu": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "car_finalize": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "car_chain_packed_floats": (c_size_t, [c_int, c_int]),
    "car_linear_x3_packed_floats": (c_size_t, [c_int, c_int]),
    "car_linear_x3_pack": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "car_linear_x3": (c_int, [_P, c_int, _P, _P, c_int, c_int, _P, c_int, c_long, c_int, _P]),
    "car_linear_x3_masked": (c_int, [_P, c_int, _P, _P, c_int, c_int, _P, c_int, c_long, c_int, _P, c_int, _P]),
    "car_chain_pack": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, _P, c_int, _P]),
    "car_ray_mid": (c_int, [_P, _P, _P, c_int, _P, _P, _P, c_int, _P, c_int, _P, _P, c_long, _P]),
    "car_ray_tail": (c_int, [_P, _P, _P, c_int, _P, _P, _P, c_int, _P, c_int, _P, c_int, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "car_plan_bytes": (c_size_t, [ctypes.POINTER(CarDims)]),
    "car_plan_build": (c_int, [ctypes.POINTER(CarDims), ctypes.POINTER(CarWeights), _P, _P]),
    "car_gmaps_floats": (c_size_t, [ctypes.POINTER(CarDims)]),
    "car_lattice_shape": (c_int, [ctypes.POINTER(CarDims), ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "car_gmeta_offset": (c_size_t, [ctypes.POINTER(CarDims)]),
    "car_workspace_find": (c_int, [ctypes.POINTER(CarDims), c_char_p, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "car_profile_enable": (None, [c_int]),
    "car_profile_count": (c_int, []),
    "car_profile_read": (c_int, [c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_float)]),
    "car_profile_reset": (None, []),
    "car_project_maps": (c_int, [ctypes.POINTER(CarDims), _P, _P, _P, _P]),
    "car_workspace_bytes": (c_size_t, [ctypes.POINTER(CarDims)]),
    "car_render_forward": (c_int, [ctypes.POINTER(CarDims), _P, ctypes.POINTER(CarInputs), ctypes.POINTER(CarOutputs), _P,
                                   c_size_t, _P]),
    "car_render_forward_phase": (c_int, [ctypes.POINTER(CarDims), _P, ctypes.POINTER(CarInputs), ctypes.POINTER(CarOutputs), _P,
                                         c_size_t, c_int, _P]),
    "car_plan_f16_bytes": (c_size_t, [ctypes.POINTER(CarDims)]),
    "car_plan_f16_build": (c_int, [ctypes.POINTER(CarDims), ctypes.POINTER(CarWeights), _P, _P]),
    "car_render_forward_f16": (c_int, [ctypes.POINTER(CarDims), _P, _P, ctypes.POINTER(CarInputs), ctypes.POINTER(CarOutputs), _P,
                                       c_size_t, c_int, _P]),
    "car_linspace": (None, [c_float, c_float, c_int, _P]),
    "car_linear_wgrad": (c_int, [_P, c_int, _P, c_int, c_long, c_int, c_int, c_int, _P, c_int, _P, _P]),
    "car_attend_backward": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P, c_int, _P, _P]),
    "car_gather_bilinear_backward": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, c_long, c_int, c_int, c_int, _P, c_int, c_int, _P]),
    "car_scatter_workspace_bytes": (c_size_t, [_P, _P, c_int, c_int, c_long, c_int]),
    "car_gather_bilinear_backward_binned": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P, _P, c_int, c_long, c_int, _P, c_int, c_int, _P, c_size_t, _P]),
    "car_relu_mask": (c_int, [_P, c_int, _P, c_int, c_long, c_int, _P]),
    "car_scale_rows": (c_int, [_P, c_int, _P, c_int, _P, c_long, c_float, c_long, c_int, c_int, _P]),
    "car_add": (c_int, [_P, c_int, _P, c_int, c_float, _P, c_int, c_float, c_long, c_int, _P]),
    "car_reduce_samples": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "car_ssim_scratch_doubles": (c_size_t, [c_int, c_int, c_int, c_int]),
    "car_ssim": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_double, _P, _P, c_size_t, _P]),
    "car_lpips_packed_floats": (c_size_t, []),
    "car_lpips_pack": (c_int, [_P, _P, _P, _P, _P]),
    "car_lpips_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_lpips": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "car_conv3x3_packed_floats": (c_size_t, [c_int, c_int]),
    "car_conv3x3_pack": (c_int, [_P, _P, c_int, c_int, _P, _P]),
    "car_conv3x3": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "car_maxpool2x2": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "car_lpips_head_scratch_doubles": (c_size_t, [c_int, c_int, c_int]),
    "car_lpips_head": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "car_lpips_backward_packed_floats": (c_size_t, []),
    "car_lpips_pack_backward": (c_int, [_P, _P, _P]),
    "car_lpips_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_lpips_train_layer_offset": (c_size_t, [c_int, c_int, c_int, c_int]),
    "car_lpips_forward_train": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "car_lpips_backward": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "car_conv3x3_backward_packed_floats": (c_size_t, [c_int, c_int]),
    "car_conv3x3_backward_pack": (c_int, [_P, c_int, c_int, _P, _P]),
    "car_conv3x3_backward": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "car_maxpool2x2_backward": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "car_lpips_head_backward": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "car_frames_table_ints": (c_size_t, []),
    "car_frames_table_slot": (c_int, [c_int, c_int]),
    "car_frames_resize_u8": (c_int, [_P, c_size_t, _P, _P, c_int, _P, _P, c_size_t, _P]),
    "car_frames_resize_f32": (c_int, [_P, c_size_t, _P, _P, c_int, _P, _P, c_size_t, _P, _P, c_size_t, _P]),
    "car_attention_entropy_scratch_doubles": (c_size_t, [c_long, c_int]),
    "car_attention_entropy": (c_int, [_P, c_long, c_int, c_int, _P, _P, c_size_t, _P]),
    "car_colormap": (c_int, [_P, c_int, c_int, c_int, c_float, _P, _P, _P]),
    "car_epipolar_overlay": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "car_image_grid_scratch_floats": (c_size_t, [c_int, c_int, c_int]),
    "car_image_grid": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_float, c_float, _P, _P, c_size_t, _P]),
    "car_essential_workspace_bytes": (c_size_t, [c_int, c_int]),
    "car_essential_solve": (c_int, [_P, _P, c_int, _P, c_int, _P, _P, _P]),
    "car_essential_score": (c_int, [_P, _P, c_int, _P, _P, c_int, c_double, _P, _P, _P]),
    "car_essential_select": (c_int, [_P, _P, c_int, _P, _P, _P, c_int, c_double, _P, _P, _P, _P]),
    "car_essential_ransac": (c_int, [_P, _P, c_int, _P, c_int, c_double, _P, _P, _P, _P, c_size_t, _P]),
}

# the matcher's entries (SuperPoint, SuperGlue): mirrors include/car_match.h, the header of their own that car_hip.h includes; bound
# and checked like SIGNATURES
MATCH_SIGNATURES = {
    "car_superpoint_packed_floats": (c_size_t, []),
    "car_superpoint_pack": (c_int, [_P, _P, _P, _P]),
    "car_superpoint_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_superpoint_dense": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "car_superpoint_conv1a": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P]),
    "car_superpoint_nms_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_superpoint_nms": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "car_superpoint_select_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_superpoint_select": (c_int, [_P, c_int, c_int, c_int, c_float, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "car_superpoint_sample": (c_int, [_P, c_int, _P, c_int, c_int, _P, _P]),
    "car_superglue_packed_floats": (c_size_t, [c_int]),
    "car_superglue_pack": (c_int, [_P, c_int, c_int, _P, _P]),
    "car_superglue_workspace_bytes": (c_size_t, [c_int, c_int]),
    "car_superglue_descriptors": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_int, c_int, c_int, _P, c_int, _P, _P, _P, c_size_t, _P]),
    "car_superglue_attention": (c_int, [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, _P, c_int, _P]),
    "car_superglue_transport_workspace_bytes": (c_size_t, [c_int, c_int]),
    "car_superglue_transport": (c_int, [_P, c_int, _P, c_int, c_float, c_int, _P, _P, c_size_t, _P]),
    "car_superglue_matches_workspace_bytes": (c_size_t, [c_int, c_int]),
    "car_superglue_matches": (c_int, [_P, c_int, c_int, c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
}

# the encoder's entries (the transformer stage of get_z): mirrors include/car_encoder.h, the header of their own that car_hip.h includes;
# bound and checked like SIGNATURES
ENCODER_SIGNATURES = {
    "car_layernorm": (c_int, [_P, c_int, _P, _P, c_int, c_double, _P, c_int, c_long, _P]),
    "car_gelu": (c_int, [_P, c_int, c_long, c_int, _P]),
    "car_mha_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_mha": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, _P, c_size_t, _P]),
    "car_vit_packed_floats": (c_size_t, [c_int, c_int]),
    "car_vit_packed_offset": (c_size_t, [c_int, c_int]),
    "car_vit_pack": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "car_vit_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_vit_blocks": (c_int, [_P, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, _P, c_size_t, _P]),
}

# training through the encoder's transformer stage (the recorded forward and the backward of the blocks): mirrors
# include/car_encoder_train.h, the header of their own that car_hip.h includes; bound and checked like SIGNATURES
ENCODER_TRAIN_SIGNATURES = {
    "car_mha_stats_floats": (c_size_t, [c_int, c_int, c_int]),
    "car_mha_stats": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_size_t, _P]),
    "car_mha_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_mha_backward": (c_int, [_P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P, c_size_t, _P]),
    "car_layernorm_backward_workspace_bytes": (c_size_t, [c_long, c_int]),
    "car_layernorm_backward": (c_int, [_P, c_int, _P, c_int, c_double, _P, c_int, _P, c_int, c_long, c_int, _P, _P, _P, c_size_t, _P]),
    "car_gelu_backward": (c_int, [_P, c_int, _P, c_int, c_long, c_int, _P]),
    "car_vit_packed_train_floats": (c_size_t, [c_int, c_int]),
    "car_vit_packed_train_offset": (c_size_t, [c_int, c_int, c_int]),
    "car_vit_pack_train": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "car_vit_saved_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "car_vit_blocks_train": (c_int, [_P, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, _P, c_size_t, _P, c_size_t, _P]),
    "car_vit_grad_offset": (c_size_t, [c_int, c_int]),
    "car_vit_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_vit_blocks_backward": (c_int, [_P, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, _P, c_size_t, _P, c_int, _P, c_size_t, _P]),
}

# the encoder's front half (the ResNetV2 trunk and the token assembly of get_z): mirrors include/car_trunk.h, the header of their own that
# car_hip.h includes; bound and checked like SIGNATURES
TRUNK_SIGNATURES = {
    "car_weight_standardize": (c_int, [_P, c_int, c_int, c_double, _P, _P]),
    "car_stem7x7": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P]),
    "car_groupnorm_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "car_groupnorm": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, c_double, _P, c_int, _P, _P, c_size_t, _P]),
    "car_maxpool3x3s2_same": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "car_conv3x3_same_packed_floats": (c_size_t, [c_int, c_int]),
    "car_conv3x3_same_pack": (c_int, [_P, c_int, c_int, _P, _P]),
    "car_conv3x3_same": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "car_pixels_stride2": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "car_trunk_packed_floats": (c_size_t, [_P]),
    "car_trunk_pack": (c_int, [_P, c_int, _P, _P, _P]),
    "car_trunk_workspace_bytes": (c_size_t, [c_int, c_int, c_int, _P]),
    "car_trunk_forward": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "car_vit_tokens_packed_floats": (c_size_t, [c_int, c_int]),
    "car_vit_tokens_pack": (c_int, [_P, _P, _P, _P, c_int, _P, _P, c_int, c_int, _P, _P]),
    "car_vit_tokens_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_vit_tokens": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
}
CAR_GN_RELU = 1                           # include/car_trunk.h

# the encoder's back half and get_z as one call (the read-out, the fusion, conv_map, the normalisation): mirrors include/car_decoder.h, the
# header of their own that car_hip.h includes; bound and checked like SIGNATURES
DECODER_SIGNATURES = {
    "car_conv3x3_pad1_packed_floats": (c_size_t, [c_int, c_int]),
    "car_conv3x3_pad1_pack": (c_int, [_P, c_int, c_int, _P, _P]),
    "car_conv3x3_pad1": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P]),
    "car_upsample2x_bilinear": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "car_readout_packed_floats": (c_size_t, [c_int]),
    "car_readout_pack": (c_int, [_P, _P, c_int, _P, _P]),
    "car_readout_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_readout": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "car_conv7x7_pad3": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P]),
    "car_normalize_rgb": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "car_decoder_packed_floats": (c_size_t, []),
    "car_decoder_pack": (c_int, [_P, c_int, _P, _P]),
    "car_decoder_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "car_decoder_forward": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "car_getz_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int]),
    "car_getz": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P, _P, _P, _P, c_int, _P, _P, _P, _P, c_size_t, _P]),
}

# the int entries that return a VALUE (the header's words); every other int entry returns a status: 0, or a negative CAR_E_* code
VALUE_ENTRIES = (
    "car_version",                # CAR_VERSION
    "car_device_cu_count",        # "Number of compute units of the current device"
    "car_fused_tile_steps",       # the step-group size of car_fused_samples_parts' `part`
    "car_profile_count",          # "stages recorded since enable / the last read"
    "car_frames_table_slot",      # the slot of (n_src, n_dst); "any other pair has no table and is refused (slot -1)"
)

_lib: Optional[ctypes.CDLL] = None
_api: Optional[ctypes.CDLL] = None


def source_hash() -> str:
    """sha256 over the kernel sources and the public headers: build() stores it next to the library, load() refuses a library built
    from anything else (a pushed .so can not silently lag behind the tree)."""
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    files += [os.path.join(os.path.dirname(here), "include", f) for f in ("car_hip.h", "car_match.h", "car_encoder.h", "car_trunk.h", "car_decoder.h", "car_encoder_train.h")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _rebuild_stale() -> None:
    """The library on disk was built from other sources than the tree's: rebuild it with the tree's own build() when hipcc is here
    (always the real HIP library, never a substitute), refuse otherwise."""
    import fcntl
    import importlib.util
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    entry = os.path.join(root, "__graft_entry__.py")
    if os.path.exists(entry) and (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        # one builder at a time: ranks spawned together (experiment_scripts --gpus N, bench.py under torchrun) all land here at once.
        # The others wait on the lock, find the stamp current and load the library the first one linked (build_library links to a
        # temporary file and renames it into place, so a concurrent dlopen never sees a half-written .so).
        with open(LIB_PATH + ".lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if not _stamp_current():
                    spec = importlib.util.spec_from_file_location("_car_graft_entry", entry)
                    mod = importlib.util.module_from_spec(spec)
                    spec.loader.exec_module(mod)
                    mod.build_library()
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
        if _stamp_current():
            return
    raise RuntimeError(f"{LIB_PATH} was built from other sources than the ones in this tree (csrc/, include/car_hip.h): rebuild it "
                       "with `python __graft_entry__.py`")


def _stamp_current() -> bool:
    stamp = LIB_PATH + ".srchash"
    try:
        return os.path.exists(LIB_PATH) and open(stamp).read().strip() == source_hash()
    except OSError:
        return False


def load() -> ctypes.CDLL:
    """Loads the HIP library (once) and sets the prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
            "The render path has no CPU/PyTorch fallback.")
    if not _stamp_current():                      # a missing stamp counts as stale: the library's sources are unknown
        _rebuild_stale()
    _lib = _bind(checked=False)
    return _lib


def _bind(checked: bool) -> ctypes.CDLL:
    """A handle of its own on the library (a second CDLL of one path has its own function objects) with SIGNATURES' prototypes;
    ``checked``: every status entry raises CarError on a negative code."""
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **MATCH_SIGNATURES, **ENCODER_SIGNATURES, **TRUNK_SIGNATURES, **DECODER_SIGNATURES,
                               **ENCODER_TRAIN_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
        if checked and res is c_int and name not in VALUE_ENTRIES:
            fn.errcheck = _errcheck
    return lib


def api() -> ctypes.CDLL:
    """The checked handle (once): what the package calls.  A value, a size (0 stays the caller's business) or text comes back as it is."""
    global _api
    if _api is None:
        load()
        _api = _bind(checked=True)
    return _api


class CarError(RuntimeError):
    """A negative status ``code`` of ``entry``, with the library's message ``text`` (car_last_error unless given)."""

    def __init__(self, code: int, entry: str, text: Optional[str] = None):
        if text is None:
            msg = load().car_last_error()
            text = msg.decode() if msg else "?"
        self.code, self.entry, self.text = code, entry, text
        super().__init__(f"{entry} failed ({code}): {self.text}")


def _errcheck(code, fn, args):
    if code < 0:
        raise CarError(code, fn.__name__)
    return code


def check_exports() -> None:
    """Every symbol the header declares must be exported (used by build() and the CPU test-suite)."""
    lib = load()
    missing = [n for n in (*SIGNATURES, *MATCH_SIGNATURES, *ENCODER_SIGNATURES, *TRUNK_SIGNATURES, *DECODER_SIGNATURES,
                             *ENCODER_TRAIN_SIGNATURES) if not hasattr(lib, n)]
    if missing:
        raise RuntimeError(f"libcar_hip.so lacks symbols: {missing}")
    if lib.car_version() < 300:
        raise RuntimeError("libcar_hip.so is older than the Python package")


def check(code: int, what: str = "") -> None:
    """The same check for a code taken from the raw handle (tests, tools) or made by hand (a size of 0 as CAR_E_ARG)."""
    if code < 0:
        raise CarError(code, what or "libcar_hip")


def user_call(fn, *args):
    """``fn(*args)`` for the user-facing wrappers: an argument the library refuses (CAR_E_ARG) is the caller's ValueError, with the
    library's bare text; anything else stays a CarError."""
    try:
        return fn(*args)
    except CarError as e:
        if e.code == CAR_E_ARG:
            raise ValueError(e.text) from None
        raise


def ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def stream():
    """The current torch stream as the ``void* stream`` of the C ABI."""
    return c_void_p(torch.cuda.current_stream().cuda_stream)
