"""ctypes binding of the C ABI declared in include/igs_rast.h (libigs_rast.so, gfx950).

There is NO CPU fallback: if the HIP library cannot be built or loaded this module raises.
"""
import ctypes as C
import os

from . import build as _build

_LIB = None
E_RETRY = -6      # IGS_RAST_E_RETRY

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
_vp, _i, _f = C.c_void_p, C.c_int, C.c_float

class RefineStepArgs(C.Structure):
    """igs_refine_step_args (include/igs_rast.h)."""
    _fields_ = [("stream", C.c_void_p),
                ("geometry_buffer", ALLOC_FN), ("geometry_user", C.c_void_p),
                ("binning_buffer", ALLOC_FN), ("binning_user", C.c_void_p),
                ("image_buffer", ALLOC_FN), ("image_user", C.c_void_p),
                ("workspace", C.c_void_p),
                ("P", C.c_int), ("D", C.c_int), ("M", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("background", C.c_void_p),
                ("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("grad_out", C.c_void_p),
                ("off_xyz", C.c_size_t), ("off_rot", C.c_size_t), ("off_sh", C.c_size_t), ("off_opacity", C.c_size_t),
                ("off_scale", C.c_size_t),
                ("lr_xyz", C.c_float), ("lr_rot", C.c_float), ("lr_sh", C.c_float), ("lr_opacity", C.c_float), ("lr_scale", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("step", C.c_int),
                ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("cam_pos", C.c_void_p),
                ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
                ("gt", C.c_void_p), ("loss_weight", C.c_float), ("lambda_dssim", C.c_float), ("lambda_depth_normal", C.c_float), ("depth_ratio", C.c_float),
                ("loss_scratch", C.c_void_p),
                ("out_images", C.c_void_p), ("radii", C.c_void_p), ("dL_dmean2D", C.c_void_p), ("loss_out", C.c_void_p),
                ("require_coord", C.c_int), ("require_depth", C.c_int), ("clamp_grads", C.c_float),
                ("color_grad_out", C.c_void_p), ("scratch_clean", C.c_int),
                ("gt_stats", C.c_void_p), ("gt_stats_valid", C.c_int), ("color_ready_event", C.c_void_p)]


class RefineMaskArgs(C.Structure):
    """igs_refine_mask_args (include/igs_rast.h): Gaussians [0, first_trainable) frozen, whole groups frozen by GROUP_* bit."""
    _fields_ = [("first_trainable", C.c_int), ("frozen_groups", C.c_uint)]


GROUP_XYZ, GROUP_ROT, GROUP_SH, GROUP_OPACITY, GROUP_SCALE = 1, 2, 4, 8, 16      # IGS_GROUP_*

_sz, _ll, _u = C.c_size_t, C.c_longlong, C.c_uint
_FORWARD = ([_vp, ALLOC_FN, _vp, ALLOC_FN, _vp, ALLOC_FN, _vp, _i, _i, _i, _vp, _i, _i]
            + [_vp] * 5 + [_f, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _i] + [_vp] * 8 + [_i, _i, _i])
_STATUS = [C.POINTER(C.c_int), C.POINTER(_u), C.POINTER(_u)]

# name: (restype, argtypes) of every function of include/igs_rast.h this binding declares, applied by lib().  One entry per function: a
# wrong count here corrupts memory instead of failing, so tests/test_host_logic.py checks every length against the header.
SIGNATURES = {
    # the rasterizer (api.hip)
    "igs_rast_version": (_i, []),
    "igs_rast_last_error": (C.c_char_p, []),
    "igs_rast_forward": (_i, _FORWARD),
    "igs_rast_forward_async": (_i, _FORWARD),
    "igs_rast_forward_finish": (_i, []),
    "igs_rast_forward_nowait": (_i, _FORWARD),
    "igs_rast_last_status": (_i, _STATUS),
    "igs_rast_last_posted_status": (_i, _STATUS),
    "igs_rast_hint_scratch_clean": (None, [_i]),
    "igs_rast_count_gaussians": (_i, ([_vp, ALLOC_FN, _vp, ALLOC_FN, _vp, ALLOC_FN, _vp, _i, _i, _i, _vp, _i, _i]
                                      + [_vp] * 5 + [_f, _vp, _vp, _vp, _vp, _vp, _f, _f, _i] + [_vp] * 4 + [_i])),
    "igs_rast_set_slab_hint": (None, [_u]),
    "igs_rast_get_slab_hint": (_u, []),
    "igs_rast_backward_workspace_bytes": (_sz, [_i]),
    "igs_rast_backward": (_i, ([_vp, _i, _i, _i, _i, _vp, _i, _i] + [_vp] * 5 + [_f, _vp, _vp, _vp, _vp, _vp, _f, _f, _f]
                               + [_vp] * 5 + [_vp] * 7 + [_vp] + [_vp] * 8 + [_i, _i, _i])),
    # V views of one Gaussian set: the two lists above with V behind the stream, [V] user / buffer / count arrays, and num_rendered [V]
    "igs_rast_views_max": (_i, []),
    "igs_rast_forward_views": (_i, [_vp, _i] + _FORWARD[1:-3] + [_vp, _i, _i, _i]),
    "igs_rast_backward_views": (_i, ([_vp, _i, _i, _i, _i, _vp, _vp, _i, _i] + [_vp] * 5 + [_f, _vp, _vp, _vp, _vp, _vp, _f, _f, _f]
                                     + [_vp] * 5 + [_vp] * 7 + [_vp] + [_vp] * 8 + [_i, _i, _i])),
    "igs_rast_mark_visible": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "igs_rast_debug_dump": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 8),
    "igs_rast_next_backward_options": (None, [_i, _f]),
    "igs_rast_nan_report_wait": (_i, []),
    "igs_rast_nan_report_handle": (_i, [_vp, _vp]),
    "igs_rast_nan_report_wait_at": (_i, [_vp, _u]),
    "igs_rast_last_backward_instance": (_i, []),
    "igs_rast_debug_poison_lds": (_i, [_vp]),
    "igs_rast_profile_enable": (_i, [_i]),
    "igs_rast_profile_read": (_i, [_vp, _vp, _vp, _vp, _i]),
    # optimiser, densification, activations, losses, PLY tables (refine_ops.hip, loss_ops.hip, io_ops.hip)
    "igs_adam_step": (_i, [_vp, _sz, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f]),
    "igs_adam_step_groups": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f]),
    "igs_adam_step_multi": (_i, [_vp, _i] + [_vp] * 8 + [_f, _f, _f]),
    "igs_adam_step_multi_dev": (_i, [_vp, _i] + [_vp] * 8 + [_f, _f, _f]),
    "igs_adam_step_multi_dev_scratch_words": (_sz, []),
    "igs_densify_stats": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "igs_densify_remap": (_i, [_vp, _i, _i] + [_vp] * 13),
    "igs_activate_fwd": (_i, [_vp, _i] + [_vp] * 6),
    "igs_activate_bwd": (_i, [_vp, _i] + [_vp] * 9),
    "igs_ssim_l1_scratch_bytes": (_sz, [_i, _i]),
    "igs_ssim_l1_loss_fwd_bwd": (_i, [_vp, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _vp]),
    "igs_ssim_gt_stats_bytes": (_sz, [_i, _i]),
    "igs_ssim_l1_loss_fwd_bwd_cached": (_i, [_vp, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _i]),
    "igs_ssim_mean_fwd_bwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "igs_depth_normal_loss_fwd_bwd": (_i, [_vp, _i, _i, _f, _f, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp]),
    "igs_l1_loss_fwd_bwd": (_i, [_vp, _sz, _vp, _vp, _vp, _vp, _f]),
    "igs_l1_mean_fwd_bwd": (_i, [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "igs_ply_to_params": (_i, [_vp, _i, _vp, _i, _vp, _i, _i] + [_vp] * 5),
    "igs_params_to_ply": (_i, [_vp, _i, _i] + [_vp] * 6),
    # the fused refine step (api.hip) and the N > 1 exchange (sh_exchange.hip)
    "igs_refine_step": (_i, [C.POINTER(RefineStepArgs)]),
    "igs_refine_step_args_size": (_sz, []),
    "igs_refine_step_masked": (_i, [C.POINTER(RefineStepArgs), C.POINTER(RefineMaskArgs)]),
    "igs_refine_mask_args_size": (_sz, []),
    "igs_refine_loss_scratch_bytes": (_sz, [_i, _i]),
    "igs_sh_grad_from_view_colors": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp]),
    "igs_adam_sh_from_view_colors": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f]),
    "igs_adam_exchange_step": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp] + [_sz] * 5 + [_f] * 10),
    # radix_sort.hip (Morton order), tile_sort.hip (debug)
    "igs_morton_order_scratch_bytes": (_sz, [_i]),
    "igs_morton_order": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp]),
    "igs_debug_tile_sort": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i]),
    # knn.hip, anchors.hip
    "igs_knn_scratch_bytes": (_sz, [_i]),
    "igs_knn_mean_dist2": (_i, [_vp, _i, _vp, _vp, _vp]),
    "igs_bbox_select_scratch_bytes": (_sz, [_i]),
    "igs_bbox_select": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "igs_fps_scratch_bytes": (_sz, [_i, _i, _i]),
    "igs_fps": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp]),
    "igs_knn_query": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp]),
    # motion.hip
    "igs_anchor_interp_fwd": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "igs_anchor_interp_index_bytes": (_sz, [_i, _i, _i, _i]),
    "igs_anchor_interp_index": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "igs_anchor_interp_bwd": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "igs_gaussian_deform_fwd": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "igs_gaussian_deform_bwd": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # lift.hip
    "igs_anchor_lift_scratch_bytes": (_sz, [_i] * 7),
    "igs_anchor_lift_bwd_scratch_bytes": (_sz, [_i] * 7),
    "igs_anchor_lift_fwd": (_i, [_vp] + [_i] * 7 + [_vp] + [_ll] * 4 + [_vp] * 4 + [_ll] * 2 + [_vp]),
    "igs_anchor_lift_bwd": (_i, [_vp] + [_i] * 7 + [_vp] * 4 + [_ll] * 2 + [_vp] + [_ll] * 4 + [_vp]),
    # cond.hip
    "igs_ray_condition_fwd": (_i, [_vp] + [_i] * 5 + [_vp] * 3),
    "igs_modln_bwd_scratch_bytes": (_sz, [_i] * 4),
    "igs_modln_fwd": (_i, [_vp] + [_i] * 5 + [_vp] + [_ll] * 4 + [_i] + [_vp] * 3 + [_f] + [_vp] * 3),
    "igs_modln_bwd": (_i, [_vp] + [_i] * 5 + [_vp] + [_ll] * 4 + [_i] + [_vp] * 11),
    # cond_fused.hip
    "igs_condition3d_pack_elems": (_ll, [_i] * 3),
    "igs_condition3d_fwd": (_i, [_vp] + [_i] * 8 + [_vp] + [_ll] * 4 + [_vp] * 2 + [_i] + [_vp] * 4 + [_f] + [_vp]),
    # cond_fused_bwd.hip
    "igs_condition3d_bwd_scratch_bytes": (_ll, [_i] * 5),
    "igs_condition3d_bwd": (_i, [_vp] + [_i] * 8 + [_vp] + [_ll] * 4 + [_vp] * 2 + [_i] + [_vp] * 5 + [_f] + [_vp] * 2 + [_ll] + [_vp] * 7),
    # upconv.hip
    "igs_upconv_pack_elems": (_ll, [_i] * 3),
    "igs_upconv_fwd": (_i, [_vp] + [_i] * 6 + [_vp] + [_ll] * 4 + [_i] + [_vp] * 3),
    # upconv_bwd.hip
    "igs_upconv_bwd_scratch_bytes": (_ll, [_i] * 6),
    "igs_upconv_bwd": (_i, [_vp] + [_i] * 6 + [_vp] + [_ll] * 4 + [_i] + [_vp] * 3 + [_ll] + [_vp] * 3),
    # attn.hip
    "igs_attn_bwd_scratch_bytes": (_sz, [_i] * 6),
    "igs_attn_fwd": (_i, [_vp] + [_i] * 6 + ([_vp] + [_ll] * 3) * 3 + [_f] + [_vp] + [_ll] * 3 + [_vp]),
    "igs_attn_bwd": (_i, [_vp] + [_i] * 6 + ([_vp] + [_ll] * 3) * 4 + [_vp] + [_vp] + [_ll] * 3 + [_f] + ([_vp] + [_ll] * 3) * 3 + [_vp]),
    # wattn.hip
    "igs_window_attn_bwd_scratch_bytes": (_sz, [_i] * 6),
    "igs_window_attn_fwd": (_i, [_vp] + [_i] * 7 + ([_vp] + [_ll] * 2) * 3 + [_f] + [_vp] + [_ll] * 2 + [_vp]),
    "igs_window_attn_bwd": (_i, [_vp] + [_i] * 7 + ([_vp] + [_ll] * 2) * 4 + [_vp] + [_vp] + [_ll] * 2 + [_f] + ([_vp] + [_ll] * 2) * 3 + [_vp]),
    # inorm.hip
    "igs_instance_norm_fwd": (_i, [_vp] * 4 + [_ll] * 2 + [_i] * 2 + [_f]),
    "igs_instance_norm_resident_max": (_ll, [_i] * 2),
    "igs_position_add": (_i, [_vp] * 5 + [_i] * 6),
    # tokens.hip
    "igs_layer_norm_fwd": (_i, [_vp, _ll, _i] + [_i, _vp, _ll] * 2 + [_vp, _vp, _f] + [_i, _vp, _ll]),
    "igs_layer_norm_bwd_scratch_bytes": (_sz, [_ll, _i]),
    "igs_layer_norm_bwd": (_i, [_vp, _ll, _i] + [_i, _vp, _ll] + [_vp, _f] + [_i, _vp, _ll] * 2 + [_vp] * 3),
    "igs_geglu_fwd": (_i, [_vp, _ll, _i, _i, _vp, _ll, _vp]),
    "igs_geglu_bwd": (_i, [_vp, _ll, _i, _i, _vp, _ll, _vp, _vp]),
    # gnorm.hip
    "igs_group_norm_tokens_fwd": (_i, [_vp, _i, _i, _i, _ll] + [_i, _vp, _ll, _ll] + [_vp, _vp, _f] + [_i, _vp, _ll] + [_vp]),
    "igs_group_norm_tokens_bwd_scratch_bytes": (_sz, [_i, _i, _i, _ll]),
    "igs_group_norm_tokens_bwd": (_i, [_vp, _i, _i, _i, _ll] + [_i, _vp, _ll, _ll] + [_vp, _vp] + [_i, _vp, _ll] + [_i, _vp, _ll, _ll] + [_vp] * 3),
    "igs_tokens_add_residual": (_i, [_vp, _i, _i, _ll] + [_i, _vp, _ll] + [_i, _vp, _ll, _ll] + [_i, _vp, _ll]),
    # mlp.hip
    "igs_mlp_heads_pack_elems": (_ll, [_i, _vp, _i, _vp]),
    "igs_mlp_heads_fwd": (_i, [_vp, _ll, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _ll, _vp, _vp, _vp]),
    "igs_mlp_heads_bwd_scratch_bytes": (_ll, [_ll, _i, _i, _vp, _i, _vp]),
    "igs_mlp_heads_bwd": (_i, [_vp, _ll, _i, _i, _i, _vp, _vp, _i, _vp] + [_vp, _ll, _vp, _vp, _vp] + [_vp, _vp, _ll] + [_vp, _vp, _vp]),
    # ffn.hip
    "igs_layer_tail_pack_elems": (_ll, [_i, _i]),
    "igs_layer_tail_fwd": (_i, [_vp, _ll, _i, _i, _i] + [_vp, _i, _ll] * 2 + [_vp, _vp, _vp, _f, _vp, _vp, _f] + [_vp, _i, _ll]),
    # ffn_bwd.hip
    "igs_layer_tail_bwd_scratch_bytes": (_ll, [_ll, _i, _i, _i]),
    "igs_layer_tail_bwd": (_i, [_vp, _ll, _i, _i, _i] + [_vp, _i, _ll] * 3 + [_vp, _vp, _vp, _vp, _f, _vp, _vp, _f] + [_vp, _ll]
                           + [_vp, _i, _ll] * 2 + [_vp] * 7),
    # proj.hip
    "igs_token_proj_pack_elems": (_ll, [_i]),
    "igs_token_proj_fwd": (_i, [_vp, _ll, _i, _i] + [_vp, _i, _ll] + [_vp, _vp] + [_vp, _i, _ll]),
    "igs_token_proj_bwd_scratch_bytes": (_ll, [_ll, _i]),
    "igs_token_proj_bwd": (_i, [_vp, _ll, _i, _i] + [_vp, _i, _ll] + [_vp, _i, _vp] + [_vp, _vp] + [_vp, _ll] + [_vp, _i, _ll] + [_vp]),
    # ssim_batch.hip
    "igs_ssim_batch_scratch_bytes": (_ll, [_i] * 5),
    "igs_ssim_batch_fwd_bwd": (_i, [_vp] + [_i] * 4 + [_vp, _vp, _f, _f] + [_vp] * 5),
    # densify.hip
    "igs_densify_plan_scratch_bytes": (_sz, [_i]),
    "igs_densify_plan": (_i, [_vp, _i] + [_vp] * 7 + [_f] * 4 + [_ll, _i] + [_vp] * 7),
}
EXPORTS = list(SIGNATURES)

VERSION = 4       # IGS_RAST_VERSION this binding was written against (include/igs_rast.h)

STAGES = ["preprocess", "depth_sort", "scan", "emit", "tile_sort", "ranges", "blend_fwd", "memset", "blend_bwd", "geom_bwd"]


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    try:
        path = _build.build()
    except Exception as e:  # noqa: BLE001
        # no hipcc on this box (or the build failed): the library that travelled with the tree is used only if it was built from
        # exactly these sources -- a stale one with another igs_refine_step_args layout would corrupt memory instead of failing
        if os.path.exists(_build.LIB) and not _build.needs_build():
            path = _build.LIB
        elif os.path.exists(_build.LIB):
            raise RuntimeError("igs_amd: libigs_rast.so is present but was built from other sources (build.stamp does not match) "
                               "and rebuilding it failed: %s" % e)
        else:
            raise RuntimeError("igs_amd: the HIP extension libigs_rast.so is missing and could not be built: %s" % e)
    # Load order matters: the library needs libamdhip64, and so does PyTorch, which ships its own copy.  Whichever is mapped
    # first serves both; if ours (from /opt/rocm) came first, torch would bring a SECOND runtime and the two would not share
    # the device (symptom: hipGetDevice -> "no ROCm-capable device is detected").  Device memory and streams come from torch
    # on this path, so torch's runtime goes first.
    import torch  # noqa: F401
    L = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.igs_rast_version() != VERSION:
        raise RuntimeError("igs_amd: libigs_rast.so reports C-ABI version %d, this binding needs %d" % (L.igs_rast_version(), VERSION))
    if L.igs_refine_step_args_size() != C.sizeof(RefineStepArgs):
        raise RuntimeError("igs_amd: igs_refine_step_args is %d bytes in the library, %d in the binding"
                           % (L.igs_refine_step_args_size(), C.sizeof(RefineStepArgs)))
    if L.igs_refine_mask_args_size() != C.sizeof(RefineMaskArgs):
        raise RuntimeError("igs_amd: igs_refine_mask_args is %d bytes in the library, %d in the binding"
                           % (L.igs_refine_mask_args_size(), C.sizeof(RefineMaskArgs)))
    _LIB = L
    return L


_EXT = None


def ext():
    """The compiled `_C` module (igs_amd/_C.*.so, igs_amd/csrc_torch/igs_torch_ext.cpp), built in-tree on first use.  No fallback:
    raises if it cannot be built or does not match the C-ABI library."""
    global _EXT
    if _EXT is not None:
        return _EXT
    lib()                                   # libigs_rast.so first (build / stamp / version checks; torch's HIP runtime mapped before ours)
    from . import build_ext as _bx
    try:
        _bx.build()
    except Exception as e:  # noqa: BLE001
        if not (os.path.exists(_bx.TARGET) and not _bx.needs_build()):
            raise RuntimeError("igs_amd: the compiled _C module is missing or stale and could not be built: %s" % e)
    import importlib
    m = importlib.import_module("igs_amd._C")
    if m.abi_version() != VERSION:
        raise RuntimeError("igs_amd: the compiled _C module was built against C-ABI version %d, this binding needs %d" % (m.abi_version(), VERSION))
    _EXT = m
    return m


def last_backward_instance():
    """{coord, depth, normal, absgrad} of the blend-backward instance the last backward on this thread launched, or None."""
    b = lib().igs_rast_last_backward_instance()
    if b < 0:
        return None
    return dict(coord=bool(b & 1), depth=bool(b & 2), normal=bool(b & 4), absgrad=bool(b & 8))


def last_error():
    return lib().igs_rast_last_error().decode("utf-8", "replace")


def profile_enable(on=True, every=1):
    """Stage marks on every `every`-th frame (an event record costs a few microseconds of stream time)."""
    lib().igs_rast_profile_enable(int(every) if on else 0)


def profile_read(reset=True):
    """{stage: (ms_sum, count)}, sum of num_rendered, number of forward calls."""
    n = len(STAGES)
    ms = (C.c_double * n)()
    cnt = (C.c_longlong * n)()
    r = C.c_double(0)
    calls = C.c_longlong(0)
    lib().igs_rast_profile_read(ms, cnt, C.byref(r), C.byref(calls), int(bool(reset)))
    return {STAGES[i]: (ms[i], cnt[i]) for i in range(n)}, r.value, calls.value
