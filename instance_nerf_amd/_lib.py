"""ctypes binding of libinr_hip.so (the C ABI in include/inr.h).

There is NO fallback: if the library is missing or a call is made without a
GPU tensor the caller gets a RuntimeError.  torch is imported first so that the
library binds to the HIP runtime already loaded by PyTorch-ROCm (same
``libamdhip64.so.7`` soname), which makes torch's streams and allocations
directly usable by the kernels.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_uint32, c_void_p

import torch  # noqa: F401  (must precede CDLL: shares the HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("INR_LIB_PATH") or os.path.join(_HERE, "csrc", "libinr_hip.so")   # env override: profiling builds only
MAX_LEVELS = 16
GRID_FX_STATE_FLOATS = 4192      # include/inr.h INR_GRID_FX_STATE_FLOATS
ROI_MAX_LEVELS = 8               # include/inr.h INR_ROI_MAX_LEVELS
NUMERICS_TABLE_F16, NUMERICS_MLP_F16 = 1, 2      # include/inr.h INR_NUMERICS_*
RAY_TABLE_FLOATS = 24            # include/inr.h INR_RAY_TABLE_FLOATS
SSIM_TAPS, SSIM_TILE_W, SSIM_TILE_H = 11, 64, 16    # include/inr.h INR_SSIM_TAPS, INR_SSIM_TILE_W, INR_SSIM_TILE_H
# include/inr.h INR_CONFUSION_MAX_K, INR_CONFUSION_BLOCK, INR_CONFUSION_PIXELS_PER_WG
CONFUSION_MAX_K, CONFUSION_BLOCK, CONFUSION_PIXELS_PER_WG = 64, 256, 1024
# include/inr.h INR_BOX_MATCH_MAX_GT, INR_BOX_MATCH_BLOCK, INR_BOX_MATCH_BOXES_PER_WG
BOX_MATCH_MAX_GT, BOX_MATCH_BLOCK, BOX_MATCH_BOXES_PER_WG = 1024, 256, 1024
# include/inr.h INR_FCOS_MAX_LEVELS, INR_FCOS_MAX_GT, INR_FCOS_BLOCK, INR_FCOS_LOCATIONS_PER_WG, INR_FCOS_LOSS_LOCATIONS_PER_WG
FCOS_MAX_LEVELS, FCOS_MAX_GT, FCOS_BLOCK, FCOS_LOCATIONS_PER_WG, FCOS_LOSS_LOCATIONS_PER_WG = 8, 1024, 256, 256, 1024
FCOS_LOSS_IOU, FCOS_LOSS_LINEAR_IOU, FCOS_LOSS_GIOU = 0, 1, 2      # include/inr.h INR_FCOS_LOSS_*


class GridDesc(Structure):
    _fields_ = [("num_levels", c_int32), ("level_dim", c_int32),
                ("offsets", c_uint32 * (MAX_LEVELS + 1)), ("scales", c_float * MAX_LEVELS),
                ("resolutions", c_uint32 * MAX_LEVELS), ("hashed", c_uint32 * MAX_LEVELS)]


P = c_void_p
_SIGS = {
    "inr_abi_version": (c_int32, []),
    "inr_last_error": (c_char_p, []),
    "inr_set_overlap_placement": (c_int32, [c_int32]),
    "inr_set_march_mode": (c_int32, [c_int32]),
    "inr_device_info": (c_int32, [c_int32, POINTER(c_int64)]),
    "inr_get_rays": (c_int32, [P, c_int64, c_float, c_float, c_float, c_float, c_int32, P, c_int64, P, P, P]),
    "inr_sample_training_batch": (c_int32, [P, c_float, c_float, c_float, c_float, c_int32, c_int32, P, c_int32, P, c_int32,
                                            c_int64, c_int64, c_int64, P, P, P, P, P, P]),
    "inr_sample_training_batch_weighted": (c_int32, [P, c_float, c_float, c_float, c_float, c_int32, c_int32, P, c_int32, P,
                                                     c_int32, P, c_int32, c_int64, c_int64, c_int64, P, P, P, P, P, P, P]),
    "inr_error_map_update": (c_int32, [P, P, P, P, c_int64, c_int32, P]),
    "inr_near_far_from_aabb": (c_int32, [P, P, P, c_int64, c_float, P, P, P]),
    "inr_near_far_from_aabb_skip": (c_int32, [P, P, P, c_int64, c_float, P, c_int64, P, P, P]),
    "inr_morton3D": (c_int32, [P, c_int64, P, P]),
    "inr_morton3D_invert": (c_int32, [P, c_int64, P, P]),
    "inr_packbits": (c_int32, [P, c_int64, c_float, P, P]),
    "inr_mark_untrained_grid": (c_int32, [P, c_int32, c_float, c_float, c_float, c_float, c_int32, c_int32, c_float, P, P]),
    "inr_occ_cell_positions": (c_int32, [P, P, c_int64, c_int32, c_float, P, P]),
    "inr_occ_update": (c_int32, [P, P, P, c_int64, c_int64, c_float, c_float, P, P, P]),
    "inr_packbits_mean": (c_int32, [P, c_int64, P, c_float, P, P, P, c_int32, c_int32, P, P]),
    "inr_occ_sample_workspace_bytes": (c_int64, [c_int64]),
    "inr_occ_sample_cells": (c_int32, [P, c_int64, P, c_int64, P, P, P]),
    "inr_march_write_fills_unowned_rows": (c_int32, [c_int64, c_int32, c_int32]),
    "inr_march_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "inr_march_rays_train_count": (c_int32, [P, P, P, c_float, c_float, c_int32, c_int64, c_int32, c_int32,
                                             P, P, P, P, P, P, c_int32, P]),
    "inr_march_rays_train_write": (c_int32, [P, P, P, c_float, c_float, c_int32, c_int64, c_int32, c_int32,
                                             c_int64, P, P, P, P, P, P, P, P, c_int32, P]),
    "inr_march_rays_patch_write": (c_int32, [P, P, P, c_float, c_float, c_int32, c_int64, c_int32, c_int32,
                                             c_int64, P, P, P, P, P, P, P, P, c_int32, P, c_int32, P]),
    "inr_nerf_bwd_packed_floats": (c_int64, []),
    "inr_nerf_pack_weights_device": (c_int32, [P, P, P, P, P, P, P, P]),
    "inr_nerf_forward_train": (c_int32, [P, P, c_int64, c_float, P, POINTER(GridDesc), P, P, P, P, P, P, P, P, P, P]),
    "inr_nerf_backward": (c_int32, [P, P, P, P, P, P, P, c_int64, c_float, P, P, P, P, P, P, P, P]),
    "inr_instance_bwd_packed_floats": (c_int64, []),
    "inr_instance_pack_weights_device": (c_int32, [P, P, P, c_int32, P, P, P]),
    "inr_instance_forward_train": (c_int32, [P, c_int64, c_float, P, POINTER(GridDesc), P, c_int32, P, P, P, P, P]),
    "inr_instance_backward": (c_int32, [P, c_int32, P, P, c_int64, P, P, P, P, P]),
    "inr_nerf_forward_enc": (c_int32, [P, P, c_int64, c_float, P, POINTER(GridDesc), P, P, P, P, P]),
    "inr_nerf_head_backward": (c_int32, [P, P, P, P, c_int64, c_float, P, P, P, P, P, P, P, P, P, P, c_int64, P]),
    "inr_instance_forward_enc": (c_int32, [P, c_int64, P, c_float, P, POINTER(GridDesc), P, c_int32, P, P, P]),
    "inr_instance_head_workspace_bytes": (c_int64, []),
    "inr_instance_head_backward": (c_int32, [P, P, P, P, c_int32, c_int64, c_int64, P, P, P, P, P, P, P, P, P, P, P, c_int64, P]),
    "inr_adam_step_multi": (c_int32, [c_int32, P, P, P, P, P, P, c_float, c_float, c_float, c_int32, c_float, P]),
    "inr_adam_ema_step_multi": (c_int32, [c_int32, P, P, P, P, P, P, c_float, c_float, c_float, c_int32, c_float, P,
                                          c_float, P]),
    "inr_adam_set_hyper": (c_int32, [P, c_int32, c_float, c_float, c_float, c_int32, P, P]),
    "inr_adam_step_multi_dev": (c_int32, [c_int32, P, P, P, P, P, P, c_float, c_float, c_float, P]),
    "inr_copy_multi": (c_int32, [c_int32, P, P, P, P]),
    "inr_adam_set_hyper_ema": (c_int32, [P, c_int32, c_float, c_float, c_float, c_int32, c_float, P, P]),
    "inr_adam_ema_step_multi_dev": (c_int32, [c_int32, P, P, P, P, P, P, c_float, c_float, c_float, P, P]),
    "inr_cross_entropy": (c_int32, [P, P, c_int64, c_int32, c_int64, P, P, P, P]),
    "inr_finish_rays": (c_int32, [P, P, P, P, P, P, c_float, c_float, c_float, c_int64, P, P, P]),
    "inr_finish_rays_mse": (c_int32, [P, P, P, P, P, c_float, c_float, c_float, P, P, c_int64, P, P, P, P, P]),
    "inr_sh_table_q": (c_int32, [P, c_int64, P, P]),
    "inr_nerf_forward_table": (c_int32, [P, P, P, c_int64, c_float, P, POINTER(GridDesc), P, c_float, P, P, c_int32, P]),
    "inr_nerf_forward_table_sliced_workspace_bytes": (c_int64, [c_int64]),
    "inr_nerf_forward_table_sliced": (c_int32, [P, P, P, c_int64, c_float, P, POINTER(GridDesc), P, c_float, P, P, P, P]),
    "inr_composite_rays_patch_forward": (c_int32, [P, P, P, P, c_int64, c_int64, c_float, P, c_int32, P, P, P, P, P, P, P]),
    "inr_march_rays_patch_write_records": (c_int32, [P, P, P, c_float, c_float, c_int32, c_int64, c_int32, c_int32,
                                                     c_int64, P, P, P, P, P, P, P, c_int32, P]),
    "inr_composite_rays_patch_forward_records": (c_int32, [P, P, P, P, c_int64, c_int64, c_float, P, P, c_float, c_int32,
                                                           c_int32, c_int32, P, c_int32, P, P, P, P, P, P, P]),
    "inr_ray_table_q": (c_int32, [P, P, c_int64, P, P]),
    "inr_nerf_forward_table_records": (c_int32, [P, P, P, c_int64, c_float, P, POINTER(GridDesc), P, c_float, P, P, c_int32, P]),
    "inr_project_masks_patch": (c_int32, [P, P, P, c_int64, c_int64, P, c_int32, c_int32, c_int32, P, c_int32, c_int32, c_int32,
                                          P, P]),
    "inr_march_rays": (c_int32, [c_int64, c_int32, P, P, P, P, c_float, c_float, c_int32, c_int32, c_int32,
                                 P, P, P, P, P, P, P]),
    "inr_composite_rays": (c_int32, [c_int64, c_int32, P, P, P, P, P, P, P, P, c_float, P, P, c_int32, P]),
    "inr_compact_alive": (c_int32, [P, c_int64, P, P, P]),
    "inr_composite_rays_extra_forward": (c_int32, [P, P, P, c_int64, c_int64, c_int32, P, P, c_int32, c_int64, P, P, P, P]),
    "inr_composite_rays_train_forward": (c_int32, [P, P, P, P, c_int64, c_int64, c_float, P, c_int32, P, P, P, P, P, P, P]),
    "inr_composite_rays_train_backward": (c_int32, [P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_float, c_int32,
                                                    P, P, P, P, P]),
    "inr_grid_encode_forward": (c_int32, [P, P, POINTER(GridDesc), c_int64, c_float, P, P]),
    "inr_grid_encode_backward": (c_int32, [P, P, POINTER(GridDesc), c_int64, c_float, P, P]),
    "inr_grid_encode_backward_ordered": (c_int32, [P, P, P, POINTER(GridDesc), c_int64, c_float, P, P]),
    "inr_grid_encode_backward_input": (c_int32, [P, P, P, POINTER(GridDesc), c_int64, c_float, P, P]),
    "inr_grid_encode_backward_levels": (c_int32, [P, P, P, POINTER(GridDesc), c_int64, c_float, P, c_int32, c_int32, P]),
    "inr_grid_encode_backward_levels_fx": (c_int32, [P, P, P, POINTER(GridDesc), c_int64, c_float, P, c_int32, c_int32, P, P]),
    "inr_grid_grad_finish_fx": (c_int32, [P, POINTER(GridDesc), c_int32, c_int32, P, P]),
    "inr_grid_fx_update": (c_int32, [P, c_int32, c_float, c_int32, P]),
    "inr_grid_encode_backward_levels_fx64": (c_int32, [P, P, P, POINTER(GridDesc), c_int64, c_float, P, P, c_int32, c_int32, P, P]),
    "inr_grid_grad_finish_fx64": (c_int32, [P, P, POINTER(GridDesc), c_int32, c_int32, P, P]),
    "inr_sh_encode_forward": (c_int32, [P, c_int64, c_int32, P, P]),
    "inr_sh_encode_backward": (c_int32, [P, P, c_int64, c_int32, P, P]),
    "inr_nerf_packed_floats": (c_int64, []),
    "inr_nerf_pack_weights": (c_int32, [P, P, P, P, P, P, c_int32]),
    "inr_instance_packed_floats": (c_int64, [c_int32]),
    "inr_instance_pack_weights": (c_int32, [P, P, P, c_int32, P, c_int32]),
    "inr_nerf_forward": (c_int32, [P, P, c_int64, P, c_float, P, POINTER(GridDesc), P, c_float, P, P, P, c_int32, P]),
    "inr_nerf_forward_dirs": (c_int32, [P, c_int64, c_float, P, POINTER(GridDesc), P, P, c_int32, P, P]),
    "inr_nerf_forward_lattice": (c_int32, [P, P, P, c_int32, c_int32, c_int32, c_float, P, POINTER(GridDesc), P, P, c_int32,
                                           c_float, P, P]),
    "inr_instance_forward": (c_int32, [P, c_int64, P, c_float, P, POINTER(GridDesc), P, c_int32, P, P]),
    "inr_instance_lattice": (c_int32, [P, P, P, c_int32, c_int32, c_int32, c_float, P, POINTER(GridDesc), P, c_float,
                                       c_float, P, POINTER(GridDesc), P, c_int32, P, P, P, P]),
    "inr_instance_volume_stats": (c_int32, [P, P, c_int32, c_int32, c_int32, c_int32, P, c_int64, P, P, P, P]),
    "inr_mesh_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "inr_mesh_count": (c_int32, [P, c_int32, c_float, c_float, P, c_int32, c_int32, c_int32, c_int32, c_int32, P, c_int64, P, P]),
    "inr_mesh_emit": (c_int32, [P, c_int32, c_float, c_float, P, c_int32, P, P, P, P, c_int32, c_int32, c_int32, c_float,
                                c_float, c_float, c_int32, P, c_int64, c_int32, c_int32, P, P, P, P, P]),
    "inr_components_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "inr_components_label": (c_int32, [P, c_int32, c_int32, c_int32, c_int32, P, c_int64, P, P]),
    "inr_components_filter": (c_int32, [P, P, P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, P, c_int64,
                                        P, P, P, P, P, P]),
    "inr_pack_mask_bits": (c_int32, [P, P, c_int64, c_int32, c_float, c_int64, P, P]),
    "inr_match_count": (c_int32, [P, P, c_int64, c_int64, c_int32, c_int32, P, P, P, P, P]),
    "inr_match_assign": (c_int32, [P, P, P, P, P, c_int64, c_int64, c_int32, c_int32, P, P, P, P]),
    "inr_pack_mask_planes": (c_int32, [P, c_int32, c_int64, P, P, P]),
    "inr_pack_label_planes": (c_int32, [P, c_int64, c_int32, c_int32, P, P, P]),
    "inr_mask_overlap": (c_int32, [P, c_int32, P, c_int32, c_int64, c_int32, P, P]),
    "inr_paste_masks": (c_int32, [P, P, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, P, P, P, P]),
    "inr_planes_to_voxel_words": (c_int32, [P, c_int32, c_int64, c_int32, P, P]),
    "inr_nms_3d_pairs": (c_int32, [P, P, c_int32, c_float, P, P]),
    "inr_nms_3d_scan": (c_int32, [P, c_int32, P, P, P]),
    "inr_roi_align_3d_set_mode": (c_int32, [c_int32]),
    "inr_roi_align_3d_forward": (c_int32, [P, P, P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32,
                                           c_int32, c_int32, c_float, P, P]),
    "inr_roi_align_3d_backward": (c_int32, [P, P, P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32,
                                            c_int32, c_int32, c_float, P, P]),
    "inr_roi_align_3d_backward_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32,
                                                            c_int32, c_int32]),
    "inr_roi_align_3d_backward_prefers_workspace": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32,
                                                              c_int32, c_int32, c_int64]),
    "inr_roi_align_3d_backward_ws": (c_int32, [P, P, P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32,
                                               c_int32, c_int32, c_float, P, P, c_int64, P]),
    "inr_roi_align_3d_pyramid_forward": (c_int32, [P, P, P, c_int32, P, P, P, P, c_int32, c_int32, c_int64, c_int32,
                                                   c_int32, c_int32, P, P]),
    "inr_roi_align_3d_pyramid_backward": (c_int32, [P, P, P, c_int32, P, P, P, P, c_int32, c_int32, c_int64, c_int32,
                                                    c_int32, c_int32, P, P]),
    "inr_nerf_render": (c_int32, [P, P, P, P, c_int64, c_int64, c_float, P, POINTER(GridDesc), P, c_float, c_float,
                                  P, P, P, P, P, c_int32, c_int32, P]),
    "inr_instance_render": (c_int32, [P, P, P, c_int64, c_int64, c_float, P, POINTER(GridDesc), P, c_int32, P, c_int32, P,
                                      c_int32, P]),
    "inr_linear_wgrad_workspace_bytes": (c_int64, []),
    "inr_linear_wgrad": (c_int32, [P, P, c_int64, c_int32, c_int32, P, P, P]),
    "inr_adam_step": (c_int32, [P, P, P, P, c_int64, c_float, c_float, c_float, c_float, c_int32, c_float, P]),
    "inr_grid2d_encode_forward": (c_int32, [P, P, POINTER(GridDesc), c_int64, c_float, P, P]),
    "inr_grid2d_encode_backward": (c_int32, [P, P, POINTER(GridDesc), c_int64, c_float, P, P]),
    "inr_sph_from_ray": (c_int32, [P, P, c_int64, c_float, P, P]),
    "inr_background_forward": (c_int32, [P, P, c_int64, c_float, P, POINTER(GridDesc), P, P, P, P, P, P, P]),
    "inr_background_workspace_bytes": (c_int64, [c_int64]),
    "inr_background_backward": (c_int32, [P, P, P, c_int64, c_float, P, POINTER(GridDesc), P, P, P, P, P, P, P]),
    "inr_ssim_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int32]),
    "inr_ssim_forward": (c_int32, [P, P, c_int64, c_int64, c_int64, c_int32, P, P, P, P, P, P, c_int64, P]),
    "inr_confusion_ids": (c_int32, [P, P, c_int64, c_int64, c_int32, P, P, P]),
    "inr_confusion_logits": (c_int32, [P, P, c_int64, c_int64, c_int32, c_int64, P, P, P]),
    "inr_box_match_gt_max": (c_int32, [P, c_int32, P, P, c_int64, P, P]),
    "inr_box_match_assign": (c_int32, [P, P, c_int32, P, P, c_int64, P, c_float, c_float, c_int32, P, P, P, P, P, P]),
    "inr_fcos_targets": (c_int32, [P, P, P, c_int32, c_int32, P, P, c_int32, P, c_float, c_int32, P, P, P, P, P, P]),
    "inr_fcos_loss_workspace_bytes": (c_int64, [c_int64]),
    "inr_fcos_loss_forward": (c_int32, [P, P, P, P, c_int32, c_int32, P, P, P, c_int32, P, P, P, P, P, P, c_int64, P]),
    "inr_fcos_loss_backward": (c_int32, [P, P, P, P, c_int32, c_int32, P, P, P, c_int32, P, P, P, P, P, P]),
}
EXPORTS = tuple(_SIGS)

ABI_VERSION = 13         # include/inr.h INR_ABI_VERSION this binding was written against
INSTANCE_STATS_WORKSPACE_BYTES = 512 * 64 * 8 * 4      # include/inr.h INR_INSTANCE_STATS_WORKSPACE_BYTES
_lib = None


def load():
    """Loads the library (once).  Raises RuntimeError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m instance_nerf_amd.build` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    # the version first: a stale library lacks the newer symbols, and binding them would fail with a bare AttributeError
    version = getattr(lib, "inr_abi_version", None)
    if version is not None:
        version.restype, version.argtypes = c_int32, []
    found = version() if version is not None else None
    if found != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} ABI version {found} != {ABI_VERSION} (include/inr.h "
                           "INR_ABI_VERSION): rebuild with `python -m instance_nerf_amd.build --force`")
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name, None)
        if fn is None:                  # exports added without a version bump (inr_ssim_*, inr_confusion_*, inr_box_match_*, inr_fcos_*): a library built before them
            raise RuntimeError(f"{LIB_PATH} does not export {name} (include/inr.h): rebuild with "
                               "`python -m instance_nerf_amd.build --force`")
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().inr_last_error()
        raise RuntimeError(f"libinr_hip {what} failed (code {rc}): {msg.decode() if msg else ''}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr():
    """The current HIP stream of the current device (every launch of the library goes on it).  The raw accessors cost
    ~0.3 us; ``torch.cuda.current_stream().cuda_stream`` ~10 us - a dozen calls per training step."""
    if _raw_stream is not None and _cur_device is not None:
        return c_void_p(_raw_stream(_cur_device()))
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=None, name="tensor", allow_none=False):
    """Device pointer of a contiguous GPU tensor, with the TORCH_CHECK-style
    argument validation the reference's extension does on the C++ side
    (/root/reference/nerf_rcnn/model/rotated_iou/cuda_op/utils.h:6-31)."""
    if t is None:
        if allow_none:
            return None
        raise RuntimeError(f"{name} must not be None")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    return c_void_p(t.data_ptr())


def ptr_or_null(t, dtype=None, name="tensor"):
    """``ptr`` for an argument the library takes as null when it holds no element: None or an empty tensor gives a null
    pointer (unchecked), anything else goes through ``ptr``."""
    return None if t is None or t.numel() == 0 else ptr(t, dtype, name)


def host_ptr(t, dtype, name="tensor"):
    if t.is_cuda or not t.is_contiguous() or t.dtype != dtype:
        raise RuntimeError(f"{name} must be a contiguous CPU {dtype} tensor")
    return c_void_p(t.data_ptr())


def make_grid_desc(table):
    """table: dict from gridencoder.level_table()."""
    d = GridDesc()
    L = int(table["num_levels"])
    d.num_levels = L
    d.level_dim = int(table["level_dim"])
    for i in range(L + 1):
        d.offsets[i] = int(table["offsets"][i])
    for i in range(L):
        d.scales[i] = float(table["scales"][i])
        d.resolutions[i] = int(table["resolutions"][i])
        d.hashed[i] = int(table["hashed"][i])
    return d
