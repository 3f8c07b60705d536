"""ctypes binding of the native libraries that _build.LIBRARIES describes: the C ABIs declared in include/rdf_hip.h,
include/rdf_frontend.h (the depth front end) and include/rdf_labels.h (glove colours to labels).

This is the only place the shared libraries are opened.  There is no CPU fallback: a missing
library, or a machine without a HIP device, raises.
"""
import ctypes
import os
import threading
import warnings

from . import _build

_c_int, _c_float, _c_void_p, _c_size_t = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t

# name -> (restype, argtypes); every symbol include/rdf_hip.h declares
SIGNATURES = {
    "rdf_eval_forest": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int,
                                 _c_void_p, _c_int, _c_void_p, _c_int, _c_float, _c_void_p]),
    "rdf_eval_tree": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p,
                               _c_void_p]),
    "rdf_composite": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p,
                               _c_void_p]),
    "rdf_layered_run": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                 _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p,
                                 _c_int, _c_float, _c_void_p]),
    "rdf_layered_run_hand": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                      _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p,
                                      _c_int, _c_float, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p]),
    "rdf_layered_run_hand_batch": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                            _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p,
                                            _c_void_p, _c_int, _c_float, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p]),
    "rdf_forest_packed_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
    "rdf_forest_pack": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_float, _c_void_p, _c_void_p]),
    "rdf_eval_forest_packed_stats": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p,
                                              _c_int, _c_void_p, _c_void_p]),
    "rdf_forest_set_deep_from": (_c_int, [_c_void_p, _c_int]),
    "rdf_forest_info": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int),
                                 ctypes.POINTER(_c_float)]),
    "rdf_forest_forget": (_c_int, [_c_void_p]),
    "rdf_forest_tune": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int,
                                 _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_eval_forest_packed": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int,
                                        _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p]),
    "rdf_eval_forest_packed_filled": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int,
                                               _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p]),
    "rdf_eval_forest_packed_split": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int,
                                              _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_int,
                                              _c_int, ctypes.POINTER(_c_int)]),
    "rdf_eval_forest_stats": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int,
                                       _c_void_p, _c_int, _c_void_p, _c_int, _c_float, _c_void_p, _c_void_p]),
    "rdf_mean_shift_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
    "rdf_mean_shift": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_fingertip_heights": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int,
                                       _c_float, _c_float, _c_float, _c_float, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_mean_shift_heights": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_int,
                                        _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_float, _c_float, _c_float, _c_void_p,
                                        _c_void_p, _c_void_p]),
    "rdf_mean_shift_heights_batch": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p,
                                              _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_float, _c_float, _c_float,
                                              _c_void_p, _c_void_p, _c_int, _c_void_p]),
    "rdf_convert_0s_to_maxuint": (_c_int, [_c_void_p, _c_size_t, _c_void_p]),
    "rdf_setup_depth_image_for_forest": (_c_int, [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "rdf_stencil_depth_image_by_group": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_flip_x": (_c_int, [_c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_prepare_hand_depth": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p]),
    "rdf_prepare_hand_depth_batch": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_int,
                                              _c_void_p]),
    "rdf_make_rgba_from_labels": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_shrink_image": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_write_pixel_groups_to_stencil_image": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_void_p]),
    "rdf_grow_groups": (_c_int, [_c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_hand_groups_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int, _c_int]),
    "rdf_hand_groups": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_void_p, _c_void_p, _c_void_p,
                                 _c_void_p, _c_void_p, _c_int, _c_void_p]),
    "rdf_train_init": (_c_int, [_c_void_p, _c_size_t, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_train_histogram": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int,
                                     _c_int, _c_int, _c_int, _c_void_p, _c_void_p]),
    "rdf_train_histogram_left": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int,
                                          _c_int, _c_int, _c_int, _c_void_p, _c_void_p]),
    "rdf_train_histogram_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
    "rdf_train_histogram_left_ws": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int,
                                             _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_train_sort_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
    "rdf_train_bits_row_bytes": (_c_size_t, [_c_int]),
    "rdf_train_sort_pixels": (_c_int, [_c_void_p, _c_void_p, _c_size_t, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_train_bits_workspace_bytes": (_c_size_t, [_c_int]),
    "rdf_train_decision_bits": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_train_count_rows": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p,
                                      _c_void_p]),
    "rdf_train_right_counts": (_c_int, [_c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p,
                                        _c_void_p]),
    "rdf_train_pick_best": (_c_int, [_c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                     _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_train_next_active": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "rdf_train_update_pixels": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p,
                                         _c_void_p]),
    "rdf_fill_u16": (_c_int, [_c_void_p, _c_size_t, ctypes.c_uint16, _c_void_p]),
    "rdf_stream_create_with_reserved_cus": (_c_int, [_c_void_p, _c_int]),
    "rdf_stream_destroy": (_c_int, [_c_void_p]),
    "rdf_stream_capture_id": (_c_int, [_c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "rdf_graph_slots_release": (_c_int, [ctypes.c_uint64]),
    "rdf_debug_sched_slots": (_c_int, [_c_void_p, _c_void_p]),
    "rdf_debug_host_overhead": (_c_int, [_c_void_p, _c_int]),
    "rdf_debug_kernel_launches": (_c_int, [_c_void_p, _c_int, _c_int]),
    "rdf_debug_kernel_key": (_c_int, [_c_int, _c_void_p]),
    "rdf_device_malloc": (_c_int, [_c_void_p, _c_size_t]),
    "rdf_device_free": (_c_int, [_c_void_p]),
    "rdf_ipc_export": (_c_int, [_c_void_p, _c_void_p]),
    "rdf_ipc_open": (_c_int, [_c_void_p, _c_void_p]),
    "rdf_ipc_close": (_c_int, [_c_void_p]),
    "rdf_memcpy_device_async": (_c_int, [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "rdf_debug_fat_kernel": (_c_int, [_c_int, ctypes.c_uint64, _c_void_p, _c_void_p]),
    "rdf_debug_floor_i32": (_c_int, [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "rdf_debug_div_f32": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "rdf_set_lds_budget_bytes": (None, [_c_int]),
    "rdf_set_block_threads": (None, [_c_int]),
    "rdf_set_scheduler": (None, [_c_int]),
    "rdf_set_compaction": (None, [_c_int]),
    "rdf_set_halo": (None, [_c_int]),
    "rdf_set_lds_levels": (None, [_c_int]),
    "rdf_set_tree_waves": (None, [_c_int]),
    "rdf_set_stage_vec": (None, [_c_int]),
    "rdf_set_group": (None, [_c_int]),
    "rdf_set_layers_one_launch": (None, [_c_int]),
    "rdf_set_rows_per_wave": (None, [_c_int]),
    "rdf_set_force_exact": (None, [_c_int]),
    "rdf_set_last_level_table": (None, [_c_int]),
    "rdf_set_deep_from": (None, [_c_int]),
    "rdf_set_fold": (None, [_c_int]),
    "rdf_set_plain_levels": (None, [_c_int]),
    "rdf_event_create": (_c_int, [ctypes.POINTER(_c_void_p)]),
    "rdf_event_record": (_c_int, [_c_void_p, _c_void_p]),
    "rdf_event_synchronize": (_c_int, [_c_void_p]),
    "rdf_event_elapsed_ms": (_c_int, [_c_void_p, _c_void_p, ctypes.POINTER(_c_float)]),
    "rdf_event_destroy": (_c_int, [_c_void_p]),
    "rdf_stream_synchronize": (_c_int, [_c_void_p]),
    "rdf_abi_version": (_c_int, []),
    "rdf_build_id": (ctypes.c_char_p, []),
    "rdf_error_string": (ctypes.c_char_p, [_c_int]),
}

ABI_VERSION = 5


class StereoConfig(ctypes.Structure):
    """RdfStereoConfig of include/rdf_labels.h, passed by value."""
    _fields_ = [("fb16", ctypes.c_int32), ("fbp16", ctypes.c_int32), ("max_disparity", ctypes.c_int32),
                ("dot_threshold", ctypes.c_uint32), ("pattern_seed", ctypes.c_uint32), ("ambient", ctypes.c_int32),
                ("ir_noise_amp", ctypes.c_int32), ("census_margin", ctypes.c_int32), ("uniqueness", ctypes.c_int32),
                ("lr_max", ctypes.c_int32), ("dq_min", ctypes.c_int32)]


class DepthFilterConfig(ctypes.Structure):
    """RdfDepthFilterConfig of include/rdf_frontend.h, passed by address (host memory)."""
    _fields_ = [(name, ctypes.c_int32) for name in ("spatial_radius", "spatial_delta", "temporal", "temporal_alpha", "temporal_delta",
                                                    "persist_need", "persist_span", "fill_mode", "max_gap")]


# library (a key of _build.LIBRARIES) -> (the ABI number this binding was written for, name -> (restype, argtypes) of every
# symbol its header declares)
BINDINGS = {
    "hip": (ABI_VERSION, SIGNATURES),
    "frontend": (2, {
        "rdf_make_plane_candidates": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                               _c_void_p]),
        "rdf_plane_inliers": (_c_int, [_c_int, _c_float, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_plane_select": (_c_int, [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_calibrate_plane_workspace_bytes": (_c_size_t, [_c_int]),
        "rdf_calibrate_plane": (_c_int, [_c_int, _c_float, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                         _c_void_p, _c_void_p]),
        "rdf_frame_front": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_float, _c_float, _c_float, _c_void_p, _c_float,
                                     _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_deproject_points": (_c_int, [_c_int, _c_int, _c_int, _c_float, _c_float, _c_float, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_transform_points": (_c_int, [_c_int, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_filter_points_by_plane": (_c_int, [_c_int, _c_float, _c_void_p, _c_void_p]),
        "rdf_remove_missing_3d_points_from_depth_image": (_c_int, [_c_int, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_gaussian_depth_filter": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_hand_state_bytes": (_c_size_t, [_c_int, _c_int]),
        "rdf_hand_state_init": (_c_int, [_c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_hand_state_set": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p]),
        "rdf_hand_state_step": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, ctypes.c_uint32,
                                         _c_void_p]),
        "rdf_depth_filter_state_bytes": (_c_size_t, [_c_int, _c_int]),
        "rdf_depth_filter": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, ctypes.POINTER(DepthFilterConfig), _c_void_p, _c_void_p,
                                      _c_void_p, _c_void_p]),
        "rdf_frontend_abi_version": (_c_int, []),
        "rdf_frontend_build_id": (ctypes.c_char_p, []),
        "rdf_frontend_error_string": (ctypes.c_char_p, [_c_int]),
    }),
    "labels": (1, {
        "rdf_split_pixels_by_nearest_color": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_apply_point_mapping": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_depths_from_points": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_color_mapping_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
        "rdf_make_color_mapping": (_c_int, [_c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                            _c_void_p]),
        "rdf_label_frame": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p,
                                     _c_void_p, _c_void_p]),
        "rdf_mask_color_image": (_c_int, [_c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p]),
        "rdf_points_center_workspace_bytes": (_c_size_t, [_c_int]),
        "rdf_points_center": (_c_int, [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_rerender_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
        "rdf_rerender": (_c_int, [_c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_float, _c_float, _c_float, _c_float,
                                  _c_float, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_score_counts_bytes": (_c_size_t, [_c_int]),
        "rdf_score_labels": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                      _c_void_p]),
        "rdf_hand_scene_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
        "rdf_hand_scene_render": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p,
                                           _c_int, _c_void_p, _c_void_p, _c_float, _c_float, _c_float, _c_float, _c_float,
                                           ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint32, _c_int, _c_void_p, _c_void_p,
                                           _c_void_p, _c_void_p]),
        "rdf_pose_cost": (_c_int, [_c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p,
                                   _c_void_p, ctypes.c_uint64, _c_void_p, _c_void_p]),
        "rdf_pose_propose": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_pose_select": (_c_int, [_c_int, _c_void_p, _c_void_p, ctypes.c_uint32, ctypes.c_uint32, _c_int, _c_void_p, _c_void_p,
                                     _c_void_p]),
        "rdf_pose_fit_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
        "rdf_pose_fit": (_c_int, [_c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int,
                                  _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_stereo_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int, _c_int]),
        "rdf_stereo_ir": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, StereoConfig, ctypes.c_uint32, _c_void_p, _c_void_p]),
        "rdf_stereo_sense": (_c_int, [_c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, StereoConfig, ctypes.c_uint32,
                                      ctypes.c_uint16, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_labels_refit_count": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_float,
                                            _c_void_p, _c_void_p, _c_void_p]),
        "rdf_labels_refit_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
        "rdf_labels_refit_apply": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, ctypes.c_uint64, _c_int, _c_void_p,
                                            _c_void_p, _c_void_p]),
        "rdf_labels_prune_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
        "rdf_labels_prune_plan": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, ctypes.c_uint64, ctypes.c_uint64, _c_int,
                                           _c_void_p, _c_void_p, _c_void_p]),
        "rdf_labels_prune_apply": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_labels_forest_posterior": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p,
                                                 _c_int, _c_int, _c_float, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_labels_confidence_counts": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p,
                                                  _c_void_p, _c_void_p]),
        "rdf_labels_composite_weights": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int,
                                                  _c_void_p, _c_void_p]),
        "rdf_labels_weighted_modes": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p,
                                               _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_float, _c_float,
                                               _c_float, _c_void_p, _c_void_p, _c_int, _c_void_p]),
        "rdf_labels_weighted_modes_list_cap": (ctypes.c_uint32, []),
        "rdf_labels_votes_count": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int,
                                            _c_float, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
        "rdf_labels_votes_fit": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                          _c_void_p, _c_void_p, _c_void_p]),
        "rdf_labels_votes_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int, _c_int, _c_int]),
        "rdf_labels_votes_cast": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int,
                                           _c_float, _c_void_p, _c_int, _c_int, _c_int, ctypes.c_uint32, _c_void_p, _c_void_p,
                                           _c_void_p]),
        "rdf_labels_vote_tips": (_c_int, [_c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int,
                                          _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_float, _c_float, _c_float, _c_void_p,
                                          _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p]),
        "rdf_labels_shape_pool": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int,
                                           _c_int, _c_float, _c_void_p, _c_void_p]),
        "rdf_labels_shape_decide": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p,
                                             _c_void_p]),
        "rdf_labels_abi_version": (_c_int, []),
        "rdf_labels_build_id": (ctypes.c_char_p, []),
        "rdf_labels_error_string": (ctypes.c_char_p, [_c_int]),
    }),
}
_loaded = {}
_load_lock = threading.Lock()     # two threads' first load() of a library: one opens and types it, both get that object


class RdfError(RuntimeError):
    pass


def _alternate(name):
    # RDF_HIP_LIBRARY: an alternate build of the same ABI for timing experiments on the forest kernel, so it redirects the
    # main library only, and being built from other sources on purpose it is exempt from the build-id check
    return os.environ.get("RDF_HIP_LIBRARY") if name == "hip" else None


def library_path(name="hip"):
    return _alternate(name) or _build.LIBRARIES[name].so


def load(name="hip"):
    """Open one of the libraries (librdf_hip.so by default) and type every entry point; once per process.  Raises if it has
    not been built, if its ABI number is not the one this binding was written for, or if it was built from other sources."""
    if name in _loaded:
        return _loaded[name]
    with _load_lock:
        return _loaded[name] if name in _loaded else _load(name)


def _load(name):
    prefix = _build.LIBRARIES[name].prefix
    path = library_path(name)
    if not os.path.exists(path):
        raise RdfError(f"{path} is missing: build it first (python __graft_entry__.py build, "
                       "or python 3d-beats_amd/_build.py). There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    abi, signatures = BINDINGS[name]
    for symbol, (res, args) in signatures.items():
        fn = getattr(lib, symbol)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = getattr(lib, prefix + "abi_version")()
    if got != abi:
        raise RdfError(f"{os.path.basename(path)} ABI {got} != expected {abi}; rebuild")
    check_build_id(lib, path, name)
    lib.error_string = getattr(lib, prefix + "error_string")    # for check()
    _loaded[name] = lib
    return lib


def check_build_id(lib, path, name="hip"):
    """The library must have been built from the sources that sit next to it: same ABI number, yesterday's kernels would
    otherwise pass every check.  RDF_HIP_LIBRARY and a deployment without sources are exempt; RDF_ALLOW_STALE_LIBRARY=1
    turns the refusal into a warning."""
    got = getattr(lib, _build.LIBRARIES[name].prefix + "build_id")()
    got = got.decode() if isinstance(got, bytes) else str(got)
    if _alternate(name) or not _build.sources_present(name):
        return got
    want = _build.source_id(name)
    if got != want:
        msg = (f"{path} was built from other sources (build id {got}, sources {want}): rebuild it "
               "(python __graft_entry__.py build).")
        if os.environ.get("RDF_ALLOW_STALE_LIBRARY") != "1":
            raise RdfError(msg)
        warnings.warn(msg)
    return got


def check(lib, code, what):
    if code != 0:
        # a handle from load() names its library's error strings; anything else offers rdf_error_string
        msg = (getattr(lib, "error_string", None) or lib.rdf_error_string)(int(code))
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        raise RdfError(f"{what} failed: {msg} (code {code})")
