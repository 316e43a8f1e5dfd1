"""ctypes bindings of include/metro_hip.h.  Loading fails loudly: there is NO CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('METRO_HIP_LIB') or os.path.join(HERE, 'libmetro_hip.so')   # override: timing experiments

METRO_MAX_JOINTS = 64
ABI_VERSION = 8          # include/metro_hip.h METRO_ABI_VERSION
METRO_PREC_F16, METRO_PREC_F32, METRO_PREC_F64, METRO_PREC_F32M = 0, 1, 2, 3
METRO_F16, METRO_F32, METRO_F64 = 0, 1, 2
PARAM_CONV_W, PARAM_BIAS, PARAM_PRO_SCALE, PARAM_PRO_SHIFT = 0, 1, 2, 3
LAYER_PREP, LAYER_CONV, LAYER_POOL, LAYER_SOFTARGMAX = 0, 1, 2, 3
FUSED_CONV1_IN_FRONT, FUSED_PROJECTION_SHORTCUT = 1, 2      # MetroLayerInfo.fused_flags (METRO_FUSED_*)
FUSED_OUT_ON_CHIP, FUSED_REBUILT_SHORTCUT, FUSED_COMPACT_SHORTCUT = 4, 8, 16


class MetroSpec(C.Structure):
    _fields_ = [('arch', C.c_int32), ('stride', C.c_int32), ('n_joints_head', C.c_int32),
                ('depth', C.c_int32), ('centered_stride', C.c_int32), ('proc_side', C.c_int32),
                ('box_size_mm', C.c_float), ('base_width', C.c_int32), ('precision', C.c_int32),
                ('n_joints_out', C.c_int32), ('permutation', C.c_int32 * METRO_MAX_JOINTS)]


class MetroParamInfo(C.Structure):
    _fields_ = [('name', C.c_char * 96), ('conv_var', C.c_char * 160), ('bn_var', C.c_char * 160),
                ('kind', C.c_int32), ('dtype', C.c_int32),
                ('c_out', C.c_int32), ('kh', C.c_int32), ('kw', C.c_int32), ('c_in', C.c_int32),
                ('kw_pad', C.c_int32), ('c_in_pad', C.c_int32),
                ('offset', C.c_int64), ('bytes', C.c_int64)]


class MetroLayerInfo(C.Structure):
    _fields_ = [('name', C.c_char * 96), ('kind', C.c_int32),
                ('h_in', C.c_int32), ('w_in', C.c_int32), ('c_in', C.c_int32),
                ('h_out', C.c_int32), ('w_out', C.c_int32), ('c_out', C.c_int32),
                ('kh', C.c_int32), ('kw', C.c_int32), ('stride', C.c_int32),
                ('dilation', C.c_int32), ('pad_top', C.c_int32), ('pad_left', C.c_int32),
                ('has_prologue', C.c_int32), ('relu', C.c_int32), ('has_residual', C.c_int32),
                ('res_stride', C.c_int32), ('res_offset', C.c_int32), ('out_dtype', C.c_int32),
                ('out_offset', C.c_int64), ('out_bytes_per_image', C.c_int64),
                ('flops_per_image', C.c_double),
                ('out2_offset', C.c_int64), ('out2_channels', C.c_int32), ('fused_flags', C.c_int32),
                ('algo_act_bytes_per_image', C.c_int64), ('algo_param_bytes', C.c_int64),
                ('out_sub_offset', C.c_int64), ('out_sub_side', C.c_int32), ('out_sub_off', C.c_int32)]


class MetroConvDesc(C.Structure):
    _fields_ = [('n', C.c_int32), ('h_in', C.c_int32), ('w_in', C.c_int32), ('c_in', C.c_int32),
                ('in_pix_stride', C.c_int32),
                ('h_out', C.c_int32), ('w_out', C.c_int32), ('c_out', C.c_int32),
                ('kh', C.c_int32), ('kw', C.c_int32), ('stride', C.c_int32), ('dilation', C.c_int32),
                ('pad_top', C.c_int32), ('pad_left', C.c_int32),
                ('has_prologue', C.c_int32), ('relu', C.c_int32), ('has_residual', C.c_int32),
                ('res_h', C.c_int32), ('res_w', C.c_int32),
                ('res_stride', C.c_int32), ('res_offset', C.c_int32), ('out_dtype', C.c_int32),
                ('in_dtype', C.c_int32)]


METRO_MAX_FRAMES = 64
METRO_WARP_HOMOGRAPHY, METRO_WARP_DISTORTED = 0, 1


class MetroFrame(C.Structure):
    _fields_ = [('data', C.c_void_p), ('h', C.c_int32), ('w', C.c_int32), ('row_stride', C.c_int32),
                ('reserved', C.c_int32)]


METRO_PIX_RGB, METRO_PIX_BGR, METRO_PIX_NV12, METRO_PIX_I420 = 0, 1, 2, 3
METRO_YUV_BT601, METRO_YUV_BT709 = 0, 1


class MetroFramePlanes(C.Structure):
    _fields_ = [('plane', C.c_void_p * 3), ('h', C.c_int32), ('w', C.c_int32), ('stride', C.c_int32 * 2),
                ('format', C.c_int32), ('matrix', C.c_int32)]


class MetroCropWarp(C.Structure):
    _fields_ = [('frame', C.c_int32), ('mode', C.c_int32), ('partial', C.c_double * 9), ('homography', C.c_float * 9),
                ('intrinsics', C.c_float * 6), ('distortion', C.c_float * 5)]


METRO_SCALE_METRO, METRO_SCALE_BONE_LENGTHS, METRO_SCALE_TRUE_ROOT_DEPTH = 0, 1, 2
METRO_COORDS_CROP, METRO_COORDS_CAMERA, METRO_COORDS_WORLD = 0, 1, 2


class MetroPlacement(C.Structure):
    _fields_ = [('keypoint_mode', C.c_int32), ('reserved', C.c_int32), ('inv_intrinsics', C.c_float * 9),
                ('rot_to_orig_cam', C.c_float * 9), ('rot_to_world', C.c_float * 9), ('cam_loc', C.c_float * 3),
                ('homography', C.c_float * 9), ('intrinsics', C.c_float * 6), ('distortion', C.c_float * 5)]


METRO_MAX_VIEWS = 32
METRO_MAX_MODES = 8            # metro_plan_bind_modes: modes per joint
METRO_MAX_MODE_RADIUS = 3
METRO_TRI_UNIFORM, METRO_TRI_COVARIANCE = 0, 1
METRO_MATCH_MAX_BOXES = 128
METRO_SMOOTH_FILTER, METRO_SMOOTH_RTS = 0, 1
METRO_SMOOTH_ISOTROPIC, METRO_SMOOTH_COVARIANCE = 0, 1
METRO_ASSOC_MAX = 128
METRO_PREDICT_MAX_DETECTIONS = 4096


class MetroViewBase(C.Structure):
    _fields_ = [('frame', C.c_int32), ('mode', C.c_int32), ('has_camera', C.c_int32), ('reserved', C.c_int32),
                ('old_matrix', C.c_double * 9), ('orig_r', C.c_double * 9), ('virt_k', C.c_double * 9),
                ('virt_r', C.c_double * 9), ('partial', C.c_double * 9), ('homography', C.c_float * 9),
                ('inv_intrinsics', C.c_float * 9), ('rot_to_orig_cam', C.c_float * 9), ('rot_to_world', C.c_float * 9),
                ('cam_loc', C.c_float * 3), ('intrinsics', C.c_float * 6), ('distortion', C.c_float * 5)]


class MetroFrameCamera(C.Structure):
    _fields_ = [('intrinsics', C.c_float * 9), ('r', C.c_float * 9), ('r_inv', C.c_float * 9), ('t', C.c_float * 3),
                ('distortion', C.c_float * 5), ('has_distortion', C.c_int32), ('world_up', C.c_double * 3),
                ('old_matrix', C.c_double * 9)]


class MetroTrackPrior(C.Structure):
    _fields_ = [('coords', C.c_int32), ('depth', C.c_int32), ('accel_psd', C.c_double), ('max_age_s', C.c_double),
                ('near_mm', C.c_double), ('sigma_floor_mm', C.c_double), ('cov_scale', C.c_double)]


METRO_TRACK_PRIOR_DEPTH_NONE, METRO_TRACK_PRIOR_DEPTH_ROOT = 0, 1


class MetroViewFusion(C.Structure):
    _fields_ = [('grid', C.c_int32), ('n_views', C.c_int32), ('weights', C.c_int32), ('extent_mm', C.c_double),
                ('floor', C.c_double), ('near_mm', C.c_double), ('min_det', C.c_double)]


class MetroSkeletonModes(C.Structure):
    _fields_ = [('scale_mm', C.c_double * 3), ('sigma_mm', C.c_double), ('sigma_rel', C.c_double), ('cov_scale', C.c_double),
                ('min_length_mm', C.c_double)]


class MetroView(C.Structure):
    _fields_ = [('cos_roll', C.c_double), ('sin_roll', C.c_double), ('zoom', C.c_double), ('flip', C.c_int32),
                ('reserved', C.c_int32)]


# symbol -> (restype, argtypes); must list every function include/metro_hip.h declares
_P = C.c_void_p
SIGNATURES = {
    'metro_plan_create': (C.c_int, [C.POINTER(MetroSpec), C.c_int32, C.POINTER(_P)]),
    'metro_plan_destroy': (C.c_int, [_P]),
    'metro_plan_workspace_bytes': (C.c_int64, [_P]),
    'metro_plan_param_bytes': (C.c_int64, [_P]),
    'metro_plan_num_params': (C.c_int32, [_P]),
    'metro_plan_param_info': (C.c_int, [_P, C.c_int32, C.POINTER(MetroParamInfo)]),
    'metro_plan_num_layers': (C.c_int32, [_P]),
    'metro_plan_layer_info': (C.c_int, [_P, C.c_int32, C.POINTER(MetroLayerInfo)]),
    'metro_plan_flops_per_image': (C.c_double, [_P]),
    'metro_plan_bind_params': (C.c_int, [_P, _P]),
    'metro_plan_layer_kernel': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_char_p, C.c_int32]),
    'metro_kernel_notes': (C.c_int, [C.c_int32]),
    'metro_last_kernel_id': (C.c_char_p, []),
    'metro_last_launch_schedule': (C.c_int, [C.POINTER(C.c_int32)]),
    'metro_plan_set_graph_max_batch': (C.c_int, [_P, C.c_int32]),
    'metro_forward': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P]),
    'metro_forward_coords01': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    'metro_forward_u8': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    'metro_forward_status': (C.c_int, [_P, _P, C.c_int32, _P, C.POINTER(C.c_int32)]),
    'metro_plan_status_offset': (C.c_int64, [_P]),
    'metro_plan_heatmaps_scratch_bytes': (C.c_int64, [_P, C.c_int32]),
    'metro_plan_bind_heatmaps': (C.c_int, [_P, _P, _P, _P, C.c_int32]),
    'metro_plan_modes_scratch_bytes': (C.c_int64, [_P, C.c_int32]),
    'metro_plan_bind_modes': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    'metro_plan_prior_scratch_bytes': (C.c_int64, [_P, C.c_int32]),
    'metro_plan_bind_prior': (C.c_int, [_P, _P, _P, _P, C.c_int32]),
    'metro_plan_bind_track_prior': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, C.POINTER(MetroTrackPrior), _P, _P, _P, _P,
                                              C.c_int32]),
    'metro_plan_bind_view_fusion': (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(MetroViewFusion), _P, _P, _P,
                                              _P, _P, C.c_int32]),
    'metro_plan_bind_skeleton_modes': (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_int32, C.POINTER(MetroSkeletonModes), _P, _P, _P, _P,
                                                 C.c_int32]),
    'metro_forward_upto': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32]),
    'metro_forward_timed': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.POINTER(C.c_float)]),
    'metro_conv_f16': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    'metro_conv_f32m': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    'metro_conv_f64acc': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    'metro_conv_f16_pair': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    'metro_conv_b1_form': (C.c_int, [C.c_int32]),
    'metro_conv_f16_gemm4w': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    'metro_conv_f16_conv1_conv2': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'metro_conv_f16_next_proj': (C.c_int, [C.POINTER(MetroConvDesc)] + [_P] * 14 + [C.c_int32, _P]),
    'metro_conv_f16_next_rebuild': (C.c_int, [C.POINTER(MetroConvDesc)] + [_P] * 13 + [C.c_int32] + [_P] * 5 + [C.c_int32, _P]),
    'metro_conv_f16_next': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P]),
    'metro_stem_pool_f16': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    'metro_stem_pool_f32in': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    'metro_stem_pool_u8in': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    'metro_prep_input_f16': (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    'metro_images_u8_to_f32': (C.c_int, [_P, C.c_int64, _P, _P]),
    'metro_warp_crop_u8': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    'metro_warp_crops_frames_u8': (C.c_int, [C.POINTER(MetroFrame), C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    'metro_warp_crops_frames_planes': (C.c_int, [C.POINTER(MetroFramePlanes), C.c_int32, _P, C.c_int32, C.c_int32, _P,
                                                 _P]),
    'metro_warp_crops_frames_u8_to_u8': (C.c_int, [C.POINTER(MetroFrame), C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    'metro_warp_crops_frames_planes_to_u8': (C.c_int, [C.POINTER(MetroFramePlanes), C.c_int32, _P, C.c_int32, C.c_int32, _P,
                                                       _P]),
    'metro_eval_metrics': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P, _P]),
    'metro_maxpool3x3s2_zeropad': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, _P]),
    'metro_softargmax_scratch_bytes': (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    'metro_softargmax01': (C.c_int, [_P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, _P, _P, _P]),
    'metro_backproject_bone_lengths': (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(MetroSpec),
                                                 C.c_int32, C.c_int32, _P, _P, _P]),
    'metro_backproject_root_depth': (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, C.c_int32, _P, _P]),
    'metro_to_orig_cam': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    'metro_place_poses': (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, _P, C.c_int32, _P, _P, C.c_int32,
                                    _P, C.c_int32, _P, _P, _P, _P]),
    'metro_expand_views': (C.c_int, [_P, C.c_int32, C.POINTER(MetroView), C.c_int32, C.c_int32, _P, _P, _P]),
    'metro_look_at_boxes': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'metro_merge_views': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    'metro_heatmap_to_25d': (C.c_int, [_P, C.c_int32, C.POINTER(MetroSpec), _P, _P]),
    'metro_head_f16_scratch_bytes': (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    'metro_head_f16': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(MetroSpec), _P, _P, _P, _P]),
    'metro_softargmax': (C.c_int, [_P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, _P, _P, _P]),
    'metro_moments_scratch_bytes': (C.c_int64, [C.POINTER(MetroSpec), C.c_int32]),
    'metro_forward_moments': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    'metro_head_f16_moments': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(MetroSpec)] + [_P] * 8),
    'metro_softargmax01_moments': (C.c_int, [_P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, _P, _P, _P, _P, _P, _P]),
    'metro_heat_marginals_scratch_bytes': (C.c_int64, [C.POINTER(MetroSpec), C.c_int32]),
    'metro_heat_marginals': (C.c_int, [_P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, _P, _P, _P, _P]),
    'metro_heat_modes': (C.c_int, [_P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    'metro_heat_posterior': (C.c_int, [_P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, _P, _P, _P]),
    'metro_place_covariances': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.POINTER(MetroSpec), _P, C.c_int32, _P, _P, _P]),
    'metro_triangulate_joints': (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.POINTER(MetroSpec), _P, C.c_int32,
                                           C.c_double, _P, _P, _P, _P]),
    'metro_view_affinity': (C.c_int, [_P, _P, _P, C.POINTER(MetroSpec), _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                      C.c_int32, _P, _P, _P]),
    'metro_triangulate_joints_cov': (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.POINTER(MetroSpec), _P, C.c_int32,
                                               C.c_double, _P, _P, _P, _P, _P]),
    'metro_view_affinity_steps': (C.c_int, [_P, _P, _P, C.POINTER(MetroSpec), _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                            C.c_double, C.c_int32, _P, _P, _P]),
    'metro_person_steps': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P]),
    'metro_person_steps_labels': (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    'metro_person_rays': (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(MetroSpec), _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    'metro_cluster_views': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P, _P, _P]),
    'metro_smooth_tracks_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'metro_smooth_tracks': (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.POINTER(MetroSpec), C.c_int32, C.c_int32,
                                      C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, _P]),
    'metro_associate_tracks_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'metro_associate_tracks': (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.POINTER(MetroSpec), C.c_int32,
                                         C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float, C.c_double, C.c_int32,
                                         C.c_double, _P, C.c_int32] + [_P] * 11),
    'metro_associate_tracks_optimal': (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.POINTER(MetroSpec), C.c_int32,
                                                 C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float, C.c_double,
                                                 C.c_int32, C.c_double, _P, C.c_int32] + [_P] * 11),
    'metro_associate_tracks_rays': (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.POINTER(MetroSpec), C.c_int32,
                                              C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float, C.c_double,
                                              C.c_int32, C.c_double, _P, C.c_int32] + [_P] * 10 +
                                    [C.c_int32, _P, _P, C.c_double, _P, _P, _P]),
    'metro_track_bone_lengths': (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, _P,
                                           C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32] +
                                 [_P] * 6),
    'metro_predict_boxes': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32] + [C.c_double] * 7 +
                            [C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_double] + [_P] * 10),
    'metro_last_error': (C.c_char_p, []),
    'metro_abi_version': (C.c_int32, []),
}

# libmetro_experimental.so (csrc/experimental/metro_experimental.h): kernels metro_forward never dispatches, kept for the
# probes in tools/ and for tests/test_gpu_kernels.py::test_conv_gemm_experimental
EXPERIMENTAL_LIB_PATH = os.path.join(HERE, 'libmetro_experimental.so')
EXPERIMENTAL_SIGNATURES = {
    'metro_conv_f16_gemm8p': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    'metro_conv_f16_gemm4d': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    'metro_conv_f16_gemm4d_geo': (C.c_int, [C.POINTER(MetroConvDesc), _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P]),
}

_lib = None
_xlib = None


class MetroError(RuntimeError):
    pass


class NonFiniteError(MetroError):
    """metro_forward_status: activations overflowed the arithmetic mode (fp16 storage tops out at 65 504)."""


def load() -> C.CDLL:
    """Loads libmetro_hip.so.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MetroError(
            f'{LIB_PATH} is missing: build it with `python -m metro_pose3d_amd.build` '
            '(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.')
    # torch first: it brings its own HIP runtime; loading this library before torch would pull a second libamdhip64
    # (the system one) into the process, whose kernels then see "no ROCm-capable device"
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)            # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.metro_abi_version() != ABI_VERSION:
        raise MetroError(f'ABI version mismatch: library {lib.metro_abi_version()}, bindings {ABI_VERSION}')
    _lib = lib
    return lib


def load_experimental() -> C.CDLL:
    """Loads libmetro_experimental.so (after the product library it links against)."""
    global _xlib
    if _xlib is not None:
        return _xlib
    load()
    if not os.path.exists(EXPERIMENTAL_LIB_PATH):
        raise MetroError(f'{EXPERIMENTAL_LIB_PATH} is missing: build it with `python -m metro_pose3d_amd.build`')
    lib = C.CDLL(EXPERIMENTAL_LIB_PATH)
    for name, (res, args) in EXPERIMENTAL_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _xlib = lib
    return lib


def check(status: int, what: str = '') -> None:
    if status == 0:
        return
    msg = load().metro_last_error().decode(errors='replace')
    if status == -1:
        raise ValueError(f'{what}: {msg}')
    if status == -5:
        raise NonFiniteError(f'{what}: {msg}')
    raise MetroError(f'{what}: status {status}: {msg}')
