"""ctypes binding of include/neuray_hip.h.

The product path loads neuray_amd/libneuray_hip.so (hipcc, gfx950) and raises if it is missing:
there is NO CPU or eager-PyTorch fallback for the hot path.  `bind()` is also used by the CPU
test-suite to bind tests/emu/_build/libneuray_emu.so (the kernel sources compiled for a CPU fiber
emulator) - test infrastructure that the package itself never loads.
"""
import ctypes as C
import os

import torch  # noqa: F401  (first: the library must resolve libamdhip64 to the HIP runtime PyTorch already loaded -
#                      loaded before torch it binds the system copy and later launches find "no ROCm-capable device")

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NEURAY_HIP_LIB', os.path.join(HERE, 'libneuray_hip.so'))   # env override: A/B debugging only
BF16_LIB_PATH = os.path.join(HERE, 'libneuray_hip_bf16.so')     # the separately reported bf16-operand variant (inference only)
BF16X3_LIB_PATH = os.path.join(HERE, 'libneuray_hip_bf16x3.so') # the split variant: hi + lo bf16 operands, 3 bf16 MFMAs per fp32 quad (inference only)

PASS_TENSORS = 68
POINT_REC = 20
VIEW_CONST = 20
QUERY_CONST = 28
DBG_FIELDS = 16
MAX_VIEWS = 16
MAX_SAMPLES = 128
MAX_BACKWARD_SAMPLES = 128     # samples per ray and pass the backward kernels take (include/neuray_hip.h): = MAX_SAMPLES

ARITH_F32, ARITH_X3 = 0, 1      # NeurayPointsArgs.arith (include/neuray_hip.h NEURAY_ARITH_*)

c_float_p = C.POINTER(C.c_float)


class NeurayPointsArgs(C.Structure):
    _fields_ = [
        ('query_const_dev', C.c_void_p), ('view_const_dev', C.c_void_p), ('coords_dev', C.c_void_p),
        ('depth_dev', C.c_void_p), ('ray_feats_nhwc_dev', C.c_void_p), ('img_feats_nhwc_dev', C.c_void_p),
        ('rgba_dev', C.c_void_p), ('packed_weights_dev', C.c_void_p), ('point_out_dev', C.c_void_p),
        ('dbg_dev', C.c_void_p),
        ('rfn', C.c_int), ('rn', C.c_int), ('dn', C.c_int), ('h', C.c_int), ('w', C.c_int), ('fh', C.c_int),
        ('fw', C.c_int), ('has_vis_head', C.c_int), ('use_vis', C.c_int), ('var_bias', C.c_float),
        ('views_per_wave', C.c_int), ('saved_dev', C.c_void_p), ('folded', C.c_int), ('slot_stats_dev', C.c_void_p),
        ('arith', C.c_int),
    ]


class NeurayRaysArgs(C.Structure):
    _fields_ = [
        ('point_rec_dev', C.c_void_p), ('depth_dev', C.c_void_p), ('pos_enc_dev', C.c_void_p),
        ('packed_weights_dev', C.c_void_p), ('hit_prob_dev', C.c_void_p), ('pixel_dev', C.c_void_p),
        ('render_depth_dev', C.c_void_p), ('ray_mask_dev', C.c_void_p), ('density_dev', C.c_void_p),
        ('rn', C.c_int), ('dn', C.c_int), ('ray_mask_view_num', C.c_int), ('ray_mask_point_num', C.c_int),
        ('att_save_dev', C.c_void_p),
    ]


class NeurayRaysBwdArgs(C.Structure):
    _fields_ = [
        ('point_rec_dev', C.c_void_p), ('depth_dev', C.c_void_p), ('pos_enc_dev', C.c_void_p),
        ('packed_weights_dev', C.c_void_p), ('d_pixel_dev', C.c_void_p), ('d_hit_prob_dev', C.c_void_p),
        ('d_render_depth_dev', C.c_void_p), ('d_point_rec_dev', C.c_void_p), ('d_ray_weights_dev', C.c_void_p),
        ('rn', C.c_int), ('dn', C.c_int), ('att_saved_dev', C.c_void_p),
    ]


class NeurayPointsBwdArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        'query_const_dev', 'view_const_dev', 'coords_dev', 'depth_dev', 'ray_feats_nhwc_dev', 'img_feats_nhwc_dev',
        'rgba_dev', 'flat_weights_dev', 'd_point_rec_dev', 'd_flat_weights_dev', 'd_ray_feats_nhwc_dev',
        'd_img_feats_nhwc_dev')] + \
        [(n, C.c_int) for n in ('rfn', 'rn', 'dn', 'h', 'w', 'fh', 'fw', 'has_vis_head', 'use_vis')] + \
        [('var_bias', C.c_float), ('packed_weights_dev', C.c_void_p), ('packed_t_weights_dev', C.c_void_p), ('saved_dev', C.c_void_p),
         ('handover_dev', C.c_void_p)]


class NeurayImageMetricsArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('pred_dev', 'gt_dev', 'quant_dev', 'sse_dev', 'ssim_dev', 'workspace_dev')] + \
        [(n, C.c_int) for n in ('n', 'gt_stride', 'input_u8', 'h', 'w', 'roi_y0', 'roi_y1', 'roi_x0', 'roi_x1', 'variant')]


SSIM_BOX11, SSIM_GAUSS11 = 0, 1   # NeurayImageMetricsArgs.variant (include/neuray_hip.h NEURAY_SSIM_*)



class NeurayLossTerm(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('pred_dev', 'ref_dev', 'mask_dev', 'coords_dev', 'range_dev', 'grad_out_dev', 'd_pred_dev')] + \
        [(n, C.c_int) for n in ('kind', 'rows', 'n', 'inner', 'stride', 'h', 'w', 'coords_i64', 'mask_u8', 'smooth_l1')] + \
        [('beta', C.c_float), ('thresh', C.c_float)]


class NeurayTrainLossArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('terms', 'value_dev', 'den_dev', 'workspace_dev')] + [('n_terms', C.c_int), ('reserved', C.c_int)]


class NeurayVisibilityArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('query_const_dev', 'view_const_dev', 'coords_dev', 'depth_dev', 'ray_feats_nhwc_dev',
                                          'packed_weights_dev')] + \
        [(n, C.c_int) for n in ('rfn', 'rn', 'dn', 'h', 'w', 'fh', 'fw', 'has_vis_head', 'use_vis')] + \
        [('var_bias', C.c_float), ('ground', C.c_float), ('alpha_dev', C.c_void_p), ('nvalid_dev', C.c_void_p)]


class NeurayProceduralArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('scene_dev', 'poses_dev', 'Ks_inv_dev', 'rgb_dev', 'depth_dev', 'mask_dev', 'prim_dev')] + \
        [(n, C.c_int) for n in ('n_prims', 'n', 'h', 'w', 'ss', 'reserved')]


class NeurayDepthConsistencyArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('depth_dev', 'poses_dev', 'Ks_dev', 'Ks_inv_dev', 'nn_ids_dev', 'count_dev', 'fused_depth_dev',
                                          'consistent_bits_dev', 'occluded_bits_dev', 'src_texel_dev')] + \
        [(n, C.c_int) for n in ('n', 'h', 'w', 'n_src')] + [('tau_px', C.c_float), ('tau_d', C.c_float)]


class NeurayFuseViewArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('depth_dev', 'poses_dev', 'Ks_dev', 'Ks_inv_dev', 'nn_ids_dev', 'count_dev', 'fused_depth_dev',
                                          'consistent_bits_dev', 'rgb_dev', 'taken_dev', 'emit_dev', 'xyz_dev', 'colour_dev', 'normal_dev')] + \
        [(n, C.c_int) for n in ('n', 'h', 'w', 'n_src', 'view', 'min_views', 'dedup', 'reserved')] + [('tau_n', C.c_float), ('reserved_f', C.c_float)]


class NeurayTsdfIntegrateArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('depth_dev', 'rgb_dev', 'poses_dev', 'Ks_dev', 'tsum_dev', 'w_dev', 'csum_dev', 'cw_dev')] + \
        [(n, C.c_float) for n in ('origin_x', 'origin_y', 'origin_z', 'voxel_size', 'trunc', 'reserved_f')] + \
        [(n, C.c_int) for n in ('nx', 'ny', 'nz', 'n', 'h', 'w', 'v0', 'v1')]


class NeuraySurfaceCellsArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('tsum_dev', 'w_dev', 'cells_dev')] + [(n, C.c_int) for n in ('nx', 'ny', 'nz', 'reserved')] + \
        [('min_weight', C.c_float), ('reserved_f', C.c_float)]


class NeuraySurfaceEmitArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('tsum_dev', 'w_dev', 'csum_dev', 'cw_dev', 'cells_dev', 'vert_offset_dev', 'quad_offset_dev',
                                          'vertices_dev', 'normals_dev', 'colours_dev', 'faces_dev')] + \
        [('n_vertices', C.c_uint), ('n_quads', C.c_uint)] + [(n, C.c_float) for n in ('origin_x', 'origin_y', 'origin_z', 'voxel_size')] + \
        [(n, C.c_int) for n in ('nx', 'ny', 'nz', 'reserved')]


class NeuraySurfaceBlocksArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('cells_dev', 'blocks_dev')] + [(n, C.c_int) for n in ('nx', 'ny', 'nz', 'reserved')]


class NeurayTsdfRaycastArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('field_dev', 'csum_dev', 'cw_dev', 'rays_dev', 'depth_range_dev', 'blocks_dev', 'depth_dev',
                                          'normal_dev', 'colours_dev', 'status_dev', 'evaluated_dev')] + \
        [(n, C.c_float) for n in ('origin_x', 'origin_y', 'origin_z', 'voxel_size', 'step', 'reserved_f')] + \
        [(n, C.c_int) for n in ('nx', 'ny', 'nz', 'n', 'h', 'w', 'reserved', 'reserved2')]


class NeurayAugmentStatsArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('mask_dev', 'depth_dev', 'row_counts_dev', 'row_part_dev', 'stats_dev')] + \
        [(n, C.c_int) for n in ('n', 'h', 'w', 'reserved')]


class NeurayAugmentDepthArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('depth_dev', 'mask_dev', 'range_in_dev', 'stats_dev', 'row_counts_dev', 'host_dev', 'range_aug_dev',
                                          'range_out_dev', 'plan_dev', 'depth_aug_dev')] + \
        [(n, C.c_int) for n in ('n', 'h', 'w', 'view0', 'rfn', 'reserved')] + [('key0', C.c_uint), ('key1', C.c_uint)]


class NeuraySampleCoordsArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('mask_dev', 'keys_dev', 'taken_dev', 'work_dev', 'coords_dev')] + \
        [(n, C.c_int) for n in ('h', 'w', 'ray_num', 'want_fg', 'view', 'reserved')] + [('key0', C.c_uint), ('key1', C.c_uint)]


class NeurayPlaneSweepArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('imgs_dev', 'gray_dev', 'cams_dev', 'depth_range_dev', 'nn_ids_dev', 'depth_dev', 'cost_dev', 'plane_dev')] + \
        [(n, C.c_int) for n in ('n', 'h', 'w', 'n_src', 'planes', 'radius', 'v0', 'v1', 'min_src', 'flags')] + \
        [('var_min', C.c_float), ('reserved_f', C.c_float)]


SWEEP_MAX_PLANES, SWEEP_COST_NONE, SWEEP_NO_SKIP = 256, 4.0, 1   # include/neuray_hip.h NEURAY_SWEEP_*
AUGMENT_STATS, AUGMENT_PLAN, AUGMENT_HOST, SAMPLE_COORDS_WORK = 8, 8, 16, 16416   # include/neuray_hip.h NEURAY_AUGMENT_*, NEURAY_SAMPLE_COORDS_WORK
TSDF_BLOCK = 8                # cells per block and axis (neuray_surface_blocks)
TSDF_MAX_POINTS = 1 << 30      # nx * ny * nz of a volume (include/neuray_hip.h)
FUSE_MAX_SRC = 16              # include/neuray_hip.h NEURAY_FUSE_MAX_SRC
PROC_HEADER, PROC_PRIM, PROC_MAX_PRIMS = 16, 48, 32   # the scene array of neuray_procedural_render (include/neuray_hip.h NEURAY_PROC_*)
LOSS_RENDER, LOSS_CONSIST, LOSS_DEPTH = 0, 1, 2   # NeurayLossTerm.kind (include/neuray_hip.h NEURAY_LOSS_*)
LOSS_MAX_TERMS = 4
DET_POINTS, DET_RAYS, DET_SELF_HIT, DET_ROWS = 0, 1, 2, 3   # neuray_deterministic_partials_floats (include/neuray_hip.h NEURAY_DET_*)

PACKED_RAY_FLOATS = 1348
RAY_ATT_SAVE = 24            # NEURAY_RAY_ATT_SAVE
# (state_dict suffix under agg_net.agg_impl., offset, shape) of the ray-part weights inside d_ray_weights (include/neuray_hip.h)
RAY_WEIGHT_SLOTS = (
    ('ray_attention.w_qs.weight', 0, (16, 16)), ('ray_attention.w_ks.weight', 256, (16, 16)),
    ('ray_attention.w_vs.weight', 512, (16, 16)), ('ray_attention.fc.weight', 768, (16, 16)),
    ('ray_attention.layer_norm.weight', 1024, (16,)), ('ray_attention.layer_norm.bias', 1040, (16,)),
    ('out_geometry_fc.0.weight', 1056, (16, 16)), ('out_geometry_fc.0.bias', 1312, (16,)),
    ('out_geometry_fc.2.weight', 1328, (1, 16)), ('out_geometry_fc.2.bias', 1344, (1,)),
)


# every symbol include/neuray_hip.h declares: (restype, argtypes)
SYMBOLS = {
    'neuray_abi_version': (C.c_int, []),
    'neuray_last_error': (C.c_char_p, []),
    'neuray_is_device_build': (C.c_int, []),
    'neuray_operand_precision': (C.c_int, []),
    'neuray_packed_pass_floats': (C.c_size_t, []),
    'neuray_points_saved_floats': (C.c_size_t, [C.c_int]),
    'neuray_pack_pass_weights': (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    'neuray_pack_pass_weights_folded': (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    'neuray_packed_points_floats_x3': (C.c_size_t, []),
    'neuray_pack_pass_weights_x3': (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    'neuray_pack_pass_index_map': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_mt19937_shuffle': (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_longlong, C.c_int]),
    'neuray_setup_views': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_setup_query': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_relayout_nhwc': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'neuray_sample_coarse_depth': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_sample_coarse_depth_jittered': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_render_points': (C.c_int, [C.POINTER(NeurayPointsArgs), C.c_void_p]),
    'neuray_render_rays': (C.c_int, [C.POINTER(NeurayRaysArgs), C.c_void_p]),
    'neuray_sample_fine_depth': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_sample_fine_depth_traced': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_interpolate_feats': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_rays_points': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    'neuray_depth_dists': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_project_points': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_alpha2hit_prob': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_inorm_forward': (C.c_int, [C.c_void_p] * 4 + [C.c_longlong] * 3 + [C.c_int] * 6 + [C.c_float] + [C.c_void_p] * 3 + [C.c_longlong, C.c_void_p]),
    'neuray_inorm_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 6),
    'neuray_upsample2x_pad_forward': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'neuray_upsample2x_pad_backward': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_direct_render_points': (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_direct_render_rays': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_direct_render_rays_backward': (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 3),
    'neuray_direct_render_points_backward': (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 6 + [C.c_void_p] * 2),
    'neuray_dist_decoder_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    'neuray_self_hit_prob': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    'neuray_mfma_selftest': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_x3_selftest': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_points_resident_workgroups': (C.c_int, [C.c_int, C.c_int]),
    'neuray_render_rays_backward': (C.c_int, [C.POINTER(NeurayRaysBwdArgs), C.c_void_p]),
    'neuray_flat_pass_floats': (C.c_size_t, []),
    'neuray_flat_tensor_offset': (C.c_size_t, [C.c_int]),
    'neuray_packed_t_floats': (C.c_size_t, []),
    'neuray_pack_pass_t_index_map': (C.c_int, [C.c_int, C.c_void_p]),
    'neuray_points_backward_handover_floats': (C.c_size_t, [C.c_int]),
    'neuray_packed_quad_ranges': (C.c_int, [C.c_int, C.c_void_p, C.c_int]),
    'neuray_render_points_backward': (C.c_int, [C.POINTER(NeurayPointsBwdArgs), C.c_void_p]),
    'neuray_self_hit_prob_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                         C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_dist_decoder_rows_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_interpolate_feats_backward_staged': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_interpolate_feats_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_group_sum_selftest': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_group_scatter_selftest': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_pair_forms_selftest': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_allreduce_selftest': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'neuray_warp_variance': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_warp_variance_layout': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_conv3d_c32_c8': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_convtranspose3d_bn_leaky': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_conv3d_bn_leaky': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    'neuray_conv3x3_x3_pack_bytes': (C.c_longlong, [C.c_int, C.c_int]),
    'neuray_conv3x3_x3_pack': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_conv3x3_x3': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_conv3x3_x3_relu': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_conv3x3_x3_wrw_workspace_floats': (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'neuray_conv3x3_x3_wrw': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_scale_shift_leaky': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_float, C.c_void_p]),
    'neuray_conv3d_c8_c1': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_convtranspose3d_c16_c8': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_diff_feats': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_image_metrics_workspace_bytes': (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    'neuray_image_metrics': (C.c_int, [C.POINTER(NeurayImageMetricsArgs), C.c_void_p]),
    'neuray_lpips_stem': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_maxpool2x2': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'neuray_lpips_head_workspace_bytes': (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    'neuray_lpips_head': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p]),
    'neuray_train_loss_workspace_bytes': (C.c_longlong, [C.POINTER(NeurayLossTerm), C.c_int]),
    'neuray_train_loss': (C.c_int, [C.POINTER(NeurayTrainLossArgs), C.c_void_p]),
    'neuray_train_loss_backward': (C.c_int, [C.POINTER(NeurayTrainLossArgs), C.c_void_p]),
    'neuray_visibility_points': (C.c_int, [C.POINTER(NeurayVisibilityArgs), C.c_void_p]),
    'neuray_visibility_rays': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the deterministic training backward
    'neuray_deterministic_partials_floats': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'neuray_reduce_partials': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    'neuray_render_rays_backward_det': (C.c_int, [C.POINTER(NeurayRaysBwdArgs), C.c_void_p, C.c_void_p]),
    'neuray_points_backward_scatter_columns': (C.c_longlong, [C.c_int]),
    'neuray_render_points_backward_det': (C.c_int, [C.POINTER(NeurayPointsBwdArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_points_backward_scatter': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    'neuray_self_hit_prob_backward_det': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_dist_decoder_rows_backward_det': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'neuray_interpolate_scatter_keys': (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 3),
    'neuray_interpolate_feats_backward_sorted': (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p] * 2),
    'neuray_inorm_chunks': (C.c_int, [C.c_int] * 4),
    'neuray_inorm_forward_det': (C.c_int, [C.c_void_p] * 4 + [C.c_longlong] * 3 + [C.c_int] * 6 + [C.c_float] + [C.c_void_p] * 4 + [C.c_longlong, C.c_void_p]),
    # procedural scenes
    'neuray_procedural_render': (C.c_int, [C.POINTER(NeurayProceduralArgs), C.c_void_p]),
    # geometry export
    'neuray_depth_consistency': (C.c_int, [C.POINTER(NeurayDepthConsistencyArgs), C.c_void_p]),
    'neuray_fuse_view': (C.c_int, [C.POINTER(NeurayFuseViewArgs), C.c_void_p]),
    # mesh export
    'neuray_tsdf_integrate': (C.c_int, [C.POINTER(NeurayTsdfIntegrateArgs), C.c_void_p]),
    'neuray_surface_cells': (C.c_int, [C.POINTER(NeuraySurfaceCellsArgs), C.c_void_p]),
    'neuray_surface_emit': (C.c_int, [C.POINTER(NeuraySurfaceEmitArgs), C.c_void_p]),
    # ray casting of a volume
    'neuray_surface_blocks': (C.c_int, [C.POINTER(NeuraySurfaceBlocksArgs), C.c_void_p]),
    'neuray_tsdf_raycast': (C.c_int, [C.POINTER(NeurayTsdfRaycastArgs), C.c_void_p]),
    'neuray_inorm_backward_det': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 7),
    # augmentation of the procedural stream
    'neuray_augment_stats': (C.c_int, [C.POINTER(NeurayAugmentStatsArgs), C.c_void_p]),
    'neuray_augment_depth': (C.c_int, [C.POINTER(NeurayAugmentDepthArgs), C.c_void_p]),
    'neuray_sample_coords': (C.c_int, [C.POINTER(NeuraySampleCoordsArgs), C.c_void_p]),
    # plane-sweep stereo
    'neuray_plane_sweep': (C.c_int, [C.POINTER(NeurayPlaneSweepArgs), C.c_void_p]),
}


class NeurayLibError(RuntimeError):
    pass


def bind(path):
    """dlopen `path` and attach prototypes for every symbol of the C ABI (raises if one is missing)."""
    lib = C.CDLL(path)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


_LIBS = {}


def load(variant='fp32'):
    """The product library (HIP, gfx950), or with variant='bf16' the bf16-operand build.  Raises loudly if it has not
    been built."""
    if variant not in _LIBS:
        path = {'fp32': LIB_PATH, 'bf16': BF16_LIB_PATH, 'bf16x3': BF16X3_LIB_PATH}[variant]
        if not os.path.exists(path):
            raise NeurayLibError(
                "neuray_amd: %s not found - build it with `python -m neuray_amd.build` (hipcc, gfx950). "
                "There is no CPU/eager fallback for the render path." % path)
        lib = bind(path)
        if lib.neuray_is_device_build() != 1:
            raise NeurayLibError("neuray_amd: %s is not a device build" % path)
        if lib.neuray_operand_precision() != {'fp32': 32, 'bf16': 16, 'bf16x3': 48}[variant]:
            raise NeurayLibError("neuray_amd: %s is not the %s build" % (path, variant))
        _LIBS[variant] = lib
    return _LIBS[variant]


def check(lib, rc):
    if rc != 0:
        raise RuntimeError("neuray_hip: " + lib.neuray_last_error().decode('utf-8', 'replace'))
