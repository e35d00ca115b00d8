"""ctypes binding of libucnerf_hip.so (the C ABI declared in include/ucnerf_hip.h).

There is no CPU fallback anywhere in this package: if the library is missing or a call fails, a
RuntimeError is raised.  Struct mirrors are checked against the library's own sizeof() table at load time.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UCNERF_LIB") or os.path.join(_HERE, "libucnerf_hip.so")   # override: A/B builds

ABI_VERSION = 6    # UCNERF_ABI_VERSION of include/ucnerf_hip.h this binding mirrors
REPACK_ALL = 0x1f  # UCNERF_REPACK_ALL: every source of ucnerf_gather_repack_masked (bits 0..2 volumes, 3 image features, 4 colours)

fp = C.POINTER(C.c_float)
i32 = C.c_int32
f32 = C.c_float
vp = C.c_void_p     # device pointers travel as integers


class RayGenParams(C.Structure):
    _fields_ = [("n", i32), ("H", i32), ("W", i32), ("grid_start", i32), ("opengl", i32), ("K", f32 * 9),
                ("c2w", f32 * 12), ("xs", vp), ("ys", vp), ("rays_d", vp), ("rays_o", vp), ("pix", vp), ("w2c_dir", f32 * 12), ("angle", vp)]


class NdcRaysParams(C.Structure):
    _fields_ = [("n", i32), ("H", i32), ("W", i32), ("variant", i32), ("focal_x", f32), ("focal_y", f32),
                ("near", f32), ("rays_o", vp), ("rays_d", vp), ("out_o", vp), ("out_d", vp)]


class DirFeatureParams(C.Structure):
    _fields_ = [("n", i32), ("has_ref", i32), ("repeat", i32), ("w2c_ref", f32 * 12), ("rays_d", vp), ("angle", vp),
                ("cos_angle", vp), ("w2c_ref_dev", vp)]


class SampleStratifiedParams(C.Structure):
    _fields_ = [("n", i32), ("S", i32), ("lindisp", i32), ("perturb", f32), ("near", f32), ("far", f32), ("rays", vp), ("noise", vp), ("z", vp),
                ("pts", vp)]


class SampleCascadeParams(C.Structure):
    _fields_ = [("n", i32), ("S", i32), ("near_far", vp), ("t_rand", vp), ("rays_o", vp), ("rays_d", vp), ("z", vp),
                ("pts", vp)]


class NdcProjectParams(C.Structure):
    _fields_ = [("m", i32), ("has_w2c", i32), ("sample_2d", i32), ("nf_stride", i32), ("w2c", f32 * 12), ("K", f32 * 9),
                ("inv_scale", f32 * 2), ("near", f32), ("far", f32), ("pts", vp), ("near_1", vp), ("far_1", vp),
                ("near_2", vp), ("far_2", vp), ("near_3", vp), ("far_3", vp), ("out_stage1", vp), ("out_stage2", vp),
                ("out_stage3", vp), ("out_ndc", vp)]


class BuildRaysTestParams(C.Structure):
    _fields_ = [("n", i32), ("S", i32), ("H", i32), ("W", i32), ("grid_start", i32), ("dv_d", i32 * 3), ("dv_h", i32 * 3), ("dv_w", i32 * 3),
                ("K", vp), ("c2w", vp), ("w2c_ref", vp), ("K_ref", vp), ("near_far_ref", vp), ("depth_values", vp * 3), ("t_rand", vp),
                ("rays_o", vp), ("rays_d", vp), ("near_far", vp), ("z", vp), ("pts", vp), ("ndc1", vp), ("ndc2", vp), ("ndc3", vp), ("ndc", vp)]


class EmbedParams(C.Structure):
    _fields_ = [("m", i32), ("n_freqs", i32), ("layout", i32), ("x", vp), ("out", vp)]


class FeatGatherParams(C.Structure):
    _fields_ = [("m", i32), ("V", i32), ("H", i32), ("W", i32), ("vol_d", i32 * 3), ("vol_h", i32 * 3),
                ("vol_w", i32 * 3), ("out_tiled", i32), ("unit_mask", i32), ("pts", vp), ("ndc1", vp), ("ndc2", vp), ("ndc3", vp),
                ("vol", vp * 3), ("conf", vp), ("imgs", vp), ("img_feat", vp), ("w2cs", vp), ("intrinsics", vp),
                ("feats", vp), ("u_out", vp)]


class ClSources(C.Structure):
    """ucnerf_cl_sources (ABI v5): the gather sources channel-last, each in its own allocation."""
    _fields_ = [("vol", vp * 3), ("img_feat", vp), ("imgs", vp), ("rgb_stride", i32), ("bf16", i32)]


class ClGrads(C.Structure):
    _fields_ = [("vol", vp * 3), ("img_feat", vp)]


class FeatGatherBwdParams(C.Structure):
    _fields_ = [("fwd", FeatGatherParams), ("g_feats", vp), ("g_vol", vp * 3), ("g_conf", vp), ("g_img_feat", vp),
                ("scratch", vp), ("g_cl", ClGrads)]


class MlpConfig(C.Structure):
    _fields_ = [("n_src", i32), ("pe_layout", i32), ("precision", i32), ("operand", i32)]


class MlpParams(C.Structure):
    _fields_ = [("cfg", MlpConfig), ("m", i32), ("S", i32), ("dirs_per_sample", i32), ("feats_tiled", i32),
                ("max_blocks", i32), ("encoded", i32), ("pts_stride", i32), ("dirs_stride", i32), ("feat_stride", i32),
                ("pts", vp), ("dirs", vp), ("feats", vp), ("wstream", vp), ("raw", vp)]


class MlpBwdParams(C.Structure):
    _fields_ = [("fwd", MlpParams), ("g_raw", vp), ("flat_params", vp), ("g_feats", vp), ("g_feat_stride", i32),
                ("g_flat", vp), ("workspace", vp), ("saved_valid", i32), ("bwd_mode", i32)]


class CompositeParams(C.Structure):
    _fields_ = [("n", i32), ("S", i32), ("variant", i32), ("white_bkgd", i32), ("raw", vp), ("z", vp), ("rays_d", vp),
                ("noise", vp), ("rgb_map", vp), ("depth_map", vp), ("acc_map", vp), ("disp_map", vp), ("weights", vp),
                ("var", vp), ("u", vp), ("wu", vp)]


class CompositeBwdParams(C.Structure):
    _fields_ = [("fwd", CompositeParams), ("g_rgb", vp), ("g_depth", vp), ("g_acc", vp), ("g_weights", vp),
                ("g_raw", vp)]


class SamplePdfParams(C.Structure):
    _fields_ = [("n", i32), ("n_bins", i32), ("n_samples", i32), ("u_stride", i32), ("n_merge", i32), ("from_coarse", i32),
                ("bins", vp),
                ("weights", vp), ("u", vp), ("z_merge", vp), ("samples", vp), ("inds", vp), ("cdf", vp),
                ("z_sorted", vp), ("merge_rank", vp)]


class MergeRowsParams(C.Structure):
    _fields_ = [("n", i32), ("na", i32), ("nb", i32), ("width", i32), ("a", vp), ("b", vp), ("rank", vp), ("out", vp)]


class CompositeMergedParams(C.Structure):
    _fields_ = [("n", i32), ("na", i32), ("nb", i32), ("white_bkgd", i32), ("raw_a", vp), ("raw_b", vp), ("rank", vp), ("z", vp), ("rgb_map", vp),
                ("depth_map", vp), ("acc_map", vp), ("disp_map", vp), ("weights", vp), ("var", vp), ("u", vp), ("wu", vp)]


class CompositeMergedBwdParams(C.Structure):
    _fields_ = [("n", i32), ("na", i32), ("nb", i32), ("white_bkgd", i32), ("raw_a", vp), ("raw_b", vp), ("rank", vp), ("z", vp), ("g_rgb", vp),
                ("g_depth", vp), ("g_acc", vp), ("g_weights", vp), ("g_raw_a", vp), ("g_raw_b", vp)]


class CompositeFoldParams(C.Structure):
    _fields_ = [("n", i32), ("S", i32), ("weights", vp), ("depth", vp), ("acc", vp), ("u", vp), ("g_var", vp), ("g_disp", vp), ("g_wu", vp),
                ("g_depth", vp), ("g_acc", vp), ("g_weights", vp), ("g_depth_out", vp), ("g_acc_out", vp), ("g_weights_out", vp), ("g_u", vp)]


class CostVolumeParams(C.Structure):
    _fields_ = [("V", i32), ("C", i32), ("H", i32), ("W", i32), ("D", i32), ("pad", i32), ("feats", vp), ("proj", vp),
                ("depth_values", vp), ("variance", vp), ("count", vp)]


class DepthRegressParams(C.Structure):
    _fields_ = [("D", i32), ("Hp", i32), ("Wp", i32), ("pad", i32), ("prob_pre", vp), ("prob_init", vp), ("depth_values", vp),
                ("prob_volume", vp), ("depth", vp), ("confidence", vp)]


class CostVolumeBwdParams(C.Structure):
    _fields_ = [("fwd", CostVolumeParams), ("g_variance", vp), ("g_feats", vp)]


class DepthRegressBwdParams(C.Structure):
    _fields_ = [("fwd", DepthRegressParams), ("g_depth", vp), ("g_confidence", vp), ("g_prob_pre", vp)]


class DepthHypothesesParams(C.Structure):
    _fields_ = [("D", i32), ("h", i32), ("w", i32), ("pad", i32), ("H", i32), ("W", i32), ("h0", i32), ("w0", i32), ("D_in", i32), ("k", f32),
                ("cur_depth", vp), ("row", vp), ("near_far", vp), ("interval", vp), ("out", vp)]


class DepthRegressBwdValuesParams(C.Structure):
    _fields_ = [("D", i32), ("Hp", i32), ("Wp", i32), ("pad", i32), ("prob_volume", vp), ("g_depth", vp), ("g_depth_values", vp)]


class DepthHypothesesBwdParams(C.Structure):
    _fields_ = [("fwd", DepthHypothesesParams), ("g_out", vp), ("scratch", vp), ("g_cur_depth", vp)]


class BuildRaysTrainParams(C.Structure):
    _fields_ = [("S", i32), ("H", i32), ("W", i32), ("P", i32), ("ps", i32), ("n_uniform", i32), ("n_coord", i32), ("coord_stride", i32),
                ("dv_d", i32 * 3), ("dv_h", i32 * 3), ("dv_w", i32 * 3), ("img_stride_c", C.c_int64), ("img_stride_h", C.c_int64),
                ("img_stride_w", C.c_int64), ("K", vp), ("c2w", vp), ("w2c_ref", vp), ("K_ref", vp), ("near_far_ref", vp), ("depth_values", vp * 3),
                ("imgs", vp), ("sel0", vp), ("sel1", vp), ("shift", vp), ("ux", vp), ("uy", vp), ("coords", vp), ("t_rand", vp), ("rays_o", vp),
                ("rays_d", vp), ("colors", vp), ("pix", vp), ("near_far", vp), ("z", vp), ("pts", vp), ("ndc1", vp), ("ndc2", vp), ("ndc3", vp),
                ("ndc", vp)]


class DepthEvalParams(C.Structure):
    _fields_ = [("n", i32), ("H", i32), ("W", i32), ("raw", i32), ("min_depth", f32), ("max_depth", f32), ("gt", vp), ("pred", vp), ("mask", vp),
                ("workspace", vp), ("out", vp)]


class ImageEvalParams(C.Structure):
    _fields_ = [("n", i32), ("H", i32), ("W", i32), ("no_ssim", i32), ("gt", vp), ("pred", vp), ("workspace", vp), ("out", vp)]


class Conv2dPackParams(C.Structure):
    _fields_ = [("cin", i32), ("cout", i32), ("K", i32), ("reserved", i32), ("weight", vp), ("packed", vp)]


class Conv2dParams(C.Structure):
    _fields_ = [("n", i32), ("cin", i32), ("H", i32), ("W", i32), ("cout", i32), ("K", i32), ("stride", i32), ("pad", i32), ("relu", i32),
                ("reserved", i32), ("x", vp), ("packed", vp), ("bias", vp), ("shift", vp), ("scale", vp), ("y", vp)]


class Maxpool2dParams(C.Structure):
    _fields_ = [("planes", C.c_int64), ("H", i32), ("W", i32), ("x", vp), ("y", vp)]


class LpipsLayerParams(C.Structure):
    _fields_ = [("n", i32), ("C", i32), ("h", i32), ("w", i32), ("accumulate", i32), ("reserved", i32), ("f0", vp), ("f1", vp), ("lin", vp),
                ("out", vp)]


class LpipsAlexParams(C.Structure):
    _fields_ = [("n", i32), ("H", i32), ("W", i32), ("reserved", i32), ("a", vp), ("b", vp), ("packed", vp * 5), ("bias", vp * 5), ("lin", vp * 5),
                ("shift", vp), ("scale", vp), ("workspace", vp), ("out", vp)]


class Conv3dPackParams(C.Structure):
    _fields_ = [("cin", i32), ("cout", i32), ("K", i32), ("transposed", i32), ("weight", vp), ("packed", vp)]


class Conv3dParams(C.Structure):
    _fields_ = [("n", i32), ("cin", i32), ("D", i32), ("H", i32), ("W", i32), ("cout", i32), ("K", i32), ("stride", i32), ("pad", i32), ("relu", i32),
                ("transposed", i32), ("reserved", i32), ("packed_floats", C.c_int64), ("x", vp), ("packed", vp), ("bias", vp), ("skip", vp), ("y", vp)]


class BnStatsParams(C.Structure):
    _fields_ = [("n", C.c_int64), ("C", C.c_int64), ("S", C.c_int64), ("workspace_triples", C.c_int64), ("y", vp), ("workspace", vp)]


class BnApplyParams(C.Structure):
    _fields_ = [("n", C.c_int64), ("C", C.c_int64), ("S", C.c_int64), ("workspace_triples", C.c_int64), ("eps", f32), ("momentum", f32), ("relu", i32),
                ("reserved", i32), ("y", vp), ("workspace", vp), ("weight", vp), ("bias", vp), ("skip", vp), ("out", vp), ("saved_mean", vp),
                ("saved_var", vp), ("running_mean", vp), ("running_var", vp), ("num_batches_tracked", vp)]


class Conv3dWgradParams(C.Structure):
    _fields_ = [("n", i32), ("cin", i32), ("D", i32), ("H", i32), ("W", i32), ("cout", i32), ("K", i32), ("stride", i32), ("pad", i32),
                ("transposed", i32), ("workspace_floats", C.c_int64), ("x", vp), ("grad_y", vp), ("workspace", vp), ("grad_weight", vp)]


class BnBwdReduceParams(C.Structure):
    _fields_ = [("n", C.c_int64), ("C", C.c_int64), ("S", C.c_int64), ("workspace_pairs", C.c_int64), ("eps", f32), ("relu", i32), ("g", vp),
                ("y", vp), ("saved_mean", vp), ("saved_var", vp), ("weight", vp), ("bias", vp), ("workspace", vp)]


class BnBwdApplyParams(C.Structure):
    _fields_ = [("n", C.c_int64), ("C", C.c_int64), ("S", C.c_int64), ("workspace_pairs", C.c_int64), ("eps", f32), ("relu", i32), ("g", vp),
                ("y", vp), ("saved_mean", vp), ("saved_var", vp), ("weight", vp), ("bias", vp), ("workspace", vp), ("grad_y", vp),
                ("grad_weight", vp), ("grad_bias", vp)]


class Conv2dWgradParams(C.Structure):
    _fields_ = [("n", i32), ("cin", i32), ("H", i32), ("W", i32), ("cout", i32), ("K", i32), ("stride", i32), ("pad", i32),
                ("workspace_floats", C.c_int64), ("x", vp), ("grad_y", vp), ("workspace", vp), ("grad_weight", vp)]


class Conv2dDgradS2Params(C.Structure):
    _fields_ = [("n", i32), ("cin", i32), ("H", i32), ("W", i32), ("cout", i32), ("K", i32), ("grad_y", vp), ("weight", vp), ("grad_x", vp)]


class Conv2dBiasGradParams(C.Structure):
    _fields_ = [("n", i32), ("cout", i32), ("OH", i32), ("OW", i32), ("grad_y", vp), ("grad_bias", vp)]


# the grouped batch-norm: each struct is its ungrouped counterpart's with G in front
class BnStatsGroupsParams(C.Structure):
    _fields_ = [("G", C.c_int64)] + BnStatsParams._fields_


class BnApplyGroupsParams(C.Structure):
    _fields_ = [("G", C.c_int64)] + BnApplyParams._fields_


class BnBwdReduceGroupsParams(C.Structure):
    _fields_ = [("G", C.c_int64)] + BnBwdReduceParams._fields_


class BnBwdApplyGroupsParams(C.Structure):
    _fields_ = [("G", C.c_int64)] + BnBwdApplyParams._fields_


class CasLossParams(C.Structure):
    _fields_ = [("n_stages", i32), ("with_weight", i32), ("n", i32 * 3), ("stage_w", f32 * 3), ("est", vp * 3), ("gt", vp * 3), ("w", vp * 3),
                ("workspace", vp), ("total", vp), ("stage_loss", vp), ("count", vp), ("wpair", vp * 3), ("status", vp)]


class CasLossBwdParams(C.Structure):
    _fields_ = [("n_stages", i32), ("n", i32 * 3), ("stage_w", f32 * 3), ("est", vp * 3), ("gt", vp * 3), ("wpair", vp * 3), ("count", vp),
                ("g_total", vp), ("g_stage", vp), ("g_est", vp * 3)]


class ImagePutParams(C.Structure):
    _fields_ = [("n", i32), ("first_pixel", i32), ("pixels", i32), ("rgb", vp), ("depth", vp), ("rgb_chw", vp), ("depth_hw", vp), ("minmax", vp)]


class DepthMinmaxParams(C.Structure):
    _fields_ = [("count", i32), ("depth", vp), ("minmax", vp)]


class DepthColormapParams(C.Structure):
    _fields_ = [("count", i32), ("range_host", C.c_double * 2), ("depth", vp), ("minmax", vp), ("table", vp), ("index", vp), ("color", vp)]


class SampleAssembleParams(C.Structure):
    _fields_ = [("N", i32), ("H", i32), ("W", i32), ("V", i32), ("h1", i32), ("w1", i32), ("h2", i32), ("w2", i32), ("frame_stride", i32),
                ("kp_total", i32), ("kp_first", i32), ("n_kp", i32), ("n_rows", i32), ("view_ids", i32 * 9), ("mean", f32 * 3), ("std", f32 * 3),
                ("unpre_mean", f32 * 3), ("unpre_std", f32 * 3), ("near_far", f32 * 2), ("frames", vp), ("depth_img", vp), ("weight_img", vp),
                ("row1", vp), ("col1", vp), ("row2", vp), ("col2", vp), ("kp_depth", vp), ("kp_weight", vp), ("kp_coord", vp), ("perm", vp),
                ("c2w", vp), ("w2c", vp), ("intrinsic", vp), ("affine", vp), ("affine_inv", vp), ("ref_proj_inv", vp), ("images", vp),
                ("images_unpre", vp), ("sd1", vp), ("sd2", vp), ("wt1", vp), ("wt2", vp), ("rays_depth", vp), ("c2ws", vp), ("w2cs", vp),
                ("intrinsics", vp), ("affine_mat", vp), ("affine_mat_inv", vp), ("proj_mats", vp), ("near_fars", vp), ("view_ids_out", vp)]


class ResizeParams(C.Structure):
    _fields_ = [("N", i32), ("Hin", i32), ("Win", i32), ("H", i32), ("W", i32), ("ksize_x", i32), ("ksize_y", i32), ("reserved", i32),
                ("src_frame_stride", C.c_int64), ("dst_frame_stride", C.c_int64), ("src", vp), ("dst", vp), ("start_x", vp), ("count_x", vp),
                ("k_x", vp), ("start_y", vp), ("count_y", vp), ("k_y", vp)]


class StepTargetsParams(C.Structure):
    _fields_ = [("H", i32), ("W", i32), ("n_total", i32), ("n_rays", i32), ("patch_num", i32), ("patch_size", i32), ("coord_is_float", i32),
                ("reserved", i32), ("sparse_depths", vp), ("sparse_weights", vp), ("dpt", vp), ("pixel_coordinates", vp), ("target_depths", vp),
                ("target_weights", vp), ("patch_dpt", vp), ("status", vp)]


class NovelAssembleParams(C.Structure):
    _fields_ = [("N", i32), ("H", i32), ("W", i32), ("V", i32), ("frame_stride", i32), ("P", i32), ("pose_index", i32), ("n_cand", i32),
                ("mean", f32 * 3), ("std", f32 * 3), ("unpre_mean", f32 * 3), ("unpre_std", f32 * 3), ("near_far", f32 * 2), ("frames", vp),
                ("c2w", vp), ("w2c", vp), ("intrinsic", vp), ("affine", vp), ("affine_inv", vp), ("poses", vp), ("cand", vp), ("intrinsic_in", vp),
                ("images", vp), ("images_unpre", vp), ("c2ws", vp), ("w2cs", vp), ("intrinsics", vp), ("affine_mat", vp), ("affine_mat_inv", vp),
                ("proj_mats", vp), ("near_fars", vp), ("view_ids_out", vp)]


class DepthConsistencyParams(C.Structure):
    _fields_ = [("N", i32), ("H", i32), ("W", i32), ("S", i32), ("min_views", i32), ("pix_thresh", f32), ("rel_thresh", f32), ("conf_thresh", f32),
                ("depth", vp), ("intrinsics", vp), ("c2ws", vp), ("w2cs", vp), ("src_ids", vp), ("conf", vp), ("count", vp), ("mask", vp), ("fused", vp)]


class PointsCompactParams(C.Structure):
    _fields_ = [("N", i32), ("H", i32), ("W", i32), ("reserved", i32), ("cap", C.c_int64), ("fused", vp), ("mask", vp), ("rgb", vp), ("intrinsics", vp),
                ("c2ws", vp), ("workspace", vp), ("points", vp), ("colors", vp), ("total", vp)]


class RenderParams(C.Structure):
    _fields_ = [("n", i32), ("S", i32), ("white_bkgd", i32), ("max_blocks", i32), ("cfg", MlpConfig), ("rays_o", vp),
                ("rays_d", vp), ("z", vp), ("w2c_ref", f32 * 12), ("K_ref", f32 * 9), ("w2c_dir", f32 * 12),
                ("near", f32), ("far", f32), ("near_far", vp), ("H", i32), ("W", i32), ("vol_d", i32 * 3),
                ("vol_h", i32 * 3), ("vol_w", i32 * 3), ("vol", vp * 3), ("conf", vp), ("imgs", vp), ("img_feat", vp),
                ("w2cs", vp), ("intrinsics", vp), ("wstream", vp), ("cl", ClSources), ("workspace", vp), ("rgb_map", vp),
                ("depth_map", vp), ("acc_map", vp), ("weights", vp), ("var", vp), ("raw", vp), ("feats", vp),
                ("ev_mlp_start", vp), ("ev_mlp_stop", vp), ("train_workspace", vp), ("dir_feat", vp), ("u_sampled", vp),
                ("wu_map", vp), ("pts_in", vp), ("ndc1_in", vp), ("ndc2_in", vp), ("ndc3_in", vp), ("ndc_in", vp), ("feats_tiled", i32), ("train_bwd_mode", i32),
                ("resample", vp), ("w2c_dir_dev", vp), ("gen_rays", vp), ("gen_depths", vp)]


class RenderBwdParams(C.Structure):
    _fields_ = [("fwd", RenderParams), ("g_rgb", vp), ("g_depth", vp), ("flat_params", vp), ("g_flat", vp),
                ("g_vol", vp * 3), ("g_conf", vp), ("g_img_feat", vp), ("workspace", vp), ("gather_scratch", vp),
                ("saved_valid", i32), ("bwd_mode", i32), ("g_cl", ClGrads)]


STRUCTS = {
    "ucnerf_ray_gen_params": RayGenParams, "ucnerf_ndc_rays_params": NdcRaysParams,
    "ucnerf_dir_feature_params": DirFeatureParams, "ucnerf_sample_stratified_params": SampleStratifiedParams,
    "ucnerf_sample_cascade_params": SampleCascadeParams, "ucnerf_ndc_project_params": NdcProjectParams,
    "ucnerf_embed_params": EmbedParams, "ucnerf_feat_gather_params": FeatGatherParams,
    "ucnerf_feat_gather_bwd_params": FeatGatherBwdParams, "ucnerf_mlp_config": MlpConfig,
    "ucnerf_mlp_params": MlpParams, "ucnerf_mlp_bwd_params": MlpBwdParams, "ucnerf_composite_params": CompositeParams,
    "ucnerf_composite_bwd_params": CompositeBwdParams, "ucnerf_sample_pdf_params": SamplePdfParams,
    "ucnerf_render_params": RenderParams, "ucnerf_render_bwd_params": RenderBwdParams,
    "ucnerf_merge_rows_params": MergeRowsParams,
    "ucnerf_cost_volume_params": CostVolumeParams, "ucnerf_depth_regress_params": DepthRegressParams,
    "ucnerf_cost_volume_bwd_params": CostVolumeBwdParams, "ucnerf_depth_regress_bwd_params": DepthRegressBwdParams,
    "ucnerf_cl_sources": ClSources, "ucnerf_cl_grads": ClGrads, "ucnerf_build_rays_test_params": BuildRaysTestParams,
}

# structs added to ABI v6 after its struct table was fixed (STRUCTS above is that table, kept as it was: additive entry points move nothing in it);
# checked against the library's sizeof() at load time like the others
ADDED_STRUCTS = {"ucnerf_depth_hypotheses_params": DepthHypothesesParams, "ucnerf_build_rays_train_params": BuildRaysTrainParams,
                 "ucnerf_composite_merged_params": CompositeMergedParams, "ucnerf_depth_eval_params": DepthEvalParams,
                 "ucnerf_image_eval_params": ImageEvalParams, "ucnerf_composite_merged_bwd_params": CompositeMergedBwdParams,
                 "ucnerf_cas_loss_params": CasLossParams, "ucnerf_cas_loss_bwd_params": CasLossBwdParams,
                 "ucnerf_image_put_params": ImagePutParams, "ucnerf_depth_minmax_params": DepthMinmaxParams,
                 "ucnerf_depth_colormap_params": DepthColormapParams,
                 "ucnerf_depth_regress_bwd_values_params": DepthRegressBwdValuesParams,
                 "ucnerf_depth_hypotheses_bwd_params": DepthHypothesesBwdParams,
                 "ucnerf_composite_fold_params": CompositeFoldParams,
                 "ucnerf_conv2d_pack_params": Conv2dPackParams, "ucnerf_conv2d_params": Conv2dParams,
                 "ucnerf_maxpool2d_params": Maxpool2dParams, "ucnerf_lpips_layer_params": LpipsLayerParams,
                 "ucnerf_lpips_alex_params": LpipsAlexParams,
                 "ucnerf_conv3d_pack_params": Conv3dPackParams, "ucnerf_conv3d_params": Conv3dParams,
                 "ucnerf_bn_stats_params": BnStatsParams, "ucnerf_bn_apply_params": BnApplyParams,
                 "ucnerf_conv3d_wgrad_params": Conv3dWgradParams, "ucnerf_bn_bwd_reduce_params": BnBwdReduceParams,
                 "ucnerf_bn_bwd_apply_params": BnBwdApplyParams,
                 "ucnerf_conv2d_wgrad_params": Conv2dWgradParams, "ucnerf_conv2d_dgrad_s2_params": Conv2dDgradS2Params,
                 "ucnerf_conv2d_bias_grad_params": Conv2dBiasGradParams,
                 "ucnerf_bn_stats_groups_params": BnStatsGroupsParams, "ucnerf_bn_apply_groups_params": BnApplyGroupsParams,
                 "ucnerf_bn_bwd_reduce_groups_params": BnBwdReduceGroupsParams, "ucnerf_bn_bwd_apply_groups_params": BnBwdApplyGroupsParams,
                 "ucnerf_step_targets_params": StepTargetsParams, "ucnerf_novel_assemble_params": NovelAssembleParams,
                 "ucnerf_depth_consistency_params": DepthConsistencyParams, "ucnerf_points_compact_params": PointsCompactParams,
                 "ucnerf_sample_assemble_params": SampleAssembleParams, "ucnerf_resize_params": ResizeParams}

# every symbol include/ucnerf_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "ucnerf_last_error": (C.c_char_p, []),
    "ucnerf_abi_version": (C.c_int, []),
    "ucnerf_sizeof": (C.c_int, [C.c_char_p]),
    "ucnerf_device_cus": (C.c_int, []),
    "ucnerf_build_flags": (C.c_char_p, []),
    "ucnerf_fused_tail_launches": (C.c_int64, []),
    "ucnerf_set_fused_tail": (C.c_int32, [C.c_int32]),
    "ucnerf_fused_tail_fits": (C.c_int32, [C.c_int32, C.c_int32]),
    "ucnerf_fused_tail_fits_resample": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "ucnerf_reuse_coarse_pays": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "ucnerf_source_hash": (C.c_char_p, []),
    "ucnerf_event_create": (C.c_void_p, []),
    "ucnerf_event_record": (C.c_int, [_P, _P]),
    "ucnerf_event_elapsed_ms": (C.c_int, [_P, _P, _P]),
    "ucnerf_event_destroy": (C.c_int, [_P]),
    "ucnerf_ray_gen": (C.c_int, [_P, _P]),
    "ucnerf_ndc_rays": (C.c_int, [_P, _P]),
    "ucnerf_dir_feature": (C.c_int, [_P, _P]),
    "ucnerf_sample_stratified": (C.c_int, [_P, _P]),
    "ucnerf_ray_gen_sample": (C.c_int, [_P, _P, _P]),
    "ucnerf_sample_cascade": (C.c_int, [_P, _P]),
    "ucnerf_ndc_project": (C.c_int, [_P, _P]),
    "ucnerf_build_rays_test": (C.c_int, [_P, _P]),
    "ucnerf_build_rays_train": (C.c_int, [_P, _P]),
    "ucnerf_embed": (C.c_int, [_P, _P]),
    "ucnerf_feat_gather_fwd": (C.c_int, [_P, _P]),
    "ucnerf_feat_gather_bwd": (C.c_int, [_P, _P]),
    "ucnerf_feat_gather_bwd_scratch_floats": (C.c_int64, [_P]),
    "ucnerf_mlp_param_count": (C.c_int64, [_P]),
    "ucnerf_mlp_stream_count": (C.c_int64, [_P]),
    "ucnerf_mlp_index_count": (C.c_int64, [_P]),
    "ucnerf_mlp_pack_index": (C.c_int, [_P, _P]),
    "ucnerf_mlp_pack": (C.c_int, [_P, _P, _P, _P, _P]),
    "ucnerf_mlp_pack_tensors": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P]),
    "ucnerf_mlp_unpack_grad": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "ucnerf_mlp_fwd": (C.c_int, [_P, _P]),
    # the guarded fp16 split (additive to ABI v6): the call of the same name plus a status / condition word
    "ucnerf_mlp_fwd_guarded": (C.c_int, [_P, _P, _P]),
    "ucnerf_mlp_fwd_if": (C.c_int, [_P, _P, _P]),
    "ucnerf_mlp_pack_guarded": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "ucnerf_mlp_pack_if": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "ucnerf_mlp_pack_tensors_guarded": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "ucnerf_mlp_pack_tensors_if": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "ucnerf_render_fused_fwd_guarded": (C.c_int, [_P, _P, _P]),
    "ucnerf_render_fused_fwd_if": (C.c_int, [_P, _P, _P]),
    "ucnerf_mlp_bwd_workspace_floats": (C.c_int64, [_P, C.c_int32]),
    "ucnerf_mlp_bwd": (C.c_int, [_P, _P]),
    "ucnerf_mlp_fwd_train": (C.c_int, [_P, _P, C.c_int32, _P]),
    "ucnerf_composite_fwd": (C.c_int, [_P, _P]),
    "ucnerf_composite_bwd": (C.c_int, [_P, _P]),
    "ucnerf_sample_pdf": (C.c_int, [_P, _P]),
    "ucnerf_composite_sample_pdf": (C.c_int, [_P, _P, _P]),
    "ucnerf_merge_rows": (C.c_int, [_P, _P]),
    "ucnerf_composite_merged_fwd": (C.c_int, [_P, _P]),
    "ucnerf_composite_merged_bwd": (C.c_int, [_P, _P]),
    # the gradient fold of var / disp / composited uncertainty (additive to ABI v6)
    "ucnerf_composite_fold_grads": (C.c_int, [_P, _P]),
    "ucnerf_cost_volume": (C.c_int, [_P, _P]),
    "ucnerf_depth_regress": (C.c_int, [_P, _P]),
    "ucnerf_cost_volume_bwd": (C.c_int, [_P, _P]),
    "ucnerf_depth_regress_bwd": (C.c_int, [_P, _P]),
    "ucnerf_depth_hypotheses": (C.c_int, [_P, _P]),
    # the gradient chain depth regression -> depth_values -> hypotheses -> previous depth (additive to ABI v6)
    "ucnerf_depth_regress_bwd_values": (C.c_int, [_P, _P]),
    "ucnerf_depth_hypotheses_bwd_scratch_floats": (C.c_int64, [_P]),
    "ucnerf_depth_hypotheses_bwd": (C.c_int, [_P, _P]),
    # the evaluation metrics (additive to ABI v6)
    "ucnerf_eval_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "ucnerf_depth_eval": (C.c_int, [_P, _P]),
    "ucnerf_image_eval": (C.c_int, [_P, _P]),
    # LPIPS: the AlexNet feature kernels and the distance (additive to ABI v6)
    "ucnerf_conv2d_packed_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "ucnerf_conv2d_pack": (C.c_int, [_P, _P]),
    "ucnerf_conv2d_bias_relu": (C.c_int, [_P, _P]),
    "ucnerf_maxpool2d": (C.c_int, [_P, _P]),
    "ucnerf_lpips_layer": (C.c_int, [_P, _P]),
    "ucnerf_lpips_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "ucnerf_lpips_alex": (C.c_int, [_P, _P]),
    # the 3-D convolutions of the cost regularisation (additive to ABI v6)
    "ucnerf_conv3d_packed_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ucnerf_conv3d_pack": (C.c_int, [_P, _P]),
    "ucnerf_conv3d": (C.c_int, [_P, _P]),
    # batch-statistic batch-norm for the CNNs under train() + no_grad (additive to ABI v6)
    "ucnerf_bn_partials": (C.c_int64, [C.c_int64, C.c_int64]),
    "ucnerf_bn_stats": (C.c_int, [_P, _P]),
    "ucnerf_bn_apply": (C.c_int, [_P, _P]),
    # CostRegNet's training route: the convolution's weight gradient and the batch-norm backward (additive to ABI v6)
    "ucnerf_conv3d_wgrad_workspace_floats": (C.c_int64, [C.c_int32] * 10),
    "ucnerf_conv3d_wgrad": (C.c_int, [_P, _P]),
    "ucnerf_bn_bwd_reduce": (C.c_int, [_P, _P]),
    "ucnerf_bn_bwd_apply": (C.c_int, [_P, _P]),
    # FeatureNet's training route: the 2-D weight gradient, the stride-2 input gradient and the bias gradient (additive to ABI v6)
    "ucnerf_conv2d_wgrad_workspace_floats": (C.c_int64, [C.c_int32] * 8),
    "ucnerf_conv2d_wgrad": (C.c_int, [_P, _P]),
    "ucnerf_conv2d_dgrad_s2": (C.c_int, [_P, _P]),
    "ucnerf_conv2d_bias_grad": (C.c_int, [_P, _P]),
    # batch-norm with the statistics kept per group of images: FeatureNet over all views in one pass (additive to ABI v6)
    "ucnerf_bn_stats_groups": (C.c_int, [_P, _P]),
    "ucnerf_bn_apply_groups": (C.c_int, [_P, _P]),
    "ucnerf_bn_bwd_reduce_groups": (C.c_int, [_P, _P]),
    "ucnerf_bn_bwd_apply_groups": (C.c_int, [_P, _P]),
    # the cascade depth loss on the device (additive to ABI v6)
    "ucnerf_cas_loss_workspace_floats": (C.c_int64, [C.c_int32, _P]),
    "ucnerf_cas_loss_fwd": (C.c_int, [_P, _P]),
    "ucnerf_cas_loss_bwd": (C.c_int, [_P, _P]),
    # a whole validation image on the device (additive to ABI v6)
    "ucnerf_image_group_pixels": (C.c_int32, []),
    "ucnerf_minmax_reset": (C.c_int, [_P, _P]),
    "ucnerf_minmax_read": (C.c_int, [_P, _P, _P]),
    "ucnerf_image_put": (C.c_int, [_P, _P]),
    "ucnerf_depth_minmax": (C.c_int, [_P, _P]),
    "ucnerf_depth_colormap": (C.c_int, [_P, _P]),
    # one sample of the dataset out of a device-resident scene (additive to ABI v6)
    "ucnerf_sample_assemble": (C.c_int, [_P, _P]),
    # Pillow's BILINEAR resize of the colour frames: coefficient tables on the host, both passes in one launch (additive to ABI v6)
    "ucnerf_resize_bilinear_ksize": (C.c_int, [C.c_int, C.c_int]),
    "ucnerf_resize_bilinear_coeffs": (C.c_int, [C.c_int, C.c_int, _P, _P, _P]),
    "ucnerf_resize_bilinear_u8": (C.c_int, [_P, _P]),
    # the training step's three target gathers in one launch (additive to ABI v6)
    "ucnerf_step_targets": (C.c_int, [_P, _P]),
    # the batch of a free camera pose: matrices in closed form, the nearest source views picked on the device (additive to ABI v6)
    "ucnerf_novel_assemble": (C.c_int, [_P, _P]),
    "ucnerf_depth_consistency": (C.c_int, [_P, _P]),
    "ucnerf_points_compact_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ucnerf_points_compact": (C.c_int, [_P, _P]),
    "ucnerf_render_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "ucnerf_render_fused_fwd": (C.c_int, [_P, _P]),
    "ucnerf_gather_repack_floats": (C.c_int64, [_P]),
    "ucnerf_gather_repack": (C.c_int, [_P, _P, _P, _P]),
    "ucnerf_gather_repack_masked": (C.c_int, [_P, _P, _P, C.c_uint32, _P]),      # (additive to ABI v6)
    "ucnerf_render_bwd_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "ucnerf_render_fused_bwd": (C.c_int, [_P, _P]),
}

_lib = None


def lib():
    """Loads the library once; raises if it is absent or its ABI does not match this binding."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64 (same SONAME as the system one).  Device pointers and streams
    # handed over by torch are only meaningful inside THAT runtime instance, so it has to be the one our
    # library binds to: make sure it is resident before dlopen() resolves libucnerf_hip.so's dependency.
    import torch
    tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tl):
        C.CDLL(tl, mode=C.RTLD_GLOBAL)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("uc_nerf_amd: %s is missing -- build it with `python -m uc_nerf_amd.build` "
                           "(there is no CPU or PyTorch fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            raise RuntimeError("uc_nerf_amd: %s does not export %s" % (LIB_PATH, name)) from e
        fn.restype, fn.argtypes = res, args
    if L.ucnerf_abi_version() != ABI_VERSION:
        raise RuntimeError("uc_nerf_amd: ABI version mismatch")
    for cname, cls in list(STRUCTS.items()) + list(ADDED_STRUCTS.items()):
        got = L.ucnerf_sizeof(cname.encode())
        if got != C.sizeof(cls):
            raise RuntimeError("uc_nerf_amd: struct %s is %d bytes in the library, %d in the binding"
                               % (cname, got, C.sizeof(cls)))
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise RuntimeError("uc_nerf_amd: %s failed (%d): %s" % (what, rc, lib().ucnerf_last_error().decode()))


def call(name, params, stream):
    """Invokes an `int f(const params*, stream)` entry point."""
    check(getattr(lib(), name)(C.addressof(params), C.c_void_p(stream)), name)
