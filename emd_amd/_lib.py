"""ctypes binding of libemd_raster.so (include/emd_raster.h).

The library is built in-tree by `emd_amd.build.build_native()` (hipcc --offload-arch=gfx950).  There is NO
fallback: if the shared object is missing or fails to load, every operator raises -- a silent CPU/eager path
would void the parity claims of this package.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libemd_raster.so")

ABI_VERSION = 31
MAX_EXTRA = 2
SETTINGS_DEV_FLOATS = 38
TILE = 16
ACTOR_STRIDE = 12
BWD_PAYLOAD = 12
SKIN_JOINTS = 24         # EMD_SKIN_JOINTS
SKIN_CHUNK = 256         # EMD_SKIN_CHUNK: most points of one chunk of the skinning point layout (csrc/skinning.hip)
SKIN_PARTIAL_FLOATS = 291  # EMD_SKIN_PARTIAL_FLOATS: one chunk's slab of the skinning backward, 24 x 12 sums of dL/dA + 3 of dL/dtrans
SEG_CHUNK = 512          # EMD_SEG_CHUNK: chunk length of the pinned association of the segmented row sum (csrc/segsum.h)


def bwd_stride(num_extra=0):
    """Pitch in floats of an accumulator row of the render backward (emd_bwd_stride of csrc/common.h): the 12 payload floats + 4 per extra
    colour set, rounded up to whole 64-byte lines."""
    return (BWD_PAYLOAD + 4 * int(num_extra) + 15) // 16 * 16


BWD_STRIDE = bwd_stride(0)

EMD_OK, EMD_ERR_INVALID, EMD_ERR_CAPACITY, EMD_ERR_HIP, EMD_ERR_WORKSPACE, EMD_ERR_DEPTH_RANGE = 0, -1, -2, -3, -4, -5
FLAG_NORMAL, FLAG_MOTION, FLAG_ABSGRAD, FLAG_NO_SYNC, FLAG_CLAMP_RGB01, FLAG_RAW_PARAMS, FLAG_SDEV_TANFOV = 1, 2, 4, 8, 16, 32, 64
FLAG_WIDE_DEPTH_SORT = 128
FLAG_BWD_WS_CLEAN = 256
FLAG_KEEP_ALL_PAIRS = 512
FLAG_BWD_RENDER_ONLY = 1024
FLAG_BWD_PROJECT_ONLY = 2048
FLAG_DETERMINISTIC = 4096

_f = C.c_void_p  # device pointers are passed as integers


class EmdSettings(C.Structure):
    _fields_ = [("image_height", C.c_int32), ("image_width", C.c_int32), ("tanfovx", C.c_float),
                ("tanfovy", C.c_float), ("bg", C.c_float * 3), ("scale_modifier", C.c_float),
                ("viewmatrix", C.c_float * 16), ("projmatrix", C.c_float * 16), ("sh_degree", C.c_int32),
                ("campos", C.c_float * 3), ("prefiltered", C.c_int32), ("debug", C.c_int32),
                ("near_plane", C.c_float)]


class EmdMotion(C.Structure):
    _fields_ = [("actor_id", _f), ("actor_pose", _f), ("num_actors", C.c_int32), ("residual_dx", _f),
                ("residual_dq", _f)]


class EmdDims(C.Structure):
    _fields_ = [("num_gaussians", C.c_int32), ("image_height", C.c_int32), ("image_width", C.c_int32),
                ("bin_capacity", C.c_int64), ("flags", C.c_int32), ("num_extra", C.c_int32)]


class EmdFwdArgs(C.Structure):
    _fields_ = [("s", EmdSettings), ("num_gaussians", C.c_int32), ("sh_coeffs", C.c_int32), ("flags", C.c_int32),
                ("bin_capacity", C.c_int64),
                ("means3D", _f), ("shs", _f), ("colors_precomp", _f), ("opacities", _f), ("scales", _f),
                ("rotations", _f), ("cov3D_precomp", _f), ("motion", EmdMotion),
                ("out_color", _f), ("out_depth", _f), ("out_normal", _f), ("out_alpha", _f), ("radii", _f),
                ("geom_ws", _f), ("geom_bytes", C.c_size_t), ("bin_ws", _f), ("bin_bytes", C.c_size_t),
                ("img_ws", _f), ("img_bytes", C.c_size_t), ("status", _f),
                ("num_rendered", C.c_int64), ("num_visible", C.c_int64), ("settings_dev", _f),
                ("num_extra", C.c_int32), ("colors_extra", _f * 2), ("out_extra", _f * 2), ("aux_stream", _f), ("shs_residual", _f * 2), ("loop_stats", _f)]


class EmdBwdArgs(C.Structure):
    _fields_ = [("s", EmdSettings), ("num_gaussians", C.c_int32), ("sh_coeffs", C.c_int32), ("flags", C.c_int32),
                ("bin_capacity", C.c_int64), ("num_rendered", C.c_int64),
                ("means3D", _f), ("shs", _f), ("colors_precomp", _f), ("opacities", _f), ("scales", _f),
                ("rotations", _f), ("cov3D_precomp", _f), ("motion", EmdMotion), ("radii", _f),
                ("geom_ws", _f), ("geom_bytes", C.c_size_t), ("bin_ws", _f), ("bin_bytes", C.c_size_t),
                ("img_ws", _f), ("img_bytes", C.c_size_t), ("status", _f),
                ("out_color", _f), ("out_depth", _f), ("out_normal", _f),
                ("dL_dcolor", _f), ("dL_ddepth", _f), ("dL_dalpha", _f), ("dL_dnormal", _f),
                ("bwd_ws", _f), ("bwd_bytes", C.c_size_t),
                ("dL_dmeans3D", _f), ("dL_dmeans2D", _f), ("dL_dmeans2D_abs", _f), ("dL_dshs", _f),
                ("dL_dcolors", _f), ("dL_dopacities", _f), ("dL_dscales", _f), ("dL_drotations", _f),
                ("dL_dcov3D", _f), ("dL_dactor_pose", _f), ("dL_dresidual_dx", _f), ("dL_dresidual_dq", _f),
                ("dL_dsh_color", _f), ("settings_dev", _f),
                ("num_extra", C.c_int32), ("colors_extra", _f * 2), ("out_extra", _f * 2), ("dL_dextra", _f * 2), ("dL_dcolors_extra", _f * 2),
                ("pair_stats", _f), ("det_ws", _f), ("det_bytes", C.c_size_t)]


SKY_CLAMP01, SKY_BLEND_S3G, SKY_BLEND_ADD, SKY_INTERLEAVED = 1, 2, 4, 8


class EmdSkyArgs(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("resolution", C.c_int32), ("flags", C.c_int32),
                ("cube", _f), ("dirs", _f), ("Kinv", C.c_float * 9), ("R", C.c_float * 9), ("T", C.c_float * 3),
                ("jitter", _f), ("acc", _f), ("mask_threshold", C.c_float), ("fill", C.c_float), ("fg", _f),
                ("sky", _f), ("out", _f), ("camera_dev", _f)]


class EmdSkyBwdArgs(C.Structure):
    _fields_ = [("f", EmdSkyArgs), ("dL_dout", _f), ("dL_dsky", _f), ("dL_dcube", _f), ("dL_dacc", _f), ("dL_dfg", _f)]


class EmdLossArgs(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("image", _f), ("gt", _f), ("depth", _f), ("gt_depth", _f),
                ("mask", _f), ("weight", _f), ("sky_mask", _f), ("lambda_dssim", C.c_float), ("lambda_depth", C.c_float),
                ("lambda_sky", C.c_float), ("max_depth", C.c_float), ("losses", _f), ("dL_dimage", _f), ("dL_ddepth", _f),
                ("dL_dweight", _f)]


HEX_FLAG_DETERMINISTIC = 1
HEX_MAX_SCALES = 8


class EmdHexArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("channels", C.c_int32), ("num_scales", C.c_int32), ("times_broadcast", C.c_int32),
                ("res", (C.c_int32 * 4) * HEX_MAX_SCALES), ("planes", (_f * 6) * HEX_MAX_SCALES), ("pts", _f), ("times", _f),
                ("aabb", C.c_float * 6), ("out", _f), ("order", _f), ("time_tables", _f)]


class EmdHexGrads(C.Structure):
    _fields_ = [("dL_dout", _f), ("dL_dplanes", (_f * 6) * HEX_MAX_SCALES), ("dL_dpts", _f), ("dL_dtimes", _f),
                ("order2d", C.c_void_p * 3), ("pos2d", C.c_void_p * 3), ("defer_rows", _f), ("defer_mask", C.c_uint32), ("flags", C.c_uint32), ("dL_dtime_sum", _f),
                ("det_ws", C.c_void_p), ("det_bytes", C.c_size_t), ("det_keep_plane", C.c_uint32)]       # (read only with HEX_FLAG_DETERMINISTIC)


PLANE_REG_SEG = 32       # EMD_PLANE_REG_SEG: rows of H one workgroup of the plane regularisers owns (csrc/plane_reg.hip)


class EmdPlaneRegArgs(C.Structure):
    _fields_ = [("channels", C.c_int32), ("num_scales", C.c_int32), ("res", (C.c_int32 * 4) * HEX_MAX_SCALES), ("planes", (_f * 6) * HEX_MAX_SCALES),
                ("plane_tv_weight", C.c_float), ("time_smoothness_weight", C.c_float), ("l1_time_planes_weight", C.c_float), ("reserved", C.c_float),
                ("out", _f), ("g", _f), ("dL_dplanes", (_f * 6) * HEX_MAX_SCALES)]


TRAINER_LOSS_CHUNK = 1024    # EMD_TRAINER_LOSS_CHUNK: pixels per fp64 partial of the trainer's loss tail and of dL/dA (csrc/trainer_loss.hip)
TRAINER_SSIM_TILE = 32       # EMD_TRAINER_SSIM_TILE: rows x floats of the [H-10][3 (W-10)] SSIM map one workgroup owns
TL_MASK_BCE, TL_MASK_SAFE_BCE = 0, 1
TL_DEPTH_L1, TL_DEPTH_L2, TL_DEPTH_SMOOTH_L1 = 0, 1, 2


class EmdTrainerLossArgs(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("mask_type", C.c_int32), ("depth_type", C.c_int32), ("normalize", C.c_int32),
                ("inverse", C.c_int32), ("rgb", _f), ("gt_rgb", _f), ("opacity", _f), ("sky_mask", _f), ("depth", _f), ("lidar_depth", _f),
                ("w_rgb", C.c_float), ("w_ssim", C.c_float), ("w_mask", C.c_float), ("safe_limit", C.c_float), ("w_depth", C.c_float),
                ("upper_bound", C.c_float), ("w_entropy", C.c_float), ("w_smooth", C.c_float), ("losses", _f), ("dL_drgb", _f),
                ("dL_dopacity", _f), ("dL_ddepth", _f)]


VANILLA_REG_CHUNK = 1024     # EMD_VANILLA_REG_CHUNK: Gaussians per fp64 partial of the VanillaGaussians regularisers (csrc/vanilla.hip)


class EmdVanillaArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("sh_coeffs", C.c_int32), ("degree", C.c_int32), ("sh_mode", C.c_int32),
                ("means", _f), ("log_scales", _f), ("quats", _f), ("opacity_logits", _f), ("features_dc", _f), ("features_rest", _f),
                ("camera_center", _f), ("opacities", _f), ("scales", _f), ("quats_out", _f), ("rgbs", _f), ("clamp_mask", _f),
                ("g_opacities", _f), ("g_scales", _f), ("g_quats", _f), ("g_rgbs", _f), ("dL_dopacity_logits", _f), ("dL_dlog_scales", _f),
                ("dL_dquats", _f), ("dL_dfeatures_dc", _f), ("dL_dfeatures_rest", _f)]


class EmdVanillaRegArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("reserved", C.c_int32), ("log_scales", _f), ("opacity_logits", _f), ("radii", _f),
                ("w_sharp", C.c_float), ("max_gauss_ratio", C.c_float), ("w_flatten", C.c_float), ("w_sparse", C.c_float),
                ("w_max_s_square", C.c_float), ("reserved1", C.c_float), ("terms", _f), ("g", _f), ("dL_dlog_scales", _f),
                ("dL_dopacity_logits", _f)]


class EmdDeformInArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("num_freqs_x", C.c_int32), ("num_freqs_t", C.c_int32), ("embed_dim", C.c_int32),
                ("ld", C.c_int32), ("reserved", C.c_int32), ("means", _f), ("point_ids", _f), ("inst_size", _f), ("inst_embed", _f),
                ("t", _f), ("out", _f)]


DENSIFY_MODE_DENSIFY, DENSIFY_MODE_PRUNE, DENSIFY_MODE_REFINE = 0, 1, 2
DENSIFY_ROLE_COPY, DENSIFY_ROLE_XYZ, DENSIFY_ROLE_SCALING, DENSIFY_ROLE_STATE, DENSIFY_ROLE_ZERO = 0, 1, 2, 3, 4
DENSIFY_MAX_TENSORS = 40


class EmdDensifyArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("mode", C.c_int32), ("scaling", _f), ("opacity", _f), ("grad_accum", _f), ("denom", _f),
                ("max_radii2D", _f), ("extra_drop", _f), ("grad_threshold", C.c_float), ("size_threshold", C.c_float),
                ("min_opacity", C.c_float), ("max_screen_size", C.c_float)]


class EmdRefineArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("do_densify", C.c_int32), ("do_cull", C.c_int32), ("use_split_screen", C.c_int32), ("cull_big", C.c_int32),
                ("use_cull_screen", C.c_int32), ("scaling", _f), ("opacity", _f), ("grad_norm", _f), ("vis_counts", _f), ("max_2Dsize", _f),
                ("grad_threshold", C.c_float), ("size_threshold", C.c_float), ("split_screen", C.c_float), ("cull_alpha", C.c_float),
                ("cull_size", C.c_float), ("cull_screen", C.c_float)]


class EmdRefineNodesArgs(C.Structure):
    """EmdRefineArgs's fields, then the actor part (include/emd_raster.h)."""
    _fields_ = EmdRefineArgs._fields_ + [("means", _f), ("rotation", _f), ("ids", _f), ("instances_size", _f), ("num_actors", C.c_int32),
                                         ("num_samples", C.c_int32), ("cull_out_of_bound", C.c_int32), ("group_by_actor", C.c_int32),
                                         ("seed", C.c_uint64), ("samples", _f)]


class EmdDensifyTensor(C.Structure):
    _fields_ = [("src", _f), ("dst", _f), ("width", C.c_int32), ("role", C.c_int32)]


class EmdDensifyGather(C.Structure):
    _fields_ = [("num_out", C.c_int32), ("num_tensors", C.c_int32), ("mode", C.c_int32), ("num_split", C.c_int32), ("src", _f), ("kind", _f),
                ("scaling", _f), ("rotation", _f), ("seed", C.c_uint64), ("samples", _f), ("split_rank", _f),
                ("tensors", EmdDensifyTensor * DENSIFY_MAX_TENSORS)]


class EmdTrackArgs(C.Structure):
    _fields_ = [("num_actors", C.c_int32), ("rows", C.c_int32), ("dim", C.c_int32), ("embed_dim", C.c_int32), ("k_coarse", C.c_int32),
                ("k_fine", C.c_int32), ("num_points", C.c_int32), ("reserved", C.c_int32), ("t", C.c_float), ("t_dev", _f), ("k_fine_dev", _f), ("weight", _f),
                ("embeddings", _f), ("point_ids", _f), ("count", _f), ("segment_start", _f), ("head_w", _f * 4), ("head_b", _f * 4), ("emb_sum", _f),
                ("trans", _f), ("rot", _f)]


class EmdTrackGrads(C.Structure):
    _fields_ = [("g_trans", _f), ("g_rot", _f), ("d_weight", _f), ("d_embeddings", _f), ("d_head_w", _f * 4), ("d_head_b", _f * 4),
                ("d_mean", _f)]


class EmdStepSelect(C.Structure):
    _fields_ = [("sel", _f), ("rows", C.c_int32), ("row_floats", C.c_int32), ("table", _f), ("out_row", _f), ("frames", _f),
                ("frame_out", _f), ("t_out", _f), ("num_frames", C.c_int32), ("k_min", C.c_int32), ("k_max", C.c_int32),
                ("k_until", C.c_int32), ("steps", _f), ("k_fine_out", _f), ("status", _f), ("status_log", _f), ("prev_sel", _f),
                ("next_sel", _f)]


class EmdTrackedPoseArgs(C.Structure):
    _fields_ = [("track", EmdTrackArgs), ("q_all", _f), ("t_all", _f), ("valid_all", _f), ("num_frames", C.c_int32), ("frame", C.c_int32),
                ("frame_dev", _f), ("pose", _f), ("head_acc", _f), ("head_acc_floats", C.c_int32), ("reserved", C.c_int32)]


class EmdTrackedPoseGrads(C.Structure):
    _fields_ = [("g_pose", _f), ("d_q_all", _f), ("d_t_all", _f), ("d_weight", _f), ("d_embeddings", _f), ("d_head_w", _f * 4),
                ("d_head_b", _f * 4)]


MLP_MAX_BRANCHES = 6


class EmdMlpTrunk(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("ka", C.c_int32), ("kb", C.c_int32), ("ld_w", C.c_int32), ("col_a", C.c_int32),
                ("col_b", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32), ("xa", _f), ("xb", _f), ("w", _f), ("b", _f), ("h", _f)]


class EmdMlpTrunkGrads(C.Structure):
    _fields_ = [("num_gh", C.c_int32), ("reserved", C.c_int32), ("g_h", _f * MLP_MAX_BRANCHES), ("d_xa", _f), ("d_xb", _f), ("d_w", _f), ("d_b", _f)]


class EmdMlpBranch(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("depth", C.c_int32), ("relu_input", C.c_int32), ("out_dim", C.c_int32), ("h", _f),
                ("w_hidden", _f * 2), ("b_hidden", _f * 2), ("w_out", _f), ("b_out", _f), ("out", _f), ("l1_sum", _f),
                ("xb", _f), ("w_in", _f), ("b_in", _f), ("kb_in", C.c_int32), ("ld_w_in", C.c_int32), ("col_in", C.c_int32), ("reserved", C.c_int32)]


class EmdMlpBranchGrads(C.Structure):
    _fields_ = [("g_out", _f), ("g_h", _f), ("d_w_hidden", _f * 2), ("d_b_hidden", _f * 2), ("d_w_out", _f), ("d_b_out", _f),
                ("l1_grad", _f), ("out", _f), ("g_h_in", _f)]


MLP_DET_MAX_TENSORS, MLP_DET_MAX_JOBS = 6, 64
MLP_DET_BRANCH_BWD, MLP_DET_TRUNK_BWD, MLP_DET_BRANCH_FWD = 0, 1, 2


class EmdMlpDetLayout(C.Structure):
    _fields_ = [("groups", C.c_int32), ("num_tensors", C.c_int32), ("pitch", C.c_int32 * MLP_DET_MAX_TENSORS),
                ("offset", C.c_size_t * MLP_DET_MAX_TENSORS), ("bytes", C.c_size_t)]


class EmdMlpDetJob(C.Structure):
    _fields_ = [("slab", _f), ("dst", _f), ("groups", C.c_int32), ("pitch", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("ld", C.c_int32), ("col0", C.c_int32), ("scale", C.c_double)]


DEFORM_MLP_MAX_LAYERS, DEFORM_MLP_MIN_GROUP_ROWS = 16, 256


class EmdDeformMlpArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("depth", C.c_int32), ("width", C.c_int32), ("in_dim", C.c_int32), ("embed_dim", C.c_int32),
                ("skip", C.c_int32), ("ld_x", C.c_int32), ("num_cus", C.c_int32), ("x", _f), ("w", _f * DEFORM_MLP_MAX_LAYERS),
                ("b", _f * DEFORM_MLP_MAX_LAYERS), ("h", _f * DEFORM_MLP_MAX_LAYERS), ("w_head", _f * 3), ("b_head", _f * 3), ("out", _f * 3)]


class EmdDeformMlpGrads(C.Structure):
    _fields_ = [("g_out", _f * 3), ("d_w", _f * DEFORM_MLP_MAX_LAYERS), ("d_b", _f * DEFORM_MLP_MAX_LAYERS), ("d_w_head", _f * 3),
                ("d_b_head", _f * 3), ("d_x", _f), ("ld_dx", C.c_int32), ("reserved", C.c_int32), ("g_h", _f * 2), ("slab", _f),
                ("slab_bytes", C.c_size_t)]


class EmdDeformMlpLayout(C.Structure):
    _fields_ = [("groups", C.c_int32), ("group_rows", C.c_int32), ("pitch_w", C.c_int32), ("pitch_b", C.c_int32), ("offset_w", C.c_size_t),
                ("offset_b", C.c_size_t), ("bytes", C.c_size_t)]


ADAM_MAX_TENSORS = 32


class EmdAdamTensor(C.Structure):
    _fields_ = [("param", _f), ("grad", _f), ("exp_avg", _f), ("exp_avg_sq", _f), ("numel", C.c_int64), ("step_size", C.c_float),
                ("bias_correction2_sqrt", C.c_float), ("one_minus_beta1", C.c_float), ("beta2", C.c_float), ("one_minus_beta2", C.c_float),
                ("eps", C.c_float), ("step_dev", _f), ("lr_dev", _f)]


class EmdAdamArgs(C.Structure):
    _fields_ = [("num_tensors", C.c_int32), ("reserved", C.c_int32), ("tensors", EmdAdamTensor * ADAM_MAX_TENSORS)]


class EmdRadixSortArgs(C.Structure):
    _fields_ = [("keys_in", _f), ("keys", _f * 2), ("vals", _f * 2), ("hist", _f), ("n_cap", C.c_int64), ("n_dev", _f), ("n_dev_overflow", _f),
                ("passes", C.c_int32), ("bits", C.c_int32), ("offset", C.c_uint32), ("range_bits", C.c_int32), ("overflow_word", _f),
                ("count_out", _f)]


class EmdBinningArgs(C.Structure):
    _fields_ = [("num_gaussians", C.c_int32), ("image_height", C.c_int32), ("image_width", C.c_int32), ("flags", C.c_int32),
                ("near_plane", C.c_float), ("bin_capacity", C.c_int64), ("depth_key", _f), ("binrec", _f), ("geom_ws", _f),
                ("geom_bytes", C.c_size_t), ("bin_ws", _f), ("bin_bytes", C.c_size_t), ("status", _f), ("tile_order", _f)]


class EmdSegSumArgs(C.Structure):
    _fields_ = [("keys", _f), ("slots", _f), ("n_dev", _f), ("n_cap", C.c_int64), ("rows", _f), ("row_pitch", C.c_int32), ("width", C.c_int32),
                ("out", _f), ("out_pitch", C.c_int32), ("reserved", C.c_int32), ("partials", _f), ("partial_bytes", C.c_size_t)]


class EmdJointChainArgs(C.Structure):
    _fields_ = [("num_instances", C.c_int32), ("reserved", C.c_int32), ("theta", _f), ("joints", _f), ("parents", _f), ("canon_inv", _f), ("A", _f)]


class EmdSkinArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("num_instances", C.c_int32), ("num_chunks", C.c_int32), ("reserved", C.c_int32), ("means", _f),
                ("quats", _f), ("opacities", _f), ("ids", _f), ("weights", _f), ("A", _f), ("trans", _f), ("valid", _f), ("order", _f),
                ("chunks", _f), ("world_means", _f), ("world_quats", _f), ("opacities_out", _f)]


class EmdNeighbourStdArgs(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("k", C.c_int32), ("num_blocks", C.c_int32), ("reserved", C.c_int32), ("idx", _f), ("rev_start", _f),
                ("rev_slot", _f), ("x", _f * 8), ("cols", C.c_int32 * 8), ("act", C.c_int32 * 8), ("weight", C.c_float * 8), ("stash", _f),
                ("terms", _f), ("g_terms", _f), ("dx", _f * 8)]


class EmdSkinGrads(C.Structure):
    _fields_ = [("g_world_means", _f), ("g_world_quats", _f), ("g_opacities_out", _f), ("d_means", _f), ("d_quats", _f), ("d_opacities", _f),
                ("d_weights", _f), ("partials", _f)]


# every symbol include/emd_raster.h declares
EXPORTED_SYMBOLS = ("emd_abi_version", "emd_last_error", "emd_raster_workspace_size", "emd_raster_forward",
                    "emd_raster_backward", "emd_backward_fill_slice", "emd_raster_export_binning", "emd_raster_export_geometry", "emd_raster_export_contributed",
                    "emd_motion_forward", "emd_motion_backward", "emd_sh_forward", "emd_sh_backward",
                    "emd_profile_enable", "emd_profile_read", "emd_profile_stage_name", "emd_activations_forward", "emd_actor_pose_forward", "emd_actor_pose_backward", "emd_l1_loss",
                    "emd_sky_forward", "emd_sky_backward", "emd_image_loss_workspace", "emd_image_loss", "emd_hexplane_forward", "emd_hexplane_backward", "emd_hexplane_order_keys", "emd_sh_grad_from_factors", "emd_densification_stats",
                    "emd_temporal_embed_forward", "emd_temporal_embed_backward", "emd_deform_input_width", "emd_deform_input_forward",
                    "emd_deform_input_backward", "emd_adam_step", "emd_track_heads_forward", "emd_track_heads_backward",
                    "emd_densify_decide", "emd_densify_index", "emd_densify_split_rank", "emd_densify_gather",
                    "emd_refine_decide", "emd_refine_index", "emd_after_train_stats", "emd_densify_scan",
                    "emd_refine_nodes_decide", "emd_refine_nodes_index_workspace", "emd_refine_nodes_index",
                    "emd_mlp_trunk_forward", "emd_mlp_trunk_backward", "emd_mlp_branch_forward", "emd_mlp_branch_backward",
                    "emd_abs_mean_backward", "emd_residual_l1_backward", "emd_tracked_pose_forward", "emd_tracked_pose_backward",
                    "emd_select_step_inputs", "emd_compact_rows", "emd_scatter_rows", "emd_l1_loss_ws",
                    "emd_knn_workspace", "emd_knn", "emd_knn_reverse_workspace", "emd_knn_reverse", "emd_embed_reg_forward", "emd_embed_reg_backward",
                    "emd_radix_sort", "emd_raster_binning", "emd_camera_grad_workspace_size", "emd_raster_backward_camera",
                    "emd_raster_det_workspace_size", "emd_raster_det_layout", "emd_segmented_row_sum_workspace", "emd_segmented_row_sum",
                    "emd_hexplane_det_workspace_size", "emd_hexplane_det_workspace_offsets",
                    "emd_sky_det_workspace_size", "emd_sky_det_workspace_offsets", "emd_sky_backward_det",
                    "emd_motion_det_workspace_size", "emd_motion_det_workspace_offsets", "emd_motion_backward_det",
                    "emd_joint_chain_forward", "emd_joint_chain_backward", "emd_skin_forward", "emd_skin_backward",
                    "emd_plane_reg_workspace_size", "emd_plane_reg_forward", "emd_plane_reg_backward",
                    "emd_affine_workspace_size", "emd_affine_forward", "emd_affine_backward", "emd_trainer_loss_workspace_size", "emd_trainer_loss",
                    "emd_mlp_det_slab_bytes", "emd_mlp_branch_forward_det", "emd_mlp_branch_backward_det", "emd_mlp_trunk_backward_det", "emd_mlp_det_reduce",
                    "emd_deform_mlp_workspace", "emd_deform_mlp_forward", "emd_deform_mlp_backward",
                    "emd_temporal_embed_backward_det",
                    "emd_track_det_workspace_size", "emd_track_det_workspace_offsets", "emd_actor_row_sum_det", "emd_track_heads_forward_det",
                    "emd_track_heads_backward_det", "emd_tracked_pose_backward_det",
                    "emd_vanilla_forward", "emd_vanilla_backward", "emd_vanilla_reg_workspace_size", "emd_vanilla_reg_forward", "emd_vanilla_reg_backward",
                    "emd_knn_segments", "emd_neighbour_std_workspace_size", "emd_neighbour_std_forward", "emd_neighbour_std_backward")
CAMERA_GRAD_FLOATS = 35
KNN_MAX_K = 32
EMBED_REG_SCRATCH_WORDS = 2048
NSTD_MAX_BLOCKS, NSTD_MAX_COLS = 8, 64                     # EMD_NSTD_MAX_BLOCKS, EMD_NSTD_MAX_COLS
NSTD_ACT = {"identity": 0, "exp": 1, "sigmoid": 2}         # EMD_NSTD_ACT_*
PROF_STAGES = 8

_lib = None


class EmdError(RuntimeError):
    pass


def load():
    """Load the HIP extension; raise loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("EMD_LIB_PATH") or LIB_PATH          # (EMD_LIB_PATH: an alternative BUILD of the same library, for A/B timing)
    if not os.path.exists(path):
        raise EmdError(f"HIP extension not built: {path} is missing. Run `python -c 'import __graft_entry__ as g; "
                       f"g.build()'` (or `make -C emd_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name in EXPORTED_SYMBOLS:
        if not hasattr(lib, name):
            raise EmdError(f"{path} does not export {name}")
    lib.emd_abi_version.restype = C.c_int
    lib.emd_last_error.restype = C.c_char_p
    v = lib.emd_abi_version()
    if v != ABI_VERSION:
        raise EmdError(f"ABI mismatch: library {v}, binding {ABI_VERSION}")
    lib.emd_raster_workspace_size.argtypes = [C.POINTER(EmdDims), C.POINTER(C.c_size_t)]
    lib.emd_raster_forward.argtypes = [C.POINTER(EmdFwdArgs), C.c_void_p]
    lib.emd_raster_backward.argtypes = [C.POINTER(EmdBwdArgs), C.c_void_p]
    lib.emd_backward_fill_slice.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.emd_raster_export_binning.argtypes = [C.POINTER(EmdDims), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_raster_export_geometry.argtypes = [C.POINTER(EmdDims), C.c_void_p, C.c_size_t] + [C.c_void_p] * 7
    lib.emd_raster_export_contributed.argtypes = [C.POINTER(EmdDims), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.emd_motion_forward.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EmdMotion),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_motion_backward.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EmdMotion)] + \
        [C.c_void_p] * 10
    lib.emd_motion_det_workspace_size.argtypes = [C.c_int32]
    lib.emd_motion_det_workspace_size.restype = C.c_size_t
    lib.emd_motion_det_workspace_offsets.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]
    lib.emd_motion_backward_det.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EmdMotion)] + \
        [C.c_void_p] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_sh_forward.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_sh_backward.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    lib.emd_activations_forward.argtypes = [C.c_int32] + [C.c_void_p] * 7
    lib.emd_actor_pose_forward.argtypes = [C.c_int32] + [C.c_void_p] * 8
    lib.emd_actor_pose_backward.argtypes = [C.c_int32] + [C.c_void_p] * 10
    lib.emd_l1_loss.argtypes = [C.c_int64] + [C.c_void_p] * 5
    lib.emd_l1_loss_ws.argtypes = [C.c_int64] + [C.c_void_p] * 6
    lib.emd_profile_enable.argtypes = [C.c_int]
    lib.emd_image_loss_workspace.argtypes = [C.c_int, C.c_int]
    lib.emd_image_loss_workspace.restype = C.c_size_t
    lib.emd_image_loss.argtypes = [C.POINTER(EmdLossArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_sh_grad_from_factors.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(EmdMotion), C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    lib.emd_densification_stats.argtypes = [C.c_int32] + [C.c_void_p] * 6
    lib.emd_compact_rows.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    lib.emd_scatter_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_float,
                                     C.c_void_p, C.c_void_p]
    lib.emd_hexplane_forward.argtypes = [C.POINTER(EmdHexArgs), C.c_void_p]
    lib.emd_hexplane_backward.argtypes = [C.POINTER(EmdHexArgs), C.POINTER(EmdHexGrads), C.c_void_p]
    lib.emd_hexplane_det_workspace_size.argtypes = [C.POINTER(EmdHexArgs), C.POINTER(C.c_size_t)]
    lib.emd_hexplane_det_workspace_offsets.argtypes = [C.POINTER(EmdHexArgs), C.c_int32, C.POINTER(C.c_size_t)]
    lib.emd_hexplane_order_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.emd_temporal_embed_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_temporal_embed_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.emd_deform_input_width.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.emd_deform_input_forward.argtypes = [C.POINTER(EmdDeformInArgs), C.c_void_p]
    lib.emd_deform_input_backward.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_adam_step.argtypes = [C.POINTER(EmdAdamArgs), C.c_void_p]
    lib.emd_densify_decide.argtypes = [C.POINTER(EmdDensifyArgs), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_densify_index.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_densify_scan.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_densify_split_rank.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.emd_densify_gather.argtypes = [C.POINTER(EmdDensifyGather), C.c_void_p]
    lib.emd_refine_decide.argtypes = [C.POINTER(EmdRefineArgs), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_refine_nodes_decide.argtypes = [C.POINTER(EmdRefineNodesArgs), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_refine_nodes_index_workspace.argtypes, lib.emd_refine_nodes_index_workspace.restype = [C.c_int32], C.c_size_t
    lib.emd_refine_nodes_index.argtypes = [C.POINTER(EmdRefineNodesArgs), C.c_int32] + [C.c_void_p] * 9 + [C.c_size_t, C.c_void_p]
    lib.emd_refine_index.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_after_train_stats.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    lib.emd_abs_mean_backward.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_residual_l1_backward.argtypes = [C.c_int64] + [C.c_void_p] * 9
    lib.emd_mlp_trunk_forward.argtypes = [C.POINTER(EmdMlpTrunk), C.c_void_p]
    lib.emd_mlp_trunk_backward.argtypes = [C.POINTER(EmdMlpTrunk), C.POINTER(EmdMlpTrunkGrads), C.c_void_p]
    lib.emd_mlp_branch_forward.argtypes = [C.POINTER(EmdMlpBranch), C.c_void_p]
    lib.emd_mlp_branch_backward.argtypes = [C.POINTER(EmdMlpBranch), C.POINTER(EmdMlpBranchGrads), C.c_void_p]
    lib.emd_mlp_det_slab_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(EmdMlpDetLayout)]
    lib.emd_mlp_det_slab_bytes.restype = C.c_size_t
    lib.emd_mlp_branch_forward_det.argtypes = [C.POINTER(EmdMlpBranch), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_mlp_branch_backward_det.argtypes = [C.POINTER(EmdMlpBranch), C.POINTER(EmdMlpBranchGrads), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_mlp_trunk_backward_det.argtypes = [C.POINTER(EmdMlpTrunk), C.POINTER(EmdMlpTrunkGrads), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_mlp_det_reduce.argtypes = [C.POINTER(EmdMlpDetJob), C.c_int, C.c_void_p]
    lib.emd_deform_mlp_workspace.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EmdDeformMlpLayout)]
    lib.emd_deform_mlp_forward.argtypes = [C.POINTER(EmdDeformMlpArgs), C.c_void_p]
    lib.emd_deform_mlp_backward.argtypes = [C.POINTER(EmdDeformMlpArgs), C.POINTER(EmdDeformMlpGrads), C.c_void_p]
    lib.emd_temporal_embed_backward_det.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    lib.emd_track_heads_forward.argtypes = [C.POINTER(EmdTrackArgs), C.c_void_p]
    lib.emd_track_det_workspace_size.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.emd_track_det_workspace_size.restype = C.c_size_t
    lib.emd_track_det_workspace_offsets.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]
    lib.emd_actor_row_sum_det.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_size_t, C.c_void_p]
    lib.emd_track_heads_forward_det.argtypes = [C.POINTER(EmdTrackArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_track_heads_backward_det.argtypes = [C.POINTER(EmdTrackArgs), C.POINTER(EmdTrackGrads), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_tracked_pose_backward_det.argtypes = [C.POINTER(EmdTrackedPoseArgs), C.POINTER(EmdTrackedPoseGrads), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_track_heads_backward.argtypes = [C.POINTER(EmdTrackArgs), C.POINTER(EmdTrackGrads), C.c_void_p]
    lib.emd_select_step_inputs.argtypes = [C.POINTER(EmdStepSelect), C.c_void_p]
    lib.emd_tracked_pose_forward.argtypes = [C.POINTER(EmdTrackedPoseArgs), C.c_void_p]
    lib.emd_tracked_pose_backward.argtypes = [C.POINTER(EmdTrackedPoseArgs), C.POINTER(EmdTrackedPoseGrads), C.c_void_p]
    lib.emd_sky_forward.argtypes = [C.POINTER(EmdSkyArgs), C.c_void_p]
    lib.emd_sky_backward.argtypes = [C.POINTER(EmdSkyBwdArgs), C.c_void_p]
    lib.emd_sky_det_workspace_size.argtypes = [C.c_int64]
    lib.emd_sky_det_workspace_size.restype = C.c_size_t
    lib.emd_sky_det_workspace_offsets.argtypes = [C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]
    lib.emd_sky_backward_det.argtypes = [C.POINTER(EmdSkyBwdArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_knn_workspace.argtypes = [C.c_int32, C.c_int32]
    lib.emd_knn_workspace.restype = C.c_size_t
    lib.emd_knn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_knn_reverse_workspace.argtypes = [C.c_int32, C.c_int32]
    lib.emd_knn_reverse_workspace.restype = C.c_size_t
    lib.emd_knn_reverse.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_embed_reg_forward.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7
    lib.emd_embed_reg_backward.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 9 + [C.c_int32, C.c_void_p]
    lib.emd_knn_segments.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_neighbour_std_workspace_size.argtypes, lib.emd_neighbour_std_workspace_size.restype = [], C.c_size_t
    lib.emd_neighbour_std_forward.argtypes = [C.POINTER(EmdNeighbourStdArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_neighbour_std_backward.argtypes = [C.POINTER(EmdNeighbourStdArgs), C.c_void_p]
    lib.emd_radix_sort.argtypes = [C.POINTER(EmdRadixSortArgs), C.c_void_p]
    lib.emd_raster_binning.argtypes = [C.POINTER(EmdBinningArgs), C.c_void_p]
    lib.emd_camera_grad_workspace_size.argtypes = [C.c_int32, C.POINTER(C.c_size_t)]
    lib.emd_raster_backward_camera.argtypes = [C.POINTER(EmdBwdArgs), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_raster_det_workspace_size.argtypes = [C.POINTER(EmdDims), C.POINTER(C.c_size_t)]
    lib.emd_raster_det_layout.argtypes = [C.POINTER(EmdDims), C.c_int32, C.POINTER(C.c_size_t)]
    lib.emd_segmented_row_sum_workspace.argtypes = [C.c_int64, C.c_int32]
    lib.emd_segmented_row_sum_workspace.restype = C.c_size_t
    lib.emd_segmented_row_sum.argtypes = [C.POINTER(EmdSegSumArgs), C.c_void_p]
    lib.emd_joint_chain_forward.argtypes = [C.POINTER(EmdJointChainArgs), C.c_void_p]
    lib.emd_joint_chain_backward.argtypes = [C.POINTER(EmdJointChainArgs)] + [C.c_void_p] * 7
    lib.emd_skin_forward.argtypes = [C.POINTER(EmdSkinArgs), C.c_void_p]
    lib.emd_skin_backward.argtypes = [C.POINTER(EmdSkinArgs), C.POINTER(EmdSkinGrads), C.c_void_p]
    lib.emd_plane_reg_workspace_size.argtypes = [C.POINTER(EmdPlaneRegArgs)]
    lib.emd_plane_reg_workspace_size.restype = C.c_size_t
    lib.emd_plane_reg_forward.argtypes = [C.POINTER(EmdPlaneRegArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_plane_reg_backward.argtypes = [C.POINTER(EmdPlaneRegArgs), C.c_void_p]
    lib.emd_affine_workspace_size.argtypes = [C.c_int64]
    lib.emd_affine_workspace_size.restype = C.c_size_t
    lib.emd_affine_forward.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emd_affine_backward.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]
    lib.emd_trainer_loss_workspace_size.argtypes = [C.POINTER(EmdTrainerLossArgs)]
    lib.emd_trainer_loss_workspace_size.restype = C.c_size_t
    lib.emd_trainer_loss.argtypes = [C.POINTER(EmdTrainerLossArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_vanilla_forward.argtypes = [C.POINTER(EmdVanillaArgs), C.c_void_p]
    lib.emd_vanilla_backward.argtypes = [C.POINTER(EmdVanillaArgs), C.c_void_p]
    lib.emd_vanilla_reg_workspace_size.argtypes = [C.c_int32]
    lib.emd_vanilla_reg_workspace_size.restype = C.c_size_t
    lib.emd_vanilla_reg_forward.argtypes = [C.POINTER(EmdVanillaRegArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_vanilla_reg_backward.argtypes = [C.POINTER(EmdVanillaRegArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.emd_profile_read.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    lib.emd_profile_stage_name.argtypes = [C.c_int]
    lib.emd_profile_stage_name.restype = C.c_char_p
    _lib = lib
    return lib


def profile_enable(on=True):
    load().emd_profile_enable(1 if on else 0)


def profile_read():
    """{stage name: (total ms, launches)} since the last read (HIP events on the launch stream)."""
    lib = load()
    ms = (C.c_double * PROF_STAGES)()
    cnt = (C.c_int64 * PROF_STAGES)()
    lib.emd_profile_read(ms, cnt, PROF_STAGES)
    return {lib.emd_profile_stage_name(i).decode(): (ms[i], cnt[i]) for i in range(PROF_STAGES)}


def check(rc, what):
    if rc != 0:
        msg = load().emd_last_error().decode("utf-8", "replace")
        raise EmdError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    """The current torch stream as the `hipStream_t` argument of an entry point, read at call time (under graph capture: the capturing stream)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(name, *args, what=None):
    """Call entry point `name`, one of those whose last parameter is the stream, on the current stream and check its return code."""
    check(getattr(load(), name)(*args, stream()), what or name)


def need_device(what, *tensors):
    """Refuse what is not a tensor on a ROCm device (None entries are skipped)."""
    if any(t is not None and not (isinstance(t, torch.Tensor) and t.device.type == "cuda") for t in tensors):
        raise EmdError(f"{what} needs tensors on a ROCm device; there is no CPU path")


def workspace_sizes(N, H, W, capacity, flags=0, num_extra=0):
    d = EmdDims(int(N), int(H), int(W), int(capacity), int(flags), int(num_extra))
    out = (C.c_size_t * 4)()
    check(load().emd_raster_workspace_size(C.byref(d), out), "emd_raster_workspace_size")
    return tuple(int(x) for x in out)


def camera_grad_workspace_size(N):
    out = C.c_size_t()
    check(load().emd_camera_grad_workspace_size(int(N), C.byref(out)), "emd_camera_grad_workspace_size")
    return int(out.value)


def det_workspace_size(N, capacity, num_extra=0):
    """Bytes of EmdBwdArgs.det_ws, the workspace of the deterministic backward (emd_raster_det_workspace_size)."""
    d = EmdDims(int(N), 1, 1, int(capacity), 0, int(num_extra))
    out = C.c_size_t()
    check(load().emd_raster_det_workspace_size(C.byref(d), C.byref(out)), "emd_raster_det_workspace_size")
    return int(out.value)


def det_layout(N, capacity, num_extra=0, num_actors=0):
    """Byte offsets inside det_ws and the result pairs of its two sorts (emd_raster_det_layout): a dict."""
    d = EmdDims(int(N), 1, 1, int(capacity), 0, int(num_extra))
    out = (C.c_size_t * 15)()
    check(load().emd_raster_det_layout(C.byref(d), int(num_actors), out), "emd_raster_det_layout")
    o = [int(x) for x in out]
    return dict(rows=o[0], keys=(o[1], o[2]), slots=(o[3], o[4]), counts=o[5], pose_rows=o[6], pose_keys=(o[7], o[8]), pose_points=(o[9], o[10]),
                sorted_buf=o[11], pose_sorted_buf=o[12], raw_keys=o[13], pose_raw_keys=o[14])


def hex_det_workspace_size(args):
    """Bytes of EmdHexGrads.det_ws for the call described by `args` (an EmdHexArgs: num_points and channels count)."""
    out = C.c_size_t()
    check(load().emd_hexplane_det_workspace_size(C.byref(args), C.byref(out)), "emd_hexplane_det_workspace_size")
    return int(out.value)


def hex_det_layout(args, plane):
    """Byte offsets inside EmdHexGrads.det_ws for plane `plane` = 1 + 6 s + p (emd_hexplane_det_workspace_offsets): a dict."""
    out = (C.c_size_t * 8)()
    check(load().emd_hexplane_det_workspace_offsets(C.byref(args), int(plane), out), "emd_hexplane_det_workspace_offsets")
    o = [int(x) for x in out]
    return dict(rows=o[0], keys=o[1], slots=o[2], time_column=o[3], raw_keys=o[4], counts=o[5], passes=o[6], bytes=o[7])


def _det_offsets(o):
    return dict(rows=o[0], raw_keys=o[1], keys=o[2], slots=o[3], counts=o[4], bytes=o[5])


def det_reduction_views(ws, offsets, n, pitch):
    """Typed views of one deterministic reduction inside the uint8 workspace tensor `ws`: rows float32 [n, pitch]; keys, slots, raw_keys int32 [n]
    (views of uint32); counts int32 [16].  `offsets`: the byte offset of each, under these names."""
    i32 = lambda off, cnt: ws[off:off + 4 * cnt].view(torch.int32)
    return dict(rows=ws[offsets["rows"]:offsets["rows"] + 4 * n * pitch].view(torch.float32).view(n, pitch), keys=i32(offsets["keys"], n),
                slots=i32(offsets["slots"], n), raw_keys=i32(offsets["raw_keys"], n), counts=i32(offsets["counts"], 16))


def _served(nbytes, what):
    """A size entry reports 0 bytes for sizes its mode does not serve."""
    if nbytes == 0:
        raise EmdError(f"the deterministic {what}")
    return int(nbytes)


def sky_det_workspace_size(num_pixels):
    """Bytes of the workspace of emd_sky_backward_det for a call of `num_pixels` pixels (or directions)."""
    return _served(load().emd_sky_det_workspace_size(int(num_pixels)), f"sky backward does not serve {num_pixels} pixels (4 P slots are numbered in 32 bits)")


def sky_det_layout(num_pixels, resolution):
    """Byte offsets inside that workspace (emd_sky_det_workspace_offsets): a dict."""
    out = (C.c_size_t * 6)()
    check(load().emd_sky_det_workspace_offsets(int(num_pixels), int(resolution), out), "emd_sky_det_workspace_offsets")
    return _det_offsets([int(x) for x in out])


def motion_det_workspace_size(n):
    """Bytes of the workspace of emd_motion_backward_det for `n` points."""
    return _served(load().emd_motion_det_workspace_size(int(n)), f"motion backward does not serve {n} points")


def motion_det_layout(n, num_actors):
    """Byte offsets inside that workspace (emd_motion_det_workspace_offsets): a dict."""
    out = (C.c_size_t * 6)()
    check(load().emd_motion_det_workspace_offsets(int(n), int(num_actors), out), "emd_motion_det_workspace_offsets")
    return _det_offsets([int(x) for x in out])

def track_det_workspace_size(num_actors, head_width=0, num_points=0, row_width=0):
    """Bytes of the workspace of the deterministic actor chain (emd_track_det_workspace_size): (A, dim + E, 0, 0) for the chain's backward,
    (A, 0, n, width) for emd_actor_row_sum_det."""
    return _served(load().emd_track_det_workspace_size(int(num_actors), int(head_width), int(num_points), int(row_width)),
                   f"actor chain does not serve {num_actors} actors, width {head_width}, {num_points} points, rows of {row_width}")


def track_det_layout(num_actors, head_width=0, num_points=0, row_width=0):
    """Offsets inside that workspace (emd_track_det_workspace_offsets): a dict; `pitch` is the slab's row pitch in floats, the rest are bytes."""
    out = (C.c_size_t * 8)()
    check(load().emd_track_det_workspace_offsets(int(num_actors), int(head_width), int(num_points), int(row_width), out), "emd_track_det_workspace_offsets")
    o = [int(x) for x in out]
    return dict(slab=o[0], pitch=o[1], dh=o[2], raw_keys=o[3], keys=o[4], slots=o[5], counts=o[6], bytes=o[7])


def actor_row_sum_det(rows, width, ids, num_actors, segment_start=None, col0=0):
    """[num_actors, width]: per actor the pinned segmented sum of rows[i, col0 : col0 + width] over the points with ids[i] == a, in ascending i
    (emd_actor_row_sum_det).  rows: contiguous fp32 [n, pitch]; ids: int32 [n]; segment_start: int32 [A + 1] when the ids are sorted by actor."""
    n, pitch = rows.shape
    out = torch.empty(int(num_actors), int(width), device=rows.device, dtype=torch.float32)
    if n == 0 or num_actors == 0 or width == 0:
        return out.zero_()
    ws = torch.empty(track_det_workspace_size(num_actors, 0, n, width), device=rows.device, dtype=torch.uint8)
    launch("emd_actor_row_sum_det", n, int(width), rows.data_ptr() + 4 * int(col0), pitch, ptr(ids), int(num_actors), ptr(segment_start), out.data_ptr(),
           int(width), ws.data_ptr(), ws.numel())
    return out


def mlp_det_layout(kind, args, grads=None):
    """The slab of one deterministic MLP call (emd_mlp_det_slab_bytes): dict(groups, pitch, offset, bytes); `args` / `grads` are the call's structs."""
    out = EmdMlpDetLayout()
    n = int(load().emd_mlp_det_slab_bytes(int(kind), C.byref(args), None if grads is None else C.byref(grads), C.byref(out)))
    k = out.num_tensors
    return dict(groups=int(out.groups), pitch=[int(x) for x in out.pitch[:k]], offset=[int(x) for x in out.offset[:k]], bytes=n)


def deform_mlp_layout(num_points, width, in_dim, num_cus):
    """The slab of emd_deform_mlp_backward (emd_deform_mlp_workspace, host only): dict(groups, group_rows, pitch_w, pitch_b, offset_w, offset_b, bytes)."""
    out = EmdDeformMlpLayout()
    check(load().emd_deform_mlp_workspace(int(num_points), int(width), int(in_dim), int(num_cus), C.byref(out)), "emd_deform_mlp_workspace")
    return {f: int(getattr(out, f)) for f, _ in EmdDeformMlpLayout._fields_}
