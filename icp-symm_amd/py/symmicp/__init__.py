"""symmicp -- ctypes bindings of libsymmicp.so (include/symmicp.h), the MI355X
symmetric-ICP engine, plus `MyICP`, a Python mirror of the reference's class
surface (reference ICP/myicp.h:7-36: LoadCloud / GetSrcCloud / GetTgtCloud /
RegisterSymm) with the additive setInputSource / setInputTarget / align names.

The library is HIP-only: there is no CPU fallback here, and loading fails
loudly when icp-symm_amd/lib/libsymmicp.so has not been built
(`make -C icp-symm_amd`, or __graft_entry__.build()).
"""
import ctypes as C
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_PKG))           # icp-symm_amd/
LIB_PATH = os.environ.get("SYMMICP_LIB") or os.path.join(_ROOT, "lib", "libsymmicp.so")      # SYMMICP_LIB: A/B builds in scratch runs

NSUM = 40
UNIQUE_ID_BYTES = 128
OK, ERR_ARG, ERR_SIZE, ERR_DEGENERATE, ERR_IO, ERR_HIP, ERR_STATE, ERR_COMM = range(8)
ERR_NO_CONSENSUS = 8
ERR_INTERNAL = 9
ORIENT_VIEWPOINT, ORIENT_DIRECTION = 0, 1
RANSAC_EVALUATED, RANSAC_REPEATED, RANSAC_EDGE, RANSAC_DEGENERATE, RANSAC_FAR = range(5)      # per-hypothesis status of ransac()
PLANE_EVALUATED, PLANE_REPEATED, PLANE_DEGENERATE, PLANE_OFF_AXIS = range(4)                  # ... of segment_plane()
MODE_QUIRKS, MODE_PAPER, MODE_P2P, MODE_PLANE, MODE_GICP, MODE_COLOR, MODE_NDT = 0, 1, 2, 3, 5, 7, 9      # (4, 6 and 8 are unassigned)
CORR_IDENTITY, CORR_BRUTE, CORR_TREE = 0, 1, 2
APPLY_DEFAULT, APPLY_INCREMENTAL, APPLY_CUMULATIVE = 0, 1, 2
LOSS_NONE, LOSS_HUBER, LOSS_TUKEY, LOSS_CAUCHY, LOSS_GEMAN_MCCLURE = range(5)
_LOSS_NAMES = {"none": LOSS_NONE, "huber": LOSS_HUBER, "tukey": LOSS_TUKEY, "cauchy": LOSS_CAUCHY,
               "geman_mcclure": LOSS_GEMAN_MCCLURE}

_STATUS_NAMES = {0: "OK", 1: "ERR_ARG", 2: "ERR_SIZE", 3: "ERR_DEGENERATE", 4: "ERR_IO", 5: "ERR_HIP",
                 6: "ERR_STATE", 7: "ERR_COMM", 8: "ERR_NO_CONSENSUS", 9: "ERR_INTERNAL"}


class SymmIcpError(RuntimeError):
    def __init__(self, status, msg=""):
        self.status = status
        super().__init__("symmicp: %s (%d) %s" % (_STATUS_NAMES.get(status, "?"), status, msg))


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("mode", C.c_int32), ("corr", C.c_int32),
                ("apply", C.c_int32), ("max_iters", C.c_int32), ("diff_threshold", C.c_float),
                ("max_corr_dist", C.c_float), ("fixed_iters", C.c_int32), ("sort_source", C.c_int32),
                ("verbose", C.c_int32), ("min_normal_dot", C.c_float), ("eps_rotation", C.c_float),
                ("eps_translation", C.c_float), ("host_loop", C.c_int32), ("reserved", C.c_int32 * 1)]


class Sums(C.Structure):
    _fields_ = [("s", C.c_double * NSUM)]


class IterResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iter", C.c_int32), ("diff", C.c_float), ("rcond", C.c_float),
                ("pairs", C.c_double), ("increment", C.c_float * 16), ("sums", Sums)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("iters", C.c_int32), ("diff_initial", C.c_float), ("diff_final", C.c_float),
                ("transform", C.c_float * 16), ("diffs", C.c_float * 64), ("seconds_total", C.c_double)]


class LoopLogEntry(C.Structure):
    _fields_ = [("sums", C.c_double * NSUM), ("increment", C.c_float * 16), ("X", C.c_float * 16), ("rcond", C.c_float),
                ("iter", C.c_int32), ("status", C.c_int32), ("solved", C.c_int32), ("list_len", C.c_int32), ("reason", C.c_int32),
                ("batch", C.c_int32), ("reserved", C.c_int32)]


# stop reasons of a device-driven run (symmicp_ctx_loop_solve state_out[1], LoopLogEntry.reason)
LOOP_RUNNING, LOOP_DONE, LOOP_REDO_PASS, LOOP_HOST_SOLVE, LOOP_SLOW = 0, 1, 2, 3, 4


class Stats(C.Structure):
    _fields_ = [("last_pass_ms", C.c_double), ("sum_pass_ms", C.c_double), ("passes", C.c_int64),
                ("build_ms", C.c_double), ("upload_ms", C.c_double), ("grid_level", C.c_int32),
                ("tree_levels", C.c_int32), ("pass_blocks", C.c_int64), ("bytes_algorithmic_per_pass", C.c_int64),
                ("kernel_ms", C.c_double * 8), ("kernel_launches", C.c_int64 * 8), ("pass_ms_head", C.c_double * 8), ("passes_timed", C.c_int64),
                ("loop_passes", C.c_int64), ("loop_straggler_passes", C.c_int64), ("packet_fallbacks", C.c_int64),
                ("allreduce_ms", C.c_double), ("allreduce_timed", C.c_int64)]


class RansacConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("hypotheses", C.c_uint32), ("seed", C.c_uint64), ("max_dist", C.c_float),
                ("edge_ratio", C.c_float), ("refits", C.c_int32), ("reserved", C.c_int32)]


class RansacResult(C.Structure):
    _fields_ = [("best_hypothesis", C.c_int32), ("evaluated", C.c_int32), ("inliers_ransac", C.c_int32), ("inliers_final", C.c_int32),
                ("rmse_final", C.c_double), ("transform", C.c_double * 16)]


class FgrConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("decrease_every", C.c_int32), ("max_tuples", C.c_uint32),
                ("tuple_trials", C.c_uint32), ("max_dist", C.c_float), ("division_factor", C.c_float), ("tuple_scale", C.c_float),
                ("seed", C.c_uint64)]


class FgrResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("inliers", C.c_int32), ("tuples_accepted", C.c_uint32), ("set_size", C.c_uint32),
                ("mu", C.c_float), ("reserved", C.c_int32), ("weight_sum", C.c_double), ("rmse", C.c_double), ("transform", C.c_double * 16)]


class IssConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("salient_radius", C.c_float), ("non_max_radius", C.c_float), ("gamma21", C.c_float),
                ("gamma32", C.c_float), ("min_neighbors", C.c_int32), ("reserved", C.c_int32)]


class ClusterConfig(C.Structure):
    """symmicp_cluster_config"""
    _fields_ = [("struct_size", C.c_uint32), ("eps", C.c_float), ("min_points", C.c_int32), ("min_cluster_size", C.c_int32),
                ("max_cluster_size", C.c_int32), ("reserved", C.c_int32)]


class RegionConfig(C.Structure):
    """symmicp_region_config"""
    _fields_ = [("struct_size", C.c_uint32), ("eps", C.c_float), ("smoothness_cos", C.c_float), ("curvature_threshold", C.c_float),
                ("min_region_size", C.c_int32), ("max_region_size", C.c_int32)]


class OrientConfig(C.Structure):
    """symmicp_orient_config"""
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_int32), ("seed_rule", C.c_int32), ("ref", C.c_float * 3)]


class OrientResult(C.Structure):
    """symmicp_orient_result"""
    _fields_ = [("graph_edges", C.c_uint64), ("tree_edges", C.c_uint64), ("components", C.c_uint64), ("largest_component", C.c_uint64),
                ("flipped", C.c_uint64), ("rounds", C.c_int32), ("reserved", C.c_int32)]


class PlaneConfig(C.Structure):
    """symmicp_plane_config"""
    _fields_ = [("struct_size", C.c_uint32), ("hypotheses", C.c_uint32), ("seed", C.c_uint64), ("max_dist", C.c_float),
                ("min_inliers", C.c_int32), ("refits", C.c_int32), ("axis", C.c_float * 3), ("max_angle_deg", C.c_float),
                ("reserved", C.c_int32)]


class PlaneResult(C.Structure):
    _fields_ = [("best_hypothesis", C.c_int32), ("evaluated", C.c_int32), ("inliers_ransac", C.c_int32), ("inliers_final", C.c_int32),
                ("rmse_final", C.c_double), ("plane", C.c_double * 4)]


class NdtConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("resolution", C.c_float), ("min_points", C.c_int32), ("eig_ratio", C.c_float),
                ("outlier_ratio", C.c_float), ("neighbors", C.c_int32)]


class BatchProblem(C.Structure):
    """symmicp_batch_problem: the row ranges of one problem in the packed pools"""
    _fields_ = [("src_first", C.c_uint32), ("src_count", C.c_uint32), ("tgt_first", C.c_uint32), ("tgt_count", C.c_uint32)]


class BatchConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("max_iters", C.c_int32), ("fixed_iters", C.c_int32),
                ("diff_threshold", C.c_float), ("max_corr_dist", C.c_float), ("min_normal_dot", C.c_float), ("eps_rotation", C.c_float),
                ("eps_translation", C.c_float), ("reserved", C.c_int32 * 3)]


class BatchResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iters", C.c_int32), ("diff_initial", C.c_float), ("diff_final", C.c_float), ("rcond", C.c_float),
                ("pivot", C.c_float * 3), ("transform", C.c_float * 16), ("diffs", C.c_float * 64), ("pairs", C.c_double), ("sums", Sums)]


BATCH_MAX_POINTS = 4096      # SYMMICP_BATCH_MAX_POINTS


class Evaluation(C.Structure):
    """symmicp_evaluation: fitness, inlier RMSE, the inlier sums and the 6x6 information matrix of one transform"""
    _fields_ = [("inliers", C.c_uint64), ("fitness", C.c_double), ("rmse", C.c_double), ("mean_d2", C.c_double), ("sum_d2", C.c_double),
                ("sum_q", C.c_double * 3), ("sum_qq", C.c_double * 6), ("information", C.c_double * 36)]


EVAL_MAX_TRANSFORMS = 4096


class PoseEdge(C.Structure):
    """symmicp_pose_edge: T takes the source node's frame to the target node's (align with cloud s as source, cloud t as target), the
    information matrix is that pair's evaluation (rotation first), uncertain = 1 for a loop closure"""
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("uncertain", C.c_int32), ("reserved", C.c_int32),
                ("transform", C.c_double * 16), ("information", C.c_double * 36)]


class PosegraphConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_iterations", C.c_int32), ("reference_node", C.c_int32), ("cg_max_iterations", C.c_int32),
                ("max_dist", C.c_double), ("preference_loop_closure", C.c_double), ("line_process_weight", C.c_double),
                ("edge_prune_threshold", C.c_double), ("min_relative_decrease", C.c_double), ("min_increment", C.c_double),
                ("cg_tolerance", C.c_double)]


class PosegraphResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("accepted_steps", C.c_int32), ("stop_reason", C.c_int32),
                ("pruned", C.c_int32), ("cg_iterations", C.c_int32), ("cost_initial", C.c_double), ("cost_final", C.c_double),
                ("mu", C.c_double), ("lambda_final", C.c_double), ("grad_max", C.c_double)]


class PosegraphIteration(C.Structure):
    """symmicp_posegraph_iteration: the record of one Levenberg-Marquardt iteration"""
    _fields_ = [("cost", C.c_double), ("cost_trial", C.c_double), ("model_decrease", C.c_double), ("grad_max", C.c_double),
                ("delta_max", C.c_double), ("hdiag_max", C.c_double), ("lambda_", C.c_double), ("cg_residual", C.c_double),
                ("cg_iterations", C.c_int32), ("accepted", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


POSEGRAPH_MAX_NODES, POSEGRAPH_MAX_EDGES = 1024, 16384
POSEGRAPH_STOP_MAX_ITERATIONS, POSEGRAPH_STOP_DECREASE, POSEGRAPH_STOP_INCREMENT = 1, 2, 3


class IndexInfo(C.Structure):
    """symmicp_index_info: what symmicp_ctx_index_info reads back of a target index (tests)"""
    _fields_ = [("struct_size", C.c_int32), ("n", C.c_uint32), ("grid_level", C.c_int32), ("gdim", C.c_int32), ("origin", C.c_float * 3),
                ("h0", C.c_float), ("h", C.c_float), ("inv_h", C.c_float), ("tree_levels", C.c_int32), ("top", C.c_int32), ("ntop", C.c_uint32),
                ("level_off", C.c_uint32 * 12), ("n_boxes", C.c_uint32), ("olevel_off", C.c_uint32 * 12), ("n_onodes", C.c_uint32),
                ("n_blocks", C.c_uint32), ("ctop_len", C.c_uint32), ("leaf_max", C.c_uint32), ("surface_like", C.c_int32),
                ("level_hist", C.c_uint32 * 16)]


KERNEL_SLOTS = ["k_search_cells", "(gap)", "k_search_walk", "k_accumulate", "k_final_reduce", "single_pass_kernel", "whole_pass"]


# every symbol include/symmicp.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "symmicp_config_default", "symmicp_create", "symmicp_destroy", "symmicp_last_error", "symmicp_set_config",
    "symmicp_version", "symmicp_set_source", "symmicp_set_target", "symmicp_align", "symmicp_begin", "symmicp_step",
    "symmicp_get_transform", "symmicp_format_result", "symmicp_get_pivot", "symmicp_get_correspondences", "symmicp_get_source",
    "symmicp_local_source_count", "symmicp_local_source_offset", "symmicp_get_certificates", "symmicp_solve", "symmicp_comm_get_unique_id",
    "symmicp_comm_init_rank", "symmicp_set_sums", "symmicp_comm_init_shm", "symmicp_shard_range", "symmicp_get_stats", "symmicp_reset_stats", "symmicp_enable_timing",
    "symmicp_pcd_read", "symmicp_pcd_write", "symmicp_estimate_normals", "symmicp_ctx_estimate_normals", "symmicp_ctx_knn",
    "symmicp_set_robust_loss", "symmicp_get_robust_loss", "symmicp_robust_weight", "symmicp_set_gicp_epsilon", "symmicp_get_gicp_epsilon",
    "symmicp_ctx_solve_probe", "symmicp_ctx_loop_solve", "symmicp_set_loop_log", "symmicp_get_loop_log",
    "symmicp_voxel_downsample", "symmicp_ctx_voxel_downsample",
    "symmicp_radius_search", "symmicp_ctx_radius_search", "symmicp_fpfh", "symmicp_ctx_fpfh",
    "symmicp_feature_nn", "symmicp_ctx_feature_nn", "symmicp_feature_correspondences", "symmicp_ctx_feature_correspondences",
    "symmicp_ransac_config_default", "symmicp_ransac", "symmicp_ctx_ransac", "symmicp_ctx_ransac_hypotheses",
    "symmicp_fgr_config_default", "symmicp_fgr", "symmicp_ctx_fgr", "symmicp_ctx_fgr_pass",
    "symmicp_ctx_index_info", "symmicp_ctx_index_arrays", "symmicp_ctx_source_share", "symmicp_ctx_radix_sort_probe", "symmicp_ctx_scan_probe",
    "symmicp_set_trim_fraction", "symmicp_get_trim_fraction", "symmicp_get_trim_state", "symmicp_ctx_select_probe",
    "symmicp_set_one_to_one", "symmicp_get_one_to_one", "symmicp_set_median_factor", "symmicp_get_median_factor",
    "symmicp_get_rejection_state", "symmicp_ctx_unique_probe",
    "symmicp_set_reciprocal", "symmicp_get_reciprocal", "symmicp_get_reciprocal_state", "symmicp_inverse_rigid", "symmicp_ctx_reverse_nn_probe",
    "symmicp_ctx_reciprocal_info",
    "symmicp_set_color_weight", "symmicp_get_color_weight", "symmicp_set_source_intensity", "symmicp_set_target_intensity",
    "symmicp_get_source_intensity", "symmicp_intensity_gradient", "symmicp_ctx_intensity_gradient", "symmicp_pcd_read_intensity",
    "symmicp_iss_config_default", "symmicp_iss_keypoints", "symmicp_ctx_iss_keypoints",
    "symmicp_batch_config_default", "symmicp_batch_align", "symmicp_ctx_batch_align",
    "symmicp_information_from_sums", "symmicp_evaluate_registration", "symmicp_ctx_evaluate_registration", "symmicp_evaluate",
    "symmicp_statistical_outlier_removal", "symmicp_ctx_statistical_outlier_removal",
    "symmicp_radius_outlier_removal", "symmicp_ctx_radius_outlier_removal",
    "symmicp_cluster_config_default", "symmicp_cluster", "symmicp_ctx_cluster",
    "symmicp_region_config_default", "symmicp_region_growing", "symmicp_ctx_region_growing",
    "symmicp_orient_config_default", "symmicp_orient_normals", "symmicp_ctx_orient_normals",
    "symmicp_plane_config_default", "symmicp_segment_plane", "symmicp_ctx_segment_plane", "symmicp_ctx_plane_hypotheses",
    "symmicp_ndt_config_default", "symmicp_set_ndt", "symmicp_get_ndt", "symmicp_ndt_gauss", "symmicp_ndt_weight", "symmicp_get_ndt_state",
    "symmicp_ctx_ndt_map", "symmicp_ndt_map", "symmicp_get_ndt_map",
    "symmicp_posegraph_config_default", "symmicp_posegraph_optimize", "symmicp_ctx_posegraph_optimize", "symmicp_ctx_posegraph_pass",
    "symmicp_posegraph_edge_error", "symmicp_posegraph_line_weight",
]

_lib = None


def _hip_runtime_first():
    """Make sure only ONE HIP runtime ends up in the process.  torch ships its own
    libamdhip64.so (found through its RPATH under the un-versioned name); if libsymmicp were
    loaded first it would pull /opt/rocm's copy and a later `import torch` would map a second
    runtime.  Importing torch first makes our NEEDED libamdhip64.so.7 resolve to torch's copy."""
    if "torch" in sys.modules or os.environ.get("SYMMICP_NO_TORCH_PRELOAD"):
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SymmIcpError(ERR_HIP, "libsymmicp.so not built at %s (run `make -C icp-symm_amd`); no CPU fallback" % LIB_PATH)
    _hip_runtime_first()
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    fp = C.POINTER(C.c_float)
    vp = C.c_void_p
    L.symmicp_config_default.argtypes = [C.POINTER(Config)]
    L.symmicp_config_default.restype = None
    L.symmicp_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.symmicp_destroy.argtypes = [vp]
    L.symmicp_destroy.restype = None
    L.symmicp_last_error.argtypes = [vp]
    L.symmicp_last_error.restype = C.c_char_p
    L.symmicp_set_config.argtypes = [vp, C.POINTER(Config)]
    for nm in ("symmicp_set_source", "symmicp_set_target"):
        getattr(L, nm).argtypes = [vp, fp, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.c_size_t]
    L.symmicp_align.argtypes = [vp, fp, C.POINTER(Result)]
    L.symmicp_begin.argtypes = [vp, fp, C.POINTER(IterResult)]
    L.symmicp_step.argtypes = [vp, C.POINTER(IterResult)]
    L.symmicp_get_transform.argtypes = [vp, fp]
    L.symmicp_get_pivot.argtypes = [vp, fp]
    L.symmicp_format_result.argtypes = [fp, C.c_char_p, C.c_size_t]
    L.symmicp_format_result.restype = C.c_size_t
    L.symmicp_get_correspondences.argtypes = [vp, C.POINTER(C.c_int32), fp, C.c_size_t]
    L.symmicp_get_source.argtypes = [vp, fp, fp, C.c_size_t]
    L.symmicp_local_source_count.argtypes = [vp]
    L.symmicp_local_source_count.restype = C.c_size_t
    L.symmicp_local_source_offset.argtypes = [vp]
    L.symmicp_local_source_offset.restype = C.c_size_t
    L.symmicp_solve.argtypes = [C.c_int, C.POINTER(Sums), fp, fp, fp, fp, fp, fp, fp]
    L.symmicp_comm_get_unique_id.argtypes = [vp]
    L.symmicp_comm_init_rank.argtypes = [vp, C.c_int, C.c_int, vp]
    L.symmicp_set_sums.argtypes = [vp, C.POINTER(Sums)]
    L.symmicp_comm_init_shm.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.symmicp_shard_range.argtypes = [C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.symmicp_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.symmicp_reset_stats.argtypes = [vp]
    L.symmicp_enable_timing.argtypes = [vp, C.c_int]
    L.symmicp_pcd_read.argtypes = [C.c_char_p, fp, fp, C.c_size_t, C.POINTER(C.c_int)]
    L.symmicp_pcd_read.restype = C.c_long
    L.symmicp_pcd_write.argtypes = [C.c_char_p, fp, fp, C.c_size_t, C.c_int]
    L.symmicp_estimate_normals.argtypes = [C.c_int, fp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, fp, fp, fp]
    L.symmicp_ctx_estimate_normals.argtypes = [vp, fp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, fp, fp, fp]
    L.symmicp_ctx_knn.argtypes = [vp, fp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_int32), fp]
    L.symmicp_set_robust_loss.argtypes = [vp, C.c_int, C.c_float]
    L.symmicp_get_robust_loss.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.symmicp_robust_weight.argtypes = [C.c_int, C.c_float, C.c_float]
    L.symmicp_robust_weight.restype = C.c_float
    L.symmicp_set_gicp_epsilon.argtypes = [vp, C.c_float]
    L.symmicp_get_gicp_epsilon.argtypes = [vp, C.POINTER(C.c_float)]
    i32p = C.POINTER(C.c_int32)
    L.symmicp_ctx_solve_probe.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Sums), C.c_size_t, fp, fp, i32p, fp, fp, fp, fp, fp, fp, fp]
    L.symmicp_ctx_loop_solve.argtypes = [vp, C.POINTER(Sums), fp, fp, i32p, fp, i32p, fp, fp, fp, fp, fp, i32p]
    L.symmicp_set_loop_log.argtypes = [vp, C.c_int]
    L.symmicp_get_loop_log.argtypes = [vp, C.POINTER(LoopLogEntry), C.c_size_t, C.POINTER(C.c_size_t)]
    vox = [fp, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_float, C.c_int, fp, fp, i32p, i32p, C.c_size_t,
           C.POINTER(C.c_size_t)]
    L.symmicp_voxel_downsample.argtypes = [C.c_int] + vox
    L.symmicp_ctx_voxel_downsample.argtypes = [vp] + vox
    rad = [fp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_float, i32p, C.POINTER(C.c_int64), i32p, fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.symmicp_radius_search.argtypes = [C.c_int] + rad
    L.symmicp_ctx_radius_search.argtypes = [vp] + rad
    fpf = [fp, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_float, fp, fp, i32p]
    L.symmicp_fpfh.argtypes = [C.c_int] + fpf
    L.symmicp_ctx_fpfh.argtypes = [vp] + fpf
    fnn = [fp, C.c_size_t, fp, C.c_size_t, i32p, fp, fp]
    L.symmicp_feature_nn.argtypes = [C.c_int] + fnn
    L.symmicp_ctx_feature_nn.argtypes = [vp] + fnn
    fco = [fp, C.c_size_t, fp, C.c_size_t, C.c_int, C.c_float, i32p, fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.symmicp_feature_correspondences.argtypes = [C.c_int] + fco
    L.symmicp_ctx_feature_correspondences.argtypes = [vp] + fco
    u8p = C.POINTER(C.c_uint8)
    rsc = [fp, C.c_size_t, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.c_size_t, i32p, C.c_size_t, C.POINTER(RansacConfig)]
    L.symmicp_ransac_config_default.argtypes = [C.POINTER(RansacConfig)]
    L.symmicp_ransac_config_default.restype = None
    L.symmicp_ransac.argtypes = [C.c_int] + rsc + [fp, C.POINTER(RansacResult), u8p, u8p, i32p]
    L.symmicp_ctx_ransac.argtypes = [vp] + rsc + [fp, C.POINTER(RansacResult), u8p, u8p, i32p]
    L.symmicp_ctx_ransac_hypotheses.argtypes = [vp] + rsc + [fp, u8p, fp]
    fgc = rsc[:-1] + [C.POINTER(FgrConfig), fp, C.POINTER(FgrResult), i32p, fp, fp, C.POINTER(C.c_double), fp]
    L.symmicp_fgr_config_default.argtypes = [C.POINTER(FgrConfig)]
    L.symmicp_fgr_config_default.restype = None
    L.symmicp_fgr.argtypes = [C.c_int] + fgc
    L.symmicp_ctx_fgr.argtypes = [vp] + fgc
    L.symmicp_ctx_fgr_pass.argtypes = [vp, fp, fp, C.c_size_t, fp, C.c_float, C.POINTER(C.c_double), fp]
    u32p, szp = C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)
    L.symmicp_ctx_index_info.argtypes = [vp, C.POINTER(IndexInfo)]
    L.symmicp_ctx_index_arrays.argtypes = [vp, fp, fp, fp, u32p, u32p, fp]
    L.symmicp_ctx_source_share.argtypes = [vp, szp, szp, i32p, i32p, u32p, u32p]
    L.symmicp_ctx_radix_sort_probe.argtypes = [vp, u32p, u32p, C.c_size_t, C.c_int]
    L.symmicp_ctx_scan_probe.argtypes = [vp, u32p, C.c_size_t]
    u64p = C.POINTER(C.c_uint64)
    L.symmicp_set_trim_fraction.argtypes = [vp, C.c_float]
    L.symmicp_get_trim_fraction.argtypes = [vp, fp]
    L.symmicp_get_trim_state.argtypes = [vp, u64p, u64p, fp]
    L.symmicp_set_one_to_one.argtypes = [vp, C.c_int]
    L.symmicp_get_one_to_one.argtypes = [vp, C.POINTER(C.c_int)]
    L.symmicp_set_median_factor.argtypes = [vp, C.c_float]
    L.symmicp_get_median_factor.argtypes = [vp, fp]
    L.symmicp_get_rejection_state.argtypes = [vp, u64p, u64p, u64p, fp]
    L.symmicp_ctx_unique_probe.argtypes = [vp, i32p, u32p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8)]
    L.symmicp_set_reciprocal.argtypes = [vp, C.c_int]
    L.symmicp_get_reciprocal.argtypes = [vp, C.POINTER(C.c_int)]
    L.symmicp_get_reciprocal_state.argtypes = [vp, u64p, u64p]
    L.symmicp_inverse_rigid.argtypes = [fp, fp]
    L.symmicp_ctx_reciprocal_info.argtypes = [vp, i32p, u64p, u64p, u64p]
    L.symmicp_ctx_reverse_nn_probe.argtypes = [vp, fp, i32p, C.c_size_t, fp, C.c_size_t, fp, i32p, fp]
    L.symmicp_ctx_select_probe.argtypes = [vp, u32p, C.c_size_t, C.c_uint64, u32p, u64p]
    L.symmicp_set_color_weight.argtypes = [vp, C.c_float]
    L.symmicp_get_color_weight.argtypes = [vp, fp]
    L.symmicp_set_source_intensity.argtypes = [vp, fp, C.c_size_t, C.c_size_t]
    L.symmicp_set_target_intensity.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.c_size_t]
    L.symmicp_get_source_intensity.argtypes = [vp, fp, C.c_size_t]
    grd = [fp, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.c_int, fp]
    L.symmicp_intensity_gradient.argtypes = [C.c_int] + grd
    L.symmicp_ctx_intensity_gradient.argtypes = [vp] + grd
    L.symmicp_pcd_read_intensity.argtypes = [C.c_char_p, fp, C.c_size_t, C.POINTER(C.c_int)]
    L.symmicp_pcd_read_intensity.restype = C.c_long
    iss = [fp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(IssConfig), i32p, C.c_size_t, szp, fp, i32p]
    L.symmicp_iss_config_default.argtypes = [C.POINTER(IssConfig)]
    L.symmicp_iss_config_default.restype = None
    L.symmicp_iss_keypoints.argtypes = [C.c_int] + iss
    L.symmicp_ctx_iss_keypoints.argtypes = [vp] + iss
    bat = [fp, fp, C.c_size_t, fp, fp, C.c_size_t, C.POINTER(BatchProblem), fp, C.c_size_t, C.POINTER(BatchConfig), C.POINTER(BatchResult), fp,
           C.POINTER(C.c_double)]
    L.symmicp_batch_config_default.argtypes = [C.POINTER(BatchConfig)]
    L.symmicp_batch_config_default.restype = None
    L.symmicp_batch_align.argtypes = [C.c_int] + bat
    L.symmicp_ctx_batch_align.argtypes = [vp] + bat
    dp, evp = C.POINTER(C.c_double), C.POINTER(Evaluation)
    L.symmicp_information_from_sums.argtypes = [C.c_uint64, dp, dp, dp]
    evl = [fp, C.c_size_t, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_float, evp, i32p, fp]
    L.symmicp_evaluate_registration.argtypes = [C.c_int] + evl
    L.symmicp_ctx_evaluate_registration.argtypes = [vp] + evl
    L.symmicp_evaluate.argtypes = [vp, fp, C.c_size_t, C.c_float, evp, i32p, fp]
    sor = [fp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_float, i32p, C.c_size_t, szp, dp, dp]
    L.symmicp_statistical_outlier_removal.argtypes = [C.c_int] + sor
    L.symmicp_ctx_statistical_outlier_removal.argtypes = [vp] + sor
    ror = [fp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_float, C.c_int, i32p, C.c_size_t, szp, i32p]
    L.symmicp_radius_outlier_removal.argtypes = [C.c_int] + ror
    L.symmicp_ctx_radius_outlier_removal.argtypes = [vp] + ror
    clu = [fp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(ClusterConfig), i32p, szp, i32p, C.c_size_t, u8p, i32p]
    L.symmicp_cluster_config_default.argtypes = [C.POINTER(ClusterConfig)]
    L.symmicp_cluster_config_default.restype = None
    L.symmicp_cluster.argtypes = [C.c_int] + clu
    L.symmicp_ctx_cluster.argtypes = [vp] + clu
    reg = [fp, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.POINTER(RegionConfig), i32p, szp, i32p,
           C.c_size_t, u8p, i32p]
    L.symmicp_region_config_default.argtypes = [C.POINTER(RegionConfig)]
    L.symmicp_region_config_default.restype = None
    L.symmicp_region_growing.argtypes = [C.c_int] + reg
    L.symmicp_ctx_region_growing.argtypes = [vp] + reg
    ori = [fp, C.c_size_t, C.c_size_t, fp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(OrientConfig), fp, u8p, i32p, i32p, szp,
           C.POINTER(OrientResult)]
    L.symmicp_orient_config_default.argtypes = [C.POINTER(OrientConfig)]
    L.symmicp_orient_config_default.restype = None
    L.symmicp_orient_normals.argtypes = [C.c_int] + ori
    L.symmicp_ctx_orient_normals.argtypes = [vp] + ori
    plc = [fp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(PlaneConfig)]
    L.symmicp_plane_config_default.argtypes = [C.POINTER(PlaneConfig)]
    L.symmicp_plane_config_default.restype = None
    L.symmicp_segment_plane.argtypes = [C.c_int] + plc + [fp, C.POINTER(PlaneResult), i32p, C.c_size_t, szp, dp, u8p, i32p]
    L.symmicp_ctx_segment_plane.argtypes = [vp] + plc + [fp, C.POINTER(PlaneResult), i32p, C.c_size_t, szp, dp, u8p, i32p]
    L.symmicp_ctx_plane_hypotheses.argtypes = [vp] + plc + [fp, u8p, fp]
    ndp = C.POINTER(NdtConfig)
    L.symmicp_ndt_config_default.argtypes = [ndp]
    L.symmicp_ndt_config_default.restype = None
    L.symmicp_set_ndt.argtypes = [vp, ndp]
    L.symmicp_get_ndt.argtypes = [vp, ndp]
    L.symmicp_ndt_gauss.argtypes = [C.c_double, dp, dp]
    L.symmicp_ndt_weight.argtypes = [C.c_float]
    L.symmicp_ndt_weight.restype = C.c_float
    L.symmicp_get_ndt_state.argtypes = [vp, dp, u64p]
    nmo = [u32p, i32p, fp, dp, fp, fp, i32p, C.c_size_t, szp]
    nmi = [fp, C.c_size_t, C.c_size_t, C.c_size_t, ndp]
    L.symmicp_ndt_map.argtypes = [C.c_int] + nmi + nmo
    L.symmicp_ctx_ndt_map.argtypes = [vp] + nmi + nmo
    L.symmicp_get_ndt_map.argtypes = [vp] + nmo
    pgc, pge, pgi = C.POINTER(PosegraphConfig), C.POINTER(PoseEdge), C.POINTER(PosegraphIteration)
    pgo = [dp, C.c_size_t, pge, C.c_size_t, pgc, dp, C.POINTER(PosegraphResult), dp, C.POINTER(C.c_uint8), pgi]
    L.symmicp_posegraph_config_default.argtypes = [pgc]
    L.symmicp_posegraph_config_default.restype = None
    L.symmicp_posegraph_optimize.argtypes = [C.c_int] + pgo
    L.symmicp_ctx_posegraph_optimize.argtypes = [vp] + pgo
    L.symmicp_ctx_posegraph_pass.argtypes = [vp, dp, C.c_size_t, pge, C.c_size_t, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32,
                                             dp, dp, dp, dp, dp, dp, pgi]
    L.symmicp_posegraph_edge_error.argtypes = [dp, dp, dp, dp]
    L.symmicp_posegraph_line_weight.argtypes = [C.c_double, C.c_double]
    L.symmicp_posegraph_line_weight.restype = C.c_double
    _lib = L
    return L


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _cloud(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("cloud must be [N,3]")
    return a


def default_config(**kw):
    cfg = Config()
    lib().symmicp_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def pcd_read(path):
    """PCD v0.7 (ascii/binary) -> (xyz [N,3] f32, normals [N,3] f32 or None). myicp.cpp:20-31."""
    L = lib()
    hn = C.c_int(0)
    n = L.symmicp_pcd_read(os.fsencode(path), None, None, 0, C.byref(hn))
    if n < 0:
        raise SymmIcpError(-n, "pcd_read(%s)" % path)
    xyz = np.zeros((n, 3), np.float32)
    nrm = np.zeros((n, 3), np.float32)
    r = L.symmicp_pcd_read(os.fsencode(path), _fptr(xyz), _fptr(nrm), n, C.byref(hn))
    if r != n:
        raise SymmIcpError(-r if r < 0 else ERR_IO, "pcd_read(%s)" % path)
    return xyz, (nrm if hn.value else None)


def pcd_read_intensity(path):
    """one scalar per point of a PCD file -> (intensity [N] f32 or None, kind): kind 1 = an `intensity` field, 2 = PCL's packed
    `rgb` / `rgba` turned into (r + g + b) / 765, 0 = the file has neither (None)"""
    L = lib()
    kind = C.c_int(0)
    n = L.symmicp_pcd_read_intensity(os.fsencode(path), None, 0, C.byref(kind))
    if n < 0:
        raise SymmIcpError(-n, "pcd_read_intensity(%s)" % path)
    if kind.value == 0:
        return None, 0
    out = np.zeros(n, np.float32)
    r = L.symmicp_pcd_read_intensity(os.fsencode(path), _fptr(out), n, C.byref(kind))
    if r != n:
        raise SymmIcpError(-r if r < 0 else ERR_IO, "pcd_read_intensity(%s)" % path)
    return out, kind.value


def pcd_write(path, xyz, nrm=None, binary=False):
    xyz = _cloud(xyz)
    nrm_p = None
    if nrm is not None:
        nrm = _cloud(nrm)
        nrm_p = _fptr(nrm)
    st = lib().symmicp_pcd_write(os.fsencode(path), _fptr(xyz), nrm_p, xyz.shape[0], int(binary))
    if st != OK:
        raise SymmIcpError(st, "pcd_write(%s)" % path)


def solve(mode, sums, pivot=None):
    """Host part of estimateTransformSymm (func.cpp:76-102) on one reduction record."""
    S = Sums()
    for k, v in enumerate(np.asarray(sums, np.float64).reshape(NSUM)):
        S.s[k] = v
    pb = np.zeros(3, np.float32); qb = np.zeros(3, np.float32); a = np.zeros(3, np.float32); t = np.zeros(3, np.float32)
    X = np.zeros(16, np.float32)
    rc = C.c_float(0)
    pv = None
    if pivot is not None:
        pivot = np.ascontiguousarray(pivot, np.float32)
        pv = _fptr(pivot)
    st = lib().symmicp_solve(mode, C.byref(S), pv, _fptr(pb), _fptr(qb), _fptr(a), _fptr(t), C.byref(rc), _fptr(X))
    return st, pb, qb, a, t, rc.value, X.reshape(4, 4)


def loss_code(loss):
    """a LOSS_* value from the enum or its name ("none", "huber", "tukey", "cauchy", "geman_mcclure"); unknown names raise
    ValueError, unknown integers pass through (the library refuses them)"""
    if isinstance(loss, str):
        try:
            return _LOSS_NAMES[loss.lower()]
        except KeyError:
            raise ValueError("unknown robust loss %r (one of %s)" % (loss, ", ".join(_LOSS_NAMES)))
    return int(loss)


def robust_weight(loss, scale, r):
    """the weight the pass kernels give a pair of residual r (symmicp_robust_weight; NaN on bad arguments).  r may be an
    array: the result is float32 of the same shape."""
    f = lib().symmicp_robust_weight
    code = loss_code(loss)
    ra = np.asarray(r, np.float32)
    out = np.array([f(code, float(scale), float(x)) for x in ra.reshape(-1)], np.float32).reshape(ra.shape)
    return out if ra.ndim else float(out)


def inverse_rigid(transform):
    """the 3x4 inverse a reciprocal pass carries the target through (symmicp_inverse_rigid): the rotation block transposed and
    -R^T t, formed in fp64 and rounded to fp32 -> (3, 4) float32; needs no GPU"""
    X = np.ascontiguousarray(np.asarray(transform, np.float32).reshape(16))
    out = np.zeros(12, np.float32)
    st = lib().symmicp_inverse_rigid(_fptr(X), _fptr(out))
    if st != 0:
        raise SymmIcpError(st, "symmicp_inverse_rigid")
    return out.reshape(3, 4)


def format_result(transform):
    """The reference's result block for a 4x4 (myicp.cpp:146-149, Eigen's default IOFormat); needs no GPU."""
    X = np.ascontiguousarray(np.asarray(transform, np.float32).reshape(16))
    n = lib().symmicp_format_result(_fptr(X), None, 0)
    buf = C.create_string_buffer(n + 1)
    lib().symmicp_format_result(_fptr(X), buf, n + 1)
    return buf.value.decode()


def estimate_normals(xyz, k=10, viewpoint=(0.0, 0.0, 0.0), device=-1):
    """k-NN PCA normals on the GPU (MyICP::estimateNormals, myicp.cpp:152-172). -> (normals, curvature)"""
    xyz = _cloud(xyz)
    n = xyz.shape[0]
    nrm = np.zeros((n, 3), np.float32)
    curv = np.zeros(n, np.float32)
    vp = np.ascontiguousarray(viewpoint, np.float32)
    st = lib().symmicp_estimate_normals(device, _fptr(xyz), 3, 1, n, k, _fptr(vp), _fptr(nrm), _fptr(curv))
    if st != OK:
        raise SymmIcpError(st, "estimate_normals")
    return nrm, curv


def _scalar(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if n is not None and a.shape[0] != n:
        raise ValueError("one value per point expected")
    return a


def intensity_gradient(xyz, nrm, intensity, k=10, device=-1):
    """the intensity's gradient on every point's tangent plane (symmicp_intensity_gradient: the k-NN set of knn() without the point
    itself, a least-squares fit in fp64) -> [N,3] f32, exactly 0 where the neighbourhood is degenerate"""
    xyz, nrm = _cloud(xyz), _cloud(nrm)
    n = xyz.shape[0]
    it = _scalar(intensity, n)
    g = np.zeros((n, 3), np.float32)
    st = lib().symmicp_intensity_gradient(device, _fptr(xyz), 3, 1, _fptr(nrm), 3, 1, _fptr(it), 1, n, k, _fptr(g))
    if st != OK:
        raise SymmIcpError(st, "intensity_gradient")
    return g


def knn(xyz, k=10, device=-1):
    """the k nearest points of the same cloud, the set estimate_normals uses -> (rows [N,k] int32, d2 [N,k] f32), ascending (d2, row)"""
    with Engine(device=device) as e:
        return e.knn(xyz, k)


def _voxel_call(fn, head, xyz, nrm, leaf, min_points, cap=None, strides=None):
    """shared body of voxel_downsample and Engine.voxel_downsample: fn(*head, <the C arguments>) -> (status, result dict or None,
    n_out).  strides = (n, xyz row, xyz col, nrm row, nrm col) reads xyz / nrm as flat f32 buffers (tests of the strided layouts)."""
    if strides is None:
        xyz = _cloud(xyz)
        nrm = None if nrm is None else _cloud(nrm)
        n, xr, xc, nr, nc = xyz.shape[0], 3, 1, 3, 1
    else:
        xyz = np.ascontiguousarray(xyz, np.float32)
        nrm = None if nrm is None else np.ascontiguousarray(nrm, np.float32)
        n, xr, xc, nr, nc = strides
    cap = n if cap is None else cap
    out = np.zeros((max(cap, 1), 3), np.float32)
    nout = None if nrm is None else np.zeros((max(cap, 1), 3), np.float32)
    cnt = np.zeros(max(cap, 1), np.int32)
    vof = np.zeros(max(n, 1), np.int32)
    m = C.c_size_t(0)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    st = fn(*head, _fptr(xyz), xr, xc, None if nrm is None else _fptr(nrm), nr, nc, n, float(leaf), int(min_points), _fptr(out),
            None if nout is None else _fptr(nout), i32(cnt), i32(vof), cap, C.byref(m))
    m = int(m.value)
    if st != OK:
        return st, None, m
    return st, dict(xyz=out[:m].copy(), nrm=None if nout is None else nout[:m].copy(), count=cnt[:m].copy(), voxel_of=vof[:n].copy()), m


def voxel_downsample(xyz, leaf, nrm=None, min_points=1, device=-1):
    """voxel-grid downsampling on the GPU (symmicp_voxel_downsample): one point per occupied voxel of edge `leaf` with at least
    min_points points, in ascending voxel key -> dict(xyz [m,3], nrm [m,3] or None, count [m], voxel_of [N] (-1: dropped))"""
    st, r, _ = _voxel_call(lib().symmicp_voxel_downsample, (int(device),), xyz, nrm, leaf, min_points)
    if st != OK:
        raise SymmIcpError(st, "voxel_downsample")
    return r


def _i32ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def ndt_config(resolution=1.0, min_points=6, eig_ratio=0.01, outlier_ratio=0.55, neighbors=7):
    """a symmicp_ndt_config (the defaults are PCL's)"""
    cfg = NdtConfig()
    lib().symmicp_ndt_config_default(C.byref(cfg))
    cfg.resolution, cfg.min_points, cfg.eig_ratio = float(resolution), int(min_points), float(eig_ratio)
    cfg.outlier_ratio, cfg.neighbors = float(outlier_ratio), int(neighbors)
    return cfg


def ndt_weight(x):
    """symmicp_ndt_weight: the NDT pass's plain-arithmetic exp(x) on (-64, 0] in fp32 (0 at and below -64 and for NaN) -> np.float32"""
    return np.float32(lib().symmicp_ndt_weight(C.c_float(float(np.float32(x)))))


def ndt_gauss(outlier_ratio=0.55):
    """symmicp_ndt_gauss: the Gauss constants (d1, d2) of an outlier ratio in (0, 1), fp64"""
    d1, d2 = C.c_double(0), C.c_double(0)
    st = lib().symmicp_ndt_gauss(C.c_double(float(outlier_ratio)), C.byref(d1), C.byref(d2))
    if st != OK:
        raise SymmIcpError(st, "ndt_gauss: the outlier ratio must lie in (0, 1)")
    return d1.value, d2.value


def _ndt_map_call(fn, head, cap, want=True):
    """shared tail of the three map entries: fn(*head, <the outputs>) -> (status, map dict or None, m)"""
    c1 = max(int(cap), 1)
    key, cnt = np.zeros(c1, np.uint32), np.zeros(c1, np.int32)
    mean, cov = np.zeros((c1, 3), np.float32), np.zeros((c1, 6), np.float64)
    axes, inv_eig = np.zeros((c1, 3, 3), np.float32), np.zeros((c1, 3), np.float32)
    grid = np.zeros(6, np.int32)
    m = C.c_size_t(0)
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    if want:
        st = fn(*head, key.ctypes.data_as(C.POINTER(C.c_uint32)), _i32ptr(cnt), _fptr(mean), dptr(cov), _fptr(axes), _fptr(inv_eig), _i32ptr(grid),
                int(cap), C.byref(m))
    else:
        st = fn(*head, None, None, None, None, None, None, None, int(cap), C.byref(m))
    m = int(m.value)
    if st != OK:
        return st, None, m
    return st, dict(key=key[:m].copy(), count=cnt[:m].copy(), mean=mean[:m].copy(), cov=cov[:m].copy(), axes=axes[:m].copy(),
                    inv_eig=inv_eig[:m].copy(), grid=grid.copy()), m


def _ndt_map(fn, head, xyz, cfg, cap=None, strides=None, want=True):
    if strides is None:
        xyz = _cloud(xyz)
        n, xr, xc = xyz.shape[0], 3, 1
    else:
        xyz = np.ascontiguousarray(xyz, np.float32)
        n, xr, xc = strides
    cap = n if cap is None else cap
    return _ndt_map_call(fn, tuple(head) + (_fptr(xyz), xr, xc, n, C.byref(cfg)), cap, want)


def ndt_map(xyz, resolution, min_points=6, eig_ratio=0.01, outlier_ratio=0.55, neighbors=7, device=-1):
    """the NDT voxel map of a cloud (symmicp_ndt_map): per kept voxel, in ascending key -> dict(key [m] u32, count [m], mean [m,3],
    cov [m,6] f64 (xx xy xz yy yz zz), axes [m,3,3] (axis r at [:, r]), inv_eig [m,3], grid = lo xyz + n xyz)"""
    st, r, _ = _ndt_map(lib().symmicp_ndt_map, (int(device),), xyz, ndt_config(resolution, min_points, eig_ratio, outlier_ratio, neighbors))
    if st != OK:
        raise SymmIcpError(st, "ndt_map")
    return r


def _radius_call(fn, head, xyz, radius, cap=None, strides=None, want_d2=True):
    """shared body of radius_search and Engine.radius_search_raw: fn(*head, <the C arguments>) -> (status, count [n] int32,
    offsets [n + 1] int64, rows [cap] int32 or None, d2 [cap] f32 or None, total).  cap None: the counts only (rows_out == NULL).
    strides = (n, row stride, col stride) reads xyz as a flat f32 buffer."""
    if strides is None:
        xyz = _cloud(xyz)
        n, xr, xc = xyz.shape[0], 3, 1
    else:
        xyz = np.ascontiguousarray(xyz, np.float32)
        n, xr, xc = strides
    count = np.zeros(max(n, 1), np.int32)
    offs = np.zeros(max(n, 1) + 1, np.int64)
    rows = d2 = None
    if cap is not None:
        rows = np.full(max(cap, 1), -1, np.int32)
        d2 = np.full(max(cap, 1), -1.0, np.float32) if want_d2 else None
    total = C.c_size_t(0)
    st = fn(*head, _fptr(xyz), xr, xc, n, float(radius), _i32ptr(count), offs.ctypes.data_as(C.POINTER(C.c_int64)),
            None if rows is None else _i32ptr(rows), None if d2 is None else _fptr(d2), 0 if cap is None else cap, C.byref(total))
    return st, count[:n], offs[:n + 1], rows, d2, int(total.value)


def _sort_lists(offs, rows, d2):
    """every CSR list ordered by (d2, row)"""
    seg = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    o = np.lexsort((rows, d2, seg))
    return rows[o], d2[o]


def _radius_search(fn, head, xyz, radius, sort):
    st, count, offs, _, _, total = _radius_call(fn, head, xyz, radius)
    if st != OK:
        return st, None
    st, count, offs, rows, d2, total = _radius_call(fn, head, xyz, radius, cap=total)
    if st != OK:
        return st, None
    rows, d2 = rows[:total], d2[:total]
    if sort and total:
        rows, d2 = _sort_lists(offs, rows, d2)
    return st, (count.copy(), offs.copy(), rows.copy(), d2.copy())


def radius_search(xyz, radius, device=-1, sort=True):
    """exact fixed-radius neighbours of every point in its own cloud (symmicp_radius_search): N(i) = {j != i : d2(i, j) <= r * r},
    fp32 -> (count [N] int32, offsets [N + 1] int64, rows [total] int32, d2 [total] f32), list i = rows[offsets[i]:offsets[i + 1]];
    sort=True orders every list by (d2, row) on the host (the library's order is the index's sorted order)"""
    st, r = _radius_search(lib().symmicp_radius_search, (int(device),), xyz, radius, sort)
    if st != OK:
        raise SymmIcpError(st, "radius_search")
    return r


def _fpfh_call(fn, head, xyz, nrm, radius, want_spfh, strides=None):
    """fn(*head, <the C arguments>) -> (status, fpfh [n,33], spfh [n,33] or None, count [n] or None).
    strides = (n, xyz row, xyz col, nrm row, nrm col) reads xyz / nrm as flat f32 buffers."""
    if strides is None:
        xyz, nrm = _cloud(xyz), _cloud(nrm)
        if nrm.shape != xyz.shape:
            raise ValueError("normals must match the cloud")
        n, xr, xc, nr, nc = xyz.shape[0], 3, 1, 3, 1
    else:
        xyz, nrm = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32)
        n, xr, xc, nr, nc = strides
    f = np.zeros((max(n, 1), 33), np.float32)
    s = np.zeros((max(n, 1), 33), np.float32) if want_spfh else None
    k = np.zeros(max(n, 1), np.int32) if want_spfh else None
    st = fn(*head, _fptr(xyz), xr, xc, _fptr(nrm), nr, nc, n, float(radius), _fptr(f), None if s is None else _fptr(s),
            None if k is None else _i32ptr(k))
    return st, f[:n], None if s is None else s[:n], None if k is None else k[:n]


def fpfh(xyz, nrm, radius, device=-1, want_spfh=False):
    """Fast Point Feature Histograms on the GPU (symmicp_fpfh; include/symmicp.h defines the arithmetic) -> fpfh [N,33] f32, or with
    want_spfh dict(fpfh=, spfh= [N,33], count= [N] neighbours within the radius).  Cost grows with the neighbour count."""
    st, f, s, k = _fpfh_call(lib().symmicp_fpfh, (int(device),), xyz, nrm, radius, want_spfh)
    if st != OK:
        raise SymmIcpError(st, "fpfh")
    return dict(fpfh=f, spfh=s, count=k) if want_spfh else f


def iss_config(salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5):
    cfg = IssConfig()
    lib().symmicp_iss_config_default(C.byref(cfg))
    cfg.salient_radius, cfg.non_max_radius = float(salient_radius), float(non_max_radius)
    cfg.gamma21, cfg.gamma32, cfg.min_neighbors = float(gamma21), float(gamma32), int(min_neighbors)
    return cfg


def _iss_call(fn, head, xyz, cfg, cap=None, strides=None, want=True):
    """fn(*head, <the C arguments>) -> (status, rows [cap] int32 or None, count, saliency [n] f32 or None, neighbors [n] int32 or
    None).  cap None: the count only (rows_out == NULL, cap 0).  strides = (n, row stride, col stride) reads xyz as a flat f32 buffer."""
    if strides is None:
        xyz = _cloud(xyz)
        n, xr, xc = xyz.shape[0], 3, 1
    else:
        xyz = np.ascontiguousarray(xyz, np.float32)
        n, xr, xc = strides
    rows = None if cap is None else np.full(max(cap, 1), -1, np.int32)
    sal = np.zeros(max(n, 1), np.float32) if want else None
    nb = np.zeros(max(n, 1), np.int32) if want else None
    count = C.c_size_t(0)
    st = fn(*head, _fptr(xyz), xr, xc, n, C.byref(cfg), None if rows is None else _i32ptr(rows), 0 if cap is None else cap, C.byref(count),
            None if sal is None else _fptr(sal), None if nb is None else _i32ptr(nb))
    return st, rows, int(count.value), None if sal is None else sal[:n], None if nb is None else nb[:n]


def _iss_keypoints(fn, head, xyz, cfg, return_saliency):
    """one call with cap = n, which always suffices (a count query first would run the kernels twice) -> (status, rows or
    dict(rows=, saliency=, neighbors=))"""
    st, rows, count, sal, nb = _iss_call(fn, head, xyz, cfg, cap=len(xyz), want=return_saliency)
    if st != OK:
        return st, None
    rows = rows[:count].copy()
    return st, (dict(rows=rows, saliency=sal, neighbors=nb) if return_saliency else rows)


def iss_keypoints(xyz, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5, return_saliency=False, device=-1):
    """Intrinsic Shape Signatures keypoints on the GPU (symmicp_iss_keypoints; include/symmicp.h defines the arithmetic) -> the
    keypoint rows [K] int32 in ascending order, or with return_saliency dict(rows=, saliency= [N] f32, neighbors= [N] int32:
    the counts within salient_radius).  Exact ties of the saliency go to the lowest row."""
    cfg = iss_config(salient_radius, non_max_radius, gamma21, gamma32, min_neighbors)
    st, r = _iss_keypoints(lib().symmicp_iss_keypoints, (int(device),), xyz, cfg, return_saliency)
    if st != OK:
        raise SymmIcpError(st, "iss_keypoints")
    return r


def _outlier_cloud(xyz, strides):
    if strides is None:
        xyz = _cloud(xyz)
        return xyz, xyz.shape[0], 3, 1
    n, xr, xc = strides
    return np.ascontiguousarray(xyz, np.float32), n, xr, xc


def _sor_call(fn, head, xyz, k, std_mul, cap=None, strides=None, want=True):
    """fn(*head, <the C arguments>) -> (status, rows [cap] int32 or None, count, mean_dist [n] f64 or None, stats [3] f64 = (mu, sd, thr)
    or None).  cap None: the count only (rows_out == NULL, cap 0).  strides = (n, row stride, col stride) reads xyz as a flat f32 buffer."""
    xyz, n, xr, xc = _outlier_cloud(xyz, strides)
    rows = None if cap is None else np.full(max(cap, 1), -1, np.int32)
    md = np.zeros(max(n, 1), np.float64) if want else None
    stats = np.zeros(3, np.float64) if want else None
    dptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    count = C.c_size_t(0)
    st = fn(*head, _fptr(xyz), xr, xc, n, int(k), float(std_mul), None if rows is None else _i32ptr(rows), 0 if cap is None else cap,
            C.byref(count), dptr(md), dptr(stats))
    return st, rows, int(count.value), None if md is None else md[:n], stats


def _ror_call(fn, head, xyz, radius, min_neighbors, cap=None, strides=None, want=True):
    """as _sor_call -> (status, rows [cap] int32 or None, count, neighbors [n] int32 or None)"""
    xyz, n, xr, xc = _outlier_cloud(xyz, strides)
    rows = None if cap is None else np.full(max(cap, 1), -1, np.int32)
    nb = np.zeros(max(n, 1), np.int32) if want else None
    count = C.c_size_t(0)
    st = fn(*head, _fptr(xyz), xr, xc, n, float(radius), int(min_neighbors), None if rows is None else _i32ptr(rows), 0 if cap is None else cap,
            C.byref(count), None if nb is None else _i32ptr(nb))
    return st, rows, int(count.value), None if nb is None else nb[:n]


def _remove_statistical_outlier(fn, head, xyz, k, std_mul, return_stats):
    """one call with cap = n, which always suffices -> (status, rows or dict(rows=, mean_dist=, mu=, sd=, thr=))"""
    st, rows, count, md, stats = _sor_call(fn, head, xyz, k, std_mul, cap=len(xyz), want=return_stats)
    if st != OK:
        return st, None
    rows = rows[:count].copy()
    return st, (dict(rows=rows, mean_dist=md, mu=float(stats[0]), sd=float(stats[1]), thr=float(stats[2])) if return_stats else rows)


def _remove_radius_outlier(fn, head, xyz, radius, min_neighbors, return_counts):
    st, rows, count, nb = _ror_call(fn, head, xyz, radius, min_neighbors, cap=len(xyz), want=return_counts)
    if st != OK:
        return st, None
    rows = rows[:count].copy()
    return st, (dict(rows=rows, neighbors=nb) if return_counts else rows)


def remove_statistical_outlier(xyz, k=20, std_mul=2.0, return_stats=False, device=-1):
    """Statistical outlier removal on the GPU (symmicp_statistical_outlier_removal; include/symmicp.h defines the arithmetic) -> the
    kept rows [K] int32 in ascending order: those whose mean distance to their k nearest neighbours (1 <= k <= 64) is at most
    mu + std_mul * sd over the cloud.  With return_stats dict(rows=, mean_dist= [N] f64, mu=, sd=, thr=)."""
    st, r = _remove_statistical_outlier(lib().symmicp_statistical_outlier_removal, (int(device),), xyz, k, std_mul, return_stats)
    if st != OK:
        raise SymmIcpError(st, "remove_statistical_outlier")
    return r


def remove_radius_outlier(xyz, radius, min_neighbors, return_counts=False, device=-1):
    """Radius outlier removal on the GPU (symmicp_radius_outlier_removal) -> the kept rows [K] int32 in ascending order: those with at
    least min_neighbors OTHER points within radius (the neighbourhoods of radius_search; PCL and Open3D count the point itself).  With
    return_counts dict(rows=, neighbors= [N] int32)."""
    st, r = _remove_radius_outlier(lib().symmicp_radius_outlier_removal, (int(device),), xyz, radius, min_neighbors, return_counts)
    if st != OK:
        raise SymmIcpError(st, "remove_radius_outlier")
    return r


def cluster_config(eps, min_points=1, min_cluster_size=0, max_cluster_size=0):
    cfg = ClusterConfig()
    lib().symmicp_cluster_config_default(C.byref(cfg))
    cfg.eps, cfg.min_points = float(eps), int(min_points)
    cfg.min_cluster_size, cfg.max_cluster_size = int(min_cluster_size), int(max_cluster_size)
    return cfg


def _cluster_call(fn, head, xyz, cfg, cap=None, strides=None, want=True):
    """fn(*head, <the C arguments>) -> (status, labels [n] int32, clusters, sizes [cap] int32 or None, core [n] uint8 or None,
    neighbors [n] int32 or None).  cap None: sizes_out == NULL, cap 0.  strides = (n, row stride, col stride) reads xyz as a flat f32
    buffer."""
    xyz, n, xr, xc = _outlier_cloud(xyz, strides)
    labels = np.full(max(n, 1), -2, np.int32)
    sizes = None if cap is None else np.full(max(cap, 1), -1, np.int32)
    core = np.zeros(max(n, 1), np.uint8) if want else None
    nb = np.zeros(max(n, 1), np.int32) if want else None
    clusters = C.c_size_t(0)
    st = fn(*head, _fptr(xyz), xr, xc, n, C.byref(cfg), _i32ptr(labels), C.byref(clusters), None if sizes is None else _i32ptr(sizes),
            0 if cap is None else cap, None if core is None else core.ctypes.data_as(C.POINTER(C.c_uint8)), None if nb is None else _i32ptr(nb))
    return st, labels[:n], int(clusters.value), sizes, None if core is None else core[:n], None if nb is None else nb[:n]


def _cluster_dbscan(fn, head, xyz, cfg, return_info):
    """one call with cap = n, which always suffices -> (status, labels or dict(labels=, clusters=, sizes=, core=, neighbors=))"""
    st, labels, clusters, sizes, core, nb = _cluster_call(fn, head, xyz, cfg, cap=len(xyz), want=return_info)
    if st != OK:
        return st, None
    if not return_info:
        return st, labels
    return st, dict(labels=labels, clusters=clusters, sizes=sizes[:clusters].copy(), core=core.astype(bool), neighbors=nb)


def cluster_dbscan(xyz, eps, min_points=1, min_cluster_size=0, max_cluster_size=0, return_info=False, device=-1):
    """DBSCAN on the GPU (symmicp_cluster; include/symmicp.h defines the result) -> labels [N] int32: the cluster of every row,
    numbered in ascending order of the clusters' lowest core rows, -1 for noise.  A row is core with at least min_points points
    within eps, ITSELF counted (min_points = 1: Euclidean clustering, every point core).  A border row joins the cluster of its
    nearest core neighbour.  Clusters whose size lies outside [min_cluster_size, max_cluster_size] (0 = no bound) become noise.
    With return_info dict(labels=, clusters=, sizes= [clusters] int32, core= [N] bool, neighbors= [N] int32)."""
    cfg = cluster_config(eps, min_points, min_cluster_size, max_cluster_size)
    st, r = _cluster_dbscan(lib().symmicp_cluster, (int(device),), xyz, cfg, return_info)
    if st != OK:
        raise SymmIcpError(st, "cluster_dbscan")
    return r


def clusters_from_labels(labels):
    """labels [N] (-1 = noise) -> PCL's shape: a list of ascending row arrays (int32), largest cluster first, exact size ties by lowest
    label (= lowest representative row)"""
    labels = np.asarray(labels)
    rows = np.nonzero(labels >= 0)[0]
    order = rows[np.argsort(labels[rows], kind="stable")]
    sizes = np.bincount(labels[rows]) if len(rows) else np.zeros(0, np.int64)
    parts = np.split(order.astype(np.int32), np.cumsum(sizes)[:-1]) if len(sizes) else []
    return [parts[k] for k in np.argsort(-sizes, kind="stable")]


def euclidean_clusters(xyz, tolerance, min_size=1, max_size=0, device=-1):
    """PCL's EuclideanClusterExtraction on the GPU (symmicp_cluster with min_points = 1): the connected parts of the cloud under
    'closer than tolerance', those of min_size .. max_size points (0 = no bound) -> a list of ascending row arrays, largest first."""
    return clusters_from_labels(cluster_dbscan(xyz, tolerance, 1, min_size, max_size, device=device))


def region_cos(deg):
    """the smoothness bound of an angle in degrees: THE conversion (the reference of the tests uses it too)"""
    return np.float32(np.cos(np.deg2rad(np.float64(deg))))


def region_config(eps, smoothness_deg=30.0, curvature_threshold=0.05, min_region_size=0, max_region_size=0, smoothness_cos=None):
    """symmicp_region_config; smoothness_cos, when given, is taken as it is instead of region_cos(smoothness_deg)"""
    cfg = RegionConfig()
    lib().symmicp_region_config_default(C.byref(cfg))
    cfg.eps, cfg.curvature_threshold = float(eps), float(curvature_threshold)
    cfg.smoothness_cos = float(region_cos(smoothness_deg) if smoothness_cos is None else smoothness_cos)
    cfg.min_region_size, cfg.max_region_size = int(min_region_size), int(max_region_size)
    return cfg


def _region_call(fn, head, xyz, nrm, curv, cfg, cap=None, strides=None, want=True):
    """fn(*head, <the C arguments>) -> (status, labels [n] int32, regions, sizes [cap] int32 or None, seed [n] uint8 or None,
    smooth [n] int32 or None).  cap None: sizes_out == NULL, cap 0.  strides = (n, xyz row, xyz col, nrm row, nrm col, curv stride)
    reads all three as flat f32 buffers.  curv None: every row a seed."""
    if strides is None:
        xyz, nrm = _cloud(xyz), _cloud(nrm)
        n, xr, xc, nr, nc, cs = xyz.shape[0], 3, 1, 3, 1, 1
        if len(nrm) != n:
            raise ValueError("a normal per point")
        if curv is not None:
            curv = _scalar(curv, n)
    else:
        n, xr, xc, nr, nc, cs = strides
        xyz, nrm = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32)
        curv = None if curv is None else np.ascontiguousarray(curv, np.float32)
    labels = np.full(max(n, 1), -2, np.int32)
    sizes = None if cap is None else np.full(max(cap, 1), -1, np.int32)
    seed = np.zeros(max(n, 1), np.uint8) if want else None
    smooth = np.zeros(max(n, 1), np.int32) if want else None
    regions = C.c_size_t(0)
    st = fn(*head, _fptr(xyz), xr, xc, _fptr(nrm), nr, nc, None if curv is None else _fptr(curv), cs, n, C.byref(cfg), _i32ptr(labels),
            C.byref(regions), None if sizes is None else _i32ptr(sizes), 0 if cap is None else cap,
            None if seed is None else seed.ctypes.data_as(C.POINTER(C.c_uint8)), None if smooth is None else _i32ptr(smooth))
    return st, labels[:n], int(regions.value), sizes, None if seed is None else seed[:n], None if smooth is None else smooth[:n]


def _region_growing(fn, head, xyz, nrm, curv, cfg, return_info):
    """one call with cap = n, which always suffices -> (status, labels or dict(labels=, regions=, sizes=, seed=, smooth=))"""
    st, labels, regions, sizes, seed, smooth = _region_call(fn, head, xyz, nrm, curv, cfg, cap=len(xyz), want=return_info)
    if st != OK:
        return st, None
    if not return_info:
        return st, labels
    return st, dict(labels=labels, regions=regions, sizes=sizes[:regions].copy(), seed=seed.astype(bool), smooth=smooth)


def region_growing(xyz, nrm, eps, smoothness_deg=30.0, curvature=None, curvature_threshold=0.05, min_region_size=0, max_region_size=0,
                   return_info=False, device=-1):
    """region-growing segmentation on the GPU (symmicp_region_growing; include/symmicp.h defines the result) -> labels [N] int32: the
    smooth surface part of every row, numbered in ascending order of the regions' lowest seed rows, -1 for unlabelled.  Two rows within
    eps are joined when their normals (of any sign) are within smoothness_deg of each other; regions are the connected parts of that graph
    on the SEED rows (curvature <= curvature_threshold; every row when curvature is None, e.g. estimate_normals' second result), and a
    non-seed row joins the region of its nearest smooth seed neighbour.  Regions whose size lies outside [min_region_size,
    max_region_size] (0 = no bound) become -1.  With return_info dict(labels=, regions=, sizes= [regions] int32, seed= [N] bool,
    smooth= [N] int32: smooth neighbours per row)."""
    cfg = region_config(eps, smoothness_deg, curvature_threshold, min_region_size, max_region_size)
    st, r = _region_growing(lib().symmicp_region_growing, (int(device),), xyz, nrm, curvature, cfg, return_info)
    if st != OK:
        raise SymmIcpError(st, "region_growing")
    return r


def orient_config(k=16, viewpoint=None, direction=None):
    """symmicp_orient_config: the seed of every component is the row closest to `viewpoint` (the default, at the origin), or the
    extreme row along `direction` (Open3D's rule with (0, 0, 1)); give at most one of the two"""
    if viewpoint is not None and direction is not None:
        raise ValueError("orient_normals: give a viewpoint or a direction, not both")
    cfg = OrientConfig()
    lib().symmicp_orient_config_default(C.byref(cfg))
    cfg.k = int(k)
    ref = direction if direction is not None else viewpoint
    if direction is not None:
        cfg.seed_rule = ORIENT_DIRECTION
    if ref is not None:
        cfg.ref[:] = [float(v) for v in ref]
    return cfg


def _orient_call(fn, head, xyz, nrm, cfg, strides=None, want=True):
    """fn(*head, <the C arguments>) -> (status, nrm_out [n,3] f32, flip [n] uint8 or None, component [n] int32 or None, tree [count,2]
    int32 (as the device left it) or None, OrientResult).  strides = (n, xyz row, xyz col, nrm row, nrm col) reads both as flat f32
    buffers."""
    if strides is None:
        xyz, nrm = _cloud(xyz), _cloud(nrm)
        n, xr, xc, nr, nc = xyz.shape[0], 3, 1, 3, 1
    else:
        n, xr, xc, nr, nc = strides
        xyz, nrm = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32)
    out = np.zeros((max(n, 1), 3), np.float32)
    flip = np.zeros(max(n, 1), np.uint8) if want else None
    comp = np.full(max(n, 1), -2, np.int32) if want else None
    tree = np.full((max(n, 1), 2), -1, np.int32) if want else None
    count, res = C.c_size_t(0), OrientResult()
    st = fn(*head, _fptr(xyz), xr, xc, _fptr(nrm), nr, nc, n, C.byref(cfg), _fptr(out),
            None if flip is None else flip.ctypes.data_as(C.POINTER(C.c_uint8)), None if comp is None else _i32ptr(comp),
            None if tree is None else _i32ptr(tree), C.byref(count) if want else None, C.byref(res))
    return (st, out[:n], None if flip is None else flip[:n], None if comp is None else comp[:n],
            None if tree is None else tree[:int(count.value)], res)


def _orient_normals(fn, head, xyz, nrm, cfg, return_info):
    st, out, flip, comp, tree, res = _orient_call(fn, head, xyz, nrm, cfg, want=return_info)
    if st != OK:
        return st, None
    if not return_info:
        return st, out
    tree = tree[np.lexsort((tree[:, 1], tree[:, 0]))]
    return st, dict(normals=out, flip=flip.astype(bool), component=comp, tree=tree, graph_edges=int(res.graph_edges), tree_edges=int(res.tree_edges),
                    components=int(res.components), largest_component=int(res.largest_component), flipped=int(res.flipped), rounds=int(res.rounds))


def orient_normals(xyz, nrm, k=16, viewpoint=None, direction=None, return_info=False, device=-1):
    """consistent normal orientation on the GPU (symmicp_orient_normals; include/symmicp.h defines the result) -> normals [N,3]: `nrm`
    with the signs of some rows inverted so that neighbouring normals agree, one orientation propagated along the minimum spanning
    forest of the symmetrised k-NN graph (Hoppe et al. 1992).  Every connected component of that graph is seeded on its own: at its row
    closest to `viewpoint` (default: the origin), flipped towards it, or at its extreme row along `direction`, flipped along it.  The
    result does not depend on the signs of `nrm`.  With return_info dict(normals=, flip= [N] bool, component= [N] int32 (the lowest
    row of the row's component), tree= [N - components, 2] int32 sorted (lo, hi), graph_edges=, tree_edges=, components=,
    largest_component=, flipped=, rounds=)."""
    st, r = _orient_normals(lib().symmicp_orient_normals, (int(device),), xyz, nrm, orient_config(k, viewpoint, direction), return_info)
    if st != OK:
        raise SymmIcpError(st, "orient_normals")
    return r


def pack_clusters(xyz, nrm, labels):
    """the bridge from labels to batch_align: the rows of every cluster with at most BATCH_MAX_POINTS points, packed cluster after
    cluster (ascending label, ascending row) -> dict(xyz= [M,3], nrm= [M,3] or None, ranges= [K,2] int64 (first, count) rows of the
    pools, labels= [K] the packed clusters' labels, rows= [M] the original row of every packed row, skipped= [(label, size), ...] the
    clusters above BATCH_MAX_POINTS, which are not packed).  A batch problem of cluster a of one cloud against cluster b of another is
    (ranges_s[a, 0], ranges_s[a, 1], ranges_t[b, 0], ranges_t[b, 1])."""
    xyz = _cloud(xyz)
    nrm = None if nrm is None else _cloud(nrm)
    labels = np.asarray(labels)
    if len(labels) != len(xyz) or (nrm is not None and len(nrm) != len(xyz)):
        raise ValueError("a label and a normal per point")
    rows, ranges, kept, skipped, at = [], [], [], [], 0
    sizes = np.bincount(labels[labels >= 0]) if (labels >= 0).any() else np.zeros(0, np.int64)
    order = np.argsort(np.where(labels >= 0, labels, len(sizes)), kind="stable")
    first = np.concatenate([[0], np.cumsum(sizes)])
    for k, m in enumerate(sizes.tolist()):
        if m == 0:
            continue
        if m > BATCH_MAX_POINTS:
            skipped.append((k, m))
            continue
        rows.append(order[first[k]:first[k] + m])
        ranges.append((at, m))
        kept.append(k)
        at += m
    rows = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    return dict(xyz=np.ascontiguousarray(xyz[rows]), nrm=None if nrm is None else np.ascontiguousarray(nrm[rows]),
                ranges=np.array(ranges, np.int64).reshape(-1, 2), labels=np.array(kept, np.int32), rows=rows, skipped=skipped)


def plane_config(max_dist, hypotheses=1000, seed=0, refits=1, min_inliers=3, axis=None, max_angle_deg=0.0):
    cfg = PlaneConfig()
    lib().symmicp_plane_config_default(C.byref(cfg))
    cfg.max_dist, cfg.hypotheses, cfg.seed, cfg.refits, cfg.min_inliers = float(max_dist), int(hypotheses), int(seed), int(refits), int(min_inliers)
    if axis is not None:
        cfg.axis[:] = [float(v) for v in axis]
    cfg.max_angle_deg = float(max_angle_deg)
    return cfg


def _plane_call(fn, head, xyz, cfg, cap=None, strides=None, want=True):
    """fn(*head, <the C arguments>) -> (status, dict(plane [4] f64, plane32 [4] f32, rows [cap] int32 or None, count, best_hypothesis,
    evaluated, inliers_ransac, inliers_final, rmse_final[, distance [n] f64, hyp_status [H] uint8, hyp_inliers [H] int32])).  cap None: the
    count only (rows_out == NULL, cap 0).  strides = (n, row stride, col stride) reads xyz as a flat f32 buffer."""
    xyz, n, xr, xc = _outlier_cloud(xyz, strides)
    H = int(cfg.hypotheses)
    rows = None if cap is None else np.full(max(cap, 1), -1, np.int32)
    dist = np.zeros(max(n, 1), np.float64) if want else None
    status = np.zeros(max(H, 1), np.uint8) if want else None
    inl = np.zeros(max(H, 1), np.int32) if want else None
    plane = np.zeros(4, np.float32)
    res = PlaneResult()
    count = C.c_size_t(0)
    st = fn(*head, _fptr(xyz), xr, xc, n, C.byref(cfg), _fptr(plane), C.byref(res), None if rows is None else _i32ptr(rows),
            0 if cap is None else cap, C.byref(count), None if dist is None else dist.ctypes.data_as(C.POINTER(C.c_double)),
            None if status is None else status.ctypes.data_as(C.POINTER(C.c_uint8)), None if inl is None else _i32ptr(inl))
    r = dict(plane=np.array(res.plane[:], np.float64), plane32=plane, rows=rows, count=int(count.value), best_hypothesis=res.best_hypothesis,
             evaluated=res.evaluated, inliers_ransac=res.inliers_ransac, inliers_final=res.inliers_final, rmse_final=res.rmse_final)
    if want:
        r["distance"], r["hyp_status"], r["hyp_inliers"] = dist[:n], status[:H], inl[:H]
    return st, r


def _segment_plane(fn, head, xyz, cfg, return_info):
    """one call with cap = n, which always suffices -> (status, (plane, rows) or the dict of _plane_call with rows cut to the count)"""
    st, r = _plane_call(fn, head, xyz, cfg, cap=len(xyz), want=return_info)
    r["rows"] = r["rows"][:r["count"]].copy()
    r["status"] = st
    return st, (r if return_info else (r["plane"], r["rows"]))


def segment_plane(xyz, max_dist, hypotheses=1000, seed=0, refits=1, min_inliers=3, axis=None, max_angle_deg=0.0, return_info=False, device=-1):
    """RANSAC plane segmentation on the GPU (symmicp_segment_plane; include/symmicp.h defines the result) -> (plane [4] float64 = (n, d)
    with n . x + d = 0, rows [K] int32: the rows within max_dist of it, ascending).  axis / max_angle_deg: only planes whose normal lies
    within that angle of the axis (PCL's perpendicular-plane model).  With return_info a dict (plane=, plane32=, rows=, count=,
    best_hypothesis=, evaluated=, inliers_ransac=, inliers_final=, rmse_final=, distance= [N] f64, hyp_status= [H], hyp_inliers= [H]).
    Raises SymmIcpError (ERR_NO_CONSENSUS) when no plane reaches max(3, min_inliers) rows."""
    cfg = plane_config(max_dist, hypotheses, seed, refits, min_inliers, axis, max_angle_deg)
    st, r = _segment_plane(lib().symmicp_segment_plane, (int(device),), xyz, cfg, return_info)
    if st != OK:
        raise SymmIcpError(st, "segment_plane")
    return r


def _segment_planes(one, xyz, max_dist, max_planes, min_inliers, hypotheses, seed, refits, axis, max_angle_deg):
    xyz = _cloud(xyz)
    labels = np.full(len(xyz), -1, np.int32)
    planes = []
    for k in range(int(max_planes)):
        left = np.nonzero(labels < 0)[0]
        if len(left) < max(3, int(min_inliers)):
            break
        cfg = plane_config(max_dist, hypotheses, int(seed) + k, refits, min_inliers, axis, max_angle_deg)
        st, r = one(np.ascontiguousarray(xyz[left]), cfg)
        if st == ERR_NO_CONSENSUS:
            break
        if st != OK:
            raise SymmIcpError(st, "segment_planes")
        plane, rows = r
        labels[left[rows]] = k
        planes.append(plane)
    return np.array(planes, np.float64).reshape(-1, 4), labels


def segment_planes(xyz, max_dist, max_planes, min_inliers, hypotheses=1000, seed=0, refits=1, axis=None, max_angle_deg=0.0, device=-1):
    """planes peeled one at a time -> (planes [P,4] float64, labels [N] int32: the plane of every row, -1 for rows on none).  Plane k is
    segment_plane on the rows not yet labelled, with seed + k; the loop stops at max_planes or at the first plane with fewer than
    max(3, min_inliers) rows.  A host loop over segment_plane."""
    one = lambda sub, cfg: _segment_plane(lib().symmicp_segment_plane, (int(device),), sub, cfg, False)
    return _segment_planes(one, xyz, max_dist, max_planes, min_inliers, hypotheses, seed, refits, axis, max_angle_deg)


def _features(f):
    f = np.ascontiguousarray(f, dtype=np.float32)
    if f.ndim != 2 or f.shape[1] != 33:
        raise ValueError("features must be [N,33]")
    return f


def _feature_nn_call(fn, head, fa, fb):
    """fn(*head, <the C arguments>) -> (status, nn [na] int32, d2 [na] f32, second [na] f32)"""
    fa, fb = _features(fa), _features(fb)
    na = fa.shape[0]
    nn = np.full(max(na, 1), -1, np.int32)
    d2 = np.zeros(max(na, 1), np.float32)
    sec = np.zeros(max(na, 1), np.float32)
    st = fn(*head, _fptr(fa), na, _fptr(fb), fb.shape[0], _i32ptr(nn), _fptr(d2), _fptr(sec))
    return st, nn[:na], d2[:na], sec[:na]


def feature_nn(fa, fb, device=-1):
    """exact nearest neighbour of every row of fa among the rows of fb in the 33-d feature space (symmicp_feature_nn;
    include/symmicp.h defines the arithmetic) -> (nn [na] int32, d2 [na] f32, second [na] f32); ties go to the lowest row"""
    st, nn, d2, sec = _feature_nn_call(lib().symmicp_feature_nn, (int(device),), fa, fb)
    if st != OK:
        raise SymmIcpError(st, "feature_nn")
    return nn, d2, sec


def _feature_corr_call(fn, head, fa, fb, mutual, max_ratio, cap=None):
    """fn(*head, <the C arguments>) -> (status, pairs [count,2] int32 or None, d2 [count] or None, count); cap None: na"""
    fa, fb = _features(fa), _features(fb)
    na = fa.shape[0]
    cap = na if cap is None else cap
    pairs = np.full((max(cap, 1), 2), -1, np.int32)
    d2 = np.zeros(max(cap, 1), np.float32)
    cnt = C.c_size_t(0)
    st = fn(*head, _fptr(fa), na, _fptr(fb), fb.shape[0], int(bool(mutual)), float(max_ratio), _i32ptr(pairs) if cap > 0 else None,
            _fptr(d2) if cap > 0 else None, cap, C.byref(cnt))
    n = int(cnt.value)
    if st != OK:
        return st, None, None, n
    return st, pairs[:n].copy(), d2[:n].copy(), n


def feature_correspondences(fa, fb, mutual=True, max_ratio=0.0, device=-1):
    """the matches ransac() consumes (symmicp_feature_correspondences): (i, nn(i)) for every row i of fa that passes the mutual
    test (nn of nn(i) is i) and the ratio test (d2 <= max_ratio^2 * second; <= 0: off) -> (pairs [count,2] int32, d2 [count] f32)"""
    st, pairs, d2, _ = _feature_corr_call(lib().symmicp_feature_correspondences, (int(device),), fa, fb, mutual, max_ratio)
    if st != OK:
        raise SymmIcpError(st, "feature_correspondences")
    return pairs, d2


def ransac_config(max_dist, hypotheses=100000, seed=0, edge_ratio=0.9, refits=1):
    cfg = RansacConfig()
    lib().symmicp_ransac_config_default(C.byref(cfg))
    cfg.max_dist, cfg.hypotheses, cfg.seed, cfg.edge_ratio, cfg.refits = float(max_dist), int(hypotheses), int(seed), float(edge_ratio), int(refits)
    return cfg


def _ransac_call(fn, head, src, tgt, pairs, cfg, want_hypotheses=False):
    """fn(*head, <the C arguments>) -> (status, result dict).  The dict is filled on failure too (identity transform)."""
    src, tgt = _cloud(src), _cloud(tgt)
    pairs = np.ascontiguousarray(pairs, np.int32)
    if pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be [m,2]")
    m, H = pairs.shape[0], int(cfg.hypotheses)
    X = np.zeros(16, np.float32)
    res = RansacResult()
    mask = np.zeros(max(m, 1), np.uint8)
    status = np.zeros(max(H, 1), np.uint8) if want_hypotheses else None
    inl = np.zeros(max(H, 1), np.int32) if want_hypotheses else None
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    st = fn(*head, _fptr(src), 3, 1, src.shape[0], _fptr(tgt), 3, 1, tgt.shape[0], _i32ptr(pairs), m, C.byref(cfg), _fptr(X), C.byref(res),
            u8(mask), u8(status), None if inl is None else _i32ptr(inl))
    r = dict(status=st, transform=X.reshape(4, 4), transform64=np.array(res.transform[:], np.float64).reshape(4, 4),
             best_hypothesis=res.best_hypothesis, evaluated=res.evaluated, inliers_ransac=res.inliers_ransac,
             inliers_final=res.inliers_final, rmse_final=res.rmse_final, inlier_mask=mask[:m].astype(bool))
    if want_hypotheses:
        r["hyp_status"], r["hyp_inliers"] = status[:H], inl[:H]
    return st, r


def ransac(src, tgt, pairs, max_dist, hypotheses=100000, seed=0, edge_ratio=0.9, refits=1, device=-1, want_hypotheses=False):
    """a rigid transform from correspondences with outliers (symmicp_ransac) -> dict(transform [4,4] f32, transform64, best_hypothesis,
    evaluated, inliers_ransac, inliers_final, rmse_final, inlier_mask [m] bool[, hyp_status [H], hyp_inliers [H]]).  Raises
    SymmIcpError (ERR_NO_CONSENSUS) when no hypothesis reaches 3 inliers."""
    st, r = _ransac_call(lib().symmicp_ransac, (int(device),), src, tgt, pairs, ransac_config(max_dist, hypotheses, seed, edge_ratio, refits),
                         want_hypotheses)
    if st != OK:
        raise SymmIcpError(st, "ransac")
    return r


def fgr_config(max_dist, iterations=64, decrease_every=4, division_factor=1.4, tuple_scale=0.95, max_tuples=1000, tuple_trials=0, seed=0):
    cfg = FgrConfig()
    lib().symmicp_fgr_config_default(C.byref(cfg))
    cfg.max_dist, cfg.iterations, cfg.decrease_every, cfg.division_factor = float(max_dist), int(iterations), int(decrease_every), float(division_factor)
    cfg.tuple_scale, cfg.max_tuples, cfg.tuple_trials, cfg.seed = float(tuple_scale), int(max_tuples), int(tuple_trials), int(seed)
    return cfg


def _fgr_call(fn, head, src, tgt, pairs, cfg, want_trace=False):
    """fn(*head, <the C arguments>) -> (status, result dict).  The dict is filled on failure too."""
    src, tgt = _cloud(src), _cloud(tgt)
    pairs = np.ascontiguousarray(pairs, np.int32)
    if pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be [m,2]")
    m, K = pairs.shape[0], max(int(cfg.iterations), 0)
    cap = max(3 * int(cfg.max_tuples) if cfg.max_tuples else m, 1)
    X = np.zeros(16, np.float32)
    res = FgrResult()
    sel = np.zeros(cap, np.int32)
    weight = np.zeros(cap, np.float32)
    trX = np.zeros((K + 1, 16), np.float32) if want_trace else None
    trS = np.zeros((max(K, 1), 40), np.float64) if want_trace else None
    trM = np.zeros(max(K, 1), np.float32) if want_trace else None
    st = fn(*head, _fptr(src), 3, 1, src.shape[0], _fptr(tgt), 3, 1, tgt.shape[0], _i32ptr(pairs), m, C.byref(cfg), _fptr(X), C.byref(res),
            _i32ptr(sel), _fptr(weight), None if trX is None else _fptr(trX),
            None if trS is None else trS.ctypes.data_as(C.POINTER(C.c_double)), None if trM is None else _fptr(trM))
    M = int(res.set_size)
    r = dict(status=st, transform=X.reshape(4, 4), transform64=np.array(res.transform[:], np.float64).reshape(4, 4),
             iterations=res.iterations, inliers=res.inliers, tuples_accepted=res.tuples_accepted, set_size=M, mu=np.float32(res.mu),
             weight_sum=res.weight_sum, rmse=res.rmse, set=sel[:M].copy(), weights=weight[:M].copy())
    if want_trace:
        r["X_trace"], r["sums_trace"], r["mu_trace"] = trX.reshape(K + 1, 4, 4), trS[:K], trM[:K]
    return st, r


def fgr(src, tgt, pairs, max_dist, iterations=64, decrease_every=4, division_factor=1.4, tuple_scale=0.95, max_tuples=1000, tuple_trials=0,
        seed=0, device=-1, want_trace=False):
    """Fast Global Registration from correspondences with outliers (symmicp_fgr): a tuple test, then the whole graduated-non-convexity
    loop in one launch -> dict(transform [4,4] f32, transform64, iterations, inliers, rmse, tuples_accepted, set_size, set [M], weights [M],
    mu, weight_sum[, X_trace [K+1,4,4], sums_trace [K,40], mu_trace [K]]).  Raises SymmIcpError (ERR_NO_CONSENSUS: no trial passed the
    tuple test; ERR_DEGENERATE: a solve failed)."""
    st, r = _fgr_call(lib().symmicp_fgr, (int(device),), src, tgt, pairs,
                      fgr_config(max_dist, iterations, decrease_every, division_factor, tuple_scale, max_tuples, tuple_trials, seed), want_trace)
    if st != OK:
        raise SymmIcpError(st, "fgr")
    return r


def batch_config(**kw):
    """symmicp_batch_config with its defaults (PAPER, 10 iterations, threshold 1, gates and eps rule off), then the given fields"""
    cfg = BatchConfig()
    lib().symmicp_batch_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k) or k == "reserved":
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def batch_problems(problems):
    """[(src_first, src_count, tgt_first, tgt_count), ...] (or an [B, 4] array) -> a ctypes array of symmicp_batch_problem"""
    rows = np.asarray(problems, np.int64).reshape(-1, 4)
    if rows.size and (rows.min() < 0 or rows.max() > 0xFFFFFFFF):
        raise ValueError("problem rows must fit 32 unsigned bits")
    return (BatchProblem * max(len(rows), 1))(*[BatchProblem(*[int(v) for v in r]) for r in rows]), len(rows)


def _batch_call(fn, head, src, src_n, tgt, tgt_n, problems, guesses, cfg, trace):
    """fn(*head, <the C arguments>) -> (status, results (a ctypes array of BatchResult), trace_X [B, max_iters + 1, 4, 4] f32 or None,
    trace_sums [B, max_iters + 1, 40] f64 or None)"""
    src, tgt, tgt_n = _cloud(src), _cloud(tgt), _cloud(tgt_n)
    src_n = None if src_n is None else _cloud(src_n)
    if (src_n is not None and len(src_n) != len(src)) or len(tgt_n) != len(tgt):
        raise ValueError("a normal per point")
    probs, B = batch_problems(problems)
    g = None
    if guesses is not None:
        g = np.ascontiguousarray(guesses, np.float32).reshape(-1, 16)
        if len(g) != B:
            raise ValueError("one 4x4 guess per problem")
    out = (BatchResult * max(B, 1))()
    rows = max(int(cfg.max_iters), 0) + 1
    tX = np.zeros((max(B, 1), rows, 16), np.float32) if trace else None
    tS = np.zeros((max(B, 1), rows, NSUM), np.float64) if trace else None
    st = fn(*head, _fptr(src), None if src_n is None else _fptr(src_n), len(src), _fptr(tgt), _fptr(tgt_n), len(tgt), probs,
            None if g is None else _fptr(g), B, C.byref(cfg), out, None if tX is None else _fptr(tX),
            None if tS is None else tS.ctypes.data_as(C.POINTER(C.c_double)))
    return st, out, (None if tX is None else tX[:B].reshape(B, rows, 4, 4)), (None if tS is None else tS[:B])


def _batch_dicts(out, B):
    res = []
    for b in range(B):
        r = out[b]
        res.append(dict(status=r.status, iters=r.iters, diff_initial=r.diff_initial, diff_final=r.diff_final, rcond=r.rcond,
                        pivot=np.array(r.pivot[:], np.float32), transform=np.array(r.transform[:], np.float32).reshape(4, 4),
                        diffs=np.array(r.diffs[:min(max(r.iters, 0) + 1, 64)], np.float32), pairs=r.pairs,
                        sums=np.array(r.sums.s[:], np.float64), raw=bytes(r)))
    return res


def _batch_align(fn, head, src, src_n, tgt, tgt_n, problems, guesses, trace, cfg):
    c = batch_config(**cfg)
    st, out, tX, tS = _batch_call(fn, head, src, src_n, tgt, tgt_n, problems, guesses, c, trace)
    if st != OK:
        return st, None
    res = _batch_dicts(out, len(np.asarray(problems).reshape(-1, 4)))
    return st, ((res, tX, tS) if trace else res)


def batch_align(src, src_n, tgt, tgt_n, problems, guesses=None, trace=False, device=-1, **cfg):
    """Many small ICP problems in one launch (symmicp_batch_align; include/symmicp.h has the contract).  src / src_n and tgt / tgt_n
    are packed [n, 3] pools, problems [(src_first, src_count, tgt_first, tgt_count), ...] row ranges of them (at most BATCH_MAX_POINTS
    rows each), guesses [B, 4, 4] or None, cfg the fields of BatchConfig (mode, max_iters, fixed_iters, diff_threshold,
    max_corr_dist, min_normal_dot, eps_rotation, eps_translation).  -> one dict per problem (status, iters, diff_initial, diff_final,
    rcond, pivot, transform, diffs, pairs, sums, raw = the result struct's bytes); with trace also trace_X [B, max_iters + 1, 4, 4]
    and trace_sums [B, max_iters + 1, 40]: (results, trace_X, trace_sums).  A degenerate problem is reported in its own status."""
    st, r = _batch_align(lib().symmicp_batch_align, (int(device),), src, src_n, tgt, tgt_n, problems, guesses, trace, cfg)
    if st != OK:
        raise SymmIcpError(st, "batch_align")
    return r


def information_from_sums(n, sum_q, sum_qq):
    """the [6, 6] float64 information matrix (rotation first) of n inliers with sum q = sum_q [3] and the upper triangle of sum q q^T =
    sum_qq [6] (xx, xy, xz, yy, yz, zz): symmicp_information_from_sums, a pure host function"""
    q = np.ascontiguousarray(sum_q, np.float64).reshape(3)
    qq = np.ascontiguousarray(sum_qq, np.float64).reshape(6)
    out = np.zeros(36, np.float64)
    dp = C.POINTER(C.c_double)
    st = lib().symmicp_information_from_sums(int(n), q.ctypes.data_as(dp), qq.ctypes.data_as(dp), out.ctypes.data_as(dp))
    if st != OK:
        raise SymmIcpError(st, "information_from_sums")
    return out.reshape(6, 6)


def _transforms(transforms):
    """None, one [4, 4] or [K, 4, 4] -> (contiguous [K, 16] float32 or None, K, single)"""
    if transforms is None:
        return None, 1, True
    X = np.ascontiguousarray(transforms, np.float32)
    single = X.ndim == 2
    X = X.reshape(-1, 16)
    return X, len(X), single


def _eval_dicts(out, K, nn, d2):
    res = []
    for k in range(K):
        e = out[k]
        r = dict(inliers=int(e.inliers), fitness=e.fitness, rmse=e.rmse, mean_d2=e.mean_d2, sum_d2=e.sum_d2,
                 sum_q=np.array(e.sum_q[:], np.float64), sum_qq=np.array(e.sum_qq[:], np.float64),
                 information=np.array(e.information[:], np.float64).reshape(6, 6), raw=bytes(e))
        if nn is not None:
            r.update(nn=nn[k], d2=d2[k])
        res.append(r)
    return res


def _eval_call(fn, head, clouds, transforms, max_dist, want_pairs, ns):
    """fn(*head, <cloud arguments>, X, K, max_dist, out, nn, d2) -> (status, one dict per transform or None, single)"""
    X, K, single = _transforms(transforms)
    out = (Evaluation * max(K, 1))()
    rows = K if 1 <= K <= EVAL_MAX_TRANSFORMS else 1
    nn = np.empty((rows, ns), np.int32) if want_pairs else None
    d2 = np.empty((rows, ns), np.float32) if want_pairs else None
    st = fn(*head, *clouds, None if X is None else _fptr(X), K, float(max_dist), out, None if nn is None else _i32ptr(nn),
            None if d2 is None else _fptr(d2))
    return st, (_eval_dicts(out, K, nn, d2) if st == OK else None), single


def _eval_clouds(src, tgt, strides=None):
    """packed [n, 3] clouds, or with strides = (src_row, src_col, ns, tgt_row, tgt_col, nt) raw float32 buffers"""
    if strides is None:
        src, tgt = _cloud(src), _cloud(tgt)
        return (_fptr(src), 3, 1, len(src), _fptr(tgt), 3, 1, len(tgt)), len(src), (src, tgt)
    sr, sc, ns, tr, tc, nt = strides
    return (_fptr(src), sr, sc, ns, _fptr(tgt), tr, tc, nt), ns, (src, tgt)


def evaluate_registration(src, tgt, transforms=None, max_dist=0.0, device=-1, want_pairs=False):
    """How good an alignment is (symmicp_evaluate_registration; include/symmicp.h has the definition): for every transform ([4, 4],
    [K, 4, 4], or None for the identity) a dict with inliers, fitness, rmse, mean_d2 (PCL's getFitnessScore), sum_d2, sum_q, sum_qq and
    information ([6, 6] float64, rotation first, about the caller's origin); with want_pairs also nn [ns] (the target row, -1 for a
    row that is no inlier) and d2 [ns].  max_dist <= 0: every row is an inlier.  One transform in -> one dict out; [K, 4, 4] -> a list."""
    args, ns, keep = _eval_clouds(src, tgt)
    st, r, single = _eval_call(lib().symmicp_evaluate_registration, (int(device),), args, transforms, max_dist, want_pairs, ns)
    if st != OK:
        raise SymmIcpError(st, "evaluate_registration")
    return r[0] if single else r


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def posegraph_config(max_dist=0.0, max_iterations=100, reference_node=0, cg_max_iterations=0, preference_loop_closure=1.0,
                     line_process_weight=0.0, edge_prune_threshold=0.25, min_relative_decrease=1e-6, min_increment=1e-9, cg_tolerance=1e-10):
    cfg = PosegraphConfig()
    lib().symmicp_posegraph_config_default(C.byref(cfg))
    cfg.max_dist, cfg.max_iterations, cfg.reference_node, cfg.cg_max_iterations = float(max_dist), int(max_iterations), int(reference_node), int(cg_max_iterations)
    cfg.preference_loop_closure, cfg.line_process_weight, cfg.edge_prune_threshold = float(preference_loop_closure), float(line_process_weight), float(edge_prune_threshold)
    cfg.min_relative_decrease, cfg.min_increment, cfg.cg_tolerance = float(min_relative_decrease), float(min_increment), float(cg_tolerance)
    return cfg


def pose_edges(edges):
    """a (PoseEdge * m) array from one, or from a sequence of PoseEdge or of (source, target, uncertain, T [4,4], information [6,6])"""
    if isinstance(edges, C.Array) and edges._type_ is PoseEdge:
        return edges
    out = (PoseEdge * max(len(edges), 1))()
    for k, e in enumerate(edges):
        if isinstance(e, PoseEdge):
            out[k] = e
            continue
        s, t, unc, T, L = e
        T, L = np.ascontiguousarray(T, np.float64), np.ascontiguousarray(L, np.float64)
        if T.shape != (4, 4) or L.shape != (6, 6):
            raise ValueError("an edge is (source, target, uncertain, T [4,4], information [6,6])")
        out[k].source, out[k].target, out[k].uncertain = int(s), int(t), int(bool(unc))
        out[k].transform[:] = T.reshape(16).tolist()
        out[k].information[:] = L.reshape(36).tolist()
    return out


def _poses(poses):
    X = np.ascontiguousarray(poses, np.float64)
    if X.ndim != 3 or X.shape[1:] != (4, 4):
        raise ValueError("poses must be [n,4,4]")
    return X


def _posegraph_call(fn, head, poses, edges, cfg, want_trace=False):
    """fn(*head, <the C arguments>) -> (status, result dict).  The dict is filled on failure too."""
    X, m = _poses(poses), len(edges)
    E = pose_edges(edges)
    out = np.zeros_like(X)
    res = PosegraphResult()
    w, pr = np.zeros(max(m, 1), np.float64), np.zeros(max(m, 1), np.uint8)
    K = max(int(cfg.max_iterations), 1)
    tr = (PosegraphIteration * K)() if want_trace else None
    st = fn(*head, _dptr(X), len(X), E, m, C.byref(cfg), _dptr(out), C.byref(res), _dptr(w), pr.ctypes.data_as(C.POINTER(C.c_uint8)), tr)
    r = dict(status=st, poses=out, weights=w[:m], pruned=pr[:m].astype(bool), iterations=res.iterations, accepted_steps=res.accepted_steps,
             stop_reason=res.stop_reason, pruned_count=res.pruned, cg_iterations=res.cg_iterations, cost_initial=res.cost_initial,
             cost_final=res.cost_final, mu=res.mu, lambda_final=res.lambda_final, grad_max=res.grad_max)
    if want_trace:
        r["trace"] = [_pg_iteration(tr[k]) for k in range(min(max(res.iterations, 0), K))]
    return st, r


def _pg_iteration(t):
    return dict(cost=t.cost, cost_trial=t.cost_trial, model_decrease=t.model_decrease, grad_max=t.grad_max, delta_max=t.delta_max,
                hdiag_max=t.hdiag_max, lam=t.lambda_, cg_residual=t.cg_residual, cg_iterations=t.cg_iterations, accepted=bool(t.accepted),
                status=t.status)


def posegraph_optimize(poses, edges, max_dist=0.0, device=-1, want_trace=False, **cfg):
    """Multiway registration's back end (symmicp_posegraph_optimize; include/symmicp.h has the definitions): Levenberg-Marquardt over the
    poses [n,4,4] (node frame -> world) of a pose graph whose edges are PoseEdge or (source, target, uncertain, T, information) entries,
    with a line process on the uncertain ones -> dict(poses [n,4,4] f64, weights [m], pruned [m] bool, iterations, accepted_steps,
    stop_reason, pruned_count, cg_iterations, cost_initial, cost_final, mu, lambda_final, grad_max[, trace]).  cfg: the fields of
    posegraph_config.  Raises SymmIcpError."""
    st, r = _posegraph_call(lib().symmicp_posegraph_optimize, (int(device),), poses, edges, posegraph_config(max_dist, **cfg), want_trace)
    if st != OK:
        raise SymmIcpError(st, "posegraph_optimize")
    return r


def posegraph_edge_error(Xs, Xt, T):
    """e = (w, tau) of one edge at the poses Xs, Xt (symmicp_posegraph_edge_error, a pure host function)"""
    a = [np.ascontiguousarray(v, np.float64).reshape(16) for v in (Xs, Xt, T)]
    e = np.zeros(6, np.float64)
    st = lib().symmicp_posegraph_edge_error(_dptr(a[0]), _dptr(a[1]), _dptr(a[2]), _dptr(e))
    if st != OK:
        raise SymmIcpError(st, "posegraph_edge_error")
    return e


def posegraph_line_weight(mu, c):
    return float(lib().symmicp_posegraph_line_weight(float(mu), float(c)))


def build_pose_graph(clouds, normals, pairs, max_dist, **engine_kwargs):
    """The front end of multiway registration: every pair (s, t, uncertain, guess or None) of `pairs` is registered with cloud s as source
    and cloud t as target on one Engine(**engine_kwargs) (set_target, set_source, align from the guess) and scored by
    evaluate_registration at max_dist -> (edges, poses): the edges as (s, t, uncertain, T [4,4] f64 -- the fp32 result with its rotation
    block moved to the nearest rotation --, information [6,6]) and initial
    poses [n,4,4] chained along the certain edges from node 0 (X_s = X_t T; a node no certain edge reaches is chained along an uncertain
    one)."""
    n = len(clouds)
    edges = []
    with Engine(**engine_kwargs) as e:
        for s, t, unc, guess in pairs:
            e.set_target(clouds[t], normals[t])
            e.set_source(clouds[s], normals[s])
            r = e.align(guess, check=True)
            ev = e.evaluate_registration(clouds[s], clouds[t], r["transform"], max_dist)
            edges.append((int(s), int(t), int(bool(unc)), _nearest_rigid(r["transform"]), ev["information"]))
    poses = [None] * n
    poses[0] = np.eye(4)
    for certain_only in (True, False):
        grown = True
        while grown:
            grown = False
            for s, t, unc, T, _ in edges:
                if unc and certain_only:
                    continue
                if poses[t] is not None and poses[s] is None:
                    poses[s], grown = poses[t] @ T, True
                elif poses[s] is not None and poses[t] is None:
                    poses[t], grown = poses[s] @ _inverse_rigid64(T), True
    if any(p is None for p in poses):
        raise ValueError("the pairs do not connect every cloud to cloud 0")
    return edges, np.stack(poses)


def _nearest_rigid(T):
    """an fp32 transform as fp64 with its rotation block moved to the nearest rotation (SVD): an fp32 rotation is orthonormal to 1e-7
    only, and chained poses would add that up"""
    out = np.eye(4)
    U, _, Vt = np.linalg.svd(np.asarray(T, np.float64)[:3, :3])
    out[:3, :3] = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    out[:3, 3] = np.asarray(T, np.float64)[:3, 3]
    return out


def _inverse_rigid64(T):
    T = np.asarray(T, np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def multiway_registration(clouds, normals, pairs, max_dist, device=-1, want_trace=False, engine_kwargs=None, **cfg):
    """build_pose_graph followed by posegraph_optimize -> its dict, plus edges and initial_poses"""
    edges, poses = build_pose_graph(clouds, normals, pairs, max_dist, **(engine_kwargs or {}))
    r = posegraph_optimize(poses, edges, max_dist, device=device, want_trace=want_trace, **cfg)
    r.update(edges=edges, initial_poses=poses)
    return r


def shard_range(n, nranks, rank):
    b, c = C.c_size_t(0), C.c_size_t(0)
    st = lib().symmicp_shard_range(n, nranks, rank, C.byref(b), C.byref(c))
    if st != OK:
        raise SymmIcpError(st, "shard_range")
    return int(b.value), int(c.value)


def comm_get_unique_id():
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    st = lib().symmicp_comm_get_unique_id(C.cast(buf, C.c_void_p))
    if st != OK:
        raise SymmIcpError(st, "comm_get_unique_id")
    return bytes(buf.raw)


class Engine:
    """Thin object wrapper over one symmicp_ctx."""

    def __init__(self, **cfg):
        self._L = lib()
        self.cfg = default_config(**cfg)
        h = C.c_void_p()
        st = self._L.symmicp_create(C.byref(self.cfg), C.byref(h))
        if st != OK:
            raise SymmIcpError(st, "symmicp_create (no usable gfx950 HIP device? there is no CPU fallback)")
        self._h = h
        self._keep = []

    def close(self):
        if getattr(self, "_h", None):
            self._L.symmicp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, st):
        if st != OK:
            raise SymmIcpError(st, (self._L.symmicp_last_error(self._h) or b"").decode())

    def set_config(self, **kw):
        for k, v in kw.items():
            setattr(self.cfg, k, v)
        self._chk(self._L.symmicp_set_config(self._h, C.byref(self.cfg)))

    def comm_init_rank(self, nranks, rank, uid):
        buf = C.create_string_buffer(uid, UNIQUE_ID_BYTES) if uid is not None else None
        self._chk(self._L.symmicp_comm_init_rank(self._h, nranks, rank, C.cast(buf, C.c_void_p) if buf else None))

    def comm_init_shm(self, nranks, rank, job_name):
        """ranks of one node: exchange the per-pass record through POSIX shared memory instead of RCCL"""
        self._chk(self._L.symmicp_comm_init_shm(self._h, nranks, rank, str(job_name).encode()))

    def set_sums(self, total):
        """external exchange (comm_init_rank(nranks, rank, None)): hand the record summed over all ranks back before step()"""
        s = Sums()
        t = np.ascontiguousarray(np.asarray(total, np.float64).reshape(-1))
        for k in range(len(s.s)):
            s.s[k] = float(t[k])
        self._chk(self._L.symmicp_set_sums(self._h, C.byref(s)))

    def set_robust_loss(self, loss, scale=1.0):
        """M-estimator weights for the PAPER / PLANE / GICP / P2P loop (LOSS_* or its name); takes effect at the next pass"""
        self._chk(self._L.symmicp_set_robust_loss(self._h, loss_code(loss), float(scale)))

    def robust_loss(self):
        """-> (loss, scale)"""
        lo, sc = C.c_int(0), C.c_float(0)
        self._chk(self._L.symmicp_get_robust_loss(self._h, C.byref(lo), C.byref(sc)))
        return lo.value, sc.value

    def set_gicp_epsilon(self, eps):
        """the eps of MODE_GICP's covariances I - (1 - eps) n n^T (0 < eps <= 1 with 1 - eps != 1 in fp32, i.e. eps > 2^-25;
        default 1e-3); takes effect at the next pass"""
        self._chk(self._L.symmicp_set_gicp_epsilon(self._h, float(eps)))

    def gicp_epsilon(self):
        ep = C.c_float(0)
        self._chk(self._L.symmicp_get_gicp_epsilon(self._h, C.byref(ep)))
        return ep.value

    def set_trim_fraction(self, fraction):
        """trimmed ICP: every pass keeps the closest `fraction` of its candidate pairs (0 < fraction <= 1; 1 = off, the default);
        takes effect at the next pass"""
        self._chk(self._L.symmicp_set_trim_fraction(self._h, float(fraction)))

    def trim_fraction(self):
        fr = C.c_float(0)
        self._chk(self._L.symmicp_get_trim_fraction(self._h, C.byref(fr)))
        return fr.value

    def set_color_weight(self, lam):
        """MODE_COLOR: the geometric rows weigh lam, the photometric ones 1 - lam (0 <= lam <= 1; default 0.968); takes effect at
        the next pass"""
        self._chk(self._L.symmicp_set_color_weight(self._h, float(lam)))

    def color_weight(self):
        lam = C.c_float(0)
        self._chk(self._L.symmicp_get_color_weight(self._h, C.byref(lam)))
        return lam.value

    def set_source_intensity(self, intensity):
        """MODE_COLOR: one scalar per source point, after set_source (a new set_source drops it)"""
        it = _scalar(intensity)
        self._chk(self._L.symmicp_set_source_intensity(self._h, _fptr(it), 1, it.shape[0]))

    def set_target_intensity(self, intensity, grad):
        """MODE_COLOR: one scalar and its tangent-plane gradient [N,3] (intensity_gradient) per target point, after set_target"""
        it = _scalar(intensity)
        g = _cloud(grad)
        if g.shape[0] != it.shape[0]:
            raise ValueError("one gradient per intensity expected")
        self._chk(self._L.symmicp_set_target_intensity(self._h, _fptr(it), 1, _fptr(g), 3, 1, it.shape[0]))

    def source_intensity(self):
        """the source's intensities as the engine holds them, read back in the caller's row order"""
        out = np.zeros(self.n_source, np.float32)
        self._chk(self._L.symmicp_get_source_intensity(self._h, _fptr(out), self.n_source))
        return out

    def intensity_gradient(self, xyz, nrm, intensity, k=10):
        """intensity_gradient on this context (symmicp_ctx_intensity_gradient); its target, source and index stay as they are"""
        xyz, nrm = _cloud(xyz), _cloud(nrm)
        n = xyz.shape[0]
        it = _scalar(intensity, n)
        g = np.zeros((n, 3), np.float32)
        self._chk(self._L.symmicp_ctx_intensity_gradient(self._h, _fptr(xyz), 3, 1, _fptr(nrm), 3, 1, _fptr(it), 1, n, k, _fptr(g)))
        return g

    def set_one_to_one(self, on):
        """one-to-one rejection: of the source points paired with one target point only the closest is kept (ties: the lowest row);
        takes effect at the next pass"""
        self._chk(self._L.symmicp_set_one_to_one(self._h, 1 if on else 0))

    def one_to_one(self):
        on = C.c_int(0)
        self._chk(self._L.symmicp_get_one_to_one(self._h, C.byref(on)))
        return bool(on.value)

    def set_reciprocal(self, on):
        """reciprocal correspondences: a pair (p, q) is kept only if p is also the nearest source point of q (implies one-to-one);
        takes effect at the next pass"""
        self._chk(self._L.symmicp_set_reciprocal(self._h, 1 if on else 0))

    def get_reciprocal(self):
        on = C.c_int(0)
        self._chk(self._L.symmicp_get_reciprocal(self._h, C.byref(on)))
        return bool(on.value)

    def reciprocal_state(self):
        """-> (n_u = claimed targets, n_r = reciprocal survivors) of the most recent pass; ERR_STATE if it was not reciprocal"""
        nu, nr = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.symmicp_get_reciprocal_state(self._h, C.byref(nu), C.byref(nr)))
        return nu.value, nr.value

    def set_median_factor(self, factor):
        """median-distance rejection: every pass keeps the pairs with d <= factor x the median pair distance (0 = off, the default);
        takes effect at the next pass"""
        self._chk(self._L.symmicp_set_median_factor(self._h, float(factor)))

    def median_factor(self):
        f = C.c_float(0)
        self._chk(self._L.symmicp_get_median_factor(self._h, C.byref(f)))
        return f.value

    def rejection_state(self):
        """-> (n_c, n_u, kept, tau_d2 as np.float32) of the most recent pass; ERR_STATE if it ran neither one-to-one nor the median"""
        nc, nu, kept, tau = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_float(0)
        self._chk(self._L.symmicp_get_rejection_state(self._h, C.byref(nc), C.byref(nu), C.byref(kept), C.byref(tau)))
        return nc.value, nu.value, kept.value, np.float32(tau.value)

    def trim_state(self):
        """-> (candidates, kept, tau_d2 as np.float32) of the most recent pass; ERR_STATE if it was not trimmed"""
        nc, kept, tau = C.c_uint64(0), C.c_uint64(0), C.c_float(0)
        self._chk(self._L.symmicp_get_trim_state(self._h, C.byref(nc), C.byref(kept), C.byref(tau)))
        return nc.value, kept.value, np.float32(tau.value)

    def set_source(self, xyz, nrm):
        """nrm may be None in MODE_PLANE (the library holds zero source normals then)"""
        xyz = _cloud(xyz)
        nrm = None if nrm is None else _cloud(nrm)
        self._chk(self._L.symmicp_set_source(self._h, _fptr(xyz), 3, 1, None if nrm is None else _fptr(nrm), 3, 1, xyz.shape[0]))
        self.n_source = xyz.shape[0]

    def set_target(self, xyz, nrm):
        """nrm may be None in MODE_NDT (the target's voxel map needs no normals)"""
        xyz = _cloud(xyz)
        nrm = None if nrm is None else _cloud(nrm)
        self._chk(self._L.symmicp_set_target(self._h, _fptr(xyz), 3, 1, None if nrm is None else _fptr(nrm), 3, 1, xyz.shape[0]))
        self.n_target = xyz.shape[0]

    def set_ndt(self, resolution=1.0, min_points=6, eig_ratio=0.01, outlier_ratio=0.55, neighbors=7):
        """the parameters of MODE_NDT (symmicp_set_ndt); on an NDT context that holds a target the map is rebuilt at once"""
        cfg = ndt_config(resolution, min_points, eig_ratio, outlier_ratio, neighbors)
        self._chk(self._L.symmicp_set_ndt(self._h, C.byref(cfg)))

    def get_ndt(self):
        """-> dict(resolution, min_points, eig_ratio, outlier_ratio, neighbors)"""
        cfg = NdtConfig()
        self._chk(self._L.symmicp_get_ndt(self._h, C.byref(cfg)))
        return dict(resolution=cfg.resolution, min_points=cfg.min_points, eig_ratio=cfg.eig_ratio, outlier_ratio=cfg.outlier_ratio,
                    neighbors=cfg.neighbors)

    def ndt_map(self, xyz, resolution, min_points=6, eig_ratio=0.01, outlier_ratio=0.55, neighbors=7):
        """ndt_map on this context (symmicp_ctx_ndt_map); its clouds, index, map and loop state stay as they are"""
        st, r, _ = self.ndt_map_raw(xyz, ndt_config(resolution, min_points, eig_ratio, outlier_ratio, neighbors))
        self._chk(st)
        return r

    def ndt_map_raw(self, xyz, cfg, cap=None, strides=None, want=True):
        """-> (status, map or None, m): the call as it is (tests of the cap protocol, the strides and the refusals)"""
        return _ndt_map(self._L.symmicp_ctx_ndt_map, (self._h,), xyz, cfg, cap, strides, want)

    def get_ndt_map(self, cap=None):
        """the map an NDT context holds after set_target (symmicp_get_ndt_map), as ndt_map returns it"""
        if cap is None:
            st, _, m = _ndt_map_call(self._L.symmicp_get_ndt_map, (self._h,), 0, want=False)
            if st not in (OK, ERR_SIZE):
                self._chk(st)
            cap = m
        st, r, _ = _ndt_map_call(self._L.symmicp_get_ndt_map, (self._h,), cap)
        self._chk(st)
        return r

    def ndt_state(self):
        """-> (score, items) of the most recent pass of an NDT context: -d1 x the sum of the weights, the number of (point, voxel) items"""
        sc, it = C.c_double(0), C.c_uint64(0)
        self._chk(self._L.symmicp_get_ndt_state(self._h, C.byref(sc), C.byref(it)))
        return sc.value, it.value

    def set_source_strided(self, xyz, xr, xc, nrm, nr, nc, n):
        self._chk(self._L.symmicp_set_source(self._h, _fptr(xyz), xr, xc, _fptr(nrm), nr, nc, n))
        self.n_source = n

    def set_target_strided(self, xyz, xr, xc, nrm, nr, nc, n):
        self._chk(self._L.symmicp_set_target(self._h, _fptr(xyz), xr, xc, _fptr(nrm), nr, nc, n))
        self.n_target = n

    @staticmethod
    def _guess(guess):
        if guess is None:
            return None, None
        g = np.ascontiguousarray(np.asarray(guess, np.float32).reshape(16))
        return g, _fptr(g)

    def _iter_dict(self, it):
        return dict(status=it.status, iter=it.iter, diff=it.diff, rcond=it.rcond, pairs=it.pairs,
                    increment=np.array(it.increment, np.float32).reshape(4, 4), sums=np.array(it.sums.s, np.float64))

    def begin(self, guess=None):
        g, gp = self._guess(guess)
        it = IterResult()
        self._chk(self._L.symmicp_begin(self._h, gp, C.byref(it)))
        return self._iter_dict(it)

    def step(self, check=True):
        it = IterResult()
        st = self._L.symmicp_step(self._h, C.byref(it))
        if check:
            self._chk(st)
        return self._iter_dict(it)

    def step_raw(self, it):
        """hot-loop variant: caller-provided IterResult, returns the status only"""
        return self._L.symmicp_step(self._h, C.byref(it))

    def align(self, guess=None, check=False):
        g, gp = self._guess(guess)
        res = Result()
        st = self._L.symmicp_align(self._h, gp, C.byref(res))
        if check:
            self._chk(st)
        n = max(0, min(res.iters, 64))
        return dict(status=st, iters=res.iters, diff_initial=res.diff_initial, diff_final=res.diff_final,
                    transform=np.frombuffer(res.transform, np.float32).reshape(4, 4).copy(),      # (frombuffer: no per-element conversion)
                    diffs=np.frombuffer(res.diffs, np.float32)[:n].copy(), seconds=res.seconds_total,
                    error=(self._L.symmicp_last_error(self._h) or b"").decode() if st != OK else "")

    def certificates(self):
        """diagnostic: (cert [n_loc, 4], neighbourhood members [n_loc, 8] as target rows, neighbourhood radius T [n_loc],
        winner row [n_loc]) of this rank's share, in its sorted order"""
        n = self.local_count()
        ce = np.zeros((n, 4), np.float32)
        hood = np.zeros((n, 8), np.uint32)
        T = np.zeros(n, np.float32)
        win = np.zeros(n, np.int32)
        self._chk(self._L.symmicp_get_certificates(self._h, _fptr(ce), hood.ctypes.data_as(C.POINTER(C.c_uint32)), _fptr(T),
                                                   win.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(n)))
        return ce, hood, T, win

    def transform(self):
        X = np.zeros(16, np.float32)
        self._chk(self._L.symmicp_get_transform(self._h, _fptr(X)))
        return X.reshape(4, 4)

    def pivot(self):
        p = np.zeros(3, np.float32)
        self._chk(self._L.symmicp_get_pivot(self._h, _fptr(p)))
        return p

    def local_count(self):
        return int(self._L.symmicp_local_source_count(self._h))

    def local_offset(self):
        return int(self._L.symmicp_local_source_offset(self._h))

    def correspondences(self):
        n = self.n_source
        idx = np.full(n, -1, np.int32)
        d2 = np.zeros(n, np.float32)
        self._chk(self._L.symmicp_get_correspondences(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(d2), n))
        return idx, d2

    def source(self):
        n = self.n_source
        xyz = np.zeros((n, 3), np.float32)
        nrm = np.zeros((n, 3), np.float32)
        self._chk(self._L.symmicp_get_source(self._h, _fptr(xyz), _fptr(nrm), n))
        return xyz, nrm

    def estimate_normals(self, xyz, k=10, viewpoint=(0.0, 0.0, 0.0)):
        """estimate_normals on this context (symmicp_ctx_estimate_normals); its target and source stay as they are"""
        xyz = _cloud(xyz)
        return self.estimate_normals_strided(xyz, 3, 1, xyz.shape[0], k, viewpoint)

    def estimate_normals_strided(self, buf, row_stride, col_stride, n, k=10, viewpoint=(0.0, 0.0, 0.0)):
        """as estimate_normals, the cloud read from the f32 array `buf` as xyz[i][c] = buf.flat[i * row_stride + c * col_stride]"""
        buf = np.ascontiguousarray(buf, np.float32)
        nrm = np.zeros((n, 3), np.float32)
        curv = np.zeros(n, np.float32)
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32)
        self._chk(self._L.symmicp_ctx_estimate_normals(self._h, _fptr(buf), row_stride, col_stride, n, k,
                                                       None if vp is None else _fptr(vp), _fptr(nrm), _fptr(curv)))
        return nrm, curv

    def knn(self, xyz, k=10):
        """symmicp_ctx_knn: -> (rows [N,k] int32, d2 [N,k] f32), each point's k nearest points of the same cloud in ascending (d2, row)"""
        xyz = _cloud(xyz)
        n = xyz.shape[0]
        rows = np.zeros((n, k), np.int32)
        d2 = np.zeros((n, k), np.float32)
        self._chk(self._L.symmicp_ctx_knn(self._h, _fptr(xyz), 3, 1, n, k, rows.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(d2)))
        return rows, d2

    def voxel_downsample(self, xyz, leaf, nrm=None, min_points=1):
        """voxel_downsample on this context (symmicp_ctx_voxel_downsample); its target, source and index stay as they are"""
        st, r, _ = _voxel_call(self._L.symmicp_ctx_voxel_downsample, (self._h,), xyz, nrm, leaf, min_points)
        self._chk(st)
        return r

    def voxel_downsample_raw(self, xyz, leaf, nrm=None, min_points=1, cap=None, strides=None):
        """the C call as it is: -> (status, result dict or None, n_out); cap defaults to N, strides as in _voxel_call"""
        return _voxel_call(self._L.symmicp_ctx_voxel_downsample, (self._h,), xyz, nrm, leaf, min_points, cap, strides)

    def radius_search(self, xyz, radius, sort=True):
        """radius_search on this context (symmicp_ctx_radius_search, both calls of the cap protocol) -> (count, offsets, rows, d2);
        its target, source and index stay as they are"""
        st, r = _radius_search(self._L.symmicp_ctx_radius_search, (self._h,), xyz, radius, sort)
        self._chk(st)
        return r

    def radius_search_raw(self, xyz, radius, cap=None, strides=None, want_d2=True):
        """the C call as it is -> (status, count, offsets, rows or None, d2 or None, total); cap None: counts only (rows_out NULL);
        strides = (n, row stride, col stride) over a flat f32 buffer"""
        return _radius_call(self._L.symmicp_ctx_radius_search, (self._h,), xyz, radius, cap, strides, want_d2)

    def fpfh(self, xyz, nrm, radius, want_spfh=False):
        """fpfh on this context (symmicp_ctx_fpfh) -> fpfh [N,33], or with want_spfh dict(fpfh=, spfh=, count=)"""
        st, f, s, k = _fpfh_call(self._L.symmicp_ctx_fpfh, (self._h,), xyz, nrm, radius, want_spfh)
        self._chk(st)
        return dict(fpfh=f, spfh=s, count=k) if want_spfh else f

    def fpfh_strided(self, xyz, nrm, radius, strides, want_spfh=True):
        """as fpfh(want_spfh=True), the clouds read from flat f32 buffers: strides = (n, xyz row, xyz col, nrm row, nrm col)"""
        st, f, s, k = _fpfh_call(self._L.symmicp_ctx_fpfh, (self._h,), xyz, nrm, radius, want_spfh, strides)
        self._chk(st)
        return dict(fpfh=f, spfh=s, count=k)

    def iss_keypoints(self, xyz, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5, return_saliency=False):
        """iss_keypoints on this context (symmicp_ctx_iss_keypoints, one call with cap = n)"""
        cfg = iss_config(salient_radius, non_max_radius, gamma21, gamma32, min_neighbors)
        st, r = _iss_keypoints(self._L.symmicp_ctx_iss_keypoints, (self._h,), xyz, cfg, return_saliency)
        self._chk(st)
        return r

    def iss_keypoints_raw(self, xyz, cfg, cap=None, strides=None):
        """one call of symmicp_ctx_iss_keypoints with a caller-chosen cap (None: rows_out == NULL) -> (status, rows, count, saliency,
        neighbors); nothing is raised"""
        return _iss_call(self._L.symmicp_ctx_iss_keypoints, (self._h,), xyz, cfg, cap, strides)

    def remove_statistical_outlier(self, xyz, k=20, std_mul=2.0, return_stats=False):
        """remove_statistical_outlier on this context (symmicp_ctx_statistical_outlier_removal, one call with cap = n)"""
        st, r = _remove_statistical_outlier(self._L.symmicp_ctx_statistical_outlier_removal, (self._h,), xyz, k, std_mul, return_stats)
        self._chk(st)
        return r

    def remove_statistical_outlier_raw(self, xyz, k, std_mul, cap=None, strides=None):
        """one call of symmicp_ctx_statistical_outlier_removal with a caller-chosen cap (None: rows_out == NULL) -> (status, rows, count,
        mean_dist, stats); nothing is raised"""
        return _sor_call(self._L.symmicp_ctx_statistical_outlier_removal, (self._h,), xyz, k, std_mul, cap, strides)

    def remove_radius_outlier(self, xyz, radius, min_neighbors, return_counts=False):
        """remove_radius_outlier on this context (symmicp_ctx_radius_outlier_removal, one call with cap = n)"""
        st, r = _remove_radius_outlier(self._L.symmicp_ctx_radius_outlier_removal, (self._h,), xyz, radius, min_neighbors, return_counts)
        self._chk(st)
        return r

    def cluster_dbscan(self, xyz, eps, min_points=1, min_cluster_size=0, max_cluster_size=0, return_info=False):
        """cluster_dbscan on this context (symmicp_ctx_cluster, one call with cap = n)"""
        cfg = cluster_config(eps, min_points, min_cluster_size, max_cluster_size)
        st, r = _cluster_dbscan(self._L.symmicp_ctx_cluster, (self._h,), xyz, cfg, return_info)
        self._chk(st)
        return r

    def orient_normals(self, xyz, nrm, k=16, viewpoint=None, direction=None, return_info=False):
        """orient_normals on this context (symmicp_ctx_orient_normals); its target, source and index stay as they are"""
        st, r = _orient_normals(self._L.symmicp_ctx_orient_normals, (self._h,), xyz, nrm, orient_config(k, viewpoint, direction), return_info)
        self._chk(st)
        return r

    def orient_normals_raw(self, xyz, nrm, cfg, strides=None, want=True):
        """one call of symmicp_ctx_orient_normals -> (status, normals, flip, component, tree, OrientResult)"""
        return _orient_call(self._L.symmicp_ctx_orient_normals, (self._h,), xyz, nrm, cfg, strides, want)

    def cluster_dbscan_raw(self, xyz, cfg, cap=None, strides=None):
        """one call of symmicp_ctx_cluster with a caller-chosen cap (None: sizes_out == NULL) -> (status, labels, clusters, sizes, core,
        neighbors)"""
        return _cluster_call(self._L.symmicp_ctx_cluster, (self._h,), xyz, cfg, cap, strides)

    def region_growing(self, xyz, nrm, eps, smoothness_deg=30.0, curvature=None, curvature_threshold=0.05, min_region_size=0, max_region_size=0,
                       return_info=False):
        """region_growing on this context (symmicp_ctx_region_growing, one call with cap = n); its clouds and index stay as they are"""
        cfg = region_config(eps, smoothness_deg, curvature_threshold, min_region_size, max_region_size)
        st, r = _region_growing(self._L.symmicp_ctx_region_growing, (self._h,), xyz, nrm, curvature, cfg, return_info)
        self._chk(st)
        return r

    def region_growing_raw(self, xyz, nrm, curv, cfg, cap=None, strides=None, want=True):
        """one call of symmicp_ctx_region_growing with a caller-chosen cap (None: sizes_out == NULL) -> (status, labels, regions, sizes,
        seed, smooth); want=False passes NULL for seed_out and smooth_out"""
        return _region_call(self._L.symmicp_ctx_region_growing, (self._h,), xyz, nrm, curv, cfg, cap, strides, want)

    def segment_plane(self, xyz, max_dist, hypotheses=1000, seed=0, refits=1, min_inliers=3, axis=None, max_angle_deg=0.0, return_info=False,
                      check=True):
        """segment_plane on this context (symmicp_ctx_segment_plane, one call with cap = n).  check=False: (status, result) instead of
        raising."""
        cfg = plane_config(max_dist, hypotheses, seed, refits, min_inliers, axis, max_angle_deg)
        st, r = _segment_plane(self._L.symmicp_ctx_segment_plane, (self._h,), xyz, cfg, return_info)
        if not check:
            return st, r
        self._chk(st)
        return r

    def segment_plane_raw(self, xyz, cfg, cap=None, strides=None, want=True):
        """one call of symmicp_ctx_segment_plane with a caller-chosen cap (None: rows_out == NULL) -> (status, dict) of _plane_call"""
        return _plane_call(self._L.symmicp_ctx_segment_plane, (self._h,), xyz, cfg, cap, strides, want)

    def segment_planes(self, xyz, max_dist, max_planes, min_inliers, hypotheses=1000, seed=0, refits=1, axis=None, max_angle_deg=0.0):
        """segment_planes on this context"""
        one = lambda sub, cfg: _segment_plane(self._L.symmicp_ctx_segment_plane, (self._h,), sub, cfg, False)
        return _segment_planes(one, xyz, max_dist, max_planes, min_inliers, hypotheses, seed, refits, axis, max_angle_deg)

    def plane_hypotheses(self, xyz, cfg, strides=None):
        """test entry (symmicp_ctx_plane_hypotheses) -> dict(hyp [H,4] f32 = n, d about the pivot, hyp_status [H] uint8, pivot [3] f32)"""
        xyz, n, xr, xc = _outlier_cloud(xyz, strides)
        H = int(cfg.hypotheses)
        hyp, status, pivot = np.zeros((H, 4), np.float32), np.zeros(H, np.uint8), np.zeros(3, np.float32)
        self._chk(self._L.symmicp_ctx_plane_hypotheses(self._h, _fptr(xyz), xr, xc, n, C.byref(cfg), _fptr(hyp),
                                                       status.ctypes.data_as(C.POINTER(C.c_uint8)), _fptr(pivot)))
        return dict(hyp=hyp, hyp_status=status, pivot=pivot)

    def remove_radius_outlier_raw(self, xyz, radius, min_neighbors, cap=None, strides=None):
        """one call of symmicp_ctx_radius_outlier_removal with a caller-chosen cap (None: rows_out == NULL) -> (status, rows, count,
        neighbors); nothing is raised"""
        return _ror_call(self._L.symmicp_ctx_radius_outlier_removal, (self._h,), xyz, radius, min_neighbors, cap, strides)

    def feature_nn(self, fa, fb):
        """feature_nn on this context (symmicp_ctx_feature_nn) -> (nn, d2, second)"""
        st, nn, d2, sec = _feature_nn_call(self._L.symmicp_ctx_feature_nn, (self._h,), fa, fb)
        self._chk(st)
        return nn, d2, sec

    def feature_correspondences(self, fa, fb, mutual=True, max_ratio=0.0):
        """feature_correspondences on this context -> (pairs [count,2], d2 [count])"""
        st, pairs, d2, _ = _feature_corr_call(self._L.symmicp_ctx_feature_correspondences, (self._h,), fa, fb, mutual, max_ratio)
        self._chk(st)
        return pairs, d2

    def feature_correspondences_raw(self, fa, fb, mutual=True, max_ratio=0.0, cap=None):
        """the C call as it is -> (status, pairs or None, d2 or None, count)"""
        return _feature_corr_call(self._L.symmicp_ctx_feature_correspondences, (self._h,), fa, fb, mutual, max_ratio, cap)

    def ransac(self, src, tgt, pairs, max_dist, hypotheses=100000, seed=0, edge_ratio=0.9, refits=1, want_hypotheses=False, check=True):
        """ransac on this context (symmicp_ctx_ransac) -> the dict of symmicp.ransac; check=False returns it on failure too (status set)"""
        st, r = _ransac_call(self._L.symmicp_ctx_ransac, (self._h,), src, tgt, pairs, ransac_config(max_dist, hypotheses, seed, edge_ratio, refits),
                             want_hypotheses)
        if check:
            self._chk(st)
        return r

    def ransac_hypotheses(self, src, tgt, pairs, max_dist, hypotheses=100000, seed=0, edge_ratio=0.9):
        """test entry (symmicp_ctx_ransac_hypotheses): what the device computed for every hypothesis -> (hyp [H,12] f32 = R row-major
        then t about the pivots, status [H] uint8, pivots [2,3] f32 = cs, ct)"""
        src, tgt = _cloud(src), _cloud(tgt)
        pairs = np.ascontiguousarray(pairs, np.int32)
        cfg = ransac_config(max_dist, hypotheses, seed, edge_ratio, 0)
        H = int(hypotheses)
        hyp = np.zeros((H, 12), np.float32)
        status = np.zeros(H, np.uint8)
        piv = np.zeros(6, np.float32)
        self._chk(self._L.symmicp_ctx_ransac_hypotheses(self._h, _fptr(src), 3, 1, src.shape[0], _fptr(tgt), 3, 1, tgt.shape[0], _i32ptr(pairs),
                                                        pairs.shape[0], C.byref(cfg), _fptr(hyp), status.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                        _fptr(piv)))
        return hyp, status, piv.reshape(2, 3)

    def fgr(self, src, tgt, pairs, max_dist, iterations=64, decrease_every=4, division_factor=1.4, tuple_scale=0.95, max_tuples=1000,
            tuple_trials=0, seed=0, want_trace=False, check=True):
        """fgr on this context (symmicp_ctx_fgr) -> the dict of symmicp.fgr; check=False returns it on failure too (status set)"""
        st, r = _fgr_call(self._L.symmicp_ctx_fgr, (self._h,), src, tgt, pairs,
                          fgr_config(max_dist, iterations, decrease_every, division_factor, tuple_scale, max_tuples, tuple_trials, seed), want_trace)
        if check:
            self._chk(st)
        return r

    def fgr_pass(self, p, q, X, mu):
        """test entry (symmicp_ctx_fgr_pass): one pass of the FGR loop on pivoted points p, q [M,3] at X and mu, through the loop
        kernel's accumulation and reduction -> (record [40] f64, weights [M] f32)"""
        p, q = _cloud(p), _cloud(q)
        if p.shape != q.shape:
            raise ValueError("p and q must have the same shape")
        X = np.ascontiguousarray(X, np.float32).reshape(16)
        sums = np.zeros(40, np.float64)
        w = np.zeros(max(len(p), 1), np.float32)
        self._chk(self._L.symmicp_ctx_fgr_pass(self._h, _fptr(p), _fptr(q), len(p), _fptr(X), C.c_float(mu),
                                               sums.ctypes.data_as(C.POINTER(C.c_double)), _fptr(w)))
        return sums, w[:len(p)]

    def posegraph_optimize(self, poses, edges, max_dist=0.0, want_trace=False, check=True, **cfg):
        """posegraph_optimize on this context's stream and scratch arena (symmicp_ctx_posegraph_optimize): its clouds, index, options and
        states stay as they were; check=False returns the dict on failure too (status set)"""
        st, r = _posegraph_call(self._L.symmicp_ctx_posegraph_optimize, (self._h,), poses, edges, posegraph_config(max_dist, **cfg), want_trace)
        if check:
            self._chk(st)
        return r

    def posegraph_pass(self, poses, edges, reference_node, mu, lam, cg_tolerance=1e-10, cg_max_iterations=0):
        """test entry (symmicp_ctx_posegraph_pass): one launch of the iteration kernel at the given poses, mu and lambda ->
        dict(e [m,6], c [m], l [m], g [n,6], hdiag [n,6,6], delta [n,6], cost, cost_trial, cg_iterations, cg_residual, ...)"""
        X, m = _poses(poses), len(edges)
        E = pose_edges(edges)
        n = len(X)
        e, c, l = np.zeros((m, 6)), np.zeros(m), np.zeros(m)
        g, h, d = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6))
        rec = PosegraphIteration()
        self._chk(self._L.symmicp_ctx_posegraph_pass(self._h, _dptr(X), n, E, m, int(reference_node), float(mu), float(lam), float(cg_tolerance),
                                                     int(cg_max_iterations), _dptr(e), _dptr(c), _dptr(l), _dptr(g), _dptr(h), _dptr(d),
                                                     C.byref(rec)))
        r = _pg_iteration(rec)
        r.update(e=e, c=c, l=l, g=g, hdiag=h, delta=d)
        return r

    def batch_align(self, src, src_n, tgt, tgt_n, problems, guesses=None, trace=False, **cfg):
        """batch_align on this context's stream and scratch arena; its clouds, options and loop state stay as they are"""
        st, r = _batch_align(self._L.symmicp_ctx_batch_align, (self._h,), src, src_n, tgt, tgt_n, problems, guesses, trace, cfg)
        self._chk(st)
        return r

    def batch_align_raw(self, src, src_n, tgt, tgt_n, problems, guesses, cfg, trace=False):
        """the C call as it is, cfg a BatchConfig -> (status, results array, trace_X, trace_sums) (tests)"""
        return _batch_call(self._L.symmicp_ctx_batch_align, (self._h,), src, src_n, tgt, tgt_n, problems, guesses, cfg, trace)

    def evaluate_registration(self, src, tgt, transforms=None, max_dist=0.0, want_pairs=False):
        """evaluate_registration on this context's stream and temporary memory (symmicp_ctx_evaluate_registration): the context's clouds,
        index, certificates, options and states stay as they were"""
        args, ns, keep = _eval_clouds(src, tgt)
        st, r, single = _eval_call(self._L.symmicp_ctx_evaluate_registration, (self._h,), args, transforms, max_dist, want_pairs, ns)
        self._chk(st)
        return r[0] if single else r

    def evaluate_registration_raw(self, src, tgt, strides, transforms=None, max_dist=0.0, want_pairs=False):
        """the same on raw float32 buffers with strides = (src_row, src_col, ns, tgt_row, tgt_col, nt) -> (status, list of dicts or None)"""
        args, ns, keep = _eval_clouds(src, tgt, strides)
        st, r, _ = _eval_call(self._L.symmicp_ctx_evaluate_registration, (self._h,), args, transforms, max_dist, want_pairs, ns)
        return st, r

    def evaluate(self, transforms=None, max_dist=0.0, want_pairs=False):
        """the same function on the clouds this context holds (symmicp_evaluate): nothing is uploaded, the source is the one set_source
        received and every transform is applied to it as it is (not composed with the context's).  transforms None: the context's
        current cumulative transform, what transform() returns.  Rows are the caller's for both clouds.  The context stays as it was."""
        ns = int(self._L.symmicp_local_source_count(self._h))
        st, r, single = _eval_call(self._L.symmicp_evaluate, (self._h,), (), transforms, max_dist, want_pairs, ns)
        self._chk(st)
        return r[0] if single else r

    def align_multistart(self, src, src_n, tgt, tgt_n, guesses, **cfg):
        """one pair refined from every guess [B, 4, 4] in one batch -> one result dict per guess"""
        g = np.ascontiguousarray(guesses, np.float32).reshape(-1, 16)
        return self.batch_align(src, src_n, tgt, tgt_n, [(0, len(src), 0, len(tgt))] * len(g), g, **cfg)

    def enable_timing(self, on=True):
        self._chk(self._L.symmicp_enable_timing(self._h, int(on)))      # 0 off, 1 per pass, 2 per kernel

    def reset_stats(self):
        self._chk(self._L.symmicp_reset_stats(self._h))

    def stats(self):
        s = Stats()
        self._chk(self._L.symmicp_get_stats(self._h, C.byref(s)))
        d = {k: getattr(s, k) for k, _ in Stats._fields_}
        d["kernel_ms"] = list(s.kernel_ms)
        d["kernel_launches"] = list(s.kernel_launches)
        d["pass_ms_head"] = list(s.pass_ms_head)
        return d

    # ---- test entry points of the device-driven loop ----
    def solve_probe(self, mode, sums, exact_rc, pivot=None, X_in=None):
        """the device's solve_core.h on records sums [n,40] (one thread each) -> dict of status [n], pbar qbar a t [n,3],
        rcond [n], out16 [n,4,4] and, with X_in [n,4,4], X_out = out16 @ X_in as the device loop composes it (mat4_mul)"""
        S = np.ascontiguousarray(np.asarray(sums, np.float64).reshape(-1, NSUM))
        n = S.shape[0]
        o = dict(status=np.zeros(n, np.int32), pbar=np.zeros((n, 3), np.float32), qbar=np.zeros((n, 3), np.float32),
                 a=np.zeros((n, 3), np.float32), t=np.zeros((n, 3), np.float32), rcond=np.zeros(n, np.float32),
                 out16=np.zeros((n, 4, 4), np.float32))
        pv = None if pivot is None else _fptr(np.ascontiguousarray(pivot, np.float32))
        xin = xout = None
        if X_in is not None:
            X_in = np.ascontiguousarray(np.asarray(X_in, np.float32).reshape(n, 4, 4))
            o["X_out"] = np.zeros((n, 4, 4), np.float32)
            xin, xout = _fptr(X_in), _fptr(o["X_out"])
        self._chk(self._L.symmicp_ctx_solve_probe(self._h, int(mode), int(bool(exact_rc)), S.ctypes.data_as(C.POINTER(Sums)), n, pv, xin,
                                                  o["status"].ctypes.data_as(C.POINTER(C.c_int32)), _fptr(o["pbar"]), _fptr(o["qbar"]),
                                                  _fptr(o["a"]), _fptr(o["t"]), _fptr(o["rcond"]), _fptr(o["out16"]), xout))
        return o

    def loop_solve(self, mode, sums, X_in=None, pivot=None, diff_threshold=1.0, fixed_iters=0, max_iters=10, iters=0, small_step=0,
                   eps_rotation=0.0, eps_translation=0.0, incremental=0):
        """one solve-only launch of the device loop's end-of-pass kernel on record `sums` and the given loop state -> dict of stop,
        reason, iters, small_step, X [4,4], Xapply [3,4] and the ring record it wrote: ring_increment, ring_X [4,4], ring_rcond,
        ring_status, ring_solved (unwritten: 0xFF bytes, i.e. NaN floats and -1 integers)"""
        S = Sums()
        for k, v in enumerate(np.asarray(sums, np.float64).reshape(NSUM)):
            S.s[k] = v
        X_in = np.ascontiguousarray(np.eye(4, dtype=np.float32) if X_in is None else np.asarray(X_in, np.float32).reshape(16))
        pv = None if pivot is None else _fptr(np.ascontiguousarray(pivot, np.float32))
        ii = np.array([mode, fixed_iters, max_iters, iters, small_step, incremental], np.int32)
        ff = np.array([diff_threshold, eps_rotation, eps_translation], np.float32)
        st = np.zeros(4, np.int32); X = np.zeros(16, np.float32); Xa = np.zeros(12, np.float32)
        ri = np.zeros(16, np.float32); rX = np.zeros(16, np.float32); rrc = np.zeros(1, np.float32); r2 = np.zeros(2, np.int32)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._chk(self._L.symmicp_ctx_loop_solve(self._h, C.byref(S), pv, _fptr(X_in), i32(ii), _fptr(ff), i32(st), _fptr(X), _fptr(Xa),
                                                 _fptr(ri), _fptr(rX), _fptr(rrc), i32(r2)))
        return dict(stop=int(st[0]), reason=int(st[1]), iters=int(st[2]), small_step=int(st[3]), X=X.reshape(4, 4), Xapply=Xa.reshape(3, 4),
                    ring_increment=ri.reshape(4, 4), ring_X=rX.reshape(4, 4), ring_rcond=float(rrc[0]), ring_status=int(r2[0]), ring_solved=int(r2[1]))

    # ---- test entry points of the index build (read-only) ----
    def index_info(self):
        """symmicp_ctx_index_info -> dict of the target index's scalars (arrays as numpy)"""
        o = IndexInfo()
        o.struct_size = C.sizeof(IndexInfo)
        self._chk(self._L.symmicp_ctx_index_info(self._h, C.byref(o)))
        d = {k: getattr(o, k) for k, _ in IndexInfo._fields_ if k != "struct_size"}
        d["origin"] = np.array(o.origin, np.float32)
        for k in ("h0", "h", "inv_h"):
            d[k] = np.float32(d[k])
        d["level_off"] = np.array(o.level_off, np.uint32)
        d["olevel_off"] = np.array(o.olevel_off, np.uint32)
        d["level_hist"] = np.array(o.level_hist, np.uint32)
        d["surface_like"] = bool(o.surface_like)
        return d

    def index_arrays(self):
        """symmicp_ctx_index_info + symmicp_ctx_index_arrays -> the info dict plus tq [n,4], tn [n,2,4], boxes [n_boxes,2,4], onodes
        [n_onodes,2,4] (f32; integer words keep their bits: view them as uint32), ctop [ctop_len] and cells [n_blocks * 512, 2] (uint32)"""
        d = self.index_info()
        gl = d["grid_level"] > 0
        d["tq"] = np.zeros((d["n"], 4), np.float32)
        d["tn"] = np.zeros((d["n"], 2, 4), np.float32)
        d["boxes"] = np.zeros((d["n_boxes"], 2, 4), np.float32)
        d["ctop"] = np.zeros(d["ctop_len"] if gl else 0, np.uint32)
        d["cells"] = np.zeros(((d["n_blocks"] if gl else 0) * 512, 2), np.uint32)
        d["onodes"] = np.zeros((d["n_onodes"], 2, 4), np.float32)
        u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)) if a.size else None
        self._chk(self._L.symmicp_ctx_index_arrays(self._h, _fptr(d["tq"]), _fptr(d["tn"]), _fptr(d["boxes"]), u32(d["ctop"]), u32(d["cells"]),
                                                   _fptr(d["onodes"])))
        return d

    def source_share(self):
        """symmicp_ctx_source_share -> dict(n_local, pkt_count, sorted, cost_keyed, order [n_local] uint32 or None, pkt_tab [pkt_count,2])"""
        nl, npk, so, ck = C.c_size_t(0), C.c_size_t(0), C.c_int32(0), C.c_int32(0)
        self._chk(self._L.symmicp_ctx_source_share(self._h, C.byref(nl), C.byref(npk), C.byref(so), C.byref(ck), None, None))
        order = np.zeros(nl.value, np.uint32) if so.value else None
        tab = np.zeros((npk.value, 2), np.uint32)
        u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)) if a is not None and a.size else None
        self._chk(self._L.symmicp_ctx_source_share(self._h, None, None, None, None, u32(order), u32(tab)))
        return dict(n_local=nl.value, pkt_count=npk.value, sorted=bool(so.value), cost_keyed=bool(ck.value), order=order, pkt_tab=tab)

    def radix_sort_probe(self, keys, vals, key_bits):
        """the build's radix sort on host arrays (symmicp_ctx_radix_sort_probe) -> (keys, vals) sorted, as new uint32 arrays"""
        k = np.array(keys, np.uint32).reshape(-1)
        v = np.array(vals, np.uint32).reshape(-1)
        if k.shape != v.shape:
            raise ValueError("keys and vals differ in length")
        u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        self._chk(self._L.symmicp_ctx_radix_sort_probe(self._h, u32(k), u32(v), k.size, int(key_bits)))
        return k, v

    def select_probe(self, keys, k):
        """the trimmed pass's radix select on a host array (symmicp_ctx_select_probe) -> (the k-th smallest key, 1 <= k <= n; the
        number of keys <= it)"""
        a = np.ascontiguousarray(np.asarray(keys, np.uint32).reshape(-1))
        kth, nle = C.c_uint32(0), C.c_uint64(0)
        self._chk(self._L.symmicp_ctx_select_probe(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size, int(k), C.byref(kth), C.byref(nle)))
        return kth.value, nle.value

    def unique_probe(self, tgt_row, d2_bits, n_t):
        """the one-to-one claim on host arrays (symmicp_ctx_unique_probe): row i claims target row tgt_row[i] (< 0: no pair) with the
        key (d2_bits[i] << 32 | i) -> bool array, True where row i wins its target"""
        r = np.ascontiguousarray(np.asarray(tgt_row, np.int32).reshape(-1))
        d = np.ascontiguousarray(np.asarray(d2_bits, np.uint32).reshape(-1))
        if r.size != d.size:
            raise ValueError("unique_probe: tgt_row and d2_bits differ in length")
        w = np.zeros(r.size, np.uint8)
        self._chk(self._L.symmicp_ctx_unique_probe(self._h, r.ctypes.data_as(C.POINTER(C.c_int32)), d.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                   r.size, int(n_t), w.ctypes.data_as(C.POINTER(C.c_uint8))))
        return w.astype(bool)

    def reverse_nn_probe(self, db, queries, labels=None, X=None):
        """the reverse search of a reciprocal pass on host arrays (symmicp_ctx_reverse_nn_probe): the index over db relabelled with
        `labels` (distinct, < 2^31; None: the row), the queries carried through inverse_rigid(X) (None: identity)
        -> (label of the nearest db point, ties to the lowest label: int32 [n_q]; its fp32 d2 [n_q])"""
        d, q = _cloud(db), _cloud(queries)
        lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
        if lab is not None and lab.size != d.shape[0]:
            raise ValueError("reverse_nn_probe: one label per db point")
        Xa = None if X is None else np.ascontiguousarray(np.asarray(X, np.float32).reshape(16))
        out = np.zeros(q.shape[0], np.int32)
        d2 = np.zeros(q.shape[0], np.float32)
        self._chk(self._L.symmicp_ctx_reverse_nn_probe(self._h, _fptr(d), None if lab is None else lab.ctypes.data_as(C.POINTER(C.c_int32)), d.shape[0],
                                                       _fptr(q), q.shape[0], None if Xa is None else _fptr(Xa),
                                                       out.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(d2)))
        return out, d2

    def reciprocal_info(self):
        """what reciprocal correspondences hold on this context (symmicp_ctx_reciprocal_info) -> dict(index_valid, index_bytes,
        index_builds, table_words)"""
        v, b, n, t = C.c_int32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.symmicp_ctx_reciprocal_info(self._h, C.byref(v), C.byref(b), C.byref(n), C.byref(t)))
        return dict(index_valid=bool(v.value), index_bytes=b.value, index_builds=n.value, table_words=t.value)

    def scan_probe(self, data):
        """the build's exclusive scan on a host array (symmicp_ctx_scan_probe) -> new uint32 array"""
        d = np.array(data, np.uint32).reshape(-1)
        self._chk(self._L.symmicp_ctx_scan_probe(self._h, d.ctypes.data_as(C.POINTER(C.c_uint32)), d.size))
        return d

    def set_loop_log(self, on=True):
        self._chk(self._L.symmicp_set_loop_log(self._h, int(bool(on))))

    def loop_log(self):
        """the device-driven passes of the last align (set_loop_log first): a list of dicts, one per pass"""
        n = C.c_size_t(0)
        self._chk(self._L.symmicp_get_loop_log(self._h, None, 0, C.byref(n)))
        buf = (LoopLogEntry * max(1, n.value))()
        self._chk(self._L.symmicp_get_loop_log(self._h, buf, n.value, C.byref(n)))
        out = []
        for e in buf[:n.value]:
            out.append(dict(sums=np.array(e.sums[:], np.float64), increment=np.array(e.increment[:], np.float32).reshape(4, 4),
                            X=np.array(e.X[:], np.float32).reshape(4, 4), rcond=e.rcond, iter=e.iter, status=e.status, solved=e.solved,
                            list_len=e.list_len, reason=e.reason, batch=e.batch,
                            # the pass's kernel (0: fused, 1: certified-only); on a batch's last entry: the pass behind it ran
                            # certified-only and was handed back to the host incomplete
                            kernel=e.reserved & 0xff, redo_certified=bool(e.reserved & 0x100)))
        return out


class MyICP:
    """Python mirror of the reference's MyICP (ICP/myicp.h:7-36).

    LoadCloud / GetSrcCloud / GetTgtCloud / RegisterSymm keep the reference's names and
    behaviour (defaults max_iters=10, diff_threshold=1.0, identity pairing, QUIRKS arithmetic,
    result printed).  setInputSource / setInputTarget / align / getFinalTransformation are the
    additive surface BASELINE.json's north_star names.
    """

    def __init__(self, mode=MODE_QUIRKS, corr=CORR_IDENTITY, max_iters=10, diff_threshold=1.0, verbose=True, **extra):
        self._cfg = dict(mode=mode, corr=corr, max_iters=max_iters, diff_threshold=diff_threshold,
                         verbose=int(bool(verbose)), **extra)
        self.cloud_src = self.cloud_tgt = None
        self.normals_src = self.normals_tgt = None
        self._final = np.eye(4, dtype=np.float32)
        self.last_result = None
        self._loss = (LOSS_NONE, 0.0)
        self._gicp_eps = None
        self._trim = 1.0
        self._one_to_one = False
        self._reciprocal = False
        self._median = 0.0
        self._color_weight = None
        self.intensity_src = self.intensity_tgt = None
        self._levels = []
        self._ndt = dict(resolution=1.0, neighbors=7, min_points=6)
        self._ndt_levels = []
        self.level_results = []
        self._global = None
        self.global_result = None
        self._have_src = self._have_tgt = False         # normals supplied by the caller through setInput* (not estimated here)
        self.multistart_results = []
        self._removed = (0, 0)
        self._planes = (np.zeros(4), np.zeros(4))
        self._orient_k = 0

    def setOrientNormals(self, k):
        """consistent normal orientation (orient_normals; 0, the default: off): the normals pre-step of each cloud is followed by the
        orientation over the k-NN graph, viewpoint at the origin.  Applies to normals the class estimates itself, never to supplied
        ones; an out-of-range k raises ERR_ARG from align()."""
        self._orient_k = int(k)

    def alignMultiStart(self, guesses):
        """one batch on the object's clouds, a problem per guess [B, 4, 4] (Engine.align_multistart with the object's mode, max_iters,
        diff_threshold, max_corr_dist, fixed_iters, min_normal_dot and eps rule; normals estimated as align does).  Adopts as final
        transformation the result with status OK and the most pairs -- ties to the smaller diff_final, then the lowest index -- and
        returns its index (-1: no problem ended OK; the final transformation stays).  Clouds above BATCH_MAX_POINTS points or a mode
        other than PAPER, P2P and PLANE raise the batch call's error: there is no fallback to a loop."""
        assert self.cloud_src is not None and self.cloud_tgt is not None
        keys = ("mode", "max_iters", "diff_threshold", "max_corr_dist", "fixed_iters", "min_normal_dot", "eps_rotation", "eps_translation")
        cfg = {k: self._cfg[k] for k in keys if k in self._cfg}
        batch_config(**cfg)
        g = np.ascontiguousarray(guesses, np.float32).reshape(-1, 16)
        if self._cfg["mode"] in (MODE_PAPER, MODE_P2P, MODE_PLANE) and max(len(self.cloud_src), len(self.cloud_tgt)) <= BATCH_MAX_POINTS and len(g):
            self.estimateNormals()
        else:      # (the call refuses: no normals are estimated for it)
            z = np.zeros_like
            st, _ = _batch_align(lib().symmicp_batch_align, (int(self._cfg.get("device", -1)),), self.cloud_src, z(self.cloud_src), self.cloud_tgt,
                                 z(self.cloud_tgt), [(0, len(self.cloud_src), 0, len(self.cloud_tgt))] * len(g), g if len(g) else None, False, cfg)
            raise SymmIcpError(st if st != OK else ERR_ARG, "alignMultiStart")
        with Engine(**dict(self._cfg, verbose=0)) as e:
            self.multistart_results = e.align_multistart(self.cloud_src, self.normals_src, self.cloud_tgt, self.normals_tgt, g, **cfg)
        best = -1
        for k, r in enumerate(self.multistart_results):
            if r["status"] == OK and (best < 0 or (r["pairs"], -r["diff_final"]) > (self.multistart_results[best]["pairs"],
                                                                                   -self.multistart_results[best]["diff_final"])):
                best = k
        if best >= 0:
            self.last_result = self.multistart_results[best]
            self._final = self.last_result["transform"]
            if self._cfg["verbose"]:
                print(format_result(self._final), end="", flush=True)
        return best

    def evaluate(self, max_dist, transform=None):
        """fitness, inlier RMSE and information matrix of `transform` (None: the final transformation) on the object's full clouds at
        max_dist (evaluate_registration's dict; <= 0: every point counts)"""
        assert self.cloud_src is not None and self.cloud_tgt is not None
        X = self._final if transform is None else np.asarray(transform, np.float32).reshape(4, 4)
        return evaluate_registration(self.cloud_src, self.cloud_tgt, X, max_dist, device=int(self._cfg.get("device", -1)))

    def getFitnessScore(self, max_range=float(np.finfo(np.float64).max)):
        """PCL's getFitnessScore: the mean squared distance from the moved source points to their nearest target points, over those
        within max_range; the largest double when none is.  (max_range is rounded to fp32; the largest double means no limit.)"""
        d = float(np.float32(min(max_range, float(np.finfo(np.float32).max))))
        r = self.evaluate(0.0 if d >= float(np.finfo(np.float32).max) else d)
        return r["mean_d2"] if r["inliers"] > 0 else float(np.finfo(np.float64).max)

    def evaluateStarts(self, max_dist):
        """every multiStartResults() transform scored on the full clouds at one common distance, in one call: a list of
        evaluate_registration dicts in the order of the guesses ([] before an alignMultiStart)"""
        if not self.multistart_results:
            return []
        X = np.stack([r["transform"] for r in self.multistart_results])
        return evaluate_registration(self.cloud_src, self.cloud_tgt, X, max_dist, device=int(self._cfg.get("device", -1)))

    def multiStartResults(self):
        """every result of the last alignMultiStart, in the order of its guesses"""
        return self.multistart_results

    def setMaxCorrespondenceDistance(self, d):
        """pairs farther apart than d are dropped (Config.max_corr_dist; <= 0: every pair is kept)"""
        self._cfg["max_corr_dist"] = float(d)

    def setVoxelLevels(self, levels):
        """coarse-to-fine alignment: [(leaf, max_iters, max_corr_dist), ...], coarse first (leaf 0: the clouds as given).  align()
        then runs one alignment per level on both clouds voxel-downsampled with the level's leaf (normals averaged), each from the
        transform of the level before (the first from the caller's guess).  CORR_IDENTITY is refused (ERR_ARG), and so is MODE_COLOR
        (intensities are not averaged per voxel yet).  [] = off."""
        levels = [(float(l), int(i), float(d)) for l, i, d in levels]
        if levels and self._cfg["mode"] == MODE_COLOR:
            raise SymmIcpError(ERR_ARG, "MODE_COLOR does not run voxel levels (intensities are not averaged per voxel yet)")
        self._levels = levels

    def setNdt(self, resolution, neighbors=7, min_points=6):
        """the parameters of MODE_NDT (Engine.set_ndt): the voxel edge, the neighbourhood (1 or 7) and the fewest points of a voxel"""
        self._ndt = dict(resolution=float(resolution), neighbors=int(neighbors), min_points=int(min_points))

    def setNdtLevels(self, levels):
        """coarse-to-fine NDT: [(resolution, max_iters), ...], coarse first.  align() in MODE_NDT then runs, per level, set_ndt with the
        level's resolution (the target's map is rebuilt at once) and an alignment of max_iters iterations started from the level
        before (the first from the caller's guess): bit for bit the transform of the same calls made by hand.  [] = off."""
        self._ndt_levels = [(float(r), int(i)) for r, i in levels]

    def _align_ndt(self, guess):
        """MODE_NDT: no normals are estimated, no index is built; the clouds go in as they are"""
        if self._levels or self._global is not None:
            raise SymmIcpError(ERR_ARG, "MODE_NDT runs neither voxel levels (setNdtLevels is its coarse-to-fine) nor the global initialisation")
        verbose = bool(self._cfg["verbose"])
        levels = self._ndt_levels or [(self._ndt["resolution"], self._cfg["max_iters"])]
        self.level_results = []
        K = len(levels)
        with Engine(**dict(self._cfg, verbose=0)) as e:
            if self._loss[0] != LOSS_NONE:
                e.set_robust_loss(*self._loss)
            if self._trim != 1.0:
                e.set_trim_fraction(self._trim)
            if self._one_to_one:
                e.set_one_to_one(True)
            if self._reciprocal:
                e.set_reciprocal(True)
            if self._median != 0.0:
                e.set_median_factor(self._median)
            e.set_ndt(**dict(self._ndt, resolution=levels[0][0]))
            e.set_target(self.cloud_tgt, None)
            e.set_source(self.cloud_src, None)
            X = guess
            for k, (res, iters) in enumerate(levels):
                if k:
                    e.set_ndt(**dict(self._ndt, resolution=res))
                if verbose and self._ndt_levels:
                    print("NDT level %d/%d: resolution %g, %d iterations" % (k + 1, K, res, iters), flush=True)
                e.set_config(max_iters=iters, verbose=int(verbose and k + 1 == K))
                r = e.align(X)
                self.level_results.append(r)
                if r["status"] != OK:
                    break
                X = r["transform"]
        self.last_result = r
        if r["status"] == OK or r["iters"] > 0:
            self._final = r["transform"]
        return r

    def setGlobalInit(self, fpfh_radius, max_dist, voxel_leaf=0.0, normal_k=10, hypotheses=100000, seed=0, mutual=True, max_ratio=0.0,
                      edge_ratio=0.9, refits=1, iss=False, iss_salient_radius=0.0, iss_non_max_radius=0.0, iss_gamma21=0.975, iss_gamma32=0.975,
                      iss_min_neighbors=5, method="ransac", fgr_iterations=64, fgr_division_factor=1.4, fgr_tuple_scale=0.95, fgr_max_tuples=1000,
                      orient_k=0):
        """global initialisation: with it set and no guess given, align() first voxel-downsamples both clouds with voxel_leaf (0: as
        given), estimates normals on the downsampled clouds when the caller supplied none (normal_k neighbours, viewpoint at the
        origin), computes FPFH features at fpfh_radius, their correspondences and a RANSAC transform, and starts the ordinary
        alignment (voxel levels included) from it.  A failure (ERR_NO_CONSENSUS among them) raises SymmIcpError.  FPFH matching
        needs normals oriented alike in both clouds: orient_k > 0 follows the estimate with orient_normals over the orient_k-NN graph
        (viewpoint at the origin; an out-of-range value raises ERR_ARG from align()).  With iss the features are still computed on the full (downsampled) clouds, but only
        the rows of their ISS keypoints (Engine.iss_keypoints with the iss_* values) are matched and given to RANSAC; fewer than 3
        keypoints in either cloud raises ERR_NO_CONSENSUS (no fall-back to the full cloud).  method "fgr" gives the correspondences to
        Fast Global Registration (Engine.fgr with max_dist, seed and the fgr_* values) instead of RANSAC, which is not run then; every
        other step is the same."""
        if method not in ("ransac", "fgr"):
            raise ValueError("method must be 'ransac' or 'fgr'")
        self._global = dict(fpfh_radius=float(fpfh_radius), max_dist=float(max_dist), voxel_leaf=float(voxel_leaf), normal_k=int(normal_k),
                            hypotheses=int(hypotheses), seed=int(seed), mutual=bool(mutual), max_ratio=float(max_ratio),
                            edge_ratio=float(edge_ratio), refits=int(refits), iss=bool(iss), iss_salient_radius=float(iss_salient_radius),
                            iss_non_max_radius=float(iss_non_max_radius), iss_gamma21=float(iss_gamma21), iss_gamma32=float(iss_gamma32),
                            iss_min_neighbors=int(iss_min_neighbors), method=method, fgr_iterations=int(fgr_iterations),
                            fgr_division_factor=float(fgr_division_factor), fgr_tuple_scale=float(fgr_tuple_scale),
                            fgr_max_tuples=int(fgr_max_tuples), orient_k=int(orient_k))

    def clearGlobalInit(self):
        self._global = None

    def globalResult(self):
        """the RANSAC (or, with method "fgr", the FGR) result dict of the last align() that ran the initialisation (plus method,
        correspondences, source_points, target_points)"""
        return self.global_result

    def _global_init(self, e):
        g = self._global
        clouds = []
        for xyz, nrm in ((self.cloud_src, self.normals_src if self._have_src else None),
                         (self.cloud_tgt, self.normals_tgt if self._have_tgt else None)):
            if g["voxel_leaf"] > 0:
                d = e.voxel_downsample(xyz, g["voxel_leaf"], nrm)
                xyz, nrm = d["xyz"], d["nrm"]
            if nrm is None:
                nrm, _ = e.estimate_normals(xyz, g["normal_k"])
                if g["orient_k"] != 0:
                    nrm = e.orient_normals(xyz, nrm, g["orient_k"])
            clouds.append((xyz, e.fpfh(xyz, nrm, g["fpfh_radius"])))
        (src, fs), (tgt, ft) = clouds
        kp = None
        if g["iss"]:
            try:
                kp = [e.iss_keypoints(x, g["iss_salient_radius"], g["iss_non_max_radius"], g["iss_gamma21"], g["iss_gamma32"], g["iss_min_neighbors"])
                      for x in (src, tgt)]
            except SymmIcpError as err:
                raise SymmIcpError(err.status, "global initialisation: ISS keypoints: " + (e._L.symmicp_last_error(e._h) or b"").decode())
            if min(len(kp[0]), len(kp[1])) < 3:
                raise SymmIcpError(ERR_NO_CONSENSUS, "global initialisation: ISS keypoints: fewer than 3 keypoints (%d in the source, %d in the target)"
                                   % (len(kp[0]), len(kp[1])))
            pairs, _ = e.feature_correspondences(fs[kp[0]], ft[kp[1]], g["mutual"], g["max_ratio"])
            pairs = np.stack([kp[0][pairs[:, 0]], kp[1][pairs[:, 1]]], 1).astype(np.int32)
        else:
            pairs, _ = e.feature_correspondences(fs, ft, g["mutual"], g["max_ratio"])
        if len(pairs) < 3:
            raise SymmIcpError(ERR_NO_CONSENSUS, "global initialisation: fewer than 3 feature correspondences")
        fgr = g["method"] == "fgr"
        if fgr:
            r = e.fgr(src, tgt, pairs, g["max_dist"], iterations=g["fgr_iterations"], division_factor=g["fgr_division_factor"],
                      tuple_scale=g["fgr_tuple_scale"], max_tuples=g["fgr_max_tuples"], seed=g["seed"], check=False)
        else:
            r = e.ransac(src, tgt, pairs, g["max_dist"], g["hypotheses"], g["seed"], g["edge_ratio"], g["refits"], check=False)
        r.update(method=g["method"])
        r.update(correspondences=len(pairs), source_points=len(src), target_points=len(tgt),
                 source_keypoints=0 if kp is None else len(kp[0]), target_keypoints=0 if kp is None else len(kp[1]))
        self.global_result = r
        if fgr:
            if self._cfg["verbose"]:
                print("global init: %d -> %d source and %d -> %d target points, %d and %d ISS keypoints, %d correspondences, FGR: %d tuples accepted, "
                      "%d set elements, %d iterations, %d inliers" % (len(self.cloud_src), len(src), len(self.cloud_tgt), len(tgt), r["source_keypoints"],
                                                                      r["target_keypoints"], len(pairs), r["tuples_accepted"], r["set_size"],
                                                                      r["iterations"], r["inliers"]), flush=True)
            if r["status"] != OK:
                raise SymmIcpError(r["status"], "global initialisation: FGR: " + (e._L.symmicp_last_error(e._h) or b"").decode())
            return r["transform"]
        if self._cfg["verbose"] and kp is not None:
            print("global init: %d -> %d source and %d -> %d target points, %d and %d ISS keypoints, %d correspondences, %d of %d hypotheses evaluated, "
                  "%d -> %d inliers" % (len(self.cloud_src), len(src), len(self.cloud_tgt), len(tgt), len(kp[0]), len(kp[1]), len(pairs), r["evaluated"],
                                        g["hypotheses"], r["inliers_ransac"], r["inliers_final"]), flush=True)
        elif self._cfg["verbose"]:
            print("global init: %d -> %d source and %d -> %d target points, %d correspondences, %d of %d hypotheses evaluated, %d -> %d inliers"
                  % (len(self.cloud_src), len(src), len(self.cloud_tgt), len(tgt), len(pairs), r["evaluated"], g["hypotheses"],
                     r["inliers_ransac"], r["inliers_final"]), flush=True)
        if r["status"] != OK:
            raise SymmIcpError(r["status"], "global initialisation: RANSAC: " + (e._L.symmicp_last_error(e._h) or b"").decode())
        return r["transform"]

    def levelResults(self):
        """one align() result dict per level of the last align()"""
        return self.level_results
    def setGicpEpsilon(self, eps):
        """the covariance eps of the next align in MODE_GICP (see Engine.set_gicp_epsilon)"""
        self._gicp_eps = float(eps)

    def setColorWeight(self, lam):
        """lambda of the next align in MODE_COLOR (see Engine.set_color_weight)"""
        self._color_weight = float(lam)

    def setTrimFraction(self, fraction):
        """trimmed ICP for the next align, every voxel level included (see Engine.set_trim_fraction; 1 = off)"""
        self._trim = float(fraction)

    def setOneToOne(self, on):
        """one-to-one rejection for the next align, every voxel level included (see Engine.set_one_to_one)"""
        self._one_to_one = bool(on)

    def setReciprocalCorrespondences(self, on):
        """reciprocal correspondences for the next align, every voxel level included (see Engine.set_reciprocal)"""
        self._reciprocal = bool(on)

    def setMedianFactor(self, factor):
        """median-distance rejection for the next align, every voxel level included (see Engine.set_median_factor; 0 = off)"""
        self._median = float(factor)

    def setRobustLoss(self, loss, scale):
        """robust loss of the next align (see Engine.set_robust_loss)"""
        self._loss = (loss_code(loss), float(scale))

    def LoadCloud(self, src_path, tgt_path):
        # myicp.cpp:20-31 (reader status is ignored there; here a bad file raises)
        self.cloud_src, _ = pcd_read(src_path)
        self.cloud_tgt, _ = pcd_read(tgt_path)
        self.intensity_src, _ = pcd_read_intensity(src_path)      # (None for files without an `intensity` or `rgb` field)
        self.intensity_tgt, _ = pcd_read_intensity(tgt_path)
        self.normals_src = self.normals_tgt = None
        self._have_src = self._have_tgt = False
        return 0

    def GetSrcCloud(self):
        return self.cloud_src

    def GetTgtCloud(self):
        return self.cloud_tgt

    def setInputSource(self, xyz, normals=None, intensity=None):
        self.cloud_src = _cloud(xyz)
        self.intensity_src = None if intensity is None else _scalar(intensity, self.cloud_src.shape[0])
        self.normals_src = None if normals is None else _cloud(normals)
        self._have_src = normals is not None

    def setInputTarget(self, xyz, normals=None, intensity=None):
        self.cloud_tgt = _cloud(xyz)
        self.intensity_tgt = None if intensity is None else _scalar(intensity, self.cloud_tgt.shape[0])
        self.normals_tgt = None if normals is None else _cloud(normals)
        self._have_tgt = normals is not None

    def _filter_clouds(self, keep_rows):
        """keep_rows(engine, cloud) -> kept rows; edits both clouds, their normals and intensities in place, in row order"""
        assert self.cloud_src is not None and self.cloud_tgt is not None
        with Engine(verbose=0) as e:
            ks, kt = keep_rows(e, self.cloud_src), keep_rows(e, self.cloud_tgt)
        self._removed = (len(self.cloud_src) - len(ks), len(self.cloud_tgt) - len(kt))
        pick = lambda a, rows: None if a is None else np.ascontiguousarray(a[rows])
        self.cloud_src, self.normals_src, self.intensity_src = (pick(a, ks) for a in (self.cloud_src, self.normals_src, self.intensity_src))
        self.cloud_tgt, self.normals_tgt, self.intensity_tgt = (pick(a, kt) for a in (self.cloud_tgt, self.normals_tgt, self.intensity_tgt))
        return OK

    def removeStatisticalOutliers(self, k, std_mul):
        """A one-shot edit of BOTH held clouds, as running PCL's StatisticalOutlierRemoval before RegisterSymm (not a stored option):
        each cloud is filtered by its own statistics (Engine.remove_statistical_outlier); the points, the normals (supplied ones stay
        'supplied') and the intensities keep the surviving rows, in row order.  -> status; outliersRemoved() has the counts.  With
        identity pairing a later align reports ERR_SIZE when the two counts end up unequal, as it does for any unequal clouds."""
        return self._filter_clouds(lambda e, x: e.remove_statistical_outlier(x, k, std_mul))

    def removeRadiusOutliers(self, radius, min_neighbors):
        """as removeStatisticalOutliers, with Engine.remove_radius_outlier (at least min_neighbors other points within radius)"""
        return self._filter_clouds(lambda e, x: e.remove_radius_outlier(x, radius, min_neighbors))

    def removeSmallClusters(self, eps, min_size):
        """as removeStatisticalOutliers, with Engine.cluster_dbscan: every connected part of a cloud (points closer than eps, min_points =
        1) with fewer than min_size points goes -- the floating blobs whose points have close neighbours and pass both filters above"""
        if int(min_size) < 1:
            raise SymmIcpError(ERR_ARG, "removeSmallClusters: min_size must be >= 1")
        return self._filter_clouds(lambda e, x: np.nonzero(e.cluster_dbscan(x, eps, 1, min_size, 0) >= 0)[0].astype(np.int32))

    def removePlane(self, max_dist, hypotheses=1000, min_inliers=3, axis=(0.0, 0.0, 0.0), max_angle_deg=0.0):
        """as removeStatisticalOutliers, with Engine.segment_plane (seed 0, one refit): the final inliers of the dominant plane go from EACH
        cloud -- the floor or the table that joins the objects standing on it into one cluster.  A cloud without a plane of
        max(3, min_inliers) points loses nothing.  planeRemoved() has the two planes."""
        planes = []

        def keep(e, x):
            st, r = e.segment_plane(x, max_dist, hypotheses, 0, 1, min_inliers, axis, max_angle_deg, check=False)
            if st not in (OK, ERR_NO_CONSENSUS):
                e._chk(st)
            planes.append(r[0] if st == OK else np.zeros(4))
            return np.setdiff1d(np.arange(len(x), dtype=np.int32), r[1] if st == OK else np.zeros(0, np.int32))

        st = self._filter_clouds(keep)
        self._planes = tuple(planes)
        return st

    def planeRemoved(self):
        """(source, target) planes [4] float64 of the last removePlane: n, d with n . x + d = 0; zeros for a cloud without one"""
        return self._planes

    def outliersRemoved(self):
        """(source, target) points removed by the last removeStatisticalOutliers / removeRadiusOutliers / removeSmallClusters / removePlane"""
        return self._removed

    def estimateNormals(self):
        # myicp.cpp:152-172: k = 10, flipped toward the origin.  Point-to-plane uses the target's normals only: in MODE_PLANE the
        # source's are not estimated (the engine runs without them unless the caller supplied them); GICP needs both
        def estimate(xyz):
            nrm, _ = estimate_normals(xyz, 10)
            return orient_normals(xyz, nrm, self._orient_k) if self._orient_k != 0 else nrm
        if self.normals_src is None and self._cfg["mode"] != MODE_PLANE:
            self.normals_src = estimate(self.cloud_src)
        if self.normals_tgt is None:
            self.normals_tgt = estimate(self.cloud_tgt)

    def RegisterP2P(self):
        # myicp.cpp:43-59: the reference stub applies an identity guess and computes nothing
        print("guess matrix:\n%s" % np.eye(4, dtype=np.float32))

    def align(self, guess=None):
        assert self.cloud_src is not None and self.cloud_tgt is not None      # myicp.cpp:102
        if self._cfg["mode"] == MODE_NDT:
            return self._align_ndt(guess)                                    # (both normals pre-steps are skipped)
        if self._levels and self._cfg["corr"] == CORR_IDENTITY:
            raise SymmIcpError(ERR_ARG, "voxel levels need nearest-neighbour pairs (CORR_IDENTITY pairs by row)")
        color = self._cfg["mode"] == MODE_COLOR
        if color and self._levels:
            raise SymmIcpError(ERR_ARG, "MODE_COLOR does not run voxel levels (intensities are not averaged per voxel yet)")
        if color and (self.intensity_src is None or self.intensity_tgt is None):
            raise SymmIcpError(ERR_STATE, "MODE_COLOR needs an intensity per point of both clouds (setInputSource / setInputTarget, or files with one)")
        self.estimateNormals()                                               # myicp.cpp:105
        if self._levels:
            return self._align_levels(guess)
        with Engine(**self._cfg) as e:
            if self._global is not None and guess is None:
                guess = self._global_init(e)
            if self._loss[0] != LOSS_NONE:
                e.set_robust_loss(*self._loss)
            if self._gicp_eps is not None:
                e.set_gicp_epsilon(self._gicp_eps)
            if self._trim != 1.0:
                e.set_trim_fraction(self._trim)
            if self._one_to_one:
                e.set_one_to_one(True)
            if self._reciprocal:
                e.set_reciprocal(True)
            if self._median != 0.0:
                e.set_median_factor(self._median)
            if self._color_weight is not None:
                e.set_color_weight(self._color_weight)
            e.set_target(self.cloud_tgt, self.normals_tgt)
            e.set_source(self.cloud_src, self.normals_src)
            if color:
                # the target's intensity gradient on its tangent planes, k = 10 (the neighbourhood of the normals)
                grad = e.intensity_gradient(self.cloud_tgt, self.normals_tgt, self.intensity_tgt, 10)
                e.set_target_intensity(self.intensity_tgt, grad)
                e.set_source_intensity(self.intensity_src)
            self.last_result = e.align(guess)
        self._final = self.last_result["transform"]
        return self.last_result

    def _align_levels(self, guess):
        verbose = bool(self._cfg["verbose"])
        self.level_results = []
        K = len(self._levels)
        with Engine(**dict(self._cfg, verbose=0)) as e:
            if self._loss[0] != LOSS_NONE:
                e.set_robust_loss(*self._loss)
            if self._gicp_eps is not None:
                e.set_gicp_epsilon(self._gicp_eps)
            if self._trim != 1.0:
                e.set_trim_fraction(self._trim)
            if self._one_to_one:
                e.set_one_to_one(True)
            if self._reciprocal:
                e.set_reciprocal(True)
            if self._median != 0.0:
                e.set_median_factor(self._median)
            X = guess
            if self._global is not None and guess is None:
                X = self._global_init(e)
            for k, (leaf, iters, dist) in enumerate(self._levels):
                if leaf > 0:
                    s = e.voxel_downsample(self.cloud_src, leaf, self.normals_src)
                    t = e.voxel_downsample(self.cloud_tgt, leaf, self.normals_tgt)
                    src, sn, tgt, tn = s["xyz"], s["nrm"], t["xyz"], t["nrm"]
                else:
                    src, sn, tgt, tn = self.cloud_src, self.normals_src, self.cloud_tgt, self.normals_tgt
                if verbose:
                    print("level %d/%d: leaf %g, source %d -> %d, target %d -> %d" % (k + 1, K, leaf, len(self.cloud_src), len(src),
                                                                                      len(self.cloud_tgt), len(tgt)), flush=True)
                e.set_config(max_iters=iters, max_corr_dist=dist, verbose=int(verbose and k + 1 == K))
                e.set_target(tgt, tn)
                e.set_source(src, sn)
                r = e.align(X)
                self.level_results.append(r)
                if r["status"] != OK:
                    break
                X = r["transform"]
        self.last_result = r
        if r["status"] == OK or r["iters"] > 0:
            self._final = r["transform"]
        return r

    def RegisterSymm(self):
        self.align()

    def getFinalTransformation(self):
        return self._final

    def GetAlignedSrcCloud(self):
        """the source moved by the final transform (the reference never writes its result back, myicp.cpp:109-111)"""
        X = self._final.astype(np.float64)
        return (self.cloud_src.astype(np.float64) @ X[:3, :3].T + X[:3, 3]).astype(np.float32)
