"""semantic-icp_amd -- MI355X-native semantic-ICP registration engine.

This Python module is plumbing only: a ctypes view of the C ABI declared in
include/sicp.h (implemented in csrc/ as hand-written gfx950 HIP kernels plus a
C++ host driver).  Tests and bench.py call the engine through it.  The C++ class
shims that keep the reference's API (SemanticIterativeClosestPoint,
EmIterativeClosestPoint, GICP, SemanticPointCloud) live in host/.

There is no CPU fallback: if libsicp.so cannot be built/loaded, or no HIP device
is present, every call raises.

The directory name contains a hyphen, so import it with
    importlib.import_module("semantic-icp_amd")
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import math
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))

MODE_GICP, MODE_EM, MODE_SEMANTIC = 0, 1, 2
SOURCE, TARGET = 0, 1
SE3_EXP, SE3_LOG, SE3_PLUS, SE3_MUL, SE3_INV = 0, 1, 2, 3, 4
LM_SEQUENCE, LM_SEQUENCE_ONE_LANE = 5, 6   # sicp_se3_device: the trust-region machine fed with given evaluations
LM_SEQUENCE_EVALS, LM_SEQUENCE_OUT = 24, 37

OK = 0
ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_READY = -1, -2, -3, -4
ERR_TOO_FEW_POINTS, ERR_BAD_LABEL, ERR_OUT_OF_MEMORY, ERR_INTERNAL = -5, -6, -7, -8
SUBMIT_FUSED_LABELS, SUBMIT_FRESH_FEATURES, SUBMIT_POSE_COVARIANCE = 1, 2, 8


class SicpParams(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("knn", C.c_int32),
        ("k_cov", C.c_int32),
        ("num_classes", C.c_int32),
        ("epsilon", C.c_double),
        ("gate_sq", C.c_double),
        ("cauchy_a", C.c_double),
        ("use_sqloss", C.c_int32),
        ("max_outer", C.c_int32),
        ("outer_tol", C.c_double),
        ("min_class_pts", C.c_int32),
        ("max_lm_iterations", C.c_int32),
        ("gradient_tolerance", C.c_double),
        ("function_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("initial_radius", C.c_double),
        ("max_radius", C.c_double),
        ("min_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
        ("max_consecutive_invalid_steps", C.c_int32),
        ("jacobi_scaling", C.c_int32),
        ("quirk_bool_probability", C.c_int32),
        ("quirk_float_products", C.c_int32),
        ("nn_method", C.c_int32),
        ("profile", C.c_int32),
        ("lm_on_device", C.c_int32),
        ("lm_batch", C.c_int32),
        ("reuse_features", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class SicpStats(C.Structure):
    _fields_ = [
        ("outer_iters", C.c_int32),
        ("total_lm_iters", C.c_int32),
        ("total_evals", C.c_int32),
        ("weights_in_search", C.c_int32),
        ("total_corr", C.c_int64),
        ("total_active", C.c_int64),
        ("final_cost", C.c_double),
        ("t_cov_ms", C.c_double),
        ("t_nn_ms", C.c_double),
        ("t_weight_ms", C.c_double),
        ("t_solve_ms", C.c_double),
        ("t_total_ms", C.c_double),
        ("cov_kernel_ms", C.c_double),
        ("nn_kernel_ms", C.c_double),
        ("weight_kernel_ms", C.c_double),
        ("acc_kernel_ms", C.c_double),
        ("cov_launches", C.c_int32),
        ("nn_launches", C.c_int32),
        ("weight_launches", C.c_int32),
        ("acc_launches", C.c_int32),
        ("lockstep_slots", C.c_int32),
        ("graph_builds", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SicpStreamResult(C.Structure):
    _fields_ = [
        ("ticket", C.c_int64),
        ("status", C.c_int32),
        ("outer_iters", C.c_int32),
        ("qt", C.c_double * 7),
        ("stats", SicpStats),
    ]


class SicpBootstrapParams(C.Structure):
    _fields_ = [
        ("box_max", C.c_double),
        ("leaf_size", C.c_double),
        ("normal_radius", C.c_double),
        ("feature_radius", C.c_double),
        ("min_sample_distance", C.c_double),
        ("max_corr_distance", C.c_double),
        ("max_iterations", C.c_int32),
        ("nr_samples", C.c_int32),
        ("k_correspondences", C.c_int32),
        ("reserved_", C.c_int32),
        ("seed", C.c_uint64),
    ]


BOOTSTRAP_MAX_IGNORE = 64


class SicpBootstrapLabelParams(C.Structure):
    _fields_ = [
        ("match_same_label", C.c_int32),
        ("score_same_label", C.c_int32),
        ("n_ignore", C.c_int32),
        ("reserved_", C.c_int32),
        ("ignore", C.c_uint32 * BOOTSTRAP_MAX_IGNORE),
    ]


class SicpBootstrapInfo(C.Structure):
    _fields_ = [
        ("n_source_keypoints", C.c_int32),
        ("n_target_keypoints", C.c_int32),
        ("max_neighbours", C.c_int32),
        ("best_iteration", C.c_int32),
        ("best_error", C.c_double),
        ("t_keypoints_ms", C.c_double),
        ("t_features_ms", C.c_double),
        ("t_match_ms", C.c_double),
        ("t_score_ms", C.c_double),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class SicpPoseCovarianceResult(C.Structure):
    """sicp_pose_covariance_result (include/sicp.h)"""
    _fields_ = [
        ("hessian", C.c_double * 21),
        ("gradient", C.c_double * 6),
        ("cost", C.c_double),
        ("cross_source", C.c_double * 21),
        ("cross_target", C.c_double * 21),
        ("covariance", C.c_double * 36),
        ("covariance_gn", C.c_double * 36),
        ("active", C.c_int64),
        ("positive_definite", C.c_int32),
        ("reserved_", C.c_int32),
    ]

    def as_dict(self):
        """6x6 arrays (hessian, cross_source, cross_target: the symmetric matrices of the upper triangles; covariance,
        covariance_gn as stored), plus the raw 21-entry triangles, gradient, cost, active and positive_definite"""
        def sym(u):
            M = np.empty((6, 6))
            M[np.triu_indices(6)] = np.asarray(u)
            M.T[np.triu_indices(6)] = np.asarray(u)
            return M
        return {
            "covariance": np.array(self.covariance).reshape(6, 6),
            "covariance_gn": np.array(self.covariance_gn).reshape(6, 6),
            "hessian": sym(self.hessian),
            "cross_source": sym(self.cross_source),
            "cross_target": sym(self.cross_target),
            "hessian21": np.array(self.hessian),
            "cross_source21": np.array(self.cross_source),
            "cross_target21": np.array(self.cross_target),
            "gradient": np.array(self.gradient),
            "cost": float(self.cost),
            "active": int(self.active),
            "positive_definite": bool(self.positive_definite),
        }


class SicpEvaluateResult(C.Structure):
    """sicp_evaluate_result (include/sicp.h)"""
    _fields_ = [
        ("n_source", C.c_int64),
        ("inliers", C.c_int64),
        ("label_agree", C.c_int64),
        ("label_outside", C.c_int64),
        ("sum_d2", C.c_double),
        ("fitness", C.c_double),
        ("inlier_rmse", C.c_double),
        ("reserved_", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


class SicpMergeParams(C.Structure):
    """sicp_merge_params (include/sicp.h)"""
    _fields_ = [
        ("leaf_size", C.c_double),
        ("crop_center", C.c_double * 3),
        ("crop_range", C.c_double),
    ]


class SicpMergeInfo(C.Structure):
    """sicp_merge_info (include/sicp.h)"""
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_out", C.c_int32),
        ("max_voxel_points", C.c_int32),
        ("has_label", C.c_int32),
        ("reserved_", C.c_int32),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


CLUSTER_MAX_IGNORE = 64


class SicpClusterParams(C.Structure):
    """sicp_cluster_params (include/sicp.h)"""
    _fields_ = [
        ("tolerance", C.c_double),
        ("min_points", C.c_int32),
        ("max_points", C.c_int32),
        ("same_label", C.c_int32),
        ("n_ignore", C.c_int32),
        ("ignore", C.c_uint32 * CLUSTER_MAX_IGNORE),
    ]


class SicpClusterInfo(C.Structure):
    """sicp_cluster_info (include/sicp.h)"""
    _fields_ = [
        ("n_points", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_components", C.c_int64),
        ("n_clustered", C.c_int64),
        ("n_clusters", C.c_int32),
        ("max_cluster_points", C.c_int32),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


FILTER_MAX_LABELS = 16


class SicpFilterParams(C.Structure):
    """sicp_filter_params (include/sicp.h)"""
    _fields_ = [
        ("mean_k", C.c_int32),
        ("min_neighbors", C.c_int32),
        ("std_mul", C.c_double),
        ("radius", C.c_double),
        ("n_drop", C.c_int32),
        ("n_protect", C.c_int32),
        ("drop", C.c_uint32 * FILTER_MAX_LABELS),
        ("protect", C.c_uint32 * FILTER_MAX_LABELS),
    ]


class SicpFilterInfo(C.Structure):
    """sicp_filter_info (include/sicp.h)"""
    _fields_ = [
        ("n_points", C.c_int64),
        ("n_finite", C.c_int64),
        ("n_tested", C.c_int64),
        ("n_protected", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_fail_stat", C.c_int64),
        ("n_fail_radius", C.c_int64),
        ("mean", C.c_double),
        ("stddev", C.c_double),
        ("threshold", C.c_double),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


DESKEW_MAX_KNOTS = 1024


class SicpDeskewInfo(C.Structure):
    """sicp_deskew_info (include/sicp.h)"""
    _fields_ = [
        ("n_points", C.c_int64),
        ("n_finite", C.c_int64),
        ("n_moved", C.c_int64),
        ("n_bad_time", C.c_int64),
        ("n_clamped_lo", C.c_int64),
        ("n_clamped_hi", C.c_int64),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


RANGE_MAX_WIDTH = 4096
RANGE_MAX_HEIGHT = 256
RANGE_MAX_WINDOW = 7
RANGE_MAX_K = 16


class SicpRangeParams(C.Structure):
    """sicp_range_params (include/sicp.h)"""
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("fov_up", C.c_double),
        ("fov_down", C.c_double),
        ("min_range", C.c_double),
        ("max_range", C.c_double),
        ("clockwise", C.c_int32),
        ("col_shift", C.c_int32),
        ("window", C.c_int32),
        ("k", C.c_int32),
        ("max_dist_sq", C.c_double),
    ]


class SicpRangeInfo(C.Structure):
    """sicp_range_info (include/sicp.h)"""
    _fields_ = [
        ("n_points", C.c_int64),
        ("n_finite", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_out_of_range", C.c_int64),
        ("n_outside_fov", C.c_int64),
        ("n_pixels_hit", C.c_int64),
        ("n_voted", C.c_int64),
        ("n_unvoted", C.c_int64),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


CAMERA_MAX_WIDTH = 4096
CAMERA_MAX_HEIGHT = 4096
CAMERA_MAX_WINDOW = 15


class SicpCameraParams(C.Structure):
    """sicp_camera_params (include/sicp.h)"""
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("fx", C.c_double),
        ("fy", C.c_double),
        ("cx", C.c_double),
        ("cy", C.c_double),
        ("k1", C.c_double),
        ("k2", C.c_double),
        ("p1", C.c_double),
        ("p2", C.c_double),
        ("k3", C.c_double),
        ("min_depth", C.c_double),
        ("max_depth", C.c_double),
        ("max_tan_sq", C.c_double),
        ("depth_scale", C.c_double),
        ("undistort_iterations", C.c_int32),
        ("window", C.c_int32),
        ("occlusion_abs", C.c_double),
        ("occlusion_rel", C.c_double),
    ]


class SicpCameraInfo(C.Structure):
    """sicp_camera_info (include/sicp.h)"""
    _fields_ = [
        ("n_points", C.c_int64),
        ("n_finite", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_outside", C.c_int64),
        ("n_pixels_hit", C.c_int64),
        ("n_labelled", C.c_int64),
        ("n_occluded", C.c_int64),
        ("n_unclassed", C.c_int64),
        ("n_valid", C.c_int64),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


PLANE_MAX_HYPOTHESES = 4096
PLANE_MAX_PLANES = 16
PLANE_MAX_IGNORE = 16


class SicpPlaneParams(C.Structure):
    """sicp_plane_params (include/sicp.h)"""
    _fields_ = [
        ("distance_threshold", C.c_double),
        ("axis", C.c_double * 3),
        ("min_cos", C.c_double),
        ("seed", C.c_uint64),
        ("num_hypotheses", C.c_int32),
        ("max_planes", C.c_int32),
        ("min_inliers", C.c_int32),
        ("refine", C.c_int32),
        ("n_ignore", C.c_int32),
        ("ignore", C.c_uint32 * PLANE_MAX_IGNORE),
    ]


class SicpPlaneInfo(C.Structure):
    """sicp_plane_info (include/sicp.h)"""
    _fields_ = [
        ("n_points", C.c_int64),
        ("n_finite", C.c_int64),
        ("n_candidates", C.c_int64),
        ("n_assigned", C.c_int64),
        ("n_planes", C.c_int32),
        ("rounds", C.c_int32),
        ("n_invalid_hypotheses", C.c_int64),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


GROUND_MAX_RINGS = 64
GROUND_MAX_SECTORS = 256
GROUND_MAX_IGNORE = 16
GROUND_EMPTY, GROUND_GROUND, GROUND_TOO_FEW, GROUND_NOT_UPRIGHT, GROUND_TOO_HIGH, GROUND_TOO_THICK = range(6)


class SicpGroundParams(C.Structure):
    """sicp_ground_params (include/sicp.h)"""
    _fields_ = [
        ("min_range", C.c_double),
        ("max_range", C.c_double),
        ("sensor_height", C.c_double),
        ("max_below", C.c_double),
        ("th_seeds", C.c_double),
        ("th_dist", C.c_double),
        ("min_cos", C.c_double),
        ("max_elevation", C.c_double),
        ("max_thickness", C.c_double),
        ("n_rings", C.c_int32),
        ("n_sectors", C.c_int32),
        ("n_lpr", C.c_int32),
        ("n_iter", C.c_int32),
        ("min_points", C.c_int32),
        ("elevation_rings", C.c_int32),
        ("select", C.c_int32),
        ("n_ignore", C.c_int32),
        ("ignore", C.c_uint32 * GROUND_MAX_IGNORE),
    ]


class SicpGroundOut(C.Structure):
    """sicp_ground_out (include/sicp.h)"""
    _fields_ = [
        ("ground", C.POINTER(C.c_uint8)),
        ("cell", C.POINTER(C.c_int32)),
        ("height", C.POINTER(C.c_double)),
        ("capacity", C.c_int32),
        ("pad_", C.c_int32),
        ("status", C.POINTER(C.c_uint8)),
        ("n_members", C.POINTER(C.c_int32)),
        ("n_ground", C.POINTER(C.c_int32)),
        ("n_fit", C.POINTER(C.c_int32)),
        ("normal", C.POINTER(C.c_double)),
        ("centroid", C.POINTER(C.c_double)),
        ("lambda_min", C.POINTER(C.c_double)),
        ("lpr", C.POINTER(C.c_double)),
    ]


class SicpGroundInfo(C.Structure):
    """sicp_ground_info (include/sicp.h)"""
    _fields_ = [
        ("n_points", C.c_int64),
        ("n_finite", C.c_int64),
        ("n_candidates", C.c_int64),
        ("n_below", C.c_int64),
        ("n_ground", C.c_int64),
        ("n_selected", C.c_int64),
        ("n_cells", C.c_int32),
        ("cells", C.c_int32 * 6),
        ("pad_", C.c_int32),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_ if name not in ("cells", "pad_")}
        d["cells"] = [int(v) for v in self.cells]
        return d


class SicpMapParams(C.Structure):
    """sicp_map_params (include/sicp.h)"""
    _fields_ = [
        ("leaf_size", C.c_double),
        ("num_classes", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class SicpMapIntegrateInfo(C.Structure):
    """sicp_map_integrate_info (include/sicp.h)"""
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_scan_voxels", C.c_int32),
        ("n_new_voxels", C.c_int32),
        ("n_voxels", C.c_int64),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class SicpMapExtractParams(C.Structure):
    """sicp_map_extract_params (include/sicp.h)"""
    _fields_ = [
        ("min_count", C.c_int32),
        ("reserved_", C.c_int32),
        ("crop_center", C.c_double * 3),
        ("crop_range", C.c_double),
    ]


class SicpMapExtractInfo(C.Structure):
    """sicp_map_extract_info (include/sicp.h)"""
    _fields_ = [
        ("n_voxels", C.c_int64),
        ("n_out", C.c_int32),
        ("max_voxel_points", C.c_int32),
        ("has_label", C.c_int32),
        ("reserved_", C.c_int32),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


MAP_MAX_PROTECT = 64


class SicpMapCarveParams(C.Structure):
    """sicp_map_carve_params (include/sicp.h)"""
    _fields_ = [
        ("max_range", C.c_double),
        ("min_rays", C.c_int32),
        ("end_margin", C.c_int32),
        ("dry_run", C.c_int32),
        ("n_protect", C.c_int32),
        ("protect", C.c_uint32 * MAP_MAX_PROTECT),
    ]


class SicpMapCarveInfo(C.Structure):
    """sicp_map_carve_info (include/sicp.h)"""
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_rays", C.c_int64),
        ("n_steps", C.c_int64),
        ("n_voxels", C.c_int64),
        ("n_touched", C.c_int32),
        ("n_hit", C.c_int32),
        ("n_removed", C.c_int32),
        ("n_spared_hit", C.c_int32),
        ("n_spared_label", C.c_int32),
        ("reserved_", C.c_int32),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


MAP_RAYCAST_MAX_IGNORE = 64


class SicpMapRaycastParams(C.Structure):
    """sicp_map_raycast_params (include/sicp.h)"""
    _fields_ = [
        ("max_range", C.c_double),
        ("min_count", C.c_int32),
        ("start_margin", C.c_int32),
        ("n_ignore", C.c_int32),
        ("reserved_", C.c_int32),
        ("ignore", C.c_uint32 * MAP_RAYCAST_MAX_IGNORE),
    ]


class SicpMapRaycastInfo(C.Structure):
    """sicp_map_raycast_info (include/sicp.h)"""
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_rays", C.c_int64),
        ("n_steps", C.c_int64),
        ("n_hits", C.c_int64),
        ("n_voxels", C.c_int64),
        ("n_visible", C.c_int32),
        ("reserved_", C.c_int32),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


MAP_ELEVATION_MAX_LABELS = 64
ELEVATION_CLASSES = ("unknown", "free", "blocked_label", "obstacle", "low_clearance", "step", "sparse")
ELEVATION_UNKNOWN, ELEVATION_FREE, ELEVATION_BLOCKED_LABEL, ELEVATION_OBSTACLE, ELEVATION_LOW_CLEARANCE, ELEVATION_STEP, \
    ELEVATION_SPARSE = range(7)


class SicpMapElevationParams(C.Structure):
    """sicp_map_elevation_params (include/sicp.h)"""
    _fields_ = [
        ("z_min", C.c_double),
        ("z_max", C.c_double),
        ("ref_z", C.c_double),
        ("min_clearance", C.c_double),
        ("max_step", C.c_double),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("cell_voxels", C.c_int32),
        ("min_count", C.c_int32),
        ("clearance_voxels", C.c_int32),
        ("use_ref_z", C.c_int32),
        ("max_extent_voxels", C.c_int32),
        ("min_neighbors", C.c_int32),
        ("n_ignore", C.c_int32),
        ("n_blocked", C.c_int32),
        ("n_drivable", C.c_int32),
        ("reserved_", C.c_int32),
        ("ignore", C.c_uint32 * MAP_ELEVATION_MAX_LABELS),
        ("blocked", C.c_uint32 * MAP_ELEVATION_MAX_LABELS),
        ("drivable", C.c_uint32 * MAP_ELEVATION_MAX_LABELS),
    ]


class SicpMapElevationOut(C.Structure):
    """sicp_map_elevation_out (include/sicp.h)"""
    _fields_ = [
        ("state", C.POINTER(C.c_uint8)),
        ("elevation", C.POINTER(C.c_float)),
        ("bottom", C.POINTER(C.c_float)),
        ("ceiling", C.POINTER(C.c_float)),
        ("label", C.POINTER(C.c_uint32)),
        ("count", C.POINTER(C.c_uint32)),
        ("level_top", C.POINTER(C.c_int32)),
        ("level_bottom", C.POINTER(C.c_int32)),
        ("n_levels", C.POINTER(C.c_int32)),
        ("step", C.POINTER(C.c_float)),
        ("neighbors", C.POINTER(C.c_uint8)),
        ("cell_class", C.POINTER(C.c_uint8)),
        ("point_cell", C.POINTER(C.c_int32)),
        ("point_height", C.POINTER(C.c_float)),
    ]


class SicpMapElevationInfo(C.Structure):
    """sicp_map_elevation_info (include/sicp.h)"""
    _fields_ = [
        ("n_voxels", C.c_int64),
        ("n_points", C.c_int64),
        ("x0", C.c_int32),
        ("y0", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("n_class", C.c_int32 * 8),
        ("cell_size", C.c_double),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "n_class"}
        d["n_class"] = [int(v) for v in self.n_class]
        return d


# the cell arrays of VoxelMap.elevation, in sicp_map_elevation_out's order, with their dtypes
ELEVATION_CELL_ARRAYS = (("state", np.uint8), ("elevation", np.float32), ("bottom", np.float32), ("ceiling", np.float32),
                         ("label", np.uint32), ("count", np.uint32), ("level_top", np.int32), ("level_bottom", np.int32),
                         ("n_levels", np.int32), ("step", np.float32), ("neighbors", np.uint8), ("cell_class", np.uint8))
ELEVATION_POINT_ARRAYS = (("point_cell", np.int32), ("point_height", np.float32))

MAP_DISTANCE_MAX_LABELS = 64


class SicpMapDistanceParams(C.Structure):
    """sicp_map_distance_params (include/sicp.h)"""
    _fields_ = [
        ("z_min", C.c_double),
        ("z_max", C.c_double),
        ("nx", C.c_int32),
        ("ny", C.c_int32),
        ("nz", C.c_int32),
        ("max_dist_voxels", C.c_int32),
        ("min_count", C.c_int32),
        ("planar", C.c_int32),
        ("n_ignore", C.c_int32),
        ("n_only", C.c_int32),
        ("ignore", C.c_uint32 * MAP_DISTANCE_MAX_LABELS),
        ("only", C.c_uint32 * MAP_DISTANCE_MAX_LABELS),
    ]


class SicpMapDistanceOut(C.Structure):
    """sicp_map_distance_out (include/sicp.h)"""
    _fields_ = [
        ("dist_sq", C.POINTER(C.c_int32)),
        ("nearest", C.POINTER(C.c_int32)),
        ("label", C.POINTER(C.c_uint32)),
        ("point_cell", C.POINTER(C.c_int32)),
        ("point_dist_sq", C.POINTER(C.c_int32)),
        ("point_nearest", C.POINTER(C.c_int32)),
        ("point_range_sq", C.POINTER(C.c_float)),
    ]


class SicpMapDistanceInfo(C.Structure):
    """sicp_map_distance_info (include/sicp.h)"""
    _fields_ = [
        ("n_voxels", C.c_int64),
        ("n_points", C.c_int64),
        ("n_points_inside", C.c_int64),
        ("x0", C.c_int32),
        ("y0", C.c_int32),
        ("z0", C.c_int32),
        ("nx", C.c_int32),
        ("ny", C.c_int32),
        ("nz", C.c_int32),
        ("n_obstacles", C.c_int32),
        ("n_reached", C.c_int32),
        ("max_dist_sq", C.c_int32),
        ("reserved_", C.c_int32),
        ("voxel_size", C.c_double),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


# the cell and point arrays of VoxelMap.distance, in sicp_map_distance_out's order, with their dtypes
DISTANCE_CELL_ARRAYS = (("dist_sq", np.int32), ("nearest", np.int32), ("label", np.uint32))
DISTANCE_POINT_ARRAYS = (("point_cell", np.int32), ("point_dist_sq", np.int32), ("point_nearest", np.int32),
                         ("point_range_sq", np.float32))


class SicpMapMergeParams(C.Structure):
    """sicp_map_merge_params (include/sicp.h)"""
    _fields_ = [
        ("min_count", C.c_int32),
        ("reserved_", C.c_int32),
        ("crop_center", C.c_double * 3),
        ("crop_range", C.c_double),
    ]


class SicpMapMergeInfo(C.Structure):
    """sicp_map_merge_info (include/sicp.h)"""
    _fields_ = [
        ("n_src_rows", C.c_int64),
        ("n_kept_rows", C.c_int64),
        ("n_kept_points", C.c_int64),
        ("n_touched", C.c_int32),
        ("n_new_voxels", C.c_int32),
        ("max_run", C.c_int32),
        ("reserved_", C.c_int32),
        ("n_voxels", C.c_int64),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


PLACE_LABEL, PLACE_HEIGHT = 0, 1
PLACE_MAX_IGNORE = 64


class SicpPlaceParams(C.Structure):
    """sicp_place_params (include/sicp.h)"""
    _fields_ = [
        ("n_rings", C.c_int32),
        ("n_sectors", C.c_int32),
        ("max_range", C.c_double),
        ("min_range", C.c_double),
        ("channel", C.c_int32),
        ("num_classes", C.c_int32),
        ("z_min", C.c_double),
        ("z_step", C.c_double),
        ("min_cell_points", C.c_int32),
        ("n_ignore", C.c_int32),
        ("ignore", C.c_uint32 * PLACE_MAX_IGNORE),
    ]


class SicpPlaceCandidate(C.Structure):
    """sicp_place_candidate (include/sicp.h)"""
    _fields_ = [
        ("id", C.c_int32),
        ("shift", C.c_int32),
        ("match", C.c_int32),
        ("either", C.c_int32),
        ("score", C.c_double),
        ("yaw", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class SicpPlaceDescribeInfo(C.Structure):
    """sicp_place_describe_info (include/sicp.h)"""
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_cells", C.c_int32),
        ("reserved_", C.c_int32),
        ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}


GRAPH_LOSS_NONE, GRAPH_LOSS_CAUCHY = 0, 1
PRIOR_POSE, PRIOR_POSITION = 0, 1  # SICP_GRAPH_PRIOR_*
GRAPH_TERMINATIONS = ("gradient", "function", "parameter", "max_iterations", "min_radius", "invalid_steps")


class SicpGraphParams(C.Structure):
    """sicp_graph_params (include/sicp.h)"""
    _fields_ = [
        ("loss", C.c_int32),
        ("max_iterations", C.c_int32),
        ("cauchy_a", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("function_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("initial_radius", C.c_double),
        ("min_radius", C.c_double),
        ("max_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
        ("max_consecutive_invalid_steps", C.c_int32),
        ("max_cg_iterations", C.c_int32),
        ("cg_eta", C.c_double),
        ("cg_check_every", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class SicpGraphInfo(C.Structure):
    """sicp_graph_info (include/sicp.h)"""
    _fields_ = [
        ("iterations", C.c_int32),
        ("accepted_steps", C.c_int32),
        ("rejected_steps", C.c_int32),
        ("invalid_steps", C.c_int32),
        ("cg_iterations", C.c_int32),
        ("termination", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("gradient_max_norm", C.c_double),
        ("radius", C.c_double),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["termination_name"] = GRAPH_TERMINATIONS[self.termination]
        return d


GRAPH_COV_OK, GRAPH_COV_NOT_CONVERGED, GRAPH_COV_UNANCHORED, GRAPH_COV_BREAKDOWN = 0, 1, 2, 3
GRAPH_COV_STATUSES = ("ok", "not_converged", "unanchored", "breakdown")


class SicpGraphCovParams(C.Structure):
    """sicp_graph_cov_params (include/sicp.h)"""
    _fields_ = [
        ("tolerance", C.c_double),
        ("max_cg_iterations", C.c_int32),
        ("check_every", C.c_int32),
        ("max_columns", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class SicpGraphCovInfo(C.Structure):
    """sicp_graph_cov_info (include/sicp.h)"""
    _fields_ = [
        ("passes", C.c_int32),
        ("cg_iterations", C.c_int32),
        ("n_ok", C.c_int32),
        ("n_failed", C.c_int32),
        ("worst_relative_residual", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class SicpError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        msg = f"{where}: {_strerror(status)} ({status})"
        if detail:
            msg += f" -- {detail}"
        super().__init__(msg)


def _load_build_module():
    spec = importlib.util.spec_from_file_location("_sicp_build", os.path.join(_PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/ for gfx950 into libsicp.so (in-tree)."""
    return _load_build_module().build_lib(force=force, verbose=verbose)


LIB_PATH = os.environ.get("SICP_LIB") or os.path.join(_PKG, "libsicp.so")  # SICP_LIB: an experimental build (tuning aid)
_lib = None

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint32)
_bp = C.POINTER(C.c_uint8)
_kp = C.POINTER(C.c_uint64)
_hp = C.POINTER(C.c_uint16)


def lib():
    """The loaded C-ABI library.  Builds it when missing and hipcc is available;
    raises if it can be neither found nor built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = C.CDLL(LIB_PATH)
        _lib.sicp_strerror.restype = C.c_char_p
        _lib.sicp_last_error.restype = C.c_char_p
        _lib.sicp_last_error.argtypes = [C.c_void_p]
        _lib.sicp_version.restype = C.c_char_p
        _lib.sicp_stream_last_error.restype = C.c_char_p
        _lib.sicp_stream_last_error.argtypes = [C.c_void_p]
        _lib.sicp_map_last_error.restype = C.c_char_p
        _lib.sicp_map_last_error.argtypes = [C.c_void_p]
        _lib.sicp_place_last_error.restype = C.c_char_p
        _lib.sicp_place_last_error.argtypes = [C.c_void_p]
        _lib.sicp_graph_last_error.restype = C.c_char_p
        _lib.sicp_graph_last_error.argtypes = [C.c_void_p]
        for name, args in {
            "sicp_device_count": [C.POINTER(C.c_int)],
            "sicp_create": [C.c_int, C.POINTER(C.c_void_p)],
            "sicp_release_pool": [C.c_int],
            "sicp_set_memory_limit": [C.c_int, C.c_int64],
            "sicp_memory_reserved": [C.c_int, C.POINTER(C.c_int64)],
            "sicp_destroy": [C.c_void_p],
            "sicp_default_params": [C.c_int, C.POINTER(SicpParams)],
            "sicp_set_params": [C.c_void_p, C.POINTER(SicpParams)],
            "sicp_get_params": [C.c_void_p, C.POINTER(SicpParams)],
            "sicp_set_cloud": [C.c_void_p, C.c_int, C.c_int32, _fp, _fp, _fp, _up],
            "sicp_set_cloud_strided": [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64],
            "sicp_set_cloud_device": [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "sicp_share_cloud": [C.c_void_p, C.c_int, C.c_void_p, C.c_int],
            "sicp_cloud_size": [C.c_void_p, C.c_int, _ip, _ip],
            "sicp_set_confusion": [C.c_void_p, C.c_int32, _dp],
            "sicp_align": [C.c_void_p, _dp, _dp, _ip, C.POINTER(SicpStats)],
            "sicp_align_batch": [C.POINTER(C.c_void_p), C.c_int32, _dp, _dp, _ip, C.POINTER(SicpStats)],
            "sicp_accumulate_batch": [C.POINTER(C.c_void_p), C.c_int32, _dp, _dp, C.c_int32, _dp],
            "sicp_search_batch": [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, _dp],
            "sicp_transform_source": [C.c_void_p, _dp, _fp, _fp, _fp],
            "sicp_fused_labels": [C.c_void_p, _dp, _up],
            "sicp_covariances": [C.c_void_p, C.c_int, _dp, _dp, _bp, _ip],
            "sicp_set_covariances": [C.c_void_p, C.c_int, _dp],
            "sicp_correspondences": [C.c_void_p, _dp, _ip, _fp, _dp],
            "sicp_accumulate": [C.c_void_p, _dp, _dp],
            "sicp_solve": [C.c_void_p, _dp, _dp, _ip, _ip, _dp],
            "sicp_se3_device": [C.c_void_p, C.c_int, C.c_int32, _dp, _dp],
            "sicp_get_stats": [C.c_void_p, C.POINTER(SicpStats)],
            "sicp_stream_create": [C.c_int, C.POINTER(SicpParams), C.c_int32, C.POINTER(C.c_void_p)],
            "sicp_stream_destroy": [C.c_void_p],
            "sicp_stream_set_confusion": [C.c_void_p, C.c_int32, _dp],
            "sicp_stream_add_cloud": [C.c_void_p, C.c_int32, _fp, _fp, _fp, _up, C.POINTER(C.c_int64)],
            "sicp_stream_add_cloud_strided": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)],
            "sicp_stream_release_cloud": [C.c_void_p, C.c_int64],
            "sicp_stream_submit": [C.c_void_p, C.c_int64, C.c_int64, _dp, C.POINTER(C.c_int64)],
            "sicp_stream_submit_ex": [C.c_void_p, C.c_int64, C.c_int64, _dp, C.c_uint32, C.POINTER(C.c_int64)],
            "sicp_stream_take_labels": [C.c_void_p, C.c_int64, C.c_int32, _up],
            "sicp_stream_take_pose_covariance": [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(SicpPoseCovarianceResult)],
            "sicp_stream_poll": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SicpStreamResult), C.POINTER(C.c_int32)],
            "sicp_stream_counters": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
            "sicp_synchronize": [C.c_void_p],
            "sicp_default_bootstrap_params": [C.POINTER(SicpBootstrapParams)],
            "sicp_bootstrap": [C.c_void_p, C.POINTER(SicpBootstrapParams), _dp, C.POINTER(SicpBootstrapInfo)],
            "sicp_bootstrap_batch": [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(SicpBootstrapParams), _dp, _ip,
                                     C.POINTER(SicpBootstrapInfo)],
            "sicp_bootstrap_keypoints": [C.c_void_p, C.c_int, C.POINTER(SicpBootstrapParams), C.c_int32, C.c_int64, _ip,
                                         C.POINTER(C.c_int64), _fp, _dp, _fp, C.POINTER(C.c_int64), _ip],
            "sicp_pose_covariance": [C.c_void_p, _dp, C.c_double, C.c_double, C.POINTER(SicpPoseCovarianceResult)],
            "sicp_pose_covariance_batch": [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_double, C.c_double,
                                           C.POINTER(SicpPoseCovarianceResult), _ip],
            "sicp_evaluate": [C.c_void_p, _dp, C.c_double, C.c_int32, C.POINTER(C.c_int64), _ip, _fp, C.POINTER(SicpEvaluateResult)],
            "sicp_evaluate_batch": [C.POINTER(C.c_void_p), C.c_int32, _dp, C.c_double, C.c_int32, C.POINTER(C.c_int64),
                                    C.POINTER(SicpEvaluateResult), _ip],
            "sicp_bootstrap_score": [C.c_void_p, C.POINTER(SicpBootstrapParams), C.c_int32, _ip, _ip, _dp, _dp, C.c_int32, _ip],
            "sicp_default_bootstrap_label_params": [C.POINTER(SicpBootstrapLabelParams)],
            "sicp_bootstrap_semantic": [C.c_void_p, C.POINTER(SicpBootstrapParams), C.POINTER(SicpBootstrapLabelParams), _dp,
                                        C.POINTER(SicpBootstrapInfo)],
            "sicp_bootstrap_semantic_batch": [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(SicpBootstrapParams),
                                              C.POINTER(SicpBootstrapLabelParams), _dp, _ip, C.POINTER(SicpBootstrapInfo)],
            "sicp_bootstrap_semantic_keypoints": [C.c_void_p, C.c_int, C.POINTER(SicpBootstrapParams),
                                                  C.POINTER(SicpBootstrapLabelParams), C.c_int32, _ip, _fp, _up],
            "sicp_bootstrap_semantic_score": [C.c_void_p, C.POINTER(SicpBootstrapParams), C.POINTER(SicpBootstrapLabelParams),
                                              C.c_int32, _ip, _ip, _dp, _dp, C.c_int32, _ip],
            "sicp_default_merge_params": [C.POINTER(SicpMergeParams)],
            "sicp_merge_clouds": [C.POINTER(C.c_void_p), _ip, C.c_int32, _dp, C.POINTER(SicpMergeParams), C.c_void_p, C.c_int, C.c_int32,
                                  _fp, _fp, _fp, _up, _up, C.POINTER(SicpMergeInfo)],
            "sicp_default_cluster_params": [C.POINTER(SicpClusterParams)],
            "sicp_cluster": [C.c_void_p, C.c_int, C.POINTER(SicpClusterParams), _ip, C.c_int32, _up, _ip, _ip, _dp, _fp, _fp,
                             C.POINTER(SicpClusterInfo)],
            "sicp_default_filter_params": [C.POINTER(SicpFilterParams)],
            "sicp_filter": [C.c_void_p, C.c_int, C.POINTER(SicpFilterParams), _bp, C.c_void_p, C.c_int, _bp, _dp, _ip,
                            C.POINTER(SicpFilterInfo)],
            "sicp_deskew": [C.c_void_p, C.c_int, _dp, C.c_int32, _dp, _dp, _dp, C.c_void_p, C.c_int, _fp, _fp, _fp, _dp,
                            C.POINTER(SicpDeskewInfo)],
            "sicp_deskew_twist_knots": [_dp, C.c_double, C.c_double, C.c_int32, _dp, _dp],
            "sicp_default_camera_params": [C.POINTER(SicpCameraParams)],
            "sicp_camera_matrices": [_dp, _dp, _dp],
            "sicp_camera_image": [C.c_void_p, C.c_int, C.POINTER(SicpCameraParams), _dp, _ip, _fp, _fp, _fp, _fp, _up, _up, _ip, _fp, _fp,
                                  _bp, C.POINTER(SicpCameraInfo)],
            "sicp_camera_labels": [C.c_void_p, C.c_int, C.POINTER(SicpCameraParams), _dp, _up, C.c_void_p, C.c_int, _up, _bp,
                                   C.POINTER(SicpCameraInfo)],
            "sicp_camera_unproject": [C.c_void_p, C.POINTER(SicpCameraParams), _dp, _hp, _fp, _up, C.c_void_p, C.c_int, _fp, _fp, _fp,
                                      _bp, C.POINTER(SicpCameraInfo)],
            "sicp_default_range_params": [C.POINTER(SicpRangeParams)],
            "sicp_range_tables": [C.POINTER(SicpRangeParams), _dp, _dp, _dp, _dp],
            "sicp_range_image": [C.c_void_p, C.c_int, C.POINTER(SicpRangeParams), _dp, _fp, _ip, _fp, _fp, _fp, _fp, _up, _up, _ip, _bp,
                                 C.POINTER(SicpRangeInfo)],
            "sicp_range_labels": [C.c_void_p, C.c_int, C.POINTER(SicpRangeParams), _dp, _fp, _up, C.c_void_p, C.c_int, _up, _bp,
                                  C.POINTER(SicpRangeInfo)],
            "sicp_default_plane_params": [C.POINTER(SicpPlaneParams)],
            "sicp_segment_planes": [C.c_void_p, C.c_int, C.POINTER(SicpPlaneParams), _bp, _ip, C.c_int32, _dp, _ip, _ip, _ip, _dp, _dp,
                                    C.POINTER(SicpPlaneInfo)],
            "sicp_default_ground_params": [C.POINTER(SicpGroundParams)],
            "sicp_ground_tables": [C.POINTER(SicpGroundParams), _dp, _dp, _dp, _dp],
            "sicp_segment_ground": [C.c_void_p, C.c_int, C.POINTER(SicpGroundParams), _bp, _dp, _dp, C.c_void_p, C.c_int,
                                    C.POINTER(SicpGroundOut), C.POINTER(SicpGroundInfo)],
            "sicp_default_map_params": [C.POINTER(SicpMapParams)],
            "sicp_default_map_extract_params": [C.POINTER(SicpMapExtractParams)],
            "sicp_map_create": [C.c_int, C.POINTER(SicpMapParams), C.POINTER(C.c_void_p)],
            "sicp_map_destroy": [C.c_void_p],
            "sicp_map_clear": [C.c_void_p],
            "sicp_map_size": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
            "sicp_map_integrate": [C.c_void_p, C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.POINTER(SicpMapIntegrateInfo)],
            "sicp_map_prune": [C.c_void_p, _dp, C.c_double, C.POINTER(C.c_int64)],
            "sicp_default_map_carve_params": [C.POINTER(SicpMapCarveParams)],
            "sicp_map_carve": [C.c_void_p, C.c_void_p, C.c_int, _dp, _dp, C.POINTER(SicpMapCarveParams), C.c_int32, _up,
                               C.POINTER(SicpMapCarveInfo)],
            "sicp_default_map_raycast_params": [C.POINTER(SicpMapRaycastParams)],
            "sicp_map_raycast": [C.c_void_p, _dp, _dp, C.c_int32, _fp, _fp, _fp, C.POINTER(SicpMapRaycastParams), C.c_void_p, C.c_int,
                                 _ip, _ip, _ip, _fp, _fp, _fp, _up, _up, _dp, C.POINTER(SicpMapRaycastInfo)],
            "sicp_default_map_elevation_params": [C.POINTER(SicpMapElevationParams)],
            "sicp_map_elevation": [C.c_void_p, _dp, C.POINTER(SicpMapElevationParams), C.POINTER(SicpMapElevationOut), C.c_void_p, C.c_int,
                                   _dp, C.POINTER(SicpMapElevationInfo)],
            "sicp_default_map_distance_params": [C.POINTER(SicpMapDistanceParams)],
            "sicp_map_distance": [C.c_void_p, _dp, C.POINTER(SicpMapDistanceParams), C.POINTER(SicpMapDistanceOut), C.c_void_p, C.c_int,
                                  _dp, C.POINTER(SicpMapDistanceInfo)],
            "sicp_map_extract": [C.c_void_p, C.POINTER(SicpMapExtractParams), C.c_void_p, C.c_int, C.c_int32, _fp, _fp, _fp, _up, _up, _up,
                                 C.POINTER(SicpMapExtractInfo)],
            "sicp_map_set_confusion": [C.c_void_p, C.c_int32, _dp],
            "sicp_map_extract_fused": [C.c_void_p, C.POINTER(SicpMapExtractParams), C.c_void_p, C.c_int, C.c_int32, _fp, _fp, _fp, _up, _up,
                                       _dp, C.POINTER(SicpMapExtractInfo)],
            "sicp_map_fused_labels": [C.c_void_p, C.c_void_p, C.c_int, _dp, C.c_int32, C.c_int32, _up, _dp],
            "sicp_default_map_merge_params": [C.POINTER(SicpMapMergeParams)],
            "sicp_map_merge": [C.c_void_p, C.c_void_p, _dp, C.POINTER(SicpMapMergeParams), C.POINTER(SicpMapMergeInfo)],
            "sicp_map_get_state": [C.c_void_p, C.c_int64, _kp, _dp, _up, _up, C.POINTER(C.c_int64)],
            "sicp_map_set_state": [C.c_void_p, C.c_int64, _kp, _dp, _up, _up],
            "sicp_default_place_params": [C.POINTER(SicpPlaceParams)],
            "sicp_place_create": [C.c_int, C.POINTER(SicpPlaceParams), C.POINTER(C.c_void_p)],
            "sicp_place_destroy": [C.c_void_p],
            "sicp_place_clear": [C.c_void_p],
            "sicp_place_size": [C.c_void_p, C.POINTER(C.c_int64)],
            "sicp_place_describe": [C.c_void_p, C.c_void_p, C.c_int, _dp, _bp, C.POINTER(SicpPlaceDescribeInfo)],
            "sicp_place_add": [C.c_void_p, C.c_void_p, C.c_int, _dp, _ip, _bp, C.POINTER(SicpPlaceDescribeInfo)],
            "sicp_place_add_descriptors": [C.c_void_p, C.c_int32, _bp, _ip],
            "sicp_place_get": [C.c_void_p, C.c_int32, C.c_int32, _bp],
            "sicp_place_query": [C.c_void_p, C.c_void_p, C.c_int, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                 C.POINTER(SicpPlaceCandidate), _ip],
            "sicp_place_query_descriptors": [C.c_void_p, C.c_int32, _bp, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                             C.POINTER(SicpPlaceCandidate), _ip],
            "sicp_place_tables": [C.c_void_p, _dp, _dp, _dp],
            "sicp_default_graph_params": [C.POINTER(SicpGraphParams)],
            "sicp_graph_create": [C.c_int, C.POINTER(SicpGraphParams), C.POINTER(C.c_void_p)],
            "sicp_graph_destroy": [C.c_void_p],
            "sicp_graph_clear": [C.c_void_p],
            "sicp_graph_size": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
            "sicp_graph_add_nodes": [C.c_void_p, C.c_int32, _dp, _bp, _ip],
            "sicp_graph_add_edges": [C.c_void_p, C.c_int32, _ip, _ip, _dp, _dp, _ip],
            "sicp_graph_add_priors": [C.c_void_p, C.c_int32, C.c_int32, _ip, _dp, _dp, _ip],
            "sicp_graph_set_edges_enabled": [C.c_void_p, C.c_int32, C.c_int32, _bp],
            "sicp_graph_get_edges_enabled": [C.c_void_p, C.c_int32, C.c_int32, _bp],
            "sicp_graph_set_priors_enabled": [C.c_void_p, C.c_int32, C.c_int32, _bp],
            "sicp_graph_get_priors_enabled": [C.c_void_p, C.c_int32, C.c_int32, _bp],
            "sicp_graph_prior_errors": [C.c_void_p, _dp, _dp, _dp, _dp],
            "sicp_graph_counts": [C.c_void_p] + [C.POINTER(C.c_int64)] * 5,
            "sicp_graph_set_poses": [C.c_void_p, C.c_int32, C.c_int32, _dp],
            "sicp_graph_get_poses": [C.c_void_p, C.c_int32, C.c_int32, _dp],
            "sicp_graph_set_fixed": [C.c_void_p, C.c_int32, C.c_int32, _bp],
            "sicp_graph_errors": [C.c_void_p, _dp, _dp, _dp, _dp],
            "sicp_graph_linearize": [C.c_void_p, _dp, _dp, _dp],
            "sicp_graph_optimize": [C.c_void_p, C.POINTER(SicpGraphInfo)],
            "sicp_default_graph_cov_params": [C.POINTER(SicpGraphCovParams)],
            "sicp_graph_marginals": [C.c_void_p, C.POINTER(SicpGraphCovParams), C.c_int32, _ip, _dp, _ip, C.POINTER(SicpGraphCovInfo)],
            "sicp_graph_relative_covariances": [C.c_void_p, C.POINTER(SicpGraphCovParams), C.c_int32, _ip, _ip, _dp, _ip,
                                                C.POINTER(SicpGraphCovInfo)],
        }.items():
            fn = getattr(_lib, name)
            fn.argtypes = args
            fn.restype = C.c_int
    return _lib


def _strerror(status: int) -> str:
    return lib().sicp_strerror(status).decode()


def version() -> str:
    return lib().sicp_version().decode()


def device_count() -> int:
    n = C.c_int(0)
    lib().sicp_device_count(C.byref(n))
    return n.value


def set_memory_limit(device: int, n_bytes: int) -> None:
    """Device memory the library may hold on `device` (0 = no limit); beyond it: SicpError(ERR_OUT_OF_MEMORY)."""
    st = lib().sicp_set_memory_limit(device, n_bytes)
    if st != OK:
        raise SicpError(st, "sicp_set_memory_limit")


def memory_reserved(device: int) -> int:
    n = C.c_int64(0)
    st = lib().sicp_memory_reserved(device, C.byref(n))
    if st != OK:
        raise SicpError(st, "sicp_memory_reserved")
    return n.value


def default_params(mode: int) -> SicpParams:
    p = SicpParams()
    st = lib().sicp_default_params(mode, C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_params")
    return p


def default_bootstrap_params(**overrides) -> SicpBootstrapParams:
    """the constants of exec/bootstrap.h (sicp_default_bootstrap_params), with any field overridden by keyword"""
    p = SicpBootstrapParams()
    st = lib().sicp_default_bootstrap_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_bootstrap_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_bootstrap_label_params(ignore=(), **overrides) -> SicpBootstrapLabelParams:
    """sicp_default_bootstrap_label_params (both flags 1, nothing ignored), with `ignore` as the list of labels to drop and
    any field overridden by keyword"""
    lp = SicpBootstrapLabelParams()
    st = lib().sicp_default_bootstrap_label_params(C.byref(lp))
    if st != OK:
        raise SicpError(st, "sicp_default_bootstrap_label_params")
    ignore = [int(v) for v in ignore]
    if len(ignore) > BOOTSTRAP_MAX_IGNORE:
        raise ValueError(f"at most {BOOTSTRAP_MAX_IGNORE} labels can be ignored")
    lp.n_ignore = len(ignore)
    for i, v in enumerate(ignore):
        lp.ignore[i] = v
    for k, v in overrides.items():
        if not hasattr(lp, k):
            raise AttributeError(k)
        setattr(lp, k, v)
    return lp


def default_merge_params(**overrides) -> SicpMergeParams:
    """sicp_default_merge_params (leaf 0.2, centre 0, no crop), with any field overridden by keyword (crop_center: 3 values)"""
    p = SicpMergeParams()
    st = lib().sicp_default_merge_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_merge_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_double * 3)(*v) if k == "crop_center" else v)
    return p


def default_cluster_params(ignore=(), **overrides) -> SicpClusterParams:
    """sicp_default_cluster_params (tolerance 0.5, min_points 10, no upper bound, same_label 1, nothing ignored), with the labels
    in `ignore` (at most CLUSTER_MAX_IGNORE) and any other field overridden by keyword"""
    p = SicpClusterParams()
    st = lib().sicp_default_cluster_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_cluster_params")
    ignore = [int(v) for v in ignore]
    if len(ignore) > CLUSTER_MAX_IGNORE:
        raise ValueError(f"at most {CLUSTER_MAX_IGNORE} labels can be ignored")
    p.n_ignore = len(ignore)
    for k, v in enumerate(ignore):
        p.ignore[k] = v
    for k, v in overrides.items():
        if not hasattr(p, k) or k == "ignore":
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_filter_params(drop=(), protect=(), **overrides) -> SicpFilterParams:
    """sicp_default_filter_params (mean_k 20, std_mul 2.0, radius test off, min_neighbors 2, empty lists), with the labels in
    `drop` and `protect` (at most FILTER_MAX_LABELS each) and any other field overridden by keyword"""
    p = SicpFilterParams()
    st = lib().sicp_default_filter_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_filter_params")
    for name, values in (("drop", drop), ("protect", protect)):
        values = [int(v) for v in values]
        if len(values) > FILTER_MAX_LABELS:
            raise ValueError(f"at most {FILTER_MAX_LABELS} labels can be in {name}")
        setattr(p, "n_" + name, len(values))
        for k, v in enumerate(values):
            getattr(p, name)[k] = v
    for k, v in overrides.items():
        if not hasattr(p, k) or k in ("drop", "protect"):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def deskew_twist_knots(delta_qt, t0: float, t1: float, n_knots: int = 33):
    """sicp_deskew_twist_knots (host only): the knots of the constant-velocity model -- delta_qt = T(t0)^-1 T(t1) is the sensor's
    motion over [t0, t1], knot k is exp(s_k log(delta)) at t0 + s_k (t1 - t0), s_k = k / (n_knots - 1).  Returns (knot_times
    [n_knots] float64, knot_qts [n_knots, 7] float64) for Engine.deskew."""
    d = np.ascontiguousarray(delta_qt, dtype=np.float64)
    if d.shape != (7,):
        raise ValueError("delta_qt must hold 7 numbers")
    m = max(int(n_knots), 1)
    kt = np.empty(m, dtype=np.float64)
    kq = np.empty((m, 7), dtype=np.float64)
    st = lib().sicp_deskew_twist_knots(_ptr(d, _dp), float(t0), float(t1), int(n_knots), _ptr(kt, _dp), _ptr(kq, _dp))
    if st != OK:
        raise SicpError(st, "sicp_deskew_twist_knots")
    return kt, kq


def default_range_params(**overrides) -> SicpRangeParams:
    """sicp_default_range_params (2048 x 64, +3 / -25 degrees, 0.5 .. 120 m, clockwise with col_shift = width / 2: the RangeNet++
    layout; the vote: window 5, k 5, max_dist_sq 1.0) with any field overridden by keyword.  A width given without a col_shift
    moves the shift to the new width / 2."""
    p = SicpRangeParams()
    st = lib().sicp_default_range_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_range_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    if "width" in overrides and "col_shift" not in overrides:
        p.col_shift = int(p.width) // 2
    return p


def _beam_table(params: SicpRangeParams, beam_elevation):
    if beam_elevation is None:
        return None
    b = np.ascontiguousarray(beam_elevation, dtype=np.float64)
    if b.shape != (max(int(params.height), 0),):
        raise ValueError(f"beam_elevation must have one entry per row ({params.height})")
    return b


def range_tables(params: SicpRangeParams, beam_elevation=None):
    """sicp_range_tables (host only): {"cos_half": [W/2], "sin_half": [W/2], "row_edge": [H+1]} float64, exactly what the kernels
    of Engine.range_image / range_labels read for these parameters and this beam table"""
    b = _beam_table(params, beam_elevation)
    half, rows = max(int(params.width) // 2, 1), max(int(params.height) + 1, 1)
    c, s = np.empty(half, dtype=np.float64), np.empty(half, dtype=np.float64)
    e = np.empty(rows, dtype=np.float64)
    st = lib().sicp_range_tables(C.byref(params), _ptr(b, _dp), _ptr(c, _dp), _ptr(s, _dp), _ptr(e, _dp))
    if st != OK:
        raise SicpError(st, "sicp_range_tables")
    return {"cos_half": c, "sin_half": s, "row_edge": e}


def default_camera_params(**overrides) -> SicpCameraParams:
    """sicp_default_camera_params (640 x 480, fx = fy = 525, cx, cy = 319.5, 239.5, no distortion, depths 0.3 .. 100 m, max_tan_sq 4,
    depth_scale 0.001, 20 undistortion passes, window 5, occlusion 0.3 m + 2 %) with any field overridden by keyword"""
    p = SicpCameraParams()
    st = lib().sicp_default_camera_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_camera_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _camera_qt(camera_qt):
    if camera_qt is None:
        return None
    q = np.ascontiguousarray(camera_qt, dtype=np.float64)
    if q.shape != (7,):
        raise ValueError("camera_qt must hold 7 numbers [qx qy qz qw tx ty tz]")
    return q


def camera_matrices(camera_qt=None):
    """sicp_camera_matrices (host only): {"cam_to_cloud": [3, 4], "cloud_to_cam": [3, 4]} float64, exactly what the kernels of
    Engine.camera_image / camera_labels / camera_unproject read for this camera pose (None: the identity)"""
    q = _camera_qt(camera_qt)
    a, b = np.empty((3, 4), dtype=np.float64), np.empty((3, 4), dtype=np.float64)
    st = lib().sicp_camera_matrices(_ptr(q, _dp), _ptr(a, _dp), _ptr(b, _dp))
    if st != OK:
        raise SicpError(st, "sicp_camera_matrices")
    return {"cam_to_cloud": a, "cloud_to_cam": b}


def default_plane_params(ignore=(), axis=None, **overrides) -> SicpPlaneParams:
    """sicp_default_plane_params (distance_threshold 0.2, no axis, seed 1, 1024 hypotheses, one plane, min_inliers 100, refine 1,
    nothing ignored), with the labels in `ignore` (at most PLANE_MAX_IGNORE), the three components of `axis` and any other field
    overridden by keyword"""
    p = SicpPlaneParams()
    st = lib().sicp_default_plane_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_plane_params")
    ignore = [int(v) for v in ignore]
    if len(ignore) > PLANE_MAX_IGNORE:
        raise ValueError(f"at most {PLANE_MAX_IGNORE} labels can be ignored")
    p.n_ignore = len(ignore)
    for k, v in enumerate(ignore):
        p.ignore[k] = v
    if axis is not None:
        axis = [float(v) for v in axis]
        if len(axis) != 3:
            raise ValueError("axis must have three components")
        p.axis = (C.c_double * 3)(*axis)
    for k, v in overrides.items():
        if not hasattr(p, k) or k in ("ignore", "axis"):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_ground_params(ignore=(), **overrides) -> SicpGroundParams:
    """sicp_default_ground_params (16 rings x 32 sectors from 2.7 m to 80 m, sensor 1.73 m above the road, n_lpr 20, th_seeds
    0.5, th_dist 0.2, 3 iterations, min_points 10, min_cos 0.707, 4 elevation rings at 0.5 m, no thickness test, select 0: Patchwork's
    KITTI values where it has them, untuned on this engine), with the labels in `ignore` (at most GROUND_MAX_IGNORE) and any other
    field overridden by keyword"""
    p = SicpGroundParams()
    st = lib().sicp_default_ground_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_ground_params")
    ignore = [int(v) for v in ignore]
    if len(ignore) > GROUND_MAX_IGNORE:
        raise ValueError(f"at most {GROUND_MAX_IGNORE} labels can be ignored")
    p.n_ignore = len(ignore)
    for k, v in enumerate(ignore):
        p.ignore[k] = v
    for k, v in overrides.items():
        if not hasattr(p, k) or k == "ignore":
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _ring_edge(params, ring_edge):
    if ring_edge is None:
        return None
    ring_edge = np.ascontiguousarray(ring_edge, dtype=np.float64)
    if ring_edge.shape != (int(params.n_rings) + 1,):
        raise ValueError(f"ring_edge must hold n_rings + 1 = {int(params.n_rings) + 1} numbers")
    return ring_edge


def ground_tables(params: SicpGroundParams, ring_edge=None):
    """sicp_ground_tables (host only): {"edge2": [R+1], "cos_half": [S/2], "sin_half": [S/2]} float64, exactly what the kernels of
    Engine.segment_ground read for these parameters and this ring table (None: uniform rings from min_range to max_range)"""
    R, S = int(params.n_rings), int(params.n_sectors)
    if not (1 <= R <= GROUND_MAX_RINGS and 4 <= S <= GROUND_MAX_SECTORS):
        raise SicpError(ERR_INVALID_ARGUMENT, "sicp_ground_tables")
    ring_edge = _ring_edge(params, ring_edge)
    e2, ch, sh = np.empty(R + 1, dtype=np.float64), np.empty(S // 2, dtype=np.float64), np.empty(S // 2, dtype=np.float64)
    st = lib().sicp_ground_tables(C.byref(params), _ptr(ring_edge, _dp), _ptr(ch, _dp), _ptr(sh, _dp), _ptr(e2, _dp))
    if st != OK:
        raise SicpError(st, "sicp_ground_tables")
    return {"edge2": e2, "cos_half": ch, "sin_half": sh}


def default_map_params(**overrides) -> SicpMapParams:
    """sicp_default_map_params (leaf 0.2, no labels), with any field overridden by keyword"""
    p = SicpMapParams()
    st = lib().sicp_default_map_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_map_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_map_extract_params(**overrides) -> SicpMapExtractParams:
    """sicp_default_map_extract_params (min_count 1, no crop), with any field overridden by keyword (crop_center: 3 values)"""
    p = SicpMapExtractParams()
    st = lib().sicp_default_map_extract_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_map_extract_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_double * 3)(*v) if k == "crop_center" else v)
    return p


def default_map_carve_params(**overrides) -> SicpMapCarveParams:
    """sicp_default_map_carve_params (every ray, min_rays 3, end_margin 1, nothing protected), with any field overridden by
    keyword; protect takes the labels themselves and sets n_protect with them"""
    p = SicpMapCarveParams()
    st = lib().sicp_default_map_carve_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_map_carve_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        if k == "protect":
            labels = [int(l) for l in v]
            if len(labels) > MAP_MAX_PROTECT:
                raise ValueError(f"at most {MAP_MAX_PROTECT} protected labels")
            p.protect = (C.c_uint32 * MAP_MAX_PROTECT)(*labels)
            if "n_protect" not in overrides:
                p.n_protect = len(labels)
        else:
            setattr(p, k, v)
    return p


def default_map_raycast_params(ignore=(), **overrides) -> SicpMapRaycastParams:
    """sicp_default_map_raycast_params (every ray, min_count 1, start_margin 1, nothing ignored), with the labels in `ignore`
    (at most MAP_RAYCAST_MAX_IGNORE; sets n_ignore with them) and any other field overridden by keyword"""
    p = SicpMapRaycastParams()
    st = lib().sicp_default_map_raycast_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_map_raycast_params")
    labels = [int(l) for l in ignore]
    if len(labels) > MAP_RAYCAST_MAX_IGNORE:
        raise ValueError(f"at most {MAP_RAYCAST_MAX_IGNORE} ignored labels")
    p.ignore = (C.c_uint32 * MAP_RAYCAST_MAX_IGNORE)(*labels)
    p.n_ignore = len(labels)
    for k, v in overrides.items():
        if not hasattr(p, k) or k == "ignore":
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_map_elevation_params(ignore=(), blocked=(), drivable=(), **overrides) -> SicpMapElevationParams:
    """sicp_default_map_elevation_params (cell_voxels 1, min_count 1, every level, clearance_voxels 10, the lowest surface,
    max_extent_voxels 2, the clearance, step and neighbour tests off, no label lists; width and height are the caller's), with
    the labels in `ignore`, `blocked` and `drivable` (at most MAP_ELEVATION_MAX_LABELS each; they set their counts) and any
    other field overridden by keyword"""
    p = SicpMapElevationParams()
    st = lib().sicp_default_map_elevation_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_map_elevation_params")
    for name, given in (("ignore", ignore), ("blocked", blocked), ("drivable", drivable)):
        labels = [int(l) for l in given]
        if len(labels) > MAP_ELEVATION_MAX_LABELS:
            raise ValueError(f"at most {MAP_ELEVATION_MAX_LABELS} {name} labels")
        setattr(p, name, (C.c_uint32 * MAP_ELEVATION_MAX_LABELS)(*labels))
        setattr(p, "n_" + name, len(labels))
    for k, v in overrides.items():
        if not hasattr(p, k) or k in ("ignore", "blocked", "drivable"):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_map_distance_params(ignore=(), only=(), **overrides) -> SicpMapDistanceParams:
    """sicp_default_map_distance_params (max_dist_voxels 10, min_count 1, the 3-D field, every level in planar mode, no label
    lists; nx, ny and nz are the caller's), with the labels in `ignore` and `only` (at most MAP_DISTANCE_MAX_LABELS each; they set
    their counts) and any other field overridden by keyword"""
    p = SicpMapDistanceParams()
    st = lib().sicp_default_map_distance_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_map_distance_params")
    for name, given in (("ignore", ignore), ("only", only)):
        labels = [int(l) for l in given]
        if len(labels) > MAP_DISTANCE_MAX_LABELS:
            raise ValueError(f"at most {MAP_DISTANCE_MAX_LABELS} {name} labels")
        setattr(p, name, (C.c_uint32 * MAP_DISTANCE_MAX_LABELS)(*labels))
        setattr(p, "n_" + name, len(labels))
    for k, v in overrides.items():
        if not hasattr(p, k) or k in ("ignore", "only"):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_map_merge_params(**overrides) -> SicpMapMergeParams:
    """sicp_default_map_merge_params (min_count 1, no crop), with any field overridden by keyword (crop_center: 3 values)"""
    p = SicpMapMergeParams()
    st = lib().sicp_default_map_merge_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_map_merge_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_double * 3)(*v) if k == "crop_center" else v)
    return p


def lidar_ray_ends(n_rings: int, n_azimuth: int, elev_min_deg: float, elev_max_deg: float, max_range: float, origin=(0.0, 0.0, 0.0)):
    """The ends of a spinning lidar's rays for VoxelMap.raycast: n_rings elevations evenly from elev_min_deg to elev_max_deg
    (both included), n_azimuth azimuths 2 pi k / n_azimuth, each end max_range from `origin` along (cos e cos a, cos e sin a,
    sin e), sensor frame.  Host numpy (float64, rounded once to float32); returns float32 [n_rings * n_azimuth, 3], ring-major:
    ray r * n_azimuth + k is ring r, azimuth k.  Neighbouring rays are then neighbours in a wave's share of the rays, and
    their lookups among the map's keys share cache lines."""
    if n_rings < 1 or n_azimuth < 1:
        raise ValueError("n_rings and n_azimuth must be >= 1")
    e = np.deg2rad(np.linspace(float(elev_min_deg), float(elev_max_deg), int(n_rings)))[:, None]
    a = (2.0 * np.pi * np.arange(int(n_azimuth)) / int(n_azimuth))[None, :]
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e) * np.ones_like(a)], axis=-1)
    ends = np.asarray(origin, dtype=np.float64).reshape(1, 1, 3) + float(max_range) * d
    return np.ascontiguousarray(ends.reshape(-1, 3).astype(np.float32))


def default_place_params(**overrides) -> SicpPlaceParams:
    """sicp_default_place_params (20 rings x 60 sectors to 40 m, the label channel, num_classes to be set), with any field
    overridden by keyword; ignore takes the labels themselves and sets n_ignore with them"""
    p = SicpPlaceParams()
    st = lib().sicp_default_place_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_place_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        if k == "ignore":
            labels = [int(l) for l in v]
            if len(labels) > PLACE_MAX_IGNORE:
                raise ValueError(f"at most {PLACE_MAX_IGNORE} ignored labels")
            p.ignore = (C.c_uint32 * PLACE_MAX_IGNORE)(*labels)
            if "n_ignore" not in overrides:
                p.n_ignore = len(labels)
        else:
            setattr(p, k, v)
    return p


def default_graph_params(**overrides) -> SicpGraphParams:
    """sicp_default_graph_params (no robust loss, the step control of the registration's inner solve, conjugate gradients to
    0.1 |g|), with any field overridden by keyword"""
    p = SicpGraphParams()
    st = lib().sicp_default_graph_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_graph_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_graph_cov_params(**overrides) -> SicpGraphCovParams:
    """sicp_default_graph_cov_params (tolerance 1e-10, automatic iteration limit and columns, one read-back per 32 iterations),
    with any field overridden by keyword.  What needs no device is refused here: a tolerance outside (0, 1), a negative
    max_cg_iterations, check_every < 1, a max_columns that is negative or no multiple of 6."""
    p = SicpGraphCovParams()
    st = lib().sicp_default_graph_cov_params(C.byref(p))
    if st != OK:
        raise SicpError(st, "sicp_default_graph_cov_params")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    _check_graph_cov_params(p)
    return p


def _check_graph_cov_params(p):
    if not (0.0 < p.tolerance < 1.0):
        raise ValueError("tolerance must lie in (0, 1)")
    if p.max_cg_iterations < 0:
        raise ValueError("max_cg_iterations must be 0 (automatic) or >= 1")
    if p.check_every < 1:
        raise ValueError("check_every must be >= 1")
    if p.max_columns < 0 or p.max_columns % 6:
        raise ValueError("max_columns must be 0 (automatic) or a multiple of 6")


def place_init_qt(yaw: float):
    """the init_qt of a loop candidate: the rotation by `yaw` about z that takes the query (source) onto the entry (target)"""
    return np.array([0.0, 0.0, math.sin(0.5 * yaw), math.cos(0.5 * yaw), 0.0, 0.0, 0.0])


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _points_and_labels(xyz, labels):
    """The caller's [n, >= 3] point array as float32 rows whose x, y, z are adjacent (any row stride; converted only
    when the dtype or the layout is something else), and the labels as uint32 (any stride)."""
    pts = np.asarray(xyz)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("points must be an [n, 3] array")
    if pts.dtype != np.float32 or pts.shape[0] == 0 or pts.strides[1] != 4 or pts.strides[0] < 12:
        pts = np.ascontiguousarray(pts[:, :3], dtype=np.float32)
    lab = None
    if labels is not None:
        lab = np.asarray(labels)
        if lab.dtype != np.uint32 or lab.ndim != 1 or (lab.shape[0] > 1 and lab.strides[0] < 4):
            lab = np.ascontiguousarray(lab, dtype=np.uint32).reshape(-1)
        if lab.shape[0] != pts.shape[0]:
            raise ValueError("one label per point")
    return pts, lab


class Engine:
    """One handle = one MI355X + one stream (include/sicp.h)."""

    def __init__(self, device: int = 0, params: SicpParams | None = None):
        self._h = C.c_void_p()
        st = lib().sicp_create(device, C.byref(self._h))
        if st != OK:
            self._h = C.c_void_p()
            raise SicpError(st, "sicp_create")
        self.n = [0, 0]
        if params is not None:
            self.set_params(params)

    def _check(self, st, where):
        if st != OK:
            detail = lib().sicp_last_error(self._h).decode() if st in (ERR_HIP, ERR_INVALID_ARGUMENT, ERR_OUT_OF_MEMORY, ERR_INTERNAL) else ""
            raise SicpError(st, where, detail)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().sicp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- configuration ----------------------------------------------------------
    def set_params(self, p: SicpParams):
        self._check(lib().sicp_set_params(self._h, C.byref(p)), "sicp_set_params")

    def get_params(self) -> SicpParams:
        p = SicpParams()
        self._check(lib().sicp_get_params(self._h, C.byref(p)), "sicp_get_params")
        return p

    def set_cloud(self, which: int, xyz, labels=None):
        pts, lab = _points_and_labels(xyz, labels)   # float32 [n, 3] as it lies in memory: no per-column copies
        self._check(
            lib().sicp_set_cloud_strided(self._h, which, pts.shape[0], pts.ctypes.data, pts.strides[0],
                                         None if lab is None else lab.ctypes.data, 0 if lab is None else lab.strides[0]),
            "sicp_set_cloud_strided",
        )
        self.n[which] = pts.shape[0]

    def set_source(self, xyz, labels=None):
        self.set_cloud(SOURCE, xyz, labels)

    def set_target(self, xyz, labels=None):
        self.set_cloud(TARGET, xyz, labels)

    def share_cloud(self, which: int, other: "Engine", other_which: int):
        """sicp_share_cloud: slot `which` refers to the device-resident cloud (tree, normals,
        histograms) in slot `other_which` of `other`; nothing is copied or rebuilt."""
        self._check(lib().sicp_share_cloud(self._h, which, other._h, other_which), "sicp_share_cloud")
        self.n[which] = other.n[other_which]

    def cloud_size(self, which: int):
        """(points handed over, finite points held in the device index)"""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(lib().sicp_cloud_size(self._h, which, C.byref(a), C.byref(b)), "sicp_cloud_size")
        return a.value, b.value

    def set_cloud_device(self, which: int, n: int, x_dev: int, y_dev: int, z_dev: int, label_dev: int | None = None):
        """sicp_set_cloud_device: SoA float32 / uint32 buffers resident on the handle's device (raw addresses)."""
        self._check(lib().sicp_set_cloud_device(self._h, which, n, x_dev, y_dev, z_dev, label_dev), "sicp_set_cloud_device")
        self.n[which] = n

    def set_confusion(self, cm):
        cm = np.ascontiguousarray(cm, dtype=np.float64)
        assert cm.ndim == 2 and cm.shape[0] == cm.shape[1]
        self._check(lib().sicp_set_confusion(self._h, cm.shape[0], _ptr(cm, _dp)), "sicp_set_confusion")

    # ---- hot path -----------------------------------------------------------------
    def align(self, init_qt=None, want_stats: bool = True):
        init = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64) if init_qt is None else np.ascontiguousarray(init_qt, dtype=np.float64)
        out = np.empty(7)
        it = C.c_int32(0)
        st = SicpStats()
        self._check(
            lib().sicp_align(self._h, _ptr(init, _dp), _ptr(out, _dp), C.byref(it), C.byref(st) if want_stats else None),
            "sicp_align",
        )
        return out, (st.as_dict() if want_stats else {"outer_iters": it.value})

    def transform_source(self, qt):
        qt = np.ascontiguousarray(qt, dtype=np.float64)
        n = self.n[SOURCE]
        ox, oy, oz = (np.empty(n, dtype=np.float32) for _ in range(3))
        self._check(lib().sicp_transform_source(self._h, _ptr(qt, _dp), _ptr(ox, _fp), _ptr(oy, _fp), _ptr(oz, _fp)), "sicp_transform_source")
        return np.stack([ox, oy, oz], axis=1)

    def fused_labels(self, qt):
        qt = np.ascontiguousarray(qt, dtype=np.float64)
        out = np.empty(self.n[SOURCE], dtype=np.uint32)
        self._check(lib().sicp_fused_labels(self._h, _ptr(qt, _dp), _ptr(out, _up)), "sicp_fused_labels")
        return out

    # ---- initial alignment without a pose prior (exec/bootstrap.h) ------------------------
    def bootstrap(self, params: SicpBootstrapParams | None = None):
        """coarse pose source -> target from no initial guess (qt[7], ready for align()) and the run's info dict"""
        p = params if params is not None else default_bootstrap_params()
        qt = np.empty(7)
        info = SicpBootstrapInfo()
        self._check(lib().sicp_bootstrap(self._h, C.byref(p), _ptr(qt, _dp), C.byref(info)), "sicp_bootstrap")
        return qt, info.as_dict()

    def bootstrap_keypoints(self, which: int, params: SicpBootstrapParams | None = None):
        """keypoints of one cloud: xyz (n,3) f32, normals (n,3), fpfh (n,33) f32, neighbour lists as CSR (offsets, idx)"""
        p = params if params is not None else default_bootstrap_params()
        n, nn = C.c_int32(0), C.c_int64(0)
        self._check(lib().sicp_bootstrap_keypoints(self._h, which, C.byref(p), 0, 0, C.byref(n), C.byref(nn), None, None, None, None, None),
                    "sicp_bootstrap_keypoints")
        xyz = np.empty((n.value, 3), dtype=np.float32)
        nrm = np.empty((n.value, 3))
        f = np.empty((n.value, 33), dtype=np.float32)
        off = np.empty(n.value + 1, dtype=np.int64)
        idx = np.empty(max(nn.value, 1), dtype=np.int32)
        self._check(lib().sicp_bootstrap_keypoints(self._h, which, C.byref(p), n.value, nn.value, C.byref(n), C.byref(nn), _ptr(xyz, _fp),
                                                   _ptr(nrm, _dp), _ptr(f, _fp), off.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(idx, _ip)),
                    "sicp_bootstrap_keypoints")
        return xyz, nrm, f, off, idx[:nn.value]

    def bootstrap_score(self, src_idx, tgt_idx, params: SicpBootstrapParams | None = None, n_source_keypoints: int | None = None):
        """hypotheses of given samples (keypoint indices, (n, nr_samples) each): M (n,3,4), truncated errors (n,), and -- when
        n_source_keypoints is given -- the feature neighbours of every source keypoint (n_source_keypoints, k)"""
        p = params if params is not None else default_bootstrap_params()
        a = np.ascontiguousarray(src_idx, dtype=np.int32).reshape(-1, p.nr_samples)
        b = np.ascontiguousarray(tgt_idx, dtype=np.int32).reshape(-1, p.nr_samples)
        n = a.shape[0]
        M = np.empty((n, 3, 4))
        err = np.empty(n)
        knn = None if n_source_keypoints is None else np.empty((n_source_keypoints, p.k_correspondences), dtype=np.int32)
        cap = 0 if knn is None else knn.size
        self._check(lib().sicp_bootstrap_score(self._h, C.byref(p), n, _ptr(a, _ip), _ptr(b, _ip), _ptr(M, _dp), _ptr(err, _dp), cap,
                                               _ptr(knn, _ip)), "sicp_bootstrap_score")
        return M, err, knn

    # ---- label-aware initial alignment (sicp_bootstrap_semantic) --------------------------
    def bootstrap_semantic(self, params: SicpBootstrapParams | None = None, label_params: SicpBootstrapLabelParams | None = None):
        """Engine.bootstrap with the clouds' labels: ignored labels are filtered out, feature neighbours and inliers must
        carry the source keypoint's label (label_params; default: both on, nothing ignored).  (qt[7], info dict)"""
        p = params if params is not None else default_bootstrap_params()
        lp = label_params if label_params is not None else default_bootstrap_label_params()
        qt = np.empty(7)
        info = SicpBootstrapInfo()
        self._check(lib().sicp_bootstrap_semantic(self._h, C.byref(p), C.byref(lp), _ptr(qt, _dp), C.byref(info)), "sicp_bootstrap_semantic")
        return qt, info.as_dict()

    def bootstrap_semantic_keypoints(self, which: int, params: SicpBootstrapParams | None = None,
                                     label_params: SicpBootstrapLabelParams | None = None):
        """keypoints of one cloud under the label params: xyz (n,3) f32 and their voted labels (n,) uint32"""
        p = params if params is not None else default_bootstrap_params()
        lp = label_params if label_params is not None else default_bootstrap_label_params()
        n = C.c_int32(0)
        self._check(lib().sicp_bootstrap_semantic_keypoints(self._h, which, C.byref(p), C.byref(lp), 0, C.byref(n), None, None),
                    "sicp_bootstrap_semantic_keypoints")
        xyz = np.empty((n.value, 3), dtype=np.float32)
        lab = np.empty(n.value, dtype=np.uint32)
        self._check(lib().sicp_bootstrap_semantic_keypoints(self._h, which, C.byref(p), C.byref(lp), n.value, C.byref(n), _ptr(xyz, _fp),
                                                            _ptr(lab, _up)), "sicp_bootstrap_semantic_keypoints")
        return xyz, lab

    def bootstrap_semantic_score(self, src_idx, tgt_idx, params: SicpBootstrapParams | None = None,
                                 label_params: SicpBootstrapLabelParams | None = None, n_source_keypoints: int | None = None):
        """Engine.bootstrap_score under the label params: M (n,3,4), label-aware errors (n,), and -- when n_source_keypoints is
        given -- every source keypoint's (label-restricted) feature neighbours (n_source_keypoints, k)"""
        p = params if params is not None else default_bootstrap_params()
        lp = label_params if label_params is not None else default_bootstrap_label_params()
        a = np.ascontiguousarray(src_idx, dtype=np.int32).reshape(-1, p.nr_samples)
        b = np.ascontiguousarray(tgt_idx, dtype=np.int32).reshape(-1, p.nr_samples)
        n = a.shape[0]
        M = np.empty((n, 3, 4))
        err = np.empty(n)
        knn = None if n_source_keypoints is None else np.empty((n_source_keypoints, p.k_correspondences), dtype=np.int32)
        cap = 0 if knn is None else knn.size
        self._check(lib().sicp_bootstrap_semantic_score(self._h, C.byref(p), C.byref(lp), n, _ptr(a, _ip), _ptr(b, _ip), _ptr(M, _dp),
                                                        _ptr(err, _dp), cap, _ptr(knn, _ip)), "sicp_bootstrap_semantic_score")
        return M, err, knn

    # ---- stage hooks -----------------------------------------------------------------
    def covariances(self, which: int, want_hist: bool = False, want_nn: bool = False):
        n = self.n[which]
        p = self.get_params()
        cov = np.empty((n, 3, 3))
        nrm = np.empty((n, 3))
        hist = np.empty((n, p.num_classes), dtype=np.uint8) if want_hist else None
        nn = np.empty((n, p.k_cov), dtype=np.int32) if want_nn else None
        self._check(lib().sicp_covariances(self._h, which, _ptr(cov, _dp), _ptr(nrm, _dp), _ptr(hist, _bp), _ptr(nn, _ip)), "sicp_covariances")
        return cov, nrm, hist, nn

    def covariance_matrices(self, which: int):
        """sicp_covariances with cov9 alone (getSourceCovariances() / getTargetCovariances()): the n 3x3 matrices in the caller's
        order.  A cloud without dropped points forms them on the device (cov9_caller_order_kernel); the bytes are those of
        covariances()[0] either way."""
        cov = np.empty((self.n[which], 3, 3))
        self._check(lib().sicp_covariances(self._h, which, _ptr(cov, _dp), None, None, None), "sicp_covariances")
        return cov

    def set_covariances(self, which: int, cov9):
        """caller-supplied covariances (n x 3 x 3 or n x 9, the caller's point order); SicpError when one is not I - (1-eps) n n^T"""
        c = np.ascontiguousarray(np.asarray(cov9, dtype=np.float64).reshape(-1, 9))
        self._check(lib().sicp_set_covariances(self._h, which, _ptr(c, _dp)), "sicp_set_covariances")

    def correspondences(self, qt):
        qt = np.ascontiguousarray(qt, dtype=np.float64)
        n, K = self.n[SOURCE], self.get_params().knn
        idx = np.empty((n, K), dtype=np.int32)
        d2 = np.empty((n, K), dtype=np.float32)
        w = np.empty((n, K))
        self._check(lib().sicp_correspondences(self._h, _ptr(qt, _dp), _ptr(idx, _ip), _ptr(d2, _fp), _ptr(w, _dp)), "sicp_correspondences")
        return idx, d2, w

    def accumulate(self, qt):
        qt = np.ascontiguousarray(qt, dtype=np.float64)
        out = np.empty(28)
        self._check(lib().sicp_accumulate(self._h, _ptr(qt, _dp), _ptr(out, _dp)), "sicp_accumulate")
        return out

    def pose_covariance(self, qt, sigma_source: float = 1.0, sigma_target: float = 1.0):
        """sicp_pose_covariance: the 6x6 covariance of the pose qt (tangent space of T * exp(delta), [upsilon; omega]) for
        isotropic point noise sigma^2 I on each cloud.  Returns SicpPoseCovarianceResult.as_dict()."""
        qt = np.ascontiguousarray(qt, dtype=np.float64)
        r = SicpPoseCovarianceResult()
        self._check(lib().sicp_pose_covariance(self._h, _ptr(qt, _dp), sigma_source, sigma_target, C.byref(r)), "sicp_pose_covariance")
        return r.as_dict()

    def evaluate(self, qt, max_dist_sq: float, num_classes: int | None = None, per_point: bool = False):
        """sicp_evaluate: how well the source fits the target at qt -- every finite source point's nearest target in the whole
        target cloud, an inlier when its float32 d^2 < max_dist_sq.  Returns SicpEvaluateResult.as_dict(), with `confusion`
        ([C, C] int64, inliers by source and target label) when num_classes is given and `nn_idx` / `nn_d2` (caller order; -1 where
        there is no inlier, -1 / NaN for a non-finite source point) when per_point is set.  Nothing on the engine changes."""
        qt = np.ascontiguousarray(qt, dtype=np.float64)
        r = SicpEvaluateResult()
        C_ = 0 if num_classes is None else int(num_classes)
        conf = None if num_classes is None else np.zeros((max(C_, 0), max(C_, 0)), dtype=np.int64)
        if conf is not None and conf.size == 0:
            conf = np.zeros((1, 1), dtype=np.int64)  # (a pointer to hand over: the library refuses the class count)
        n = self.n[SOURCE]
        idx = np.empty(n, dtype=np.int32) if per_point else None
        d2 = np.empty(n, dtype=np.float32) if per_point else None
        self._check(lib().sicp_evaluate(self._h, _ptr(qt, _dp), max_dist_sq, C_, _ptr(conf, C.POINTER(C.c_int64)), _ptr(idx, _ip),
                                        _ptr(d2, _fp), C.byref(r)), "sicp_evaluate")
        out = r.as_dict()
        if conf is not None:
            out["confusion"] = conf
        if per_point:
            out["nn_idx"], out["nn_d2"] = idx, d2
        return out

    def cluster(self, which: int = SOURCE, params: SicpClusterParams | None = None):
        """sicp_cluster: the objects of the cloud in slot `which` -- connected components of the points closer than the tolerance
        (and, with same_label, of equal label), those within the size bounds numbered by their smallest caller index.  Returns
        {"cluster_id": [n_points] int32 (-1: in no cluster), "label": uint32, "count": int32, "first_index": int32, "centroid":
        [n_clusters, 3] float64, "bbox_min" / "bbox_max": [n_clusters, 3] float32, "info": SicpClusterInfo.as_dict()}.  The table
        is sized by a first call without arrays.  Nothing on the engine changes."""
        p = params if params is not None else default_cluster_params()
        info = SicpClusterInfo()
        fn = lib().sicp_cluster
        self._check(fn(self._h, which, C.byref(p), None, 0, None, None, None, None, None, None, C.byref(info)), "sicp_cluster")
        k = info.n_clusters
        cid = np.empty(max(int(info.n_points), 1), dtype=np.int32)
        lab = np.empty(max(k, 1), dtype=np.uint32)
        cnt, first = (np.empty(max(k, 1), dtype=np.int32) for _ in range(2))
        cen = np.empty((max(k, 1), 3), dtype=np.float64)
        lo, hi = (np.empty((max(k, 1), 3), dtype=np.float32) for _ in range(2))
        self._check(fn(self._h, which, C.byref(p), _ptr(cid, _ip), k, _ptr(lab, _up), _ptr(cnt, _ip), _ptr(first, _ip), _ptr(cen, _dp),
                       _ptr(lo, _fp), _ptr(hi, _fp), C.byref(info)), "sicp_cluster")
        return {"cluster_id": cid[:int(info.n_points)], "label": lab[:k], "count": cnt[:k], "first_index": first[:k], "centroid": cen[:k],
                "bbox_min": lo[:k], "bbox_max": hi[:k], "info": info.as_dict()}

    def filter(self, which: int = SOURCE, params: SicpFilterParams | None = None, mask=None, dst: "Engine | None" = None,
               dst_which: int | None = None):
        """sicp_filter: which points of the cloud in slot `which` stay -- the statistical and radius outlier tests of `params` on
        the points that `mask` ([n_points], 0 removes), the drop labels and the protect labels leave to be tested.  Returns
        {"keep": [n_points] uint8, "mean_dist": float64 (NaN: not tested), "neighbors": int32 (-1: not tested), "info":
        SicpFilterInfo.as_dict()}.  With dst the kept points become that Engine's slot dst_which (default: `which`) as if they
        had been handed to set_cloud; dst may be this engine.  Without dst nothing on the engine changes."""
        p = params if params is not None else default_filter_params()
        n = self.n[which] if which in (SOURCE, TARGET) else 0
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != (n,):
                raise ValueError(f"mask must have one entry per point ({n})")
        keep = np.empty(max(n, 1), dtype=np.uint8)
        md = np.empty(max(n, 1), dtype=np.float64)
        nb = np.empty(max(n, 1), dtype=np.int32)
        info = SicpFilterInfo()
        dw = which if dst_which is None else dst_which
        self._check(lib().sicp_filter(self._h, which, C.byref(p), _ptr(mask, _bp), None if dst is None else dst._h, dw, _ptr(keep, _bp),
                                      _ptr(md, _dp), _ptr(nb, _ip), C.byref(info)), "sicp_filter")
        if dst is not None:
            dst.n[dw] = int(info.n_kept)
        return {"keep": keep[:n], "mean_dist": md[:n], "neighbors": nb[:n], "info": info.as_dict()}

    def deskew(self, which: int, times, knot_times, knot_qts, ref_qt=None, dst: "Engine | None" = None, dst_which: int | None = None,
               want_points: bool = True):
        """sicp_deskew: every point of the cloud in slot `which` moved to one instant -- times [n_points] float64 is when each
        point was measured, knot_times [n_knots] (ascending) and knot_qts [n_knots, 7] the sensor's trajectory, ref_qt the pose
        whose sensor frame the result is in (None: the last knot's).  Returns {"points": [n_points, 3] float32 (None without
        want_points), "knots": [n_knots, 7] float64, the relative knots the kernel read, "info": SicpDeskewInfo.as_dict()}.  With
        dst the moved points and the cloud's labels become that Engine's slot dst_which (default: `which`) as if they had been
        handed to set_cloud; dst may be this engine.  Without dst nothing on the engine changes."""
        n = self.n[which] if which in (SOURCE, TARGET) else 0
        times = np.ascontiguousarray(times, dtype=np.float64)
        if times.shape != (n,):
            raise ValueError(f"times must have one entry per point ({n})")
        kt = np.ascontiguousarray(knot_times, dtype=np.float64)
        kq = np.ascontiguousarray(knot_qts, dtype=np.float64)
        if kt.ndim != 1 or kq.shape != (kt.shape[0], 7):
            raise ValueError("knot_times must be [n_knots] and knot_qts [n_knots, 7]")
        if ref_qt is not None:
            ref_qt = np.ascontiguousarray(ref_qt, dtype=np.float64)
            if ref_qt.shape != (7,):
                raise ValueError("ref_qt must hold 7 numbers")
        nk = int(kt.shape[0])
        out = np.empty((3, max(n, 1)), dtype=np.float32) if want_points else None
        knots = np.empty((max(nk, 1), 7), dtype=np.float64)
        info = SicpDeskewInfo()
        dw = which if dst_which is None else dst_which
        ox, oy, oz = (None, None, None) if out is None else (out[0], out[1], out[2])
        self._check(lib().sicp_deskew(self._h, which, _ptr(times, _dp), nk, _ptr(kt, _dp), _ptr(kq, _dp), _ptr(ref_qt, _dp),
                                      None if dst is None else dst._h, dw, _ptr(ox, _fp), _ptr(oy, _fp), _ptr(oz, _fp),
                                      _ptr(knots, _dp), C.byref(info)), "sicp_deskew")
        if dst is not None:
            dst.n[dw] = int(info.n_points)
        return {"points": None if out is None else np.ascontiguousarray(out[:, :n].T), "knots": knots[:nk], "info": info.as_dict()}

    @staticmethod
    def _origin(sensor_origin):
        if sensor_origin is None:
            return None
        o = np.ascontiguousarray(sensor_origin, dtype=np.float32)
        if o.shape != (3,):
            raise ValueError("sensor_origin must hold 3 numbers")
        return o

    def range_image(self, which: int = SOURCE, params: SicpRangeParams | None = None, sensor_origin=None, beam_elevation=None,
                    per_point: bool = True):
        """sicp_range_image: the spherical projection of the cloud in slot `which` about sensor_origin (None: 0 0 0) into
        height x width pixels, each won by its nearest point.  Returns {"index": int32 (-1: empty), "range_sq", "range" (its root,
        taken here), "x", "y", "z": float32, "label", "count": uint32, all [H, W]; with per_point "pixel": [n_points] int32
        (row * W + col or -1) and "visible": [n_points] uint8; "info": SicpRangeInfo.as_dict()}.  Nothing on the engine changes."""
        p = params if params is not None else default_range_params()
        b, o = _beam_table(p, beam_elevation), self._origin(sensor_origin)
        n = self.n[which] if which in (SOURCE, TARGET) else 0
        H, W = max(int(p.height), 1), max(int(p.width), 1)
        index = np.empty((H, W), dtype=np.int32)
        r2, x, y, z = (np.empty((H, W), dtype=np.float32) for _ in range(4))
        label, count = (np.empty((H, W), dtype=np.uint32) for _ in range(2))
        pixel = np.empty(max(n, 1), dtype=np.int32) if per_point else None
        visible = np.empty(max(n, 1), dtype=np.uint8) if per_point else None
        info = SicpRangeInfo()
        self._check(lib().sicp_range_image(self._h, which, C.byref(p), _ptr(b, _dp), _ptr(o, _fp), _ptr(index, _ip), _ptr(r2, _fp),
                                           _ptr(x, _fp), _ptr(y, _fp), _ptr(z, _fp), _ptr(label, _up), _ptr(count, _up),
                                           _ptr(pixel, _ip), _ptr(visible, _bp), C.byref(info)), "sicp_range_image")
        out = {"index": index, "range_sq": r2, "range": np.sqrt(r2), "x": x, "y": y, "z": z, "label": label, "count": count,
               "info": info.as_dict()}
        if per_point:
            out["pixel"], out["visible"] = pixel[:n], visible[:n]
        return out

    def range_labels(self, which: int, pixel_label, params: SicpRangeParams | None = None, sensor_origin=None, beam_elevation=None,
                     dst: "Engine | None" = None, dst_which: int | None = None):
        """sicp_range_labels: pixel_label [H, W] uint32 (a network's class per pixel of range_image's picture, 0: none) carried
        back onto the points of the cloud in slot `which` by the vote of the k nearest occupied pixels of the window.  Returns
        {"labels": [n_points] uint32, "votes": [n_points] uint8, "info": SicpRangeInfo.as_dict()}.  With dst the points with
        their new labels become that Engine's slot dst_which (default: `which`) as if they had been handed to set_cloud; dst may
        be this engine.  Without dst nothing on the engine changes."""
        p = params if params is not None else default_range_params()
        b, o = _beam_table(p, beam_elevation), self._origin(sensor_origin)
        n = self.n[which] if which in (SOURCE, TARGET) else 0
        if pixel_label is not None:
            pixel_label = np.ascontiguousarray(pixel_label, dtype=np.uint32)
            if pixel_label.size != max(int(p.height), 0) * max(int(p.width), 0):
                raise ValueError(f"pixel_label must have one entry per pixel ({p.height} x {p.width})")
        labels = np.empty(max(n, 1), dtype=np.uint32)
        votes = np.empty(max(n, 1), dtype=np.uint8)
        info = SicpRangeInfo()
        dw = which if dst_which is None else dst_which
        self._check(lib().sicp_range_labels(self._h, which, C.byref(p), _ptr(b, _dp), _ptr(o, _fp), _ptr(pixel_label, _up),
                                            None if dst is None else dst._h, dw, _ptr(labels, _up), _ptr(votes, _bp),
                                            C.byref(info)), "sicp_range_labels")
        if dst is not None:
            dst.n[dw] = int(info.n_points)
        return {"labels": labels[:n], "votes": votes[:n], "info": info.as_dict()}

    def camera_image(self, which: int = SOURCE, params: SicpCameraParams | None = None, camera_qt=None, per_point: bool = False):
        """sicp_camera_image: the cloud in slot `which` through the pinhole camera of `params` at pose camera_qt (camera -> cloud,
        None: the identity) into height x width pixels, each won by its nearest point.  Returns {"index": int32 (-1: empty),
        "depth", "x", "y", "z": float32, "label", "count": uint32, all [H, W]; with per_point "pixel": [n_points] int32
        (row * W + col or -1), "u", "v": float32 (NaN: out of view) and "visible": uint8; "info": SicpCameraInfo.as_dict()}.
        Nothing on the engine changes."""
        p = params if params is not None else default_camera_params()
        q = _camera_qt(camera_qt)
        n = self.n[which] if which in (SOURCE, TARGET) else 0
        H, W = max(int(p.height), 1), max(int(p.width), 1)
        index = np.empty((H, W), dtype=np.int32)
        depth, x, y, z = (np.empty((H, W), dtype=np.float32) for _ in range(4))
        label, count = (np.empty((H, W), dtype=np.uint32) for _ in range(2))
        pixel = np.empty(max(n, 1), dtype=np.int32) if per_point else None
        u, v = ((np.empty(max(n, 1), dtype=np.float32) if per_point else None) for _ in range(2))
        visible = np.empty(max(n, 1), dtype=np.uint8) if per_point else None
        info = SicpCameraInfo()
        self._check(lib().sicp_camera_image(self._h, which, C.byref(p), _ptr(q, _dp), _ptr(index, _ip), _ptr(depth, _fp), _ptr(x, _fp),
                                            _ptr(y, _fp), _ptr(z, _fp), _ptr(label, _up), _ptr(count, _up), _ptr(pixel, _ip),
                                            _ptr(u, _fp), _ptr(v, _fp), _ptr(visible, _bp), C.byref(info)), "sicp_camera_image")
        out = {"index": index, "depth": depth, "x": x, "y": y, "z": z, "label": label, "count": count, "info": info.as_dict()}
        if per_point:
            out["pixel"], out["u"], out["v"], out["visible"] = pixel[:n], u[:n], v[:n], visible[:n]
        return out

    def camera_labels(self, which: int, pixel_label, params: SicpCameraParams | None = None, camera_qt=None,
                      dst: "Engine | None" = None, dst_which: int | None = None):
        """sicp_camera_labels: pixel_label [H, W] uint32 (an image network's class per pixel, 0: none) carried onto the points of
        the cloud in slot `which` that the camera sees; a point behind a nearer surface, outside the image or in a pixel of class 0
        keeps its label.  Returns {"labels": [n_points] uint32, "state": [n_points] uint8 (0: no pixel, 1: labelled, 2: occluded,
        3: class 0), "info": SicpCameraInfo.as_dict()}.  With dst the points with their new labels become that Engine's slot
        dst_which (default: `which`) as if they had been handed to set_cloud; dst may be this engine (a rig of cameras: one call
        each).  Without dst nothing on the engine changes."""
        p = params if params is not None else default_camera_params()
        q = _camera_qt(camera_qt)
        n = self.n[which] if which in (SOURCE, TARGET) else 0
        if pixel_label is not None:
            pixel_label = np.ascontiguousarray(pixel_label, dtype=np.uint32)
            if pixel_label.size != max(int(p.height), 0) * max(int(p.width), 0):
                raise ValueError(f"pixel_label must have one entry per pixel ({p.height} x {p.width})")
        labels = np.empty(max(n, 1), dtype=np.uint32)
        state = np.empty(max(n, 1), dtype=np.uint8)
        info = SicpCameraInfo()
        dw = which if dst_which is None else dst_which
        self._check(lib().sicp_camera_labels(self._h, which, C.byref(p), _ptr(q, _dp), _ptr(pixel_label, _up),
                                             None if dst is None else dst._h, dw, _ptr(labels, _up), _ptr(state, _bp),
                                             C.byref(info)), "sicp_camera_labels")
        if dst is not None:
            dst.n[dw] = int(info.n_points)
        return {"labels": labels[:n], "state": state[:n], "info": info.as_dict()}

    def camera_unproject(self, depth, params: SicpCameraParams | None = None, camera_qt=None, label=None,
                         dst: "Engine | None" = None, dst_which: int = SOURCE, want_points: bool = True):
        """sicp_camera_unproject: a depth frame [H, W] -- uint16 (times depth_scale) or float32 (metres) -- back-projected through
        the camera of `params` at pose camera_qt into H W points in the cloud's frame, NaN where the depth is invalid.  With dst
        the points (and `label` [H, W] uint32, if given) become that Engine's slot dst_which as if they had been handed to
        set_cloud; dst may be this engine.  Returns {"info": SicpCameraInfo.as_dict()} and, with want_points, "xyz": [H W, 3]
        float32 and "valid": [H, W] uint8."""
        p = params if params is not None else default_camera_params()
        q = _camera_qt(camera_qt)
        H, W = max(int(p.height), 0), max(int(p.width), 0)
        d = np.ascontiguousarray(depth)
        if d.dtype not in (np.uint16, np.float32):
            raise TypeError("depth must be uint16 or float32")
        if d.size != H * W:
            raise ValueError(f"depth must have one entry per pixel ({p.height} x {p.width})")
        if label is not None:
            label = np.ascontiguousarray(label, dtype=np.uint32)
            if label.size != H * W:
                raise ValueError(f"label must have one entry per pixel ({p.height} x {p.width})")
        npx = max(H * W, 1)
        x, y, z = ((np.empty(npx, dtype=np.float32) if want_points else None) for _ in range(3))
        valid = np.empty(npx, dtype=np.uint8) if want_points else None
        info = SicpCameraInfo()
        self._check(lib().sicp_camera_unproject(self._h, C.byref(p), _ptr(q, _dp), _ptr(d if d.dtype == np.uint16 else None, _hp),
                                                _ptr(d if d.dtype == np.float32 else None, _fp), _ptr(label, _up),
                                                None if dst is None else dst._h, dst_which, _ptr(x, _fp), _ptr(y, _fp), _ptr(z, _fp),
                                                _ptr(valid, _bp), C.byref(info)), "sicp_camera_unproject")
        if dst is not None:
            dst.n[dst_which] = int(info.n_points)
        out = {"info": info.as_dict()}
        if want_points:
            out["xyz"] = np.stack([x[:H * W], y[:H * W], z[:H * W]], axis=1)
            out["valid"] = valid[:H * W].reshape(H, W)
        return out

    def segment_planes(self, which: int = SOURCE, params: SicpPlaneParams | None = None, mask=None):
        """sicp_segment_planes: the dominant planes of the cloud in slot `which` by RANSAC -- per round num_hypotheses three-point
        planes scored over the candidates (finite, `mask` ([n_points], 0 leaves a point out) non-zero, label not ignored) no earlier
        plane took, the winner refitted and its members re-selected with refine.  Returns {"plane_id": [n_points] int32 (-1: in no
        plane), "coeff": [n_planes, 4] float64 (unit normal, offset), "count", "hyp_index", "hyp_count": int32, "centroid":
        [n_planes, 3] float64, "rms": float64, "info": SicpPlaneInfo.as_dict()}.  The tables are sized by max_planes: one call.
        Nothing on the engine changes."""
        p = params if params is not None else default_plane_params()
        n = self.n[which] if which in (SOURCE, TARGET) else 0
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != (n,):
                raise ValueError(f"mask must have one entry per point ({n})")
        cap = max(int(p.max_planes), 1)
        pid = np.empty(max(n, 1), dtype=np.int32)
        coeff = np.empty((cap, 4), dtype=np.float64)
        cnt, hi, hc = (np.empty(cap, dtype=np.int32) for _ in range(3))
        cen = np.empty((cap, 3), dtype=np.float64)
        rms = np.empty(cap, dtype=np.float64)
        info = SicpPlaneInfo()
        self._check(lib().sicp_segment_planes(self._h, which, C.byref(p), _ptr(mask, _bp), _ptr(pid, _ip), cap, _ptr(coeff, _dp),
                                              _ptr(cnt, _ip), _ptr(hi, _ip), _ptr(hc, _ip), _ptr(cen, _dp), _ptr(rms, _dp),
                                              C.byref(info)), "sicp_segment_planes")
        k = int(info.n_planes)
        return {"plane_id": pid[:n], "coeff": coeff[:k], "count": cnt[:k], "hyp_index": hi[:k], "hyp_count": hc[:k], "centroid": cen[:k],
                "rms": rms[:k], "info": info.as_dict()}

    def segment_ground(self, which: int = SOURCE, params: SicpGroundParams | None = None, mask=None, sensor_origin=None, ring_edge=None,
                       dst: "Engine | None" = None, dst_which: int | None = None):
        """sicp_segment_ground: the piecewise-planar ground of the cloud in slot `which` on a polar grid of n_rings x n_sectors
        cells around sensor_origin (None: 0 0 0; z is up), one plane per cell fitted from the cell's lowest candidates (finite,
        `mask` ([n_points], 0 leaves a point out) non-zero, label not ignored, not under the road) upward, and every point's height
        above the local ground.  ring_edge ([n_rings + 1], ascending) replaces the uniform rings.  Returns {"ground": [n_points]
        uint8, "cell": int32 (-1: outside the rings), "height": float64 (NaN: no ground model), per cell [n_rings n_sectors]
        "status": uint8 (GROUND_*), "n_members", "n_ground", "n_fit": int32, "normal", "centroid": [.., 3] float64, "lambda_min",
        "lpr": float64, "info": SicpGroundInfo.as_dict()}.  With dst and params.select = 1 (the points that are not ground) or 2
        (the ground points) the selection becomes that Engine's slot dst_which (default: `which`) as if it had been handed to
        set_cloud; dst may be this engine.  Without dst nothing on the engine changes."""
        p = params if params is not None else default_ground_params()
        n = self.n[which] if which in (SOURCE, TARGET) else 0
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != (n,):
                raise ValueError(f"mask must have one entry per point ({n})")
        if sensor_origin is not None:
            sensor_origin = np.ascontiguousarray(sensor_origin, dtype=np.float64)
            if sensor_origin.shape != (3,):
                raise ValueError("sensor_origin must hold 3 numbers")
        ring_edge = _ring_edge(p, ring_edge)
        cap = max(int(p.n_rings), 1) * max(int(p.n_sectors), 1)
        m = max(n, 1)
        arr = {"ground": np.empty(m, np.uint8), "cell": np.empty(m, np.int32), "height": np.empty(m, np.float64),
               "status": np.empty(cap, np.uint8), "n_members": np.empty(cap, np.int32), "n_ground": np.empty(cap, np.int32),
               "n_fit": np.empty(cap, np.int32), "normal": np.empty((cap, 3), np.float64), "centroid": np.empty((cap, 3), np.float64),
               "lambda_min": np.empty(cap, np.float64), "lpr": np.empty(cap, np.float64)}
        out = SicpGroundOut()
        out.capacity = cap
        for k, a in arr.items():
            setattr(out, k, a.ctypes.data_as(dict(SicpGroundOut._fields_)[k]))
        info = SicpGroundInfo()
        dw = which if dst_which is None else dst_which
        self._check(lib().sicp_segment_ground(self._h, which, C.byref(p), _ptr(mask, _bp), _ptr(sensor_origin, _dp), _ptr(ring_edge, _dp),
                                              None if dst is None else dst._h, dw, C.byref(out), C.byref(info)), "sicp_segment_ground")
        if dst is not None and int(p.select) != 0:
            dst.n[dw] = int(info.n_selected)
        res = {k: (a[:n] if k in ("ground", "cell", "height") else a) for k, a in arr.items()}
        res["info"] = info.as_dict()
        return res

    def solve(self, init_qt):
        init = np.ascontiguousarray(init_qt, dtype=np.float64)
        out = np.empty(7)
        it, ev, fc = C.c_int32(), C.c_int32(), C.c_double()
        self._check(lib().sicp_solve(self._h, _ptr(init, _dp), _ptr(out, _dp), C.byref(it), C.byref(ev), C.byref(fc)), "sicp_solve")
        return out, dict(lm_iters=it.value, evals=ev.value, cost=fc.value)

    def se3_device(self, op: int, x):
        """sicp_se3_device: csrc/se3.hpp evaluated on the GPU (op = SE3_EXP / LOG / PLUS / MUL / INV), one row per item."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = x.shape[0]
        out = np.empty((n, LM_SEQUENCE_OUT if op >= LM_SEQUENCE else 6 if op == SE3_LOG else 7))
        self._check(lib().sicp_se3_device(self._h, op, n, _ptr(x, _dp), _ptr(out, _dp)), "sicp_se3_device")
        return out

    def stats(self):
        st = SicpStats()
        self._check(lib().sicp_get_stats(self._h, C.byref(st)), "sicp_get_stats")
        return st.as_dict()

    def synchronize(self):
        self._check(lib().sicp_synchronize(self._h), "sicp_synchronize")


# ---- lock-step batch over several engines (one per scan pair) ---------------------------------
def _handles(engines):
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    return arr


def align_batch(engines, init_qts=None, want_stats: bool = True):
    """sicp_align_batch: every engine registers its own pair, advanced in lock step.
    Returns [(qt, stats)] in the order of `engines`; per pair identical to Engine.align."""
    n = len(engines)
    init = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64), (n, 1)) if init_qts is None else \
        np.ascontiguousarray(init_qts, dtype=np.float64).reshape(n, 7)
    out = np.empty((n, 7))
    its = np.zeros(n, dtype=np.int32)
    sts = (SicpStats * n)()
    rc = lib().sicp_align_batch(_handles(engines), n, _ptr(init, _dp), _ptr(out, _dp), _ptr(its, _ip), sts if want_stats else None)
    if rc != 0:
        msgs = "; ".join(m for m in (lib().sicp_last_error(e._h).decode() for e in engines) if m)
        raise RuntimeError(f"sicp_align_batch failed: {_strerror(rc)} ({rc}) {msgs}")
    return [(out[p].copy(), (sts[p].as_dict() if want_stats else {"outer_iters": int(its[p])})) for p in range(n)]


def bootstrap_batch(engines, params: SicpBootstrapParams | None = None):
    """sicp_bootstrap_batch: Engine.bootstrap for every engine's pair in one call (the same params for all).
    Returns [(status, qt, info)] in the order of `engines`: per pair identical to Engine.bootstrap, qt None and info
    {"error": message} for a pair that failed.  Raises SicpError only when the whole call is refused."""
    n = len(engines)
    p = params if params is not None else default_bootstrap_params()
    out = np.empty((max(n, 1), 7))
    unset = -(2 ** 31)
    status = np.full(max(n, 1), unset, dtype=np.int32)
    infos = (SicpBootstrapInfo * max(n, 1))()
    rc = lib().sicp_bootstrap_batch(_handles(engines) if n else None, n, C.byref(p), _ptr(out, _dp), _ptr(status, _ip), infos)
    if rc != OK and (n == 0 or status[0] == unset):
        raise SicpError(rc, "sicp_bootstrap_batch", lib().sicp_last_error(engines[0]._h).decode() if n else "")
    res = []
    for i in range(n):
        if status[i] == OK:
            res.append((OK, out[i].copy(), infos[i].as_dict()))
        else:
            res.append((int(status[i]), None, {"error": lib().sicp_last_error(engines[i]._h).decode()}))
    return res


def bootstrap_semantic_batch(engines, params: SicpBootstrapParams | None = None, label_params: SicpBootstrapLabelParams | None = None):
    """sicp_bootstrap_semantic_batch: Engine.bootstrap_semantic for every engine's pair in one call (the same params for
    all).  Returns [(status, qt, info)] as bootstrap_batch does; per pair identical to the lone call."""
    n = len(engines)
    p = params if params is not None else default_bootstrap_params()
    lp = label_params if label_params is not None else default_bootstrap_label_params()
    out = np.empty((max(n, 1), 7))
    unset = -(2 ** 31)
    status = np.full(max(n, 1), unset, dtype=np.int32)
    infos = (SicpBootstrapInfo * max(n, 1))()
    rc = lib().sicp_bootstrap_semantic_batch(_handles(engines) if n else None, n, C.byref(p), C.byref(lp), _ptr(out, _dp),
                                             _ptr(status, _ip), infos)
    if rc != OK and (n == 0 or status[0] == unset):
        raise SicpError(rc, "sicp_bootstrap_semantic_batch", lib().sicp_last_error(engines[0]._h).decode() if n else "")
    res = []
    for i in range(n):
        if status[i] == OK:
            res.append((OK, out[i].copy(), infos[i].as_dict()))
        else:
            res.append((int(status[i]), None, {"error": lib().sicp_last_error(engines[i]._h).decode()}))
    return res


def pose_covariance_batch(engines, qts, sigma_source: float = 1.0, sigma_target: float = 1.0):
    """sicp_pose_covariance_batch: Engine.pose_covariance for every engine at its row of qts.  Returns [(status, dict or
    None)] in the order of `engines`; per pair identical to the lone call.  Raises SicpError only when the whole call is
    refused."""
    n = len(engines)
    qts = np.ascontiguousarray(qts, dtype=np.float64).reshape(n, 7) if n else np.zeros((1, 7))
    out = (SicpPoseCovarianceResult * max(n, 1))()
    unset = -(2 ** 31)
    status = np.full(max(n, 1), unset, dtype=np.int32)
    rc = lib().sicp_pose_covariance_batch(_handles(engines) if n else None, n, _ptr(qts, _dp), sigma_source, sigma_target, out,
                                          _ptr(status, _ip))
    if rc != OK and (n == 0 or status[0] == unset):
        raise SicpError(rc, "sicp_pose_covariance_batch", lib().sicp_last_error(engines[0]._h).decode() if n else "")
    return [(OK, out[i].as_dict()) if status[i] == OK else (int(status[i]), None) for i in range(n)]


def evaluate_batch(engines, qts, max_dist_sq: float, num_classes: int | None = None):
    """sicp_evaluate_batch: Engine.evaluate (without per-point outputs) for every engine at its row of qts.  Returns [(status,
    dict or None)] in the order of `engines`; per pair identical to the lone call, `confusion` included when num_classes is
    given.  Raises SicpError only when the whole call is refused."""
    n = len(engines)
    qts = np.ascontiguousarray(qts, dtype=np.float64).reshape(n, 7) if n else np.zeros((1, 7))
    out = (SicpEvaluateResult * max(n, 1))()
    unset = -(2 ** 31)
    status = np.full(max(n, 1), unset, dtype=np.int32)
    C_ = 0 if num_classes is None else int(num_classes)
    conf = None if num_classes is None else np.zeros((max(n, 1), max(C_, 1), max(C_, 1)), dtype=np.int64)
    rc = lib().sicp_evaluate_batch(_handles(engines) if n else None, n, _ptr(qts, _dp), max_dist_sq, C_, _ptr(conf, C.POINTER(C.c_int64)),
                                   out, _ptr(status, _ip))
    if rc != OK and (n == 0 or status[0] == unset):
        raise SicpError(rc, "sicp_evaluate_batch", lib().sicp_last_error(engines[0]._h).decode() if n else "")
    res = []
    for i in range(n):
        if status[i] != OK:
            res.append((int(status[i]), None))
            continue
        d = out[i].as_dict()
        if conf is not None:
            d["confusion"] = conf[i].copy()
        res.append((OK, d))
    return res


def merge_clouds(parts, qts=None, params: SicpMergeParams | None = None, dst=None, want_points: bool = True):
    """sicp_merge_clouds: the clouds in `parts` -- a list of (Engine, which) -- each at its row of qts (None: identities),
    cropped and reduced on the voxel grid of `params` to one cloud; with dst = (Engine, which) that slot becomes the result as
    if it had been handed to set_cloud.  Returns {"xyz": [n_out, 3] float32, "labels": uint32 or None, "count": uint32,
    "info": SicpMergeInfo.as_dict()}; with want_points=False no arrays are asked for and xyz / labels / count are None.  The
    buffers are sized by the sum of the parts' finite points."""
    n = len(parts)
    p = params if params is not None else default_merge_params()
    hs = _handles([e for e, _ in parts]) if n else None
    which = np.array([w for _, w in parts] if n else [0], dtype=np.int32)
    q = None if qts is None else np.ascontiguousarray(qts, dtype=np.float64).reshape(max(n, 1), 7)
    cap = 0
    x = y = z = lab = cnt = None
    if want_points and n:
        cap = sum(e.cloud_size(w)[1] for e, w in parts)
        x, y, z = (np.empty(max(cap, 1), dtype=np.float32) for _ in range(3))
        lab, cnt = (np.empty(max(cap, 1), dtype=np.uint32) for _ in range(2))
    info = SicpMergeInfo()
    rc = lib().sicp_merge_clouds(hs, _ptr(which, _ip), n, _ptr(q, _dp), C.byref(p), None if dst is None else dst[0]._h,
                                 0 if dst is None else dst[1], cap, _ptr(x, _fp), _ptr(y, _fp), _ptr(z, _fp), _ptr(lab, _up),
                                 _ptr(cnt, _up), C.byref(info))
    if rc != OK:
        raise SicpError(rc, "sicp_merge_clouds", lib().sicp_last_error(parts[0][0]._h).decode() if n else "")
    if dst is not None:
        dst[0].n[dst[1]] = info.n_out
    m = info.n_out
    return {
        "xyz": None if x is None else np.stack([x[:m], y[:m], z[:m]], axis=1),
        "labels": lab[:m].copy() if (lab is not None and info.has_label) else None,
        "count": None if cnt is None else cnt[:m].copy(),
        "info": info.as_dict(),
    }


class VoxelMap:
    """sicp_map_*: a voxel map that lives on the device between calls -- per voxel of merge_clouds' grid the float64 sums, the
    count and (num_classes > 0) the label histogram of every point integrated so far.  integrate() adds an Engine's cloud at a
    pose; extract() gives the next target, to arrays and / or straight into an Engine's slot."""

    def __init__(self, device: int = 0, params: SicpMapParams | None = None):
        self._m = C.c_void_p()
        p = params if params is not None else default_map_params()
        self.num_classes = int(p.num_classes)
        self.leaf_size = float(p.leaf_size)
        st = lib().sicp_map_create(device, C.byref(p), C.byref(self._m))
        if st != OK:
            self._m = C.c_void_p()
            raise SicpError(st, "sicp_map_create")

    def _check(self, st, where):
        if st != OK:
            raise SicpError(st, where, lib().sicp_map_last_error(self._m).decode())

    def close(self):
        if getattr(self, "_m", None) and self._m.value:
            lib().sicp_map_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def integrate(self, engine: "Engine", which: int = SOURCE, qt=None, crop_center=None, crop_range: float = 0.0):
        """sicp_map_integrate: the finite points of engine's slot `which`, at pose qt (None: identity), cropped about crop_center
        (None: the origin) with crop_range (0: no crop), into their voxels.  Returns SicpMapIntegrateInfo.as_dict()."""
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64).reshape(7)
        c = None if crop_center is None else np.ascontiguousarray(crop_center, dtype=np.float64).reshape(3)
        info = SicpMapIntegrateInfo()
        self._check(lib().sicp_map_integrate(self._m, engine._h, which, _ptr(q, _dp), _ptr(c, _dp), crop_range, C.byref(info)),
                    "sicp_map_integrate")
        return info.as_dict()

    def extract(self, min_count: int = 1, crop_center=None, crop_range: float = 0.0, dst: "Engine | None" = None, dst_which: int = TARGET,
                want_points: bool = True, want_hist: bool = False):
        """sicp_map_extract: one point per voxel with at least min_count points whose centroid passes the crop, ascending key;
        with dst that Engine's slot dst_which becomes the result as if it had been handed to set_cloud.  Returns {"xyz", "labels"
        (None when the map keeps none), "count", "hist" ([n_out, num_classes + 1] with want_hist, else None), "info"}; with
        want_points=False no arrays are asked for."""
        p = default_map_extract_params(min_count=min_count, crop_range=crop_range,
                                       crop_center=(0.0, 0.0, 0.0) if crop_center is None else tuple(crop_center))
        cap = 0
        x = y = z = lab = cnt = hist = None
        if want_points or want_hist:
            cap = self.size()[0]
        if want_points:
            x, y, z = (np.empty(max(cap, 1), dtype=np.float32) for _ in range(3))
            lab, cnt = (np.empty(max(cap, 1), dtype=np.uint32) for _ in range(2))
        if want_hist:
            hist = np.empty((max(cap, 1), self.num_classes + 1), dtype=np.uint32)
        info = SicpMapExtractInfo()
        self._check(lib().sicp_map_extract(self._m, C.byref(p), None if dst is None else dst._h, dst_which, cap, _ptr(x, _fp), _ptr(y, _fp),
                                           _ptr(z, _fp), _ptr(lab, _up), _ptr(cnt, _up), _ptr(hist, _up), C.byref(info)),
                    "sicp_map_extract")
        if dst is not None:
            dst.n[dst_which] = info.n_out
        m = info.n_out
        return {
            "xyz": None if x is None else np.stack([x[:m], y[:m], z[:m]], axis=1),
            "labels": lab[:m].copy() if (lab is not None and info.has_label) else None,
            "count": None if cnt is None else cnt[:m].copy(),
            "hist": None if hist is None else hist[:m].copy(),
            "info": info.as_dict(),
        }

    def set_confusion(self, cm):
        """sicp_map_set_confusion: cm[r, s] = how often a point of class s + 1 is observed with label r + 1 ([C, C], C the map's
        num_classes; zero entries allowed).  Replaces the matrix set before."""
        cm = np.ascontiguousarray(cm, dtype=np.float64)
        if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
            raise ValueError("the confusion matrix must be square")
        self._check(lib().sicp_map_set_confusion(self._m, cm.shape[0], _ptr(cm, _dp)), "sicp_map_set_confusion")

    def extract_fused(self, min_count: int = 1, crop_center=None, crop_range: float = 0.0, dst: "Engine | None" = None,
                      dst_which: int = TARGET, want_points: bool = True):
        """sicp_map_extract_fused: extract()'s selection, order, points and counts, with the maximum a-posteriori class under the
        confusion matrix as the label and its posterior probability (0 and 0.0 for a voxel without evidence).  Returns {"xyz",
        "labels", "count", "confidence", "info"}; with want_points=False no arrays are asked for."""
        p = default_map_extract_params(min_count=min_count, crop_range=crop_range,
                                       crop_center=(0.0, 0.0, 0.0) if crop_center is None else tuple(crop_center))
        cap = 0
        x = y = z = lab = cnt = conf = None
        if want_points:
            cap = self.size()[0]
            x, y, z = (np.empty(max(cap, 1), dtype=np.float32) for _ in range(3))
            lab, cnt = (np.empty(max(cap, 1), dtype=np.uint32) for _ in range(2))
            conf = np.empty(max(cap, 1), dtype=np.float64)
        info = SicpMapExtractInfo()
        self._check(lib().sicp_map_extract_fused(self._m, C.byref(p), None if dst is None else dst._h, dst_which, cap, _ptr(x, _fp),
                                                 _ptr(y, _fp), _ptr(z, _fp), _ptr(lab, _up), _ptr(cnt, _up), _ptr(conf, _dp), C.byref(info)),
                    "sicp_map_extract_fused")
        if dst is not None:
            dst.n[dst_which] = info.n_out
        m = info.n_out
        return {
            "xyz": None if x is None else np.stack([x[:m], y[:m], z[:m]], axis=1),
            "labels": None if lab is None else lab[:m].copy(),
            "count": None if cnt is None else cnt[:m].copy(),
            "confidence": None if conf is None else conf[:m].copy(),
            "info": info.as_dict(),
        }

    def fused_labels(self, engine: "Engine", which: int = SOURCE, qt=None, include_own: bool = True, min_count: int = 1,
                     want_confidence: bool = True):
        """sicp_map_fused_labels: every point of engine's slot `which` (caller order), at pose qt (None: identity), relabelled
        from the voxel it falls into -- the voxel's histogram (when it has min_count points) and, with include_own, the point's
        own label as one more observation, through the confusion matrix.  Returns (labels, confidence); confidence is None
        with want_confidence=False.  A point without evidence keeps its own label with confidence 0."""
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64).reshape(7)
        n = engine.cloud_size(which)[0]
        labels = np.empty(max(n, 1), dtype=np.uint32)
        conf = np.empty(max(n, 1), dtype=np.float64) if want_confidence else None
        self._check(lib().sicp_map_fused_labels(self._m, engine._h, which, _ptr(q, _dp), int(bool(include_own)), min_count,
                                                _ptr(labels, _up), _ptr(conf, _dp)), "sicp_map_fused_labels")
        return labels[:n].copy(), None if conf is None else conf[:n].copy()

    def carve(self, engine: "Engine", which: int = SOURCE, qt=None, sensor_origin=None, params: SicpMapCarveParams | None = None,
              want_miss: bool = False):
        """sicp_map_carve: removes the voxels that at least params.min_rays rays of engine's slot `which` -- from sensor_origin (in
        the scan's own frame; None: 0 0 0) to every finite point, at pose qt (None: identity) -- pass through, that hold no return
        of the scan and whose label is not protected.  Returns {"miss": with want_miss the rays through every row the map had
        before the call, ascending key (extract's default order), else None; "info": SicpMapCarveInfo.as_dict()}."""
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64).reshape(7)
        o = None if sensor_origin is None else np.ascontiguousarray(sensor_origin, dtype=np.float64).reshape(3)
        p = params if params is not None else default_map_carve_params()
        cap = self.size()[0] if want_miss else 0
        miss = np.zeros(max(cap, 1), dtype=np.uint32) if want_miss else None
        info = SicpMapCarveInfo()
        self._check(lib().sicp_map_carve(self._m, engine._h, which, _ptr(q, _dp), _ptr(o, _dp), C.byref(p), cap, _ptr(miss, _up),
                                         C.byref(info)), "sicp_map_carve")
        return {"miss": None if miss is None else miss[:cap].copy(), "info": info.as_dict()}

    def raycast(self, ends, qt=None, sensor_origin=None, params: SicpMapRaycastParams | None = None, dst: "Engine | None" = None,
                dst_which: int = TARGET):
        """sicp_map_raycast: ray i runs from sensor_origin (None: 0 0 0) to ends[i] ([n, 3], both in the sensor's frame, at pose qt;
        None: identity) and stops at the first opaque voxel.  Returns {"row": the hit's row in extract()'s default order (-1: none),
        "step": its index in the walk, "length": the walk's steps (-1: the end cast no ray), "xyz": the hit voxel's centroid,
        "labels", "count", "range_sq": squared distance from the origin to that centroid (-1.0: none), "info":
        SicpMapRaycastInfo.as_dict()}.  With dst the distinct voxels hit, ascending key, become that Engine's slot dst_which as if
        handed to set_cloud."""
        e = np.ascontiguousarray(ends, dtype=np.float32).reshape(-1, 3)
        n = len(e)
        ex, ey, ez = (np.ascontiguousarray(e[:, a]) if n else np.zeros(1, np.float32) for a in range(3))
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64).reshape(7)
        o = None if sensor_origin is None else np.ascontiguousarray(sensor_origin, dtype=np.float64).reshape(3)
        p = params if params is not None else default_map_raycast_params()
        row, step, length = (np.empty(max(n, 1), dtype=np.int32) for _ in range(3))
        x, y, z = (np.empty(max(n, 1), dtype=np.float32) for _ in range(3))
        lab, cnt = (np.empty(max(n, 1), dtype=np.uint32) for _ in range(2))
        r2 = np.empty(max(n, 1), dtype=np.float64)
        info = SicpMapRaycastInfo()
        self._check(lib().sicp_map_raycast(self._m, _ptr(q, _dp), _ptr(o, _dp), n, _ptr(ex, _fp), _ptr(ey, _fp), _ptr(ez, _fp), C.byref(p),
                                           None if dst is None else dst._h, dst_which, _ptr(row, _ip), _ptr(step, _ip), _ptr(length, _ip),
                                           _ptr(x, _fp), _ptr(y, _fp), _ptr(z, _fp), _ptr(lab, _up), _ptr(cnt, _up), _ptr(r2, _dp),
                                           C.byref(info)), "sicp_map_raycast")
        if dst is not None:
            dst.n[dst_which] = info.n_visible
        return {"row": row[:n].copy(), "step": step[:n].copy(), "length": length[:n].copy(),
                "xyz": np.stack([x[:n], y[:n], z[:n]], axis=1), "labels": lab[:n].copy(), "count": cnt[:n].copy(),
                "range_sq": r2[:n].copy(), "info": info.as_dict()}

    def elevation(self, center, width: int, height: int, params: SicpMapElevationParams | None = None, engine: "Engine | None" = None,
                  which: int = SOURCE, qt=None, want=None):
        """sicp_map_elevation: the map as a 2.5-D grid of height x width cells about center (x, y) -- per cell the surface one can
        stand on.  Returns a dict of [height, width] arrays "state", "elevation", "bottom", "ceiling", "label", "count",
        "level_top", "level_bottom", "n_levels", "step", "neighbors", "cell_class" (ELEVATION_*), and "info"
        (SicpMapElevationInfo.as_dict(): x0, y0, cell_size, n_class ...).  With an engine also "point_cell" and "point_height":
        for every point of its slot `which` (caller order), at pose qt (None: identity), its cell (-1: none) and its height above
        that cell's elevation (NaN: none).  `want` (None: everything) names the arrays to ask for; the others are not returned.
        params (None: the defaults) is not modified; width and height are set from the arguments."""
        p = SicpMapElevationParams()
        C.memmove(C.byref(p), C.byref(params if params is not None else default_map_elevation_params()), C.sizeof(p))
        p.width, p.height = int(width), int(height)
        c = np.ascontiguousarray(center, dtype=np.float64).reshape(2)
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64).reshape(7)
        names = [n for n, _ in ELEVATION_CELL_ARRAYS] + ([n for n, _ in ELEVATION_POINT_ARRAYS] if engine is not None else [])
        if want is not None:
            unknown = [n for n in want if n not in [a for a, _ in ELEVATION_CELL_ARRAYS + ELEVATION_POINT_ARRAYS]]
            if unknown:
                raise KeyError(unknown[0])
            names = list(want)
        n_cells = max(p.width, 0) * max(p.height, 0)
        n_points = 0
        if engine is not None and any(n in names for n, _ in ELEVATION_POINT_ARRAYS):
            try:
                n_points = engine.cloud_size(which)[0]
            except SicpError:
                pass  # (no cloud, a bad slot: the call below refuses and names the cause)
        out = SicpMapElevationOut()
        arrays = {}
        for name, dt in ELEVATION_CELL_ARRAYS + ELEVATION_POINT_ARRAYS:
            if name not in names:
                continue
            cells = (name, dt) in ELEVATION_CELL_ARRAYS
            a = np.zeros(max(n_cells if cells else n_points, 1), dtype=dt)
            arrays[name] = a
            setattr(out, name, a.ctypes.data_as(dict(SicpMapElevationOut._fields_)[name]))
        info = SicpMapElevationInfo()
        self._check(lib().sicp_map_elevation(self._m, _ptr(c, _dp), C.byref(p), C.byref(out), None if engine is None else engine._h, which,
                                             _ptr(q, _dp), C.byref(info)), "sicp_map_elevation")
        res = {}
        for name, a in arrays.items():
            cells = name in [n for n, _ in ELEVATION_CELL_ARRAYS]
            res[name] = a[:n_cells].reshape(p.height, p.width).copy() if cells else a[:n_points].copy()
        res["info"] = info.as_dict()
        return res

    def distance(self, center, shape, params: SicpMapDistanceParams | None = None, engine: "Engine | None" = None, which: int = SOURCE,
                 qt=None, want=None):
        """sicp_map_distance: the truncated Euclidean distance field of the map on a window of shape = (nx, ny, nz) voxels about
        center (x, y, z).  Returns a dict of [nz, ny, nx] arrays "dist_sq" (squared distance to the nearest obstacle voxel in
        voxels, -1 beyond params.max_dist_voxels), "nearest" (that voxel's row in get_state()'s order, -1) and "label" (its
        label), and "info" (SicpMapDistanceInfo.as_dict(): x0, y0, z0, n_obstacles, n_reached, max_dist_sq, voxel_size ...).  With
        an engine also "point_cell", "point_dist_sq", "point_nearest" and, in 3-D mode, "point_range_sq": for every point of its
        slot `which` (caller order) at pose qt (None: identity) its cell (-1: none), that cell's values, and its squared metric
        distance to the nearest voxel's centroid (NaN: none).  `want` (None: everything) names the arrays to ask for; the others
        are not returned.  params (None: the defaults) is not modified; nx, ny and nz are set from shape."""
        p = SicpMapDistanceParams()
        C.memmove(C.byref(p), C.byref(params if params is not None else default_map_distance_params()), C.sizeof(p))
        p.nx, p.ny, p.nz = (int(v) for v in shape)
        c = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64).reshape(7)
        point_names = [n for n, _ in DISTANCE_POINT_ARRAYS if not (p.planar and n == "point_range_sq")]
        names = [n for n, _ in DISTANCE_CELL_ARRAYS] + (point_names if engine is not None else [])
        if want is not None:
            unknown = [n for n in want if n not in [a for a, _ in DISTANCE_CELL_ARRAYS + DISTANCE_POINT_ARRAYS]]
            if unknown:
                raise KeyError(unknown[0])
            names = list(want)
        n_cells = max(p.nx, 0) * max(p.ny, 0) * max(p.nz, 0)
        n_points = 0
        if engine is not None and any(n in names for n, _ in DISTANCE_POINT_ARRAYS):
            try:
                n_points = engine.cloud_size(which)[0]
            except SicpError:
                pass  # (no cloud, a bad slot: the call below refuses and names the cause)
        out = SicpMapDistanceOut()
        arrays = {}
        for name, dt in DISTANCE_CELL_ARRAYS + DISTANCE_POINT_ARRAYS:
            if name not in names:
                continue
            cells = (name, dt) in DISTANCE_CELL_ARRAYS
            a = np.zeros(max(n_cells if cells else n_points, 1), dtype=dt)
            arrays[name] = a
            setattr(out, name, a.ctypes.data_as(dict(SicpMapDistanceOut._fields_)[name]))
        info = SicpMapDistanceInfo()
        self._check(lib().sicp_map_distance(self._m, _ptr(c, _dp), C.byref(p), C.byref(out), None if engine is None else engine._h, which,
                                            _ptr(q, _dp), C.byref(info)), "sicp_map_distance")
        res = {}
        for name, a in arrays.items():
            cells = name in [n for n, _ in DISTANCE_CELL_ARRAYS]
            # (a cell array is handed over as it is: a window can hold 64 MB an array)
            res[name] = a[:n_cells].reshape(p.nz, p.ny, p.nx) if cells else a[:n_points].copy()
        res["info"] = info.as_dict()
        return res

    def merge(self, src: "VoxelMap", qt=None, min_count: int = 1, crop_center=None, crop_range: float = 0.0):
        """sicp_map_merge: src's voxels with at least min_count points, moved by qt (src's frame -> this map's; None: identity)
        and cropped about crop_center (None: the origin, this map's frame) with crop_range (0: no crop), added into this map with
        their sums, counts and histograms; src is not modified.  Returns SicpMapMergeInfo.as_dict()."""
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64).reshape(7)
        p = default_map_merge_params(min_count=min_count, crop_range=crop_range,
                                     crop_center=(0.0, 0.0, 0.0) if crop_center is None else tuple(crop_center))
        info = SicpMapMergeInfo()
        self._check(lib().sicp_map_merge(self._m, src._m, _ptr(q, _dp), C.byref(p), C.byref(info)), "sicp_map_merge")
        return info.as_dict()

    def get_state(self):
        """sicp_map_get_state: the map's exact contents, rows in ascending key (extract's default order) -- {"key" uint64 [n], "sums"
        float64 [n, 3], "count" uint32 [n], "hist" uint32 [n, num_classes + 1] (None when the map keeps no labels), "leaf_size",
        "num_classes"}: what from_state() and set_state() take, and all a caller has to store."""
        n = self.size()[0]
        key = np.empty(max(n, 1), dtype=np.uint64)
        sums = np.empty((max(n, 1), 3), dtype=np.float64)
        count = np.empty(max(n, 1), dtype=np.uint32)
        hist = np.empty((max(n, 1), self.num_classes + 1), dtype=np.uint32) if self.num_classes > 0 else None
        rows = C.c_int64()
        self._check(lib().sicp_map_get_state(self._m, n, _ptr(key, _kp), _ptr(sums, _dp), _ptr(count, _up), _ptr(hist, _up),
                                             C.byref(rows)), "sicp_map_get_state")
        return {"key": key[:n].copy(), "sums": sums[:n].copy(), "count": count[:n].copy(), "hist": None if hist is None else hist[:n].copy(),
                "leaf_size": self.leaf_size, "num_classes": self.num_classes}

    def set_state(self, state):
        """sicp_map_set_state: the map's contents become exactly the rows of `state` (a get_state() dict; its leaf_size and
        num_classes must be this map's).  A refusal names the offending row and leaves the map as it was."""
        if int(state["num_classes"]) != self.num_classes or float(state["leaf_size"]) != self.leaf_size:
            raise ValueError("the state's leaf_size / num_classes are not this map's")
        key = np.ascontiguousarray(state["key"], dtype=np.uint64).reshape(-1)
        n = len(key)
        sums = np.ascontiguousarray(state["sums"], dtype=np.float64).reshape(-1, 3)
        count = np.ascontiguousarray(state["count"], dtype=np.uint32).reshape(-1)
        hist = None
        if self.num_classes > 0:
            hist = np.ascontiguousarray(state["hist"], dtype=np.uint32).reshape(-1, self.num_classes + 1)
        if len(sums) != n or len(count) != n or (hist is not None and len(hist) != n):
            raise ValueError("key, sums, count and hist differ in length")
        self._check(lib().sicp_map_set_state(self._m, n, _ptr(key, _kp), _ptr(sums, _dp), _ptr(count, _up), _ptr(hist, _up)),
                    "sicp_map_set_state")

    @classmethod
    def from_state(cls, state, device: int = 0):
        """a new map with state's leaf_size and num_classes holding exactly its rows"""
        vm = cls(device, default_map_params(leaf_size=float(state["leaf_size"]), num_classes=int(state["num_classes"])))
        try:
            vm.set_state(state)
        except Exception:
            vm.close()
            raise
        return vm

    def prune(self, center, range):
        """sicp_map_prune: drops the voxels whose centroid lies further than `range` from `center`; returns their number"""
        c = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
        n = C.c_int64(0)
        self._check(lib().sicp_map_prune(self._m, _ptr(c, _dp), range, C.byref(n)), "sicp_map_prune")
        return n.value

    def clear(self):
        self._check(lib().sicp_map_clear(self._m), "sicp_map_clear")

    def size(self):
        """(voxels, points)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(lib().sicp_map_size(self._m, C.byref(a), C.byref(b)), "sicp_map_size")
        return a.value, b.value


class PlaceDB:
    """sicp_place_*: a database of scan descriptors that lives on the device -- R rings x S sectors of uint8 cell codes per
    scan, by label or by height.  add() describes an Engine's cloud and appends it; query() returns the best earlier scans
    for a new one with the yaw between them (place_init_qt(yaw) is the init_qt of the registration that follows)."""

    def __init__(self, device: int = 0, params: SicpPlaceParams | None = None):
        self._db = C.c_void_p()
        p = params if params is not None else default_place_params()
        self.n_rings, self.n_sectors = int(p.n_rings), int(p.n_sectors)
        st = lib().sicp_place_create(device, C.byref(p), C.byref(self._db))
        if st != OK:
            self._db = C.c_void_p()
            raise SicpError(st, "sicp_place_create")

    def _check(self, st, where):
        if st != OK:
            raise SicpError(st, where, lib().sicp_place_last_error(self._db).decode())

    def close(self):
        if getattr(self, "_db", None) and self._db.value:
            lib().sicp_place_destroy(self._db)
            self._db = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _origin(sensor_origin):
        return None if sensor_origin is None else np.ascontiguousarray(sensor_origin, dtype=np.float64).reshape(3)

    def _descs(self, desc):
        d = np.ascontiguousarray(desc, dtype=np.uint8)
        if d.ndim == 2:
            d = d[None]
        if d.ndim != 3 or d.shape[1:] != (self.n_rings, self.n_sectors):
            raise ValueError(f"descriptors must be [n, {self.n_rings}, {self.n_sectors}] uint8")
        return d

    def describe(self, engine: "Engine", which: int = SOURCE, sensor_origin=None):
        """sicp_place_describe: (desc[R, S] uint8, SicpPlaceDescribeInfo.as_dict()) of engine's slot `which`"""
        o = self._origin(sensor_origin)
        desc = np.empty((self.n_rings, self.n_sectors), dtype=np.uint8)
        info = SicpPlaceDescribeInfo()
        self._check(lib().sicp_place_describe(self._db, engine._h, which, _ptr(o, _dp), _ptr(desc, _bp), C.byref(info)), "sicp_place_describe")
        return desc, info.as_dict()

    def add(self, engine: "Engine", which: int = SOURCE, sensor_origin=None) -> int:
        """sicp_place_add: describe + append; returns the new entry's id"""
        o = self._origin(sensor_origin)
        new_id = C.c_int32(-1)
        self._check(lib().sicp_place_add(self._db, engine._h, which, _ptr(o, _dp), C.byref(new_id), None, None), "sicp_place_add")
        return new_id.value

    def add_descriptors(self, desc) -> int:
        """sicp_place_add_descriptors: [n, R, S] (or one [R, S]) descriptors appended as they are; returns the first one's id"""
        d = self._descs(desc)
        first = C.c_int32(-1)
        self._check(lib().sicp_place_add_descriptors(self._db, d.shape[0], _ptr(d, _bp), C.byref(first)), "sicp_place_add_descriptors")
        return first.value

    def get(self, first: int = 0, count: int = -1):
        """sicp_place_get: entries first .. first+count-1 (count = -1: to the end) as [count, R, S] uint8"""
        n = self.size() - first if count < 0 else count
        out = np.empty((max(n, 0), self.n_rings, self.n_sectors), dtype=np.uint8)
        self._check(lib().sicp_place_get(self._db, first, count, _ptr(out, _bp) if out.size else None), "sicp_place_get")
        return out

    def query(self, engine_or_descs, which: int = SOURCE, sensor_origin=None, first: int = 0, count: int = -1, top_k: int = 5,
              min_score: float = 0.0):
        """sicp_place_query (an Engine: its slot `which` is described first) or sicp_place_query_descriptors (one [R, S]
        descriptor or a batch [n, R, S]).  Returns the candidates, best first, as a list of dicts {id, shift, match, either,
        score, yaw}; for a batch a list of such lists."""
        cap = max(int(top_k), 1)
        if isinstance(engine_or_descs, Engine):
            o = self._origin(sensor_origin)
            out = (SicpPlaceCandidate * cap)()
            found = C.c_int32(0)
            self._check(lib().sicp_place_query(self._db, engine_or_descs._h, which, _ptr(o, _dp), first, count, top_k, min_score, out,
                                               C.byref(found)), "sicp_place_query")
            return [out[k].as_dict() for k in range(found.value)]
        lone = np.asarray(engine_or_descs).ndim == 2
        d = self._descs(engine_or_descs)
        n_q = d.shape[0]
        out = (SicpPlaceCandidate * (cap * max(n_q, 1)))()
        found = np.zeros(max(n_q, 1), dtype=np.int32)
        self._check(lib().sicp_place_query_descriptors(self._db, n_q, _ptr(d, _bp), first, count, top_k, min_score, out, _ptr(found, _ip)),
                    "sicp_place_query_descriptors")
        rows = [[out[q * cap + k].as_dict() for k in range(int(found[q]))] for q in range(n_q)]
        return rows[0] if lone else rows

    def tables(self):
        """sicp_place_tables: {"cos_half": [S/2], "sin_half": [S/2], "edge2": [R+1]} float64, as the device holds them"""
        c, s = (np.empty(self.n_sectors // 2, dtype=np.float64) for _ in range(2))
        e = np.empty(self.n_rings + 1, dtype=np.float64)
        self._check(lib().sicp_place_tables(self._db, _ptr(c, _dp), _ptr(s, _dp), _ptr(e, _dp)), "sicp_place_tables")
        return {"cos_half": c, "sin_half": s, "edge2": e}

    def size(self) -> int:
        n = C.c_int64(0)
        self._check(lib().sicp_place_size(self._db, C.byref(n)), "sicp_place_size")
        return n.value

    def clear(self):
        self._check(lib().sicp_place_clear(self._db), "sicp_place_clear")


class PoseGraph:
    """sicp_graph_*: a pose graph that lives on the device.  Node i is a pose qt[7] (node -> world); an edge (i, j, z, omega)
    measures z ~ T_i^-1 T_j -- what align() returns with node j's scan as the source and node i's as the target -- with the 6x6
    information matrix omega = inv(pose_covariance(...)["covariance"]).  optimize() moves the free nodes to the minimum of
    1/2 sum rho(r^T omega r)."""

    def __init__(self, device: int = 0, params: SicpGraphParams | None = None):
        self._g = C.c_void_p()
        p = params if params is not None else default_graph_params()
        st = lib().sicp_graph_create(device, C.byref(p), C.byref(self._g))
        if st != OK:
            self._g = C.c_void_p()
            raise SicpError(st, "sicp_graph_create")

    def _check(self, st, where):
        if st != OK:
            raise SicpError(st, where, lib().sicp_graph_last_error(self._g).decode())

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            lib().sicp_graph_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _poses(qt):
        q = np.ascontiguousarray(qt, dtype=np.float64)
        if q.ndim == 1:
            q = q[None]
        if q.ndim != 2 or q.shape[1] != 7:
            raise ValueError("poses must be [n, 7] float64")
        return q

    def add_nodes(self, qt, fixed=None) -> int:
        """sicp_graph_add_nodes: [n, 7] poses (or one), fixed[n] flags or None; returns the first new node's id"""
        q = self._poses(qt)
        f = None
        if fixed is not None:
            f = np.ascontiguousarray(np.broadcast_to(np.asarray(fixed, dtype=bool), (q.shape[0],)), dtype=np.uint8)
        first = C.c_int32(-1)
        self._check(lib().sicp_graph_add_nodes(self._g, q.shape[0], _ptr(q, _dp), _ptr(f, _bp), C.byref(first)), "sicp_graph_add_nodes")
        return first.value

    def add_edges(self, i, j, z, omega) -> int:
        """sicp_graph_add_edges: ends i[m], j[m], measurements z[m, 7], information matrices omega[m, 6, 6]; returns the first
        new edge's id"""
        zz = self._poses(z)
        m = zz.shape[0]
        ii = np.ascontiguousarray(np.atleast_1d(i), dtype=np.int32)
        jj = np.ascontiguousarray(np.atleast_1d(j), dtype=np.int32)
        om = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1, 6, 6)
        if ii.shape != (m,) or jj.shape != (m,) or om.shape[0] != m:
            raise ValueError("i[m], j[m], z[m, 7] and omega[m, 6, 6] must agree on m")
        first = C.c_int32(-1)
        self._check(lib().sicp_graph_add_edges(self._g, m, _ptr(ii, _ip), _ptr(jj, _ip), _ptr(zz, _dp), _ptr(om, _dp), C.byref(first)),
                    "sicp_graph_add_edges")
        return first.value

    def add_priors(self, nodes, z, omega, kind: int = PRIOR_POSE) -> int:
        """sicp_graph_add_priors: priors of one kind on nodes[m].  PRIOR_POSE: z[m, 7] ~ T_k, omega[m, 6, 6] in the tangent of
        z exp(delta) (the inverse of a marginals() block, without conversion).  PRIOR_POSITION: z[m, 3] ~ t_k in the world frame
        (a GPS fix), omega[m, 3, 3].  Returns the first new prior's id."""
        nn = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
        m = nn.shape[0]
        dz, do = (7, 6) if kind == PRIOR_POSE else (3, 3)
        zz = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, dz)
        om = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1, do, do)
        if nn.ndim != 1 or zz.shape[0] != m or om.shape[0] != m:
            raise ValueError("nodes[m], z[m, 7 or 3] and omega[m, 6, 6 or 3, 3] must agree on m")
        first = C.c_int32(-1)
        self._check(lib().sicp_graph_add_priors(self._g, kind, m, _ptr(nn, _ip), _ptr(zz, _dp), _ptr(om, _dp), C.byref(first)),
                    "sicp_graph_add_priors")
        return first.value

    def _set_enabled(self, fn, where, enabled, first):
        f = np.ascontiguousarray(np.atleast_1d(np.asarray(enabled, dtype=bool)), dtype=np.uint8)
        self._check(fn(self._g, first, f.shape[0], _ptr(f, _bp)), where)

    def _get_enabled(self, fn, where, have, first, count):
        n = have - first if count is None else count
        out = np.zeros(max(n, 0), dtype=np.uint8)
        if n == 0 and count is None:
            return out.astype(bool)
        self._check(fn(self._g, first, n, _ptr(out, _bp)), where)
        return out.astype(bool)

    def set_edges_enabled(self, enabled, first: int = 0):
        """sicp_graph_set_edges_enabled: switch the edges first, first + 1, ... on or off; a disabled edge keeps its id and is still
        reported by errors(), but contributes to nothing"""
        self._set_enabled(lib().sicp_graph_set_edges_enabled, "sicp_graph_set_edges_enabled", enabled, first)

    def edges_enabled(self, first: int = 0, count: int | None = None):
        """sicp_graph_get_edges_enabled: [count] bool (count = None: to the end)"""
        return self._get_enabled(lib().sicp_graph_get_edges_enabled, "sicp_graph_get_edges_enabled", self.counts()["edges"], first, count)

    def set_priors_enabled(self, enabled, first: int = 0):
        """sicp_graph_set_priors_enabled"""
        self._set_enabled(lib().sicp_graph_set_priors_enabled, "sicp_graph_set_priors_enabled", enabled, first)

    def priors_enabled(self, first: int = 0, count: int | None = None):
        """sicp_graph_get_priors_enabled: [count] bool (count = None: to the end)"""
        return self._get_enabled(lib().sicp_graph_get_priors_enabled, "sicp_graph_get_priors_enabled", self.counts()["priors"], first, count)

    def prior_errors(self):
        """sicp_graph_prior_errors at the current poses: {"chi2": [P], "residual": [P, 6] (a position prior: r, then three zeros),
        "weight": [P], "cost": the graph's whole cost}"""
        m = self.counts()["priors"]
        chi2, w, r = np.empty(m), np.empty(m), np.empty((m, 6))
        cost = C.c_double(0.0)
        self._check(lib().sicp_graph_prior_errors(self._g, _ptr(chi2, _dp), _ptr(r, _dp), _ptr(w, _dp), C.byref(cost)),
                    "sicp_graph_prior_errors")
        return {"chi2": chi2, "residual": r, "weight": w, "cost": cost.value}

    def counts(self):
        """sicp_graph_counts: {"nodes", "edges", "edges_enabled", "priors", "priors_enabled"}"""
        v = [C.c_int64(0) for _ in range(5)]
        self._check(lib().sicp_graph_counts(self._g, *[C.byref(x) for x in v]), "sicp_graph_counts")
        return dict(zip(("nodes", "edges", "edges_enabled", "priors", "priors_enabled"), (x.value for x in v)))

    def set_poses(self, qt, first: int = 0):
        q = self._poses(qt)
        self._check(lib().sicp_graph_set_poses(self._g, first, q.shape[0], _ptr(q, _dp)), "sicp_graph_set_poses")

    def poses(self, first: int = 0, count: int | None = None):
        """sicp_graph_get_poses: [count, 7] float64 (count = None: to the end)"""
        n = self.size()[0] - first if count is None else count
        out = np.empty((max(n, 0), 7), dtype=np.float64)
        if n == 0 and count is None:
            return out
        self._check(lib().sicp_graph_get_poses(self._g, first, n, _ptr(out, _dp)), "sicp_graph_get_poses")
        return out

    def set_fixed(self, fixed, first: int = 0):
        f = np.ascontiguousarray(np.atleast_1d(np.asarray(fixed, dtype=bool)), dtype=np.uint8)
        self._check(lib().sicp_graph_set_fixed(self._g, first, f.shape[0], _ptr(f, _bp)), "sicp_graph_set_fixed")

    def errors(self):
        """sicp_graph_errors at the current poses: {"chi2": [M], "residual": [M, 6], "weight": [M], "cost": float}"""
        m = self.size()[1]
        chi2, w, r = np.empty(m), np.empty(m), np.empty((m, 6))
        cost = C.c_double(0.0)
        self._check(lib().sicp_graph_errors(self._g, _ptr(chi2, _dp), _ptr(r, _dp), _ptr(w, _dp), C.byref(cost)), "sicp_graph_errors")
        return {"chi2": chi2, "residual": r, "weight": w, "cost": cost.value}

    def linearize(self):
        """sicp_graph_linearize at the current poses: {"gradient": [N, 6], "diag_blocks": [N, 6, 6], "cost": float}"""
        n = self.size()[0]
        g, H = np.empty((n, 6)), np.empty((n, 6, 6))
        cost = C.c_double(0.0)
        self._check(lib().sicp_graph_linearize(self._g, _ptr(g, _dp), _ptr(H, _dp), C.byref(cost)), "sicp_graph_linearize")
        return {"gradient": g, "diag_blocks": H, "cost": cost.value}

    def optimize(self):
        """sicp_graph_optimize: SicpGraphInfo.as_dict() (termination_name: one of GRAPH_TERMINATIONS)"""
        info = SicpGraphInfo()
        self._check(lib().sicp_graph_optimize(self._g, C.byref(info)), "sicp_graph_optimize")
        return info.as_dict()

    def _covariances(self, a, b, params):
        if params is not None:
            _check_graph_cov_params(params)
        bb = np.ascontiguousarray(np.atleast_1d(b), dtype=np.int32)
        n = bb.shape[0]
        cov, status, info = np.empty((n, 6, 6)), np.empty(n, dtype=np.int32), SicpGraphCovInfo()
        pp = None if params is None else C.byref(params)
        if a is None:
            self._check(lib().sicp_graph_marginals(self._g, pp, n, _ptr(bb, _ip), _ptr(cov, _dp), _ptr(status, _ip), C.byref(info)),
                        "sicp_graph_marginals")
        else:
            aa = np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32)
            if aa.shape != bb.shape:
                raise ValueError("a[n] and b[n] must agree on n")
            self._check(lib().sicp_graph_relative_covariances(self._g, pp, n, _ptr(aa, _ip), _ptr(bb, _ip), _ptr(cov, _dp),
                                                              _ptr(status, _ip), C.byref(info)), "sicp_graph_relative_covariances")
        return cov, status, info.as_dict()

    def marginals(self, nodes, params: SicpGraphCovParams | None = None):
        """sicp_graph_marginals: (cov [n, 6, 6], status [n] of GRAPH_COV_*, info dict).  cov[q] is the block of H^-1 at nodes[q],
        in the tangent space of T <- T exp(delta); NaN where the status is GRAPH_COV_UNANCHORED or GRAPH_COV_BREAKDOWN."""
        return self._covariances(None, nodes, params)

    def relative_covariances(self, a, b, params: SicpGraphCovParams | None = None):
        """sicp_graph_relative_covariances: (cov [n, 6, 6], status [n], info dict).  cov[q] is the covariance of T_a^-1 T_b under
        z exp(delta), the convention of an edge's omega: inv(cov[q] + pose_covariance(...)["covariance"]) gates
        log(z_graph^-1 z_measured) before add_edges."""
        return self._covariances(a, b, params)

    def size(self):
        """(nodes, edges)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(lib().sicp_graph_size(self._g, C.byref(a), C.byref(b)), "sicp_graph_size")
        return a.value, b.value

    def clear(self):
        self._check(lib().sicp_graph_clear(self._g), "sicp_graph_clear")


def accumulate_batch(engines, qts, repeat: int = 1):
    """sicp_accumulate_batch: the 28 sums of every engine's current correspondences from one launch
    (issued `repeat` times back to back for timing).  Returns (out28 [n, 28], kernel_ms per launch)."""
    n = len(engines)
    qts = np.ascontiguousarray(qts, dtype=np.float64).reshape(n, 7)
    out = np.empty((n, 28))
    ms = C.c_double(0.0)
    rc = lib().sicp_accumulate_batch(_handles(engines), n, _ptr(qts, _dp), _ptr(out, _dp), repeat, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"sicp_accumulate_batch failed: {_strerror(rc)} ({rc})")
    return out, ms.value


def search_batch(engines, qts=None, what: int = 0, use_hint: bool = True, repeat: int = 1):
    """sicp_search_batch: the search kernels of every engine as one job launch (what = 0 the K-correspondence
    search at poses qts, 1 / 2 the k_cov self-search of the source / target cloud, 3 the search of 0 with the EM weights
    in its epilogue as an align() launches it), issued `repeat` times.
    Returns kernel milliseconds per repetition (all engines' searches together)."""
    n = len(engines)
    if qts is None:
        qts = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64), (n, 1))
    qts = np.ascontiguousarray(qts, dtype=np.float64).reshape(n, 7)
    ms = C.c_double(0.0)
    rc = lib().sicp_search_batch(_handles(engines), n, _ptr(qts, _dp), what, 1 if use_hint else 0, repeat, C.byref(ms))
    if rc != 0:
        msgs = "; ".join(m for m in (lib().sicp_last_error(e._h).decode() for e in engines) if m)
        raise RuntimeError(f"sicp_search_batch failed: {_strerror(rc)} ({rc}) {msgs}")
    return ms.value


class Stream:
    """sicp_stream_*: an open sequence of registrations on one device (continuous batching without the closed
    batch).  add_cloud() uploads and indexes a scan once; submit() queues source -> target; poll() hands back
    finished registrations as (ticket, qt, stats) in order of completion."""

    def __init__(self, device: int, params: SicpParams, max_in_flight: int = 256, confusion=None):
        self._s = C.c_void_p()
        st = lib().sicp_stream_create(device, C.byref(params), max_in_flight, C.byref(self._s))
        if st != OK:
            self._s = C.c_void_p()
            raise SicpError(st, "sicp_stream_create")
        if confusion is not None:
            cm = np.ascontiguousarray(confusion, dtype=np.float64)
            self._check(lib().sicp_stream_set_confusion(self._s, cm.shape[0], _ptr(cm, _dp)), "sicp_stream_set_confusion")

    def _check(self, st, where):
        if st != OK:
            raise SicpError(st, where, lib().sicp_stream_last_error(self._s).decode())

    def close(self):
        if getattr(self, "_s", None) and self._s.value:
            lib().sicp_stream_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_cloud(self, xyz, labels=None) -> int:
        pts, lab = _points_and_labels(xyz, labels)   # float32 [n, 3] as it lies in memory: no per-column copies
        cid = C.c_int64(0)
        self._check(lib().sicp_stream_add_cloud_strided(self._s, pts.shape[0], pts.ctypes.data, pts.strides[0],
                                                        None if lab is None else lab.ctypes.data, 0 if lab is None else lab.strides[0], C.byref(cid)),
                    "sicp_stream_add_cloud_strided")
        return cid.value

    def release_cloud(self, cloud_id: int):
        self._check(lib().sicp_stream_release_cloud(self._s, cloud_id), "sicp_stream_release_cloud")

    def submit(self, source_id: int, target_id: int, init_qt=None, fused_labels: bool = False, fresh_features: bool = False,
               pose_covariance: bool = False) -> int:
        """fused_labels: getFusedLabels at the final pose comes with the result (take_labels); fresh_features: the
        normals / histograms of both clouds are recomputed for this registration, like an align() of the reference;
        pose_covariance: the sums of the pose covariance at the final pose come with the result (take_pose_covariance)"""
        init = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64) if init_qt is None else np.ascontiguousarray(init_qt, dtype=np.float64)
        t = C.c_int64(0)
        flags = ((SUBMIT_FUSED_LABELS if fused_labels else 0) | (SUBMIT_FRESH_FEATURES if fresh_features else 0) |
                 (SUBMIT_POSE_COVARIANCE if pose_covariance else 0))
        if flags:
            self._check(lib().sicp_stream_submit_ex(self._s, source_id, target_id, _ptr(init, _dp), flags, C.byref(t)), "sicp_stream_submit_ex")
        else:
            self._check(lib().sicp_stream_submit(self._s, source_id, target_id, _ptr(init, _dp), C.byref(t)), "sicp_stream_submit")
        return t.value

    def take_labels(self, ticket: int, n_source: int):
        out = np.empty(n_source, dtype=np.uint32)
        self._check(lib().sicp_stream_take_labels(self._s, ticket, n_source, _ptr(out, _up)), "sicp_stream_take_labels")
        return out

    def take_pose_covariance(self, ticket: int, sigma_source: float = 1.0, sigma_target: float = 1.0):
        """sicp_stream_take_pose_covariance: the dict of Engine.pose_covariance for a registration submitted with
        pose_covariance=True, once poll() has returned it; works once per ticket"""
        r = SicpPoseCovarianceResult()
        self._check(lib().sicp_stream_take_pose_covariance(self._s, ticket, sigma_source, sigma_target, C.byref(r)),
                    "sicp_stream_take_pose_covariance")
        return r.as_dict()

    def poll(self, wait: int = 0, max_results: int = 1024):
        buf = (SicpStreamResult * max_results)()
        n = C.c_int32(0)
        self._check(lib().sicp_stream_poll(self._s, wait, max_results, buf, C.byref(n)), "sicp_stream_poll")
        return [(r.ticket, r.status, np.array(r.qt[:]), r.stats.as_dict()) for r in buf[: n.value]]

    def drain(self):
        """everything submitted so far, finished"""
        out = self.poll(wait=2)
        while True:
            more = self.poll(wait=0)
            if not more:
                return out
            out += more

    def counters(self):
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(lib().sicp_stream_counters(self._s, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "sicp_stream_counters")
        return dict(submitted=a.value, completed=b.value, busy_evals=c.value, slot_evals=d.value,
                    busy_fraction=(c.value / d.value) if d.value else 0.0)
