"""ctypes mirror of include/lld_amd.h.

The struct layouts here are the single Python-side definition of the C ABI; the product library
(`lld_slam_amd/csrc/liblld_amd.so`, symbols ``lld_*``) and the test-only CPU oracle
(`oracle/liblld_oracle.so`, symbols ``lldo_*``) are both bound through :class:`Lib`.

Nothing in this module touches the oracle; see ``oracle/oracle_py.py`` for that loader (tests only).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
c_uint32_p = C.POINTER(C.c_uint32)
c_uint8_p = C.POINTER(C.c_uint8)

LLD_OK = 0
LLD_ERR_INVALID = -1
LLD_ERR_NO_DEVICE = -2
LLD_ERR_HIP = -3
LLD_ERR_ALLOC = -4
LLD_ERR_UNSUPPORTED = -5


class Camera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double)]


class BAWindow(C.Structure):
    _fields_ = [
        ("cam", Camera),
        ("n_cams", C.c_int32), ("n_free_cams", C.c_int32),
        ("cam_qt", c_double_p),
        ("n_points", C.c_int32),
        ("pt_xyz", c_double_p),
        ("pt_obs_start", c_int32_p),
        ("n_pt_obs", C.c_int32),
        ("pt_obs_cam", c_int32_p),
        ("pt_obs_uvr", c_double_p),
        ("pt_obs_inv_sigma2", c_double_p),
        ("n_lines", C.c_int32),
        ("line_x0", c_double_p),
        ("line_dir", c_double_p),
        ("ln_obs_start", c_int32_p),
        ("n_ln_obs", C.c_int32),
        ("ln_obs_cam", c_int32_p),
        ("ln_obs_left", c_double_p),
        ("ln_obs_right", c_double_p),
        ("ln_obs_octave", c_int32_p),
    ]


class LineStereoParams(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("b", C.c_double), ("tau", C.c_double), ("min_line_length", C.c_int32), ("is_stereo", C.c_int32)]


class LineTrackParams(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("T_curr", C.c_double * 16), ("b", C.c_double), ("thr_reproj_base", C.c_double), ("md_thr", C.c_double),
                ("sx", C.c_double), ("sy", C.c_double), ("monocular", C.c_int32), ("use_grid", C.c_int32)]


class LineLastKfParams(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("T_curr", C.c_double * 16), ("T_last", C.c_double * 16), ("b", C.c_double), ("thr_reproj_base", C.c_double),
                ("md_thr", C.c_double), ("sx", C.c_double), ("sy", C.c_double), ("use_grid", C.c_int32), ("pad", C.c_int32)]


class BAParams(C.Structure):
    _fields_ = [
        ("gamma", C.c_double),
        ("its_round1", C.c_int32), ("its_round2", C.c_int32), ("ln_filter", C.c_int32), ("max_trials", C.c_int32),
        ("pcg_rel_tol", C.c_double),
        ("pcg_max_iter", C.c_int32), ("reduced_solver", C.c_int32), ("protocol", C.c_int32), ("robust_points", C.c_int32),
        ("abort_after_trials", C.c_int32), ("deterministic", C.c_int32),
    ]


class BAStats(C.Structure):
    _fields_ = [
        ("chi2_round1", C.c_double), ("chi2_final", C.c_double),
        ("lm_iterations", C.c_int32 * 2), ("lm_trials", C.c_int32 * 2),
        ("pcg_iterations", C.c_int32), ("n_pt_obs_outlier", C.c_int32),
        ("n_ln_edge_outlier", C.c_int32), ("n_lines_removed", C.c_int32),
        ("aborted", C.c_int32), ("reserved", C.c_int32),
    ]


class BAResult(C.Structure):
    _fields_ = [
        ("cam_qt", c_double_p), ("pt_xyz", c_double_p), ("line_x0", c_double_p), ("line_dir", c_double_p),
        ("pt_obs_outlier", c_uint8_p), ("ln_edge_outlier", c_uint8_p), ("line_removed", c_uint8_p),
        ("stats", BAStats),
    ]


class PoseProblem(C.Structure):
    _fields_ = [
        ("cam", Camera),
        ("pose_qt", C.c_double * 7),
        ("n_points", C.c_int32),
        ("pt_xw", c_double_p), ("pt_uvr", c_double_p), ("pt_inv_sigma2", c_double_p),
        ("n_lines", C.c_int32),
        ("ln_x0", c_double_p), ("ln_dir", c_double_p), ("ln_left", c_double_p), ("ln_right", c_double_p),
        ("ln_octave", c_int32_p),
        ("ln_frame_index", c_int32_p),
    ]


class PoseParams(C.Structure):
    _fields_ = [("gamma", C.c_double), ("n_rounds", C.c_int32), ("its_per_round", C.c_int32),
                ("max_trials", C.c_int32), ("reserved", C.c_int32)]


class PoseResult(C.Structure):
    _fields_ = [
        ("pose_qt", C.c_double * 7),
        ("n_inliers", C.c_int32), ("lm_iterations", C.c_int32), ("lm_trials", C.c_int32), ("reserved", C.c_int32),
        ("chi2", C.c_double),
        ("pt_outlier", c_uint8_p), ("ln_outlier", c_uint8_p),
    ]


def _p(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def as_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# Every symbol include/lld_amd.h declares (checked by tests/test_abi.py against the built library).
class Sim3Problem(C.Structure):
    _fields_ = [("fx1", C.c_double), ("fy1", C.c_double), ("cx1", C.c_double), ("cy1", C.c_double),
                ("fx2", C.c_double), ("fy2", C.c_double), ("cx2", C.c_double), ("cy2", C.c_double),
                ("s12_q", C.c_double * 4), ("s12_t", C.c_double * 3), ("s12_s", C.c_double), ("n", C.c_int32), ("reserved", C.c_int32),
                ("p1c", c_double_p), ("p2c", c_double_p), ("obs1", c_double_p), ("obs2", c_double_p), ("inv_sigma2_1", c_double_p),
                ("inv_sigma2_2", c_double_p)]


class Sim3Params(C.Structure):
    _fields_ = [("th2", C.c_double), ("fix_scale", C.c_int32), ("its_first", C.c_int32), ("its_more_bad", C.c_int32),
                ("its_more_clean", C.c_int32), ("min_inliers", C.c_int32), ("max_trials", C.c_int32)]


class Sim3Result(C.Structure):
    _fields_ = [("s12_q", C.c_double * 4), ("s12_t", C.c_double * 3), ("s12_s", C.c_double), ("dropped", c_uint8_p), ("n_inliers", C.c_int32),
                ("n_bad_first", C.c_int32), ("lm_iterations", C.c_int32 * 2), ("lm_trials", C.c_int32 * 2), ("chi2", C.c_double)]


class PnPParams(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32),
                ("epsilon", C.c_float), ("th2", C.c_float)]


class PnPProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("xyz", c_float_p), ("uv", c_float_p), ("sigma2", c_float_p), ("kp_index", c_int32_p),
                ("n_keypoints", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("seed", C.c_uint32)]


class PnPResult(C.Structure):
    _fields_ = [("Tcw", C.c_float * 12), ("has_pose", C.c_int32), ("n_inliers", C.c_int32), ("no_more", C.c_int32),
                ("iterations", C.c_int32), ("best_inliers", C.c_int32), ("n_keypoints", C.c_int32), ("inlier", c_uint8_p)]


class PnPHypothesis(C.Structure):
    _fields_ = [("n_inliers", C.c_int32), ("record", C.c_int32), ("refine", C.c_int32), ("refined_inliers", C.c_int32),
                ("R", C.c_double * 9), ("t", C.c_double * 3)]


class Sim3SolverParams(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32)]


class Sim3SolverProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("xyz1", c_float_p), ("xyz2", c_float_p), ("sigma2_1", c_float_p), ("sigma2_2", c_float_p),
                ("index1", c_int32_p), ("n1", C.c_int32), ("Rcw1", C.c_float * 9), ("tcw1", C.c_float * 3), ("Rcw2", C.c_float * 9),
                ("tcw2", C.c_float * 3), ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float), ("fix_scale", C.c_int32),
                ("seed", C.c_uint32)]


class Sim3SolverResult(C.Structure):
    _fields_ = [("T12", C.c_float * 12), ("R", C.c_float * 9), ("t", C.c_float * 3), ("s", C.c_float), ("has_pose", C.c_int32),
                ("n_inliers", C.c_int32), ("no_more", C.c_int32), ("iterations", C.c_int32), ("best_inliers", C.c_int32),
                ("n1", C.c_int32), ("inlier", c_uint8_p)]


class Sim3SolverHypothesis(C.Structure):
    _fields_ = [("n_inliers", C.c_int32), ("record", C.c_int32), ("idx", C.c_int32 * 3), ("s", C.c_float), ("R", C.c_float * 9),
                ("t", C.c_float * 3), ("T12", C.c_float * 12)]


class InitializerParams(C.Structure):
    _fields_ = [("sigma", C.c_float), ("iterations", C.c_int32), ("min_parallax", C.c_float), ("min_triangulated", C.c_int32),
                ("seed", C.c_uint32)]


class InitializerResult(C.Structure):
    _fields_ = [("success", C.c_int32), ("model", C.c_int32), ("SH", C.c_float), ("SF", C.c_float), ("RH", C.c_float),
                ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("n_inliers_H", C.c_int32), ("n_inliers_F", C.c_int32),
                ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("n_good", C.c_int32 * 8), ("parallax", C.c_float * 8),
                ("best_index", C.c_int32), ("n_matches", C.c_int32), ("win_H", C.c_int32), ("win_F", C.c_int32),
                ("inlier_H", c_uint8_p), ("inlier_F", c_uint8_p), ("p3d", c_float_p), ("triangulated", c_uint8_p)]


class InitializerHypothesis(C.Structure):
    _fields_ = [("idx", C.c_int32 * 8), ("M", C.c_float * 9), ("score", C.c_float), ("n_inliers", C.c_int32)]


class MapPointRefreshIn(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_obs", C.c_int32), ("n_kf", C.c_int32), ("n_levels", C.c_int32), ("flags", C.c_uint32),
                ("obs_start", c_int32_p), ("obs_kf", c_int32_p), ("obs_desc", c_uint32_p), ("kf_ow", c_float_p), ("kf_bad", c_uint8_p),
                ("pos", c_float_p), ("bad", c_uint8_p), ("ref_kf", c_int32_p), ("ref_level", c_int32_p), ("level_scale", c_float_p)]


class MapPointRefreshOut(C.Structure):
    _fields_ = [("desc", c_uint32_p), ("best_obs", c_int32_p), ("best_median", c_int32_p), ("normal", c_float_p),
                ("min_distance", c_float_p), ("max_distance", c_float_p), ("updated", c_uint8_p)]


class MapLineDistinctiveIn(C.Structure):
    _fields_ = [("n_lines", C.c_int32), ("n_obs", C.c_int32), ("n_kf", C.c_int32), ("dim", C.c_int32), ("obs_start", c_int32_p),
                ("obs_kf", c_int32_p), ("obs_desc", c_float_p), ("kf_bad", c_uint8_p), ("bad", c_uint8_p)]


class MapLineDistinctiveOut(C.Structure):
    _fields_ = [("desc", c_float_p), ("best_obs", c_int32_p), ("best_median", c_int32_p), ("updated", c_uint8_p)]


class NewPointsKf(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mb", C.c_float), ("mbf", C.c_float), ("scale_factor", C.c_float), ("median_depth", C.c_float), ("n_levels", C.c_int32),
                ("scale_factors", C.c_float * 16), ("level_sigma2", C.c_float * 16)]


class NewPointsIn(C.Structure):
    _fields_ = [("kf1", NewPointsKf), ("monocular", C.c_int32), ("n_keys1", C.c_int32), ("keys1_xy", c_float_p), ("keys1_raw_xy", c_float_p),
                ("ur1", c_float_p), ("depth1", c_float_p), ("octave1", c_int32_p), ("n_pairs", C.c_int32), ("reserved", C.c_int32),
                ("kf2", C.POINTER(NewPointsKf)), ("key_start", c_int32_p), ("keys2_xy", c_float_p), ("keys2_raw_xy", c_float_p),
                ("ur2", c_float_p), ("depth2", c_float_p), ("octave2", c_int32_p), ("match_start", c_int32_p), ("matches", c_int32_p)]


class NewPointsOut(C.Structure):
    _fields_ = [("status", c_uint8_p), ("source", c_uint8_p), ("x3d", c_float_p), ("pair_status", c_uint8_p), ("n_new", c_int32_p),
                ("new_match", c_int32_p), ("n_new_total", C.c_int32)]


class CovisibilityParams(C.Structure):
    _fields_ = [("th", C.c_int32), ("th_obs", C.c_int32), ("redundant_ratio", C.c_double)]


class CovisibilityIn(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32), ("n_queries", C.c_int32), ("n_entries", C.c_int32),
                ("monocular", C.c_int32), ("flags", C.c_uint32), ("params", CovisibilityParams), ("obs_start", c_int32_p),
                ("obs_kf", c_int32_p), ("obs_octave", c_int32_p), ("point_bad", c_uint8_p), ("point_nobs", c_int32_p),
                ("query_kf", c_int32_p), ("q_start", c_int32_p), ("q_point", c_int32_p), ("q_octave", c_int32_p), ("q_depth", c_float_p),
                ("q_th_depth", c_float_p)]


class CovisibilityOut(C.Structure):
    _fields_ = [("conn_capacity", C.c_int32), ("ordered_capacity", C.c_int32), ("n_conn", C.c_int32), ("n_ordered", C.c_int32),
                ("conn_start", c_int32_p), ("conn_kf", c_int32_p), ("conn_weight", c_int32_p), ("ordered_start", c_int32_p),
                ("ordered_kf", c_int32_p), ("ordered_weight", c_int32_p), ("n_max", c_int32_p), ("kf_max", c_int32_p),
                ("updated", c_uint8_p), ("n_mps", c_int32_p), ("n_redundant", c_int32_p), ("redundant", c_uint8_p),
                ("phase_ms", c_float_p)]


class MapCorrPoints(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_obs", C.c_int32), ("n_levels", C.c_int32), ("reserved", C.c_int32), ("pos", c_float_p),
                ("bad", c_uint8_p), ("obs_start", c_int32_p), ("obs_kf", c_int32_p), ("ref_kf", c_int32_p), ("ref_level", c_int32_p),
                ("level_scale", c_float_p)]


class LoopCorrectIn(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_conn", C.c_int32), ("cur", C.c_int32), ("n_entries", C.c_int32), ("kf_tcw", c_float_p),
                ("conn", c_int32_p), ("scw", c_double_p), ("kf_start", c_int32_p), ("kf_point", c_int32_p), ("already", c_uint8_p),
                ("points", MapCorrPoints)]


class LoopCorrectOut(C.Structure):
    _fields_ = [("corrected_sim3", c_double_p), ("non_corrected_sim3", c_double_p), ("tiw_corrected", c_float_p),
                ("ow_corrected", c_float_p), ("scw_f32", c_float_p), ("pos", c_float_p), ("corrected_by", c_int32_p), ("normal", c_float_p),
                ("min_distance", c_float_p), ("max_distance", c_float_p), ("updated", c_uint8_p)]


class EssentialGraphApplyIn(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("reserved", C.c_int32), ("sim3_before", c_double_p), ("sim3_after", c_double_p),
                ("corr_kf", c_int32_p), ("points", MapCorrPoints)]


class EssentialGraphApplyOut(C.Structure):
    _fields_ = [("tiw", c_float_p), ("ow", c_float_p), ("pos", c_float_p), ("normal", c_float_p), ("min_distance", c_float_p),
                ("max_distance", c_float_p), ("updated", c_uint8_p)]


class GlobalBAApplyIn(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_origins", C.c_int32), ("n_points", C.c_int32), ("reserved", C.c_int32), ("kf_tcw", c_float_p),
                ("kf_in_gba", c_uint8_p), ("kf_tcw_gba", c_float_p), ("parent", c_int32_p), ("origins", c_int32_p), ("pos", c_float_p),
                ("bad", c_uint8_p), ("in_gba", c_uint8_p), ("pos_gba", c_float_p), ("ref_kf", c_int32_p)]


class GlobalBAApplyOut(C.Structure):
    _fields_ = [("visited", c_uint8_p), ("tcw_new", c_float_p), ("tcw_before", c_float_p), ("ow_new", c_float_p), ("pos", c_float_p),
                ("moved", c_uint8_p)]


class PoseGraph(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("sim3", c_double_p), ("fixed", c_uint8_p), ("edge_i", c_int32_p),
                ("edge_j", c_int32_p), ("edge_sji", c_double_p)]


class PoseGraphParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("fix_scale", C.c_int32), ("lambda_init", C.c_double), ("max_trials", C.c_int32),
                ("pcg_max_iter", C.c_int32), ("pcg_rel_tol", C.c_double), ("solver", C.c_int32), ("reserved", C.c_int32)]


class PoseGraphResult(C.Structure):
    _fields_ = [("sim3", c_double_p), ("chi2", C.c_double), ("lm_iterations", C.c_int32), ("lm_trials", C.c_int32), ("pcg_iterations", C.c_int32),
                ("solver_used", C.c_int32)]


class FrameStereoParams(C.Structure):
    """lld_frame_stereo_params (include/lld_amd.h): the constants of a stereo Frame built on the device."""
    _fields_ = [("grid_min_x", C.c_float), ("grid_min_y", C.c_float), ("grid_width_inv", C.c_float), ("grid_height_inv", C.c_float),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("mb", C.c_float), ("mbf", C.c_float),
                ("left_angle", c_float_p), ("right_angle", c_float_p), ("keypoints_on_device", C.c_int32), ("n_levels", C.c_int32),
                ("level_scale", c_float_p), ("level_sigma2", c_float_p), ("level_inv_sigma2", c_float_p)]


class FrameMonoParams(C.Structure):
    """lld_frame_mono_params (include/lld_amd.h): the constants of an RGB-D or monocular Frame built on the device."""
    _fields_ = [("grid_min_x", C.c_float), ("grid_min_y", C.c_float), ("grid_width_inv", C.c_float), ("grid_height_inv", C.c_float),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("dist", C.c_float * 5), ("n_dist", C.c_int32), ("mbf", C.c_float), ("keypoints_on_device", C.c_int32), ("n_levels", C.c_int32),
                ("reserved", C.c_int32), ("left_angle", c_float_p), ("level_scale", c_float_p), ("level_sigma2", c_float_p),
                ("level_inv_sigma2", c_float_p)]


class DepthImage(C.Structure):
    """lld_depth_image (include/lld_amd.h): imDepth as GrabImageRGBD receives it, before convertTo."""
    _fields_ = [("data", C.c_void_p), ("cols", C.c_int32), ("rows", C.c_int32), ("step", C.c_int32), ("type", C.c_int32), ("factor", C.c_float),
                ("on_device", C.c_int32)]


DEPTH_F32, DEPTH_U16 = 0, 1


class RefKeyFrame(C.Structure):
    """lld_ref_keyframe (include/lld_amd.h): mpReferenceKF as lld_frame_track_reference_keyframe reads it."""
    _fields_ = [("n", C.c_int32), ("desc", c_uint32_p), ("angle", c_float_p), ("point_id", c_int32_p), ("world_pos", c_float_p),
                ("has_obs", c_uint8_p), ("n_nodes", C.c_int32), ("node", c_int32_p), ("node_start", c_int32_p), ("feature", c_int32_p)]


class RelocCandidate(C.Structure):
    """lld_reloc_candidate (include/lld_amd.h): what lld_frame_relocalize needs of a candidate keyframe beyond lld_ref_keyframe."""
    _fields_ = [("max_distance", c_float_p), ("min_distance", c_float_p), ("point_desc", c_uint32_p), ("is_bad", C.c_int32), ("seed", C.c_uint32)]


class RelocResult(C.Structure):
    """lld_reloc_result (include/lld_amd.h)."""
    _fields_ = [("matched", C.c_int32), ("winner", C.c_int32), ("round", C.c_int32), ("n_good", C.c_int32), ("n_rounds", C.c_int32), ("n_kept", C.c_int32),
                ("Tcw", C.c_float * 16),
                ("n_bow", c_int32_p), ("discarded", c_uint8_p), ("rounds", c_int32_p), ("n_good_last", c_int32_p), ("rungs", c_int32_p),
                ("n_additional1", c_int32_p), ("n_additional2", c_int32_p)]


class FrameLinesBuild(C.Structure):
    """lld_frame_lines_build (include/lld_amd.h): both line sets with both descriptor sets, and TwoFrameLineMatcher's parameters."""
    _fields_ = [("n_left", C.c_int32), ("left", c_float_p), ("left_octave", c_int32_p), ("desc_left", c_float_p),
                ("n_right", C.c_int32), ("right", c_float_p), ("right_octave", c_int32_p), ("desc_right", c_float_p),
                ("dim", C.c_int32), ("reserved", C.c_int32), ("sx", C.c_double), ("sy", C.c_double), ("stereo", LineStereoParams)]


class FrameNewLinesParams(C.Structure):
    """lld_frame_new_lines_params."""
    _fields_ = [("thr_reproj_base", C.c_double), ("md_thr", C.c_double), ("use_grid", C.c_int32), ("first_new_id", C.c_int32)]


class FrameNewLinesResult(C.Structure):
    """lld_frame_new_lines_result."""
    _fields_ = [("n_created", C.c_int32), ("n_held", C.c_int32), ("match_last", c_int32_p), ("created", c_uint8_p), ("x0", c_double_p),
                ("dir", c_double_p), ("new_id", c_int32_p)]


class FrameFinishParams(C.Structure):
    """lld_frame_finish_params (include/lld_amd.h): mThDepth, MapPoint::nNextId and NeedNewKeyFrame's scalars."""
    _fields_ = [("th_depth", C.c_float), ("first_new_id", C.c_int32), ("force", C.c_int32), ("only_tracking", C.c_int32), ("mapper_stopped", C.c_int32),
                ("mapper_idle", C.c_int32), ("keyframes_in_queue", C.c_int32), ("set_not_stop_ok", C.c_int32), ("monocular", C.c_int32),
                ("max_frames", C.c_int32), ("min_frames", C.c_int32), ("n_keyframes", C.c_int32), ("n_ref_matches", C.c_int32),
                ("n_matches_inliers", C.c_int32), ("sensor_rgbd", C.c_int32), ("reserved", C.c_int32), ("frame_id", C.c_int64), ("last_reloc_frame_id", C.c_int64), ("last_keyframe_id", C.c_int64),
                ("depth", c_float_p)]


class FrameFinishResult(C.Structure):
    """lld_frame_finish_result."""
    _fields_ = [("n_tracked_close", C.c_int32), ("n_non_tracked_close", C.c_int32), ("need", C.c_int32), ("interrupt_ba", C.c_int32), ("made", C.c_int32),
                ("n_visited", C.c_int32), ("n_created", C.c_int32), ("reserved", C.c_int32), ("created", c_uint8_p), ("new_id", c_int32_p),
                ("x3d", c_float_p), ("kp_point_id", c_int32_p), ("order", c_int32_p)]


class FramePointsParams(C.Structure):
    """lld_frame_points_params: params / view are lld_track_params* / lld_frame_view* (the structs of tracking.py / orb_search.py by reference)."""
    _fields_ = [("mode", C.c_int32), ("th_depth", C.c_float), ("first_new_id", C.c_int32), ("reserved", C.c_int32), ("params", C.c_void_p),
                ("view", C.c_void_p), ("pose_qt", c_double_p), ("depth", c_float_p)]


class MapLimits(C.Structure):
    """lld_map_limits."""
    _fields_ = [("max_keyframes", C.c_int32), ("max_points", C.c_int32), ("max_lines", C.c_int32), ("line_dim", C.c_int32), ("max_observations", C.c_int32),
                ("max_kf_points", C.c_int32), ("max_kf_lines", C.c_int32), ("max_children", C.c_int32), ("max_local_points", C.c_int32),
                ("max_local_lines", C.c_int32)]


class LocalMapResult(C.Structure):
    """lld_local_map_result: stage1 / stage2 are lld_track_result* (tracking.TrackResult by reference)."""
    _fields_ = [("status", C.c_int32), ("n_voted", C.c_int32), ("n_local_keyframes", C.c_int32), ("n_local_points", C.c_int32), ("n_local_lines", C.c_int32),
                ("n_bad_cleared", C.c_int32), ("ref_keyframe", C.c_int32), ("vote_empty", C.c_int32), ("stage2_ran", C.c_int32), ("reserved", C.c_int32),
                ("local_keyframes", c_int32_p), ("local_points", c_int32_p), ("local_lines", c_int32_p), ("mp_in_view", c_uint8_p),
                ("stage1", C.c_void_p), ("stage2", C.c_void_p)]


class MapCovisibilityIn(C.Structure):
    """lld_map_covisibility_in."""
    _fields_ = [("n_queries", C.c_int32), ("monocular", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_int32), ("params", CovisibilityParams),
                ("kf_slot", c_int32_p)]


class MapCovisibilityOut(C.Structure):
    """lld_map_covisibility_out."""
    _fields_ = [("lists", CovisibilityOut), ("status", c_uint8_p)]


class MapBaIn(C.Structure):
    """lld_map_ba_in."""
    _fields_ = [("n_keyframes", C.c_int32), ("n_levels", C.c_int32), ("kf_slot", c_int32_p), ("inv_level_sigma2", c_float_p), ("cam", Camera)]


class MapBaWindowOut(C.Structure):
    """lld_map_ba_window_out."""
    _fields_ = [("cam_capacity", C.c_int32), ("point_capacity", C.c_int32), ("pt_obs_capacity", C.c_int32), ("line_capacity", C.c_int32),
                ("ln_obs_capacity", C.c_int32),
                ("n_cams", C.c_int32), ("n_free_cams", C.c_int32), ("n_local_cams", C.c_int32), ("n_points", C.c_int32), ("n_pt_obs", C.c_int32),
                ("n_lines", C.c_int32), ("n_ln_obs", C.c_int32), ("status", C.c_int32),
                ("cam_slot", c_int32_p), ("cam_qt", c_double_p), ("point_slot", c_int32_p), ("pt_xyz", c_double_p), ("pt_obs_start", c_int32_p),
                ("pt_obs_cam", c_int32_p), ("pt_obs_uvr", c_double_p), ("pt_obs_inv_sigma2", c_double_p),
                ("line_slot", c_int32_p), ("line_x0", c_double_p), ("line_dir", c_double_p), ("ln_obs_start", c_int32_p), ("ln_obs_cam", c_int32_p),
                ("ln_obs_left", c_double_p), ("ln_obs_right", c_double_p), ("ln_obs_octave", c_int32_p), ("phase_ms", c_float_p)]


class MapBaIds(C.Structure):
    """lld_map_ba_ids."""
    _fields_ = [("status", C.c_int32), ("n_local_cams", C.c_int32), ("cam_slot", c_int32_p), ("point_slot", c_int32_p), ("line_slot", c_int32_p),
                ("n_marked_bad", C.c_int32), ("reserved", C.c_int32), ("marked_bad_slot", c_int32_p), ("window", BAWindow)]


class MapBaApplyIn(C.Structure):
    """lld_map_ba_apply_in."""
    _fields_ = [("n_cams", C.c_int32), ("n_points", C.c_int32), ("n_pt_obs", C.c_int32), ("n_lines", C.c_int32), ("n_ln_obs", C.c_int32), ("n_levels", C.c_int32),
                ("cam_qt", c_double_p), ("pt_xyz", c_double_p), ("line_x0", c_double_p), ("line_dir", c_double_p),
                ("pt_obs_outlier", c_uint8_p), ("ln_edge_outlier", c_uint8_p), ("line_removed", c_uint8_p), ("level_scale", c_float_p)]


class MapBaApplyOut(C.Structure):
    """lld_map_ba_apply_out."""
    _fields_ = [("n_local_cams", C.c_int32), ("n_pt_obs_erased", C.c_int32), ("n_ln_obs_erased", C.c_int32), ("n_points_bad", C.c_int32),
                ("n_lines_bad", C.c_int32), ("n_index_skipped", C.c_int32),
                ("tcw", c_float_p), ("ow", c_float_p), ("pt_pos", c_float_p), ("pt_normal", c_float_p), ("pt_min_distance", c_float_p),
                ("pt_max_distance", c_float_p), ("pt_n_obs", c_int32_p), ("pt_ref_kf", c_int32_p), ("pt_row_len", c_int32_p), ("pt_flags", c_uint8_p),
                ("ln_bad", c_uint8_p), ("ln_n_obs", c_int32_p), ("ln_row_len", c_int32_p), ("phase_ms", c_float_p)]


class MapRefreshPointsIn(C.Structure):
    """lld_map_refresh_points_in."""
    _fields_ = [("n", C.c_int32), ("flags", C.c_uint32), ("n_levels", C.c_int32), ("reserved", C.c_int32), ("slot", c_int32_p), ("level_scale", c_float_p)]


class MapRefreshPointsOut(C.Structure):
    """lld_map_refresh_points_out."""
    _fields_ = [("desc", c_uint32_p), ("best_obs", c_int32_p), ("best_median", c_int32_p), ("normal", c_float_p), ("min_distance", c_float_p),
                ("max_distance", c_float_p), ("updated", c_uint8_p), ("phase_ms", c_float_p)]


class MapRefreshLinesIn(C.Structure):
    """lld_map_refresh_lines_in."""
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("slot", c_int32_p)]


class MapRefreshLinesOut(C.Structure):
    """lld_map_refresh_lines_out."""
    _fields_ = [("desc", c_float_p), ("best_obs", c_int32_p), ("best_median", c_int32_p), ("updated", c_uint8_p), ("phase_ms", c_float_p)]


class FrameViewStruct(C.Structure):
    """lld_frame_view (orb_search.FrameView has the same layout; orb_search imports this module, so lld_map_fuse_in embeds this one)."""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float), ("log_scale_factor", C.c_float), ("n_levels", C.c_int32)]


class MapFuseIn(C.Structure):
    """lld_map_fuse_in."""
    _fields_ = [("target", C.c_int32), ("n_points", C.c_int32), ("point_slot", c_int32_p), ("source_keyframe", C.c_int32), ("th", C.c_float),
                ("view", FrameViewStruct), ("grid_min_x", C.c_float), ("grid_min_y", C.c_float), ("grid_width_inv", C.c_float), ("grid_height_inv", C.c_float),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("n_levels", C.c_int32), ("reserved", C.c_int32),
                ("level_scale", c_float_p), ("level_inv_sigma2", c_float_p)]


class MapFuseOut(C.Structure):
    """lld_map_fuse_out."""
    _fields_ = [("n_fused", C.c_int32), ("n_added", C.c_int32), ("n_replaced", C.c_int32), ("reserved", C.c_int32),
                ("match", c_int32_p), ("action", c_uint8_p), ("other", c_int32_p), ("survivor_capacity", C.c_int32), ("n_survivors", C.c_int32),
                ("survivor", c_int32_p), ("phase_ms", c_float_p)]


MAP_FUSE_NONE, MAP_FUSE_ADDED, MAP_FUSE_CANDIDATE_REPLACED, MAP_FUSE_HOLDER_REPLACED, MAP_FUSE_HOLDER_BAD, MAP_FUSE_SKIPPED = 0, 1, 2, 3, 4, 5
LANDMARK_DESCRIPTOR, LANDMARK_NORMAL_DEPTH = 1, 2
LANDMARK_MAX_OBS, LANDMARK_MAX_LINE_OBS = 1024, 64
ORB_MAX_LEVELS = 16
MAP_REFRESH_NO_INDEX, MAP_REFRESH_NO_DESCRIPTOR, MAP_REFRESH_NO_REFERENCE = 4, 8, 16
MAP_BA_MAX_LOCAL = 1024
MAP_BA_NO_FEATURE_DATA = 1
MAP_APPLY_WENT_BAD, MAP_APPLY_REFRESHED, MAP_APPLY_NO_REFERENCE, MAP_APPLY_INDEX_SKIPPED = 1, 2, 4, 8
MAP_ROWS = dict(point_obs=0, point_idx=1, kf_points=2, kf_lines=3, line_obs=4, line_idx=5)
MAP_COVIS_MAX_CONNECTED = 4096
MAP_COVIS_WRITE_COV = 4
MAP_COVIS_CONN_OVERFLOW, MAP_COVIS_NO_KEYPOINT_DATA = 1, 2
LOCAL_MAP_KEYFRAME_OVERFLOW, LOCAL_MAP_POINT_OVERFLOW, LOCAL_MAP_LINE_OVERFLOW = 1, 2, 4
MAP_MAX_LOCAL_KEYFRAMES = 1280
POINTS_LAST_FRAME, POINTS_INITIALIZATION = 0, 1
RELOC_RUNG_POSE1, RELOC_RUNG_SEARCH1, RELOC_RUNG_POSE2, RELOC_RUNG_SEARCH2, RELOC_RUNG_POSE3 = 1, 2, 4, 8, 16


PRODUCT_SYMBOLS = [
    "lld_status_string", "lld_ctx_create", "lld_ctx_destroy", "lld_ctx_stream", "lld_ctx_synchronize", "lld_ctx_release_cache",
    "lld_se3_from_tcw_f32", "lld_se3_to_tcw_f32", "lld_orb_inv_level_sigma2",
    "lld_ba_params_default", "lld_local_ba",
    "lld_local_ba_stopflag", "lld_ba_batch_create", "lld_ba_batch_solve", "lld_ba_batch_download", "lld_ba_batch_download_range", "lld_ba_batch_stats",
    "lld_ba_batch_result_records", "lld_ba_batch_set_phase_timing", "lld_ba_batch_phase_ms", "lld_ba_batch_kernel_stats", "lld_ba_batch_set_groups",
    "lld_ba_batch_destroy", "lld_ba_chol_plan",
    "lld_device_count", "lld_ba_multi_shard", "lld_ba_multi_create", "lld_ba_multi_solve", "lld_ba_multi_result_records", "lld_ba_multi_verify_gathered",
    "lld_ba_multi_download", "lld_ba_multi_times_ms", "lld_ba_multi_destroy",
    "lld_pose_params_default", "lld_pose_opt",
    "lld_pose_batch_create", "lld_pose_batch_solve", "lld_pose_batch_download", "lld_pose_batch_destroy",
    "lld_match_hamming256", "lld_match_hamming256_csr", "lld_match_hamming256_batch_dev",
    "lld_match_l2f32", "lld_match_l2f32_batch_dev", "lld_line_match_greedy", "lld_line_match_stereo",
    "lld_line_track_match", "lld_line_hough_cells", "lld_line_match_last_frame",
    "lld_orb_search_run", "lld_orb_search_batch", "lld_orb_search_local_points", "lld_orb_search_last_frame", "lld_orb_fuse_search", "lld_orb_search_projected", "lld_orb_search_by_sim3",
    "lld_compute_stereo_matches",
    "lld_frame_create", "lld_frame_search_last_frame", "lld_frame_search_local_points", "lld_frame_destroy",
    "lld_frame_set_lines", "lld_track_params_default", "lld_frame_track_motion_model", "lld_frame_track_local_map", "lld_frame_track_download", "lld_frame_track_set_state",
    "lld_frame_compute_bow", "lld_frame_track_reference_keyframe", "lld_frame_relocalize",
    "lld_frame_build_lines", "lld_frame_lines_download", "lld_frame_new_map_lines",
    "lld_frame_track_finish", "lld_frame_create_stereo_points",
    "lld_sim3_params_default", "lld_optimize_sim3", "lld_optimize_sim3_batch",
    "lld_pose_graph_params_default", "lld_optimize_essential_graph",
    "lld_orb_extractor_create", "lld_orb_extractor_destroy", "lld_orb_extractor_levels_get", "lld_orb_extract", "lld_orb_extractor_pyramids",
    "lld_orb_extractor_descriptors",
    "lld_bow_vocab_read_text", "lld_bow_vocab_create", "lld_bow_vocab_destroy", "lld_bow_vocab_info_get", "lld_bow_transform", "lld_bow_score",
    "lld_kfdb_create", "lld_kfdb_destroy", "lld_kfdb_add", "lld_kfdb_erase", "lld_kfdb_clear", "lld_kfdb_set_covisibles",
    "lld_kfdb_detect_loop_candidates", "lld_kfdb_detect_relocalization_candidates",
    "lld_pnp_params_default", "lld_pnp_batch_create", "lld_pnp_batch_iterate", "lld_pnp_batch_download", "lld_pnp_batch_hypotheses",
    "lld_pnp_batch_destroy", "lld_pnp_find", "lld_pnp_batch_find",
    "lld_sim3solver_params_default", "lld_sim3solver_batch_create", "lld_sim3solver_batch_iterate", "lld_sim3solver_batch_find",
    "lld_sim3solver_batch_download", "lld_sim3solver_batch_hypotheses", "lld_sim3solver_batch_destroy", "lld_sim3solver_find",
    "lld_initializer_params_default", "lld_initializer_create", "lld_initializer_initialize", "lld_initializer_hypotheses",
    "lld_initializer_destroy", "lld_initializer_find",
    "lld_mappoint_refresh", "lld_mapline_distinctive",
    "lld_new_points_triangulate",
    "lld_covisibility_params_default", "lld_covisibility",
    "lld_loop_correct", "lld_essential_graph_apply", "lld_global_ba_apply",
    "lld_frame_build_stereo_keypoints", "lld_frame_build_stereo", "lld_frame_stereo_download",
    "lld_frame_build_mono_keypoints", "lld_frame_build_mono", "lld_frame_keypoints_download", "lld_frame_image_bounds",
    "lld_map_create", "lld_map_destroy", "lld_map_clear", "lld_map_set_points", "lld_map_set_observations", "lld_map_set_keyframes", "lld_map_set_lines",
    "lld_frame_track_update_local_map", "lld_frame_track_local_map_resident", "lld_frame_local_map_download",
    "lld_map_set_observations_indexed", "lld_map_set_keyframe_keypoints", "lld_map_set_covisibles", "lld_map_covisibility", "lld_map_download_links",
    "lld_map_set_keyframe_features", "lld_map_set_keyframe_poses", "lld_map_set_line_observations", "lld_map_ba_window", "lld_map_local_ba",
    "lld_map_set_point_refs", "lld_map_ba_apply", "lld_map_download_rows",
    "lld_map_set_keyframe_descriptors", "lld_map_set_keyframe_line_descriptors", "lld_map_refresh_points", "lld_map_refresh_lines",
    "lld_map_download_points", "lld_map_download_lines",
    "lld_map_fuse", "lld_map_download_point_counts",
]


def product_library_path() -> str:
    if os.environ.get("LLD_AMD_LIB"):          # kernel experiments: an alternative build of the same ABI
        return os.environ["LLD_AMD_LIB"]
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "liblld_amd.so")


class Lib:
    """Thin typed view over one shared library exporting the ABI with a given symbol prefix."""

    def __init__(self, path: str, prefix: str):
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                "There is no fallback path.")
        self.path = path
        self.prefix = prefix
        self.dll = C.CDLL(path)
        self._bind()

    def fn(self, name):
        return getattr(self.dll, self.prefix + name)

    def has(self, name) -> bool:
        try:
            self.fn(name)
            return True
        except AttributeError:
            return False

    def _bind(self):
        vp = C.c_void_p
        f = self.fn
        f("se3_from_tcw_f32").argtypes = [c_float_p, c_double_p]; f("se3_from_tcw_f32").restype = None
        f("se3_to_tcw_f32").argtypes = [c_double_p, c_float_p]; f("se3_to_tcw_f32").restype = None
        f("orb_inv_level_sigma2").argtypes = [C.c_float, C.c_int, c_float_p]; f("orb_inv_level_sigma2").restype = None
        f("ba_params_default").argtypes = [C.POINTER(BAParams)]; f("ba_params_default").restype = None
        f("pose_params_default").argtypes = [C.POINTER(PoseParams)]; f("pose_params_default").restype = None
        f("local_ba").argtypes = [vp, C.POINTER(BAWindow), C.POINTER(BAParams), C.POINTER(C.c_int), C.POINTER(BAResult)]
        f("local_ba").restype = C.c_int
        f("pose_opt").argtypes = [vp, C.POINTER(PoseProblem), C.POINTER(PoseParams), C.POINTER(PoseResult)]
        f("pose_opt").restype = C.c_int
        f("match_hamming256").argtypes = [vp, c_uint32_p, C.c_int, c_uint32_p, C.c_int, c_uint8_p,
                                          c_int32_p, c_int32_p, c_int32_p, c_int32_p]
        f("match_hamming256").restype = C.c_int
        f("match_hamming256_csr").argtypes = [vp, c_uint32_p, C.c_int, c_uint32_p, C.c_int, c_int32_p, c_int32_p,
                                              c_int32_p, c_int32_p, c_int32_p, c_int32_p]
        f("match_hamming256_csr").restype = C.c_int
        f("match_l2f32").argtypes = [vp, c_float_p, C.c_int, c_float_p, C.c_int, C.c_int, c_uint8_p,
                                     c_int32_p, c_double_p, c_int32_p, c_double_p]
        f("match_l2f32").restype = C.c_int
        f("line_match_greedy").argtypes = [vp, c_float_p, C.c_int, c_float_p, C.c_int, C.c_int, c_uint8_p, C.c_double,
                                           c_int32_p, c_double_p]
        f("line_match_greedy").restype = C.c_int
        f("line_match_stereo").argtypes = [vp, C.POINTER(LineStereoParams), c_float_p, c_int32_p, c_float_p, C.c_int, c_float_p, c_int32_p,
                                           c_float_p, C.c_int, C.c_int, c_int32_p, c_double_p, c_uint8_p]
        f("line_match_stereo").restype = C.c_int
        f("line_track_match").argtypes = [vp, C.POINTER(LineTrackParams), C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p, c_float_p,
                                          C.c_int, c_float_p, c_int32_p, C.c_int, c_float_p, c_int32_p, c_uint8_p, c_float_p, C.c_int,
                                          c_int32_p, c_double_p, c_uint8_p]
        f("line_track_match").restype = C.c_int
        f("line_hough_cells").argtypes = [c_float_p, C.c_int, C.c_double, C.c_double, c_int32_p]
        f("line_hough_cells").restype = C.c_int
        f("line_match_last_frame").argtypes = [vp, C.POINTER(LineLastKfParams), C.c_int, c_float_p, C.c_int, c_float_p, c_int32_p, c_uint8_p, c_float_p,
                                               C.c_int, c_float_p, c_int32_p, C.c_int, c_float_p, c_int32_p, c_uint8_p, c_float_p, C.c_int,
                                               c_int32_p, c_uint8_p, c_double_p, c_double_p]
        f("line_match_last_frame").restype = C.c_int
        if self.prefix == "lld_":
            f("status_string").argtypes = [C.c_int]; f("status_string").restype = C.c_char_p
            f("ctx_create").argtypes = [C.c_int, C.POINTER(vp)]; f("ctx_create").restype = C.c_int
            f("ctx_destroy").argtypes = [vp]; f("ctx_destroy").restype = None
            f("ctx_stream").argtypes = [vp]; f("ctx_stream").restype = vp
            f("ctx_synchronize").argtypes = [vp]; f("ctx_synchronize").restype = C.c_int
            f("ctx_release_cache").argtypes = [vp]; f("ctx_release_cache").restype = C.c_int
            f("ba_batch_create").argtypes = [vp, C.c_int, C.POINTER(BAWindow), C.POINTER(BAParams), C.POINTER(vp)]
            f("ba_batch_create").restype = C.c_int
            f("ba_batch_solve").argtypes = [vp, C.POINTER(C.c_int)]; f("ba_batch_solve").restype = C.c_int
            f("ba_batch_download").argtypes = [vp, C.c_int, C.POINTER(BAResult)]; f("ba_batch_download").restype = C.c_int
            f("ba_batch_download_range").argtypes = [vp, C.c_int, C.c_int, C.POINTER(BAResult)]; f("ba_batch_download_range").restype = C.c_int
            f("ba_batch_stats").argtypes = [vp, C.POINTER(BAStats)]; f("ba_batch_stats").restype = C.c_int
            f("ba_batch_result_records").argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
            f("ba_batch_result_records").restype = C.c_int
            f("ba_batch_phase_ms").argtypes = [vp, c_double_p]; f("ba_batch_phase_ms").restype = C.c_int
            f("ba_batch_set_phase_timing").argtypes = [vp, C.c_int]; f("ba_batch_set_phase_timing").restype = C.c_int
            f("ba_batch_kernel_stats").argtypes = [vp, C.c_int, C.POINTER(C.c_int64), c_double_p]
            f("ba_batch_kernel_stats").restype = C.c_int
            f("ba_batch_set_groups").argtypes = [vp, C.c_int]; f("ba_batch_set_groups").restype = C.c_int
            f("ba_batch_destroy").argtypes = [vp]; f("ba_batch_destroy").restype = None
            f("pose_batch_create").argtypes = [vp, C.c_int, C.POINTER(PoseProblem), C.POINTER(PoseParams), C.POINTER(vp)]
            f("pose_batch_create").restype = C.c_int
            f("pose_batch_solve").argtypes = [vp]; f("pose_batch_solve").restype = C.c_int
            f("pose_batch_download").argtypes = [vp, C.c_int, C.POINTER(PoseResult)]; f("pose_batch_download").restype = C.c_int
            f("pose_batch_destroy").argtypes = [vp]; f("pose_batch_destroy").restype = None
            f("match_hamming256_batch_dev").argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
            f("match_hamming256_batch_dev").restype = C.c_int
            f("match_l2f32_batch_dev").argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]
            f("match_l2f32_batch_dev").restype = C.c_int
            f("pnp_params_default").argtypes = [C.POINTER(PnPParams)]; f("pnp_params_default").restype = None
            f("pnp_batch_create").argtypes = [vp, C.c_int32, C.POINTER(PnPProblem), C.POINTER(PnPParams), C.POINTER(vp)]
            f("pnp_batch_create").restype = C.c_int
            f("pnp_batch_iterate").argtypes = [vp, C.c_int32, c_uint8_p]; f("pnp_batch_iterate").restype = C.c_int
            f("pnp_batch_find").argtypes = [vp, c_uint8_p]; f("pnp_batch_find").restype = C.c_int
            f("pnp_batch_download").argtypes = [vp, C.POINTER(PnPResult)]; f("pnp_batch_download").restype = C.c_int
            f("pnp_batch_hypotheses").argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(PnPHypothesis), c_int32_p, c_int32_p]
            f("pnp_batch_hypotheses").restype = C.c_int
            f("pnp_batch_destroy").argtypes = [vp]; f("pnp_batch_destroy").restype = None
            f("pnp_find").argtypes = [vp, C.POINTER(PnPProblem), C.POINTER(PnPParams), C.POINTER(PnPResult)]
            f("pnp_find").restype = C.c_int
            f("sim3solver_params_default").argtypes = [C.POINTER(Sim3SolverParams)]; f("sim3solver_params_default").restype = None
            f("sim3solver_batch_create").argtypes = [vp, C.c_int32, C.POINTER(Sim3SolverProblem), C.POINTER(Sim3SolverParams), C.POINTER(vp)]
            f("sim3solver_batch_create").restype = C.c_int
            f("sim3solver_batch_iterate").argtypes = [vp, C.c_int32, c_uint8_p]; f("sim3solver_batch_iterate").restype = C.c_int
            f("sim3solver_batch_find").argtypes = [vp, c_uint8_p]; f("sim3solver_batch_find").restype = C.c_int
            f("sim3solver_batch_download").argtypes = [vp, C.POINTER(Sim3SolverResult)]; f("sim3solver_batch_download").restype = C.c_int
            f("sim3solver_batch_hypotheses").argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(Sim3SolverHypothesis), c_int32_p, c_int32_p]
            f("sim3solver_batch_hypotheses").restype = C.c_int
            f("sim3solver_batch_destroy").argtypes = [vp]; f("sim3solver_batch_destroy").restype = None
            f("sim3solver_find").argtypes = [vp, C.POINTER(Sim3SolverProblem), C.POINTER(Sim3SolverParams), C.POINTER(Sim3SolverResult)]
            f("sim3solver_find").restype = C.c_int
            f("initializer_params_default").argtypes = [C.POINTER(InitializerParams)]; f("initializer_params_default").restype = None
            f("initializer_create").argtypes = [vp, c_float_p, C.c_int32, c_float_p, C.POINTER(InitializerParams), C.POINTER(vp)]
            f("initializer_create").restype = C.c_int
            f("initializer_initialize").argtypes = [vp, C.c_int32, c_float_p, C.c_int32, c_int32_p, C.POINTER(InitializerResult)]
            f("initializer_initialize").restype = C.c_int
            f("initializer_hypotheses").argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(InitializerHypothesis), c_int32_p]
            f("initializer_hypotheses").restype = C.c_int
            f("initializer_destroy").argtypes = [vp]; f("initializer_destroy").restype = None
            f("initializer_find").argtypes = [vp, c_float_p, C.c_int32, c_float_p, C.c_int32, c_float_p, C.c_int32, c_int32_p,
                                              C.POINTER(InitializerParams), C.POINTER(InitializerResult)]
            f("initializer_find").restype = C.c_int
            f("mappoint_refresh").argtypes = [vp, C.POINTER(MapPointRefreshIn), C.POINTER(MapPointRefreshOut)]
            f("mappoint_refresh").restype = C.c_int
            f("mapline_distinctive").argtypes = [vp, C.POINTER(MapLineDistinctiveIn), C.POINTER(MapLineDistinctiveOut)]
            f("mapline_distinctive").restype = C.c_int
            f("new_points_triangulate").argtypes = [vp, C.POINTER(NewPointsIn), C.POINTER(NewPointsOut)]
            f("new_points_triangulate").restype = C.c_int
            f("covisibility_params_default").argtypes = [C.POINTER(CovisibilityParams)]
            f("covisibility_params_default").restype = None
            f("covisibility").argtypes = [vp, C.POINTER(CovisibilityIn), C.POINTER(CovisibilityOut)]
            f("covisibility").restype = C.c_int
            f("loop_correct").argtypes = [vp, C.POINTER(LoopCorrectIn), C.POINTER(LoopCorrectOut)]; f("loop_correct").restype = C.c_int
            f("essential_graph_apply").argtypes = [vp, C.POINTER(EssentialGraphApplyIn), C.POINTER(EssentialGraphApplyOut)]
            f("essential_graph_apply").restype = C.c_int
            f("global_ba_apply").argtypes = [vp, C.POINTER(GlobalBAApplyIn), C.POINTER(GlobalBAApplyOut)]
            f("global_ba_apply").restype = C.c_int
            # (frame, vocabulary, levelsup, lld_bow_result* or NULL); (frame, lld_track_params*, lld_frame_view*, pose_qt, lld_ref_keyframe*):
            # the structs of vocabulary.py / tracking.py / orb_search.py pass by reference
            f("frame_compute_bow").argtypes = [vp, vp, C.c_int, vp]; f("frame_compute_bow").restype = C.c_int
            f("frame_build_lines").argtypes = [vp, C.POINTER(FrameLinesBuild)]; f("frame_build_lines").restype = C.c_int
            f("frame_lines_download").argtypes = [vp, c_int32_p, c_double_p]; f("frame_lines_download").restype = C.c_int
            f("frame_new_map_lines").argtypes = [vp, vp, C.POINTER(FrameNewLinesParams), C.POINTER(FrameNewLinesResult)]
            f("frame_new_map_lines").restype = C.c_int
            f("frame_track_finish").argtypes = [vp, C.POINTER(FrameFinishParams), C.POINTER(FrameFinishResult)]; f("frame_track_finish").restype = C.c_int
            f("frame_create_stereo_points").argtypes = [vp, C.POINTER(FramePointsParams), C.POINTER(FrameFinishResult)]
            f("frame_create_stereo_points").restype = C.c_int
            f("frame_track_reference_keyframe").argtypes = [vp, vp, vp, c_double_p, C.POINTER(RefKeyFrame)]
            f("frame_track_reference_keyframe").restype = C.c_int
            # (frame, lld_track_params*, lld_frame_view*, pose_qt, n_candidates, lld_ref_keyframe[], lld_reloc_candidate[], lld_pnp_params*, lld_reloc_result*)
            f("frame_relocalize").argtypes = [vp, vp, vp, c_double_p, C.c_int32, C.POINTER(RefKeyFrame), C.POINTER(RelocCandidate), C.POINTER(PnPParams),
                                              C.POINTER(RelocResult)]
            f("frame_relocalize").restype = C.c_int


_PRODUCT = None


def product() -> Lib:
    """The HIP library.  Raises if it has not been built — the product path never falls back to CPU."""
    global _PRODUCT
    if _PRODUCT is None:
        # PyTorch wheels bundle their own libamdhip64.so (soname libamdhip64.so.7).  Two HIP runtimes in one process
        # cannot both own the GPU, so when torch is importable it is loaded first: liblld_amd.so's DT_NEEDED
        # libamdhip64.so.7 then resolves to the runtime torch already mapped.  C/C++ hosts simply link /opt/rocm's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _PRODUCT = Lib(product_library_path(), "lld_")
    return _PRODUCT
