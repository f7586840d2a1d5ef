"""The three places where the loop-closing thread moves the map, each as one device call: LoopClosing::CorrectLoop's correction
(lld_loop_correct), the write-back of Optimizer::OptimizeEssentialGraph (lld_essential_graph_apply) and the map update after a global
bundle adjustment (lld_global_ba_apply).  The rules, the conventions and the limits are those of include/lld_amd.h: keyframe tables in
pointer order, observations in CSR form in std::map order, a Sim3 as 8 doubles, a float pose as the 12 floats of [R|t]."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import (EssentialGraphApplyIn, EssentialGraphApplyOut, GlobalBAApplyIn, GlobalBAApplyOut, LoopCorrectIn, LoopCorrectOut,
                  c_double_p, c_float_p, c_int32_p, c_uint8_p)

MAX_KF = 65536               # LLD_MAPCORR_MAX_KF
MAX_POINTS = 1 << 23         # LLD_MAPCORR_MAX_POINTS
MAX_ENTRIES = 1 << 24        # LLD_MAPCORR_MAX_ENTRIES
MOVED = 1                    # LLD_MAPCORR_MOVED; bit 1 of `updated` is landmarks.NORMAL_DEPTH
NORMAL_DEPTH = 2


class LoopCorrectionError(RuntimeError):
    def __init__(self, what, status):
        super().__init__(f"{what} failed with status {status}")
        self.status = status


@dataclass
class LoopCorrection:
    """Per connected keyframe (in conn order): corrected_sim3 / non_corrected_sim3 (n_conn x 8), tiw_corrected (n_conn x 12),
    ow_corrected (n_conn x 3), scw_f32 (n_conn x 12).  Per point: pos, corrected_by (rank in conn, or -1), normal, min_distance,
    max_distance, updated (bit 0 moved, bit 1 normal / depth)."""
    corrected_sim3: np.ndarray
    non_corrected_sim3: np.ndarray
    tiw_corrected: np.ndarray
    ow_corrected: np.ndarray
    scw_f32: np.ndarray
    pos: np.ndarray
    corrected_by: np.ndarray
    normal: np.ndarray
    min_distance: np.ndarray
    max_distance: np.ndarray
    updated: np.ndarray


@dataclass
class EssentialGraphApplied:
    tiw: np.ndarray
    ow: np.ndarray
    pos: np.ndarray
    normal: np.ndarray
    min_distance: np.ndarray
    max_distance: np.ndarray
    updated: np.ndarray


@dataclass
class GlobalBAApplied:
    """visited (n_kf); tcw_new / tcw_before (n_kf x 12) and ow_new (n_kf x 3) of the visited keyframes; pos and moved (0 untouched,
    1 from pos_gba, 2 through the reference keyframe)."""
    visited: np.ndarray
    tcw_new: np.ndarray
    tcw_before: np.ndarray
    ow_new: np.ndarray
    pos: np.ndarray
    moved: np.ndarray


def _arr(a, dtype, shape=None):
    a = np.ascontiguousarray(a, dtype)
    return a if shape is None else a.reshape(shape)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _inout(a, dtype, shape):
    """A private copy of the caller's current values (entries the rule leaves alone keep them), zeros when none were given."""
    return np.zeros(shape, dtype) if a is None else np.array(a, dtype).reshape(shape)


def _run(ctx, fn, a, o, r, keep):
    st = ctx.lib.fn(fn)(ctx.handle, C.byref(a), C.byref(o))
    del keep                                 # the inputs had to live until here
    if st != abi.LLD_OK:
        raise LoopCorrectionError("lld_" + fn, st)
    return r


def _points(P, keep, pos, bad, obs_start, obs_kf, ref_kf, ref_level, level_scale):
    """Fills an lld_mapcorr_points; `keep` holds the arrays alive for the call."""
    keep += [_arr(pos, np.float32, (-1, 3)), _arr(bad, np.uint8), _arr(obs_start, np.int32), _arr(obs_kf, np.int32), _arr(ref_kf, np.int32),
             _arr(ref_level, np.int32), _arr(level_scale, np.float32)]
    pos, bad, obs_start, obs_kf, ref_kf, ref_level, level_scale = keep[-7:]
    P.n_points, P.n_obs, P.n_levels = len(bad), len(obs_kf), len(level_scale)
    P.pos = _ptr(pos, c_float_p); P.bad = _ptr(bad, c_uint8_p); P.obs_start = _ptr(obs_start, c_int32_p); P.obs_kf = _ptr(obs_kf, c_int32_p)
    P.ref_kf = _ptr(ref_kf, c_int32_p); P.ref_level = _ptr(ref_level, c_int32_p); P.level_scale = _ptr(level_scale, c_float_p)
    return len(bad), pos


def correct_loop(ctx, kf_tcw, conn, cur, scw, kf_start, kf_point, pos, bad, already, obs_start, obs_kf, ref_kf, ref_level, level_scale,
                 normal=None, min_distance=None, max_distance=None):
    """One lld_loop_correct call: LoopClosing::CorrectLoop, src/LoopClosing.cc:440-518.  normal / min_distance / max_distance: the
    points' current values, returned unchanged where the rule leaves them alone.  (ctx = None, here and below: nothing is called and
    the prepared (in struct, out struct, result, arrays kept alive) are returned - the refusal tests edit them.)"""
    keep = [_arr(kf_tcw, np.float32, (-1, 12)), _arr(conn, np.int32), _arr(scw, np.float64, (8,)), _arr(kf_start, np.int32),
            _arr(kf_point, np.int32), _arr(already, np.uint8)]
    kf_tcw, conn, scw, kf_start, kf_point, already = keep
    a = LoopCorrectIn()
    a.n_kf, a.n_conn, a.cur, a.n_entries = len(kf_tcw), len(conn), int(cur), len(kf_point)
    a.kf_tcw = _ptr(kf_tcw, c_float_p); a.conn = _ptr(conn, c_int32_p); a.scw = _ptr(scw, c_double_p)
    a.kf_start = _ptr(kf_start, c_int32_p); a.kf_point = _ptr(kf_point, c_int32_p); a.already = _ptr(already, c_uint8_p)
    n, pos = _points(a.points, keep, pos, bad, obs_start, obs_kf, ref_kf, ref_level, level_scale)
    nc = len(conn)
    r = LoopCorrection(np.zeros((nc, 8)), np.zeros((nc, 8)), np.zeros((nc, 12), np.float32), np.zeros((nc, 3), np.float32),
                       np.zeros((nc, 12), np.float32), np.array(pos, np.float32).reshape(n, 3), np.full(n, -1, np.int32),
                       _inout(normal, np.float32, (n, 3)), _inout(min_distance, np.float32, (n,)), _inout(max_distance, np.float32, (n,)),
                       np.zeros(n, np.uint8))
    o = LoopCorrectOut()
    o.corrected_sim3 = _ptr(r.corrected_sim3, c_double_p); o.non_corrected_sim3 = _ptr(r.non_corrected_sim3, c_double_p)
    o.tiw_corrected = _ptr(r.tiw_corrected, c_float_p); o.ow_corrected = _ptr(r.ow_corrected, c_float_p); o.scw_f32 = _ptr(r.scw_f32, c_float_p)
    o.pos = _ptr(r.pos, c_float_p); o.corrected_by = _ptr(r.corrected_by, c_int32_p); o.normal = _ptr(r.normal, c_float_p)
    o.min_distance = _ptr(r.min_distance, c_float_p); o.max_distance = _ptr(r.max_distance, c_float_p); o.updated = _ptr(r.updated, c_uint8_p)
    return _run(ctx, "loop_correct", a, o, r, keep) if ctx is not None else (a, o, r, keep)


def apply_essential_graph(ctx, sim3_before, sim3_after, corr_kf, pos, bad, obs_start, obs_kf, ref_kf, ref_level, level_scale, normal=None,
                          min_distance=None, max_distance=None):
    """One lld_essential_graph_apply call: Optimizer.cc:1601-1653.  sim3_before / sim3_after are the sim3 arrays
    Optimizer.OptimizeEssentialGraph takes and returns."""
    keep = [_arr(sim3_before, np.float64, (-1, 8)), _arr(sim3_after, np.float64, (-1, 8)), _arr(corr_kf, np.int32)]
    before, after, corr_kf = keep
    if len(after) != len(before):
        raise ValueError("sim3_before and sim3_after differ in length")
    a = EssentialGraphApplyIn()
    a.n_kf = len(before)
    a.sim3_before = _ptr(before, c_double_p); a.sim3_after = _ptr(after, c_double_p); a.corr_kf = _ptr(corr_kf, c_int32_p)
    n, pos = _points(a.points, keep, pos, bad, obs_start, obs_kf, ref_kf, ref_level, level_scale)
    nk = len(before)
    r = EssentialGraphApplied(np.zeros((nk, 12), np.float32), np.zeros((nk, 3), np.float32), np.array(pos, np.float32).reshape(n, 3),
                              _inout(normal, np.float32, (n, 3)), _inout(min_distance, np.float32, (n,)),
                              _inout(max_distance, np.float32, (n,)), np.zeros(n, np.uint8))
    o = EssentialGraphApplyOut()
    o.tiw = _ptr(r.tiw, c_float_p); o.ow = _ptr(r.ow, c_float_p); o.pos = _ptr(r.pos, c_float_p); o.normal = _ptr(r.normal, c_float_p)
    o.min_distance = _ptr(r.min_distance, c_float_p); o.max_distance = _ptr(r.max_distance, c_float_p); o.updated = _ptr(r.updated, c_uint8_p)
    return _run(ctx, "essential_graph_apply", a, o, r, keep) if ctx is not None else (a, o, r, keep)


def apply_global_ba(ctx, kf_tcw, kf_in_gba, kf_tcw_gba, parent, origins, pos, bad, in_gba, pos_gba, ref_kf):
    """One lld_global_ba_apply call: LoopClosing.cc:678-739."""
    keep = [_arr(kf_tcw, np.float32, (-1, 12)), _arr(kf_in_gba, np.uint8), _arr(kf_tcw_gba, np.float32, (-1, 12)), _arr(parent, np.int32),
            _arr(origins, np.int32), _arr(pos, np.float32, (-1, 3)), _arr(bad, np.uint8), _arr(in_gba, np.uint8),
            _arr(pos_gba, np.float32, (-1, 3)), _arr(ref_kf, np.int32)]
    kf_tcw, kf_in_gba, kf_tcw_gba, parent, origins, pos, bad, in_gba, pos_gba, ref_kf = keep
    nk, n = len(kf_tcw), len(bad)
    a = GlobalBAApplyIn()
    a.n_kf, a.n_origins, a.n_points = nk, len(origins), n
    a.kf_tcw = _ptr(kf_tcw, c_float_p); a.kf_in_gba = _ptr(kf_in_gba, c_uint8_p); a.kf_tcw_gba = _ptr(kf_tcw_gba, c_float_p)
    a.parent = _ptr(parent, c_int32_p); a.origins = _ptr(origins, c_int32_p); a.pos = _ptr(pos, c_float_p); a.bad = _ptr(bad, c_uint8_p)
    a.in_gba = _ptr(in_gba, c_uint8_p); a.pos_gba = _ptr(pos_gba, c_float_p); a.ref_kf = _ptr(ref_kf, c_int32_p)
    r = GlobalBAApplied(np.zeros(nk, np.uint8), np.array(kf_tcw, np.float32), np.array(kf_tcw, np.float32), np.zeros((nk, 3), np.float32),
                        np.array(pos, np.float32).reshape(n, 3), np.zeros(n, np.uint8))
    o = GlobalBAApplyOut()
    o.visited = _ptr(r.visited, c_uint8_p); o.tcw_new = _ptr(r.tcw_new, c_float_p); o.tcw_before = _ptr(r.tcw_before, c_float_p)
    o.ow_new = _ptr(r.ow_new, c_float_p); o.pos = _ptr(r.pos, c_float_p); o.moved = _ptr(r.moved, c_uint8_p)
    return _run(ctx, "global_ba_apply", a, o, r, keep) if ctx is not None else (a, o, r, keep)
