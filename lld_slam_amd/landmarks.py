"""MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth and MapLine::ComputeDistinctiveDescriptors for a batch of
landmarks on the device (lld_mappoint_refresh, lld_mapline_distinctive).  The rules and the deviations are those of
include/lld_amd.h.  Observations are in CSR form and listed in the order in which the reference's std::map iterates."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import (MapLineDistinctiveIn, MapLineDistinctiveOut, MapPointRefreshIn, MapPointRefreshOut, c_float_p, c_int32_p,
                  c_uint8_p, c_uint32_p)

MAX_OBS = 1024               # LLD_LANDMARK_MAX_OBS
MAX_LINE_OBS = 64            # LLD_LANDMARK_MAX_LINE_OBS
MAX_LINE_DIM = 128           # LLD_LANDMARK_MAX_LINE_DIM
DESCRIPTOR = 1               # LLD_LANDMARK_DESCRIPTOR
NORMAL_DEPTH = 2             # LLD_LANDMARK_NORMAL_DEPTH


class LandmarkError(RuntimeError):
    def __init__(self, what, status):
        super().__init__(f"{what} failed with status {status}")
        self.status = status


@dataclass
class MapPointRefresh:
    """desc (n x 8 uint32), best_obs / best_median (n, -1 where nothing was written), normal (n x 3), min_distance /
    max_distance (n), updated (n: bit 0 descriptor, bit 1 normal / depth).  The arrays of a part that was not selected are None
    unless the caller passed them in."""
    desc: np.ndarray | None
    best_obs: np.ndarray | None
    best_median: np.ndarray | None
    normal: np.ndarray | None
    min_distance: np.ndarray | None
    max_distance: np.ndarray | None
    updated: np.ndarray


@dataclass
class MapLineDistinctive:
    desc: np.ndarray
    best_obs: np.ndarray
    best_median: np.ndarray
    updated: np.ndarray


def _arr(a, dtype, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype)
    return a if shape is None else a.reshape(shape)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _inout(a, dtype, shape):
    """A private copy of the caller's current values (entries the rule leaves alone keep them), zeros when none were given."""
    return np.zeros(shape, dtype) if a is None else np.array(a, dtype).reshape(shape)


def refresh_map_points(ctx, obs_start, obs_kf, bad, obs_desc=None, kf_bad=None, kf_ow=None, pos=None, ref_kf=None, ref_level=None,
                       level_scale=None, flags=DESCRIPTOR | NORMAL_DEPTH, desc=None, normal=None, min_distance=None,
                       max_distance=None):
    """One lld_mappoint_refresh call.  obs_start (n+1), obs_kf (n_obs), bad (n) always; obs_desc (n_obs x 8 uint32) and kf_bad
    (n_kf) for the descriptor part; kf_ow (n_kf x 3), pos (n x 3), ref_kf, ref_level (n) and level_scale for the normal / depth
    part.  desc / normal / min_distance / max_distance: the landmarks' current values, returned unchanged where the reference
    would return early."""
    obs_start = _arr(obs_start, np.int32); obs_kf = _arr(obs_kf, np.int32); bad = _arr(bad, np.uint8)
    n = len(bad)
    obs_desc = _arr(obs_desc, np.uint32, (-1, 8)); kf_bad = _arr(kf_bad, np.uint8); kf_ow = _arr(kf_ow, np.float32, (-1, 3))
    pos = _arr(pos, np.float32, (-1, 3)); ref_kf = _arr(ref_kf, np.int32); ref_level = _arr(ref_level, np.int32)
    level_scale = _arr(level_scale, np.float32)
    n_kf = len(kf_bad) if kf_bad is not None else (len(kf_ow) if kf_ow is not None else 0)
    a = MapPointRefreshIn()
    a.n_points, a.n_obs, a.n_kf = n, len(obs_kf), n_kf
    a.n_levels = 0 if level_scale is None else len(level_scale)
    a.flags = int(flags)
    a.obs_start = _ptr(obs_start, c_int32_p); a.obs_kf = _ptr(obs_kf, c_int32_p); a.obs_desc = _ptr(obs_desc, c_uint32_p)
    a.kf_ow = _ptr(kf_ow, c_float_p); a.kf_bad = _ptr(kf_bad, c_uint8_p); a.pos = _ptr(pos, c_float_p); a.bad = _ptr(bad, c_uint8_p)
    a.ref_kf = _ptr(ref_kf, c_int32_p); a.ref_level = _ptr(ref_level, c_int32_p); a.level_scale = _ptr(level_scale, c_float_p)
    want_d, want_n = bool(flags & DESCRIPTOR), bool(flags & NORMAL_DEPTH)
    r = MapPointRefresh(None, None, None, None, None, None, np.zeros(n, np.uint8))
    if want_d or desc is not None:
        r.desc = _inout(desc, np.uint32, (n, 8))
    if want_d:
        r.best_obs = np.full(n, -1, np.int32); r.best_median = np.full(n, -1, np.int32)
    if want_n or normal is not None:
        r.normal = _inout(normal, np.float32, (n, 3))
    if want_n or min_distance is not None:
        r.min_distance = _inout(min_distance, np.float32, (n,))
    if want_n or max_distance is not None:
        r.max_distance = _inout(max_distance, np.float32, (n,))
    o = MapPointRefreshOut()
    o.desc = _ptr(r.desc, c_uint32_p); o.best_obs = _ptr(r.best_obs, c_int32_p); o.best_median = _ptr(r.best_median, c_int32_p)
    o.normal = _ptr(r.normal, c_float_p); o.min_distance = _ptr(r.min_distance, c_float_p)
    o.max_distance = _ptr(r.max_distance, c_float_p); o.updated = _ptr(r.updated, c_uint8_p)
    st = ctx.lib.fn("mappoint_refresh")(ctx.handle, C.byref(a), C.byref(o))
    if st != abi.LLD_OK:
        raise LandmarkError("lld_mappoint_refresh", st)
    return r


def distinctive_line_descriptors(ctx, obs_start, obs_kf, obs_desc, kf_bad, bad, desc=None, dim=None):
    """One lld_mapline_distinctive call.  obs_desc: n_obs x dim float32 (dim is needed only when there is no observation)."""
    obs_start = _arr(obs_start, np.int32); obs_kf = _arr(obs_kf, np.int32); bad = _arr(bad, np.uint8); kf_bad = _arr(kf_bad, np.uint8)
    obs_desc = np.ascontiguousarray(obs_desc, np.float32)
    if dim is None:
        dim = obs_desc.shape[1]
    n = len(bad)
    a = MapLineDistinctiveIn()
    a.n_lines, a.n_obs, a.n_kf, a.dim = n, len(obs_kf), len(kf_bad), int(dim)
    a.obs_start = _ptr(obs_start, c_int32_p); a.obs_kf = _ptr(obs_kf, c_int32_p); a.obs_desc = _ptr(obs_desc, c_float_p)
    a.kf_bad = _ptr(kf_bad, c_uint8_p); a.bad = _ptr(bad, c_uint8_p)
    r = MapLineDistinctive(_inout(desc, np.float32, (n, max(int(dim), 1))), np.full(n, -1, np.int32), np.full(n, -1, np.int32),
                           np.zeros(n, np.uint8))
    o = MapLineDistinctiveOut()
    o.desc = _ptr(r.desc, c_float_p); o.best_obs = _ptr(r.best_obs, c_int32_p); o.best_median = _ptr(r.best_median, c_int32_p)
    o.updated = _ptr(r.updated, c_uint8_p)
    st = ctx.lib.fn("mapline_distinctive")(ctx.handle, C.byref(a), C.byref(o))
    if st != abi.LLD_OK:
        raise LandmarkError("lld_mapline_distinctive", st)
    return r
