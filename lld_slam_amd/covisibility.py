"""KeyFrame::UpdateConnections, the vote of Tracking::UpdateLocalKeyFrames and the redundancy count of
LocalMapping::KeyFrameCulling for a batch of keyframes on the device (lld_covisibility).  The rules are those of
include/lld_amd.h.  Keyframes are slots numbered in the order in which the reference's std::map<KeyFrame*, ...> iterates; the
observations are in the CSR layout of lld_mappoint_refresh."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import CovisibilityIn, CovisibilityOut, c_float_p, c_int32_p, c_uint8_p

MAX_KF = 16384               # LLD_COVIS_MAX_KF
CONNECTIONS = 1              # LLD_COVIS_CONNECTIONS
CULLING = 2                  # LLD_COVIS_CULLING


class CovisibilityError(RuntimeError):
    """status is the library's; n_conn / n_ordered are the totals a call with a short capacity reports (None otherwise)."""

    def __init__(self, what, status, n_conn=None, n_ordered=None):
        super().__init__(f"{what} failed with status {status}")
        self.status = status
        self.n_conn = n_conn
        self.n_ordered = n_ordered


@dataclass
class Connections:
    """conn_start / ordered_start (n_queries+1); conn_kf, conn_weight: mConnectedKeyFrameWeights in map order; ordered_kf,
    ordered_weight: mvpOrderedConnectedKeyFrames / mvOrderedWeights; n_max, kf_max; updated (0: the reference returns early)."""
    conn_start: np.ndarray
    conn_kf: np.ndarray
    conn_weight: np.ndarray
    ordered_start: np.ndarray
    ordered_kf: np.ndarray
    ordered_weight: np.ndarray
    n_max: np.ndarray
    kf_max: np.ndarray
    updated: np.ndarray


@dataclass
class Culling:
    n_mps: np.ndarray
    n_redundant: np.ndarray
    redundant: np.ndarray


def _arr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def default_params(ctx):
    p = abi.CovisibilityParams()
    ctx.lib.fn("covisibility_params_default")(C.byref(p))
    return p


def capacity_bound(n_kf, obs_start, q_start, q_point):
    """Entries that always suffice for either list: the sum over the queries of min(n_kf, observations of the query's entries)."""
    obs_start = np.asarray(obs_start, np.int64); q_start = np.asarray(q_start, np.int64); q_point = np.asarray(q_point, np.int64)
    per_entry = obs_start[q_point + 1] - obs_start[q_point] if len(q_point) else np.zeros(0, np.int64)
    cs = np.concatenate([[0], np.cumsum(per_entry)])
    return int(np.minimum(cs[q_start[1:]] - cs[q_start[:-1]], n_kf).sum())


def covisibility(ctx, n_kf, obs_start, obs_kf, point_bad, query_kf, q_start, q_point, flags, obs_octave=None, point_nobs=None,
                 q_octave=None, q_depth=None, q_th_depth=None, monocular=False, th=None, th_obs=None, redundant_ratio=None,
                 conn_capacity=None, ordered_capacity=None, phase_ms=None):
    """One lld_covisibility call.  Returns (Connections or None, Culling or None) by `flags`.  conn_capacity / ordered_capacity
    default to capacity_bound(); a short one raises CovisibilityError carrying the totals.  phase_ms: a float32 array of 3 that
    receives the upload, kernel and download times."""
    obs_start = _arr(obs_start, np.int32); obs_kf = _arr(obs_kf, np.int32); point_bad = _arr(point_bad, np.uint8)
    query_kf = _arr(query_kf, np.int32); q_start = _arr(q_start, np.int32); q_point = _arr(q_point, np.int32)
    obs_octave = _arr(obs_octave, np.int32); point_nobs = _arr(point_nobs, np.int32); q_octave = _arr(q_octave, np.int32)
    q_depth = _arr(q_depth, np.float32); q_th_depth = _arr(q_th_depth, np.float32)
    nq = len(query_kf)
    a = CovisibilityIn()
    a.n_kf, a.n_points, a.n_obs, a.n_queries, a.n_entries = int(n_kf), len(point_bad), len(obs_kf), nq, len(q_point)
    a.monocular = 1 if monocular else 0
    a.flags = int(flags)
    a.params = default_params(ctx)
    if th is not None:
        a.params.th = int(th)
    if th_obs is not None:
        a.params.th_obs = int(th_obs)
    if redundant_ratio is not None:
        a.params.redundant_ratio = float(redundant_ratio)
    a.obs_start = _ptr(obs_start, c_int32_p); a.obs_kf = _ptr(obs_kf, c_int32_p); a.obs_octave = _ptr(obs_octave, c_int32_p)
    a.point_bad = _ptr(point_bad, c_uint8_p); a.point_nobs = _ptr(point_nobs, c_int32_p); a.query_kf = _ptr(query_kf, c_int32_p)
    a.q_start = _ptr(q_start, c_int32_p); a.q_point = _ptr(q_point, c_int32_p); a.q_octave = _ptr(q_octave, c_int32_p)
    a.q_depth = _ptr(q_depth, c_float_p); a.q_th_depth = _ptr(q_th_depth, c_float_p)
    o = CovisibilityOut()
    conn = cull = None
    if flags & CONNECTIONS:
        if conn_capacity is None or ordered_capacity is None:
            try:
                bound = capacity_bound(n_kf, obs_start, q_start, q_point)
            except (IndexError, ValueError):
                bound = 0                       # malformed lists: the library refuses them
            conn_capacity = bound if conn_capacity is None else conn_capacity
            ordered_capacity = bound if ordered_capacity is None else ordered_capacity
        conn = Connections(np.zeros(nq + 1, np.int32), np.zeros(max(conn_capacity, 1), np.int32), np.zeros(max(conn_capacity, 1), np.int32),
                           np.zeros(nq + 1, np.int32), np.zeros(max(ordered_capacity, 1), np.int32),
                           np.zeros(max(ordered_capacity, 1), np.int32), np.zeros(nq, np.int32), np.zeros(nq, np.int32),
                           np.zeros(nq, np.uint8))
        o.conn_capacity, o.ordered_capacity = int(conn_capacity), int(ordered_capacity)
        o.conn_start = _ptr(conn.conn_start, c_int32_p); o.conn_kf = _ptr(conn.conn_kf, c_int32_p)
        o.conn_weight = _ptr(conn.conn_weight, c_int32_p); o.ordered_start = _ptr(conn.ordered_start, c_int32_p)
        o.ordered_kf = _ptr(conn.ordered_kf, c_int32_p); o.ordered_weight = _ptr(conn.ordered_weight, c_int32_p)
        o.n_max = _ptr(conn.n_max, c_int32_p); o.kf_max = _ptr(conn.kf_max, c_int32_p); o.updated = _ptr(conn.updated, c_uint8_p)
    if flags & CULLING:
        cull = Culling(np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.zeros(nq, np.uint8))
        o.n_mps = _ptr(cull.n_mps, c_int32_p); o.n_redundant = _ptr(cull.n_redundant, c_int32_p)
        o.redundant = _ptr(cull.redundant, c_uint8_p)
    if phase_ms is not None:
        assert phase_ms.dtype == np.float32 and phase_ms.size >= 3 and phase_ms.flags.c_contiguous
        o.phase_ms = _ptr(phase_ms, c_float_p)
    o.n_conn = o.n_ordered = -1
    st = ctx.lib.fn("covisibility")(ctx.handle, C.byref(a), C.byref(o))
    if st != abi.LLD_OK:
        short = st == abi.LLD_ERR_INVALID and o.n_conn >= 0
        raise CovisibilityError("lld_covisibility", st, o.n_conn if short else None, o.n_ordered if short else None)
    if conn is not None and nq:
        conn.conn_kf = conn.conn_kf[:o.n_conn]; conn.conn_weight = conn.conn_weight[:o.n_conn]
        conn.ordered_kf = conn.ordered_kf[:o.n_ordered]; conn.ordered_weight = conn.ordered_weight[:o.n_ordered]
    elif conn is not None:
        conn.conn_kf = conn.conn_kf[:0]; conn.conn_weight = conn.conn_weight[:0]
        conn.ordered_kf = conn.ordered_kf[:0]; conn.ordered_weight = conn.ordered_weight[:0]
    return conn, cull


def update_connections(ctx, n_kf, obs_start, obs_kf, point_bad, query_kf, q_start, q_point, th=None, conn_capacity=None,
                       ordered_capacity=None):
    """KeyFrame::UpdateConnections for every query (query_kf = -1: the vote of Tracking::UpdateLocalKeyFrames)."""
    return covisibility(ctx, n_kf, obs_start, obs_kf, point_bad, query_kf, q_start, q_point, CONNECTIONS, th=th,
                        conn_capacity=conn_capacity, ordered_capacity=ordered_capacity)[0]


def keyframe_culling(ctx, n_kf, obs_start, obs_kf, obs_octave, point_bad, point_nobs, query_kf, q_start, q_point, q_octave, q_depth,
                     q_th_depth, monocular=False, th_obs=None, redundant_ratio=None):
    """The redundancy count of LocalMapping::KeyFrameCulling for every query."""
    return covisibility(ctx, n_kf, obs_start, obs_kf, point_bad, query_kf, q_start, q_point, CULLING, obs_octave=obs_octave,
                        point_nobs=point_nobs, q_octave=q_octave, q_depth=q_depth, q_th_depth=q_th_depth, monocular=monocular,
                        th_obs=th_obs, redundant_ratio=redundant_ratio)[1]
