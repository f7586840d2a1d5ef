"""The loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:287-451) on the device: one keyframe against several
neighbours in one lld_new_points_triangulate call.  The rules, their quirks and the deviation are those of include/lld_amd.h."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import NewPointsIn, NewPointsKf, NewPointsOut, c_float_p, c_int32_p, c_uint8_p

MAX_PAIRS = 64               # LLD_NEWPTS_MAX_PAIRS
MAX_MATCHES = 65536          # LLD_NEWPTS_MAX_MATCHES
MAX_LEVELS = 16              # LLD_ORB_MAX_LEVELS
(NEW, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, DIST_ZERO, SCALE, NO_DEPTH, PAIR_SKIPPED) = range(11)   # LLD_NEWPTS_*
SRC_TRIANGULATED, SRC_STEREO1, SRC_STEREO2 = range(3)                                                      # LLD_NEWPTS_SRC_*
OUTPUTS = ("status", "source", "x3d", "pair_status", "n_new", "new_match")


class NewPointsError(RuntimeError):
    def __init__(self, what, status):
        super().__init__(f"{what} failed with status {status}")
        self.status = status


@dataclass
class NewPoints:
    """status / source (n_matches uint8), x3d (n_matches x 3, zeros unless NEW), pair_status (n_pairs uint8), n_new (n_pairs),
    new_match (n_new_total global match indices in creation order), n_new_total.  An output that was not asked for is None."""
    status: np.ndarray | None
    source: np.ndarray | None
    x3d: np.ndarray | None
    pair_status: np.ndarray | None
    n_new: np.ndarray | None
    new_match: np.ndarray | None
    n_new_total: int


def keyframe_record(kf) -> NewPointsKf:
    """lld_new_points_kf from a mapping with Rcw (3x3), tcw, fx, fy, cx, cy, mb, scale_factors, level_sigma2 and, where they are
    read, mbf, scale_factor (keyframe 1) and median_depth (neighbours in monocular mode)."""
    r = NewPointsKf()
    r.Rcw[:] = [float(x) for x in np.asarray(kf["Rcw"], np.float32).reshape(9)]
    r.tcw[:] = [float(x) for x in np.asarray(kf["tcw"], np.float32).reshape(3)]
    for k in ("fx", "fy", "cx", "cy", "mb"):
        setattr(r, k, float(kf[k]))
    for k in ("mbf", "scale_factor", "median_depth"):
        setattr(r, k, float(kf.get(k, 0.0)))
    sf = np.asarray(kf["scale_factors"], np.float32); s2 = np.asarray(kf["level_sigma2"], np.float32)
    r.n_levels = int(kf.get("n_levels", len(sf)))
    for i in range(min(len(sf), MAX_LEVELS)):
        r.scale_factors[i] = float(sf[i]); r.level_sigma2[i] = float(s2[i])
    return r


def _keys(k, raw_key="raw_xy"):
    xy = np.ascontiguousarray(k["xy"], np.float32).reshape(-1, 2)
    raw = k.get(raw_key)
    raw = None if raw is None else np.ascontiguousarray(raw, np.float32).reshape(-1, 2)
    return (xy, raw, np.ascontiguousarray(k["ur"], np.float32), np.ascontiguousarray(k["depth"], np.float32),
            np.ascontiguousarray(k["octave"], np.int32))


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def pack_problem(kf1, keys1, kf2, key_start, keys2, match_start, matches, monocular=False):
    """(lld_new_points_in, number of matches) for the arguments of triangulate_new_points; the struct keeps its arrays alive."""
    recs = (NewPointsKf * max(len(kf2), 1))(*[keyframe_record(k) for k in kf2])
    xy1, raw1, ur1, d1, o1 = _keys(keys1)
    xy2, raw2, ur2, d2, o2 = _keys(keys2)
    key_start = np.ascontiguousarray(key_start, np.int32); match_start = np.ascontiguousarray(match_start, np.int32)
    matches = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
    a = NewPointsIn()
    a.kf1 = keyframe_record(kf1)
    a.monocular = int(monocular)
    a.n_keys1 = len(xy1)
    a.keys1_xy = _ptr(xy1, c_float_p); a.keys1_raw_xy = _ptr(raw1, c_float_p); a.ur1 = _ptr(ur1, c_float_p)
    a.depth1 = _ptr(d1, c_float_p); a.octave1 = _ptr(o1, c_int32_p)
    a.n_pairs = len(kf2)
    a.kf2 = recs
    a.key_start = _ptr(key_start, c_int32_p)
    a.keys2_xy = _ptr(xy2, c_float_p); a.keys2_raw_xy = _ptr(raw2, c_float_p); a.ur2 = _ptr(ur2, c_float_p)
    a.depth2 = _ptr(d2, c_float_p); a.octave2 = _ptr(o2, c_int32_p)
    a.match_start = _ptr(match_start, c_int32_p); a.matches = _ptr(matches, c_int32_p)
    a._keep = (recs, xy1, raw1, ur1, d1, o1, xy2, raw2, ur2, d2, o2, key_start, match_start, matches)
    return a, len(matches)


def triangulate_new_points(ctx, kf1, keys1, kf2, key_start, keys2, match_start, matches, monocular=False, outputs=OUTPUTS):
    """One lld_new_points_triangulate call.  kf1: the current keyframe's record (see keyframe_record); keys1: mapping with xy
    (mvKeysUn), ur (mvuRight), depth (mvDepth), octave and optionally raw_xy (mvKeys); kf2: the neighbours' records; keys2: their
    keypoints concatenated under key_start (n_pairs + 1); matches (n_matches x 2: idx1, idx2 within the pair's keyframe)
    concatenated under match_start (n_pairs + 1).  outputs: the names of the arrays wanted."""
    a, n = pack_problem(kf1, keys1, kf2, key_start, keys2, match_start, matches, monocular)
    n_pairs = len(kf2)
    want = set(outputs)
    unknown = want - set(OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    r = NewPoints(np.zeros(n, np.uint8) if "status" in want else None, np.zeros(n, np.uint8) if "source" in want else None,
                  np.zeros((n, 3), np.float32) if "x3d" in want else None, np.zeros(n_pairs, np.uint8) if "pair_status" in want else None,
                  np.zeros(n_pairs, np.int32) if "n_new" in want else None, np.full(n, -1, np.int32) if "new_match" in want else None, 0)
    o = NewPointsOut()
    o.status = _ptr(r.status, c_uint8_p); o.source = _ptr(r.source, c_uint8_p); o.x3d = _ptr(r.x3d, c_float_p)
    o.pair_status = _ptr(r.pair_status, c_uint8_p); o.n_new = _ptr(r.n_new, c_int32_p); o.new_match = _ptr(r.new_match, c_int32_p)
    st = ctx.lib.fn("new_points_triangulate")(ctx.handle, C.byref(a), C.byref(o))
    if st != abi.LLD_OK:
        raise NewPointsError("lld_new_points_triangulate", st)
    r.n_new_total = int(o.n_new_total)
    if r.new_match is not None:
        r.new_match = r.new_match[:r.n_new_total].copy()
    return r
