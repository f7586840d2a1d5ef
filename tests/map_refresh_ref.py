"""lld_map_refresh_points / lld_map_refresh_lines restated in plain Python on the map model of tests/map_ba_scenes.py (include/lld_amd.h,
"landmark refresh on the resident map"): a gather of the stored rows, the index rows and the keyframes' descriptor rows into the scene form
tests/landmark_ref.py takes, then refresh_map_points_ref / distinctive_lines_ref, plus the rules that decide which landmarks are flagged and
left alone.  No kernel's structure is followed.  numpy only.

Beyond map_ba_scenes' fields: a keyframe may hold desc ((n_keypoints, 8) uint32, mDescriptors) and ldesc ((n_keylines, dim) float32,
mDescriptorsLines); a point desc (8 uint32), nrm, mind, maxd, ref_kf (tests/map_ba_apply_ref.py's names); a line desc (dim float32).  A
keyframe slot that is no key of the map was never set: it is bad and has no centre."""
import numpy as np

import landmark_ref as LM
from map_ba_apply_ref import centre

DESCRIPTOR, NORMAL_DEPTH, NO_INDEX, NO_DESCRIPTOR, NO_REFERENCE = 1, 2, 4, 8, 16
f32 = np.float32


def kf_table(m, extra=()):
    """(n_kf, kf_bad, kf_ow): the keyframe table by slot; a slot never set is bad, a keyframe without features has the centre 0 (never read)."""
    K = m["keyframes"]
    seen = [kf for p in m["points"].values() for kf, _ in (p["obs"] or [])] + [kf for l in m["lines"].values() for kf, _ in (l["obs"] or [])]
    n_kf = max(list(K) + seen + list(extra) + [0]) + 1
    bad = np.array([1 if s not in K else K[s]["bad"] for s in range(n_kf)], np.uint8)
    ow = np.array([centre(K[s]["Tcw"]) if s in K and "uvr" in K[s] else np.zeros(3, f32) for s in range(n_kf)], f32).reshape(-1, 3)
    return n_kf, bad, ow


def has_centre(m, s):
    return s in m["keyframes"] and "uvr" in m["keyframes"][s]


def point_flags(m, s, flags, n_levels):
    """(early, guard bits, level) of point slot s: early = the routine returns before it reads anything; a guard bit = not written at all."""
    K, p = m["keyframes"], m["points"].get(s)
    if p is None or p["bad"] or not p["obs"]:
        return True, 0, 0
    if not p.get("indexed", True):
        return False, NO_INDEX, 0
    g, level = 0, 0
    if flags & DESCRIPTOR:
        for kf, idx in p["obs"]:
            if kf in K and not K[kf]["bad"] and ("desc" not in K[kf] or idx >= len(K[kf]["desc"])):
                g |= NO_DESCRIPTOR
    if flags & NORMAL_DEPTH:
        ref = p.get("ref_kf", -1)
        ok = ref >= 0 and has_centre(m, ref) and all(has_centre(m, kf) for kf, _ in p["obs"])
        if ok:
            idx = dict(p["obs"]).get(ref, 0)                                # observations[pRefKF]: 0 for a keyframe that is no observer
            octs = K[ref].get("octave")
            ok = octs is not None and idx < len(octs) and 0 <= octs[idx] < n_levels
            if ok:
                level = int(octs[idx])
        if not ok:
            g |= NO_REFERENCE
    return False, g, level


def gather_points(m, slots, flags, level_scale):
    """The named points as a landmark_ref scene (a point that returns early or is flagged is `bad` there: left alone), the prior values, and
    the guard bits per query."""
    K, P = m["keyframes"], m["points"]
    n_levels = 0 if level_scale is None else len(level_scale)
    n_kf, kf_bad, kf_ow = kf_table(m)
    start, obs_kf, obs_desc = [0], [], []
    n = len(slots)
    bad = np.zeros(n, np.uint8); guard = np.zeros(n, np.uint8); ref_kf = np.zeros(n, np.int32); ref_level = np.zeros(n, np.int32)
    pos = np.zeros((n, 3), f32)
    prior = dict(desc=np.zeros((n, 8), np.uint32), normal=np.zeros((n, 3), f32), min_distance=np.zeros(n, f32), max_distance=np.zeros(n, f32))
    for q, s in enumerate(int(v) for v in slots):
        early, g, level = point_flags(m, s, flags, n_levels)
        p = P.get(s)
        if p is not None:
            pos[q] = p["pos"]
            prior["desc"][q] = p.get("desc", 0); prior["normal"][q] = p.get("nrm", 0); prior["min_distance"][q] = p.get("mind", 0); prior["max_distance"][q] = p.get("maxd", 0)
        guard[q] = g
        if early or g:
            bad[q] = 1
        else:
            for kf, idx in p["obs"]:
                obs_kf.append(kf)
                live = kf in K and not K[kf]["bad"] and "desc" in K[kf] and idx < len(K[kf]["desc"])
                obs_desc.append(np.asarray(K[kf]["desc"][idx], np.uint32) if live else np.zeros(8, np.uint32))     # a bad observer's row is not read
            ref_kf[q] = max(p.get("ref_kf", -1), 0); ref_level[q] = level
        start.append(len(obs_kf))
    sc = dict(obs_start=np.array(start, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_desc=np.array(obs_desc, np.uint32).reshape(-1, 8), kf_ow=kf_ow, kf_bad=kf_bad,
              pos=pos, bad=bad, ref_kf=ref_kf, ref_level=ref_level, n_levels=n_levels, level_scale=None if level_scale is None else np.asarray(level_scale, f32))
    return sc, prior, guard


def refresh_points(m, slots, flags=DESCRIPTOR | NORMAL_DEPTH, level_scale=None):
    """What lld_map_refresh_points must return for the point slots `slots` of m: desc, best_obs, best_median, normal, min_distance,
    max_distance (the rows behind the call) and updated.  m is not changed (write_points does that)."""
    sc, prior, guard = gather_points(m, slots, flags, level_scale)
    out = LM.refresh_map_points_ref(sc, flags, prior)
    out["updated"] = (out["updated"] | guard).astype(np.uint8)
    return out


def write_points(m, slots, out):
    """the model after the call"""
    for q, s in enumerate(int(v) for v in slots):
        if out["updated"][q] & DESCRIPTOR:
            m["points"][s]["desc"] = out["desc"][q].copy()
        if out["updated"][q] & NORMAL_DEPTH:
            m["points"][s]["nrm"] = out["normal"][q].copy(); m["points"][s]["mind"] = out["min_distance"][q]; m["points"][s]["maxd"] = out["max_distance"][q]


def gather_lines(m, slots, dim):
    K, L = m["keyframes"], m["lines"]
    n_kf, kf_bad, _ = kf_table(m)
    start, obs_kf, obs_desc = [0], [], []
    n = len(slots)
    bad = np.zeros(n, np.uint8); guard = np.zeros(n, np.uint8); prior = np.zeros((n, dim), f32)
    for q, s in enumerate(int(v) for v in slots):
        l = L.get(s)
        if l is not None:
            prior[q] = l.get("desc", 0)
        if l is None or l["bad"] or not l["obs"]:                            # a line never set is bad
            bad[q] = 1
        else:
            for kf, idx in l["obs"]:
                if kf in K and not K[kf]["bad"] and ("ldesc" not in K[kf] or idx >= len(K[kf]["ldesc"])):
                    guard[q] |= NO_DESCRIPTOR
            if guard[q]:
                bad[q] = 1
            else:
                for kf, idx in l["obs"]:
                    obs_kf.append(kf)
                    live = kf in K and not K[kf]["bad"]
                    obs_desc.append(np.asarray(K[kf]["ldesc"][idx], f32) if live else np.zeros(dim, f32))
        start.append(len(obs_kf))
    sc = dict(obs_start=np.array(start, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_desc=np.array(obs_desc, f32).reshape(-1, dim), kf_bad=kf_bad, bad=bad, dim=dim)
    return sc, prior, guard


def refresh_lines(m, slots, dim):
    """What lld_map_refresh_lines must return: desc, best_obs, best_median, updated."""
    sc, prior, guard = gather_lines(m, slots, dim)
    out = LM.distinctive_lines_ref(sc, prior)
    out["updated"] = (out["updated"] | guard).astype(np.uint8)
    return out


def write_lines(m, slots, out):
    for q, s in enumerate(int(v) for v in slots):
        if out["updated"][q] & DESCRIPTOR:
            m["lines"][s]["desc"] = out["desc"][q].copy()
