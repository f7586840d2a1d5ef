"""lld_map_ba_apply restated in plain Python on the map model of tests/map_ba_ref.py (include/lld_amd.h, "a local BA's result applied to the
resident map"): the last third of Optimizer::LocalBundleAdjustment, object by object, as the reference walks it.  No kernel's structure is
followed.  numpy only.

Beyond map_ba_ref's fields a point may hold n_obs (default: the length of its row), nrm (3,) float32, mind, maxd (default 0) and ref_kf (a
keyframe slot or -1; when NO point of the map has the key, lld_map_set_point_refs was never called).  apply() works on a deep copy and
returns (the mutated map, what lld_map_ba_apply_out must hold)."""
import copy

import numpy as np

WENT_BAD, REFRESHED, NO_REFERENCE, INDEX_SKIPPED = 1, 2, 4, 8
f32 = np.float32


def centre(Tcw):
    """KeyFrame::SetPose: Ow = -Rcw^T tcw, each entry a three-term sum in double in index order, rounded once."""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    ow = np.zeros(3, f32)
    for i in range(3):
        s = np.float64(T[0, i]) * np.float64(T[0, 3])
        s += np.float64(T[1, i]) * np.float64(T[1, 3])
        s += np.float64(T[2, i]) * np.float64(T[2, 3])
        ow[i] = -f32(s)
    return ow


def norm3(v):
    s = np.float64(v[0]) * np.float64(v[0])
    s += np.float64(v[1]) * np.float64(v[1])
    s += np.float64(v[2]) * np.float64(v[2])
    return np.sqrt(s)


def has_refs(m):
    return any("ref_kf" in p for p in m["points"].values())


def point_n_obs(p):
    return int(p.get("n_obs", len(p["obs"])))


def update_normal_and_depth(m, p, level_scale):
    """MapPoint::UpdateNormalAndDepth (:330-371) of a point that is not bad and has observations.  True: refreshed."""
    K = m["keyframes"]
    ref = p.get("ref_kf", -1)
    centre_of = lambda s: centre(K[s]["Tcw"]) if s in K and "uvr" in K[s] else None
    if ref < 0 or centre_of(ref) is None or any(centre_of(kf) is None for kf, _ in p["obs"]):
        return False
    idx = dict(p["obs"]).get(ref, 0)                                       # observations[pRefKF]: 0 for a keyframe that is no observer
    octs = K[ref].get("octave")
    if octs is None or idx >= len(octs) or not 0 <= octs[idx] < len(level_scale):
        return False
    pos = np.asarray(p["pos"], f32)
    n = np.zeros(3, f32)
    for kf, _ in p["obs"]:
        d = (pos - centre_of(kf)).astype(f32)
        inv = f32(1.0 / norm3(d))
        n = (n + (d * inv).astype(f32)).astype(f32)
    invn = f32(1.0 / np.float64(len(p["obs"])))
    p["nrm"] = (n * invn).astype(f32)
    dist = f32(norm3((pos - centre_of(ref)).astype(f32)))
    ls = np.asarray(level_scale, f32)
    p["maxd"] = f32(dist * ls[octs[idx]])
    p["mind"] = f32(p["maxd"] / ls[-1])
    return True


def apply(m, win, res, level_scale, se3_to_tcw):
    """win: a window of map_ba_ref.ba_window (status 0) on m; res: cam_qt, pt_xyz, line_x0, line_dir, pt_obs_outlier, ln_edge_outlier [n][2],
    line_removed; se3_to_tcw: lld_se3_to_tcw_f32 (SE3Quat -> float 4x4)."""
    m = copy.deepcopy(m)
    K, P, L = m["keyframes"], m["points"], m["lines"]
    refs = has_refs(m)
    g = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    cam_slot = [int(s) for s in win["cam_slot"]]
    out = dict(n_pt_obs_erased=0, n_ln_obs_erased=0, n_points_bad=0, n_lines_bad=0, n_index_skipped=0, n_local_cams=int(win["n_local_cams"]))
    po = np.asarray(g("pt_obs_outlier")).reshape(-1); lo = np.asarray(g("ln_edge_outlier")).reshape(-1, 2); rm = np.asarray(g("line_removed")).reshape(-1)

    def erase_match(kf, idx, rows):                                          # mvpMapPoints[idx] = NULL, by index
        row = K[kf][rows] if kf in K else []
        if idx < len(row):
            row[idx] = -1
            return 0
        return 1

    flags = np.zeros(len(win["point_slot"]), np.uint8)
    # ---- the erase list, mono edges first (:1282-1310), and the erasures (:1336-1345)
    for q, s in enumerate(int(v) for v in win["point_slot"]):
        p = P[s]
        n_obs = point_n_obs(p)
        run = [(e, cam_slot[win["pt_obs_cam"][e]]) for e in range(win["pt_obs_start"][q], win["pt_obs_start"][q + 1]) if po[e]]
        stereo = lambda kf: K[kf]["uvr"][dict(p["obs"])[kf]][2] >= 0
        order = [kf for _, kf in run if not stereo(kf)] + [kf for _, kf in run if stereo(kf)]
        skipped = 0
        for kf in order:
            if p["bad"]:
                break                                                        # mObservations is empty: nothing happens any more
            idx = dict(p["obs"])[kf]
            skipped += erase_match(kf, idx, "points")                        # KeyFrame::EraseMapPointMatch(pMP)
            n_obs -= 2 if K[kf]["uvr"][idx][2] >= 0 else 1
            p["obs"] = [o for o in p["obs"] if o[0] != kf]
            out["n_pt_obs_erased"] += 1
            if refs and p.get("ref_kf", -1) == kf and p["obs"]:
                p["ref_kf"] = p["obs"][0][0]                                 # mObservations.begin()->first
            if n_obs <= 2:                                                   # SetBadFlag
                p["bad"] = 1
                for okf, oidx in p["obs"]:
                    skipped += erase_match(okf, oidx, "points")
                p["obs"] = []
                if refs:
                    p["ref_kf"] = -1                                         # (the reference leaves an order-dependent value)
                out["n_points_bad"] += 1
                flags[q] |= WENT_BAD
        p["n_obs"] = n_obs
        if skipped:
            flags[q] |= INDEX_SKIPPED
            out["n_index_skipped"] += skipped
    ln_bad_now = set()
    for l, s in enumerate(int(v) for v in win["line_slot"]):
        if rm[l]:
            continue
        ln = L[s]
        for e in range(win["ln_obs_start"][l], win["ln_obs_start"][l + 1]):
            if not (lo[e, 0] or lo[e, 1]) or ln["bad"]:
                continue
            kf = cam_slot[win["ln_obs_cam"][e]]
            at = dict(ln["obs"])
            if kf not in at:
                continue
            idx = at[kf]
            out["n_index_skipped"] += erase_match(kf, idx, "lines")
            partner = not np.all(np.asarray(K[kf]["kl_right"], f32)[idx] == f32(-1))
            ln["n_obs"] -= 2 if partner else 1
            ln["obs"] = [o for o in ln["obs"] if o[0] != kf]
            out["n_ln_obs_erased"] += 1
            if ln["n_obs"] <= 4:                                             # MapLine::SetBadFlag: the row is cleared first, so no observer's entry is found
                ln["bad"] = 1; ln["obs"] = []
                out["n_lines_bad"] += 1
                ln_bad_now.add(s)
    # ---- the poses (:1364-1370)
    tcw = []
    for c in range(out["n_local_cams"]):
        T = np.asarray(se3_to_tcw(np.asarray(g("cam_qt"), np.float64).reshape(-1, 7)[c]), f32).reshape(4, 4)
        K[cam_slot[c]]["Tcw"] = T
        tcw.append(T)
    out["tcw"] = np.array(tcw, f32).reshape(-1, 4, 4)
    out["ow"] = np.array([centre(T) for T in tcw], f32).reshape(-1, 3)
    # ---- the points (:1373-1379)
    xyz = np.asarray(g("pt_xyz"), np.float64).reshape(-1, 3)
    for q, s in enumerate(int(v) for v in win["point_slot"]):
        p = P[s]
        p["pos"] = xyz[q].astype(f32)
        if p["bad"] or not p["obs"]:
            continue
        if update_normal_and_depth(m, p, level_scale):
            flags[q] |= REFRESHED
        else:
            flags[q] |= NO_REFERENCE
    # ---- the lines (:1382-1386)
    for l, s in enumerate(int(v) for v in win["line_slot"]):
        if not rm[l]:
            L[s]["x0"] = np.asarray(g("line_x0"), np.float64).reshape(-1, 3)[l].copy(); L[s]["dir"] = np.asarray(g("line_dir"), np.float64).reshape(-1, 3)[l].copy()
    pts = [P[int(s)] for s in win["point_slot"]]
    z3 = np.zeros(3, f32)
    out.update(pt_pos=np.array([p["pos"] for p in pts], f32).reshape(-1, 3), pt_normal=np.array([p.get("nrm", z3) for p in pts], f32).reshape(-1, 3),
               pt_min_distance=np.array([p.get("mind", 0) for p in pts], f32), pt_max_distance=np.array([p.get("maxd", 0) for p in pts], f32),
               pt_n_obs=np.array([p["n_obs"] for p in pts], np.int32), pt_ref_kf=np.array([p.get("ref_kf", -1) if refs else -1 for p in pts], np.int32),
               pt_row_len=np.array([len(p["obs"]) for p in pts], np.int32), pt_flags=flags)
    lns = [L[int(s)] for s in win["line_slot"]]
    out.update(ln_bad=np.array([l["bad"] for l in lns], np.uint8), ln_n_obs=np.array([l["n_obs"] for l in lns], np.int32),
               ln_row_len=np.array([len(l["obs"]) for l in lns], np.int32))
    return m, out


def rows_of(m, kind, slots):
    """what DeviceMap.rows(kind, slots) must return for map m"""
    K, P, L = m["keyframes"], m["points"], m["lines"]
    def one(s):
        if kind == "point_obs": return [o[0] for o in P[s]["obs"]] if s in P else []
        if kind == "point_idx": return [o[1] for o in P[s]["obs"]] if s in P and P[s].get("indexed", True) else []
        if kind == "kf_points": return list(K[s]["points"]) if s in K else []
        if kind == "kf_lines": return list(K[s]["lines"]) if s in K else []
        if kind == "line_obs": return [o[0] for o in L[s]["obs"]] if s in L and L[s]["obs"] is not None else []
        if kind == "line_idx": return [o[1] for o in L[s]["obs"]] if s in L and L[s]["obs"] is not None else []
        raise KeyError(kind)
    return [one(int(s)) for s in slots]
