"""lld_map_ba_window restated in plain Python on map tables (include/lld_amd.h, "the local BA window from the resident map"): what the
device must return, array for array.  No kernel's structure is followed: sets and lists, one landmark after the other.  numpy only.

A map is a dict of three dicts by slot (tests/map_ba_scenes.py builds and uploads them):
  keyframes  key (order_key), bad, points [point slot or -1 per keypoint], lines [line slot or -1 per keyline]; and, when the keyframe has
             features: mn_id, Tcw (4, 4) float32, uvr (n_kp, 3) float32, kl_left / kl_right (n_kl, 4) float32, kl_octave (n_kl, 2) int;
             and, when it has a keypoint row: octave [n_kp]
  points     bad, pos (3,) float32, obs [(keyframe slot, keypoint index)] in stored order, indexed (False: the row carries no indices)
  lines      bad, x0 / dir (3,) float64, obs [(keyframe slot, keyline index)] in stored order or None (no observation row), n_obs
A slot that is no key of its dict was never set.
Besides the window the result holds marked_bad: the keyframe slots the walk marks fixed although they are bad (what lld_map_local_ba
reports as marked_bad_slot), as a sorted list."""
import numpy as np

NO_FEATURE_DATA = 1
MAX_LOCAL = 1024
COUNTS = ("n_cams", "n_free_cams", "n_local_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs")
ARRAYS = ("cam_slot", "cam_qt", "point_slot", "pt_xyz", "pt_obs_start", "pt_obs_cam", "pt_obs_uvr", "pt_obs_inv_sigma2", "line_slot", "line_x0", "line_dir",
          "ln_obs_start", "ln_obs_cam", "ln_obs_left", "ln_obs_right", "ln_obs_octave")


class Refused(Exception):
    """LLD_ERR_INVALID before anything is queued."""


def has_features(k):
    return "uvr" in k


def camera_ok(k):
    """the feature rows the window reads of a camera have the lengths of its point and line rows"""
    return (has_features(k) and len(k["uvr"]) == len(k["points"]) and len(k["kl_left"]) == len(k["lines"]) and k.get("octave") is not None
            and len(k["octave"]) == len(k["points"]))


def ba_window(m, kf_slots, inv_level_sigma2, se3_from_tcw, max_keyframes=None):
    K, P, L = m["keyframes"], m["points"], m["lines"]
    kf_slots = [int(s) for s in kf_slots]
    n = len(kf_slots)
    if n < 1 or n > MAX_LOCAL or len(set(kf_slots)) != n:
        raise Refused()
    for s in kf_slots:
        if s < 0 or (max_keyframes is not None and s >= max_keyframes) or s not in K:
            raise Refused()
    sig = np.asarray(inv_level_sigma2, np.float32)
    status = 0
    is_bad = lambda s: s not in K or bool(K[s]["bad"])

    # :940-950
    local = set(kf_slots)
    listed = [s for i, s in enumerate(kf_slots) if i == 0 or not K[s]["bad"]]
    # :955-984
    lp, ll, seen_p, seen_l = [], [], set(), set()
    for s in listed:
        for p in K[s]["points"]:
            if p < 0 or p not in P or P[p]["bad"] or p in seen_p:
                continue
            seen_p.add(p); lp.append(p)
        for l in K[s]["lines"]:
            if l < 0 or l not in L or L[l]["bad"]:
                continue
            if L[l].get("obs") is None:
                status |= NO_FEATURE_DATA                   # not bad, and nothing to judge it by
                continue
            if L[l]["n_obs"] < 4 or l in seen_l:
                continue
            seen_l.add(l); ll.append(l)
    # :990-1018, with every stored index held to the observer's rows
    fixed, fixed_mark, marked_bad = [], set(), set()

    def visit(kf):
        if kf not in local and kf not in fixed_mark:
            fixed_mark.add(kf); fixed.append(kf)

    def visit_bad(kf):                                      # mnBAFixedForKF is set on it all the same; it is no camera (a slot never set is bad)
        if kf not in local:
            marked_bad.add(kf)

    for p in lp:
        row = P[p]["obs"]
        if row and not P[p].get("indexed", True):
            status |= NO_FEATURE_DATA
            continue
        for kf, idx in row:
            if is_bad(kf):
                visit_bad(kf)
                continue
            visit(kf)
            octs = K[kf].get("octave")
            if octs is None or idx < 0 or idx >= len(octs) or idx >= len(K[kf]["points"]):
                status |= NO_FEATURE_DATA
            elif not 0 <= octs[idx] < len(sig):
                status |= NO_FEATURE_DATA
    for l in ll:
        for kf, idx in L[l]["obs"]:
            if is_bad(kf):
                visit_bad(kf)
                continue
            visit(kf)
            if idx < 0 or idx >= len(K[kf]["lines"]):
                status |= NO_FEATURE_DATA
    # the cameras
    mn = lambda s: int(K[s]["mn_id"]) if has_features(K[s]) else 0
    free = sorted((s for s in listed if mn(s) != 0), key=lambda s: (mn(s), kf_slots.index(s)))
    cams = free + [s for s in listed if mn(s) == 0] + fixed
    for s in cams:
        if not camera_ok(K[s]):
            status |= NO_FEATURE_DATA
    if status:
        return dict({c: 0 for c in COUNTS}, status=status)
    cam_index = {s: i for i, s in enumerate(cams)}

    r = dict(status=0, marked_bad=sorted(marked_bad), n_cams=len(cams), n_free_cams=len(free), n_local_cams=len(listed), n_points=len(lp), n_lines=len(ll))
    r["cam_slot"] = np.array(cams, np.int32)
    r["cam_qt"] = np.array([se3_from_tcw(K[s]["Tcw"]) for s in cams], np.float64).reshape(-1, 7)
    r["point_slot"] = np.array(lp, np.int32)
    r["pt_xyz"] = np.array([np.asarray(P[p]["pos"], np.float32).astype(np.float64) for p in lp], np.float64).reshape(-1, 3)
    start, cam, uvr, s2 = [0], [], [], []
    for p in lp:
        for kf, idx in P[p]["obs"]:
            if is_bad(kf):
                continue
            cam.append(cam_index[kf])
            uvr.append(np.asarray(K[kf]["uvr"], np.float32)[idx].astype(np.float64))
            s2.append(np.float64(sig[K[kf]["octave"][idx]]))
        start.append(len(cam))
    r["pt_obs_start"] = np.array(start, np.int32); r["pt_obs_cam"] = np.array(cam, np.int32)
    r["pt_obs_uvr"] = np.array(uvr, np.float64).reshape(-1, 3); r["pt_obs_inv_sigma2"] = np.array(s2, np.float64)
    r["n_pt_obs"] = len(cam)
    r["line_slot"] = np.array(ll, np.int32)
    r["line_x0"] = np.array([L[l]["x0"] for l in ll], np.float64).reshape(-1, 3)
    r["line_dir"] = np.array([L[l]["dir"] for l in ll], np.float64).reshape(-1, 3)
    start, cam, left, right, octv = [0], [], [], [], []
    for l in ll:
        kept = [(int(K[kf]["mn_id"]), j, kf, idx) for j, (kf, idx) in enumerate(L[l]["obs"]) if not is_bad(kf)]
        for _, _, kf, idx in sorted(kept):                                # proj_map is keyed by mnId
            cam.append(cam_index[kf])
            left.append(np.asarray(K[kf]["kl_left"], np.float32)[idx].astype(np.float64))
            right.append(np.asarray(K[kf]["kl_right"], np.float32)[idx].astype(np.float64))
            octv.append([int(v) for v in K[kf]["kl_octave"][idx]])
        start.append(len(cam))
    r["ln_obs_start"] = np.array(start, np.int32); r["ln_obs_cam"] = np.array(cam, np.int32)
    r["ln_obs_left"] = np.array(left, np.float64).reshape(-1, 4); r["ln_obs_right"] = np.array(right, np.float64).reshape(-1, 4)
    r["ln_obs_octave"] = np.array(octv, np.int32).reshape(-1, 2)
    r["n_ln_obs"] = len(cam)
    return r
