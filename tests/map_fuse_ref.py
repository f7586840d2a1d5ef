"""lld_map_fuse restated in plain Python on the map model of tests/map_ba_scenes.py / map_refresh_scenes.py (include/lld_amd.h, "duplicate
map points fused on the resident map"): ORBmatcher::Fuse(pKF, vpMapPoints, th) as adapters/lld_matcher_adapter.cc restates it - the search
of every candidate first, then the walk over the matched ones in list order.  No kernel's structure is followed.  numpy only.

The search is written from the rules of include/lld_amd.h ("guided ORB search": LLD_ORB_CAND_GRID, the LEVEL and CHI2 gates, the float /
double mixture of the projection), candidate by candidate and keypoint by keypoint in GetFeaturesInArea's order; it imports nothing of the
library.  Every float operation is an explicit np.float32 operation; a float compared with a double literal is compared in Python floats.

A view is a dict: Rcw (9), tcw (3), Ow (3), fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y, log_scale_factor, n_levels.  A grid is the tuple
(min_x, min_y, width_inv, height_inv, cols, rows).  A keyframe of the model holds key, bad, points, uvr, octave, desc; a point bad, pos, nrm,
mind, maxd, desc, obs [(keyframe slot, keypoint index)] and n_obs.  fuse() works on a deep copy."""
import copy
import ctypes
import ctypes.util

import numpy as np

import map_refresh_ref as RF

NONE, ADDED, CANDIDATE_REPLACED, HOLDER_REPLACED, HOLDER_BAD, SKIPPED = 0, 1, 2, 3, 4, 5
TH_LOW = 50
MAX_OBS = 1024                                     # LLD_LANDMARK_MAX_OBS
f32, f64 = np.float32, np.float64

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.argtypes = [ctypes.c_float]; _libm.logf.restype = ctypes.c_float


def popcount(a, b):
    return int(np.unpackbits((np.asarray(a, np.uint32) ^ np.asarray(b, np.uint32)).view(np.uint8)).sum())


def c_round(x):
    """C round(): half away from zero"""
    return int(np.floor(abs(float(x)) + 0.5) * (1 if x >= 0 else -1))


def gemm(R, P, t):
    """`R*P + t` as one cv::gemm on float data: double accumulation in k order, one rounding"""
    return np.array([f32(f64(R[r, 0]) * f64(P[0]) + f64(R[r, 1]) * f64(P[1]) + f64(R[r, 2]) * f64(P[2]) + f64(t[r])) for r in range(3)], f32)


def dot(a, b):
    return float(f64(a[0]) * f64(b[0]) + f64(a[1]) * f64(b[1]) + f64(a[2]) * f64(b[2]))


def predict_scale(max_distance, dist, log_scale_factor, n_levels):
    """MapPoint::PredictScale (src/MapPoint.cc:402-417): float ratio, the platform's float log, float quotient, ceil, clamp"""
    with np.errstate(all="ignore"):
        ratio = f32(f32(max_distance) / f32(dist))
        q = f32(f32(_libm.logf(float(ratio))) / f32(log_scale_factor))
        n = int(np.ceil(q)) if np.isfinite(q) else (0 if q < 0 or np.isnan(q) else n_levels)
    return 0 if n < 0 else (n_levels - 1 if n >= n_levels else n)


def project(view, p):
    """The projection loop of Fuse for one point (src/ORBmatcher.cc:852-890): (u, v, ur, level) or None"""
    R = np.asarray(view["Rcw"], f32).reshape(3, 3); t = np.asarray(view["tcw"], f32); Ow = np.asarray(view["Ow"], f32)
    fx, fy, cx, cy, bf = (f32(view[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    P = np.asarray(p["pos"], f32)
    Pc = gemm(R, P, t)
    if Pc[2] < 0:
        return None
    with np.errstate(all="ignore"):
        invz = f32(f32(1.0) / Pc[2])
        u = f32(f32(fx * f32(Pc[0] * invz)) + cx); v = f32(f32(fy * f32(Pc[1] * invz)) + cy)
    if not (u >= f32(view["min_x"]) and u < f32(view["max_x"]) and v >= f32(view["min_y"]) and v < f32(view["max_y"])):      # KeyFrame::IsInImage
        return None
    ur = f32(u - f32(bf * invz))
    PO = (P - Ow).astype(f32)
    dist = f32(np.sqrt(dot(PO, PO)))
    if dist < f32(f32(0.8) * f32(p.get("mind", 0))) or dist > f32(f32(1.2) * f32(p.get("maxd", 0))):
        return None
    if dot(PO, np.asarray(p.get("nrm", np.zeros(3)), f32)) < 0.5 * float(dist):
        return None
    return u, v, ur, predict_scale(p.get("maxd", 0), dist, view["log_scale_factor"], int(view["n_levels"]))


def grid_cells(uvr, grid):
    """KeyFrame::AssignFeaturesToGrid + PosInGrid: cell -> keypoint indices in index order; a keypoint outside the grid is in no cell"""
    min_x, min_y, winv, hinv, cols, rows = grid
    cells = {}
    for k in range(len(uvr)):
        px = c_round(f32(f32(f32(uvr[k][0]) - f32(min_x)) * f32(winv))); py = c_round(f32(f32(f32(uvr[k][1]) - f32(min_y)) * f32(hinv)))
        if 0 <= px < cols and 0 <= py < rows:
            cells.setdefault((px, py), []).append(k)
    return cells


def search_one(kf, cells, proj, desc, grid, level_scale, inv_sigma2, th):
    """bestIdx of one projected point among the keyframe's keypoints (src/ORBmatcher.cc:892-934), or -1"""
    u, v, ur, lvl = proj
    min_x, min_y, winv, hinv, cols, rows = grid
    r = f32(f32(th) * f32(level_scale[lvl]))
    lo, hi = (lambda x: int(np.floor(x))), (lambda x: int(np.ceil(x)))
    x0 = max(0, lo(f32(f32(f32(u - f32(min_x)) - r) * f32(winv))))
    if x0 >= cols: return -1
    x1 = min(cols - 1, hi(f32(f32(f32(u - f32(min_x)) + r) * f32(winv))))
    if x1 < 0: return -1
    y0 = max(0, lo(f32(f32(f32(v - f32(min_y)) - r) * f32(hinv))))
    if y0 >= rows: return -1
    y1 = min(rows - 1, hi(f32(f32(f32(v - f32(min_y)) + r) * f32(hinv))))
    if y1 < 0: return -1
    best, best_idx = 256, -1
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for k in cells.get((ix, iy), ()):
                kx, ky, kur = (f32(c) for c in kf["uvr"][k])
                if not (abs(f32(kx - u)) < r and abs(f32(ky - v)) < r):
                    continue
                o = int(kf["octave"][k])
                if o < 0 or o < lvl - 1 or o > lvl:
                    continue
                ex, ey = f32(u - kx), f32(v - ky)
                e2 = f32(f32(ex * ex) + f32(ey * ey))
                if kur >= 0:
                    er = f32(ur - kur)
                    e2 = f32(e2 + f32(er * er))
                    if float(f32(e2 * f32(inv_sigma2[o]))) > 7.8: continue
                elif float(f32(e2 * f32(inv_sigma2[o]))) > 5.99: continue
                d = popcount(desc, kf["desc"][k])
                if d < best:
                    best, best_idx = d, k
    return best_idx if best <= TH_LOW else -1


def skipped(m, target, s):
    p = m["points"].get(s) if s >= 0 else None
    return p is None or bool(p["bad"]) or any(kf == target for kf, _ in p["obs"])


def search(m, target, slots, view, grid, level_scale, inv_sigma2, th=3.0):
    """match per candidate: the search alone"""
    kf = m["keyframes"][target]
    cells = grid_cells(kf["uvr"], grid)
    out = np.full(len(slots), -1, np.int32)
    for i, s in enumerate(int(v) for v in slots):
        if skipped(m, target, s):
            continue
        p = m["points"][s]
        proj = project(view, p)
        if proj is not None:
            out[i] = search_one(kf, cells, proj, p.get("desc", np.zeros(8, np.uint32)), grid, level_scale, inv_sigma2, th)
    return out


def n_obs_of(p):
    return int(p.get("n_obs", len(p["obs"])))


def stereo(m, kf, idx):
    k = m["keyframes"].get(kf)
    return k is not None and "uvr" in k and idx < len(k["uvr"]) and k["uvr"][idx][2] >= 0


def key_of(m, kf):
    return m["keyframes"][kf]["key"] if kf in m["keyframes"] else 0


def set_match(m, kf, idx, v):
    k = m["keyframes"].get(kf)
    if k is not None and idx < len(k["points"]):
        k["points"][idx] = v


def add_observation(m, s, kf, idx):
    """MapPoint::AddObservation (src/MapPoint.cc:67-78); the entry goes where std::map<KeyFrame*, size_t> would hold it"""
    p = m["points"][s]
    if any(o[0] == kf for o in p["obs"]):
        return
    at = 0
    while at < len(p["obs"]) and key_of(m, p["obs"][at][0]) <= key_of(m, kf):
        at += 1
    p["obs"].insert(at, (kf, idx))
    p["n_obs"] = n_obs_of(p) + (2 if stereo(m, kf, idx) else 1)


def replace(m, loser, surv):
    """loser->Replace(survivor) (src/MapPoint.cc:176-220) without mnFound / mnVisible and the descriptor; False: the same point"""
    if loser == surv:
        return False
    pl = m["points"][loser]
    obs = pl["obs"]
    pl["n_obs"] = n_obs_of(pl)                                                # nObs stays what it was
    pl["obs"] = []; pl["bad"] = 1
    for kf, idx in obs:
        if not any(o[0] == kf for o in m["points"][surv]["obs"]):
            set_match(m, kf, idx, surv); add_observation(m, surv, kf, idx)
        else:
            set_match(m, kf, idx, -1)
    return True


def fuse(m, target, slots, view, grid, level_scale, inv_sigma2, th=3.0, source_keyframe=-1):
    """(the map behind the call, what lld_map_fuse_out must hold).  With source_keyframe >= 0 the candidates are that keyframe's point row.
    A survivor row longer than LLD_LANDMARK_MAX_OBS: (m unchanged, None) - the call is refused."""
    if source_keyframe >= 0:
        slots = list(m["keyframes"][source_keyframe]["points"])
    slots = [int(s) for s in slots]
    match = search(m, target, slots, view, grid, level_scale, inv_sigma2, th)
    before = m
    m = copy.deepcopy(m)
    P, K = m["points"], m["keyframes"]
    n = len(slots)
    action = np.zeros(n, np.uint8); other = np.full(n, -1, np.int32)
    survivors = []
    n_fused = n_added = n_replaced = 0
    for i, s in enumerate(slots):
        b = int(match[i])
        if b < 0:
            continue
        if skipped(m, target, s):                                            # replaced or attached by an earlier step (:848)
            action[i] = SKIPPED
            continue
        h = K[target]["points"][b]
        if h < 0:
            add_observation(m, s, target, b); set_match(m, target, b, s)
            action[i] = ADDED; n_added += 1
        elif h not in P or P[h]["bad"]:
            action[i] = HOLDER_BAD; other[i] = h
        else:
            other[i] = h; n_replaced += 1
            if n_obs_of(P[h]) > n_obs_of(P[s]):
                action[i] = CANDIDATE_REPLACED; loser, surv = s, h
            else:
                action[i] = HOLDER_REPLACED; loser, surv = h, s
            if replace(m, loser, surv) and surv not in survivors:
                survivors.append(surv)
        n_fused += 1
    if any(len(P[s]["obs"]) > MAX_OBS for s in survivors):
        return before, None
    # ComputeDistinctiveDescriptors of every survivor, once, on the rows the call leaves (a survivor that went bad later keeps its descriptor)
    if survivors:
        RF.write_points(m, survivors, RF.refresh_points(m, survivors, RF.DESCRIPTOR))
    return m, dict(n_fused=n_fused, n_added=n_added, n_replaced=n_replaced, match=match, action=action, other=other, survivor=np.array(survivors, np.int32))


def gathered(m, target, slots):
    """What a caller without the resident search gathers for lld_orb_fuse_search: the keyframe's arrays and the candidates' (skip included)"""
    kf = m["keyframes"][target]
    uvr = np.asarray(kf["uvr"], f32).reshape(-1, 3)
    n = len(slots)
    mp = dict(world_pos=np.zeros((n, 3), f32), normal=np.zeros((n, 3), f32), max_distance=np.zeros(n, f32), min_distance=np.zeros(n, f32), desc=np.zeros((n, 8), np.uint32),
              skip=np.zeros(n, np.uint8))
    for i, s in enumerate(int(v) for v in slots):
        if skipped(m, target, s):
            mp["skip"][i] = 1
            continue
        p = m["points"][s]
        mp["world_pos"][i] = p["pos"]; mp["normal"][i] = p.get("nrm", 0); mp["max_distance"][i] = p.get("maxd", 0); mp["min_distance"][i] = p.get("mind", 0)
        mp["desc"][i] = p.get("desc", 0)
    return dict(desc=np.asarray(kf["desc"], np.uint32).reshape(-1, 8), xy=uvr[:, :2].copy(), octave=np.asarray(kf["octave"], np.int32), uright=uvr[:, 2].copy()), mp


def counts_of(m, slots):
    """what DeviceMap.point_counts(slots) must return for map m"""
    return np.array([n_obs_of(m["points"][s]) if s in m["points"] else 0 for s in slots], np.int32)
