"""Times the landmark refresh on the resident map against the gathering calls, two routes on one build and one MI355X, alternating in one
process, on README's landmark shapes:

  * 2000 MapPoints with 2-40 observations over 30 keyframes, both parts (SearchInNeighbors);
  * 5000 MapPoints, normal / depth only (LocalBundleAdjustment's tail);
  * 300 MapLines of dim 72.

  (A) lld_map_refresh_points / lld_map_refresh_lines: the slot list travels up, the map's rows are rewritten in place
  (B) lld_mappoint_refresh / lld_mapline_distinctive with the CSR ALREADY FLAT in host memory - a floor for the old route, which also walks
      the observation maps before the call and sends the results back into the map (lld_map_set_points / lld_map_set_lines) after it

  (C) on objects, host clock (examples/map_refresh_harness `time`, the first shape and the lines in one graph):
      MapOnDevice::RefreshMapPoints + ComputeDistinctiveDescriptors against lld_landmark_adapter followed by MapOnDevice::UpdatePoints /
      UpdateLines, on two identical graphs

Both routes are held to equal results, bit for bit, before anything is timed.  HIP events around the whole call (upload, kernels, download
and wait included), medians of --reps with interquartile ranges.  The bar is the project's own: route A's median below route B's by more
than the larger interquartile range; a miss is reported as a miss.  Needs an MI355X.

  python tools/time_map_refresh.py [--reps 200] [--out profiles/map_refresh_time.json]

The kernels' own times come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_map_refresh.py --reps 20"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import landmark_ref as L  # noqa: E402
from lld_slam_amd import Context  # noqa: E402
from lld_slam_amd.device_map import DeviceMap  # noqa: E402
from lld_slam_amd.landmarks import DESCRIPTOR, NORMAL_DEPTH, distinctive_line_descriptors, refresh_map_points  # noqa: E402


def quart(v):
    v = np.sort(np.asarray(v, np.float64))
    return dict(median=round(float(v[len(v) // 2]), 4), q1=round(float(v[len(v) // 4]), 4), q3=round(float(v[(3 * len(v)) // 4]), 4))


def verdict(new, old):
    iqr = max(new["q3"] - new["q1"], old["q3"] - old["q1"])
    return bool(new["median"] < old["median"] - iqr)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fa, fb, reps):
    for _ in range(5): fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(once(fa)); tb.append(once(fb))
    return quart(ta), quart(tb)


def rows_of(sc, n_kf):
    """keyframe k's feature row = the landmarks observing it in landmark order; per observation its index there"""
    rows = [[] for _ in range(n_kf)]; idx = np.zeros(len(sc["obs_kf"]), np.int32)
    for i in range(len(sc["bad"])):
        for o in range(sc["obs_start"][i], sc["obs_start"][i + 1]):
            k = int(sc["obs_kf"][o]); idx[o] = len(rows[k]); rows[k].append(i)
    return rows, idx


def open_map(ctx, pts, lns):
    """A resident map that holds both scenes: landmark i is slot i, keyframe k slot k with order_key k + 1 (the scenes list observers in
    ascending keyframe index), centre kf_ow[k] (identity rotation); mpRefKF = the first observer, its keypoint's octave = ref_level."""
    n_kf = len(pts["kf_bad"]); dim = lns["dim"]
    assert n_kf == len(lns["kf_bad"])
    n, nl = len(pts["bad"]), len(lns["bad"])
    prow, pidx = rows_of(pts, n_kf); lrow, lidx = rows_of(lns, n_kf)
    first = pts["obs_start"][:-1].clip(max=max(len(pts["obs_kf"]) - 1, 0))
    has = np.diff(pts["obs_start"]) > 0
    pts["ref_kf"] = np.where(has, pts["obs_kf"][first], 0).astype(np.int32)
    rng = np.random.default_rng(1)
    octave = [rng.integers(0, pts["n_levels"], len(r)).astype(np.int32) for r in prow]
    for i in np.flatnonzero(has):
        o = pts["obs_start"][i]; octave[pts["obs_kf"][o]][pidx[o]] = pts["ref_level"][i]
    dm = DeviceMap(ctx, max_keyframes=n_kf, max_points=n, max_lines=nl, line_dim=dim, max_observations=len(pts["obs_kf"]) + 8, max_kf_points=len(pts["obs_kf"]) + 8,
                   max_kf_lines=len(lns["obs_kf"]) + 8, max_children=8, max_local_points=64, max_local_lines=16)
    ks = list(range(n_kf)); none = [[] for _ in ks]
    bad = np.maximum(pts["kf_bad"], lns["kf_bad"]); pts["kf_bad"] = lns["kf_bad"] = bad
    dm.set_keyframes(ks, [k + 1 for k in ks], bad, [-1] * n_kf, none, none, prow, lrow)
    dm.set_keyframe_keypoints(ks, [o.tolist() for o in octave], [[0.0] * len(r) for r in prow], [0.0] * n_kf)
    T = np.tile(np.eye(4, dtype=np.float32), (n_kf, 1, 1)); T[:, :3, 3] = -pts["kf_ow"]
    dm.set_keyframe_features(ks, [k + 1 for k in ks], T, [np.zeros((len(r), 3), np.float32) for r in prow], [np.zeros((len(r), 4), np.float32) for r in lrow],
                             [np.zeros((len(r), 4), np.float32) for r in lrow], [np.zeros((len(r), 2), np.int32) for r in lrow])
    sl = np.arange(n, dtype=np.int32)
    dm.set_points(sl, pts["pos"], np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 8), np.uint32), pts["bad"])
    dm.set_observations_indexed(sl, start=pts["obs_start"], kf_slot=pts["obs_kf"], kp_index=pidx, n_obs=np.diff(pts["obs_start"]))
    dm.set_point_refs(sl, np.where(has, pts["ref_kf"], -1))
    z = np.zeros((nl, 3))
    dm.set_lines(np.arange(nl), z, z, z, z, np.zeros((nl, dim), np.float32), lns["bad"])
    per = lambda start: [list(zip(lns["obs_kf"][a:b].tolist(), lidx[a:b].tolist())) for a, b in zip(start[:-1], start[1:])]
    dm.set_line_observations(np.arange(nl), per(lns["obs_start"]), (2 * np.diff(lns["obs_start"])).tolist())
    kd = [np.zeros((len(r), 8), np.uint32) for r in prow]; kl = [np.zeros((len(r), dim), np.float32) for r in lrow]
    for o, k in enumerate(pts["obs_kf"]): kd[k][pidx[o]] = pts["obs_desc"][o]
    for o, k in enumerate(lns["obs_kf"]): kl[k][lidx[o]] = lns["obs_desc"][o]
    dm.set_keyframe_descriptors(ks, kd); dm.set_keyframe_line_descriptors(ks, kl)
    return dm


def objects_case(reps):
    """The first shape (and the 300 lines) as an object graph through examples/map_refresh_harness `time`: host clock, (a)
    MapOnDevice::RefreshMapPoints + ComputeDistinctiveDescriptors against (b) lld_landmark_adapter followed by MapOnDevice::UpdatePoints /
    UpdateLines, alternating in one process on two identical graphs."""
    n = 2000
    counts = np.minimum(np.random.default_rng(n).integers(2, 41, n), 30)
    pts = L.make_point_scene(100 + n, n_kf=30, counts=counts, p_bad=0.02, p_all_bad=0.0)
    lns = L.make_line_scene(7, n_lines=300, n_kf=30, dim=72, scaled=True)
    lns["kf_bad"] = pts["kf_bad"].copy()
    pts["ref_kf"] = pts["obs_kf"][pts["obs_start"][:-1]].astype(np.int32)          # mpRefKF: the first observer
    prior = dict(desc=np.zeros((n, 8), np.uint32), normal=np.zeros((n, 3), np.float32), min_distance=np.zeros(n, np.float32), max_distance=np.zeros(n, np.float32))
    blob, _ = L.object_scene_blob(pts, lns, DESCRIPTOR | NORMAL_DEPTH, prior, np.zeros((300, 72), np.float32))
    harness = os.path.join(ROOT, "examples", "map_refresh_harness")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.bin")
        with open(path, "wb") as f:
            f.write(blob)
        r = subprocess.run([harness, "time", path, str(reps)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("map_refresh_harness time failed: " + r.stdout[-400:] + r.stderr)
    d = json.loads(r.stdout)
    qa, qb = quart(d["map_route_ms"]), quart(d["adapter_and_update_ms"])
    assert d["written_map"] == d["written_adapter"], "the routes on objects disagree"
    return dict(case="on objects, host clock: 2000 points both parts + 300 lines of dim 72", points=d["points"], lines=d["lines"], written=d["written_map"],
                a_map_on_device_refresh_ms=qa, b_landmark_adapter_then_update_points_ms=qb, met=verdict(qa, qb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"reps": a.reps, "timer": "HIP events around the whole call, routes alternating in one process, medians with quartiles",
           "bar": "route A's median below route B's by more than the larger interquartile range",
           "route_b": "the CSR already flat in host memory: a floor for the gathering route", "cases": []}
    with Context(0) as ctx:
        lns = L.make_line_scene(7, n_lines=300, n_kf=30, dim=72, scaled=True)
        for name, n, flags in (("SearchInNeighbors: 2000 points, 2-40 observations, both parts", 2000, DESCRIPTOR | NORMAL_DEPTH),
                               ("LocalBundleAdjustment tail: 5000 points, normal / depth", 5000, NORMAL_DEPTH)):
            counts = np.minimum(np.random.default_rng(n).integers(2, 41, n), 30)     # 2-40 observations, at most one per keyframe
            pts = L.make_point_scene(100 + n, n_kf=30, counts=counts, p_bad=0.02, p_all_bad=0.0)
            with open_map(ctx, pts, lns) as dm:
                slots = np.arange(n, dtype=np.int32)
                fa = lambda: dm.refresh_points(slots, flags, pts["level_scale"])
                fb = lambda: refresh_map_points(ctx, pts["obs_start"], pts["obs_kf"], pts["bad"], obs_desc=pts["obs_desc"], kf_bad=pts["kf_bad"], kf_ow=pts["kf_ow"],
                                                pos=pts["pos"], ref_kf=pts["ref_kf"], ref_level=pts["ref_level"], level_scale=pts["level_scale"], flags=flags)
                ga, gb = fa(), fb()
                assert np.array_equal(ga["updated"], gb.updated), "the routes disagree: updated"
                for k in ("desc", "best_obs", "best_median", "normal", "min_distance", "max_distance"):
                    if getattr(gb, k) is not None:
                        assert ga[k].tobytes() == getattr(gb, k).tobytes(), "the routes disagree: " + k
                qa, qb = alternate(fa, fb, a.reps)
                res["cases"].append(dict(case=name, points=n, observations=int(len(pts["obs_kf"])), keyframes=30, flags=flags, written=int(np.sum(ga["updated"] != 0)),
                                         a_lld_map_refresh_points_ms=qa, b_lld_mappoint_refresh_flat_csr_ms=qb, met=verdict(qa, qb)))
                if n == 2000:
                    ls = np.arange(len(lns["bad"]), dtype=np.int32)
                    fa = lambda: dm.refresh_lines(ls)
                    fb = lambda: distinctive_line_descriptors(ctx, lns["obs_start"], lns["obs_kf"], lns["obs_desc"], lns["kf_bad"], lns["bad"])
                    ga, gb = fa(), fb()
                    for k in ("desc", "best_obs", "best_median", "updated"):
                        assert ga[k].tobytes() == getattr(gb, k).tobytes(), "the line routes disagree: " + k
                    qa, qb = alternate(fa, fb, a.reps)
                    res["cases"].append(dict(case="300 lines of dim 72", lines=len(ls), observations=int(len(lns["obs_kf"])), written=int(np.sum(ga["updated"] != 0)),
                                             a_lld_map_refresh_lines_ms=qa, b_lld_mapline_distinctive_flat_csr_ms=qb, met=verdict(qa, qb)))
    res["cases"].append(objects_case(a.reps))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
