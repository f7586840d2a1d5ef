"""Times covisibility on the resident map (lld_map_covisibility) against the two routes the project had before it, on one MI355X, on the
shape of the README's covisibility row (31 keyframes x 1500 map points, 7750 points, about 46 500 observations; tools/time_covisibility.py
builds it).  Three cases each: UpdateConnections for 30 keyframes, KeyFrameCulling's count over 30, UpdateConnections for one keyframe.
  1. flat tables: lld_map_covisibility against lld_covisibility on the same build and the same data, alternating in this process.  Per call
     the HIP-event times of upload + kernels + download (phase_ms of either call) and the host clock around the whole call, which for
     lld_covisibility includes packing the observation table into the pinned block.  The outputs are compared for equality (slot = index and
     order_key ascends with it, so no renumbering is needed).
  2. objects: examples/map_covis_harness `time`: MapOnDevice::UpdateConnections / KeyFrameCulling against the host loops on an identical copy
     of the graph, alternating, host clock.
Medians of --reps with quartiles.  `met`: the new median is below the other route's by more than the larger interquartile range.
Writes the JSON to --out; --scene-out keeps the scene blob (for a profiler run of the harness)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import covis_scenes as S  # noqa: E402
from time_covisibility import local_map  # noqa: E402

HARNESS = os.path.join(ROOT, "examples", "map_covis_harness")


def quart(v):
    v = np.sort(np.asarray(v, np.float64))
    return dict(median=round(float(v[len(v) // 2]), 4), q1=round(float(v[len(v) // 4]), 4), q3=round(float(v[(3 * len(v)) // 4]), 4))


def verdict(new, old):
    iqr = max(new["q3"] - new["q1"], old["q3"] - old["q1"])
    return bool(new["median"] < old["median"] - iqr)


def flat_tables(world, reps):
    from lld_slam_amd import Context, covisibility as CV
    from lld_slam_amd.device_map import DeviceMap
    n_kf = len(world.kfs)
    cases = []
    with Context(0) as ctx:
        L = dict(max_keyframes=n_kf, max_points=len(world.obs), max_lines=1, line_dim=8, max_observations=sum(len(o) for o in world.obs) + 8,
                 max_kf_points=sum(len(k.keys) for k in world.kfs) + 8, max_kf_lines=0, max_children=8, max_local_points=64, max_local_lines=1)
        with DeviceMap(ctx, **L) as dm:
            slots = list(range(n_kf)); pts = list(range(len(world.obs))); n = len(pts)
            dm.set_keyframes(slots, [k + 1 for k in slots], [0] * n_kf, [-1] * n_kf, [[]] * n_kf, [[]] * n_kf, [[key[3] for key in k.keys] for k in world.kfs], [[]] * n_kf)
            dm.set_keyframe_keypoints(slots, [[key[0] for key in k.keys] for k in world.kfs], [[key[1] for key in k.keys] for k in world.kfs], [k.th_depth for k in world.kfs])
            dm.set_points(pts, np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 8), np.uint32), world.bad)
            dm.set_observations_indexed(pts, rows=[list(o.items()) for o in world.obs], n_obs=world.nobs)
            for name, queries, conn in (("UpdateConnections", slots[:-1], True), ("KeyFrameCulling", slots[:-1], False), ("UpdateConnections_one", [n_kf - 1], True)):
                sc = world.flat(queries)
                flags = CV.CONNECTIONS if conn else CV.CULLING
                kw = {} if conn else dict(obs_octave=sc["obs_octave"], point_nobs=sc["point_nobs"], q_octave=sc["q_octave"], q_depth=sc["q_depth"], q_th_depth=sc["q_th_depth"])
                ph = np.zeros(3, np.float32)
                old = lambda: CV.covisibility(ctx, sc["n_kf"], sc["obs_start"], sc["obs_kf"], sc["point_bad"], sc["query_kf"], sc["q_start"], sc["q_point"], flags,
                                              monocular=sc["monocular"], phase_ms=ph, **kw)
                new = lambda: dm.covisibility(queries, connections=conn, culling=not conn, phase_ms=ph)
                a, b = old(), new()
                if conn:
                    for k in ("conn_start", "conn_kf", "conn_weight", "ordered_start", "ordered_kf", "ordered_weight", "n_max", "kf_max", "updated"):
                        assert np.array_equal(getattr(a[0], k), b[k]), k
                else:
                    for k in ("n_mps", "n_redundant", "redundant"):
                        assert np.array_equal(getattr(a[1], k), b[k]), k
                assert not b["status"].any()
                t = dict(old_ev=[], new_ev=[], old_wall=[], new_wall=[])
                for _ in range(reps):
                    for tag, f in (("old", old), ("new", new)):
                        t0 = time.perf_counter(); f(); t[tag + "_wall"].append((time.perf_counter() - t0) * 1e3); t[tag + "_ev"].append(float(ph.sum()))
                c = dict(case=name, keyframes=len(queries), lld_covisibility_events_ms=quart(t["old_ev"]), lld_map_covisibility_events_ms=quart(t["new_ev"]),
                         lld_covisibility_wall_ms=quart(t["old_wall"]), lld_map_covisibility_wall_ms=quart(t["new_wall"]), outputs_equal=True)
                c["met_events"] = verdict(c["lld_map_covisibility_events_ms"], c["lld_covisibility_events_ms"])
                c["met_wall"] = verdict(c["lld_map_covisibility_wall_ms"], c["lld_covisibility_wall_ms"])
                cases.append(c)
    return cases


def objects(world, reps, scene_out):
    n_kf = len(world.kfs)
    with tempfile.TemporaryDirectory() as tmp:
        path = scene_out or os.path.join(tmp, "scene.bin")
        with open(path, "wb") as f:
            f.write(world.blob(list(range(n_kf - 1)), n_kf - 1))
        out = subprocess.run([HARNESS, path, "time", str(reps)], capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit(out.stderr)
    cases = []
    for line in out.stdout.strip().split("\n"):
        c = json.loads(line)
        new = dict(median=c["resident_ms"], q1=c["resident_q1"], q3=c["resident_q3"]); old = dict(median=c["host_loop_ms"], q1=c["host_q1"], q3=c["host_q3"])
        cases.append(dict(case=c["case"], keyframes=c["keyframes"], resident_ms=new, host_loop_ms=old, met=verdict(new, old)))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene-out", default=None)
    a = ap.parse_args()
    world = local_map(0)
    res = {"reps": a.reps, "keyframes": len(world.kfs), "points_per_keyframe": 1500, "map_points": len(world.obs), "observations": int(sum(len(o) for o in world.obs)),
           "bar": "new median below the other route's by more than the larger interquartile range",
           "objects_host_clock": objects(world, a.reps, a.scene_out), "flat_tables": flat_tables(world, a.reps)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
