"""Times one ORBmatcher::Fuse on the resident map against the gathering route, two routes on one build and one MI355X, alternating in one
process: one target keyframe of 2000 keypoints x 1500 candidates on a map of 31 keyframes (the shape of one call of
LocalMapping::SearchInNeighbors).  The call mutates the map, so the map is cleared and sent again before every repetition (not timed).

  (A) lld_map_fuse: the candidate slots travel up; search, walk, row upload and the survivors' descriptors in one call
  (B) on the same build, with its inputs ALREADY FLAT in host memory and the walk's outcome already known: lld_orb_fuse_search on the
      gathered keypoints and candidates, the setters that push the changed rows (lld_map_set_points, lld_map_set_observations_indexed,
      lld_map_set_keyframes) and lld_map_refresh_points for the survivors - a floor for the old route, which also gathers from objects
      before the call and walks objects after it

Both routes are held to the plain-Python restatement (tests/map_fuse_ref.py) and to each other's map before anything is timed.  HIP
events around the whole route (uploads, kernels, downloads and waits included), medians of --reps with interquartile ranges.  The bar is
the project's own: route A's median below route B's by more than the larger interquartile range; a miss is reported as a miss.
The intervals of (A) and (B) include the Python wrappers' own work (ctypes struct packing, numpy conversions of arrays that are already
numpy arrays): a few tens of microseconds on either side.

  (C) on objects, host clock (examples/map_fuse_harness `time`): MapOnDevice::SearchInNeighbors of the same target on an object graph of the
      same shape (its keyframes' observations placed where the points project, so that both passes fuse) against the reference's loop
      over lld_matcher_adapter, lld_landmark_adapter and lld_covisibility_adapter followed by MapOnDevice::UpdatePoints / UpdateKeyFrames,
      on two identical graphs loaded again before every repetition

NOT measured here: the kernels' own times, maps with thousands of keyframes.  Needs an MI355X.

  python tools/time_map_fuse.py [--reps 200] [--out profiles/map_fuse_time.json]"""
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
import map_ba_apply_ref as A  # noqa: E402
import map_fuse_ref as F  # noqa: E402
import map_fuse_scenes as FS  # noqa: E402
import map_refresh_scenes as RS  # noqa: E402
from lld_slam_amd import Context, abi, orb_search  # noqa: E402
from lld_slam_amd.device_map import DeviceMap  # noqa: E402


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


def rows_state(dm):
    n_pt, n_kf = dm.limits.max_points, dm.limits.max_keyframes
    return (dm.rows("point_obs", range(n_pt)), dm.rows("point_idx", range(n_pt)), dm.rows("kf_points", range(n_kf)), dm.point_counts(range(n_pt)).tolist(),
            {k: v.tobytes() for k, v in dm.download_points(range(n_pt)).items()})


def objects_case(a):
    """(C): examples/map_fuse_harness time on the object graph of the same shape"""
    import test_gpu_map_fuse_cpp as CPP
    m, c, _ = FS.random_scene(1, a.keypoints, a.candidates, n_other=30, objects=True, check=False)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.bin")
        with open(path, "wb") as f:
            f.write(CPP.object_scene(m, c, []))
        r = subprocess.run([os.path.join(ROOT, "examples", "map_fuse_harness"), "time", path, str(a.reps)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("map_fuse_harness time failed: " + r.stdout[-400:] + r.stderr)
    d = json.loads(r.stdout)
    assert d["fused_map"] == d["fused_adapter"], "the routes on objects disagree"
    qa, qb = quart(d["map_route_ms"]), quart(d["adapter_and_update_ms"])
    return dict(case="on objects, host clock: SearchInNeighbors, %d keypoints, 31 keyframes" % a.keypoints, fused=d["fused_map"], a_map_on_device_search_in_neighbors_ms=qa,
                b_adapters_then_update_ms=qb, met=verdict(qa, qb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--candidates", type=int, default=1500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m, c, slots = FS.random_scene(1, a.keypoints, a.candidates, n_other=30)
    m2, exp = FS.run_ref(m, c, slots)
    tg = c["target"]
    view = FS.view_struct(c["view"])
    # route B's inputs, flat, and the walk's outcome as the rows its setters send
    kf, mp = F.gathered(m, tg, slots)
    KF = orb_search.Frame(kf["desc"], kf["xy"], kf["octave"], kf["uright"], np.zeros(len(kf["octave"]), np.float32), 0.0, 0.0, FS.WIDTH, FS.HEIGHT,
                          FS.SCALE, (FS.SCALE * FS.SCALE).astype(np.float32), FS.INV_SIGMA2)
    P, P2, K, K2 = m["points"], m2["points"], m["keyframes"], m2["keyframes"]
    ch_pt = sorted(s for s in P if P[s]["obs"] != P2[s]["obs"] or P[s]["bad"] != P2[s]["bad"] or P[s]["n_obs"] != P2[s]["n_obs"])
    ch_kf = sorted(s for s in K if K[s]["points"] != K2[s]["points"])
    surv = [int(s) for s in exp["survivor"]]
    # route B's arrays, built ONCE here: numpy arrays and (start, flat) CSR pairs, so that the timed region packs no Python lists
    from lld_slam_amd.device_map import csr
    z3 = np.zeros(3, np.float32)
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    ch_pt_a = i32(ch_pt)
    pt_args = (ch_pt_a, np.array([P2[s]["pos"] for s in ch_pt], np.float32), np.array([P2[s].get("nrm", z3) for s in ch_pt], np.float32),
               np.array([P2[s]["mind"] for s in ch_pt], np.float32), np.array([P2[s]["maxd"] for s in ch_pt], np.float32),
               np.array([P[s]["desc"] for s in ch_pt], np.uint32), np.array([P2[s]["bad"] for s in ch_pt], np.uint8))
    obs_start, obs_kf = csr([[o[0] for o in P2[s]["obs"]] for s in ch_pt]); _, obs_idx = csr([[o[1] for o in P2[s]["obs"]] for s in ch_pt])
    obs_n = i32([P2[s]["n_obs"] for s in ch_pt])
    empty = (np.zeros(len(ch_kf) + 1, np.int32), np.zeros(1, np.int32))
    kf_args = (i32(ch_kf), np.array([K2[s]["key"] for s in ch_kf], np.uint64), np.array([K2[s]["bad"] for s in ch_kf], np.uint8), np.full(len(ch_kf), -1, np.int32),
               empty, empty, csr([K2[s]["points"] for s in ch_kf]), empty)
    surv_a, slots_a = i32(surv), i32(slots)
    res = {"reps": a.reps, "timer": "HIP events around the whole route, routes alternating in one process, the map cleared and sent again before every repetition",
           "bar": "route A's median below route B's by more than the larger interquartile range",
           "route_b": "lld_orb_fuse_search on flat inputs + the setters for the changed rows + lld_map_refresh_points for the survivors: a floor for the gathering route",
           "includes": "the Python wrappers' ctypes packing on both routes; route B's arrays are numpy arrays and CSR pairs built before the timed region",
           "not_measured": ["kernel-only times", "maps with thousands of keyframes"]}
    with Context(0) as ctx, DeviceMap(ctx, **FS.limits(m)) as dm:
        def reset():
            dm.clear(); RS.upload(dm, m)

        def route_a():
            return dm.fuse(tg, view, c["grid"], c["level_scale"], c["inv_sigma2"], point_slot=slots_a)

        def route_b():
            out, _ = orb_search.fuse_search_points(ctx.lib, ctx.handle, KF, view, mp, 3.0)
            dm.set_points(*pt_args)
            dm.set_observations_indexed(ch_pt_a, start=obs_start, kf_slot=obs_kf, kp_index=obs_idx, n_obs=obs_n)
            dm.set_keyframes(*kf_args)
            if surv:
                dm.refresh_points(surv_a, abi.LANDMARK_DESCRIPTOR)
            return out

        reset(); ga = route_a(); sa = rows_state(dm)
        reset(); gb = route_b(); sb = rows_state(dm)
        assert np.array_equal(ga["match"], gb.match) and np.array_equal(ga["match"], exp["match"]), "the routes disagree: match"
        assert np.array_equal(ga["action"], exp["action"]) and np.array_equal(ga["survivor"], exp["survivor"]), "lld_map_fuse against the restatement"
        assert sa == sb, "the routes leave different maps"
        assert sa[0] == A.rows_of(m2, "point_obs", range(dm.limits.max_points)), "the map against the restatement"
        for _ in range(3):
            reset(); route_a(); reset(); route_b()
        ta, tb, phases = [], [], []
        ph = np.zeros(4, np.float32)
        for _ in range(a.reps):
            reset(); ta.append(once(route_a))
            reset(); tb.append(once(route_b))
        for _ in range(min(a.reps, 50)):
            reset(); dm.fuse(tg, view, c["grid"], c["level_scale"], c["inv_sigma2"], point_slot=slots_a, phase_ms=ph); phases.append(ph.copy())
        qa, qb = quart(ta), quart(tb)
        res.update(case="one Fuse: %d keypoints x %d candidates, 31 keyframes" % (a.keypoints, a.candidates), n_fused=int(exp["n_fused"]), n_added=int(exp["n_added"]),
                   n_replaced=int(exp["n_replaced"]), n_survivors=len(surv), changed_point_rows=len(ch_pt), changed_keyframe_rows=len(ch_kf),
                   a_lld_map_fuse_ms=qa, b_fuse_search_setters_refresh_ms=qb, met=verdict(qa, qb),
                   a_phase_ms_median=dict(zip(("upload", "search", "walk_rows_refresh", "download"), np.median(np.array(phases), axis=0).round(4).tolist())))
    res["on_objects"] = objects_case(a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
