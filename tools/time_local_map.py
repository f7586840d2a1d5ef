"""Times one frame of the Tracking chain with Tracking::UpdateLocalMap between its stages, two ways on the SAME library, on README's chain shape
(2000 keypoints, 1200 last-frame points, a map of 40 keyframes, about 2500 local points and 260 local lines):
  A  the route through the host, the only one the library offered before: stage 1 -> lld_frame_track_download -> the two loops of UpdateLocalMap in
     compiled C++ on flat tables (examples/local_map_host.cpp, built here as a shared object) -> the local points and lines gathered out of flat
     arrays (numpy take) -> lld_frame_track_local_map -> lld_frame_track_download;
  B  the resident map: stage 1 -> lld_frame_track_update_local_map -> lld_frame_track_local_map_resident -> lld_frame_local_map_download (lists
     included).
Route A on flat tables is a floor for a real caller, which gathers out of objects on top.  Both routes are driven through the Python wrappers,
so part of what separates them is Python: route A builds the dicts of two downloads and takes its arrays with numpy, route B builds one download's.
A kernel trace is a run of its own (see --only and --merge-trace).
Each frame is bracketed by the host clock - route A's cost is host work and a synchronisation - and by two HIP events on the context's stream.
Medians and quartiles of --reps frames after --warmup; the routes alternate in blocks of 20 so that a drift of the machine meets both.
Bar: B's host-clock median below A's by more than the larger interquartile range, and both routes return the same integers (asserted).
Writes profiles/local_map_time.json when --out is given.  Needs an MI355X."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KF = 40


def quartiles(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(median_ms=float(med), q1_ms=float(q1), q3_ms=float(q3), iqr_ms=float(q3 - q1), min_ms=float(a[0]))


def host_loops():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "liblocal_map_host.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "examples", "local_map_host.cpp"), "-o", so])
    return C.CDLL(so)


class Tables(C.Structure):
    _fields_ = [("n_keyframes", C.c_int), ("n_points", C.c_int), ("n_lines", C.c_int), ("kf_key", C.c_void_p), ("kf_bad", C.c_void_p), ("kf_parent", C.c_void_p)] + \
               [(k, C.c_void_p) for k in ("cov_start", "cov", "child_start", "child", "point_start", "point", "line_start", "line", "pt_state", "obs_start", "obs", "ln_bad")]


def flat_tables(SC, m, L):
    keep = SC.flat_tables(m, L)
    T = Tables(L["max_keyframes"], L["max_points"], L["max_lines"])
    for k, v in keep.items():
        setattr(T, k, v.ctypes.data)
    return T, keep


def merge_trace(record_path, db_path):
    """Adds the medians of the map_* kernels of a rocprofv3 kernel trace (its sqlite database) to an existing record as "kernel_trace"."""
    import re
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, duration from kernels").fetchall()
    by = {}
    for name, ns in rows:
        k = re.search(r"(map_[A-Za-z_0-9]+_kernel)", name)
        if k: by.setdefault(k.group(1), []).append(ns)
    with open(record_path) as f:
        rec = json.load(f)
    rec["kernel_trace"] = dict(tool="rocprofv3 --kernel-trace --stats -d DIR -o lm -- python tools/time_local_map.py --only B_resident --reps 60 --warmup 20, "
                                    "then tools/time_local_map.py --merge-trace DIR/lm_results.db --out RECORD",
                               kernels={k: dict(calls=len(v), median_us=round(float(np.median(v)) / 1e3, 2)) for k, v in sorted(by.items())})
    with open(record_path, "w") as f:
        json.dump(rec, f, indent=1); f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("A_host", "B_resident"), default=None, help="time one route alone (for a kernel trace of its own)")
    ap.add_argument("--merge-trace", default=None, metavar="DB", help="no timing: merge the kernel medians of this rocprofv3 database into the record at --out")
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.out, a.merge_trace)
    import local_map_scenes as SC
    CH = SC
    from lld_slam_amd import Context, abi, synth
    from lld_slam_amd.abi import c_int32_p
    from lld_slam_amd.device_map import DeviceMap
    from lld_slam_amd.tracking import DeviceTrackedFrame
    sc = CH.as_slots(synth.make_tracking_scene(0))
    hl = host_loops().local_map_host_update
    hl.restype = None
    hl.argtypes = [C.POINTER(Tables), c_int32_p, c_int32_p, c_int32_p, C.c_int, C.c_int, C.c_int, c_int32_p, c_int32_p, c_int32_p, c_int32_p]
    res = {"reps": a.reps, "warmup": a.warmup, "library": os.path.relpath(abi.product_library_path(), ROOT),
           "timer": "the host clock around the whole frame; HIP events on the context's stream around the same calls alongside"}
    with Context(0) as ctx:
        lib = ctx.lib
        hip = C.CDLL("libamdhip64.so")
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]; hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]; hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        stream = C.c_void_p(lib.fn("ctx_stream")(ctx.handle))
        stage1 = lambda tf_: tf_.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc.get("last_lines"))
        with DeviceTrackedFrame(ctx, sc["frame"], sc["cam"], sc["lines"]) as tf0:
            stage1(tf0)
            r1 = tf0.download(stage2=False)[0]
        m = CH.make_map(sc, np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]), 0, n_kf=N_KF)
        L = CH.tracking_limits(sc, m, n_kf=N_KF, max_local_points=3072, max_local_lines=320)
        T, keep = flat_tables(SC, m, L)
        mp = {k: np.ascontiguousarray(sc["map_points"][k]) for k in ("world_pos", "normal", "min_distance", "max_distance", "desc")}
        has_obs = (keep["obs_start"][1:] > keep["obs_start"][:-1]).astype(np.uint8)
        ld = CH.line_data(sc)
        lt = {k: np.ascontiguousarray(np.array([ld[s][k] for s in range(len(ld))])) for k in ("X0", "dir", "X1", "X2", "desc")}
        nt = sc["frame"].n
        lst = np.zeros(abi.MAP_MAX_LOCAL_KEYFRAMES, np.int32); n_lst = np.zeros(1, np.int32); scal = np.zeros(5, np.int32)
        lp = np.zeros(L["max_local_points"], np.int32); ll = np.zeros(L["max_local_lines"], np.int32); n_loc = np.zeros(2, np.int32)
        p32 = lambda v: v.ctypes.data_as(c_int32_p)
        with DeviceMap(ctx, **L) as dm, DeviceTrackedFrame(ctx, sc["frame"], sc["cam"], sc["lines"]) as tf:
            SC.upload(dm, m, CH.point_data(sc), ld, dim=L["line_dim"])

            def route_a():
                stage1(tf)
                g1 = tf.download(stage2=False)[0]
                ids = np.where(g1["kp_outlier"] != 0, -1, g1["kp_point_id"]).astype(np.int32)
                hl(C.byref(T), p32(lst), p32(n_lst), p32(ids), nt, L["max_local_points"], L["max_local_lines"], p32(scal), p32(lp), p32(ll), p32(n_loc))
                pts_i, lns_i = lp[:n_loc[0]], ll[:n_loc[1]]
                pts = {k: v[pts_i] for k, v in mp.items()}; pts["has_obs"] = has_obs[pts_i]
                lines = {k: v[lns_i] for k, v in lt.items()}; lines["id"] = lns_i
                tf.track_local_map(pts, pts_i, lines)
                s1, s2 = tf.download()
                return dict(stages=[s1, s2], local_keyframes=lst[:n_lst[0]].copy(), local_points=pts_i.copy(), local_lines=lns_i.copy(), ref_keyframe=int(scal[3]))

            def route_b():
                stage1(tf)
                tf.update_local_map(dm)
                tf.track_local_map_resident(dm)
                return tf.local_map_download(dm)
            routes = {k: v for k, v in (("A_host", route_a), ("B_resident", route_b)) if a.only in (None, k)}
            ra, rb = route_a(), route_b()
            n = len(ra["local_points"])
            for k in ("local_keyframes", "local_points", "local_lines"):
                assert ra[k].tolist() == rb[k].tolist(), k
            assert ra["ref_keyframe"] == rb["ref_keyframe"] and rb["status"] == 0 and rb["stage2_ran"] == 1
            for s in range(2):
                CH.same_dict(rb["stages"][s], ra["stages"][s], "stage %d" % (s + 1), skip=("mp_in_view",))
            np.testing.assert_array_equal(rb["stages"][1]["mp_in_view"][:n], ra["stages"][1]["mp_in_view"])
            res["shape"] = dict(keypoints=nt, last_points=int(len(sc["last_ids"])), keyframes=N_KF, local_keyframes=len(ra["local_keyframes"]), local_points=n,
                                local_lines=len(ra["local_lines"]), max_local_points=L["max_local_points"], max_local_lines=L["max_local_lines"],
                                stage2_inliers=ra["stages"][1]["n_inliers"])
            wall = {k: [] for k in routes}; dev = {k: [] for k in routes}
            done = 0
            while done < a.warmup + a.reps:
                for name, fn in routes.items():
                    for i in range(20):
                        assert hip.hipEventRecord(e0, stream) == 0
                        t0 = time.perf_counter()
                        fn()
                        t1 = time.perf_counter()
                        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
                        ms = C.c_float()
                        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                        if done + i >= a.warmup:
                            wall[name].append((t1 - t0) * 1e3); dev[name].append(float(ms.value))
                done += 20
            for name in routes:
                res[name] = dict(host_wall=quartiles(wall[name][:a.reps]), hip_events=quartiles(dev[name][:a.reps]))
    if a.only:
        print(json.dumps(res, indent=1))
        return
    A, B = res["A_host"]["host_wall"], res["B_resident"]["host_wall"]
    iqr = max(A["iqr_ms"], B["iqr_ms"])
    res["bar"] = dict(rule="B's host-clock median below A's by more than the larger interquartile range; same integers asserted before timing",
                      gain_ms=A["median_ms"] - B["median_ms"], larger_iqr_ms=iqr, met=bool(A["median_ms"] - B["median_ms"] > iqr))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
