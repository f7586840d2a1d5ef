"""Times "extractor output -> resident frame ready for lld_frame_track_motion_model" on the KITTI-sized pair of
synth.make_stereo_scene(0), after one lld_orb_extract, two ways:
  * parent route  the host results of lld_orb_extract -> lld_compute_stereo_matches (device pyramids) -> lld_frame_create, on a library
                  built from the parent commit (--parent-lib, loaded through LLD_AMD_LIB in a child process of its own);
  * new call      lld_frame_build_stereo followed by a stream synchronisation, as host wall time and as HIP-event time.
Every struct is filled before the timed window, so both windows hold only the C calls.  Medians and quartiles of --reps calls after
--warmup calls; each route runs in a fresh child process.  --kernel-stats DIR (optional) adds the Hamming stage alone from rocprofv3
--kernel-trace --stats runs of the two workers made beforehand (DIR/parent, DIR/new): orb_search_kernel against stereo_rows_kernel.
Writes profiles/frame_build_time.json when --out is given.  Needs an MI355X."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KITTI = (2000, 1.2, 8, 12, 7)


def quartiles(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(median_ms=float(med), q1_ms=float(q1), q3_ms=float(q3), iqr_ms=float(q3 - q1), min_ms=float(a[0]))


def worker(route, reps, warmup):
    import orb_extract_ref as R
    from lld_slam_amd import Context, abi, orb_search, synth
    from lld_slam_amd.abi import c_float_p, c_int32_p
    from lld_slam_amd.orb_extractor import ORBextractor
    sc = synth.make_stereo_scene(0)
    out = {"route": route, "library": abi.product_library_path()}
    with Context(0) as ctx, ORBextractor(ctx, *KITTI, R.seeded_pattern(7), max_cols=1241, max_rows=376, max_images=2) as ex:
        lib = ctx.lib
        L, Rf = ex([sc["left"][0], sc["right"][0]])
        out["n_left"], out["n_right"] = L.n, Rf.n
        sync = lib.fn("ctx_synchronize")
        destroy = lib.fn("frame_destroy"); destroy.argtypes = [C.c_void_p]; destroy.restype = None
        wall, dev = [], []
        if route == "parent":
            kl, kr = orb_search.keypoints_struct(L), orb_search.keypoints_struct(Rf)
            P, keep = ex.stereo_pyramids(0, 1)
            ur = np.empty(L.n, np.float32); dep = np.empty(L.n, np.float32)
            r = orb_search.StereoResult(); r.u_right = ur.ctypes.data_as(c_float_p); r.depth = dep.ctypes.data_as(c_float_p)
            csm = lib.fn("compute_stereo_matches")
            csm.argtypes = [C.c_void_p, C.POINTER(orb_search.Keypoints), C.POINTER(orb_search.Keypoints), C.POINTER(orb_search.StereoPyramids), C.c_float,
                            C.c_float, C.POINTER(orb_search.StereoResult)]
            csm.restype = C.c_int
            L.uright = ur                                                       # lld_frame_create reads what lld_compute_stereo_matches wrote
            prep = orb_search.prepare(L, np.zeros((0, 8), np.uint32), candidates=orb_search.CAND_GRID, accept_max=orb_search.TH_HIGH)
            assert prep.s.t_uright and C.addressof(prep.s.t_uright.contents) == ur.ctypes.data
            create = lib.fn("frame_create"); create.argtypes = [C.c_void_p, C.POINTER(orb_search.OrbSearch), C.POINTER(C.c_void_p)]; create.restype = C.c_int
            mb, mbf = float(np.float32(sc["mb"])), float(np.float32(sc["mbf"]))
            for it in range(warmup + reps):
                h = C.c_void_p()
                t0 = time.perf_counter()
                st = csm(ctx.handle, C.byref(kl), C.byref(kr), C.byref(P), mb, mbf, C.byref(r))
                st |= create(ctx.handle, C.byref(prep.s), C.byref(h))          # (synchronises itself)
                t1 = time.perf_counter()
                assert st == 0
                destroy(h)
                if it >= warmup: wall.append((t1 - t0) * 1e3)
            out["n_matches"] = int(r.n_matches)
        else:
            hip = C.CDLL("libamdhip64.so")
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]; hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            hip.hipEventSynchronize.argtypes = [C.c_void_p]; hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            e0, e1 = C.c_void_p(), C.c_void_p()
            assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
            stream = C.c_void_p(lib.fn("ctx_stream")(ctx.handle))
            prm, keep = orb_search.frame_stereo_params(L, sc["mb"], sc["mbf"])
            build = lib.fn("frame_build_stereo")
            build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.FrameStereoParams), C.POINTER(C.c_void_p)]; build.restype = C.c_int
            h = C.c_void_p()
            for it in range(warmup + reps):
                assert hip.hipEventRecord(e0, stream) == 0
                t0 = time.perf_counter()
                st = build(ex.handle, 0, 1, C.byref(prm), C.byref(h))
                st |= sync(ctx.handle)
                t1 = time.perf_counter()
                assert st == 0 and hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
                ms = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                if it < warmup + reps - 1: destroy(h)
                if it >= warmup: wall.append((t1 - t0) * 1e3); dev.append(float(ms.value))
            built = orb_search.StereoBuiltFrame(lib, ctx.handle, L, h)
            out["n_matches"] = int(built.download().n_matches)
            built.close()
            out["hip_events"] = quartiles(dev)
        out["host_wall"] = quartiles(wall)
    print("RESULT " + json.dumps(out))


def kernel_stats(d, names):
    """Per-call average and calls of the named kernels from the *_kernel_stats.csv files under d."""
    res = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for n in names:
                if n in row.get("Name", ""):
                    res[n] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, total_us=float(row["TotalDurationNs"]) / 1e3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--route", choices=("parent", "new"), default=None, help="run one route in this process (used by the driver and under rocprofv3)")
    ap.add_argument("--parent-lib", default=os.environ.get("LLD_AMD_PARENT_LIB"))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.route:
        return worker(a.route, a.reps, a.warmup)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: a liblld_amd.so built from the parent commit is needed")
    res = {"workload": "synth.make_stereo_scene(0), 1241x376, ORBextractor(2000, 1.2, 8, 12, 7), after one lld_orb_extract", "reps": a.reps, "warmup": a.warmup,
           "timer": "host clock around the C calls (each window ends in a synchronisation); HIP events on the context's stream for the new call"}
    for route in ("parent", "new"):
        env = dict(os.environ)
        if route == "parent":
            env["LLD_AMD_LIB"] = a.parent_lib
        else:
            env.pop("LLD_AMD_LIB", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                             capture_output=True, text=True, timeout=900, env=env)
        if out.returncode != 0:
            raise SystemExit(out.stdout + out.stderr)
        res[route] = json.loads([l for l in out.stdout.split("\n") if l.startswith("RESULT ")][-1][7:])
    p, n = res["parent"]["host_wall"], res["new"]["host_wall"]
    assert res["parent"]["n_matches"] == res["new"]["n_matches"], "the two routes disagree"
    spread = max(p["iqr_ms"], n["iqr_ms"])
    res["bar"] = dict(rule="new median below the parent median by more than the larger interquartile range", larger_iqr_ms=spread,
                      difference_ms=p["median_ms"] - n["median_ms"], met=bool(p["median_ms"] - n["median_ms"] > spread))
    if a.kernel_stats:
        res["hamming_stage"] = dict(source="rocprofv3 --kernel-trace --stats, one run per route",
                                    parent=kernel_stats(os.path.join(a.kernel_stats, "parent"), ["orb_search_kernel"]),
                                    new=kernel_stats(os.path.join(a.kernel_stats, "new"), ["stereo_rows_kernel"]))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
