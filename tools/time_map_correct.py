"""Times the loop-closing thread's three map corrections on the device against the routes that existed before them.

  1, 2  flat arrays (examples/loop_correct_harness scene out REPS flat): ONE new call (lld_loop_correct / lld_essential_graph_apply /
        lld_global_ba_apply) against the reference's loop in compiled C++ on the same arrays with lld_mappoint_refresh for
        UpdateNormalAndDepth - one call per connected keyframe for CorrectLoop, one after the loop for the
        essential graph, none for the global BA.  HIP events on the context's stream around the whole window of either route; the
        routes alternate in one process; medians of --reps with interquartile ranges.  The harness compares what the two routes
        leave (positions, normals, depths, poses) bit for bit and fails otherwise.  The standing bar: the new median lies below the
        other route's by more than the larger interquartile range.
  3     the normal / depth kernels alone on the 100 000-point map, from a run of its own:
            rocprofv3 --kernel-trace --stats -d DIR -o nd -- python tools/time_map_correct.py --kernels
        runs lld_essential_graph_apply (mc_normal<8>, mc_normal<64>) and then lld_mappoint_refresh(NORMAL_DEPTH) on the positions and
        centres it returned (lm_normal_wave) --kernel-reps times each; --kernel-stats DIR reads the per-kernel totals into the result.
  4     the whole adapter call on objects, gather and scatter included (the harness without `flat`), against the reference's loops on
        a second copy of the objects; host clock around calls that end in a synchronise.  No bar is set for it.

Sizes: CorrectLoop on 31 connected keyframes x 1500 map points of a 7750-point map (the map of tools/time_covisibility.py); the other
two on 1000 keyframes and 100 000 points with about 600 000 observations.  Writes profiles/map_correct_time.json with --out.  Needs an MI355X."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loopcorr_ref as R  # noqa: E402
import loopcorr_scenes as S  # noqa: E402

HARNESS = os.path.join(ROOT, "examples", "loop_correct_harness")
NAMES = {1: "CorrectLoop", 2: "essential graph write-back", 3: "global BA map update"}


def scenes():
    rng = np.random.default_rng(0)
    return {1: S.make_loop_scene(0, n_kf=31, n_conn=31, cur_rank=30, per_kf=1500, s=0.9, n_points=7750, p_noobs=0.0),
            2: S.make_graph_scene(1, n_kf=1000, counts=rng.integers(2, 11, 100000)),
            3: S.make_gba_scene(2, n_chains=20, n_extra=960, n=100000)}


def kernels_worker(reps):
    """Item 3, to be run under rocprofv3: the packed kernels and lm_normal_wave on the same map, positions and centres."""
    from lld_slam_amd import Context, landmarks, loop_correction as LC
    sc = scenes()[2]
    with Context(0) as ctx:
        for _ in range(reps):
            got = LC.apply_essential_graph(ctx, *[sc[k] for k in ("sim3_before", "sim3_after", "corr_kf", "pos", "bad", "obs_start", "obs_kf", "ref_kf",
                                                                   "ref_level", "level_scale")])
        for _ in range(reps):
            one = landmarks.refresh_map_points(ctx, sc["obs_start"], sc["obs_kf"], sc["bad"], kf_ow=got.ow, pos=got.pos, ref_kf=sc["ref_kf"],
                                               ref_level=sc["ref_level"], level_scale=sc["level_scale"], flags=landmarks.NORMAL_DEPTH)
    assert R.bits_equal(one.normal, got.normal) and R.bits_equal(one.min_distance, got.min_distance) and R.bits_equal(one.max_distance, got.max_distance)
    counts = np.diff(sc["obs_start"])
    print(json.dumps(dict(points=len(counts), observations=int(counts.sum()), points_up_to_8=int(((counts > 0) & (counts <= 8)).sum()),
                          points_above_8=int((counts > 8).sum()), outputs_bit_equal=True)))


def kernel_stats(d):
    """Per-call averages of the three kernels from the rocprofv3 run under d: its *_kernel_stats.csv, or its rocpd database through
    tools/rocpd_summary.py where the profiler writes only that."""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        rows += [(r.get("Name", ""), int(r["Calls"]), float(r["AverageNs"]) / 1e3) for r in csv.DictReader(open(path))]
    if not rows:
        for path in glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True):
            text = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocpd_summary.py"), path], capture_output=True, text=True).stdout
            for line in text.split("\n"):
                f = line.split()
                if len(f) >= 7 and ("mc_normal" in line or "lm_normal_wave" in line):
                    rows.append((" ".join(f[:-6]), int(f[-6]), float(f[-4])))          # name, calls, total_ms, avg_us, min_us, max_us, pct
    res = {}
    for name, calls, avg_us in rows:
        if "lm_normal_wave" in name:
            res["lm_normal_wave"] = dict(calls=calls, average_us=avg_us)
        elif "mc_normal" in name:
            res["mc_normal<8>" if ("Li8E" in name or "<8>" in name) else "mc_normal<64>"] = dict(calls=calls, average_us=avg_us)
    if len(res) == 3:
        res["packed_us_per_map"] = round(res["mc_normal<8>"]["average_us"] + res["mc_normal<64>"]["average_us"], 2)
        res["lm_normal_wave_us_per_map"] = res["lm_normal_wave"]["average_us"]
    return res


def objects_agree(adapter, host):
    for k in ("corrected_by", "corrected_ref", "kf_gba_mark", "n_set_pos", "n_set_pose"):
        assert np.array_equal(adapter[k], host[k]), k
    for k in ("tcw", "pos", "ow", "normal", "min_distance", "max_distance", "tcw_gba", "tcw_before"):
        assert R.ulp_steps(adapter[k], host[k]).max() <= 1, k
    return {k: int((R.ulp_steps(adapter[k], host[k]) > 0).sum()) for k in ("tcw", "pos", "normal")}


def harness(args):
    run = subprocess.run([HARNESS] + args, capture_output=True, text=True, timeout=1500)
    if run.returncode != 0:
        raise SystemExit(run.stdout + run.stderr)
    return json.loads(run.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--kernels", action="store_true", help="run item 3's calls in this process (under rocprofv3)")
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None, help="directory of the rocprofv3 run of --kernels")
    ap.add_argument("--out", default=None)
    ap.add_argument("--add-kernel-stats-to", default=None, help="an earlier --out file: only add --kernel-stats to it (needs no GPU)")
    a = ap.parse_args()
    if a.kernels:
        return kernels_worker(a.kernel_reps)
    if a.add_kernel_stats_to:
        res = json.load(open(a.add_kernel_stats_to))
        res["normal_depth_kernels"] = dict(source="rocprofv3 --kernel-trace --stats, a run of its own on the 100 000-point map", **kernel_stats(a.kernel_stats))
        json.dump(res, open(a.out or a.add_kernel_stats_to, "w"), indent=1)
        return print(json.dumps(res["normal_depth_kernels"]))
    res = {"reps": a.reps, "bar": "new median below the other route's by more than the larger interquartile range (flat arrays)", "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        for kind, sc in scenes().items():
            blob, eff = S.object_scene_blob(kind, sc)
            path, out = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "out.bin")
            with open(path, "wb") as f:
                f.write(blob)
            flat = harness([path, out, str(a.reps), "flat"])
            flat["bar_met"] = bool(flat["previous_route_ms"] - flat["one_call_ms"] > max(flat["one_call_iqr_ms"], flat["previous_route_iqr_ms"]))
            objs = harness([path, out, str(a.reps)])
            adapter, host = S.read_object_dump(out)
            case = dict(name=NAMES[kind], n_kf=flat["n_kf"], n_points=flat["n_points"], observations=int(len(eff["obs_kf"])), flat_arrays=flat,
                        objects=dict(timer="host clock around calls that end in a stream synchronise", values_not_bit_equal=objects_agree(adapter, host),
                                     **{k: objs[k] for k in ("adapter_ms", "adapter_iqr_ms", "host_ms", "host_iqr_ms")}))
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    if a.kernel_stats:
        res["normal_depth_kernels"] = dict(source="rocprofv3 --kernel-trace --stats, a run of its own on the 100 000-point map", **kernel_stats(a.kernel_stats))
        print(json.dumps(res["normal_depth_kernels"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
