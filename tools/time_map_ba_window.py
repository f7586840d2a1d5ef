"""Times the local BA window assembled on the resident map (lld_map_ba_window, lld_map_local_ba) against the walk over objects it replaces, on
one MI355X, on one object graph of LBA-B size (synth.make_lba_b: 60 keyframes of which 50 are free, 10 000 points with six observations
each, 2 000 lines with five).
  (a) assembly, objects: examples/map_ba_harness `time` with the stop flag raised, so that both routes return before solving -
      MapOnDevice::LocalBundleAdjustment (one lld_map_local_ba call: slot list up, window down) against the gather of
      adapters/lld_optimizer_adapter.cc:32-151 on an identical copy of the graph.  Host clock, the two routes alternating in one process.
  (b) the whole call, objects: the same with the flag lowered - solve, erase lists, write-back, and on the map route the push-back of what
      changed (poses, points, lines, the keyframes that lost a match).
  (c) flat tables: lld_map_ba_window alone on a DeviceMap holding the same window as a map; HIP events for upload, kernels and download
      (phase_ms) and the host clock around the call.
Medians of --reps with quartiles.  `met` for (a) and (b): the map route's median is below the host route's by more than the larger
interquartile range.  Writes the JSON to --out; --problem-out keeps the harness input (for a profiler run of the harness)."""
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

HARNESS = os.path.join(ROOT, "examples", "map_ba_harness")


def quart(v):
    v = np.sort(np.asarray(v, np.float64))
    return dict(median=round(float(v[len(v) // 2]), 4), q1=round(float(v[len(v) // 4]), 4), q3=round(float(v[(3 * len(v)) // 4]), 4))


def verdict(new, old):
    iqr = max(new["q3"] - new["q1"], old["q3"] - old["q1"])
    return bool(new["median"] < old["median"] - iqr)


def objects(w, reps, problem_out):
    from test_cpp_adapter import _as_dict
    from test_cpp_harness import write_ba
    with tempfile.TemporaryDirectory() as tmp:
        path = problem_out or os.path.join(tmp, "lba_b.bin")
        write_ba(path, _as_dict(w))
        r = subprocess.run([HARNESS, "time", path, str(reps)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("map_ba_harness time failed: " + r.stderr)
    d = json.loads(r.stdout)
    out = {k: d[k] for k in ("n_cams", "n_free_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs", "graph_differences")}
    for case, name in (("assembly", "a_assembly_stop_flag_raised"), ("whole", "b_whole_call")):
        host, dev = quart(d[case + "_host_ms"]), quart(d[case + "_map_ms"])
        out[name] = dict(map_route_ms=dev, host_adapter_ms=host, met=verdict(dev, host))
    return out


def flat_tables(w, reps):
    import map_ba_scenes as S
    from lld_slam_amd import Context
    from lld_slam_amd.device_map import DeviceMap
    m, q, table = S.map_of_window(w, 1)
    with Context(0) as ctx, DeviceMap(ctx, **S.limits_for(m)) as dm:
        S.upload(dm, m)
        first = dm.ba_window(q, w.cam, table)
        caps = [first[c] for c in DeviceMap.BA_COUNTS]
        ph = np.zeros(3, np.float32)
        ev, wall = [], []
        for r in range(-5, reps):
            t0 = time.perf_counter()
            got = dm.ba_window(q, w.cam, table, capacities=caps, phase_ms=ph)
            t1 = time.perf_counter()
            if r >= 0:
                ev.append(ph.copy()); wall.append((t1 - t0) * 1e3)
        assert got["status"] == 0 and all(got[c] == first[c] for c in DeviceMap.BA_COUNTS)
        ev = np.array(ev)
        return dict(counts={c: int(first[c]) for c in ("n_cams", "n_free_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs")}, upload_events_ms=quart(ev[:, 0]),
                    kernels_events_ms=quart(ev[:, 1]), download_events_ms=quart(ev[:, 2]), events_total_ms=quart(ev.sum(1)),
                    wall_ms_with_the_python_wrapper=quart(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_ba_window_time.json"))
    ap.add_argument("--problem-out", default=None)
    ap.add_argument("--skip-flat", action="store_true")
    a = ap.parse_args()
    from lld_slam_amd import synth
    w = synth.make_lba_b(0)
    res = dict(reps=a.reps, window="synth.make_lba_b(0)", bar="map route's median below the host route's by more than the larger interquartile range")
    res["objects_host_clock"] = objects(w, a.reps, a.problem_out)
    if not a.skip_flat:
        res["c_flat_tables"] = flat_tables(w, a.reps)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
