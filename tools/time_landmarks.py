"""HIP-event medians of the landmark refresh on the device (lld_mappoint_refresh), upload and download included:
  * one SearchInNeighbors-sized refresh: 2000 MapPoints with 2-40 observations over 30 keyframes, both parts;
  * one LocalBundleAdjustment-tail refresh: 5000 MapPoints, normal / depth only.
With --cpu the same two are also timed through tests/landmark_ref.py (numpy, one landmark at a time; NOT the reference's C++).
Writes profiles/landmark_time.json when --out is given.  Needs an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import landmark_ref as L  # noqa: E402
from lld_slam_amd import Context  # noqa: E402
from lld_slam_amd.landmarks import DESCRIPTOR, NORMAL_DEPTH, refresh_map_points  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--cpu", action="store_true", help="also time tests/landmark_ref.py (numpy, not the reference)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"reps": a.reps, "timer": "HIP events around the call, upload and download included, median", "cases": []}
    with Context(0) as ctx:
        for name, n, flags in (("SearchInNeighbors", 2000, DESCRIPTOR | NORMAL_DEPTH), ("LocalBundleAdjustment tail", 5000, NORMAL_DEPTH)):
            counts = np.minimum(np.random.default_rng(n).integers(2, 41, n), 30)     # 2-40 observations, at most one per keyframe
            sc = L.make_point_scene(100 + n, n_kf=30, counts=counts, p_bad=0.02, p_all_bad=0.0)

            def call():
                return refresh_map_points(ctx, sc["obs_start"], sc["obs_kf"], sc["bad"], obs_desc=sc["obs_desc"], kf_bad=sc["kf_bad"],
                                          kf_ow=sc["kf_ow"], pos=sc["pos"], ref_kf=sc["ref_kf"], ref_level=sc["ref_level"],
                                          level_scale=sc["level_scale"], flags=flags)
            out = call()
            timed(call, 5)
            med, mn = timed(call, a.reps)
            case = {"case": name, "points": n, "observations": int(len(sc["obs_kf"])), "keyframes": int(len(sc["kf_bad"])), "flags": flags,
                    "written": int(np.sum(out.updated != 0)), "ms_median": med, "ms_min": mn}
            if a.cpu:
                t = time.perf_counter()
                L.refresh_map_points_ref(sc, flags)
                case["numpy_restatement_ms"] = (time.perf_counter() - t) * 1e3
            res["cases"].append(case)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
