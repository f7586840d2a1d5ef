"""HIP-event medians of lld_new_points_triangulate on the device, upload and download included:
  * one call for 10 pairs x 300 matches (a whole CreateNewMapPoints in stereo mode);
  * one call for 1 pair x 300 matches (the unit adapters/ would use, one neighbour at a time).
These are end-to-end figures of the Python call, not device intervals: the two events are recorded on torch's current stream while
the work runs on the context's own stream, which the call synchronises before it returns, so an interval is close to the host wall
time of the call - the ctypes packing of up to 11 keyframe records, the host-side validation and gather, the transfers and the two
kernels together.  With --cpu the same two are also timed through
tests/newpoints_ref.py (numpy; NOT the reference's C++).  Writes profiles/new_points_time.json when --out is given.  Needs an MI355X."""
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
import newpoints_ref as R  # noqa: E402
from lld_slam_amd import Context  # noqa: E402
from lld_slam_amd.new_points import triangulate_new_points  # noqa: E402


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
    ap.add_argument("--cpu", action="store_true", help="also time tests/newpoints_ref.py (numpy, not the reference)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"reps": a.reps, "timer": "HIP events around the call, upload and download included, median", "cases": []}
    with Context(0) as ctx:
        for name, nm in (("10 pairs x 300 matches", [300] * 10), ("1 pair x 300 matches", [300])):
            pb = R.make_scene(31, nm)

            def call():
                return triangulate_new_points(ctx, pb["kf1"], pb["keys1"], pb["kf2"], pb["key_start"], pb["keys2"], pb["match_start"],
                                              pb["matches"], monocular=pb["monocular"])
            out = call()
            timed(call, 20)
            med, mn = timed(call, a.reps)
            case = {"case": name, "pairs": len(nm), "matches": int(len(pb["matches"])), "new": out.n_new_total, "ms_median": med, "ms_min": mn}
            if a.cpu:
                t = time.perf_counter()
                R.triangulate(pb)
                case["numpy_restatement_ms"] = (time.perf_counter() - t) * 1e3
            res["cases"].append(case)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
