"""HIP-event medians of Initializer::Initialize on the device (lld_initializer_initialize) for about 500 and 2000 matches at 200
iterations, on a handle that already exists (the reference frame is uploaded once, as in Tracking::MonocularInitialization).
Writes profiles/initializer_time.json when --out is given.  Needs an MI355X."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import initializer_ref as I  # noqa: E402
from lld_slam_amd import Context  # noqa: E402
from lld_slam_amd.initializer import Initializer, problem_from_scene  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"iterations": 200, "reps": a.reps, "cases": []}
    with Context(0) as ctx:
        for n in (500, 2000):
            sc = I.make_scene(400 + n, n, 0.8)
            K, k1, k2, m = problem_from_scene(sc)
            with Initializer(ctx, K, k1, seed=sc["seed"]) as ini:
                out = ini.Initialize(k2, m)
                timed(lambda: ini.Initialize(k2, m), 3)
                med, mn = timed(lambda: ini.Initialize(k2, m), a.reps)
            res["cases"].append({"matches": n, "keypoints": int(len(k1)), "success": bool(out.success), "model": int(out.model),
                                 "initialize_ms_median": med, "initialize_ms_min": mn})
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
