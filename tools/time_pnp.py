"""HIP-event medians of Tracking::Relocalization's PnP step on the device (lld_pnp_*): one relocalisation of 20 candidates with
30-400 matches (create, then iterate(5) rounds over the live candidates until every one has bNoMore), and one candidate's find().
Writes profiles/pnp_time.json when --out is given.  Needs an MI355X."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_ref as P  # noqa: E402
from lld_slam_amd import Context  # noqa: E402
from lld_slam_amd.pnp import PnPsolver, PnPsolverBatch  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    scenes = [P.make_scene(100 + i, int(rng.integers(30, 401)), float(rng.choice([0.3, 0.6, 0.9]))) for i in range(20)]
    res = {"candidates": 20, "matches": [int(len(s["xyz"])) for s in scenes], "reps": a.reps}
    with Context(0) as ctx:
        rounds = []

        def relocalise():
            with PnPsolverBatch(ctx, scenes) as b:
                live = np.ones(20, bool)
                k = 0
                while live.any():
                    outs = b.iterate(5, live)
                    live &= ~np.array([o.no_more for o in outs])
                    k += 1
                rounds.append(k)

        timed(relocalise, 3)
        res["relocalisation_ms_median"], res["relocalisation_ms_min"] = timed(relocalise, a.reps)
        res["rounds"] = int(np.median(rounds))

        def find_one():
            with PnPsolver(ctx, scenes[0]) as s:
                s.find()

        timed(find_one, 3)
        res["find_ms_median"], res["find_ms_min"] = timed(find_one, a.reps)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
