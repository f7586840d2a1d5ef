"""HIP-event medians of LoopClosing::ComputeSim3's Sim3Solver step on the device (lld_sim3solver_*): one loop closing of 5
candidates with 20-600 matches (create, then iterate(5) rounds over the live candidates until one returns a pose or every one has
bNoMore), and one candidate's find().  Writes profiles/sim3solver_time.json when --out is given.  Needs an MI355X."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3solver_ref as S  # noqa: E402
from lld_slam_amd import Context  # noqa: E402
from lld_slam_amd.sim3solver import Sim3Solver, Sim3SolverBatch  # noqa: E402


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
    # the true loop is the last candidate: the four before it (wrong places, few consistent matches) run their budgets first
    ratios = [0.05, 0.08, 0.1, 0.12, 0.25]
    scenes = [S.make_scene(100 + i, int(rng.integers(20, 601)), ratios[i]) for i in range(5)]
    res = {"candidates": 5, "matches": [int(len(s["index1"])) for s in scenes], "inlier_ratio": ratios, "reps": a.reps}
    with Context(0) as ctx:
        rounds = []

        def loop_closing():
            with Sim3SolverBatch(ctx, scenes) as b:
                live = np.ones(len(scenes), bool)
                k = 0
                while live.any():
                    outs = b.iterate(5, live)
                    k += 1
                    if any(o.T12 is not None for o in outs):
                        break
                    live &= ~np.array([o.no_more for o in outs])
                rounds.append(k)

        timed(loop_closing, 3)
        res["loop_closing_ms_median"], res["loop_closing_ms_min"] = timed(loop_closing, a.reps)
        res["rounds"] = int(np.median(rounds))
        res["round_ms_median"] = res["loop_closing_ms_median"] / max(res["rounds"], 1)

        def find_one():
            with Sim3Solver(ctx, scenes[0]) as s:
                s.find()

        timed(find_one, 3)
        res["find_ms_median"], res["find_ms_min"] = timed(find_one, a.reps)
        res["find_matches"] = res["matches"][0]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
