"""Times the covisibility counting on the device against the same loops on the host (examples/covisibility_harness --time):
  * one batched UpdateConnections over the local keyframes of one map (30 keyframes of about 1500 map points each);
  * one KeyFrameCulling over the same keyframes (a scene in which nothing is culled, so that one device call does it);
  * UpdateConnections for a single keyframe of the same map.
The device figures are HIP-event times of the upload, the kernels and the download inside lld_covisibility; adapter_ms is the
host clock around the whole adapter call (gather, device call, apply), host_loop_ms the host clock around the plain std::map loops
on the same objects in the same process.  Medians of --reps, after a warm-up call.  Writes profiles/covisibility_time.json when
--out is given.  Needs an MI355X."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import covis_scenes as S  # noqa: E402

HARNESS = os.path.join(ROOT, "examples", "covisibility_harness")


def local_map(seed, n_kf=31, per_kf=1500, n_points=7750):
    """n_kf keyframes (the last one is the current keyframe) that each hold per_kf of n_points map points: about six observations a
    point.  Octaves spread over 0-7, so few points have three observers at the same or a finer scale and nothing is culled."""
    rng = np.random.default_rng(seed)
    kfs = []
    for k in range(n_kf):
        pts = rng.choice(n_points, size=per_kf, replace=False)
        keys = [(int(o), float(d), 4.0 if s else -1.0, int(p))
                for p, o, d, s in zip(pts, rng.integers(0, 8, per_kf), rng.random(per_kf) * 60, rng.random(per_kf) < 0.5)]
        kfs.append(S.KF(k, k, 35.0, keys))
    return S.World(kfs, n_points, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    world = local_map(0)
    n_kf = len(world.kfs)
    res = {"reps": a.reps, "timer": "HIP events inside the call for upload / kernels / download; host clock for adapter_ms and host_loop_ms; medians",
           "keyframes": n_kf, "points_per_keyframe": 1500, "map_points": len(world.obs), "observations": int(sum(len(o) for o in world.obs)),
           "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        for name, update in (("batched", list(range(n_kf - 1))), ("single keyframe", [n_kf - 1])):
            path = os.path.join(tmp, "scene.bin")
            with open(path, "wb") as f:
                # either list leaves the current keyframe connected to its 30 local keyframes, which the culling then visits
                f.write(world.blob(update, n_kf - 1))
            out = subprocess.run([HARNESS, path, "--time", str(a.reps)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit(out.stderr)
            for line in out.stdout.strip().split("\n"):
                case = json.loads(line)
                if case["case"] == "KeyFrameCulling" and name != "batched":
                    continue                    # the same culling as in the first run
                case["update_list"] = name
                res["cases"].append(case)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
