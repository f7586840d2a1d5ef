"""Times the write-back of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1334-1386) on the resident map, two routes on one build and
one MI355X, on flat tables of LBA-B size (synth.make_lba_b as a map: tests/map_ba_scenes.py map_of_window, the graph of
tools/time_map_ba_window.py):

  (A) lld_map_ba_apply: the device changes the rows, only the result travels
  (B) the route a caller has without it: examples/map_ba_apply_host.cpp's tail on the host's tables, then the lld_map_set_* calls for
      the rows that changed (poses, every window point, the observation rows that lost an entry, the keyframe rows that lost a match,
      the lines)

examples/map_ba_harness apply_time runs both: one solve, untimed, whose result both routes receive; the routes alternate in one
process; before every repetition, untimed, the map is cleared, uploaded again and the window assembled, so that every repetition meets
the same map; HIP events on the context's stream around the whole route.  Medians of --reps with interquartile ranges.  The bar is the
project's own: route A's median below route B's by more than the larger interquartile range; a miss is reported as a miss.

  python tools/time_map_ba_apply.py [--reps 200] [--out profiles/map_ba_apply_time.json] [--scene-out FILE]

The kernels' own times come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- examples/map_ba_harness apply_time FILE 20"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

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


def write_scene(path):
    import map_ba_apply_scenes as AS
    import map_ba_ref as R
    import map_ba_scenes as S
    from lld_slam_amd import abi, host, synth
    lib = abi.product()
    w = synth.make_lba_b(0)
    m, q, table = S.map_of_window(w, 1)
    AS.complete(m, 1)
    win = R.ba_window(m, q, table, lambda T: host.se3_from_tcw_f32(lib, T))
    assert win["status"] == 0
    scale = (np.float32(1.2) ** np.arange(len(table))).astype(np.float32)
    # the result in the file is a placeholder: apply_time solves the window once and gives both routes that result
    AS.write_scene(path, m, q, win, AS.flags_for(win), np.zeros((win["n_local_cams"], 16), np.float32), S.limits_for(m), cam=w.cam, sigma2=table, level_scale=scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_ba_apply_time.json"))
    ap.add_argument("--scene-out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.scene_out or os.path.join(tmp, "lba_b_scene.bin")
        write_scene(path)
        r = subprocess.run([HARNESS, "apply_time", path, str(a.reps)], capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise RuntimeError("map_ba_harness apply_time failed: " + r.stdout[-400:] + r.stderr)
    d = json.loads(r.stdout)
    dev, hst = quart(d["apply_ms"]), quart(d["host_tail_and_setters_ms"])
    res = dict(reps=a.reps, window="synth.make_lba_b(0) as a map (tests/map_ba_scenes.py map_of_window)",
               counts={k: d[k] for k in ("n_cams", "n_local_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs")},
               erased_observations=d["erased"][0], landmarks_gone_bad=d["gone_bad"][0],
               bar="route A's median below route B's by more than the larger interquartile range",
               a_lld_map_ba_apply_ms=dev, b_host_tail_and_setters_ms=hst, met=verdict(dev, hst))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
