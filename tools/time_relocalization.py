#!/usr/bin/env python3
"""Time of Tracking::Relocalization on one lost frame, two routes on the same build, HIP events on the context's stream, medians of
`repeats` after warm-up.  The frame: 2000 keypoints (synth.make_tracking_scene); candidates of 1000 keypoints built by
tests/reloc_scenes.make_candidate; the synthetic vocabulary of ORBvoc's size (bow_ref.make_vocab: k 10, L 6), levelsup 4.
  workloads
    twenty        20 candidates whose SearchByBoW counts spread over about 30-300 (near the shape of the PnPsolver row of README), their MapPoints
                  consistent with the frame in u, v but not in depth: every round hands out poses whose PoseOptimization ends below 10 inliers,
                  until every solver has spent its budget - the routine at its longest
    five_first    5 candidates, the first wins in round 1
  routes
    (a) the single call: lld_frame_compute_bow + lld_frame_relocalize (DeviceTrackedFrame.relocalize)
    (b) call by call (lld_slam_amd.tracking.relocalize_call_by_call): lld_bow_transform, lld_orb_search_run per candidate,
        lld_pnp_batch_* with a download per round, lld_pose_opt / lld_orb_search_projected per rung, lld_frame_track_set_state on success.
        The keyframes' FeatureVectors exist before the frame arrives in both routes.
The bar: (a)'s median below (b)'s by more than the larger of the two interquartile ranges.
    python tools/time_relocalization.py [out.json=profiles/relocalization_time.json] [repeats=200]      (prints and writes one JSON object)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import bow_ref as B  # noqa: E402
import reloc_scenes as RS2  # noqa: E402
from lld_slam_amd import Context, synth, tracking  # noqa: E402
from lld_slam_amd import vocabulary as voc  # noqa: E402
from time_bow import Events  # noqa: E402

INTS = ("matched", "winner", "round", "n_good", "n_rounds", "n_kept")
ARRAYS = ("n_bow", "discarded", "rounds", "n_good_last", "rungs", "n_additional1", "n_additional2")


def spread(t):
    t = np.asarray(t)
    q1, q3 = np.percentile(t, [25, 75])
    return dict(median_ms=round(float(np.median(t)), 4), iqr_ms=round(float(q3 - q1), 4), min_ms=round(float(t.min()), 4), p90_ms=round(float(np.percentile(t, 90)), 4), repeats=int(t.size))


def workloads(sc, vocab, levelsup):
    rng = np.random.default_rng(41)
    twenty = [RS2.make_candidate(sc, rng, dict(ray=int(m * 0.62), wrong=int(m * 0.38)), n_kf=1000) for m in np.linspace(52, 520, 20)]
    five = [RS2.make_candidate(sc, rng, g, n_kf=1000) for g in (dict(good=220, wrong=40), dict(good=120, wrong=60), dict(good=60, wrong=60), dict(good=12, wrong=40), dict(good=90, wrong=30))]
    for kf in twenty + five:                                             # KeyFrame::ComputeBoW, when the keyframe was made
        fv = vocab.transform(kf["desc"], levelsup)
        kf.update(node=fv.node, node_start=fv.node_start, feature=fv.feature)
    return dict(twenty=twenty, five_first=five)


def main(out_path, repeats=200, warm=10, levelsup=4):
    V = B.make_vocab(22, k=10, L=6, p_early_leaf=0.002, p_stop=0.02)
    sc = synth.make_tracking_scene(0, n_lines=0)
    F = sc["frame"]; T0 = np.asarray(sc["Tcw_guess"], np.float32)
    res = {}
    with Context(0) as ctx, voc.ORBVocabulary.from_arrays(ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=2, max_features=4096) as vocab:
        ev = Events(ctx.stream())
        for wname, cands in workloads(sc, vocab, levelsup).items():
            seeds = list(range(100, 100 + len(cands)))
            with tracking.DeviceTrackedFrame(ctx, F, sc["cam"]) as tf:
                last = {}

                def route_a():
                    tf.compute_bow(vocab, levelsup)
                    last["a"] = tf.relocalize(cands, seeds, T0)
                    last["a1"] = tf.download(stage2=False)[0]

                def route_b():
                    r = tracking.relocalize_call_by_call(ctx, vocab, levelsup, F, sc["cam"], cands, seeds)
                    if r["matched"]:
                        tf.set_state(r["Tcw"], r["kp_point_id"], r["kp_world_pos"], r["kp_has_obs"], r["kp_outlier"])
                    last["b"] = r

                w = {}
                for name, fn in (("a_single_call", route_a), ("b_call_by_call", route_b)):
                    for _ in range(warm):
                        fn()
                    t, wall = [], []
                    for _ in range(repeats):
                        t0 = time.perf_counter()
                        t.append(ev.time(fn))
                        wall.append((time.perf_counter() - t0) * 1e3)
                    w[name] = dict(events=spread(t), host_wall=spread(wall))
                a, b = last["a"], last["b"]
                w["same_result"] = bool(all(a[k] == b[k] for k in INTS) and all(np.array_equal(a[k], b[k]) for k in ARRAYS)
                                        and np.array_equal(last["a1"]["kp_point_id"], b["kp_point_id"]) and np.array_equal(last["a1"]["kp_outlier"], b["kp_outlier"]))
                w["run"] = dict(matched=a["matched"], winner=a["winner"], rounds=a["n_rounds"], kept=a["n_kept"], n_bow=[int(x) for x in a["n_bow"]],
                                attempts=int((a["rungs"] != 0).sum()))
                ea, eb = w["a_single_call"]["events"], w["b_call_by_call"]["events"]
                w["a_below_b_by_more_than_the_larger_iqr"] = bool(eb["median_ms"] - ea["median_ms"] > max(ea["iqr_ms"], eb["iqr_ms"]))
                res[wname] = w
    res["shape"] = dict(frame_keypoints=int(F.n), candidate_keypoints=1000, vocabulary=dict(k=10, L=6, words=int(V["is_leaf"].sum())), levelsup=levelsup)
    txt = json.dumps(res, indent=1)
    print(txt)
    if out_path:
        with open(out_path, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "relocalization_time.json"), int(sys.argv[2]) if len(sys.argv) > 2 else 200)
