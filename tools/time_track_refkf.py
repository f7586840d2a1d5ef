#!/usr/bin/env python3
"""Time of Tracking::TrackReferenceKeyFrame + TrackLocalMap on one frame, two routes on the same build, HIP events on the context's stream,
medians of `repeats` after warm-up.  The frame: 2000 keypoints and 300 stereo lines (synth.make_tracking_scene), a 2000-keypoint reference
keyframe (tests/refkf_scenes.make_keyframe), the synthetic vocabulary of ORBvoc's size (bow_ref.make_vocab: k 10, L 6), levelsup 4.
  (a) the device-resident sequence: lld_frame_compute_bow (no host result), lld_frame_track_reference_keyframe, lld_frame_track_local_map,
      lld_frame_track_download;
  (b) the call-by-call route: lld_bow_transform (host result), the node merge on the host, lld_orb_search_run (CSR, sequential),
      lld_pose_opt on host-gathered edges, the discard on the host, lld_frame_track_set_state, lld_frame_track_local_map, the download.
      The keyframe's FeatureVector exists before the frame arrives in both routes.
The bar: (a)'s median below (b)'s by more than the larger of the two interquartile ranges.
    python tools/time_track_refkf.py [out.json=profiles/track_refkf_time.json] [repeats=200]      (prints and writes one JSON object)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import bow_ref as B  # noqa: E402
import refkf_scenes as RS  # noqa: E402
from lld_slam_amd import Context, Optimizer, ORBmatcher, host, synth, tracking  # noqa: E402
from lld_slam_amd import vocabulary as voc  # noqa: E402
from time_bow import Events  # noqa: E402


def spread(t):
    t = np.asarray(t)
    q1, q3 = np.percentile(t, [25, 75])
    return dict(median_ms=round(float(np.median(t)), 4), iqr_ms=round(float(q3 - q1), 4), min_ms=round(float(t.min()), 4), p90_ms=round(float(np.percentile(t, 90)), 4), repeats=int(t.size))


def main(out_path, repeats=200, warm=20, levelsup=4):
    V = B.make_vocab(22, k=10, L=6, p_early_leaf=0.002, p_stop=0.02)
    sc = synth.make_tracking_scene(0)
    F = sc["frame"]
    kf = RS.make_keyframe(sc, np.random.default_rng(5), 2000, 0.6)
    T_last = np.asarray(sc["Tcw_guess"], np.float32)
    with Context(0) as ctx, voc.ORBVocabulary.from_arrays(ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=2, max_features=4096) as vocab:
        fvK = vocab.transform(kf["desc"], levelsup)                      # KeyFrame::ComputeBoW, when the keyframe was made
        kf.update(node=fvK.node, node_start=fvK.node_start, feature=fvK.feature)
        KF = RS.keyframe_frame(kf)
        valid = (kf["point_id"] >= 0).astype(np.uint8)
        ev = Events(ctx.stream())
        matcher, optim = ORBmatcher(ctx, 0.7, True), Optimizer(ctx)
        with tracking.DeviceTrackedFrame(ctx, F, sc["cam"], sc["lines"]) as tf:
            last = {}

            def route_a():
                tf.compute_bow(vocab, levelsup)
                tf.track_reference_keyframe(T_last, kf)
                tf.track_local_map(sc["map_points"], sc["map_ids"], sc["local_lines"])
                last["a"] = tf.download()

            def route_b():
                fvF = vocab.transform(F.desc, levelsup)
                nd = voc.common_nodes(fvK, fvF)
                out = matcher.SearchByBoWFrame(KF, F, nd, valid)
                slot = np.where(out.owner >= 0, out.query_kp[np.maximum(out.owner, 0)], -1)
                has = slot >= 0
                world = np.where(has[:, None], kf["world_pos"][np.maximum(slot, 0)], 0).astype(np.float32)
                qt = host.se3_from_tcw_f32(ctx.lib, T_last)
                prob, idx = tracking.pose_frame_from_matches(F, sc["cam"], qt, world, has)
                po = optim.PoseOptimization(prob, 0.5)
                bad = np.zeros(F.n, bool); bad[idx[po.pt_outlier != 0]] = True
                ids = np.where(has & ~bad, kf["point_id"][np.maximum(slot, 0)], -1).astype(np.int32)
                seen = kf["point_id"][slot[bad]]
                obs = np.where(ids >= 0, kf["has_obs"][np.maximum(slot, 0)], 0).astype(np.uint8)
                Tcw = host.se3_to_tcw_f32(ctx.lib, po.pose_qt) if len(idx) >= 3 else T_last
                tf.set_state(Tcw, ids, world, obs, None, seen)
                tf.track_local_map(sc["map_points"], sc["map_ids"], sc["local_lines"])
                last["b"] = tf.download()

            res = {}
            for name, fn in (("a_device_chain", route_a), ("b_call_by_call", route_b)):
                for _ in range(warm):
                    fn()
                t, w = [], []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    t.append(ev.time(fn))
                    w.append((time.perf_counter() - t0) * 1e3)
                res[name] = dict(events=spread(t), host_wall=spread(w))
            a2, b2 = last["a"][1], last["b"][1]
            res["same_result"] = bool(np.array_equal(a2["kp_point_id"], b2["kp_point_id"]) and np.array_equal(a2["kp_outlier"], b2["kp_outlier"]))
            res["matches"] = dict(search_by_bow=last["a"][0]["n_search"], after_stage1=last["a"][0]["n_points"], at_the_end=a2["n_points"], lines_at_the_end=a2["n_lines"])
    ea, eb = res["a_device_chain"]["events"], res["b_call_by_call"]["events"]
    res["a_below_b_by_more_than_the_larger_iqr"] = bool(eb["median_ms"] - ea["median_ms"] > max(ea["iqr_ms"], eb["iqr_ms"]))
    res["shape"] = dict(frame_keypoints=int(F.n), keyframe_keypoints=2000, local_map_points=int(len(sc["map_ids"])), vocabulary=dict(k=10, L=6, words=int(V["is_leaf"].sum())), levelsup=levelsup)
    txt = json.dumps(res, indent=1)
    print(txt)
    if out_path:
        with open(out_path, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "track_refkf_time.json"), int(sys.argv[2]) if len(sys.argv) > 2 else 200)
