"""The TrackReferenceKeyFrame scenes (tests/refkf_scenes.py) are what their names say - asserted with the CPU reference alone
(tests/refkf_ref.py), so that no comparison of tests/test_gpu_track_refkf.py passes on an empty case."""
import numpy as np
import pytest

import bow_ref
import refkf_ref as RR
import refkf_scenes as RS


@pytest.fixture(scope="module")
def records(oracle):
    return {name: RR.track(RS.make_scene(name)) for name in RS.NAMES}


@pytest.mark.parametrize("name", ["main", "chunks", "deep_levelsup", "duplicates", "rotation_outliers"])
def test_main_scenes_track(records, name):
    r1, r2 = records[name]
    assert r1["n_search"] >= 15 and r1["n_points_map"] >= 10, (r1["n_search"], r1["n_points_map"])
    assert r1["n_lines_matched"] == 0 and r1["n_lines"] == 0                     # TrackReferenceKeyFrame adds no lines ...
    assert r2["n_lines_matched"] > 0 and r2["n_search"] > 0                      # ... and TrackLocalMap finds them, and further points


def test_node_shapes():
    """16 nodes of a few features; two nodes of more than 64 frame features (the chunk loop); one node under the root."""
    for name, n_nodes, most in (("main", 16, 64), ("chunks", 2, 10 ** 6), ("deep_levelsup", 1, 10 ** 6)):
        S = RS.make_scene(name)
        fv = RR.frame_bow(S)
        sizes = np.diff(fv["node_start"])
        assert len(fv["node"]) == n_nodes and sizes.max() <= most, (name, len(fv["node"]), sizes.max())
        if name != "main":
            assert sizes.min() > 64 and np.diff(S["kf"]["node_start"]).min() > 64
    assert RR.frame_bow(RS.make_scene("deep_levelsup"))["node"].tolist() == [0]


def test_in_node_occupancy_occurs_in_the_main_scene(oracle):
    """At least one keyframe feature's nearest frame feature in its node was taken by an earlier one."""
    S = RS.make_scene("main")
    n, slot = RR.search(S, check_orientation=False)
    kf, F = S["kf"], S["sc"]["frame"]
    nd = RR.common_nodes(kf, RR.frame_bow(S))
    blocked = 0
    for i in range(nd["n_nodes"]):
        fi = nd["idx2"][nd["start2"][i]:nd["start2"][i + 1]]
        for q in nd["idx1"][nd["start1"][i]:nd["start1"][i + 1]]:
            if kf["point_id"][q] < 0: continue
            best = fi[np.argmin(bow_ref.distance(F.desc[fi], kf["desc"][q][None]))]
            blocked += int(slot[best] >= 0 and slot[best] != q and np.nonzero(kf["feature"] == slot[best])[0][0] < np.nonzero(kf["feature"] == q)[0][0])
    assert blocked >= 1


def test_disjoint_and_empty_keyframes_match_nothing(records):
    for name in ("disjoint_nodes", "kf_all_null", "kf_empty"):
        r1, r2 = records[name]
        assert r1["n_search"] == 0 and r1["n_points"] == 0 and r1["n_point_edges"] == 0 and np.all(r1["kp_point_id"] == -1), name
        assert r2["n_search"] > 15                                              # TrackLocalMap from the handed-in pose still works
    assert np.any(RS.make_scene("kf_all_null")["kf"]["node_start"][1:] > 0) and RS.make_scene("kf_empty")["kf"]["desc"].shape[0] == 0
    S = RS.make_scene("disjoint_nodes")
    assert len(np.intersect1d(S["kf"]["node"], RR.frame_bow(S)["node"])) == 0 and len(S["kf"]["node"]) > 0


def test_histogram_scene_removes_matches(oracle):
    S = RS.make_scene("rotation_outliers")
    n_with, _ = RR.search(S, True); n_without, _ = RR.search(S, False)
    assert n_without - n_with >= 1, (n_with, n_without)


def test_duplicate_scene_has_contested_features(oracle):
    S = RS.make_scene("duplicates")
    _, slot = RR.search(S)
    F, kf = S["sc"]["frame"], S["kf"]
    contested = 0
    for a, b, k1, k2 in S["contest"]:
        assert bow_ref.distance(kf["desc"][k2], F.desc[a]) < bow_ref.distance(kf["desc"][k2], F.desc[b])    # the second wants a as well
        contested += int(slot[a] == k1 and slot[b] == k2)
    assert contested >= 1, contested


def test_failure_exit_scene(records):
    r1, _ = records["failure_exit"]
    assert 5 <= r1["n_search"] < 15, r1["n_search"]


def test_weak_pose_scene(records):
    r1, _ = records["weak_pose"]
    assert r1["n_search"] >= 15 and r1["n_points_map"] < 10, (r1["n_search"], r1["n_points_map"])


def test_discard_happens_and_is_handed_to_the_local_map(records):
    """Some scene discards a MapPoint of the local map in stage 1: TrackLocalMap must then not match it again (mnLastFrameSeen, :808)."""
    seen = 0
    for name in RS.NAMES:
        r1, r2 = records[name]
        S = RS.make_scene(name)
        gone = r1["kp_point_id"][r1["kp_outlier"] != 0]
        gone = gone[np.isin(gone, S["sc"]["map_ids"])]
        seen += len(gone)
        assert not np.any(np.isin(gone, r2["kp_point_id"]))
    assert seen >= 1
