"""CPU: the checker of the per-frame chain (oracle/oracle_tracking.py) - its own Frame::UpdatePoseMatrices, its stage functions, the failure exit of
TrackWithMotionModel - and the boundary scenes of tests/track_scenes.py, each of which must land exactly on its rule's boundary."""
import numpy as np
import pytest

import oracle_tracking as OT
import track_scenes as TS
from lld_slam_amd import orb_search, synth


def test_pose_view_known_answer():
    """A 90 degree turn about z and t = (1, 2, 3): Ow = -Rᵀt = (-2, 1, -3); the camera's floats, the bounds, log(1.2f) in float."""
    T = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], np.float32)
    F = synth.make_orb_frame(0, 10)
    cam = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
    v = OT.pose_view(T, cam, F)
    np.testing.assert_array_equal(np.array(v.Rcw, np.float32), T[:3, :3].reshape(9))
    np.testing.assert_array_equal(np.array(v.tcw, np.float32), [1, 2, 3])
    np.testing.assert_array_equal(np.array(v.Ow, np.float32), [-2, 1, -3])
    assert [v.fx, v.fy, v.cx, v.cy, v.bf] == [float(np.float32(c)) for c in cam]
    assert (v.min_x, v.max_x, v.min_y, v.max_y) == tuple(float(np.float32(x)) for x in (F.min_x, F.max_x, F.min_y, F.max_y))
    assert np.float32(v.log_scale_factor) == np.float32(np.log(np.float32(1.2))) and v.n_levels == 8
    # one rounding of a double sum: -(0.1f * 0.3f + 0.2f * 0.7f + 0 * 1) is not the float sum of float products
    T2 = np.eye(4, dtype=np.float32); T2[:3, :3] = [[0.1, 0.6, 0.0], [0.2, -0.3, 0.0], [0.0, 0.0, 1.0]]; T2[:3, 3] = [0.3, 0.7, 0.0]
    v2 = OT.pose_view(T2, cam, F)
    f = lambda x: float(np.float32(x))
    assert v2.Ow[0] == f(-(f(0.1) * f(0.3) + f(0.2) * f(0.7)))
    assert v2.Ow[1] == f(-(f(0.6) * f(0.3) + f(-0.3) * f(0.7)))


@pytest.mark.parametrize("scene", [0, 1, 2, 3, 10])
def test_pose_view_equals_the_previous_view(scene):
    """The checker's own view equals what it read from lld_slam_amd.orb_search.frame_view before, byte for byte, over the chain's scenes."""
    sc = synth.make_tracking_scene(scene)
    for T in (sc["Tcw_guess"], sc["Tcw_true"], np.asarray(sc["Tcw_true"], np.float32) * np.float32(1.0001)):
        assert bytes(OT.pose_view(T, sc["cam"], sc["frame"])) == bytes(orb_search.frame_view(T, sc["cam"], sc["frame"]))


def test_pose_problem_is_plain():
    sc = synth.make_tracking_scene(0)
    OT.track_frame(sc)
    for p in OT.track_frame.last_problems:
        assert type(p) is OT.PoseProblem and p.pt_xw.dtype == np.float64 and p.ln_octave.dtype == np.int32
        assert p.n_points == p.pt_uvr.shape[0] == p.pt_inv_sigma2.shape[0] and p.n_lines == p.ln_left.shape[0] == p.ln_frame_index.shape[0]


@pytest.mark.parametrize("name", TS.NAMES)
def test_boundary_scene_hits_its_count(name):
    key, want, params, _ = TS.BOUNDARIES[name]
    sc, p = TS.scene(name)                                                   # (asserts the count itself)
    rec = OT.track_frame(sc, **p)[0]
    assert rec[key] == want
    if key == "n_search_first":
        assert rec["used_wide"] == int(want < 20)
    if name.startswith("fail_") and "narrow" not in name and want < 20:
        assert rec["used_wide"] == 1
    if name.endswith("_narrow"):
        assert rec["used_wide"] == 0
    if key == "n_point_edges":
        fr = OT.new_frame(sc); fr.set_pose_matrix(sc["Tcw_guess"])
        assert np.array_equal(rec["pose_qt"], fr.pose_qt) == (want < 3)     # below 3 points the pose stays the prediction's


@pytest.mark.parametrize("name,fails", [("fail_0", True), ("fail_9_wide", True), ("fail_10_wide", False), ("fail_9_narrow", True), ("fail_10_narrow", False)])
def test_failure_state(name, fails):
    """What the reference leaves at :913-917: the raw matches of the search used and nothing else."""
    sc, p = TS.scene(name)
    st = OT.motion_model_failure_state(sc, **p)
    if not fails:
        assert st is None
        return
    rec = OT.track_frame(sc, **p)[0]                                         # runs on: its record's ids are the search's matches
    np.testing.assert_array_equal(st["kp_point_id"], rec["kp_point_id"])
    assert int(np.count_nonzero(st["kp_point_id"] >= 0)) == st["n_search"] == rec["n_search"] < 10
    assert not st["kp_outlier"].any() and np.all(st["ln_line_id"] == -1) and not st["ln_outlier"].any()
    np.testing.assert_array_equal(st["Tcw"], np.asarray(sc["Tcw_guess"], np.float32))
    assert len(st["seen_point_id"]) == 0 and len(st["tracked_line_id"]) == 0
    ids = st["kp_point_id"][st["kp_point_id"] >= 0]
    np.testing.assert_array_equal(np.sort(ids), np.unique(ids))             # one keypoint per MapPoint
    # TrackLocalMap from it finds the frame again
    e2 = OT.track_local_map(sc, st["frame"])
    assert e2["n_points"] > 20 and e2["n_lines_matched"] > 0


def test_failure_state_of_a_tiny_scene():
    """Three points of the last frame, one of them far from its keypoint: two raw matches, the pose is the prediction, no lines."""
    sc = TS.derive(3)
    wp = np.array(sc["last"]["world_pos"], np.float32); wp[1] += np.float32(5.0); sc["last"]["world_pos"] = wp
    st = OT.motion_model_failure_state(sc)
    n1, n, wide = OT.motion_model_search(sc, OT.new_frame(sc))
    assert st is not None and wide == 1 and st["n_search"] == n == int(np.count_nonzero(st["kp_point_id"] >= 0))
    assert 1 not in set(st["kp_point_id"].tolist()) and n <= 2
    np.testing.assert_array_equal(st["Tcw"], np.asarray(sc["Tcw_guess"], np.float32))


@pytest.mark.parametrize("scene", [4, 5])
def test_local_map_from_a_state_equals_the_chain(scene):
    """track_local_map on a frame rebuilt by frame_from_state from what stage 1 left equals the whole sequence's stage 2."""
    sc = synth.make_tracking_scene(scene)
    fr = OT.new_frame(sc)
    rec1 = OT.motion_model_rest(sc, fr, OT.motion_model_search(sc, fr))
    e2 = OT.track_local_map(sc, fr)
    keep = (rec1["kp_point_id"] >= 0) & (rec1["kp_outlier"] == 0)
    ids = np.where(keep, rec1["kp_point_id"], -1)
    world = np.asarray(sc["map_points"]["world_pos"], np.float32)[np.maximum(ids, 0)]
    obs = np.asarray(sc["map_points"]["has_obs"], np.uint8)[np.maximum(ids, 0)]
    seen = rec1["kp_point_id"][(rec1["kp_point_id"] >= 0) & (rec1["kp_outlier"] != 0)]
    LL = sc["last_lines"]; row = {int(i): k for k, i in enumerate(LL["id"])}
    lkeep = (rec1["ln_line_id"] >= 0) & (rec1["ln_outlier"] == 0)
    lid = np.where(lkeep, rec1["ln_line_id"], -1)
    x0 = np.array([LL["X0"][row[int(i)]] if i >= 0 else np.zeros(3) for i in lid]); dr = np.array([LL["dir"][row[int(i)]] if i >= 0 else np.zeros(3) for i in lid])
    thrown = rec1["ln_line_id"][(rec1["ln_line_id"] >= 0) & (rec1["ln_outlier"] != 0)]
    from lld_slam_amd import host
    import oracle_py as O
    T = host.se3_to_tcw_f32(O.lib(), rec1["pose_qt"])
    fr2 = OT.frame_from_state(sc, T, ids, world, obs, None, seen, lid, x0, dr, rec1["ln_outlier"], thrown)
    g2 = OT.track_local_map(sc, fr2)
    for k in e2:
        np.testing.assert_array_equal(np.asarray(g2[k]), np.asarray(e2[k]), err_msg=k)
