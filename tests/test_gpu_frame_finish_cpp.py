"""lld_frame_track_finish from compiled C++ (examples/frame_finish_harness.cpp): over include/lld_amd.hpp against the Python route, the host loops
it replaces (examples/frame_finish_host.cpp) against the restatement, and adapters/lld_tracking_adapter.cc's NeedNewKeyFrame / CreateNewKeyFrame /
DropOutliers / UpdateLastFrame on the object doubles: the same integers and float32 positions, and the object graph the reference's loops leave."""
import os
import subprocess

import numpy as np
import pytest

import frame_finish_ref as REF
import frame_finish_scenes as FS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "frame_finish_harness")
# a keyframe made by an idle mapper; a keyframe made past a busy one (InterruptBA, two keyframes waiting) on the scene with the odd depths
CASES = {"close150": {}, "special": dict(mapper_idle=0, keyframes_in_queue=2, last_keyframe_id=60)}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "frame_finish_harness"], check=True, capture_output=True)
    d = tmp_path_factory.mktemp("frame_finish")
    out = {}
    for name, over in CASES.items():
        sc = FS.scene(name)
        FS.write_harness_scene(str(d / f"{name}.bin"), sc, **over)
        r = subprocess.run([HARNESS, str(d / f"{name}.bin"), str(d / f"{name}.out")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[name] = FS.read_harness_result(str(d / f"{name}.out"), sc["depth"].size)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_hpp_route_and_host_loops_equal_the_python_route(gpu_ctx, results, name):
    sc = FS.scene(name); over = CASES[name]
    _, e = FS.expect_finish(sc, **over)
    g = FS.device_finish(gpu_ctx, sc, **over)
    FS.same_result(g, e, "python route")
    FS.same_result(results[name]["hpp"], g, "TrackedFrame::Finish")
    FS.same_result(results[name]["host"], e, "host loops")
    assert g["made"] == 1 and g["n_created"] > 40 and g["interrupt_ba"] == (1 if over else 0)


@pytest.mark.parametrize("name", list(CASES))
def test_adapter_leaves_the_reference_object_graph(results, name):
    import oracle_tracking as OT
    sc = FS.scene(name); over = CASES[name]
    a = results[name]["adapter"]
    # the adapter forms the view from the Frame double's own UpdatePoseMatrices (the sums of oracle_tracking.pose_view)
    v = OT.pose_view(sc["T"], FS.CAM, sc["F"])
    Rcw, Ow = np.array(v.Rcw, np.float32), np.array(v.Ow, np.float32)
    st, e = REF.track_finish(sc["state"], sc["depth"], sc["F"].xy, FS.CAM, Rcw, Ow, FS.TH, FS.FIRST_ID, dict(sc["p"], **over))
    made = e["created"] != 0
    assert (a["need"], a["interrupt_ba"], a["made"]) == (e["need"], e["interrupt_ba"], e["made"]) and a["n_map_points"] == e["n_created"] == int(made.sum())
    np.testing.assert_array_equal(a["frame_ids"], e["kp_point_id"])                       # mCurrentFrame.mvpMapPoints when Track() returns
    # pKF took the frame's points after the cleaning and before the drop (:1375), then the new ones (:1416): the flagged points stay in it
    cleaned = REF.clean_vo_matches(sc["state"])["kp_id"]
    np.testing.assert_array_equal(a["kf_ids"], np.where(made, e["new_id"], cleaned))
    assert ((cleaned >= 0) & (e["kp_point_id"] < 0) & ~made).sum() >= 1
    np.testing.assert_array_equal(a["obs_index"], np.where(made, 1, -1))                  # one observation each, in pKF at its keypoint; in the map
    np.testing.assert_array_equal(FS.bits(a["world"]), FS.bits(e["x3d"]))
    np.testing.assert_array_equal(a["map_order"], FS.FIRST_ID + np.arange(int(made.sum())))   # mnId in construction order = the ids the device gave
    # UpdateLastFrame on the same frame: temporal points in visiting order, entered into mLastFrame.mvpMapPoints, no observation
    L = results[name]["last_frame"]
    st1, e1 = REF.create_points(sc["state"], sc["depth"], sc["F"].xy, FS.CAM, Rcw, Ow, FS.TH, FS.FIRST_ID, keyframe=False)
    np.testing.assert_array_equal(L["frame_ids"], st1["kp_id"])
    np.testing.assert_array_equal(FS.bits(L["world"]), FS.bits(e1["x3d"]))
    np.testing.assert_array_equal(L["temporal_ids"], FS.FIRST_ID + np.arange(e1["n_created"]))
    assert e1["n_created"] > 40
