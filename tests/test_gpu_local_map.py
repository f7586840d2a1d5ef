"""Tracking::UpdateLocalMap on the resident map (lld_map_*, lld_frame_track_update_local_map) against the plain-Python restatement of
src/Tracking.cc:1667-1835 in tests/local_map_ref.py: lists, counts, reference keyframe, cleared keypoints and status, all integers, all equal."""
import ctypes as C

import numpy as np
import pytest

import local_map_ref as REF
import local_map_scenes as SC
from lld_slam_amd import abi, synth
from lld_slam_amd.device_map import DeviceMap
from lld_slam_amd.tracking import DeviceTrackedFrame

pytestmark = pytest.mark.gpu

NT = 256
SCENES = SC.all_scenes()


@pytest.fixture(scope="module")
def frame(gpu_ctx):
    F = synth.make_orb_frame(0, NT)
    with DeviceTrackedFrame(gpu_ctx, F, synth.KITTI_CAM) as tf:
        yield tf


def held(tf):
    """What the frame holds now (mvpMapPoints as ids): lld_frame_track_finish reports it; nothing is created without depth."""
    return tf.finish(35.0, 10 ** 6, depth=np.full(NT, -1, np.float32), force=0)["kp_point_id"]


def one_frame(tf, dm, ids):
    kp = np.full(NT, -1, np.int32); kp[:len(ids)] = ids
    tf.set_state(np.eye(4, dtype=np.float32), kp, np.zeros((NT, 3), np.float32))
    tf.update_local_map(dm)
    return tf.local_map_download(dm, stage2=False), held(tf)[:len(ids)]


def same(got, kept, exp, name):
    for k in ("status", "n_voted", "n_bad_cleared", "ref_keyframe", "vote_empty"):
        assert got[k] == exp[k], (name, k, got[k], exp[k])
    assert kept.tolist() == exp["frame_ids"], (name, "cleared keypoints")
    if exp["status"] & REF.KEYFRAME_OVERFLOW:
        return
    assert got["local_keyframes"].tolist() == exp["local_keyframes"], (name, "local keyframes")
    assert (got["n_local_keyframes"], got["n_local_points"], got["n_local_lines"]) == (len(exp["local_keyframes"]), len(exp["local_points"]), len(exp["local_lines"])), name
    if not exp["status"] & REF.POINT_OVERFLOW:
        assert got["local_points"].tolist() == exp["local_points"], (name, "local points")
    else:
        assert got["local_points"] is None
    if not exp["status"] & REF.LINE_OVERFLOW:
        assert got["local_lines"].tolist() == exp["local_lines"], (name, "local lines")
    else:
        assert got["local_lines"] is None


def run_scene(ctx, tf, sc):
    L = sc["limits"]; m = sc["map"]
    state = REF.new_state()
    results = []
    with DeviceMap(ctx, **L) as dm:
        SC.upload(dm, m)
        for step in sc["steps"]:
            if "bad_points" in step:
                for s in step["bad_points"]: m["points"][s]["bad"] = 1
                SC.upload_points(dm, m, step["bad_points"])
                continue
            got, kept = one_frame(tf, dm, step["frame"])
            exp = REF.update_local_map(state, m, step["frame"], L["max_local_points"], L["max_local_lines"])
            same(got, kept, exp, sc["name"])
            results.append((got, exp))
    return results


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scene_matches_the_reference(gpu_ctx, frame, sc):
    import copy
    res = run_scene(gpu_ctx, frame, copy.deepcopy(sc))
    name = sc["name"]
    # each scene shows what it was made for (a scene that lost its point would pass vacuously)
    last = res[-1][1]
    if name.startswith("random"):
        assert last["n_voted"] >= 8 and len(last["local_points"]) > 100
    if name == "empty_vote":
        assert last["vote_empty"] == 1 and last["local_keyframes"] == [0, 1] and last["local_points"] == [0, 2, 3] and res[0][1]["local_points"] == [0, 1, 2, 3]
    if name == "bad_voted":
        assert last["ref_keyframe"] == 1 and 0 not in last["local_keyframes"]
    if name == "tie":
        assert last["ref_keyframe"] == 3
    if name == "parent_break_0":
        assert last["local_keyframes"] == [0, 1, 2, 3, 4, 5, 6, 8]
    if name in ("parent_break_2", "parent_break_2_bad"):
        assert last["local_keyframes"] == [0, 1, 2, 3, 4, 5, 6, 8]
    if name == "parent_break_None":
        assert last["local_keyframes"] == [0, 1, 2, 3, 4, 7]
    if name == "neighbours":
        assert last["local_keyframes"] == [0, 1, 2, 3, 11, 13]
    if name == "children":
        assert last["local_keyframes"] == [0, 1, 2, 4, 3, 6]
    if name == "limit_80":
        assert len(last["local_keyframes"]) == 90
    if name == "limit_80_inside":
        assert len(last["local_keyframes"]) == 81
    if name == "voted_1024":
        assert last["status"] == 0 and len(last["local_keyframes"]) == 1024
    if name == "voted_1025":
        assert last["status"] == REF.KEYFRAME_OVERFLOW
    if name == "list_full_plus0":
        assert last["status"] == 0 and len(last["local_points"]) == 16 and len(last["local_lines"]) == 4
    if name == "list_full_plus1":
        assert last["status"] == REF.POINT_OVERFLOW | REF.LINE_OVERFLOW
    if name == "lines_over":
        assert last["status"] == REF.LINE_OVERFLOW
    if name == "point_details":
        assert last["local_points"] == [5, 6, 8, 10] and last["local_lines"] == [0, 2] and last["n_bad_cleared"] == 2


def test_overflow_keeps_stage2_from_running(gpu_ctx):
    """After an overflow lld_frame_track_local_map_resident leaves the frame as the vote left it, and the record says that it did not run."""
    sc = SC.voted_overflow(1025)
    sc2 = synth.make_tracking_scene(3, n_kp=300, n_map=400, n_last=200, n_lines=0)
    with DeviceMap(gpu_ctx, **sc["limits"]) as dm, DeviceTrackedFrame(gpu_ctx, sc2["frame"], sc2["cam"]) as tf:
        SC.upload(dm, sc["map"])
        nt = sc2["frame"].n
        for ids, ran in (([1], 1), ([0], 0)):
            kp = np.full(nt, -1, np.int32); kp[0] = ids[0]; kp[5] = 7000                           # a temporal point next to the voter
            tf.set_state(sc2["Tcw_true"], kp, np.ones((nt, 3), np.float32))
            tf.update_local_map(dm)
            tf.track_local_map_resident(dm)
            got = tf.local_map_download(dm)
            after = tf.finish(35.0, 10 ** 6, depth=np.full(nt, -1, np.float32), force=0)["kp_point_id"]
            assert got["stage2_ran"] == ran and (got["status"] == 0) == bool(ran)
            if not ran:
                s2 = got["stages"][1]
                assert np.all(s2["kp_point_id"] == -1) and all(s2[c] == 0 for c in ("n_points", "n_search", "n_in_view", "n_edges", "n_inliers")) and not s2["pose_qt"].any()
                assert after[0] == 0 and after[5] == 7000 and np.all(np.delete(after, [0, 5]) == -1)


def test_rows_are_replaced_any_number_of_times(gpu_ctx, frame):
    """An observation row replaced by a longer, a shorter and an empty one, 200 times over inside the limits: the pool never refuses, and the
    whole vote is the reference's afterwards."""
    sc = SC.random_map(3)
    m = sc["map"]; L = dict(sc["limits"])
    rng = np.random.default_rng(5)
    pts = sorted(m["points"]); kfs = sorted(m["keyframes"])
    L["max_observations"] = sum(len(p["obs"]) for p in m["points"].values()) + 12 * 4       # room for four full rows more, no slack beyond
    with DeviceMap(gpu_ctx, **L) as dm:
        SC.upload(dm, m)
        orig = {s: list(m["points"][s]["obs"]) for s in pts}
        victims = []
        for it in range(200):
            # four other rows every time: the long rows go to the pool's tail until it is full and the pool is repacked
            back = victims
            victims = [pts[i] for i in rng.permutation(len(pts))[:4]]
            for s in back: m["points"][s]["obs"] = list(orig[s])
            for j, s in enumerate(victims):
                n = (len(kfs), 1, 0, int(rng.integers(0, len(kfs) + 1)))[(it + j) % 4]
                m["points"][s]["obs"] = [int(k) for k in rng.permutation(kfs)[:n]]
            rows = list(dict.fromkeys(back + victims))
            dm.set_observations(rows, rows=[m["points"][s]["obs"] for s in rows])
        ids = [p for p in pts[:150]] + victims
        exp = REF.update_local_map(REF.new_state(), m, ids, L["max_local_points"], L["max_local_lines"])
        got, kept = one_frame(frame, dm, ids)
        same(got, kept, exp, "row replacement")
        # keyframe rows too: point lists shrink and grow
        for it in range(50):
            for s in kfs[:3]:
                n = (64, 3, 0, 40)[(it + s) % 4]
                m["keyframes"][s]["points"] = [int(pts[j]) for j in rng.integers(0, len(pts), n)]
            SC.upload_keyframes(dm, m, kfs[:3])
        exp = REF.update_local_map(REF.new_state(), m, ids, L["max_local_points"], L["max_local_lines"])
        got, kept = one_frame(frame, dm, ids)
        same(got, kept, exp, "keyframe rows")


def test_refusals_leave_the_map_as_it_was(gpu_ctx, frame):
    sc = SC.random_map(4)
    m = sc["map"]; L = sc["limits"]
    ids = sc["steps"][0]["frame"]
    exp = REF.update_local_map(REF.new_state(), m, ids, L["max_local_points"], L["max_local_lines"])
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    with DeviceMap(gpu_ctx, **L) as dm:
        SC.upload(dm, m)
        lib = gpu_ctx.lib
        p0 = sorted(m["points"])[0]; k0 = sorted(m["keyframes"])[0]; l0 = sorted(m["lines"])[0]
        z3 = np.zeros((1, 3), np.float32); z1 = np.zeros(1, np.float32); d8 = np.zeros((1, 8), np.uint32); b1 = np.ones(1, np.uint8)
        zd = np.zeros((1, 3)); dl = np.zeros((1, SC.LINE_DIM), np.float32)
        bad_calls = [
            lambda: dm.set_points([L["max_points"]], z3, z3, z1, z1, d8, b1),                              # slot out of range
            lambda: dm.set_points([-1], z3, z3, z1, z1, d8, b1),
            lambda: dm.set_points([p0, p0], np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), np.zeros(2, np.float32), np.zeros(2, np.float32),
                                  np.zeros((2, 8), np.uint32), np.ones(2, np.uint8)),                        # a slot twice
            lambda: dm.set_observations([p0], start=[0, 1], kf_slot=[L["max_keyframes"]]),                # referenced slot out of range
            lambda: dm.set_observations([p0], start=[1, 2], kf_slot=[k0, k0]),                            # start not from 0
            lambda: dm.set_observations([p0, p0 + 1], start=[0, 2, 1], kf_slot=[k0, k0]),                 # start descends
            lambda: dm.set_observations([p0], start=[0, L["max_observations"] + 1], kf_slot=[k0] * (L["max_observations"] + 1)),   # total beyond the limit
            lambda: dm.set_keyframes([k0], [1], [1], [L["max_keyframes"]], [[]], [[]], [[]], [[]]),       # parent out of range
            lambda: dm.set_keyframes([k0], [1], [1], [-1], [[k0]], [[]], [[L["max_points"]]], [[]]),      # point slot out of range
            lambda: dm.set_keyframes([k0], [1], [1], [-1], [[]], [[-1]], [[]], [[]]),                      # child -1
            lambda: dm.set_keyframes([k0], [1], [1], [-1], [[]], [[]], [[]], [[L["max_lines"]]]),
            lambda: dm.set_keyframes([k0], [1], [1], [-1], [[]], [[]], [[-1] * (L["max_kf_points"] + 1)], [[]]),   # total beyond the limit
            lambda: dm.set_keyframes([L["max_keyframes"]], [1], [1], [-1], [[]], [[]], [[]], [[]]),
            lambda: dm.set_lines([L["max_lines"]], zd, zd, zd, zd, dl, b1),
        ]
        for i, call in enumerate(bad_calls):
            with pytest.raises(RuntimeError) as e:
                call()
            assert e.value.status in (abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED), i
        # NULL required pointers, through the C interface itself
        one = i32([p0]).ctypes.data_as(abi.c_int32_p)
        assert lib.fn("map_set_points")(dm.handle, 1, one, None, None, None, None, None, None) == abi.LLD_ERR_INVALID
        assert lib.fn("map_set_observations")(dm.handle, 1, one, None, None) == abi.LLD_ERR_INVALID
        assert lib.fn("map_set_lines")(dm.handle, 1, i32([l0]).ctypes.data_as(abi.c_int32_p), None, None, None, None, None, None) == abi.LLD_ERR_INVALID
        assert lib.fn("map_set_keyframes")(dm.handle, 1, i32([k0]).ctypes.data_as(abi.c_int32_p), *([None] * 11)) == abi.LLD_ERR_INVALID
        assert lib.fn("map_set_points")(None, 1, one, None, None, None, None, None, None) == abi.LLD_ERR_INVALID
        h = C.c_void_p()
        assert lib.fn("map_create")(gpu_ctx.handle, None, C.byref(h)) == abi.LLD_ERR_INVALID
        got, kept = one_frame(frame, dm, ids)
        same(got, kept, exp, "after the refusals")
