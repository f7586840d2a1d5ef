"""lld_frame_track_finish / lld_frame_create_stereo_points: the tail of Tracking::Track (src/Tracking.cc:429-476), NeedNewKeyFrame's counts
and decision, and the depth-ordered stereo points of CreateNewKeyFrame, UpdateLastFrame and StereoInitialization on the resident frame,
against the literal restatement tests/frame_finish_ref.py.  Every comparison is bit-exact: counts, flags, ids, visiting ranks and the float32
positions.  The state is entered with lld_frame_track_set_state except in the chain tests, which run both stages first."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import frame_finish_ref as REF
import frame_finish_scenes as FS
from lld_slam_amd import abi, orb_search
from lld_slam_amd.tracking import DeviceTrackedFrame

pytestmark = pytest.mark.gpu

INVALID = abi.LLD_ERR_INVALID


def view_arrays(v):
    return np.array(v.Rcw, np.float32), np.array(v.Ow, np.float32)


# ---------------------------------------------------------------------------------------------- 1. the crafted scenes
@pytest.mark.parametrize("name", FS.NAMES)
def test_finish_on_crafted_scenes(gpu_ctx, name):
    sc = FS.scene(name)
    _, e = FS.expect_finish(sc)
    g = FS.device_finish(gpu_ctx, sc)
    print("%s: nt %d, close %d + %d, visited %d, created %d" % (name, sc["depth"].size, e["n_tracked_close"], e["n_non_tracked_close"], e["n_visited"], e["n_created"]))
    FS.same_result(g, e, name)
    assert g["made"] == 1


def test_nothing_made_still_cleans_and_drops(gpu_ctx):
    sc = FS.scene("close99")                                                  # (66 close keypoints without a tracked point: bNeedToInsertClose stays false)
    for over in (dict(last_keyframe_id=99, min_frames=50), dict(set_not_stop_ok=0), dict(only_tracking=1), dict(mapper_stopped=1)):
        _, e = FS.expect_finish(sc, **over)
        g = FS.device_finish(gpu_ctx, sc, **over)
        FS.same_result(g, e, str(over))
        assert g["made"] == 0 and g["n_created"] == 0 and g["n_visited"] == 0 and not g["created"].any() and np.all(g["order"] == -1)
        st = sc["state"]
        gone = (st["kp_id"] >= 0) & ((st["kp_obs"] == 0) | (st["kp_outlier"] != 0))
        assert gone.sum() > 20 and np.all(g["kp_point_id"][gone] == -1) and np.array_equal(g["kp_point_id"][~gone], st["kp_id"][~gone])
    assert FS.expect_finish(sc, set_not_stop_ok=0)[1]["need"] == 1


def test_force_both_ways(gpu_ctx):
    sc = FS.scene("close99")
    for force, over in ((1, dict(last_keyframe_id=99, min_frames=50)), (0, {}), (1, dict(only_tracking=1))):
        _, e = FS.expect_finish(sc, force=force, **over)
        g = FS.device_finish(gpu_ctx, sc, force=force, **over)
        FS.same_result(g, e, str((force, over)))
        assert g["made"] == force and g["need"] == (0 if over else 1) and (g["n_created"] > 0) == bool(force)


def test_decision_rows_on_the_device(gpu_ctx):
    """NeedNewKeyFrame's comparisons in the reference's types, each condition flipped alone, on one frame (the counts of the scene: 30 close)."""
    sc = FS.scene("few")
    base = dict(only_tracking=0, mapper_stopped=0, mapper_idle=1, keyframes_in_queue=0, set_not_stop_ok=1, monocular=0, max_frames=30, min_frames=10, n_keyframes=10,
                n_ref_matches=200, n_matches_inliers=100, frame_id=100, last_reloc_frame_id=0, last_keyframe_id=95)
    big = 1 << 33
    rows = [dict(), dict(last_keyframe_id=70), dict(min_frames=5), dict(min_frames=5, mapper_idle=0), dict(n_matches_inliers=49), dict(n_matches_inliers=50),
            dict(last_keyframe_id=70, n_matches_inliers=150), dict(last_keyframe_id=70, n_matches_inliers=149), dict(last_keyframe_id=70, n_matches_inliers=15, n_ref_matches=400),
            dict(last_keyframe_id=70, n_matches_inliers=16, n_ref_matches=400), dict(last_keyframe_id=70, n_keyframes=1), dict(last_keyframe_id=70, n_keyframes=1, n_matches_inliers=79),
            dict(last_keyframe_id=70, monocular=1, n_matches_inliers=179), dict(last_keyframe_id=70, monocular=1, n_matches_inliers=180), dict(monocular=1, n_matches_inliers=49),
            dict(last_keyframe_id=70, n_keyframes=1, n_ref_matches=5, n_matches_inliers=2), dict(last_keyframe_id=70, monocular=1, n_ref_matches=10, n_matches_inliers=9),
            dict(last_keyframe_id=70, mapper_idle=0, keyframes_in_queue=2), dict(last_keyframe_id=70, mapper_idle=0, keyframes_in_queue=3),
            dict(last_keyframe_id=70, mapper_idle=0, monocular=1), dict(last_keyframe_id=70, mapper_idle=0, keyframes_in_queue=2, set_not_stop_ok=0),
            dict(last_keyframe_id=70, only_tracking=1), dict(last_keyframe_id=70, mapper_stopped=1), dict(last_keyframe_id=70, last_reloc_frame_id=80, n_keyframes=31),
            dict(last_keyframe_id=70, last_reloc_frame_id=80, n_keyframes=30), dict(last_keyframe_id=70, last_reloc_frame_id=70, n_keyframes=31),
            dict(frame_id=big + 100, last_keyframe_id=big + 70, last_reloc_frame_id=big), dict(frame_id=big + 100, last_keyframe_id=big + 95, last_reloc_frame_id=big),
            dict(last_keyframe_id=70, n_matches_inliers=-1)]
    seen = set()
    with DeviceTrackedFrame(gpu_ctx, sc["F"], FS.CAM) as tf:
        for over in rows:
            p = dict(base, **over)
            FS.load_state(tf, sc)
            g = tf.finish(FS.TH, FS.FIRST_ID, depth=sc["depth"], **p)
            if p["n_matches_inliers"] < 0: p["n_matches_inliers"] = 0                 # after set_state the stage-2 record reads as empty
            _, e = REF.track_finish(sc["state"], sc["depth"], sc["F"].xy, FS.CAM, *view_arrays(FS.view_of(sc)), FS.TH, FS.FIRST_ID, p)
            FS.same_result(g, e, str(over))
            seen.add((g["need"], g["interrupt_ba"], g["made"]))
    assert seen == {(0, 0, 0), (1, 0, 1), (1, 1, 1), (0, 1, 0), (1, 1, 0)}
    # the close-point rule decides alone: 150 close keypoints, fewer than 100 of them tracked, more than 70 not
    sc = FS.scene("close150")
    _, e = FS.expect_finish(sc, **base)
    assert e["n_tracked_close"] < 100 and e["n_non_tracked_close"] > 70 and e["need"] == 1
    FS.same_result(FS.device_finish(gpu_ctx, sc, **base), e, "bNeedToInsertClose")


# ---------------------------------------------------------------------------------------------- 2. lld_frame_create_stereo_points
def test_last_frame_points_are_temporal_and_use_the_new_pose(gpu_ctx):
    sc = FS.scene("close150")
    T1 = FS.pose(7)
    with DeviceTrackedFrame(gpu_ctx, sc["F"], FS.CAM) as tf:
        for T in (T1, None):
            FS.load_state(tf, sc)
            g = tf.create_stereo_points(abi.POINTS_LAST_FRAME, 300, FS.TH, Tcw_f32=T, depth=sc["depth"])
            v = FS.view_of(sc, T)
            st1, e = REF.create_points(sc["state"], sc["depth"], sc["F"].xy, FS.CAM, *view_arrays(v), FS.TH, 300, keyframe=False)
            e.update(n_tracked_close=0, n_non_tracked_close=0, need=0, interrupt_ba=0, made=1, kp_point_id=st1["kp_id"])      # (no cleaning, no drop)
            FS.same_result(g, e, "last frame")
            assert g["n_created"] > 50 and g["n_visited"] == 151
            # the new points carry no observation: the tail of Track() on the same handle cleans them away (and, made, replaces them)
            for force in (0, 1):
                if force: FS.load_state(tf, sc, T=T); tf.create_stereo_points(abi.POINTS_LAST_FRAME, 300, FS.TH, depth=sc["depth"])
                g2 = tf.finish(FS.TH, 900, depth=sc["depth"], force=force, **sc["p"])
                _, e2 = REF.track_finish(st1, sc["depth"], sc["F"].xy, FS.CAM, *view_arrays(v), FS.TH, 900, sc["p"], force)
                FS.same_result(g2, e2, "finish after last-frame points")
                assert not np.any((g2["kp_point_id"] >= 300) & (g2["kp_point_id"] < 900))
        assert not np.array_equal(view_arrays(FS.view_of(sc, T1))[1], view_arrays(FS.view_of(sc))[1])


def test_initialization_points_in_index_order(gpu_ctx):
    sc = FS.scene("special")
    eye = np.eye(4, dtype=np.float32)
    v = FS.view_of(sc, eye)
    _, e = REF.initialization_points(sc["depth"], sc["F"].xy, FS.CAM, *view_arrays(v), 5)
    e.update(n_tracked_close=0, n_non_tracked_close=0, need=0, interrupt_ba=0, made=1)
    e["kp_point_id"] = e["new_id"]
    with DeviceTrackedFrame(gpu_ctx, sc["F"], FS.CAM) as tf:                     # a frame without a tracking state gets one
        g = tf.create_stereo_points(abi.POINTS_INITIALIZATION, 5, depth=sc["depth"])
        FS.same_result(g, e, "initialization")
        made = np.flatnonzero(g["created"])
        assert made.size == int((sc["depth"] > 0).sum()) and np.array_equal(g["new_id"][made], 5 + np.arange(made.size))
        # ... and on a frame that has one, at another pose: the state is a new frame's again
        FS.load_state(tf, sc)
        T = FS.pose(3)
        g = tf.create_stereo_points(abi.POINTS_INITIALIZATION, 5, Tcw_f32=T, depth=sc["depth"])
        _, e2 = REF.initialization_points(sc["depth"], sc["F"].xy, FS.CAM, *view_arrays(FS.view_of(sc, T)), 5)
        FS.same_result(g, e2, "initialization on a used frame", arrays=("created", "new_id", "x3d", "order"))
        # the frame now has a pose and holds the points: the temporal points of the next frame's UpdateLastFrame find nothing to add
        g3 = tf.create_stereo_points(abi.POINTS_LAST_FRAME, 4000, FS.TH, depth=sc["depth"])
        assert g3["n_created"] == 0 and g3["n_visited"] == 108 and np.array_equal(g3["kp_point_id"], g["new_id"])


# ---------------------------------------------------------------------------------------------- 3. depth from the frame itself
@pytest.fixture(scope="module")
def built_scene(gpu_ctx):
    """The stereo frame the device builds from the chain scene's keypoints, its downloaded mvuRight / mvDepth and the tracking scene around it."""
    ss = FS.chain_keypoints()
    built = orb_search.build_stereo_frame_keypoints(gpu_ctx.lib, gpu_ctx.handle, ss["L"], ss["R"], ss["left"], ss["right"], ss["inv_scale"], ss["mb"], ss["mbf"])
    try:
        st = built.download()
    finally:
        built.close()
    return dict(ss=ss, u_right=st.u_right.copy(), depth=st.depth.copy(), sc=FS.chain_scene(st.u_right, st.depth))


def build(gpu_ctx, ss):
    return orb_search.build_stereo_frame_keypoints(gpu_ctx.lib, gpu_ctx.handle, ss["L"], ss["R"], ss["left"], ss["right"], ss["inv_scale"], ss["mb"], ss["mbf"])


def test_host_depths_equal_the_resident_route(gpu_ctx, built_scene):
    ss, sc = built_scene["ss"], built_scene["sc"]
    F, cam, depth, th = sc["frame"], sc["cam"], built_scene["depth"], sc["th_depth"]
    state = FS.random_state(F.n, 41)
    T = FS.pose(2)
    v = orb_search.frame_view(T, cam, F)
    _, e = REF.track_finish(state, depth, F.xy, cam, *view_arrays(v), th, 50, REF.DECISION_DEFAULTS)
    assert e["n_created"] > 20 and e["n_visited"] < int((depth > 0).sum())
    got = []
    for tf, d in ((DeviceTrackedFrame.from_stereo_build(gpu_ctx, build(gpu_ctx, ss), cam), None), (DeviceTrackedFrame(gpu_ctx, F, cam), depth)):
        with tf:
            tf.set_state(T, state["kp_id"], state["kp_world"], state["kp_obs"], state["kp_outlier"])
            got.append(tf.finish(th, 50, depth=d, **REF.DECISION_DEFAULTS))
            FS.same_result(got[-1], e, "built frame" if d is None else "host depths")
            # the last-frame points read the same depths
            tf.set_state(T, state["kp_id"], state["kp_world"], state["kp_obs"], state["kp_outlier"])
            g = tf.create_stereo_points(abi.POINTS_LAST_FRAME, 50, th, depth=d)
            _, e1 = REF.create_points(state, depth, F.xy, cam, *view_arrays(v), th, 50, keyframe=False)
            FS.same_result(g, e1, "last frame", arrays=("created", "new_id", "x3d", "order"))


# ---------------------------------------------------------------------------------------------- 4. the chain: build, stage 1, stage 2, finish, new map lines
def line_scene():
    import frame_lines_scenes as FL
    return FL.last_kf_scene(0)


def oracle_new_lines(oracle, sc, view_cur, view_last, S, lm_c, lm_l, n_last_held_skip=None):
    """oracle.line_match_last_frame with the chain frame's constants (its camera, its image bounds); nothing occupied, nothing skipped."""
    import oracle_tracking as OT
    fx, fy, cx, cy, bf = [float(np.float32(c)) for c in sc["cam"]]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]); b = float(np.float32(np.float32(bf) / np.float32(fx)))
    cur, last = S["cur"], S["last"]; n = cur["left_lines"].shape[0]; nl = last["left_lines"].shape[0]
    c = dict(left_lines=cur["left_lines"], right_lines=cur["right_lines"], line_matches=lm_c, desc=cur["desc"], occupied=np.zeros(n, np.uint8))
    l = dict(left_lines=last["left_lines"], right_lines=last["right_lines"], line_matches=lm_l, desc=last["desc"], left_octave=last["left_octave"], skip=np.zeros(nl, np.uint8))
    F = sc["frame"]
    return oracle.line_match_last_frame(K, OT.frame_lines_camera(view_cur), OT.frame_lines_camera(view_last), b, 6.0, 0.9, 1.0 / float(F.max_x), 1.0 / float(F.max_y), c, l, 1)


@pytest.mark.parametrize("rgbd", [1, 0])
def test_chain_build_stages_finish_new_map_lines(gpu_ctx, oracle, built_scene, rgbd):
    """Build, stage 1, stage 2, finish, lld_frame_new_map_lines on one handle.  The expected entry state is derived from the downloaded stage-2
    record as the reference leaves the frame after TrackLocalMap (src/Tracking.cc:1155-1175): rgbd = 1 - no point leaves, mvbOutlier stays;
    rgbd = 0 (mSensor == System::STEREO) - the flagged points have left (:1171-1172), mvbOutlier stays."""
    import frame_lines_scenes as FL
    import oracle_tracking as OT
    ss, sc = built_scene["ss"], built_scene["sc"]
    S = line_scene()
    with DeviceTrackedFrame.from_stereo_build(gpu_ctx, build(gpu_ctx, ss), sc["cam"], S["cur"]) as tf, DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], S["last"]) as last:
        view_last = FL.set_line_state(last, S["T_last"], S["last_state"])
        tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"])
        tf.track_local_map(sc["map_points"], sc["map_ids"])
        r1, r2 = tf.download()
        st, (out, e), p = FS.chain_expect(gpu_ctx.lib, sc, r2, rgbd, sensor_rgbd=rgbd)
        g = tf.finish(sc["th_depth"], FS.FIRST_ID, **dict(p, n_matches_inliers=-1))
        print("rgbd %d: stage 2 held %d (%d flagged); close %d + %d, visited %d, created %d, dropped %d" % (
            rgbd, (r2["kp_point_id"] >= 0).sum(), r2["kp_outlier"].sum(), e["n_tracked_close"], e["n_non_tracked_close"], e["n_visited"], e["n_created"],
            ((st["kp_id"] >= 0) & (st["kp_obs"] != 0) & (st["kp_outlier"] != 0)).sum()))
        FS.same_result(g, e, "chain")
        assert g["made"] == 1 and g["n_created"] >= 20 and r2["kp_outlier"].sum() >= 1
        assert ((st["kp_id"] >= 0) & (st["kp_obs"] == 0) & (e["created"] != 0)).sum() >= 1
        assert ((sc["depth"] > sc["th_depth"]) & (e["order"] < 0)).sum() >= 1
        # the line half of the handle is untouched: MatchLinesLastKF on it equals the oracle's, from the view stage 2 left
        from lld_slam_amd import host
        T2 = np.asarray(host.se3_to_tcw_f32(gpu_ctx.lib, np.asarray(r2["pose_qt"], np.float64)), np.float32).reshape(4, 4)
        lm_c = FL.oracle_stereo(oracle, S["cur"])[0]; lm_l = FL.oracle_stereo(oracle, S["last"])[0]
        o = oracle_new_lines(oracle, sc, OT.pose_view(T2, sc["cam"], sc["frame"]), view_last, S, lm_c, lm_l)
        gl = tf.new_map_lines(last, 40000)
        np.testing.assert_array_equal(gl["match_last"], o[0]); np.testing.assert_array_equal(gl["created"], o[1])
        ok = o[1].astype(bool)
        np.testing.assert_allclose(gl["dir"][ok], o[3][ok], atol=1e-7); np.testing.assert_allclose(gl["x0"][ok], o[2][ok], rtol=1e-6, atol=1e-6)
        assert gl["n_created"] == int(ok.sum()) and gl["n_held"] == 0


# ---------------------------------------------------------------------------------------------- 5. refusals
def finish_call(tf, depth, frame=..., params=..., want_out=True, **over):
    nt = tf.F.n
    P = abi.FrameFinishParams()
    P.th_depth = float(FS.TH); P.first_new_id = FS.FIRST_ID; P.force = -1
    for k, v in dict(REF.DECISION_DEFAULTS, **over).items(): setattr(P, k, v)
    d = None if depth is None else np.ascontiguousarray(depth, np.float32)
    P.depth = None if d is None else d.ctypes.data_as(abi.c_float_p)
    R, a = tf._finish_result()
    return tf.lib.fn("frame_track_finish")(tf.res.handle if frame is ... else frame, C.byref(P) if params is ... else params, C.byref(R) if want_out else None)


def points_call(tf, depth, mode=abi.POINTS_LAST_FRAME, th=float(FS.TH), first=10, with_view=False, with_pose=..., with_params=True, frame=..., params=..., want_out=True):
    from lld_slam_amd.host import se3_from_tcw_f32
    P = abi.FramePointsParams()
    P.mode = mode; P.th_depth = th; P.first_new_id = first
    T = np.eye(4, dtype=np.float32); view = orb_search.frame_view(T, tf.cam, tf.F); qt = np.ascontiguousarray(se3_from_tcw_f32(tf.lib, T), np.float64)
    if with_view: P.view = C.addressof(view)
    if with_view if with_pose is ... else with_pose: P.pose_qt = qt.ctypes.data_as(abi.c_double_p)
    if with_params: P.params = C.addressof(tf.params)
    d = None if depth is None else np.ascontiguousarray(depth, np.float32)
    P.depth = None if d is None else d.ctypes.data_as(abi.c_float_p)
    R, a = tf._finish_result()
    return tf.lib.fn("frame_create_stereo_points")(tf.res.handle if frame is ... else frame, C.byref(P) if params is ... else params, C.byref(R) if want_out else None)


def test_refusals_leave_the_frame_unchanged(gpu_ctx, built_scene):
    sc = FS.scene("close100")
    d = sc["depth"]
    _, e = FS.expect_finish(sc)
    nan = float("nan")
    with DeviceTrackedFrame(gpu_ctx, sc["F"], FS.CAM) as tf:
        assert finish_call(tf, d) == INVALID                                      # no tracking state at all
        assert points_call(tf, d) == INVALID                                      # ... and no pose for the last-frame points
        FS.load_state(tf, sc)
        for kw in (dict(frame=None), dict(params=None), dict(want_out=False)):
            assert finish_call(tf, d, **kw) == INVALID, kw
            assert points_call(tf, d, **kw) == INVALID, kw
        assert finish_call(tf, None) == INVALID and points_call(tf, None) == INVALID            # a frame of lld_frame_create keeps no depth
        for over in (dict(th_depth=0.0), dict(th_depth=-1.0), dict(th_depth=nan), dict(first_new_id=-1), dict(first_new_id=2 ** 31 - 160), dict(force=2), dict(force=-2)):
            assert finish_call(tf, d, **over) == INVALID, over
        for kw in (dict(th=0.0), dict(th=nan), dict(first=-1), dict(first=2 ** 31 - 160), dict(mode=2), dict(mode=-1), dict(with_view=True, with_pose=False),
                   dict(with_view=False, with_pose=True), dict(with_view=True, with_params=False), dict(mode=abi.POINTS_INITIALIZATION)):
            assert points_call(tf, d, **kw) == INVALID, kw
        FS.same_result(tf.finish(FS.TH, FS.FIRST_ID, depth=d, **sc["p"]), e, "after the refusals")            # the state of the valid set_state is intact
        FS.load_state(tf, sc)
        assert finish_call(tf, d, first_new_id=2 ** 31 - 1 - 160) == abi.LLD_OK                                # the largest first id the call takes
    # a frame whose last chain call was stage 1: NeedNewKeyFrame has no mnMatchesInliers to read
    bs = built_scene["sc"]
    with DeviceTrackedFrame(gpu_ctx, bs["frame"], bs["cam"]) as tf:
        tf.track_with_motion_model(bs["Tcw_guess"], bs["last"], bs["last_ids"])
        assert finish_call(tf, bs["depth"]) == INVALID
        tf.track_local_map(bs["map_points"], bs["map_ids"])
        r2 = tf.download()[1]
        st, (out, e2), p = FS.chain_expect(gpu_ctx.lib, bs, r2, 0)
        FS.same_result(tf.finish(bs["th_depth"], FS.FIRST_ID, depth=bs["depth"], **p), e2, "stage 1, refusal, stage 2, finish")
