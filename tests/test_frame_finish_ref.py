"""tests/frame_finish_ref.py, the restatement the GPU tests of lld_frame_track_finish compare against, on cases worked by hand, and the
conditions those GPU tests rest on, held on the restatement alone.  CPU only."""
import numpy as np
import pytest

import frame_finish_ref as REF
import frame_finish_scenes as FS

F32 = np.float32
ROT_Z = F32([0, -1, 0, 1, 0, 0, 0, 0, 1])        # mRcw: a quarter turn about z, so mRwc = mRcw.t() = [[0,1,0],[-1,0,0],[0,0,1]]
OW = F32([1, 2, 3])
CAM128 = (128.0, 128.0, 0.0, 0.0, 50.0)          # invfx = 1/128 exactly


def state(ids, obs, out):
    n = len(ids)
    return dict(kp_id=np.int32(ids), kp_obs=np.uint8(obs), kp_outlier=np.uint8(out), kp_world=np.zeros((n, 3), F32))


def test_five_keypoints_by_hand():
    depth = F32([4.0, -1.0, 2.0, 2.0, 50.0])
    xy = F32([[128, 64], [1, 1], [128, 64], [-64, 128], [0, 0]])
    # 0: held, observed; 1: none, no depth; 2: held, NOT observed, flagged; 3: none; 4: held, observed, flagged (an outlier, far)
    st = state([7, -1, 8, -1, 9], [1, 0, 0, 0, 1], [0, 1, 1, 0, 1])
    p = dict(REF.DECISION_DEFAULTS)
    out, r = REF.track_finish(st, depth, xy, CAM128, ROT_Z, OW, 10.0, 500, p)
    # clean VO: keypoint 2 loses its point and its flag.  close (< 10): 0 tracked; 2 and 3 not.  4 is far.
    assert (r["n_tracked_close"], r["n_non_tracked_close"]) == (1, 2)
    assert r["need"] == 1 and r["made"] == 1 and r["interrupt_ba"] == 0
    # sorted pairs: (2.0, 2), (2.0, 3), (4.0, 0), (50.0, 4): four entries, all visited; new points on 2 and 3, in that order
    assert r["n_visited"] == 4 and r["n_created"] == 2
    assert r["order"].tolist() == [2, -1, 0, 1, 3]
    assert r["created"].tolist() == [0, 0, 1, 1, 0] and r["new_id"].tolist() == [-1, -1, 500, 501, -1]
    # keypoint 2: xc = (128*2/128, 64*2/128, 2) = (2, 1, 2); Rwc xc = (1, -2, 2); + Ow = (2, 0, 5).  keypoint 3: xc = (-1, 2, 2) -> (2, 1, 2) + Ow = (3, 3, 5)
    assert r["x3d"][2].tolist() == [2.0, 0.0, 5.0] and r["x3d"][3].tolist() == [3.0, 3.0, 5.0]
    assert np.all(r["x3d"][[0, 1, 4]] == 0)
    # the outlier drop: 4 leaves; the point made on 2 stays (its flag was cleaned)
    assert r["kp_point_id"].tolist() == [7, -1, 500, 501, -1]
    assert out["kp_outlier"].tolist() == [0, 1, 0, 0, 1] and out["kp_obs"].tolist()[2:4] == [1, 1]
    # nothing made: the cleaning and the drop still happen
    out0, r0 = REF.track_finish(st, depth, xy, CAM128, ROT_Z, OW, 10.0, 500, p, force=0)
    assert r0["made"] == 0 and r0["need"] == 1 and r0["n_visited"] == 0 and r0["n_created"] == 0 and r0["kp_point_id"].tolist() == [7, -1, -1, -1, -1]
    # a new point on a keypoint whose stale flag is set leaves the frame again (:474), but was made
    st2 = state([-1], [0], [1])
    _, r2 = REF.track_finish(st2, F32([3.0]), F32([[0, 0]]), CAM128, ROT_Z, OW, 10.0, 9, p)
    assert r2["created"].tolist() == [1] and r2["new_id"].tolist() == [9] and r2["kp_point_id"].tolist() == [-1]


def test_the_walk_by_hand():
    """103 candidates, the first 99 close: rank 99 is far but nPoints is 100 there; rank 100 is far with nPoints 101 and ends the walk."""
    n = 103
    depth = F32(np.r_[0.5 + 0.1 * np.arange(99), 40.0, 41.0, 42.0, 43.0])
    xy = np.zeros((n, 2), F32)
    st = state([-1] * n, [0] * n, [0] * n)
    _, r = REF.create_points(st, depth, xy, CAM128, ROT_Z, OW, 35.0, 0)
    assert r["n_visited"] == 101 and r["n_created"] == 101 and r["order"][100] == 100 and r["order"][101] == -1 and r["order"][102] == -1
    # exactly mThDepth at rank 100 does not end it; the next far one does
    depth[99] = depth[100] = 35.0                                       # ranks 99 and 100 hold 35.0, rank 101 holds 42.0
    _, r = REF.create_points(st, depth, xy, CAM128, ROT_Z, OW, 35.0, 0)
    assert r["n_visited"] == 102
    # equal depths keep index order; a held, observed point is visited and counted but not replaced; temporal points carry no observation
    depth = F32([5, 5, 5, 5]); st = state([-1, 3, -1, 4], [0, 1, 0, 0], [0] * 4)
    out, r = REF.create_points(st, depth, np.zeros((4, 2), F32), CAM128, ROT_Z, OW, 35.0, 20, keyframe=False)
    assert r["order"].tolist() == [0, 1, 2, 3] and r["new_id"].tolist() == [20, -1, 21, 22] and out["kp_obs"].tolist() == [0, 1, 0, 0]
    # StereoInitialization: index order whatever the depths
    _, r = REF.initialization_points(F32([9, -1, 3, np.inf, np.nan, 0, 1]), np.zeros((7, 2), F32), CAM128, ROT_Z, OW, 5)
    assert r["new_id"].tolist() == [5, -1, 6, 7, -1, -1, 8] and r["order"].tolist() == [0, -1, 1, 2, -1, -1, 3]


BASE = dict(only_tracking=0, mapper_stopped=0, mapper_idle=1, keyframes_in_queue=0, set_not_stop_ok=1, monocular=0, max_frames=30, min_frames=10, n_keyframes=10,
            n_ref_matches=200, n_matches_inliers=100, frame_id=100, last_reloc_frame_id=0, last_keyframe_id=95)


def need(ntc=200, nntc=0, **over):
    p = dict(BASE, **over)
    return REF.need_new_keyframe(p, ntc, nntc, p["n_matches_inliers"])


def test_decision_rows_by_hand():
    # the base row: c1a (100 >= 125), c1b (100 >= 105), c1c (100 < 50) all false, c2 (100 < 150 and > 15) true
    assert need() == (False, False)
    assert need(last_keyframe_id=70) == (True, False)                                  # c1a alone
    assert need(min_frames=5) == (True, False)                                         # c1b alone
    assert need(min_frames=5, mapper_idle=0) == (False, False)                         # ... needs an idle mapper
    assert need(n_matches_inliers=49) == (True, False)                                 # c1c alone: 49 < 200 * 0.25
    assert need(n_matches_inliers=50) == (False, False)                                # 50 < 50 is false
    assert need(ntc=99, nntc=71) == (True, False)                                      # c1c by bNeedToInsertClose (which also serves c2)
    assert need(ntc=100, nntc=71) == (False, False) and need(ntc=99, nntc=70) == (False, False)
    # c2 flipped alone under a true c1a
    assert need(last_keyframe_id=70, n_matches_inliers=150) == (False, False)          # 150 < 150 is false
    assert need(last_keyframe_id=70, n_matches_inliers=149) == (True, False)
    assert need(last_keyframe_id=70, n_matches_inliers=15, n_ref_matches=400) == (False, False)   # not > 15
    assert need(last_keyframe_id=70, n_matches_inliers=16, n_ref_matches=400) == (True, False)
    assert need(last_keyframe_id=70, n_matches_inliers=150, ntc=99, nntc=71) == (True, False)
    # thRefRatio: 0.4f below two keyframes, 0.9f monocular (where c1c is off)
    assert need(last_keyframe_id=70, n_keyframes=1) == (False, False) and need(last_keyframe_id=70, n_keyframes=1, n_matches_inliers=79) == (True, False)
    assert need(last_keyframe_id=70, monocular=1, n_matches_inliers=179) == (True, False) and need(last_keyframe_id=70, monocular=1, n_matches_inliers=180) == (False, False)
    assert need(monocular=1, n_matches_inliers=49) == (False, False)
    # 0.75f is exact, 0.4f and 0.9f are not: 5 * 0.4f = 2.0000000298 rounds to 2.0f, 10 * 0.9f = 9.0000003576 rounds to 9.0f
    assert F32(5) * F32(0.4) == F32(2) and F32(10) * F32(0.9) == F32(9)
    # the mapper is busy: InterruptBA, and a keyframe only while fewer than three wait
    assert need(last_keyframe_id=70, mapper_idle=0, keyframes_in_queue=2) == (True, True)
    assert need(last_keyframe_id=70, mapper_idle=0, keyframes_in_queue=3) == (False, True)
    assert need(last_keyframe_id=70, mapper_idle=0, keyframes_in_queue=0, monocular=1, n_matches_inliers=100) == (False, True)
    # the early exits
    assert need(last_keyframe_id=70, only_tracking=1) == (False, False) and need(last_keyframe_id=70, mapper_stopped=1) == (False, False)
    assert need(last_keyframe_id=70, last_reloc_frame_id=80, n_keyframes=31) == (False, False)     # 100 < 110 and 31 > 30
    assert need(last_keyframe_id=70, last_reloc_frame_id=80, n_keyframes=30) == (True, False)
    assert need(last_keyframe_id=70, last_reloc_frame_id=70, n_keyframes=31) == (True, False)      # 100 < 100 is false
    # ids beyond 32 bits
    big = 1 << 33
    assert need(frame_id=big + 100, last_keyframe_id=big + 70, last_reloc_frame_id=big) == (True, False)
    assert need(frame_id=big + 100, last_keyframe_id=big + 95, last_reloc_frame_id=big) == (False, False)


VISITED = dict(close99=101, close100=101, close150=151, all_close=200, few=60, at_threshold=131, special=108, inf_breaks=101, n0=0, n1=1, n1_none=0, n4096=2501)


@pytest.mark.parametrize("name", FS.NAMES)
def test_crafted_scenes_are_what_the_gpu_tests_need(name):
    sc = FS.scene(name)
    out, r = FS.expect_finish(sc)
    assert r["made"] == 1
    if name in VISITED:
        assert r["n_visited"] == VISITED[name]
    d = sc["depth"]; st = sc["state"]; n = d.size
    if n >= 128:
        vis = r["order"] >= 0
        held = st["kp_id"] >= 0
        assert (vis & held & (st["kp_obs"] != 0)).sum() >= 5 and (vis & held & (st["kp_obs"] == 0)).sum() >= 5     # held points with and without observations
        assert (vis & (st["kp_outlier"] != 0)).sum() >= 5                                                           # outliers in the visited set ...
        if name not in ("all_close", "few", "inf_breaks"):
            assert ((~vis) & (d > 0) & (st["kp_outlier"] != 0) & held).sum() >= 1                                    # ... and outside it
        assert (held & (st["kp_obs"] != 0) & (st["kp_outlier"] != 0)).sum() >= 1                                     # a held outlier the drop removes
        assert ((r["created"] != 0) & (r["kp_point_id"] < 0)).sum() >= 1                                             # a new point on a stale flag: made, then dropped
        assert 0 < r["n_created"] < r["n_visited"] or name == "n4096"
    if name == "close100":
        far = np.sort(d[d > FS.TH])
        assert r["order"][np.flatnonzero(d == far[0])[0]] == 100 and r["order"][np.flatnonzero(d == far[1])[0]] == -1
    if name == "at_threshold":
        at = d == FS.TH
        assert at.sum() == 10 and np.all(r["order"][at] >= 120) and np.all(r["order"][at] < 130)
        ntc, nntc = REF.close_counts(REF.clean_vo_matches(st), d, FS.TH)
        assert ntc + nntc == 120                                                                                     # == mThDepth is not close
    if name == "ties":
        vis_d = d[r["order"] >= 0]
        assert np.unique(vis_d).size < vis_d.size and (d == FS.TH).sum() >= 5
        o = r["order"]; k = np.flatnonzero(o >= 0); k = k[np.argsort(o[k])]
        same = d[k][1:] == d[k][:-1]
        assert same.sum() > 50 and np.all(k[1:][same] > k[:-1][same])                                               # equal depths: ascending index
    if name == "special":
        assert np.all(r["order"][~(d > 0)] == -1) and np.isinf(d[r["order"] == r["n_visited"] - 1][0]) == False
        assert (r["order"][np.isposinf(d)] == -1).all()                                                              # the +inf entries sort behind the far ones: not reached
    if name == "inf_breaks":
        k = np.flatnonzero(r["order"] == 100)[0]
        assert np.isposinf(d[k]) and k == np.flatnonzero(np.isposinf(d))[0] and np.isinf(r["x3d"][k]).any() == bool(r["created"][k])


def test_chain_scene_is_what_the_gpu_test_needs(oracle):
    """The chain scene on the oracle's own run of both stages: the tail creates at least 20 points, replaces at least one held point without
    observations, drops at least one outlier and leaves at least one far keypoint unvisited - in the RGB-D reading (TrackLocalMap leaves the
    flagged points in the frame); in the STEREO reading the flagged points are gone already (src/Tracking.cc:1171-1172), the rest holds."""
    import oracle_orbsearch as OS
    import oracle_tracking as OT
    ss = FS.chain_keypoints()
    n, ur, dep, br, sad = OS.compute_stereo_matches(ss["L"], ss["R"], ss["left"], ss["right"], ss["inv_scale"], ss["mb"], ss["mbf"])
    sc = FS.chain_scene(ur, dep)
    e1, e2 = OT.track_frame(sc)
    assert e2["n_points_map"] > 30 and int(e2["kp_outlier"].sum()) >= 1
    for rgbd in (1, 0):
        st, (out, r), p = FS.chain_expect(oracle.lib(), sc, e2, rgbd)
        assert r["need"] == 1 and r["made"] == 1
        assert r["n_created"] >= 20
        assert ((st["kp_id"] >= 0) & (st["kp_obs"] == 0) & (r["created"] != 0)).sum() >= 1
        assert ((sc["depth"] > sc["th_depth"]) & (r["order"] < 0)).sum() >= 1
        dropped = ((st["kp_id"] >= 0) & (st["kp_obs"] != 0) & (st["kp_outlier"] != 0)).sum()
        assert dropped >= 1 if rgbd else dropped == 0
