"""The frame chain through the resident map - stage 1 -> lld_frame_track_update_local_map -> lld_frame_track_local_map_resident -> finish -
against the route through the host on the same build: stage 1 -> download -> tests/local_map_ref.py -> lld_frame_track_local_map with the
arrays gathered in the reference's order -> finish.  Both stage records (pose included), the finish record and mp_in_view are equal bit for bit."""
import numpy as np
import pytest

import local_map_ref as REF
import local_map_scenes as SC
from lld_slam_amd import synth
from lld_slam_amd.device_map import DeviceMap
from lld_slam_amd.tracking import DeviceTrackedFrame

pytestmark = pytest.mark.gpu

N_KF = SC.N_KF
as_slots, make_map, point_data, line_data, limits, same_dict = SC.as_slots, SC.make_map, SC.point_data, SC.line_data, SC.tracking_limits, SC.same_dict


def scene():
    return as_slots(synth.make_tracking_scene(11, n_kp=300, n_map=400, n_last=200, n_lines=70, n_map_lines=60, n_last_lines=30))


def gathered(sc, m, exp):
    mp = sc["map_points"]; lp = np.asarray(exp["local_points"], np.int64)
    pts = {k: np.asarray(mp[k])[lp] for k in ("world_pos", "normal", "min_distance", "max_distance", "desc")}
    pts["has_obs"] = np.array([len(m["points"][int(p)]["obs"]) > 0 for p in lp], np.uint8)
    ld = line_data(sc); ls = exp["local_lines"]
    lines = {k: np.array([ld[s][k] for s in ls]) for k in ("X0", "dir", "X1", "X2", "desc")}
    lines["id"] = np.asarray(ls, np.int32)
    return pts, lp.astype(np.int32), lines


def finish(tf, sc):
    F = sc["frame"]; bf = np.float32(sc["cam"][4])
    dep = np.where(F.uright >= 0, bf / np.maximum(F.xy[:, 0] - F.uright, np.float32(0.5)), np.float32(-1)).astype(np.float32)
    return tf.finish(35.0 * float(bf) / sc["cam"][0], 10 ** 6, depth=dep, force=1)


def both_routes(ctx, sc, stage1, dm, m, state, what, prepare=lambda tf: None, held=None):
    """One frame on both routes.  held: what the frame holds after stage 1 when its record does not say (lld_frame_track_set_state leaves it empty)."""
    L = dm.limits
    with DeviceTrackedFrame(ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf:
        prepare(tf); stage1(tf)
        r1 = tf.download(stage2=False)[0]
        ids = np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]).tolist() if held is None else list(held)
        exp = REF.update_local_map(state, m, ids, L.max_local_points, L.max_local_lines)
        assert exp["status"] == 0 and exp["n_bad_cleared"] == 0 and exp["n_voted"] >= 4 and len(exp["local_points"]) > 200, what
        pts, pid, lines = gathered(sc, m, exp)
        tf.track_local_map(pts, pid, lines if sc.get("lines") is not None else None)
        a1, a2 = tf.download()
        afin = finish(tf, sc)
    with DeviceTrackedFrame(ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf:
        prepare(tf); stage1(tf)
        tf.update_local_map(dm)
        tf.track_local_map_resident(dm)
        got = tf.local_map_download(dm)
        bfin = finish(tf, sc)
    assert got["status"] == 0 and got["stage2_ran"] == 1
    assert got["local_keyframes"].tolist() == exp["local_keyframes"] and got["local_points"].tolist() == exp["local_points"] and got["local_lines"].tolist() == exp["local_lines"], what
    assert got["ref_keyframe"] == exp["ref_keyframe"]
    b1, b2 = got["stages"]
    n = len(exp["local_points"])
    assert a2["n_search"] > 20 and a2["n_inliers"] > 20, what                   # stage 2 did find and optimise something
    same_dict(b1, a1, what + ": stage 1")
    same_dict(b2, a2, what + ": stage 2", skip=("mp_in_view",))
    np.testing.assert_array_equal(b2["mp_in_view"][:n], a2["mp_in_view"], err_msg=what + ": mp_in_view")
    assert not b2["mp_in_view"][n:].any()
    same_dict(bfin, afin, what + ": finish")
    return m, r1


def motion_model(sc):
    return lambda tf: tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc.get("last_lines"))


def stage1_record(ctx, sc, stage1, prepare=lambda tf: None):
    with DeviceTrackedFrame(ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf:
        prepare(tf); stage1(tf)
        return tf.download(stage2=False)[0]


def open_map(ctx, sc, m):
    dm = DeviceMap(ctx, **limits(sc, m))
    SC.upload(dm, m, point_data(sc), line_data(sc), dim=sc["lines"]["desc"].shape[1])
    return dm


def test_motion_model_then_a_second_frame_on_a_changed_map(gpu_ctx):
    sc = scene()
    state = REF.new_state()
    r1 = stage1_record(gpu_ctx, sc, motion_model(sc))
    m = make_map(sc, np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]), 0)
    with open_map(gpu_ctx, sc, m) as dm:
        both_routes(gpu_ctx, sc, motion_model(sc), dm, m, state, "frame 1")
        # LocalMapping between the frames: a keyframe joins, points move, some turn bad
        rng = np.random.default_rng(5)
        held = np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"])
        free = np.setdiff1d(np.arange(len(m["points"])), held[held >= 0])
        live = [int(p) for p in free if not m["points"][int(p)]["bad"]]
        moved = live[:30]; newly_bad = live[30:45]
        sc2 = dict(sc, map_points=dict(sc["map_points"], world_pos=np.array(sc["map_points"]["world_pos"], np.float32)))
        sc2["map_points"]["world_pos"][moved] += rng.normal(0, 0.05, (len(moved), 3)).astype(np.float32)
        for p in newly_bad: m["points"][p]["bad"] = 1
        new_kf = [s for s in range(N_KF + 4) if s not in m["keyframes"]][0]
        first = sorted(m["keyframes"])[0]
        joined = live[45:120]
        m["keyframes"][new_kf] = dict(key=3, bad=0, parent=first, cov=[first], child=[], points=joined + [-1] + moved[:5], lines=[0, 1])
        m["keyframes"][first]["child"].append(new_kf); m["keyframes"][first]["cov"].insert(0, new_kf)
        for p in joined[:40]: m["points"][p]["obs"].append(new_kf)
        SC.upload_keyframes(dm, m, [new_kf, first])
        SC.upload_points(dm, m, moved + newly_bad + joined[:40], point_data(sc2))
        both_routes(gpu_ctx, sc2, motion_model(sc2), dm, m, state, "frame 2")


def test_set_state_as_stage_1(gpu_ctx):
    sc = scene()
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf:
        motion_model(sc)(tf)
        r1 = tf.download(stage2=False)[0]
    from lld_slam_amd import host
    keep = (r1["kp_point_id"] >= 0) & (r1["kp_outlier"] == 0)
    ids = np.where(keep, r1["kp_point_id"], -1).astype(np.int32)
    world = np.where(keep[:, None], np.asarray(sc["map_points"]["world_pos"], np.float32)[np.maximum(ids, 0)], 0).astype(np.float32)
    obs = np.where(keep, np.asarray(sc["map_points"]["has_obs"])[np.maximum(ids, 0)], 0).astype(np.uint8)
    seen = r1["kp_point_id"][(r1["kp_point_id"] >= 0) & (r1["kp_outlier"] != 0)]
    T = host.se3_to_tcw_f32(gpu_ctx.lib, r1["pose_qt"])
    m = make_map(sc, ids, 1)
    with open_map(gpu_ctx, sc, m) as dm:
        both_routes(gpu_ctx, sc, lambda tf: tf.set_state(T, ids, world, obs, np.zeros(len(ids), np.uint8), seen), dm, m, REF.new_state(), "set_state",
                    held=ids.tolist())


def test_reference_keyframe_as_stage_1(gpu_ctx):
    import refkf_scenes as RS
    from lld_slam_amd.vocabulary import ORBVocabulary
    S = RS.make_scene("main"); sc = as_slots(S["sc"]); V = S["vocab"]
    voc = ORBVocabulary(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=2, max_features=512)
    try:
        run = lambda tf: tf.track_reference_keyframe(S["Tcw_last"], S["kf"])
        bow = lambda tf: tf.compute_bow(voc, S["levelsup"])
        r1 = stage1_record(gpu_ctx, sc, run, bow)
        m = make_map(sc, np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]), 2)
        with open_map(gpu_ctx, sc, m) as dm:
            both_routes(gpu_ctx, sc, run, dm, m, REF.new_state(), "reference keyframe", prepare=bow)
    finally:
        voc.close()


@pytest.mark.parametrize("which", ["points", "lines"])
def test_a_skipped_stage_2_leaves_the_frame_as_it_was(gpu_ctx, which):
    """A local list beyond its limit: stage 2 does not run and the record says so; the frame - what it holds, its pose and view, what it
    discarded and tracked - is as stage 1 left it, shown by a stage 2 on a map with room that follows on the SAME frame and equals, bit for
    bit, the stage 2 of a frame that never met the overflow."""
    sc = scene()
    r1 = stage1_record(gpu_ctx, sc, motion_model(sc))
    m = make_map(sc, np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]), 4)
    tight = dict(limits(sc, m), **({"max_local_points": 16} if which == "points" else {"max_local_lines": 2}))
    bit = REF.POINT_OVERFLOW if which == "points" else REF.LINE_OVERFLOW
    with open_map(gpu_ctx, sc, m) as roomy, DeviceMap(gpu_ctx, **tight) as small:
        SC.upload(small, m, point_data(sc), line_data(sc), dim=tight["line_dim"])
        with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf:
            motion_model(sc)(tf)
            tf.update_local_map(roomy); tf.track_local_map_resident(roomy)
            clean = tf.local_map_download(roomy)
            clean_fin = finish(tf, sc)
        with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf:
            motion_model(sc)(tf)
            tf.update_local_map(small); tf.track_local_map_resident(small)
            over = tf.local_map_download(small)
            assert over["status"] == bit and over["stage2_ran"] == 0
            assert over["local_keyframes"].tolist() == clean["local_keyframes"].tolist()
            assert (over["local_points"] is None) == (which == "points") and (over["local_lines"] is None) == (which == "lines")
            s2 = over["stages"][1]
            assert np.all(s2["kp_point_id"] == -1) and np.all(s2["ln_line_id"] == -1) and not s2["pose_qt"].any() and s2["chi2"] == 0
            assert all(s2[c] == 0 for c in ("n_points", "n_search", "n_in_view", "n_edges", "n_inliers", "n_lines", "n_lines_matched", "n_discarded"))
            same_dict(over["stages"][0], clean["stages"][0], "stage 1")
            tf.update_local_map(roomy); tf.track_local_map_resident(roomy)
            after = tf.local_map_download(roomy)
            after_fin = finish(tf, sc)
    assert after["status"] == 0 and after["stage2_ran"] == 1 and clean["stages"][1]["n_inliers"] > 20
    same_dict(after["stages"][1], clean["stages"][1], "stage 2 after the skipped one")
    same_dict(after_fin, clean_fin, "finish after the skipped one")


def test_resident_stage_2_wants_this_frames_update_first(gpu_ctx):
    """lld_frame_track_local_map_resident refuses lists that are not this frame's: no update since the last stage 1, or one on another map."""
    from lld_slam_amd import abi
    sc = scene()
    r1 = stage1_record(gpu_ctx, sc, motion_model(sc))
    m = make_map(sc, np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]), 5)
    with open_map(gpu_ctx, sc, m) as dm, open_map(gpu_ctx, sc, m) as other, DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf:
        def refused():
            with pytest.raises(RuntimeError, match="lld_frame_track_local_map_resident") as e:
                tf.track_local_map_resident(dm)
            assert e.value.status == abi.LLD_ERR_INVALID
        motion_model(sc)(tf)
        refused()                                                          # no update at all
        tf.update_local_map(other)
        refused()                                                          # an update on another map
        tf.update_local_map(dm)
        motion_model(sc)(tf)
        refused()                                                          # a new stage 1 since
        tf.update_local_map(dm); tf.track_local_map_resident(dm)
        got = tf.local_map_download(dm)
    assert got["status"] == 0 and got["stage2_ran"] == 1 and got["stages"][1]["n_inliers"] > 20


def test_another_frames_update_takes_the_lists(gpu_ctx):
    """The lists live in the map: after another frame's update on it, this frame's stage 2 is refused until it has run its own update again."""
    from lld_slam_amd import abi
    sc = scene()
    r1 = stage1_record(gpu_ctx, sc, motion_model(sc))
    m = make_map(sc, np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]), 5)
    with open_map(gpu_ctx, sc, m) as dm, DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf, \
            DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc.get("lines")) as other:
        motion_model(sc)(tf); tf.update_local_map(dm)
        motion_model(sc)(other); other.update_local_map(dm)
        with pytest.raises(RuntimeError, match="lld_frame_track_local_map_resident") as e:
            tf.track_local_map_resident(dm)
        assert e.value.status == abi.LLD_ERR_INVALID
        other.track_local_map_resident(dm)
        assert other.local_map_download(dm)["stage2_ran"] == 1
        tf.update_local_map(dm); tf.track_local_map_resident(dm)
        assert tf.local_map_download(dm)["stage2_ran"] == 1
