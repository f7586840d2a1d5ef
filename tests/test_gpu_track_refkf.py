"""lld_frame_compute_bow + lld_frame_track_reference_keyframe: Tracking::TrackReferenceKeyFrame (src/Tracking.cc:773-817) as an entry of the
device-resident chain, against the CPU reference's own run of it and of the TrackLocalMap that follows (tests/refkf_ref.py).  Per scene of
tests/refkf_scenes.py: the BowVector / FeatureVector exact, the ids and flags of both stages exact, every counter equal, pose and chi2 within
the bars of tests/test_gpu_track_chain.py and LM counts within its slack rule.

deep_levelsup is the main scene with levelsup alone changed.  On a world of its own (refkf_scenes seed 302) that case agrees in every id, flag
and counter of both stages and in chi2 to 2e-14 relative, while stage 2 - the unchanged TrackLocalMap - spends 16 LM iterations / 100 trials
on the device against 12 / 64 in the reference: outside the 3 / 8 slack of tests/test_gpu_track_chain.py (the pose kernel's LM counts)."""
import dataclasses

import numpy as np
import pytest

import refkf_ref as RR
import refkf_scenes as RS
from lld_slam_amd import ORBmatcher, abi, host, orb_search, synth
from lld_slam_amd.tracking import DeviceTrackedFrame, ref_keyframe_struct
from lld_slam_amd.vocabulary import ORBVocabulary, common_nodes
from test_gpu_track_chain import COUNTERS, same_record

pytestmark = pytest.mark.gpu

BOW_FIELDS = ("word", "value", "node", "node_start", "feature", "feature_word", "feature_nid")


@pytest.fixture(scope="module")
def vocs(gpu_ctx):
    made = {}

    def get(S):
        key = (S["vocab"]["k"], S["vocab"]["L"], S["name"])
        if key not in made:
            V = S["vocab"]
            made[key] = ORBVocabulary(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=2, max_features=512)
        return made[key]
    yield get
    for v in made.values():
        v.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """The reference's records, computed once per scene."""
    return {name: RR.track(RS.make_scene(name)) for name in RS.NAMES}


def open_frame(gpu_ctx, S):
    sc = S["sc"]
    return DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc.get("lines"))


def run_chain(tf, S, voc, bow_on_host=False):
    sc = S["sc"]
    bow = tf.compute_bow(voc, S["levelsup"], host=bow_on_host)
    if len(S["kf"]["angle"]):
        voc.transform(S["kf"]["desc"], S["levelsup"])                     # the vocabulary moves on: the frame's FeatureVector must not care
    tf.track_reference_keyframe(S["Tcw_last"], S["kf"])
    tf.track_local_map(sc["map_points"], sc["map_ids"], sc.get("local_lines"))
    r1, r2 = tf.download()
    return bow, r1, r2


@pytest.mark.parametrize("name", RS.NAMES)
def test_compute_bow_is_exact(gpu_ctx, vocs, name):
    S = RS.make_scene(name); voc = vocs(S)
    with open_frame(gpu_ctx, S) as tf:
        got = tf.compute_bow(voc, S["levelsup"], host=True)
        again = tf.compute_bow(voc, S["levelsup"], host=True)
    via_transform = voc.transform(S["sc"]["frame"].desc, S["levelsup"])
    ref = RR.frame_bow(S)
    for f in BOW_FIELDS:
        g = getattr(got, f)
        assert g.shape == ref[f].shape, f
        view = (lambda a: np.ascontiguousarray(a).view(np.uint64)) if f == "value" else (lambda a: np.asarray(a))
        np.testing.assert_array_equal(view(g), view(getattr(via_transform, f)), err_msg=f)
        np.testing.assert_array_equal(view(g), view(getattr(again, f)), err_msg=f)
        np.testing.assert_array_equal(view(g), view(ref[f].astype(g.dtype)), err_msg=f)


@pytest.mark.parametrize("name", RS.NAMES)
def test_chain_against_the_reference(gpu_ctx, vocs, expected, name):
    S = RS.make_scene(name)
    with open_frame(gpu_ctx, S) as tf:
        _, g1, g2 = run_chain(tf, S, vocs(S))
    e1, e2 = expected[name]
    print(name, "stage 1", {k: (g1[k], e1[k]) for k in ("n_search", "n_points", "n_points_map", "n_discarded", "n_point_edges", "n_inliers", "lm_iterations", "lm_trials")},
          "chi2", g1["chi2"], e1["chi2"], "stage 2", {k: (g2[k], e2[k]) for k in ("n_search", "n_points", "n_lines", "n_inliers")}, "chi2", g2["chi2"], e2["chi2"])
    same_record(g1, e1)
    same_record(g2, e2)                                                    # ... which also proves the discard's ids reached SearchLocalPoints
    assert g1["used_wide"] == 0 and g1["n_search_first"] == g1["n_search"] and g1["n_lines_matched"] == 0 and g1["n_lines"] == 0


def test_empty_frame(gpu_ctx, vocs):
    """nt = 0: empty vectors, LLD_OK, and a stage that matches nothing."""
    S = RS.make_scene("main"); sc = S["sc"]; F = sc["frame"]
    E = dataclasses.replace(F, desc=F.desc[:0].copy(), xy=F.xy[:0].copy(), octave=F.octave[:0].copy(), uright=F.uright[:0].copy(), angle=F.angle[:0].copy()).normalise()
    with DeviceTrackedFrame(gpu_ctx, E, sc["cam"]) as tf:
        bow = tf.compute_bow(vocs(S), S["levelsup"], host=True)
        assert len(bow.word) == 0 and len(bow.node) == 0 and bow.node_start.tolist() == [0]
        tf.track_reference_keyframe(S["Tcw_last"], S["kf"])
        r1 = tf.download(stage2=False)[0]
        assert r1["n_search"] == 0 and r1["n_points"] == 0 and r1["n_point_edges"] == 0


@pytest.mark.parametrize("name", RS.NAMES)
def test_equals_the_call_by_call_host_route(gpu_ctx, vocs, expected, name):
    """lld_bow_transform for both sides, the node merge on the host, lld_orb_search_run's SearchByBoW, the reference's PoseOptimization and
    discard handed in with lld_frame_track_set_state, then TrackLocalMap: the same ids and flags as the chained stage."""
    S = RS.make_scene(name); sc = S["sc"]; kf = S["kf"]; voc = vocs(S)
    e1, _ = expected[name]
    with open_frame(gpu_ctx, S) as tf:
        _, g1, g2 = run_chain(tf, S, voc)
    fvK, fvF = voc.transform([np.asarray(kf["desc"], np.uint32).reshape(-1, 8), sc["frame"].desc], S["levelsup"])
    if name == "disjoint_nodes":                                         # (that keyframe's FeatureVector is hand-made: the host route takes it as given)
        fvK = dataclasses.replace(fvK, node=np.asarray(kf["node"], np.int32))
    np.testing.assert_array_equal(fvK.node, kf["node"]); np.testing.assert_array_equal(fvK.feature, kf["feature"])
    nd = common_nodes(fvK, fvF)
    valid = (np.asarray(kf["point_id"]) >= 0).astype(np.uint8)
    out = ORBmatcher(gpu_ctx, 0.7, True).SearchByBoWFrame(RS.keyframe_frame(kf), sc["frame"], nd, valid)
    qk = out.query_kp if len(out.query_kp) else np.zeros(1, np.int64)       # (no common node: no query, no owner)
    slot = np.where(out.owner >= 0, qk[np.maximum(out.owner, 0)], -1)
    pad = lambda a, dt: np.concatenate([np.asarray(a, dt), np.zeros((1,) + np.asarray(a).shape[1:], dt)])   # (an empty keyframe: nothing to gather from)
    kf_id, kf_world, kf_obs = pad(kf["point_id"], np.int32), pad(kf["world_pos"], np.float32), pad(kf["has_obs"], np.uint8)
    ids = np.where(slot >= 0, kf_id[np.maximum(slot, 0)], -1).astype(np.int32)
    assert out.n_matches == g1["n_search"]
    np.testing.assert_array_equal(ids, g1["kp_point_id"])
    keep = (ids >= 0) & (e1["kp_outlier"] == 0)                           # the reference's PoseOptimization and discard
    world = np.where(keep[:, None], kf_world[np.maximum(slot, 0)], 0).astype(np.float32)
    obs = np.where(keep, kf_obs[np.maximum(slot, 0)], 0).astype(np.uint8)
    seen = ids[(ids >= 0) & (e1["kp_outlier"] != 0)]
    T = host.se3_to_tcw_f32(gpu_ctx.lib, e1["pose_qt"]) if e1["n_point_edges"] >= 3 else S["Tcw_last"]
    with open_frame(gpu_ctx, S) as tf:
        tf.set_state(T, np.where(keep, ids, -1).astype(np.int32), world, obs, np.zeros(len(ids), np.uint8), seen)
        tf.track_local_map(sc["map_points"], sc["map_ids"], sc.get("local_lines"))
        _, h2 = tf.download()
    for k in ("kp_point_id", "kp_outlier", "ln_line_id", "ln_outlier", "mp_in_view"):
        np.testing.assert_array_equal(h2[k], g2[k], err_msg=k)
    for k in COUNTERS:
        assert h2[k] == g2[k], (k, h2[k], g2[k])


def test_handle_is_reusable(gpu_ctx, vocs):
    """Twice on one frame, and after a TrackWithMotionModel on the same handle: bit-identical records."""
    S = RS.make_scene("main"); sc = S["sc"]; voc = vocs(S)
    with open_frame(gpu_ctx, S) as tf:
        first = run_chain(tf, S, voc)[1:]
        second = run_chain(tf, S, voc)[1:]
        tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc.get("last_lines"))
        tf.track_local_map(sc["map_points"], sc["map_ids"], sc.get("local_lines"))
        mm = tf.download()
        tf.track_reference_keyframe(S["Tcw_last"], S["kf"])               # the FeatureVector of the first compute_bow is still the frame's
        tf.track_local_map(sc["map_points"], sc["map_ids"], sc.get("local_lines"))
        third = tf.download()
    assert mm[0]["n_search"] > 0 and first[0]["n_search"] >= 15
    for other in (second, third):
        for a, b in zip(first, other):
            same_record(a, b, exact_pose=True)


def test_frame_built_on_the_device(gpu_ctx):
    """A frame of lld_frame_build_stereo_keypoints gives the records of the same frame uploaded with lld_frame_create."""
    import bow_ref
    sc = synth.make_stereo_scene(2, n=300, width=416, height=240)
    L = sc["L"]
    fx = float(np.float32(sc["mbf"]) / np.float32(sc["mb"]))
    cam = (fx, fx, 208.0, 120.0, float(sc["mbf"]))
    V = bow_ref.make_vocab(77, k=4, L=3)
    rng = np.random.default_rng(77)
    built = orb_search.build_stereo_frame_keypoints(gpu_ctx.lib, gpu_ctx.handle, L, sc["R"], sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    st = built.download()
    F2 = dataclasses.replace(L, uright=st.u_right.copy()).normalise()
    has = np.nonzero(st.depth > 0)[0]
    assert len(has) > 60
    z = st.depth[has].astype(np.float64)
    world = np.stack([(L.xy[has, 0] - cam[2]) * z / fx, (L.xy[has, 1] - cam[3]) * z / fx, z], 1).astype(np.float32)
    kf = dict(desc=RS.flip_bits(rng, L.desc[has], 4), angle=L.angle[has].copy(), point_id=np.arange(len(has), dtype=np.int32), world_pos=world)
    RS.add_feature_vector(kf, bow_ref.Tree(V), 1)
    T = np.eye(4, dtype=np.float32); T[:3, 3] = [0.03, -0.01, 0.02]
    recs = []
    with ORBVocabulary(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=1, max_features=512) as voc:
        for tf in (DeviceTrackedFrame.from_stereo_build(gpu_ctx, built, cam), DeviceTrackedFrame(gpu_ctx, F2, cam)):
            with tf:
                bow = tf.compute_bow(voc, 1, host=True)
                tf.track_reference_keyframe(T, kf)
                recs.append((bow, tf.download(stage2=False)[0]))
    for f in BOW_FIELDS:
        np.testing.assert_array_equal(getattr(recs[0][0], f), getattr(recs[1][0], f), err_msg=f)
    same_record(recs[0][1], recs[1][1], exact_pose=True)
    assert recs[0][1]["n_search"] >= 15 and recs[0][1]["n_points"] >= 10


def test_refusals(gpu_ctx, vocs, expected):
    """Every refusal returns LLD_ERR_INVALID before anything is queued and leaves the frame as it was: the valid call that follows is right."""
    import ctypes as C
    from lld_slam_amd import Context
    S = RS.make_scene("main"); sc = S["sc"]; kf = S["kf"]; voc = vocs(S)
    V = S["vocab"]

    def bad(**kw):
        d = dict(kf)
        for k, v in kw.items(): d[k] = v
        return d
    with open_frame(gpu_ctx, S) as tf:
        raw_bow = gpu_ctx.lib.fn("frame_compute_bow"); raw = gpu_ctx.lib.fn("frame_track_reference_keyframe")
        with pytest.raises(RuntimeError):
            tf.track_reference_keyframe(S["Tcw_last"], kf)                # no lld_frame_compute_bow yet
        # compute_bow: nulls, another context's vocabulary, more keypoints than the vocabulary takes
        assert raw_bow(None, voc.handle, 1, None) == abi.LLD_ERR_INVALID and raw_bow(tf.res.handle, None, 1, None) == abi.LLD_ERR_INVALID
        with Context(0) as other:
            with ORBVocabulary(other, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=1, max_features=512) as v2:
                assert raw_bow(tf.res.handle, v2.handle, 1, None) == abi.LLD_ERR_INVALID
        with ORBVocabulary(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=1, max_features=sc["frame"].n - 1) as small:
            assert raw_bow(tf.res.handle, small.handle, 1, None) == abi.LLD_ERR_INVALID
        with pytest.raises(RuntimeError):
            tf.track_reference_keyframe(S["Tcw_last"], kf)                # none of those gave the frame a FeatureVector
        tf.compute_bow(voc, S["levelsup"])
        view = orb_search.frame_view(S["Tcw_last"], sc["cam"], sc["frame"])
        qt = np.ascontiguousarray(host.se3_from_tcw_f32(gpu_ctx.lib, S["Tcw_last"]), np.float64)
        assert raw(tf.res.handle, C.byref(tf.params), C.byref(view), qt.ctypes.data_as(abi.c_double_p), None) == abi.LLD_ERR_INVALID      # a null kf
        feat = np.array(kf["feature"]); feat_hi = feat.copy(); feat_hi[3] = len(kf["angle"]); feat_lo = feat.copy(); feat_lo[0] = -1
        node_eq = np.array(kf["node"]); node_eq[2] = node_eq[1]
        node_desc = np.array(kf["node"])[::-1].copy()
        start_bad = np.array(kf["node_start"]); start_bad[1] = start_bad[2] + 1
        too_many = orb_search.MAX_KEYPOINTS + 1
        for d in (bad(feature=feat_hi), bad(feature=feat_lo), bad(node=node_eq), bad(node=node_desc), bad(node_start=start_bad),
                  bad(desc=np.zeros((too_many, 8), np.uint32), angle=np.zeros(too_many, np.float32), point_id=np.full(too_many, -1, np.int32),
                      world_pos=np.zeros((too_many, 3), np.float32), has_obs=None)):
            with pytest.raises(RuntimeError):
                tf.track_reference_keyframe(S["Tcw_last"], d)
        K, keep = ref_keyframe_struct(kf)
        K.n = -1
        assert raw(tf.res.handle, C.byref(tf.params), C.byref(view), qt.ctypes.data_as(abi.c_double_p), C.byref(K)) == abi.LLD_ERR_INVALID
        fx = tf.params.cam.fx
        tf.params.cam.fx = 0.0
        with pytest.raises(RuntimeError):
            tf.track_reference_keyframe(S["Tcw_last"], kf)
        tf.params.cam.fx = fx; fy = tf.params.cam.fy; tf.params.cam.fy = -1.0
        with pytest.raises(RuntimeError):
            tf.track_reference_keyframe(S["Tcw_last"], kf)
        tf.params.cam.fy = fy
        tf.track_reference_keyframe(S["Tcw_last"], kf)                    # and now the valid call
        tf.track_local_map(sc["map_points"], sc["map_ids"], sc.get("local_lines"))
        g1, g2 = tf.download()
        # a frame without level_inv_sigma2 (PoseOptimization's information) is refused; the same frame with it is taken: nothing else differs
        F = sc["frame"]
        K, keep = ref_keyframe_struct(kf)
        status = {}
        for with_sigma2 in (False, True):
            p = orb_search.prepare(F, np.zeros((0, 8), np.uint32), candidates=orb_search.CAND_GRID, accept_max=orb_search.TH_HIGH)
            if not with_sigma2: p.s.level_inv_sigma2 = None
            h = C.c_void_p()
            assert gpu_ctx.lib.fn("frame_create")(gpu_ctx.handle, C.byref(p.s), C.byref(h)) == abi.LLD_OK
            try:
                assert raw_bow(h, voc.handle, S["levelsup"], None) == abi.LLD_OK
                status[with_sigma2] = raw(h, C.byref(tf.params), C.byref(view), qt.ctypes.data_as(abi.c_double_p), C.byref(K))
            finally:
                gpu_ctx.lib.fn("frame_destroy")(h)
        assert status == {False: abi.LLD_ERR_INVALID, True: abi.LLD_OK}, status
    same_record(g1, expected["main"][0]); same_record(g2, expected["main"][1])
