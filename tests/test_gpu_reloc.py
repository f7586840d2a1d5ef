"""lld_frame_relocalize: Tracking::Relocalization (src/Tracking.cc:1837-1998) as one call on the device-resident chain, against the CPU
reference's own run of the routine (tests/reloc_ref.py) on the scenes of tests/reloc_scenes.py - one per exit; tests/test_oracle_reloc_scenes.py
holds the scenes to their exits and margins.  The record's integers, the ids and the flags are exact; the pose stays within the bar the
chain's stage 1 is held to (test_gpu_track_chain.POSE_TOL, as tests/test_gpu_track_refkf.py applies it)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import reloc_ref as RF
import reloc_scenes as RS2
from lld_slam_amd import abi, host, orb_search, synth
from lld_slam_amd.tracking import DeviceTrackedFrame, ref_keyframe_struct, relocalize_call_by_call
from lld_slam_amd.vocabulary import ORBVocabulary
from test_gpu_track_chain import COUNTERS, POSE_TOL, same_record

pytestmark = pytest.mark.gpu

INTS = ("matched", "winner", "round", "n_good", "n_rounds", "n_kept")
PER_CANDIDATE = ("n_bow", "discarded", "rounds", "n_good_last", "rungs", "n_additional1", "n_additional2")


@pytest.fixture(scope="module")
def vocs(gpu_ctx):
    made = {}

    def get(S):
        if S["name"] not in made:
            V = S["vocab"]
            made[S["name"]] = ORBVocabulary(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=2, max_features=512)
        return made[S["name"]]
    yield get
    for v in made.values():
        v.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """The reference's run of every scene, computed once."""
    return {name: RF.relocalize(RS2.make_scene(name)) for name in RS2.NAMES}


def open_frame(gpu_ctx, S):
    return DeviceTrackedFrame(gpu_ctx, S["sc"]["frame"], S["sc"]["cam"])


def run(tf, S, voc, candidates=None, seeds=None):
    tf.compute_bow(voc, S["levelsup"])
    return tf.relocalize(S["candidates"] if candidates is None else candidates, S["seeds"] if seeds is None else seeds, S["Tcw0"], S["pnp"])


def same_integers(g, e, what=""):
    for k in INTS:
        assert g[k] == e[k], (what, k, g[k], e[k])
    for k in PER_CANDIDATE:
        np.testing.assert_array_equal(g[k], e[k], err_msg=f"{what} {k}")


@pytest.mark.parametrize("name", RS2.NAMES)
def test_against_the_reference(gpu_ctx, vocs, expected, name):
    S = RS2.make_scene(name); e = expected[name]
    with open_frame(gpu_ctx, S) as tf:
        g = run(tf, S, vocs(S))
        r1 = tf.download(stage2=False)[0]
    print(name, {k: (g[k], e[k]) for k in INTS}, {k: (g[k].tolist(), e[k].tolist()) for k in PER_CANDIDATE})
    same_integers(g, e, name)
    np.testing.assert_array_equal(r1["kp_point_id"], e["kp_point_id"]); np.testing.assert_array_equal(r1["kp_outlier"], e["kp_outlier"])
    if e["matched"]:
        dq = float(np.max(np.abs(r1["pose_qt"][:4] - e["pose_qt"][:4])))
        dt = float(np.linalg.norm(r1["pose_qt"][4:] - e["pose_qt"][4:]) / max(1.0, np.linalg.norm(e["pose_qt"][4:])))
        print(name, "dq", dq, "dt", dt)
        assert dq <= POSE_TOL and dt <= POSE_TOL, (dq, dt)
        np.testing.assert_array_equal(g["Tcw"], host.se3_to_tcw_f32(gpu_ctx.lib, r1["pose_qt"]))      # mTcw = Converter::toCvMat of the optimised pose
        held = e["kp_point_id"] >= 0
        assert r1["n_inliers"] == e["n_good"] and r1["n_points"] == int(held.sum()) and r1["n_points_map"] == int((held & (e["kp_obs"] != 0)).sum())
        assert r1["n_search"] == e["n_bow"][e["winner"]] and r1["n_lines"] == 0 and r1["n_discarded"] == 0
    else:
        np.testing.assert_array_equal(g["Tcw"], np.asarray(S["Tcw0"], np.float32).reshape(4, 4))      # the pose handed in
        assert r1["n_points"] == 0 and r1["n_inliers"] == 0


@pytest.mark.parametrize("name", RS2.NAMES)
def test_equals_the_call_by_call_route(gpu_ctx, vocs, name):
    """INTEGRATION.md section 11's call-by-call recipe on the same context: the same integers, ids and flags."""
    S = RS2.make_scene(name); voc = vocs(S)
    with open_frame(gpu_ctx, S) as tf:
        g = run(tf, S, voc)
        r1 = tf.download(stage2=False)[0]
    h = relocalize_call_by_call(gpu_ctx, voc, S["levelsup"], S["sc"]["frame"], S["sc"]["cam"], S["candidates"], S["seeds"], S["pnp"])
    same_integers(g, h, name)
    np.testing.assert_array_equal(r1["kp_point_id"], h["kp_point_id"]); np.testing.assert_array_equal(r1["kp_outlier"], h["kp_outlier"])


@pytest.mark.parametrize("name", ("keeps_outliers", "late_round"))
def test_track_local_map_follows(gpu_ctx, vocs, expected, name):
    """lld_frame_track_local_map straight after relocalize = the same call after lld_frame_track_set_state with the reference's state."""
    S = RS2.make_scene(name); sc = S["sc"]; e = expected[name]
    assert e["matched"]
    with open_frame(gpu_ctx, S) as tf:
        run(tf, S, vocs(S))
        tf.track_local_map(sc["map_points"], sc["map_ids"])
        _, g2 = tf.download()
    with open_frame(gpu_ctx, S) as tf:
        tf.set_state(e["Tcw"], e["kp_point_id"], e["kp_world"], e["kp_obs"], e["kp_outlier"])
        tf.track_local_map(sc["map_points"], sc["map_ids"])
        _, h2 = tf.download()
    assert g2["n_search"] > 0 and g2["n_inliers"] >= 50
    for k in ("kp_point_id", "kp_outlier", "mp_in_view"):
        np.testing.assert_array_equal(g2[k], h2[k], err_msg=k)
    for k in COUNTERS:
        assert g2[k] == h2[k], (k, g2[k], h2[k])


def test_handle_is_reusable(gpu_ctx, vocs, expected):
    """Relocalize twice with different candidates, then a motion-model frame on the same handle."""
    S = RS2.make_scene("second_wins_same_round"); sc = S["sc"]; voc = vocs(S)
    swapped = [S["candidates"][1], S["candidates"][0]]
    with open_frame(gpu_ctx, S) as tf:
        a = run(tf, S, voc); a1 = tf.download(stage2=False)[0]
        b = run(tf, S, voc, swapped, [S["seeds"][1], S["seeds"][0]]); b1 = tf.download(stage2=False)[0]
        tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"])
        tf.track_local_map(sc["map_points"], sc["map_ids"])
        mm = tf.download()
        c = run(tf, S, voc); c1 = tf.download(stage2=False)[0]
    with open_frame(gpu_ctx, S) as tf:
        tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"])
        tf.track_local_map(sc["map_points"], sc["map_ids"])
        fresh = tf.download()
    same_integers(a, expected["second_wins_same_round"])
    assert (b["matched"], b["winner"], b["round"]) == (1, 0, 1) and b["rounds"].tolist() == [1, 0]      # the winner came first this time: the other is never reached
    np.testing.assert_array_equal(a1["kp_point_id"], b1["kp_point_id"]); np.testing.assert_array_equal(a1["pose_qt"], b1["pose_qt"])
    for x, y in zip(mm, fresh):
        same_record(x, y, exact_pose=True)
    same_integers(c, a)
    same_record(c1, a1, exact_pose=True)


def test_frame_built_on_the_device(gpu_ctx):
    """A frame of lld_frame_build_stereo_keypoints gives the record of the same frame uploaded with lld_frame_create."""
    import bow_ref
    import refkf_scenes as RS
    sc = synth.make_stereo_scene(2, n=300, width=416, height=240)
    L = sc["L"]
    fx = float(np.float32(sc["mbf"]) / np.float32(sc["mb"]))
    cam = (fx, fx, 208.0, 120.0, float(sc["mbf"]))
    V = bow_ref.make_vocab(77, k=4, L=3)
    rng = np.random.default_rng(78)
    built = orb_search.build_stereo_frame_keypoints(gpu_ctx.lib, gpu_ctx.handle, L, sc["R"], sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    st = built.download()
    F2 = dataclasses.replace(L, uright=st.u_right.copy()).normalise()
    has = np.nonzero(st.depth > 0)[0]
    assert len(has) > 80
    z = st.depth[has].astype(np.float64)
    world = np.stack([(L.xy[has, 0] - cam[2]) * z / fx, (L.xy[has, 1] - cam[3]) * z / fx, z], 1).astype(np.float32)
    dist = np.linalg.norm(world, axis=1)
    maxd = (dist * 1.2 ** L.octave[has]).astype(np.float32)
    kf = dict(desc=RS.flip_bits(rng, L.desc[has], 4), angle=L.angle[has].copy(), point_id=np.arange(len(has), dtype=np.int32), world_pos=world,
              max_distance=maxd, min_distance=(maxd / 1.2 ** 7).astype(np.float32))
    RS.add_feature_vector(kf, bow_ref.Tree(V), 1)
    recs = []
    with ORBVocabulary(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=1, max_features=512) as voc:
        for tf in (DeviceTrackedFrame.from_stereo_build(gpu_ctx, built, cam), DeviceTrackedFrame(gpu_ctx, F2, cam)):
            with tf:
                tf.compute_bow(voc, 1)
                recs.append((tf.relocalize([kf], [5]), tf.download(stage2=False)[0]))
    same_integers(recs[0][0], recs[1][0])
    same_record(recs[0][1], recs[1][1], exact_pose=True)
    assert recs[0][0]["n_kept"] == 1 and recs[0][0]["rounds"][0] >= 1 and recs[0][0]["rungs"][0] & abi.RELOC_RUNG_POSE1      # the routine ran: a pose and its ladder


def test_refusals(gpu_ctx, vocs, expected):
    """Every refusal is decided on the host before a launch, returns LLD_ERR_INVALID and leaves the frame usable: the valid call that follows is right."""
    S = RS2.make_scene("first_wins"); sc = S["sc"]; voc = vocs(S); cands = S["candidates"]
    V = S["vocab"]

    def bad(i, **kw):
        out = [dict(c) for c in cands]
        out[i].update(kw)
        return out
    with open_frame(gpu_ctx, S) as tf:
        raw = gpu_ctx.lib.fn("frame_relocalize")
        with pytest.raises(RuntimeError):
            tf.relocalize(cands, S["seeds"], S["Tcw0"])                                      # no lld_frame_compute_bow yet
        tf.compute_bow(voc, S["levelsup"])
        view = orb_search.frame_view(S["Tcw0"], sc["cam"], sc["frame"])
        qt = np.ascontiguousarray(host.se3_from_tcw_f32(gpu_ctx.lib, S["Tcw0"]), np.float64)
        K, keep = ref_keyframe_struct(cands[0])
        kfs = (abi.RefKeyFrame * 1)(K); ex = (abi.RelocCandidate * 1)()
        maxd = np.ascontiguousarray(cands[0]["max_distance"], np.float32); mind = np.ascontiguousarray(cands[0]["min_distance"], np.float32)
        ex[0].max_distance = maxd.ctypes.data_as(abi.c_float_p); ex[0].min_distance = mind.ctypes.data_as(abi.c_float_p); ex[0].seed = S["seeds"][0]
        prm = abi.PnPParams(); gpu_ctx.lib.fn("pnp_params_default")(C.byref(prm))
        res = abi.RelocResult()
        args = lambda **kw: [kw.get("frame", tf.res.handle), kw.get("params", C.byref(tf.params)), kw.get("view", C.byref(view)), kw.get("qt", qt.ctypes.data_as(abi.c_double_p)),
                             kw.get("n", 1), kw.get("kfs", kfs), kw.get("ex", ex), kw.get("prm", C.byref(prm)), kw.get("res", C.byref(res))]
        for kw in (dict(frame=None), dict(params=None), dict(view=None), dict(qt=None), dict(kfs=None), dict(ex=None), dict(prm=None), dict(res=None),
                   dict(n=0), dict(n=-1), dict(n=257)):
            assert raw(*args(**kw)) == abi.LLD_ERR_INVALID, kw
        feat = np.array(cands[1]["feature"]); feat_hi = feat.copy(); feat_hi[3] = len(cands[1]["angle"])
        node_eq = np.array(cands[1]["node"]); node_eq[2] = node_eq[1]
        start_bad = np.array(cands[1]["node_start"]); start_bad[1] = start_bad[2] + 1
        for c in (bad(1, feature=feat_hi), bad(1, node=node_eq), bad(1, node_start=start_bad), bad(2, max_distance=None), bad(0, min_distance=None)):
            with pytest.raises(RuntimeError):
                tf.relocalize(c, S["seeds"], S["Tcw0"])
        for k_, v in (("epsilon", 0.0), ("max_iterations", 0), ("probability", 1.0), ("th2", -1.0)):
            with pytest.raises(RuntimeError):
                tf.relocalize(cands, S["seeds"], S["Tcw0"], {k_: v})
        fx = tf.params.cam.fx
        tf.params.cam.fx = 0.0
        with pytest.raises(RuntimeError):
            tf.relocalize(cands, S["seeds"], S["Tcw0"])
        tf.params.cam.fx = fx; fy = tf.params.cam.fy; tf.params.cam.fy = -1.0
        with pytest.raises(RuntimeError):
            tf.relocalize(cands, S["seeds"], S["Tcw0"])
        tf.params.cam.fy = fy
        g = tf.relocalize(cands, S["seeds"], S["Tcw0"], S["pnp"])                            # and now the valid call
        r1 = tf.download(stage2=False)[0]
        # a frame without level_inv_sigma2, and one without angles, is refused; the same frame with both is taken and gives the same record
        status = {}
        for what in ("no_inv_sigma2", "no_angle", "complete"):
            p = orb_search.prepare(sc["frame"], np.zeros((0, 8), np.uint32), candidates=orb_search.CAND_GRID, accept_max=orb_search.TH_HIGH)
            if what == "no_inv_sigma2": p.s.level_inv_sigma2 = None
            if what == "no_angle": p.s.t_angle = None
            h = C.c_void_p()
            assert gpu_ctx.lib.fn("frame_create")(gpu_ctx.handle, C.byref(p.s), C.byref(h)) == abi.LLD_OK
            try:
                assert gpu_ctx.lib.fn("frame_compute_bow")(h, voc.handle, S["levelsup"], None) == abi.LLD_OK
                status[what] = raw(*args(frame=h))
            finally:
                gpu_ctx.lib.fn("frame_destroy")(h)
        assert status == {"no_inv_sigma2": abi.LLD_ERR_INVALID, "no_angle": abi.LLD_ERR_INVALID, "complete": abi.LLD_OK}, status
        assert (res.matched, res.winner, res.n_good) == (1, 0, expected["first_wins"]["n_good"])      # (candidate 0 alone with its seed: it wins as it does among three)
    same_integers(g, expected["first_wins"])
    np.testing.assert_array_equal(r1["kp_point_id"], expected["first_wins"]["kp_point_id"])
