"""The numpy restatement of the loop-closing thread's three map corrections (tests/loopcorr_ref.py) against itself and against known
answers: the batched rule the device follows equals the reference's interleaved loop, an identity correction moves nothing, a pure
scale doubles, and the global-BA walk on a tree of optimised keyframes copies their poses.  CPU only."""
import numpy as np

import loopcorr_ref as R
import loopcorr_scenes as S

f32 = np.float32
OUTS = ("corrected_sim3", "non_corrected_sim3", "tiw_corrected", "ow_corrected", "scw_f32", "pos", "corrected_by", "normal",
        "min_distance", "max_distance", "updated")


def test_batched_rule_equals_the_literal_loop_on_200_scenes():
    """owner = the smallest rank and the centre chosen by rank, against :474-518 with SetPose interleaved: every output, bit for bit.
    The rank rule is not vacuous: with the centres on entry alone some normals come out different."""
    rank_rule_mattered = 0
    for seed in range(200):
        n_conn = 1 + seed % 5
        sc = S.make_loop_scene(seed, n_kf=5 + seed % 4, n_conn=n_conn, cur_rank=(seed // 5) % n_conn, per_kf=10, s=[1.0, 0.7, 1.3][seed % 3])
        lit, bat = R.correct_loop_literal(sc), R.correct_loop_batched(sc)
        for k in OUTS:
            assert R.bits_equal(lit[k], bat[k]), (seed, k)
        old_only = R.loop_normals(sc, np.where(bat["corrected_by"] >= 0, 0, -1), bat["pos"], bat["ow_corrected"])
        rank_rule_mattered += not R.bits_equal(old_only[0], lit["normal"])
    assert rank_rule_mattered > 100


def test_identity_correction_keeps_poses_and_positions():
    """mg2oScw = the current keyframe's own pose as a Sim3 with s = 1: CorrectedSiw = Sic*Scw is every keyframe's own pose again.  The
    poses return equal up to the float roundings of Tic = Tiw*Twc (each entry off by 2^-24 relative: the rotation by 2^-24, tic by
    2^-24 |tic| <= 2^-24 2 tmax, Ow inside Twc by 2^-24 tmax), which Ric*tcw + tic sums to less than 2^-24 (3 + 2 + 2) tmax < 2^-21 tmax
    with tmax the longest translation of the scene.  The positions return up to the float roundings of Tic = Tiw*Twc, which CorrectedSiw carries and Siw does not: each of its entries is
    off by half a float ulp, 2^-24 relative, so a coordinate is off by at most 2^-24 (3 max|P| + max|t|) per map, and there are two
    maps and the final rounding: 2^-22 (3 max|P| + max|t|) bounds it.  (Exactly representable poses give equal bits: next test.)"""
    for seed in range(5):
        sc = S.make_loop_scene(seed, n_kf=8, n_conn=5, cur_rank=seed % 5, per_kf=12)
        # orthonormal poses: the float rotation of a real map is only orthonormal to float rounding, and the test is about this code
        for k in range(len(sc["kf_tcw"])):
            q, t, _ = R.sim3_of_pose(sc["kf_tcw"][k])
            nq = np.sqrt(sum(x * x for x in q))
            sc["kf_tcw"][k] = R.se3_of_sim3(([x / nq for x in q], t, 1.0))
        cur = sc["kf_tcw"][sc["conn"][sc["cur"]]]
        sc["scw"] = R.sim3_flat(R.sim3_of_pose(cur))
        out = R.correct_loop_literal(sc)
        tmax = max(1.0, np.sqrt((sc["kf_tcw"][:, [3, 7, 11]].astype(np.float64) ** 2).sum(1)).max())
        for r, k in enumerate(sc["conn"]):
            assert np.abs(out["tiw_corrected"][r].astype(np.float64) - sc["kf_tcw"][k]).max() <= 2.0 ** -21 * tmax, (seed, r)
        moved = out["corrected_by"] >= 0
        assert moved.any()
        bound = 2.0 ** -22 * (3 * np.abs(sc["pos"]).max() + np.abs(sc["kf_tcw"][:, [3, 7, 11]]).max())
        assert np.abs(out["pos"][moved].astype(np.float64) - sc["pos"][moved]).max() <= bound


def test_identity_sim3_exactly():
    """The textbook case, exact in floating point: every pose the identity rotation with a translation, mg2oScw = the current pose,
    s = 1.  Then every product is exact: every pose comes back equal, and every position within 1 float ulp - in fact equal."""
    sc = S.make_loop_scene(3, n_kf=6, n_conn=4, cur_rank=1, per_kf=10)
    for k in range(6):
        sc["kf_tcw"][k] = np.array([1, 0, 0, k - 2.0, 0, 1, 0, 0.5 * k, 0, 0, 1, -0.25 * k], f32)
    sc["pos"] = np.round(sc["pos"] * 64) / f32(64)             # a few bits only: the sums stay exact
    sc["scw"] = R.sim3_flat(R.sim3_of_pose(sc["kf_tcw"][sc["conn"][1]]))
    out = R.correct_loop_literal(sc)
    assert np.array_equal(out["tiw_corrected"], sc["kf_tcw"][sc["conn"]])
    assert R.ulp_steps(out["pos"], sc["pos"]).max() <= 1 and np.array_equal(out["pos"], sc["pos"])
    assert (out["corrected_by"] >= 0).any()


def test_pure_scale_doubles_the_positions_owned_by_cur():
    """The current keyframe at the identity pose and a pure scale about the origin.  The points cur owns are mapped by
    CorrectedSwc = mg2oScw^-1 after Siw = identity, so it is the scale of Swc that multiplies them: Swc with s = 2 (mg2oScw with
    s = 0.5) doubles every position exactly, and mg2oScw with s = 2 halves it.  The corrected pose is the identity either way
    (t/s = 0)."""
    for s, factor in ((2.0, 0.5), (0.5, 2.0)):
        sc = S.make_loop_scene(1, n_kf=6, n_conn=3, cur_rank=0, per_kf=10)
        sc["kf_tcw"][sc["conn"][0]] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32)
        sc["scw"] = np.array([0, 0, 0, 1, 0, 0, 0, s])
        out = R.correct_loop_literal(sc)
        mine = out["corrected_by"] == 0
        assert mine.sum() >= 5
        assert R.bits_equal(out["pos"][mine], (sc["pos"][mine] * f32(factor)).astype(f32))
        assert R.bits_equal(out["tiw_corrected"][0], np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32))


def test_essential_graph_identity_and_normals_use_new_centres():
    sc = S.make_graph_scene(2)
    same = dict(sc); same["sim3_after"] = sc["sim3_before"]
    out = R.essential_graph_literal(same)
    ok = sc["bad"] == 0
    assert R.ulp_steps(out["pos"][ok], sc["pos"][ok]).max() <= 1
    out = R.essential_graph_literal(sc)
    n, mn, mx, did = R.graph_normals(sc, out["pos"], out["ow"])
    assert R.bits_equal(n, out["normal"]) and R.bits_equal(mn, out["min_distance"]) and R.bits_equal(mx, out["max_distance"])
    assert np.array_equal(did, (out["updated"] & 2) != 0) and np.array_equal((out["updated"] & 1) != 0, ok)


def test_global_ba_tree_of_optimised_keyframes():
    """Only optimised keyframes below the origins: tcw_new == tcw_gba, and a point that Global BA did not optimise is moved by
    T_new^-1 T_before (checked in double to float accuracy)."""
    sc = S.make_gba_scene(4, n_chains=0)
    sc["kf_in_gba"][sc["unvisited"]] = 0
    out = R.global_ba_literal(sc)
    vis = out["visited"] != 0
    assert vis.sum() == len(vis) - 2 and not vis[sc["unvisited"]].any()
    assert R.bits_equal(out["tcw_new"][vis], sc["kf_tcw_gba"][vis]) and R.bits_equal(out["tcw_before"][vis], sc["kf_tcw"][vis])
    two = np.flatnonzero(out["moved"] == 2)
    assert len(two) > 20 and (out["moved"][:4] == 0).all() and (out["moved"][sc["bad"] != 0] == 0).all()
    assert R.bits_equal(out["pos"][out["moved"] == 1], sc["pos_gba"][out["moved"] == 1])
    for p in two:
        r = sc["ref_kf"][p]
        Tb = sc["kf_tcw"][r].astype(np.float64).reshape(3, 4); Tn = sc["kf_tcw_gba"][r].astype(np.float64).reshape(3, 4)
        Xc = (Tb[:, :3] * sc["pos"][p].astype(np.float64)[None]).sum(1) + Tb[:, 3]
        want = (Tn[:, :3].T * (Xc - Tn[:, 3])[None]).sum(1)
        assert np.allclose(out["pos"][p], want, rtol=0, atol=2e-5), p


def test_global_ba_chains_compose_top_down():
    """A keyframe Global BA did not see takes (Tchild*Twc_parent)*mTcwGBA_parent from its parent's NEW mTcwGBA, depth by depth."""
    sc = S.make_gba_scene(5)
    out = R.global_ba_literal(sc)
    n_kf = len(sc["parent"])
    depth = np.zeros(n_kf, int)
    for k in np.flatnonzero(out["visited"]):
        d, c = 0, k
        while not sc["kf_in_gba"][c]:
            c = sc["parent"][c]; d += 1
        depth[k] = d
        if d:
            par = sc["parent"][k]
            want = R.mul44(R.mul44(sc["kf_tcw"][k], R.inverse_of(sc["kf_tcw"][par])), out["tcw_new"][par])
            assert R.bits_equal(out["tcw_new"][k], want)
    assert {1, 2, 3} <= set(depth.tolist())
