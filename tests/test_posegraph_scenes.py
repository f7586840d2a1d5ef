"""CPU: the essential graphs of tests/posegraph_scenes.py reach the paths of the tile Cholesky that synth's band graphs never do,
the witness (an independent tile-level symbolic factorisation) agrees with a numeric Cholesky, and the oracle closes their loops."""
import numpy as np
import pytest

import posegraph_scenes as S
from lld_slam_amd import synth


def test_witness_is_the_pattern_of_a_numeric_cholesky():
    """On a random SPD matrix with the block pattern of a scene's H, the tiles of the numeric factor that are not zero are exactly
    the witness's pattern (generic values: no cancellation)."""
    rng = np.random.default_rng(7)
    for name in ("short_free", "reparented"):
        gr, _ = S.scene(name)
        hidx = S.unknown_index(gr); nu = int((hidx >= 0).sum()); n = 7 * nu; NT = (n + 15) // 16
        H = np.zeros((16 * NT, 16 * NT))
        for i, j in zip(gr.edge_i, gr.edge_j):
            a, b = hidx[i], hidx[j]
            if a >= 0 and b >= 0 and a != b:
                B = rng.normal(size=(7, 7)); H[7 * a:7 * a + 7, 7 * b:7 * b + 7] += B; H[7 * b:7 * b + 7, 7 * a:7 * a + 7] += B.T
        H += np.diag(np.abs(H).sum(1) + 1.0)                       # diagonally dominant; the padding rows are the identity
        L = np.linalg.cholesky(H)
        nz = np.abs(L).reshape(NT, 16, NT, 16).max(axis=(1, 3)) > 0
        np.testing.assert_array_equal(nz, S.symbolic_cholesky(S.tile_pattern(gr)))


def test_band_graphs_of_synth_have_no_fill():
    """Why the scenes exist: synth's graphs (loop edge onto the fixed keyframe 0) factor without a single fill tile."""
    for gid, n, covis in ((0, 120, 3), (3, 300, 3), (1, 120, 6)):
        w = S.witness(synth.make_essential_graph(gid, n, covis=covis))
        assert w["fill"] == 0 and w["max_k"] <= 3 and w["back_groups"] == 1 and w["i_lt_j"] == 0 and w["fixed"] == [0]


def test_scenes_reach_their_paths():
    w = {name: S.witness(S.scene(name)[0]) for name in S.SCENES}
    for name, x in w.items():
        assert len(S.scene(name)[0].fixed) <= 300
        assert x["fill"] > 0, name                                 # the symbolic merge creates tiles the assembly did not have
        assert x["max_k"] >= 4 and x["back_groups"] >= 2, name     # wavefront 3, q > 0, more than one back-substitution workgroup
        assert 0 not in x["fixed"] or len(x["fixed"]) > 1, name    # a fixed vertex away from keyframe 0
    for name in ("mid_loop", "many_to_many", "three_laps", "reparented", "fixed_many"):
        assert w[name]["max_k"] >= 17, name                        # the second pass of pg_chol_col's k0 loop
    assert w["reparented"]["i_lt_j"] > 20
    fixed = w["fixed_many"]["fixed"]
    gr, _ = S.scene("fixed_many")
    assert len(fixed) >= 3 and 17 in fixed
    assert 7 * (S.unknown_index(gr)[:17] >= 0).sum() % 16 == 0     # the unknowns before keyframe 17 end on a tile boundary
    lc = S.scene("many_to_many")[0]
    assert len(set(zip(lc.edge_i[:72].tolist(), lc.edge_j[:72].tolist()))) == 72 and (lc.fixed[lc.edge_j[:72]] == 0).sum() >= 64


def test_reversed_edges_reach_both_orders():
    gr, _ = S.scene("mid_loop")
    rv, flip = S.reverse_edges(gr, seed=1)
    assert 0.4 < flip.mean() < 0.6
    assert (rv.edge_i < rv.edge_j).sum() == flip.sum()
    # reversing twice gives the same graph back
    back, _ = S.reverse_edges(rv, seed=1)
    np.testing.assert_array_equal(back.edge_i, gr.edge_i)
    np.testing.assert_allclose(back.edge_sji, gr.edge_sji, atol=1e-12)


def test_padding_graphs_cover_every_residue():
    residues = set()
    for nu in S.PADDING_SIZES:
        gr = S.make_padding_graph(nu)
        hidx = S.unknown_index(gr)
        assert int((hidx >= 0).sum()) == nu
        residues.add((7 * nu) % 16)
        if nu >= 3:
            assert any(hidx[i] >= 0 and hidx[j] >= 0 and abs(int(i) - int(j)) == nu - 1 for i, j in zip(gr.edge_i, gr.edge_j))
    assert residues == set(range(16))


@pytest.mark.parametrize("name", ["mid_loop", "many_to_many"])
def test_oracle_closes_the_loop_of_the_scenes(oracle, name):
    """Like test_essential_graph_closes_the_loop: the keyframes between pLoopKF and the corrected tail move toward the ground
    truth (relative to the fixed pLoopKF) and pLoopKF stays put."""
    gr, fix = S.scene(name)
    o = oracle.optimize_essential_graph(gr, bFixScale=fix)
    lk, n, nc = gr.meta["loop_kf"], len(gr.fixed), gr.meta["n_corrected"]
    before = S.relative_error(gr.sim3, gr.meta["gt"], lk)[lk + 1:n - nc].mean()
    after = S.relative_error(o.sim3, gr.meta["gt"], lk)[lk + 1:n - nc].mean()
    assert after < 0.5 * before, (before, after)
    np.testing.assert_array_equal(o.sim3[lk], gr.sim3[lk])
    assert o.chi2 < 0.05 and o.lm_iterations >= 2
