"""The Sim3Solver restatement (tests/sim3solver_ref.py) checked on its own: Horn against the generator's truth and against an
Umeyama / SVD solve, the truncated thresholds, the RANSAC budget, and iterate()'s loop rules (AND condition, the return before
the bNoMore test, ties replacing the best, draws per iteration).  CPU only."""
import math

import numpy as np
import pytest

import sim3solver_ref as S
from pnp_ref import GlibcRand


def _truth(sc):
    return sc["s12"] * sc["R12"], sc["t12"]


@pytest.mark.parametrize("fix", [False, True])
def test_horn_recovers_s12_on_noise_free_data(fix):
    sc = S.make_scene(11, 60, 1.0, fix_scale=fix, variant="exact")
    ref = S.solver_from_scene(sc)
    sR, t = _truth(sc)
    rng = np.random.default_rng(0)
    for _ in range(40):
        idx = list(rng.choice(ref.N, 3, replace=False))
        h = ref.hypothesis(idx)
        assert np.abs(h["T12"][:, :3] - sR).max() < 1e-5
        assert abs(float(h["s"]) - sc["s12"]) < 1e-5 * sc["s12"]
        assert np.abs(h["R"] - sc["R12"]).max() < 1e-5
        assert np.abs(h["t"] - t).max() < 1e-5 * 30.0            # points up to 30 m away: float positions carry ~1e-6 m
        # T21 is the inverse of T12
        T12 = np.vstack([h["T12"].astype(np.float64), [0, 0, 0, 1]]); T21 = np.vstack([h["T21"].astype(np.float64), [0, 0, 0, 1]])
        assert np.abs(T12 @ T21 - np.eye(4)).max() < 1e-5


def _umeyama(src, dst, with_scale):
    """dst ~ s R src + t (Umeyama 1991), in double."""
    mu_s, mu_d = src.mean(0), dst.mean(0)
    xs, xd = src - mu_s, dst - mu_d
    C = xd.T @ xs
    U, D, Vt = np.linalg.svd(C)
    E = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        E[2, 2] = -1
    R = U @ E @ Vt
    s = np.trace(np.diag(D) @ E) / (xs * xs).sum() if with_scale else 1.0
    return R, s, mu_d - s * R @ mu_s


@pytest.mark.parametrize("fix", [False, True])
def test_horn_agrees_with_umeyama_on_three_points(fix):
    sc = S.make_scene(12, 200, 0.5, fix_scale=fix)             # noisy points and outliers: a least-squares fit, not an exact one
    ref = S.solver_from_scene(sc)
    rng = np.random.default_rng(1)
    for _ in range(60):
        idx = list(rng.choice(ref.N, 3, replace=False))
        h = ref.hypothesis(idx)
        R, s, t = _umeyama(ref.X2[idx].astype(np.float64), ref.X1[idx].astype(np.float64), not fix)
        scale = max(1.0, float(np.abs(ref.X1[idx]).max()))
        assert np.abs(h["R"] - R).max() < 2e-4
        assert abs(float(h["s"]) - s) < 2e-4 * s
        assert np.abs(h["t"] - t).max() < 2e-4 * scale


def test_thresholds_are_truncated():
    assert S.max_error([1.0, 1.44, 2.0736, 2.986]).tolist() == [9.0, 13.0, 19.0, 27.0]
    assert S.max_error(S.LEVEL_SIGMA2).tolist() == [float(int(9.210 * float(s))) for s in S.LEVEL_SIGMA2]
    assert S.max_error(S.LEVEL_SIGMA2)[:4].tolist() == [9.0, 13.0, 19.0, 27.0]


def test_iteration_budget():
    table = {20: 1, 21: 3, 40: 35, 15: 1, 0: 1}
    for N, want in table.items():
        assert S.ransac_constants(N) == want, N
    assert S.ransac_constants(200) == 300                        # ceil(...) = 4603, capped by maxIterations
    assert S.ransac_constants(40, max_iterations=10) == 10
    eps = np.float32(20) / np.float32(40)
    assert S.ransac_constants(40) == math.ceil(math.log(1 - 0.99) / math.log(1 - float(eps) ** 3))


def _advanced(seed, draws):
    g = GlibcRand(seed)
    for _ in range(draws):
        g.rand()
    return g


def test_each_iteration_draws_three():
    sc = S.make_scene(13, 200, 0.1)
    ref = S.solver_from_scene(sc)
    o = ref.iterate(5)
    assert o["T12"] is None and len(ref.hyps) == 5
    assert ref.rng.ring == _advanced(sc["seed"], 15).ring and ref.rng.head == _advanced(sc["seed"], 15).head


def test_and_loop_draws_nothing_after_the_budget():
    sc = S.make_scene(14, 200, 0.1)
    ref = S.solver_from_scene(sc, (0.99, 20, 7))
    outs = [ref.iterate(5) for _ in range(3)]
    assert ref.n_iterations == 7
    assert [o["no_more"] for o in outs] == [False, True, True]
    ring, head = list(ref.rng.ring), ref.rng.head
    o = ref.iterate(5)
    assert ref.hyps == [] and o["no_more"] and o["T12"] is None and ref.n_iterations == 7
    assert ref.rng.ring == ring and ref.rng.head == head


def test_success_on_the_last_budgeted_iteration_is_not_no_more():
    sc = S.make_scene(15, 21, 1.0, variant="exact")             # every sample fits all 21 > 20 correspondences
    ref = S.solver_from_scene(sc, (0.99, 20, 1))
    o = ref.iterate(5)
    assert ref.max_its == 1 and ref.n_iterations == 1
    assert o["T12"] is not None and o["n_inliers"] == 21 and not o["no_more"]
    assert o["inliers"][sc["index1"]].all() and o["inliers"].sum() == 21
    o = ref.iterate(5)
    assert o["no_more"] and o["T12"] is None and o["n_inliers"] == 0 and not o["inliers"].any()


def test_n_at_and_below_min_inliers():
    ref = S.solver_from_scene(S.make_scene(16, 20, 1.0, variant="exact"))
    o = ref.iterate(5)                                            # budget 1; 20 inliers are not > 20
    assert ref.n_iterations == 1 and o["no_more"] and o["T12"] is None and ref.best_inliers == 20
    sc = S.make_scene(17, 15, 1.0, variant="exact")
    ref = S.solver_from_scene(sc)
    o = ref.iterate(5)
    assert o["no_more"] and ref.hyps == [] and ref.n_iterations == 0
    assert ref.rng.ring == GlibcRand(sc["seed"]).ring


def test_ties_replace_the_best_and_identity_is_nan():
    ref = S.solver_from_scene(S.make_scene(18, 50, 1.0, variant="identity"))
    ref.iterate(5)
    assert [h["n_inliers"] for h in ref.hyps] == [0] * 5 and all(h["record"] for h in ref.hyps)
    assert ref.best is ref.hyps[-1]                               # >=: the last of equal counts is the best
    assert np.isnan(ref.best["R"]).all() and np.isnan(ref.best["T12"]).all()


def test_first_hypothesis_is_best_even_with_no_inliers():
    ref = S.solver_from_scene(S.make_scene(19, 100, 0.0))
    ref.iterate(1)
    assert ref.best is ref.hyps[0] and ref.best_inliers == ref.hyps[0]["n_inliers"]


def test_find_continues_the_state():
    sc = S.make_scene(20, 300, 0.2)
    a = S.solver_from_scene(sc)
    a.iterate(5); a.iterate(5)
    o = a.find()                                                  # iterate(mRansacMaxIts) from mnIterations = 10
    assert a.n_iterations == min(a.max_its, 10 + len(a.hyps)) and (o["T12"] is not None or a.n_iterations == a.max_its)
