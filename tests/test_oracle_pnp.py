"""tests/pnp_ref.py on its own: the rand() stream against the machine's glibc, EPnP on exact data, SetRansacParameters' budget
with its float truncations, and iterate()'s quirks (the || loop, Refine's strict >, N < minInliers).  CPU only."""
import ctypes
import math

import numpy as np
import pytest

import pnp_ref as P


@pytest.mark.parametrize("seed", [0, 1, 2, 7, 12345, 2**31 - 1, 2**31 + 5, 2**32 - 1])
def test_stream_equals_glibc_rand(seed):
    libc = ctypes.CDLL("libc.so.6")
    libc.rand.restype = ctypes.c_int
    libc.srand(ctypes.c_uint(seed))
    want = [libc.rand() for _ in range(1000)]
    assert P.glibc_rand_sequence(seed, 1000) == want


def test_seed_zero_acts_as_one():
    assert P.glibc_rand_sequence(0, 50) == P.glibc_rand_sequence(1, 50)


def _exact(sc):
    xyz = sc["xyz"].astype(np.float64)
    Xc = xyz @ sc["R"].T + sc["t"]
    uv = np.stack([sc["fx"] * Xc[:, 0] / Xc[:, 2] + sc["cx"], sc["fy"] * Xc[:, 1] / Xc[:, 2] + sc["cy"]], 1)
    return xyz, uv


@pytest.mark.parametrize("n", [5, 6, 12, 50, 400])
def test_epnp_exact_on_noise_free_points(n):
    sc = P.make_scene(100 + n, n, variant="exact")
    xyz, uv = _exact(sc)
    R, t, err = P.compute_pose(xyz, uv, sc["fx"], sc["fy"], sc["cx"], sc["cy"])
    assert np.abs(R - sc["R"]).max() < 1e-9 and np.abs(t - sc["t"]).max() < 1e-9 * max(1.0, np.abs(sc["t"]).max())
    assert err < 1e-8


def test_epnp_minimal_sets_on_noise_free_points():
    """With 4 points the 5 Gauss-Newton steps from the crude beta approximations do not always converge (a property of the
    reference's EPnP, whatever the basis); the ones that do give the true pose to 1e-9, and they are not rare."""
    sc = P.make_scene(5, 60, variant="exact")
    xyz, uv = _exact(sc)
    rng = np.random.default_rng(0)
    good = 0
    for _ in range(40):
        idx = rng.choice(60, 4, replace=False)
        R, t, _ = P.compute_pose(xyz[idx], uv[idx], sc["fx"], sc["fy"], sc["cx"], sc["cy"])
        good += np.abs(R - sc["R"]).max() < 1e-9 and np.abs(t - sc["t"]).max() < 1e-8
    assert good >= 5


def test_null_basis_is_orthonormal_null_space():
    rng = np.random.default_rng(1)
    M = rng.normal(size=(8, 12))
    B = np.array(P.householder_null4([[float(M[r][a]) for r in range(8)] for a in range(12)]))
    assert np.abs(M @ B.T).max() < 1e-14 and np.abs(B @ B.T - np.eye(4)).max() < 1e-14


def test_find_on_noise_free_scene():
    sc = P.make_scene(9, 300, variant="exact")
    s = P.solver_from_scene(sc)
    o = s.find()
    assert o["Tcw"] is not None and o["n_inliers"] == 300
    assert np.abs(o["Tcw"][:, :3] - sc["R"]).max() < 1e-5 and np.abs(o["Tcw"][:, 3] - sc["t"]).max() < 1e-4
    assert o["inliers"][sc["kp_index"]].all() and o["inliers"].sum() == 300


@pytest.mark.parametrize("N", [4, 9, 10, 19, 20, 21, 2000])
def test_budget_formula(N):
    mi, its, eps = P.ransac_constants(N)
    want_min = max(int(np.float32(N) * np.float32(0.5)), 10, 4)
    assert mi == want_min
    e = np.float32(0.5)
    if e < np.float32(want_min) / np.float32(N):
        e = np.float32(want_min) / np.float32(N)
    assert eps == e
    if want_min == N:
        assert its == 1
    elif want_min > N:                                      # epsilon > 1: the quotient is NaN, (int)NaN is INT_MIN -> 1
        assert its == 1
    else:
        assert its == max(1, min(300, math.ceil(math.log(1 - 0.99) / math.log(1 - float(e) ** 3))))
    if N == 2000:
        assert (mi, its) == (1000, 35)
    if N == 10:
        assert (mi, its) == (10, 1)
    if N == 20:
        assert (mi, its) == (10, 35)
    if N == 21:
        assert mi == 10 and eps == np.float32(0.5)


def test_float_truncation_of_min_inliers():
    # int nMinInliers = N*mRansacEpsilon multiplies in float: 100 * 0.29f is 29.0f, while the double product 28.999999999999996
    # would truncate to 28.
    assert int(100 * 0.29) == 28
    assert P.ransac_constants(100, 0.99, 4, 300, 4, 0.29)[0] == 29


def test_or_loop_runs_n_more_after_budget():
    sc = P.make_scene(11, 60, inlier_ratio=0.05)          # nothing refines: the budget is spent
    s = P.solver_from_scene(sc)
    o = s.iterate(s.max_its)
    assert o["no_more"] and s.n_iterations == s.max_its
    s.iterate(5)
    assert s.n_iterations == s.max_its + 5 and len(s.hyps) == 5


def test_refine_needs_strictly_more_than_min_inliers():
    sc = P.make_scene(12, 30, variant="exact")
    s = P.solver_from_scene(sc, (0.99, 30, 300, 4, 0.5, 5.991))
    assert s.min_inliers == 30 and s.max_its == 1
    o = s.iterate(5)                                        # every hypothesis that converges has 30 inliers: never > 30
    assert all(h[0] <= 30 for h in s.hyps) and all(not r for r in s.refines)
    assert o["no_more"]
    if s.best_inliers == 30:
        assert o["Tcw"] is not None and o["n_inliers"] == 30
    s2 = P.solver_from_scene(sc, (0.99, 29, 300, 4, 0.5, 5.991))
    o2 = s2.find()
    assert o2["Tcw"] is not None and o2["n_inliers"] == 30 and any(s2.refines)


def test_too_few_correspondences_draws_nothing():
    sc = P.make_scene(13, 8)
    s = P.solver_from_scene(sc)
    before = list(s.rng.ring)
    o = s.iterate(5)
    assert o["no_more"] and o["Tcw"] is None and s.n_iterations == 0 and s.rng.ring == before and s.hyps == []
