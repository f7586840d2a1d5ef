"""tests/initializer_ref.py pinned on the CPU: the sample stream against glibc rand() values, ground truth on noise-free scenes,
the branch every named scene must take (with its margin), and the Jacobi-based null vectors / SVD against numpy.linalg.svd."""
import numpy as np
import pytest

import initializer_ref as I
from pnp_ref import glibc_rand_sequence


def test_sets_follow_the_glibc_stream():
    assert glibc_rand_sequence(1, 3) == [1804289383, 846930886, 1681692777]     # rand() after srand(1)
    N, its = 37, 5
    sets = I.build_sets(N, its, 0)                                              # seed 0 is srand(1)
    r = glibc_rand_sequence(1, 8 * its)
    k = 0
    for it in range(its):
        avail = list(range(N))
        for j in range(8):
            i = int(r[k] / 2147483648.0 * len(avail)); k += 1
            assert sets[it, j] == avail[i]
            avail[i] = avail[-1]; avail.pop()
        assert len(set(sets[it])) == 8
    assert not np.array_equal(I.build_sets(N, its, 7), sets)


def _run(variant, n=400, ratio=0.9, seed=21, **kw):
    sc = I.make_scene(seed, n, ratio, variant=variant)
    ref = I.ref_from_scene(sc, **kw)
    return sc, ref, ref.initialize(sc["keys2"], sc["matches12"])


def test_exact_general_scene_recovers_the_truth():
    sc, ref, o = _run("exact", 300)
    assert o["success"] and o["model"] == 1 and o["RH"] < 0.25
    assert np.abs(o["R21"] - sc["R21"]).max() < 1e-4
    t = sc["t21"] / np.linalg.norm(sc["t21"])
    assert np.abs(o["t21"] - t).max() < 1e-3                                    # the sign is fixed by the cheirality test
    tri = o["triangulated"].astype(bool)
    assert tri.sum() > 0.9 * 300
    scale = 1.0 / np.linalg.norm(sc["t21"])                                     # |t21| = 1 fixes the scale
    assert np.abs(o["p3d"][tri] - sc["X1"][tri] * scale).max() < 2e-2 * np.abs(sc["X1"][tri] * scale).max()


def test_general_takes_F_and_planar_takes_H_with_margin():
    _, _, g = _run("general")
    assert g["model"] == 1 and g["RH"] < 0.25 and g["success"]
    assert sorted(g["n_good"][:4])[-2] < 0.35 * max(g["n_good"][:4])            # far from the 0.7 similarity bound
    assert max(g["n_good"][:4]) > 0.97 * g["n_inliers_F"] and max(g["n_good"][:4]) > 300   # against 0.9*N and 50
    assert g["parallax"][g["best_index"]] > 3.0                                 # far from minParallax = 1
    # A plane is fitted by F as well as by H, and F's one-dimensional error scores at least as much per match, so RH of a plane
    # stays just below 0.5: 0.45 is the margin there is against 0.40.  Faugeras' second physical solution reconstructs about 0.62
    # of the points on this plane (tilted 40 degrees, 8 m away); 0.68 keeps a clear distance from the 0.75 bound.
    sc, _, p = _run("planar")
    assert p["model"] == 0 and p["RH"] > 0.45 and p["success"]
    good = sorted(int(x) for x in p["n_good"])
    assert good[-2] < 0.68 * good[-1]
    assert good[-1] > 0.97 * p["n_inliers_H"] and good[-1] > 300                # against 0.9*N and minTriangulated = 50
    assert p["parallax"][p["best_index"]] > 3.0                                 # against minParallax = 1
    assert np.abs(p["R21"] - sc["R21"]).max() < 0.02


def test_no_winner_in_either_model_gives_zeros():
    """Every keypoint of frame 2 at one pixel: every score is NaN, `>` never holds, neither model has a winner, RH is 0/0 and
    falls to F, which has no matrix to reconstruct from.  The result is all zeros with success false and no motion run."""
    sc, ref, o = _run("collapsed", 60)
    assert all(np.isnan(h["score"]) for h in ref.hyps_H + ref.hyps_F)
    assert (o["win_H"], o["win_F"]) == (-1, -1) and o["SH"] == 0 and o["SF"] == 0 and np.isnan(o["RH"])
    assert o["model"] == 1 and not o["success"] and o["best_index"] == -1 and ref.motions == []
    assert not o["H21"].any() and not o["F21"].any() and o["n_inliers_H"] == 0 and o["n_inliers_F"] == 0
    assert not o["inlier_H"].any() and not o["inlier_F"].any() and not o["n_good"].any() and not o["parallax"].any()
    assert not o["R21"].any() and not o["t21"].any() and not o["p3d"].any() and not o["triangulated"].any()


def test_pure_rotation_fails_on_parallax():
    _, _, o = _run("rotation")
    assert not o["success"]
    assert o["n_good"].max() > 300 and o["parallax"][:4].max() < 0.6


def test_all_wrong_matches_fail():
    _, _, o = _run("wrong", 200)
    assert not o["success"]


def test_eight_matches_run():
    _, ref, o = _run("exact", 8)
    assert o["n_matches"] == 8 and sorted(ref.sets[0]) == list(range(8))


@pytest.mark.parametrize("shape", [(3, 3), (8, 9), (16, 9), (4, 4)])
def test_jacobi_null_vector_and_svd_against_numpy(shape):
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    A = rng.normal(0, 1, (50,) + shape).astype(np.float32)
    if shape == (4, 4):
        A[:, 3] = A[:, 0] - 2 * A[:, 1]                                         # give it a null space
    x = I.null_vector_batch(A)
    for a, v in zip(A, x):
        U, w, Vt = np.linalg.svd(a.astype(np.float64))
        ref = Vt[-1]
        gap = (w[-2] - w[-1]) / w[0]
        assert min(np.abs(v - ref).max(), np.abs(v + ref).max()) < 1e-5 / max(gap, 1e-3)
    if shape == (3, 3):
        U, w, Vt = I.svd3(A)
        for a, u, s, vt in zip(A, U, w, Vt):
            assert np.allclose(s, np.linalg.svd(a.astype(np.float64), compute_uv=False), rtol=1e-5, atol=1e-6)
            assert np.abs(u @ np.diag(s) @ vt - a).max() < 1e-5
            assert np.abs(u.T @ u - np.eye(3)).max() < 1e-5
        B = A.copy(); B[:, :, 2] = B[:, :, 0] + B[:, :, 1]                      # rank 2: U is completed
        B[0] = 0; B[1, :, 1] = 2 * B[1, :, 0]                                   # rank 0 and rank 1
        U, w, Vt = I.svd3(B)
        for a, u, s, vt in zip(B, U, w, Vt):
            assert np.abs(u @ np.diag(s) @ vt - a).max() < 1e-5
            assert np.abs(u.T @ u - np.eye(3)).max() < 1e-5
            assert abs(abs(np.linalg.det(u.astype(np.float64))) - 1) < 1e-5
