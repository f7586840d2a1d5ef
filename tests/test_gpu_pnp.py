"""lld_pnp_* (PnPsolver on the device) against the restatement tests/pnp_ref.py, over whole Relocalization-style rounds of
iterate(5): per hypothesis (inlier counts identical; R and t within 1e-9 relative for every eligible one) and per call (has_pose,
Tcw as float bits within 1 ulp, vbInliers, nInliers, bNoMore, mnIterations identical).  A count difference is only reported
together with the correspondences whose error2 lies within one float ulp of their threshold; the test still fails on it."""
import numpy as np
import pytest

import pnp_ref as P
from lld_slam_amd import abi
from lld_slam_amd.pnp import PnPError, PnPsolver, PnPsolverBatch

pytestmark = pytest.mark.gpu


def near_threshold(ref, R, t):
    _, _, e2 = ref._check(R, t)
    thr = ref.max_error.astype(np.float32)
    close = np.abs(e2.astype(np.float64) - thr) <= np.spacing(thr).astype(np.float64)
    return np.flatnonzero(close)


def ulp_equal(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib).max() <= 1


def compare_call(ref, out_ref, got, hyps, what):
    nw, nr, recs = hyps
    assert nr == len(ref.hyps), f"{what}: iterations run {nr} vs {len(ref.hyps)}"
    for k, (cnt, R, t) in enumerate(ref.hyps):
        h = recs[k]
        if h["n_inliers"] != cnt:
            pts = near_threshold(ref, R, t)
            pytest.fail(f"{what}: hypothesis {k} count {h['n_inliers']} vs {cnt}; correspondences within 1 ulp of the threshold: {pts}")
        if cnt >= ref.min_inliers:
            scale = max(1.0, np.abs(R).max())
            assert np.abs(h["R"] - R).max() <= 1e-9 * scale, f"{what}: hypothesis {k} R"
            assert np.abs(h["t"] - t).max() <= 1e-9 * max(1.0, np.abs(t).max()), f"{what}: hypothesis {k} t"
    assert got.no_more == out_ref["no_more"], what
    assert got.iterations == ref.n_iterations, what
    assert got.best_inliers == ref.best_inliers, what
    assert (got.Tcw is None) == (out_ref["Tcw"] is None), what
    if got.Tcw is not None:
        assert ulp_equal(got.Tcw, out_ref["Tcw"]), f"{what}: Tcw {got.Tcw} vs {out_ref['Tcw']}"
    assert got.n_inliers == out_ref["n_inliers"], what
    assert np.array_equal(got.inliers, out_ref["inliers"]), what


def run_rounds(ctx, scenes, params=(0.99, 10, 300, 4, 0.5, 5.991), n=5, active0=None,
               skip=None, max_rounds=80):
    refs = [P.solver_from_scene(sc, params) for sc in scenes]
    live = [True] * len(scenes) if active0 is None else list(active0)
    with PnPsolverBatch(ctx, scenes, params) as b:
        for rnd in range(max_rounds):
            act = list(live)
            if skip is not None:
                act = [a and not skip(rnd, i) for i, a in enumerate(act)]
            if not any(act):
                if not any(live):
                    break
                continue
            outs = b.iterate(n, act)
            for i, on in enumerate(act):
                if not on:
                    continue
                o = refs[i].iterate(n)
                compare_call(refs[i], o, outs[i], b.hypotheses(i), f"round {rnd} solver {i}")
                if o["no_more"]:
                    live[i] = False
    return refs


CASES = [(4, 0.9, None), (15, 0.9, None), (50, 0.9, None), (50, 0.6, None), (200, 0.6, None), (200, 0.3, None),
         (1000, 0.6, None), (2000, 0.9, None), (8192, 0.6, None), (60, 0.6, "coplanar"), (80, 0.6, "behind"),
         (90, 0.6, "duplicate"), (40, 1.0, "exact"), (12, 1.0, "collapsed")]


@pytest.mark.parametrize("n,ratio,variant", CASES)
def test_rounds_match_restatement(gpu_ctx, n, ratio, variant):
    sc = P.make_scene(1000 + n + int(ratio * 10), n, ratio, variant=variant)
    run_rounds(gpu_ctx, [sc])


def test_low_inlier_ratio_exhausts_budget(gpu_ctx):
    sc = P.make_scene(77, 300, 0.3)
    refs = run_rounds(gpu_ctx, [sc])
    assert refs[0].n_iterations >= refs[0].max_its


def test_batch_of_40_mixed_candidates(gpu_ctx):
    rng = np.random.default_rng(5)
    scenes = []
    for i in range(40):
        n = int(rng.integers(4, 400))
        ratio = float(rng.choice([0.9, 0.6, 0.3]))
        variant = [None, None, None, "coplanar", "behind", "duplicate"][i % 6]
        scenes.append(P.make_scene(2000 + i, n, ratio, variant=variant))
    run_rounds(gpu_ctx, scenes)
    # the same candidates each alone on the device: identical outputs round by round
    with PnPsolverBatch(gpu_ctx, scenes) as b:
        alone = [PnPsolverBatch(gpu_ctx, [sc]) for sc in scenes[:8]]
        for _ in range(4):
            outs = b.iterate(5)
            for i, a in enumerate(alone):
                o = a.iterate(5)[0]
                g = outs[i]
                assert (o.Tcw is None) == (g.Tcw is None) and o.iterations == g.iterations and o.no_more == g.no_more
                assert o.n_inliers == g.n_inliers and np.array_equal(o.inliers, g.inliers)
                if o.Tcw is not None:
                    assert np.array_equal(o.Tcw.view(np.uint32), g.Tcw.view(np.uint32))
        for a in alone:
            a.close()


def test_active_masks_skip_solvers(gpu_ctx):
    scenes = [P.make_scene(3000 + i, 150, [0.3, 0.6, 0.9][i % 3]) for i in range(9)]
    run_rounds(gpu_ctx, scenes, skip=lambda rnd, i: (rnd + i) % 3 == 0)


def test_find_matches_restatement(gpu_ctx):
    for seed, n, ratio in [(1, 100, 0.6), (2, 500, 0.3), (3, 30, 0.9)]:
        sc = P.make_scene(4000 + seed, n, ratio)
        ref = P.solver_from_scene(sc)
        o = ref.find()
        with PnPsolver(gpu_ctx, sc) as s:
            g = s.find()
        assert (g.Tcw is None) == (o["Tcw"] is None) and g.n_inliers == o["n_inliers"]
        assert g.iterations == ref.n_iterations and np.array_equal(g.inliers, o["inliers"])
        if g.Tcw is not None:
            assert ulp_equal(g.Tcw, o["Tcw"])


def test_too_few_correspondences(gpu_ctx):
    sc = P.make_scene(9, 8)
    with PnPsolver(gpu_ctx, sc) as s:
        g = s.iterate(5)
        assert g.no_more and g.Tcw is None and g.iterations == 0 and g.n_inliers == 0 and not g.inliers.any()
        assert s.hypotheses(0)[:2] == (0, 0)


def _refused(ctx, scenes, params=(0.99, 10, 300, 4, 0.5, 5.991)):
    with pytest.raises(PnPError) as e:
        PnPsolverBatch(ctx, scenes, params)
    return e.value.status


def test_refusals(gpu_ctx):
    base = P.make_scene(10, 40)
    assert _refused(gpu_ctx, [base], (0.99, 10, 300, 5, 0.5, 5.991)) == abi.LLD_ERR_UNSUPPORTED
    assert _refused(gpu_ctx, [base], (0.99, 10, 0, 4, 0.5, 5.991)) == abi.LLD_ERR_INVALID
    assert _refused(gpu_ctx, [base], (0.99, 10, 65537, 4, 0.5, 5.991)) == abi.LLD_ERR_INVALID
    assert _refused(gpu_ctx, [base] * 257) == abi.LLD_ERR_UNSUPPORTED
    big = P.make_scene(11, 8193, n_keypoints=8193)
    assert _refused(gpu_ctx, [big]) == abi.LLD_ERR_UNSUPPORTED
    many_kp = dict(base, n_keypoints=8193)
    assert _refused(gpu_ctx, [many_kp]) == abi.LLD_ERR_UNSUPPORTED
    bad = dict(base, kp_index=np.where(np.arange(40) == 3, base["n_keypoints"], base["kp_index"]).astype(np.int32))
    assert _refused(gpu_ctx, [bad]) == abi.LLD_ERR_INVALID
    dup = dict(base, kp_index=np.concatenate([base["kp_index"][:39], base["kp_index"][:1]]).astype(np.int32))
    assert _refused(gpu_ctx, [dup]) == abi.LLD_ERR_INVALID
    neg = dict(base, kp_index=np.concatenate([[-1], base["kp_index"][1:]]).astype(np.int32))
    assert _refused(gpu_ctx, [neg]) == abi.LLD_ERR_INVALID
    assert _refused(gpu_ctx, [dict(base, fx=0.0)]) == abi.LLD_ERR_INVALID
    assert _refused(gpu_ctx, [dict(base, fy=-1.0)]) == abi.LLD_ERR_INVALID
    assert _refused(gpu_ctx, []) == abi.LLD_ERR_INVALID
    with PnPsolverBatch(gpu_ctx, [base]) as b:
        for n, st in [(0, abi.LLD_ERR_INVALID), (-3, abi.LLD_ERR_INVALID), (65537, abi.LLD_ERR_UNSUPPORTED)]:
            with pytest.raises(PnPError) as e:
                b.iterate(n)
            assert e.value.status == st
        o = b.iterate(5)[0]                                   # a refused call changed nothing
        ref = P.solver_from_scene(base)
        r = ref.iterate(5)
        assert o.iterations == ref.n_iterations and o.n_inliers == r["n_inliers"]


def test_refine_over_exactly_four_inliers(gpu_ctx):
    """min_inliers 4 and N <= 9 give nMinInliers = 4, so a best set of 4 reaches Refine: its basis is the minimal-set QR one."""
    params = (0.99, 4, 300, 4, 0.5, 5.991)
    scenes = [P.make_scene(5000 + i, 6 + i % 4, 0.5) for i in range(24)]
    refs = run_rounds(gpu_ctx, scenes, params=params)
    assert any(4 in r.refine_sizes for r in refs)


def test_find_continues_the_solver_state(gpu_ctx):
    """find() after iterate() continues the same solver, as the reference's find() does."""
    for seed, n, ratio in [(1, 120, 0.3), (2, 300, 0.6)]:
        sc = P.make_scene(6000 + seed, n, ratio)
        ref = P.solver_from_scene(sc)
        r1 = ref.iterate(5)
        r2 = ref.find()
        with PnPsolver(gpu_ctx, sc) as s:
            g1 = s.iterate(5)
            g2 = s.find()
        for g, o in ((g1, r1), (g2, r2)):
            assert (g.Tcw is None) == (o["Tcw"] is None) and g.n_inliers == o["n_inliers"] and g.no_more == o["no_more"]
            assert np.array_equal(g.inliers, o["inliers"])
            if g.Tcw is not None:
                assert ulp_equal(g.Tcw, o["Tcw"])
        assert g2.iterations == ref.n_iterations
