"""lld_sim3solver_* (Sim3Solver on the device) against the restatement tests/sim3solver_ref.py, over whole LoopClosing-style
rounds of iterate(5): per hypothesis (inlier counts identical; for every hypothesis that becomes a best, sR / t / s within 1 float
ulp) and per call (has_pose, T12 within 1 ulp, vbInliers, nInliers, bNoMore, mnIterations, mnBestInliers identical).  A count
difference is only reported together with the correspondences whose error lies within one float ulp of their threshold; the test
still fails on it.  Also: the chain into lld_optimize_sim3 and every refusal."""
import ctypes as C

import numpy as np
import pytest

import sim3solver_ref as S
from lld_slam_amd import Optimizer, abi
from lld_slam_amd.host import Sim3Pair
from lld_slam_amd.sim3solver import Sim3Solver, Sim3SolverBatch, Sim3SolverError, problem_from_scene

pytestmark = pytest.mark.gpu


def ulps(a, b):
    """Largest distance in float ulps (NaN == NaN)."""
    a = np.asarray(a, np.float32).reshape(-1); b = np.asarray(b, np.float32).reshape(-1)
    both_nan = np.isnan(a) & np.isnan(b)
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia); ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.where(both_nan, 0, np.abs(ia - ib))
    return int(d.max()) if d.size else 0


def near_threshold(ref, h):
    _, _, e1, e2 = ref.check(h)
    out = []
    for e, thr in ((e1, ref.err1), (e2, ref.err2)):
        out.append(np.flatnonzero(np.abs(e.astype(np.float64) - thr) <= np.spacing(thr).astype(np.float64)))
    return out


def compare_call(ref, out_ref, got, hyps, what):
    nw, nr, recs = hyps
    assert nr == len(ref.hyps), f"{what}: iterations run {nr} vs {len(ref.hyps)}"
    for k, h in enumerate(ref.hyps):
        g = recs[k]
        assert g["idx"] == h["idx"], f"{what}: hypothesis {k} sample {g['idx']} vs {h['idx']}"
        if g["n_inliers"] != h["n_inliers"]:
            pytest.fail(f"{what}: hypothesis {k} count {g['n_inliers']} vs {h['n_inliers']}; correspondences within 1 ulp of "
                        f"the thresholds (err1, err2): {near_threshold(ref, h)}")
        assert bool(g["record"]) == bool(h["record"]), f"{what}: hypothesis {k} record"
        if h["record"]:
            assert ulps(g["T12"], h["T12"]) <= 1, f"{what}: hypothesis {k} sR|t {g['T12']} vs {h['T12']}"
            assert ulps(g["R"], h["R"]) <= 1 and ulps(g["t"], h["t"]) <= 1 and ulps(g["s"], h["s"]) <= 1, f"{what}: hypothesis {k}"
    assert got.no_more == out_ref["no_more"], what
    assert got.iterations == ref.n_iterations, what
    assert got.best_inliers == ref.best_inliers, what
    assert (got.T12 is None) == (out_ref["T12"] is None), what
    if got.T12 is not None:
        assert ulps(got.T12, out_ref["T12"]) <= 1, f"{what}: T12 {got.T12} vs {out_ref['T12']}"
    assert got.n_inliers == out_ref["n_inliers"], what
    assert np.array_equal(got.inliers, out_ref["inliers"]), what
    if ref.best is not None:                                  # GetEstimatedRotation / Translation / Scale
        assert ulps(got.R, ref.best["R"]) <= 1 and ulps(got.t, ref.best["t"]) <= 1 and ulps(got.s, ref.best["s"]) <= 1, what


def run_rounds(ctx, scenes, params=S.DEFAULT_PARAMS, n=5, active0=None, skip=None, max_rounds=40):
    refs = [S.solver_from_scene(sc, params) for sc in scenes]
    live = [True] * len(scenes) if active0 is None else list(active0)
    with Sim3SolverBatch(ctx, scenes, params) as b:
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


CASES = [(n, r, fix) for n in (20, 21, 40, 200, 1000, 8192) for r in (0.9, 0.5, 0.2) for fix in (False, True)]


@pytest.mark.parametrize("n,ratio,fix", CASES)
def test_rounds_match_restatement(gpu_ctx, n, ratio, fix):
    sc = S.make_scene(100 + n + int(ratio * 10) + 7 * fix, n, ratio, fix_scale=fix)
    run_rounds(gpu_ctx, [sc], max_rounds=12 if n >= 1000 else 40)


VARIANTS = [(60, "exact"), (60, "collinear"), (90, "duplicate"), (80, "behind"), (50, "identity")]


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("n,variant", VARIANTS)
def test_variants_match_restatement(gpu_ctx, n, variant, fix):
    sc = S.make_scene(500 + n, n, 0.6, fix_scale=fix, variant=variant)
    refs = run_rounds(gpu_ctx, [sc])
    if variant == "identity":                                 # every rotation NaN: no inliers, and the first hypothesis is the best
        assert refs[0].best_inliers == 0 and np.isnan(refs[0].best["R"]).all()


def test_n_equal_and_below_min_inliers(gpu_ctx):
    eq = S.make_scene(31, 20, 1.0, variant="exact")           # N == minInliers: budget 1, 20 inliers are not > 20
    below = S.make_scene(32, 15, 1.0, variant="exact")        # N < minInliers: bNoMore with no draws
    refs = run_rounds(gpu_ctx, [eq, below])
    assert refs[0].max_its == 1 and refs[0].n_iterations == 1
    assert refs[1].n_iterations == 0


def test_batch_of_40_mixed_candidates(gpu_ctx):
    rng = np.random.default_rng(5)
    scenes = []
    for i in range(40):
        n = int(rng.integers(20, 600))
        ratio = float(rng.choice([0.9, 0.5, 0.2]))
        variant = [None, None, None, "collinear", "behind", "duplicate", "exact", "identity"][i % 8]
        scenes.append(S.make_scene(2000 + i, n, ratio, fix_scale=bool(i % 2), variant=variant))
    run_rounds(gpu_ctx, scenes)
    # the same candidates each alone on the device: identical outputs round by round
    with Sim3SolverBatch(gpu_ctx, scenes) as b:
        alone = [Sim3SolverBatch(gpu_ctx, [sc]) for sc in scenes[:8]]
        for _ in range(4):
            outs = b.iterate(5)
            for i, a in enumerate(alone):
                o = a.iterate(5)[0]
                g = outs[i]
                assert (o.T12 is None) == (g.T12 is None) and o.iterations == g.iterations and o.no_more == g.no_more
                assert o.n_inliers == g.n_inliers and np.array_equal(o.inliers, g.inliers)
                if o.T12 is not None:
                    assert np.array_equal(o.T12.view(np.uint32), g.T12.view(np.uint32))
        for a in alone:
            a.close()


def test_active_masks_skip_solvers(gpu_ctx):
    scenes = [S.make_scene(3000 + i, 150, [0.2, 0.5, 0.9][i % 3], fix_scale=bool(i % 2)) for i in range(9)]
    run_rounds(gpu_ctx, scenes, skip=lambda rnd, i: (rnd + i) % 3 == 0)


@pytest.mark.parametrize("ratio", [0.2, 0.5])
def test_find_and_find_continuing_state(gpu_ctx, ratio):
    sc = S.make_scene(41, 300, ratio)
    ref = S.solver_from_scene(sc)
    with Sim3Solver(gpu_ctx, sc) as s:
        o = ref.find()
        compare_call(ref, o, s.find(), s.hypotheses(0), "find")
    ref = S.solver_from_scene(sc)
    with Sim3Solver(gpu_ctx, sc) as s:
        for k in range(3):
            o = ref.iterate(5)
            compare_call(ref, o, s.iterate(5), s.hypotheses(0), f"iterate {k}")
        o = ref.find()
        compare_call(ref, o, s.find(), s.hypotheses(0), "find after iterate")
        assert s.GetEstimatedScale() == float(ref.GetEstimatedScale()) or np.isnan(s.GetEstimatedScale())


def test_iterate_after_budget_draws_nothing(gpu_ctx):
    sc = S.make_scene(43, 200, 0.1)
    ref = S.solver_from_scene(sc, (0.99, 20, 12))
    with Sim3SolverBatch(gpu_ctx, [sc], (0.99, 20, 12)) as b:
        for k in range(6):
            o = ref.iterate(5)
            g = b.iterate(5)[0]
            compare_call(ref, o, g, b.hypotheses(0), f"call {k}")
        assert ref.n_iterations == 12 and g.no_more and g.T12 is None
        nw, nr, _ = b.hypotheses(0)
        assert (nw, nr) == (0, 0)


def test_lld_sim3solver_find_single_entry(gpu_ctx):
    sc = S.make_scene(44, 120, 0.7)
    ref = S.solver_from_scene(sc)
    o = ref.find()
    p = problem_from_scene(sc)
    par = abi.Sim3SolverParams(0.99, 20, 300)
    inl = np.zeros(p.n1, np.uint8)
    r = abi.Sim3SolverResult()
    r.inlier = inl.ctypes.data_as(abi.c_uint8_p)
    assert gpu_ctx.lib.fn("sim3solver_find")(gpu_ctx.handle, C.byref(p.c), C.byref(par), C.byref(r)) == abi.LLD_OK
    assert bool(r.has_pose) == (o["T12"] is not None) and r.n_inliers == o["n_inliers"] and r.iterations == ref.n_iterations
    assert np.array_equal(inl, o["inliers"])
    if r.has_pose:
        assert ulps(np.array(r.T12[:]), o["T12"]) <= 1


def _quat(R):
    """Rotation matrix -> (x, y, z, w)."""
    R = np.asarray(R, np.float64)
    w = np.sqrt(max(0.0, 1.0 + np.trace(R))) / 2.0
    x = np.copysign(np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2.0, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2.0, R[1, 0] - R[0, 1])
    return np.array([x, y, z, w])


@pytest.mark.parametrize("fix", [False, True])
def test_chain_into_optimize_sim3(gpu_ctx, fix):
    """ComputeSim3's next steps consume the solver's output: its inliers and (R, t, s) seed lld_optimize_sim3, which keeps >= 20
    inliers and lands near the generator's S12."""
    sc = S.make_scene(77 + fix, 400, 0.6, noise=0.2, fix_scale=fix)
    ref = S.solver_from_scene(sc)
    with Sim3SolverBatch(gpu_ctx, [sc]) as b:
        for _ in range(60):
            g = b.iterate(5)[0]
            if g.T12 is not None or g.no_more:
                break
    assert g.T12 is not None and g.n_inliers > 20
    sel = np.flatnonzero(g.inliers[ref.index1])             # correspondences in vpMatched12 order
    pair = Sim3Pair(K1=ref.K1, K2=ref.K2, s12_q=_quat(g.R), s12_t=g.t.astype(np.float64), s12_s=float(g.s),
                    p1c=ref.X1[sel].astype(np.float64), p2c=ref.X2[sel].astype(np.float64),
                    obs1=ref.P1im1[sel].astype(np.float64), obs2=ref.P2im2[sel].astype(np.float64),
                    inv_sigma2_1=1.0 / np.asarray(sc["sigma2_1"], np.float64)[sel],
                    inv_sigma2_2=1.0 / np.asarray(sc["sigma2_2"], np.float64)[sel])
    out = Optimizer(gpu_ctx).OptimizeSim3(pair, th2=10.0, bFixScale=fix)
    assert out.n_inliers >= 20
    q = np.asarray(out.s12_q); x, y, z, w = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert np.abs(R - sc["R12"]).max() < 0.02
    assert abs(out.s12_s - sc["s12"]) < 0.02 * sc["s12"]
    assert np.linalg.norm(np.asarray(out.s12_t) - sc["t12"]) < 0.1


def _expect(status, fn, *a):
    with pytest.raises(Sim3SolverError) as e:
        fn(*a)
    assert e.value.status == status


def test_refusals(gpu_ctx):
    INVALID, UNSUPPORTED = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED
    good = S.make_scene(9, 50, 0.8)

    def with_(**kw):
        d = dict(good); d.update(kw); return d
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [])
    _expect(UNSUPPORTED, Sim3SolverBatch, gpu_ctx, [good] * 257)
    _expect(UNSUPPORTED, Sim3SolverBatch, gpu_ctx, [good], (0.99, 2, 300))
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [good], (0.99, 20, 0))
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [good], (0.99, 20, 65537))
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [good], (1.0, 20, 300))
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [good], (0.0, 20, 300))
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [with_(K1=(0.0, 700.0, 600.0, 180.0))])
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [with_(K2=(700.0, -1.0, 600.0, 180.0))])
    idx = good["index1"].copy(); idx[3] = idx[2]
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [with_(index1=idx)])
    idx = good["index1"].copy(); idx[-1] = good["n1"]
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [with_(index1=idx)])
    s2 = good["sigma2_2"].copy(); s2[5] = np.nan
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [with_(sigma2_2=s2)])
    s2 = good["sigma2_1"].copy(); s2[5] = -1.0
    _expect(INVALID, Sim3SolverBatch, gpu_ctx, [with_(sigma2_1=s2)])
    big = S.make_scene(10, 8193, 0.8, n1=8193)
    _expect(UNSUPPORTED, Sim3SolverBatch, gpu_ctx, [big])
    _expect(UNSUPPORTED, Sim3SolverBatch, gpu_ctx, [with_(n1=8193)])
    with Sim3SolverBatch(gpu_ctx, [good]) as b:
        _expect(INVALID, b.iterate, 0)
        _expect(UNSUPPORTED, b.iterate, 65537)
        assert b.lib.fn("sim3solver_batch_hypotheses")(b.handle, 1, 0, None, C.byref(C.c_int32()), C.byref(C.c_int32())) == INVALID
        assert b.lib.fn("sim3solver_batch_download")(b.handle, None) == INVALID
    p = problem_from_scene(good)
    par = abi.Sim3SolverParams(0.99, 20, 300)
    r = abi.Sim3SolverResult()
    assert gpu_ctx.lib.fn("sim3solver_find")(None, C.byref(p.c), C.byref(par), C.byref(r)) == INVALID
    assert gpu_ctx.lib.fn("sim3solver_find")(gpu_ctx.handle, None, C.byref(par), C.byref(r)) == INVALID
