"""lld_initializer_* (Initializer on the device) against the restatement tests/initializer_ref.py.  Compared exactly: the
sampled sets, every hypothesis's inlier count and score (bit for bit), the winners, SH, SF, the model, both inlier masks, nGood
of every motion hypothesis, best_index, vbTriangulated and success.  Within 1 float ulp: the winning H21 / F21, R21, t21, vP3D.
parallax: see PARALLAX_TOL.  A count or score difference is reported with the matches whose chi-square lies within one ulp of a
threshold; the test still fails on it.  Also the chain from SearchForInitialization and every refusal."""
import ctypes as C

import numpy as np
import pytest

import initializer_ref as I
from lld_slam_amd import abi
from lld_slam_amd.initializer import Initializer, InitializerError, output_from_result, problem_from_scene

pytestmark = pytest.mark.gpu

# Device acos against glibc's: each is within an ulp of double of the true value, and parallax = (float)(acos(c)*180/pi) rounds
# that to float, so the two floats differ by at most 1 float ulp (a double-ulp difference can only move the float rounding by
# one step).  Asserted as 1 ulp; the measured value on the test scenes is printed by the tests (not yet measured on a device).
PARALLAX_TOL = 1


def ulps(a, b):
    """Largest distance in float ulps (NaN == NaN)."""
    a = np.asarray(a, np.float32).reshape(-1); b = np.asarray(b, np.float32).reshape(-1)
    both_nan = np.isnan(a) & np.isnan(b)
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia); ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.where(both_nan, 0, np.abs(ia - ib))
    return int(d.max()) if d.size else 0


def near_threshold(ref, h, is_F):
    if is_F:
        _, _, c1, c2 = I.check_fundamental(h["M"], ref.k1, ref.k2, ref.sigma); th = np.float32(3.841)
    else:
        _, _, c1, c2 = I.check_homography(h["M"], h["Minv"], ref.k1, ref.k2, ref.sigma); th = np.float32(5.991)
    return [np.flatnonzero(np.abs(c.astype(np.float64) - th) <= np.spacing(th)) for c in (c1, c2)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).reshape(-1).view(np.uint32), np.asarray(b, np.float32).reshape(-1).view(np.uint32)) \
        or (np.isnan(a).all() and np.isnan(b).all())


def compare(ref, o, got, ini, what):
    for model, hyps in ((0, ref.hyps_H), (1, ref.hyps_F)):
        recs = ini.hypotheses(model)
        assert len(recs) == len(hyps), what
        for k, (g, h) in enumerate(zip(recs, hyps)):
            assert g["idx"] == [int(x) for x in h["idx"]], f"{what}: model {model} hypothesis {k} set {g['idx']} vs {h['idx']}"
            if g["n_inliers"] != h["n_inliers"] or not same_bits(g["score"], h["score"]):
                pytest.fail(f"{what}: model {model} hypothesis {k}: count {g['n_inliers']} vs {h['n_inliers']}, score {g['score']!r} "
                            f"vs {h['score']!r}, M ulps {ulps(g['M'], h['M'])}; matches within 1 ulp of the threshold: "
                            f"{near_threshold(ref, h, model == 1)}")
    assert (got.win_H, got.win_F) == (o["win_H"], o["win_F"]), what
    assert same_bits(got.SH, o["SH"]) and same_bits(got.SF, o["SF"]), f"{what}: SH {got.SH} {o['SH']} SF {got.SF} {o['SF']}"
    assert got.model == o["model"] and got.n_matches == o["n_matches"], what
    assert (got.n_inliers_H, got.n_inliers_F) == (o["n_inliers_H"], o["n_inliers_F"]), what
    assert np.array_equal(got.inlier_H, o["inlier_H"]) and np.array_equal(got.inlier_F, o["inlier_F"]), what
    assert ulps(got.H21, o["H21"]) <= 1 and ulps(got.F21, o["F21"]) <= 1, what
    assert np.array_equal(got.n_good, o["n_good"]), f"{what}: nGood {got.n_good} vs {o['n_good']}"
    d = ulps(got.parallax, o["parallax"])
    print(f"{what}: parallax ulps {d}")
    assert d <= PARALLAX_TOL, f"{what}: parallax {got.parallax} vs {o['parallax']}"
    assert got.best_index == o["best_index"] and got.success == o["success"], what
    assert np.array_equal(got.triangulated, o["triangulated"]), what
    assert ulps(got.R21, o["R21"]) <= 1 and ulps(got.t21, o["t21"]) <= 1, f"{what}: R21 {got.R21} vs {o['R21']}"
    assert ulps(got.p3d, o["p3d"]) <= 1, what


def run_scene(ctx, sc, what, **kw):
    ref = I.ref_from_scene(sc, **kw)
    o = ref.initialize(sc["keys2"], sc["matches12"])
    p = dict(I.DEFAULT_PARAMS); p["seed"] = sc["seed"]; p.update(kw)
    K, k1, k2, m = problem_from_scene(sc)
    with Initializer(ctx, K, k1, **p) as ini:
        got = ini.Initialize(k2, m)
        compare(ref, o, got, ini, what)
    return o, got


@pytest.mark.parametrize("n", [8, 9, 100, 500, 2000, 8192])
@pytest.mark.parametrize("ratio", [0.9, 0.5, 0.2])
def test_sizes_and_inlier_ratios(gpu_ctx, n, ratio):
    extra = 0.0 if n == 8192 else 0.25
    sc = I.make_scene(300 + n + int(10 * ratio), n, ratio, extra=extra)
    run_scene(gpu_ctx, sc, f"n {n} ratio {ratio}")


@pytest.mark.parametrize("variant,n", [("general", 400), ("planar", 400), ("rotation", 400), ("exact", 300), ("wrong", 200), ("exact", 8)])
def test_variants(gpu_ctx, variant, n):
    sc = I.make_scene(21, n, 0.9, variant=variant)
    o, got = run_scene(gpu_ctx, sc, variant)
    if variant in ("general", "planar") or (variant, n) == ("exact", 300):
        assert got.success and got.model == (0 if variant == "planar" else 1)
    if variant in ("rotation", "wrong"):
        assert not got.success


@pytest.mark.parametrize("iterations,sigma,seed", [(1, 1.0, 0), (1000, 1.0, 0), (200, 2.0, 0), (200, 1.0, 12345)])
def test_parameters(gpu_ctx, iterations, sigma, seed):
    sc = I.make_scene(55, 500, 0.7)
    run_scene(gpu_ctx, sc, f"iterations {iterations} sigma {sigma} seed {seed}", iterations=iterations, sigma=sigma, seed=seed)


def test_no_winner_in_either_model_gives_zeros(gpu_ctx):
    """Every keypoint of frame 2 at one pixel: every score is NaN, neither model has a winner, RH is 0/0 and falls to F, which
    has nothing to reconstruct from: zeros, success false, no motion hypothesis run."""
    sc = I.make_scene(21, 60, variant="collapsed")
    o, got = run_scene(gpu_ctx, sc, "collapsed")
    assert (got.win_H, got.win_F) == (-1, -1) and got.SH == 0 and got.SF == 0 and np.isnan(got.RH)
    assert got.model == 1 and not got.success and got.best_index == -1
    assert not got.H21.any() and not got.F21.any() and got.n_inliers_H == 0 and got.n_inliers_F == 0
    assert not got.inlier_H.any() and not got.inlier_F.any() and not got.n_good.any() and not got.parallax.any()
    assert not got.R21.any() and not got.t21.any() and not got.p3d.any() and not got.triangulated.any()
    for model in (0, 1):
        assert all(np.isnan(h["score"]) for h in ini_hyps(gpu_ctx, sc, model))


def ini_hyps(ctx, sc, model):
    K, k1, k2, m = problem_from_scene(sc)
    with Initializer(ctx, K, k1, seed=sc["seed"]) as ini:
        ini.Initialize(k2, m)
        return ini.hypotheses(model)


def test_one_iteration_of_wrong_matches(gpu_ctx):
    """Every match wrong, one iteration: H scores nothing (no winner for H) while F scores its own sample."""
    sc = I.make_scene(77, 40, variant="wrong")
    o, got = run_scene(gpu_ctx, sc, "wrong, 1 iteration", iterations=1)
    assert got.win_H == o["win_H"] and got.win_F == o["win_F"]


def test_two_calls_one_handle_and_a_second_handle(gpu_ctx):
    a = I.make_scene(61, 500, 0.8)
    b = I.make_scene(62, 500, 0.8, variant="planar")
    K, k1, k2a, ma = problem_from_scene(a)
    _, k1b, k2b, mb = problem_from_scene(b)
    # frame b's current frame against a's reference frame: the matches are nonsense but valid
    with Initializer(gpu_ctx, K, k1, seed=3) as one, Initializer(gpu_ctx, K, k1b, seed=3) as other:
        r1 = one.Initialize(k2a, ma)
        r2 = one.Initialize(k2b, ma)
        r3 = other.Initialize(k2b, mb)
        for keys2, m, got in ((k2a, ma, r1), (k2b, ma, r2)):
            with Initializer(gpu_ctx, K, k1, seed=3) as fresh:
                want = fresh.Initialize(keys2, m)
            for f in ("success", "model", "best_index", "win_H", "win_F"):
                assert getattr(got, f) == getattr(want, f)
            for f in ("SH", "SF", "H21", "F21", "R21", "t21", "p3d", "parallax", "n_good", "inlier_H", "inlier_F", "triangulated"):
                assert np.array_equal(np.asarray(getattr(got, f)), np.asarray(getattr(want, f)), equal_nan=True), f
        ref = I.ref_from_scene(b, seed=3)
        compare(ref, ref.initialize(b["keys2"], b["matches12"]), r3, other, "second handle")


def test_null_optional_outputs_and_find(gpu_ctx):
    sc = I.make_scene(63, 300, 0.9)
    K, k1, k2, m = problem_from_scene(sc)
    with Initializer(gpu_ctx, K, k1, seed=sc["seed"]) as ini:
        full = ini.Initialize(k2, m)
        bare = ini.Initialize(k2, m, want_inliers=False, want_points=False)
    assert bare.inlier_H is None and bare.p3d is None
    assert bare.success == full.success and np.array_equal(bare.R21, full.R21) and np.array_equal(bare.n_good, full.n_good)
    par = abi.InitializerParams(1.0, 200, 1.0, 50, sc["seed"])
    r = abi.InitializerResult()
    Kf, a1, a2 = K.reshape(-1).copy(), k1.reshape(-1).copy(), k2.reshape(-1).copy()
    fp = lambda a: a.ctypes.data_as(abi.c_float_p)
    st = gpu_ctx.lib.fn("initializer_find")(gpu_ctx.handle, fp(Kf), len(k1), fp(a1), len(k2), fp(a2), len(m),
                                            m.ctypes.data_as(abi.c_int32_p), C.byref(par), C.byref(r))
    assert st == abi.LLD_OK
    one = output_from_result(r)
    assert one.success == full.success and np.array_equal(one.R21, full.R21) and np.array_equal(one.t21, full.t21)


def test_chain_from_search_for_initialization(gpu_ctx):
    """SearchForInitialization's vnMatches12 goes straight into Initialize; the device result equals the restatement's."""
    from lld_slam_amd import ORBmatcher, synth
    F1, F2, prev = synth.make_init_pair(3)
    n, m, _ = ORBmatcher(gpu_ctx, 0.9, True).SearchForInitialization(F1, F2, prev, 100)
    assert n >= 100
    K = np.array([[I.CAM["fx"], 0, I.CAM["cx"]], [0, I.CAM["fy"], I.CAM["cy"]], [0, 0, 1]], np.float32)
    ref = I.InitializerRef(K, F1.xy)
    o = ref.initialize(F2.xy, m)
    assert o["n_matches"] == n
    with Initializer(gpu_ctx, K, F1.xy) as ini:
        compare(ref, o, ini.Initialize(F2.xy, m), ini, "chain")


def _expect(status, fn, *a, **k):
    with pytest.raises(InitializerError) as e:
        fn(*a, **k)
    assert e.value.status == status


def test_refusals(gpu_ctx):
    INVALID, UNSUPPORTED = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED
    sc = I.make_scene(9, 50, 0.8)
    K, k1, k2, m = problem_from_scene(sc)
    _expect(INVALID, Initializer, gpu_ctx, K, k1[:0])
    _expect(UNSUPPORTED, Initializer, gpu_ctx, K, np.zeros((8193, 2), np.float32))
    _expect(INVALID, Initializer, gpu_ctx, K, k1, iterations=0)
    _expect(INVALID, Initializer, gpu_ctx, K, k1, iterations=4097)
    _expect(INVALID, Initializer, gpu_ctx, K, k1, sigma=0.0)
    _expect(INVALID, Initializer, gpu_ctx, K, k1, sigma=float("inf"))
    _expect(INVALID, Initializer, gpu_ctx, K, k1, sigma=float("nan"))
    Kb = K.copy(); Kb[0, 0] = 0
    _expect(INVALID, Initializer, gpu_ctx, Kb, k1)
    Kb = K.copy(); Kb[1, 1] = -1
    _expect(INVALID, Initializer, gpu_ctx, Kb, k1)
    kb = k1.copy(); kb[3, 1] = np.nan
    _expect(INVALID, Initializer, gpu_ctx, K, kb)
    _expect(INVALID, Initializer, gpu_ctx, np.zeros(4, np.float32), k1)         # K NULL
    with Initializer(gpu_ctx, K, k1) as ini:
        _expect(INVALID, ini.Initialize, k2[:0], m)
        _expect(UNSUPPORTED, ini.Initialize, np.zeros((8193, 2), np.float32), m)
        _expect(INVALID, ini.Initialize, k2, m[:-1])                            # n12 != n1
        mb = m.copy(); mb[np.flatnonzero(m >= 0)[0]] = len(k2)
        _expect(INVALID, ini.Initialize, k2, mb)
        mb = np.full_like(m, -1); mb[:7] = np.arange(7)
        _expect(INVALID, ini.Initialize, k2, mb)                                # fewer than 8 matches
        kb = k2.copy(); kb[0, 0] = np.inf
        _expect(INVALID, ini.Initialize, kb, m)
        assert ini.lib.fn("initializer_initialize")(ini.handle, len(k2), None, len(m), m.ctypes.data_as(abi.c_int32_p),
                                                    C.byref(abi.InitializerResult())) == INVALID
        assert ini.lib.fn("initializer_hypotheses")(ini.handle, 2, 0, None, C.byref(C.c_int32())) == INVALID
        assert ini.hypotheses(0) == []                                          # no call yet
        got = ini.Initialize(k2, m)                                             # the handle and the context are still usable
        assert got.n_matches == 50
