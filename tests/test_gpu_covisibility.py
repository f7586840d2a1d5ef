"""lld_covisibility on the device against tests/covis_ref.py.  Every output is an integer, so every comparison is exact equality:
the hand-worked cases, the wavefront and lane-group boundaries of the observation walk, the keyframe-table sizes up to the limit,
empty queries, duplicates, bad points, query_kf = -1, many uneven queries, the capacity protocol, random scenes, the flags, the
run-to-run bytes and every refusal."""
import numpy as np
import pytest

import covis_ref as R
import covis_scenes as S
from lld_slam_amd import abi
from lld_slam_amd import covisibility as CV

pytestmark = pytest.mark.gpu

CONN_KEYS = ("conn_start", "conn_kf", "conn_weight", "ordered_start", "ordered_kf", "ordered_weight", "n_max", "kf_max", "updated")
CULL_KEYS = ("n_mps", "n_redundant", "redundant")


def run(ctx, sc, flags, **kw):
    cull = bool(flags & CV.CULLING)
    return CV.covisibility(ctx, sc["n_kf"], sc["obs_start"], sc["obs_kf"], sc["point_bad"], sc["query_kf"], sc["q_start"], sc["q_point"],
                           flags, obs_octave=sc["obs_octave"] if cull else None, point_nobs=sc["point_nobs"] if cull else None,
                           q_octave=sc["q_octave"] if cull else None, q_depth=sc["q_depth"] if cull else None,
                           q_th_depth=sc["q_th_depth"] if cull else None, monocular=sc["monocular"], **kw)


def same_conn(got, want):
    for k in CONN_KEYS:
        g = getattr(got, k)
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (k, g, want[k])


def same_cull(got, want):
    for k in CULL_KEYS:
        g = getattr(got, k)
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (k, g, want[k])


def check_both(ctx, sc):
    conn, cull = run(ctx, sc, CV.CONNECTIONS | CV.CULLING)
    same_conn(conn, R.update_connections_ref(sc)); same_cull(cull, R.keyframe_culling_ref(sc))
    return conn, cull


@pytest.mark.parametrize("name", sorted(S.CONN_CASES))
def test_connections_hand_worked(gpu_ctx, name):
    sc, exp = S.CONN_CASES[name]()
    same_conn(run(gpu_ctx, sc, CV.CONNECTIONS)[0], S.expected_conn([exp]))
    same_conn(run(gpu_ctx, sc, CV.CONNECTIONS)[0], R.update_connections_ref(sc))


@pytest.mark.parametrize("name", sorted(S.CULL_CASES))
def test_culling_hand_worked(gpu_ctx, name):
    sc, exp = S.CULL_CASES[name]()
    got = run(gpu_ctx, sc, CV.CULLING)[1]
    assert (int(got.n_mps[0]), int(got.n_redundant[0]), int(got.redundant[0])) == exp
    same_cull(got, R.keyframe_culling_ref(sc))


def test_observation_counts_at_the_lane_and_wavefront_boundaries(gpu_ctx):
    n_kf = 256
    b = S.Builder(n_kf)
    rng = np.random.default_rng(7)
    pts = []
    for n in (1, 15, 16, 17, 63, 64, 65, 200):
        kfs = sorted(rng.choice(np.arange(1, n_kf), size=n, replace=False).tolist())
        pts.append(b.point([(k, int(rng.integers(0, 4))) for k in kfs], nobs=n + 3))
    b.query(0, [(p, 1, 1.0) for p in pts] * 16)                                # every point 16 times: the long ones reach th = 15
    b.query(0, [(p, 0, 1.0) for p in pts])
    conn, cull = check_both(gpu_ctx, b.scene())
    assert conn.n_max[0] >= 16 and conn.ordered_start[1] > 200 and conn.ordered_start[2] - conn.ordered_start[1] == 1


@pytest.mark.parametrize("th", [1000, 15, 4])
def test_sparse_slots_over_three_passes_give_slots_not_ranks(gpu_ctx, th):
    """The staged keys carry a keyframe's rank among the connected ones, the outputs its slot: connected slots that are sparse over more
    than one 256-lane pass of the table, in a second query whose staging range starts behind the first's.  The lists are written out by
    hand (the lower slot of the tied maxima wins, and its rank, 3, is not its slot; equal weights come out in descending slot order)."""
    b = S.Builder(600); own = 7
    pts = S._shared(b, own, {5: 3, 255: 2, 256: 4, 300: 6, 599: 6})
    b.query(own, pts); b.query(599, pts[:3])
    sc = b.scene()
    got = run(gpu_ctx, sc, CV.CONNECTIONS, th=th)[0]
    same_conn(got, R.update_connections_ref(sc, th))
    assert got.conn_start.tolist() == [0, 5, 7] and got.conn_kf.tolist() == [5, 255, 256, 300, 599, 5, 7]
    assert got.conn_weight.tolist() == [3, 2, 4, 6, 6, 3, 3] and got.n_max.tolist() == [6, 3] and got.kf_max.tolist() == [300, 5]
    if th == 4:
        assert got.ordered_start.tolist() == [0, 3, 4] and got.ordered_kf.tolist() == [599, 300, 256, 5] and got.ordered_weight.tolist() == [6, 6, 4, 3]
    else:
        assert got.ordered_kf.tolist() == [300, 5] and got.ordered_weight.tolist() == [6, 3]


@pytest.mark.parametrize("n_kf", [1, 64, 65, 16384])
def test_keyframe_table_sizes(gpu_ctx, n_kf):
    rng = np.random.default_rng(n_kf)
    b = S.Builder(n_kf)
    used = sorted({0, n_kf - 1, n_kf // 2, *rng.choice(n_kf, size=min(n_kf, 90), replace=False).tolist()})
    pts = []
    for _ in range(120):
        k = int(rng.integers(1, min(len(used), 9) + 1))
        pts.append(b.point([(int(s), int(rng.integers(0, 8))) for s in rng.choice(used, size=k, replace=False)], nobs=k + 2))
    strong = [b.point([used[0], used[-1]]) for _ in range(17)]                  # weight 17 between the first and the last slot
    b.query(used[0], pts + strong); b.query(used[-1], strong + pts[:40]); b.query(-1, pts)
    conn, _ = check_both(gpu_ctx, b.scene())
    if n_kf > 1:
        assert conn.ordered_kf[0] == used[-1] and conn.ordered_weight[0] >= 17


def test_densely_connected_query_at_the_largest_table(gpu_ctx):
    """One query connected to about 12000 of 16384 keyframes with th = 1: the longest list the in-LDS sort can meet (16384 keys,
    128 KB of LDS), next to a small query in the same call."""
    rng = np.random.default_rng(11)
    n_kf = CV.MAX_KF
    b = S.Builder(n_kf)
    slots = rng.choice(np.arange(1, n_kf), size=12000, replace=False)
    pts = [b.point([0] + sorted(int(x) for x in slots[i:i + 50])) for i in range(0, 12000, 50)]          # 240 points of 51 observations
    pts += [b.point([0] + sorted(int(x) for x in rng.choice(slots, size=30, replace=False))) for _ in range(100)]   # weights 2, 3, ...
    b.query(0, pts); b.query(int(slots[0]), pts[:3])
    sc = b.scene()
    got = run(gpu_ctx, sc, CV.CONNECTIONS, th=1)[0]
    same_conn(got, R.update_connections_ref(sc, 1))
    assert got.ordered_start[1] == 12000 and got.ordered_weight[0] > got.ordered_weight[11999] == 1


def test_keyframe_table_above_the_limit_is_unsupported(gpu_ctx):
    b = S.Builder(CV.MAX_KF + 1); b.query(0, [b.point([0, CV.MAX_KF])])
    for flags in (CV.CONNECTIONS, CV.CULLING, CV.CONNECTIONS | CV.CULLING):
        with pytest.raises(CV.CovisibilityError) as e:
            run(gpu_ctx, b.scene(), flags)
        assert e.value.status == abi.LLD_ERR_UNSUPPORTED


def test_empty_query_duplicate_bad_point_and_minus_one(gpu_ctx):
    b = S.Builder(6)
    shared = [b.point([(0, 1), (1, 1), (2, 2), (3, 0)], nobs=5) for _ in range(16)]
    bad = [b.point([(0, 0), (4, 0), (5, 0), (1, 0)], bad=True, nobs=6) for _ in range(20)]
    b.query(0, [(p, 1, 2.0) for p in shared + bad])
    b.query(1, [])                                                            # nothing between two non-empty queries
    b.query(2, [(shared[0], 0, 1.0)] * 15 + [(bad[0], 0, 1.0)])               # one point 15 times: weight 15 by duplicates alone
    b.query(-1, [(p, 7, 1.0) for p in shared])                                # a Frame's vote: its own slot is nobody's
    sc = b.scene()
    conn, cull = check_both(gpu_ctx, sc)
    assert conn.updated.tolist() == [1, 0, 1, 1] and conn.kf_max.tolist() == [1, -1, 0, 0]
    assert conn.conn_kf[conn.conn_start[0]:conn.conn_start[1]].tolist() == [1, 2, 3]        # the bad points' keyframes 4, 5 are absent
    assert conn.ordered_weight[conn.ordered_start[2]:conn.ordered_start[3]].tolist() == [15, 15, 15]
    assert conn.ordered_kf[conn.ordered_start[3]:conn.ordered_start[4]].tolist() == [3, 2, 1, 0]
    assert cull.n_mps.tolist() == [16, 0, 15, 16] and cull.redundant.tolist() == [1, 0, 1, 1]


def test_seventy_uneven_queries(gpu_ctx):
    rng = np.random.default_rng(70)
    n_kf = 70
    b = S.Builder(n_kf)
    for _ in range(500):
        k = int(rng.integers(1, 20))
        b.point([(int(s), int(rng.integers(0, 8))) for s in rng.choice(n_kf, size=k, replace=False)], bad=rng.random() < 0.03,
                nobs=k + int(rng.integers(0, 3)))
    for q in range(70):
        n = [0, 1, 3, 37, 200, 701][q % 6] + q
        b.query(q if q % 9 else -1, [(int(p), int(rng.integers(0, 8)), float(rng.random() * 50 - 1)) for p in rng.integers(0, 500, n)])
    check_both(gpu_ctx, b.scene())


def test_short_capacity_reports_the_totals(gpu_ctx):
    sc = S.random_scene(5)
    want = R.update_connections_ref(sc)
    n_conn, n_ord = len(want["conn_kf"]), len(want["ordered_kf"])
    for cc, oc in ((n_conn - 1, n_ord), (n_conn, n_ord - 1), (0, 0)):
        with pytest.raises(CV.CovisibilityError) as e:
            run(gpu_ctx, sc, CV.CONNECTIONS, conn_capacity=cc, ordered_capacity=oc)
        assert e.value.status == abi.LLD_ERR_INVALID and (e.value.n_conn, e.value.n_ordered) == (n_conn, n_ord)
    same_conn(run(gpu_ctx, sc, CV.CONNECTIONS, conn_capacity=n_conn, ordered_capacity=n_ord)[0], want)


@pytest.fixture(scope="module")
def random_scenes():
    return {seed: S.random_scene(seed, minus_one=(seed == 2)) for seed in (0, 1, 2)}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_scenes(gpu_ctx, random_scenes, seed):
    check_both(gpu_ctx, random_scenes[seed])


def test_random_scene_monocular_and_other_parameters(gpu_ctx):
    sc = S.random_scene(4, monocular=True)
    same_cull(run(gpu_ctx, sc, CV.CULLING)[1], R.keyframe_culling_ref(sc))
    same_cull(run(gpu_ctx, sc, CV.CULLING, th_obs=2, redundant_ratio=0.5)[1], R.keyframe_culling_ref(sc, 2, 0.5))
    same_conn(run(gpu_ctx, sc, CV.CONNECTIONS, th=1)[0], R.update_connections_ref(sc, 1))
    same_conn(run(gpu_ctx, sc, CV.CONNECTIONS, th=1000)[0], R.update_connections_ref(sc, 1000))


def test_flags_together_equal_one_at_a_time_and_repeats_are_bytewise_equal(gpu_ctx, random_scenes):
    sc = random_scenes[1]
    both = run(gpu_ctx, sc, CV.CONNECTIONS | CV.CULLING)
    conn, cull = run(gpu_ctx, sc, CV.CONNECTIONS)[0], run(gpu_ctx, sc, CV.CULLING)[1]
    again = run(gpu_ctx, sc, CV.CONNECTIONS | CV.CULLING)
    for k in CONN_KEYS:
        assert getattr(both[0], k).tobytes() == getattr(conn, k).tobytes() == getattr(again[0], k).tobytes(), k
    for k in CULL_KEYS:
        assert getattr(both[1], k).tobytes() == getattr(cull, k).tobytes() == getattr(again[1], k).tobytes(), k


def test_phase_times_are_reported(gpu_ctx, random_scenes):
    ms = np.full(3, -1, np.float32)
    run(gpu_ctx, random_scenes[0], CV.CONNECTIONS | CV.CULLING, phase_ms=ms)
    assert np.all(ms >= 0) and np.all(ms < 1000)


def test_no_queries_is_ok_and_touches_nothing(gpu_ctx):
    b = S.Builder(3); b.point([0, 1])
    conn, cull = run(gpu_ctx, b.scene(), CV.CONNECTIONS | CV.CULLING)
    assert len(conn.conn_kf) == 0 and conn.conn_start.tolist() == [0] and len(cull.n_mps) == 0


def _broken(mut):
    sc = S.random_scene(9, n_kf=8, n_points=30)
    mut(sc)
    return sc


def _set(key, idx, val):
    def f(sc):
        sc[key] = sc[key].copy(); sc[key][idx] = val
    return f


INVALID = {
    "obs_start_first": _set("obs_start", 0, 1),
    "obs_start_decreasing": lambda sc: sc.__setitem__("obs_start", np.concatenate([sc["obs_start"][:3], [sc["obs_start"][2] - 1], sc["obs_start"][4:]]).astype(np.int32)),
    "obs_start_last": lambda sc: sc.__setitem__("obs_start", np.concatenate([sc["obs_start"][:-1], [sc["obs_start"][-1] - 1]]).astype(np.int32)),
    "q_start_first": _set("q_start", 0, 1),
    "q_start_decreasing": lambda sc: sc.__setitem__("q_start", np.concatenate([sc["q_start"][:3], [sc["q_start"][2] - 1], sc["q_start"][4:]]).astype(np.int32)),
    "q_start_last": lambda sc: sc.__setitem__("q_start", np.concatenate([sc["q_start"][:-1], [sc["q_start"][-1] - 1]]).astype(np.int32)),
    "obs_kf_negative": _set("obs_kf", 5, -1),
    "obs_kf_n_kf": _set("obs_kf", 5, 8),
    "query_kf_below": _set("query_kf", 2, -2),
    "query_kf_n_kf": _set("query_kf", 2, 8),
    "q_point_negative": _set("q_point", 4, -1),
    "q_point_n_points": _set("q_point", 4, 30),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_lists_are_refused(gpu_ctx, name):
    sc = _broken(INVALID[name])
    for flags in (CV.CONNECTIONS, CV.CULLING):
        with pytest.raises(CV.CovisibilityError) as e:
            run(gpu_ctx, sc, flags, conn_capacity=1000, ordered_capacity=1000)
        assert e.value.status == abi.LLD_ERR_INVALID and e.value.n_conn is None


def test_invalid_flags_sizes_and_pointers_are_refused(gpu_ctx):
    import ctypes as C
    sc = S.random_scene(9, n_kf=8, n_points=30)
    for flags in (0, 4, 7):
        with pytest.raises(CV.CovisibilityError) as e:
            run(gpu_ctx, sc, flags, conn_capacity=1000, ordered_capacity=1000)
        assert e.value.status == abi.LLD_ERR_INVALID
    with pytest.raises(CV.CovisibilityError) as e:
        run(gpu_ctx, sc, CV.CONNECTIONS, conn_capacity=-1, ordered_capacity=10)
    assert e.value.status == abi.LLD_ERR_INVALID
    # the culling part without its arrays
    with pytest.raises(CV.CovisibilityError) as e:
        CV.covisibility(gpu_ctx, sc["n_kf"], sc["obs_start"], sc["obs_kf"], sc["point_bad"], sc["query_kf"], sc["q_start"], sc["q_point"], CV.CULLING)
    assert e.value.status == abi.LLD_ERR_INVALID
    # the raw entry point: NULL structs, negative sizes, NULL required arrays
    fn = gpu_ctx.lib.fn("covisibility")
    a, o = abi.CovisibilityIn(), abi.CovisibilityOut()
    assert fn(gpu_ctx.handle, None, C.byref(o)) == abi.LLD_ERR_INVALID and fn(gpu_ctx.handle, C.byref(a), None) == abi.LLD_ERR_INVALID
    assert fn(None, C.byref(a), C.byref(o)) == abi.LLD_ERR_INVALID
    a.flags = CV.CONNECTIONS
    for field in ("n_kf", "n_points", "n_obs", "n_queries", "n_entries"):
        setattr(a, field, -1)
        assert fn(gpu_ctx.handle, C.byref(a), C.byref(o)) == abi.LLD_ERR_INVALID, field
        setattr(a, field, 0)
    a.n_queries = 1                                                           # every array is NULL
    assert fn(gpu_ctx.handle, C.byref(a), C.byref(o)) == abi.LLD_ERR_INVALID
