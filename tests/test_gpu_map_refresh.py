"""lld_map_refresh_points / lld_map_refresh_lines - MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth and
MapLine::ComputeDistinctiveDescriptors on the resident map's tables - against the plain-Python restatement (tests/map_refresh_ref.py, held
to hand-worked scenes by tests/test_map_refresh_ref.py) and against lld_mappoint_refresh / lld_mapline_distinctive on the CSR gathered from
the same model.  Every comparison is bit for bit, floats included."""
import copy

import numpy as np
import pytest

import map_ba_apply_scenes as AS
import map_ba_scenes as S
import map_refresh_ref as R
import map_refresh_scenes as RS
from lld_slam_amd import abi, landmarks
from lld_slam_amd.device_map import DeviceMap

pytestmark = pytest.mark.gpu

LS = RS.LEVEL_SCALE
BOTH = R.DESCRIPTOR | R.NORMAL_DEPTH
POINT_KEYS = ("desc", "best_obs", "best_median", "normal", "min_distance", "max_distance", "updated")
LINE_KEYS = ("desc", "best_obs", "best_median", "updated")


def same(got, exp, keys, what):
    for k in keys:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k, g.dtype, e.dtype, g.shape, e.shape)
        assert g.tobytes() == e.tobytes(), (what, k, [(i, a, b) for i, (a, b) in enumerate(zip(g.tolist(), e.tolist())) if a != b][:4])


def fresh(gpu_ctx, m, dim=S.LINE_DIM, **over):
    dm = DeviceMap(gpu_ctx, **RS.limits(m, dim, **over))
    RS.upload(dm, m)
    return dm


def fixed_rows(dm):
    """every fixed row of every slot as the device holds it"""
    sl = AS.all_slots(dm)
    return dm.download_points(sl["pt"]), dm.download_lines(sl["ln"])


def model_points(m, slots, dim=None):
    P = m["points"]
    z = lambda s, k, d: P[s].get(k, d) if s in P else d
    return dict(pos=np.array([z(s, "pos", np.zeros(3)) for s in slots], np.float32).reshape(-1, 3), normal=np.array([z(s, "nrm", np.zeros(3)) for s in slots], np.float32).reshape(-1, 3),
                min_distance=np.array([z(s, "mind", 0) for s in slots], np.float32), max_distance=np.array([z(s, "maxd", 0) for s in slots], np.float32),
                desc=np.array([z(s, "desc", np.zeros(8)) for s in slots], np.uint32).reshape(-1, 8),
                state=np.array([0 if s not in P else 2 if P[s]["bad"] else 1 for s in slots], np.uint8))


def model_lines(m, slots, dim):
    L = m["lines"]
    return dict(desc=np.array([L[s].get("desc", np.zeros(dim)) if s in L else np.zeros(dim) for s in slots], np.float32).reshape(-1, dim),
                bad=np.array([1 if s not in L else L[s]["bad"] for s in slots], np.uint8))


def all_rows(dm):
    sl = AS.all_slots(dm)
    return {kind: dm.rows(kind, sl[which]) for kind, which in AS.POOLS}


def refresh_points_checked(gpu_ctx, dm, m, slots, flags, what):
    """one call held to the restatement and to lld_mappoint_refresh on the gathered CSR; the model follows"""
    exp = R.refresh_points(m, slots, flags, LS)
    got = dm.refresh_points(slots, flags, LS if flags & R.NORMAL_DEPTH else None)
    same(got, exp, POINT_KEYS, what)
    sc, prior, guard = R.gather_points(m, slots, flags, LS)
    old = landmarks.refresh_map_points(gpu_ctx, sc["obs_start"], sc["obs_kf"], sc["bad"], sc["obs_desc"], sc["kf_bad"], sc["kf_ow"], sc["pos"], sc["ref_kf"], sc["ref_level"],
                                       LS, flags, prior["desc"], prior["normal"], prior["min_distance"], prior["max_distance"])
    for k in POINT_KEYS[:-1]:
        o = getattr(old, k)
        if o is not None:
            assert np.asarray(got[k]).tobytes() == np.asarray(o).tobytes(), (what, "the gathering call", k)
    assert np.array_equal(got["updated"], old.updated | guard), (what, "the gathering call: updated")
    R.write_points(m, slots, exp)
    return got


def refresh_lines_checked(gpu_ctx, dm, m, slots, dim, what):
    exp = R.refresh_lines(m, slots, dim)
    got = dm.refresh_lines(slots)
    same(got, exp, LINE_KEYS, what)
    sc, prior, guard = R.gather_lines(m, slots, dim)
    old = landmarks.distinctive_line_descriptors(gpu_ctx, sc["obs_start"], sc["obs_kf"], sc["obs_desc"], sc["kf_bad"], sc["bad"], prior, dim)
    for k in LINE_KEYS[:-1]:
        assert np.asarray(got[k]).tobytes() == np.asarray(getattr(old, k)).tobytes(), (what, "the gathering call", k)
    assert np.array_equal(got["updated"], old.updated | guard), (what, "the gathering call: updated")
    R.write_lines(m, slots, exp)
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. random maps
@pytest.mark.parametrize("seed,flags", [(0, BOTH), (1, BOTH), (0, R.DESCRIPTOR), (1, R.NORMAL_DEPTH)])
def test_random_maps(gpu_ctx, seed, flags):
    m, _ = S.random_map(seed)
    RS.dress(m, seed)
    rng = np.random.default_rng(seed)
    with fresh(gpu_ctx, m) as dm:
        sl = AS.all_slots(dm)
        slots = rng.permutation(sl["pt"]).tolist()                          # every slot, the never-set ones too
        got = refresh_points_checked(gpu_ctx, dm, m, slots, flags, "random %d" % seed)
        u = got["updated"]
        K = m["keyframes"]
        assert np.count_nonzero(u == flags) > 100 and np.count_nonzero(u == 0) > 10                       # refreshed; bad, never set or without observations
        assert any(p["obs"] and any(kf not in K for kf, _ in p["obs"]) for p in m["points"].values())     # never-set observers
        assert any(K[kf]["bad"] for p in m["points"].values() for kf, _ in p["obs"] if kf in K)           # bad observers
        if flags & R.NORMAL_DEPTH:
            assert np.count_nonzero(u & R.NO_REFERENCE) > 0
        lslots = rng.permutation(sl["ln"]).tolist()
        lgot = refresh_lines_checked(gpu_ctx, dm, m, lslots, S.LINE_DIM, "random %d lines" % seed)
        assert np.count_nonzero(lgot["updated"] == R.DESCRIPTOR) > 10 and np.count_nonzero(lgot["updated"] == 0) > 2
        assert len(set(lgot["best_median"].tolist())) > 2                   # the truncated medians differ: the selection chooses
        # the tables hold what the calls returned, every other value is the uploaded one
        pts, lns = fixed_rows(dm)
        same(pts, model_points(m, sl["pt"]), ("pos", "normal", "min_distance", "max_distance", "desc", "state"), "tables")
        same(lns, model_lines(m, sl["ln"], S.LINE_DIM), ("desc", "bad"), "line tables")


# ---------------------------------------------------------------------------------------------------------------- 2. widths
POINT_ROWS = (1, 2, 63, 64, 65, 257, 1024, 1025)           # both sides of rf_point_wave's 64, a second trip of rf_point_block's 256 lanes, the limit and one past it
LINE_ROWS = (1, 2, 64, 65)


@pytest.fixture(scope="module")
def wide_map():
    return RS.widths(POINT_ROWS, LINE_ROWS[:3], seed=3)


def test_point_rows_at_every_width(gpu_ctx, wide_map):
    m = copy.deepcopy(wide_map)
    with fresh(gpu_ctx, m) as dm:
        for i, w in enumerate(POINT_ROWS[:-1]):
            got = refresh_points_checked(gpu_ctx, dm, m, [i], BOTH, "row of %d" % w)
            assert got["updated"][0] == BOTH and len(m["points"][i]["obs"]) == w
        before = fixed_rows(dm), all_rows(dm)
        for slots in ([7], [0, 7, 3]):
            with pytest.raises(RuntimeError, match="lld_map_refresh_points") as e:
                dm.refresh_points(slots, BOTH, LS)
            assert e.value.status == abi.LLD_ERR_UNSUPPORTED
        after = fixed_rows(dm), all_rows(dm)
        same(after[0][0], before[0][0], ("pos", "normal", "min_distance", "max_distance", "desc", "state"), "refused")
        assert after[1] == before[1]
        # the normal part alone has no limit of its own but the row's: the long row is refused there too; a list that mixes both launch paths
        m2 = copy.deepcopy(wide_map)
        RS.upload_points(dm, m2)
        refresh_points_checked(gpu_ctx, dm, m2, [5, 0, 6, 3, 4, 1, 2], BOTH, "both paths in one list")
        for i in range(7):
            assert np.array_equal(m2["points"][i]["desc"], m["points"][i]["desc"]) and np.array_equal(m2["points"][i]["nrm"], m["points"][i]["nrm"])


@pytest.mark.parametrize("dim", [1, 72, 128])
def test_line_rows_and_line_dims(gpu_ctx, dim):
    m = RS.widths((1,), LINE_ROWS, seed=dim, dim=dim)
    with fresh(gpu_ctx, m, dim) as dm:
        for i, w in enumerate(LINE_ROWS[:-1]):
            got = refresh_lines_checked(gpu_ctx, dm, m, [i], dim, "line row of %d, dim %d" % (w, dim))
            assert got["updated"][0] == R.DESCRIPTOR
        before = fixed_rows(dm)
        with pytest.raises(RuntimeError, match="lld_map_refresh_lines") as e:
            dm.refresh_lines([1, 3])
        assert e.value.status == abi.LLD_ERR_UNSUPPORTED
        same(fixed_rows(dm)[1], before[1], ("desc", "bad"), "refused")


@pytest.mark.parametrize("n", [1, 256, 257])
def test_query_list_lengths(gpu_ctx, n):
    m, _ = S.random_map(2)
    RS.dress(m, 2)
    with fresh(gpu_ctx, m) as dm:
        slots = np.random.default_rng(n).permutation(dm.limits.max_points)[:n].tolist()
        refresh_points_checked(gpu_ctx, dm, m, slots, BOTH, "%d queries" % n)


# ---------------------------------------------------------------------------------------------------------------- 2b. ties
def tie_map(point_cases, line_cases, first_bad, dim=S.LINE_DIM):
    """Point slot i / line slot i has the observers keyframes 0 .. N-1 in slot order, for (N, t) = the i-th case, and their descriptor rows are
    landmark_ref.tie_rows(N, t): row t wins by the tie rule alone.  first_bad: keyframe 0 is bad, so every first kept position is 1."""
    sc = S.Scene()
    for s in range(max(N for N, _ in list(point_cases) + list(line_cases))):
        sc.kf(s, s + 1, [i for i, (N, _) in enumerate(point_cases) if s < N], [i for i, (N, _) in enumerate(line_cases) if s < N], bad=int(first_bad and s == 0))
    for i in range(len(point_cases)): sc.pt(i)
    for i in range(len(line_cases)): sc.ln(i)
    m = sc.link()
    rows = [R.LM.tie_rows(N, t, i) for i, (N, t) in enumerate(point_cases)], [R.LM.tie_rows(N, t, i, dim) for i, (N, t) in enumerate(line_cases)]
    for s, k in m["keyframes"].items():
        k["desc"] = np.array([rows[0][i][s] for i in k["points"]], np.uint32).reshape(-1, 8)
        k["ldesc"] = np.array([rows[1][i][s] for i in k["lines"]], np.float32).reshape(-1, dim)
    return m


def test_identical_rows_elect_the_first_kept(gpu_ctx):
    sizes = [2, 3, 64, 65, 66, 257, RS.MAX_OBS]          # stored rows; kept: one less - both kernels at their ends, a lane's second row, the limit
    m = tie_map([(N, 0) for N in sizes], [], first_bad=True)
    slots = list(range(len(sizes)))
    exp = R.refresh_points(m, slots, R.DESCRIPTOR)
    assert np.all(exp["best_obs"] == 1) and np.all(exp["best_median"] == 0) and np.all(exp["updated"] == R.DESCRIPTOR)
    with fresh(gpu_ctx, m) as dm:
        refresh_points_checked(gpu_ctx, dm, m, slots, R.DESCRIPTOR, "identical rows")


# (N, t): rf_point_wave; rf_point_block at its first size, then at the limit: the first lane of the second wavefront, the last lane, a lane's
# second row, and a row inside the second trip
@pytest.mark.parametrize("N,t", [(64, 31), (65, 32), (RS.MAX_OBS, 64), (RS.MAX_OBS, 255), (RS.MAX_OBS, 256), (RS.MAX_OBS, 300)])
def test_the_first_of_equal_medians_wins_at_row(gpu_ctx, N, t):
    m = tie_map([(N, t)], [], first_bad=False)
    exp = R.refresh_points(m, [0], R.DESCRIPTOR)
    assert exp["best_obs"].tolist() == [t] and exp["best_median"].tolist() == [0]                          # the scene does what it claims
    sc, _, _ = R.gather_points(m, [0], R.DESCRIPTOR, None)
    assert R.LM.select_from_table(R.LM.hamming_table(sc["obs_desc"]), False)[2][:t].min() > 0              # ... and every outlier's median is positive
    with fresh(gpu_ctx, m) as dm:
        refresh_points_checked(gpu_ctx, dm, m, [0], R.DESCRIPTOR, "row %d of %d" % (t, N))


@pytest.mark.parametrize("dim", [33, 128])
def test_line_ties(gpu_ctx, dim):
    m = tie_map([], [(2, 0), (RS.MAX_LINE_OBS, 0)], first_bad=True, dim=dim)
    exp = R.refresh_lines(m, [0, 1], dim)
    assert np.all(exp["best_obs"] == 1) and np.all(exp["best_median"] == 0) and np.all(exp["updated"] == R.DESCRIPTOR)
    with fresh(gpu_ctx, m, dim) as dm:
        refresh_lines_checked(gpu_ctx, dm, m, [0, 1], dim, "identical line rows, dim %d" % dim)
    m = tie_map([], [(RS.MAX_LINE_OBS, 31)], first_bad=False, dim=dim)
    exp = R.refresh_lines(m, [0], dim)
    assert exp["best_obs"].tolist() == [31] and exp["best_median"].tolist() == [0]
    assert R.LM.select_from_table(R.LM.l2_table(R.LM.tie_rows(RS.MAX_LINE_OBS, 31, 0, dim)), True)[2][:31].min() > 0
    with fresh(gpu_ctx, m, dim) as dm:
        refresh_lines_checked(gpu_ctx, dm, m, [0], dim, "line row 31, dim %d" % dim)


# ---------------------------------------------------------------------------------------------------------------- 3. guards
def guard_scene():
    sc = S.Scene()
    sc.kf(0, 1, [0, 1, 2, 3, 4]); sc.kf(1, 2, [4, 3, 2, 1, 0]); sc.kf(2, 3, [0, 1, 2, 3, 4], features=False); sc.kf(3, 4, [9])
    sc.pt(0, obs=[(0, 0), (1, 99)])                                        # a stored index beyond the observer's descriptor row
    sc.pt(1, obs=[(0, 1), (1, 3)], indexed=False)                           # no index row
    sc.pt(2, obs=[(0, 2), (1, 2)])                                          # reference -1
    sc.pt(3, obs=[(0, 3), (1, 1), (2, 3)])                                  # an observer without a centre
    sc.pt(4, obs=[(0, 4), (1, 0)])                                          # sound
    m = RS.dress(sc.link(), 0, never_set=0)
    for p in range(5): m["points"][p]["ref_kf"] = 0
    m["points"][2]["ref_kf"] = -1
    return m


def test_guards_flag_and_leave_the_landmark_alone(gpu_ctx):
    m = guard_scene()
    with fresh(gpu_ctx, m) as dm:
        before = dm.download_points([0, 1, 2, 3, 4])
        got = refresh_points_checked(gpu_ctx, dm, m, [0, 1, 2, 3, 4], BOTH, "guards")
        assert got["updated"].tolist() == [R.NO_DESCRIPTOR, R.NO_INDEX, R.NO_REFERENCE, R.NO_REFERENCE, BOTH]
        after = dm.download_points([0, 1, 2, 3, 4])
        for k in before:
            assert before[k][:4].tobytes() == after[k][:4].tobytes(), k
        assert before["desc"][4].tobytes() != after["desc"][4].tobytes() and before["normal"][4].tobytes() != after["normal"][4].tobytes()
        # each part alone reads only what it needs
        d = dm.refresh_points([0, 1, 2, 3], R.DESCRIPTOR)["updated"].tolist()
        assert d == [R.NO_DESCRIPTOR, R.NO_INDEX, R.DESCRIPTOR, R.DESCRIPTOR]


def test_a_map_without_the_optional_tables(gpu_ctx):
    """no descriptor pools, no point refs, no BA tables: everything is flagged or returns early, nothing is followed"""
    sc = S.Scene()
    sc.kf(0, 1, [0, 1], [0], features=False, keypoints=False); sc.kf(1, 2, [1, 0], [0], features=False, keypoints=False)
    sc.pt(0); sc.pt(1, indexed=False); sc.ln(0, no_row=True)
    m = sc.link()
    with DeviceMap(gpu_ctx, **RS.limits(m)) as dm:
        S.upload_keyframes(dm, m); RS.upload_points(dm, m); RS.upload_lines(dm, m)
        dm.set_observations([0, 1], rows=[[0, 1], [0, 1]])
        assert dm.refresh_points([0, 1], BOTH, LS)["updated"].tolist() == [R.NO_INDEX, R.NO_INDEX]
        dm.set_observations_indexed([0], rows=[m["points"][0]["obs"]], n_obs=[2])
        assert dm.refresh_points([0, 1], BOTH, LS)["updated"].tolist() == [R.NO_DESCRIPTOR | R.NO_REFERENCE, R.NO_INDEX]
        got = dm.refresh_lines([0, 1])
        assert got["updated"].tolist() == [0, 0] and got["best_obs"].tolist() == [-1, -1]


# ---------------------------------------------------------------------------------------------------------------- 4., 5. what a call touches
def test_unnamed_slots_and_every_row_pool_stay(gpu_ctx):
    m, _ = S.random_map(4)
    RS.dress(m, 4)
    with fresh(gpu_ctx, m) as dm:
        sl = AS.all_slots(dm)
        rows0 = all_rows(dm); pts0, lns0 = fixed_rows(dm)
        named = sl["pt"][::2]; lnamed = sl["ln"][1::2]
        refresh_points_checked(gpu_ctx, dm, m, named, BOTH, "half the points")
        refresh_lines_checked(gpu_ctx, dm, m, lnamed, S.LINE_DIM, "half the lines")
        assert all_rows(dm) == rows0
        pts1, lns1 = fixed_rows(dm)
        for k in pts0:
            assert pts0[k][1::2].tobytes() == pts1[k][1::2].tobytes(), k
        for k in ("pos", "state"):
            assert pts0[k].tobytes() == pts1[k].tobytes(), k
        assert pts0["desc"][::2].tobytes() != pts1["desc"][::2].tobytes()
        for k in lns0:
            assert lns0[k][::2].tobytes() == lns1[k][::2].tobytes(), k
        same(pts1, model_points(m, sl["pt"]), ("normal", "min_distance", "max_distance", "desc"), "named")
        same(lns1, model_lines(m, sl["ln"], S.LINE_DIM), ("desc",), "named lines")


def test_the_result_does_not_depend_on_the_query_list(gpu_ctx):
    m, _ = S.random_map(6)
    RS.dress(m, 6)
    with fresh(gpu_ctx, m) as dm:
        sl = AS.all_slots(dm)
        rng = np.random.default_rng(6)
        a = np.array(sl["pt"]); b = rng.permutation(a); c = b[: len(b) // 3]
        ra = dm.refresh_points(a, BOTH, LS); ta = dm.download_points(sl["pt"])
        RS.upload_points(dm, m)                                             # the uploaded values again
        rb = dm.refresh_points(b, BOTH, LS); tb = dm.download_points(sl["pt"])
        RS.upload_points(dm, m)
        rc = dm.refresh_points(c, BOTH, LS); tc = dm.download_points(c)
        for k in POINT_KEYS:
            assert ra[k][b].tobytes() == rb[k].tobytes() and ra[k][c].tobytes() == rc[k].tobytes(), k
        for k in ta:
            assert ta[k].tobytes() == tb[k].tobytes() and ta[k][c].tobytes() == tc[k].tobytes(), k
        la = dm.refresh_lines(sl["ln"]); RS.upload_lines(dm, m)
        lb = dm.refresh_lines(sl["ln"][::-1])
        for k in LINE_KEYS:
            assert la[k][::-1].tobytes() == lb[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- 6. the new pools repack
def tail_passes_cap(limit, rows, grown, per):
    """RowPool's arithmetic: rows of `rows` entries packed at first, then one row replaced by each length of `grown` (every one longer than
    its capacity, so it goes to the tail): True when the tail passes twice the limit, i.e. the pool is repacked"""
    tail = per * sum(rows)
    for n in grown:
        tail += per * n
        if tail > 2 * limit:
            return True
    return False


def test_descriptor_rows_survive_a_repack(gpu_ctx):
    sc = S.Scene()
    for s in range(3): sc.kf(s, s + 1, [0, 1, 2, 3], [0, 1])
    for p in range(4): sc.pt(p)
    for l in range(2): sc.ln(l, n_obs=6)
    m = RS.dress(sc.link(), 9, never_set=0)
    for p in range(4): m["points"][p]["ref_kf"] = p % 3
    L = RS.limits(m)
    grown_p, grown_l = list(range(5, 13)), list(range(3, 9))
    assert tail_passes_cap(8 * L["max_kf_points"], [4, 4, 4], grown_p, 8) and tail_passes_cap(S.LINE_DIM * L["max_kf_lines"], [2, 2, 2], grown_l, S.LINE_DIM)
    rng = np.random.default_rng(9)
    with fresh(gpu_ctx, m) as dm:
        for step in range(len(grown_p)):
            np_, nl_ = grown_p[step], grown_l[min(step, len(grown_l) - 1)]
            k = S.Scene().kf(0, 1, [0, 1, 2, 3] + [-1] * (np_ - 4), [0, 1] + [-1] * (nl_ - 2))
            k["desc"] = rng.integers(0, 2 ** 32, (np_, 8), dtype=np.uint64).astype(np.uint32)
            k["ldesc"] = (rng.normal(0, 1, (nl_, S.LINE_DIM)) * 50).astype(np.float32)
            m["keyframes"][0] = k
            S.upload_keyframes(dm, m, [0]); RS.upload_descriptors(dm, m, [0])
            refresh_points_checked(gpu_ctx, dm, m, [3, 1, 0, 2], BOTH, "row of %d" % np_)
            refresh_lines_checked(gpu_ctx, dm, m, [1, 0], S.LINE_DIM, "line row of %d" % nl_)
        # a row that no longer matches the keyframe's point row is refused, one past the pool's limit too; nothing changes
        before = fixed_rows(dm)
        for bad in (np.zeros((3, 8), np.uint32), np.zeros((13, 8), np.uint32)):
            with pytest.raises(RuntimeError, match="lld_map_set_keyframe_descriptors") as e:
                dm.set_keyframe_descriptors([0], [bad])
            assert e.value.status == abi.LLD_ERR_INVALID
        with pytest.raises(RuntimeError, match="lld_map_set_keyframe_line_descriptors") as e:
            dm.set_keyframe_line_descriptors([0, 0], [m["keyframes"][0]["ldesc"]] * 2)
        assert e.value.status == abi.LLD_ERR_INVALID
        got = dm.refresh_points([0, 1, 2, 3], BOTH, LS)
        same(got, R.refresh_points(m, [0, 1, 2, 3], BOTH, LS), POINT_KEYS, "after the refusals")
        # lld_map_clear empties the pools: every live observer is then without a descriptor row
        dm.clear(); RS.upload(dm, dict(m, keyframes={s: {k: v for k, v in kf.items() if k not in ("desc", "ldesc")} for s, kf in m["keyframes"].items()}))
        assert dm.refresh_points([0], R.DESCRIPTOR)["updated"].tolist() == [R.NO_DESCRIPTOR]
        assert dm.refresh_lines([0])["updated"].tolist() == [R.NO_DESCRIPTOR]
        assert before[0]["state"].tolist() == fixed_rows(dm)[0]["state"].tolist()


# ---------------------------------------------------------------------------------------------------------------- 7. downstream
def test_a_staged_ba_window_is_stale_after_a_refresh(gpu_ctx):
    import map_ba_ref as BR
    from lld_slam_amd import host
    m, q = S.random_map(5, n_kf=8)
    RS.dress(m, 5, never_set=0)
    se3 = lambda T: host.se3_from_tcw_f32(abi.product(), T)
    win = BR.ba_window(m, q, S.SIGMA2, se3)
    res = AS.crafted(win, 5, se3_from_tcw=se3)
    with fresh(gpu_ctx, m) as dm:
        assert dm.ba_window(q, S.CAM, S.SIGMA2)["status"] == 0
        assert dm.refresh_points([dm.limits.max_points - 1], BOTH, LS)["updated"].tolist() == [0]      # a never-set slot: nothing written, the window stays
        dm.ba_apply(res, LS, n_local_cams=win["n_local_cams"])
        RS.upload(dm, m)
        assert dm.ba_window(q, S.CAM, S.SIGMA2)["status"] == 0
        live = [s for s, p in m["points"].items() if not p["bad"] and p["obs"]][:3]
        assert dm.refresh_points(live, R.DESCRIPTOR)["updated"].tolist() == [R.DESCRIPTOR] * 3
        with pytest.raises(RuntimeError, match="lld_map_ba_apply") as e:
            dm.ba_apply(res, LS, n_local_cams=win["n_local_cams"])
        assert e.value.status == abi.LLD_ERR_INVALID
        assert dm.ba_window(q, S.CAM, S.SIGMA2)["status"] == 0
        assert dm.refresh_lines(sorted(m["lines"]))["updated"].any()
        with pytest.raises(RuntimeError, match="lld_map_ba_apply"):
            dm.ba_apply(res, LS, n_local_cams=win["n_local_cams"])


def test_the_frame_chain_reads_the_refreshed_rows(gpu_ctx):
    """UpdateLocalMap + stage 2 on the refreshed map equal the same chain on a fresh map that was sent the refreshed values"""
    import local_map_scenes as SC
    from lld_slam_amd import synth
    from lld_slam_amd.tracking import DeviceTrackedFrame
    import test_gpu_local_map_chain as CH
    sc = CH.scene()
    stage1 = CH.motion_model(sc)
    r1 = CH.stage1_record(gpu_ctx, sc, stage1)
    held = np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"])
    lm = SC.make_map(sc, held, 0)
    K = lm["keyframes"]
    rng = np.random.default_rng(21)
    pd, ld = SC.point_data(sc), SC.line_data(sc)
    dim = sc["lines"]["desc"].shape[1]
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    Tg = np.asarray(sc["Tcw_guess"], np.float32).reshape(4, 4)

    def chain(dm):
        with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc.get("lines")) as tf:
            stage1(tf); tf.update_local_map(dm); tf.track_local_map_resident(dm)
            return tf.local_map_download(dm)

    slots = sorted(K)
    pts = sorted(lm["points"]); lns = sorted(lm["lines"])
    with CH.open_map(gpu_ctx, sc, lm) as dm:
        # what the refresh reads beyond the local map's tables: index rows, octaves, poses near the frame's, mpRefKF, descriptor rows
        first = {s: {} for s in slots}
        for s in slots:
            for i, p in enumerate(K[s]["points"]):
                if p >= 0: first[s].setdefault(p, i)
        lfirst = {s: {l: i for i, l in reversed(list(enumerate(K[s]["lines"])))} for s in slots}
        dm.set_observations_indexed(pts, rows=[[(kf, first[kf][p]) for kf in lm["points"][p]["obs"]] for p in pts], n_obs=[len(lm["points"][p]["obs"]) for p in pts])
        dm.set_keyframe_keypoints(slots, [rng.integers(0, 8, len(K[s]["points"])).tolist() for s in slots], [[0.0] * len(K[s]["points"]) for s in slots], [0.0] * len(slots))
        poses = []
        for s in slots:
            T = Tg.copy(); T[:3, 3] += rng.normal(0, 0.05, 3).astype(np.float32); poses.append(T)
        dm.set_keyframe_features(slots, list(range(1, len(slots) + 1)), poses, [np.zeros((len(K[s]["points"]), 3), np.float32) for s in slots],
                                 [np.zeros((len(K[s]["lines"]), 4), np.float32) for s in slots], [np.zeros((len(K[s]["lines"]), 4), np.float32) for s in slots],
                                 [np.zeros((len(K[s]["lines"]), 2), np.int32) for s in slots])
        dm.set_point_refs(pts, [lm["points"][p]["obs"][0] if lm["points"][p]["obs"] else -1 for p in pts])
        lobs = {l: [(s, lfirst[s][l]) for s in slots if l in lfirst[s]] for l in lns}
        dm.set_line_observations(lns, [lobs[l] for l in lns], [2 * len(lobs[l]) for l in lns])
        dm.set_keyframe_descriptors(slots, [np.array([RS.flipped(rng, pd[p]["desc"], 12) if p >= 0 else np.zeros(8, np.uint32) for p in K[s]["points"]], np.uint32).reshape(-1, 8)
                                            for s in slots])
        dm.set_keyframe_line_descriptors(slots, [np.array([ld[l]["desc"] + rng.normal(0, 0.02, dim) if l >= 0 else np.zeros(dim) for l in K[s]["lines"]], np.float32).reshape(-1, dim)
                                                 for s in slots])
        named = pts[::2]
        rp = dm.refresh_points(named, BOTH, scale)
        rl = dm.refresh_lines(lns)
        assert np.count_nonzero(rp["updated"] == BOTH) > 50 and np.count_nonzero(rl["updated"] == R.DESCRIPTOR) > 20
        got = chain(dm)
    with CH.open_map(gpu_ctx, sc, lm) as dm:
        dm.set_points(named, np.array([pd[p]["world_pos"] for p in named], np.float32), rp["normal"], rp["min_distance"], rp["max_distance"], rp["desc"],
                      [lm["points"][p]["bad"] for p in named])
        dm.set_lines(lns, *[np.array([ld[l][k] for l in lns], np.float64) for k in ("X0", "dir", "X1", "X2")], rl["desc"], [lm["lines"][l]["bad"] for l in lns])
        want = chain(dm)
    assert got["status"] == 0 and got["stage2_ran"] == 1 and got["n_local_points"] > 200
    for k in ("local_keyframes", "local_points", "local_lines"):
        assert got[k].tolist() == want[k].tolist(), k
    assert got["ref_keyframe"] == want["ref_keyframe"]
    assert got["stages"][1]["n_search"] > 20 and got["stages"][1]["n_inliers"] > 20
    for a, b, what in zip(got["stages"], want["stages"], ("stage 1", "stage 2")):
        SC.same_dict(a, b, what)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_change_nothing(gpu_ctx):
    m, _ = S.random_map(7)
    RS.dress(m, 7)
    with fresh(gpu_ctx, m) as dm:
        before = fixed_rows(dm), all_rows(dm)
        live = [s for s, p in m["points"].items() if not p["bad"] and p["obs"]][:4]
        lines = sorted(m["lines"])[:3]

        def refused(call, name):
            with pytest.raises(RuntimeError, match=name) as e:
                call()
            assert e.value.status == abi.LLD_ERR_INVALID
        P = "lld_map_refresh_points"
        refused(lambda: dm.refresh_points(live + live[:1], BOTH, LS), P)                     # a slot named twice
        refused(lambda: dm.refresh_points(live, 0, LS), P)                                   # flags zero
        refused(lambda: dm.refresh_points(live, 4 | BOTH, LS), P)                            # an unknown bit
        refused(lambda: dm.refresh_points(live, BOTH, LS, omit=("updated",)), P)             # NULL updated
        refused(lambda: dm.refresh_points(live, BOTH, np.zeros(0, np.float32)), P)           # n_levels = 0
        refused(lambda: dm.refresh_points(live, BOTH, np.ones(abi.ORB_MAX_LEVELS + 1, np.float32)), P)   # one past LLD_ORB_MAX_LEVELS
        refused(lambda: dm.refresh_points(live, R.NORMAL_DEPTH, None), P)                    # no level table
        refused(lambda: dm.refresh_points(live + [dm.limits.max_points], BOTH, LS), P)       # out of range
        refused(lambda: dm.refresh_points(live + [-1], BOTH, LS), P)
        Lr = "lld_map_refresh_lines"
        refused(lambda: dm.refresh_lines(lines + lines[:1]), Lr)
        refused(lambda: dm.refresh_lines(lines, omit=("updated",)), Lr)
        refused(lambda: dm.refresh_lines([dm.limits.max_lines]), Lr)
        refused(lambda: dm.download_points([dm.limits.max_points]), "lld_map_download_points")
        refused(lambda: dm.download_lines([-1]), "lld_map_download_lines")
        after = fixed_rows(dm), all_rows(dm)
        for x, y in zip(before[0], after[0]):
            for k in x:
                assert x[k].tobytes() == y[k].tobytes(), k
        assert before[1] == after[1]
        # n = 0, and every optional output left out
        assert dm.refresh_points([], BOTH, LS)["updated"].size == 0 and dm.refresh_lines([])["updated"].size == 0
        assert dm.download_points([])["state"].size == 0 and dm.download_lines([])["bad"].size == 0
        got = dm.refresh_points(live, BOTH, LS, omit=POINT_KEYS[:-1])
        assert list(got) == ["updated"] and got["updated"].tolist() == R.refresh_points(m, live, BOTH, LS)["updated"].tolist()
        assert dm.refresh_lines(lines, omit=LINE_KEYS[:-1])["updated"].tolist() == R.refresh_lines(m, lines, S.LINE_DIM)["updated"].tolist()
        ms = np.zeros(3, np.float32)
        dm.refresh_points(live, BOTH, LS, phase_ms=ms)
        assert (ms >= 0).all() and ms.sum() > 0
