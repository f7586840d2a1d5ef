"""lld_mappoint_refresh / lld_mapline_distinctive on the device against tests/landmark_ref.py.  desc, best_obs, best_median and
updated are exact; normal, min_distance and max_distance are bit for bit equal (the device's double division, double square root
and float division are correctly rounded, include/lld_amd.h)."""
import functools

import numpy as np
import pytest

import landmark_ref as L
from lld_slam_amd import abi
from lld_slam_amd.landmarks import (DESCRIPTOR, MAX_LINE_DIM, MAX_LINE_OBS, MAX_OBS, NORMAL_DEPTH, LandmarkError,
                                    distinctive_line_descriptors, refresh_map_points)

pytestmark = pytest.mark.gpu
BOTH = DESCRIPTOR | NORMAL_DEPTH


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def run_points(ctx, sc, flags=BOTH, prior=None):
    prior = prior or {}
    return refresh_map_points(ctx, sc["obs_start"], sc["obs_kf"], sc["bad"], obs_desc=sc["obs_desc"], kf_bad=sc["kf_bad"],
                              kf_ow=sc["kf_ow"], pos=sc["pos"], ref_kf=sc["ref_kf"], ref_level=sc["ref_level"],
                              level_scale=sc["level_scale"], flags=flags, **prior)


def check_points(got, exp, what=""):
    assert np.array_equal(got.updated, exp["updated"]), what
    assert np.array_equal(got.best_obs, exp["best_obs"]) and np.array_equal(got.best_median, exp["best_median"]), what
    assert np.array_equal(got.desc, exp["desc"]), what
    for k in ("normal", "min_distance", "max_distance"):
        assert np.array_equal(bits(getattr(got, k)), bits(exp[k])), f"{what}: {k}"


def run_lines(ctx, sc, desc=None):
    return distinctive_line_descriptors(ctx, sc["obs_start"], sc["obs_kf"], sc["obs_desc"], sc["kf_bad"], sc["bad"], desc=desc, dim=sc["dim"])


def check_lines(got, exp, what=""):
    assert np.array_equal(got.updated, exp["updated"]), what
    assert np.array_equal(got.best_obs, exp["best_obs"]) and np.array_equal(got.best_median, exp["best_median"]), what
    assert np.array_equal(bits(got.desc), bits(exp["desc"])), what


@functools.lru_cache(maxsize=None)
def big_scene():
    sc = L.make_point_scene(7, 3000)
    return sc, L.refresh_map_points_ref(sc)


def kept_counts(sc):
    return [len(L.kept_positions(sc, i)) for i in range(len(sc["bad"]))]


def test_every_path_size(gpu_ctx):
    # N = 1, 2, 3, the last of the wavefront path and the first of the workgroup path, the limit; no bad keyframe: N = the count
    sc = L.make_point_scene(1, counts=[1, 2, 3, 63, 64, 65, 66, 130, 257, MAX_OBS], p_kf_bad=0, p_bad=0, p_all_bad=0)
    assert kept_counts(sc) == [1, 2, 3, 63, 64, 65, 66, 130, 257, MAX_OBS]
    exp = L.refresh_map_points_ref(sc)
    assert np.all(exp["best_obs"][:2] == 0) and np.all(exp["best_median"][:2] == 0) and np.all(exp["updated"] == BOTH)
    check_points(run_points(gpu_ctx, sc), exp)


def test_paths_are_chosen_by_kept_observations(gpu_ctx):
    # 81 keyframes, 16 bad: point 0 sees all (65 kept: workgroup path), point 1 sees 0..79 (80 listed, 64 kept: wavefront path,
    # compacted over two chunks of the list)
    sc = L.make_point_scene(2, counts=[81, 80], n_kf=81, p_kf_bad=0, p_bad=0, p_all_bad=0)
    sc["obs_kf"][81:] = np.arange(80)
    sc["kf_bad"][:] = 0
    sc["kf_bad"][3:19] = 1
    assert kept_counts(sc) == [65, 64]
    exp = L.refresh_map_points_ref(sc)
    assert exp["best_obs"][1] >= 0
    check_points(run_points(gpu_ctx, sc), exp)


def test_one_landmark(gpu_ctx):
    sc = L.make_point_scene(3, counts=[17], p_kf_bad=0.2, p_bad=0, p_all_bad=0)
    check_points(run_points(gpu_ctx, sc), L.refresh_map_points_ref(sc))


def test_3000_ragged_landmarks_in_one_call(gpu_ctx):
    sc, exp = big_scene()
    assert np.any(exp["updated"] == 0) and np.any(exp["updated"] == NORMAL_DEPTH) and np.sum(exp["updated"] == BOTH) > 2500
    check_points(run_points(gpu_ctx, sc), exp)


def test_early_returns_and_best_obs_counts_bad_keyframes(gpu_ctx):
    # points: 0 only good observer last; 1 every observer bad; 2 a bad point; 3 full; 4 empty; 5 full
    sc = L.make_point_scene(4, counts=[6, 5, 9, 12, 0, 7], n_kf=20, p_kf_bad=0, p_bad=0, p_all_bad=0)
    s = sc["obs_start"]
    sc["kf_bad"][:] = 0
    sc["kf_bad"][sc["obs_kf"][s[0]:s[1] - 1]] = 1
    sc["kf_bad"][sc["obs_kf"][s[0 + 1] - 1]] = 0
    # point 1 observes bad keyframes only: relist it on point 0's bad keyframes
    sc["obs_kf"][s[1]:s[2]] = sc["obs_kf"][s[0]:s[0] + 5]
    sc["bad"][2] = 1
    prior = dict(desc=np.full((6, 8), 0xABCD0123, np.uint32), normal=np.full((6, 3), -3.5, np.float32),
                 min_distance=np.full(6, 77.0, np.float32), max_distance=np.full(6, 99.0, np.float32))
    exp = L.refresh_map_points_ref(sc, prior=prior)
    assert exp["best_obs"][0] == 5 and exp["best_median"][0] == 0
    assert list(exp["updated"][[1, 2, 4]]) == [NORMAL_DEPTH, 0, 0] and list(exp["best_obs"][[1, 2, 4]]) == [-1, -1, -1]
    assert exp["updated"][3] == BOTH and exp["updated"][5] == BOTH
    got = run_points(gpu_ctx, sc, prior=prior)
    check_points(got, exp)
    assert np.all(got.desc[[1, 2, 4]] == 0xABCD0123) and np.all(got.normal[[2, 4]] == -3.5) and got.max_distance[4] == 99.0


def test_flags_select_each_part_alone(gpu_ctx):
    sc = L.make_point_scene(5, 120)
    n = len(sc["bad"])
    rng = np.random.default_rng(0)
    prior = dict(desc=rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32), normal=rng.normal(size=(n, 3)).astype(np.float32),
                 min_distance=rng.random(n).astype(np.float32), max_distance=rng.random(n).astype(np.float32))
    exp = L.refresh_map_points_ref(sc, DESCRIPTOR, prior)
    got = run_points(gpu_ctx, sc, DESCRIPTOR, prior)
    check_points(got, exp, "descriptor only")
    assert np.array_equal(bits(got.normal), bits(prior["normal"])) and np.array_equal(bits(got.max_distance), bits(prior["max_distance"]))
    assert not np.any(got.updated & NORMAL_DEPTH)
    exp = L.refresh_map_points_ref(sc, NORMAL_DEPTH, prior)
    got = run_points(gpu_ctx, sc, NORMAL_DEPTH, prior)
    assert got.best_obs is None and got.best_median is None
    assert np.array_equal(got.updated, exp["updated"]) and np.array_equal(got.desc, prior["desc"])
    for k in ("normal", "min_distance", "max_distance"):
        assert np.array_equal(bits(getattr(got, k)), bits(exp[k])), k
    # the part that is not selected needs none of its inputs
    got2 = refresh_map_points(gpu_ctx, sc["obs_start"], sc["obs_kf"], sc["bad"], kf_ow=sc["kf_ow"], pos=sc["pos"], ref_kf=sc["ref_kf"],
                              ref_level=sc["ref_level"], level_scale=sc["level_scale"], flags=NORMAL_DEPTH,
                              normal=prior["normal"], min_distance=prior["min_distance"], max_distance=prior["max_distance"])
    assert np.array_equal(bits(got2.normal), bits(got.normal)) and got2.desc is None


def test_result_does_not_depend_on_the_batch_order(gpu_ctx):
    sc = L.make_point_scene(6, counts=list(np.random.default_rng(6).integers(1, 50, 300)) + [70, 90, 300])
    a = run_points(gpu_ctx, sc)
    order = np.random.default_rng(1).permutation(len(sc["bad"]))
    b = run_points(gpu_ctx, L.subset(sc, order))
    for k in ("desc", "best_obs", "best_median", "updated"):
        assert np.array_equal(getattr(a, k)[order], getattr(b, k)), k
    for k in ("normal", "min_distance", "max_distance"):
        assert np.array_equal(bits(getattr(a, k)[order]), bits(getattr(b, k))), k
    check_points(a, L.refresh_map_points_ref(sc))
    half = order[:100]                        # and on which landmarks share the call
    c = run_points(gpu_ctx, L.subset(sc, half))
    assert np.array_equal(a.desc[half], c.desc) and np.array_equal(bits(a.normal[half]), bits(c.normal))


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dim", [72, 33])
def test_lines(gpu_ctx, scaled, dim):
    counts = [1, 2, 3, 63, MAX_LINE_OBS] + list(np.random.default_rng(dim).integers(0, 30, 150))
    sc = L.make_line_scene(30 + dim, dim=dim, scaled=scaled, counts=counts, n_kf=70)
    exp = L.distinctive_lines_ref(sc)
    u = exp["updated"] > 0
    if scaled:
        assert len(np.unique(exp["best_median"][u])) > 5
    else:
        assert set(np.unique(exp["best_median"][u]).tolist()) <= {0, 1}
    prior = np.full((len(counts), dim), 0.25, np.float32)
    exp = L.distinctive_lines_ref(sc, prior)
    got = run_lines(gpu_ctx, sc, prior)
    check_lines(got, exp)
    assert np.any(~u) and np.all(got.desc[~u] == 0.25)
    order = np.random.default_rng(2).permutation(len(counts))
    again = run_lines(gpu_ctx, L.subset(sc, order, lines=True), prior)
    assert np.array_equal(bits(got.desc[order]), bits(again.desc)) and np.array_equal(got.best_obs[order], again.best_obs)


def test_one_line_and_the_largest_dim(gpu_ctx):
    sc = L.make_line_scene(9, dim=MAX_LINE_DIM, scaled=True, counts=[40], n_kf=64, p_kf_bad=0.2, p_bad=0, p_all_bad=0)
    check_lines(run_lines(gpu_ctx, sc), L.distinctive_lines_ref(sc))


# Which row wins among equal medians, and at which lane: random 256-bit rows rarely tie, so these scenes make every candidate tie.
def run_descriptors(ctx, sc):
    return refresh_map_points(ctx, sc["obs_start"], sc["obs_kf"], sc["bad"], obs_desc=sc["obs_desc"], kf_bad=sc["kf_bad"], flags=DESCRIPTOR)


def check_descriptors(got, exp):
    assert np.array_equal(got.updated, exp["updated"]) and np.array_equal(got.desc, exp["desc"])
    assert np.array_equal(got.best_obs, exp["best_obs"]) and np.array_equal(got.best_median, exp["best_median"])


def test_identical_rows_elect_the_first_kept(gpu_ctx):
    # lists of N observers whose first keyframe is bad and whose rows are all the same: every median is 0, list position 1 wins
    sizes = [2, 3, 64, 65, 66, 257, MAX_OBS]              # kept: one less - both paths at their ends, a lane's second row, the limit
    sc = L.tie_scene([(N, 0) for N in sizes], first_bad=True)
    assert kept_counts(sc) == [N - 1 for N in sizes]
    exp = L.refresh_map_points_ref(sc, DESCRIPTOR)
    assert np.all(exp["best_obs"] == 1) and np.all(exp["best_median"] == 0) and np.all(exp["updated"] == DESCRIPTOR)
    check_descriptors(run_descriptors(gpu_ctx, sc), exp)


# (N, t): the wavefront path; the workgroup path at its first size, then at the limit: the first lane of the second wavefront, the last lane,
# a lane's second row, and a row inside the second trip
TIE_POINTS = [(64, 31), (65, 32), (MAX_OBS, 64), (MAX_OBS, 255), (MAX_OBS, 256), (MAX_OBS, 300)]


@pytest.mark.parametrize("N,t", TIE_POINTS)
def test_the_first_of_equal_medians_wins_at_row(gpu_ctx, N, t):
    sc = L.tie_scene([(N, t)], first_bad=False)
    exp = L.refresh_map_points_ref(sc, DESCRIPTOR)
    assert exp["best_obs"].tolist() == [t] and exp["best_median"].tolist() == [0]          # the scene does what it claims
    assert L.select_from_table(L.hamming_table(sc["obs_desc"]), False)[2][:t].min() > 0    # ... and every outlier's median is positive
    check_descriptors(run_descriptors(gpu_ctx, sc), exp)


@pytest.mark.parametrize("dim", [33, MAX_LINE_DIM])
def test_line_ties(gpu_ctx, dim):
    sc = L.tie_scene([(2, 0), (MAX_LINE_OBS, 0)], first_bad=True, dim=dim)
    exp = L.distinctive_lines_ref(sc)
    assert np.all(exp["best_obs"] == 1) and np.all(exp["best_median"] == 0) and np.all(exp["updated"] == DESCRIPTOR)
    check_lines(run_lines(gpu_ctx, sc), exp, "identical rows")
    sc = L.tie_scene([(MAX_LINE_OBS, 31)], first_bad=False, dim=dim)
    exp = L.distinctive_lines_ref(sc)
    assert exp["best_obs"].tolist() == [31] and exp["best_median"].tolist() == [0]
    assert L.select_from_table(L.l2_table(sc["obs_desc"]), True)[2][:31].min() > 0
    check_lines(run_lines(gpu_ctx, sc), exp, "row 31")


def status_of(fn):
    with pytest.raises(LandmarkError) as e:
        fn()
    return e.value.status


def test_refusals(gpu_ctx):
    sc = L.make_point_scene(8, 10, p_bad=0, p_all_bad=0)
    INV, UNS = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED

    def with_(**kw):
        return lambda: run_points(gpu_ctx, dict(sc, **kw))

    start = sc["obs_start"].copy(); start[3] = start[4] + 1
    assert status_of(with_(obs_start=start)) == INV                                    # not monotone
    start = sc["obs_start"].copy(); start[0] = 1
    assert status_of(with_(obs_start=start)) == INV
    start = sc["obs_start"].copy(); start[-1] -= 1
    assert status_of(with_(obs_start=start)) == INV                                    # does not end at n_obs
    kf = sc["obs_kf"].copy(); kf[5] = len(sc["kf_bad"])
    assert status_of(with_(obs_kf=kf)) == INV
    kf = sc["obs_kf"].copy(); kf[0] = -1
    assert status_of(with_(obs_kf=kf)) == INV
    ref = sc["ref_kf"].copy(); ref[2] = len(sc["kf_bad"])
    assert status_of(with_(ref_kf=ref)) == INV
    lvl = sc["ref_level"].copy(); lvl[7] = sc["n_levels"]
    assert status_of(with_(ref_level=lvl)) == INV
    lvl = sc["ref_level"].copy(); lvl[7] = -1
    assert status_of(with_(ref_level=lvl)) == INV
    assert status_of(with_(level_scale=np.ones(17, np.float32))) == INV                # n_levels above LLD_ORB_MAX_LEVELS
    assert status_of(with_(level_scale=np.zeros(0, np.float32))) == INV                # n_levels = 0
    assert status_of(lambda: run_points(gpu_ctx, sc, 0)) == INV and status_of(lambda: run_points(gpu_ctx, sc, 4)) == INV
    for missing in ("obs_desc", "kf_bad", "kf_ow", "pos", "ref_kf", "ref_level"):      # NULL required pointers
        assert status_of(with_(**{missing: None})) == INV, missing
    # an out-of-range reference of a point the rule skips is never read
    ref = sc["ref_kf"].copy(); ref[2] = 10 ** 6
    bad = sc["bad"].copy(); bad[2] = 1
    got = run_points(gpu_ctx, dict(sc, ref_kf=ref, bad=bad))
    check_points(got, L.refresh_map_points_ref(dict(sc, bad=bad)))
    # above the limit: nothing is queued, nothing is written
    over = L.make_point_scene(9, counts=[4, MAX_OBS + 1], p_kf_bad=0, p_bad=0, p_all_bad=0)
    assert status_of(lambda: run_points(gpu_ctx, over)) == UNS
    assert status_of(lambda: run_points(gpu_ctx, over, NORMAL_DEPTH)) == UNS
    # n_points = 0 is fine
    empty = refresh_map_points(gpu_ctx, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8))
    assert len(empty.updated) == 0
    # lines
    ls = L.make_line_scene(10, 8, dim=16)
    assert status_of(lambda: run_lines(gpu_ctx, dict(ls, obs_kf=np.full_like(ls["obs_kf"], 99)))) == INV
    start = ls["obs_start"].copy(); start[2] = start[3] + 1
    assert status_of(lambda: run_lines(gpu_ctx, dict(ls, obs_start=start))) == INV
    assert status_of(lambda: run_lines(gpu_ctx, dict(ls, dim=0))) == INV
    over = L.make_line_scene(11, dim=8, counts=[MAX_LINE_OBS + 1])
    assert status_of(lambda: run_lines(gpu_ctx, over)) == UNS
    wide = L.make_line_scene(12, 3, dim=MAX_LINE_DIM + 1)
    assert status_of(lambda: run_lines(gpu_ctx, wide)) == UNS
    none = distinctive_line_descriptors(gpu_ctx, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 72), np.float32),
                                        np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    assert len(none.updated) == 0
