"""tests/landmark_ref.py pinned on its own (CPU): the median index and the first-of-equals rule against hand-worked tables, the
vectorised selection against the reference's loops written out, the normal and distances against a float64 evaluation, the
bad-keyframe asymmetry between the two routines, and the conditions that keep the GPU tests honest."""
import numpy as np
import pytest

import landmark_ref as L


def rows_with_distances(first_row):
    """N descriptors with DescriptorDistance(0, j) = first_row[j] and disjoint flipped bits: d(i, j) = first_row[i] + first_row[j]."""
    rows = np.zeros((len(first_row), 8), np.uint32)
    bit = 0
    for j, d in enumerate(first_row):
        for _ in range(d):
            rows[j, bit >> 5] |= np.uint32(1 << (bit & 31))
            bit += 1
    return rows


def test_median_index_table():
    assert [L.median_index(N) for N in range(1, 7)] == [0, 0, 1, 1, 2, 2]
    assert [L.median_index(N) for N in (63, 64, 65, 1024)] == [31, 31, 32, 511]


# first_row -> (winner, median), worked by hand from d(i, j) = a_i + a_j, d(i, i) = 0
HAND = [
    ([0], 0, 0),                             # N = 1: the diagonal
    ([0, 9], 0, 0),                          # N = 2: index 0 is the diagonal zero of either row; the first wins
    ([0, 2, 4], 0, 2),                       # rows sorted: [0,2,4] [0,2,6] [0,4,6] -> medians 2, 2, 4: first of equals
    ([5, 1, 3], 1, 4),                       # [0,6,8] [0,4,6] [0,4,8] -> 6, 4, 4: row 1 before row 2
    ([4, 3, 0, 2], 2, 2),                    # index 1: [0,4,6,7] [0,3,5,7] [0,2,3,4] [0,2,5,6] -> 4, 3, 2, 2
    ([1, 1, 1, 1, 1], 0, 2),                 # index 2: every row [0,2,2,2,2]
    ([6, 2, 4, 0, 2, 8], 3, 2),              # index 2: row 3 = [0,2,2,4,6,8] -> 2; rows 1, 4 = [0,2,4,6,8,10] -> 4
]


@pytest.mark.parametrize("first_row,winner,median", HAND)
def test_selection_against_hand_tables(first_row, winner, median):
    rows = rows_with_distances(first_row)
    D = L.hamming_table(rows)
    a = np.array(first_row)
    assert np.array_equal(D, (a[:, None] + a[None, :]) * (1 - np.eye(len(a), dtype=int)))
    w, m, _ = L.select_from_table(D, False)
    assert (w, m) == (winner, median)
    assert L.select_point_loops(rows) == (winner, median)


def test_first_of_equal_medians_wins_not_the_last():
    rows = rows_with_distances([3, 3, 3, 3])
    assert L.select_from_table(L.hamming_table(rows), False)[:2] == (0, 6)
    rows = rows_with_distances([3, 1, 1, 5])                  # [0,4,4,8] [0,2,4,6] [0,2,4,6] [0,6,6,8] -> 4, 2, 2, 6
    assert L.select_from_table(L.hamming_table(rows), False)[:2] == (1, 2)


SC = L.make_point_scene(11, 400)
REF = L.refresh_map_points_ref(SC)


def test_vectorised_selection_equals_the_loops_row_for_row():
    for i in range(0, 120):
        r = L.distinctive(SC, i)
        kept = L.kept_positions(SC, i)
        if SC["bad"][i] or not kept:
            assert r is None
            continue
        rows = SC["obs_desc"][[SC["obs_start"][i] + k for k in kept]]
        w, m = L.select_point_loops(rows)
        assert (kept[w], m) == r[:2] and np.array_equal(rows[w], r[2])
    for scaled in (False, True):
        ls = L.make_line_scene(3, 40, dim=24, scaled=scaled)
        for i in range(40):
            r = L.distinctive(ls, i, lines=True)
            kept = L.kept_positions(ls, i)
            if ls["bad"][i] or not kept:
                assert r is None
                continue
            rows = ls["obs_desc"][[ls["obs_start"][i] + k for k in kept]]
            w, m = L.select_line_loops(rows)
            assert (kept[w], m) == r[:2]


def test_int_median_truncates_before_the_comparison():
    # medians 1.9 and 1.2 as floats: both truncate to 1, so row 0 keeps the win although row 1's float median is smaller
    D = np.array([[0, 1.9, 1.9], [1.9, 0, 1.2], [1.9, 1.2, 0]], np.float32)
    w, m, med = L.select_from_table(D, True)
    assert (w, m) == (0, 1) and list(med) == [1, 1, 1]
    assert int(np.argmin(np.partition(D, 1, axis=1)[:, 1])) == 1


def test_normal_and_distances_within_float_rounding_of_float64():
    checked = 0
    for i in range(len(SC["bad"])):
        r = L.normal_depth(SC, i)
        if r is None:
            assert SC["bad"][i] or SC["obs_start"][i] == SC["obs_start"][i + 1]
            continue
        n = SC["obs_start"][i + 1] - SC["obs_start"][i]
        e_n, e_min, e_max = L.normal_depth_f64(SC, i)
        # before the division by n every term carries at most 4 roundings of 2^-24 relative to a value <= 1 (the subtraction, its
        # effect on the norm, the reciprocal, the product) and every partial sum one relative to a value <= n; the reciprocal of n
        # and the last product add two: at most (4 + n/2 + 2) * 2^-24 after the division, below (n + 8) * 2^-24.
        assert np.all(np.abs(r[0] - e_n) <= (n + 8) * 2.0 ** -24)
        # dist: the subtraction, the cast of the norm; one product for max, one quotient more for min (relative 2^-24 each, + slack 1)
        assert abs(r[2] - e_max) <= 4 * 2.0 ** -24 * e_max and abs(r[1] - e_min) <= 5 * 2.0 ** -24 * e_min
        assert r[0].dtype == np.float32 and r[1].dtype == np.float32 and r[2].dtype == np.float32
        checked += 1
    assert checked > 300


def test_bad_keyframes_are_skipped_by_the_descriptor_rule_only():
    sc = L.make_point_scene(5, 6, n_kf=6, counts=[4] * 6, p_kf_bad=0, p_bad=0, p_all_bad=0)
    good = L.refresh_map_points_ref(sc)
    sc2 = dict(sc, kf_bad=np.ones(6, np.uint8))                # every observer bad
    out = L.refresh_map_points_ref(sc2)
    assert np.all(out["updated"] == L.NORMAL_DEPTH) and np.all(out["best_obs"] == -1)
    for k in ("normal", "min_distance", "max_distance"):       # the normal / depth rule does not look at isBad()
        assert np.array_equal(out[k].view(np.uint32), good[k].view(np.uint32))
    # one good observer, last in the list: best_obs counts the bad ones before it
    kb = np.ones(6, np.uint8); kb[sc["obs_kf"][3]] = 0
    out = L.refresh_map_points_ref(dict(sc, kf_bad=kb))
    assert out["best_obs"][0] == 3 and out["best_median"][0] == 0 and np.array_equal(out["desc"][0], sc["obs_desc"][3])


def test_generated_point_scenes_keep_the_gpu_tests_honest():
    n = len(SC["bad"])
    ties = non0 = 0
    for i in np.flatnonzero(REF["updated"] & 1):
        kept = L.kept_positions(SC, i)
        _, m, med = L.select_from_table(L.hamming_table(SC["obs_desc"][[SC["obs_start"][i] + k for k in kept]]), False)
        ties += int((med == m).sum() >= 2)
        non0 += int(REF["best_obs"][i] != kept[0])
    assert ties >= n / 4 and non0 >= n / 4
    assert np.any(SC["bad"]) and np.any(SC["kf_bad"])
    assert np.any((REF["updated"] == L.NORMAL_DEPTH) & (SC["bad"] == 0))       # a point whose every observer is bad
    assert len(set(np.diff(SC["obs_start"]).tolist())) > 10                    # ragged


def test_generated_line_scenes_keep_the_gpu_tests_honest():
    unit = L.make_line_scene(21, 200)
    r = L.distinctive_lines_ref(unit)
    u = r["updated"] > 0
    assert set(np.unique(r["best_median"][u]).tolist()) <= {0, 1}
    for i in np.flatnonzero(u):                                               # every integer median of every row, not only the best
        rows = unit["obs_desc"][[unit["obs_start"][i] + k for k in L.kept_positions(unit, i)]]
        assert set(L.select_from_table(L.l2_table(rows), True)[2].tolist()) <= {0, 1}
        assert r["best_obs"][i] == L.kept_positions(unit, i)[0]               # the first kept row wins
    scaled = L.make_line_scene(21, 200, scaled=True)
    r = L.distinctive_lines_ref(scaled)
    first = np.array([(L.kept_positions(scaled, i) or [-1])[0] for i in range(200)])
    assert np.sum((r["updated"] > 0) & (r["best_obs"] != first)) >= 200 / 4
