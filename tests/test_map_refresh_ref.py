"""tests/map_refresh_ref.py (the restatement the GPU tests of lld_map_refresh_* compare with) held to scenes worked out by hand.  CPU only."""
import numpy as np

import map_ba_scenes as S
import map_refresh_ref as R

f32 = np.float32
SCALE = np.array([1.0, 1.5, 2.0, 4.0], f32)


def low_bits(n):
    """a descriptor with its n lowest bits set: the distance of low_bits(a) and low_bits(b) is |a - b|"""
    d = np.zeros(8, np.uint32)
    for b in range(n):
        d[b >> 5] |= np.uint32(1 << (b & 31))
    return d


def scene(descs, bad=(), keys=None):
    """point 0 observed by keyframes 0 .. n-1 (keypoint 1 of each, keypoint 0 is point 9), stored in ascending key; descs[s] = low bits of
    keyframe s's row for it"""
    sc = S.Scene()
    for s, nb in enumerate(descs):
        k = sc.kf(s, s + 1, [9, 0], bad=s in bad, key=None if keys is None else keys[s])
        k["desc"] = np.stack([low_bits(200), low_bits(nb)])
    sc.pt(0); sc.pt(9)
    m = sc.link()
    m["points"][0].update(ref_kf=0, desc=low_bits(77))
    return m


def test_three_observers_the_middle_median_wins():
    # rows 0, 10 and 8 bits: distances 0-1 = 10, 0-2 = 8, 1-2 = 2.  N = 3, index (int)(0.5 * 2) = 1 of each sorted row:
    # row 0 (0, 8, 10) -> 8; row 1 (0, 2, 10) -> 2; row 2 (0, 2, 8) -> 2.  The first strictly smallest: row 1, median 2.
    m = scene([0, 10, 8])
    out = R.refresh_points(m, [0], R.DESCRIPTOR)
    assert (out["best_obs"][0], out["best_median"][0], out["updated"][0]) == (1, 2, R.DESCRIPTOR)
    assert np.array_equal(out["desc"][0], low_bits(10))


def test_of_two_equal_medians_the_first_in_row_order_wins():
    # the same rows stored in the order 2, 1, 0 (descending key): rows 8, 10, 0 bits -> medians 2, 2, 8: position 0 (keyframe 2) wins
    m = scene([0, 10, 8], keys=[30, 20, 10])
    assert [o[0] for o in m["points"][0]["obs"]] == [2, 1, 0]
    out = R.refresh_points(m, [0], R.DESCRIPTOR)
    assert (out["best_obs"][0], out["best_median"][0]) == (0, 2)
    assert np.array_equal(out["desc"][0], low_bits(8))


def test_a_bad_observer_changes_the_winner():
    # rows 0, 10, 8, 0 bits.  N = 4, index (int)1.5 = 1: row 0 sorted (0, 0, 8, 10) -> 0: position 0 wins with median 0.
    m = scene([0, 10, 8, 0])
    out = R.refresh_points(m, [0], R.DESCRIPTOR)
    assert (out["best_obs"][0], out["best_median"][0]) == (0, 0)
    # keyframe 3 bad: the three rows of the first test; the position counts the bad observer's entry too (here it is behind the winner)
    out = R.refresh_points(scene([0, 10, 8, 0], bad=[3]), [0], R.DESCRIPTOR)
    assert (out["best_obs"][0], out["best_median"][0]) == (1, 2)
    # keyframe 0 bad: rows 10, 8, 0 bits -> sorted rows (0, 2, 10), (0, 2, 8), (0, 8, 10): stored position 1 (keyframe 1) wins
    out = R.refresh_points(scene([0, 10, 8, 0], bad=[0]), [0], R.DESCRIPTOR)
    assert (out["best_obs"][0], out["best_median"][0]) == (1, 2) and np.array_equal(out["desc"][0], low_bits(10))


def test_all_observers_bad_nothing_is_written_but_the_normal_counts_them():
    m = scene([0, 10, 8], bad=[0, 1, 2])
    out = R.refresh_points(m, [0], R.DESCRIPTOR | R.NORMAL_DEPTH, SCALE)
    assert (out["best_obs"][0], out["best_median"][0], out["updated"][0]) == (-1, -1, R.NORMAL_DEPTH)
    assert np.array_equal(out["desc"][0], low_bits(77))                    # what the point held
    out = R.refresh_points(m, [0], R.DESCRIPTOR)
    assert out["updated"][0] == 0


def test_normal_and_depth_of_one_observer_by_hand():
    # keyframe 2's centre is -(2, 4, 6); the point 3 along x and 4 along z from it: normal (0.6, 0, 0.8), distance 5.  The point is keypoint 1
    # of keyframe 2: octave 1, scale 1.5 -> max 7.5, min 7.5 / 4
    sc = S.Scene()
    sc.kf(2, 1, [9, 0]); sc.pt(0); sc.pt(9)
    m = sc.link()
    m["points"][0].update(pos=np.array([1, -4, -2], f32), ref_kf=2)
    out = R.refresh_points(m, [0], R.NORMAL_DEPTH, SCALE)
    assert out["updated"][0] == R.NORMAL_DEPTH
    assert np.array_equal(out["normal"][0], np.array([f32(3) * f32(0.2), 0, f32(4) * f32(0.2)], f32))
    assert (out["max_distance"][0], out["min_distance"][0]) == (f32(7.5), f32(7.5) / f32(4))


def test_a_reference_keyframe_that_is_no_observer_reads_keypoint_0():
    sc = S.Scene()
    sc.kf(1, 1, [5, 5, 0]); sc.kf(2, 2, [0]); sc.kf(3, 3, [6, 6, 6, 6])
    for p in (0, 5, 6): sc.pt(p)
    m = sc.link()
    m["keyframes"][3]["octave"] = [3, 1, 1, 1]
    dist = f32(np.sqrt(3.0 ** 2 + 6.5 ** 2 + 9.25 ** 2))                   # (0, 0.5, 0.25) - -(3, 6, 9)
    m["points"][0]["ref_kf"] = 3
    out = R.refresh_points(m, [0], R.NORMAL_DEPTH, SCALE)
    assert (out["max_distance"][0], out["min_distance"][0], out["updated"][0]) == (f32(dist * f32(4)), f32(f32(dist * f32(4)) / f32(4)), R.NORMAL_DEPTH)
    # an observer as reference: keyframe 1 holds the point at keypoint 2, octave 2
    m["points"][0]["ref_kf"] = 1
    d1 = f32(np.sqrt(1.0 ** 2 + 2.5 ** 2 + 3.25 ** 2))
    out = R.refresh_points(m, [0], R.NORMAL_DEPTH, SCALE)
    assert out["max_distance"][0] == f32(d1 * f32(2))


def test_the_flag_rules():
    m = scene([0, 10, 8])
    m["points"][0]["ref_kf"] = -1
    out = R.refresh_points(m, [0], R.DESCRIPTOR | R.NORMAL_DEPTH, SCALE)
    assert out["updated"][0] == R.NO_REFERENCE and np.array_equal(out["desc"][0], low_bits(77))     # not written at all
    assert R.refresh_points(m, [0], R.DESCRIPTOR)["updated"][0] == R.DESCRIPTOR                      # the descriptor part alone does not read it
    m = scene([0, 10, 8])
    m["points"][0]["obs"][1] = (1, 2)                                        # one past keyframe 1's descriptor rows
    assert R.refresh_points(m, [0], R.DESCRIPTOR | R.NORMAL_DEPTH, SCALE)["updated"][0] == R.NO_DESCRIPTOR
    m["points"][0]["ref_kf"] = 1                                             # ... and, as the reference, one past its octaves
    assert R.refresh_points(m, [0], R.DESCRIPTOR | R.NORMAL_DEPTH, SCALE)["updated"][0] == R.NO_DESCRIPTOR | R.NO_REFERENCE
    m["keyframes"][1]["bad"] = 1                                             # a bad observer's row is not read
    assert R.refresh_points(m, [0], R.DESCRIPTOR)["updated"][0] == R.DESCRIPTOR
    m = scene([0, 10, 8]); m["points"][0]["indexed"] = False
    assert R.refresh_points(m, [0], R.DESCRIPTOR | R.NORMAL_DEPTH, SCALE)["updated"][0] == R.NO_INDEX
    m = scene([0, 10, 8]); del m["keyframes"][2]["uvr"]                       # an observer without a centre
    assert R.refresh_points(m, [0], R.NORMAL_DEPTH, SCALE)["updated"][0] == R.NO_REFERENCE
    m = scene([0, 10, 8]); m["points"][0]["bad"] = 1
    assert R.refresh_points(m, [0, 4], R.DESCRIPTOR | R.NORMAL_DEPTH, SCALE)["updated"].tolist() == [0, 0]       # bad, never set


def test_the_line_median_is_truncated_before_it_is_compared():
    # one-dimensional rows 0, 1.7, 2.9: distances 1.7, 2.9, 1.2.  Sorted rows (0, 1.7, 2.9), (0, 1.2, 1.7), (0, 1.2, 2.9): the float medians
    # 1.7, 1.2, 1.2 would elect row 1; `int median` makes them 1, 1, 1 and the first row stays
    sc = S.Scene()
    for s, v in enumerate((0.0, 1.7, 2.9)):
        sc.kf(s, s + 1, [], [0])["ldesc"] = np.array([[v, 0.0]], f32)
    sc.ln(0)
    m = sc.link()
    m["lines"][0]["desc"] = np.array([9, 9], f32)
    out = R.refresh_lines(m, [0, 1], 2)
    assert (out["best_obs"][0], out["best_median"][0]) == (0, 1) and out["updated"].tolist() == [R.DESCRIPTOR, 0]
    assert np.array_equal(out["desc"][0], np.array([0, 0], f32))
    # rows 0, 2.6, 2.9: medians 2.6, 0.3 (b-c), 0.3 -> ints 2, 0, 0: row 1
    m["keyframes"][1]["ldesc"] = np.array([[2.6, 0.0]], f32)
    out = R.refresh_lines(m, [0], 2)
    assert (out["best_obs"][0], out["best_median"][0]) == (1, 0)
    # a live observer without a descriptor row: flagged, the line keeps its row
    del m["keyframes"][2]["ldesc"]
    out = R.refresh_lines(m, [0], 2)
    assert out["updated"][0] == R.NO_DESCRIPTOR and np.array_equal(out["desc"][0], np.array([9, 9], f32))


def test_write_back():
    m = scene([0, 10, 8])
    out = R.refresh_points(m, [0, 9], R.DESCRIPTOR | R.NORMAL_DEPTH, SCALE)
    R.write_points(m, [0, 9], out)
    assert np.array_equal(m["points"][0]["desc"], low_bits(10)) and m["points"][0]["maxd"] == out["max_distance"][0]
    assert out["updated"][1] == R.NO_REFERENCE and "desc" not in m["points"][9]       # point 9 has no reference keyframe
