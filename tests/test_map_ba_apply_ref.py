"""The plain-Python restatement of lld_map_ba_apply (tests/map_ba_apply_ref.py) on scenes small enough that the outcome is written out by
hand here, from the rules in include/lld_amd.h and the docstrings of the scenes (tests/map_ba_apply_scenes.py).  The GPU tests hold the
device to the restatement; this file holds the restatement to paper.  CPU only (the library is loaded for its two pose conversions)."""
import numpy as np

import map_ba_apply_ref as A
import map_ba_apply_scenes as AS
import map_ba_ref as R
import map_ba_scenes as S
from lld_slam_amd import abi, host

f32 = np.float32


def run(name, move_lines=False):
    lib = abi.product()
    m, q, fl = AS.NAMED[name]()
    win = R.ba_window(m, q, S.SIGMA2, lambda T: host.se3_from_tcw_f32(lib, T))
    assert win["status"] == 0
    res = AS.flags_for(win, **fl)
    if move_lines:
        res["line_x0"] = res["line_x0"] + 1.0
    m2, out = A.apply(m, win, res, AS.LEVEL_SCALE, lambda qt: host.se3_to_tcw_f32(lib, qt))
    return m, m2, out, win


def rows(m2, what, key="points"):
    return {s: list(k[key]) for s, k in m2[what].items()} if what == "keyframes" else {s: list(p["obs"]) for s, p in m2[what].items()}


def test_a_point_that_lands_on_three_and_one_that_lands_on_two():
    m, m2, out, win = run("survives_and_dies")
    assert win["point_slot"].tolist() == [0, 1]
    # point 0 loses its stereo observation in keyframe 2 (5 - 2 = 3); point 1 its stereo one in keyframe 1 (4 - 2 = 2): SetBadFlag clears
    # keypoint 1 of keyframes 2 and 3 too
    assert rows(m2, "keyframes") == {1: [0, -1], 2: [-1, -1], 3: [0, -1]}
    assert rows(m2, "points") == {0: [(1, 0), (3, 0)], 1: []}
    assert out["pt_n_obs"].tolist() == [3, 2] and out["pt_row_len"].tolist() == [2, 0] and out["pt_ref_kf"].tolist() == [1, -1]
    assert out["pt_flags"].tolist() == [A.REFRESHED, A.WENT_BAD]
    assert (out["n_pt_obs_erased"], out["n_points_bad"], out["n_index_skipped"]) == (2, 1, 0)
    assert (m2["points"][0]["bad"], m2["points"][1]["bad"]) == (0, 1)
    # the bad point keeps normal and distances, and still gets its position
    assert m2["points"][1]["nrm"].tobytes() == m["points"][1]["nrm"].tobytes() and m2["points"][1]["maxd"] == m["points"][1]["maxd"]


def test_a_mono_erasure_counts_one():
    """point 0 of the first scene with its mono observation (keyframe 1, keypoint 0) flagged instead: 5 - 1 = 4"""
    lib = abi.product()
    m, q, _ = AS.NAMED["survives_and_dies"]()
    win = R.ba_window(m, q, S.SIGMA2, lambda T: host.se3_from_tcw_f32(lib, T))
    m2, out = A.apply(m, win, AS.flags_for(win, point_kfs=[(0, 1)]), AS.LEVEL_SCALE, lambda qt: host.se3_to_tcw_f32(lib, qt))
    assert out["pt_n_obs"].tolist() == [4, 4] and m2["keyframes"][1]["points"] == [-1, 1] and m2["points"][0]["obs"] == [(2, 0), (3, 0)]
    assert out["pt_ref_kf"].tolist() == [2, 1]                             # its reference keyframe was keyframe 1: now the first of the row


def test_an_erased_reference_keyframe_and_one_that_is_no_observer():
    m, m2, out, win = run("ref_erased_and_stranger")
    assert win["point_slot"].tolist() == [0, 1]
    assert rows(m2, "keyframes") == {1: [-1, 1], 2: [0, 1], 3: [-1], 4: [5, 0]}
    assert rows(m2, "points") == {0: [(2, 0), (4, 1)], 1: [(1, 1), (2, 1)], 5: [(4, 0)]}
    assert out["pt_n_obs"].tolist() == [4, 4] and out["pt_ref_kf"].tolist() == [2, 4] and out["pt_flags"].tolist() == [A.REFRESHED, A.REFRESHED]
    # keyframe s sits at -(s, 2 s, 3 s).  Point 0 = (0, 0.5, 0.25) against keyframe 2, keypoint 0 (octave 0, scale 1): |(2, 4.5, 6.25)|.
    # Point 1 = (1, 1.5, 1.25) against keyframe 4, which does not observe it: keypoint 0 (octave 0): |(5, 9.5, 13.25)|.
    assert out["ow"].tolist() == [[-1, -2, -3], [-2, -4, -6]]
    assert out["pt_max_distance"].tolist() == [f32(np.sqrt(63.3125)), f32(np.sqrt(290.8125))]
    assert out["pt_min_distance"].tolist() == [f32(f32(np.sqrt(63.3125)) / AS.LEVEL_SCALE[-1]), f32(f32(np.sqrt(290.8125)) / AS.LEVEL_SCALE[-1])]
    # the normal of point 1: the mean of the unit vectors from keyframes 1 and 2
    d1, d2 = np.array([2, 3.5, 4.25]), np.array([3, 5.5, 7.25])
    want = (d1 / np.linalg.norm(d1) + d2 / np.linalg.norm(d2)) / 2
    assert np.allclose(out["pt_normal"][1], want, rtol=0, atol=2e-7)


def test_the_cascade_of_a_bad_point():
    m, m2, out, win = run("cascade")
    assert win["point_slot"].tolist() == [0, 3]
    # keypoint 1 of the bad keyframe 3 held point 7: cleared all the same.  Keyframe 4 was never set: index 3 is outside its (empty) row.
    assert rows(m2, "keyframes") == {1: [-1, 3], 2: [-1, 3], 3: [3, -1]}
    assert rows(m2, "points") == {0: [], 3: [(1, 1), (2, 1), (3, 0)], 7: [(3, 1)]}
    assert out["pt_flags"].tolist() == [A.WENT_BAD | A.INDEX_SKIPPED, A.REFRESHED] and out["pt_n_obs"].tolist() == [2, 6] and out["pt_ref_kf"].tolist() == [-1, 1]
    assert (out["n_pt_obs_erased"], out["n_points_bad"], out["n_index_skipped"]) == (1, 1, 1)


def test_lines():
    m, m2, out, win = run("lines", move_lines=True)
    assert win["line_slot"].tolist() == [0, 1, 2]
    # line 0 went bad through keyframe 2 (both flags: one erasure, 6 - 2 = 4): keyframes 1 and 3 keep their entries.  Line 1 lost keyframe 3,
    # whose keyline has no partner (7 - 1).  Line 2 was removed: flags, row and position stay.
    assert rows(m2, "keyframes", "lines") == {1: [0, 1, 2], 2: [-1, 1, 2], 3: [0, -1]}
    assert rows(m2, "lines") == {0: [], 1: [(1, 1), (2, 1)], 2: [(1, 2), (2, 2)]}
    assert out["ln_bad"].tolist() == [1, 0, 0] and out["ln_n_obs"].tolist() == [4, 6, 4] and out["ln_row_len"].tolist() == [0, 2, 2]
    assert (out["n_ln_obs_erased"], out["n_lines_bad"]) == (2, 1)
    for l, moved in ((0, True), (1, True), (2, False)):
        assert np.array_equal(m2["lines"][l]["x0"], m["lines"][l]["x0"] + 1.0) == moved and np.array_equal(m2["lines"][l]["x0"], m["lines"][l]["x0"]) != moved


def test_the_centre_is_one_rounded_product():
    T = np.eye(4, dtype=f32); T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]; T[:3, 3] = [0.1, 0.2, 0.3]
    assert A.centre(T).tolist() == [-f32(0.2), f32(0.1), -f32(0.3)]


def test_the_random_seeds_show_every_case():
    """what tests/test_gpu_map_ba_apply.py asserts of its seeds, here without a device"""
    lib = abi.product()
    for seed, n_kf in [(0, 12), (1, 12), (4, 12), (5, 8)]:
        m, q = S.random_map(seed, n_kf=n_kf)
        AS.complete(m, seed)
        win = R.ba_window(m, q, S.SIGMA2, lambda T: host.se3_from_tcw_f32(lib, T))
        res = AS.crafted(win, seed, se3_from_tcw=lambda T: host.se3_from_tcw_f32(lib, T))
        m2, out = A.apply(m, win, res, AS.LEVEL_SCALE, lambda qt: host.se3_to_tcw_f32(lib, qt))
        moved = [s for k, s in enumerate(int(v) for v in win["point_slot"]) if not out["pt_flags"][k] & A.WENT_BAD and m2["points"][s]["ref_kf"] != m["points"][s]["ref_kf"]]
        assert out["n_points_bad"] > 0 and moved and out["n_lines_bad"] > 0 and res.line_removed.sum() > 0, seed
        # a bad point's observers lost their entries; a surviving point's row and its observers' rows agree
        for s, p in m2["points"].items():
            for kf, idx in p["obs"]:
                if not p["bad"] and kf in m2["keyframes"] and s in win["point_slot"]:
                    assert m2["keyframes"][kf]["points"][idx] in (s, -1)
