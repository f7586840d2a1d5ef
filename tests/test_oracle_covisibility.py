"""tests/covis_ref.py (the plain-Python restatement of KeyFrame::UpdateConnections and KeyFrameCulling's count) against cases
whose answers are worked out by hand in tests/covis_scenes.py.  CPU only."""
import numpy as np
import pytest

import covis_ref as R
import covis_scenes as S


@pytest.mark.parametrize("name", sorted(S.CONN_CASES))
def test_connections_hand_worked(name):
    sc, exp = S.CONN_CASES[name]()
    got = R.update_connections_ref(sc)
    want = S.expected_conn([exp])
    for k in want:
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


def test_connections_tie_goes_by_descending_slot():
    got = R.update_connections_ref(S.conn_tie()[0])
    assert got["ordered_kf"].tolist() == [3, 2, 1] and got["ordered_weight"].tolist() == [20, 16, 16]


def test_connections_fallback_takes_the_lower_of_two_equal_maxima():
    got = R.update_connections_ref(S.conn_fallback_equal_maxima()[0])
    assert got["ordered_kf"].tolist() == [1] and got["ordered_weight"].tolist() == [5] and got["kf_max"].tolist() == [1]


def test_connections_threshold_is_inclusive_at_15():
    got = R.update_connections_ref(S.conn_14_15()[0])
    assert got["ordered_kf"].tolist() == [2] and got["conn_kf"].tolist() == [1, 2]


def test_connections_empty_counter_returns_early():
    got = R.update_connections_ref(S.conn_empty()[0])
    assert got["updated"].tolist() == [0] and got["conn_start"].tolist() == [0, 0] and got["ordered_start"].tolist() == [0, 0]


def test_connections_minus_one_excludes_nobody_and_duplicates_count_twice():
    b = S.Builder(3)
    p = b.point([0, 1, 2])
    b.query(-1, [p, p]); b.query(0, [p])
    got = R.update_connections_ref(b.scene())
    assert got["conn_kf"].tolist() == [0, 1, 2, 1, 2] and got["conn_weight"].tolist() == [2, 2, 2, 1, 1]
    assert got["ordered_kf"].tolist() == [0, 1] and got["kf_max"].tolist() == [0, 1]


@pytest.mark.parametrize("name", sorted(S.CULL_CASES))
def test_culling_hand_worked(name):
    sc, exp = S.CULL_CASES[name]()
    got = R.keyframe_culling_ref(sc)
    assert (int(got["n_mps"][0]), int(got["n_redundant"][0]), int(got["redundant"][0])) == exp, name


def test_culling_break_does_not_depend_on_the_order():
    sc = S.random_scene(3)
    a = R.keyframe_culling_ref(sc)
    rev = dict(sc)
    rng = np.random.default_rng(0)
    ok, oo = sc["obs_kf"].copy(), sc["obs_octave"].copy()
    for p in range(len(sc["point_bad"])):
        s, e = sc["obs_start"][p], sc["obs_start"][p + 1]
        perm = rng.permutation(e - s)
        ok[s:e] = sc["obs_kf"][s:e][perm]; oo[s:e] = sc["obs_octave"][s:e][perm]
    rev["obs_kf"], rev["obs_octave"] = ok, oo
    b = R.keyframe_culling_ref(rev)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_random_scene_covers_both_sides_of_the_thresholds():
    sc = S.random_scene(1)
    c = R.update_connections_ref(sc)
    assert c["conn_weight"].min() < 15 <= c["conn_weight"].max() and len(c["ordered_kf"]) < len(c["conn_kf"])
    k = R.keyframe_culling_ref(sc)
    assert 0 < k["n_redundant"].sum() < k["n_mps"].sum()
    nent = np.diff(sc["q_start"])
    assert np.all(k["n_mps"] < nent)                 # depth and bad points drop some entries


def test_object_model_requery_changes_a_later_verdict():
    w, current, expect = S.requery_world()
    w.update_connections(list(range(len(w.kfs))))
    once = R.keyframe_culling_ref(w.flat(w.kfs[current].ordered))
    assert [k for q, k in enumerate(w.kfs[current].ordered) if once["redundant"][q]] == expect["single_call"]
    flagged, calls = w.keyframe_culling(current)
    assert flagged == expect["flagged"] and calls == expect["calls"]
