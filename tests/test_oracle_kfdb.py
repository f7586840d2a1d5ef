"""The KeyFrameDatabase restatement (tests/kfdb_ref.py) on hand-built known answers: the rules of include/lld_amd.h that decide
ids, order and counters.  CPU only."""
import numpy as np
import pytest

import kfdb_ref as K

F32 = np.float32


def run(name):
    ops, exp = K.SCENARIOS[name]
    return K.run_ops(K.KeyFrameDatabase(64), ops), exp


@pytest.mark.parametrize("name", [n for n, (_, e) in K.SCENARIOS.items() if isinstance(e[0], tuple)])
def test_known_answers(name):
    got, exp = run(name)
    assert len(got) == len(exp)
    for (ids, acc, _), (eids, eacc) in zip(got, exp):
        assert ids == eids and [float(a) for a in acc] == eacc


def test_truncation_at_the_strict_boundary():
    (r,), (stats,) = run("truncation_boundary")
    assert r[2] == stats and r[0] == [1, 3]            # 8 common words are not > (int)(10*0.8f)
    for m in range(1, 3000):
        assert int(F32(m) * F32(0.8)) == (4 * m) // 5   # the float product never rounds up across an integer here


def test_stale_reloc_score_changes_the_second_query():
    got, _ = run("stale_reloc_score")
    fresh, _ = run("stale_reloc_score_fresh")
    assert got[1][0] == [2] and fresh[0][0] == [1]
    assert got[1][2]["n_scored"] == 1 and got[1][2]["n_sharing"] == 2


def test_query_id_zero_and_a_repeated_id_return_nothing():
    got, _ = run("query_id_zero_and_repeated")
    assert [g[2]["n_sharing"] for g in got] == [0, 0, 2, 0, 2, 0]


def test_connected_keyframes_are_not_listed():
    db = K.KeyFrameDatabase(64)
    got = K.run_ops(db, K.SCENARIOS["connected_left_out"][0])
    assert got[0][2]["n_sharing"] == 1 and db.kfs[1].mnLoopWords == 1 and db.kfs[1].mnLoopQuery == 0


def test_two_entries_with_one_best_give_one_output():
    db = K.KeyFrameDatabase(64)
    ops = [o for o in K.SCENARIOS["same_best_once"][0] if o[0] != "reloc"]
    K.run_ops(db, ops)
    ids, acc, stats = db.detect_relocalization_candidates(1, K._v({0: 1.0}))
    assert ids == [3] and stats["n_scored"] == 3


def test_bestscore_tie_keeps_the_first():
    got, _ = run("best_score_tie")
    assert got[0][0] == [3]


def test_min_score_is_inclusive_and_retention_strict():
    got, _ = run("min_score_vs_retain")
    assert got[0][0] == [1] and got[2][0] == []
    assert F32(0.75) * F32(0.5) == F32(0.375)


def test_summation_order_of_accscore():
    got, _ = run("summation_order")
    assert got[0][0] == [4]
    seq = F32(F32(F32(0.75) + F32(K.E25)) + F32(K.E25))
    other = F32(F32(0.75) + F32(F32(K.E25) + F32(K.E25)))
    assert seq == F32(0.75) and other > F32(0.75) * F32(1.0)


def test_erase_then_readd_goes_to_the_end():
    got, _ = run("erase_then_readd")
    assert got[0][0] == [1, 2] and got[1][0] == [2, 1]


def test_clear_keeps_the_registers():
    db = K.KeyFrameDatabase(64)
    got = K.run_ops(db, K.SCENARIOS["clear_keeps_registers"][0])
    assert got[2][0] == [2] and db.kfs[1].mnRelocQuery == 7


def test_refusals_leave_the_restatement_unchanged():
    db = K.KeyFrameDatabase(16, max_keyframes=3, max_words=6)
    db.add(1, K._v({0: 0.5, 1: 0.5}))
    for bad in (lambda: db.add(1, K._v({2: 1.0})), lambda: db.add(2, (np.array([3, 2]), np.array([0.5, 0.5]))),
                lambda: db.add(2, K._v({16: 1.0})), lambda: db.add_many([2, 2], [K._v({2: 1.0})] * 2),
                lambda: db.add(2, K._v({i: 0.2 for i in range(2, 7)})), lambda: db.set_covisibles(1, [5, 6, 7])):
        with pytest.raises(K.Refused):
            bad()
    assert db.in_db == {1} and len(db.kfs) == 1 and db.live_words == 2


def test_trajectory_generator_is_seeded_and_revisits():
    a = K.trajectory(3, 60, 5000, words_per_kf=50)
    b = K.trajectory(3, 60, 5000, words_per_kf=50)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a[2], b[2]))
    place = a[1]
    assert any(place[i] < max(place[:i]) - 1 for i in range(1, 60))
    cov = K.covisibility(a[0], a[2])
    assert sum(len(v) for v in cov.values()) > 60
