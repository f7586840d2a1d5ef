"""tests/map_covis_ref.py (the restatement of lld_map_covisibility on map tables) held to tests/covis_ref.py (the restatement on flat arrays,
itself held to the hand-worked scenes and the oracle): every scene is loaded into tables under a random slot permutation and an independent
random order_key assignment; with the slots renamed by key rank the answers must be identical.  CPU only."""
import numpy as np
import pytest

import covis_ref as R
import covis_scenes as S
import map_covis_ref as M


def load(sc, seed):
    """The scene's keyframe k is the k-th in map order: it gets a random slot and the k-th smallest of random 64-bit keys."""
    rng = np.random.default_rng(seed)
    nk, npt = int(sc["n_kf"]), len(sc["point_bad"])
    kf_slot = rng.permutation(nk + 5)[:nk]
    kf_key = np.sort(rng.choice(1 << 40, size=nk, replace=False)) + 1
    pt_slot = rng.permutation(npt + 7)[:npt]
    T = M.tables_from_scene(sc, kf_slot, kf_key, pt_slot)
    return T, [int(kf_slot[k]) for k in sc["query_kf"]], {int(s): k for k, s in enumerate(kf_slot)}


def same(a, b, names):
    for k in names:
        assert np.array_equal(a[k], b[k]), k


CONN = ("conn_start", "conn_kf", "conn_weight", "ordered_start", "ordered_kf", "ordered_weight", "n_max", "kf_max", "updated")
CULL = ("n_mps", "n_redundant", "redundant")


@pytest.mark.parametrize("name", sorted(S.CONN_CASES))
def test_hand_worked_connections(name):
    sc, exp = S.CONN_CASES[name]()
    for seed in range(3):
        T, queries, back = load(sc, seed)
        r = M.renumber(M.covisibility(T, queries), back)
        same(r, S.expected_conn([exp]), CONN)
        same(r, R.update_connections_ref(sc), CONN)
        assert not r["status"].any()


@pytest.mark.parametrize("name", sorted(S.CULL_CASES))
def test_hand_worked_culling(name):
    sc, exp = S.CULL_CASES[name]()
    for seed in range(3):
        T, queries, _ = load(sc, seed)
        r = M.covisibility(T, queries, connections=False, culling=True, monocular=sc["monocular"])
        assert (int(r["n_mps"][0]), int(r["n_redundant"][0]), int(r["redundant"][0])) == exp and not r["status"].any()
        same(r, R.keyframe_culling_ref(sc), CULL)


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_scenes(seed, mono):
    sc = S.random_scene(seed, monocular=mono)
    T, queries, back = load(sc, 100 + seed)
    r = M.renumber(M.covisibility(T, queries, culling=True, monocular=mono), back)
    same(r, R.update_connections_ref(sc), CONN)
    same(r, R.keyframe_culling_ref(sc), CULL)
    assert not r["status"].any()


def test_slot_order_does_not_decide_ties():
    """tie: 16, 16, 20 - with the slots in reverse key order the equal weights still go by descending order_key."""
    sc, exp = S.conn_tie()
    T = M.tables_from_scene(sc, [3, 2, 1, 0], [10, 20, 30, 40], np.arange(len(sc["point_bad"])))
    r = M.renumber(M.covisibility(T, [3]), {3: 0, 2: 1, 1: 2, 0: 3})
    same(r, S.expected_conn([exp]), CONN)


def test_never_set_point_and_doubled_entry():
    sc, _ = S.cull_nobs_3_4()                                   # two points seen by 1, 2, 3; keyframe 0 holds both
    T = M.tables_from_scene(sc, [0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [0, 1])
    row = T["kf"][0]
    # a third entry names a point the map does not hold, a fourth repeats point 1
    for p in (9, 1):
        row["points"].append(p); row["octave"].append(0); row["depth"].append(1.0)
    r = M.covisibility(T, [0], culling=True)
    assert r["conn_kf"].tolist() == [1, 2, 3] and r["conn_weight"].tolist() == [3, 3, 3]          # point 1 counts twice, point 9 not at all
    assert (int(r["n_mps"][0]), int(r["n_redundant"][0])) == (4, 2)                                # point 9 is counted in n_mps, never redundant
    row["depth"][2] = -1.0                                                                         # ... and takes the depth test
    assert int(M.covisibility(T, [0], connections=False, culling=True)["n_mps"][0]) == 3
    assert int(M.covisibility(T, [0], connections=False, culling=True, monocular=True)["n_mps"][0]) == 4


def test_status_bits():
    sc, _ = S.cull_nobs_3_4()
    T = M.tables_from_scene(sc, [0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [0, 1])
    T["pt"][1]["idx"] = None                                    # a row set without indices
    r = M.covisibility(T, [0], culling=True)
    assert r["status"].tolist() == [M.NO_KEYPOINT_DATA] and (int(r["n_mps"][0]), int(r["n_redundant"][0]), int(r["redundant"][0])) == (0, 0, 0)
    assert r["conn_kf"].tolist() == [1, 2, 3]                   # the connections do not need them
    T["pt"][1]["idx"] = [0, 0, 99]                              # an index beyond the observer's keypoint row
    assert M.covisibility(T, [0], connections=False, culling=True)["status"].tolist() == [M.NO_KEYPOINT_DATA]
    T["pt"][1]["idx"] = [0, 0, 0]
    T["kf"][0]["octave"] = T["kf"][0]["octave"][:-1]            # the keyframe's keypoint row is stale
    assert M.covisibility(T, [0], connections=False, culling=True)["status"].tolist() == [M.NO_KEYPOINT_DATA]
    # more distinct observers than MAX_CONNECTED
    kf = {0: dict(key=1, points=list(range(M.MAX_CONNECTED + 1)), octave=None, depth=None, th_depth=0.0)}
    pt = {}
    for i in range(M.MAX_CONNECTED + 1):
        kf[i + 1] = dict(key=i + 2, points=[], octave=None, depth=None, th_depth=0.0)
        pt[i] = dict(bad=False, nobs=1, obs=[i + 1], idx=None)
    r = M.covisibility(dict(kf=kf, pt=pt), [0])
    assert r["status"].tolist() == [M.CONN_OVERFLOW] and r["updated"].tolist() == [0] and r["conn_start"].tolist() == [0, 0] and r["kf_max"].tolist() == [-1]
    kf[0]["points"].pop()
    r = M.covisibility(dict(kf=kf, pt=pt), [0], th=1)
    assert r["status"].tolist() == [0] and len(r["conn_kf"]) == M.MAX_CONNECTED and r["ordered_kf"][0] == M.MAX_CONNECTED
