"""The scenes of tests/reloc_scenes.py take the exit they are named after when the CPU reference (tests/reloc_ref.py) runs them, and every
threshold decision of the run is taken with room to spare.  That is what lets tests/test_gpu_reloc.py demand exact integers: a device
PoseOptimization that classifies one edge differently still takes the same rungs.

Margins (observed on these scenes, stated here): SearchByBoW's count stays MARGIN_BOW away from 15; every nGood / nadditional + nGood
comparison stays MARGIN_GOOD away from its threshold (10, 30, 50); no correspondence of any hypothesis or refined pose of any PnP call
lies within one float spacing of its mvMaxError (test_gpu_pnp.near_threshold's notion).  A scene that does not clear them gets another
seed or other group sizes, not a looser test."""
import numpy as np
import pytest

import reloc_ref as RF
import reloc_scenes as RS2
from test_gpu_pnp import near_threshold

MARGIN_BOW = 3
MARGIN_GOOD = 3

R = RF


@pytest.fixture(scope="module")
def runs(oracle):
    return {name: RF.relocalize(RS2.make_scene(name)) for name in RS2.NAMES}


@pytest.mark.parametrize("name", RS2.NAMES)
def test_scene_shapes(name):
    S = RS2.make_scene(name)
    assert S["sc"]["frame"].n == RS2.N_KP and 3 <= len(S["candidates"]) <= 5
    for kf in S["candidates"]:
        assert len(kf["angle"]) == RS2.N_KF
        ids = np.asarray(kf["point_id"]); ids = ids[ids >= 0]
        assert len(np.unique(ids)) == len(ids)                               # one observation per MapPoint inside a keyframe


@pytest.mark.parametrize("name", RS2.NAMES)
def test_every_decision_clears_its_threshold(runs, name):
    r = runs[name]
    for what, value, thr in r["decisions"]:
        margin = MARGIN_BOW if what == "nmatches" else MARGIN_GOOD
        # `value < thr` false means value >= thr: a distance of `margin` on either side, counted from the first integer of that side
        assert value <= thr - 1 - margin or value >= thr + margin, (name, what, value, thr)
    for i, o, hyps in r["pnp_calls"]:
        ref = r["solvers"][i]
        for cnt, Rm, t in hyps:
            assert len(near_threshold(ref, Rm, t)) == 0, (name, i)


def test_first_wins(runs):
    r = runs["first_wins"]
    assert (r["matched"], r["winner"], r["round"]) == (1, 0, 1) and r["rungs"][0] == R.POSE1 and r["n_good"] >= 50
    assert r["rounds"].tolist() == [1, 0, 0]                                 # the candidates behind the winner are never reached


def test_second_wins_same_round(runs):
    r = runs["second_wins_same_round"]
    assert (r["matched"], r["winner"], r["round"]) == (1, 1, 1)
    assert r["rungs"][0] == R.POSE1 and 0 <= r["n_good_last"][0] < 10 and r["rungs"][1] == R.POSE1 and r["rounds"].tolist() == [1, 1, 0]


def test_coarse_search(runs):
    r = runs["coarse_search"]; w = r["winner"]
    assert r["matched"] == 1 and r["rungs"][w] == R.POSE1 | R.SEARCH1 | R.POSE2 and r["n_additional1"][w] > 0 and r["n_good"] >= 50


def test_narrow_search(runs):
    r = runs["narrow_search"]
    full = R.POSE1 | R.SEARCH1 | R.POSE2 | R.SEARCH2 | R.POSE3
    assert r["rungs"][0] == full and r["n_additional2"][0] > 0 and r["n_good_last"][0] < 50      # the whole ladder and its final discard, and still no match
    assert (r["matched"], r["winner"]) == (1, 1)


def test_keeps_outliers(runs):
    r = runs["keeps_outliers"]; w = r["winner"]
    assert r["matched"] == 1 and r["rungs"][w] == R.POSE1 | R.SEARCH1 | R.POSE2
    held = r["kp_point_id"] >= 0
    assert r["kp_outlier"][held].sum() >= 3 and held.sum() - r["kp_outlier"][held].sum() == r["n_good"]   # flagged points stay in mvpMapPoints (:1952-1956)


def test_late_round(runs):
    r = runs["late_round"]; w = r["winner"]
    assert r["matched"] == 1 and r["round"] >= 3 and r["rounds"][w] == r["round"]
    early = [i for i in range(len(r["rounds"])) if i != w and r["discarded"][i] and 1 <= r["rounds"][i] < r["round"]]
    assert early, "another candidate hits bNoMore before the winner's round"


def test_all_discarded_bow(runs):
    r = runs["all_discarded_bow"]
    assert r["matched"] == 0 and r["n_kept"] == 0 and r["n_rounds"] == 0 and (r["n_bow"] < 15).all() and r["discarded"].all()


def test_bad_keyframe(runs):
    r = runs["bad_keyframe"]
    assert r["discarded"][0] == 1 and r["n_bow"][0] == 0 and r["rounds"][0] == 0 and (r["matched"], r["winner"]) == (1, 1)


def test_no_match(runs):
    r = runs["no_match"]
    assert r["matched"] == 0 and r["n_kept"] == 3 and r["discarded"].all() and r["n_rounds"] >= 2 and (r["rounds"] >= 1).all()
    assert (r["kp_point_id"] == -1).all()
