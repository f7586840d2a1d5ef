"""Tracking scenes on the boundaries of TrackWithMotionModel / PoseOptimization's rules, derived from synth.make_tracking_scene by trimming the
last frame's points and lines or taking Observations() from some of its MapPoints.  Each scene is found by a scan and then pinned by the
oracle's own count (oracle/oracle_tracking.py): the rotation histogram of SearchByProjection makes the counts non-monotonic in the trim, so
nothing here assumes a count from a neighbour's.  Shared by tests/test_oracle_track_scenes.py, tests/test_gpu_track_chain_edges.py and
tests/test_cpp_adapter.py."""
import functools

import numpy as np

import oracle_tracking as OT
from lld_slam_amd import synth

BASE = dict(scene_id=30, n_kp=600, n_map=700, n_last=300)

# name: (counter, value, oracle parameters, reference).  The counter is a field of the oracle's stage-1 record.
BOUNDARIES = {
    "wide_19": ("n_search_first", 19, {}, "Tracking.cc:907 (the 2*th search runs)"),
    "wide_20": ("n_search_first", 20, {}, "Tracking.cc:907 (it does not)"),
    "fail_9_wide": ("n_search", 9, {}, "Tracking.cc:913, after the wide retry"),
    "fail_10_wide": ("n_search", 10, {}, "Tracking.cc:913, after the wide retry"),
    "fail_9_narrow": ("n_search", 9, dict(wide_retry=False), "Tracking.cc:913, no wide retry"),
    "fail_10_narrow": ("n_search", 10, dict(wide_retry=False), "Tracking.cc:913, no wide retry"),
    "fail_0": ("n_search", 0, {}, "Tracking.cc:913, nothing matched"),
    "pose_2": ("n_point_edges", 2, {}, "Optimizer.cc:809 (returns before optimising)"),
    "pose_3": ("n_point_edges", 3, {}, "Optimizer.cc:809 (optimises)"),
    "edges_9": ("n_edges", 9, {}, "Optimizer.cc:878 (lines not classified)"),
    "edges_10": ("n_edges", 10, {}, "Optimizer.cc:878 (lines classified)"),
    "map_6": ("n_points_map", 6, {}, "Tracking.cc:992 (false)"),
    "map_7": ("n_points_map", 7, {}, "Tracking.cc:992 (true)"),
    "only_20": ("n_points", 20, {}, "Tracking.cc:990, localisation mode (false)"),
    "only_21": ("n_points", 21, {}, "Tracking.cc:990, localisation mode (true)"),
    "vo_9": ("n_points_map", 9, {}, "Tracking.cc:989, mbVO = true"),
    "vo_10": ("n_points_map", 10, {}, "Tracking.cc:989, mbVO = false"),
}


def _base():
    return synth.make_tracking_scene(BASE["scene_id"], n_kp=BASE["n_kp"], n_map=BASE["n_map"], n_last=BASE["n_last"])


def derive(m, n_lines=None, n_obs=None, base=None):
    """The base scene with the last frame cut to its first `m` points, its MapLines to the first `n_lines` (None: all), and Observations() > 0
    kept for only the first `n_obs` of those points (None: as generated) - in the last frame AND the local map, one MapPoint per id."""
    sc = _base() if base is None else base
    # one MapLine object per id, as in the running system and the adapter's object graph: a line bad in one list is bad in the other
    bad = set()
    for L in (sc["last_lines"], sc["local_lines"]): bad |= set(int(i) for i in np.asarray(L["id"])[np.asarray(L["skip"]) != 0])
    for L in (sc["last_lines"], sc["local_lines"]): L["skip"] = np.isin(L["id"], list(bad)).astype(np.uint8)
    last = {k: np.asarray(v)[:m].copy() for k, v in sc["last"].items()}
    sc["last"] = last; sc["last_ids"] = np.asarray(sc["last_ids"])[:m].copy()
    if n_lines is not None:
        sc["last_lines"] = {k: np.asarray(v)[:n_lines].copy() for k, v in sc["last_lines"].items()}
    if n_obs is not None:
        obs = last["has_obs"].copy(); obs[n_obs:] = 0; last["has_obs"] = obs
        mp = dict(sc["map_points"]); mobs = np.asarray(mp["has_obs"]).copy()
        mobs[sc["last_ids"]] = obs                                           # last_ids index the local map (map_ids = arange)
        mp["has_obs"] = mobs; sc["map_points"] = mp
    return sc


def stage1(sc, **params):
    """The oracle's TrackWithMotionModel record, run on past the failure exit as the device chain does."""
    fr = OT.new_frame(sc)
    p = dict(params)
    searched = OT.motion_model_search(sc, fr, wide_retry=p.pop("wide_retry", True), direction=p.pop("direction", 0))
    return OT.motion_model_rest(sc, fr, searched, **p)


def _search_counts(sc, wide_retry=True):
    n1, n, wide = OT.motion_model_search(sc, OT.new_frame(sc), wide_retry=wide_retry)
    return dict(n_search_first=n1, n_search=n, used_wide=wide, n_point_edges=n)


def _first(values, make, count, want):
    for v in values:
        sc = make(v)
        if count(sc) == want:
            return v
    raise AssertionError(f"no trim hits {want}")


@functools.lru_cache(maxsize=None)
def _knobs(name):
    """(m, n_lines, n_obs) of the scene `name`: the first in scan order whose count is the boundary's."""
    key, want, params, _ = BOUNDARIES[name]
    wide = params.get("wide_retry", True)
    if key in ("n_search_first", "n_search", "n_point_edges"):
        m = _first(range(0, BASE["n_last"] + 1), derive, lambda sc: _search_counts(sc, wide)[key], want)
        return m, None, None
    if key == "n_edges":
        # a few points (at least three: optimised) and a cut of the MapLines that brings the edges to 9 or 10 (a line adds one or two)
        for m in range(4, 10):
            for n_ll in range(0, 141):
                rec = stage1(derive(m, n_lines=n_ll))
                if rec["n_edges"] > want:
                    break
                if rec["n_edges"] == want and rec["n_point_edges"] >= 3 and rec["n_lines_matched"] > 0:
                    return m, n_ll, None
        raise AssertionError(f"no trim hits {want}")
    if key == "n_points":
        m = _first(range(20, BASE["n_last"] + 1), derive, lambda sc: stage1(sc)["n_points"], want)
        return m, None, None
    if key == "n_points_map":
        # enough matches to pass the failure exit (and, for mbVO, the n_points > 20 of localisation mode), fewer of them with observations.
        # (28 for nmatchesMap 6 / 7: from 30 of them the device's stage-2 LM spends 9 trials fewer than the oracle's, over the chain tests' slack)
        m = _knobs("_points_30" if name.startswith("vo_") else "_points_28")[0]
        k = _first(range(0, m + 1), lambda k: derive(m, n_obs=k), lambda sc: stage1(sc)["n_points_map"], want)
        return m, None, k
    raise KeyError(name)


BOUNDARIES["_points_28"] = ("n_search", 28, {}, "")
BOUNDARIES["_points_30"] = ("n_search", 30, {}, "")


def scene(name):
    """(scene, oracle parameters) of the boundary `name`; asserts that the oracle's count is the boundary's."""
    key, want, params, _ = BOUNDARIES[name]
    m, n_ll, n_obs = _knobs(name)
    sc = derive(m, n_lines=n_ll, n_obs=n_obs)
    rec = stage1(sc, **params)
    assert rec[key] == want, (name, key, rec[key], want)
    if key == "n_edges":
        assert rec["n_point_edges"] >= 3 and rec["n_lines_matched"] > 0, (name, rec["n_point_edges"], rec["n_lines_matched"])
    if key in ("n_points_map", "n_points"):
        assert rec["n_search"] >= 10, (name, rec["n_search"])
    if name.startswith("vo_"):
        assert rec["n_points"] > 20, (name, rec["n_points"])
    return sc, dict(params)


NAMES = tuple(n for n in BOUNDARIES if not n.startswith("_"))
