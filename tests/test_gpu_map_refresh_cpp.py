"""The C++ layer of the landmark refresh on the resident map (include/lld_amd.hpp: lld_amd::DeviceMap::SetKeyFrameDescriptors,
SetKeyFrameLineDescriptors, RefreshPoints, RefreshLines, DownloadPoints, DownloadLines) against the Python wrapper and the restatement:
examples/map_refresh_harness builds a map by formula and prints every output; the same map is built here through DeviceMap and as a model
of tests/map_refresh_ref.py.  And the route on objects: adapters/lld_map_adapter.cc's MapOnDevice::RefreshMapPoints /
ComputeDistinctiveDescriptors on one object graph against adapters/lld_landmark_adapter.cc on an identical one (the harness's `objects`
mode).  Bit for bit, member by member."""
import os
import subprocess

import numpy as np
import pytest

import map_refresh_ref as R
from lld_slam_amd.device_map import DeviceMap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "map_refresh_harness")
N_KF, N_PTS, N_LNS, DIM = 5, 6, 2, 8
SCALE = np.array([1.0, 1.2, 1.44, 1.728], np.float32)
QUERY, LQUERY = [4, 1, 5, 0, 3, 2], [1, 0]


def word(s, i, w):
    M = 0xffffffff
    h = (s * 2654435761 + i * 40503 + w * 97 + 1) & M
    h = (h * 2246822519) & M; h ^= h >> 15; h = (h * 3266489917) & M; h ^= h >> 13
    return h


def formula_map():
    """the map of examples/map_refresh_harness.cpp as a model of tests/map_refresh_ref.py"""
    m = dict(keyframes={}, points={}, lines={})
    for s in range(N_KF):
        T = np.eye(4, dtype=np.float32); T[:3, 3] = [-(s + 1), -0.5 * s, -0.25 * s]
        m["keyframes"][s] = dict(key=100 - 7 * s, bad=int(s == 3), points=[(i + s) % N_PTS for i in range(N_PTS)], lines=[1 - j if s % 2 else j for j in range(N_LNS)],
                                 octave=[(i + s) % 4 for i in range(N_PTS)], mn_id=s + 1, Tcw=T, uvr=np.zeros((N_PTS, 3), np.float32), kl_left=np.zeros((N_LNS, 4), np.float32),
                                 kl_right=np.zeros((N_LNS, 4), np.float32), kl_octave=np.zeros((N_LNS, 2), np.int32),
                                 desc=np.array([[word(s, i, w) for w in range(8)] for i in range(N_PTS)], np.uint32),
                                 ldesc=np.array([[((31 * s + 17 * j + 7 * c) % 23) * 1.5 for c in range(DIM)] for j in range(N_LNS)], np.float32))
    for p in range(N_PTS):
        m["points"][p] = dict(bad=0, pos=np.array([0.5 * p, 1.0 + p, 5.0 + 0.25 * p], np.float32), obs=[(s, (p - s) % N_PTS) for s in range(N_KF - 1, -1, -1) if (s + p) % 3 != 0],
                              ref_kf=p % N_KF, indexed=True)
    for l in range(N_LNS):
        m["lines"][l] = dict(bad=0, x0=np.zeros(3), dir=np.zeros(3), obs=[(s, 1 - l if s % 2 else l) for s in range(N_KF - 1, -1, -1)], n_obs=2 * N_KF)
    return m


def through_python(gpu_ctx, m):
    K = m["keyframes"]; ks = sorted(K); none = [[] for _ in ks]
    with DeviceMap(gpu_ctx, max_keyframes=N_KF, max_points=N_PTS, max_lines=N_LNS, line_dim=DIM, max_observations=64, max_kf_points=64, max_kf_lines=32, max_children=4,
                   max_local_points=8, max_local_lines=2) as dm:
        dm.set_keyframes(ks, [K[s]["key"] for s in ks], [K[s]["bad"] for s in ks], [-1] * N_KF, none, none, [K[s]["points"] for s in ks], [K[s]["lines"] for s in ks])
        dm.set_keyframe_keypoints(ks, [K[s]["octave"] for s in ks], [[0.0] * N_PTS for _ in ks], [0.0] * N_KF)
        dm.set_keyframe_features(ks, [K[s]["mn_id"] for s in ks], [K[s]["Tcw"] for s in ks], [K[s]["uvr"] for s in ks], [K[s]["kl_left"] for s in ks],
                                 [K[s]["kl_right"] for s in ks], [K[s]["kl_octave"] for s in ks])
        ps = sorted(m["points"]); P = m["points"]
        dm.set_points(ps, np.array([P[p]["pos"] for p in ps]), np.zeros((N_PTS, 3)), np.zeros(N_PTS), np.zeros(N_PTS), np.zeros((N_PTS, 8), np.uint32), [0] * N_PTS)
        dm.set_observations_indexed(ps, rows=[P[p]["obs"] for p in ps], n_obs=[len(P[p]["obs"]) for p in ps])
        dm.set_point_refs(ps, [P[p]["ref_kf"] for p in ps])
        ls = sorted(m["lines"]); z = np.zeros((N_LNS, 3))
        dm.set_lines(ls, z, z, z, z, np.zeros((N_LNS, DIM), np.float32), [0] * N_LNS)
        dm.set_line_observations(ls, [m["lines"][l]["obs"] for l in ls], [m["lines"][l]["n_obs"] for l in ls])
        dm.set_keyframe_descriptors(ks, [K[s]["desc"] for s in ks]); dm.set_keyframe_line_descriptors(ks, [K[s]["ldesc"] for s in ks])
        rp = dm.refresh_points(QUERY, level_scale=SCALE); rl = dm.refresh_lines(LQUERY)
        return rp, rl, dm.download_points(ps), dm.download_lines(ls)


def flat(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.uint32) if a.dtype == np.float32 else a).reshape(-1).astype(np.int64).tolist()


def test_the_cpp_layer_equals_the_python_wrapper_and_the_restatement(gpu_ctx):
    assert os.path.exists(HARNESS), "examples/map_refresh_harness is built by build()"
    r = subprocess.run([HARNESS, "formula"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-400:]
    cpp = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.strip()}
    m = formula_map()
    rp, rl, held, lheld = through_python(gpu_ctx, m)
    names = dict(p_updated=rp["updated"], p_best_obs=rp["best_obs"], p_best_median=rp["best_median"], p_desc=rp["desc"], p_normal=rp["normal"], p_min=rp["min_distance"],
                 p_max=rp["max_distance"], l_updated=rl["updated"], l_best_obs=rl["best_obs"], l_best_median=rl["best_median"], l_desc=rl["desc"], t_pos=held["pos"],
                 t_normal=held["normal"], t_min=held["min_distance"], t_max=held["max_distance"], t_desc=held["desc"], t_state=held["state"], t_ldesc=lheld["desc"],
                 t_lbad=lheld["bad"])
    assert set(cpp) == set(names)
    for k, v in names.items():
        assert cpp[k] == flat(v), k
    ep = R.refresh_points(m, QUERY, R.DESCRIPTOR | R.NORMAL_DEPTH, SCALE); el = R.refresh_lines(m, LQUERY, DIM)
    for k in ("updated", "best_obs", "best_median", "desc", "normal", "min_distance", "max_distance"):
        assert np.asarray(rp[k]).tobytes() == np.asarray(ep[k]).tobytes(), k
    for k in ("updated", "best_obs", "best_median", "desc"):
        assert np.asarray(rl[k]).tobytes() == np.asarray(el[k]).tobytes(), k
    assert rp["updated"].tolist() == [3] * N_PTS and rl["updated"].tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------------------------- the object graphs
def object_scene(flags):
    """the scene of tests/test_gpu_landmark_cpp.py: ragged rows (empty ones too), bad keyframes and points, one mpRefKF that is no observer"""
    import landmark_ref as L
    n_kf, dim = 40, 72
    pts = L.make_point_scene(51, 150, n_kf=n_kf, counts=list(np.random.default_rng(5).integers(0, 41, 148)) + [40, 40])
    lns = L.make_line_scene(52, n_kf=n_kf, dim=dim, scaled=True, counts=np.random.default_rng(6).integers(0, 25, 60))
    lns["kf_bad"] = pts["kf_bad"].copy()
    n, nl = len(pts["bad"]), len(lns["bad"])
    absent = None
    for i in range(n):
        s, e = pts["obs_start"][i], pts["obs_start"][i + 1]
        if absent is None and not pts["bad"][i] and 2 <= e - s < n_kf:
            pts["ref_kf"][i] = next(k for k in range(n_kf) if k not in set(pts["obs_kf"][s:e].tolist()))
            absent = i
        elif e > s:
            pts["ref_kf"][i] = pts["obs_kf"][s + (i % (e - s))]
    rng = np.random.default_rng(3)
    prior = dict(desc=rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32), normal=rng.normal(size=(n, 3)).astype(np.float32),
                 min_distance=rng.random(n).astype(np.float32), max_distance=rng.random(n).astype(np.float32))
    prior_lines = rng.normal(size=(nl, dim)).astype(np.float32)
    blob, ref_level = L.object_scene_blob(pts, lns, flags, prior, prior_lines)
    exp = L.refresh_map_points_ref(dict(pts, ref_level=ref_level), flags, prior)
    expl = L.distinctive_lines_ref(lns, prior_lines)
    return blob, exp, expl, absent


@pytest.mark.parametrize("flags", [R.DESCRIPTOR | R.NORMAL_DEPTH, R.DESCRIPTOR, R.NORMAL_DEPTH])
def test_the_two_object_graphs_agree_member_by_member(gpu_ctx, tmp_path, flags):
    """MapOnDevice::RefreshMapPoints / ComputeDistinctiveDescriptors on one graph, adapters/lld_landmark_adapter.cc on an identical one: every
    member of every MapPoint and MapLine, the return values, the restatement, and the map's own rows"""
    assert os.path.exists(HARNESS), "examples/map_refresh_harness is built by build()"
    blob, exp, expl, absent = object_scene(flags)
    path = tmp_path / "scene.bin"
    path.write_bytes(blob)
    r = subprocess.run([HARNESS, "objects", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-400:]
    rows = {"A": [], "B": [], "T": []}
    for ln in r.stdout.splitlines():
        w = ln.split()
        rows[w[0]].append(w[1:])
    n, nl = len(exp["updated"]), len(expl["updated"])
    assert len(rows["A"]) == len(rows["B"]) == 1 + n + nl and len(rows["T"]) == n + nl
    for a, b in zip(rows["A"], rows["B"]):
        assert a == b, (a[:2], "the map route and the gathering adapter differ")
    assert rows["T"] == rows["A"][1:], "the map holds what the objects hold"
    assert [int(x) for x in rows["A"][0][1:]] == [int(np.sum(exp["updated"] != 0)), int(np.sum(expl["updated"] != 0))]
    if flags & R.NORMAL_DEPTH:
        assert exp["updated"][absent] & R.NORMAL_DEPTH
    assert np.any(exp["updated"] == 0) and np.any(exp["updated"] == flags)
    hexw = lambda ws: np.array([int(x, 16) for x in ws], np.uint32)
    for i in range(n):
        a = rows["A"][1 + i]
        assert a[0] == "P" and int(a[1]) == i
        w = hexw(a[2:])
        assert np.array_equal(w[:8], exp["desc"][i]) and np.array_equal(w[8:11], exp["normal"][i].view(np.uint32)), i
        assert w[11] == exp["min_distance"][i:i + 1].view(np.uint32)[0] and w[12] == exp["max_distance"][i:i + 1].view(np.uint32)[0], i
    for i in range(nl):
        a = rows["A"][1 + n + i]
        assert a[0] == "L" and int(a[1]) == i and np.array_equal(hexw(a[2:]), expl["desc"][i].view(np.uint32)), i
