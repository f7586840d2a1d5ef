"""The C++ layer of lld_map_fuse on objects (examples/map_fuse_harness.cpp): MapOnDevice::Fuse and MapOnDevice::SearchInNeighbors
(adapters/lld_map_adapter.cc) on one object graph against ORBmatcher::Fuse of adapters/lld_matcher_adapter.cc and the reference's
SearchInNeighbors loop over the gathering adapters on an identical graph - every member the routines write of every MapPoint and KeyFrame and
the return values - then the map's own rows against the objects, and, for one Fuse, everything against the plain-Python restatement
(tests/map_fuse_ref.py), which tests/test_gpu_map_fuse.py holds the Python wrapper to."""
import os
import subprocess

import numpy as np
import pytest

import map_fuse_ref as F
import map_fuse_scenes as FS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "map_fuse_harness")


def object_scene(m, c, slots, th=3.0):
    """the file examples/map_fuse_harness.cpp reads: keyframe s is slot s, point slot s is mnId s; every keyframe's covisibility list is the
    target first (for the target: every other keyframe), then the next four slots"""
    K, P = m["keyframes"], m["points"]
    n_kf = max(K) + 1
    assert sorted(K) == list(range(n_kf)) and [K[s]["key"] for s in range(n_kf)] == sorted(K[s]["key"] for s in K)
    n_pts = max(list(P) + [0]) + 1
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    f4 = lambda v: np.asarray(v, np.float32).tobytes()
    t = c["target"]
    v = c["view"]
    out = [i32(n_kf, n_pts, len(c["level_scale"]), t, len(slots)), f4([th]), f4([v["fx"], v["fy"], v["cx"], v["cy"], v["bf"]]), f4([v["min_x"], v["max_x"], v["min_y"], v["max_y"]]),
           f4(c["grid"][2:4]), f4([v["log_scale_factor"]]), f4(c["level_scale"]), f4(c["inv_sigma2"])]
    for s in range(n_kf):
        k = K[s]
        out += [i32(k["bad"]), f4(k["Tcw"]), f4(FS.view_of(k["Tcw"])["Ow"]), i32(len(k["points"]))]
        for i in range(len(k["points"])):
            out += [f4(k["uvr"][i]), i32(k["octave"][i]), np.asarray(k["desc"][i], np.uint32).tobytes(), i32(k["points"][i])]
        cov = [o for o in range(n_kf) if o != t][:10] if s == t else [t] + [(s + d) % n_kf for d in range(1, 6) if (s + d) % n_kf not in (s, t)][:4]
        out += [i32(len(cov)), i32(*cov)]
    z3 = np.zeros(3, np.float32)
    for s in range(n_pts):
        p = P.get(s)
        if p is None:
            out += [i32(0, 1), f4(z3), f4(z3), f4([0, 0]), np.zeros(8, np.uint32).tobytes(), i32(0, -1, 0)]
            continue
        out += [i32(1, p["bad"]), f4(p["pos"]), f4(p["nrm"]), f4([p["mind"], p["maxd"]]), np.asarray(p["desc"], np.uint32).tobytes(), i32(F.n_obs_of(p), p.get("ref_kf", -1), len(p["obs"]))]
        out += [i32(kf, idx) for kf, idx in p["obs"]]
    out.append(i32(*slots) if len(slots) else b"")
    return b"".join(out)


def run(tmp_path, mode, blob):
    path = tmp_path / "scene.bin"
    path.write_bytes(blob)
    r = subprocess.run([HARNESS, mode, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr
    rec = {"A": {}, "B": {}, "T": {}}
    for line in r.stdout.splitlines():
        w = line.split()
        rec[w[0]][(w[1],) if w[1] == "R" else (w[1], int(w[2]))] = w[2:] if w[1] == "R" else w[3:]
    return rec


def objects_of(rec):
    """per point: bad, nObs, mnFound, mnVisible, mpReplaced, mark, observations; per keyframe its matches"""
    pts, kfs = {}, {}
    for (kind, *i), w in rec.items():
        if kind == "P":
            v = [int(x) for x in w]
            pts[i[0]] = dict(bad=v[0], n_obs=v[1], found=v[2], visible=v[3], replaced=v[4], mark=v[5], obs=list(zip(v[7::2], v[8::2])))
            assert len(pts[i[0]]["obs"]) == v[6]
        elif kind == "K":
            v = [int(x) for x in w]
            kfs[i[0]] = dict(mark=v[0], parent=v[1], points=v[3:])
            assert len(kfs[i[0]]["points"]) == v[2]
    return pts, kfs


def map_rows_match_the_objects(rec, pts, kfs):
    T = rec["T"]
    for s, p in pts.items():
        assert [int(x) for x in T[("0", s)][1:]] == [kf for kf, _ in p["obs"]], ("point_obs", s)
        assert [int(x) for x in T[("1", s)][1:]] == [i for _, i in p["obs"]], ("point_idx", s)
        assert int(T[("3", s)][0]) == p["n_obs"] and int(T[("3", s)][1]) == (2 if p["bad"] else 1), ("n_obs / state", s)
    for s, k in kfs.items():
        assert [int(x) for x in T[("2", s)][1:]] == k["points"], ("kf_points", s)


def test_one_fuse_on_objects(tmp_path):
    m, c, slots = FS.random_scene(3, 65, 65, objects=True, check=False)
    m2, exp = FS.run_ref(m, c, slots)
    assert exp["n_fused"] > 16 and set(exp["action"].tolist()) >= {1, 2, 3, 4, 5}
    rec = run(tmp_path, "fuse", object_scene(m, c, slots))
    A, B = rec["A"], rec["B"]
    assert int(A[("R",)][0]) == int(B[("R",)][0]) == exp["n_fused"]
    pa, ka = objects_of(A); pb, kb = objects_of(B)
    assert pa == pb and ka == kb                                            # every member but the descriptors, which ORBmatcher::Fuse of the adapter leaves alone
    surv = set(int(s) for s in exp["survivor"])
    assert all(A[k] == B[k] for k in A if k[0] == "C" or (k[0] == "D" and k[1] not in surv))
    # ... against the restatement: rows, counts, flags, the survivors' descriptors
    for s, p in m2["points"].items():
        assert pa[s]["obs"] == p["obs"] and pa[s]["bad"] == p["bad"] and pa[s]["n_obs"] == F.n_obs_of(p), s
        assert [int(x, 16) for x in A[("D", s)][:8]] == np.asarray(p["desc"], np.uint32).tolist(), ("descriptor", s)
    for s, k in m2["keyframes"].items():
        assert ka[s]["points"] == list(k["points"]), s
    # mnFound / mnVisible: the survivor gained the loser's (MapPoint.cc:210-211); the harness starts them at 1 + i % 5 and 2 + i % 7
    found = {s: 1 + s % 5 for s in pa}; vis = {s: 2 + s % 7 for s in pa}
    for i, a in enumerate(exp["action"]):
        loser, sv = (slots[i], int(exp["other"][i])) if a == F.CANDIDATE_REPLACED else (int(exp["other"][i]), slots[i]) if a == F.HOLDER_REPLACED else (None, None)
        if loser is not None and loser != sv:
            found[sv] += found[loser]; vis[sv] += vis[loser]
            assert pa[loser]["replaced"] == sv
    assert all(pa[s]["found"] == found[s] and pa[s]["visible"] == vis[s] for s in pa)
    map_rows_match_the_objects(rec, pa, ka)


def test_search_in_neighbors_on_objects(tmp_path):
    m, c, slots = FS.random_scene(3, 65, 65, objects=True, check=False)
    t = c["target"]
    assert t != 0                                                           # (the marks start at 0: pKF's mnId must not be)
    before = {s: list(k["points"]) for s, k in m["keyframes"].items()}
    rec = run(tmp_path, "neighbors", object_scene(m, c, []))
    A, B = rec["A"], rec["B"]
    assert int(A[("R",)][0]) == int(B[("R",)][0]) > 8
    pa, ka = objects_of(A); pb, kb = objects_of(B)
    assert pa == pb and ka == kb
    # descriptors, normals and distances of every point that is not bad; covisibility lists and weights of every keyframe
    assert all(A[k] == B[k] for k in A if k[0] == "C" or (k[0] == "D" and not pa[k[1]]["bad"]))
    # both passes fused something: a neighbour's row changed (pKF's points into it), and pKF's row changed
    assert ka[t]["points"] != before[t] and any(ka[s]["points"] != before[s] for s in ka if s != t)
    assert any(p["replaced"] >= 0 for p in pa.values()) and sum(k["mark"] == t for k in ka.values()) > 2 and sum(p["mark"] == t for p in pa.values()) > 20
    assert A[("C", t)] != ["0"] and ka[t]["parent"] >= 0                    # UpdateConnections ran: pKF has its list and its parent
    map_rows_match_the_objects(rec, pa, ka)
    # the map holds the refreshed descriptors of pKF's live points
    for s in set(ka[t]["points"]) - {-1}:
        if not pa[s]["bad"]:
            assert rec["T"][("3", s)][2:10] == A[("D", s)][:8] and rec["T"][("3", s)][10:15] == A[("D", s)][8:13], s
