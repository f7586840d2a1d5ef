"""The C++ route to new map points: examples/new_points_harness builds KeyFrame / MapPoint / Map test doubles from a scene file and
runs adapters/lld_localmapping_adapter.cc on them - LocalMapping::CreateNewMapPoints with its sequential neighbour loop, ComputeF12
on the host, the SearchForTriangulation adapter, one lld_new_points_triangulate call per neighbour, the reference's bookkeeping
and one landmark refresh at the end.  Expected: the same loop here with the oracle's SearchForTriangulation (the matcher path of
tests/test_cpp_adapter.py), tests/newpoints_ref.py and tests/landmark_ref.py."""
import functools
import os
import subprocess

import numpy as np
import pytest

import landmark_ref as L
import newpoints_ref as R
import oracle_orbsearch as OS
from initializer_ref import inv3, mm
from lld_slam_amd.orb_search import Frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "new_points_harness")
F32 = np.float32
N_NODES = 24


def compute_f12(kf1, kf2):
    """LocalMapping::ComputeF12 (:537-554) with the product and inverse rules of include/lld_amd.h."""
    R12 = mm(kf1["Rcw"], kf2["Rcw"].T)
    t12 = (-mm(R12, kf2["tcw"]) + kf1["tcw"]).astype(F32)
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], F32)
    K = lambda k: np.array([[k["fx"], 0, k["cx"]], [0, k["fy"], k["cy"]], [0, 0, 1]], F32)
    return mm(mm(mm(inv3(K(kf1).T.copy()), tx), R12), inv3(K(kf2)))


@functools.lru_cache(maxsize=None)
def object_scene():
    """The seeded scene of newpoints_ref (4 neighbours, the second below the baseline gate) plus what the matcher needs: a
    descriptor per keypoint (a neighbour's matched keypoint carries keyframe 1's with up to 12 bits flipped), a vocabulary node per
    keypoint, and keypoints shared between the neighbours' matches, so that a later neighbour would re-use them."""
    pb = R.make_scene(41, [150, 120, 150, 150], n_keys1=400)
    rng = np.random.default_rng(4)
    n1 = len(pb["keys1"]["ur"])
    rand_desc = lambda n: rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    desc1 = rand_desc(n1)
    node1 = (np.arange(n1) % N_NODES).astype(np.int32)
    kfs = [dict(kf=pb["kf1"], keys=pb["keys1"], desc=desc1, node=node1)]
    ks, ms = pb["key_start"], pb["match_start"]
    for p, kf2 in enumerate(pb["kf2"]):
        k2 = {k: v[ks[p]:ks[p + 1]].copy() for k, v in pb["keys2"].items()}
        n2 = len(k2["ur"])
        d2 = rand_desc(n2); nd2 = rng.integers(0, N_NODES, n2).astype(np.int32)
        for i1, i2 in pb["matches"][ms[p]:ms[p + 1]]:
            flips = np.zeros(8, np.uint32)
            for bit in rng.integers(0, 256, rng.integers(0, 13)):
                flips[bit // 32] ^= np.uint32(1) << np.uint32(bit % 32)
            d2[i2] = desc1[i1] ^ flips; nd2[i2] = node1[i1]
        kfs.append(dict(kf=kf2, keys=k2, desc=d2, node=nd2))
    return pb, kfs


def blob(kfs, monocular, stop_at):
    kf0 = kfs[0]["kf"]
    out = [np.array([len(kfs), len(kf0["scale_factors"]), int(monocular), stop_at], np.int32).tobytes(),
           np.array([kf0["scale_factor"]], F32).tobytes(), kf0["scale_factors"].astype(F32).tobytes(), kf0["level_sigma2"].astype(F32).tobytes()]
    for e in kfs:
        kf, k = e["kf"], e["keys"]
        T = np.eye(4, dtype=F32); T[:3, :3] = kf["Rcw"]; T[:3, 3] = kf["tcw"]
        out += [T.tobytes(), np.array([kf[q] for q in ("fx", "fy", "cx", "cy", "mb", "mbf")], F32).tobytes(), np.array([len(k["ur"])], np.int32).tobytes()]
        for i in range(len(k["ur"])):
            out += [np.array([k["xy"][i, 0], k["xy"][i, 1], k["raw_xy"][i, 0], k["raw_xy"][i, 1], k["ur"][i], k["depth"][i]], F32).tobytes(),
                    np.array([k["octave"][i]], np.int32).tobytes(), e["desc"][i].astype(np.uint32).tobytes()]
        nodes = [(n, np.flatnonzero(e["node"] == n).astype(np.int32)) for n in range(N_NODES) if np.any(e["node"] == n)]
        out.append(np.array([len(nodes)], np.int32).tobytes())
        for n, idx in nodes:
            out += [np.array([n, len(idx)], np.int32).tobytes(), idx.tobytes()]
    return b"".join(out)


def csr(node):
    order = np.argsort(node, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=N_NODES))]).astype(np.int32)
    return start, order


def frame_of(e):
    k = e["keys"]
    return Frame(desc=e["desc"], xy=k["xy"], octave=k["octave"], uright=k["ur"], angle=np.zeros(len(k["ur"]), F32))


def expected(kfs, monocular, stop_at):
    """CreateNewMapPoints on the same scene: (per neighbour visited (k, skipped, n_matches, n_new), created points, early)."""
    cur = kfs[0]
    has1 = np.zeros(len(cur["keys"]["ur"]), np.uint8)
    Ow1 = R.derived(cur["kf"])[1]
    visited, points, calls, early = [], [], 0, False
    s1, i1 = csr(cur["node"])
    for k in range(1, len(kfs)):
        if k > 1:
            calls += 1
            if stop_at > 0 and calls >= stop_at:
                early = True
                break
        nb = kfs[k]
        if R.pair_gate(cur["kf"], nb["kf"], monocular)[0]:
            visited.append((k, 1, 0, 0))
            continue
        F12 = compute_f12(cur["kf"], nb["kf"])
        Rd, Od = nb["kf"]["Rcw"].astype(np.float64), Ow1.astype(np.float64)     # C2 = R2w*Cw+t2w as the matcher adapter forms it: one rounding
        C2 = (((Rd[:, 0] * Od[0] + Rd[:, 1] * Od[1]) + Rd[:, 2] * Od[2]) + nb["kf"]["tcw"].astype(np.float64)).astype(F32)
        invz = F32(1.0) / C2[2]
        epipole = (float(nb["kf"]["fx"] * C2[0] * invz + nb["kf"]["cx"]), float(nb["kf"]["fy"] * C2[1] * invz + nb["kf"]["cy"]))
        s2, i2 = csr(nb["node"])
        _, m12 = OS.search_for_triangulation(frame_of(cur), frame_of(nb), N_NODES, s1, i1, s2, i2, has1, np.zeros(len(nb["keys"]["ur"]), np.uint8),
                                             F12, epipole, False, False)
        matches = np.array([(a, m12[a]) for a in range(len(m12)) if m12[a] >= 0], np.int32).reshape(-1, 2)
        r = R.triangulate_pair(cur["kf"], cur["keys"], nb["kf"], nb["keys"], matches, monocular)
        new = np.flatnonzero(r["status"] == R.NEW)
        for q in new:
            points.append((k, int(matches[q, 0]), int(matches[q, 1]), r["x3d"][q]))
            has1[matches[q, 0]] = 1
        visited.append((k, 0, len(matches), len(new)))
    return visited, points, early, {k: compute_f12(cur["kf"], kfs[k]["kf"]) for k in range(1, len(kfs))}


def refreshed(kfs, points):
    """tests/landmark_ref.py on the new points: two observations each, in keyframe index order (the std::map order of the doubles)."""
    n = len(points)
    sc = dict(obs_start=np.arange(0, 2 * n + 1, 2, dtype=np.int32), obs_kf=np.array([[0, k] for k, _, _, _ in points], np.int32).reshape(-1),
              obs_desc=np.array([[kfs[0]["desc"][a], kfs[k]["desc"][b]] for k, a, b, _ in points], np.uint32).reshape(-1, 8),
              kf_bad=np.zeros(len(kfs), np.uint8), kf_ow=np.array([R.derived(e["kf"])[1] for e in kfs], F32),
              pos=np.array([x for _, _, _, x in points], F32).reshape(-1, 3), bad=np.zeros(n, np.uint8), ref_kf=np.zeros(n, np.int32),
              ref_level=np.array([kfs[0]["keys"]["octave"][a] for _, a, _, _ in points], np.int32),
              level_scale=kfs[0]["kf"]["scale_factors"], n_levels=len(kfs[0]["kf"]["scale_factors"]))
    return L.refresh_map_points_ref(sc)


def run(tmp_path, kfs, monocular, stop_at):
    assert os.path.exists(HARNESS), "examples/new_points_harness is built by build()"
    path = tmp_path / "scene.bin"
    path.write_bytes(blob(kfs, monocular, stop_at))
    out = subprocess.run([HARNESS, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [l.split() for l in out.stdout.strip("\n").split("\n")]
    return ({int(r[1]): np.array([int(x, 16) for x in r[2:]], np.uint32) for r in rows if r[0] == "F"},
            [[int(x) for x in r[1:]] for r in rows if r[0] == "R"][0], [tuple(int(x) for x in r[1:]) for r in rows if r[0] == "N"],
            [([int(x) for x in r[1:5]], np.array([int(x, 16) for x in r[5:]], np.uint32)) for r in rows if r[0] == "P"])


def compare(tmp_path, stop_at):
    pb, kfs = object_scene()
    F, (nnew, early), visited, pts = run(tmp_path, kfs, pb["monocular"], stop_at)
    e_visited, e_pts, e_early, e_F = expected(kfs, pb["monocular"], stop_at)
    for k, f in e_F.items():
        assert np.array_equal(F[k], f.reshape(-1).view(np.uint32)), "ComputeF12 of neighbour %d" % k
    assert visited == e_visited and bool(early) == e_early and nnew == len(e_pts) == len(pts)
    ref = refreshed(kfs, e_pts)
    for q, ((ids, w), (k, a, b, x)) in enumerate(zip(pts, e_pts)):             # the same points in the same order
        assert ids == [0, k, a, b], q
        assert np.array_equal(w[:3], x.view(np.uint32)), q
        assert np.array_equal(w[3:11], ref["desc"][q]), q                       # the same descriptors, normals and depth limits
        assert np.array_equal(w[11:14], ref["normal"][q].view(np.uint32)), q
        assert w[14] == ref["min_distance"][q:q + 1].view(np.uint32)[0] and w[15] == ref["max_distance"][q:q + 1].view(np.uint32)[0], q
    return pb, visited, pts


def test_created_points_equal_the_restatements(tmp_path):
    pb, visited, pts = compare(tmp_path, 0)
    assert [v[1] for v in visited] == [0, 1, 0, 0] and all(v[3] > 40 for v in visited if not v[1])
    # a later neighbour never re-uses a keypoint of the current keyframe that an earlier one consumed, although the scene offers it
    idx1 = [ids[2] for ids, _ in pts]
    assert len(set(idx1)) == len(idx1)
    ms = pb["match_start"]
    offered = [set(pb["matches"][ms[p]:ms[p + 1], 0].tolist()) for p in range(len(pb["kf2"]))]
    taken_first = {ids[2] for ids, _ in pts if ids[1] == 1}
    assert len(taken_first & offered[2]) > 20 and len(taken_first & offered[3]) > 20
    for p in range(len(pb["kf2"])):                                            # nor a keypoint of the neighbour twice
        idx2 = [ids[3] for ids, _ in pts if ids[1] == p + 1]
        assert len(set(idx2)) == len(idx2)


@pytest.mark.parametrize("stop_at", [1, 2])
def test_early_return_when_the_predicate_fires(tmp_path, stop_at):
    _, visited, pts = compare(tmp_path, stop_at)
    assert len(visited) == stop_at and {ids[1] for ids, _ in pts} <= set(range(1, stop_at + 1))
    assert len(pts) > 40                                                        # the points created before the return are kept and refreshed
