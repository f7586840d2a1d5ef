"""The C++ route to the landmark refresh: examples/landmark_harness builds KeyFrame / MapPoint / MapLine test doubles from a scene
file and runs adapters/lld_landmark_adapter.cc on them (gather in std::map order, one device call, scatter).  The members after
the call must equal tests/landmark_ref.py's bit for bit; a landmark the reference returns early on keeps what it held."""
import os
import subprocess

import numpy as np
import pytest

import landmark_ref as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "landmark_harness")


def words(ws):
    return np.array([int(x, 16) for x in ws], np.uint32)


@pytest.mark.parametrize("flags", [L.DESCRIPTOR | L.NORMAL_DEPTH, L.NORMAL_DEPTH])
def test_members_after_the_adapter_equal_the_restatement(gpu_ctx, tmp_path, flags):
    assert os.path.exists(HARNESS), "examples/landmark_harness is built by build()"
    n_kf, dim = 40, 72
    pts = L.make_point_scene(51, 150, n_kf=n_kf, counts=list(np.random.default_rng(5).integers(0, 41, 148)) + [40, 40])
    lns = L.make_line_scene(52, n_kf=n_kf, dim=dim, scaled=True, counts=np.random.default_rng(6).integers(0, 25, 60))
    lns["kf_bad"] = pts["kf_bad"].copy()                                      # one keyframe array serves both
    n, nl = len(pts["bad"]), len(lns["bad"])
    # a point whose mpRefKF is not among its observations: the first good point that does not see keyframe r
    absent = None
    for i in range(n):
        s, e = pts["obs_start"][i], pts["obs_start"][i + 1]
        if not pts["bad"][i] and e - s >= 2 and e - s < n_kf:
            r = next(k for k in range(n_kf) if k not in set(pts["obs_kf"][s:e].tolist()))
            pts["ref_kf"][i] = r
            absent = i
            break
    assert absent is not None
    for i in range(n):                                                        # every other reference keyframe is an observer
        s, e = pts["obs_start"][i], pts["obs_start"][i + 1]
        if i != absent and e > s:
            pts["ref_kf"][i] = pts["obs_kf"][s + (i % (e - s))]
    rng = np.random.default_rng(3)
    prior = dict(desc=rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32), normal=rng.normal(size=(n, 3)).astype(np.float32),
                 min_distance=rng.random(n).astype(np.float32), max_distance=rng.random(n).astype(np.float32))
    prior_lines = rng.normal(size=(nl, dim)).astype(np.float32)
    blob, ref_level = L.object_scene_blob(pts, lns, flags, prior, prior_lines)
    assert ref_level[absent] == pts["ref_kf"][absent] % pts["n_levels"]       # the octave of keypoint 0 of that keyframe
    path = tmp_path / "scene.bin"
    path.write_bytes(blob)
    out = subprocess.run([HARNESS, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l.split() for l in out.stdout.strip("\n").split("\n")]
    assert len(lines) == 1 + n + nl and lines[0][0] == "R"
    exp = L.refresh_map_points_ref(dict(pts, ref_level=ref_level), flags, prior)
    expl = L.distinctive_lines_ref(lns, prior_lines)
    assert [int(x) for x in lines[0][1:]] == [int(np.sum(exp["updated"] != 0)), int(np.sum(expl["updated"] != 0))]
    assert exp["updated"][absent] & L.NORMAL_DEPTH and np.any(exp["updated"] == 0)
    for i in range(n):
        l = lines[1 + i]
        assert l[0] == "P" and int(l[1]) == i
        w = words(l[2:])
        assert np.array_equal(w[:8], exp["desc"][i]), i
        assert np.array_equal(w[8:11], exp["normal"][i].view(np.uint32)), i
        assert w[11] == exp["min_distance"][i:i + 1].view(np.uint32)[0] and w[12] == exp["max_distance"][i:i + 1].view(np.uint32)[0], i
    for i in range(nl):
        l = lines[1 + n + i]
        assert l[0] == "L" and int(l[1]) == i
        assert np.array_equal(words(l[2:]), expl["desc"][i].view(np.uint32)), i
