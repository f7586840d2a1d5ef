"""The C++ route to local bundle adjustment on the resident map: examples/map_ba_harness builds two identical copies of the object graph
examples/adapter_harness runs `ba` on (examples/lba_graph.h: shuffled addresses, permuted mnIds, a local keyframe with mnId 0, a bad
covisible keyframe that also observes, a bad MapPoint, a MapLine with two observations), runs lld_adapter::LocalBundleAdjustment on one and
MapOnDevice::LocalBundleAdjustment on the other, and compares in place: the traces' windows and outputs byte for byte, then both graphs -
poses, positions, matches, observations and the visit marks.  A second call, with a neighbour as pKF, runs on the map as the first call's
push-back left it and must again equal the host adapter's: that is the proof that poses, points, lines and erased observations reached the
device."""
import os
import re
import subprocess

import pytest

from lld_slam_amd import synth
from test_cpp_adapter import _as_dict
from test_cpp_harness import write_ba

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "map_ba_harness")


@pytest.mark.parametrize("wid,kw,seed", [
    (0, dict(), 1),
    (1, dict(mono_frac=0.2, mono_line_frac=0.25, n_fixed=3), 2),
    (4, dict(n_free=10, n_fixed=3, n_points=700, n_lines=120, outlier_frac=0.15), 3),
])
def test_map_route_equals_the_host_adapter_on_identical_graphs(gpu_ctx, tmp_path, wid, kw, seed):
    assert os.path.exists(HARNESS), "examples/map_ba_harness is built by build()"
    w = synth.make_lba_small(wid, **kw)
    write_ba(tmp_path / "in.bin", _as_dict(w))
    r = subprocess.run([HARNESS, "check", str(tmp_path / "in.bin"), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip("\n").split("\n")
    assert len(lines) == 3 and lines[2] == "differences 0", r.stdout + r.stderr
    calls = [dict(zip(("call", "pkf", "cams", "free", "points", "pt_obs", "lines", "ln_obs"), [int(x) for x in re.findall(r"-?\d+", l.split(";")[0])])) for l in lines[:2]]
    tails = [[int(x) for x in re.findall(r"\d+", ";".join(l.split(";")[2:]))] for l in lines[:2]]          # erased points, erased lines, address inversions, bad marked
    first, second = calls
    # the first window is the input's: every camera, every point and line but the ones the reference skips
    assert (first["cams"], first["free"], first["points"], first["lines"]) == (w.n_cams, w.n_free_cams, w.n_points, w.n_lines)
    assert first["pt_obs"] == w.n_pt_obs and first["ln_obs"] == w.n_ln_obs
    assert second["pkf"] != first["pkf"] and second["points"] > 0 and second["lines"] > 0 and second["free"] == first["free"]
    # the first call erased observations (so the second call's rows came through the push-back), pointer order is not mnId order, and in
    # the second call the bad keyframe that observes local points was marked fixed although it is no camera
    assert tails[0][0] + tails[0][1] > 0 and tails[0][2] > 0 and (tails[0][3], tails[1][3]) == (0, 1)     # (a neighbour in the first call: marked local)
    assert second["pt_obs"] + second["ln_obs"] < first["pt_obs"] + first["ln_obs"]
