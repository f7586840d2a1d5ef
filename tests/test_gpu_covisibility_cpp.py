"""The C++ route to the covisibility counting: examples/covisibility_harness builds KeyFrame / MapPoint test doubles from a scene
file, runs adapters/lld_covisibility_adapter.cc on them (UpdateConnections for a list of keyframes in one device call, then
KeyFrameCulling with a fresh call after every keyframe it flags) and prints the members.  They must equal what the same loops
give over tests/covis_ref.py (the object model of tests/covis_scenes.py)."""
import os
import subprocess

import pytest

import covis_scenes as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "covisibility_harness")


def run_harness(tmp_path, world, update, current):
    assert os.path.exists(HARNESS), "examples/covisibility_harness is built by build()"
    path = tmp_path / "scene.bin"
    path.write_bytes(world.blob(update, current))
    out = subprocess.run([HARNESS, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [l.split() for l in out.stdout.strip("\n").split("\n")]


def pairs(words):
    return [tuple(int(x) for x in w.split(":")) for w in words]


def compare(lines, world, update, current):
    n_kf = len(world.kfs)
    world.update_connections(update)
    assert lines[0][0] == "U"
    members = []
    for k in range(n_kf):
        l = lines[1 + k]
        bars = [i for i, w in enumerate(l) if w == "|"]
        assert l[0] == "K" and int(l[1]) == k and len(bars) == 2
        members.append((int(l[2]), int(l[3]), pairs(l[bars[0] + 1:bars[1]]), pairs(l[bars[1] + 1:])))
    for k, kf in enumerate(world.kfs):
        parent, first, conn, ordered = members[k]
        assert conn == sorted(kf.conn.items()), ("mConnectedKeyFrameWeights", k)
        assert ordered == list(zip(kf.ordered, kf.ordered_w)), ("ordered keyframes and weights", k)
        assert parent == kf.parent and first == (1 if kf.first else 0), ("parent", k)
    assert int(lines[0][1]) == sum(1 for k in update if world.kfs[k].conn)      # every listed keyframe with a non-empty counter
    flagged, calls = world.keyframe_culling(current)
    c = lines[1 + n_kf]
    assert c[0] == "C" and [int(x) for x in c[2:]] == flagged and int(c[1]) == calls
    for p in range(len(world.obs)):
        l = lines[2 + n_kf + p]
        assert l[0] == "P" and [int(x) for x in l[1:]] == [p, 1 if world.bad[p] else 0, world.nobs[p], len(world.obs[p])]
    return flagged, calls


def test_requery_after_a_cull_changes_a_later_verdict(gpu_ctx, tmp_path):
    world, current, expect = S.requery_world()
    update = list(range(len(world.kfs)))
    lines = run_harness(tmp_path, world, update, current)
    flagged, calls = compare(lines, world, update, current)
    assert flagged == expect["flagged"] and calls == expect["calls"]          # one call alone would have flagged 1 and 4 too


@pytest.mark.parametrize("seed,monocular", [(1, False), (2, True)])
def test_random_world_members_equal_the_model(gpu_ctx, tmp_path, seed, monocular):
    world = S.random_world(seed, monocular=monocular)
    update = [3, 0, 7, 11, 1, 2, 5, 4, 6, 8, 10, 9, 3]                         # every keyframe, one of them twice
    lines = run_harness(tmp_path, world, update, 5)
    compare(lines, world, update, 5)


def test_partial_update_list_touches_the_neighbours_ordered_lists(gpu_ctx, tmp_path):
    world = S.random_world(3, n_kf=8, n_points=260)
    update = [2, 6]                                                            # the others only receive AddConnection
    lines = run_harness(tmp_path, world, update, 2)
    compare(lines, world, update, 2)
    assert any(kf.conn and kf.idx not in update for kf in world.kfs)
