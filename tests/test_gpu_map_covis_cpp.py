"""The C++ route to covisibility on the resident map: examples/map_covis_harness builds KeyFrame / MapPoint test doubles from a scene file,
mirrors them in a MapOnDevice (adapters/lld_map_adapter.cc, EnableCovisibility), runs MapOnDevice::UpdateConnections for a list of keyframes
and MapOnDevice::KeyFrameCulling, and prints the members.  They must equal the object model of tests/covis_scenes.py, on the three worlds
tests/test_gpu_covisibility_cpp.py uses.  The harness also reads the mirrored map back.  Through lld_map_covisibility: every keyframe that is
left counts what the restatement counts on the model's tables, so the observation rows each SetBadFlag changed did reach the map.  Through
lld_map_download_links, after UpdateConnections and again after the culling walk: every keyframe's parent, cov row and child row on the
device are the model's parent, ordered[:10] and children - the rows Tracking::UpdateLocalMap extends its list by, which only WRITE_COV and
the adapter's pushes (lld_map_set_covisibles, UpdateKeyFrames) wrote."""
import copy
import os
import subprocess

import pytest

import covis_scenes as S
import map_covis_ref as M
from test_gpu_covisibility_cpp import compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "map_covis_harness")


def run_harness(tmp_path, world, update, current):
    assert os.path.exists(HARNESS), "examples/map_covis_harness is built by build()"
    path = tmp_path / "scene.bin"
    path.write_bytes(world.blob(update, current))
    out = subprocess.run([HARNESS, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [l.split() for l in out.stdout.strip("\n").split("\n")]


def check(lines, world, update, current):
    """Members and the culling line as covisibility_harness prints them; then the M lines against the model as it stands after the walk."""
    after_update = copy.deepcopy(world)
    after_update.update_connections(update)
    got = compare(lines, world, update, current)                    # (moves `world` through both routines)
    n_kf = len(world.kfs)
    # the links the map held after each routine, read back from the device: parent, the best ten covisibles in their order, the children.
    # These are the rows Tracking::UpdateLocalMap extends its list by, and nothing but the adapter's pushes and WRITE_COV wrote them.
    for tag, model in (("R1", after_update), ("R2", world)):
        rows = [l for l in lines if l[0] == tag]
        assert [int(l[1]) for l in rows] == list(range(n_kf))
        for l, kf in zip(rows, model.kfs):
            bars = [i for i, w in enumerate(l) if w == "|"]
            assert len(bars) == 2
            assert int(l[2]) == kf.parent, (tag, "parent", kf.idx)
            assert [int(x) for x in l[bars[0] + 1:bars[1]]] == kf.ordered[:10], (tag, "cov row", kf.idx)
            assert [int(x) for x in l[bars[1] + 1:]] == sorted(kf.children), (tag, "children", kf.idx)
    assert any(len(kf.ordered) > 1 for kf in after_update.kfs) and any(kf.parent >= 0 for kf in after_update.kfs)
    lines = [l for l in lines if l[0] not in ("R1", "R2")]
    tail = lines[2 + n_kf + len(world.obs):]
    live = [k.idx for k in world.kfs if not k.bad]
    T = dict(kf={k.idx: dict(key=k.idx + 1, points=[key[3] for key in k.keys]) for k in world.kfs},
             pt={p: dict(bad=world.bad[p], obs=list(o)) for p, o in enumerate(world.obs)})
    assert [int(l[1]) for l in tail] == live and all(l[0] == "M" and l[2] == "|" for l in tail)
    for l, k in zip(tail, live):
        conn = M.connections_query(T, k)[0]
        assert [tuple(int(x) for x in w.split(":")) for w in l[3:]] == conn, ("the mirrored map", k)
    return got


def test_requery_after_a_cull_changes_a_later_verdict(gpu_ctx, tmp_path):
    world, current, expect = S.requery_world()
    update = list(range(len(world.kfs)))
    flagged, calls = check(run_harness(tmp_path, world, update, current), world, update, current)
    assert flagged == expect["flagged"] and calls == expect["calls"]


@pytest.mark.parametrize("seed,monocular", [(1, False), (2, True)])
def test_random_world_members_equal_the_model(gpu_ctx, tmp_path, seed, monocular):
    world = S.random_world(seed, monocular=monocular)
    update = [3, 0, 7, 11, 1, 2, 5, 4, 6, 8, 10, 9, 3]                         # every keyframe, one of them twice
    check(run_harness(tmp_path, world, update, 5), world, update, 5)


def test_partial_update_list_touches_the_neighbours_ordered_lists(gpu_ctx, tmp_path):
    world = S.random_world(3, n_kf=8, n_points=260)
    update = [2, 6]                                                            # the others only receive AddConnection
    check(run_harness(tmp_path, world, update, 2), world, update, 2)
    assert any(kf.conn and kf.idx not in update for kf in world.kfs)
