"""Tracking::UpdateLocalMap on the resident map past the fixed widths of its kernels (lld_map.hip), against the plain-Python restatement in
tests/local_map_ref.py: child rows longer than the 32 entries kept in LDS and than one 64-lane trip behind them, point and line rows and
keyframe lists longer than a tile of 256, a frame of more than 256 keypoints, the marks' bit set at its largest and with a partial last
word, and the extension loop's limit of 80 from both sides.  All integers, all equal; every scene asserts that it crossed its width."""
import copy

import numpy as np
import pytest

import local_map_ref as REF
import local_map_scenes as SC
from lld_slam_amd import abi, synth
from lld_slam_amd.device_map import DeviceMap
from lld_slam_amd.tracking import DeviceTrackedFrame
from test_gpu_local_map import same

pytestmark = pytest.mark.gpu

SCENES = SC.width_scenes() + [SC.frame_1000(), SC.slots_scene(1 << 18)]


@pytest.fixture(scope="module")
def frames(gpu_ctx):
    """one resident frame of 256 keypoints and one of 1 000"""
    out = {}
    with DeviceTrackedFrame(gpu_ctx, synth.make_orb_frame(0, 256), synth.KITTI_CAM) as a, DeviceTrackedFrame(gpu_ctx, synth.make_orb_frame(0, 1000), synth.KITTI_CAM) as b:
        out[256], out[1000] = a, b
        yield out


def one_frame(tf, nt, dm, ids):
    kp = np.full(nt, -1, np.int32); kp[:len(ids)] = ids
    tf.set_state(np.eye(4, dtype=np.float32), kp, np.zeros((nt, 3), np.float32))
    tf.update_local_map(dm)
    got = tf.local_map_download(dm, stage2=False)
    kept = tf.finish(35.0, 10 ** 6, depth=np.full(nt, -1, np.float32), force=0)["kp_point_id"]
    return got, kept[:len(ids)]


def run_scene(ctx, frames, sc):
    sc = copy.deepcopy(sc)
    L, m, state, out = sc["limits"], sc["map"], REF.new_state(), []
    nt = 1000 if any(len(s.get("frame", ())) > 256 for s in sc["steps"]) else 256
    with DeviceMap(ctx, **L) as dm:
        SC.upload(dm, m)
        for step in sc["steps"]:
            got, kept = one_frame(frames[nt], nt, dm, step["frame"])
            exp = REF.update_local_map(state, m, step["frame"], L["max_local_points"], L["max_local_lines"])
            same(got, kept, exp, sc["name"])
            out.append((got, exp))
    return out


@pytest.mark.parametrize("sc", SCENES, ids=[s["name"] for s in SCENES])
def test_scene_matches_the_reference(gpu_ctx, frames, sc):
    res = run_scene(gpu_ctx, frames, sc)
    name, K = sc["name"], sc["map"]["keyframes"]
    got, last = res[-1]
    if name.startswith("children_"):
        n = int(name.split("_")[1])
        rows = [K[v]["child"] for v in range(6)]
        kfs = got["local_keyframes"].tolist()
        # the child row is n long, two consecutive entries share it, and the winners sit where the walk changes: LDS, the first HBM entry,
        # the last (partial) trip, HBM behind a bad LDS child with the smallest key; one winner's key is above 2^63
        assert all(len(r) == n for r in rows) and n > SC.CHILD_LDS and rows[0] == rows[1] and len(kfs) == 12
        assert [rows[v].index(kfs[6 + v]) for v in range(4)] == SC.children_winner_positions(n)
        assert K[kfs[9]]["key"] > 2 ** 63 and min(K[c]["key"] for c in rows[3][:SC.CHILD_LDS]) == 1 and K[rows[3][3]]["bad"]
        assert sum(1 for c in rows[2] if c in kfs[:8]) >= 4                                  # marked children in the row
    if name in ("row_257", "row_513"):
        n = int(name.split("_")[1])
        assert len(K[1]["points"]) == len(K[1]["lines"]) == n > (n - 1) // SC.TILE * SC.TILE >= SC.TILE        # two or three tiles
        assert last["status"] == 0 and got["n_local_points"] == sc["limits"]["max_local_points"] and got["n_local_lines"] == sc["limits"]["max_local_lines"]
        assert got["local_lines"].tolist().count(200) == 1 and K[1]["lines"][SC.TILE] == 200 and got["local_points"][:3].tolist() == [n + 1, 2, 255]
        # the second tile has first occurrences to write behind the first one's (the point row's entry 256 among them)
        assert (K[1]["points"][SC.TILE] == 200) == (n > 257) and got["local_points"][-1] == (SC.TILE if n == 257 else n - 3)
    if name == "row_257_over":
        assert last["status"] == REF.POINT_OVERFLOW | REF.LINE_OVERFLOW and got["n_local_points"] == sc["limits"]["max_local_points"] + 1
    if name == "prefix_600":
        kfs = got["local_keyframes"].tolist()
        assert len(kfs) == 600 > 2 * SC.TILE and kfs != sorted(kfs) and got["n_local_points"] == 1500 and got["n_local_lines"] == 86
        own = [sum(1 for p in K[k]["points"][:3] if p // 3 == k) for k in kfs]               # every listed keyframe moves the lists
        assert min(own) >= 2
    if name == "voted_40":
        assert got["local_keyframes"].tolist() == list(range(80))                           # every entry is visited, the list ends at 80
    if name == "voted_80":
        assert got["local_keyframes"].tolist() == list(range(80)) + [80]                    # 80 is not more than 80: the first entry is visited
    if name == "voted_81":
        assert got["local_keyframes"].tolist() == list(range(81))                           # no entry is visited
    if name == "frame_1000":
        assert [e["n_bad_cleared"] for _, e in res] == [2, 4] and [e["n_voted"] for _, e in res] == [6, 2]
        assert [g["n_bad_cleared"] for g, _ in res] == [2, 4] and res[0][0]["local_keyframes"].tolist() == [5, 4, 3, 2, 1, 0]
    if name.startswith("slots_"):
        nk = sc["limits"]["max_keyframes"]
        want = SC.slots_expected(nk)                                                         # written out by hand
        for k, v in want.items():
            assert (got[k].tolist() if isinstance(got[k], np.ndarray) else got[k]) == v, (name, k)
        assert nk in (33, 1 << 18) and max(want["local_keyframes"]) == nk - 1


def test_one_keyframe_slot_too_many_is_refused(gpu_ctx):
    L = dict(SC.slots_scene(33)["limits"], max_keyframes=(1 << 18) + 1)
    with pytest.raises(RuntimeError) as e:
        DeviceMap(gpu_ctx, **L)
    assert e.value.status == abi.LLD_ERR_UNSUPPORTED
    with DeviceMap(gpu_ctx, **dict(L, max_keyframes=1 << 18)) as dm:
        assert dm.handle is not None
