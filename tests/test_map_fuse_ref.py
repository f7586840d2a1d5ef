"""The plain-Python restatement of lld_map_fuse (tests/map_fuse_ref.py) held to scenes small enough to be worked out on paper
(tests/map_fuse_scenes.py, "the paper scenes": the expectation is written out next to each map), the interface of the call (structs, constants,
prototypes, exported symbols), and the scene builders' own guarantees.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import map_fuse_ref as F
import map_fuse_scenes as FS
from lld_slam_amd import abi, device_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(FS.PAPER))
def test_paper_scenes(name):
    m, c, slots, want = FS.PAPER[name]()
    m2, out = FS.run_ref(m, c, slots)
    assert out["match"].tolist() == want["match"], (name, out["match"])
    assert out["action"].tolist() == want["action"] and out["other"].tolist() == want["other"], (name, out["action"], out["other"])
    assert out["survivor"].tolist() == want["survivor"]
    acts = want["action"]
    assert out["n_fused"] == sum(a in (1, 2, 3, 4) for a in acts) and out["n_added"] == acts.count(1) and out["n_replaced"] == sum(a in (2, 3) for a in acts)
    for s, n in want["n_obs"].items():
        assert F.n_obs_of(m2["points"][s]) == n, (name, "n_obs", s)
    assert sorted(s for s, p in m2["points"].items() if p["bad"]) == sorted(want["bad"])
    for s, row in want["obs"].items():
        assert m2["points"][s]["obs"] == row, (name, "obs", s, m2["points"][s]["obs"])
    for kf, row in want["points"].items():
        assert m2["keyframes"][kf]["points"] == row, (name, "points", kf, m2["keyframes"][kf]["points"])
    # whatever the expectation does not name is as it was, and the input map was not touched
    for s, p in m["points"].items():
        if s not in want["obs"]:
            assert m2["points"][s]["obs"] == p["obs"] and m2["points"][s]["bad"] == p["bad"] and m2["points"][s]["n_obs"] == p["n_obs"]
    for kf, k in m["keyframes"].items():
        if kf not in want["points"]:
            assert m2["keyframes"][kf]["points"] == k["points"]
    # a survivor's descriptor is one of its observers' rows; nobody else's descriptor moved
    for s, p in m["points"].items():
        if s in want["survivor"]:
            rows = [m2["keyframes"][kf]["desc"][i].tolist() for kf, i in m2["points"][s]["obs"]]
            assert m2["points"][s]["desc"].tolist() in rows
        else:
            assert np.array_equal(m2["points"][s]["desc"], p["desc"])


def test_the_tie_is_decided_by_the_grid_and_not_by_the_index():
    m, c, slots, want = FS.tie_between_cells()
    kf = m["keyframes"][0]
    assert np.array_equal(kf["desc"][0], kf["desc"][1]) and kf["uvr"][0][0] > kf["uvr"][1][0]
    cells = F.grid_cells(kf["uvr"], FS.GRID)
    assert cells == {(31, 20): [0], (29, 20): [1]}
    # with the two keypoints in one column the lower index wins: the order of the cells decided above
    kf["uvr"][0][0] = np.float32(304); kf["uvr"][1][0] = np.float32(296)
    assert set(F.grid_cells(kf["uvr"], FS.GRID)) == {(30, 20)}
    assert F.search(m, 0, slots, c["view"], c["grid"], c["level_scale"], c["inv_sigma2"]).tolist() == [0]


def test_the_search_skips_what_the_reference_skips():
    m, c, slots, _ = FS.replace_each_way()
    P = m["points"]
    held = m["keyframes"][0]["points"][0]
    never = max(P) + 1
    bad = slots[1]; P[bad]["bad"] = 1
    got = F.search(m, 0, [-1, never, bad, held, slots[0]], c["view"], c["grid"], c["level_scale"], c["inv_sigma2"])
    assert got.tolist() == [-1, -1, -1, -1, 0]


def test_source_keyframe_is_the_row_as_a_list():
    m, c, slots = FS.random_scene(1)
    src = next(s for s in m["keyframes"] if s != c["target"] and len(m["keyframes"][s]["points"]) > 4)
    a = FS.run_ref(m, c, list(m["keyframes"][src]["points"]))
    b = FS.run_ref(m, c, None, source_keyframe=src)
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_scenes_fuse_and_take_every_action(seed):
    m, c, slots = FS.random_scene(seed)                                     # asserts a quarter fused and every action taken
    m2, out = FS.run_ref(m, c, slots)
    assert -1 in slots and len(set(slots)) < len(slots) and any(s >= 0 and s not in m["points"] for s in slots)
    # the rows stay parallel and in key order, Observations() is the stereo-weighted length wherever the walk wrote it
    K = m2["keyframes"]
    for s, p in m2["points"].items():
        keys = [K[kf]["key"] for kf, _ in p["obs"]]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        if not p["bad"]:
            assert p["n_obs"] == sum(2 if F.stereo(m2, kf, i) else 1 for kf, i in p["obs"]), s
            for kf, i in p["obs"]:
                assert K[kf]["points"][i] == s, (s, kf, i)


def test_rows_and_limit_scenes_do_what_they_say():
    m, c, slots, what = FS.rows_scene()
    m2, out = FS.run_ref(m, c, slots)
    assert out["action"].tolist() == [a for _, a in what]
    for s, h, (L, a) in zip(slots, out["other"], what):
        loser = s if a == F.CANDIDATE_REPLACED else int(h)
        assert len(m["points"][loser]["obs"]) == L and m2["points"][loser]["obs"] == []
    m, c, slots = FS.limit_scene(False)
    m2, out = FS.run_ref(m, c, slots)
    assert out["action"].tolist() == [F.HOLDER_REPLACED] and len(m2["points"][slots[0]]["obs"]) == F.MAX_OBS
    m, c, slots = FS.limit_scene(True)
    assert FS.run_ref(m, c, slots)[1] is None


# ---------------------------------------------------------------------------------------------------------------- the interface
NAMES = ["lld_map_fuse", "lld_map_download_point_counts"]


def test_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    assert callable(device_map.DeviceMap.fuse) and callable(device_map.DeviceMap.point_counts)


def test_struct_layouts_constants_and_prototypes(tmp_path):
    structs = [("lld_map_fuse_in", abi.MapFuseIn), ("lld_map_fuse_out", abi.MapFuseOut), ("lld_frame_view", abi.FrameViewStruct)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += ('printf("%d\\n%d\\n%d\\n%d\\n%d\\n%d\\n", LLD_MAP_FUSE_NONE, LLD_MAP_FUSE_ADDED, LLD_MAP_FUSE_CANDIDATE_REPLACED, LLD_MAP_FUSE_HOLDER_REPLACED, '
             'LLD_MAP_FUSE_HOLDER_BAD, LLD_MAP_FUSE_SKIPPED);')
    want += [abi.MAP_FUSE_NONE, abi.MAP_FUSE_ADDED, abi.MAP_FUSE_CANDIDATE_REPLACED, abi.MAP_FUSE_HOLDER_REPLACED, abi.MAP_FUSE_HOLDER_BAD, abi.MAP_FUSE_SKIPPED]
    assert want[-6:] == [F.NONE, F.ADDED, F.CANDIDATE_REPLACED, F.HOLDER_REPLACED, F.HOLDER_BAD, F.SKIPPED] and F.MAX_OBS == abi.LANDMARK_MAX_OBS
    calls = ["lld_map_fuse((lld_map*)0, (const lld_map_fuse_in*)0, (lld_map_fuse_out*)0)",
             "lld_map_download_point_counts((lld_map*)0, 0, (const int32_t*)0, (int32_t*)0)"]
    for call in calls:
        body += f'printf("%zu\\n", sizeof({call}));'
    want += [ctypes.sizeof(ctypes.c_int)] * len(calls)
    src = tmp_path / "map_fuse.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "map_fuse"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_null_handles_are_refused_without_a_device():
    dll = ctypes.CDLL(abi.product_library_path())
    for n in NAMES:
        getattr(dll, n).restype = ctypes.c_int
    a, o = abi.MapFuseIn(), abi.MapFuseOut()
    assert dll.lld_map_fuse(None, ctypes.byref(a), ctypes.byref(o)) == abi.LLD_ERR_INVALID
    assert dll.lld_map_download_point_counts(None, 0, None, None) == abi.LLD_ERR_INVALID
