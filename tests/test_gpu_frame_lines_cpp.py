"""lld_frame_build_lines / lld_frame_new_map_lines from compiled C++ (examples/frame_lines_harness.cpp): over include/lld_amd.hpp against the Python
route's integers, and through adapters/lld_tracking_adapter.cc on the object doubles against the host adapters of adapters/lld_line_adapter.cc."""
import os
import subprocess

import numpy as np
import pytest

import frame_lines_scenes as FS
from lld_slam_amd.tracking import DeviceTrackedFrame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "frame_lines_harness")
SEED, FIRST = 0, 300


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "frame_lines_harness"], check=True, capture_output=True)
    d = tmp_path_factory.mktemp("frame_lines")
    S = FS.last_kf_scene(SEED)
    FS.write_pair_scene(str(d / "in.bin"), S, FIRST)
    r = subprocess.run([HARNESS, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return S, FS.read_pair_result(str(d / "out.bin"), 96, 96)


def test_hpp_route_equals_the_python_route(gpu_ctx, result):
    S, R = result
    h = R["hpp"]
    with DeviceTrackedFrame(gpu_ctx, FS.keypoint_frame(), FS.CAM, S["cur"]) as cur, DeviceTrackedFrame(gpu_ctx, FS.keypoint_frame(), FS.CAM, S["last"]) as last:
        FS.set_line_state(cur, S["T_cur"], S["cur_state"]); FS.set_line_state(last, S["T_last"], S["last_state"])
        np.testing.assert_array_equal(h["cur_matches"], cur.lines_download()[0])
        np.testing.assert_array_equal(h["last_matches"], last.lines_download()[0])
        g = cur.new_map_lines(last, FIRST)
        for k in ("match_last", "new_id", "created"):
            np.testing.assert_array_equal(h[k], g[k], err_msg=k)
        assert (h["n_created"], h["n_held"], h["ret"]) == (g["n_created"], g["n_held"], g["n_created"] + g["n_held"]) and g["n_created"] >= 3
        # the chain on the frame afterwards: an empty local map, the stage record lists what the frame holds - the created lines under their new ids
        cur.track_local_map(dict(world_pos=np.zeros((0, 3), np.float32), normal=np.zeros((0, 3), np.float32), max_distance=np.zeros(0, np.float32),
                                 min_distance=np.zeros(0, np.float32), desc=np.zeros((0, 8), np.uint32), has_obs=np.zeros(0, np.uint8), skip=np.zeros(0, np.uint8)),
                            np.zeros(0, np.int32))
        r2 = cur.download()[1]
    np.testing.assert_array_equal(h["stage2_line_id"], r2["ln_line_id"])
    want = S["cur_state"]["ln_line_id"].copy(); want[g["created"] != 0] = g["new_id"][g["created"] != 0]
    np.testing.assert_array_equal(h["stage2_line_id"], want)


def test_adapter_forms_on_the_object_doubles(oracle, result):
    S, R = result
    dev, host = R["device"], R["host"]
    # the constructor form: mCurrentFrame.line_matches = the host MatchLines adapter's = the oracle's
    np.testing.assert_array_equal(R["ctor_matches"], R["host_matches"])
    np.testing.assert_array_equal(R["ctor_matches"], FS.oracle_stereo(oracle, S["cur"])[0])
    # MatchLinesLastKF on FrameOnDevices creates the MapLines lld_adapter::MatchLinesLastKF creates from host arrays
    assert dev["ret"] == host["ret"] and dev["n_map"] == host["n_map"]
    for k in ("match_last", "created_id", "bookkeeping", "frame_ids", "kf_ids"):
        np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
    made = dev["created_id"] >= 0
    assert made.sum() >= 3 and dev["n_map"] == made.sum() and np.all(dev["bookkeeping"][made] == 1)
    np.testing.assert_array_equal(dev["created_id"][made], FIRST + np.arange(made.sum()))      # MapLine::nNextId in creation order
    np.testing.assert_array_equal(dev["kf_ids"][made], dev["created_id"][made])
    np.testing.assert_array_equal(dev["frame_ids"], np.where(made, dev["created_id"], S["cur_state"]["ln_line_id"]))
    np.testing.assert_allclose(dev["dir"], host["dir"], atol=1e-7)                            # the same kernel on the same cameras; the bar of the oracle comparison
    np.testing.assert_allclose(dev["x0"], host["x0"], rtol=1e-6, atol=1e-6)
    # and both are what the oracle makes of the same object graph (skip: the last frame holds a line the current frame holds)
    from lld_slam_amd import orb_search
    F = FS.keypoint_frame()
    vc = orb_search.frame_view(S["T_cur"], FS.CAM, F); vl = orb_search.frame_view(S["T_last"], FS.CAM, F)
    c_id = S["cur_state"]["ln_line_id"]; l_id = FS.adapter_last_ids(S)
    occ = (c_id >= 0).astype(np.uint8); skip = ((l_id >= 0) & np.isin(l_id, c_id[c_id >= 0])).astype(np.uint8)
    assert skip.sum() >= 1
    om, oc, ox, od = FS.oracle_last_kf(oracle, vc, vl, S["cur"], S["last"], R["ctor_matches"], FS.oracle_stereo(oracle, S["last"])[0], occ, skip, 1)
    np.testing.assert_array_equal(dev["match_last"], om)
    np.testing.assert_array_equal(made, oc.astype(bool))
    assert dev["ret"] == int(oc.sum() + occ.sum())
