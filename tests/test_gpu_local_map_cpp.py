"""lld_amd::DeviceMap and TrackedFrame::UpdateLocalMap / TrackLocalMapResident / DownloadLocalMap from compiled C++ (examples/local_map_harness)
against the Python wrapper on the same scene and map: the same lists, counts, reference keyframe, both stage records bit for bit and
mp_in_view; and the harness's own host route (examples/local_map_host.cpp + TrackedFrame::TrackLocalMap) gives the same again."""
import os
import subprocess

import numpy as np
import pytest

import local_map_scenes as SC
from lld_slam_amd import abi, synth
from lld_slam_amd.device_map import DeviceMap
from lld_slam_amd.tracking import _COUNTERS, DeviceTrackedFrame, write_harness_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "local_map_harness")


class Cursor:
    def __init__(self, path):
        self.b = open(path, "rb").read(); self.at = 0

    def take(self, dtype, n):
        a = np.frombuffer(self.b, dtype, n, self.at); self.at += a.nbytes
        return a

    def record(self, nt, nl):
        d = dict(pose_qt=self.take(np.float64, 7), chi2=self.take(np.float64, 1))
        d.update(zip(_COUNTERS, self.take(np.int32, 14).tolist()))
        d.update(kp_point_id=self.take(np.int32, nt), kp_outlier=self.take(np.uint8, nt), ln_line_id=self.take(np.int32, nl), ln_outlier=self.take(np.uint8, nl))
        return d


def same_record(g, e, what):
    for k in ("pose_qt", "chi2"):
        np.testing.assert_array_equal(np.atleast_1d(np.asarray(g[k], np.float64)).view(np.uint64), np.atleast_1d(np.asarray(e[k], np.float64)).view(np.uint64), err_msg=what + k)
    for k in _COUNTERS:
        assert g[k] == e[k], (what, k, g[k], e[k])
    for k in ("kp_point_id", "kp_outlier", "ln_line_id", "ln_outlier"):
        np.testing.assert_array_equal(g[k], e[k], err_msg=what + k)


@pytest.mark.parametrize("with_lines", [True, False], ids=["lines", "no_lines"])
def test_cpp_wrapper_equals_the_python_wrapper(gpu_ctx, tmp_path, with_lines):
    assert os.path.exists(HARNESS), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    sc = SC.as_slots(synth.make_tracking_scene(12, n_kp=300, n_map=400, n_last=200, n_lines=70, n_map_lines=60, n_last_lines=30))
    stage1 = lambda tf: tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc.get("last_lines") if with_lines else None)
    lines = sc["lines"] if with_lines else None
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], lines) as tf:
        stage1(tf)
        r1 = tf.download(stage2=False)[0]
    m = SC.make_map(sc, np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]), 3)
    # without frame lines the map still holds its lines and the limit is 0 in one case: LocalMapRecord binds a list of one entry then
    L = SC.tracking_limits(sc, m, max_local_lines=64 if with_lines else 0)
    if not with_lines:
        for k in m["keyframes"].values(): k["lines"] = []
    with DeviceMap(gpu_ctx, **L) as dm, DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], lines) as tf:
        SC.upload(dm, m, SC.point_data(sc), SC.line_data(sc), dim=L["line_dim"])
        stage1(tf)
        tf.update_local_map(dm)
        tf.track_local_map_resident(dm)
        py = tf.local_map_download(dm)
    scene_file, map_file, out_file = (str(tmp_path / n) for n in ("scene.bin", "map.bin", "out.bin"))
    sc_file = dict(sc) if with_lines else {k: v for k, v in sc.items() if k not in ("lines", "last_lines", "local_lines")}
    nl = write_harness_scene(scene_file, sc_file)
    SC.write_map_file(map_file, sc, m, L)
    r = subprocess.run([HARNESS, scene_file, map_file, out_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)              # 3: its resident and host routes differ
    nt = sc["frame"].n
    c = Cursor(out_file)
    head = c.take(np.int32, 12).tolist()
    names = ("status", "n_voted", "n_local_keyframes", "n_local_points", "n_local_lines", "n_bad_cleared", "ref_keyframe", "vote_empty", "stage2_ran")
    for k, v in zip(names, head):
        assert py[k] == v, (k, py[k], v)
    assert py["status"] == 0 and py["stage2_ran"] == 1 and py["n_local_points"] > 200 and (py["n_local_lines"] > 20) == with_lines
    lists = [c.take(np.int32, head[2]), c.take(np.int32, head[3]), c.take(np.int32, head[4])]
    for got, k in zip(lists, ("local_keyframes", "local_points", "local_lines")):
        assert got.tolist() == py[k].tolist(), k
    in_view = c.take(np.uint8, L["max_local_points"])
    np.testing.assert_array_equal(in_view, py["stages"][1]["mp_in_view"])
    b1, b2, a1, a2 = (c.record(nt, nl) for _ in range(4))
    same_record(b1, py["stages"][0], "C++ resident stage 1: "); same_record(b2, py["stages"][1], "C++ resident stage 2: ")
    same_record(a1, b1, "C++ host stage 1: "); same_record(a2, b2, "C++ host stage 2: ")
    assert b2["n_search"] > 20 and b2["n_inliers"] > 20
    host_lists = [c.take(np.int32, head[9]), c.take(np.int32, head[10]), c.take(np.int32, head[11])]
    for got, e in zip(host_lists, lists):
        assert got.tolist() == e.tolist()
    np.testing.assert_array_equal(c.take(np.uint8, head[10]), in_view[:head[10]])
    assert c.at == len(c.b) and abi.MAP_MAX_LOCAL_KEYFRAMES >= head[2]


def test_adapter_leaves_the_graph_of_the_host_routine(gpu_ctx, tmp_path):
    """On object doubles, MapOnDevice + FrameOnDevice::TrackLocalMap(MapOnDevice&) leave what host UpdateLocalMap (examples/local_map_host.cpp on
    tables gathered from the objects) + the existing FrameOnDevice::TrackLocalMap leave: mvpLocalKeyFrames, mvpLocalMapPoints, local_lines and
    their descriptors' length, mpReferenceKF (Tracking's and the frame's), the frame's MapPoints, MapLines, outlier flags and pose, every
    MapPoint's mnVisible / mnFound / mnLastFrameSeen / mbTrackInView / mnTrackReferenceForFrame, every MapLine's tracked_last_id and mark, every
    keyframe's mark - once after Upload and once after UpdatePoints / UpdateKeyFrames on a changed map."""
    assert os.path.exists(HARNESS), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    sc = SC.as_slots(synth.make_tracking_scene(12, n_kp=300, n_map=400, n_last=200, n_lines=70, n_map_lines=60, n_last_lines=30))
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc["lines"]) as tf:
        tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc.get("last_lines"))
        r1 = tf.download(stage2=False)[0]
    m = SC.make_map(sc, np.where(r1["kp_outlier"] != 0, -1, r1["kp_point_id"]), 6)
    L = SC.tracking_limits(sc, m)
    scene_file, map_file, out_file = (str(tmp_path / n) for n in ("scene.bin", "map.bin", "out.bin"))
    write_harness_scene(scene_file, sc)
    SC.write_map_file(map_file, sc, m, L)
    r = subprocess.run([HARNESS, "objects", scene_file, map_file, out_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(r.stdout)
    assert r.returncode in (0, 3), (r.returncode, r.stdout, r.stderr)         # 3: the graphs differ - shown member by member below
    c = Cursor(out_file)
    head = c.take(np.int32, 5).tolist()
    assert head[0] == 4
    host1, dev1, host2, dev2 = (c.take(np.int32, n) for n in head[1:])
    assert c.at == len(c.b)
    for host, dev, what in ((host1, dev1, "after Upload"), (host2, dev2, "after UpdatePoints / UpdateKeyFrames")):
        assert host.shape == dev.shape, what
        diff = np.flatnonzero(host != dev)
        assert diff.size == 0, (what, "first differing words", diff[:10].tolist(), host[diff[:10]].tolist(), dev[diff[:10]].tolist())
        n_kf, n_pt, n_ln, ref, ref_frame, inliers = host[:6].tolist()
        assert n_kf >= 4 and n_pt > 200 and n_ln > 20 and ref >= 0 and ref_frame == ref and inliers > 20, (what, host[:6].tolist())
    # the change between the frames reached the device: 15 points turned bad and left the local map, 20 joined a keyframe
    p1 = set(host1[6 + host1[0]:6 + host1[0] + host1[1]].tolist()); p2 = set(host2[6 + host2[0]:6 + host2[0] + host2[1]].tolist())
    assert len(p1 - p2) >= 1 and r.returncode == 0
