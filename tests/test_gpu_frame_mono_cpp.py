"""The C++ route to the device-built RGB-D / monocular Frame: examples/frame_mono_harness extracts the 416x240 grey image with
lld_amd::ORBextractor, builds the frame with lld_amd::MonoFrame and runs the Tracking chain on it.  Its printed image bounds, mvKeysUn /
mvuRight / mvDepth and the two poses must equal, bit for bit, the numpy restatement and what the Python route
(ORBextractor.build_mono_frame + DeviceTrackedFrame.from_built) gives on the same scene file's contents."""
import os
import subprocess

import numpy as np
import pytest

import frame_mono_ref as M
from lld_slam_amd import abi, orb_search
from lld_slam_amd.orb_extractor import ORBextractor
from lld_slam_amd.tracking import DeviceTrackedFrame
from test_gpu_frame_mono import CAM, CAM5, DIST5, H, MBF, PATTERN, SMALL, W, _queries, bits, frame_of, scene  # noqa: F401  (the module's scene fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "frame_mono_harness")
TH_MOTION, TH_LOCAL = 15.0, 3.0


def write_scene(path, grey, depth, factor, dist, view, T, last, mp, ids, monocular=0):
    f32 = lambda a: np.ascontiguousarray(a, np.float32); i32 = lambda a: np.ascontiguousarray(a, np.int32); u8 = lambda a: np.ascontiguousarray(a, np.uint8)
    d_type = -1 if depth is None else (abi.DEPTH_F32 if depth.dtype == np.float32 else abi.DEPTH_U16)
    d_cols, d_rows = (0, 0) if depth is None else (depth.shape[1], depth.shape[0])
    d5 = list(dist) + [0.0] * (5 - len(dist))
    with open(path, "wb") as f:
        i32([W, H, SMALL[0], SMALL[2], SMALL[3], SMALL[4], len(ids), len(ids), len(dist), d_type, d_cols, d_rows, monocular, 0, 0, 0]).tofile(f)
        f32([SMALL[1], MBF, factor] + list(CAM) + d5 + [TH_MOTION, TH_LOCAL, 0, 0]).tofile(f)
        i32(PATTERN).reshape(1024).tofile(f)
        u8(grey).tofile(f)
        if depth is not None:
            np.ascontiguousarray(depth).tofile(f)
        np.array([float(np.float32(c)) for c in CAM5] + [0.5], np.float64).tofile(f)
        f.write(bytes(view)); f32(T).tofile(f)
        f32(last["world_pos"]).tofile(f); u8(last["valid"]).tofile(f); i32(last["octave"]).tofile(f); f32(last["angle"]).tofile(f)
        np.ascontiguousarray(last["desc"], np.uint32).tofile(f); u8(last["has_obs"]).tofile(f); i32(ids).tofile(f)
        f32(mp["world_pos"]).tofile(f); f32(mp["normal"]).tofile(f); f32(mp["max_distance"]).tofile(f); f32(mp["min_distance"]).tofile(f)
        np.ascontiguousarray(mp["desc"], np.uint32).tofile(f); u8(mp["has_obs"]).tofile(f); u8(mp["skip"]).tofile(f); i32(ids).tofile(f)


def test_harness_equals_python_route(gpu_ctx, scene, tmp_path):  # noqa: F811
    assert os.path.exists(HARNESS), "examples/frame_mono_harness is built by build()"
    depth, factor = scene["raw16"], 1.0 / 5000.0
    e = scene["e"]
    exp = M.build(e["xy"], CAM, DIST5, MBF, depth, factor)                      # the CPU extraction's keypoints through the restatement
    b = M.image_bounds(W, H, CAM, DIST5)
    Fh = frame_of(e)
    Fh.xy = exp["xy_un"].copy(); Fh.min_x, Fh.max_x, Fh.min_y, Fh.max_y = [float(x) for x in b]
    st_exp = orb_search.MonoKeypoints(exp["xy_un"], exp["u_right"], exp["depth"])
    last, mp, ids = _queries(Fh, st_exp, np.random.default_rng(9))
    T = np.eye(4, dtype=np.float32); T[:3, 3] = [0.01, -0.004, 0.008]
    view = orb_search.frame_view(T, CAM5, Fh)
    path = tmp_path / "scene.bin"
    write_scene(path, scene["grey"], depth, factor, DIST5, view, T, last, mp, ids)
    out = subprocess.run([HARNESS, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l.split() for l in out.stdout.strip("\n").split("\n")]

    with ORBextractor(gpu_ctx, *SMALL, PATTERN, max_cols=W, max_rows=H, max_images=1) as ex:
        L = ex(scene["grey"])
        built = ex.build_mono_frame(L, CAM, DIST5, MBF, depth=depth, depth_factor=factor)
        st = built.download()
        with DeviceTrackedFrame.from_built(gpu_ctx, built, CAM5, th_motion=TH_MOTION, th_local=TH_LOCAL) as tf:
            tf.track_with_motion_model(T, last, ids)
            tf.track_local_map(mp, ids)
            recs = tf.download()
    assert lines[0] == ["N", str(L.n)] and L.n == len(e["octave"]) > 400
    assert lines[1][0] == "B" and np.array_equal(np.array([int(x, 16) for x in lines[1][1:]], np.uint32), b.view(np.uint32))
    K = [l for l in lines if l[0] == "K"]
    assert [int(l[1]) for l in K] == list(range(L.n))
    got = np.array([[int(x, 16) for x in l[2:6]] for l in K], np.uint32)
    for name, want in (("restatement", st_exp), ("Python route", st)):
        assert np.array_equal(got[:, 0:2], bits(want.xy_un)), name
        assert np.array_equal(got[:, 2], bits(want.u_right)) and np.array_equal(got[:, 3], bits(want.depth)), name
    assert (st.depth > 0).sum() > 300
    P = [l for l in lines if l[0] == "P"]
    assert len(P) == 2
    for l, r in zip(P, recs):
        assert np.array_equal(np.array([int(x, 16) for x in l[2:9]], np.uint64), np.ascontiguousarray(r["pose_qt"]).view(np.uint64)), f"pose of stage {l[1]}"
        assert [int(x) for x in l[9:12]] == [r["n_inliers"], r["n_search"], r["n_points"]]
    assert recs[0]["n_search"] > 50 and recs[1]["n_inliers"] > 20
