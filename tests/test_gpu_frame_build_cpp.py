"""The C++ route to the device-built stereo Frame: examples/frame_build_harness extracts the 416x240 pair with lld_amd::ORBextractor,
builds the frame with lld_amd::StereoFrame and runs the Tracking chain on it.  Its printed mvuRight / mvDepth / n_matches and the
two poses must equal, bit for bit, what the Python route (ORBextractor.build_stereo_frame + DeviceTrackedFrame.from_stereo_build)
gives on the same scene file's contents."""
import os
import subprocess

import numpy as np
import pytest

from lld_slam_amd import orb_search
from lld_slam_amd.orb_extractor import ORBextractor
from lld_slam_amd.tracking import DeviceTrackedFrame
from test_gpu_frame_build import H, PATTERN, SMALL, W, _queries, small  # noqa: F401  (the module's scene fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "frame_build_harness")


def write_scene(path, sc, cam, view, T, last, mp, ids, repeats=0):
    f32 = lambda a: np.ascontiguousarray(a, np.float32); i32 = lambda a: np.ascontiguousarray(a, np.int32); u8 = lambda a: np.ascontiguousarray(a, np.uint8)
    with open(path, "wb") as f:
        i32([W, H, SMALL[0], SMALL[2], SMALL[3], SMALL[4], len(ids), len(ids), repeats, 0, 0, 0]).tofile(f)
        f32([SMALL[1], sc["mb"], sc["mbf"]]).tofile(f)
        i32(PATTERN).reshape(1024).tofile(f)
        u8(sc["left"][0]).tofile(f); u8(sc["right"][0]).tofile(f)
        np.array([float(np.float32(c)) for c in cam] + [0.5], np.float64).tofile(f)
        f.write(bytes(view)); f32(T).tofile(f)
        f32(last["world_pos"]).tofile(f); u8(last["valid"]).tofile(f); i32(last["octave"]).tofile(f); f32(last["angle"]).tofile(f)
        np.ascontiguousarray(last["desc"], np.uint32).tofile(f); u8(last["has_obs"]).tofile(f); i32(ids).tofile(f)
        f32(mp["world_pos"]).tofile(f); f32(mp["normal"]).tofile(f); f32(mp["max_distance"]).tofile(f); f32(mp["min_distance"]).tofile(f)
        np.ascontiguousarray(mp["desc"], np.uint32).tofile(f); u8(mp["has_obs"]).tofile(f); u8(mp["skip"]).tofile(f); i32(ids).tofile(f)


def test_harness_equals_python_route(gpu_ctx, small, tmp_path):  # noqa: F811
    assert os.path.exists(HARNESS), "examples/frame_build_harness is built by build()"
    s = small[0]; sc = s["sc"]
    fx = float(np.float32(sc["mbf"]) / np.float32(sc["mb"]))
    cam = (fx, fx, W / 2.0, H / 2.0, float(sc["mbf"]))
    n_exp, ur_exp, dep_exp = s["exp"][0], s["exp"][1], s["exp"][2]
    last, mp, ids = _queries(s["L"], ur_exp, dep_exp, cam, np.random.default_rng(9))
    T = np.eye(4, dtype=np.float32); T[:3, 3] = [0.03, -0.01, 0.02]
    view = orb_search.frame_view(T, cam, s["L"])
    path = tmp_path / "scene.bin"
    write_scene(path, sc, cam, view, T, last, mp, ids)
    out = subprocess.run([HARNESS, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l.split() for l in out.stdout.strip("\n").split("\n")]

    with ORBextractor(gpu_ctx, *SMALL, PATTERN, max_cols=W, max_rows=H, max_images=2) as ex:
        L, _ = ex([sc["left"][0], sc["right"][0]])
        built = ex.build_stereo_frame(L, sc["mb"], sc["mbf"])
        st = built.download()
        with DeviceTrackedFrame.from_stereo_build(gpu_ctx, built, cam) as tf:
            tf.track_with_motion_model(T, last, ids)
            tf.track_local_map(mp, ids)
            recs = tf.download()
    assert lines[0] == ["N", str(L.n), str(st.n_matches)] and st.n_matches == n_exp > 100
    S = [l for l in lines if l[0] == "S"]
    assert [int(l[1]) for l in S] == list(range(L.n))
    assert np.array_equal(np.array([int(l[2], 16) for l in S], np.uint32), st.u_right.view(np.uint32))
    assert np.array_equal(np.array([int(l[3], 16) for l in S], np.uint32), st.depth.view(np.uint32))
    P = [l for l in lines if l[0] == "P"]
    assert len(P) == 2
    for l, r in zip(P, recs):
        assert np.array_equal(np.array([int(x, 16) for x in l[2:9]], np.uint64), np.ascontiguousarray(r["pose_qt"]).view(np.uint64)), f"pose of stage {l[1]}"
        assert [int(x) for x in l[9:12]] == [r["n_inliers"], r["n_search"], r["n_points"]]
    assert recs[1]["n_inliers"] > 20
