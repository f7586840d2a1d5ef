"""lld_frame_build_mono*: the structs of include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror prints
sizeof and offsetof), the exported symbols, the Python entry points, and lld_frame_image_bounds (host only) against the numpy
restatement.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np

import frame_mono_ref as M
from lld_slam_amd import abi, orb_extractor, orb_search, tracking
from lld_slam_amd.abi import DepthImage, FrameMonoParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_frame_build_mono_keypoints", "lld_frame_build_mono", "lld_frame_keypoints_download", "lld_frame_image_bounds"]


def test_frame_mono_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    assert callable(orb_extractor.ORBextractor.build_mono_frame)
    assert callable(orb_search.build_mono_frame_keypoints)
    assert callable(orb_search.MonoBuiltFrame.download)
    assert callable(tracking.DeviceTrackedFrame.from_built)
    assert callable(tracking.DeviceTrackedFrame.from_stereo_build)


def test_frame_mono_struct_layouts(tmp_path):
    structs = [("lld_frame_mono_params", FrameMonoParams), ("lld_depth_image", DepthImage), ("lld_keypoints", orb_search.Keypoints)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n%d\\n%d\\n", LLD_ORB_MAX_KEYPOINTS, LLD_ORB_MAX_LEVELS, LLD_DEPTH_F32, LLD_DEPTH_U16);'
    want += [orb_search.MAX_KEYPOINTS, orb_search.MAX_LEVELS, abi.DEPTH_F32, abi.DEPTH_U16]
    # the prototypes as the header declares them (unevaluated: nothing is linked)
    body += ('printf("%zu\\n", sizeof(lld_frame_build_mono_keypoints((lld_ctx*)0, (const lld_keypoints*)0, (const lld_depth_image*)0,'
             ' (const lld_frame_mono_params*)0, (lld_frame**)0)));'
             'printf("%zu\\n", sizeof(lld_frame_build_mono((lld_orb_extractor*)0, 0, (const lld_depth_image*)0, (const lld_frame_mono_params*)0, (lld_frame**)0)));'
             'printf("%zu\\n", sizeof(lld_frame_keypoints_download((lld_frame*)0, (float*)0, (float*)0, (float*)0)));'
             'printf("%zu\\n", sizeof(lld_frame_image_bounds(1, 1, 1.f, 1.f, 0.f, 0.f, (const float*)0, 4, (float*)0)));')
    want += [ctypes.sizeof(ctypes.c_int)] * 4
    src = tmp_path / "frame_mono.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "frame_mono"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


def test_image_bounds_against_the_restatement():
    lib = abi.product()
    cams = [(M.CAM, M.W, M.H), ((517.306408, 516.469215, 318.643040, 255.313989), 640, 480), ((458.654, 457.296, 367.215, 248.375), 752, 480)]
    dists = [M.DIST5, M.DIST5[:4], (0.262383, -0.953104, -0.005358, 0.002628, 1.163314), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)]
    n = 0
    for cam, w, h in cams:
        for dist in dists:
            exp = M.image_bounds(w, h, cam, dist)
            if not np.all(np.isfinite(exp)):
                continue
            got = orb_search.image_bounds(lib, w, h, cam, dist)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (cam, dist, got, exp)
            n += 1
    assert n >= 6
    b = orb_search.image_bounds(lib, M.W, M.H, M.CAM, M.DIST5)
    assert b[0] != 0 and b[1] != M.W                                           # the distorted camera does move the corners


def test_image_bounds_without_distortion_and_refusals():
    lib = abi.product()
    for dist in ((0, 0, 0, 0), (0, 0, 0, 0, 0), (0.0, -0.9, 0.01, 0.002, 1.1), (0.0, 0.5, 0.01, 0.002)):
        assert np.array_equal(orb_search.image_bounds(lib, M.W, M.H, M.CAM, dist), np.float32([0, M.W, 0, M.H]))
    INV = abi.LLD_ERR_INVALID
    raw = orb_search.image_bounds_raw
    assert raw(lib, 0, M.H, M.CAM, M.DIST5)[0] == INV and raw(lib, M.W, -1, M.CAM, M.DIST5)[0] == INV
    for cam in ((0.0, 335.7, 207.1, 127.6), (336.25, -1.0, 207.1, 127.6), (float("nan"), 335.7, 207.1, 127.6), (336.25, float("inf"), 207.1, 127.6),
                (336.25, 335.7, float("nan"), 127.6)):
        assert raw(lib, M.W, M.H, cam, M.DIST5)[0] == INV, cam
    for nd in (0, 3, 6, -1):
        assert raw(lib, M.W, M.H, M.CAM, M.DIST5, n_dist=nd)[0] == INV, nd
    assert raw(lib, M.W, M.H, M.CAM, (0.2, float("nan"), 0, 0))[0] == INV and raw(lib, M.W, M.H, M.CAM, (0.2, 0, 0, 0, float("inf")))[0] == INV
    assert raw(lib, M.W, M.H, M.CAM, None, n_dist=4)[0] == INV
    fn = lib.fn("frame_image_bounds")
    d = np.float32(M.DIST5)
    assert fn(M.W, M.H, *[float(np.float32(c)) for c in M.CAM], d.ctypes.data_as(abi.c_float_p), 5, None) == INV
    assert raw(lib, M.W, M.H, M.CAM, M.DIST5)[0] == abi.LLD_OK                # after the refusals, a valid call succeeds
