"""lld_frame_track_finish / lld_frame_create_stereo_points: the structs of include/lld_amd.h against their ctypes mirrors (a C99 program
compiled with -Werror prints sizeof and offsetof), the prototypes, the exported symbols and the Python entry points.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, tracking
from lld_slam_amd.abi import FrameFinishParams, FrameFinishResult, FramePointsParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_frame_track_finish", "lld_frame_create_stereo_points"]


def test_frame_finish_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    for name in ("finish", "create_stereo_points"):
        assert callable(getattr(tracking.DeviceTrackedFrame, name))
    lib = abi.product()
    assert lib.fn("frame_track_finish").restype is ctypes.c_int and len(lib.fn("frame_track_finish").argtypes) == 3
    assert lib.fn("frame_create_stereo_points").restype is ctypes.c_int and len(lib.fn("frame_create_stereo_points").argtypes) == 3


def test_frame_finish_struct_layouts(tmp_path):
    structs = [("lld_frame_finish_params", FrameFinishParams), ("lld_frame_finish_result", FrameFinishResult), ("lld_frame_points_params", FramePointsParams)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n%d\\n", LLD_POINTS_LAST_FRAME, LLD_POINTS_INITIALIZATION, LLD_ORB_MAX_KEYPOINTS);'
    want += [abi.POINTS_LAST_FRAME, abi.POINTS_INITIALIZATION, 4096]
    # the prototypes as the header declares them (unevaluated: nothing is linked)
    body += ('printf("%zu\\n", sizeof(lld_frame_track_finish((lld_frame*)0, (const lld_frame_finish_params*)0, (lld_frame_finish_result*)0)));'
             'printf("%zu\\n", sizeof(lld_frame_create_stereo_points((lld_frame*)0, (const lld_frame_points_params*)0, (lld_frame_finish_result*)0)));')
    want += [ctypes.sizeof(ctypes.c_int)] * 2
    src = tmp_path / "frame_finish.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "frame_finish"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
