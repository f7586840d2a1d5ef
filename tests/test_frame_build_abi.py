"""lld_frame_build_stereo*: the struct of include/lld_amd.h against its ctypes mirror (a C99 program compiled with -Werror prints
sizeof and offsetof), the exported symbols and the Python entry points.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, orb_extractor, orb_search, tracking
from lld_slam_amd.abi import FrameStereoParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_frame_build_stereo_keypoints", "lld_frame_build_stereo", "lld_frame_stereo_download"]


def test_frame_build_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    assert callable(orb_extractor.ORBextractor.build_stereo_frame)
    assert callable(orb_search.build_stereo_frame_keypoints)
    assert callable(tracking.DeviceTrackedFrame.from_stereo_build)


def test_frame_build_struct_layouts(tmp_path):
    structs = [("lld_frame_stereo_params", FrameStereoParams), ("lld_keypoints", orb_search.Keypoints),
               ("lld_stereo_pyramids", orb_search.StereoPyramids), ("lld_stereo_result", orb_search.StereoResult)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n", LLD_ORB_MAX_KEYPOINTS, LLD_ORB_MAX_LEVELS);'
    want += [orb_search.MAX_KEYPOINTS, orb_search.MAX_LEVELS]
    # the prototypes as the header declares them (unevaluated: nothing is linked)
    body += ('printf("%zu\\n", sizeof(lld_frame_build_stereo_keypoints((lld_ctx*)0, (const lld_keypoints*)0, (const lld_keypoints*)0,'
             ' (const lld_stereo_pyramids*)0, (const lld_frame_stereo_params*)0, (lld_frame**)0)));'
             'printf("%zu\\n", sizeof(lld_frame_build_stereo((lld_orb_extractor*)0, 0, 1, (const lld_frame_stereo_params*)0, (lld_frame**)0)));'
             'printf("%zu\\n", sizeof(lld_frame_stereo_download((lld_frame*)0, (lld_stereo_result*)0)));')
    want += [ctypes.sizeof(ctypes.c_int)] * 3
    src = tmp_path / "frame_build.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "frame_build"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
