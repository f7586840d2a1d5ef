"""lld_mappoint_refresh / lld_mapline_distinctive: the structs of include/lld_amd.h against their ctypes mirrors (a C99 program
compiled with -Werror prints sizeof and offsetof), the limits, the flag values and the exported symbols.  CPU only."""
import ctypes
import os
import subprocess

import lld_slam_amd
from lld_slam_amd import abi, landmarks
from lld_slam_amd.abi import MapLineDistinctiveIn, MapLineDistinctiveOut, MapPointRefreshIn, MapPointRefreshOut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_mappoint_refresh", "lld_mapline_distinctive"]


def test_landmark_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    assert lld_slam_amd.refresh_map_points is landmarks.refresh_map_points
    assert lld_slam_amd.distinctive_line_descriptors is landmarks.distinctive_line_descriptors


def test_landmark_struct_layouts(tmp_path):
    structs = [("lld_mappoint_refresh_in", MapPointRefreshIn), ("lld_mappoint_refresh_out", MapPointRefreshOut),
               ("lld_mapline_distinctive_in", MapLineDistinctiveIn), ("lld_mapline_distinctive_out", MapLineDistinctiveOut)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += ('printf("%d\\n%d\\n%d\\n%u\\n%u\\n", LLD_LANDMARK_MAX_OBS, LLD_LANDMARK_MAX_LINE_OBS, LLD_LANDMARK_MAX_LINE_DIM, '
             'LLD_LANDMARK_DESCRIPTOR, LLD_LANDMARK_NORMAL_DEPTH);')
    want += [landmarks.MAX_OBS, landmarks.MAX_LINE_OBS, landmarks.MAX_LINE_DIM, landmarks.DESCRIPTOR, landmarks.NORMAL_DEPTH]
    src = tmp_path / "landmark.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "landmark"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
