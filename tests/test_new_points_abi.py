"""lld_new_points_triangulate: the structs of include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror
prints sizeof and offsetof), the limits, the status and source constants and the exported symbol.  CPU only."""
import ctypes
import os
import subprocess

import lld_slam_amd
from lld_slam_amd import abi, new_points
from lld_slam_amd.abi import NewPointsIn, NewPointsKf, NewPointsOut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS = ["NEW", "LOW_PARALLAX", "W_ZERO", "Z1", "Z2", "REPROJ1", "REPROJ2", "DIST_ZERO", "SCALE", "NO_DEPTH", "PAIR_SKIPPED"]
SOURCE = ["SRC_TRIANGULATED", "SRC_STEREO1", "SRC_STEREO2"]


def test_new_points_symbol_is_listed_and_exported():
    assert "lld_new_points_triangulate" in abi.PRODUCT_SYMBOLS
    dll = ctypes.CDLL(abi.product_library_path())
    assert hasattr(dll, "lld_new_points_triangulate")
    assert lld_slam_amd.triangulate_new_points is new_points.triangulate_new_points
    assert lld_slam_amd.NewPointsError is new_points.NewPointsError


def test_new_points_struct_layouts_and_constants(tmp_path):
    structs = [("lld_new_points_kf", NewPointsKf), ("lld_new_points_in", NewPointsIn), ("lld_new_points_out", NewPointsOut)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    for name in ["MAX_PAIRS", "MAX_MATCHES"] + STATUS + SOURCE:
        body += f'printf("%d\\n", LLD_NEWPTS_{name});'
        want.append(getattr(new_points, name))
    body += 'printf("%d\\n", LLD_ORB_MAX_LEVELS);'
    want.append(new_points.MAX_LEVELS)
    src = tmp_path / "newpts.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "newpts"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
    assert [getattr(new_points, n) for n in STATUS] == list(range(11)) and [getattr(new_points, n) for n in SOURCE] == [0, 1, 2]
    assert new_points.MAX_PAIRS == 64 and new_points.MAX_MATCHES == 65536
