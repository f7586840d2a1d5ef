"""lld_covisibility: the structs of include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror prints
sizeof and offsetof), the defines, the default parameters and the exported symbols.  CPU only."""
import ctypes
import os
import subprocess

import lld_slam_amd
from lld_slam_amd import abi, covisibility
from lld_slam_amd.abi import CovisibilityIn, CovisibilityOut, CovisibilityParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_covisibility_params_default", "lld_covisibility"]


def test_covisibility_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    assert lld_slam_amd.update_connections is covisibility.update_connections
    assert lld_slam_amd.keyframe_culling is covisibility.keyframe_culling
    assert lld_slam_amd.CovisibilityError is covisibility.CovisibilityError


def test_covisibility_default_params():
    dll = ctypes.CDLL(abi.product_library_path())
    p = CovisibilityParams()
    dll.lld_covisibility_params_default.argtypes = [ctypes.POINTER(CovisibilityParams)]
    dll.lld_covisibility_params_default.restype = None
    dll.lld_covisibility_params_default(ctypes.byref(p))
    assert (p.th, p.th_obs, p.redundant_ratio) == (15, 3, 0.9)


def test_covisibility_struct_layouts(tmp_path):
    structs = [("lld_covisibility_params", CovisibilityParams), ("lld_covisibility_in", CovisibilityIn),
               ("lld_covisibility_out", CovisibilityOut)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%u\\n%u\\n", LLD_COVIS_MAX_KF, LLD_COVIS_CONNECTIONS, LLD_COVIS_CULLING);'
    want += [covisibility.MAX_KF, covisibility.CONNECTIONS, covisibility.CULLING]
    src = tmp_path / "covisibility.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "covisibility"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
