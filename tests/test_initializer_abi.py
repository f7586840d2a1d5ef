"""lld_initializer_*: the structs of include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror prints
sizeof and offsetof), the limits and the exported symbols.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, initializer
from lld_slam_amd.abi import InitializerHypothesis, InitializerParams, InitializerResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_initializer_params_default", "lld_initializer_create", "lld_initializer_initialize", "lld_initializer_hypotheses",
         "lld_initializer_destroy", "lld_initializer_find"]


def test_initializer_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)


def test_initializer_struct_layouts(tmp_path):
    structs = [("lld_initializer_params", InitializerParams), ("lld_initializer_result", InitializerResult),
               ("lld_initializer_hypothesis", InitializerHypothesis)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n", LLD_INIT_MAX_KEYPOINTS, LLD_INIT_MAX_ITERATIONS);'
    want += [initializer.MAX_KEYPOINTS, initializer.MAX_ITERATIONS]
    src = tmp_path / "initializer.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "initializer"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


def test_initializer_params_default_is_tracking():
    p = InitializerParams()
    abi.product().fn("initializer_params_default")(ctypes.byref(p))
    assert (p.sigma, p.iterations, p.min_parallax, p.min_triangulated, p.seed) == (1.0, 200, 1.0, 50, 0)   # Tracking.cc:596
    assert initializer.DEFAULT_PARAMS == (1.0, 200, 1.0, 50, 0)
