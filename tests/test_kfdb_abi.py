"""lld_kfdb_*: the struct of include/lld_amd.h against its ctypes mirror (a C99 program compiled with -Werror prints sizeof and
offsetof) and the exported symbols.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi
from lld_slam_amd.keyframe_database import MAX_COVISIBLES, MAX_KEYFRAMES, KfdbResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_kfdb_create", "lld_kfdb_destroy", "lld_kfdb_add", "lld_kfdb_erase", "lld_kfdb_clear", "lld_kfdb_set_covisibles",
         "lld_kfdb_detect_loop_candidates", "lld_kfdb_detect_relocalization_candidates"]


def test_kfdb_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)


def test_kfdb_result_layout(tmp_path):
    fields = [f for f, _ in KfdbResult._fields_]
    body = 'printf("%zu\\n", sizeof(lld_kfdb_result));' + "".join(f'printf("%zu\\n", offsetof(lld_kfdb_result, {f}));' for f in fields)
    body += 'printf("%d\\n%d\\n", LLD_KFDB_MAX_KEYFRAMES, LLD_KFDB_MAX_COVISIBLES);'
    src = tmp_path / "kf.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "kf"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(KfdbResult)] + [getattr(KfdbResult, f).offset for f in fields] + [MAX_KEYFRAMES, MAX_COVISIBLES]
