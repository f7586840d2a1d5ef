"""The TrackReferenceKeyFrame entry of the chain exists in liblld_amd.so, and the ctypes mirror of lld_ref_keyframe has the C struct's layout."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

from lld_slam_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lld_frame_compute_bow", "lld_frame_track_reference_keyframe", "lld_frame_track_local_map")


def test_symbols_exist():
    lib = abi.product()
    for s in SYMBOLS:
        assert hasattr(lib.dll, s), s
        assert s in abi.PRODUCT_SYMBOLS, s


def test_ref_keyframe_layout_matches_the_header():
    fields = [n for n, _ in abi.RefKeyFrame._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"lld_amd.h\"\nint main(void) {\n  printf(\"%zu\", sizeof(lld_ref_keyframe));\n"
    for f in fields:
        src += "  printf(\" %%zu\", offsetof(lld_ref_keyframe, %s));\n" % f
    src += "  printf(\" %zu\\n\", sizeof(lld_track_params));\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c"); exe = os.path.join(d, "layout")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(abi.RefKeyFrame)
    assert got[1:-1] == [getattr(abi.RefKeyFrame, f).offset for f in fields]
    from lld_slam_amd.tracking import TrackParams
    assert got[-1] == C.sizeof(TrackParams)                                      # lld_track_params kept its size
