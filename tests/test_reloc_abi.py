"""lld_frame_relocalize exists in liblld_amd.so, and the ctypes mirrors of lld_reloc_candidate / lld_reloc_result have the C structs' layout."""
import ctypes as C
import os
import subprocess
import tempfile

from lld_slam_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exists():
    lib = abi.product()
    assert hasattr(lib.dll, "lld_frame_relocalize")
    assert "lld_frame_relocalize" in abi.PRODUCT_SYMBOLS


def _layout(c_name, struct):
    fields = [n for n, _ in struct._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"lld_amd.h\"\nint main(void) {\n  printf(\"%%zu\", sizeof(%s));\n" % c_name
    for f in fields:
        src += "  printf(\" %%zu\", offsetof(%s, %s));\n" % (c_name, f)
    src += "  printf(\"\\n\");\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c"); exe = os.path.join(d, "layout")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(struct), c_name
    assert got[1:] == [getattr(struct, f).offset for f in fields], c_name


def test_reloc_candidate_layout_matches_the_header():
    _layout("lld_reloc_candidate", abi.RelocCandidate)


def test_reloc_result_layout_matches_the_header():
    _layout("lld_reloc_result", abi.RelocResult)


def test_rung_bits_match_the_header():
    names = ("POSE1", "SEARCH1", "POSE2", "SEARCH2", "POSE3")
    src = "#include <stdio.h>\n#include \"lld_amd.h\"\nint main(void) {\n  printf(\"" + " ".join(["%d"] * len(names)) + "\\n\", " + \
          ", ".join("LLD_RELOC_RUNG_" + n for n in names) + ");\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "rungs.c"); exe = os.path.join(d, "rungs")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == [getattr(abi, "RELOC_RUNG_" + n) for n in names]
