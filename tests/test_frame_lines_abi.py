"""lld_frame_build_lines / lld_frame_lines_download / lld_frame_new_map_lines: the structs of include/lld_amd.h against their ctypes mirrors
(a C99 program compiled with -Werror prints sizeof and offsetof), the prototypes, the exported symbols and the Python entry points.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, tracking
from lld_slam_amd.abi import FrameLinesBuild, FrameNewLinesParams, FrameNewLinesResult, LineStereoParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_frame_build_lines", "lld_frame_lines_download", "lld_frame_new_map_lines"]


def test_frame_lines_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    for name in ("lines_download", "new_map_lines", "_build_lines"):
        assert callable(getattr(tracking.DeviceTrackedFrame, name))


def test_frame_lines_struct_layouts(tmp_path):
    structs = [("lld_frame_lines_build", FrameLinesBuild), ("lld_frame_new_lines_params", FrameNewLinesParams),
               ("lld_frame_new_lines_result", FrameNewLinesResult), ("lld_line_stereo_params", LineStereoParams), ("lld_frame_lines", tracking.FrameLines)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n", LLD_LINE_DIM_MAX, LLD_LINE_LDS_CEILING);'
    want += [128, 150 * 1024]
    # the prototypes as the header declares them (unevaluated: nothing is linked)
    body += ('printf("%zu\\n", sizeof(lld_frame_build_lines((lld_frame*)0, (const lld_frame_lines_build*)0)));'
             'printf("%zu\\n", sizeof(lld_frame_lines_download((lld_frame*)0, (int32_t*)0, (double*)0)));'
             'printf("%zu\\n", sizeof(lld_frame_new_map_lines((lld_frame*)0, (lld_frame*)0, (const lld_frame_new_lines_params*)0, (lld_frame_new_lines_result*)0)));')
    want += [ctypes.sizeof(ctypes.c_int)] * 3
    src = tmp_path / "frame_lines.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "frame_lines"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


def test_frame_lines_scenes_are_what_the_gpu_tests_need(oracle):
    """The conditions the GPU tests rest on, held on the CPU oracle's own results: the wide-baseline stereo scenes match at least a fifth of
    their left lines with more than one gated candidate in at least half the rows, and the two-frame scenes create at least 3 lines with at
    least one occupied line and one skipped one."""
    import numpy as np
    import frame_lines_scenes as FS
    from lld_slam_amd import orb_search
    for seed in (0, 1, 2, 3):
        m, _, g = FS.oracle_stereo(oracle, FS.wide_stereo_scene(seed))
        assert (m >= 0).sum() * 5 >= m.size and (g.sum(1) > 1).sum() * 2 >= m.size
    F = FS.keypoint_frame()
    for seed in (0, 3, 5):
        S = FS.last_kf_scene(seed)
        vc = orb_search.frame_view(S["T_cur"], FS.CAM, F); vl = orb_search.frame_view(S["T_last"], FS.CAM, F)
        occ, skip = FS.host_flags(S["cur_state"], S["last_state"])
        lm_c = FS.oracle_stereo(oracle, S["cur"])[0]; lm_l = FS.oracle_stereo(oracle, S["last"])[0]
        for use_grid in (0, 1):
            o = FS.oracle_last_kf(oracle, vc, vl, S["cur"], S["last"], lm_c, lm_l, occ, skip, use_grid)
            assert o[1].sum() >= 3 and occ.sum() >= 1 and skip.sum() >= 1
