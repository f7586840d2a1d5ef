"""The interface of lld_map_refresh_points / _lines, the two descriptor setters and the two fixed-row downloads: the structs of
include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror prints sizeof and offsetof), the constants, the
prototypes, the exported symbols and the Python entry points.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, device_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_map_set_keyframe_descriptors", "lld_map_set_keyframe_line_descriptors", "lld_map_refresh_points", "lld_map_refresh_lines",
         "lld_map_download_points", "lld_map_download_lines"]


def test_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    for name in ("set_keyframe_descriptors", "set_keyframe_line_descriptors", "refresh_points", "refresh_lines", "download_points", "download_lines"):
        assert callable(getattr(device_map.DeviceMap, name))


def test_struct_layouts_constants_and_prototypes(tmp_path):
    structs = [("lld_map_refresh_points_in", abi.MapRefreshPointsIn), ("lld_map_refresh_points_out", abi.MapRefreshPointsOut),
               ("lld_map_refresh_lines_in", abi.MapRefreshLinesIn), ("lld_map_refresh_lines_out", abi.MapRefreshLinesOut),
               ("lld_map_limits", abi.MapLimits), ("lld_map_ba_apply_out", abi.MapBaApplyOut)]       # the neighbours keep their layouts
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += ('printf("%d\\n%d\\n%d\\n%d\\n%d\\n%d\\n%d\\n%d\\n", (int)LLD_LANDMARK_DESCRIPTOR, (int)LLD_LANDMARK_NORMAL_DEPTH, LLD_MAP_REFRESH_NO_INDEX, '
             'LLD_MAP_REFRESH_NO_DESCRIPTOR, LLD_MAP_REFRESH_NO_REFERENCE, LLD_LANDMARK_MAX_OBS, LLD_LANDMARK_MAX_LINE_OBS, LLD_ORB_MAX_LEVELS);')
    want += [abi.LANDMARK_DESCRIPTOR, abi.LANDMARK_NORMAL_DEPTH, abi.MAP_REFRESH_NO_INDEX, abi.MAP_REFRESH_NO_DESCRIPTOR, abi.MAP_REFRESH_NO_REFERENCE,
             abi.LANDMARK_MAX_OBS, abi.LANDMARK_MAX_LINE_OBS, abi.ORB_MAX_LEVELS]
    # the five bits of an updated byte are distinct
    bits = [abi.LANDMARK_DESCRIPTOR, abi.LANDMARK_NORMAL_DEPTH, abi.MAP_REFRESH_NO_INDEX, abi.MAP_REFRESH_NO_DESCRIPTOR, abi.MAP_REFRESH_NO_REFERENCE]
    assert sum(bits) == 31 and all(b & (b - 1) == 0 for b in bits)
    # every output array has a place in the Python wrapper
    assert [f for f, _ in abi.MapRefreshPointsOut._fields_ if f != "phase_ms"] == [a[0] for a in device_map.DeviceMap.REFRESH_POINT]
    assert [f for f, _ in abi.MapRefreshLinesOut._fields_ if f != "phase_ms"] == [a[0] for a in device_map.DeviceMap.REFRESH_LINE]
    i32, f32p = "(const int32_t*)0", "(float*)0"
    calls = [f"lld_map_set_keyframe_descriptors((lld_map*)0, 0, {i32}, {i32}, (const uint32_t*)0)",
             f"lld_map_set_keyframe_line_descriptors((lld_map*)0, 0, {i32}, {i32}, (const float*)0)",
             "lld_map_refresh_points((lld_map*)0, (const lld_map_refresh_points_in*)0, (lld_map_refresh_points_out*)0)",
             "lld_map_refresh_lines((lld_map*)0, (const lld_map_refresh_lines_in*)0, (lld_map_refresh_lines_out*)0)",
             f"lld_map_download_points((lld_map*)0, 0, {i32}, {f32p}, {f32p}, {f32p}, {f32p}, (uint32_t*)0, (uint8_t*)0)",
             f"lld_map_download_lines((lld_map*)0, 0, {i32}, {f32p}, (uint8_t*)0)"]
    for c in calls:
        body += f'printf("%zu\\n", sizeof({c}));'
    want += [ctypes.sizeof(ctypes.c_int)] * len(calls)
    src = tmp_path / "map_refresh.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "map_refresh"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


def test_null_handles_are_refused_without_a_device():
    dll = ctypes.CDLL(abi.product_library_path())
    for n in NAMES:
        getattr(dll, n).restype = ctypes.c_int
    a, o = abi.MapRefreshPointsIn(), abi.MapRefreshPointsOut()
    assert dll.lld_map_refresh_points(None, ctypes.byref(a), ctypes.byref(o)) == abi.LLD_ERR_INVALID
    assert dll.lld_map_refresh_lines(None, None, None) == abi.LLD_ERR_INVALID
    assert dll.lld_map_set_keyframe_descriptors(None, 0, None, None, None) == abi.LLD_ERR_INVALID
    assert dll.lld_map_set_keyframe_line_descriptors(None, 0, None, None, None) == abi.LLD_ERR_INVALID
    assert dll.lld_map_download_points(None, 0, None, None, None, None, None, None, None) == abi.LLD_ERR_INVALID
    assert dll.lld_map_download_lines(None, 0, None, None, None) == abi.LLD_ERR_INVALID
