"""The resident map's interface (lld_map_*, lld_frame_track_update_local_map, lld_frame_track_local_map_resident, lld_frame_local_map_download):
the structs of include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror prints sizeof and offsetof), the constants,
the prototypes, the exported symbols and the Python entry points.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, device_map, tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_map_create", "lld_map_destroy", "lld_map_clear", "lld_map_set_points", "lld_map_set_observations", "lld_map_set_keyframes", "lld_map_set_lines",
         "lld_frame_track_update_local_map", "lld_frame_track_local_map_resident", "lld_frame_local_map_download"]


def test_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    for name in ("update_local_map", "track_local_map_resident", "local_map_download"):
        assert callable(getattr(tracking.DeviceTrackedFrame, name))
    for name in ("set_points", "set_observations", "set_keyframes", "set_lines", "clear", "close"):
        assert callable(getattr(device_map.DeviceMap, name))


def test_struct_layouts_constants_and_prototypes(tmp_path):
    structs = [("lld_map_limits", abi.MapLimits), ("lld_local_map_result", abi.LocalMapResult)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n%d\\n%d\\n", LLD_LOCAL_MAP_KEYFRAME_OVERFLOW, LLD_LOCAL_MAP_POINT_OVERFLOW, LLD_LOCAL_MAP_LINE_OVERFLOW, LLD_MAP_MAX_LOCAL_KEYFRAMES);'
    want += [abi.LOCAL_MAP_KEYFRAME_OVERFLOW, abi.LOCAL_MAP_POINT_OVERFLOW, abi.LOCAL_MAP_LINE_OVERFLOW, abi.MAP_MAX_LOCAL_KEYFRAMES]
    # the prototypes as the header declares them (unevaluated: nothing is linked)
    i32, u8, f32, f64 = "(const int32_t*)0", "(const uint8_t*)0", "(const float*)0", "(const double*)0"
    calls = [f"lld_map_create((lld_ctx*)0, (const lld_map_limits*)0, (lld_map**)0)", "lld_map_clear((lld_map*)0)",
             f"lld_map_set_points((lld_map*)0, 0, {i32}, {f32}, {f32}, {f32}, {f32}, (const uint32_t*)0, {u8})",
             f"lld_map_set_observations((lld_map*)0, 0, {i32}, {i32}, {i32})",
             f"lld_map_set_keyframes((lld_map*)0, 0, {i32}, (const uint64_t*)0, {u8}, {i32}, {i32}, {i32}, {i32}, {i32}, {i32}, {i32}, {i32}, {i32})",
             f"lld_map_set_lines((lld_map*)0, 0, {i32}, {f64}, {f64}, {f64}, {f64}, {f32}, {u8})",
             "lld_frame_track_update_local_map((lld_frame*)0, (lld_map*)0)",
             "lld_frame_track_local_map_resident((lld_frame*)0, (const lld_track_params*)0, (lld_map*)0)",
             "lld_frame_local_map_download((lld_frame*)0, (lld_map*)0, (lld_local_map_result*)0)"]
    for c in calls:
        body += f'printf("%zu\\n", sizeof({c}));'
    want += [ctypes.sizeof(ctypes.c_int)] * len(calls)
    src = tmp_path / "local_map.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "local_map"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
