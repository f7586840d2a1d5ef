"""The interface of lld_map_ba_apply, lld_map_set_point_refs and lld_map_download_rows: the structs of include/lld_amd.h against their ctypes
mirrors (a C99 program compiled with -Werror prints sizeof and offsetof), the constants, the prototypes, the exported symbols and the Python
entry points.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, device_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_map_set_point_refs", "lld_map_ba_apply", "lld_map_download_rows"]


def test_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    for name in ("set_point_refs", "ba_apply", "rows"):
        assert callable(getattr(device_map.DeviceMap, name))


def test_struct_layouts_constants_and_prototypes(tmp_path):
    structs = [("lld_map_ba_apply_in", abi.MapBaApplyIn), ("lld_map_ba_apply_out", abi.MapBaApplyOut),
               ("lld_map_limits", abi.MapLimits), ("lld_map_ba_ids", abi.MapBaIds)]               # the neighbours keep their layouts
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n%d\\n%d\\n", LLD_MAP_APPLY_WENT_BAD, LLD_MAP_APPLY_REFRESHED, LLD_MAP_APPLY_NO_REFERENCE, LLD_MAP_APPLY_INDEX_SKIPPED);'
    want += [abi.MAP_APPLY_WENT_BAD, abi.MAP_APPLY_REFRESHED, abi.MAP_APPLY_NO_REFERENCE, abi.MAP_APPLY_INDEX_SKIPPED]
    kinds = ("POINT_OBS", "POINT_IDX", "KF_POINTS", "KF_LINES", "LINE_OBS", "LINE_IDX")
    for k in kinds:
        body += f'printf("%d\\n", LLD_MAP_ROWS_{k});'
        want.append(abi.MAP_ROWS[k.lower()])
    assert sorted(abi.MAP_ROWS.values()) == list(range(6))
    # every output array has a place in the Python wrapper
    arrays = [f for f, t in abi.MapBaApplyOut._fields_ if t in (abi.c_int32_p, abi.c_float_p, abi.c_uint8_p) and f != "phase_ms"]
    assert arrays == ["tcw", "ow"] + [a[0] for a in device_map.DeviceMap.APPLY_POINT] + [a[0] for a in device_map.DeviceMap.APPLY_LINE]
    assert [f for f, t in abi.MapBaApplyOut._fields_ if t == ctypes.c_int32] == list(device_map.DeviceMap.APPLY_COUNTS)
    # the result arrays are lld_ba_result's, under the same names
    assert [f for f, _ in abi.MapBaApplyIn._fields_[6:13]] == [f for f, _ in abi.BAResult._fields_[:7]]
    i32 = "(const int32_t*)0"
    calls = [f"lld_map_set_point_refs((lld_map*)0, 0, {i32}, {i32})",
             "lld_map_ba_apply((lld_map*)0, (const lld_map_ba_apply_in*)0, (lld_map_ba_apply_out*)0)",
             f"lld_map_download_rows((lld_map*)0, LLD_MAP_ROWS_KF_POINTS, 0, {i32}, (int32_t*)0, 0, (int32_t*)0)"]
    for c in calls:
        body += f'printf("%zu\\n", sizeof({c}));'
    want += [ctypes.sizeof(ctypes.c_int)] * len(calls)
    src = tmp_path / "map_ba_apply.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "map_ba_apply"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
