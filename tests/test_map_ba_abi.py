"""The interface of the local BA window on the resident map (lld_map_set_keyframe_features, lld_map_set_keyframe_poses,
lld_map_set_line_observations, lld_map_ba_window, lld_map_local_ba): the structs of include/lld_amd.h against their ctypes mirrors (a C99
program compiled with -Werror prints sizeof and offsetof), the constants, the prototypes, the exported symbols and the Python entry points.
CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, device_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_map_set_keyframe_features", "lld_map_set_keyframe_poses", "lld_map_set_line_observations", "lld_map_ba_window", "lld_map_local_ba"]


def test_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    for name in ("set_keyframe_features", "set_keyframe_poses", "set_line_observations", "ba_window", "local_ba"):
        assert callable(getattr(device_map.DeviceMap, name))


def test_struct_layouts_constants_and_prototypes(tmp_path):
    structs = [("lld_map_ba_in", abi.MapBaIn), ("lld_map_ba_window_out", abi.MapBaWindowOut), ("lld_map_ba_ids", abi.MapBaIds),
               ("lld_map_limits", abi.MapLimits), ("lld_ba_window", abi.BAWindow)]          # the limits and the window keep their layouts
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n", LLD_MAP_BA_MAX_LOCAL, LLD_MAP_BA_NO_FEATURE_DATA);'
    want += [abi.MAP_BA_MAX_LOCAL, abi.MAP_BA_NO_FEATURE_DATA]
    assert abi.MAP_BA_MAX_LOCAL == 1024 and abi.MAP_BA_NO_FEATURE_DATA != 0
    assert ctypes.sizeof(abi.MapLimits) == 40
    # every array of the window has a capacity, a count and a place in the Python wrapper
    arrays = [f for f, t in abi.MapBaWindowOut._fields_ if t in (abi.c_int32_p, abi.c_double_p)]
    assert arrays == [a[0] for a in device_map.DeviceMap.BA_ARRAYS]
    # the prototypes as the header declares them (unevaluated: nothing is linked)
    i32, f32 = "(const int32_t*)0", "(const float*)0"
    calls = [f"lld_map_set_keyframe_features((lld_map*)0, 0, {i32}, (const uint64_t*)0, {f32}, {i32}, {f32}, {i32}, {f32}, {f32}, {i32})",
             f"lld_map_set_keyframe_poses((lld_map*)0, 0, {i32}, {f32})",
             f"lld_map_set_line_observations((lld_map*)0, 0, {i32}, {i32}, {i32}, {i32}, {i32})",
             "lld_map_ba_window((lld_map*)0, (const lld_map_ba_in*)0, (lld_map_ba_window_out*)0)",
             "lld_map_local_ba((lld_map*)0, (const lld_map_ba_in*)0, (const lld_ba_params*)0, (volatile const unsigned char*)0, (lld_ba_result*)0, (lld_map_ba_ids*)0)"]
    for c in calls:
        body += f'printf("%zu\\n", sizeof({c}));'
    want += [ctypes.sizeof(ctypes.c_int)] * len(calls)
    src = tmp_path / "map_ba.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "map_ba"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
