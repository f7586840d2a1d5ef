"""The interface of covisibility on the resident map (lld_map_set_observations_indexed, lld_map_set_keyframe_keypoints, lld_map_set_covisibles,
lld_map_covisibility): the structs of include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror prints sizeof and
offsetof), the constants, the prototypes, the exported symbols and the Python entry points.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, device_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_map_set_observations_indexed", "lld_map_set_keyframe_keypoints", "lld_map_set_covisibles", "lld_map_covisibility", "lld_map_download_links"]


def test_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)
    for name in ("set_observations_indexed", "set_keyframe_keypoints", "set_covisibles", "covisibility", "links"):
        assert callable(getattr(device_map.DeviceMap, name))


def test_struct_layouts_constants_and_prototypes(tmp_path):
    structs = [("lld_map_covisibility_in", abi.MapCovisibilityIn), ("lld_map_covisibility_out", abi.MapCovisibilityOut),
               ("lld_map_limits", abi.MapLimits)]           # the limits keep their layout
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += ('printf("%d\\n%u\\n%d\\n%d\\n%u\\n%u\\n", LLD_MAP_COVIS_MAX_CONNECTED, LLD_MAP_COVIS_WRITE_COV, LLD_MAP_COVIS_CONN_OVERFLOW, '
             'LLD_MAP_COVIS_NO_KEYPOINT_DATA, LLD_COVIS_CONNECTIONS, LLD_COVIS_CULLING);')
    want += [abi.MAP_COVIS_MAX_CONNECTED, abi.MAP_COVIS_WRITE_COV, abi.MAP_COVIS_CONN_OVERFLOW, abi.MAP_COVIS_NO_KEYPOINT_DATA, 1, 2]
    assert abi.MAP_COVIS_MAX_CONNECTED >= 4096 and abi.MAP_COVIS_WRITE_COV not in (1, 2)
    assert ctypes.sizeof(abi.MapLimits) == 40
    # the prototypes as the header declares them (unevaluated: nothing is linked)
    i32, f32 = "(const int32_t*)0", "(const float*)0"
    calls = [f"lld_map_set_observations_indexed((lld_map*)0, 0, {i32}, {i32}, {i32}, {i32}, {i32})",
             f"lld_map_set_keyframe_keypoints((lld_map*)0, 0, {i32}, {i32}, {i32}, {f32}, {f32})",
             f"lld_map_set_covisibles((lld_map*)0, 0, {i32}, {i32}, {i32})",
             "lld_map_covisibility((lld_map*)0, (const lld_map_covisibility_in*)0, (lld_map_covisibility_out*)0)",
             f"lld_map_download_links((lld_map*)0, 0, {i32}, (int32_t*)0, (int32_t*)0, (int32_t*)0, (int32_t*)0, 0, (int32_t*)0)"]
    for c in calls:
        body += f'printf("%zu\\n", sizeof({c}));'
    want += [ctypes.sizeof(ctypes.c_int)] * len(calls)
    src = tmp_path / "map_covis.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "map_covis"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
