"""lld_map_*: the map as flat tables resident in HBM (include/lld_amd.h, "the resident map").  DeviceMap owns the handle; the frame chain's
DeviceTrackedFrame.update_local_map / track_local_map_resident (tracking.py) run Tracking::UpdateLocalMap and stage 2 on it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .abi import c_double_p, c_float_p, c_int32_p, c_uint8_p, c_uint32_p

c_uint64_p = C.POINTER(C.c_uint64)


def csr(rows, dtype=np.int32):
    """(start [n+1], flat) of a list of lists."""
    start = np.zeros(len(rows) + 1, np.int32)
    for i, r in enumerate(rows):
        start[i + 1] = start[i] + len(r)
    flat = np.array([v for r in rows for v in r], dtype) if start[-1] else np.zeros(0, dtype)
    return start, flat


class DeviceMap:
    """limits: the fields of lld_map_limits as keywords (max_keyframes, max_points, max_lines, line_dim, max_observations, max_kf_points,
    max_kf_lines, max_children, max_local_points, max_local_lines)."""

    def __init__(self, ctx, **limits):
        self.ctx, self.lib = ctx, ctx.lib
        self.limits = abi.MapLimits(**{k: int(v) for k, v in limits.items()})
        f = self.lib.fn
        f("map_create").argtypes = [C.c_void_p, C.POINTER(abi.MapLimits), C.POINTER(C.c_void_p)]; f("map_create").restype = C.c_int
        f("map_destroy").argtypes = [C.c_void_p]; f("map_destroy").restype = None
        f("map_clear").argtypes = [C.c_void_p]; f("map_clear").restype = C.c_int
        f("map_set_points").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_float_p, c_float_p, c_float_p, c_float_p, c_uint32_p, c_uint8_p]
        f("map_set_points").restype = C.c_int
        f("map_set_observations").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p]; f("map_set_observations").restype = C.c_int
        f("map_set_keyframes").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_uint64_p, c_uint8_p, c_int32_p] + [c_int32_p] * 8
        f("map_set_keyframes").restype = C.c_int
        f("map_set_lines").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p, c_float_p, c_uint8_p]
        f("map_set_lines").restype = C.c_int
        h = C.c_void_p()
        self.handle = None
        self._check(f("map_create")(ctx.handle, C.byref(self.limits), C.byref(h)), "lld_map_create")
        self.handle = h

    def _check(self, st, what):
        if st != abi.LLD_OK:
            err = RuntimeError(f"{what} failed: {self.lib.fn('status_string')(st).decode()}")
            err.status = st
            raise err

    def close(self):
        if self.handle is not None:
            self.lib.fn("map_destroy")(self.handle); self.handle = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def clear(self):
        self._check(self.lib.fn("map_clear")(self.handle), "lld_map_clear")

    @staticmethod
    def _p(a, dtype, ptr):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype)
        return a, a.ctypes.data_as(ptr)

    def set_points(self, slot, world_pos, normal, min_distance, max_distance, desc, bad):
        k = [self._p(slot, np.int32, c_int32_p), self._p(world_pos, np.float32, c_float_p), self._p(normal, np.float32, c_float_p),
             self._p(min_distance, np.float32, c_float_p), self._p(max_distance, np.float32, c_float_p), self._p(desc, np.uint32, c_uint32_p),
             self._p(bad, np.uint8, c_uint8_p)]
        self._check(self.lib.fn("map_set_points")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_points")

    def set_observations(self, slot, rows=None, start=None, kf_slot=None):
        """rows: one list of keyframe slots per entry of `slot`; or the CSR arrays themselves."""
        if rows is not None:
            start, kf_slot = csr(rows)
        k = [self._p(slot, np.int32, c_int32_p), self._p(start, np.int32, c_int32_p), self._p(kf_slot, np.int32, c_int32_p)]
        self._check(self.lib.fn("map_set_observations")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_observations")

    def set_keyframes(self, slot, order_key, bad, parent, cov, child, point, line):
        """cov / child / point / line: one list per keyframe, or (start, flat) pairs."""
        lists = [x if isinstance(x, tuple) else csr(x) for x in (cov, child, point, line)]
        k = [self._p(slot, np.int32, c_int32_p), self._p(order_key, np.uint64, c_uint64_p), self._p(bad, np.uint8, c_uint8_p), self._p(parent, np.int32, c_int32_p)]
        for st, fl in lists:
            k.append(self._p(st, np.int32, c_int32_p)); k.append(self._p(fl, np.int32, c_int32_p))
        self._check(self.lib.fn("map_set_keyframes")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_keyframes")

    def set_lines(self, slot, x0, dir, x1, x2, desc, bad):
        k = [self._p(slot, np.int32, c_int32_p), self._p(x0, np.float64, c_double_p), self._p(dir, np.float64, c_double_p), self._p(x1, np.float64, c_double_p),
             self._p(x2, np.float64, c_double_p), self._p(desc, np.float32, c_float_p), self._p(bad, np.uint8, c_uint8_p)]
        self._check(self.lib.fn("map_set_lines")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_lines")
