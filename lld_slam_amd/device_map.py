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
        f("map_set_observations_indexed").argtypes = [C.c_void_p, C.c_int32] + [c_int32_p] * 5; f("map_set_observations_indexed").restype = C.c_int
        f("map_set_keyframe_keypoints").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p, c_float_p, c_float_p]
        f("map_set_keyframe_keypoints").restype = C.c_int
        f("map_set_covisibles").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p]; f("map_set_covisibles").restype = C.c_int
        f("map_covisibility").argtypes = [C.c_void_p, C.POINTER(abi.MapCovisibilityIn), C.POINTER(abi.MapCovisibilityOut)]
        f("map_covisibility").restype = C.c_int
        f("map_download_links").argtypes = [C.c_void_p, C.c_int32] + [c_int32_p] * 5 + [C.c_int32, c_int32_p]; f("map_download_links").restype = C.c_int
        self._bind_ba()
        self._bind_apply()
        self._bind_refresh()
        self._bind_fuse()
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

    def set_observations_indexed(self, slot, rows=None, n_obs=None, start=None, kf_slot=None, kp_index=None):
        """rows: per entry of `slot` one list of (keyframe slot, keypoint index in that keyframe); or the CSR arrays themselves.
        n_obs: MapPoint::Observations() per point (the stereo-weighted count)."""
        if rows is not None:
            start, kf_slot = csr([[o[0] for o in r] for r in rows])
            _, kp_index = csr([[o[1] for o in r] for r in rows])
        k = [self._p(slot, np.int32, c_int32_p), self._p(start, np.int32, c_int32_p), self._p(kf_slot, np.int32, c_int32_p),
             self._p(kp_index, np.int32, c_int32_p), self._p(n_obs, np.int32, c_int32_p)]
        self._check(self.lib.fn("map_set_observations_indexed")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_observations_indexed")

    def set_keyframe_keypoints(self, slot, octave, depth, th_depth):
        """octave / depth: one list per keyframe with one entry per keypoint, or (start, flat) pairs with the same start; th_depth per keyframe."""
        st, oc = octave if isinstance(octave, tuple) else csr(octave)
        _, dp = depth if isinstance(depth, tuple) else csr(depth, np.float32)
        k = [self._p(slot, np.int32, c_int32_p), self._p(st, np.int32, c_int32_p), self._p(oc, np.int32, c_int32_p), self._p(dp, np.float32, c_float_p),
             self._p(th_depth, np.float32, c_float_p)]
        self._check(self.lib.fn("map_set_keyframe_keypoints")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_keyframe_keypoints")

    def set_covisibles(self, slot, cov):
        """cov: one list per keyframe (GetBestCovisibilityKeyFrames(10) in its order), or a (start, flat) pair.  Only the cov rows change."""
        st, fl = cov if isinstance(cov, tuple) else csr(cov)
        k = [self._p(slot, np.int32, c_int32_p), self._p(st, np.int32, c_int32_p), self._p(fl, np.int32, c_int32_p)]
        self._check(self.lib.fn("map_set_covisibles")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_covisibles")

    def links(self, kf_slots):
        """lld_map_download_links: (parent [n], cov: one list per keyframe as the device holds it, child: one list per keyframe in the row's order)."""
        s = np.ascontiguousarray(kf_slots, np.int32); n = len(s)
        parent = np.zeros(n, np.int32); ncov = np.zeros(n, np.int32); cov = np.zeros((n, 10), np.int32); start = np.zeros(n + 1, np.int32)
        p = lambda a: a.ctypes.data_as(c_int32_p)
        fn = self.lib.fn("map_download_links")
        st = fn(self.handle, n, p(s), p(parent), p(ncov), p(cov), p(start), 0, None)
        child = np.zeros(max(int(start[-1]), 1), np.int32)
        if st == abi.LLD_ERR_INVALID and start[-1] > 0:
            st = fn(self.handle, n, p(s), p(parent), p(ncov), p(cov), p(start), int(start[-1]), p(child))
        self._check(st, "lld_map_download_links")
        return parent, [cov[i, :ncov[i]].tolist() for i in range(n)], [child[start[i]:start[i + 1]].tolist() for i in range(n)]

    def covisibility(self, kf_slots, connections=True, culling=False, write_cov=False, monocular=False, th=None, th_obs=None, redundant_ratio=None,
                     conn_capacity=None, ordered_capacity=None, phase_ms=None, flags=None):
        """lld_map_covisibility for the keyframes kf_slots.  Returns a dict of arrays: conn_start, conn_kf, conn_weight, ordered_start, ordered_kf,
        ordered_weight, n_max, kf_max, updated (connections); n_mps, n_redundant, redundant (culling); status.  Every keyframe is a slot.
        Without capacities the call is made with a guess and repeated once with the totals the library reports; with them a short one raises
        (the error carries status, n_conn and n_ordered).  flags overrides the three booleans."""
        kf_slots = np.ascontiguousarray(kf_slots, np.int32)
        nq = len(kf_slots)
        if flags is None:
            flags = (1 if connections else 0) | (2 if culling else 0) | (abi.MAP_COVIS_WRITE_COV if write_cov else 0)
        a = abi.MapCovisibilityIn()
        a.n_queries, a.monocular, a.flags = nq, 1 if monocular else 0, int(flags)
        self.lib.fn("covisibility_params_default")(C.byref(a.params))
        if th is not None: a.params.th = int(th)
        if th_obs is not None: a.params.th_obs = int(th_obs)
        if redundant_ratio is not None: a.params.redundant_ratio = float(redundant_ratio)
        a.kf_slot = kf_slots.ctypes.data_as(c_int32_p)
        retry = conn_capacity is None and ordered_capacity is None
        caps = [64 * nq if conn_capacity is None else int(conn_capacity), 64 * nq if ordered_capacity is None else int(ordered_capacity)]
        while True:
            r = dict(conn_start=np.zeros(nq + 1, np.int32), conn_kf=np.zeros(max(caps[0], 1), np.int32), conn_weight=np.zeros(max(caps[0], 1), np.int32),
                     ordered_start=np.zeros(nq + 1, np.int32), ordered_kf=np.zeros(max(caps[1], 1), np.int32), ordered_weight=np.zeros(max(caps[1], 1), np.int32),
                     n_max=np.zeros(nq, np.int32), kf_max=np.zeros(nq, np.int32), updated=np.zeros(nq, np.uint8),
                     n_mps=np.zeros(nq, np.int32), n_redundant=np.zeros(nq, np.int32), redundant=np.zeros(nq, np.uint8), status=np.zeros(nq, np.uint8))
            o = abi.MapCovisibilityOut()
            o.lists.conn_capacity, o.lists.ordered_capacity = caps
            for name in ("conn_start", "conn_kf", "conn_weight", "ordered_start", "ordered_kf", "ordered_weight", "n_max", "kf_max", "n_mps", "n_redundant"):
                setattr(o.lists, name, r[name].ctypes.data_as(c_int32_p))
            o.lists.updated = r["updated"].ctypes.data_as(c_uint8_p); o.lists.redundant = r["redundant"].ctypes.data_as(c_uint8_p)
            o.status = r["status"].ctypes.data_as(c_uint8_p)
            if phase_ms is not None:
                assert phase_ms.dtype == np.float32 and phase_ms.size >= 3 and phase_ms.flags.c_contiguous
                o.lists.phase_ms = phase_ms.ctypes.data_as(c_float_p)
            o.lists.n_conn = o.lists.n_ordered = -1
            st = self.lib.fn("map_covisibility")(self.handle, C.byref(a), C.byref(o))
            short = st == abi.LLD_ERR_INVALID and o.lists.n_conn >= 0
            if short and retry:
                caps, retry = [o.lists.n_conn, o.lists.n_ordered], False
                continue
            if st != abi.LLD_OK:
                err = RuntimeError(f"lld_map_covisibility failed: {self.lib.fn('status_string')(st).decode()}")
                err.status, err.n_conn, err.n_ordered = st, (o.lists.n_conn if short else None), (o.lists.n_ordered if short else None)
                raise err
            break
        if flags & 1:
            nc, no = (o.lists.n_conn, o.lists.n_ordered) if nq else (0, 0)
            r["conn_kf"] = r["conn_kf"][:nc]; r["conn_weight"] = r["conn_weight"][:nc]
            r["ordered_kf"] = r["ordered_kf"][:no]; r["ordered_weight"] = r["ordered_weight"][:no]
        else:
            for name in ("conn_start", "conn_kf", "conn_weight", "ordered_start", "ordered_kf", "ordered_weight", "n_max", "kf_max", "updated"):
                del r[name]
        if not flags & 2:
            for name in ("n_mps", "n_redundant", "redundant"):
                del r[name]
        return r

    # ------------------------------------------------------------------ the local BA window (lld_map_ba.hip)
    def _bind_ba(self):
        f = self.lib.fn
        f("map_set_keyframe_features").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_uint64_p, c_float_p, c_int32_p, c_float_p, c_int32_p, c_float_p, c_float_p,
                                                   c_int32_p]
        f("map_set_keyframe_features").restype = C.c_int
        f("map_set_keyframe_poses").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_float_p]; f("map_set_keyframe_poses").restype = C.c_int
        f("map_set_line_observations").argtypes = [C.c_void_p, C.c_int32] + [c_int32_p] * 5; f("map_set_line_observations").restype = C.c_int
        f("map_ba_window").argtypes = [C.c_void_p, C.POINTER(abi.MapBaIn), C.POINTER(abi.MapBaWindowOut)]; f("map_ba_window").restype = C.c_int
        f("map_local_ba").argtypes = [C.c_void_p, C.POINTER(abi.MapBaIn), C.c_void_p, C.c_void_p, C.POINTER(abi.BAResult), C.POINTER(abi.MapBaIds)]
        f("map_local_ba").restype = C.c_int

    def set_keyframe_features(self, slot, mn_id, Tcw, kp_uvr, kl_left, kl_right, kl_octave):
        """Per keyframe: mn_id, Tcw (4x4 float), and one array per keyframe in the lists kp_uvr [(n_kp, 3)], kl_left / kl_right [(n_kl, 4)],
        kl_octave [(n_kl, 2)]; kl_right = -1 and right octave 0 for a keyline without a partner."""
        cat = lambda rows, w, dt: (np.concatenate([np.asarray(r, dt).reshape(-1, w) for r in rows]) if len(rows) else np.zeros((0, w), dt))
        kp_start = np.concatenate([[0], np.cumsum([np.asarray(r).reshape(-1, 3).shape[0] for r in kp_uvr])]).astype(np.int32)
        kl_start = np.concatenate([[0], np.cumsum([np.asarray(r).reshape(-1, 4).shape[0] for r in kl_left])]).astype(np.int32)
        k = [self._p(slot, np.int32, c_int32_p), self._p(mn_id, np.uint64, c_uint64_p), self._p(np.asarray(Tcw, np.float32).reshape(-1, 16), np.float32, c_float_p),
             self._p(kp_start, np.int32, c_int32_p), self._p(cat(kp_uvr, 3, np.float32), np.float32, c_float_p), self._p(kl_start, np.int32, c_int32_p),
             self._p(cat(kl_left, 4, np.float32), np.float32, c_float_p), self._p(cat(kl_right, 4, np.float32), np.float32, c_float_p),
             self._p(cat(kl_octave, 2, np.int32), np.int32, c_int32_p)]
        self._check(self.lib.fn("map_set_keyframe_features")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_keyframe_features")

    def set_keyframe_poses(self, slot, Tcw):
        k = [self._p(slot, np.int32, c_int32_p), self._p(np.asarray(Tcw, np.float32).reshape(-1, 16), np.float32, c_float_p)]
        self._check(self.lib.fn("map_set_keyframe_poses")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_keyframe_poses")

    def set_line_observations(self, slot, rows, n_obs):
        """rows: per line one list of (keyframe slot, keyline index) in std::map iteration order; n_obs: MapLine::Observations() per line."""
        start, kf_slot = csr([[o[0] for o in r] for r in rows])
        _, index = csr([[o[1] for o in r] for r in rows])
        k = [self._p(slot, np.int32, c_int32_p), self._p(start, np.int32, c_int32_p), self._p(kf_slot, np.int32, c_int32_p), self._p(index, np.int32, c_int32_p),
             self._p(n_obs, np.int32, c_int32_p)]
        self._check(self.lib.fn("map_set_line_observations")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_line_observations")

    def _ba_in(self, kf_slots, cam, inv_level_sigma2):
        s = np.ascontiguousarray(kf_slots, np.int32); sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        a = abi.MapBaIn()
        a.n_keyframes, a.n_levels = len(s), len(sig)
        a.kf_slot = s.ctypes.data_as(c_int32_p); a.inv_level_sigma2 = sig.ctypes.data_as(c_float_p)
        a.cam = abi.Camera(*[float(v) for v in cam])
        return a, (s, sig)

    BA_ARRAYS = (("cam_slot", np.int32, 0, 1), ("cam_qt", np.float64, 0, 7), ("point_slot", np.int32, 1, 1), ("pt_xyz", np.float64, 1, 3),
                 ("pt_obs_start", np.int32, 1, -1), ("pt_obs_cam", np.int32, 2, 1), ("pt_obs_uvr", np.float64, 2, 3), ("pt_obs_inv_sigma2", np.float64, 2, 1),
                 ("line_slot", np.int32, 3, 1), ("line_x0", np.float64, 3, 3), ("line_dir", np.float64, 3, 3), ("ln_obs_start", np.int32, 3, -1),
                 ("ln_obs_cam", np.int32, 4, 1), ("ln_obs_left", np.float64, 4, 4), ("ln_obs_right", np.float64, 4, 4), ("ln_obs_octave", np.int32, 4, 2))
    BA_COUNTS = ("n_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs")

    def ba_window(self, kf_slots, cam, inv_level_sigma2, capacities=None, phase_ms=None, fill=0):
        """lld_map_ba_window.  Returns a dict: the seven counts, status, and - when the status is 0 - the arrays of the window and the three slot
        lists, cut to their counts.  Without capacities (cameras, points, point observations, lines, line observations) the call is made with a
        guess and repeated once with the counts the library reports; with them a short one raises (the error carries status and counts).
        fill: the byte the arrays hold before the call (for tests that look at what a call leaves untouched; see raw)."""
        a, keep = self._ba_in(kf_slots, cam, inv_level_sigma2)
        retry = capacities is None
        caps = [64, 1024, 4096, 64, 256] if capacities is None else [int(c) for c in capacities]
        while True:
            o = abi.MapBaWindowOut()
            o.cam_capacity, o.point_capacity, o.pt_obs_capacity, o.line_capacity, o.ln_obs_capacity = caps
            raw = {}
            for name, dt, which, w in self.BA_ARRAYS:
                arr = np.full(caps[which] + 1 if w < 0 else max(caps[which], 1) * w, fill, np.uint8).repeat(np.dtype(dt).itemsize).view(dt)
                raw[name] = arr
                setattr(o, name, arr.ctypes.data_as(c_int32_p if dt == np.int32 else c_double_p))
            if phase_ms is not None:
                assert phase_ms.dtype == np.float32 and phase_ms.size >= 3 and phase_ms.flags.c_contiguous
                o.phase_ms = phase_ms.ctypes.data_as(c_float_p)
            o.n_cams = -1
            st = self.lib.fn("map_ba_window")(self.handle, C.byref(a), C.byref(o))
            counts = dict(n_cams=o.n_cams, n_free_cams=o.n_free_cams, n_local_cams=o.n_local_cams, n_points=o.n_points, n_pt_obs=o.n_pt_obs,
                          n_lines=o.n_lines, n_ln_obs=o.n_ln_obs)
            short = st == abi.LLD_ERR_INVALID and o.n_cams >= 0
            if short and retry:
                caps, retry = [counts[k] for k in self.BA_COUNTS], False
                continue
            if st != abi.LLD_OK:
                err = RuntimeError(f"lld_map_ba_window failed: {self.lib.fn('status_string')(st).decode()}")
                err.status, err.counts, err.raw = st, (counts if short else None), raw
                raise err
            break
        r = dict(counts, status=o.status, raw=raw)
        if o.status == 0:
            for name, dt, which, w in self.BA_ARRAYS:
                n = counts[self.BA_COUNTS[which]]
                r[name] = raw[name][:n + 1] if w < 0 else raw[name][:n * w].reshape((n, w) if w > 1 else (n,))
        return r

    def local_ba(self, kf_slots, cam, inv_level_sigma2, stop=False, params=None):
        """lld_map_local_ba.  Returns (BAOutput or None, ids): ids holds status, n_local_cams, cam_slot, point_slot, line_slot and window (a
        host.Window copy of what was solved); None when the status is not 0."""
        from . import host
        a, keep = self._ba_in(kf_slots, cam, inv_level_sigma2)
        res, ids = abi.BAResult(), abi.MapBaIds()
        flag = C.c_ubyte(1 if stop else 0)
        if params is None:
            params = host.ba_params(self.lib)
        self._check(self.lib.fn("map_local_ba")(self.handle, C.byref(a), C.byref(params), C.byref(flag), C.byref(res), C.byref(ids)), "lld_map_local_ba")
        out = dict(status=ids.status, n_local_cams=ids.n_local_cams)
        if ids.status:
            return None, out
        w = ids.window
        cp = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(max(n, 1),))[:n].astype(dt, copy=True) if n else np.zeros(0, dt)
        nc, npt, npo, nl, nlo = w.n_cams, w.n_points, w.n_pt_obs, w.n_lines, w.n_ln_obs
        out.update(cam_slot=cp(ids.cam_slot, nc, np.int32), point_slot=cp(ids.point_slot, npt, np.int32), line_slot=cp(ids.line_slot, nl, np.int32),
                   marked_bad_slot=cp(ids.marked_bad_slot, ids.n_marked_bad, np.int32))
        out["window"] = host.Window(tuple(getattr(w.cam, k) for k in ("fx", "fy", "cx", "cy", "bf")), w.n_free_cams, cp(w.cam_qt, 7 * nc, np.float64).reshape(-1, 7),
                                    cp(w.pt_xyz, 3 * npt, np.float64).reshape(-1, 3), cp(w.pt_obs_start, npt + 1, np.int32), cp(w.pt_obs_cam, npo, np.int32),
                                    cp(w.pt_obs_uvr, 3 * npo, np.float64).reshape(-1, 3), cp(w.pt_obs_inv_sigma2, npo, np.float64),
                                    cp(w.line_x0, 3 * nl, np.float64).reshape(-1, 3), cp(w.line_dir, 3 * nl, np.float64).reshape(-1, 3),
                                    cp(w.ln_obs_start, nl + 1, np.int32), cp(w.ln_obs_cam, nlo, np.int32), cp(w.ln_obs_left, 4 * nlo, np.float64).reshape(-1, 4),
                                    cp(w.ln_obs_right, 4 * nlo, np.float64).reshape(-1, 4), cp(w.ln_obs_octave, 2 * nlo, np.int32).reshape(-1, 2))
        bo = host.BAOutput(cp(res.cam_qt, 7 * nc, np.float64).reshape(-1, 7), cp(res.pt_xyz, 3 * npt, np.float64).reshape(-1, 3),
                           cp(res.line_x0, 3 * nl, np.float64).reshape(-1, 3), cp(res.line_dir, 3 * nl, np.float64).reshape(-1, 3),
                           cp(res.pt_obs_outlier, npo, np.uint8), cp(res.ln_edge_outlier, 2 * nlo, np.uint8).reshape(-1, 2), cp(res.line_removed, nl, np.uint8),
                           host.stats_dict(res.stats))
        return bo, out

    # ------------------------------------------------------------------ a local BA's result applied to the map (lld_map_apply.hip)
    def _bind_apply(self):
        f = self.lib.fn
        f("map_set_point_refs").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_int32_p]; f("map_set_point_refs").restype = C.c_int
        f("map_ba_apply").argtypes = [C.c_void_p, C.POINTER(abi.MapBaApplyIn), C.POINTER(abi.MapBaApplyOut)]; f("map_ba_apply").restype = C.c_int
        f("map_download_rows").argtypes = [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, c_int32_p, C.c_int32, c_int32_p]; f("map_download_rows").restype = C.c_int

    def set_point_refs(self, slot, ref_kf):
        """MapPoint::mpRefKF per point slot as a keyframe slot, -1: unknown."""
        k = [self._p(slot, np.int32, c_int32_p), self._p(ref_kf, np.int32, c_int32_p)]
        self._check(self.lib.fn("map_set_point_refs")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_point_refs")

    APPLY_POINT = (("pt_pos", np.float32, 3), ("pt_normal", np.float32, 3), ("pt_min_distance", np.float32, 1), ("pt_max_distance", np.float32, 1),
                   ("pt_n_obs", np.int32, 1), ("pt_ref_kf", np.int32, 1), ("pt_row_len", np.int32, 1), ("pt_flags", np.uint8, 1))
    APPLY_LINE = (("ln_bad", np.uint8, 1), ("ln_n_obs", np.int32, 1), ("ln_row_len", np.int32, 1))
    APPLY_COUNTS = ("n_local_cams", "n_pt_obs_erased", "n_ln_obs_erased", "n_points_bad", "n_lines_bad", "n_index_skipped")

    def ba_apply(self, result, level_scale, n_local_cams=None, phase_ms=None, counts=None):
        """lld_map_ba_apply: `result` (a host.BAOutput, or anything with cam_qt, pt_xyz, line_x0, line_dir, pt_obs_outlier, ln_edge_outlier and
        line_removed) applied to the window this map assembled last.  n_local_cams sizes tcw / ow (default: every camera of the result).
        counts overrides the five counts sent (for tests of the refusals).  Returns a dict: the six counts, tcw, ow, and the per-point and
        per-line arrays of lld_map_ba_apply_out."""
        g = (lambda k: result[k]) if isinstance(result, dict) else (lambda k: getattr(result, k))
        cam_qt = np.ascontiguousarray(g("cam_qt"), np.float64).reshape(-1, 7); pt_xyz = np.ascontiguousarray(g("pt_xyz"), np.float64).reshape(-1, 3)
        x0 = np.ascontiguousarray(g("line_x0"), np.float64).reshape(-1, 3); d = np.ascontiguousarray(g("line_dir"), np.float64).reshape(-1, 3)
        po = np.ascontiguousarray(g("pt_obs_outlier"), np.uint8).reshape(-1); lo = np.ascontiguousarray(g("ln_edge_outlier"), np.uint8).reshape(-1, 2)
        rm = np.ascontiguousarray(g("line_removed"), np.uint8).reshape(-1); ls = np.ascontiguousarray(level_scale, np.float32)
        a = abi.MapBaApplyIn()
        a.n_cams, a.n_points, a.n_pt_obs, a.n_lines, a.n_ln_obs = (len(cam_qt), len(pt_xyz), len(po), len(x0), len(lo)) if counts is None else counts
        a.n_levels = len(ls)
        a.cam_qt = cam_qt.ctypes.data_as(c_double_p); a.pt_xyz = pt_xyz.ctypes.data_as(c_double_p); a.line_x0 = x0.ctypes.data_as(c_double_p)
        a.line_dir = d.ctypes.data_as(c_double_p); a.pt_obs_outlier = po.ctypes.data_as(c_uint8_p); a.ln_edge_outlier = lo.ctypes.data_as(c_uint8_p)
        a.line_removed = rm.ctypes.data_as(c_uint8_p); a.level_scale = ls.ctypes.data_as(c_float_p)
        nloc = len(cam_qt) if n_local_cams is None else int(n_local_cams)
        r = dict(tcw=np.zeros((max(nloc, 1), 16), np.float32), ow=np.zeros((max(nloc, 1), 3), np.float32))
        for name, dt, w in self.APPLY_POINT:
            r[name] = np.zeros((max(len(pt_xyz), 1), w) if w > 1 else max(len(pt_xyz), 1), dt)
        for name, dt, w in self.APPLY_LINE:
            r[name] = np.zeros(max(len(x0), 1), dt)
        o = abi.MapBaApplyOut()
        ptr = {np.float32: c_float_p, np.int32: c_int32_p, np.uint8: c_uint8_p}
        for name, arr in r.items():
            setattr(o, name, arr.ctypes.data_as(ptr[arr.dtype.type]))
        if phase_ms is not None:
            assert phase_ms.dtype == np.float32 and phase_ms.size >= 3 and phase_ms.flags.c_contiguous
            o.phase_ms = phase_ms.ctypes.data_as(c_float_p)
        self._check(self.lib.fn("map_ba_apply")(self.handle, C.byref(a), C.byref(o)), "lld_map_ba_apply")
        nloc = o.n_local_cams
        r["tcw"] = r["tcw"][:nloc].reshape(-1, 4, 4); r["ow"] = r["ow"][:nloc]
        for name, _, _ in self.APPLY_POINT:
            r[name] = r[name][:len(pt_xyz)]
        for name, _, _ in self.APPLY_LINE:
            r[name] = r[name][:len(x0)]
        r.update({k: getattr(o, k) for k in self.APPLY_COUNTS})
        return r

    def rows(self, kind, slots):
        """lld_map_download_rows: the rows of one pool as the device holds them, one list per slot.  kind: a key of abi.MAP_ROWS or its value."""
        kind = abi.MAP_ROWS[kind] if isinstance(kind, str) else int(kind)
        s = np.ascontiguousarray(slots, np.int32); n = len(s)
        start = np.zeros(n + 1, np.int32)
        p = lambda a: a.ctypes.data_as(c_int32_p)
        fn = self.lib.fn("map_download_rows")
        st = fn(self.handle, kind, n, p(s), p(start), 0, None)
        data = np.zeros(max(int(start[-1]), 1), np.int32)
        if st == abi.LLD_ERR_INVALID and start[-1] > 0:
            st = fn(self.handle, kind, n, p(s), p(start), int(start[-1]), p(data))
        self._check(st, "lld_map_download_rows")
        return [data[start[i]:start[i + 1]].tolist() for i in range(n)]

    # ------------------------------------------------------------------ landmark refresh on the map's tables (lld_map_refresh.hip)
    def _bind_refresh(self):
        f = self.lib.fn
        f("map_set_keyframe_descriptors").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_uint32_p]; f("map_set_keyframe_descriptors").restype = C.c_int
        f("map_set_keyframe_line_descriptors").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_float_p]
        f("map_set_keyframe_line_descriptors").restype = C.c_int
        f("map_refresh_points").argtypes = [C.c_void_p, C.POINTER(abi.MapRefreshPointsIn), C.POINTER(abi.MapRefreshPointsOut)]; f("map_refresh_points").restype = C.c_int
        f("map_refresh_lines").argtypes = [C.c_void_p, C.POINTER(abi.MapRefreshLinesIn), C.POINTER(abi.MapRefreshLinesOut)]; f("map_refresh_lines").restype = C.c_int
        f("map_download_points").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_float_p, c_float_p, c_float_p, c_float_p, c_uint32_p, c_uint8_p]
        f("map_download_points").restype = C.c_int
        f("map_download_lines").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_float_p, c_uint8_p]; f("map_download_lines").restype = C.c_int

    def _set_kf_desc(self, name, slot, desc, dtype, ptr, width):
        rows = [np.ascontiguousarray(d, dtype).reshape(-1, width) for d in desc]
        start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        flat = np.concatenate(rows) if rows else np.zeros((0, width), dtype)
        k = [self._p(slot, np.int32, c_int32_p), self._p(start, np.int32, c_int32_p), self._p(flat, dtype, ptr)]
        self._check(self.lib.fn(name)(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_" + name)

    def set_keyframe_descriptors(self, slot, desc):
        """desc: per keyframe mDescriptors as an (n_keypoints, 8) uint32 array, one row per entry of its point row."""
        self._set_kf_desc("map_set_keyframe_descriptors", slot, desc, np.uint32, c_uint32_p, 8)

    def set_keyframe_line_descriptors(self, slot, desc):
        """desc: per keyframe mDescriptorsLines as an (n_keylines, line_dim) float32 array, one row per entry of its line row."""
        self._set_kf_desc("map_set_keyframe_line_descriptors", slot, desc, np.float32, c_float_p, self.limits.line_dim)

    REFRESH_POINT = (("desc", np.uint32, 8), ("best_obs", np.int32, 1), ("best_median", np.int32, 1), ("normal", np.float32, 3), ("min_distance", np.float32, 1),
                     ("max_distance", np.float32, 1), ("updated", np.uint8, 1))
    REFRESH_LINE = (("desc", np.float32, 0), ("best_obs", np.int32, 1), ("best_median", np.int32, 1), ("updated", np.uint8, 1))
    _PTR = {np.float32: c_float_p, np.int32: c_int32_p, np.uint8: c_uint8_p, np.uint32: c_uint32_p}

    def refresh_points(self, slots, flags=abi.LANDMARK_DESCRIPTOR | abi.LANDMARK_NORMAL_DEPTH, level_scale=None, phase_ms=None, omit=()):
        """lld_map_refresh_points for the point slots `slots`.  Returns a dict of per-query arrays: desc, best_obs, best_median, normal,
        min_distance, max_distance (what the map holds behind the call) and updated.  omit: names of output arrays passed as NULL."""
        s = np.ascontiguousarray(slots, np.int32); n = len(s)
        a = abi.MapRefreshPointsIn()
        a.n, a.flags = n, int(flags)
        a.slot = s.ctypes.data_as(c_int32_p)
        ls = None
        if level_scale is not None:
            ls = np.ascontiguousarray(level_scale, np.float32)
            a.n_levels = len(ls); a.level_scale = ls.ctypes.data_as(c_float_p)
        r, o = {}, abi.MapRefreshPointsOut()
        for name, dt, w in self.REFRESH_POINT:
            if name in omit:
                continue
            r[name] = np.zeros((max(n, 1), w) if w > 1 else max(n, 1), dt)
            setattr(o, name, r[name].ctypes.data_as(self._PTR[dt]))
        if phase_ms is not None:
            assert phase_ms.dtype == np.float32 and phase_ms.size >= 3 and phase_ms.flags.c_contiguous
            o.phase_ms = phase_ms.ctypes.data_as(c_float_p)
        self._check(self.lib.fn("map_refresh_points")(self.handle, C.byref(a), C.byref(o)), "lld_map_refresh_points")
        return {k: v[:n] for k, v in r.items()}

    def refresh_lines(self, slots, phase_ms=None, omit=()):
        """lld_map_refresh_lines for the line slots `slots`: desc (n x line_dim), best_obs, best_median, updated."""
        s = np.ascontiguousarray(slots, np.int32); n = len(s)
        a = abi.MapRefreshLinesIn()
        a.n = n; a.slot = s.ctypes.data_as(c_int32_p)
        r, o = {}, abi.MapRefreshLinesOut()
        for name, dt, w in self.REFRESH_LINE:
            if name in omit:
                continue
            r[name] = np.zeros((max(n, 1), self.limits.line_dim) if w == 0 else max(n, 1), dt)
            setattr(o, name, r[name].ctypes.data_as(self._PTR[dt]))
        if phase_ms is not None:
            assert phase_ms.dtype == np.float32 and phase_ms.size >= 3 and phase_ms.flags.c_contiguous
            o.phase_ms = phase_ms.ctypes.data_as(c_float_p)
        self._check(self.lib.fn("map_refresh_lines")(self.handle, C.byref(a), C.byref(o)), "lld_map_refresh_lines")
        return {k: v[:n] for k, v in r.items()}

    def download_points(self, slots):
        """lld_map_download_points: pos, normal, min_distance, max_distance, desc and state of the point slots as the device holds them."""
        s = np.ascontiguousarray(slots, np.int32); n = len(s)
        r = dict(pos=np.zeros((max(n, 1), 3), np.float32), normal=np.zeros((max(n, 1), 3), np.float32), min_distance=np.zeros(max(n, 1), np.float32),
                 max_distance=np.zeros(max(n, 1), np.float32), desc=np.zeros((max(n, 1), 8), np.uint32), state=np.zeros(max(n, 1), np.uint8))
        self._check(self.lib.fn("map_download_points")(self.handle, n, s.ctypes.data_as(c_int32_p), *[v.ctypes.data_as(self._PTR[v.dtype.type]) for v in r.values()]),
                    "lld_map_download_points")
        return {k: v[:n] for k, v in r.items()}

    def download_lines(self, slots):
        """lld_map_download_lines: desc (n x line_dim) and bad of the line slots as the device holds them."""
        s = np.ascontiguousarray(slots, np.int32); n = len(s)
        r = dict(desc=np.zeros((max(n, 1), self.limits.line_dim), np.float32), bad=np.zeros(max(n, 1), np.uint8))
        self._check(self.lib.fn("map_download_lines")(self.handle, n, s.ctypes.data_as(c_int32_p), r["desc"].ctypes.data_as(c_float_p), r["bad"].ctypes.data_as(c_uint8_p)),
                    "lld_map_download_lines")
        return {k: v[:n] for k, v in r.items()}

    # ------------------------------------------------------------------ duplicate map points fused on the map's tables (lld_map_fuse.hip)
    def _bind_fuse(self):
        f = self.lib.fn
        f("map_fuse").argtypes = [C.c_void_p, C.POINTER(abi.MapFuseIn), C.POINTER(abi.MapFuseOut)]; f("map_fuse").restype = C.c_int
        f("map_download_point_counts").argtypes = [C.c_void_p, C.c_int32, c_int32_p, c_int32_p]; f("map_download_point_counts").restype = C.c_int

    def fuse(self, target, view, grid, level_scale, level_inv_sigma2, point_slot=None, source_keyframe=-1, th=3.0, n_points=None, survivor_capacity=None,
             phase_ms=None):
        """lld_map_fuse: one ORBmatcher::Fuse(pKF, vpMapPoints, th) into keyframe slot `target`.  view: pKF's lld_frame_view (orb_search.FrameView,
        as orb_search.frame_view builds it); grid: (min_x, min_y, width_inv, height_inv, cols, rows) as lld_orb_search carries them; the candidates
        are point_slot (-1 = a NULL entry) or, with source_keyframe >= 0, that keyframe's point row as the map holds it.  Returns a dict:
        n_fused, n_added, n_replaced, match, action, other (per candidate) and survivor.  A refusal raises; the error carries status and
        n_survivors."""
        ls = np.ascontiguousarray(level_scale, np.float32); sig = np.ascontiguousarray(level_inv_sigma2, np.float32)
        a = abi.MapFuseIn()
        ps = None
        if point_slot is not None:
            ps = np.ascontiguousarray(point_slot, np.int32)
            a.point_slot = ps.ctypes.data_as(c_int32_p)
        n = (len(ps) if ps is not None else len(self.rows("kf_points", [source_keyframe])[0])) if n_points is None else int(n_points)
        a.target, a.n_points, a.source_keyframe, a.th = int(target), n, int(source_keyframe), float(np.float32(th))
        C.memmove(C.byref(a.view), C.byref(view), C.sizeof(abi.FrameViewStruct))
        a.grid_min_x, a.grid_min_y, a.grid_width_inv, a.grid_height_inv = [float(np.float32(v)) for v in grid[:4]]
        a.grid_cols, a.grid_rows = int(grid[4]), int(grid[5])
        a.n_levels = len(ls); a.level_scale = ls.ctypes.data_as(c_float_p); a.level_inv_sigma2 = sig.ctypes.data_as(c_float_p)
        cap = max(n, 0) if survivor_capacity is None else int(survivor_capacity)
        r = dict(match=np.full(max(n, 1), -1, np.int32), action=np.zeros(max(n, 1), np.uint8), other=np.full(max(n, 1), -1, np.int32), survivor=np.zeros(max(cap, 1), np.int32))
        o = abi.MapFuseOut()
        o.match = r["match"].ctypes.data_as(c_int32_p); o.action = r["action"].ctypes.data_as(c_uint8_p); o.other = r["other"].ctypes.data_as(c_int32_p)
        o.survivor = r["survivor"].ctypes.data_as(c_int32_p); o.survivor_capacity = cap
        if phase_ms is not None:
            assert phase_ms.dtype == np.float32 and phase_ms.size >= 4 and phase_ms.flags.c_contiguous
            o.phase_ms = phase_ms.ctypes.data_as(c_float_p)
        st = self.lib.fn("map_fuse")(self.handle, C.byref(a), C.byref(o))
        if st != abi.LLD_OK:
            err = RuntimeError(f"lld_map_fuse failed: {self.lib.fn('status_string')(st).decode()}")
            err.status, err.n_survivors = st, o.n_survivors
            raise err
        n = max(n, 0)
        return dict(n_fused=o.n_fused, n_added=o.n_added, n_replaced=o.n_replaced, match=r["match"][:n], action=r["action"][:n], other=r["other"][:n],
                    survivor=r["survivor"][:o.n_survivors].copy())

    def point_counts(self, slots):
        """lld_map_download_point_counts: MapPoint::Observations() of the point slots as the device holds it."""
        s = np.ascontiguousarray(slots, np.int32); n = len(s)
        out = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.fn("map_download_point_counts")(self.handle, n, s.ctypes.data_as(c_int32_p), out.ctypes.data_as(c_int32_p)), "lld_map_download_point_counts")
        return out[:n]

    def set_lines(self, slot, x0, dir, x1, x2, desc, bad):
        k = [self._p(slot, np.int32, c_int32_p), self._p(x0, np.float64, c_double_p), self._p(dir, np.float64, c_double_p), self._p(x1, np.float64, c_double_p),
             self._p(x2, np.float64, c_double_p), self._p(desc, np.float32, c_float_p), self._p(bad, np.uint8, c_uint8_p)]
        self._check(self.lib.fn("map_set_lines")(self.handle, len(k[0][0]), *[p for _, p in k]), "lld_map_set_lines")
