"""ORBextractor::operator() on the device (lld_orb_extract): ctypes mirrors of the structs of include/lld_amd.h and a class with the
reference's constructor whose call returns the keypoints and descriptors in the shape of orb_search.Frame."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .abi import c_float_p, c_int32_p, c_uint32_p, c_uint8_p
from .orb_search import Frame, MonoBuiltFrame, StereoBuiltFrame, StereoMatches, StereoPyramids, StereoResult, frame_stereo_params, keypoints_struct

MAX_LEVELS = 16


class OrbExtractorParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32), ("ini_th_fast", C.c_int32),
                ("min_th_fast", C.c_int32), ("max_cols", C.c_int32), ("max_rows", C.c_int32), ("max_images", C.c_int32),
                ("pattern", c_int32_p)]


class OrbExtractorLevels(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("max_keypoints", C.c_int32),
                ("scale_factor", C.c_float * MAX_LEVELS), ("inv_scale_factor", C.c_float * MAX_LEVELS),
                ("level_sigma2", C.c_float * MAX_LEVELS), ("inv_level_sigma2", C.c_float * MAX_LEVELS),
                ("features_per_level", C.c_int32 * MAX_LEVELS), ("umax", C.c_int32 * 16)]


class OrbImage(C.Structure):
    _fields_ = [("data", c_uint8_p), ("cols", C.c_int32), ("rows", C.c_int32), ("step", C.c_int32), ("on_device", C.c_int32)]


class OrbLevelStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_candidates", "cells_min_th", "cells_empty", "iterations", "sorted_rounds",
                                          "finish_unchanged", "n_keypoints", "features_wanted")]


STATS_FIELDS = [f for f, _ in OrbLevelStats._fields_]


class OrbFeatures(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("n", C.c_int32), ("xy", c_float_p), ("octave", c_int32_p), ("angle", c_float_p),
                ("response", c_float_p), ("size", c_float_p), ("desc", c_uint32_p), ("stats", C.POINTER(OrbLevelStats))]


def _fn(lib, name, argtypes, restype=C.c_int):
    f = lib.fn(name)
    f.argtypes = argtypes
    f.restype = restype
    return f


class ORBextractor:
    """ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) with the caller's `pattern` ([256][4] or [512][2]
    ints: ORBextractor::pattern).  Calling it on one image (or a list of up to `max_images`) returns one Frame per image plus
    `.keypoints` fields; `.stereo_pyramids(...)` hands the device pyramid to lld_compute_stereo_matches."""

    def __init__(self, ctx, nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast, pattern, max_cols=1241, max_rows=376,
                 max_images=2):
        self.ctx = ctx
        self.lib = ctx.lib
        self._pattern = np.ascontiguousarray(np.asarray(pattern, np.int32).reshape(1024))
        P = OrbExtractorParams(int(nfeatures), float(np.float32(scale_factor)), int(nlevels), int(ini_th_fast), int(min_th_fast),
                               int(max_cols), int(max_rows), int(max_images), self._pattern.ctypes.data_as(c_int32_p))
        h = C.c_void_p()
        st = _fn(self.lib, "orb_extractor_create", [C.c_void_p, C.POINTER(OrbExtractorParams), C.POINTER(C.c_void_p)])(
            ctx.handle, C.byref(P), C.byref(h))
        if st != abi.LLD_OK:
            raise ValueError(f"lld_orb_extractor_create failed: {self.lib.fn('status_string')(st).decode()} (status {st})")
        self.handle = h
        self.n_levels = int(nlevels)
        L = OrbExtractorLevels()
        _fn(self.lib, "orb_extractor_levels_get", [C.c_void_p, C.POINTER(OrbExtractorLevels)])(h, C.byref(L))
        n = self.n_levels
        self.scale_factors = np.array(L.scale_factor[:n], np.float32)
        self.inv_scale_factors = np.array(L.inv_scale_factor[:n], np.float32)
        self.level_sigma2 = np.array(L.level_sigma2[:n], np.float32)
        self.inv_level_sigma2 = np.array(L.inv_level_sigma2[:n], np.float32)
        self.features_per_level = np.array(L.features_per_level[:n], np.int32)
        self.umax = np.array(L.umax[:16], np.int32)
        self.max_keypoints = int(L.max_keypoints)
        self._extract = _fn(self.lib, "orb_extract", [C.c_void_p, C.c_int, C.POINTER(OrbImage), C.POINTER(OrbFeatures)])

    def extract_raw(self, images):
        """images: list of 2-D uint8 arrays (host) or (device pointer, cols, rows, step) tuples.  Returns (status, list of dicts)."""
        n = len(images)
        ims = (OrbImage * max(n, 1))()
        outs = (OrbFeatures * max(n, 1))()
        keep, res = [], []
        cap = self.max_keypoints
        for i, im in enumerate(images):
            if isinstance(im, tuple):
                ptr, cols, rows, step = im
                ims[i] = OrbImage(C.cast(C.c_void_p(ptr), c_uint8_p), cols, rows, step, 1)
            else:
                a = np.asarray(im, np.uint8)
                if a.strides[1] != 1:
                    a = np.ascontiguousarray(a)
                keep.append(a)
                ims[i] = OrbImage(a.ctypes.data_as(c_uint8_p), a.shape[1], a.shape[0], a.strides[0], 0)
            r = dict(xy=np.zeros((cap, 2), np.float32), octave=np.zeros(cap, np.int32), angle=np.zeros(cap, np.float32),
                     response=np.zeros(cap, np.float32), size=np.zeros(cap, np.float32), desc=np.zeros((cap, 8), np.uint32),
                     stats=(OrbLevelStats * self.n_levels)())
            o = outs[i]
            o.capacity = cap
            o.xy = r["xy"].ctypes.data_as(c_float_p); o.octave = r["octave"].ctypes.data_as(c_int32_p)
            o.angle = r["angle"].ctypes.data_as(c_float_p); o.response = r["response"].ctypes.data_as(c_float_p)
            o.size = r["size"].ctypes.data_as(c_float_p); o.desc = r["desc"].ctypes.data_as(c_uint32_p)
            o.stats = C.cast(r["stats"], C.POINTER(OrbLevelStats))
            res.append(r)
        st = self._extract(self.handle, n, ims, outs)
        for i, r in enumerate(res):
            k = outs[i].n if st == abi.LLD_OK else 0
            for f in ("xy", "octave", "angle", "response", "size", "desc"):
                r[f] = r[f][:k]
            r["stats"] = np.array([[getattr(s, f) for f in STATS_FIELDS] for s in r["stats"]], np.int32)
            r["n"] = k
        return st, res

    def __call__(self, images):
        """ORBextractor::operator() on one image (returns a Frame) or a list of images (returns a list): keypoints in the
        reference's order, descriptors [n][8] u32.  The Frame also carries `response`, `size` and per-level `stats`."""
        single = isinstance(images, np.ndarray) or (isinstance(images, tuple) and isinstance(images[0], int))
        ims = [images] if single else list(images)
        st, res = self.extract_raw(ims)
        if st != abi.LLD_OK:
            raise ValueError(f"lld_orb_extract failed: {self.lib.fn('status_string')(st).decode()} (status {st})")
        frames = []
        for r, im in zip(res, ims):
            cols, rows = (im[1], im[2]) if isinstance(im, tuple) else (im.shape[1], im.shape[0])
            F = Frame(desc=r["desc"], xy=r["xy"], octave=r["octave"], uright=np.full(r["n"], -1, np.float32), angle=r["angle"],
                      max_x=float(cols), max_y=float(rows), scale=self.scale_factors.copy(), sigma2=self.level_sigma2.copy(),
                      inv_sigma2=self.inv_level_sigma2.copy()).normalise()
            F.response, F.size, F.stats = r["response"], r["size"], r["stats"]
            frames.append(F)
        return frames[0] if single else frames

    def pyramid(self, image_index):
        """(level pointers, cols, rows, step) of image `image_index` of the last call (device memory)."""
        n = self.n_levels
        lv = (c_uint8_p * n)(); cols = np.zeros(n, np.int32); rows = np.zeros(n, np.int32); step = np.zeros(n, np.int32)
        st = _fn(self.lib, "orb_extractor_pyramids", [C.c_void_p, C.c_int, C.POINTER(c_uint8_p), c_int32_p, c_int32_p, c_int32_p])(
            self.handle, int(image_index), lv, cols.ctypes.data_as(c_int32_p), rows.ctypes.data_as(c_int32_p), step.ctypes.data_as(c_int32_p))
        if st != abi.LLD_OK:
            raise ValueError(f"lld_orb_extractor_pyramids failed (status {st})")
        return lv, cols, rows, step

    def stereo_pyramids(self, left_index=0, right_index=1):
        """The on-device StereoPyramids (on_device = 1) of the last call's left / right images for lld_compute_stereo_matches.
        Returns (struct, keep-alive)."""
        lp, cols, rows, lstep = self.pyramid(left_index)
        rp, _, _, rstep = self.pyramid(right_index)
        keep = dict(lp=lp, rp=rp, cols=cols, rows=rows, lstep=lstep, rstep=rstep, scale=self.scale_factors.copy(),
                    inv=self.inv_scale_factors.copy())
        P = StereoPyramids(); P.n_levels = self.n_levels
        P.left = C.cast(lp, C.POINTER(c_uint8_p)); P.right = C.cast(rp, C.POINTER(c_uint8_p))
        P.cols = cols.ctypes.data_as(c_int32_p); P.rows = rows.ctypes.data_as(c_int32_p)
        P.left_step = lstep.ctypes.data_as(c_int32_p); P.right_step = rstep.ctypes.data_as(c_int32_p)
        P.scale_factors = keep["scale"].ctypes.data_as(c_float_p); P.inv_scale_factors = keep["inv"].ctypes.data_as(c_float_p)
        P.on_device = 1
        return P, keep

    def build_stereo_frame_raw(self, left_index, right_index, params):
        """lld_frame_build_stereo as it is: (status, handle)."""
        h = C.c_void_p()
        st = _fn(self.lib, "frame_build_stereo", [C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.FrameStereoParams), C.POINTER(C.c_void_p)])(
            self.handle, int(left_index), int(right_index), None if params is None else C.byref(params), C.byref(h))
        return st, h

    def build_stereo_frame(self, L: Frame, mb, mbf, left_index=0, right_index=1) -> StereoBuiltFrame:
        """Frame::Frame's device part on images left_index / right_index of the last call (lld_frame_build_stereo): the stereo
        search, the refinement and the resident frame, without the keypoints leaving HBM.  `L`: the Frame the last call returned
        for the left image (image bounds for the grid; the host's view of the keypoints).  Queued, not waited for."""
        prm, keep = frame_stereo_params(L, mb, mbf)
        st, h = self.build_stereo_frame_raw(left_index, right_index, prm)
        if st != abi.LLD_OK:
            raise RuntimeError(f"lld_frame_build_stereo failed: {self.lib.fn('status_string')(st).decode()} (status {st})")
        return StereoBuiltFrame(self.lib, self.ctx.handle, L, h)

    def build_mono_frame_raw(self, image_index, depth, params):
        """lld_frame_build_mono as it is: (status, handle).  depth: an abi.DepthImage or None."""
        h = C.c_void_p()
        st = _fn(self.lib, "frame_build_mono", [C.c_void_p, C.c_int, C.POINTER(abi.DepthImage), C.POINTER(abi.FrameMonoParams), C.POINTER(C.c_void_p)])(
            self.handle, int(image_index), None if depth is None else C.byref(depth), None if params is None else C.byref(params), C.byref(h))
        return st, h

    def build_mono_frame(self, L: Frame, cam, dist, mbf, depth=None, depth_factor=1.0, image_index=0) -> MonoBuiltFrame:
        """Frame::Frame's device part for an RGB-D (depth given) or monocular image of the last call (lld_frame_build_mono):
        UndistortKeyPoints and ComputeStereoFromRGBD without the keypoints leaving HBM.  `L`: the Frame the last call returned for that
        image; cam: (fx, fy, cx, cy, ...); dist: mDistCoef (4 or 5 floats); depth: a float32 / uint16 image as GrabImageRGBD receives
        it (or a device tuple, orb_search.depth_image_struct) with depth_factor = mDepthMapFactor.  Queued, not waited for."""
        from .orb_search import depth_image_struct, frame_mono_params, mono_host_frame
        H = mono_host_frame(self.lib, L, cam, dist)
        prm, keep = frame_mono_params(H, cam, dist, mbf)
        D, keep2 = depth_image_struct(depth, depth_factor)
        st, h = self.build_mono_frame_raw(image_index, D, prm)
        if st != abi.LLD_OK:
            raise RuntimeError(f"lld_frame_build_mono failed: {self.lib.fn('status_string')(st).decode()} (status {st})")
        return MonoBuiltFrame(self.lib, self.ctx.handle, H, h)

    def close(self):
        if getattr(self, "handle", None):
            _fn(self.lib, "orb_extractor_destroy", [C.c_void_p], None)(self.handle)
            self.handle = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()
    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compute_stereo_matches_device(ctx, L: Frame, R: Frame, ex: ORBextractor, mb, mbf, left_index=0, right_index=1) -> StereoMatches:
    """Frame::ComputeStereoMatches (lld_compute_stereo_matches) reading the extractor's device pyramid in place (on_device = 1)."""
    kl, kr = keypoints_struct(L), keypoints_struct(R)
    P, keep = ex.stereo_pyramids(left_index, right_index)
    out = StereoMatches(np.empty(L.n, np.float32), np.empty(L.n, np.float32), np.empty(L.n, np.int32), np.empty(L.n, np.int32), 0)
    r = StereoResult(); r.u_right = out.u_right.ctypes.data_as(c_float_p); r.depth = out.depth.ctypes.data_as(c_float_p)
    r.best_r = out.best_r.ctypes.data_as(c_int32_p); r.sad = out.sad.ctypes.data_as(c_int32_p)
    fn = _fn(ctx.lib, "compute_stereo_matches", [C.c_void_p, C.POINTER(type(kl)), C.POINTER(type(kr)), C.POINTER(StereoPyramids), C.c_float,
                                                 C.c_float, C.POINTER(StereoResult)])
    st = fn(ctx.handle, C.byref(kl), C.byref(kr), C.byref(P), float(np.float32(mb)), float(np.float32(mbf)), C.byref(r))
    if st != abi.LLD_OK:
        raise RuntimeError(f"lld_compute_stereo_matches failed (status {st})")
    out.n_matches = r.n_matches
    return out
