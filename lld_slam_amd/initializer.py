"""ORB-SLAM2's Initializer on the device (lld_initializer_*): the H / F RANSAC of the monocular bootstrap and the reconstruction
of the motion.  A handle lives as long as the reference's object; the rules and the two deviations are those of include/lld_amd.h."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import InitializerHypothesis, InitializerParams, InitializerResult, c_float_p, c_int32_p, c_uint8_p

MAX_KEYPOINTS = 8192         # LLD_INIT_MAX_KEYPOINTS
MAX_ITERATIONS = 4096        # LLD_INIT_MAX_ITERATIONS
DEFAULT_PARAMS = (1.0, 200, 1.0, 50, 0)    # sigma, iterations (Tracking.cc:596), minParallax, minTriangulated (:116-118), seed


class InitializerError(RuntimeError):
    def __init__(self, what, status):
        super().__init__(f"{what} failed with status {status}")
        self.status = status


@dataclass
class InitializerOutput:
    """Initialize()'s outputs: success, R21 (3x3) / t21 (3) / vP3D (n1 x 3) / vbTriangulated (n1) (zeros unless success), and the
    intermediate results: the model run (0 H, 1 F), SH / SF / RH, the winning H21 / F21 with their inlier counts and masks (N),
    nGood / parallax of every motion hypothesis, the hypothesis examined and the winning iterations."""
    success: bool
    model: int
    SH: np.float32
    SF: np.float32
    RH: np.float32
    H21: np.ndarray
    F21: np.ndarray
    n_inliers_H: int
    n_inliers_F: int
    R21: np.ndarray
    t21: np.ndarray
    n_good: np.ndarray
    parallax: np.ndarray
    best_index: int
    n_matches: int
    win_H: int
    win_F: int
    inlier_H: np.ndarray | None
    inlier_F: np.ndarray | None
    p3d: np.ndarray | None
    triangulated: np.ndarray | None


def _params(params):
    p = InitializerParams()
    p.sigma, p.iterations, p.min_parallax, p.min_triangulated, p.seed = params
    return p


def problem_from_scene(sc):
    """(K, keys1, keys2, matches12) of a two-view scene dict (K 3x3, keys1 n1 x 2, keys2 n2 x 2, matches12 int[n1])."""
    return (np.asarray(sc["K"], np.float32).reshape(3, 3), np.asarray(sc["keys1"], np.float32).reshape(-1, 2),
            np.asarray(sc["keys2"], np.float32).reshape(-1, 2), np.asarray(sc["matches12"], np.int32).reshape(-1))


class Initializer:
    """Initializer(ReferenceFrame, sigma, iterations): K and the reference frame's undistorted keypoints stay on the device."""

    def __init__(self, ctx, K, keys1, sigma=1.0, iterations=200, min_parallax=1.0, min_triangulated=50, seed=0):
        self.ctx = ctx
        self.lib = ctx.lib
        self.handle = None
        self._K = np.ascontiguousarray(K, np.float32).reshape(-1)
        self._keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1)
        self.n1 = len(self._keys1) // 2
        self._params = _params((sigma, iterations, min_parallax, min_triangulated, int(seed) & 0xFFFFFFFF))
        h = C.c_void_p()
        st = self.lib.fn("initializer_create")(ctx.handle, self._K.ctypes.data_as(c_float_p) if self._K.size == 9 else None, self.n1,
                                               self._keys1.ctypes.data_as(c_float_p), C.byref(self._params), C.byref(h))
        if st != abi.LLD_OK:
            raise InitializerError("lld_initializer_create", st)
        self.handle = h

    def Initialize(self, keys2, vMatches12, want_inliers=True, want_points=True):
        """Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated) -> InitializerOutput.  keys2: the current
        frame's undistorted keypoints (n2 x 2); vMatches12[i]: the keypoint of frame 2 matched to keypoint i, or negative."""
        k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1)
        m = np.ascontiguousarray(vMatches12, np.int32).reshape(-1)
        r = InitializerResult()
        inl_H = inl_F = p3d = tri = None
        if want_inliers:
            inl_H = np.zeros(max(self.n1, 1), np.uint8); inl_F = np.zeros(max(self.n1, 1), np.uint8)
            r.inlier_H = inl_H.ctypes.data_as(c_uint8_p); r.inlier_F = inl_F.ctypes.data_as(c_uint8_p)
        if want_points:
            p3d = np.zeros((self.n1, 3), np.float32); tri = np.zeros(self.n1, np.uint8)
            r.p3d = p3d.ctypes.data_as(c_float_p); r.triangulated = tri.ctypes.data_as(c_uint8_p)
        st = self.lib.fn("initializer_initialize")(self.handle, len(k2) // 2, k2.ctypes.data_as(c_float_p), len(m),
                                                   m.ctypes.data_as(c_int32_p), C.byref(r))
        if st != abi.LLD_OK:
            raise InitializerError("lld_initializer_initialize", st)
        return output_from_result(r, inl_H, inl_F, p3d, tri)

    def hypotheses(self, model, capacity=None):
        """Diagnostic: the last call's hypotheses of one model (0 H, 1 F) in iteration order: dicts with idx (8), M (3x3),
        score (float32), n_inliers."""
        fn = self.lib.fn("initializer_hypotheses")
        n = C.c_int32()
        st = fn(self.handle, model, 0, None, C.byref(n))
        if st != abi.LLD_OK:
            raise InitializerError("lld_initializer_hypotheses", st)
        m = n.value if capacity is None else min(capacity, n.value)
        buf = (InitializerHypothesis * max(m, 1))()
        st = fn(self.handle, model, m, buf, C.byref(n))
        if st != abi.LLD_OK:
            raise InitializerError("lld_initializer_hypotheses", st)
        return [dict(idx=list(h.idx), M=np.array(h.M[:], np.float32).reshape(3, 3), score=np.float32(h.score),
                     n_inliers=h.n_inliers) for h in buf[:m]]

    def close(self):
        if getattr(self, "handle", None):
            self.lib.fn("initializer_destroy")(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def output_from_result(r, inl_H=None, inl_F=None, p3d=None, tri=None):
    N = r.n_matches
    return InitializerOutput(
        bool(r.success), r.model, np.float32(r.SH), np.float32(r.SF), np.float32(r.RH),
        np.array(r.H21[:], np.float32).reshape(3, 3), np.array(r.F21[:], np.float32).reshape(3, 3), r.n_inliers_H, r.n_inliers_F,
        np.array(r.R21[:], np.float32).reshape(3, 3), np.array(r.t21[:], np.float32), np.array(r.n_good[:], np.int32),
        np.array(r.parallax[:], np.float32), r.best_index, N, r.win_H, r.win_F,
        None if inl_H is None else inl_H[:N].copy(), None if inl_F is None else inl_F[:N].copy(), p3d, tri)
