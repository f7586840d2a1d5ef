"""ORB-SLAM2's PnPsolver on the device (lld_pnp_*): a batch of independent solvers, one per relocalisation candidate, whose
RANSAC state stays in HBM between iterate() calls.  The rules and the two deviations are those of include/lld_amd.h."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import PnPHypothesis, PnPParams, PnPProblem, PnPResult, c_float_p, c_int32_p, c_uint8_p

MAX_CORRESPONDENCES = 8192   # LLD_PNP_MAX_CORRESPONDENCES
MAX_KEYPOINTS = 8192         # LLD_PNP_MAX_KEYPOINTS
MAX_SOLVERS = 256            # LLD_PNP_MAX_SOLVERS
MAX_ITERATIONS = 65536       # LLD_PNP_MAX_ITERATIONS
DEFAULT_PARAMS = (0.99, 10, 300, 4, 0.5, 5.991)     # SetRansacParameters as Tracking::Relocalization calls it


class PnPError(RuntimeError):
    def __init__(self, what, status):
        super().__init__(f"{what} failed with status {status}")
        self.status = status


@dataclass
class PnPOutput:
    """iterate()'s return: Tcw (3x4 float32) or None, bNoMore, vbInliers (uint8[n_keypoints]), nInliers, and the solver's
    mnIterations / mnBestInliers after the call."""
    Tcw: np.ndarray | None
    no_more: bool
    inliers: np.ndarray
    n_inliers: int
    iterations: int
    best_inliers: int


def _params(params):
    p = PnPParams()
    p.probability, p.min_inliers, p.max_iterations, p.min_set, p.epsilon, p.th2 = params
    return p


class _Problem:
    """One solver's correspondences, kept alive for the C struct."""

    def __init__(self, xyz, uv, sigma2, kp_index, n_keypoints, fx, fy, cx, cy, seed=0):
        self.xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1)
        self.uv = np.ascontiguousarray(uv, np.float32).reshape(-1)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        self.kp = np.ascontiguousarray(kp_index, np.int32).reshape(-1)
        self.n_keypoints = int(n_keypoints)
        n = len(self.kp)
        self.c = PnPProblem(n, self.xyz.ctypes.data_as(c_float_p), self.uv.ctypes.data_as(c_float_p),
                            self.sigma2.ctypes.data_as(c_float_p), self.kp.ctypes.data_as(c_int32_p), self.n_keypoints,
                            float(fx), float(fy), float(cx), float(cy), int(seed) & 0xFFFFFFFF)


def problem_from_scene(sc):
    return _Problem(sc["xyz"], sc["uv"], sc["sigma2"], sc["kp_index"], sc["n_keypoints"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["seed"])


class PnPsolverBatch:
    """n PnPsolvers (PnPsolver(F, vpMapPointMatches) + SetRansacParameters) resident on the device.  Each problem is a dict
    with xyz, uv, sigma2, kp_index, n_keypoints, fx, fy, cx, cy, seed."""

    def __init__(self, ctx, problems, params=DEFAULT_PARAMS):
        self.ctx = ctx
        self.lib = ctx.lib
        self._p = [p if isinstance(p, _Problem) else problem_from_scene(p) for p in problems]
        arr = (PnPProblem * len(self._p))(*[p.c for p in self._p])
        self._params = _params(params)
        h = C.c_void_p()
        st = self.lib.fn("pnp_batch_create")(ctx.handle, len(self._p), arr, C.byref(self._params), C.byref(h))
        if st != abi.LLD_OK:
            raise PnPError("lld_pnp_batch_create", st)
        self.handle = h
        self.n = len(self._p)

    def iterate(self, nIterations=5, active=None):
        """iterate(nIterations) on every active solver (one device-resident sequence); returns the outputs of all solvers
        (inactive ones keep their previous outputs)."""
        self.iterate_async(nIterations, active)
        return self.download()

    def iterate_async(self, nIterations=5, active=None):
        act = None
        if active is not None:
            self._act = np.ascontiguousarray(np.asarray(active, bool).astype(np.uint8))
            act = self._act.ctypes.data_as(c_uint8_p)
        st = self.lib.fn("pnp_batch_iterate")(self.handle, int(nIterations), act)
        if st != abi.LLD_OK:
            raise PnPError("lld_pnp_batch_iterate", st)

    def find(self, active=None):
        """find() on every active solver: iterate(mRansacMaxIts) of each, continuing its state."""
        act = None
        if active is not None:
            self._act = np.ascontiguousarray(np.asarray(active, bool).astype(np.uint8))
            act = self._act.ctypes.data_as(c_uint8_p)
        st = self.lib.fn("pnp_batch_find")(self.handle, act)
        if st != abi.LLD_OK:
            raise PnPError("lld_pnp_batch_find", st)
        return self.download()

    def download(self):
        res = (PnPResult * self.n)()
        bufs = []
        for i, p in enumerate(self._p):
            b = np.zeros(max(p.n_keypoints, 1), np.uint8)
            bufs.append(b)
            res[i].inlier = b.ctypes.data_as(c_uint8_p)
        st = self.lib.fn("pnp_batch_download")(self.handle, res)
        if st != abi.LLD_OK:
            raise PnPError("lld_pnp_batch_download", st)
        out = []
        for i, p in enumerate(self._p):
            r = res[i]
            T = np.array(r.Tcw[:], np.float32).reshape(3, 4) if r.has_pose else None
            out.append(PnPOutput(T, bool(r.no_more), bufs[i][:p.n_keypoints].copy(), r.n_inliers, r.iterations, r.best_inliers))
        return out

    def hypotheses(self, solver, capacity=None):
        """Diagnostic: (n_window, n_run, records) of the last iterate call of one solver; records is a list of dicts with
        n_inliers, record, refine (-1 / 0 / 1), refined_inliers, R (3x3), t (3)."""
        cap = capacity if capacity is not None else MAX_ITERATIONS
        nw, nr = C.c_int32(), C.c_int32()
        st = self.lib.fn("pnp_batch_hypotheses")(self.handle, solver, 0, None, C.byref(nw), C.byref(nr))
        if st != abi.LLD_OK:
            raise PnPError("lld_pnp_batch_hypotheses", st)
        m = min(cap, nw.value)
        buf = (PnPHypothesis * max(m, 1))()
        st = self.lib.fn("pnp_batch_hypotheses")(self.handle, solver, m, buf, C.byref(nw), C.byref(nr))
        if st != abi.LLD_OK:
            raise PnPError("lld_pnp_batch_hypotheses", st)
        recs = [dict(n_inliers=h.n_inliers, record=h.record, refine=h.refine, refined_inliers=h.refined_inliers,
                     R=np.array(h.R[:]).reshape(3, 3), t=np.array(h.t[:])) for h in buf[:m]]
        return nw.value, nr.value, recs

    def close(self):
        if getattr(self, "handle", None):
            self.lib.fn("pnp_batch_destroy")(self.handle)
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


class PnPsolver(PnPsolverBatch):
    """One PnPsolver: iterate(n) -> PnPOutput and find() -> PnPOutput, both on this solver's state."""

    def __init__(self, ctx, problem, params=DEFAULT_PARAMS):
        super().__init__(ctx, [problem], params)
        self._problem = self._p[0]

    def iterate(self, nIterations=5):
        return super().iterate(nIterations)[0]

    def find(self):
        """find() (:159-163): iterate(mRansacMaxIts) continuing this solver's state, as the reference's find() does."""
        return super().find()[0]
