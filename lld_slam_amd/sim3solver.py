"""ORB-SLAM2's Sim3Solver on the device (lld_sim3solver_*): a batch of independent solvers, one per loop candidate, whose RANSAC
state stays in HBM between iterate() calls.  The rules and the two deviations are those of include/lld_amd.h."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ransac_batch import RansacBatch
from .abi import Sim3SolverHypothesis, Sim3SolverParams, Sim3SolverProblem, Sim3SolverResult, c_float_p, c_int32_p

MAX_CORRESPONDENCES = 8192   # LLD_SIM3S_MAX_CORRESPONDENCES
MAX_KEYPOINTS = 8192         # LLD_SIM3S_MAX_KEYPOINTS
MAX_SOLVERS = 256            # LLD_SIM3S_MAX_SOLVERS
MAX_ITERATIONS = 65536       # LLD_SIM3S_MAX_ITERATIONS
DEFAULT_PARAMS = (0.99, 20, 300)     # SetRansacParameters as LoopClosing::ComputeSim3 calls it (LoopClosing.cc:277)


class Sim3SolverError(RuntimeError):
    def __init__(self, what, status):
        super().__init__(f"{what} failed with status {status}")
        self.status = status


@dataclass
class Sim3SolverOutput:
    """iterate()'s return: T12 (3x4 float32 [sR | t]) or None, bNoMore, vbInliers (uint8[n1]), nInliers, the solver's
    mnIterations / mnBestInliers after the call, and GetEstimatedRotation / Translation / Scale (the best hypothesis)."""
    T12: np.ndarray | None
    no_more: bool
    inliers: np.ndarray
    n_inliers: int
    iterations: int
    best_inliers: int
    R: np.ndarray
    t: np.ndarray
    s: float


def _params(params):
    p = Sim3SolverParams()
    p.probability, p.min_inliers, p.max_iterations = params
    return p


class _Problem:
    """One solver's correspondences, kept alive for the C struct."""

    def __init__(self, xyz1, xyz2, sigma2_1, sigma2_2, index1, n1, Rcw1, tcw1, Rcw2, tcw2, K1, K2, fix_scale, seed=0):
        self.xyz1 = np.ascontiguousarray(xyz1, np.float32).reshape(-1)
        self.xyz2 = np.ascontiguousarray(xyz2, np.float32).reshape(-1)
        self.sigma2_1 = np.ascontiguousarray(sigma2_1, np.float32).reshape(-1)
        self.sigma2_2 = np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        self.index1 = np.ascontiguousarray(index1, np.int32).reshape(-1)
        self.n1 = int(n1)
        c = Sim3SolverProblem()
        c.n = len(self.index1)
        c.xyz1 = self.xyz1.ctypes.data_as(c_float_p); c.xyz2 = self.xyz2.ctypes.data_as(c_float_p)
        c.sigma2_1 = self.sigma2_1.ctypes.data_as(c_float_p); c.sigma2_2 = self.sigma2_2.ctypes.data_as(c_float_p)
        c.index1 = self.index1.ctypes.data_as(c_int32_p)
        c.n1 = self.n1
        for dst, src, m in (("Rcw1", Rcw1, 9), ("tcw1", tcw1, 3), ("Rcw2", Rcw2, 9), ("tcw2", tcw2, 3)):
            getattr(c, dst)[:] = [float(v) for v in np.asarray(src, np.float32).reshape(m)]
        c.fx1, c.fy1, c.cx1, c.cy1 = (float(v) for v in K1)
        c.fx2, c.fy2, c.cx2, c.cy2 = (float(v) for v in K2)
        c.fix_scale = 1 if fix_scale else 0
        c.seed = int(seed) & 0xFFFFFFFF
        self.c = c


def problem_from_scene(sc):
    return _Problem(sc["xyz1"], sc["xyz2"], sc["sigma2_1"], sc["sigma2_2"], sc["index1"], sc["n1"], sc["Rcw1"], sc["tcw1"],
                    sc["Rcw2"], sc["tcw2"], sc["K1"], sc["K2"], sc["fix_scale"], sc["seed"])


class Sim3SolverBatch(RansacBatch):
    """n Sim3Solvers (Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) + SetRansacParameters) resident on the device.  Each
    problem is a dict with xyz1, xyz2, sigma2_1, sigma2_2, index1, n1, Rcw1, tcw1, Rcw2, tcw2, K1, K2, fix_scale, seed."""
    prefix, Error, max_iterations = "sim3solver", Sim3SolverError, MAX_ITERATIONS
    Problem, ProblemC, ResultC, HypothesisC = _Problem, Sim3SolverProblem, Sim3SolverResult, Sim3SolverHypothesis
    from_scene, make_params = staticmethod(problem_from_scene), staticmethod(_params)

    def __init__(self, ctx, problems, params=DEFAULT_PARAMS):
        super().__init__(ctx, problems, params)

    @staticmethod
    def n_flags(p):
        return p.n1

    @staticmethod
    def output(r, inliers):
        T = np.array(r.T12[:], np.float32).reshape(3, 4) if r.has_pose else None
        return Sim3SolverOutput(T, bool(r.no_more), inliers, r.n_inliers, r.iterations, r.best_inliers,
                                np.array(r.R[:], np.float32).reshape(3, 3), np.array(r.t[:], np.float32), np.float32(r.s))

    def hypotheses(self, solver, capacity=None):
        """Diagnostic: (n_window, n_run, records) of the last iterate call of one solver; records is a list of dicts with
        n_inliers, record, idx (3), s, R (3x3), t (3), T12 (3x4), all floats as float32."""
        nw, nr, hyps = self._hypotheses(solver, capacity)
        return nw, nr, [dict(n_inliers=h.n_inliers, record=h.record, idx=list(h.idx), s=np.float32(h.s),
                             R=np.array(h.R[:], np.float32).reshape(3, 3), t=np.array(h.t[:], np.float32),
                             T12=np.array(h.T12[:], np.float32).reshape(3, 4)) for h in hyps]


class Sim3Solver(Sim3SolverBatch):
    """One Sim3Solver: iterate(n) and find() -> Sim3SolverOutput on this solver's state, and the reference's getters."""

    def __init__(self, ctx, problem, params=DEFAULT_PARAMS):
        super().__init__(ctx, [problem], params)
        self._last = None

    def iterate(self, nIterations=5):
        self._last = super().iterate(nIterations)[0]
        return self._last

    def find(self):
        """find() (:209-213): iterate(mRansacMaxIts) continuing this solver's state, as the reference's find() does."""
        self._last = super().find()[0]
        return self._last

    def _state(self):
        return self._last if self._last is not None else self.download()[0]

    def GetEstimatedRotation(self):
        return self._state().R.copy()

    def GetEstimatedTranslation(self):
        return self._state().t.copy()

    def GetEstimatedScale(self):
        return float(self._state().s)
