"""ORB-SLAM2's PnPsolver on the device (lld_pnp_*): a batch of independent solvers, one per relocalisation candidate, whose
RANSAC state stays in HBM between iterate() calls.  The rules and the two deviations are those of include/lld_amd.h."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ransac_batch import RansacBatch
from .abi import PnPHypothesis, PnPParams, PnPProblem, PnPResult, c_float_p, c_int32_p

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


class PnPsolverBatch(RansacBatch):
    """n PnPsolvers (PnPsolver(F, vpMapPointMatches) + SetRansacParameters) resident on the device.  Each problem is a dict
    with xyz, uv, sigma2, kp_index, n_keypoints, fx, fy, cx, cy, seed."""
    prefix, Error, max_iterations = "pnp", PnPError, MAX_ITERATIONS
    Problem, ProblemC, ResultC, HypothesisC = _Problem, PnPProblem, PnPResult, PnPHypothesis
    from_scene, make_params = staticmethod(problem_from_scene), staticmethod(_params)

    def __init__(self, ctx, problems, params=DEFAULT_PARAMS):
        super().__init__(ctx, problems, params)

    @staticmethod
    def n_flags(p):
        return p.n_keypoints

    @staticmethod
    def output(r, inliers):
        T = np.array(r.Tcw[:], np.float32).reshape(3, 4) if r.has_pose else None
        return PnPOutput(T, bool(r.no_more), inliers, r.n_inliers, r.iterations, r.best_inliers)

    def hypotheses(self, solver, capacity=None):
        """Diagnostic: (n_window, n_run, records) of the last iterate call of one solver; records is a list of dicts with
        n_inliers, record, refine (-1 / 0 / 1), refined_inliers, R (3x3), t (3)."""
        nw, nr, hyps = self._hypotheses(solver, capacity)
        return nw, nr, [dict(n_inliers=h.n_inliers, record=h.record, refine=h.refine, refined_inliers=h.refined_inliers,
                             R=np.array(h.R[:]).reshape(3, 3), t=np.array(h.t[:])) for h in hyps]


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
