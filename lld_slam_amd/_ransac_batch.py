"""What the device-resident RANSAC batches (lld_pnp_batch_*, lld_sim3solver_batch_*) share on the Python side: the handle, the
status-checking call, the active mask, iterate / find / download, the two-call hypotheses fetch, close."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .abi import c_uint8_p


class RansacBatch:
    """A subclass sets the attributes below and defines from_scene(dict) -> Problem, make_params(tuple) -> the C params struct,
    n_flags(problem) -> the length of that solver's vbInliers, and output(result, inliers) -> its output dataclass."""
    prefix = None                   # "pnp": lld_pnp_batch_create, ...
    Error = RuntimeError            # raised as Error(entry point, status)
    Problem = None                  # the Python holder of one problem (its C struct in .c)
    ProblemC = ResultC = HypothesisC = None
    max_iterations = 0              # the most hypotheses one call can hold

    def __init__(self, ctx, problems, params):
        self.ctx = ctx
        self.lib = ctx.lib
        self._p = [p if isinstance(p, self.Problem) else self.from_scene(p) for p in problems]
        arr = (self.ProblemC * len(self._p))(*[p.c for p in self._p])
        self._params = self.make_params(params)
        h = C.c_void_p()
        self._call("create", ctx.handle, len(self._p), arr, C.byref(self._params), C.byref(h))
        self.handle = h
        self.n = len(self._p)

    def _call(self, name, *args):
        st = self.lib.fn(f"{self.prefix}_batch_{name}")(*args)
        if st != abi.LLD_OK:
            raise self.Error(f"lld_{self.prefix}_batch_{name}", st)

    def _active(self, active):
        if active is None:
            return None
        self._act = np.ascontiguousarray(np.asarray(active, bool).astype(np.uint8))
        return self._act.ctypes.data_as(c_uint8_p)

    def iterate(self, nIterations=5, active=None):
        """iterate(nIterations) on every active solver (one device-resident sequence); returns the outputs of all solvers
        (inactive ones keep their previous outputs)."""
        self.iterate_async(nIterations, active)
        return self.download()

    def iterate_async(self, nIterations=5, active=None):
        self._call("iterate", self.handle, int(nIterations), self._active(active))

    def find(self, active=None):
        """find() on every active solver: iterate(mRansacMaxIts) of each, continuing its state."""
        self._call("find", self.handle, self._active(active))
        return self.download()

    def download(self):
        res = (self.ResultC * self.n)()
        bufs = [np.zeros(max(self.n_flags(p), 1), np.uint8) for p in self._p]
        for r, b in zip(res, bufs):
            r.inlier = b.ctypes.data_as(c_uint8_p)
        self._call("download", self.handle, res)
        return [self.output(r, b[:self.n_flags(p)].copy()) for r, b, p in zip(res, bufs, self._p)]

    def _hypotheses(self, solver, capacity):
        """(n_window, n_run, HypothesisC records) of the last iterate call of one solver: the count first, then the records."""
        cap = capacity if capacity is not None else self.max_iterations
        nw, nr = C.c_int32(), C.c_int32()
        self._call("hypotheses", self.handle, solver, 0, None, C.byref(nw), C.byref(nr))
        m = min(cap, nw.value)
        buf = (self.HypothesisC * max(m, 1))()
        self._call("hypotheses", self.handle, solver, m, buf, C.byref(nw), C.byref(nr))
        return nw.value, nr.value, buf[:m]

    def close(self):
        if getattr(self, "handle", None):
            self.lib.fn(f"{self.prefix}_batch_destroy")(self.handle)
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
