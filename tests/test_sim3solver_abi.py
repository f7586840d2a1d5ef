"""lld_sim3solver_*: the structs of include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror prints
sizeof and offsetof), the limits and the exported symbols.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, sim3solver
from lld_slam_amd.abi import Sim3SolverHypothesis, Sim3SolverParams, Sim3SolverProblem, Sim3SolverResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_sim3solver_params_default", "lld_sim3solver_batch_create", "lld_sim3solver_batch_iterate",
         "lld_sim3solver_batch_find", "lld_sim3solver_batch_download", "lld_sim3solver_batch_hypotheses",
         "lld_sim3solver_batch_destroy", "lld_sim3solver_find"]


def test_sim3solver_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)


def test_sim3solver_struct_layouts(tmp_path):
    structs = [("lld_sim3solver_params", Sim3SolverParams), ("lld_sim3solver_problem", Sim3SolverProblem),
               ("lld_sim3solver_result", Sim3SolverResult), ("lld_sim3solver_hypothesis", Sim3SolverHypothesis)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += ('printf("%d\\n%d\\n%d\\n%d\\n", LLD_SIM3S_MAX_CORRESPONDENCES, LLD_SIM3S_MAX_KEYPOINTS, LLD_SIM3S_MAX_SOLVERS, '
             'LLD_SIM3S_MAX_ITERATIONS);')
    want += [sim3solver.MAX_CORRESPONDENCES, sim3solver.MAX_KEYPOINTS, sim3solver.MAX_SOLVERS, sim3solver.MAX_ITERATIONS]
    src = tmp_path / "sim3solver.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sim3solver"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


def test_sim3solver_params_default_is_loop_closing():
    p = Sim3SolverParams()
    abi.product().fn("sim3solver_params_default")(ctypes.byref(p))
    assert (p.probability, p.min_inliers, p.max_iterations) == (0.99, 20, 300)     # LoopClosing.cc:277, not the header's 6
    assert sim3solver.DEFAULT_PARAMS == (0.99, 20, 300)
