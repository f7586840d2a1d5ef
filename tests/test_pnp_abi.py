"""lld_pnp_*: the structs of include/lld_amd.h against their ctypes mirrors (a C99 program compiled with -Werror prints sizeof
and offsetof), the limits and the exported symbols.  CPU only."""
import ctypes
import os
import subprocess

from lld_slam_amd import abi, pnp
from lld_slam_amd.abi import PnPHypothesis, PnPParams, PnPProblem, PnPResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lld_pnp_params_default", "lld_pnp_batch_create", "lld_pnp_batch_iterate", "lld_pnp_batch_download",
         "lld_pnp_batch_hypotheses", "lld_pnp_batch_destroy", "lld_pnp_find", "lld_pnp_batch_find"]


def test_pnp_symbols_are_listed_and_exported():
    assert all(n in abi.PRODUCT_SYMBOLS for n in NAMES)
    dll = ctypes.CDLL(abi.product_library_path())
    assert all(hasattr(dll, n) for n in NAMES)


def test_pnp_struct_layouts(tmp_path):
    structs = [("lld_pnp_params", PnPParams), ("lld_pnp_problem", PnPProblem), ("lld_pnp_result", PnPResult),
               ("lld_pnp_hypothesis", PnPHypothesis)]
    body, want = "", []
    for cname, py in structs:
        body += f'printf("%zu\\n", sizeof({cname}));'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'printf("%zu\\n", offsetof({cname}, {f}));'
            want.append(getattr(py, f).offset)
    body += 'printf("%d\\n%d\\n%d\\n%d\\n", LLD_PNP_MAX_CORRESPONDENCES, LLD_PNP_MAX_KEYPOINTS, LLD_PNP_MAX_SOLVERS, LLD_PNP_MAX_ITERATIONS);'
    want += [pnp.MAX_CORRESPONDENCES, pnp.MAX_KEYPOINTS, pnp.MAX_SOLVERS, pnp.MAX_ITERATIONS]
    src = tmp_path / "pnp.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "pnp"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


def test_pnp_params_default_is_relocalization():
    p = PnPParams()
    abi.product().fn("pnp_params_default")(ctypes.byref(p))
    assert (p.probability, p.min_inliers, p.max_iterations, p.min_set) == (0.99, 10, 300, 4)
    assert (ctypes.c_float(p.epsilon).value, ctypes.c_float(p.th2).value) == (ctypes.c_float(0.5).value, ctypes.c_float(5.991).value)
    assert pnp.DEFAULT_PARAMS[:4] == (0.99, 10, 300, 4)
