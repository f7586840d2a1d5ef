"""examples/map_ba_apply_host.cpp - the tail of LocalBundleAdjustment as a host runs it on flat tables, the route a caller has without
lld_map_ba_apply - compiled with the host compiler into a stand-alone program and held to tests/map_ba_apply_ref.py on the named scenes and
on the random maps of the GPU tests, bit for bit: outputs and all six row tables.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import map_ba_apply_ref as A
import map_ba_apply_scenes as AS
import map_ba_ref as R
import map_ba_scenes as S
from lld_slam_amd import abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("n_local_cams", "n_pt_obs_erased", "n_ln_obs_erased", "n_points_bad", "n_lines_bad", "n_index_skipped", "tcw", "ow", "pt_pos", "pt_normal", "pt_min_distance",
       "pt_max_distance", "pt_n_obs", "pt_ref_kf", "pt_row_len", "pt_flags", "ln_bad", "ln_n_obs", "ln_row_len")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("map_ba_apply_host") / "check"
    ex = os.path.join(ROOT, "examples")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ex, "map_ba_apply_host_check.cpp"),
                           os.path.join(ex, "map_ba_apply_host.cpp")])
    return str(exe)


def scenes():
    for name in sorted(AS.NAMED):
        yield name
    for seed, n_kf in [(0, 12), (1, 12), (4, 12), (5, 8)]:
        yield (seed, n_kf)


@pytest.mark.parametrize("which", list(scenes()), ids=str)
def test_the_host_tail_equals_the_restatement(program, tmp_path, which):
    lib = abi.product()
    se3 = lambda T: host.se3_from_tcw_f32(lib, T)
    tcw = lambda qt: host.se3_to_tcw_f32(lib, qt)
    if isinstance(which, str):
        m, q, fl = AS.NAMED[which]()
        win = R.ba_window(m, q, S.SIGMA2, se3)
        res = AS.flags_for(win, **fl)
    else:
        m, q = S.random_map(which[0], n_kf=which[1])
        AS.complete(m, which[0])
        win = R.ba_window(m, q, S.SIGMA2, se3)
        res = AS.crafted(win, which[0], se3_from_tcw=se3)
    limits = S.limits_for(m)
    m2, exp = A.apply(m, win, res, AS.LEVEL_SCALE, tcw)
    scene, answer = str(tmp_path / "scene.bin"), str(tmp_path / "answer.bin")
    AS.write_scene(scene, m, q, win, res, exp["tcw"], limits)
    subprocess.check_call([program, scene, answer])
    got, rows = AS.read_answer(answer, win, limits)
    for k in OUT:
        g, e = got[k], exp[k]
        if isinstance(e, np.ndarray):
            assert g.dtype == e.dtype and g.tobytes() == e.tobytes(), (which, k, g, e)
        else:
            assert g == e, (which, k, g, e)
    sl = dict(kf=range(limits["max_keyframes"]), pt=range(limits["max_points"]), ln=range(limits["max_lines"]))
    for kind, w in AS.POOLS:
        assert rows[kind] == A.rows_of(m2, kind, sl[w]), (which, kind)
