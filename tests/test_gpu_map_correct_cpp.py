"""The C++ route to the loop-closing thread's map corrections: examples/loop_correct_harness builds KeyFrame / MapPoint / Map test
doubles from a scene file, runs adapters/lld_loopclosing_adapter.cc on them (gather in pointer order, ONE device call, scatter) and,
on a second copy of the objects, the host route: the reference's loop in compiled C++ with UpdateNormalAndDepth through
RefreshMapPoints.  The members after the adapter must equal tests/loopcorr_ref.py's within the bars of test_gpu_map_correct.py, and
the adapter's objects must equal the host route's object for object within the same bars."""
import os
import subprocess

import numpy as np
import pytest

import loopcorr_ref as R
import loopcorr_scenes as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "loop_correct_harness")
f32 = np.float32


def run_harness(tmp_path, kind, sc):
    assert os.path.exists(HARNESS), "examples/loop_correct_harness is built by build()"
    blob, sc = S.object_scene_blob(kind, sc)
    (tmp_path / "scene.bin").write_bytes(blob)
    out = subprocess.run([HARNESS, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    adapter, host = S.read_object_dump(str(tmp_path / "out.bin"))
    return sc, adapter, host


def adjacent(a, b, what):
    steps = R.ulp_steps(a, b)
    print(f"{what}: {int((steps > 0).sum())} of {steps.size} values differ")
    assert steps.max() <= 1, what


def same_objects(adapter, host, once_rounded=("tcw", "pos"), doubles=("corrected", "non_corrected"), scale=1.0):
    """Object for object: integers and marks exact, the floats that are one double rounded once equal or adjacent, the Sim3 doubles
    within 1e-13 x scale, everything else bit for bit on equal inputs - checked as equal or adjacent too, since an adjacent
    position may move a normal by its own rounding."""
    for k in ("corrected_by", "corrected_ref", "kf_gba_mark", "has_corrected", "has_non_corrected", "n_set_pos", "n_set_pose"):
        assert np.array_equal(adapter[k], host[k]), k
    for k in once_rounded:
        adjacent(adapter[k], host[k], "adapter against host route: " + k)
    for k in doubles:
        assert np.abs(adapter[k] - host[k]).max() <= 1e-13 * scale, k
    if all(R.bits_equal(adapter[k], host[k]) for k in once_rounded):
        for k in ("ow", "normal", "min_distance", "max_distance", "tcw_gba", "tcw_before"):
            assert R.bits_equal(adapter[k], host[k]), k
    else:
        for k in ("ow", "normal", "min_distance", "max_distance", "tcw_gba", "tcw_before"):
            adjacent(adapter[k], host[k], "adapter against host route: " + k)


def test_correct_loop_on_objects(gpu_ctx, tmp_path):
    sc, adapter, host = run_harness(tmp_path, 1, S.make_loop_scene(81, n_kf=12, n_conn=5, cur_rank=3, per_kf=40, s=0.7))
    exp = R.correct_loop_literal(sc)
    conn, own = sc["conn"], exp["corrected_by"]
    tmax = max(1.0, float(np.abs(exp["corrected_sim3"][:, 4:7]).max()))
    # keyframes: SetPose once for the connected ones, Ow written with it, the two maps filled for exactly them
    in_conn = np.zeros(12, bool); in_conn[conn] = True
    assert np.array_equal(adapter["has_corrected"], in_conn) and np.array_equal(adapter["has_non_corrected"], in_conn)
    assert np.array_equal(adapter["n_set_pose"], in_conn.astype(np.int64))
    adjacent(adapter["tcw"][conn], exp["tiw_corrected"], "tiw")
    assert R.bits_equal(adapter["tcw"][~in_conn], sc["kf_tcw"][~in_conn])
    assert R.bits_equal(adapter["ow"], np.array([R.centre_of(T) for T in adapter["tcw"]], f32).reshape(-1, 3))
    assert np.abs(adapter["corrected"][conn] - exp["corrected_sim3"]).max() <= 1e-13 * tmax
    assert np.abs(adapter["non_corrected"][conn] - exp["non_corrected_sim3"]).max() <= 1e-13 * tmax
    # points: mnCorrectedByKF = the current keyframe's id (slot + 1), mnCorrectedReference = the owner's id
    cur_id = conn[sc["cur"]] + 1
    moved = own >= 0
    assert np.array_equal(adapter["corrected_by"][moved], np.full(moved.sum(), cur_id))
    assert np.array_equal(adapter["corrected_by"][~moved], np.where(sc["already"][~moved] != 0, cur_id, 0))
    assert np.array_equal(adapter["corrected_ref"][moved], conn[own[moved]] + 1) and (adapter["corrected_ref"][~moved] == 0).all()
    assert np.array_equal(adapter["n_set_pos"], moved.astype(np.int64))
    adjacent(adapter["pos"], exp["pos"], "pos")
    normal, mn, mx, _ = R.loop_normals(sc, own, adapter["pos"], adapter["ow"][conn])
    assert R.bits_equal(adapter["normal"], normal) and R.bits_equal(adapter["min_distance"], mn) and R.bits_equal(adapter["max_distance"], mx)
    same_objects(adapter, host, scale=tmax)


def test_essential_graph_on_objects(gpu_ctx, tmp_path):
    sc, adapter, host = run_harness(tmp_path, 2, S.make_graph_scene(82, n_kf=10, n=150))
    exp = R.essential_graph_literal(sc)
    adjacent(adapter["tcw"], exp["tiw"], "tiw")
    assert (adapter["n_set_pose"] == 1).all()
    assert R.bits_equal(adapter["ow"], np.array([R.centre_of(T) for T in adapter["tcw"]], f32).reshape(-1, 3))
    adjacent(adapter["pos"], exp["pos"], "pos")
    assert np.array_equal(adapter["n_set_pos"], (sc["bad"] == 0).astype(np.int64))
    normal, mn, mx, _ = R.graph_normals(sc, adapter["pos"], adapter["ow"])
    assert R.bits_equal(adapter["normal"], normal) and R.bits_equal(adapter["min_distance"], mn) and R.bits_equal(adapter["max_distance"], mx)
    same_objects(adapter, host, doubles=())


def test_global_ba_update_on_objects(gpu_ctx, tmp_path):
    sc, adapter, host = run_harness(tmp_path, 3, S.make_gba_scene(83))
    exp = R.global_ba_literal(sc)
    v = exp["visited"] != 0
    assert np.array_equal(adapter["kf_gba_mark"] == 77, v) and np.array_equal(adapter["n_set_pose"], v.astype(np.int64))
    assert R.bits_equal(adapter["tcw"][v], exp["tcw_new"][v]) and R.bits_equal(adapter["tcw"][~v], sc["kf_tcw"][~v])
    assert R.bits_equal(adapter["tcw_gba"][v], exp["tcw_new"][v]) and R.bits_equal(adapter["tcw_before"][v], exp["tcw_before"][v])
    assert R.bits_equal(adapter["ow"][v], exp["ow_new"][v])
    assert R.bits_equal(adapter["pos"], exp["pos"]) and np.array_equal(adapter["n_set_pos"], (exp["moved"] != 0).astype(np.int64))
    for k in ("tcw", "ow", "tcw_gba", "tcw_before", "pos", "kf_gba_mark", "n_set_pose", "n_set_pos"):
        assert R.bits_equal(adapter[k], host[k]), k
