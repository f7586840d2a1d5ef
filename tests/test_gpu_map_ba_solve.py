"""lld_map_local_ba - the window assembled on the resident map and solved in one call - against lld_local_ba on the window the
plain-Python restatement (tests/map_ba_ref.py) assembles from the same map.  The two windows are byte-equal, so with the default
deterministic = 2 the project's bit-reproducibility is the bar: poses, positions, outlier flags and statistics must be identical."""
import numpy as np
import pytest

import map_ba_ref as R
import map_ba_scenes as S
from lld_slam_amd import abi, host, synth
from lld_slam_amd.device_map import DeviceMap

pytestmark = pytest.mark.gpu

WINDOW = ("cam_qt", "pt_xyz", "pt_obs_start", "pt_obs_cam", "pt_obs_uvr", "pt_obs_inv_sigma2", "line_x0", "line_dir", "ln_obs_start", "ln_obs_cam", "ln_obs_left",
          "ln_obs_right", "ln_obs_octave")
RESULT = ("cam_qt", "pt_xyz", "line_x0", "line_dir", "pt_obs_outlier", "ln_edge_outlier", "line_removed")


def window_of(ref, cam):
    return host.Window(cam, ref["n_free_cams"], *[ref[k] for k in WINDOW])


@pytest.fixture(scope="module")
def solved(gpu_ctx):
    """per window id: the map, the query, the restatement's window and lld_local_ba's answer on it - computed once"""
    out = {}
    for wid in (0, 1):
        w = synth.make_lba_small(wid)
        m, q, table = S.map_of_window(w, 100 + wid)
        ref = R.ba_window(m, q, table, lambda T: host.se3_from_tcw_f32(abi.product(), T))
        assert ref["status"] == 0 and ref["n_free_cams"] == w.n_free_cams and ref["n_cams"] == w.n_cams and ref["n_lines"] > 0
        win = window_of(ref, w.cam)
        out[wid] = dict(m=m, q=q, table=table, ref=ref, cam=w.cam, want=host.Optimizer(gpu_ctx).LocalBundleAdjustment(win),
                        want_stopped=host.Optimizer(gpu_ctx).LocalBundleAdjustment(win, pbStopFlag=True))
    return out


def same_solution(got, ids, sc, want):
    ref = sc["ref"]
    assert ids["status"] == 0 and ids["n_local_cams"] == ref["n_local_cams"]
    for k in ("cam_slot", "point_slot", "line_slot"):
        assert np.array_equal(ids[k], ref[k]), k
    assert ids["window"].n_free_cams == ref["n_free_cams"] and tuple(ids["window"].cam) == tuple(float(v) for v in sc["cam"])
    for k in WINDOW:
        assert getattr(ids["window"], k).tobytes() == ref[k].tobytes(), k
    for k in RESULT:
        assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), k
    assert got.stats == want.stats


@pytest.mark.parametrize("wid", [0, 1])
def test_map_local_ba_equals_local_ba_on_the_restated_window(gpu_ctx, solved, wid):
    sc = solved[wid]
    with DeviceMap(gpu_ctx, **S.limits_for(sc["m"])) as dm:
        S.upload(dm, sc["m"])
        got, ids = dm.local_ba(sc["q"], sc["cam"], sc["table"])
        same_solution(got, ids, sc, sc["want"])
        assert got.stats["lm_iterations"][0] > 0 and not got.stats["aborted"]
        # the map's tables were not changed: the second call (which finds its buffers large enough) gives the same
        got, ids = dm.local_ba(sc["q"], sc["cam"], sc["table"])
        same_solution(got, ids, sc, sc["want"])


def test_stop_flag_up_before_the_call(gpu_ctx, solved):
    sc = solved[0]
    with DeviceMap(gpu_ctx, **S.limits_for(sc["m"])) as dm:
        S.upload(dm, sc["m"])
        got, ids = dm.local_ba(sc["q"], sc["cam"], sc["table"], stop=True)
        same_solution(got, ids, sc, sc["want_stopped"])
        assert got.stats["aborted"] == 1 and got.stats["lm_iterations"] == [0, 0] and got.stats["lm_trials"] == [0, 0]


def test_missing_feature_data_solves_nothing(gpu_ctx, solved):
    sc = solved[0]
    with DeviceMap(gpu_ctx, **S.limits_for(sc["m"])) as dm:
        S.upload_keyframes(dm, sc["m"], features=False); S.upload_points(dm, sc["m"]); S.upload_lines(dm, sc["m"])
        got, ids = dm.local_ba(sc["q"], sc["cam"], sc["table"])
        assert got is None and ids["status"] == abi.MAP_BA_NO_FEATURE_DATA


@pytest.mark.parametrize("name,want", [("bad_neighbour", []), ("bad_observer_inside", [1]), ("never_set_observer", [1, 4])])
def test_bad_keyframes_marked_fixed_are_reported(gpu_ctx, name, want):
    """marked_bad_slot, in no order: the bad observers (a slot never set is one) the walk marks fixed without making them cameras; a bad
    neighbour is marked local and is none of them.  The stop flag is up: the window is assembled, nothing is solved."""
    m, q = S.NAMED[name]()
    ref = R.ba_window(m, q, S.SIGMA2, lambda T: host.se3_from_tcw_f32(abi.product(), T))
    assert ref["marked_bad"] == want
    with DeviceMap(gpu_ctx, **S.limits_for(m)) as dm:
        S.upload(dm, m)
        got, ids = dm.local_ba(q, S.CAM, S.SIGMA2, stop=True)
        assert ids["status"] == 0 and np.array_equal(ids["cam_slot"], ref["cam_slot"]) and np.array_equal(ids["point_slot"], ref["point_slot"])
        assert sorted(ids["marked_bad_slot"].tolist()) == want
