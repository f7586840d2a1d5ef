"""lld_map_ba_window - the window of Optimizer::LocalBundleAdjustment assembled on the resident map - against the plain-Python restatement on
map tables (tests/map_ba_ref.py, held to a transcription of the reference's walk and to hand-worked windows by tests/test_map_ba_ref.py).
Every array of the device's window must equal the restatement's byte for byte: integers, doubles copied through, and floats widened."""
import copy

import numpy as np
import pytest

import map_ba_ref as R
import map_ba_scenes as S
from lld_slam_amd import abi, host
from lld_slam_amd.device_map import DeviceMap

pytestmark = pytest.mark.gpu

FILL = 0xA5
# the widths lld_map_ba.hip fixes
K_SCAN_TILE = 256            # kScanTile: entries one workgroup of ba_scan_kernel scans at a time
K_GROUP = 16                 # kGroup: lanes that walk one landmark's row in ba_visit_kernel / ba_fill_kernel
WAVEFRONT = 64


def se3(T):
    return host.se3_from_tcw_f32(abi.product(), T)


def ref_of(m, q, dm=None):
    return R.ba_window(m, q, S.SIGMA2, se3, max_keyframes=None if dm is None else dm.limits.max_keyframes)


def same(got, ref, what=""):
    for c in R.COUNTS + ("status",):
        assert got[c] == ref[c], (what, c, got[c], ref[c])
    if ref["status"] == 0:
        for name in R.ARRAYS:
            assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape, (what, name, got[name].shape, ref[name].shape)
            assert got[name].tobytes() == ref[name].tobytes(), (what, name, got[name], ref[name])


def untouched(raw):
    return all(np.all(a.view(np.uint8) == FILL) for a in raw.values())


def run(dm, m, q, what="", **kw):
    got = dm.ba_window(q, S.CAM, S.SIGMA2, fill=FILL, **kw)
    ref = ref_of(m, q, dm)
    same(got, ref, what)
    return got, ref


def check(gpu_ctx, m, q, what=""):
    with DeviceMap(gpu_ctx, **S.limits_for(m)) as dm:
        S.upload(dm, m)
        return run(dm, m, q, what)


@pytest.mark.parametrize("seed,n_kf", [(0, 12), (1, 12), (2, 9), (3, 6), (4, 12), (5, 8)])
def test_random_maps(gpu_ctx, seed, n_kf):
    m, q = S.random_map(seed, n_kf=n_kf)
    got, ref = check(gpu_ctx, m, q)
    assert got["n_points"] > 20 and got["n_pt_obs"] > got["n_points"] and got["n_lines"] > 0 and got["n_cams"] > got["n_local_cams"]


@pytest.mark.parametrize("name", sorted(S.NAMED))
def test_named_scenes(gpu_ctx, name):
    m, q = S.NAMED[name]()
    got, ref = check(gpu_ctx, m, q, name)
    if name in S.HAND:                                                   # ... and the device gives the hand-worked lists themselves
        e = S.HAND[name]
        for k in ("cam_slot", "point_slot", "pt_obs_start", "pt_obs_cam", "line_slot", "ln_obs_start", "ln_obs_cam"):
            assert got[k].tolist() == e[k], (name, k)


@pytest.mark.parametrize("kw", [dict(n_points=K_SCAN_TILE + 1), dict(n_points=2 * K_SCAN_TILE), dict(n_observers=K_GROUP + 1), dict(n_observers=WAVEFRONT + 1),
                                dict(n_line_observers=K_GROUP + 1), dict(n_line_observers=WAVEFRONT + 1), dict(n_local=abi.MAP_BA_MAX_LOCAL)],
                         ids=lambda k: "%s%d" % next(iter(k.items())))
def test_one_past_every_width(gpu_ctx, kw):
    m, q = S.wide(**kw)
    got, ref = check(gpu_ctx, m, q, str(kw))
    if "n_points" in kw: assert got["n_points"] == kw["n_points"]
    # the stored rows are one past the width; every seventh / ninth observer is bad and left out of the run
    if "n_observers" in kw: assert got["pt_obs_start"][1] == sum(s % 7 != 3 for s in range(kw["n_observers"])) and got["n_cams"] > 3
    if "n_line_observers" in kw:
        assert got["n_ln_obs"] == sum(s % 9 != 4 for s in range(kw["n_line_observers"])) and np.all(np.diff(got["ln_obs_cam"][:-3]) < 0)   # mn_id descends along the row
    if "n_local" in kw: assert got["n_local_cams"] > 900 and got["n_cams"] == got["n_local_cams"] + 1


def test_refusals_change_nothing(gpu_ctx):
    m, q = S.random_map(0)
    with DeviceMap(gpu_ctx, **S.limits_for(m)) as dm:
        S.upload(dm, m)
        never = next(s for s in range(dm.limits.max_keyframes) if s not in m["keyframes"])
        wide_m, wide_q = S.wide(n_local=abi.MAP_BA_MAX_LOCAL)
        for bad_q in ([], [q[0], q[1], q[0]], [q[0], dm.limits.max_keyframes], [q[0], -1], [never], list(range(abi.MAP_BA_MAX_LOCAL + 1))):
            with pytest.raises(RuntimeError) as e:
                dm.ba_window(bad_q, S.CAM, S.SIGMA2, fill=FILL)
            assert e.value.status == abi.LLD_ERR_INVALID and e.value.counts is None and untouched(e.value.raw), bad_q
        with pytest.raises(RuntimeError) as e:
            dm.ba_window(q, S.CAM, [], fill=FILL)
        assert e.value.status == abi.LLD_ERR_INVALID
        with pytest.raises(RuntimeError) as e:
            dm.ba_window(q, S.CAM, S.SIGMA2, capacities=[4, -1, 4, 4, 4], fill=FILL)
        assert e.value.status == abi.LLD_ERR_INVALID
        run(dm, m, q)
    # one keyframe more than LLD_MAP_BA_MAX_LOCAL, all of them set
    with DeviceMap(gpu_ctx, **S.limits_for(wide_m)) as dm:
        S.upload(dm, wide_m)
        with pytest.raises(RuntimeError) as e:
            dm.ba_window(list(range(abi.MAP_BA_MAX_LOCAL + 1)), S.CAM, S.SIGMA2)
        assert e.value.status == abi.LLD_ERR_INVALID


def spoil(m, how):
    """fixed_through_line with one piece of feature data missing; returns what to upload again to repair it"""
    K = m["keyframes"]
    if how == "camera_without_features": del K[2]["uvr"]
    if how == "camera_without_keypoints": K[2]["octave"] = None
    if how == "feature_row_of_another_length": K[1]["points"] = K[1]["points"] + [-1]
    if how == "keyline_row_of_another_length": K[3]["lines"] = K[3]["lines"] + [-1]
    if how == "point_index_outside_the_row": m["points"][0]["obs"][2] = (2, 2)
    if how == "octave_outside_the_table": K[1]["octave"][0] = S.N_LEVELS
    if how == "point_row_without_indices": m["points"][0]["indexed"] = False
    if how == "line_without_a_row": m["lines"][0]["obs"] = None
    if how == "line_index_outside_the_row": m["lines"][0]["obs"][0] = (3, 2)


SPOILS = ["camera_without_features", "camera_without_keypoints", "feature_row_of_another_length", "keyline_row_of_another_length", "point_index_outside_the_row",
          "octave_outside_the_table", "point_row_without_indices", "line_without_a_row", "line_index_outside_the_row"]


@pytest.mark.parametrize("how", SPOILS)
def test_missing_feature_data_is_a_status_not_a_window(gpu_ctx, how):
    good, q = S.fixed_through_line()
    m = copy.deepcopy(good)
    spoil(m, how)
    with DeviceMap(gpu_ctx, **S.limits_for(good, max_kf_points=64, max_kf_lines=64)) as dm:
        if how.endswith("of_another_length"):                            # the rows grow after the features were set: the feature rows are stale
            S.upload(dm, good); S.upload_keyframes(dm, m, keypoints=False, features=False)
        else:
            S.upload(dm, m)
        got = dm.ba_window(q, S.CAM, S.SIGMA2, fill=FILL)
        assert got["status"] == abi.MAP_BA_NO_FEATURE_DATA and all(got[c] == 0 for c in R.COUNTS) and untouched(got["raw"]), how
        assert ref_of(m, q)["status"] == R.NO_FEATURE_DATA
        # the map is as it was: with the missing piece sent, the window is the good map's
        S.upload(dm, good)
        run(dm, good, q, how)


def test_a_map_without_any_feature_table(gpu_ctx):
    m, q = S.bad_neighbour()
    with DeviceMap(gpu_ctx, **S.limits_for(m)) as dm:
        S.upload_keyframes(dm, m, keypoints=False, features=False); S.upload_points(dm, m)
        got = dm.ba_window(q, S.CAM, S.SIGMA2, fill=FILL)
        assert got["status"] == abi.MAP_BA_NO_FEATURE_DATA and untouched(got["raw"])
        with pytest.raises(RuntimeError) as e:
            dm.ba_window([0, 0], S.CAM, S.SIGMA2)
        assert e.value.status == abi.LLD_ERR_INVALID
        S.upload(dm, m)
        run(dm, m, q)


def test_capacity_protocol(gpu_ctx):
    m, q = S.random_map(1)
    ref = ref_of(m, q)
    exact = [ref[c] for c in DeviceMap.BA_COUNTS]
    with DeviceMap(gpu_ctx, **S.limits_for(m)) as dm:
        S.upload(dm, m)
        for k in range(5):
            caps = list(exact); caps[k] -= 1
            with pytest.raises(RuntimeError) as e:
                dm.ba_window(q, S.CAM, S.SIGMA2, capacities=caps, fill=FILL)
            assert e.value.status == abi.LLD_ERR_INVALID and untouched(e.value.raw), k
            assert all(e.value.counts[c] == ref[c] for c in R.COUNTS), (k, e.value.counts)
        with pytest.raises(RuntimeError) as e:
            dm.ba_window(q, S.CAM, S.SIGMA2, capacities=[0] * 5, fill=FILL)
        assert all(e.value.counts[c] == ref[c] for c in R.COUNTS)
        run(dm, m, q, capacities=exact)
        run(dm, m, q, capacities=[c + 7 for c in exact])
        run(dm, m, q)                                                   # the wrapper's own short call, then the exact one


def test_rows_replaced_between_two_calls(gpu_ctx):
    m, q = S.random_map(4)
    rng = np.random.default_rng(7)
    with DeviceMap(gpu_ctx, **S.limits_for(m)) as dm:
        S.upload(dm, m)
        first, _ = run(dm, m, q)
        # a BA moved poses
        moved = [int(s) for s in first["cam_slot"][:3]]
        for s in moved: m["keyframes"][s]["Tcw"] = S.random_pose(rng)
        dm.set_keyframe_poses(moved, [m["keyframes"][s]["Tcw"] for s in moved])
        second, _ = run(dm, m, q, "poses")
        assert second["cam_qt"].tobytes() != first["cam_qt"].tobytes()
        # a point turned bad
        p = int(first["point_slot"][5])
        m["points"][p]["bad"] = 1
        S.upload_points(dm, m, [p])
        third, _ = run(dm, m, q, "bad point")
        assert third["n_points"] == second["n_points"] - 1
        # an observation erased: EraseMapPointMatch and EraseObservation
        p = int(third["point_slot"][0])
        kf, idx = m["points"][p]["obs"].pop(0)
        m["keyframes"][kf]["points"][idx] = -1
        S.upload_points(dm, m, [p]); S.upload_keyframes(dm, m, [kf], keypoints=False, features=False)
        run(dm, m, q, "erased observation")
        # a line's row and a keyframe's features replaced by longer ones
        l = int(third["line_slot"][0])
        extra = next(s for s in m["keyframes"] if s not in [o[0] for o in m["lines"][l]["obs"]])
        m["lines"][l]["obs"].append((extra, 0)); m["lines"][l]["n_obs"] += 1
        S.upload_lines(dm, m, [l])
        run(dm, m, q, "longer line row")
        # Map::clear and a fresh upload
        dm.clear()
        S.upload(dm, m)
        run(dm, m, q, "after clear")


def test_setters_refuse_before_anything_changes(gpu_ctx):
    m, q = S.fixed_through_line()
    K = m["keyframes"]
    with DeviceMap(gpu_ctx, **S.limits_for(m)) as dm:
        S.upload_keyframes(dm, m, features=False); S.upload_points(dm, m); S.upload_lines(dm, m)
        feat = lambda s, k: dm.set_keyframe_features(s, [k_["mn_id"] for k_ in k], [k_["Tcw"] for k_ in k], [k_["uvr"] for k_ in k], [k_["kl_left"] for k_ in k],
                                                     [k_["kl_right"] for k_ in k], [k_["kl_octave"] for k_ in k])

        def refused(call):
            with pytest.raises(RuntimeError) as e:
                call()
            assert e.value.status == abi.LLD_ERR_INVALID
        refused(lambda: dm.set_keyframe_poses([0], [K[0]["Tcw"]]))                                  # no features yet
        short = dict(K[0], uvr=K[0]["uvr"][:0])
        refused(lambda: feat([0], [short]))                                                          # a keypoint row of another length
        lines_short = dict(K[0], kl_left=K[0]["kl_left"][:0], kl_right=K[0]["kl_right"][:0], kl_octave=K[0]["kl_octave"][:0])
        refused(lambda: feat([0], [lines_short]))
        refused(lambda: feat([4], [K[0]]))                                                           # a keyframe never set
        refused(lambda: feat([0, 0], [K[0], K[0]]))
        refused(lambda: dm.set_line_observations([0], [[(0, -1)]], [4]))
        refused(lambda: dm.set_line_observations([0], [[(99, 0)]], [4]))
        refused(lambda: dm.set_line_observations([0], [[(0, 0)]], [-1]))
        refused(lambda: dm.set_line_observations([0, 0], [[], []], [4, 4]))
        S.upload_keyframes(dm, m, rows=False, keypoints=False)
        refused(lambda: dm.set_keyframe_poses([0, 4], [K[0]["Tcw"]] * 2))
        run(dm, m, q)
