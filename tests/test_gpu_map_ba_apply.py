"""lld_map_ba_apply - the last third of Optimizer::LocalBundleAdjustment run on the resident map's tables - against the plain-Python
restatement (tests/map_ba_apply_ref.py, held to hand-worked scenes by tests/test_map_ba_apply_ref.py).  After every apply: the call's
outputs, all six row pools as the device holds them (lld_map_download_rows, every slot), the next BA window and covisibility with culling
for every keyframe must equal the restatement on its mutated map - bit for bit, floats included."""
import numpy as np
import pytest

import local_map_ref as LREF
import map_ba_apply_ref as A
import map_ba_apply_scenes as AS
import map_ba_ref as R
import map_ba_scenes as S
import map_covis_ref as M
from lld_slam_amd import abi, host, synth
from lld_slam_amd.device_map import DeviceMap

pytestmark = pytest.mark.gpu

K_GROUP = 16                 # kGroup of lld_map_apply.hip: lanes per window point
WAVEFRONT = 64
OUT = ("n_local_cams", "n_pt_obs_erased", "n_ln_obs_erased", "n_points_bad", "n_lines_bad", "n_index_skipped", "tcw", "ow", "pt_pos", "pt_normal", "pt_min_distance",
       "pt_max_distance", "pt_n_obs", "pt_ref_kf", "pt_row_len", "pt_flags", "ln_bad", "ln_n_obs", "ln_row_len")
RANDOM = [(0, 12), (1, 12), (4, 12), (5, 8)]           # seeds whose restated outcome shows every case (asserted in the test)


def se3(T):
    return host.se3_from_tcw_f32(abi.product(), T)


def tcw(qt):
    return host.se3_to_tcw_f32(abi.product(), qt)


def window_ref(m, q, sigma2=S.SIGMA2):
    return R.ba_window(m, q, sigma2, se3)


def same_window(got, ref, what):
    for c in R.COUNTS + ("status",):
        assert got[c] == ref[c], (what, c, got[c], ref[c])
    if ref["status"] == 0:
        for name in R.ARRAYS:
            assert got[name].tobytes() == ref[name].tobytes(), (what, name)


def same_out(got, exp, what):
    for k in OUT:
        g, e = got[k], exp[k]
        if isinstance(e, np.ndarray):
            assert g.dtype == e.dtype and g.shape == e.shape, (what, k, g.dtype, e.dtype, g.shape, e.shape)
            assert g.tobytes() == e.tobytes(), (what, k, g, e)
        else:
            assert g == e, (what, k, g, e)


def device_rows(dm):
    sl = AS.all_slots(dm)
    return {kind: dm.rows(kind, sl[which]) for kind, which in AS.POOLS}


def same_rows(dm, m, what):
    sl = AS.all_slots(dm)
    for kind, which in AS.POOLS:
        got, exp = dm.rows(kind, sl[which]), A.rows_of(m, kind, sl[which])
        assert got == exp, (what, kind, [(s, g, e) for s, g, e in zip(sl[which], got, exp) if g != e][:4])


def same_consumers(dm, m, q, what, sigma2=S.SIGMA2, cam=S.CAM):
    same_window(dm.ba_window(q, cam, sigma2), window_ref(m, q, sigma2), what + ": next window")
    kfs = sorted(m["keyframes"])
    got = dm.covisibility(kfs, culling=True, th=2)
    exp = M.covisibility(AS.covis_tables(m), kfs, culling=True, th=2)
    for k, e in exp.items():
        n = len(e)
        assert np.array_equal(got[k][:n], e), (what, "covisibility", k)


def apply_and_check(dm, m, q, res, what, sigma2=S.SIGMA2, cam=S.CAM, level_scale=AS.LEVEL_SCALE, assemble=True):
    """the window is assembled (unless the caller just did), the result applied, and everything held to the restatement; returns its map and outputs"""
    win = window_ref(m, q, sigma2)
    assert win["status"] == 0, what
    if assemble:
        same_window(dm.ba_window(q, cam, sigma2), win, what + ": window")
    m2, exp = A.apply(m, win, res, level_scale, tcw)
    got = dm.ba_apply(res, level_scale, n_local_cams=win["n_local_cams"])
    same_out(got, exp, what)
    same_rows(dm, m2, what)
    same_consumers(dm, m2, q, what, sigma2, cam)
    return m2, exp, win


def fresh(gpu_ctx, m, **over):
    dm = DeviceMap(gpu_ctx, **S.limits_for(m, **over))
    AS.upload(dm, m)
    return dm


# ---------------------------------------------------------------------------------------------------------------- random maps
@pytest.mark.parametrize("seed,n_kf", RANDOM)
def test_random_maps(gpu_ctx, seed, n_kf):
    m, q = S.random_map(seed, n_kf=n_kf)
    AS.complete(m, seed)
    win = window_ref(m, q)
    res = AS.crafted(win, seed, se3_from_tcw=se3)
    with fresh(gpu_ctx, m) as dm:
        m2, exp, _ = apply_and_check(dm, m, q, res, "seed %d" % seed)
    # the restatement alone shows every case
    flags = exp["pt_flags"]
    moved = [s for qq, s in enumerate(int(v) for v in win["point_slot"]) if not flags[qq] & A.WENT_BAD and m2["points"][s]["ref_kf"] != m["points"][s]["ref_kf"]]
    assert exp["n_points_bad"] > 0 and moved and exp["n_lines_bad"] > 0 and res.line_removed.sum() > 0
    assert (flags & A.REFRESHED).any() and (flags & A.NO_REFERENCE).any() and 0.1 < res.pt_obs_outlier.mean() < 0.2


# ---------------------------------------------------------------------------------------------------------------- the named scenes
@pytest.mark.parametrize("name", sorted(AS.NAMED))
def test_named_scenes(gpu_ctx, name):
    m, q, fl = AS.NAMED[name]()
    res = AS.flags_for(window_ref(m, q), **fl)
    with fresh(gpu_ctx, m) as dm:
        apply_and_check(dm, m, q, res, name)


def test_a_map_without_point_refs(gpu_ctx):
    """lld_map_set_point_refs never called: every reference is unknown, nothing is refreshed, everything else happens"""
    m, q = S.random_map(1)
    AS.complete(m, 1, refs=False)
    res = AS.crafted(window_ref(m, q), 1, se3_from_tcw=se3)
    with fresh(gpu_ctx, m) as dm:
        _, exp, _ = apply_and_check(dm, m, q, res, "no refs")
    assert not (exp["pt_flags"] & A.REFRESHED).any() and (exp["pt_flags"] & A.NO_REFERENCE).any() and (exp["pt_ref_kf"] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- widths
def erase_pattern(win, how):
    n = int(win["pt_obs_start"][1])                                         # the run of the wide point (window point 0)
    po = np.zeros(int(win["n_pt_obs"]), np.uint8)
    po[:n] = dict(first=[1] + [0] * (n - 1), last=[0] * (n - 1) + [1], every_other=[1, 0] * n, all=[1] * n)[how][:n]
    return po


@pytest.mark.parametrize("n_observers", [K_GROUP + 1, WAVEFRONT + 1])
@pytest.mark.parametrize("how", ["first", "last", "every_other", "all"])
def test_rows_one_past_a_width(gpu_ctx, n_observers, how):
    m, q = S.wide(n_observers=n_observers)
    AS.complete(m)
    m["points"][0]["ref_kf"] = m["points"][0]["obs"][0][0]                  # the first observer: erased by three of the four patterns
    # the observations the window holds (the bad observers' are not in it) weigh n_obs - 2: erasing all of them is what makes the point bad
    m["points"][0]["n_obs"] = 2 + sum(AS.stereo_weight(m, kf, i) for kf, i in m["points"][0]["obs"] if not m["keyframes"][kf]["bad"])
    win = window_ref(m, q)
    assert win["point_slot"][0] == 0 and win["pt_obs_start"][1] > n_observers * 0.8
    res = AS.flags_for(win); res["pt_obs_outlier"] = erase_pattern(win, how)
    res["pt_xyz"] = res["pt_xyz"] + 0.25
    with fresh(gpu_ctx, m) as dm:
        m2, exp, _ = apply_and_check(dm, m, q, res, "%d %s" % (n_observers, how))
    assert (exp["pt_flags"][0] & A.WENT_BAD != 0) == (how == "all") and len(m2["points"][0]["obs"]) == exp["pt_row_len"][0]


@pytest.mark.parametrize("n_points", [257, 512])
def test_more_window_points_than_a_workgroup_takes(gpu_ctx, n_points):
    m, q = S.wide(n_points=n_points)
    AS.complete(m)
    win = window_ref(m, q)
    assert win["n_points"] == n_points
    res = AS.crafted(win, n_points, frac=0.3, se3_from_tcw=se3)
    with fresh(gpu_ctx, m) as dm:
        _, exp, _ = apply_and_check(dm, m, q, res, "%d points" % n_points)
    assert exp["n_points_bad"] > 0 and exp["pt_flags"][-1] != 0


# ---------------------------------------------------------------------------------------------------------------- the host's bookkeeping
def churn(dm, pool, free_slots, room, moved_needed, observer):
    """rows of `room` entries set on slot after slot that never had a row and emptied again: every one goes to the pool's tail"""
    moved = 0
    for s in free_slots:
        if moved > moved_needed:
            return
        row = [(observer, 0)] * room
        if pool == "points":
            dm.set_observations_indexed([s], rows=[row], n_obs=[0]); dm.set_observations_indexed([s], rows=[[]], n_obs=[0])
        else:
            dm.set_line_observations([s], [row], [0]); dm.set_line_observations([s], [[]], [0])
        moved += room
    assert moved > moved_needed, (pool, moved, moved_needed)


def test_rows_survive_a_repack_and_freed_entries_can_be_used(gpu_ctx):
    seed = 0
    m, q = S.random_map(seed)
    AS.complete(m, seed)
    res = AS.crafted(window_ref(m, q), seed, se3_from_tcw=se3)
    free_pt = [s for s in range(512, 512 + 160)]; free_ln = [s for s in range(64, 64 + 60)]
    lim = S.limits_for(m, max_points=512 + 162, max_lines=64 + 62)
    observer = sorted(m["keyframes"])[0]
    live = lambda mm: (sum(len(p["obs"]) for p in mm["points"].values()), sum(len(l["obs"] or ()) for l in mm["lines"].values()))
    with DeviceMap(gpu_ctx, **lim) as dm:
        AS.upload(dm, m)
        m2, exp, _ = apply_and_check(dm, m, q, res, "before the churn")
        (p0, l0), (p1, l1) = live(m), live(m2)
        assert p1 < p0 and l1 < l0
        # the limits count what is left: a row that fits only because the apply freed its entries is accepted, one entry more is refused
        room_p, room_l = lim["max_observations"] - p1, lim["max_kf_lines"] - l1
        assert room_p > lim["max_observations"] - p0 and room_l > lim["max_kf_lines"] - l0
        dm.set_observations_indexed([free_pt[-1]], rows=[[(observer, 0)] * room_p], n_obs=[0])
        dm.set_line_observations([free_ln[-1]], [[(observer, 0)] * room_l], [0])
        before = device_rows(dm)
        for call in (lambda: dm.set_observations_indexed([free_pt[-2]], rows=[[(observer, 0)]], n_obs=[0]), lambda: dm.set_line_observations([free_ln[-2]], [[(observer, 0)]], [0])):
            with pytest.raises(RuntimeError) as e:
                call()
            assert e.value.status == abi.LLD_ERR_UNSUPPORTED
        assert device_rows(dm) == before
        dm.set_observations_indexed([free_pt[-1]], rows=[[]], n_obs=[0]); dm.set_line_observations([free_ln[-1]], [[]], [0])
        # both pools of the points' rows and both of the lines' are repacked from the host's copies (twice the limit is the pool) ...
        churn(dm, "points", free_pt[:-2], room_p, 2 * lim["max_observations"] - p0, observer)
        churn(dm, "lines", free_ln[:-2], room_l, 2 * lim["max_kf_lines"] - l0, observer)
        # ... and the keyframes' point and line rows, which hold the apply's -1 entries: every row is sent again, longer by one entry and back
        K = m2["keyframes"]
        for rounds in range(3):
            for s in sorted(K):
                for extra in ([-1], []):
                    k = K[s]
                    dm.set_keyframes([s], [k["key"]], [k["bad"]], [-1], [[]], [[]], [k["points"] + extra * (rounds + 1)], [k["lines"] + extra * (rounds + 1)])
                    kk = dict(k, octave=k["octave"] + [0] * len(extra) * (rounds + 1))
                    dm.set_keyframe_keypoints([s], [kk["octave"]], [[0.0] * len(kk["octave"])], [0.0])
                    pad = len(extra) * (rounds + 1)
                    dm.set_keyframe_features([s], [k["mn_id"]], [k["Tcw"]], [np.concatenate([k["uvr"], np.zeros((pad, 3), np.float32)])],
                                             [np.concatenate([k["kl_left"], np.zeros((pad, 4), np.float32)])], [np.concatenate([k["kl_right"], np.zeros((pad, 4), np.float32)])],
                                             [np.concatenate([k["kl_octave"], np.zeros((pad, 2), np.int32)])])
        same_rows(dm, m2, "after the churn")
        same_consumers(dm, m2, q, "after the churn")


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(gpu_ctx):
    m, q = S.random_map(4)
    AS.complete(m, 4)
    win = window_ref(m, q)
    res = AS.crafted(win, 4, se3_from_tcw=se3)
    counts = [int(win[k]) for k in ("n_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs")]

    def refused(dm, status=abi.LLD_ERR_INVALID, **kw):
        before = device_rows(dm)
        with pytest.raises(RuntimeError) as e:
            dm.ba_apply(res, AS.LEVEL_SCALE, n_local_cams=win["n_local_cams"], **kw)
        assert e.value.status == status
        assert device_rows(dm) == before

    with fresh(gpu_ctx, m) as dm:
        refused(dm)                                                         # no window was assembled
        with pytest.raises(RuntimeError):
            dm.ba_window(q, S.CAM, S.SIGMA2, capacities=[1, 1, 1, 1, 1])     # a short capacity: no complete window either
        refused(dm)
        dm.ba_window(q, S.CAM, S.SIGMA2)
        p = sorted(m["points"])[0]
        dm.set_point_refs([p], [m["points"][p]["ref_kf"]])                   # a setter between window and apply (it changes no value)
        refused(dm)
        dm.ba_window(q, S.CAM, S.SIGMA2)
        for k in range(5):                                                  # a count that is not the window's
            c = list(counts); c[k] += 1
            refused(dm, counts=c)
        f = dm.lib.fn("map_ba_apply")                                       # NULL arguments
        before = device_rows(dm)
        assert f(dm.handle, None, None) == abi.LLD_ERR_INVALID
        a, o = abi.MapBaApplyIn(), abi.MapBaApplyOut()
        a.n_cams, a.n_points, a.n_pt_obs, a.n_lines, a.n_ln_obs = counts
        a.n_levels = 4
        import ctypes
        assert f(dm.handle, ctypes.byref(a), ctypes.byref(o)) == abi.LLD_ERR_INVALID          # every array NULL
        assert device_rows(dm) == before
        # the window is still the map's: the apply goes through, and a second one of the same window does not
        m2, exp = A.apply(m, win, res, AS.LEVEL_SCALE, tcw)
        same_out(dm.ba_apply(res, AS.LEVEL_SCALE, n_local_cams=win["n_local_cams"]), exp, "after the refusals")
        refused(dm)
        same_rows(dm, m2, "after the refusals")
        # lld_map_download_rows: unknown kind, slot out of range, short capacity
        g = dm.lib.fn("map_download_rows")
        one = np.array([0], np.int32); st = np.zeros(2, np.int32); p32 = lambda x: x.ctypes.data_as(abi.c_int32_p)
        assert g(dm.handle, 6, 1, p32(one), p32(st), 0, None) == abi.LLD_ERR_INVALID
        far = np.array([dm.limits.max_points], np.int32)
        assert g(dm.handle, 0, 1, p32(far), p32(st), 0, None) == abi.LLD_ERR_INVALID
        s = next(s for s, p in m2["points"].items() if len(p["obs"]) > 1)
        assert g(dm.handle, 0, 1, p32(np.array([s], np.int32)), p32(st), 1, p32(one)) == abi.LLD_ERR_INVALID and st[1] == len(m2["points"][s]["obs"])
        # lld_map_set_point_refs: a reference out of range, a slot twice
        for slots, refs in (([s], [dm.limits.max_keyframes]), ([s], [-2]), ([s, s], [0, 0]), ([dm.limits.max_points], [0])):
            with pytest.raises(RuntimeError) as e:
                dm.set_point_refs(slots, refs)
            assert e.value.status == abi.LLD_ERR_INVALID
        same_rows(dm, m2, "after the refused setters")
        dm.clear()
        assert all(r == [] for rows in device_rows(dm).values() for r in rows)


# ---------------------------------------------------------------------------------------------------------------- with the solver
WINDOW = ("cam_qt", "pt_xyz", "pt_obs_start", "pt_obs_cam", "pt_obs_uvr", "pt_obs_inv_sigma2", "line_x0", "line_dir", "ln_obs_start", "ln_obs_cam", "ln_obs_left",
          "ln_obs_right", "ln_obs_octave")
RESULT = ("cam_qt", "pt_xyz", "line_x0", "line_dir", "pt_obs_outlier", "ln_edge_outlier", "line_removed")


def test_a_solved_window_applied_and_solved_again(gpu_ctx):
    w = synth.make_lba_small(0)
    m, q, table = S.map_of_window(w, 100)
    AS.complete(m, 100)
    scale = (np.float32(1.2) ** np.arange(len(table))).astype(np.float32)
    with fresh(gpu_ctx, m) as dm:
        bo, ids = dm.local_ba(q, w.cam, table)
        assert ids["status"] == 0 and bo.pt_obs_outlier.sum() > 0
        m2, exp, win = apply_and_check(dm, m, q, bo, "solved", sigma2=table, cam=w.cam, level_scale=scale, assemble=False)
        assert exp["n_pt_obs_erased"] > 0 and (exp["pt_flags"] & A.REFRESHED).sum() > 0.5 * win["n_points"]
        again, ids_again = dm.local_ba(q, w.cam, table)
    with fresh(gpu_ctx, m2) as dm:
        want, ids_want = dm.local_ba(q, w.cam, table)
    assert ids_again["status"] == 0 and ids_want["status"] == 0
    for k in ("cam_slot", "point_slot", "line_slot"):
        assert np.array_equal(ids_again[k], ids_want[k]), k
    for k in WINDOW:
        assert getattr(ids_again["window"], k).tobytes() == getattr(ids_want["window"], k).tobytes(), k
    for k in RESULT:
        assert getattr(again, k).tobytes() == getattr(want, k).tobytes(), k
    assert again.stats == want.stats


# ---------------------------------------------------------------------------------------------------------------- a consumer
def test_update_local_map_on_an_applied_map(gpu_ctx):
    from lld_slam_amd.tracking import DeviceTrackedFrame
    from test_gpu_local_map import one_frame, same as same_local_map
    seed = 5
    m, q = S.random_map(seed, n_kf=8)
    AS.complete(m, seed)
    win = window_ref(m, q)
    res = AS.crafted(win, seed, se3_from_tcw=se3)
    m2, exp = A.apply(m, win, res, AS.LEVEL_SCALE, tcw)
    went_bad = [int(s) for s, f in zip(win["point_slot"], exp["pt_flags"]) if f & A.WENT_BAD]
    alive = [s for s, p in m2["points"].items() if not p["bad"] and p["obs"]]
    ids = went_bad[:6] + alive[:40]
    every_pt = {s for k in m2["keyframes"].values() for s in k["points"] if s >= 0} | set(m2["points"])
    every_ln = {s for k in m2["keyframes"].values() for s in k["lines"] if s >= 0} | set(m2["lines"])
    lm = dict(keyframes={s: dict(k, parent=None, cov=[], child=[]) for s, k in m2["keyframes"].items()},
              points={s: dict(bad=m2["points"][s]["bad"], obs=[o[0] for o in m2["points"][s]["obs"]]) if s in m2["points"] else dict(bad=1, obs=[]) for s in every_pt},
              lines={s: m2["lines"][s] if s in m2["lines"] else dict(bad=1) for s in every_ln})
    lim = S.limits_for(m, max_local_points=1024, max_local_lines=128)
    want = LREF.update_local_map(LREF.new_state(), lm, ids, lim["max_local_points"], lim["max_local_lines"])
    assert want["n_bad_cleared"] == len(went_bad[:6]) > 0 and want["n_voted"] > 2                 # the bad points vote for nothing
    with DeviceTrackedFrame(gpu_ctx, synth.make_orb_frame(0, 256), synth.KITTI_CAM) as tf, DeviceMap(gpu_ctx, **lim) as dm:
        AS.upload(dm, m)
        dm.ba_window(q, S.CAM, S.SIGMA2)
        dm.ba_apply(res, AS.LEVEL_SCALE, n_local_cams=win["n_local_cams"])
        got, kept = one_frame(tf, dm, ids)
        same_local_map(got, kept, want, "applied map")
