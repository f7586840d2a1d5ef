"""lld_map_fuse - ORBmatcher::Fuse(pKF, vpMapPoints, th) on the resident map's tables - against the plain-Python restatement
(tests/map_fuse_ref.py, held to paper scenes by tests/test_map_fuse_ref.py) and, for the search, against lld_orb_fuse_search on the inputs
gathered from the same model.  After every call: match, action, other, the counts and the survivors, then all six row pools, the fixed
point rows and Observations() over EVERY slot of the map - bit for bit - so that a row nobody named is seen not to have changed."""
import copy
import ctypes as C

import numpy as np
import pytest

import map_ba_apply_ref as A
import map_ba_apply_scenes as AS
import map_ba_scenes as S
import map_fuse_ref as F
import map_fuse_scenes as FS
import map_refresh_scenes as RS
from lld_slam_amd import abi, orb_search, synth
from lld_slam_amd.device_map import DeviceMap

pytestmark = pytest.mark.gpu

FIXED = ("pos", "normal", "min_distance", "max_distance", "desc", "state")


def fresh(gpu_ctx, m, **over):
    dm = DeviceMap(gpu_ctx, **FS.limits(m, **over))
    RS.upload(dm, m)
    return dm


def device_state(dm):
    sl = AS.all_slots(dm)
    return {kind: dm.rows(kind, sl[which]) for kind, which in AS.POOLS}, dm.download_points(sl["pt"]), dm.point_counts(sl["pt"])


def model_points(m, slots):
    P = m["points"]
    z = lambda s, k, d: P[s].get(k, d) if s in P else d
    return dict(pos=np.array([z(s, "pos", np.zeros(3)) for s in slots], np.float32).reshape(-1, 3), normal=np.array([z(s, "nrm", np.zeros(3)) for s in slots], np.float32).reshape(-1, 3),
                min_distance=np.array([z(s, "mind", 0) for s in slots], np.float32), max_distance=np.array([z(s, "maxd", 0) for s in slots], np.float32),
                desc=np.array([z(s, "desc", np.zeros(8)) for s in slots], np.uint32).reshape(-1, 8),
                state=np.array([0 if s not in P else 2 if P[s]["bad"] else 1 for s in slots], np.uint8))


def same_state(dm, m, what):
    sl = AS.all_slots(dm)
    rows, pts, cnt = device_state(dm)
    for kind, which in AS.POOLS:
        exp = A.rows_of(m, kind, sl[which])
        assert rows[kind] == exp, (what, kind, [(s, g, e) for s, g, e in zip(sl[which], rows[kind], exp) if g != e][:4])
    exp = model_points(m, sl["pt"])
    for k in FIXED:
        assert pts[k].tobytes() == exp[k].tobytes(), (what, k, [s for s in sl["pt"] if pts[k][s].tobytes() != exp[k][s].tobytes()][:6])
    assert np.array_equal(cnt, F.counts_of(m, sl["pt"])), (what, "n_obs", np.flatnonzero(cnt != F.counts_of(m, sl["pt"]))[:6])


def unchanged(dm, before, what):
    rows, pts, cnt = device_state(dm)
    assert rows == before[0], what
    assert all(pts[k].tobytes() == before[1][k].tobytes() for k in FIXED) and np.array_equal(cnt, before[2]), what


def old_route(gpu_ctx, m, c, slots, th):
    """lld_orb_fuse_search on what a caller without the resident map gathers"""
    kf, mp = F.gathered(m, c["target"], slots)
    KF = orb_search.Frame(kf["desc"], kf["xy"], kf["octave"], kf["uright"], np.zeros(len(kf["octave"]), np.float32), 0.0, 0.0, FS.WIDTH, FS.HEIGHT,
                          FS.SCALE, (FS.SCALE * FS.SCALE).astype(np.float32), FS.INV_SIGMA2)
    out, _ = orb_search.fuse_search_points(gpu_ctx.lib, gpu_ctx.handle, KF, FS.view_struct(c["view"]), mp, th)
    return out.match


def call(dm, c, slots=None, th=3.0, **kw):
    return dm.fuse(c["target"], FS.view_struct(c["view"]), c["grid"], c["level_scale"], c["inv_sigma2"], point_slot=slots, th=th, **kw)


def fuse_checked(gpu_ctx, dm, m, c, slots, what, th=3.0, source_keyframe=-1):
    """one call held to the restatement, its search to lld_orb_fuse_search, and the whole map to the restatement's; returns the model behind it"""
    m2, exp = FS.run_ref(m, c, slots, th, source_keyframe)
    listed = list(m["keyframes"][source_keyframe]["points"]) if source_keyframe >= 0 else slots
    old = old_route(gpu_ctx, m, c, listed, th)
    got = call(dm, c, None if source_keyframe >= 0 else slots, th, source_keyframe=source_keyframe, n_points=len(listed))
    assert np.array_equal(got["match"], old), (what, "match against lld_orb_fuse_search", np.flatnonzero(got["match"] != old)[:6])
    for k in ("match", "action", "other", "survivor"):
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])
    for k in ("n_fused", "n_added", "n_replaced"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    same_state(dm, m2, what)
    return m2, exp


# ---------------------------------------------------------------------------------------------------------------- 1. the paper scenes
@pytest.mark.parametrize("name", sorted(FS.PAPER))
def test_paper_scenes(gpu_ctx, name):
    m, c, slots, want = FS.PAPER[name]()
    with fresh(gpu_ctx, m) as dm:
        same_state(dm, m, name + ": uploaded")
        m2, exp = fuse_checked(gpu_ctx, dm, m, c, slots, name)
    assert exp["action"].tolist() == want["action"] and exp["match"].tolist() == want["match"]
    assert exp["other"].tolist() == want["other"] and exp["survivor"].tolist() == want["survivor"]


# ---------------------------------------------------------------------------------------------------------------- 2. shapes
# fu_search_kernel: one wavefront per candidate and four per workgroup (lists of 1, 4, 5: one workgroup, exactly one, one more), 64 lanes
# striding over the target's keypoints (1, 63, 64, 65 and 257: a second and a fifth trip)
@pytest.mark.parametrize("n_target,n_cand", [(1, 1), (63, 4), (64, 5), (65, 64), (257, 65), (65, 257)])
def test_random_maps_at_every_width(gpu_ctx, n_target, n_cand):
    big = n_target >= 63 and n_cand >= 64
    m, c, slots = FS.random_scene(100, n_target, n_cand, check=big)      # (a seed whose restated outcome takes every action at the three big sizes)
    with fresh(gpu_ctx, m) as dm:
        m2, exp = fuse_checked(gpu_ctx, dm, m, c, slots, "%d x %d" % (n_target, n_cand))
        if big:
            assert exp["n_fused"] * 4 >= n_cand and set(exp["action"].tolist()) >= {1, 2, 3, 4, 5}
            assert -1 in slots and len(set(slots)) < len(slots) and any(s >= 0 and s not in m["points"] for s in slots) and any(s in m["points"] and m["points"][s]["bad"] for s in slots)
        # a second fuse on the same map: the first one's survivors and losers are candidates and holders now
        again = [s for s in slots if s >= 0][::-1] + [int(s) for s in exp["survivor"]]
        fuse_checked(gpu_ctx, dm, m2, c, again, "%d x %d again" % (n_target, n_cand))


def test_source_keyframe_against_the_same_list_uploaded(gpu_ctx):
    m, c, slots = FS.random_scene(5, 65, 65)
    # the candidates are the row of the keyframe with the most points: -1 entries, bad points, points already in the target
    src = max((s for s in m["keyframes"] if s != c["target"]), key=lambda s: len(m["keyframes"][s]["points"]))
    row = list(m["keyframes"][src]["points"])
    with fresh(gpu_ctx, m) as dm:
        m2, exp = fuse_checked(gpu_ctx, dm, m, c, None, "source keyframe", source_keyframe=src)
    assert exp["n_fused"] > 4
    with fresh(gpu_ctx, m) as dm:
        m3, exp3 = fuse_checked(gpu_ctx, dm, m, c, row, "the same list uploaded")
    for k in exp:
        assert np.array_equal(exp[k], exp3[k]), k


def test_observation_rows_of_1_17_and_65_move(gpu_ctx):
    m, c, slots, what = FS.rows_scene((1, 17, 65))
    with fresh(gpu_ctx, m) as dm:
        m2, exp = fuse_checked(gpu_ctx, dm, m, c, slots, "rows")
    assert exp["action"].tolist() == [a for _, a in what]
    for s, h, (L, a) in zip(slots, exp["other"], what):
        loser, surv = (s, int(h)) if a == F.CANDIDATE_REPLACED else (int(h), s)
        assert len(m["points"][loser]["obs"]) == L and m2["points"][loser]["obs"] == [] and len(m2["points"][surv]["obs"]) >= L
    lens = [len(m2["points"][int(s)]["obs"]) for s in exp["survivor"]]
    assert len(lens) == 6 and min(lens) <= 64 < max(lens)                  # both descriptor kernels ran


def test_a_survivor_row_at_the_limit_and_one_beyond(gpu_ctx):
    m, c, slots = FS.limit_scene(False)
    with fresh(gpu_ctx, m) as dm:
        m2, exp = fuse_checked(gpu_ctx, dm, m, c, slots, "at the limit")
        assert len(m2["points"][slots[0]]["obs"]) == abi.LANDMARK_MAX_OBS and exp["survivor"].tolist() == slots
    m, c, slots = FS.limit_scene(True)
    assert FS.run_ref(m, c, slots)[1] is None
    with fresh(gpu_ctx, m) as dm:
        before = device_state(dm)
        with pytest.raises(RuntimeError, match="lld_map_fuse") as e:
            call(dm, c, slots)
        assert e.value.status == abi.LLD_ERR_UNSUPPORTED
        unchanged(dm, before, "one beyond the limit")


# ---------------------------------------------------------------------------------------------------------------- 3. where a grown row goes
def burn(dm, free_slots, amount, observer):
    """`amount` entries at the tails of the observation and index pools are used up and freed again: a row set on a free slot and emptied"""
    for s, n in zip(free_slots, amount):
        dm.set_observations_indexed([s], rows=[[(observer, 0)] * n], n_obs=[0]); dm.set_observations_indexed([s], rows=[[]], n_obs=[0])


def test_a_grown_row_in_place_at_the_tail_and_behind_a_repack(gpu_ctx):
    """RowPool places a row in its old place when it fits the capacity the row once had, at the pool's tail otherwise, and repacks the pool
    when the tail is used up (the pools hold twice their limit).  Three maps, one call each, the same outcome: only the placement differs."""
    m, c, slots, _ = FS.same_keypoint_twice()
    A_, B_ = slots
    live = sum(len(p["obs"]) for p in m["points"].values())                  # 3
    spare = 8
    lim = FS.limits(m, spare_points=spare, max_observations=live + 6)        # the pools: 2 (live + 6) = 18 entries
    free = list(range(lim["max_points"] - spare, lim["max_points"]))
    # 1. in place: both rows were longer once
    with DeviceMap(gpu_ctx, **lim) as dm:
        RS.upload(dm, m)
        dm.set_observations_indexed([A_, B_], rows=[m["points"][A_]["obs"] + [(0, 0)] * 2, m["points"][B_]["obs"] + [(0, 0)] * 2], n_obs=[0, 0])
        dm.set_observations_indexed([A_, B_], rows=[m["points"][A_]["obs"], m["points"][B_]["obs"]], n_obs=[m["points"][A_]["n_obs"], m["points"][B_]["n_obs"]])
        fuse_checked(gpu_ctx, dm, m, c, slots, "in place")
    # 2. at the tail: what every other test of this file does - a fresh row has no room to grow
    with DeviceMap(gpu_ctx, **lim) as dm:
        RS.upload(dm, m)
        fuse_checked(gpu_ctx, dm, m, c, slots, "at the tail")
    # 3. behind a repack: the tail stands at 3; 6 + 6 burnt entries leave 3 free, the call's rows (A: 0 entries, B: 4) need 4 at the tail
    with DeviceMap(gpu_ctx, **lim) as dm:
        RS.upload(dm, m)
        burn(dm, free[:2], [6, 6], observer=1)
        assert 2 * lim["max_observations"] - (live + 12) < 4
        m2, _ = fuse_checked(gpu_ctx, dm, m, c, slots, "behind a repack")
        # ... and the repacked pools take rows again
        dm.set_observations_indexed([free[2]], rows=[[(1, 0)] * 5], n_obs=[0]); dm.set_observations_indexed([free[2]], rows=[[]], n_obs=[0])
        same_state(dm, m2, "after the repack")


# ---------------------------------------------------------------------------------------------------------------- 4. the consumers
def same_window(a, b, what):
    for k in ("n_cams", "n_free_cams", "n_local_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs", "status"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    if a["status"] == 0:
        for name, _, _, _ in DeviceMap.BA_ARRAYS:
            assert a[name].tobytes() == b[name].tobytes(), (what, name)


def test_the_fused_map_serves_covisibility_the_ba_window_and_the_local_map(gpu_ctx):
    from lld_slam_amd.tracking import DeviceTrackedFrame
    from test_gpu_local_map import one_frame
    m, c, slots = FS.random_scene(8, 65, 65)
    kfs = sorted(m["keyframes"])
    q = kfs[:4]
    sig = FS.INV_SIGMA2
    lim = dict(max_local_points=2048)
    with fresh(gpu_ctx, m, **lim) as dm, DeviceTrackedFrame(gpu_ctx, synth.make_orb_frame(0, 256), synth.KITTI_CAM) as tf:
        w = dm.ba_window(q, S.CAM, sig)                                     # a window staged before the fuse ...
        assert w["status"] == 0 and w["n_points"] > 0
        m2, exp = fuse_checked(gpu_ctx, dm, m, c, slots, "before the consumers")
        assert exp["n_replaced"] > 2 and exp["n_added"] > 2
        with pytest.raises(RuntimeError, match="lld_map_ba_apply") as e:    # ... is stale behind it
            dm.ba_apply(AS.flags_for(w), FS.SCALE, n_local_cams=w["n_local_cams"])
        assert e.value.status == abi.LLD_ERR_INVALID
        ids = [int(s) for s in exp["survivor"][:20]] + [s for s, p in m2["points"].items() if p["bad"]][:10] + [s for s, p in m2["points"].items() if not p["bad"]][:60]
        got = dm.covisibility(kfs, culling=True, th=1), dm.ba_window(q, S.CAM, sig), one_frame(tf, dm, ids)
        with fresh(gpu_ctx, m2, **lim) as dm2:                              # a fresh map sent the restatement's rows
            want = dm2.covisibility(kfs, culling=True, th=1), dm2.ba_window(q, S.CAM, sig), one_frame(tf, dm2, ids)
            dm2.ba_apply(AS.flags_for(want[1]), FS.SCALE, n_local_cams=want[1]["n_local_cams"])      # (a window nothing came after is applied)
    for k in want[0]:
        assert np.array_equal(got[0][k], want[0][k]), ("covisibility", k)
    assert want[0]["conn_weight"].size > 0
    same_window(got[1], want[1], "window")
    (lm_got, kept_got), (lm_want, kept_want) = got[2], want[2]
    assert np.array_equal(kept_got, kept_want) and lm_want["n_voted"] > 2 and lm_want["n_bad_cleared"] > 0
    for k in ("status", "n_voted", "n_bad_cleared", "ref_keyframe", "vote_empty", "n_local_keyframes", "n_local_points", "n_local_lines"):
        assert lm_got[k] == lm_want[k], ("local map", k)
    for k in ("local_keyframes", "local_points"):
        assert np.array_equal(lm_got[k], lm_want[k]), ("local map", k)


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_change_nothing(gpu_ctx):
    m, c, slots = FS.random_scene(10, 65, 65)
    tg = c["target"]
    other = next(s for s in m["keyframes"] if s != tg)
    never_kf = max(m["keyframes"]) + 1
    with fresh(gpu_ctx, m) as dm:
        before = device_state(dm)
        view = FS.view_struct(c["view"])

        def refused(status=abi.LLD_ERR_INVALID, **kw):
            a = dict(target=tg, view=view, grid=c["grid"], level_scale=c["level_scale"], level_inv_sigma2=c["inv_sigma2"], point_slot=slots)
            a.update(kw)
            with pytest.raises(RuntimeError, match="lld_map_fuse") as e:
                dm.fuse(**a)
            assert e.value.status == status, (kw, e.value.status)
            unchanged(dm, before, kw)
            return e.value

        refused(target=-1); refused(target=dm.limits.max_keyframes); refused(target=never_kf)                    # out of range, never set
        refused(n_points=-1)
        refused(point_slot=slots[:-1] + [dm.limits.max_points]); refused(point_slot=slots[:-1] + [-2])           # a slot out of range
        refused(source_keyframe=other)                                                                           # both
        refused(point_slot=None, n_points=3)                                                                     # neither
        refused(point_slot=None, source_keyframe=never_kf, n_points=0); refused(point_slot=None, source_keyframe=other, n_points=1 + len(m["keyframes"][other]["points"]))
        refused(th=0.0); refused(th=-3.0)
        for k in ("fx", "fy"):
            v = FS.view_struct(dict(c["view"], **{k: 0.0}))
            refused(view=v)
        refused(level_scale=c["level_scale"][:4], level_inv_sigma2=c["inv_sigma2"][:4])                          # not the view's n_levels
        refused(grid=c["grid"][:4] + (0, 48))
        e = refused(survivor_capacity=0)                                                                         # fewer than the call needs
        assert e.n_survivors == len(FS.run_ref(m, c, slots)[1]["survivor"]) > 0
        f = dm.lib.fn("map_fuse")
        a, o = abi.MapFuseIn(), abi.MapFuseOut()
        assert f(dm.handle, None, C.byref(o)) == abi.LLD_ERR_INVALID and f(dm.handle, C.byref(a), None) == abi.LLD_ERR_INVALID
        unchanged(dm, before, "NULL arguments")
        # n_points = 0 is fine and touches nothing
        got = call(dm, c, [])
        assert got["n_fused"] == 0 and len(got["match"]) == 0
        unchanged(dm, before, "n_points = 0")
        fuse_checked(gpu_ctx, dm, m, c, slots, "after the refusals")
    # a target whose descriptor row is missing
    m_nd = copy.deepcopy(m); del m_nd["keyframes"][tg]["desc"]
    with fresh(gpu_ctx, m_nd) as dm:
        before = device_state(dm)
        with pytest.raises(RuntimeError) as e:
            call(dm, c, slots)
        assert e.value.status == abi.LLD_ERR_INVALID
        unchanged(dm, before, "no descriptor rows")
    # a live total beyond the limit: two adds where the observation pools have room for what the map holds and one entry more
    m, c, slots, _ = FS.add_stereo_and_mono()
    live = sum(len(p["obs"]) for p in m["points"].values())
    assert sum(len(p["obs"]) for p in FS.run_ref(m, c, slots)[0]["points"].values()) == live + 2
    with fresh(gpu_ctx, m, max_observations=live + 1) as dm:
        before = device_state(dm)
        with pytest.raises(RuntimeError) as e:
            call(dm, c, slots)
        assert e.value.status == abi.LLD_ERR_UNSUPPORTED
        unchanged(dm, before, "beyond the limit")
        fuse_checked(gpu_ctx, dm, m, c, slots[:1], "one add fits")
