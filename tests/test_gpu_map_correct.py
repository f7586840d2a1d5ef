"""lld_loop_correct / lld_essential_graph_apply / lld_global_ba_apply on the device against tests/loopcorr_ref.py, the sequential
restatement in the reference's loop order, and against the routes that existed before them (the host loop with one
lld_mappoint_refresh per connected keyframe).

Bars: every integer and flag is exact.  Everything of the global-BA update is bit for bit (float products in the gemm rule).  Ow, normal
and the distances are bit for bit against the restatement evaluated on the device's own returned float poses and positions.  The Sim3
doubles are within 1e-13 x max(1, the largest |translation| of the scene): fewer than about 40 double operations at 1.1e-16 each on
operands of that size.  Positions, tiw and scw_f32 are each one double rounded once to float: equal or the adjacent float; the count of
values that are not bit-equal is printed (and expected to be 0: the device code is compiled without contraction)."""
import ctypes as C
import functools

import numpy as np
import pytest

import loopcorr_ref as R
import loopcorr_scenes as S
from lld_slam_amd import abi
from lld_slam_amd.landmarks import MAX_OBS, NORMAL_DEPTH, refresh_map_points
from lld_slam_amd.loop_correction import MOVED, LoopCorrectionError, apply_essential_graph, apply_global_ba, correct_loop

pytestmark = pytest.mark.gpu
f32 = np.float32
POINTS = ("pos", "bad", "obs_start", "obs_kf", "ref_kf", "ref_level", "level_scale")
PRIOR = ("normal", "min_distance", "max_distance")


def loop_args(sc):
    return [sc[k] for k in ("kf_tcw", "conn", "cur", "scw", "kf_start", "kf_point", "pos", "bad", "already", "obs_start", "obs_kf", "ref_kf",
                            "ref_level", "level_scale")], {k: sc[k] for k in PRIOR}


def run_loop(ctx, sc):
    a, kw = loop_args(sc)
    return correct_loop(ctx, *a, **kw)


def graph_args(sc):
    return [sc[k] for k in ("sim3_before", "sim3_after", "corr_kf") + POINTS], {k: sc[k] for k in PRIOR}


def run_graph(ctx, sc):
    a, kw = graph_args(sc)
    return apply_essential_graph(ctx, *a, **kw)


def gba_args(sc):
    return [sc[k] for k in ("kf_tcw", "kf_in_gba", "kf_tcw_gba", "parent", "origins", "pos", "bad", "in_gba", "pos_gba", "ref_kf")]


def once_rounded(got, exp, what):
    """One double rounded once to float on either side: equal or adjacent.  Prints how many are not bit-equal."""
    steps = R.ulp_steps(got, exp)
    print(f"{what}: {int((steps > 0).sum())} of {steps.size} values differ from the restatement (largest {int(steps.max()) if steps.size else 0} float steps)")
    assert steps.size == 0 or steps.max() <= 1, what
    return int((steps > 0).sum())


def sim3_close(got, exp, scale, what):
    assert np.abs(got - exp).max() <= 1e-13 * max(1.0, scale), what


def check_loop(got, sc, what):
    exp = R.correct_loop_literal(sc)
    assert np.array_equal(got.corrected_by, exp["corrected_by"]) and np.array_equal(got.updated, exp["updated"]), what
    tmax = float(np.abs(exp["corrected_sim3"][:, 4:7]).max())
    sim3_close(got.corrected_sim3, exp["corrected_sim3"], tmax, what + " corrected_sim3")
    sim3_close(got.non_corrected_sim3, exp["non_corrected_sim3"], tmax, what + " non_corrected_sim3")
    differ = once_rounded(got.tiw_corrected, exp["tiw_corrected"], what + " tiw") + once_rounded(got.scw_f32, exp["scw_f32"], what + " scw_f32")
    differ += once_rounded(got.pos, exp["pos"], what + " pos")
    # on the device's own poses and positions: bit for bit
    assert R.bits_equal(got.ow_corrected, np.array([R.centre_of(T) for T in got.tiw_corrected], f32).reshape(-1, 3)), what
    normal, mn, mx, did = R.loop_normals(sc, got.corrected_by, got.pos, got.ow_corrected)
    assert np.array_equal(did, (got.updated & NORMAL_DEPTH) != 0), what
    assert R.bits_equal(got.normal, normal) and R.bits_equal(got.min_distance, mn) and R.bits_equal(got.max_distance, mx), what
    still = (got.updated & MOVED) == 0                         # an entry the rule leaves alone keeps its input value
    assert R.bits_equal(got.pos[still], sc["pos"][still]) and (got.corrected_by[still] == -1).all(), what
    return exp, differ


# ------------------------------------------------------------------------------------------------------------------ loop 1
def test_loop_current_keyframe_alone(gpu_ctx):
    sc = S.make_loop_scene(11, n_kf=4, n_conn=1, cur_rank=0, per_kf=40, s=0.7)
    exp, _ = check_loop(run_loop(gpu_ctx, sc), sc, "n_conn = 1")
    assert (exp["corrected_by"] == 0).sum() > 10
    assert R.bits_equal(exp["corrected_sim3"][0], sc["scw"])


@pytest.mark.parametrize("s", [1.0, 0.7])
@pytest.mark.parametrize("cur", [0, 2, 4])
def test_loop_five_connected_keyframes(gpu_ctx, cur, s):
    """12 keyframes in the table, 5 connected, 40 points each; a point held by three connected keyframes, a slot listed twice, bad,
    already-corrected and observation-free points; reference keyframes at a rank below, at and above the owner's and outside conn."""
    sc = S.make_loop_scene(20 + cur, n_kf=12, n_conn=5, cur_rank=cur, per_kf=40, s=s)
    lists = [set(sc["kf_point"][sc["kf_start"][r]:sc["kf_start"][r + 1]].tolist()) for r in range(5)]
    assert 0 in lists[0] & lists[1] & lists[2]
    assert (sc["kf_point"][:sc["kf_start"][1]] == 1).sum() == 2
    exp, _ = check_loop(run_loop(gpu_ctx, sc), sc, f"cur {cur} s {s}")
    own = exp["corrected_by"]
    listed = np.zeros(len(own), bool); listed[sc["kf_point"]] = True
    assert (listed & (sc["bad"] != 0)).any() and (listed & (sc["already"] != 0)).any()
    noobs = np.diff(sc["obs_start"]) == 0
    assert (exp["updated"][noobs & (own >= 0)] == MOVED).all() and (noobs & (own >= 0)).any()
    rank = np.full(12, 99); rank[sc["conn"]] = np.arange(5)
    ref_rank = rank[sc["ref_kf"]]
    live = (own >= 0) & ~noobs
    for rel in (ref_rank[live] < own[live], ref_rank[live] == own[live], (ref_rank[live] > own[live]) & (ref_rank[live] < 99), ref_rank[live] == 99):
        assert rel.any()


def test_loop_more_than_one_workgroup_of_every_kernel(gpu_ctx):
    """33 connected keyframes x 300 points: 9900 entries, 6600 points, 300 keyframes in the table (two blocks of the keyframe kernel)."""
    sc = S.make_loop_scene(31, n_kf=300, n_conn=33, cur_rank=17, per_kf=300, s=0.7)
    exp, differ = check_loop(run_loop(gpu_ctx, sc), sc, "33 x 300")
    assert (np.bincount(exp["corrected_by"][exp["corrected_by"] >= 0], minlength=33) > 0).all()
    print("33 x 300: values not bit-equal to the restatement:", differ)


def test_loop_equals_the_per_keyframe_route(gpu_ctx):
    """The route documented before this entry point: the host loop over the connected keyframes with one
    lld_mappoint_refresh(NORMAL_DEPTH) per keyframe for the points it corrects, SetPose after each.  Every float bit for bit."""
    sc = S.make_loop_scene(41, n_kf=12, n_conn=5, cur_rank=1, per_kf=40, s=0.7)
    got = run_loop(gpu_ctx, sc)
    K = R.loop_poses(sc)
    pos = np.array(sc["pos"]); normal = np.array(sc["normal"]); mn = np.array(sc["min_distance"]); mx = np.array(sc["max_distance"])
    ow = np.array([R.centre_of(T) for T in sc["kf_tcw"]], f32).reshape(-1, 3)
    already = sc["already"] != 0
    for r, k in enumerate(sc["conn"]):
        mine = []
        for p in sc["kf_point"][sc["kf_start"][r]:sc["kf_start"][r + 1]]:
            if sc["bad"][p] or already[p]:
                continue
            pos[p] = R.correct_point(K["non"][r], R.sim3_inverse(K["corrected"][r]), pos[p]); already[p] = True; mine.append(p)
        if mine:
            mine = np.array(mine)
            s, e = sc["obs_start"][mine], sc["obs_start"][mine + 1]
            idx = np.concatenate([np.arange(a, b) for a, b in zip(s, e)]).astype(np.int64)
            one = refresh_map_points(gpu_ctx, np.concatenate([[0], np.cumsum(e - s)]), sc["obs_kf"][idx], sc["bad"][mine], kf_ow=ow, pos=pos[mine],
                                     ref_kf=sc["ref_kf"][mine], ref_level=sc["ref_level"][mine], level_scale=sc["level_scale"], flags=NORMAL_DEPTH,
                                     normal=normal[mine], min_distance=mn[mine], max_distance=mx[mine])
            normal[mine], mn[mine], mx[mine] = one.normal, one.min_distance, one.max_distance
        ow[k] = R.centre_of(R.se3_of_sim3(K["corrected"][r]))
    assert R.bits_equal(got.pos, pos) and R.bits_equal(got.normal, normal) and R.bits_equal(got.min_distance, mn) and R.bits_equal(got.max_distance, mx)


# ------------------------------------------------------------------------------------------------------------------ loop 2 and the packing
def check_graph(ctx, got, sc, what):
    exp = R.essential_graph_literal(sc)
    assert np.array_equal(got.updated, exp["updated"]), what
    differ = once_rounded(got.tiw, exp["tiw"], what + " tiw") + once_rounded(got.pos, exp["pos"], what + " pos")
    assert R.bits_equal(got.ow, np.array([R.centre_of(T) for T in got.tiw], f32).reshape(-1, 3)), what
    normal, mn, mx, did = R.graph_normals(sc, got.pos, got.ow)
    assert np.array_equal(did, (got.updated & NORMAL_DEPTH) != 0), what
    assert R.bits_equal(got.normal, normal) and R.bits_equal(got.min_distance, mn) and R.bits_equal(got.max_distance, mx), what
    still = got.updated == 0
    assert R.bits_equal(got.pos[still], sc["pos"][still]) and R.bits_equal(got.normal[still], sc["normal"][still]), what
    # no restatement needed: one lld_mappoint_refresh on the returned positions and centres
    one = refresh_map_points(ctx, sc["obs_start"], sc["obs_kf"], sc["bad"], kf_ow=got.ow, pos=got.pos, ref_kf=sc["ref_kf"], ref_level=sc["ref_level"],
                             level_scale=sc["level_scale"], flags=NORMAL_DEPTH, **{k: sc[k] for k in PRIOR})
    assert R.bits_equal(one.normal, got.normal) and R.bits_equal(one.min_distance, got.min_distance) and R.bits_equal(one.max_distance, got.max_distance)
    assert np.array_equal(one.updated, got.updated & NORMAL_DEPTH), what
    return differ


def test_graph_small(gpu_ctx):
    sc = S.make_graph_scene(51, n_kf=8, n=100)
    assert (sc["corr_kf"] != sc["ref_kf"]).sum() > 20 and sc["bad"].any() and (np.diff(sc["obs_start"]) == 0).any()
    check_graph(gpu_ctx, run_graph(gpu_ctx, sc), sc, "8 x 100")


def test_graph_whole_map(gpu_ctx):
    sc = S.make_graph_scene(52, n_kf=300, n=20000)
    differ = check_graph(gpu_ctx, run_graph(gpu_ctx, sc), sc, "300 x 20000")
    print("300 x 20000: values not bit-equal to the restatement:", differ)


def test_normal_depth_packing_at_every_size(gpu_ctx):
    """1, 2, 7, 8 observations share a wavefront eight points at a time; 9, 63, 64 take a wavefront; 65, 200 and the limit take it in
    chunks.  The same scene with the points reversed lands every point in another group and another lane: the same bits per point."""
    counts = [1, 2, 7, 8, 9, 63, 64, 65, 200, MAX_OBS] + [3, 0, 8, 5, 9, 1, 64, 6, 8, 8, 2, 70, 8]
    sc = S.make_graph_scene(53, n_kf=MAX_OBS, counts=counts)
    sc["bad"][:10] = 0
    assert np.diff(sc["obs_start"]).tolist() == counts
    got = run_graph(gpu_ctx, sc)
    check_graph(gpu_ctx, got, sc, "packing")
    assert (got.updated[:10] == (MOVED | NORMAL_DEPTH)).all()
    rev = S.reversed_points(sc, extra=("corr_kf",))
    again = run_graph(gpu_ctx, rev)
    for k in ("pos", "normal", "min_distance", "max_distance", "updated"):
        assert R.bits_equal(getattr(again, k)[::-1], getattr(got, k)), k


# ------------------------------------------------------------------------------------------------------------------ loop 3
def test_global_ba_update(gpu_ctx):
    """Two origins; chains of depth 0, 1 and 3 (and 2 on the way) below optimised keyframes; points that are optimised, that move
    through a visited reference keyframe, whose reference keyframe is not visited, and bad ones.  Bit for bit."""
    sc = S.make_gba_scene(61)
    exp = R.global_ba_literal(sc)
    got = apply_global_ba(gpu_ctx, *gba_args(sc))
    assert np.array_equal(got.visited, exp["visited"]) and np.array_equal(got.moved, exp["moved"])
    v = exp["visited"] != 0
    assert not v[sc["unvisited"]].any() and v.sum() == len(v) - 2 and len(sc["origins"]) == 2
    assert set(np.unique(exp["moved"]).tolist()) == {0, 1, 2} and (exp["moved"][:4] == 0).all() and sc["bad"].any()
    depth = []
    for k in np.flatnonzero(v):
        d, c = 0, k
        while not sc["kf_in_gba"][c]:
            c = sc["parent"][c]; d += 1
        depth.append(d)
    assert {0, 1, 3} <= set(depth)
    for k in ("tcw_new", "tcw_before", "ow_new"):
        assert R.bits_equal(getattr(got, k)[v], exp[k][v]), k
    assert R.bits_equal(got.pos, exp["pos"])
    assert R.bits_equal(got.tcw_new[~v], sc["kf_tcw"][~v])     # what the caller passed in


def test_global_ba_two_blocks_of_points(gpu_ctx):
    sc = S.make_gba_scene(62, n_chains=12, n_extra=300, n=3000)
    exp = R.global_ba_literal(sc)
    got = apply_global_ba(gpu_ctx, *gba_args(sc))
    v = exp["visited"] != 0
    assert np.array_equal(got.visited, exp["visited"]) and np.array_equal(got.moved, exp["moved"])
    assert R.bits_equal(got.tcw_new[v], exp["tcw_new"][v]) and R.bits_equal(got.ow_new[v], exp["ow_new"][v]) and R.bits_equal(got.pos, exp["pos"])


# ------------------------------------------------------------------------------------------------------------------ refusals
def refused(ctx, prepare, args, kw, fn, edit):
    """Prepares the call, lets `edit(a, o)` spoil it, makes it and returns the status; a call that was refused must not have changed
    one byte of any output array."""
    a, o, r, keep = prepare(None, *args, **kw)
    edit(a, o)
    outs = [x for x in vars(r).values() if isinstance(x, np.ndarray)]
    before = [x.tobytes() for x in outs]
    st = ctx.lib.fn(fn)(ctx.handle, C.byref(a), C.byref(o))
    assert st == abi.LLD_OK or [x.tobytes() for x in outs] == before, "a refused call wrote to its outputs"
    return st


def test_loop_refusals(gpu_ctx):
    sc = S.make_loop_scene(71, n_kf=8, n_conn=4, cur_rank=1, per_kf=10)
    INV, UNS = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED

    def st(edit=lambda a, o: None, **kw):
        a, k = loop_args(dict(sc, **kw))
        return refused(gpu_ctx, correct_loop, a, k, "loop_correct", edit)

    def null(which, *path):
        def edit(a, o):
            obj = a if which == "in" else o
            for name in path[:-1]:
                obj = getattr(obj, name)
            setattr(obj, path[-1], None)
        return edit

    assert st() == abi.LLD_OK
    for path in (("kf_tcw",), ("conn",), ("scw",), ("kf_start",), ("kf_point",), ("already",), ("points", "pos"), ("points", "bad"),
                 ("points", "obs_start"), ("points", "obs_kf"), ("points", "ref_kf"), ("points", "ref_level"), ("points", "level_scale")):
        assert st(null("in", *path)) == INV, path
    for name in ("corrected_sim3", "non_corrected_sim3", "tiw_corrected", "ow_corrected", "scw_f32", "pos", "corrected_by", "normal",
                 "min_distance", "max_distance", "updated"):
        assert st(null("out", name)) == INV, name
    for field in ("n_kf", "n_conn", "n_entries"):
        assert st(lambda a, o, f=field: setattr(a, f, -1)) == INV, field
    assert st(lambda a, o: setattr(a.points, "n_points", -1)) == INV and st(lambda a, o: setattr(a.points, "n_obs", -1)) == INV
    for cur in (-1, 4):
        assert st(cur=cur) == INV
    conn = sc["conn"].copy(); conn[2] = conn[0]
    assert st(conn=conn) == INV                                                         # a slot repeated in conn
    conn = sc["conn"].copy(); conn[3] = 8
    assert st(conn=conn) == INV
    ks = sc["kf_start"].copy(); ks[0] = 1
    assert st(kf_start=ks) == INV
    ks = sc["kf_start"].copy(); ks[2] = ks[3] + 1
    assert st(kf_start=ks) == INV
    kp = sc["kf_point"].copy(); kp[5] = len(sc["bad"])
    assert st(kf_point=kp) == INV
    os_ = sc["obs_start"].copy(); os_[0] = 1
    assert st(obs_start=os_) == INV
    os_ = sc["obs_start"].copy(); os_[3] = os_[4] + 1
    assert st(obs_start=os_) == INV
    ok = sc["obs_kf"].copy(); ok[0] = 8
    assert st(obs_kf=ok) == INV
    live = int(np.flatnonzero((R.owners(sc) >= 0) & (np.diff(sc["obs_start"]) > 0))[0])
    lv = sc["ref_level"].copy(); lv[live] = len(sc["level_scale"])
    assert st(ref_level=lv) == INV
    rk = sc["ref_kf"].copy(); rk[live] = -1
    assert st(ref_kf=rk) == INV
    dead = int(np.flatnonzero(R.owners(sc) < 0)[0])             # ... but never read for a point the rule skips
    lv = sc["ref_level"].copy(); lv[dead] = 99
    assert st(ref_level=lv) == abi.LLD_OK
    assert st(level_scale=np.ones(17, f32)) == INV
    for bad_value in (np.nan, np.inf):
        T = sc["kf_tcw"].copy(); T[3, 7] = bad_value
        assert st(kf_tcw=T) == INV
        scw = sc["scw"].copy(); scw[5] = bad_value
        assert st(scw=scw) == INV
    for scale in (0.0, -1.0):
        scw = sc["scw"].copy(); scw[7] = scale
        assert st(scw=scw) == INV
    over = S.make_graph_scene(72, n_kf=MAX_OBS + 1, counts=[3, MAX_OBS + 1])
    a, k = graph_args(over)
    assert refused(gpu_ctx, apply_essential_graph, a, k, "essential_graph_apply", lambda a, o: None) == UNS
    # n_points = 0
    empty = correct_loop(gpu_ctx, sc["kf_tcw"], sc["conn"], sc["cur"], sc["scw"], np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros((0, 3), f32),
                         np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                         np.zeros(0, np.int32), sc["level_scale"])
    assert R.bits_equal(empty.tiw_corrected, run_loop(gpu_ctx, sc).tiw_corrected)


def test_graph_and_global_ba_refusals(gpu_ctx):
    INV = abi.LLD_ERR_INVALID
    sc = S.make_graph_scene(73, n_kf=6, n=30)

    def gst(edit=lambda a, o: None, **kw):
        a, k = graph_args(dict(sc, **kw))
        return refused(gpu_ctx, apply_essential_graph, a, k, "essential_graph_apply", edit)

    assert gst() == abi.LLD_OK
    for name in ("sim3_before", "sim3_after", "corr_kf"):
        assert gst(lambda a, o, n=name: setattr(a, n, None)) == INV, name
    for name in ("tiw", "ow", "pos", "normal", "min_distance", "max_distance", "updated"):
        assert gst(lambda a, o, n=name: setattr(o, n, None)) == INV, name
    good = int(np.flatnonzero(sc["bad"] == 0)[0])
    ck = sc["corr_kf"].copy(); ck[good] = 6
    assert gst(corr_kf=ck) == INV
    for which in ("sim3_before", "sim3_after"):
        s3 = sc[which].copy(); s3[2, 7] = 0.0
        assert gst(**{which: s3}) == INV
        s3 = sc[which].copy(); s3[4, 1] = np.nan
        assert gst(**{which: s3}) == INV
    assert gst(lambda a, o: setattr(a, "n_kf", -1)) == INV

    sg = S.make_gba_scene(74)

    def bst(edit=lambda a, o: None, **kw):
        return refused(gpu_ctx, apply_global_ba, gba_args(dict(sg, **kw)), {}, "global_ba_apply", edit)

    assert bst() == abi.LLD_OK
    for name in ("kf_tcw", "kf_in_gba", "kf_tcw_gba", "parent", "origins", "pos", "bad", "in_gba", "pos_gba", "ref_kf"):
        assert bst(lambda a, o, n=name: setattr(a, n, None)) == INV, name
    for name in ("visited", "tcw_new", "tcw_before", "ow_new", "pos", "moved"):
        assert bst(lambda a, o, n=name: setattr(o, n, None)) == INV, name
    n_kf = len(sg["parent"])
    par = sg["parent"].copy(); par[sg["unvisited"][0]] = n_kf
    assert bst(parent=par) == INV                                                       # out of range
    a_, b_ = sg["unvisited"]                                                             # b_ hangs below a_: close the cycle
    par = sg["parent"].copy(); par[a_] = b_
    assert bst(parent=par) == INV
    par = sg["parent"].copy(); par[a_] = a_
    assert bst(parent=par) == INV
    gb = sg["kf_in_gba"].copy(); gb[b_] = 1                                              # optimised, but the walk does not reach it
    assert bst(kf_in_gba=gb) == INV
    p = int(np.flatnonzero((sg["bad"] == 0) & (sg["in_gba"] == 0))[0])
    ref = sg["ref_kf"].copy(); ref[p] = n_kf
    assert bst(ref_kf=ref) == INV
    p = int(np.flatnonzero(sg["bad"] != 0)[0])                                           # a bad point's reference keyframe is never read
    ref = sg["ref_kf"].copy(); ref[p] = n_kf
    assert bst(ref_kf=ref) == abi.LLD_OK
    assert bst(origins=np.array([sg["origins"][0], sg["origins"][0]])) == INV
    assert bst(origins=np.array([n_kf])) == INV
    T = sg["kf_tcw"].copy(); T[0, 0] = np.inf
    assert bst(kf_tcw=T) == INV
    with pytest.raises(LoopCorrectionError) as e:
        apply_global_ba(gpu_ctx, *gba_args(dict(sg, parent=par)))
    assert e.value.status == INV


# ------------------------------------------------------------------------------------------------------------------ the shared rule
@functools.lru_cache(maxsize=None)
def landmark_scene():
    import landmark_ref as L
    sc = L.make_point_scene(7, 600, p_kf_bad=0)
    return sc, L.refresh_map_points_ref(sc, NORMAL_DEPTH)


def test_mappoint_refresh_returns_the_same_bits(gpu_ctx):
    """lm_normal_wave now takes its term, centre and final write from the header the packed kernels use: on landmark_ref's scene it
    returns what it returned before, the restatement's bits."""
    sc, exp = landmark_scene()
    one = refresh_map_points(gpu_ctx, sc["obs_start"], sc["obs_kf"], sc["bad"], kf_ow=sc["kf_ow"], pos=sc["pos"], ref_kf=sc["ref_kf"],
                             ref_level=sc["ref_level"], level_scale=sc["level_scale"], flags=NORMAL_DEPTH)
    for k in ("normal", "min_distance", "max_distance"):
        assert R.bits_equal(getattr(one, k), exp[k]), k
    assert np.array_equal(one.updated, exp["updated"])


def test_limits_are_refused_before_anything_is_queued(gpu_ctx):
    """One past LLD_MAPCORR_MAX_KF for each entry point, one past LLD_MAPCORR_MAX_POINTS and one past LLD_MAPCORR_MAX_ENTRIES, on
    tables that are otherwise valid (INVALID takes precedence): LLD_ERR_UNSUPPORTED, outputs untouched."""
    from lld_slam_amd.loop_correction import MAX_ENTRIES, MAX_KF, MAX_POINTS
    UNS = abi.LLD_ERR_UNSUPPORTED
    eye = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32)
    unit = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    one_scale = np.ones(1, f32)

    def no_points(n=0, bad=1):
        return [np.zeros((n, 3), f32), np.full(n, bad, np.uint8), np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(n, np.int32),
                np.zeros(n, np.int32), one_scale]

    nk = MAX_KF + 1
    pos, bad, start, okf, ref, lvl, scale = no_points()
    loop = [np.tile(eye, (nk, 1)), np.zeros(1, np.int32), 0, unit, np.zeros(2, np.int32), np.zeros(0, np.int32), pos, bad, np.zeros(0, np.uint8),
            start, okf, ref, lvl, scale]
    assert refused(gpu_ctx, correct_loop, loop, {}, "loop_correct", lambda a, o: None) == UNS
    loop[0] = np.tile(eye, (MAX_KF, 1))
    assert refused(gpu_ctx, correct_loop, loop, {}, "loop_correct", lambda a, o: None) == abi.LLD_OK      # the limit itself is accepted
    graph = [np.tile(unit, (nk, 1)), np.tile(unit, (nk, 1)), np.zeros(0, np.int32)] + no_points()
    assert refused(gpu_ctx, apply_essential_graph, graph, {}, "essential_graph_apply", lambda a, o: None) == UNS
    gba = [np.tile(eye, (nk, 1)), np.eye(1, nk, dtype=np.uint8)[0], np.tile(eye, (nk, 1)), np.full(nk, -1, np.int32), np.zeros(1, np.int32),
           np.zeros((0, 3), f32), np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros((0, 3), f32), np.zeros(0, np.int32)]
    assert refused(gpu_ctx, apply_global_ba, gba, {}, "global_ba_apply", lambda a, o: None) == UNS
    # points: every one bad and without observations, so that nothing else is wrong with the table
    graph = [unit[None], unit[None], np.zeros(MAX_POINTS + 1, np.int32)] + no_points(MAX_POINTS + 1)
    assert refused(gpu_ctx, apply_essential_graph, graph, {}, "essential_graph_apply", lambda a, o: None) == UNS
    # entries: one connected keyframe that lists its one (bad) point one time too many
    pos, bad, start, okf, ref, lvl, scale = no_points(1)
    loop = [eye[None], np.zeros(1, np.int32), 0, unit, np.array([0, MAX_ENTRIES + 1], np.int32), np.zeros(MAX_ENTRIES + 1, np.int32), pos, bad,
            np.zeros(1, np.uint8), start, okf, ref, lvl, scale]
    assert refused(gpu_ctx, correct_loop, loop, {}, "loop_correct", lambda a, o: None) == UNS
