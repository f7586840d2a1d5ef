"""lld_map_ba_window and lld_map_local_ba past the widths lld_map_ba.hip fixes that tests/test_gpu_map_ba_window.py stops short of: more
landmarks than one trip of the grid-stride kernels covers, line rows and keyframe lists longer than a tile of 256, more fixed cameras than
one stride of their ranking, and lld_map_local_ba's kept capacities under windows that grow and shrink on one map.  Every window is
byte-equal to the plain-Python restatement's (tests/map_ba_ref.py)."""
import numpy as np
import pytest

import map_ba_ref as R
import map_ba_scenes as S
from lld_slam_amd import host, synth
from lld_slam_amd.device_map import DeviceMap
from test_gpu_map_ba_solve import WINDOW, same_solution, window_of
from test_gpu_map_ba_window import check, se3

pytestmark = pytest.mark.gpu

TILE = 256                   # kThreads / kScanTile: a row or a list is walked 256 entries at a time
TRIP = 512 * 16              # kGrid * kGroups: landmarks per trip of ba_visit_kernel / ba_fill_kernel


@pytest.mark.parametrize("kw", [dict(n_points=TRIP + 1), dict(n_points=TRIP - 2, n_lines=5), dict(n_lines=TILE + 1), dict(n_lines=2 * TILE + 1), dict(n_local_spread=600),
                                dict(n_fixed=300)], ids=lambda k: "-".join("%s%d" % i for i in k.items()))
def test_past_the_widths(gpu_ctx, kw):
    m, q = S.wide(**kw)
    got, ref = check(gpu_ctx, m, q, str(kw))
    K = m["keyframes"]
    if "n_points" in kw:
        nl = kw.get("n_lines", 0)
        assert got["n_points"] == kw["n_points"] and got["n_lines"] == nl and got["n_points"] + nl > TRIP             # a second trip
        if nl:                                                                                                       # lines on both sides of the boundary
            assert got["n_points"] < TRIP - 1 and got["n_points"] + nl > TRIP + 1 and np.diff(got["ln_obs_start"]).tolist() == [2, 3, 2, 3, 2]
        else:
            assert np.diff(got["pt_obs_start"])[-3:].tolist() == [2, 3, 3]                                           # the last landmark's run: the bad observer left out
    if "n_lines" in kw and "n_points" not in kw:
        n = kw["n_lines"]
        assert got["n_lines"] == n + 2 and len(K[0]["lines"]) > n > (n - 1) // TILE * TILE >= TILE and K[0]["lines"][TILE] == K[0]["lines"][200]
        assert got["line_slot"].tolist().count(K[0]["lines"][200]) == 1 and sorted(set(np.diff(got["ln_obs_start"]).tolist())) == [1, 2, 3]
    if "n_local_spread" in kw:
        assert got["n_local_cams"] > 2 * TILE and got["n_points"] == 2 * got["n_local_cams"] and got["n_lines"] == got["n_local_cams"]
        assert got["n_pt_obs"] > got["n_points"] and got["n_ln_obs"] > got["n_lines"]                                # shared with earlier keyframes
    if "n_fixed" in kw:
        fixed = got["cam_slot"][got["n_local_cams"]:].tolist()
        keys = [K[s]["key"] for s in fixed]
        disorder = lambda v: sum(a > b for a, b in zip(v, v[1:]))
        assert len(fixed) > TILE and disorder(fixed) > 50 and disorder(keys) > 50                                    # neither slot order nor key order


# ---------------------------------------------------------------------------------------------------------------- capacities kept between calls
def shifted(m, q, k0, p0, l0):
    """the map and the query with every keyframe, point and line slot moved up"""
    sp = lambda v: v + p0 if v >= 0 else v
    sl = lambda v: v + l0 if v >= 0 else v
    out = dict(keyframes={}, points={}, lines={})
    for s, k in m["keyframes"].items():
        out["keyframes"][s + k0] = dict(k, points=[sp(v) for v in k["points"]], lines=[sl(v) for v in k["lines"]])
    for s, p in m["points"].items(): out["points"][s + p0] = dict(p, obs=[(kf + k0, i) for kf, i in p["obs"]])
    for s, l in m["lines"].items(): out["lines"][s + l0] = dict(l, obs=[(kf + k0, i) for kf, i in l["obs"]])
    return out, [s + k0 for s in q]


def same_window(ids, ref, what):
    assert ids["status"] == 0 and ids["n_local_cams"] == ref["n_local_cams"] and ids["window"].n_free_cams == ref["n_free_cams"], what
    for k in ("cam_slot", "point_slot", "line_slot"):
        assert np.array_equal(ids[k], ref[k]), (what, k)
    for k in WINDOW:
        assert getattr(ids["window"], k).tobytes() == ref[k].tobytes(), (what, k)
    assert sorted(ids["marked_bad_slot"].tolist()) == ref["marked_bad"] and len(set(ids["marked_bad_slot"].tolist())) == len(ref["marked_bad"]), what


def test_windows_that_grow_and_shrink_on_one_map(gpu_ctx):
    """lld_map_local_ba keeps the capacities of its last call.  With the stop flag up (the window is assembled, nothing is solved): a small
    window, one several times larger in every count, the small one again, and the small one with more bad observers marked fixed than any
    call before it - only that capacity is short.  Then one full solve of the small window."""
    ws = synth.make_lba_small(0, n_free=3, n_fixed=1, n_points=40, n_lines=8)
    wl = synth.make_lba_small(1, n_free=12, n_fixed=4)
    ms, qs, ts = S.map_of_window(ws, 100)
    ml, ql, tl = S.map_of_window(wl, 101)
    ml, ql = shifted(ml, ql, 16, 64, 16)
    m = {k: {**ms[k], **ml[k]} for k in ("keyframes", "points", "lines")}
    assert len(m["keyframes"]) == len(ms["keyframes"]) + len(ml["keyframes"]) and len(m["points"]) == 340 and len(m["lines"]) == 68
    never = list(range(max(m["keyframes"]) + 1, max(m["keyframes"]) + 41))              # keyframe slots never set: bad observers
    L = S.limits_for(m, max_keyframes=never[-1] + 1)
    L["max_observations"] += len(never)
    ref = lambda q, t: R.ba_window(m, q, t, se3, max_keyframes=L["max_keyframes"])
    with DeviceMap(gpu_ctx, **L) as dm:
        S.upload(dm, m)
        small, large = ref(qs, ts), ref(ql, tl)
        for c in ("n_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs"):
            assert large[c] >= 3 * small[c] > 0, c
        assert small["marked_bad"] == large["marked_bad"] == []
        for what, q, t, w, r in (("small", qs, ts, ws, small), ("large", ql, tl, wl, large), ("small again", qs, ts, ws, small)):
            got, ids = dm.local_ba(q, w.cam, t, stop=True)
            same_window(ids, r, what)
            assert got.stats["aborted"] == 1 and got.stats["lm_iterations"] == [0, 0]
        # the same query; forty observers more, all of them bad: nothing of the window moves, only the list of the bad marked ones grows
        pts = [int(p) for p in small["point_slot"][:len(never)]]
        for p, s in zip(pts, never): m["points"][p]["obs"].append((s, 0))
        S.upload_points(dm, m, pts)
        more = ref(qs, ts)
        assert more["marked_bad"] == never and all(more[k].tobytes() == small[k].tobytes() for k in R.ARRAYS)
        got, ids = dm.local_ba(qs, ws.cam, ts, stop=True)
        same_window(ids, more, "more bad observers")
        # ... and the full solve is lld_local_ba's on the restated window, bit for bit
        want = host.Optimizer(gpu_ctx).LocalBundleAdjustment(window_of(more, ws.cam))
        got, ids = dm.local_ba(qs, ws.cam, ts)
        same_solution(got, ids, dict(ref=more, cam=ws.cam), want)
        assert got.stats["lm_iterations"][0] > 0 and not got.stats["aborted"] and sorted(ids["marked_bad_slot"].tolist()) == never
