"""The resident map's row pools under churn (RowPool in lld_map_tables.h): a replacement longer than a row's capacity goes to the pool's
tail, and when the tail is exhausted the pool is repacked from the host's copy.  tests/test_gpu_map_covis.py drives the observation, index,
point-row, octave and depth pools through that; here one small map is churned until the child rows, the line rows, the keypoint features
(three words per keypoint), the keyline features (ten per keyline) and the lines' observation and index rows have each repacked, with the
limits tight.  On the way and at the end UpdateLocalMap, covisibility with culling and the BA window equal their restatements on the Python
copy of the map, and a replacement one entry past a limit is refused and changes nothing."""
import numpy as np
import pytest

import local_map_ref as REF
import map_ba_scenes as S
import map_covis_ref as M
from lld_slam_amd import abi, synth
from lld_slam_amd.device_map import DeviceMap
from lld_slam_amd.tracking import DeviceTrackedFrame
from test_gpu_local_map import one_frame, same as same_local_map
from test_gpu_map_ba_window import run as run_ba_window
from test_gpu_map_covis import CONN, CULL, same as same_covis

pytestmark = pytest.mark.gpu

N_OBSERVING, N_KF, N_PT, N_LN, ROUNDS = 6, 10, 30, 8, 40     # keyframes with points and lines, keyframes set, points, lines
QUERY = [0, 2, 4]


@pytest.fixture(scope="module")
def frame(gpu_ctx):
    with DeviceTrackedFrame(gpu_ctx, synth.make_orb_frame(0, 256), synth.KITTI_CAM) as tf:
        yield tf


def features(k, rng):
    """keypoints and features for the rows of keyframe k as they are now"""
    n, nl = len(k["points"]), len(k["lines"])
    k["octave"] = rng.integers(0, S.N_LEVELS, n).tolist(); k["depth"] = (rng.random(n) * 60).astype(np.float32).tolist(); k["th_depth"] = 35.0
    k["uvr"] = (rng.random((n, 3)) * 300).astype(np.float32)
    k["kl_left"] = (rng.random((nl, 4)) * 300).astype(np.float32); k["kl_right"] = (k["kl_left"] - np.float32(3)).astype(np.float32)
    k["kl_octave"] = rng.integers(0, 4, (nl, 2)).astype(np.int32)


def small_map(rng):
    keys = (rng.permutation(N_KF) * 10 + 5).tolist(); mn = (rng.permutation(N_KF) + 1).tolist()
    K = {s: dict(key=int(keys[s]), bad=0, parent=None if s == 0 else int(rng.integers(0, s)), cov=rng.permutation(N_KF)[:4].tolist(), child=[], points=[], lines=[],
                 mn_id=int(mn[s]), Tcw=S.random_pose(rng)) for s in range(N_KF)}
    for s in range(1, N_KF): K[K[s]["parent"]]["child"].append(s)
    by_key = lambda kfs: sorted((int(s) for s in kfs), key=lambda s: K[s]["key"])
    P, L = {}, {}
    for p in range(N_PT):
        obs = []
        for s in by_key(rng.choice(N_OBSERVING, int(rng.integers(2, 5)), replace=False)):
            if rng.random() < 0.2: K[s]["points"].append(-1)
            obs.append((s, len(K[s]["points"]))); K[s]["points"].append(p)
        P[p] = dict(bad=int(p % 9 == 4), pos=rng.normal(size=3).astype(np.float32), obs=obs, indexed=True)
    for l in range(N_LN):
        obs = []
        for s in by_key(rng.choice(N_OBSERVING, 3, replace=False)):
            obs.append((s, len(K[s]["lines"]))); K[s]["lines"].append(l)
        L[l] = dict(bad=int(l == 5), x0=rng.normal(size=3), dir=rng.normal(size=3), obs=obs, n_obs=6)
    for s in range(N_OBSERVING): features(K[s], rng)
    return dict(keyframes=K, points=P, lines=L)


def push_keyframes(dm, m, slots):
    K = [m["keyframes"][s] for s in slots]
    dm.set_keyframes(slots, [k["key"] for k in K], [k["bad"] for k in K], [-1 if k["parent"] is None else k["parent"] for k in K], [k["cov"] for k in K],
                     [k["child"] for k in K], [k["points"] for k in K], [k["lines"] for k in K])
    ft = [(s, k) for s, k in zip(slots, K) if "uvr" in k]
    if ft:
        dm.set_keyframe_keypoints([s for s, _ in ft], [k["octave"] for _, k in ft], [k["depth"] for _, k in ft], [k["th_depth"] for _, k in ft])
        dm.set_keyframe_features([s for s, _ in ft], [k["mn_id"] for _, k in ft], [k["Tcw"] for _, k in ft], [k["uvr"] for _, k in ft], [k["kl_left"] for _, k in ft],
                                 [k["kl_right"] for _, k in ft], [k["kl_octave"] for _, k in ft])


def answers(dm, tf, m, L, what):
    """the three consumers against their restatements on m; returns what the device gave"""
    K, P = m["keyframes"], m["points"]
    ids = list(range(0, N_PT, 2)) + [4, 13]
    lm = dict(keyframes=K, points={p: dict(bad=v["bad"], obs=[o[0] for o in v["obs"]]) for p, v in P.items()}, lines=m["lines"])
    got, kept = one_frame(tf, dm, ids)
    exp = REF.update_local_map(REF.new_state(), lm, ids, L["max_local_points"], L["max_local_lines"])
    same_local_map(got, kept, exp, what)
    assert exp["n_bad_cleared"] > 0 and len(exp["local_keyframes"]) > exp["n_voted"] and len(exp["local_lines"]) > 3
    T = dict(kf={s: dict(key=k["key"], points=k["points"], octave=k.get("octave"), depth=k.get("depth"), th_depth=k.get("th_depth", 0.0)) for s, k in K.items()},
             pt={p: dict(bad=bool(v["bad"]), nobs=len(v["obs"]), obs=[o[0] for o in v["obs"]], idx=[o[1] for o in v["obs"]]) for p, v in P.items()})
    q = list(range(N_OBSERVING))
    cov = dm.covisibility(q, culling=True, th=2)
    same_covis(cov, M.covisibility(T, q, culling=True, th=2), CONN + CULL + ("status",), what)
    assert not cov["status"].any() and cov["n_mps"].sum() > 20 and cov["n_redundant"].max() > 0
    ba, ref = run_ba_window(dm, m, QUERY, what)
    assert ba["status"] == 0 and ba["n_cams"] > ba["n_local_cams"] and ba["n_lines"] > 2
    lists = [got[k].tolist() for k in ("local_keyframes", "local_points", "local_lines")] + [kept.tolist()]
    return lists, {k: v.tolist() for k, v in cov.items()}, {k: ba[k].tobytes() for k in ("cam_slot", "point_slot", "line_slot") + tuple(S_ARRAYS)}


S_ARRAYS = ("cam_qt", "pt_xyz", "pt_obs_start", "pt_obs_cam", "pt_obs_uvr", "pt_obs_inv_sigma2", "line_x0", "line_dir", "ln_obs_start", "ln_obs_cam", "ln_obs_left",
            "ln_obs_right", "ln_obs_octave")


def test_every_pool_repacks_under_churn(gpu_ctx, frame):
    rng = np.random.default_rng(0x9001)
    m = small_map(rng)
    K, P, Ls = m["keyframes"], m["points"], m["lines"]
    total = lambda key: sum(len(k[key]) for k in K.values())
    live = dict(child=total("child"), kpt=total("points"), kln=total("lines"), lobs=sum(len(l["obs"]) for l in Ls.values()))
    grow_p, grow_l = (ROUNDS - 1) // N_OBSERVING + 2, (ROUNDS - 1) // N_OBSERVING + 1            # the longest temporary growth of a point / line row
    # tight: the live totals plus the growth planned (the line rows and the lines' observation rows share max_kf_lines)
    L = dict(max_keyframes=N_KF + ROUNDS + 1, max_points=N_PT + 2, max_lines=N_LN + 1, line_dim=S.LINE_DIM, max_observations=sum(len(p["obs"]) for p in P.values()),
             max_kf_points=live["kpt"] + grow_p, max_kf_lines=max(live["kln"] + grow_l, live["lobs"] + ROUNDS), max_children=live["child"] + ROUNDS,
             max_local_points=64, max_local_lines=16)
    limit = dict(child=L["max_children"], kln=L["max_kf_lines"], kuvr=3 * L["max_kf_points"], kkl=10 * L["max_kf_lines"], lobs=L["max_kf_lines"], lidx=L["max_kf_lines"])
    start = dict(child=live["child"], kln=live["kln"], kuvr=3 * live["kpt"], kkl=10 * live["kln"], lobs=live["lobs"], lidx=live["lobs"])
    moved = dict.fromkeys(limit, 0)                                   # entries of rows longer than ever before: each went to its pool's tail
    with DeviceMap(gpu_ctx, **L) as dm:
        push_keyframes(dm, m, sorted(K)); S.upload_points(dm, m); S.upload_lines(dm, m)
        answers(dm, frame, m, L, "fresh")
        for r in range(ROUNDS):
            s, v = r % N_OBSERVING, r // N_OBSERVING
            k = K[s]
            base_p, base_l = list(k["points"]), list(k["lines"])
            # the point and line rows grow (longer at every visit), features and keypoints follow ...
            k["points"] = base_p + [next(p for p in range(N_PT) if p not in base_p)] + [-1] * (v + 1)
            k["lines"] = base_l + [next(l for l in range(N_LN) if l not in base_l)] + [-1] * v
            # ... a child row grows by one child, for good
            c = K[(r * 3) % N_KF]
            c["child"] = c["child"] + [int((r * 7 + 6) % N_KF)]
            features(k, rng)
            push_keyframes(dm, m, sorted({s, (r * 3) % N_KF}))
            moved["kln"] += len(k["lines"]); moved["kuvr"] += 3 * len(k["points"]); moved["kkl"] += 10 * len(k["lines"]); moved["child"] += len(c["child"])
            if r % 8 == 3:
                answers(dm, frame, m, L, "round %d, grown" % r)
            # ... and shrink again
            k["points"], k["lines"] = base_p, base_l
            features(k, rng)
            push_keyframes(dm, m, [s])
            # a line's observation row grows by one observer (a keyframe slot never set: bad), for good
            l = r % N_LN
            Ls[l]["obs"] = Ls[l]["obs"] + [(N_KF + 1 + r, r % 3)]
            S.upload_lines(dm, m, [l])
            moved["lobs"] += len(Ls[l]["obs"]); moved["lidx"] += len(Ls[l]["obs"])
            if r % 8 == 7:
                answers(dm, frame, m, L, "round %d" % r)
        for pool in limit:                                            # every tail was exhausted at least once: twice the limit is the pool
            assert moved[pool] > 2 * limit[pool] - start[pool], (pool, moved[pool], limit[pool], start[pool])
        before = answers(dm, frame, m, L, "after the churn")
        # the child rows and the lines' observation rows are at their limits: one entry more is refused, whole call, nothing moves
        assert total("child") == L["max_children"] and sum(len(l["obs"]) for l in Ls.values()) == L["max_kf_lines"]
        with pytest.raises(RuntimeError) as e:
            dm.set_keyframes([0], [K[0]["key"]], [0], [-1], [K[0]["cov"]], [K[0]["child"] + [1]], [K[0]["points"][:2]], [[]])
        assert e.value.status == abi.LLD_ERR_UNSUPPORTED
        with pytest.raises(RuntimeError) as e:
            dm.set_line_observations([0], [Ls[0]["obs"] + [(1, 0)]], [9])
        assert e.value.status == abi.LLD_ERR_UNSUPPORTED
        assert answers(dm, frame, m, L, "after the refusals") == before
