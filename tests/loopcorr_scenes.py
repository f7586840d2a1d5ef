"""Seeded scenes for the loop-correction tests (tests/loopcorr_ref.py restates the rules).  Keyframe slots are in pointer order, so the
connected keyframes of a scene are ascending slots and the observers of a point are ascending slots.  It does not import lld_slam_amd."""
import numpy as np

f32 = np.float32


def random_pose(rng, spread=3.0):
    """A float Tcw[12]: a rotation from a random unit quaternion, rounded to float (so not exactly orthonormal, as in a real map)."""
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R, rng.normal(0, spread, (3, 1))], axis=1).astype(f32).reshape(12)


def random_sim3(rng, s=None, small=False):
    """8 doubles: a unit quaternion (a small rotation when `small`), a translation, a scale."""
    q = np.array([0, 0, 0, 1.0]) + rng.normal(0, 0.05, 4) if small else rng.normal(size=4)
    q /= np.linalg.norm(q)
    t = rng.normal(0, 0.3 if small else 2.0, 3)
    return np.concatenate([q, t, [rng.uniform(0.6, 1.5) if s is None else s]])


def _point_table(rng, n, n_kf, counts, n_levels=8, p_bad=0.05, forced=None):
    """pos, bad, the observation CSR (ascending distinct slots; forced[p] = slots that must observe p), ref_kf / ref_level, prior
    normals and depths."""
    start, kf = [0], []
    for p in range(n):
        must = sorted(set(forced.get(p, []))) if forced else []
        c = min(max(int(counts[p]), len(must)), n_kf) if counts[p] > 0 else 0
        obs = set(must[:c])
        if c > len(obs):
            rest = np.setdiff1d(np.arange(n_kf), np.array(sorted(obs), np.int64))
            obs |= set(rng.choice(rest, c - len(obs), replace=False).tolist())
        kf.extend(sorted(obs))
        start.append(len(kf))
    return dict(pos=(rng.normal(0, 1.0, (n, 3)) + np.array([0, 0, 8.0])).astype(f32), bad=(rng.random(n) < p_bad).astype(np.uint8),
                obs_start=np.array(start, np.int32), obs_kf=np.array(kf, np.int32), ref_kf=rng.integers(0, n_kf, n).astype(np.int32),
                ref_level=rng.integers(0, n_levels, n).astype(np.int32), level_scale=(f32(1.2) ** np.arange(n_levels)).astype(f32),
                normal=rng.normal(0, 1, (n, 3)).astype(f32), min_distance=rng.uniform(1, 2, n).astype(f32),
                max_distance=rng.uniform(5, 9, n).astype(f32))


def make_loop_scene(seed, n_kf=12, n_conn=5, cur_rank=2, per_kf=40, s=1.0, scw=None, p_already=0.05, p_noobs=0.04, n_points=None):
    """CorrectLoop: n_conn connected keyframes among n_kf, each holding per_kf point slots.  Point 0 is held by the first three
    connected keyframes (when there are three), point 1 is listed twice by rank 0, and the reference keyframes are drawn from the
    whole table: ranks below, at and above the owner's and keyframes outside conn all occur."""
    rng = np.random.default_rng(seed)
    conn = np.sort(rng.choice(n_kf, n_conn, replace=False)).astype(np.int32)
    n = max(2, (n_conn * per_kf * 2) // 3) if n_points is None else n_points
    kf_start, kf_point, forced = [0], [], {}
    for r in range(n_conn):
        lst = rng.integers(0, n, per_kf).tolist()              # slots may repeat
        if r < 3 and n_conn >= 3:
            lst[0] = 0
        if r == 0 and per_kf >= 3:
            lst[1] = 1; lst[2] = 1
        for p in lst:
            forced.setdefault(p, []).append(int(conn[r]))
        kf_point += lst
        kf_start.append(len(kf_point))
    counts = rng.integers(1, 10, n)
    counts[rng.random(n) < p_noobs] = 0
    sc = _point_table(rng, n, n_kf, counts, forced=forced)
    sc.update(kf_tcw=np.array([random_pose(rng) for _ in range(n_kf)], f32), conn=conn, cur=int(cur_rank),
              scw=random_sim3(rng, s, small=True) if scw is None else np.array(scw, np.float64), kf_start=np.array(kf_start, np.int32),
              kf_point=np.array(kf_point, np.int32), already=(rng.random(n) < p_already).astype(np.uint8))
    return sc


def make_graph_scene(seed, n_kf=8, n=100, counts=None):
    """The essential graph's write-back: a Sim3 before and after per keyframe (after = a small Sim3 times before, scales away from
    1), corr_kf different from ref_kf for about half of the points."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 10, n) if counts is None else np.asarray(counts)
    n = len(counts)
    sc = _point_table(rng, n, n_kf, counts)
    before = np.array([random_sim3(rng, 1.0) for _ in range(n_kf)])
    after = before + np.concatenate([rng.normal(0, 0.01, (n_kf, 4)), rng.normal(0, 0.2, (n_kf, 3)), rng.uniform(-0.2, 0.3, (n_kf, 1))], axis=1)
    corr = np.where(rng.random(n) < 0.5, sc["ref_kf"], rng.integers(0, n_kf, n)).astype(np.int32)
    sc.update(sim3_before=before, sim3_after=after, corr_kf=corr)
    return sc


def make_gba_scene(seed, n_chains=4, n_extra=10, n=200):
    """Global BA's map update: two origins; below optimised keyframes hang chains of keyframes Global BA did not see, of depth 1 and 3
    (an optimised leaf has depth 0), one of them with an optimised keyframe below it again; one root that is no origin, whose subtree
    stays unvisited.  Points: optimised, moved through a visited reference keyframe, with an unvisited one, bad."""
    rng = np.random.default_rng(seed)
    parent, in_gba = [-1, -1], [1, 1]                          # slots 0 and 1: the origins
    def add(par, gba):
        parent.append(par); in_gba.append(gba); return len(parent) - 1
    for _ in range(n_extra):                                   # optimised keyframes anywhere below the origins
        add(int(rng.integers(0, len(parent))), 1)
    n_opt = len(parent)
    for c in range(n_chains):
        k = add(int(rng.integers(0, n_opt)), 0)                # depth 1
        if c % 2 == 0:
            k = add(k, 0); add(k, 0)                           # depth 3 ...
            k = add(k, 0)                                      # ... and a sibling at depth 3
            if c == 0:
                add(k, 1)                                      # an optimised keyframe below the chain
    lone = add(-1, 0)                                          # a root that is no origin: never visited
    add(lone, 0)
    n_kf = len(parent)
    perm = rng.permutation(n_kf)                               # slots are pointer order: unrelated to the tree
    par = np.full(n_kf, -1, np.int32)
    for k in range(n_kf):
        par[perm[k]] = -1 if parent[k] < 0 else perm[parent[k]]
    gba = np.zeros(n_kf, np.uint8); gba[perm] = np.array(in_gba, np.uint8)
    unvisited = np.array([perm[lone], perm[lone + 1]], np.int32)
    ref = rng.integers(0, n_kf, n).astype(np.int32)
    ref[:4] = unvisited[[0, 1, 0, 1]]
    bad = (rng.random(n) < 0.1).astype(np.uint8); pt_gba = (rng.random(n) < 0.5).astype(np.uint8)
    bad[:4] = 0; pt_gba[:4] = 0                                # these four really read their unvisited reference keyframe
    return dict(kf_tcw=np.array([random_pose(rng) for _ in range(n_kf)], f32), kf_in_gba=gba,
                kf_tcw_gba=np.array([random_pose(rng) for _ in range(n_kf)], f32), parent=par,
                origins=np.array([perm[0], perm[1]], np.int32), pos=(rng.normal(0, 1.0, (n, 3)) + np.array([0, 0, 8.0])).astype(f32),
                bad=bad, in_gba=pt_gba,
                pos_gba=rng.normal(0, 3.0, (n, 3)).astype(f32), ref_kf=ref, unvisited=unvisited)


def reversed_points(sc, extra=()):
    """The same point table with the points in reverse order (the keyframe tables unchanged)."""
    n = len(sc["bad"])
    order = np.arange(n)[::-1]
    s, e = sc["obs_start"][order], sc["obs_start"][order + 1]
    idx = np.concatenate([np.arange(a, b) for a, b in zip(s, e)]).astype(np.int64)
    out = dict(sc)
    out["obs_start"] = np.concatenate([[0], np.cumsum(e - s)]).astype(np.int32)
    out["obs_kf"] = sc["obs_kf"][idx]
    for k in ("pos", "bad", "ref_kf", "ref_level", "normal", "min_distance", "max_distance") + tuple(extra):
        out[k] = sc[k][order]
    return out


# ------------------------------------------------------------------ the object scenes of examples/loop_correct_harness
KF_RECORD, POINT_RECORD = 59, 11             # doubles per keyframe / per point in the harness's dump


def object_scene_blob(kind, sc):
    """scene.bin of examples/loop_correct_harness.cpp for kind 1 (CorrectLoop), 2 (essential graph) or 3 (global BA), and the scene
    the objects amount to: a point whose reference keyframe is not among its observers reads keypoint 0 of that keyframe
    (std::map::operator[]), whose octave the harness sets to slot % n_levels."""
    import struct
    sc = dict(sc)
    n_kf, n = len(sc["kf_tcw"]) if "kf_tcw" in sc else len(sc["sim3_before"]), len(sc["bad"])
    if kind == 3:
        sc.update(obs_start=np.zeros(n + 1, np.int32), obs_kf=np.zeros(0, np.int32), ref_level=np.zeros(n, np.int32), level_scale=np.ones(1, f32),
                  normal=np.zeros((n, 3), f32), min_distance=np.zeros(n, f32), max_distance=np.zeros(n, f32))
    n_levels = len(sc["level_scale"])
    lvl = np.array(sc["ref_level"], np.int32)
    for p in range(n):
        if sc["ref_kf"][p] not in sc["obs_kf"][sc["obs_start"][p]:sc["obs_start"][p + 1]]:
            lvl[p] = sc["ref_kf"][p] % n_levels
    sc["ref_level"] = lvl
    tcw = sc["kf_tcw"] if "kf_tcw" in sc else np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32), (n_kf, 1))
    blob = [struct.pack("<4i", kind, n_kf, n_levels, n), sc["level_scale"].astype(f32).tobytes(), np.ascontiguousarray(tcw, f32).tobytes()]
    for p in range(n):
        s, e = sc["obs_start"][p], sc["obs_start"][p + 1]
        blob += [struct.pack("<i", int(sc["bad"][p])), sc["pos"][p].astype(f32).tobytes(), struct.pack("<2i", int(sc["ref_kf"][p]), int(lvl[p])),
                 sc["normal"][p].astype(f32).tobytes(), struct.pack("<2fi", float(sc["min_distance"][p]), float(sc["max_distance"][p]), int(e - s)),
                 sc["obs_kf"][s:e].astype(np.int32).tobytes()]
    if kind == 1:
        blob += [struct.pack("<2i", len(sc["conn"]), int(sc["cur"])), sc["conn"].astype(np.int32).tobytes(), np.asarray(sc["scw"], np.float64).tobytes()]
        for r in range(len(sc["conn"])):
            lst = sc["kf_point"][sc["kf_start"][r]:sc["kf_start"][r + 1]]
            blob += [struct.pack("<i", len(lst)), lst.astype(np.int32).tobytes()]
        blob.append(sc["already"].astype(np.int32).tobytes())
    elif kind == 2:
        blob += [np.ascontiguousarray(sc["sim3_before"], np.float64).tobytes(), np.ascontiguousarray(sc["sim3_after"], np.float64).tobytes(),
                 sc["corr_kf"].astype(np.int32).tobytes()]
    else:
        for k in range(n_kf):
            blob += [struct.pack("<i", int(sc["kf_in_gba"][k])), sc["kf_tcw_gba"][k].astype(f32).tobytes(), struct.pack("<i", int(sc["parent"][k]))]
        blob += [struct.pack("<i", len(sc["origins"])), sc["origins"].astype(np.int32).tobytes()]
        for p in range(n):
            blob += [struct.pack("<i", int(sc["in_gba"][p])), sc["pos_gba"][p].astype(f32).tobytes()]
    return b"".join(blob), sc


def read_object_dump(path):
    """out.bin of the harness -> (adapter, host), each a dict of per-keyframe and per-point members."""
    raw = np.fromfile(path, np.uint8)
    n_kf, n = np.frombuffer(raw[:8].tobytes(), np.int32)
    d = np.frombuffer(raw[8:].tobytes(), np.float64)
    per = n_kf * KF_RECORD + n * POINT_RECORD
    assert len(d) == 2 * per
    out = []
    for half in (d[:per], d[per:]):
        k = half[:n_kf * KF_RECORD].reshape(n_kf, KF_RECORD); p = half[n_kf * KF_RECORD:].reshape(n, POINT_RECORD)
        out.append(dict(tcw=k[:, 0:12].astype(f32), ow=k[:, 12:15].astype(f32), tcw_gba=k[:, 15:27].astype(f32), tcw_before=k[:, 27:39].astype(f32),
                        kf_gba_mark=k[:, 39].astype(np.int64), n_set_pose=k[:, 40].astype(np.int64), has_corrected=k[:, 41] != 0, corrected=k[:, 42:50],
                        has_non_corrected=k[:, 50] != 0, non_corrected=k[:, 51:59], pos=p[:, 0:3].astype(f32), normal=p[:, 3:6].astype(f32),
                        min_distance=p[:, 6].astype(f32), max_distance=p[:, 7].astype(f32), corrected_by=p[:, 8].astype(np.int64),
                        corrected_ref=p[:, 9].astype(np.int64), n_set_pos=p[:, 10].astype(np.int64)))
    return out
