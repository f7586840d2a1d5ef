"""Scenes for the covisibility tests: a small builder, the hand-worked cases with the answers worked out by hand, seeded random
scenes, and an object model (keyframes with keypoints, map points with observation maps) with the loops that
adapters/lld_covisibility_adapter.cc runs, driven by tests/covis_ref.py.  Imports nothing from the library."""
import struct

import numpy as np

import covis_ref as R


class Builder:
    """Map points with (keyframe slot, octave) observations and queries with (point, octave, depth) entries."""

    def __init__(self, n_kf, monocular=False):
        self.n_kf, self.monocular = n_kf, monocular
        self.points, self.queries = [], []

    def point(self, obs, bad=False, nobs=None):
        """obs: [(slot, octave)] or [slot]; listed in slot order as the std::map holds them.  nobs defaults to the list length."""
        obs = sorted((o, 0) if isinstance(o, (int, np.integer)) else tuple(o) for o in obs)
        self.points.append((obs, bad, len(obs) if nobs is None else nobs))
        return len(self.points) - 1

    def query(self, kf, entries, th_depth=40.0):
        """entries: [(point, octave, depth)] or [point]."""
        self.queries.append((kf, [(e, 0, 1.0) if isinstance(e, (int, np.integer)) else tuple(e) for e in entries], th_depth))
        return len(self.queries) - 1

    def scene(self):
        obs = [o for p in self.points for o in p[0]]
        ent = [e for q in self.queries for e in q[1]]
        return dict(n_kf=self.n_kf, monocular=self.monocular,
                    obs_start=np.cumsum([0] + [len(p[0]) for p in self.points]).astype(np.int32),
                    obs_kf=np.array([o[0] for o in obs], np.int32), obs_octave=np.array([o[1] for o in obs], np.int32),
                    point_bad=np.array([p[1] for p in self.points], np.uint8), point_nobs=np.array([p[2] for p in self.points], np.int32),
                    query_kf=np.array([q[0] for q in self.queries], np.int32),
                    q_start=np.cumsum([0] + [len(q[1]) for q in self.queries]).astype(np.int32),
                    q_point=np.array([e[0] for e in ent], np.int32), q_octave=np.array([e[1] for e in ent], np.int32),
                    q_depth=np.array([e[2] for e in ent], np.float32), q_th_depth=np.array([q[2] for q in self.queries], np.float32))


def _shared(b, own, weights):
    """Points seen by `own` and by one other keyframe each: weights = {slot: how many}.  Returns the point ids."""
    return [b.point([own, kf]) for kf, w in sorted(weights.items()) for _ in range(w)]


# ---- connections, worked by hand: (scene, expected dict per query 0)
def conn_tie():
    b = Builder(4); b.query(0, _shared(b, 0, {1: 16, 2: 16, 3: 20}))
    return b.scene(), dict(conn=[(1, 16), (2, 16), (3, 20)], ordered=[(3, 20), (2, 16), (1, 16)], n_max=20, kf_max=3, updated=1)


def conn_fallback_equal_maxima():
    b = Builder(4); b.query(0, _shared(b, 0, {1: 5, 2: 5, 3: 3}))
    return b.scene(), dict(conn=[(1, 5), (2, 5), (3, 3)], ordered=[(1, 5)], n_max=5, kf_max=1, updated=1)


def conn_14_15():
    b = Builder(3); b.query(0, _shared(b, 0, {1: 14, 2: 15}))
    return b.scene(), dict(conn=[(1, 14), (2, 15)], ordered=[(2, 15)], n_max=15, kf_max=2, updated=1)


def conn_empty():
    b = Builder(3); b.query(1, [b.point([1]) for _ in range(7)])
    return b.scene(), dict(conn=[], ordered=[], n_max=0, kf_max=-1, updated=0)


CONN_CASES = dict(tie=conn_tie, fallback=conn_fallback_equal_maxima, w14_15=conn_14_15, empty=conn_empty)


# ---- culling, worked by hand: (scene, (n_mps, n_redundant, redundant) of query 0)
def cull_nobs_3_4():
    b = Builder(5)
    a = b.point([1, 2, 3], nobs=3)                   # three qualifying observations, but Observations() == 3 is not > 3
    c = b.point([1, 2, 3], nobs=4)
    b.query(0, [a, c])
    return b.scene(), (2, 1, 0)


def cull_octave():
    b = Builder(5)
    a = b.point([(1, 3), (2, 3), (3, 3)], nobs=6)    # level + 1: counts
    c = b.point([(1, 3), (2, 3), (3, 4)], nobs=6)    # one at level + 2: two left
    b.query(0, [(a, 2, 1.0), (c, 2, 1.0)])
    return b.scene(), (2, 1, 0)


def cull_2_3():
    b = Builder(5)
    a = b.point([1, 2], nobs=4)
    c = b.point([1, 2, 3], nobs=4)
    b.query(0, [a, c])
    return b.scene(), (2, 1, 0)


def cull_own():
    b = Builder(5)
    a = b.point([0, 1, 2], nobs=4)                   # the query's own observation is not counted: two left
    c = b.point([0, 1, 2, 3], nobs=4)
    b.query(0, [a, c])
    return b.scene(), (2, 1, 0)


def _depth(mono):
    b = Builder(5, monocular=mono)
    pts = [b.point([1, 2, 3], nobs=4) for _ in range(4)]
    b.query(0, [(pts[0], 0, 10.0), (pts[1], 0, np.nextafter(np.float32(10), np.float32(11))), (pts[2], 0, -1.0), (pts[3], 0, 0.0)],
            th_depth=10.0)
    return b.scene(), ((4, 4, 1) if mono else (2, 2, 1))


def cull_depth():
    return _depth(False)


def cull_depth_monocular():
    return _depth(True)


def _ratio(n_red):
    b = Builder(5)
    b.query(0, [b.point([1, 2, 3], nobs=4) for _ in range(n_red)] + [b.point([1], nobs=4) for _ in range(20 - n_red)])
    return b.scene(), (20, n_red, 1 if n_red == 19 else 0)     # 0.9 * 20 = 18.0: 18 > 18.0 is false


def cull_ratio_18():
    return _ratio(18)


def cull_ratio_19():
    return _ratio(19)


CULL_CASES = dict(nobs_3_4=cull_nobs_3_4, octave=cull_octave, count_2_3=cull_2_3, own=cull_own, depth=cull_depth,
                  depth_monocular=cull_depth_monocular, ratio_18=cull_ratio_18, ratio_19=cull_ratio_19)


def expected_conn(exp_by_query):
    """The flat arrays of a list of hand-worked per-query answers."""
    out = dict(conn_start=[0], conn_kf=[], conn_weight=[], ordered_start=[0], ordered_kf=[], ordered_weight=[], n_max=[], kf_max=[],
               updated=[])
    for e in exp_by_query:
        out["conn_kf"] += [c[0] for c in e["conn"]]; out["conn_weight"] += [c[1] for c in e["conn"]]
        out["ordered_kf"] += [c[0] for c in e["ordered"]]; out["ordered_weight"] += [c[1] for c in e["ordered"]]
        out["conn_start"].append(len(out["conn_kf"])); out["ordered_start"].append(len(out["ordered_kf"]))
        out["n_max"].append(e["n_max"]); out["kf_max"].append(e["kf_max"]); out["updated"].append(e["updated"])
    return {k: np.array(v, np.uint8 if k == "updated" else np.int32) for k, v in out.items()}


def random_scene(seed, n_kf=40, n_points=300, obs_range=(2, 12), p_bad=0.05, th_depth=35.0, monocular=False, minus_one=False):
    """Every keyframe is a query over the points it observes (plus a few it does not), octaves 0-7, about a third of the depths
    beyond th_depth, some negative.  Weights straddle th = 15 at these sizes."""
    rng = np.random.default_rng(seed)
    b = Builder(n_kf, monocular)
    seen = [[] for _ in range(n_kf)]
    for p in range(n_points):
        k = int(rng.integers(obs_range[0], obs_range[1] + 1))
        kfs = sorted(rng.choice(n_kf, size=min(k, n_kf), replace=False).tolist())
        nobs = len(kfs) + int(rng.integers(0, len(kfs) + 1))        # some observations are stereo and weigh two
        b.point([(kf, int(rng.integers(0, 8))) for kf in kfs], bad=rng.random() < p_bad, nobs=nobs)
        for kf in kfs:
            seen[kf].append(p)
    for kf in range(n_kf):
        ents = list(seen[kf]) + rng.integers(0, n_points, 3).tolist()
        rng.shuffle(ents)
        depth = np.where(rng.random(len(ents)) < 0.33, th_depth + 1 + rng.random(len(ents)) * 10, rng.random(len(ents)) * th_depth)
        depth = np.where(rng.random(len(ents)) < 0.05, -1.0, depth)
        b.query(-1 if (minus_one and kf % 7 == 0) else kf, [(p, int(rng.integers(0, 8)), float(d)) for p, d in zip(ents, depth)], th_depth)
    return b.scene()


# ---- the object model of the C++ route -------------------------------------------------------------------------------------------
class KF:
    def __init__(self, idx, mn_id, th_depth, keys):
        self.idx, self.mn_id, self.th_depth = idx, mn_id, th_depth
        self.keys = keys                             # [(octave, depth, uright, point index or -1)]
        self.conn, self.ordered, self.ordered_w = {}, [], []
        self.first, self.parent, self.children, self.bad = True, -1, set(), False

    def update_best(self):                           # KeyFrame::UpdateBestCovisibles
        pairs = sorted((w, k) for k, w in self.conn.items())
        self.ordered = [k for w, k in reversed(pairs)]; self.ordered_w = [w for w, k in reversed(pairs)]

    def add_connection(self, k, w):                  # KeyFrame::AddConnection
        if self.conn.get(k) == w:
            return
        self.conn[k] = w
        self.update_best()


class World:
    """Keyframes live in one array, so pointer order is index order and a keyframe's slot is its index."""

    def __init__(self, kfs, n_points, monocular):
        self.kfs, self.monocular = kfs, monocular
        self.obs = [dict() for _ in range(n_points)]   # point -> {kf index: keypoint index}
        self.nobs = [0] * n_points
        self.bad = [False] * n_points
        for kf in kfs:
            for i, (_, _, ur, p) in enumerate(kf.keys):
                if p >= 0 and kf.idx not in self.obs[p]:            # MapPoint::AddObservation
                    self.obs[p][kf.idx] = i
                    self.nobs[p] += 2 if ur >= 0 else 1

    def flat(self, queries):
        b = Builder(len(self.kfs), self.monocular)
        for p, o in enumerate(self.obs):
            b.point([(k, self.kfs[k].keys[i][0]) for k, i in o.items()], bad=self.bad[p], nobs=self.nobs[p])
        for k in queries:
            kf = self.kfs[k]
            b.query(k, [(p, o, d) for (o, d, _, p) in kf.keys if p >= 0], kf.th_depth)
        return b.scene()

    def update_connections(self, lst):
        if not lst:
            return
        r = R.update_connections_ref(self.flat(lst))
        for q, k in enumerate(lst):
            if not r["updated"][q]:
                continue
            kf = self.kfs[k]
            s, e = r["ordered_start"][q], r["ordered_start"][q + 1]
            for j in sorted(range(s, e), key=lambda j: r["ordered_kf"][j]):      # AddConnection on the listed neighbours, in map order
                self.kfs[int(r["ordered_kf"][j])].add_connection(k, int(r["ordered_weight"][j]))
            cs, ce = r["conn_start"][q], r["conn_start"][q + 1]
            kf.conn = {int(r["conn_kf"][j]): int(r["conn_weight"][j]) for j in range(cs, ce)}
            kf.ordered = [int(x) for x in r["ordered_kf"][s:e]]; kf.ordered_w = [int(x) for x in r["ordered_weight"][s:e]]
            if kf.first and kf.mn_id != 0:
                kf.parent = kf.ordered[0]
                self.kfs[kf.parent].children.add(k)
                kf.first = False

    def set_bad_flag(self, k):
        kf = self.kfs[k]
        if kf.mn_id == 0:
            return
        for n in list(kf.conn):
            if k in self.kfs[n].conn:
                del self.kfs[n].conn[k]
                self.kfs[n].update_best()
        for i, (_, _, ur, p) in enumerate(kf.keys):
            if p >= 0 and k in self.obs[p]:
                i0 = self.obs[p].pop(k)
                self.nobs[p] -= 2 if kf.keys[i0][2] >= 0 else 1
                if self.nobs[p] <= 2:
                    self.bad[p] = True
        kf.conn, kf.ordered, kf.bad = {}, [], True      # mvOrderedWeights is not cleared there

    def keyframe_culling(self, current):
        """Returns (flagged keyframes in order, device calls the adapter makes)."""
        local = list(self.kfs[current].ordered)
        flagged, calls, at = [], 0, 0
        while at < len(local):
            rest = [(i, k) for i, k in enumerate(local) if i >= at and self.kfs[k].mn_id != 0]      # the origin is never culled
            if not rest:
                break
            r = R.keyframe_culling_ref(self.flat([k for _, k in rest])); calls += 1
            at = len(local)
            for q, (i, k) in enumerate(rest):
                if r["redundant"][q]:
                    self.set_bad_flag(k); flagged.append(k)      # observations are erased: count again for the rest
                    at = i + 1
                    break
        return flagged, calls

    def blob(self, update_list, current):
        out = struct.pack("<5i", len(self.kfs), len(self.obs), 1 if self.monocular else 0, len(update_list), current)
        for kf in self.kfs:
            out += struct.pack("<ifi", kf.mn_id, kf.th_depth, len(kf.keys))
            for (o, d, ur, p) in kf.keys:
                out += struct.pack("<iffi", o, d, ur, p)
        out += struct.pack("<%di" % len(update_list), *update_list)
        return out


def requery_world():
    """Six keyframes (0 is the origin, 5 the current one).  G1: 20 points seen by 0, 1, 2, 3, 5; G2: 16 stereo points seen by 1, 3,
    4, 5.  Keyframe 5 orders its neighbours [3, 1, 2, 0, 4] (36, 36, 20, 20, 16; ties by descending slot).  In one call every one
    of them is redundant.  Walking them: 3 is flagged, which leaves G2 with two other observers, so 1 (20 of 36) and 4 (0 of 16)
    are no longer redundant; 2 still is (G1 keeps 0, 1, 5); 0 is the origin.  So the flagged keyframes are [3, 2], in three calls."""
    g1, g2 = list(range(20)), list(range(20, 36))
    members = {0: g1, 1: g1 + g2, 2: g1, 3: g1 + g2, 4: g2, 5: g1 + g2}
    kfs = []
    for k in range(6):
        keys = []
        for j, p in enumerate(members[k]):
            keys.append((j % 2, 1.0 + j, 5.0 if p >= 20 else -1.0, p))     # octaves 0 / 1: never more than one level apart
            if j % 5 == 0:
                keys.append((0, 1.0, -1.0, -1))      # a keypoint without a map point
        kfs.append(KF(k, k, 60.0, keys))
    w = World(kfs, 36, False)
    return w, 5, dict(single_call=[3, 1, 2, 0, 4], flagged=[3, 2], calls=3)


def random_world(seed, n_kf=12, n_points=200, monocular=False):
    rng = np.random.default_rng(seed)
    keys = [[] for _ in range(n_kf)]
    for p in range(n_points):
        k = int(rng.integers(2, 7))
        base_oct = int(rng.integers(0, 6))
        for kf in rng.choice(n_kf, size=k, replace=False).tolist():
            keys[kf].append((base_oct + int(rng.integers(0, 3)), float(rng.random() * 50 - 2), 3.0 if rng.random() < 0.5 else -1.0, p))
    kfs = []
    for k in range(n_kf):
        ks = keys[k]
        rng.shuffle(ks)
        ks = [tuple(x) for x in ks]
        ks.insert(len(ks) // 2, (0, 1.0, -1.0, -1))
        kfs.append(KF(k, k, 35.0, ks))
    return World(kfs, n_points, monocular)
