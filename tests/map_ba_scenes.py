"""Small maps for the tests of lld_map_ba_window (tests/map_ba_ref.py holds the map format), their upload into a DeviceMap, and the
hand-worked scenes: maps small enough that the expected window is written out by hand below, next to the map.  numpy only, but for
map_of_window, which asks the library for a pose matrix.

Features follow fixed formulas, so that a window can be worked out on paper (N_LEVELS = 4, SIGMA2 = 1, 1/2, 1/4, 1/8):
  keypoint i of keyframe s   u = 100 s + i, v = 100 s + i + 0.5, uR = u - 2 (or -1), octave = i % 4
  keyline j of keyframe s    left = (100 s + j, 50 s + j, 100 s + j + 10, 50 s + j + 5), right = left - (3, 0, 3, 0), octaves (j % 4, (j + 1) % 4);
                             without a partner right = -1 four times and the right octave is 0
  pose of keyframe s         identity rotation, translation (s, 2 s, 3 s): SE3Quat (0, 0, 0, 1, s, 2 s, 3 s)
  point p                    (p, p + 0.5, p + 0.25);   line l: x0 = (l, 0.1 l, 2), dir = (0, 1, 0.001 l)"""
import numpy as np

N_LEVELS = 4
SIGMA2 = np.array([1.0, 0.5, 0.25, 0.125], np.float32)
CAM = (500.0, 510.0, 320.0, 240.0, 40.0)
LINE_DIM = 8


class Scene:
    """kf / pt / ln add objects; link() gives every point and line without an explicit row the observations its keyframes' rows imply, in
    ascending order_key (the iteration order of std::map<KeyFrame*, size_t>)."""

    def __init__(self):
        self.m = dict(keyframes={}, points={}, lines={})

    def kf(self, s, mn_id, points=(), lines=(), bad=0, key=None, mono=(), no_partner=(), features=True, keypoints=True):
        points, lines = list(points), list(lines)
        k = dict(key=int(1000 + s if key is None else key), bad=int(bad), points=points, lines=lines)
        i = np.arange(len(points)); j = np.arange(len(lines))
        if features:
            u = (100 * s + i).astype(np.float32)
            ur = np.where(np.isin(i, list(mono)), np.float32(-1), u - 2).astype(np.float32)
            left = np.stack([100 * s + j, 50 * s + j, 100 * s + j + 10, 50 * s + j + 5], 1).astype(np.float32).reshape(-1, 4)
            lone = np.isin(j, list(no_partner))
            right = np.where(lone[:, None], np.float32(-1), left - np.array([3, 0, 3, 0], np.float32)).astype(np.float32).reshape(-1, 4)
            k.update(mn_id=int(mn_id), Tcw=pose(s), uvr=np.stack([u, u + np.float32(0.5), ur], 1).astype(np.float32).reshape(-1, 3), kl_left=left, kl_right=right,
                     kl_octave=np.stack([j % 4, np.where(lone, 0, (j + 1) % 4)], 1).astype(np.int32).reshape(-1, 2))
        if keypoints:
            k["octave"] = (i % 4).tolist()
        self.m["keyframes"][s] = k
        return k

    def pt(self, p, bad=0, obs=None, indexed=True):
        self.m["points"][p] = dict(bad=int(bad), pos=np.array([p, p + 0.5, p + 0.25], np.float32), obs=obs, indexed=indexed)

    def ln(self, l, bad=0, obs=None, n_obs=None, no_row=False):
        self.m["lines"][l] = dict(bad=int(bad), x0=np.array([l, 0.1 * l, 2.0]), dir=np.array([0.0, 1.0, 0.001 * l]), obs=obs, n_obs=n_obs, no_row=no_row)

    def link(self):
        K = self.m["keyframes"]
        order = sorted(K, key=lambda s: K[s]["key"])
        for what, rows in (("points", "points"), ("lines", "lines")):
            for x, o in self.m[what].items():
                if o["obs"] is None and not o.get("no_row"):
                    o["obs"] = [(s, K[s][rows].index(x)) for s in order if x in K[s][rows]]
        for o in self.m["lines"].values():
            if o["n_obs"] is None:
                o["n_obs"] = 0 if o["obs"] is None else len(o["obs"])
            o.pop("no_row")
        return self.m


def pose(s):
    T = np.eye(4, dtype=np.float32); T[:3, 3] = [s, 2 * s, 3 * s]
    return T


def random_pose(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4, dtype=np.float32); T[:3, :3] = R; T[:3, 3] = rng.normal(size=3) * 3
    return T


def limits_for(m, **over):
    K = m["keyframes"].values()
    L = dict(max_keyframes=max(m["keyframes"], default=0) + 2, max_points=max([p for k in K for p in k["points"]] + list(m["points"]) + [0]) + 2,
             max_lines=max([l for k in K for l in k["lines"]] + list(m["lines"]) + [0]) + 2, line_dim=LINE_DIM,
             max_observations=sum(len(p["obs"]) for p in m["points"].values()) + 8, max_kf_points=sum(len(k["points"]) for k in K) + 8,
             max_kf_lines=max(sum(len(k["lines"]) for k in K), sum(len(l["obs"] or ()) for l in m["lines"].values())) + 8, max_children=8,
             max_local_points=64, max_local_lines=16)
    L.update(over)
    return L


# ---------------------------------------------------------------------------------------------------------------- uploading a map dict
def upload_keyframes(dm, m, slots=None, rows=True, keypoints=True, features=True):
    slots = sorted(m["keyframes"]) if slots is None else list(slots)
    K = [m["keyframes"][s] for s in slots]
    none = [[] for _ in slots]
    if rows:
        dm.set_keyframes(slots, [k["key"] for k in K], [k["bad"] for k in K], [-1] * len(slots), none, none, [k["points"] for k in K], [k["lines"] for k in K])
    kp = [(s, k) for s, k in zip(slots, K) if k.get("octave") is not None]
    if keypoints and kp:
        dm.set_keyframe_keypoints([s for s, _ in kp], [k["octave"] for _, k in kp], [[0.0] * len(k["octave"]) for _, k in kp], [0.0] * len(kp))
    ft = [(s, k) for s, k in zip(slots, K) if "uvr" in k]
    if features and ft:
        dm.set_keyframe_features([s for s, _ in ft], [k["mn_id"] for _, k in ft], [k["Tcw"] for _, k in ft], [k["uvr"] for _, k in ft], [k["kl_left"] for _, k in ft],
                                 [k["kl_right"] for _, k in ft], [k["kl_octave"] for _, k in ft])


def upload_points(dm, m, slots=None):
    slots = sorted(m["points"]) if slots is None else list(slots)
    if not slots:
        return
    n = len(slots)
    P = [m["points"][s] for s in slots]
    z = lambda *shape: np.zeros((n,) + shape, np.float32)
    dm.set_points(slots, np.array([p["pos"] for p in P], np.float32), z(3), z(), z(), np.zeros((n, 8), np.uint32), [p["bad"] for p in P])
    ix = [(s, p) for s, p in zip(slots, P) if p.get("indexed", True)]
    if ix:
        dm.set_observations_indexed([s for s, _ in ix], rows=[p["obs"] for _, p in ix], n_obs=[len(p["obs"]) for _, p in ix])
    pl = [(s, p) for s, p in zip(slots, P) if not p.get("indexed", True)]
    if pl:
        dm.set_observations([s for s, _ in pl], rows=[[o[0] for o in p["obs"]] for _, p in pl])


def upload_lines(dm, m, slots=None):
    slots = sorted(m["lines"]) if slots is None else list(slots)
    if not slots:
        return
    n = len(slots)
    Ls = [m["lines"][s] for s in slots]
    x0 = np.array([l["x0"] for l in Ls], np.float64); d = np.array([l["dir"] for l in Ls], np.float64)
    dm.set_lines(slots, x0, d, x0, x0 + d, np.zeros((n, LINE_DIM), np.float32), [l["bad"] for l in Ls])
    ob = [(s, l) for s, l in zip(slots, Ls) if l["obs"] is not None]
    if ob:
        dm.set_line_observations([s for s, _ in ob], [l["obs"] for _, l in ob], [l["n_obs"] for _, l in ob])


def upload(dm, m):
    upload_keyframes(dm, m); upload_points(dm, m); upload_lines(dm, m)


# ---------------------------------------------------------------------------------------------------------------- random maps
def random_map(seed, n_kf=12, n_kp=64, n_pts=300, n_lines=40, n_kl=10):
    """A map and a query.  Slot order, order_key order and mn_id order are three different shuffles; some keyframes are bad; some points and
    lines are bad, some slots in the rows were never set; the stored order of every observation row is ascending order_key."""
    rng = np.random.default_rng(0xBA5E + seed)
    sc = Scene()
    kf_slots = rng.permutation(16)[:n_kf].tolist()
    keys = [int(k) for k in rng.integers(1, 2 ** 64 - 2, n_kf, dtype=np.uint64)]
    mn_ids = rng.permutation(3 * n_kf)[:n_kf].tolist()
    if seed % 2 == 0 and 0 not in mn_ids:
        mn_ids[int(rng.integers(0, n_kf))] = 0
    pt_slots = rng.permutation(512)[:n_pts].tolist()
    ln_slots = rng.permutation(64)[:n_lines].tolist()
    for s, key, mn in zip(kf_slots, keys, mn_ids):
        pts = rng.permutation(n_pts)[:n_kp]
        row = [int(pt_slots[j]) if rng.random() < 0.75 else -1 for j in pts]
        lns = rng.permutation(n_lines)[:n_kl]
        lrow = [int(ln_slots[j]) if rng.random() < 0.85 else -1 for j in lns]
        k = sc.kf(s, mn, row, lrow, bad=rng.random() < 0.15, key=key, mono=np.flatnonzero(rng.random(n_kp) < 0.2), no_partner=np.flatnonzero(rng.random(n_kl) < 0.3))
        k["Tcw"] = random_pose(rng)
        k["uvr"] = (k["uvr"] + rng.random(k["uvr"].shape).astype(np.float32) * (k["uvr"] >= 0)).astype(np.float32)
        k["octave"] = rng.integers(0, N_LEVELS, n_kp).tolist()
    for p in pt_slots:
        if rng.random() < 0.97:                                            # the others stay never set
            sc.pt(p, bad=rng.random() < 0.06)
    for l in ln_slots:
        if rng.random() < 0.95:
            sc.ln(l, bad=rng.random() < 0.1)
    m = sc.link()
    for l in m["lines"].values():
        l["n_obs"] = len(l["obs"]) + int(rng.integers(0, 3))               # stereo observations count twice
        l["x0"] = rng.normal(size=3); l["dir"] = rng.normal(size=3)
    for p in m["points"].values():
        p["pos"] = rng.normal(size=3).astype(np.float32)
    others = rng.permutation(kf_slots).tolist()
    lo = min(4, n_kf - 2)
    query = others[:int(rng.integers(lo, max(lo + 1, n_kf - 2)))]              # some keyframes stay outside: the fixed cameras
    return m, query


# ---------------------------------------------------------------------------------------------------------------- a synthetic BA window as a map
def map_of_window(w, seed):
    """A synthetic window as a map: cameras become keyframes (slots and order keys shuffled), every observation a keypoint or keyline of its
    camera, points and lines get their observation rows.  The free cameras are the query; the first fixed camera joins it with mn_id 0."""
    rng = np.random.default_rng(seed)
    from lld_slam_amd import abi, host
    lib = abi.product()
    nc = w.n_cams
    slot = rng.permutation(nc + 3)[:nc].tolist()
    key = [int(k) for k in rng.integers(1, 2 ** 63, nc)]
    mn = (rng.permutation(4 * nc)[:nc] + 1).tolist()
    mn[w.n_free_cams] = 0
    table = np.unique(w.pt_obs_inv_sigma2.astype(np.float32))[::-1].copy()
    rows = [dict(points=[], uvr=[], octave=[], lines=[], left=[], right=[], loct=[]) for _ in range(nc)]
    m = dict(keyframes={}, points={}, lines={})
    for p in range(w.n_points):
        obs = []
        for e in range(w.pt_obs_start[p], w.pt_obs_start[p + 1]):
            c = int(w.pt_obs_cam[e]); r = rows[c]
            obs.append((key[c], slot[c], len(r["points"])))
            r["points"].append(p); r["uvr"].append(w.pt_obs_uvr[e]); r["octave"].append(int(np.flatnonzero(table == np.float32(w.pt_obs_inv_sigma2[e]))[0]))
        m["points"][p] = dict(bad=0, pos=w.pt_xyz[p].astype(np.float32), obs=[(s, i) for _, s, i in sorted(obs)], indexed=True)
    for l in range(w.n_lines):
        obs = []
        for e in range(w.ln_obs_start[l], w.ln_obs_start[l + 1]):
            c = int(w.ln_obs_cam[e]); r = rows[c]
            obs.append((key[c], slot[c], len(r["lines"])))
            r["lines"].append(l); r["left"].append(w.ln_obs_left[e]); r["right"].append(w.ln_obs_right[e]); r["loct"].append(w.ln_obs_octave[e])
        m["lines"][l] = dict(bad=0, x0=w.line_x0[l].copy(), dir=w.line_dir[l].copy(), obs=[(s, i) for _, s, i in sorted(obs)], n_obs=2 * len(obs))
    for c in range(nc):
        r = rows[c]
        m["keyframes"][slot[c]] = dict(key=key[c], bad=0, points=r["points"], lines=r["lines"], mn_id=mn[c], Tcw=host.se3_to_tcw_f32(lib, w.cam_qt[c]),
                                       uvr=np.array(r["uvr"], np.float32).reshape(-1, 3), octave=r["octave"], kl_left=np.array(r["left"], np.float32).reshape(-1, 4),
                                       kl_right=np.array(r["right"], np.float32).reshape(-1, 4), kl_octave=np.array(r["loct"], np.int32).reshape(-1, 2))
    free = rng.permutation(w.n_free_cams).tolist()
    query = [slot[c] for c in free] + [slot[w.n_free_cams]]
    return m, query, table


# ---------------------------------------------------------------------------------------------------------------- the named scenes
def bad_neighbour():
    """1: keyframe 1 is bad and a neighbour: marked local, not listed, never fixed.  Point 2 is seen by it and by 3 only: not local."""
    sc = Scene()
    sc.kf(0, 5, [0, 1]); sc.kf(1, 6, [0, 2], bad=1); sc.kf(2, 7, [1, 3]); sc.kf(3, 8, [3, 2])
    for p in range(4): sc.pt(p)
    return sc.link(), [0, 1, 2]


def pkf_bad():
    """2: kf_slot[0] is bad: it is a camera all the same, its points are local, its observations are dropped."""
    sc = Scene()
    sc.kf(0, 5, [0, 1], bad=1); sc.kf(1, 6, [1, 2]); sc.kf(2, 7, [0])
    for p in range(3): sc.pt(p)
    return sc.link(), [0, 1]


def mn_id_zero():
    """3: the local keyframe with mn_id 0 goes behind the free cameras; slot order, key order and mn_id order all differ."""
    sc = Scene()
    sc.kf(4, 3, [0, 1], key=30); sc.kf(2, 0, [1, 2], key=10); sc.kf(7, 1, [2, 0], key=20); sc.kf(1, 9, [0], key=5)
    for p in range(3): sc.pt(p)
    return sc.link(), [4, 2, 7]


def first_occurrence():
    """4: point 5 is keypoint 2 of the second listed keyframe and keypoint 0 of the third: listed once, where the second has it."""
    sc = Scene()
    sc.kf(0, 1, [9, 8]); sc.kf(1, 2, [7, 6, 5]); sc.kf(2, 3, [5, 9, 4])
    for p in (4, 5, 6, 7, 8, 9): sc.pt(p)
    return sc.link(), [0, 1, 2]


def skipped_entries():
    """5: a bad point, a slot never set and a -1 in the rows."""
    sc = Scene()
    sc.kf(0, 1, [0, -1, 1, 2, 3], [0, -1, 1, 2]); sc.kf(1, 2, [3, 1, -1], [2, 0, 1])
    sc.pt(0); sc.pt(1, bad=1); sc.pt(3)                                    # 2 never set
    sc.ln(0, n_obs=4); sc.ln(1, bad=1, n_obs=4)                            # 2 never set
    return sc.link(), [0, 1]


def line_counts():
    """6: line 0 has n_obs 3 (skipped, unmarked), line 1 has n_obs 4 in a row of two (stereo observations count twice)."""
    sc = Scene()
    sc.kf(0, 1, [0], [0, 1]); sc.kf(1, 2, [0], [1, 0]); sc.kf(2, 3, [], [0])
    sc.pt(0); sc.ln(0, n_obs=3); sc.ln(1, n_obs=4)
    return sc.link(), [0, 1]


def line_order():
    """7: the observers of line 0 in pointer (key) order are 2, 1, 0; in mn_id order 0, 1, 2."""
    sc = Scene()
    sc.kf(0, 1, [0], [0], key=30); sc.kf(1, 2, [0], [-1, 0], key=20); sc.kf(2, 3, [0], [0], key=10)
    sc.pt(0); sc.ln(0, n_obs=6)
    return sc.link(), [0, 1]


def fixed_through_line():
    """8: keyframe 3 sees no local point, only local line 0; keyframe 2 is fixed through point 0, which is walked first."""
    sc = Scene()
    sc.kf(0, 4, [0], [0]); sc.kf(1, 5, [0], [0]); sc.kf(2, 6, [0, 1], []); sc.kf(3, 7, [1], [0, 1], key=1)
    sc.pt(0); sc.pt(1); sc.ln(0, n_obs=5); sc.ln(1, n_obs=4)
    return sc.link(), [0, 1]


def bad_observer_inside():
    """9: the row of point 0 is keyframes 3, 1 (bad), 2, 0 in stored order."""
    sc = Scene()
    sc.kf(0, 1, [0], key=40); sc.kf(1, 2, [0], bad=1, key=20); sc.kf(2, 3, [5, 0], key=30); sc.kf(3, 4, [6, 7, 0], key=10)
    sc.pt(0)
    return sc.link(), [0, 2]


def never_set_observer():
    """9b: the same row with a keyframe slot in it that was never set (slot 4): bad, like keyframe 1 - marked fixed, no camera, not in the run."""
    m, q = bad_observer_inside()
    m["points"][0]["obs"].insert(1, (4, 0))
    return m, q


def empty_run():
    """10: point 1 is seen by the bad kf_slot[0] alone, point 2 has an empty row: both stay in the window with empty runs."""
    sc = Scene()
    sc.kf(0, 1, [0, 1, 2], bad=1); sc.kf(1, 2, [0])
    sc.pt(0); sc.pt(1); sc.pt(2, obs=[])
    return sc.link(), [0, 1]


def monocular():
    """11: keypoints without a right coordinate."""
    sc = Scene()
    sc.kf(0, 1, [0, 1, 2], mono=[0, 2]); sc.kf(1, 2, [2, 1, 0], mono=[1])
    for p in range(3): sc.pt(p)
    return sc.link(), [0, 1]


def lone_line():
    """12: a left keyline without a partner: right = -1, right octave 0."""
    sc = Scene()
    sc.kf(0, 1, [0], [0, 1], no_partner=[1]); sc.kf(1, 2, [0], [1, 0], no_partner=[0, 1])
    sc.pt(0); sc.ln(0, n_obs=4); sc.ln(1, n_obs=4)
    return sc.link(), [0, 1]


def no_lines():
    """13: a map without lines."""
    sc = Scene()
    sc.kf(0, 1, [0, 1]); sc.kf(1, 2, [1, 0]); sc.kf(2, 3, [1])
    sc.pt(0); sc.pt(1)
    return sc.link(), [0, 1]


def trip(n_points, n_lines):
    """n_points local points and n_lines local lines in the row of keyframe 0 (slot 4), past the 8 192 landmarks one trip of the grid-stride
    kernels covers.  Observers, written out (link() would search every row for every landmark): keyframe 0 all of them, local keyframe 1
    (slot 2) every 1 000th point, the last three points and every line, fixed keyframe 2 (slot 0) the last two points and the odd lines,
    bad keyframe 3 (slot 1) the last point and the last line."""
    sc = Scene()
    P, Ls = list(range(n_points)), list(range(n_lines))
    rows = {4: P, 2: sorted(set(P[::1000] + P[-3:])), 0: P[-2:], 1: P[-1:]}
    lrows = {4: Ls, 2: Ls[::-1], 0: Ls[1::2], 1: Ls[-1:]}
    for s, mn, key, bad in ((4, 7, 40, 0), (2, 3, 10, 0), (0, 9, 30, 0), (1, 5, 20, 1)):
        sc.kf(s, mn, rows[s], lrows[s], bad=bad, key=key, mono=[1], no_partner=[0])
    order = (2, 1, 0, 4)                                                   # ascending order_key
    at = {s: {p: i for i, p in enumerate(rows[s])} for s in rows}; lat = {s: {l: i for i, l in enumerate(lrows[s])} for s in lrows}
    for p in P: sc.pt(p, obs=[(s, at[s][p]) for s in order if p in at[s]])
    for l in Ls: sc.ln(l, obs=[(s, lat[s][l]) for s in order if l in lat[s]], n_obs=4)
    return sc.link(), [4, 2]


def line_rows(n):
    """n local lines in the row of keyframe 0, between them a -1 at every 16th entry, a bad line at every 21st, one with three observations
    at every 25th and, at entry 256, entry 200 again; fixed keyframe 1 observes all of them, local keyframe 2 every third (and lists five
    of them before its own)."""
    sc = Scene()
    row, live, j = [], [], 0
    while len(live) < n:
        k = len(row)
        if k == 256: row.append(row[200])
        elif k % 16 == 5: row.append(-1)
        else:
            row.append(j)
            if k % 21 != 9 and k % 25 != 13: live.append(j)
            j += 1
    others = [l for l in row if l >= 0 and l not in set(live)]
    assert row[200] in live and len(set(live)) == n
    row1 = [l for l in dict.fromkeys(row) if l >= 0][::-1]
    row2 = live[7:40:8] + [j, j + 1] + live[::3]
    sc.kf(0, 3, [0], row); sc.kf(1, 1, [0], row1, key=5, no_partner=range(0, len(row1), 4)); sc.kf(2, 2, [1, 0], row2, key=2000)
    sc.pt(0); sc.pt(1)
    for k, l in enumerate(others): sc.ln(l, bad=k % 2 == 0, n_obs=4 if k % 2 == 0 else 3)
    for l in live + [j, j + 1]: sc.ln(l, n_obs=4 + l % 3)
    return sc.link(), [0, 2]


def local_spread(n):
    """n listed keyframes, mn_id and order_key each scrambled against slot order, every eleventh bad; each has two points and a line of its
    own, every fourth one of an earlier keyframe's points and every sixth an earlier one's line."""
    sc = Scene()
    for s in range(n):
        pts = [2 * s, 2 * s + 1] + ([2 * ((s * 5) % max(s, 1))] if s % 4 == 0 else [])
        lns = [s] + ([(s * 7) % max(s, 1)] if s % 6 == 0 else [])
        sc.kf(s, 1 + (s * 389) % n, pts, lns, bad=(s % 11 == 5), key=5000 + (s * 77) % n)
    for p in range(2 * n): sc.pt(p)
    for l in range(n): sc.ln(l, n_obs=4)
    return sc.link(), list(range(n))


def fixed_cameras(n):
    """three local keyframes with 40 points and two lines each; n other keyframes (every thirteenth bad) observe one to three of the points
    and every tenth a line, order_key scrambled against slot order: first visits spread over the landmarks and over the rows' positions"""
    sc = Scene()
    for s in range(3): sc.kf(s, s + 1, list(range(40 * s, 40 * s + 40)), [2 * s, 2 * s + 1], key=10 ** 6 + s)
    for f in range(n):
        pts = sorted({(f * 37) % 120, (f * 53 + 7) % 120} | ({(f * 11) % 120} if f % 3 == 0 else set()))
        sc.kf(3 + f, 10 + f, pts, [f % 6] if f % 10 == 0 else [], bad=(f % 13 == 6), key=1000 + 3 * ((f * 389) % n))
    for p in range(120): sc.pt(p)
    for l in range(6): sc.ln(l, n_obs=4)
    return sc.link(), [0, 1, 2]


def wide(n_points=None, n_observers=None, n_line_observers=None, n_local=None, n_lines=None, n_local_spread=None, n_fixed=None):
    """14: one past a width.  n_points local points in one keyframe; a point with n_observers observers; a line with n_line_observers
    observers (mn_id descending along the row); n_local listed keyframes.  Past 8 192 landmarks: trip(n_points, n_lines or 0).
    n_lines alone: line_rows; n_local_spread: local_spread; n_fixed: fixed_cameras."""
    if n_points and n_points > 8000: return trip(n_points, n_lines or 0)
    if n_lines: return line_rows(n_lines)
    if n_local_spread: return local_spread(n_local_spread)
    if n_fixed: return fixed_cameras(n_fixed)
    sc = Scene()
    if n_points:
        sc.kf(0, 1, list(range(n_points))); sc.kf(1, 2, [3, 1])
        for p in range(n_points): sc.pt(p)
        return sc.link(), [0, 1]
    if n_observers:
        for s in range(n_observers): sc.kf(s, n_observers - s, [0, s + 1], bad=(s % 7 == 3))
        for p in range(n_observers + 1): sc.pt(p)
        return sc.link(), [0, 1, 2]
    if n_line_observers:
        for s in range(n_line_observers): sc.kf(s, 2 * n_line_observers - s, [0], [0], bad=(s % 9 == 4))
        sc.pt(0); sc.ln(0, n_obs=2 * n_line_observers)
        return sc.link(), [0, 1, 2]
    for s in range(n_local + 1): sc.kf(s, (s * 7919) % 2003 + (s > 1000) * 2003, [s % 5, (s + 1) % 5], [s % 3], bad=(s % 11 == 5))
    for p in range(5): sc.pt(p)
    for l in range(3): sc.ln(l, n_obs=4)
    return sc.link(), list(range(n_local))


NAMED = dict(bad_neighbour=bad_neighbour, pkf_bad=pkf_bad, mn_id_zero=mn_id_zero, first_occurrence=first_occurrence, skipped_entries=skipped_entries,
             line_counts=line_counts, line_order=line_order, fixed_through_line=fixed_through_line, bad_observer_inside=bad_observer_inside, never_set_observer=never_set_observer,
             empty_run=empty_run, monocular=monocular, lone_line=lone_line, no_lines=no_lines)

# ---------------------------------------------------------------------------------------------------------------- worked out by hand
# Only what the rules decide is written out: the lists, the runs, and one column per feature array (u of uvr, xs of left / right).
HAND = dict(
    # listed 0, 2 (1 is bad).  Points: kf 0 gives 0, 1; kf 2 gives 3 (1 is there already).  Point 2 is not local.  Rows in key order
    # (1000 + slot): point 0 = kf 0 (kp 0), kf 1 bad; point 1 = kf 0 (kp 1), kf 2 (kp 0); point 3 = kf 2 (kp 1), kf 3 (kp 0) -> 3 is fixed.
    # Cameras by mn_id: 0 (5), 2 (7); then fixed 3.
    bad_neighbour=dict(cam_slot=[0, 2, 3], n_free_cams=2, n_local_cams=2, point_slot=[0, 1, 3], pt_obs_start=[0, 1, 3, 5], pt_obs_cam=[0, 0, 1, 1, 2],
                       pt_u=[0, 1, 200, 201, 300], pt_sig=[1, 0.5, 1, 0.5, 1], line_slot=[], ln_obs_start=[0], ln_obs_cam=[]),
    # listed 4, 2, 7.  mn_id: 4 -> 3, 2 -> 0, 7 -> 1, 1 -> 9.  Free cameras by mn_id: 7 (1), 4 (3); then 2 (mn_id 0); fixed: 1 (sees point 0).
    # Points: kf 4 gives 0, 1; kf 2 gives 2.  Key order: 1 (5), 2 (10), 7 (20), 4 (30).
    # point 0: kf 1 kp 0, kf 7 kp 1, kf 4 kp 0; point 1: kf 2 kp 0, kf 4 kp 1; point 2: kf 2 kp 1, kf 7 kp 0.
    mn_id_zero=dict(cam_slot=[7, 4, 2, 1], n_free_cams=2, n_local_cams=3, point_slot=[0, 1, 2], pt_obs_start=[0, 3, 5, 7], pt_obs_cam=[3, 0, 1, 2, 1, 2, 0],
                    pt_u=[100, 701, 400, 200, 401, 201, 700], pt_sig=[1, 0.5, 1, 1, 0.5, 0.5, 1], line_slot=[], ln_obs_start=[0], ln_obs_cam=[]),
    # listed 0, 1.  Line 0: n_obs 6, observers in key order 2 (kl 0), 1 (kl 1), 0 (kl 0); by mn_id 0 (1), 1 (2), 2 (3).  Keyframe 2 is fixed,
    # first met through point 0 (row: 2, 1, 0).  Cameras: 0, 1, 2.
    line_order=dict(cam_slot=[0, 1, 2], n_free_cams=2, n_local_cams=2, point_slot=[0], pt_obs_start=[0, 3], pt_obs_cam=[2, 1, 0], pt_u=[200, 100, 0],
                    pt_sig=[1, 1, 1], line_slot=[0], ln_obs_start=[0, 3], ln_obs_cam=[0, 1, 2], ln_left_xs=[0, 101, 200], ln_right_xs=[-3, 98, 197],
                    ln_obs_octave=[[0, 1], [1, 2], [0, 1]]),
    # listed 0, 1.  Point 0: rows of 0, 1, 2 -> key order 0, 1, 2: 2 becomes fixed first.  Point 1 is not local.  Line 0 (n_obs 5): key order
    # 3 (key 1, kl 0), 0, 1 -> 3 becomes fixed second; by mn_id: 0 (4), 1 (5), 3 (7).  Line 1 is seen by 3 only: not local.
    fixed_through_line=dict(cam_slot=[0, 1, 2, 3], n_free_cams=2, n_local_cams=2, point_slot=[0], pt_obs_start=[0, 3], pt_obs_cam=[0, 1, 2], pt_u=[0, 100, 200],
                            pt_sig=[1, 1, 1], line_slot=[0], ln_obs_start=[0, 3], ln_obs_cam=[0, 1, 3], ln_left_xs=[0, 100, 300], ln_right_xs=[-3, 97, 297],
                            ln_obs_octave=[[0, 1], [0, 1], [0, 1]]),
    # listed 0 (bad, first) and 1.  Points 0, 1, 2.  Point 0: observers 0 (bad, dropped), 1 -> camera 1 (mn_id 2), kp 0 of kf 1.
    empty_run=dict(cam_slot=[0, 1], n_free_cams=2, n_local_cams=2, point_slot=[0, 1, 2], pt_obs_start=[0, 1, 1, 1], pt_obs_cam=[1], pt_u=[100], pt_sig=[1],
                   line_slot=[], ln_obs_start=[0], ln_obs_cam=[]),
    # line 0 has n_obs 3: skipped.  Line 1 (n_obs 4): kf 0 kl 1, kf 1 kl 0.
    line_counts=dict(cam_slot=[0, 1], n_free_cams=2, n_local_cams=2, point_slot=[0], pt_obs_start=[0, 2], pt_obs_cam=[0, 1], pt_u=[0, 100], pt_sig=[1, 1],
                     line_slot=[1], ln_obs_start=[0, 2], ln_obs_cam=[0, 1], ln_left_xs=[1, 100], ln_right_xs=[-2, 97], ln_obs_octave=[[1, 2], [0, 1]]),
)
