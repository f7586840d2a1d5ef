"""Small maps for the resident-map tests (tests/local_map_ref.py holds the format).  A scene is a dict: map, limits (lld_map_limits as
keywords), steps - each {"frame": [point slot per keypoint]} (one UpdateLocalMap) or {"bad_points": [slots]} (a change of the map between
two frames).  Every scene is a few kilobytes.  numpy only."""
import numpy as np

LINE_DIM = 8


class Builder:
    def __init__(self):
        self.m = dict(keyframes={}, points={}, lines={})

    def kf(self, slot, key, bad=0, parent=None, cov=(), child=(), points=(), lines=()):
        self.m["keyframes"][slot] = dict(key=int(key), bad=int(bad), parent=parent, cov=list(cov), child=list(child), points=list(points), lines=list(lines))

    def pt(self, slot, obs=(), bad=0):
        self.m["points"][slot] = dict(bad=int(bad), obs=list(obs))

    def ln(self, slot, bad=0):
        self.m["lines"][slot] = dict(bad=int(bad))


def limits_for(m, max_local_points=512, max_local_lines=64, **over):
    tot = lambda k: sum(len(kf[k]) for kf in m["keyframes"].values())
    L = dict(max_keyframes=max(m["keyframes"], default=0) + 1, max_points=max(m["points"], default=0) + 1, max_lines=max(m["lines"], default=0) + 1,
             line_dim=LINE_DIM, max_observations=sum(len(p["obs"]) for p in m["points"].values()) + 8, max_kf_points=tot("points") + 8,
             max_kf_lines=tot("lines") + 8, max_children=tot("child") + 8, max_local_points=max_local_points, max_local_lines=max_local_lines)
    L.update(over)
    return L


def scene(name, b, steps, **lim):
    return dict(name=name, map=b.m, limits=limits_for(b.m, **lim), steps=steps)


# ---------------------------------------------------------------------------------------------------------------- uploading a map dict
def upload_keyframes(dm, m, slots=None):
    slots = sorted(m["keyframes"]) if slots is None else list(slots)
    if not slots:
        return
    K = [m["keyframes"][s] for s in slots]
    dm.set_keyframes(slots, [k["key"] for k in K], [k["bad"] for k in K], [-1 if k["parent"] is None else k["parent"] for k in K],
                     [k["cov"] for k in K], [k["child"] for k in K], [k["points"] for k in K], [k["lines"] for k in K])


def upload_points(dm, m, slots=None, data=None):
    """data: optional dict slot -> dict(world_pos, normal, min_distance, max_distance, desc); zeros otherwise."""
    slots = sorted(m["points"]) if slots is None else list(slots)
    if not slots:
        return
    n = len(slots)
    get = lambda k, shape, dt: np.array([data[s][k] for s in slots], dt).reshape((n,) + shape) if data else np.zeros((n,) + shape, dt)
    dm.set_points(slots, get("world_pos", (3,), np.float32), get("normal", (3,), np.float32), get("min_distance", (), np.float32),
                  get("max_distance", (), np.float32), get("desc", (8,), np.uint32), [m["points"][s]["bad"] for s in slots])
    dm.set_observations(slots, rows=[m["points"][s]["obs"] for s in slots])


def upload_lines(dm, m, slots=None, data=None, dim=LINE_DIM):
    slots = sorted(m["lines"]) if slots is None else list(slots)
    if not slots:
        return
    n = len(slots)
    get = lambda k, shape, dt: np.array([data[s][k] for s in slots], dt).reshape((n,) + shape) if data else np.zeros((n,) + shape, dt)
    dm.set_lines(slots, get("X0", (3,), np.float64), get("dir", (3,), np.float64), get("X1", (3,), np.float64), get("X2", (3,), np.float64),
                 get("desc", (dim,), np.float32), [m["lines"][s]["bad"] for s in slots])


def upload(dm, m, point_data=None, line_data=None, dim=LINE_DIM):
    upload_keyframes(dm, m); upload_points(dm, m, data=point_data); upload_lines(dm, m, data=line_data, dim=dim)


# ---------------------------------------------------------------------------------------------------------------- the scenes
def random_map(seed, n_kf=12, n_kp=64, n_pts=300, n_lines=40, n_frame=200):
    rng = np.random.default_rng(0x10CA1 + seed)
    b = Builder()
    kf_slots = rng.permutation(16)[:n_kf].tolist()                       # slot order shuffled against key order
    keys = [int(k) for k in rng.integers(1, 2 ** 64 - 2, n_kf, dtype=np.uint64)]
    pt_slots = rng.permutation(512)[:n_pts].tolist()
    ln_slots = rng.permutation(64)[:n_lines].tolist()
    by_key = [s for _, s in sorted(zip(keys, kf_slots))]
    rows = {s: [int(pt_slots[j]) if rng.random() < 0.7 else -1 for j in rng.integers(0, n_pts, n_kp)] for s in kf_slots}
    lrows = {s: [int(ln_slots[j]) if rng.random() < 0.8 else -1 for j in rng.integers(0, n_lines, 8)] for s in kf_slots}
    parent = {s: (None if i == 0 or rng.random() < 0.2 else by_key[int(rng.integers(0, i))]) for i, s in enumerate(by_key)}
    for s, k in zip(kf_slots, keys):
        others = [o for o in kf_slots if o != s]
        cov = rng.permutation(others)[:int(rng.integers(0, 12))].tolist()
        child = [c for c in kf_slots if parent[c] == s] + ([int(rng.choice(others))] if rng.random() < 0.3 else [])
        b.kf(s, k, bad=rng.random() < 0.12, parent=parent[s], cov=cov, child=rng.permutation(child).tolist(), points=rows[s], lines=lrows[s])
    for p in pt_slots:
        obs = [s for s in kf_slots if p in rows[s]]
        b.pt(p, obs=rng.permutation(obs).tolist(), bad=rng.random() < 0.06)
    for l in ln_slots:
        b.ln(l, bad=rng.random() < 0.1)
    ids = []
    for _ in range(n_frame):
        r = rng.random()
        ids.append(-1 if r < 0.3 else 512 + int(rng.integers(0, 50)) if r < 0.36 else int(rng.integers(0, 512)))     # NULL, temporal, a slot (set or not)
    return scene("random%d" % seed, b, [{"frame": ids}])


def chain_of(b, n, first_slot=0, pts_each=1, key=lambda i: 100 + i):
    """n keyframes, keyframe i observing pts_each points of its own; returns the frame ids that vote for all of them."""
    ids = []
    for i in range(n):
        ps = [first_slot + i * pts_each + j for j in range(pts_each)]
        b.kf(i, key(i), points=ps)
        for p in ps:
            b.pt(p, obs=[i]); ids.append(p)
    return ids


def empty_vote():
    b = Builder()
    b.kf(0, 10, points=[0, 1, 2], lines=[0]); b.kf(1, 20, points=[2, 3], parent=0)
    for p, o in ((0, [0]), (1, [0]), (2, [0, 1]), (3, [1])):
        b.pt(p, obs=o)
    b.ln(0)
    return scene("empty_vote", b, [{"frame": [0, 3, -1]}, {"bad_points": [1]}, {"frame": [900, -1, 901]}])


def bad_voted():
    b = Builder()
    b.kf(0, 30, bad=1, points=[0, 1, 2]); b.kf(1, 20, points=[3]); b.kf(2, 10, points=[4])
    for p in range(3): b.pt(p, obs=[0, 1] if p < 2 else [0])
    b.pt(3, obs=[1]); b.pt(4, obs=[2])
    return scene("bad_voted", b, [{"frame": [0, 1, 2, 4]}])


def tie():
    b = Builder()                                                       # slot order reversed against key order
    b.kf(3, 10, points=[0]); b.kf(2, 20, points=[1]); b.kf(1, 30, points=[2]); b.kf(0, 2 ** 63 + 5, points=[3])
    b.pt(0, obs=[3]); b.pt(1, obs=[2, 1, 0]); b.pt(2, obs=[1, 2, 0]); b.pt(3, obs=[3])
    return scene("tie", b, [{"frame": [0, 1, 2, 3]}])


def parent_break(where, bad_parent=False):
    b = Builder()
    ids = chain_of(b, 5)
    for i in range(5, 9): b.kf(i, 200 + i)
    b.m["keyframes"][8]["bad"] = int(bad_parent)
    if where is not None:
        b.m["keyframes"][where]["parent"] = 8
        b.m["keyframes"][where]["cov"] = [5]; b.m["keyframes"][where]["child"] = [6]
    b.m["keyframes"][4]["cov"] = [7]                                    # reached only when the loop was not left
    b.m["keyframes"][1]["parent"] = 0                                   # a marked parent: no push, no break
    return scene("parent_break_%s%s" % (where, "_bad" if bad_parent else ""), b, [{"frame": ids}])


def neighbours():
    b = Builder()
    ids = chain_of(b, 4)
    for i in range(4, 18): b.kf(i, 300 + i, bad=1 if i < 10 else 0)
    b.m["keyframes"][0]["cov"] = [1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 10]     # ten marked or bad ones, the eleventh is ignored
    b.m["keyframes"][1]["cov"] = [4, 0, 11, 12]                          # bad, marked, then the first free one
    b.m["keyframes"][2]["cov"] = [11, 13]                                # 11 is marked by then
    return scene("neighbours", b, [{"frame": ids}])


def children():
    b = Builder()
    ids = chain_of(b, 3)
    b.kf(3, 50); b.kf(4, 40); b.kf(5, 30, bad=1); b.kf(6, 2 ** 63 + 1); b.kf(7, 45)
    b.m["keyframes"][0]["child"] = [6, 3, 5, 4, 1]                      # by key: 5 (bad), 4, then 3; 1 is marked
    b.m["keyframes"][1]["child"] = [6, 3, 4]                             # 4 is marked by then: 3
    b.m["keyframes"][2]["child"] = [6, 4, 3]                             # only 6 left, the greatest key
    return scene("children", b, [{"frame": ids}])


def limit_80():
    b = Builder()
    ids = chain_of(b, 90, pts_each=2)
    for i in range(90): b.m["keyframes"][i]["cov"] = [90 + i % 5]
    for i in range(90, 95): b.kf(i, 1000 + i)
    b2 = Builder()                                                      # 79 voted: the list passes 80 inside the loop
    ids2 = chain_of(b2, 79)
    for i in range(79): b2.m["keyframes"][i]["cov"] = [79 + i]; b2.m["keyframes"][i]["child"] = [160 + i]
    for i in range(79, 240): b2.kf(i, 1000 + i)
    return [scene("limit_80", b, [{"frame": ids}]), scene("limit_80_inside", b2, [{"frame": ids2}])]


def voted_overflow(n):
    b = Builder()
    for i in range(n): b.kf(i, 7 * ((i * 389) % n) + 1, points=[0] if i % 300 == 0 else [])
    b.pt(0, obs=list(range(n)))
    b.kf(n, 5, points=[1]); b.pt(1, obs=[n])
    # a frame that votes for n keyframes through one MapPoint; before it, one that leaves a one-keyframe list behind
    return scene("voted_%d" % n, b, [{"frame": [1]}, {"frame": [0]}])


def list_overflow():
    out = []
    for extra in (0, 1):
        b = Builder()
        b.kf(0, 1, points=list(range(10)) + [-1] + list(range(5)), lines=[0, 1, 2]); b.kf(1, 2, points=list(range(8, 16 + extra)), lines=[2, 3] + [4] * extra)
        for p in range(16 + extra): b.pt(p, obs=[0] if p < 10 else [1])
        for l in range(4 + extra): b.ln(l)
        out.append(scene("list_full_plus%d" % extra, b, [{"frame": [0, 12]}], max_local_points=16, max_local_lines=4))
    b = Builder()                                                       # lines alone overflow
    b.kf(0, 1, points=[0], lines=[0, 1, 2]); b.pt(0, obs=[0])
    for l in range(3): b.ln(l)
    out.append(scene("lines_over", b, [{"frame": [0]}], max_local_points=16, max_local_lines=2))
    return out


def point_details():
    b = Builder()
    b.kf(0, 10, points=[5, -1, 5, 6, 7, 40], lines=[1, 1, 0]); b.kf(1, 20, points=[6, 5, 8, 9], lines=[0, 2]); b.kf(2, 30, points=[9, 5, 10, 7])
    b.pt(5, obs=[0, 1, 2]); b.pt(6, obs=[0, 1]); b.pt(7, obs=[0, 2], bad=1); b.pt(8, obs=[1]); b.pt(9, obs=[2, 1], bad=1); b.pt(10, obs=[2]); b.pt(11, obs=[])
    b.ln(0); b.ln(1, bad=1); b.ln(2)
    # held: a live point, a bad one (cleared, no vote), an id at max_points, beyond it, a never-set slot, one without observations
    return scene("point_details", b, [{"frame": [5, 9, 64, 1000, 3, 11, -1, 10, 7]}], max_points=64)


# ---------------------------------------------------------------------------------------------------------------- past the kernels' widths
# (lld_map.hip: kChildLds = 32 children of a visited entry in LDS and 64 per trip behind them, rows and prefix sums in tiles of 256, one
# lane per keypoint in blocks of 256, the marks a bit set of (max_keyframes + 31) / 32 words, the extension loop's limit of 80)
CHILD_LDS, WAVE, TILE = 32, 64, 256
CHILD0 = 10                                        # children_long: the children's first slot


def children_winner_positions(n):
    """where children_long(n) puts the winner of its first four voted keyframes: among the LDS-resident ones, at the first position walked
    in HBM, at the row's last position (for n = 97 and 161 a trip of its own), and inside the first HBM trip behind a bad LDS child"""
    return [5, CHILD_LDS, n - 1, 40 if n > 41 else CHILD_LDS]


def children_long(n):
    """Six voted keyframes (slots 0..5, listed in slot order), each with a child row of the same n children in an order of its own; 0 and 1
    share one row.  The children that are neither bad nor marked, by key: 150, 160, 170, 2^63 + 5, then 2^63 + 1000 + j.  The smallest key of
    all (1) belongs to a bad child at position 3 of every row; two voted keyframes (marked from the start, keys 100 and 101) are children too."""
    rng = np.random.default_rng(0xC41D + n)
    b = Builder()
    ids = chain_of(b, 6)
    kids = list(range(CHILD0, CHILD0 + n - 2))
    perm = rng.permutation(len(kids)).tolist()
    bad_small, winners, rest = kids[perm[0]], [kids[j] for j in perm[1:5]], [kids[j] for j in perm[5:]]
    b.kf(bad_small, 1, bad=1)
    for w, k in zip(winners, (150, 160, 170, 2 ** 63 + 5)): b.kf(w, k)
    for j, s in enumerate(rest):
        if j % 4 == 0: b.kf(s, 2 ** 63 + 1000 + j)                        # live, behind every winner
        else: b.kf(s, int(rng.integers(2, 2 ** 64 - 2, dtype=np.uint64)) if j % 4 != 1 else 2 + j, bad=1)
    pos = children_winner_positions(n)

    def row(places):                                                    # {child: position}; the bad smallest key at 3
        places = dict(places); places[bad_small] = 3
        others = [c for c in [0, 1] + kids if c not in places]
        others = [others[j] for j in rng.permutation(len(others))]
        r = [None] * n
        for c, p in places.items(): r[p] = c
        it = iter(others)
        return [c if c is not None else next(it) for c in r]
    shared = row({winners[0]: pos[0], winners[1]: pos[1]})
    rows = [shared, list(shared), row({winners[2]: pos[2]}), row({winners[3]: pos[3]}), row({}), row({})]
    for i in range(6): b.m["keyframes"][i]["child"] = rows[i]
    return scene("children_%d" % n, b, [{"frame": ids}])


def long_row(n, over=False):
    """Keyframe 1 (listed second) has a point row and a line row of n entries: -1 at every 17th, a bad slot at every 19th, a slot never set at
    every 23rd.  Entry 256, the first of the second tile, repeats entry 200 - but for the point row of 257 entries, where it is a slot of
    its own, so that the second tile has something to write behind the first one's; a last entry beyond 256 repeats entry 10.  Keyframe 0
    (listed first) already holds entries 2, 255 and n - 2.  The limits are the lists' lengths; over: one less."""
    b = Builder()
    row, bad, unset = [], set(), set()
    for j in range(n):
        if j % 17 == 3: row.append(-1)
        elif j % 19 == 5: row.append(j); bad.add(j)
        elif j % 23 == 7: row.append(j); unset.add(j)
        else: row.append(j)
    lrow = list(row)
    lrow[TILE] = lrow[200]
    if n - 1 > TILE: row[TILE] = row[200]; row[n - 1] = lrow[n - 1] = row[10]
    first = [row[2], row[TILE - 1], row[n - 2]]
    assert all(s >= 0 and s not in bad and s not in unset for s in first + [row[200], row[10], row[TILE]])
    b.kf(0, 10, points=[n + 1] + first, lines=first[::-1]); b.kf(1, 20, points=row, lines=lrow)
    for s in sorted(set(row + [n + 1, n + 40]) - {-1} - unset):          # n + 40: a set slot beyond every slot never set
        b.pt(s, obs=[k for k in (0, 1) if s in b.m["keyframes"][k]["points"]], bad=s in bad)
        if s != n + 1: b.ln(s, bad=s in bad)
    n_pts = len(set(row + [n + 1]) - {-1} - unset - bad); n_lns = len(set(lrow) - {-1} - unset - bad)
    return scene("row_%d%s" % (n, "_over" if over else ""), b, [{"frame": [n + 1, row[0]]}], max_local_points=n_pts - over, max_local_lines=n_lns - over)


def prefix_600():
    """600 voted, listed keyframes (one MapPoint votes for all of them), key order scrambled against slot order; each has two or three
    points of its own, every fifth one of another keyframe's, every seventh a line of its own, every 21st another one's."""
    n = 600
    b = Builder()
    for i in range(n):
        pts = [3 * i, 3 * i + 1] + ([3 * i + 2] if i % 2 else []) + ([3 * ((i * 7 + 1) % n)] if i % 5 == 0 else [])
        lns = ([i // 7] if i % 7 == 0 else []) + ([(i // 7 + 40) % 86] if i % 21 == 0 else [])
        b.kf(i, 7 * ((i * 389) % n) + 1, points=pts, lines=lns)
        for p in pts[:3 if i % 2 else 2]: b.pt(p, obs=[i])
    for l in range(86): b.ln(l)
    b.pt(3 * n, obs=list(range(n)))
    return scene("prefix_600", b, [{"frame": [3 * n]}], max_local_points=2048, max_local_lines=128)


def voted_n(n):
    """n voted keyframes, each with one unmarked covisible neighbour of its own.  The loop visits an entry while the list holds at most 80:
    with 40 voted it visits every entry and ends at 80, with 80 voted it visits the first entry (81 listed), with 81 none (81 listed)."""
    b = Builder()
    ids = chain_of(b, n)
    for i in range(n): b.m["keyframes"][i]["cov"] = [n + i]
    for i in range(n, 2 * n): b.kf(i, 1000 + i)
    return scene("voted_%d" % n, b, [{"frame": ids}])


FRAME_1000_KP = (255, 256, 257, 511, 512, 999)


def frame_1000():
    """A frame of 1 000 keypoints that holds MapPoints at the last keypoint of the first block of 256 and at keypoints of the three blocks
    behind it only; in the second frame the live and the bad ones have changed places."""
    b = Builder()
    for k in range(6): b.kf(k, 60 - k, points=[k])
    for p, obs in enumerate(([0], [1], [1, 2], [3], [3, 4], [5])): b.pt(p, obs=obs)
    for p in (6, 7, 8): b.pt(p, obs=[0, 5], bad=1)
    steps = []
    for at in (dict(zip(FRAME_1000_KP, (0, 6, 2, 7, 4, 5))), dict(zip(FRAME_1000_KP, (6, 1, 7, 3, 8, 8)))):
        steps.append({"frame": [at.get(k, -1) for k in range(1000)]})
    return scene("frame_1000", b, steps)


def slot_roles(nk):
    """the keyframe slots of slots_scene(nk): the bits 0 and 31 of the first word, bit 0 of the second and the bits of the last word"""
    if nk == 1 << 18:
        return dict(V1=nk - 1, V2=0, V3=32, N=nk - 32, C=31, N2=33, C3=30, P=nk - 31)
    assert nk == 33
    return dict(V1=32, V2=0, V3=1, N=31, C=30, N2=2, C3=3, P=29)


def slots_scene(nk):
    """max_keyframes = nk.  Voted V1, V2, V3 in key order.  V1: cov [V2 (marked), N], children [V3 (marked), C], parent V2 (marked).
    V2: cov [N, C, V1 (all marked by then), N2], children [N, C].  V3: children [C3, V1], parent P: pushed, and the loop is left."""
    r = slot_roles(nk)
    V1, V2, V3, N, C, N2, C3, P = (r[k] for k in ("V1", "V2", "V3", "N", "C", "N2", "C3", "P"))
    b = Builder()
    b.kf(V1, 10, parent=V2, cov=[V2, N], child=[V3, C], points=[5, 1]); b.kf(V2, 20, cov=[N, C, V1, N2], child=[N, C], points=[1, 2], lines=[0])
    b.kf(V3, 30, parent=P, child=[C3, V1], points=[3]); b.kf(N, 40, points=[4]); b.kf(C, 50, points=[2, 0]); b.kf(N2, 60); b.kf(C3, 70, points=[6])
    b.kf(P, 80, points=[7, 5])
    for p, obs in ((5, [V1]), (1, [V1, V2]), (3, [V3]), (0, []), (2, []), (4, []), (6, []), (7, [])): b.pt(p, obs=obs)
    b.ln(0)
    return scene("slots_%d" % nk, b, [{"frame": [5, 1, 3]}], max_keyframes=nk)


def slots_expected(nk):
    """slots_scene(nk)'s answer, written out by hand"""
    r = slot_roles(nk)
    return dict(local_keyframes=[r[k] for k in ("V1", "V2", "V3", "N", "C", "N2", "C3", "P")], local_points=[5, 1, 2, 3, 4, 0, 6, 7], local_lines=[0],
                ref_keyframe=r["V1"], n_voted=3, n_bad_cleared=0, status=0, vote_empty=0)


def width_scenes():
    return [children_long(n) for n in (33, 96, 97, 161)] + [long_row(257), long_row(513), long_row(257, over=True), prefix_600(), voted_n(40), voted_n(80), voted_n(81),
                                                            slots_scene(33)]


def all_scenes():
    """every scene a frame of 256 keypoints can hold and whose dense text file is small"""
    s = [random_map(i) for i in range(10)]
    s += [empty_vote(), bad_voted(), tie(), parent_break(0), parent_break(2), parent_break(None), parent_break(2, bad_parent=True), neighbours(), children()]
    s += limit_80() + [voted_overflow(1024), voted_overflow(1025)] + list_overflow() + [point_details()]
    return s + width_scenes()


# ---------------------------------------------------------------------------------------------------------------- a scene as a text file
def write_text(path, sc):
    """The scene as examples/local_map_host_check.cpp reads it: dense tables over every slot inside the limits."""
    m, L = sc["map"], sc["limits"]
    out = [L["max_keyframes"], L["max_points"], L["max_lines"], L["max_local_points"], L["max_local_lines"]]
    lst = lambda v: [len(v)] + [int(x) for x in v]
    for s in range(L["max_keyframes"]):
        k = m["keyframes"].get(s)
        out += [0, 1, -1, 0, 0, 0, 0] if k is None else [k["key"], k["bad"], -1 if k["parent"] is None else k["parent"]] + lst(k["cov"]) + lst(k["child"]) + lst(k["points"]) + lst(k["lines"])
    for s in range(L["max_points"]):
        p = m["points"].get(s)
        out += [0, 0] if p is None else [2 if p["bad"] else 1] + lst(p["obs"])
    for s in range(L["max_lines"]):
        l = m["lines"].get(s)
        out.append(1 if l is None else l["bad"])
    out.append(len(sc["steps"]))
    for step in sc["steps"]:
        out += [0] + lst(step["frame"]) if "frame" in step else [1] + lst(step["bad_points"])
    with open(path, "w") as f:
        f.write(" ".join(str(int(x)) for x in out) + "\n")


# ---------------------------------------------------------------------------------------------------------------- maps over a tracking scene
# (synth.make_tracking_scene: the chain tests, examples/local_map_harness.cpp and tools/time_local_map.py share them)
N_KF = 8
LINE_ID0 = 1000                                    # synth.make_tracking_lines numbers its MapLines from here; slot = id - 1000


def as_slots(sc):
    sc = dict(sc)
    for k in ("last_lines", "local_lines"):
        if sc.get(k) is not None:
            sc[k] = dict(sc[k], id=np.asarray(sc[k]["id"], np.int32) - LINE_ID0)
    return sc


def make_map(sc, held, seed, n_kf=N_KF):
    """A map over the scene's MapPoints / MapLines: N_KF keyframes in shuffled slots, every point with observations observed by one to three
    of them, some points and lines bad (none the frame holds: the host route cannot take a MapPoint out of the device frame)."""
    rng = np.random.default_rng(77 + seed)
    mp = sc["map_points"]; n = len(mp["has_obs"]); ll = sc.get("local_lines"); n_ln = 0 if ll is None else len(ll["id"])
    b = Builder()
    slots = rng.permutation(n_kf + 2)[:n_kf].tolist()
    rows = {s: [] for s in slots}; lrows = {s: [] for s in slots}
    free = np.setdiff1d(np.arange(n), np.asarray(held)[np.asarray(held) >= 0])
    bad = set(rng.choice(free, max(1, len(free) // 12), replace=False).tolist())
    for p in range(n):
        obs = rng.choice(slots, int(rng.integers(1, 4)), replace=False).tolist() if mp["has_obs"][p] else []
        for s in (obs or [slots[p % n_kf]]):
            rows[s].append(p)
            if rng.random() < 0.2: rows[s].append(-1)
            if rng.random() < 0.05: rows[s].append(p)
        b.pt(p, obs=obs, bad=p in bad)
    for l in range(n_ln):
        for s in rng.choice(slots, int(rng.integers(1, 3)), replace=False).tolist():
            lrows[s].append(l)
        b.ln(l, bad=rng.random() < 0.08)
    keys = rng.integers(1, 2 ** 63, n_kf).tolist()
    for i, s in enumerate(slots):
        others = [o for o in slots if o != s]
        b.kf(s, keys[i], parent=None if i == 0 else slots[int(rng.integers(0, i))], cov=rng.permutation(others)[:3].tolist(), child=[],
             points=rng.permutation(rows[s]).tolist(), lines=rng.permutation(lrows[s]).tolist())
    for s in slots:
        p = b.m["keyframes"][s]["parent"]
        if p is not None: b.m["keyframes"][p]["child"].append(s)
    return b.m


def point_data(sc):
    mp = sc["map_points"]
    return {p: {k: mp[k][p] for k in ("world_pos", "normal", "min_distance", "max_distance", "desc")} for p in range(len(mp["has_obs"]))}


def line_data(sc):
    ll = sc["local_lines"]
    return {int(s): {k: ll[k][i] for k in ("X0", "dir", "X1", "X2", "desc")} for i, s in enumerate(ll["id"])}


def tracking_limits(sc, m, n_kf=N_KF, max_local_points=512, max_local_lines=64):
    return limits_for(m, max_local_points=max_local_points, max_local_lines=max_local_lines, max_keyframes=n_kf + 4, line_dim=sc["lines"]["desc"].shape[1],
                         max_observations=4 * len(m["points"]), max_kf_points=8 * len(m["points"]), max_kf_lines=4 * max(len(m["lines"]), 1), max_children=64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def same_dict(g, e, what, skip=()):
    assert set(g) == set(e), what
    for k in g:
        if k in skip: continue
        if isinstance(g[k], np.ndarray):
            np.testing.assert_array_equal(bits(g[k]), bits(e[k]), err_msg="%s: %s" % (what, k))
        elif isinstance(g[k], float):
            assert np.float64(g[k]).view(np.uint64) == np.float64(e[k]).view(np.uint64), (what, k, g[k], e[k])
        else:
            assert g[k] == e[k], (what, k, g[k], e[k])


def csr(rows):
    start = np.zeros(len(rows) + 1, np.int32)
    for i, r in enumerate(rows): start[i + 1] = start[i] + len(r)
    return start, np.array([v for r in rows for v in r], np.int32).reshape(-1)


def flat_tables(m, L):
    """The map as dense flat tables over every slot inside the limits (what examples/local_map_host.h reads): dict of arrays."""
    nk, npt, nl = L["max_keyframes"], L["max_points"], L["max_lines"]
    kf = lambda s, k, d: m["keyframes"][s][k] if s in m["keyframes"] else d
    T = dict(kf_key=np.array([kf(s, "key", 0) for s in range(nk)], np.uint64), kf_bad=np.array([kf(s, "bad", 1) for s in range(nk)], np.uint8),
             kf_parent=np.array([-1 if kf(s, "parent", None) is None else kf(s, "parent", None) for s in range(nk)], np.int32),
             pt_state=np.array([0 if s not in m["points"] else 2 if m["points"][s]["bad"] else 1 for s in range(npt)], np.uint8),
             ln_bad=np.array([1 if s not in m["lines"] else m["lines"][s]["bad"] for s in range(nl)], np.uint8))
    for name, key in (("cov", "cov"), ("child", "child"), ("point", "points"), ("line", "lines")):
        T[name + "_start"], T[name] = csr([kf(s, key, []) for s in range(nk)])
    T["obs_start"], T["obs"] = csr([m["points"][s]["obs"] if s in m["points"] else [] for s in range(npt)])
    return {k: np.ascontiguousarray(v) for k, v in T.items()}


def write_map_file(path, sc, m, L):
    """The map with its payload as examples/local_map_harness.cpp reads it: int32 header (the ten limits in lld_map_limits order), then the flat
    tables in the order below, then the points' and lines' data by dense slot."""
    T = flat_tables(m, L)
    pd, ld = point_data(sc), line_data(sc)
    npt, nl, dim = L["max_points"], L["max_lines"], L["line_dim"]
    col = lambda d, n, k, shape, dt: np.ascontiguousarray(np.array([d[s][k] if s in d else np.zeros(shape, dt) for s in range(n)], dt).reshape((n,) + shape))
    with open(path, "wb") as f:
        np.array([L[k] for k in ("max_keyframes", "max_points", "max_lines", "line_dim", "max_observations", "max_kf_points", "max_kf_lines", "max_children",
                                 "max_local_points", "max_local_lines")], np.int32).tofile(f)
        for k in ("kf_key", "kf_bad", "kf_parent", "cov_start", "cov", "child_start", "child", "point_start", "point", "line_start", "line", "pt_state",
                  "obs_start", "obs", "ln_bad"):
            T[k].tofile(f)
        for k, shape, dt in (("world_pos", (3,), np.float32), ("normal", (3,), np.float32), ("min_distance", (), np.float32), ("max_distance", (), np.float32),
                             ("desc", (8,), np.uint32)):
            col(pd, npt, k, shape, dt).tofile(f)
        for k, shape, dt in (("X0", (3,), np.float64), ("dir", (3,), np.float64), ("X1", (3,), np.float64), ("X2", (3,), np.float64), ("desc", (dim,), np.float32)):
            col(ld, nl, k, shape, dt).tofile(f)

