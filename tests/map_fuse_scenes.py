"""Maps for the tests of lld_map_fuse (tests/map_fuse_ref.py holds the rules): a target keyframe whose keypoints are the projections of 3D
points, candidates aimed at those keypoints (so that the search finds them), holders of every kind, observation rows of chosen lengths in
other keyframes - as the map model of tests/map_ba_scenes.py / map_refresh_scenes.py, with their upload.  numpy only (view_struct asks the
package for the ctypes mirror of lld_frame_view).

The camera is (fx, fy, cx, cy, bf) = (500, 500, 320, 240, 40) on a 640 x 480 image with the 64 x 48 grid, eight levels of factor 1.2.  A
point aimed at keypoint k of octave o lies within a pixel of it, has mfMaxDistance = dist * scale[o] / sqrt(1.2) (PredictScale gives o),
the normal towards the camera and the keypoint's descriptor with a few bits flipped."""
import numpy as np

import map_fuse_ref as F
import map_refresh_scenes as RS

f32 = np.float32
CAM = (500.0, 500.0, 320.0, 240.0, 40.0)
WIDTH, HEIGHT = 640.0, 480.0
GRID = (0.0, 0.0, f32(64) / f32(WIDTH), f32(48) / f32(HEIGHT), 64, 48)
N_LEVELS = 8


def levels(factor=1.2, n=N_LEVELS):
    s = np.ones(n, f32)
    for i in range(1, n):
        s[i] = f32(s[i - 1] * f32(factor))
    sig = (s * s).astype(f32)
    return s, (f32(1.0) / sig).astype(f32)


SCALE, INV_SIGMA2 = levels()


def view_of(Tcw):
    T = np.asarray(Tcw, f32).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(f32)
    return dict(Rcw=R.reshape(9).copy(), tcw=t.copy(), Ow=Ow, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], bf=CAM[4], min_x=0.0, max_x=WIDTH, min_y=0.0, max_y=HEIGHT,
                log_scale_factor=float(np.log(f32(1.2))), n_levels=N_LEVELS)


def view_struct(view):
    from lld_slam_amd import orb_search
    v = orb_search.FrameView()
    for i in range(9): v.Rcw[i] = float(view["Rcw"][i])
    for i in range(3): v.tcw[i] = float(view["tcw"][i]); v.Ow[i] = float(view["Ow"][i])
    for k in ("fx", "fy", "cx", "cy", "bf", "min_x", "max_x", "min_y", "max_y", "log_scale_factor"):
        setattr(v, k, float(f32(view[k])))
    v.n_levels = int(view["n_levels"])
    return v


def small_pose(rng):
    a = rng.normal(size=3) * 0.05
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    T = np.eye(4, dtype=f32); T[:3, :3] = Rx @ Ry @ Rz; T[:3, 3] = rng.normal(size=3) * 0.5
    return T


class Builder:
    """Keyframe slot `target` is pKF; the other keyframes only lend observations.  Keys are a shuffle of the slots, so key order is not slot order."""

    def __init__(self, seed, n_other=8, target=None, bad_others=(), objects=False):
        self.rng = rng = np.random.default_rng(0xF05E + seed)
        n = n_other + 1
        self.target = int(rng.integers(0, n)) if target is None else target
        keys = (rng.permutation(n) + 1) * 7
        self.objects = objects                          # for an object graph: keys in slot order (pointer order), observations where the point projects
        if objects:
            keys = (np.arange(n) + 1) * 7
        self.T = small_pose(rng)
        self.view = view_of(self.T)
        self.K = {s: dict(key=int(keys[s]), bad=int(s in bad_others and s != self.target), points=[], uvr=[], octave=[], desc=[], Tcw=self.T if s == self.target else small_pose(rng), mn_id=s + 1)
                  for s in range(n)}
        self.others = [s for s in range(n) if s != self.target]
        self.P = {}
        self.aim = {}                                   # target keypoint -> (camera point, octave, descriptor)
        self.next_slot = 0

    def rand_desc(self):
        return self.rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)

    def keypoint(self, octave=None, mono=None, uv=None, depth=None, desc=None):
        """a keypoint of the target: the projection of a 3D point in front of it; returns its index"""
        rng = self.rng
        u, v = (rng.uniform(24, WIDTH - 24), rng.uniform(24, HEIGHT - 24)) if uv is None else uv
        z = rng.uniform(5, 15) if depth is None else depth
        o = int(rng.integers(0, N_LEVELS)) if octave is None else octave
        mono = rng.random() < 0.25 if mono is None else mono
        d = self.rand_desc() if desc is None else np.asarray(desc, np.uint32)
        k = self.K[self.target]
        k["points"].append(-1); k["uvr"].append((f32(u), f32(v), f32(-1) if mono else f32(u - CAM[4] / z))); k["octave"].append(o); k["desc"].append(d)
        i = len(k["points"]) - 1
        self.aim[i] = (np.array([(u - CAM[2]) * z / CAM[0], (v - CAM[3]) * z / CAM[1], z]), o, d)
        return i

    def slot(self):
        self.next_slot += 1
        return self.next_slot - 1

    def point(self, aim=None, observers=1, bad=0, slot=None, flips=6, offset=None, octave=None, obs_mono=None):
        """a map point aimed at target keypoint `aim` (None: somewhere behind the camera), observed by `observers` (a count of other keyframes
        or their slots): a new keypoint of each of them"""
        rng = self.rng
        s = self.slot() if slot is None else slot
        R, t = self.T[:3, :3].astype(np.float64), self.T[:3, 3].astype(np.float64)
        if aim is None:
            Xc, o, base = np.array([rng.normal(), rng.normal(), -rng.uniform(2, 9)]), int(rng.integers(0, N_LEVELS)), self.rand_desc()
        else:
            Xc, o, base = self.aim[aim]
            o = o if octave is None else octave
            dxy = rng.uniform(-0.7, 0.7, 2) if offset is None else np.asarray(offset, float)
            Xc = Xc + np.array([dxy[0] * Xc[2] / CAM[0], dxy[1] * Xc[2] / CAM[1], 0.0])       # dxy pixels beside the keypoint, same depth
        pos = (R.T @ (Xc - t)).astype(f32)
        PO = pos.astype(np.float64) - self.view["Ow"].astype(np.float64)
        dist = np.linalg.norm(PO)
        maxd = f32(dist * float(SCALE[o]) / np.sqrt(1.2))
        p = dict(bad=int(bad), pos=pos, nrm=(PO / dist).astype(f32), maxd=maxd, mind=f32(maxd / SCALE[-1]), desc=RS.flipped(rng, base, flips), obs=[], indexed=True, base=base)
        self.P[s] = p
        kfs = list(rng.permutation(self.others)[:observers]) if isinstance(observers, (int, np.integer)) else list(observers)
        for kf in kfs:
            self.observe(s, int(kf), obs_mono)
        return s

    def observe(self, s, kf, mono=None):
        """point s becomes a new keypoint of keyframe kf"""
        rng = self.rng
        k = self.K[kf]
        u, v = rng.uniform(0, WIDTH), rng.uniform(0, HEIGHT)
        mono = rng.random() < 0.25 if mono is None else mono
        ur, octave = u - 3, int(rng.integers(0, N_LEVELS))
        proj = F.project(view_of(k["Tcw"]), self.P[s]) if self.objects else None
        if proj is not None:                           # the keypoint is the point's own projection into this keyframe, at the predicted level
            u, v, ur, octave = proj
        k["points"].append(s); k["uvr"].append((f32(u), f32(v), f32(-1) if mono else f32(ur))); k["octave"].append(int(octave))
        k["desc"].append(RS.flipped(rng, self.P[s]["base"], 6))
        self.P[s]["obs"].append((kf, len(k["points"]) - 1))

    def hold(self, i, s):
        """target keypoint i holds point s"""
        self.K[self.target]["points"][i] = s
        self.P[s]["obs"].append((self.target, i))

    def finish(self):
        K, P = self.K, self.P
        z = lambda w, dt=f32: np.zeros((0, w), dt)
        for k in K.values():
            n = len(k["points"])
            k["uvr"] = np.array(k["uvr"], f32).reshape(n, 3); k["desc"] = np.array(k["desc"], np.uint32).reshape(n, 8); k["lines"] = []
            k["kl_left"] = z(4); k["kl_right"] = z(4); k["kl_octave"] = z(2, np.int32)
        m = dict(keyframes=K, points=P, lines={})
        for p in P.values():
            p.pop("base")
            p["obs"].sort(key=lambda o: K[o[0]]["key"])                      # std::map<KeyFrame*, size_t> order
            p["n_obs"] = sum(2 if F.stereo(m, kf, idx) else 1 for kf, idx in p["obs"])
            p["ref_kf"] = p["obs"][0][0] if p["obs"] else -1
        return m


def call_of(b):
    """the arguments every route takes beside the map and the candidates"""
    return dict(target=b.target, view=b.view, grid=GRID, level_scale=SCALE, inv_sigma2=INV_SIGMA2)


def run_ref(m, c, slots, th=3.0, source_keyframe=-1):
    return F.fuse(m, c["target"], slots, c["view"], c["grid"], c["level_scale"], c["inv_sigma2"], th, source_keyframe)


HOLDERS = ("none", "more", "fewer", "equal", "bad", "never")


def add_holder(b, i, kind):
    """target keypoint i gets a holder of `kind`; the counts are against a candidate with two observers (n_obs 2 .. 4)"""
    if kind == "none":
        return -1
    if kind == "never":
        s = b.slot()                                                         # a slot no point is ever set in
        b.K[b.target]["points"][i] = s
        return s
    s = b.point(aim=i, observers=dict(more=6, fewer=0, equal=2, bad=2)[kind], bad=int(kind == "bad"))
    b.hold(i, s)
    if kind == "bad":
        b.P[s]["obs"] = []                                                   # SetBadFlag emptied the row; the keyframes' entries are what Replace left
    return s


def random_scene(seed, n_target=65, n_cand=65, n_other=8, check=True, objects=False):
    """(map, call arguments, candidate slots).  With check: the restatement alone fuses at least a quarter of the candidates and takes every
    action at least once - asserted here, on the CPU."""
    b = Builder(seed, n_other, bad_others=(1,) if n_other > 3 else (), objects=objects)
    rng = b.rng
    for i in range(n_target):
        b.keypoint()
    kinds = rng.choice(len(HOLDERS), n_target, p=[0.5, 0.15, 0.15, 0.1, 0.1, 0.0] if objects else [0.4, 0.15, 0.15, 0.1, 0.1, 0.1])   # (an object is never "never set")
    for i in range(n_target):
        add_holder(b, i, HOLDERS[kinds[i]])
    slots = []
    unset = b.slot()
    for c in range(n_cand):
        u = rng.random()
        if n_cand >= 8:                                                      # one of every special kind, whatever the draw
            u = {2: 0.70, 3: 0.74, 4: 0.78, 5: 0.85, 6: 0.90, 7: 0.95}.get(c, u)
        if u < 0.66 or not slots:
            slots.append(b.point(aim=int(rng.integers(0, n_target)), observers=int(rng.integers(1, min(5, n_other + 1)))))
        elif u < 0.72: slots.append(-1)
        elif u < 0.76: slots.append(-1 if objects else unset)
        elif u < 0.81: slots.append(b.point(aim=int(rng.integers(0, n_target)), observers=2, bad=1))
        elif u < 0.88: slots.append(slots[int(rng.integers(0, len(slots)))])             # a slot named twice
        elif u < 0.93: slots.append(b.point(aim=None, observers=2))                        # behind the camera
        else:
            held = [s for s in b.K[b.target]["points"] if s >= 0 and s in b.P]
            slots.append(held[int(rng.integers(0, len(held)))] if held else -1)           # already in the target
    m = b.finish()
    c = call_of(b)
    if check:
        _, out = run_ref(m, c, slots)
        assert out["n_fused"] * 4 >= n_cand, (seed, out["n_fused"], n_cand)
        assert set(out["action"].tolist()) >= {1, 2, 3, 4, 5}, (seed, sorted(set(out["action"].tolist())))
        assert len(out["survivor"]) > 0
    return m, c, slots


def rows_scene(rows=(1, 17, 65), seed=0):
    """For every L of rows, two target keypoints: at the first the candidate (a row of L entries) loses to a holder with more observations and
    its row moves; at the second the holder (a row of L entries, the target among them) loses to the candidate.  Returns (m, c, slots, what):
    what[i] = (L, expected action) per candidate."""
    L_max = max(rows)
    b = Builder(seed, n_other=2 * L_max + 4, target=0)
    slots, what = [], []
    for L in rows:
        i = b.keypoint(mono=True)
        h = b.point(aim=i, observers=b.others[L_max:2 * L_max + 2], obs_mono=True); b.hold(i, h)
        slots.append(b.point(aim=i, observers=b.others[:L], obs_mono=True)); what.append((L, F.CANDIDATE_REPLACED))
        i = b.keypoint(mono=True)
        h = b.point(aim=i, observers=b.others[:L - 1], obs_mono=True); b.hold(i, h)
        slots.append(b.point(aim=i, observers=b.others[L_max // 2:L_max // 2 + L + 1], obs_mono=True)); what.append((L, F.HOLDER_REPLACED))
    return b.finish(), call_of(b), slots, what


def limit_scene(beyond, seed=0):
    """One candidate with 1000 observers replaces a holder whose row (the target and 23 or, with `beyond`, 24 other keyframes the candidate
    does not have) joins its own: a survivor row of exactly LLD_LANDMARK_MAX_OBS entries, or one more."""
    b = Builder(seed, n_other=1030, target=0)
    i = b.keypoint(mono=True)
    h = b.point(aim=i, observers=b.others[1000:1000 + (24 if beyond else 23)], obs_mono=True); b.hold(i, h)
    s = b.point(aim=i, observers=b.others[:1000], obs_mono=True)
    return b.finish(), call_of(b), [s]


# ---------------------------------------------------------------------------------------------------------------- the paper scenes
# Small enough to be worked out by hand.  The target is keyframe 0 with key 10, keyframe s has key 10 (s + 1): a row in key order is a row in
# slot order and the target's entry goes first.  Unless said otherwise every keypoint and every observation is monocular, so Observations()
# is the length of the row.  Point slots are handed out in the order the points are made (written at each scene).  Each scene returns
# (m, call arguments, candidate slots, expectation): match, action, other, survivor, n_obs {slot: Observations()}, bad [slots],
# obs {slot: [(keyframe, index)]} and points {keyframe: row} for what the call touches.
def paper(n_other=4):
    b = Builder(0, n_other, target=0)
    for s, k in b.K.items():
        k["key"] = 10 * (s + 1)
    return b


def done(b, slots, **expect):
    return b.finish(), call_of(b), slots, expect


def add_stereo_and_mono():
    """Keypoint 0 is stereo, keypoint 1 mono, both free.  A (slot 0, seen by keyframe 1 at its keypoint 0) lands on keypoint 0: its row gains
    (0, 0) in front (key 10 < 20) and Observations() 1 + 2; B (slot 1, keyframe 1 keypoint 1) lands on keypoint 1: 1 + 1."""
    b = paper()
    b.keypoint(mono=False, uv=(100, 100)); b.keypoint(mono=True, uv=(400, 300))
    A = b.point(aim=0, observers=[1], obs_mono=True); B = b.point(aim=1, observers=[1], obs_mono=True)
    return done(b, [A, B], match=[0, 1], action=[1, 1], other=[-1, -1], survivor=[], n_obs={A: 3, B: 2}, bad=[], obs={A: [(0, 0), (1, 0)], B: [(0, 1), (1, 1)]},
                points={0: [A, B], 1: [A, B]})


def replace_each_way():
    """Keypoint 0: holder H0 (slot 0; keyframes 1, 2, 3 and the target: 4) against C0 (slot 1; keyframe 4: 1): C0 is replaced, keyframe 4's entry
    becomes H0, H0 has 5.  Keypoint 1: H1 (slot 2; the target alone: 1) against C1 (slot 3; keyframes 1, 2: 2): H1 is replaced, C1 gains the
    target: 3.  Keypoint 2: H2 (slot 4; keyframe 1 and the target: 2) against C2 (slot 5; keyframes 2, 3: 2): a tie replaces the holder, C2 gains
    the target and keyframe 1: 4.  Keyframe 1's row is [H0, C1, H2] -> [H0, C1, C2]."""
    b = paper()
    for uv in ((100, 100), (300, 200), (500, 400)): b.keypoint(mono=True, uv=uv)
    H0 = b.point(aim=0, observers=[1, 2, 3], obs_mono=True); b.hold(0, H0); C0 = b.point(aim=0, observers=[4], obs_mono=True)
    H1 = b.point(aim=1, observers=[], obs_mono=True); b.hold(1, H1); C1 = b.point(aim=1, observers=[1, 2], obs_mono=True)
    H2 = b.point(aim=2, observers=[1], obs_mono=True); b.hold(2, H2); C2 = b.point(aim=2, observers=[2, 3], obs_mono=True)
    return done(b, [C0, C1, C2], match=[0, 1, 2], action=[2, 3, 3], other=[H0, H1, H2], survivor=[H0, C1, C2], n_obs={H0: 5, C0: 1, H1: 1, C1: 3, H2: 2, C2: 4},
                bad=[C0, H1, H2], obs={H0: [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)], C0: [], H1: [], C1: [(0, 1), (1, 1), (2, 1)], H2: [], C2: [(0, 2), (1, 2), (2, 2), (3, 1)]},
                points={0: [H0, C1, C2], 1: [H0, C1, C2], 4: [H0]})


def survivor_already_there():
    """H (slot 0; keyframes 1, 2 and the target: 3) against C (slot 1; keyframe 2 at its keypoint 1: 1): C is replaced; H is in keyframe 2 already,
    so C's entry there is cleared and nothing is added."""
    b = paper()
    b.keypoint(mono=True, uv=(200, 200))
    H = b.point(aim=0, observers=[1, 2], obs_mono=True); b.hold(0, H); C = b.point(aim=0, observers=[2], obs_mono=True)
    return done(b, [C], match=[0], action=[2], other=[H], survivor=[H], n_obs={H: 3, C: 1}, bad=[C], obs={H: [(0, 0), (1, 0), (2, 0)], C: []}, points={0: [H], 2: [H, -1]})


def same_keypoint_twice():
    """Two candidates on the free keypoint 0.  A (slot 0; keyframe 1: 1) is added: 2.  B (slot 1; keyframes 2, 3: 2) then meets A as the holder:
    2 > 2 is false, A is replaced, B gains the target and keyframe 1: 4."""
    b = paper()
    b.keypoint(mono=True, uv=(200, 200))
    A = b.point(aim=0, observers=[1], obs_mono=True); B = b.point(aim=0, observers=[2, 3], obs_mono=True)
    return done(b, [A, B], match=[0, 0], action=[1, 3], other=[-1, A], survivor=[B], n_obs={A: 2, B: 4}, bad=[A], obs={A: [], B: [(0, 0), (1, 0), (2, 0), (3, 0)]},
                points={0: [B], 1: [B]})


def attached_meanwhile():
    """C (slot 1; keyframes 1, 2: 2) is named twice.  The first time it replaces H (slot 0; the target alone: 1) and so sits in the target; the
    second time the search's match still stands, and the re-test skips it."""
    b = paper()
    b.keypoint(mono=True, uv=(200, 200))
    H = b.point(aim=0, observers=[], obs_mono=True); b.hold(0, H); C = b.point(aim=0, observers=[1, 2], obs_mono=True)
    return done(b, [C, C], match=[0, 0], action=[3, 5], other=[H, -1], survivor=[C], n_obs={H: 1, C: 3}, bad=[H], obs={H: [], C: [(0, 0), (1, 0), (2, 0)]}, points={0: [C]})


def bad_holder():
    """The holder (slot 0; it left its entries in keyframes 1 and 2 and the target behind) is bad: counted as fused, nothing done."""
    b = paper()
    b.keypoint(mono=True, uv=(200, 200))
    H = b.point(aim=0, observers=[1, 2], bad=1, obs_mono=True); b.hold(0, H); b.P[H]["obs"] = []
    C = b.point(aim=0, observers=[1], obs_mono=True)
    return done(b, [C], match=[0], action=[4], other=[H], survivor=[], n_obs={C: 1}, bad=[H], obs={C: [(1, 1)], H: []}, points={0: [H], 1: [H, C]})


def tie_between_cells():
    """Keypoints 0 at u = 306 (column 31) and 1 at u = 294 (column 29), same row, octave 6, the same descriptor; the candidate projects to
    u = 300 with r = 3 * 1.2^6 = 8.96 and is 6 pixels from both (chi2 36 / 8.92 = 4.04).  Equal distances: column 29 is visited first, so
    keypoint 1 wins although keypoint 0 has the lower index."""
    b = paper()
    d = b.rand_desc()
    b.keypoint(octave=6, mono=True, uv=(306, 200), depth=8.0, desc=d); b.keypoint(octave=6, mono=True, uv=(294, 200), depth=8.0, desc=d)
    C = b.point(aim=0, observers=[1], obs_mono=True, offset=(-6, 0), flips=0)
    return done(b, [C], match=[1], action=[1], other=[-1], survivor=[], n_obs={C: 2}, bad=[], obs={C: [(0, 1), (1, 0)]}, points={0: [-1, C]})


PAPER = dict(add_stereo_and_mono=add_stereo_and_mono, replace_each_way=replace_each_way, survivor_already_there=survivor_already_there,
             same_keypoint_twice=same_keypoint_twice, attached_meanwhile=attached_meanwhile, bad_holder=bad_holder, tie_between_cells=tie_between_cells)


def limits(m, spare_points=0, **over):
    L = RS.limits(m)
    L["max_points"] = max(L["max_points"], max([s for k in m["keyframes"].values() for s in k["points"]] + [0]) + 2) + spare_points
    L["max_observations"] += 3 * len(m["points"]) + 64                      # room for what a fuse adds
    L.update(over)
    return L
