"""Maps and crafted results for the tests of lld_map_ba_apply (tests/map_ba_apply_ref.py holds the rules): what tests/map_ba_scenes.py
builds, completed with the fields the apply reads (n_obs, normal, distances, mpRefKF), their upload, random results, and hand-made scenes
whose outcome is written out in tests/test_map_ba_apply_ref.py.  numpy only."""
import numpy as np

import map_ba_scenes as S

LEVEL_SCALE = np.array([1.0, 1.2, 1.44, 1.728], np.float32)
f32 = np.float32


def stereo_weight(m, kf, idx):
    k = m["keyframes"].get(kf)
    return 2 if k is not None and "uvr" in k and idx < len(k["uvr"]) and k["uvr"][idx][2] >= 0 else 1


def complete(m, seed=0, refs=True):
    """n_obs as AddObservation counts it (2 for a keypoint with a right coordinate), a normal and distances to be overwritten, and mpRefKF:
    mostly an observer, now and then a keyframe that does not observe the point, now and then -1."""
    rng = np.random.default_rng(0xA991 + seed)
    kfs = sorted(m["keyframes"])
    for p in m["points"].values():
        p["n_obs"] = sum(stereo_weight(m, kf, idx) for kf, idx in p["obs"]) if p.get("indexed", True) else len(p["obs"])
        p["nrm"] = rng.normal(size=3).astype(f32); p["mind"] = f32(rng.random()); p["maxd"] = f32(1 + rng.random())
        if refs:
            u = rng.random()
            p["ref_kf"] = int(p["obs"][int(rng.integers(len(p["obs"])))][0]) if p["obs"] and u < 0.85 else int(kfs[int(rng.integers(len(kfs)))]) if u < 0.95 else -1
    return m


def upload(dm, m):
    S.upload_keyframes(dm, m)
    slots = sorted(m["points"])
    if slots:
        P = [m["points"][s] for s in slots]
        n = len(slots)
        dm.set_points(slots, np.array([p["pos"] for p in P], f32), np.array([p.get("nrm", np.zeros(3)) for p in P], f32), np.array([p.get("mind", 0) for p in P], f32),
                      np.array([p.get("maxd", 0) for p in P], f32), np.zeros((n, 8), np.uint32), [p["bad"] for p in P])
        dm.set_observations_indexed(slots, rows=[p["obs"] for p in P], n_obs=[int(p.get("n_obs", len(p["obs"]))) for p in P])
        if any("ref_kf" in p for p in P):
            dm.set_point_refs(slots, [p.get("ref_kf", -1) for p in P])
    S.upload_lines(dm, m)


def all_slots(dm):
    return dict(kf=list(range(dm.limits.max_keyframes)), pt=list(range(dm.limits.max_points)), ln=list(range(dm.limits.max_lines)))


POOLS = (("point_obs", "pt"), ("point_idx", "pt"), ("kf_points", "kf"), ("kf_lines", "kf"), ("line_obs", "ln"), ("line_idx", "ln"))


class Result(dict):
    """the arrays of lld_ba_result"""
    __getattr__ = dict.__getitem__


def crafted(win, seed, frac=0.15, removed=0.1, se3_from_tcw=None):
    """A result for window `win`: new poses, positions and lines, `frac` of the point observations and line edges flagged, `removed` of the
    lines removed."""
    rng = np.random.default_rng(0xC4AF + seed)
    nc, npt, npo, nl, nlo = (int(win[k]) for k in ("n_cams", "n_points", "n_pt_obs", "n_lines", "n_ln_obs"))
    cam_qt = np.array(win["cam_qt"], np.float64).reshape(-1, 7).copy()
    if se3_from_tcw is not None:
        for c in range(nc):
            cam_qt[c] = se3_from_tcw(S.random_pose(rng))
    return Result(cam_qt=cam_qt, pt_xyz=rng.normal(size=(npt, 3)) * 4, line_x0=rng.normal(size=(nl, 3)), line_dir=rng.normal(size=(nl, 3)),
                  pt_obs_outlier=(rng.random(npo) < frac).astype(np.uint8), ln_edge_outlier=(rng.random((nlo, 2)) < frac).astype(np.uint8),
                  line_removed=(rng.random(nl) < removed).astype(np.uint8))


def flags_for(win, point_kfs=(), line_kfs=(), both=(), removed=()):
    """A result that keeps the window's poses and positions and flags the named observations: point_kfs [(point slot, keyframe slot)], line_kfs
    [(line slot, keyframe slot)] (first edge flag; in `both`: both flags), removed [line slot]."""
    cam = [int(s) for s in win["cam_slot"]]
    po = np.zeros(int(win["n_pt_obs"]), np.uint8); lo = np.zeros((int(win["n_ln_obs"]), 2), np.uint8); rm = np.zeros(int(win["n_lines"]), np.uint8)
    for q, s in enumerate(int(v) for v in win["point_slot"]):
        for e in range(win["pt_obs_start"][q], win["pt_obs_start"][q + 1]):
            if (s, cam[win["pt_obs_cam"][e]]) in set(point_kfs): po[e] = 1
    for l, s in enumerate(int(v) for v in win["line_slot"]):
        rm[l] = s in set(removed)
        for e in range(win["ln_obs_start"][l], win["ln_obs_start"][l + 1]):
            if (s, cam[win["ln_obs_cam"][e]]) in set(line_kfs): lo[e, 0] = 1
            if (s, cam[win["ln_obs_cam"][e]]) in set(both): lo[e] = 1
    return Result(cam_qt=np.array(win["cam_qt"], np.float64), pt_xyz=np.array(win["pt_xyz"], np.float64), line_x0=np.array(win["line_x0"], np.float64),
                  line_dir=np.array(win["line_dir"], np.float64), pt_obs_outlier=po, ln_edge_outlier=lo, line_removed=rm)


def covis_tables(m):
    """the map as tests/map_covis_ref.py reads it (upload_keyframes sends depth 0 and th_depth 0 for every keypoint)"""
    kf = {s: dict(key=k["key"], points=list(k["points"]), octave=k.get("octave"), depth=None if k.get("octave") is None else [0.0] * len(k["octave"]), th_depth=0.0)
          for s, k in m["keyframes"].items()}
    pt = {s: dict(bad=p["bad"], nobs=int(p.get("n_obs", len(p["obs"]))), obs=[o[0] for o in p["obs"]], idx=[o[1] for o in p["obs"]]) for s, p in m["points"].items()}
    return dict(kf=kf, pt=pt)


# ---------------------------------------------------------------------------------------------------------------- the named scenes
# Keypoint i of keyframe s has uR = 100 s + i - 2 (>= 0 from keyframe 1 on) unless i is in mono: an observation there weighs 2, a mono one 1.
# The query is [1, 2] everywhere; keyframes 3.. are fixed cameras.  Keyframe 0 is not used.
def survives_and_dies():
    """Point 0 (kf 1 kp 0 mono, kf 2 kp 0 stereo, kf 3 kp 0 stereo: n_obs 5) loses kf 2: n_obs 3, it stays.  Point 1 (kf 1 kp 1 stereo, kf 2 kp 1
    mono, kf 3 kp 1 mono: n_obs 4) loses kf 1: n_obs 2, it goes bad and kf 2, kf 3 lose their entries."""
    sc = S.Scene()
    sc.kf(1, 1, [0, 1], mono=[0]); sc.kf(2, 2, [0, 1], mono=[1]); sc.kf(3, 3, [0, 1], mono=[1])
    sc.pt(0); sc.pt(1)
    m = complete(sc.link(), refs=False)
    for p, r in ((0, 1), (1, 1)): m["points"][p]["ref_kf"] = r
    return m, [1, 2], dict(point_kfs=[(0, 2), (1, 1)])


def ref_erased_and_stranger():
    """Point 0 (kf 1, 2, 3, 4 all stereo: n_obs 8) has mpRefKF = kf 1 and loses kf 1 and kf 3: the reference becomes kf 2, the first of the
    row (2, 4).  Point 1 (kf 1, 2 stereo: n_obs 4) has mpRefKF = kf 4, which does not observe it: its level is keypoint 0 of kf 4."""
    sc = S.Scene()
    sc.kf(1, 1, [0, 1]); sc.kf(2, 2, [0, 1]); sc.kf(3, 3, [0]); sc.kf(4, 4, [5, 0])
    sc.pt(0); sc.pt(1); sc.pt(5)
    m = complete(sc.link(), refs=False)
    m["points"][0]["ref_kf"] = 1; m["points"][1]["ref_kf"] = 4; m["points"][5]["ref_kf"] = 4
    return m, [1, 2], dict(point_kfs=[(0, 1), (0, 3)])


def cascade():
    """Point 0's row is kf 1 (kp 0, stereo), kf 2 (kp 0, mono), kf 3 (kp 1; bad, its point row holds point 7 there), kf 4 (kp 3; never set):
    n_obs 4.  It loses kf 1: n_obs 2, bad.  The cascade clears kp 0 of kf 2, kp 1 of kf 3 although that entry is point 7, and skips kf 4."""
    sc = S.Scene()
    sc.kf(1, 1, [0, 3]); sc.kf(2, 2, [0, 3], mono=[0]); sc.kf(3, 3, [3, 7], bad=1)
    sc.pt(0, obs=[(1, 0), (2, 0), (3, 1), (4, 3)]); sc.pt(3); sc.pt(7, obs=[(3, 1)])
    m = complete(sc.link(), refs=False)
    m["points"][0]["n_obs"] = 4
    for p in (0, 3, 7): m["points"][p]["ref_kf"] = 1
    return m, [1, 2], dict(point_kfs=[(0, 1)])


def lines():
    """Line 0 (kf 1, 2, 3 kl 0, all with partners: n_obs 6) loses kf 2 (both flags set: one erasure): n_obs 4, bad - kf 1 and kf 3 keep their
    entries, kf 2 lost its.  Line 1 (kf 1, 2, 3 kl 1; kf 3's without a partner; n_obs 7) loses kf 3: n_obs 6, it stays with the row (1, 2).
    Line 2 (kf 1, 2 kl 2, n_obs 4) is removed: its flags do nothing and its position stays."""
    sc = S.Scene()
    sc.kf(1, 1, [0], [0, 1, 2]); sc.kf(2, 2, [0], [0, 1, 2]); sc.kf(3, 3, [0], [0, 1], no_partner=[1])
    sc.pt(0); sc.ln(0, n_obs=6); sc.ln(1, n_obs=7); sc.ln(2, n_obs=4)
    m = complete(sc.link())
    return m, [1, 2], dict(both=[(0, 2), (2, 1)], line_kfs=[(1, 3), (2, 2)], removed=[2])


NAMED = dict(survives_and_dies=survives_and_dies, ref_erased_and_stranger=ref_erased_and_stranger, cascade=cascade, lines=lines)


# ---------------------------------------------------------------------------------------------------------------- scene and answer files
def write_scene(path, m, query, win, res, tcw_local, limits, cam=S.CAM, sigma2=S.SIGMA2, level_scale=LEVEL_SCALE):
    """The file examples/map_ba_apply_scene.h reads: the map as flat tables over every slot of `limits`, the window, the result and the
    local cameras' poses as float matrices.  Keyframes with features must have one feature per row entry."""
    K, P, L = m["keyframes"], m["points"], m["lines"]
    nk, npt, nl = limits["max_keyframes"], limits["max_points"], limits["max_lines"]
    i32 = lambda v: np.asarray(v, np.int32).reshape(-1); u8 = lambda v: np.asarray(v, np.uint8).reshape(-1)
    f4 = lambda v: np.asarray(v, np.float32).reshape(-1); f8 = lambda v: np.asarray(v, np.float64).reshape(-1)
    start = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    flat = lambda rows, dt=np.int32: np.array([v for r in rows for v in r], dt).reshape(-1)
    refs = any("ref_kf" in p for p in P.values())
    kf = [K.get(s) for s in range(nk)]
    feat = [k is not None and "uvr" in k for k in kf]
    kp = [k["points"] if k else [] for k in kf]; kl = [k["lines"] if k else [] for k in kf]
    z = lambda n, w: np.zeros((n, w), np.float32)
    out = [i32([nk, npt, nl, len(sigma2), win["n_cams"], win["n_local_cams"], win["n_points"], win["n_pt_obs"], win["n_lines"], win["n_ln_obs"], int(refs), len(query)]),
           i32([limits[k] for k in ("max_keyframes", "max_points", "max_lines", "line_dim", "max_observations", "max_kf_points", "max_kf_lines", "max_children",
                                    "max_local_points", "max_local_lines")]),
           f8(cam), f4(sigma2), f4(level_scale), i32(query),
           u8([k is not None for k in kf]), u8([bool(k and k["bad"]) for k in kf]), u8(feat), u8([bool(k and k.get("octave") is not None) for k in kf]),
           np.array([k["key"] if k else 0 for k in kf], np.uint64), np.array([k["mn_id"] if f else 0 for k, f in zip(kf, feat)], np.uint64),
           f4([k["Tcw"] if f else np.eye(4) for k, f in zip(kf, feat)]),
           start(kp), flat(kp), start(kl), flat(kl),
           i32(np.concatenate([i32(k["octave"]) if k and k.get("octave") is not None else np.zeros(len(r), np.int32) for k, r in zip(kf, kp)] + [np.zeros(0, np.int32)])),
           f4(np.concatenate([np.asarray(k["uvr"], np.float32).reshape(-1, 3) if f else z(len(r), 3) for k, f, r in zip(kf, feat, kp)] + [z(0, 3)])),
           f4(np.concatenate([np.asarray(k["kl_left"], np.float32).reshape(-1, 4) if f else z(len(r), 4) for k, f, r in zip(kf, feat, kl)] + [z(0, 4)])),
           f4(np.concatenate([np.asarray(k["kl_right"], np.float32).reshape(-1, 4) if f else z(len(r), 4) for k, f, r in zip(kf, feat, kl)] + [z(0, 4)])),
           i32(np.concatenate([np.asarray(k["kl_octave"], np.int32).reshape(-1, 2) if f else np.zeros((len(r), 2), np.int32) for k, f, r in zip(kf, feat, kl)]
                              + [np.zeros((0, 2), np.int32)]))]
    pt = [P.get(s) for s in range(npt)]
    obs = [p["obs"] if p else [] for p in pt]
    out += [u8([0 if p is None else 2 if p["bad"] else 1 for p in pt]), f4([p["pos"] if p else np.zeros(3) for p in pt]), f4([p.get("nrm", np.zeros(3)) if p else np.zeros(3) for p in pt]),
            f4([p.get("mind", 0) if p else 0 for p in pt]), f4([p.get("maxd", 0) if p else 0 for p in pt]), i32([p.get("n_obs", len(p["obs"])) if p else 0 for p in pt]),
            i32([p.get("ref_kf", -1) if p else -1 for p in pt]), start(obs), flat([[o[0] for o in r] for r in obs]), flat([[o[1] for o in r] for r in obs])]
    ln = [L.get(s) for s in range(nl)]
    lobs = [l["obs"] if l and l["obs"] is not None else [] for l in ln]
    out += [u8([l is not None for l in ln]), u8([l is None or bool(l["bad"]) for l in ln]), u8([l is not None and l["obs"] is not None for l in ln]),
            f8([l["x0"] if l else np.zeros(3) for l in ln]), f8([l["dir"] if l else np.zeros(3) for l in ln]), i32([l["n_obs"] if l else -1 for l in ln]),
            start(lobs), flat([[o[0] for o in r] for r in lobs]), flat([[o[1] for o in r] for r in lobs])]
    out += [i32(win[k]) for k in ("cam_slot", "point_slot", "pt_obs_start", "pt_obs_cam", "line_slot", "ln_obs_start", "ln_obs_cam")]
    g = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    out += [f8(g("cam_qt")), f4(tcw_local), f8(g("pt_xyz")), f8(g("line_x0")), f8(g("line_dir")), u8(g("pt_obs_outlier")), u8(g("ln_edge_outlier")), u8(g("line_removed"))]
    with open(path, "wb") as f:
        for a in out:
            f.write(np.ascontiguousarray(a).tobytes())


def read_answer(path, win, limits):
    """what map_ba_apply_host_check and map_ba_harness apply write: the outputs of lld_map_ba_apply_out and the six pools over every slot"""
    buf = open(path, "rb").read()
    at = [0]

    def take(dt, n, shape=None):
        a = np.frombuffer(buf, dt, n, at[0]).copy(); at[0] += a.nbytes
        return a if shape is None else a.reshape(shape)
    r = dict(zip(("n_local_cams", "n_pt_obs_erased", "n_ln_obs_erased", "n_points_bad", "n_lines_bad", "n_index_skipped"), take(np.int32, 6).tolist()))
    nloc, npt, nl = r["n_local_cams"], int(win["n_points"]), int(win["n_lines"])
    r["tcw"] = take(np.float32, 16 * nloc, (-1, 4, 4)); r["ow"] = take(np.float32, 3 * nloc, (-1, 3))
    r["pt_pos"] = take(np.float32, 3 * npt, (-1, 3)); r["pt_normal"] = take(np.float32, 3 * npt, (-1, 3))
    r["pt_min_distance"] = take(np.float32, npt); r["pt_max_distance"] = take(np.float32, npt)
    for k in ("pt_n_obs", "pt_ref_kf", "pt_row_len"): r[k] = take(np.int32, npt)
    r["pt_flags"] = take(np.uint8, npt); r["ln_bad"] = take(np.uint8, nl); r["ln_n_obs"] = take(np.int32, nl); r["ln_row_len"] = take(np.int32, nl)
    n_of = dict(pt=limits["max_points"], kf=limits["max_keyframes"], ln=limits["max_lines"])
    rows = {}
    for kind, which in POOLS:
        start = take(np.int32, n_of[which] + 1); data = take(np.int32, int(start[-1]))
        rows[kind] = [data[start[i]:start[i + 1]].tolist() for i in range(n_of[which])]
    assert at[0] == len(buf)
    return r, rows
