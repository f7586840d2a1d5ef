"""Maps for the tests of lld_map_refresh_points / _lines (tests/map_refresh_ref.py holds the rules): what tests/map_ba_scenes.py builds,
dressed with the keyframes' descriptor rows, the landmarks' current values and mpRefKF, their upload into a DeviceMap, and the crafted maps
whose rows have the lengths at which the kernels change path.  numpy only."""
import numpy as np

import map_ba_apply_scenes as AS
import map_ba_scenes as S

f32 = np.float32
LEVEL_SCALE = AS.LEVEL_SCALE                       # N_LEVELS = 4, as the octaves of map_ba_scenes
WAVE, MAX_OBS, MAX_LINE_OBS = 64, 1024, 64         # rf_point_wave's rows, LLD_LANDMARK_MAX_OBS, LLD_LANDMARK_MAX_LINE_OBS


def flipped(rng, base, max_flips=6):
    d = np.array(base, np.uint32)
    for b in rng.integers(0, 256, rng.integers(0, max_flips + 1)):
        d[b >> 5] ^= np.uint32(1 << (b & 31))
    return d


def dress(m, seed, dim=S.LINE_DIM, never_set=0.05, all_scaled=False):
    """Descriptor rows for every keyframe (a point's base pattern with a few bits flipped per observer, so that equal medians are common; a
    line's unit-norm base row with noise, half of the lines scaled by about 100 so that the truncated medians differ), current values for
    every landmark, mpRefKF (AS.complete), and never-set keyframe slots in some observation rows."""
    rng = np.random.default_rng(0xDE5C + seed)
    K, P, L = m["keyframes"], m["points"], m["lines"]
    every_pt = {s for k in K.values() for s in k["points"] if s >= 0} | set(P)
    every_ln = {s for k in K.values() for s in k["lines"] if s >= 0} | set(L)
    base = {p: rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32) for p in every_pt}
    lbase = {}
    for l in every_ln:
        v = np.abs(rng.normal(0, 1, dim)); lbase[l] = (v / np.linalg.norm(v)) * (rng.uniform(95, 105) if l % 2 or all_scaled else 1.0)
    for k in K.values():
        k["desc"] = np.array([flipped(rng, base[p]) if p >= 0 else rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32) for p in k["points"]],
                             np.uint32).reshape(-1, 8)
        rows = [lbase[l] + rng.normal(0, 1, dim) * rng.uniform(0.005, 0.06) * np.linalg.norm(lbase[l]) if l >= 0 else rng.normal(0, 1, dim) for l in k["lines"]]
        k["ldesc"] = np.array(rows, f32).reshape(-1, dim)
    free = [s for s in range(max(K) + 2) if s not in K]
    for p in P.values():
        if free and p["obs"] and rng.random() < never_set:
            p["obs"].insert(int(rng.integers(0, len(p["obs"]) + 1)), (free[0], int(rng.integers(0, 4))))
    AS.complete(m, seed)
    for s, p in P.items():
        p["desc"] = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
    for l in L.values():
        l["desc"] = rng.normal(0, 1, dim).astype(f32)
    return m


def limits(m, dim=S.LINE_DIM, **over):
    L = S.limits_for(m, line_dim=dim)
    L["max_keyframes"] = max(L["max_keyframes"], max([kf for p in m["points"].values() for kf, _ in p["obs"]] + [0]) + 1)
    L.update(over)
    return L


def upload_points(dm, m, slots=None):
    slots = sorted(m["points"]) if slots is None else list(slots)
    if not slots:
        return
    P = [m["points"][s] for s in slots]
    z3 = np.zeros(3, f32)
    dm.set_points(slots, np.array([p["pos"] for p in P], f32), np.array([p.get("nrm", z3) for p in P], f32), np.array([p.get("mind", 0) for p in P], f32),
                  np.array([p.get("maxd", 0) for p in P], f32), np.array([p.get("desc", np.zeros(8)) for p in P], np.uint32), [p["bad"] for p in P])


def upload_lines(dm, m, slots=None):
    slots = sorted(m["lines"]) if slots is None else list(slots)
    if not slots:
        return
    Ls = [m["lines"][s] for s in slots]
    dim = dm.limits.line_dim
    x0 = np.array([l["x0"] for l in Ls], np.float64); d = np.array([l["dir"] for l in Ls], np.float64)
    dm.set_lines(slots, x0, d, x0, x0 + d, np.array([l.get("desc", np.zeros(dim)) for l in Ls], f32), [l["bad"] for l in Ls])


def upload_descriptors(dm, m, slots=None):
    slots = sorted(m["keyframes"]) if slots is None else list(slots)
    K = m["keyframes"]
    pt = [s for s in slots if "desc" in K[s]]; ln = [s for s in slots if "ldesc" in K[s]]
    if pt: dm.set_keyframe_descriptors(pt, [K[s]["desc"] for s in pt])
    if ln: dm.set_keyframe_line_descriptors(ln, [K[s]["ldesc"] for s in ln])


def upload(dm, m):
    S.upload_keyframes(dm, m)
    upload_points(dm, m)
    slots = sorted(m["points"])
    ix = [s for s in slots if m["points"][s].get("indexed", True)]; pl = [s for s in slots if not m["points"][s].get("indexed", True)]
    if ix: dm.set_observations_indexed(ix, rows=[m["points"][s]["obs"] for s in ix], n_obs=[int(m["points"][s].get("n_obs", len(m["points"][s]["obs"]))) for s in ix])
    if pl: dm.set_observations(pl, rows=[[o[0] for o in m["points"][s]["obs"]] for s in pl])
    refs = [s for s in slots if "ref_kf" in m["points"][s]]
    if refs: dm.set_point_refs(refs, [m["points"][s]["ref_kf"] for s in refs])
    upload_lines(dm, m)
    ob = [s for s in sorted(m["lines"]) if m["lines"][s]["obs"] is not None]
    if ob: dm.set_line_observations(ob, [m["lines"][s]["obs"] for s in ob], [m["lines"][s]["n_obs"] for s in ob])
    upload_descriptors(dm, m)


def widths(point_rows, line_rows, seed=0, dim=S.LINE_DIM):
    """One map whose point slot i has an observation row of point_rows[i] entries and whose line slot i one of line_rows[i]: keyframe s sees
    every landmark with a longer row than s, every seventh keyframe is bad, key order is scrambled against slot order."""
    sc = S.Scene()
    n = max(list(point_rows) + list(line_rows))
    for s in range(n):
        sc.kf(s, s + 1, [i for i, w in enumerate(point_rows) if s < w], [i for i, w in enumerate(line_rows) if s < w], bad=(s % 7 == 3), key=1 + (s * 389) % 2003)
    at = {s: ({p: i for i, p in enumerate(k["points"])}, {l: i for i, l in enumerate(k["lines"])}) for s, k in sc.m["keyframes"].items()}
    order = sorted(sc.m["keyframes"], key=lambda s: sc.m["keyframes"][s]["key"])
    for i, w in enumerate(point_rows): sc.pt(i, obs=[(s, at[s][0][i]) for s in order if s < w])
    for i, w in enumerate(line_rows): sc.ln(i, obs=[(s, at[s][1][i]) for s in order if s < w], n_obs=2 * w)
    m = dress(sc.link(), seed, dim, never_set=0, all_scaled=True)
    for p in m["points"].values():
        p["ref_kf"] = p["obs"][len(p["obs"]) // 2][0]                      # an observer: every point of this map can be refreshed
    return m
