"""A plain-Python restatement of lld_map_covisibility (include/lld_amd.h, "covisibility on the resident map"): KeyFrame::UpdateConnections
(src/KeyFrame.cc:312-402) and the redundancy count of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:646-694) on the map's tables -
rows by slot, order_key for map order, -1 entries in the point rows, keypoint rows beside them.  It imports nothing from the library.

Tables:
  kf[slot] = dict(key, points=[point slot or -1 per keypoint], octave=[...] or None, depth=[...] or None, th_depth)     a keyframe that is set
  pt[slot] = dict(bad, nobs, obs=[keyframe slot ...], idx=[keypoint index ...] or None)                                 a point that is set
A slot missing from pt is a point never set: its row is empty, it is not bad and its Observations() is 0.

One deliberate difference from the reference's text: KeyFrameCulling stops counting an observation row at th_obs, the device walks the whole
row (the test `count >= th_obs` does not depend on that) and so answers NO_KEYPOINT_DATA for an unusable index anywhere in a walked row."""
import numpy as np

TH = 15
TH_OBS = 3
REDUNDANT_RATIO = 0.9
MAX_CONNECTED = 4096
CONN_OVERFLOW, NO_KEYPOINT_DATA = 1, 2


def connections_query(T, own, th=TH):
    """(conn [(slot, weight)] in ascending order_key, ordered [(slot, weight)], n_max, kf_max, updated, status)"""
    counter = {}
    for p in T["kf"][own]["points"]:
        if p < 0:
            continue
        pt = T["pt"].get(p)
        if pt is None or pt["bad"]:
            continue
        for k in pt["obs"]:
            if k != own:
                counter[k] = counter.get(k, 0) + 1
    if not counter:
        return [], [], 0, -1, 0, 0
    if len(counter) > MAX_CONNECTED:
        return [], [], 0, -1, 0, CONN_OVERFLOW
    key = lambda k: T["kf"][k]["key"]
    nmax, kfmax, pairs = 0, None, []
    in_map_order = sorted(counter, key=key)                  # the std::map walks its keys in ascending (pointer) order
    for k in in_map_order:
        w = counter[k]
        if w > nmax:
            nmax, kfmax = w, k
        if w >= th:
            pairs.append((w, key(k), k))
    if not pairs:
        pairs.append((nmax, key(kfmax), kfmax))
    pairs.sort()                                             # pair<int, KeyFrame*>: by weight, then by pointer
    ordered = []
    for w, _, k in pairs:
        ordered.insert(0, (k, w))                            # push_front
    return [(k, counter[k]) for k in in_map_order], ordered, nmax, kfmax, 1, 0


def culling_query(T, own, monocular, th_obs=TH_OBS, ratio=REDUNDANT_RATIO):
    """(n_mps, n_redundant, redundant, status)"""
    kf = T["kf"][own]
    n = len(kf["points"])
    if kf["octave"] is None or kf["depth"] is None or len(kf["octave"]) != n or len(kf["depth"]) != n:
        return 0, 0, 0, NO_KEYPOINT_DATA
    th_depth = np.float32(kf["th_depth"])
    n_mps = n_red = 0
    for j, p in enumerate(kf["points"]):
        if p < 0:
            continue
        pt = T["pt"].get(p)
        if pt is not None and pt["bad"]:
            continue
        if not monocular:
            d = np.float32(kf["depth"][j])
            if d > th_depth or d < 0:
                continue
        n_mps += 1
        if pt is None:
            continue
        if len(pt["idx"] or []) != len(pt["obs"]):              # the row came without indices: its Observations() is not known either
            return 0, 0, 0, NO_KEYPOINT_DATA
        if pt["nobs"] <= th_obs:
            continue
        level, cnt = kf["octave"][j], 0
        for k, i in zip(pt["obs"], pt["idx"]):
            if k == own:
                continue
            other = T["kf"].get(k)
            row = other["octave"] if other is not None and other["octave"] is not None else []
            if i >= len(row):
                return 0, 0, 0, NO_KEYPOINT_DATA
            if row[i] <= level + 1:
                cnt += 1
        if cnt >= th_obs:
            n_red += 1
    return n_mps, n_red, 1 if n_red > ratio * n_mps else 0, 0


def covisibility(T, queries, connections=True, culling=False, monocular=False, th=TH, th_obs=TH_OBS, ratio=REDUNDANT_RATIO):
    """The arrays DeviceMap.covisibility returns."""
    out = dict(status=[0] * len(queries))
    if connections:
        out.update(conn_start=[0], conn_kf=[], conn_weight=[], ordered_start=[0], ordered_kf=[], ordered_weight=[], n_max=[], kf_max=[], updated=[])
    if culling:
        out.update(n_mps=[], n_redundant=[], redundant=[])
    for q, own in enumerate(queries):
        if culling:
            nm, nr, red, st = culling_query(T, own, monocular, th_obs, ratio)
            out["n_mps"].append(nm); out["n_redundant"].append(nr); out["redundant"].append(red); out["status"][q] |= st
        if connections:
            conn, ordered, nmax, kfmax, upd, st = connections_query(T, own, th)
            out["conn_kf"] += [c[0] for c in conn]; out["conn_weight"] += [c[1] for c in conn]
            out["ordered_kf"] += [c[0] for c in ordered]; out["ordered_weight"] += [c[1] for c in ordered]
            out["conn_start"].append(len(out["conn_kf"])); out["ordered_start"].append(len(out["ordered_kf"]))
            out["n_max"].append(nmax); out["kf_max"].append(kfmax); out["updated"].append(upd); out["status"][q] |= st
    return {k: np.array(v, np.uint8 if k in ("updated", "redundant", "status") else np.int32) for k, v in out.items()}


def cov_row(T, own, th=TH):
    """GetBestCovisibilityKeyFrames(10) after UpdateConnections, or None where lld_map_covisibility leaves the row alone."""
    _, ordered, _, _, upd, st = connections_query(T, own, th)
    return [k for k, _ in ordered[:10]] if upd and not st else None


# ---- a flat scene of tests/covis_scenes.py as tables -----------------------------------------------------------------------------------
def tables_from_scene(sc, kf_slot, kf_key, pt_slot):
    """Keyframe k of the scene gets slot kf_slot[k] and order_key kf_key[k], point p slot pt_slot[p].  A keyframe's keypoints are the entries of
    its query (each keyframe is queried at most once), followed by one keypoint without a map point per observation it makes, which carries
    that observation's octave: the scene gives the octave per observation, the map gives it through the observer's keypoint row."""
    nk = int(sc["n_kf"])
    kf = {int(kf_slot[k]): dict(key=int(kf_key[k]), points=[], octave=[], depth=[], th_depth=0.0) for k in range(nk)}
    seen = set()
    for q, k in enumerate(sc["query_kf"]):
        k = int(k)
        assert k >= 0 and k not in seen
        seen.add(k)
        row = kf[int(kf_slot[k])]
        for e in range(int(sc["q_start"][q]), int(sc["q_start"][q + 1])):
            row["points"].append(int(pt_slot[sc["q_point"][e]])); row["octave"].append(int(sc["q_octave"][e])); row["depth"].append(float(sc["q_depth"][e]))
        row["th_depth"] = float(sc["q_th_depth"][q])
    pt = {}
    for p in range(len(sc["point_bad"])):
        obs, idx = [], []
        for o in range(int(sc["obs_start"][p]), int(sc["obs_start"][p + 1])):
            row = kf[int(kf_slot[sc["obs_kf"][o]])]
            obs.append(int(kf_slot[sc["obs_kf"][o]])); idx.append(len(row["points"]))
            row["points"].append(-1); row["octave"].append(int(sc["obs_octave"][o])); row["depth"].append(1.0)
        pt[int(pt_slot[p])] = dict(bad=bool(sc["point_bad"][p]), nobs=int(sc["point_nobs"][p]), obs=obs, idx=idx)
    return dict(kf=kf, pt=pt)


def renumber(r, slot_to_kf):
    """A result on slots, with every keyframe renamed by slot_to_kf (a dict): comparable with covis_ref on a scene whose keyframes are
    numbered in map order."""
    r = dict(r)
    for name in ("conn_kf", "ordered_kf", "kf_max"):
        if name in r:
            r[name] = np.array([slot_to_kf[int(s)] if s >= 0 else -1 for s in r[name]], np.int32)
    return r
