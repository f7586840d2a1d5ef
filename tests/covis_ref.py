"""A plain-Python restatement of the covisibility counting the library runs on the device (lld_covisibility, include/lld_amd.h):
KeyFrame::UpdateConnections (src/KeyFrame.cc:312-402) and the redundancy count of LocalMapping::KeyFrameCulling
(src/LocalMapping.cc:633-697), on the same flat arrays.  It is written the way the reference works - a dict per query that is
then walked in slot order (the std::map), sorted pairs pushed to the front, the early break - and imports nothing from the
library.

A scene is a dict: n_kf; obs_start, obs_kf, obs_octave (CSR over the map points); point_bad, point_nobs; query_kf (-1: exclude
nobody); q_start, q_point, q_octave, q_depth (CSR over the queries); q_th_depth; monocular."""
import numpy as np

TH = 15
TH_OBS = 3
REDUNDANT_RATIO = 0.9


def update_connections_query(sc, q, th=TH):
    """One query: (conn [(slot, weight)] in slot order, ordered [(slot, weight)], n_max, kf_max, updated)."""
    own = int(sc["query_kf"][q])
    counter = {}
    for e in range(int(sc["q_start"][q]), int(sc["q_start"][q + 1])):
        p = int(sc["q_point"][e])
        if sc["point_bad"][p]:
            continue
        for o in range(int(sc["obs_start"][p]), int(sc["obs_start"][p + 1])):
            kf = int(sc["obs_kf"][o])
            if kf == own:
                continue
            counter[kf] = counter.get(kf, 0) + 1
    if not counter:
        return [], [], 0, -1, 0
    nmax, kfmax = 0, None
    pairs = []
    for kf in sorted(counter):                       # the std::map walks its keys in ascending order
        w = counter[kf]
        if w > nmax:
            nmax, kfmax = w, kf
        if w >= th:
            pairs.append((w, kf))
    if not pairs:
        pairs.append((nmax, kfmax))
    pairs.sort()                                     # pair<int, KeyFrame*>: by weight, then by pointer
    ordered = []
    for w, kf in pairs:
        ordered.insert(0, (kf, w))                   # push_front
    return [(kf, counter[kf]) for kf in sorted(counter)], ordered, nmax, kfmax, 1


def update_connections_ref(sc, th=TH):
    nq = len(sc["query_kf"])
    out = dict(conn_start=[0], conn_kf=[], conn_weight=[], ordered_start=[0], ordered_kf=[], ordered_weight=[], n_max=[], kf_max=[],
               updated=[])
    for q in range(nq):
        conn, ordered, nmax, kfmax, upd = update_connections_query(sc, q, th)
        out["conn_kf"] += [c[0] for c in conn]; out["conn_weight"] += [c[1] for c in conn]
        out["ordered_kf"] += [c[0] for c in ordered]; out["ordered_weight"] += [c[1] for c in ordered]
        out["conn_start"].append(len(out["conn_kf"])); out["ordered_start"].append(len(out["ordered_kf"]))
        out["n_max"].append(nmax); out["kf_max"].append(kfmax); out["updated"].append(upd)
    return {k: np.array(v, np.uint8 if k == "updated" else np.int32) for k, v in out.items()}


def keyframe_culling_query(sc, q, th_obs=TH_OBS, ratio=REDUNDANT_RATIO):
    own = int(sc["query_kf"][q])
    th_depth = np.float32(sc["q_th_depth"][q])
    n_mps = n_red = 0
    for e in range(int(sc["q_start"][q]), int(sc["q_start"][q + 1])):
        p = int(sc["q_point"][e])
        if sc["point_bad"][p]:
            continue
        if not sc["monocular"]:
            d = np.float32(sc["q_depth"][e])
            if d > th_depth or d < 0:
                continue
        n_mps += 1
        if int(sc["point_nobs"][p]) > th_obs:
            level = int(sc["q_octave"][e])
            n = 0
            for o in range(int(sc["obs_start"][p]), int(sc["obs_start"][p + 1])):
                if int(sc["obs_kf"][o]) == own:
                    continue
                if int(sc["obs_octave"][o]) <= level + 1:
                    n += 1
                    if n >= th_obs:
                        break
            if n >= th_obs:
                n_red += 1
    return n_mps, n_red, 1 if n_red > ratio * n_mps else 0


def keyframe_culling_ref(sc, th_obs=TH_OBS, ratio=REDUNDANT_RATIO):
    r = [keyframe_culling_query(sc, q, th_obs, ratio) for q in range(len(sc["query_kf"]))]
    return dict(n_mps=np.array([x[0] for x in r], np.int32), n_redundant=np.array([x[1] for x in r], np.int32),
                redundant=np.array([x[2] for x in r], np.uint8))
