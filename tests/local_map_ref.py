"""Tracking::UpdateLocalMap (src/Tracking.cc:1667-1835 of the reference) restated in plain Python over dicts and lists: the independent
reference of the resident-map tests.  It imports nothing from the package under test.

A map is a dict:
  keyframes  {slot: dict(key, bad, parent (slot or None), cov [slots, GetBestCovisibilityKeyFrames order], child [slots], points [slot or -1 per
             keypoint], lines [slot or -1])}
  points     {slot: dict(bad, obs [keyframe slots])}
  lines      {slot: dict(bad)}
`state` carries what Tracking keeps between frames: dict(local_keyframes=[...]) (mvpLocalKeyFrames).  The limits (1024 voted keyframes,
max_local_points, max_local_lines) are the library's: the reference has none, so they are applied on top as the interface documents them."""

KEYFRAME_OVERFLOW, POINT_OVERFLOW, LINE_OVERFLOW = 1, 2, 4
MAX_VOTED = 1024


def new_state():
    return dict(local_keyframes=[])


def update_local_keyframes(state, m, frame_ids):
    """:1726-1835.  frame_ids: mCurrentFrame.mvpMapPoints as point slots (-1: NULL; a slot the map does not hold: a temporal point).  Returns
    (frame_ids after the bad ones left, n_voted, n_cleared, pKFmax or None, vote_empty, overflow)."""
    kfs, pts = m["keyframes"], m["points"]
    ids = list(frame_ids)
    counter = {}
    cleared = 0
    for i, pid in enumerate(ids):
        if pid < 0 or pid not in pts:
            continue
        p = pts[pid]
        if not p["bad"]:
            for kf in p["obs"]:
                counter[kf] = counter.get(kf, 0) + 1
        else:
            ids[i] = -1
            cleared += 1
    if not counter:
        return ids, 0, cleared, None, True, False
    if len(counter) > MAX_VOTED:
        return ids, len(counter), cleared, None, False, True
    best, kf_max = 0, None
    local = []
    marked = set()
    for kf in sorted(counter, key=lambda s: kfs[s]["key"]):            # std::map<KeyFrame*,int>: pointer order
        if kfs[kf]["bad"]:
            continue
        if counter[kf] > best:
            best, kf_max = counter[kf], kf
        local.append(kf)
        marked.add(kf)
    n_first = len(local)                                                # itEndKF is taken before the pushes
    for i in range(n_first):
        if len(local) > 80:
            break
        kf = kfs[local[i]]
        for nb in kf["cov"][:10]:
            if not kfs[nb]["bad"] and nb not in marked:
                local.append(nb); marked.add(nb)
                break
        for ch in sorted(kf["child"], key=lambda s: kfs[s]["key"]):     # std::set<KeyFrame*>
            if not kfs[ch]["bad"] and ch not in marked:
                local.append(ch); marked.add(ch)
                break
        par = kf["parent"]
        if par is not None and par >= 0 and par not in marked:
            local.append(par); marked.add(par)
            break                                                       # leaves the outer loop (:1824)
    state["local_keyframes"] = local
    return ids, len(counter), cleared, kf_max, False, False


def update_local_points(state, m):
    """:1677-1723 -> (mvpLocalMapPoints, local_lines) as slots."""
    kfs, pts, lns = m["keyframes"], m["points"], m["lines"]
    lp, ll = [], []
    seen_p, seen_l = set(), set()
    for kf in state["local_keyframes"]:
        for s in kfs[kf]["points"]:
            if s < 0 or s in seen_p or s not in pts:
                continue
            if not pts[s]["bad"]:
                lp.append(s); seen_p.add(s)
        for s in kfs[kf]["lines"]:
            if s < 0 or s in seen_l or s not in lns:
                continue
            if not lns[s]["bad"]:
                ll.append(s); seen_l.add(s)
    return lp, ll


def update_local_map(state, m, frame_ids, max_local_points, max_local_lines):
    ids, n_voted, cleared, kf_max, empty, overflow = update_local_keyframes(state, m, frame_ids)
    out = dict(frame_ids=ids, n_voted=n_voted, n_bad_cleared=cleared, ref_keyframe=-1 if kf_max is None else kf_max, vote_empty=int(empty),
               status=KEYFRAME_OVERFLOW if overflow else 0)
    if overflow:
        return out
    lp, ll = update_local_points(state, m)
    out.update(local_keyframes=list(state["local_keyframes"]), local_points=lp, local_lines=ll)
    if len(lp) > max_local_points:
        out["status"] |= POINT_OVERFLOW
    if len(ll) > max_local_lines:
        out["status"] |= LINE_OVERFLOW
    return out
