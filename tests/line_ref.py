"""Plain numpy restatements of the line matchers, shared by the CPU and the GPU tests (a helper module, not a test file):
TwoFrameLineMatcher::MatchLines (src/TwoFrameLineMatcher.cc:26-124), GetHoughCoordinates / SubselectWithGrid (src/LineMatching.cc:63-180),
Tracking::AddLinesFrom (src/Tracking.cc:996-1124) and Tracking::MatchLinesLastKF (:1474-1592).  Nothing here comes
from the package under test.  Degenerate lines (coincident end points, zero direction) are not restated: numpy has no integer cast of
NaN; they stay with the oracle comparison."""
import numpy as np


# ---------------------------------------------------------------- GetHoughCoordinates
def _hough_centre(leq, sx, sy):
    """src/LineMatching.cc:63-110: centre cell and the signs of the rounding residues, (di, sd, ai, sa)."""
    l = np.array(leq, float); l[0] /= sx; l[1] /= sy
    l = l / np.hypot(l[0], l[1])
    if l[1] < 0:
        l = -l
    dl = abs(l[2] / np.sqrt(2.0)) * 50
    di = int(np.floor(dl + 0.5)); di = max(min(di, 49), 0)
    sd = 1 if dl - di < 0 else -1
    al = np.arctan2(l[1], l[0]) / 3.14159265 * 50
    ai = int(np.floor(al + 0.5)); ai = max(min(ai, 49), 0)
    sa = 1 if al - ai < 0 else -1
    return di, sd, ai, sa


def hough_naive(leq, sx, sy, step_dist=3, step_ang=3):
    """src/LineMatching.cc:63-152 read line by line."""
    di, sd, ai, sa = _hough_centre(leq, sx, sy)
    ang = []
    amax = max(ai, ai + sa)
    for i in range(amax, amax + step_ang):
        ang.append((i + 50 if i < 0 else i) % 50)
    amin = min(ai, ai + sa)
    for i in range(amin, amin - step_ang, -1):
        ang.append((i + 50 if i < 0 else i) % 50)
    dist = []
    dmax = max(di, di + sd)
    for i in range(dmax, dmax + step_dist):
        if 0 <= i < 49:
            dist.append(i)
    dmin = min(di, di + sd)
    for i in range(dmin, dmin - step_dist, -1):
        if 0 <= i < 49:
            dist.append(i)
    return dist, ang, di, ai


def hough_window_origin(leq, sx, sy):
    """(ang_min, dist_min): the smaller of the centre cell and its shifted neighbour, per axis.  The window of step 3 is the six angle
    cells ang_min - 2 .. ang_min + 3 (modulo 50) times the six distance rows dist_min - 2 .. dist_min + 3 (those in 0..48)."""
    di, sd, ai, sa = _hough_centre(leq, sx, sy)
    return min(ai, ai + sa), min(di, di + sd)


def line_cells(lines, sx, sy):
    """The centre cell (di, ai) of every KeyLine [n,4]: the grid fill this build defines."""
    ll = np.asarray(lines, np.float64)
    out = np.zeros((ll.shape[0], 2), np.int64)
    for si in range(ll.shape[0]):
        leq = np.cross([ll[si, 0], ll[si, 1], 1.0], [ll[si, 2], ll[si, 3], 1.0])
        _, _, di, ai = hough_naive(leq, sx, sy, 0, 0)
        out[si] = di, ai
    return out


def _window_mask(leq, cells, sx, sy):
    dist, ang, _, _ = hough_naive(leq, sx, sy)
    return np.isin(cells[:, 0], dist) & np.isin(cells[:, 1], ang)


def _image_line(K, R, t, X0, d):
    a = K @ (R.T @ (X0 - t)); b = K @ (R.T @ (X0 + d - t))
    l = np.cross(a, b)
    return l / np.hypot(l[0], l[1])


def _err_l1(kl, l):
    """vgl::LineReprojErrorL1 of KeyLines [n,4] against the image line l."""
    return np.abs(kl[:, 0] * l[0] + kl[:, 1] * l[1] + l[2]) + np.abs(kl[:, 2] * l[0] + kl[:, 3] * l[1] + l[2])


def l2_rows(a, B):
    """MatchLineDescriptors of one descriptor against the rows of B: float difference, double accumulation in ascending component."""
    df = (np.asarray(B, np.float32) - np.asarray(a, np.float32)[None, :]).astype(np.float32)
    acc = np.zeros(df.shape[0])
    for k in range(df.shape[1]):
        acc = acc + df[:, k].astype(np.float64) ** 2
    return np.sqrt(acc)


def dist_matrix(dl, dr):
    dl = np.asarray(dl, np.float32); dr = np.asarray(dr, np.float32)
    return np.stack([l2_rows(dl[j], dr) for j in range(dl.shape[0])]) if dl.shape[0] else np.zeros((0, dr.shape[0]))


# ---------------------------------------------------------------- Tracking::AddLinesFrom
def track_row_lines(P, L):
    """The projected image line of every map line in the left and the right camera."""
    K, T = P["K"], P["T_curr"]; R, t = T[:3, :3], T[:3, 3]
    tr = t + R @ np.array([P["b"], 0, 0])
    return [(_image_line(K, R, t, L["X0"][i], L["dir"][i]), _image_line(K, R, tr, L["X0"][i], L["dir"][i])) for i in range(L["X0"].shape[0])]


def track_naive(P, L, F, monocular=False, use_grid=True, want_gate=False):
    """Tracking::AddLinesFrom.  want_gate: also the order-independent gate matrix - [i][si] = 1 iff the pair passes every test but the
    descriptor threshold under the INITIAL occupancy; skipped rows and rows with a main point behind the camera are zero."""
    T = P["T_curr"]; R, t = T[:3, :3], T[:3, 3]
    n_map, n_cur = L["X0"].shape[0], F["left_lines"].shape[0]
    ll = F["left_lines"].astype(np.float64)
    cells = line_cells(ll, P["sx"], P["sy"])
    occ0 = F["occupied"].astype(bool) if F.get("occupied") is not None else np.zeros(n_cur, bool)
    occ = occ0.copy()
    lm = np.asarray(F["line_matches"], np.int64)
    thr = P["thr_reproj_base"] * 1.44 ** np.asarray(F["left_octave"], np.float64)
    rows = track_row_lines(P, L)
    matches = -np.ones(n_map, np.int64)
    gate = np.zeros((n_map, n_cur), np.uint8)
    for i in range(n_map):
        if L.get("skip") is not None and L["skip"][i]:
            continue
        if (R.T @ (L["X1"][i] - t))[2] < 0 or (R.T @ (L["X2"][i] - t))[2] < 0:
            continue
        lleft, lright = rows[i]
        g = _window_mask(lleft, cells, P["sx"], P["sy"]) if use_grid else np.ones(n_cur, bool)
        if not monocular:
            g = g & (lm >= 0)
        se = _err_l1(ll, lleft)
        se2 = np.zeros(n_cur)
        if not monocular:
            kr = F["right_lines"].astype(np.float64)[np.maximum(lm, 0)] if F["right_lines"].shape[0] else np.zeros((n_cur, 4))
            se2 = _err_l1(kr, lright)
        g = g & ~((se > thr) | (se2 > thr))
        gate[i] = g & ~occ0
        md, mid = 1e10, -1
        cand = np.flatnonzero(g & ~occ)
        if cand.size:
            cd = l2_rows(L["desc"][i], F["desc"][cand])
            k = int(np.argmin(cd))                                           # the first minimum: strict '<' in ascending index
            if cd[k] < md:
                md, mid = cd[k], int(cand[k])
        if md > P["md_thr"] or mid < 0:
            continue
        occ[mid] = True; matches[i] = mid
    return (matches, gate) if want_gate else matches


# ---------------------------------------------------------------- TwoFrameLineMatcher::MatchLines
def greedy_naive(D_or_descriptors, tau, gate=None):
    """The sequential loop of src/TwoFrameLineMatcher.cc:26-77.  D_or_descriptors: the [nq][nt] distance matrix, or (desc_left,
    desc_right).  Left line j takes the untaken, gated right line with the smallest distance below tau (strict), lowest index on ties."""
    D = dist_matrix(*D_or_descriptors) if isinstance(D_or_descriptors, tuple) else np.asarray(D_or_descriptors, np.float64)
    nq, nt = D.shape
    taken = np.zeros(nt, bool); out = -np.ones(nq, np.int64)
    for j in range(nq):
        ok = ~taken & (D[j] < tau)
        if gate is not None:
            ok &= np.asarray(gate[j]) != 0
        cand = np.flatnonzero(ok)
        if cand.size:
            bj = int(cand[np.argmin(D[j, cand])])
            taken[bj] = True; out[j] = bj
    return out


def sweeps_to_fixed_point(D, tau, gate=None, list_len=8):
    """A property of an INPUT of the greedy matcher.  Jacobi sweeps of its rule with complete preference lists: in a sweep every left
    line takes the first entry of its (distance, index)-sorted admissible list that no line with a smaller index took in the sweep
    before.  Returns (sweeps until no pick changes, the last, idle one included; the fixed point; the number of lines whose final pick
    lies beyond their list_len best or that end unmatched with >= list_len admissible candidates)."""
    D = np.asarray(D, np.float64); nq, nt = D.shape
    adm = D < tau
    if gate is not None:
        adm &= np.asarray(gate).reshape(nq, nt) != 0
    order = np.lexsort((np.broadcast_to(np.arange(nt), D.shape), np.where(adm, D, np.inf)), axis=1)
    n_adm = adm.sum(1)
    pref = np.where(np.arange(nt)[None, :] < n_adm[:, None], order, -1)
    pick = -np.ones(nq, np.int64); sweeps = 0; jj = np.arange(nq)
    big = np.iinfo(np.int64).max
    while True:
        blk = np.full(nt + 1, big)
        np.minimum.at(blk, np.where(pick >= 0, pick, nt), jj)
        blk[nt] = -1                                                      # the padding entry is never free
        free = blk[np.where(pref >= 0, pref, nt)] >= jj[:, None]
        first = np.argmax(free, axis=1)
        new = np.where(free.any(1), pref[jj, first], -1) if nt else pick
        sweeps += 1
        if np.array_equal(new, pick):
            break
        pick = new
    rank = np.where(pick >= 0, np.argmax(pref == pick[:, None], axis=1), -1) if nt else pick
    beyond = int(np.sum((rank >= list_len) | ((pick < 0) & (n_adm >= list_len))))
    return sweeps, pick, beyond


def normalized_line_eq(kl, K):
    l = K.T @ np.cross([kl[0], kl[1], 1.0], [kl[2], kl[3], 1.0])
    return l / np.linalg.norm(l[:2])


def triangulate_line(R, t1, t2, l1, l2):
    """vgl::TriangulateLine (src/vgl.cc:78-108) for two cameras with one rotation; None when the planes are too parallel."""
    n1, n2 = R @ l1, R @ l2
    if abs(n1 @ n2) / np.linalg.norm(n1) / np.linalg.norm(n2) > 0.975:
        return None
    d = np.cross(n1, n2); d /= np.linalg.norm(d)
    X0 = np.linalg.solve(np.stack([n1, n2, d]), np.array([n1 @ t1, n2 @ t2, 0.0]))
    return X0, d


def naive_match(s, tau, min_len, is_stereo=True):
    """TwoFrameLineMatcher::MatchLines with numpy linear algebra (np.linalg.solve / lstsq instead of the QR restatement)."""
    K, b = s["K"], s["b"]
    def leq(kl):
        l = K.T @ np.cross([kl[0], kl[1], 1.0], [kl[2], kl[3], 1.0]); return l / np.linalg.norm(l[:2])
    nL, nR = s["left"].shape[0], s["right"].shape[0]
    L = s["left"].astype(np.float64); R = s["right"].astype(np.float64)
    gate = np.zeros((nL, nR), np.uint8)
    eqL = [leq(k) for k in L]; eqR = [leq(k) for k in R]
    lenL = np.hypot(L[:, 0] - L[:, 2], L[:, 1] - L[:, 3]); lenR = np.hypot(R[:, 0] - R[:, 2], R[:, 1] - R[:, 3])
    for j in range(nL):
        for oi in range(nR):
            if (is_stereo and s["left_octave"][j] != s["right_octave"][oi]) or lenL[j] < min_len or lenR[oi] < min_len: continue
            n1, n2 = eqL[j], eqR[oi]
            if abs(n1 @ n2) / np.linalg.norm(n1) / np.linalg.norm(n2) > 0.975: continue
            d = np.cross(n1, n2); d /= np.linalg.norm(d)
            X0 = np.linalg.solve(np.stack([n1, n2, d]), np.array([0.0, n2 @ np.array([b, 0, 0]), 0.0]))
            if np.linalg.norm(X0) < 0.5: continue
            ok = True
            for e in (0, 2):
                M = np.stack([np.array([L[j, e], L[j, e + 1], 1.0]), -K @ d], 1)
                p = np.linalg.lstsq(M, K @ X0, rcond=None)[0][1]
                if (X0 + p * d)[2] < 0: ok = False
            gate[j, oi] = ok
    taken = np.zeros(nR, bool); out = -np.ones(nL, np.int64)
    for j in range(nL):
        best, bj = np.inf, -1
        for oi in range(nR):
            if taken[oi] or not gate[j, oi]: continue
            diff = (s["desc_left"][j] - s["desc_right"][oi]).astype(np.float32)
            dd = float(np.sqrt(np.sum(diff.astype(np.float64) ** 2)))
            if dd < best and dd < tau: best, bj = dd, oi
        if bj >= 0: taken[bj] = True
        out[j] = bj
    return out, gate


# ---------------------------------------------------------------- Tracking::MatchLinesLastKF
def lastkf_row_lines(P, cur):
    """Per line of the current frame: None where the reference skips it before the candidate loop (holds a map line, no stereo partner,
    TriangulateLine refuses), else the triangulated line projected into the left and the right camera of the last frame."""
    K = P["K"]; R, t = P["T_curr"][:3, :3], P["T_curr"][:3, 3]; Rl, tl = P["T_last"][:3, :3], P["T_last"][:3, 3]
    tr = t + R @ np.array([P["b"], 0, 0]); tlr = tl + Rl @ np.array([P["b"], 0, 0])
    cl = cur["left_lines"].astype(np.float64); cr = cur["right_lines"].astype(np.float64)
    out = []
    for i in range(cl.shape[0]):
        ri = int(cur["line_matches"][i])
        if (cur.get("occupied") is not None and cur["occupied"][i]) or ri < 0:
            out.append(None); continue
        tri = triangulate_line(R, t, tr, normalized_line_eq(cl[i], K), normalized_line_eq(cr[ri], K))
        out.append(None if tri is None else (_image_line(K, Rl, tl, *tri), _image_line(K, Rl, tlr, *tri)))
    return out


def lastkf_naive(P, cur, last, use_grid=True):
    """src/Tracking.cc:1474-1561.  Returns (match_last [n_cur], over [n_cur][2]): over[i] = (se > thr, se2 > thr) of the accepted
    match of line i - (False, False), (True, False) or (False, True), the reference rejects only (True, True)."""
    n_cur, n_last = cur["left_lines"].shape[0], last["left_lines"].shape[0]
    ll = last["left_lines"].astype(np.float64)
    llm = np.asarray(last["line_matches"], np.int64)
    lr = last["right_lines"].astype(np.float64)[np.maximum(llm, 0)] if last["right_lines"].shape[0] else np.zeros((n_last, 4))
    cells = line_cells(ll, P["sx"], P["sy"])
    thr = P["thr_reproj_base"] * 1.44 ** np.asarray(last["left_octave"], np.float64)
    ok_last = llm >= 0
    if last.get("skip") is not None:
        ok_last = ok_last & ~last["skip"].astype(bool)
    match = -np.ones(n_cur, np.int64); over = np.zeros((n_cur, 2), bool)
    for i, row in enumerate(lastkf_row_lines(P, cur)):
        if row is None or n_last == 0:
            continue
        lleft, lright = row
        g = ok_last & (_window_mask(lleft, cells, P["sx"], P["sy"]) if use_grid else True)
        a, b = _err_l1(ll, lleft) > thr, _err_l1(lr, lright) > thr
        cand = np.flatnonzero(g & ~(a & b))
        if not cand.size:
            continue
        cd = l2_rows(cur["desc"][i], last["desc"][cand])
        k = int(np.argmin(cd))
        if cd[k] >= 1e10 or cd[k] > P["md_thr"]:
            continue
        match[i] = cand[k]; over[i] = a[cand[k]], b[cand[k]]
    return match, over


def lastkf_created(P, cur, last, match):
    """The second half of MatchLinesLastKF (src/Tracking.cc:1563-1592) for the accepted matches: vgl::MultiTriangulateLine over the four
    views (numpy SVD and least squares), ReprojectKeyLineTo3D of the current left KeyLine, the depth test of both end points in all
    four views.  Returns created [n_cur] (1 where the reference constructs the MapLine)."""
    K = P["K"]; R, t = P["T_curr"][:3, :3], P["T_curr"][:3, 3]; Rl, tl = P["T_last"][:3, :3], P["T_last"][:3, 3]
    tr = t + R @ np.array([P["b"], 0, 0]); tlr = tl + Rl @ np.array([P["b"], 0, 0])
    Rs, ts = [R, R, Rl, Rl], [t, tr, tl, tlr]
    cl = cur["left_lines"].astype(np.float64); cr = cur["right_lines"].astype(np.float64)
    ll = last["left_lines"].astype(np.float64); lr = last["right_lines"].astype(np.float64)
    created = np.zeros(cl.shape[0], np.uint8)
    for i in np.flatnonzero(np.asarray(match) >= 0):
        li = int(match[i])
        leqs = [normalized_line_eq(cl[i], K), normalized_line_eq(cr[int(cur["line_matches"][i])], K),
                normalized_line_eq(ll[li], K), normalized_line_eq(lr[int(last["line_matches"][li])], K)]
        N = np.stack([Rv @ (l / np.linalg.norm(l)) for Rv, l in zip(Rs, leqs)])
        if any(abs(N[0] @ N[k]) / np.linalg.norm(N[0]) / np.linalg.norm(N[k]) > 0.975 for k in range(1, 4)):
            continue
        d = np.linalg.svd(N)[2][2]
        X0 = np.linalg.lstsq(N, np.array([N[k] @ ts[k] for k in range(4)]), rcond=None)[0]
        X0 = X0 - (X0 @ d) * d
        X0c, dc = R.T @ (X0 - t), R.T @ d
        front = True
        for e in (0, 2):
            M = np.stack([np.array([cl[i, e], cl[i, e + 1], 1.0]), -K @ dc], 1)
            p = X0 + np.linalg.lstsq(M, K @ X0c, rcond=None)[0][1] * d
            if any((Rv.T @ (p - tv))[2] < 0 for Rv, tv in zip(Rs, ts)):
                front = False
        created[i] = front
    return created
