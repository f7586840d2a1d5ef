"""Known-answer tests pinning oracle/lldo_orbsearch.cpp (the CPU restatement of the reference's guided ORB searches):
each C++ routine is checked against an independent, deliberately naive numpy/Python restatement of the same reference
lines at small sizes, plus hand-made cases for the tie / ordering / histogram rules.  No GPU."""
import numpy as np
import pytest

import oracle_orbsearch as OS
from lld_slam_amd import orb_search, synth
from lld_slam_amd.orb_search import Frame, orb_levels
from orbsearch_ref import popcount, py_features_in_area, py_grid, py_rot_bin, py_search_for_initialization, py_search_map, py_three_maxima

f32 = np.float32


# --------------------------------------------------------------------------------------------------------------------
def test_scale_tables_are_cumulative_float_products():
    s, s2, inv = orb_levels(1.2, 8)
    assert s.dtype == np.float32 and s[0] == 1.0 and s[1] == f32(1.2) and s[2] == f32(f32(1.2) * f32(1.2))
    assert np.array_equal(s2, s * s) and np.array_equal(inv, f32(1.0) / s2)


@pytest.mark.parametrize("seed", [0, 1])
def test_features_in_area_matches_the_naive_restatement(seed):
    F = synth.make_orb_frame(seed, 600)
    cells = py_grid(F)
    rng = np.random.default_rng(seed)
    for _ in range(300):
        x, y = rng.uniform(-40, F.max_x + 40), rng.uniform(-40, F.max_y + 40)
        r = float(rng.choice([2.5, 4.0, 7.0, 15.0, 40.0]) * F.scale[rng.integers(0, 8)])
        lv = int(rng.integers(0, 8)); mode = rng.integers(0, 4)
        mn, mx = [(-1, -1), (lv - 1, lv), (lv, -1), (0, lv)][mode]
        got = OS.features_in_area(F, x, y, r, mn, mx).tolist()
        assert got == py_features_in_area(F, cells, x, y, r, mn, mx)


def test_features_in_area_visits_columns_then_rows_then_insertion_order():
    # five keypoints: two share a cell (index order inside the cell), the others sit in cells visited later / earlier
    xy = np.array([[100, 100], [100.5, 100.2], [100, 120], [125, 90], [80, 130]], f32)
    F = Frame(desc=np.zeros((5, 8), np.uint32), xy=xy, octave=np.zeros(5, np.int32), uright=-np.ones(5, f32), angle=np.zeros(5, f32))
    got = OS.features_in_area(F, 100.0, 105.0, 60.0).tolist()
    cells = py_grid(F)
    order = sorted(range(5), key=lambda k: ([c for c, v in cells.items() if k in v][0], k))
    assert got == order and got.index(0) < got.index(1)
    # |dx| < r is strict: a keypoint exactly r away is not returned
    assert 3 not in OS.features_in_area(F, 100.0, 90.0, 25.0).tolist()
    assert 3 in OS.features_in_area(F, 100.0, 90.0, 25.001).tolist()


def test_three_maxima_known_answers():
    def run(c): return OS.three_maxima(np.array(c + [0] * (30 - len(c)), np.int32)).tolist()
    assert run([5, 9, 7, 1]) == [1, 2, 0]
    assert run([10, 10, 10, 10]) == [0, 1, 2]                 # strict '>' keeps the first of equal bins
    assert run([100, 9, 8]) == [0, -1, -1]                    # max2 < 0.1*max1 drops both
    assert run([100, 10, 9]) == [0, 1, -1]                    # 10 is not < 10.0; 9 is
    assert run([0] * 30) == [-1, -1, -1]
    rng = np.random.default_rng(3)
    for _ in range(200):
        c = rng.integers(0, 40, 30).tolist()
        assert run(c) == py_three_maxima(c)


@pytest.mark.parametrize("seed,th", [(0, 1.0), (1, 3.0)])
def test_search_by_projection_map_matches_the_naive_restatement(seed, th):
    F = synth.make_orb_frame(10 + seed, 500, n_clusters=30)
    q = synth.make_projection_queries(F, seed, 400, dup_frac=0.3)
    n, slot = OS.search_by_projection_map(F, q["desc"], q["valid"], q["uv"], q["ur"], q["level"], q["view_cos"], q["obs"], q["occupied"], th, 0.8)
    n_py, slot_py = py_search_map(F, q, th, 0.8)
    assert n == n_py and n > 50
    np.testing.assert_array_equal(slot, slot_py)


def test_search_by_projection_frame_rotation_filter_and_overwrites():
    """Frame-to-frame search: queries without observations do not block, so a later query can overwrite their keypoint,
    and the rotation filter NULLs every slot recorded in a dropped bin (src/ORBmatcher.cc:1425-1462)."""
    F = synth.make_orb_frame(20, 500, n_clusters=30)
    q = synth.make_projection_queries(F, 5, 450, dup_frac=0.4)
    q["obs"][::3] = 0
    n, slot = OS.search_by_projection_frame(F, q["desc"], q["valid"], q["uv"], q["ur"], q["level"], q["angle"], q["obs"], q["occupied"], 0, 7.0, True)
    n0, slot0 = OS.search_by_projection_frame(F, q["desc"], q["valid"], q["uv"], q["ur"], q["level"], q["angle"], q["obs"], q["occupied"], 0, 7.0, False)
    # reconstruct the filter from the unfiltered run: bins of every accepted (query -> keypoint) event
    cells = py_grid(F)
    events, sl, so = [], np.where(q["occupied"] != 0, 1 << 20, -1), q["occupied"].copy()
    for i in range(450):
        if not q["valid"][i]: continue
        o = int(q["level"][i]); rad = f32(f32(7.0) * F.scale[o]); best, bi = 256, -1
        for k in py_features_in_area(F, cells, q["uv"][i, 0], q["uv"][i, 1], rad, o - 1, o + 1):
            if sl[k] >= 0 and so[k]: continue
            if F.uright[k] > 0 and abs(f32(q["ur"][i] - F.uright[k])) > rad: continue
            d = popcount(q["desc"][i], F.desc[k])
            if d < best: best, bi = d, k
        if best <= 100:
            sl[bi] = i; so[bi] = q["obs"][i]; events.append((i, bi))
    assert len(events) == n0 and np.array_equal(sl, slot0)
    assert len({k for _, k in events}) < len(events)                     # the scene does contain overwrites
    bins = [py_rot_bin(q["angle"][i], F.angle[k]) for i, k in events]
    keep = py_three_maxima(np.bincount(bins, minlength=30).tolist())
    for (i, k), b in zip(events, bins):
        if b not in keep: sl[k] = -1
    assert n == len(events) - sum(b not in keep for b in bins)
    np.testing.assert_array_equal(slot, sl)
    assert 0 < n < n0


def test_bow_frame_search_is_order_dependent_and_ratio_tested():
    F1, F2, nd = synth.make_bow_pair(0, 600, n_nodes=120)
    valid = (np.random.default_rng(0).random(F1.n) < 0.9).astype(np.uint8)
    n, fm = OS.search_by_bow_frame(F1, F2, nd["n_nodes"], nd["start1"], nd["idx1"], nd["start2"], nd["idx2"], valid, 0.7, False)
    # naive restatement (src/ORBmatcher.cc:183-251)
    fm_py = -np.ones(F2.n, np.int64); n_py = 0
    for node in range(nd["n_nodes"]):
        for a in nd["idx1"][nd["start1"][node]:nd["start1"][node + 1]]:
            if not valid[a]: continue
            b1 = b2 = 256; bi = -1
            for b in nd["idx2"][nd["start2"][node]:nd["start2"][node + 1]]:
                if fm_py[b] >= 0: continue
                d = popcount(F1.desc[a], F2.desc[b])
                if d < b1: b2, b1, bi = b1, d, b
                elif d < b2: b2 = d
            if b1 <= 50 and f32(b1) < f32(f32(0.7) * f32(b2)):
                fm_py[bi] = a; n_py += 1
    assert n == n_py and n > 100
    np.testing.assert_array_equal(fm, fm_py)
    assert len(set(fm[fm >= 0].tolist())) == n                           # a KF keypoint is used once


def test_triangulation_prefers_the_last_of_equal_distances():
    """`dist>bestDist -> continue` (src/ORBmatcher.cc:733): with equal distances the LATER candidate replaces the earlier."""
    d = np.zeros((1, 8), np.uint32)
    t = np.zeros((3, 8), np.uint32); t[:, 1] = 1                         # all three at distance 1
    KF1 = Frame(desc=d, xy=np.array([[600, 180]], f32), octave=np.zeros(1, np.int32), uright=np.array([550], f32), angle=np.zeros(1, f32))
    KF2 = Frame(desc=t, xy=np.array([[500, 180], [520, 180], [540, 180]], f32), octave=np.zeros(3, np.int32), uright=np.array([450, 470, 490], f32),
                angle=np.zeros(3, f32))
    F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)               # pure x-translation: epipolar lines are the rows
    n, m12 = OS.search_for_triangulation(KF1, KF2, 1, [0, 1], [0], [0, 3], [0, 1, 2], [0], [0, 0, 0], F12, (1e6, 180.0), False, False)
    assert n == 1 and m12.tolist() == [2]
    # off the epipolar line by more than sqrt(3.84) px -> rejected
    KF2.xy[2, 1] = 183.0
    n, m12 = OS.search_for_triangulation(KF1, KF2, 1, [0, 1], [0], [0, 3], [0, 1, 2], [0], [0, 0, 0], F12, (1e6, 180.0), False, False)
    assert m12.tolist() == [1]


def test_stereo_search_row_band_and_thresholds():
    L, R = synth.make_stereo_pair(0, 500)
    br, bd = OS.stereo_search(L, R, 376, 0.0, 100.0)
    # naive restatement (src/Frame.cc:541-613)
    rows = [[] for _ in range(376)]
    for iR in range(R.n):
        r = f32(f32(2.0) * R.scale[R.octave[iR]])
        for yi in range(int(np.floor(f32(R.xy[iR, 1] - r))), int(np.ceil(f32(R.xy[iR, 1] + r))) + 1):
            if 0 <= yi < 376: rows[yi].append(iR)
    exp = -np.ones(L.n, np.int64)
    for iL in range(L.n):
        cand = rows[int(L.xy[iL, 1])]
        minU, maxU = f32(L.xy[iL, 0] - f32(100.0)), f32(L.xy[iL, 0] - f32(0.0))
        if not cand or maxU < 0: continue
        best, bi = 100, 0
        for iR in cand:
            if R.octave[iR] < L.octave[iL] - 1 or R.octave[iR] > L.octave[iL] + 1: continue
            if minU <= R.xy[iR, 0] <= maxU:
                d = popcount(L.desc[iL], R.desc[iR])
                if d < best: best, bi = d, iR
        if best < 75: exp[iL] = bi
    np.testing.assert_array_equal(br, exp)
    assert (br >= 0).sum() > 100


def test_is_in_frustum_matches_a_numpy_restatement():
    """Frame::isInFrustum (src/Frame.cc:333-389) + MapPoint::PredictScale: the C++ restatement against numpy with the same
    float32 / float64 mixture, and the rejection reasons all occur in the scene."""
    from lld_slam_amd import orb_search as S
    F = synth.make_orb_frame(3, 800)
    T, mp = synth.make_local_map(F, 3, 1500)
    view = S.frame_view(T, synth.KITTI_CAM, F)
    k, inv, uvr, lvl, vc = OS.is_in_frustum(view, mp)
    R = np.array(view.Rcw, f32).reshape(3, 3); t = np.array(view.tcw, f32); Ow = np.array(view.Ow, f32)
    reasons = {"skip": 0, "behind": 0, "image": 0, "dist": 0, "angle": 0, "ok": 0}
    for i in range(1500):
        P = mp["world_pos"][i]
        if mp["skip"][i]:
            reasons["skip"] += 1; assert not inv[i]; continue
        Pc = (R.astype(np.float64) @ P.astype(np.float64) + t.astype(np.float64)).astype(f32)      # not bit-identical to the k-ordered sum, see below
        Pc = np.array([f32(np.float64(R[r, 0]) * np.float64(P[0]) + np.float64(R[r, 1]) * np.float64(P[1]) + np.float64(R[r, 2]) * np.float64(P[2])
                           + np.float64(t[r])) for r in range(3)], f32)
        if Pc[2] < 0: reasons["behind"] += 1; assert not inv[i]; continue
        invz = f32(1.0) / Pc[2]
        u = f32(f32(f32(view.fx) * Pc[0]) * invz) + f32(view.cx); v = f32(f32(f32(view.fy) * Pc[1]) * invz) + f32(view.cy)
        if u < view.min_x or u > view.max_x or v < view.min_y or v > view.max_y: reasons["image"] += 1; assert not inv[i]; continue
        PO = (P - Ow).astype(f32)
        dist = f32(np.sqrt(np.sum(PO.astype(np.float64) ** 2)))
        if dist < f32(0.8) * mp["min_distance"][i] or dist > f32(1.2) * mp["max_distance"][i]: reasons["dist"] += 1; assert not inv[i]; continue
        vcos = f32(np.float64(PO[0]) * np.float64(mp["normal"][i, 0]) + np.float64(PO[1]) * np.float64(mp["normal"][i, 1])
                   + np.float64(PO[2]) * np.float64(mp["normal"][i, 2])) if False else f32((PO.astype(np.float64) @ mp["normal"][i].astype(np.float64)) / np.float64(dist))
        if vcos < 0.5: reasons["angle"] += 1; assert not inv[i]; continue
        reasons["ok"] += 1
        assert inv[i]
        assert uvr[i, 0] == u and uvr[i, 1] == v and uvr[i, 2] == f32(u - f32(f32(view.bf) * invz))
        assert abs(float(vc[i]) - float(vcos)) <= 1.2e-7 * abs(float(vcos))          # numpy's dot may associate differently: one float ulp
        q = np.log(f32(mp["max_distance"][i] / dist)) / f32(view.log_scale_factor)
        if abs(q - round(float(q))) > 1e-4:
            assert lvl[i] == min(max(int(np.ceil(q)), 0), 7)
    assert k == reasons["ok"] and all(c > 20 for c in reasons.values()), reasons


# ---------------------------------------------------------------------- Frame::ComputeStereoMatches, whole routine (with images)
def _numpy_refine(sc, iL, iR):
    """Independent numpy statement of the SAD refinement of one pair (src/Frame.cc:615-688): (sad, uR) or None."""
    L, R = sc["L"], sc["R"]
    o = int(L.octave[iL]); sf = sc["inv_scale"][o]
    f32 = np.float32
    su = int(np.round(f32(L.xy[iL, 0] * sf))); sv = int(np.round(f32(L.xy[iL, 1] * sf))); sr = int(np.round(f32(R.xy[iR, 0] * sf)))
    imL, imR = sc["left"][o].astype(np.int64), sc["right"][o].astype(np.int64)
    h, w = imL.shape
    if sr < 0 or sr + 11 >= w or su - 5 < 0 or su + 5 >= w or sv - 5 < 0 or sv + 5 >= h or sr - 10 < 0 or sr + 10 >= w:
        return None
    pl = imL[sv - 5:sv + 6, su - 5:su + 6] - imL[sv, su]
    d = np.array([np.abs(pl - (imR[sv - 5:sv + 6, sr + k - 5:sr + k + 6] - imR[sv, sr + k])).sum() for k in range(-5, 6)])
    b = int(np.argmin(d))                                      # first minimum
    if b == 0 or b == 10:
        return None
    d1, d2, d3 = f32(d[b - 1]), f32(d[b]), f32(d[b + 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = (d1 - d3) / (f32(2.0) * (d1 + d3 - f32(2.0) * d2))
    if delta < -1 or delta > 1:
        return None
    return int(d[b]), f32(L.scale[o] * (f32(sr) + f32(b - 5) + delta))


def test_compute_stereo_matches_whole_routine():
    sc = synth.make_stereo_scene(0, 1200)
    L, R = sc["L"], sc["R"]
    n, ur, dep, br, sad = OS.compute_stereo_matches(L, R, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    # stage 1 equals the Hamming-only restatement
    br0, _ = OS.stereo_search(L, R, sc["left"][0].shape[0], 0.0, float(np.float32(sc["mbf"]) / np.float32(sc["mb"])))
    np.testing.assert_array_equal(br, br0)
    assert (br >= 0).sum() > 700 and (sad >= 0).sum() > 600 and 0 < n < (sad >= 0).sum()
    # stage 2 against an independent numpy statement
    for iL in np.nonzero(br >= 0)[0][:300]:
        ref = _numpy_refine(sc, iL, br[iL])
        if ref is None:
            assert sad[iL] == -1
            continue
        s_ref, u_ref = ref
        disparity = np.float32(L.xy[iL, 0] - u_ref)
        if not (disparity >= 0 and disparity < np.float32(sc["mbf"]) / np.float32(sc["mb"])):
            assert sad[iL] == -1
            continue
        assert sad[iL] == s_ref
        if ur[iL] >= 0 and disparity > 0:
            assert ur[iL] == u_ref and dep[iL] == np.float32(np.float32(sc["mbf"]) / disparity)
    # stage 3: median of the pushed distances, everything at or above 1.5f*1.4f*median is cleared
    pushed = np.sort(sad[sad >= 0])
    th = np.float32(np.float32(1.5) * np.float32(1.4)) * np.float32(pushed[len(pushed) // 2])
    keep = (sad >= 0) & (sad.astype(np.float32) < th)
    np.testing.assert_array_equal(ur >= 0, keep)
    np.testing.assert_array_equal(dep >= 0, keep)
    assert n == keep.sum()
    # and the answer is the scene's disparity
    true = np.full(L.n, np.nan); true[sc["src"]] = sc["d_true"]
    err = np.abs((L.xy[keep, 0] - ur[keep]) - true[keep])
    assert np.nanmedian(err) < 1.5


def test_compute_stereo_matches_degenerate_inputs():
    sc = synth.make_stereo_scene(1, 300)
    L, R = sc["L"], sc["R"]
    # keypoints pushed against the image border: the patches leave the image, no stereo match (and no crash)
    L.xy[:40, 0] = 2.0; R.xy[:40, 0] = 1.0
    n, ur, dep, br, sad = OS.compute_stereo_matches(L, R, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    assert (ur[:40] < 0).all()
    # no right keypoints at all
    from lld_slam_amd.orb_search import Frame
    E = Frame(desc=np.zeros((0, 8), np.uint32), xy=np.zeros((0, 2), np.float32), octave=np.zeros(0, np.int32), uright=np.zeros(0, np.float32),
              angle=np.zeros(0, np.float32))
    n, ur, dep, br, sad = OS.compute_stereo_matches(L, E, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    assert n == 0 and (ur < 0).all() and (br < 0).all()


@pytest.mark.parametrize("pid,window,nn,ori", [(0, 30, 0.9, True), (1, 100, 0.9, True), (2, 60, 0.7, False)])
def test_search_for_initialization_matches_the_naive_restatement(pid, window, nn, ori):
    F1, F2, prev = synth.make_init_pair(pid, n=500)
    n, m, pm = OS.search_for_initialization(F1, F2, prev, window, nn, ori)
    pn, pm12, pprev, steals = py_search_for_initialization(F1, F2, prev, window, nn, ori)
    assert n == pn and n > 80
    np.testing.assert_array_equal(m, pm12); np.testing.assert_array_equal(pm, pprev)
    assert steals > 0                                                        # the scene does exercise the take-over rule


def test_search_for_initialization_takes_a_keypoint_from_a_worse_holder():
    """Three level-0 queries on one keypoint of F2: distances 6, 3 (takes over), 3 (an equal distance does not), a level-1 query is
    skipped, the stale histogram entry of the displaced query still counts."""
    scale, sigma2, inv = orb_levels()
    d0 = np.zeros(8, np.uint32)
    def desc(bits):
        d = d0.copy(); d[0] = (1 << bits) - 1; return d
    F2 = Frame(desc=np.stack([d0, np.full(8, 0xffffffff, np.uint32)]), xy=np.array([[100, 100], [400, 200]], f32), octave=np.zeros(2, np.int32), uright=-np.ones(2, f32),
               angle=np.array([10, 10], f32), min_x=0.0, min_y=0.0, max_x=1241.0, max_y=376.0).normalise()
    F1 = Frame(desc=np.stack([desc(6), desc(3), desc(3) ^ np.array([0, 1, 0, 0, 0, 0, 0, 0], np.uint32) ^ np.array([1, 0, 0, 0, 0, 0, 0, 0], np.uint32), desc(1)]),
               xy=np.array([[101, 100], [99, 101], [100, 99], [100, 100]], f32), octave=np.array([0, 0, 0, 1], np.int32), uright=-np.ones(4, f32),
               angle=np.array([200, 12, 12, 12], f32), min_x=0.0, min_y=0.0, max_x=1241.0, max_y=376.0).normalise()
    n, m, pm = OS.search_for_initialization(F1, F2, F1.xy.copy(), 10, 0.9, True)
    assert popcount(F1.desc[2], F2.desc[0]) == 3
    assert n == 1 and m.tolist() == [-1, 0, -1, -1]
    np.testing.assert_array_equal(pm[1], F2.xy[0]); np.testing.assert_array_equal(pm[0], F1.xy[0])


@pytest.mark.parametrize("seed", [0, 1])
def test_projection_loops_of_the_sim3_and_relocalisation_matchers(seed):
    """lldo_project_general against the restatements it overlaps with and a numpy restatement of what differs:
    routine 0 / 2 (SearchByProjection(KF, Scw) :311-358, Fuse(KF, Scw) :1000-1048) are Fuse(KF, vpMapPoints)'s loop (:841-890) without
    the stereo coordinate - `1/z` in float and float(1.0/z) are the same number (double rounding of a quotient is innocuous at
    53 >= 2*24+2 bits); routine 3 with the identity as second transform drops the viewing-angle test and takes the distance
    from the camera-frame point; routine 1 has no depth test, inclusive bounds and `fx*xc*invzc+cx`."""
    F = synth.make_orb_frame(500 + seed, 1500)
    T, mp = synth.make_local_map(F, 500 + seed, 2000)
    view = orb_search.frame_view(T, synth.KITTI_CAM, F)
    vf, uvf, urf, lf = OS.project_fuse(view, mp)
    for routine in (0, 2):
        v, uv, lvl = OS.project_general(view, mp, routine)
        np.testing.assert_array_equal(v, vf)
        np.testing.assert_array_equal(uv[v != 0], uvf[v != 0]); np.testing.assert_array_equal(lvl[v != 0], lf[v != 0])
    # numpy restatement of the shared head
    R = np.array(view.Rcw, np.float32).reshape(3, 3).astype(np.float64); t = np.array(view.tcw, np.float32).astype(np.float64)
    Ow = np.array(view.Ow, np.float32)
    P = mp["world_pos"].astype(np.float32)
    Pc = (P.astype(np.float64) @ R.T + t).astype(np.float32)
    f32 = np.float32
    fx, fy, cx, cy = f32(view.fx), f32(view.fy), f32(view.cx), f32(view.cy)
    skip = mp["skip"] != 0
    maxD = f32(1.2) * mp["max_distance"]; minD = f32(0.8) * mp["min_distance"]
    with np.errstate(all="ignore"):
        # routine 1
        invz = (1.0 / Pc[:, 2].astype(np.float64)).astype(np.float32)
        u = fx * Pc[:, 0] * invz + cx; v_ = fy * Pc[:, 1] * invz + cy
        inb = ~((u < f32(view.min_x)) | (u > f32(view.max_x)) | (v_ < f32(view.min_y)) | (v_ > f32(view.max_y)))
        PO = P - Ow
        dist = np.sqrt((PO.astype(np.float64) ** 2).sum(1)).astype(np.float32)
        band = ~((dist < minD) | (dist > maxD))
        exp1 = ~skip & inb & band
        v1, uv1, l1 = OS.project_general(view, mp, 1)
        np.testing.assert_array_equal(v1 != 0, exp1)
        np.testing.assert_array_equal(uv1[exp1], np.stack([u, v_], 1)[exp1])
        ratio = mp["max_distance"] / dist
        lv = np.clip(np.ceil(np.log(ratio) / f32(view.log_scale_factor)), 0, view.n_levels - 1).astype(np.int32)
        np.testing.assert_array_equal(l1[exp1], lv[exp1])
        assert (exp1 & (Pc[:, 2] < 0)).sum() >= 0 and 500 < exp1.sum() < 1900
        # routine 3, identity second transform
        x = Pc[:, 0] * invz; y = Pc[:, 1] * invz
        u3 = fx * x + cx; v3 = fy * y + cy
        inimg = (u3 >= f32(view.min_x)) & (u3 < f32(view.max_x)) & (v3 >= f32(view.min_y)) & (v3 < f32(view.max_y))
        d3 = np.sqrt((Pc.astype(np.float64) ** 2).sum(1)).astype(np.float32)
        exp3 = ~skip & ~(Pc[:, 2] < 0) & inimg & ~((d3 < minD) | (d3 > maxD))
        v3o, uv3, l3 = OS.project_general(view, mp, 3, np.eye(3), np.zeros(3))
        np.testing.assert_array_equal(v3o != 0, exp3)
        np.testing.assert_array_equal(uv3[exp3], np.stack([u3, v3], 1)[exp3])
        assert (exp3 & (vf == 0)).sum() > 20                                 # points the 60-degree test of Fuse rejects
    # routine 3 with a real second transform: the composition equals one transform by the product up to float rounding
    sR = (0.9 * synth._rodrigues(np.array([0.02, -0.01, 0.03]))).astype(np.float32); t2 = np.array([0.1, -0.05, 0.2], np.float32)
    v3b, uv3b, _ = OS.project_general(view, mp, 3, sR, t2)
    Pc2 = (Pc.astype(np.float64) @ sR.astype(np.float64).T + t2.astype(np.float64)).astype(np.float32)
    with np.errstate(all="ignore"):
        iz = (1.0 / Pc2[:, 2].astype(np.float64)).astype(np.float32)
        ub = fx * (Pc2[:, 0] * iz) + cx
    k = v3b != 0
    assert k.sum() > 300
    np.testing.assert_array_equal(uv3b[k, 0], ub[k])


def test_device_logf_restatement_equals_the_platform_libm():
    """The device cannot call the host's libm, and MapPoint::PredictScale's ceil(log(ratio) / logScaleFactor) moves by a level when logf is an
    ulp off at a boundary: the device carries glibc's logf algorithm (lld_orb_search.hip glibc_logf).  oracle/lldo_orbsearch.cpp holds the
    same restatement; here it must equal std::log(float) of THIS host bit for bit - 20 M random floats and 8193 neighbours of every 1.2^k."""
    bad, first = OS.glibc_logf_differences(20_000_000, 7)
    assert bad == 0, first
