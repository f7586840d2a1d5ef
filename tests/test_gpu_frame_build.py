"""lld_frame_build_stereo / lld_frame_build_stereo_keypoints / lld_frame_stereo_download: the stereo Frame built on the device, against
the oracle's Frame::ComputeStereoMatches (oracle_orbsearch.compute_stereo_matches), the existing device route
(compute_stereo_matches_device) and, for "the frame is a frame", lld_frame_create on the downloaded arrays.  Everything bit for bit."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import orb_extract_ref as R
import oracle_orbsearch as OS
from lld_slam_amd import Context, abi, orb_search, synth
from lld_slam_amd.orb_extractor import ORBextractor, compute_stereo_matches_device
from lld_slam_amd.orb_search import Frame
from lld_slam_amd.tracking import DeviceTrackedFrame

pytestmark = pytest.mark.gpu

SMALL = (500, 1.2, 8, 12, 7)
KITTI = (2000, 1.2, 8, 12, 7)
PATTERN = R.seeded_pattern(7)
W, H = 416, 240                       # the smallest size at which all eight levels stay >= 62 px
FIELDS = ("u_right", "depth", "best_r", "sad")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, exp, what=""):
    """got: StereoMatches; exp: StereoMatches or the oracle's (n, ur, dep, br, sad)."""
    if isinstance(exp, tuple):
        exp = orb_search.StereoMatches(exp[1], exp[2], exp[3], exp[4], exp[0])
    assert got.n_matches == exp.n_matches, f"{what} n_matches {got.n_matches} vs {exp.n_matches}"
    for f in FIELDS:
        g, e = bits(getattr(got, f)), bits(getattr(exp, f))
        assert np.array_equal(g, e), f"{what} {f} differs at {np.nonzero(g != e)[0][:8]}"


def ref_frame(e, T, w, h):
    return Frame(desc=e["desc"], xy=e["xy"], octave=e["octave"], uright=np.full(len(e["octave"]), -1, np.float32), angle=e["angle"],
                 max_x=float(w), max_y=float(h), scale=T["scale"], sigma2=T["sigma2"], inv_sigma2=T["inv_sigma2"]).normalise()


@pytest.fixture(scope="module")
def small():
    """Per pair id: the scene, the CPU extraction of both images and the oracle's ComputeStereoMatches on it.  Computed once, never changed."""
    T = R.level_tables(*SMALL[:3])
    out = {}
    for pid in (0, 1):
        sc = synth.make_stereo_scene(pid, width=W, height=H)
        el, er = R.extract(sc["left"][0], *SMALL, PATTERN), R.extract(sc["right"][0], *SMALL, PATTERN)
        L, Rf = ref_frame(el, T, W, H), ref_frame(er, T, W, H)
        exp = OS.compute_stereo_matches(L, Rf, el["levels"], er["levels"], T["inv_scale"], sc["mb"], sc["mbf"])
        out[pid] = dict(sc=sc, el=el, er=er, L=L, R=Rf, exp=exp, T=T)
    return out


@pytest.fixture(scope="module")
def small_ex(gpu_ctx):
    with ORBextractor(gpu_ctx, *SMALL, PATTERN, max_cols=W, max_rows=H, max_images=2) as ex:
        yield ex


def test_oracle_figures(small):
    """What the two small pairs exercise, from the CPU alone: every octave, > 200 matches, and a median cut that removes some."""
    for pid, n_kept, n_cut in ((0, 226, 3), (1, 203, 6)):
        s = small[pid]
        assert (s["L"].n, s["R"].n) == (511, 511) and np.all(np.bincount(s["L"].octave, minlength=8) > 0)
        n, ur, dep, br, sad = s["exp"]
        assert n == n_kept and int((sad >= 0).sum()) - n == n_cut and int((ur >= 0).sum()) == n


@pytest.mark.parametrize("pid", [0, 1])
def test_extractor_route_small(gpu_ctx, small, small_ex, pid):
    s = small[pid]; sc = s["sc"]
    L, Rf = small_ex([sc["left"][0], sc["right"][0]])
    assert np.array_equal(L.xy, s["L"].xy) and np.array_equal(Rf.desc, s["R"].desc)
    built = small_ex.build_stereo_frame(L, sc["mb"], sc["mbf"])
    try:
        got = built.download()
    finally:
        built.close()
    dev = compute_stereo_matches_device(gpu_ctx, L, Rf, small_ex, sc["mb"], sc["mbf"])
    assert got.n_matches > 100
    assert_same(got, s["exp"], "oracle"); assert_same(got, dev, "lld_compute_stereo_matches")


def _download(ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, C.cast(ptr, C.c_void_p), nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def test_extractor_route_kitti(gpu_ctx):
    sc = synth.make_stereo_scene(0)
    with ORBextractor(gpu_ctx, *KITTI, PATTERN, max_cols=1241, max_rows=376, max_images=2) as ex:
        L, Rf = ex([sc["left"][0], sc["right"][0]])
        built = ex.build_stereo_frame(L, sc["mb"], sc["mbf"])
        try:
            got = built.download()
        finally:
            built.close()
        dev = compute_stereo_matches_device(gpu_ctx, L, Rf, ex, sc["mb"], sc["mbf"])
        # the oracle reads the pyramids the extractor built (held to the CPU restatement, level by level, by test_gpu_orb_extract.py)
        levels = []
        for im in (0, 1):
            lv, cols, rows, step = ex.pyramid(im)
            levels.append([_download(lv[l], int(rows[l]) * int(step[l])).reshape(rows[l], step[l]) for l in range(8)])
        inv = ex.inv_scale_factors.copy()
    exp = OS.compute_stereo_matches(L, Rf, levels[0], levels[1], inv, sc["mb"], sc["mbf"])
    assert L.n > 1500 and got.n_matches > 100
    assert_same(got, exp, "oracle"); assert_same(got, dev, "lld_compute_stereo_matches")


# ---------------------------------------------------------------------------------------------- keypoint route, crafted
@pytest.fixture(scope="module")
def crafted():
    sc = synth.make_stereo_scene(2, n=300, width=W, height=H)
    exp = OS.compute_stereo_matches(sc["L"], sc["R"], sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    return dict(sc=sc, exp=exp)


def sub(F, idx):
    return dataclasses.replace(F, desc=F.desc[idx].copy(), xy=F.xy[idx].copy(), octave=F.octave[idx].copy(), uright=F.uright[idx].copy(),
                               angle=F.angle[idx].copy()).normalise()


def run_keypoints(ctx, sc, L, Rf, device=None):
    built = orb_search.build_stereo_frame_keypoints(ctx.lib, ctx.handle, L, Rf, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"], device=device)
    try:
        return built.download()
    finally:
        built.close()


def check_keypoints(ctx, sc, L, Rf, what):
    exp = OS.compute_stereo_matches(L, Rf, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    got = run_keypoints(ctx, sc, L, Rf)
    assert_same(got, exp, what)
    return got, exp


def test_keypoints_as_is(gpu_ctx, crafted):
    sc = crafted["sc"]
    got = run_keypoints(gpu_ctx, sc, sc["L"], sc["R"])
    assert got.n_matches > 100 and sc["L"].n == 300 and sc["L"].scale.shape[0] == 8
    assert_same(got, crafted["exp"], "scene")


def test_keypoints_tie_rule(gpu_ctx, crafted):
    sc = crafted["sc"]; L, Rf = sc["L"], sc["R"]
    br = crafted["exp"][3]
    iL = int(np.nonzero(br >= 0)[0][7]); j = int(br[iL])
    n = Rf.n
    # the duplicate at a higher index: the first candidate in ascending iR keeps the match
    hi = sub(Rf, np.r_[np.arange(n), j])
    got, _ = check_keypoints(gpu_ctx, sc, L, hi, "duplicate above")
    assert got.best_r[iL] == j and np.array_equal(got.best_r, br)
    # the duplicate at index 0: it takes over (every other index moves up by one)
    lo = sub(Rf, np.r_[j, np.arange(n)])
    got, _ = check_keypoints(gpu_ctx, sc, L, lo, "duplicate below")
    assert got.best_r[iL] == 0


def _flip(desc, k):
    d = desc.copy()
    for b in range(k):
        d[b >> 5] ^= np.uint32(1) << np.uint32(b & 31)
    return d


def test_keypoints_threshold_74_75(gpu_ctx, crafted):
    sc = crafted["sc"]; L = sc["L"]
    br = crafted["exp"][3]
    iL = int(np.nonzero(br >= 0)[0][11]); j = int(br[iL])
    for k, accepted in ((74, True), (75, False)):
        Rf = sub(sc["R"], np.arange(sc["R"].n))
        # every other candidate of iL is pushed out of its disparity range, so the crafted one decides alone
        band = np.abs(Rf.xy[:, 1] - L.xy[iL, 1]) < 20
        band[j] = False
        Rf.xy[band, 0] = L.xy[iL, 0] + 50.0
        Rf.desc[j] = _flip(L.desc[iL], k)
        got, exp = check_keypoints(gpu_ctx, sc, L, Rf, f"distance {k}")
        assert (exp[3][iL] == j) == accepted and (got.best_r[iL] == j) == accepted


def test_keypoints_left_of_image_and_row_bands(gpu_ctx, crafted):
    sc = crafted["sc"]
    L, Rf = sub(sc["L"], np.arange(300)), sub(sc["R"], np.arange(sc["R"].n))
    br = crafted["exp"][3]
    m = np.nonzero(br >= 0)[0]
    L.xy[m[:3], 0] = np.float32([-0.5, -3.0, -1e-3])                          # uL - minD < 0: skipped
    Rf.xy[br[m[3:9]], 1] = np.float32([0.25, -1.5, 1.0, H - 0.5, H + 1.5, H - 1.0])   # bands that reach above row 0 and below the last row
    got, exp = check_keypoints(gpu_ctx, sc, L, Rf, "edges")
    assert np.all(got.best_r[m[:3]] == -1) and got.n_matches > 50


def test_keypoints_empty_sides(gpu_ctx, crafted):
    sc = crafted["sc"]; L, Rf = sc["L"], sc["R"]
    none = np.zeros(0, np.int64)
    got, _ = check_keypoints(gpu_ctx, sc, L, sub(Rf, none), "n_right = 0")
    assert got.n_matches == 0 and np.all(got.best_r == -1) and np.all(got.u_right == -1)
    iL = int(np.nonzero(crafted["exp"][1] >= 0)[0][0])
    got, _ = check_keypoints(gpu_ctx, sc, sub(L, np.array([iL])), Rf, "n_left = 1")
    assert got.n_matches == 1 and bits(got.u_right)[0] == bits(crafted["exp"][1])[iL]
    got = run_keypoints(gpu_ctx, sc, sub(L, none), Rf)                         # Frame.cc:108: an empty frame, not an error
    assert got.n_matches == 0 and got.u_right.shape == (0,)


def test_keypoints_device_pointers(gpu_ctx, crafted):
    import torch
    sc = crafted["sc"]; L, Rf = sc["L"], sc["R"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()
    t = dict(lxy=up(L.xy), ldesc=up(L.desc), langle=up(L.angle), rxy=up(Rf.xy), roct=up(Rf.octave), rdesc=up(Rf.desc))
    torch.cuda.synchronize()
    got = run_keypoints(gpu_ctx, sc, L, Rf, device={k: v.data_ptr() for k, v in t.items()})
    assert_same(got, crafted["exp"], "device pointers")
    assert_same(got, run_keypoints(gpu_ctx, sc, L, Rf), "host pointers")


# ---------------------------------------------------------------------------------------------- the frame is a frame
def _queries(L, ur, depth, cam, rng):
    """MapPoints un-projected from the frame's own stereo keypoints (camera at the origin), descriptors with a few flipped bits."""
    fx, fy, cx, cy, bf = [np.float32(c) for c in cam]
    idx = np.nonzero(depth > 0)[0]
    z = depth[idx].astype(np.float32)
    P = np.stack([(L.xy[idx, 0] - cx) * z / fx, (L.xy[idx, 1] - cy) * z / fy, z], 1).astype(np.float32)
    desc = L.desc[idx].copy()
    for r in range(len(idx)):
        for b in rng.integers(0, 256, 6):
            desc[r, b >> 5] ^= np.uint32(1) << np.uint32(b & 31)
    dist = np.linalg.norm(P, axis=1).astype(np.float32)
    maxd = (dist * L.scale[L.octave[idx]]).astype(np.float32)
    last = dict(world_pos=P, valid=np.ones(len(idx), np.uint8), octave=L.octave[idx].copy(), angle=L.angle[idx].copy(), desc=desc,
                has_obs=np.ones(len(idx), np.uint8))
    mp = dict(world_pos=P, normal=(P / dist[:, None]).astype(np.float32), max_distance=maxd, min_distance=(maxd / L.scale[-1]).astype(np.float32),
              desc=desc, has_obs=np.ones(len(idx), np.uint8), skip=np.zeros(len(idx), np.uint8))
    return last, mp, np.arange(len(idx), dtype=np.int32)


def test_built_frame_is_a_frame(gpu_ctx, small, small_ex):
    s = small[0]; sc = s["sc"]
    fx = float(np.float32(sc["mbf"]) / np.float32(sc["mb"]))
    cam = (fx, fx, W / 2.0, H / 2.0, float(sc["mbf"]))
    L, _ = small_ex([sc["left"][0], sc["right"][0]])
    built = small_ex.build_stereo_frame(L, sc["mb"], sc["mbf"])
    st = built.download()
    F2 = dataclasses.replace(L, uright=st.u_right.copy()).normalise()             # what the host would hand lld_frame_create
    last, mp, ids = _queries(L, st.u_right, st.depth, cam, np.random.default_rng(5))
    assert len(ids) > 100
    T = np.eye(4, dtype=np.float32); T[:3, 3] = [0.03, -0.01, 0.02]
    view = orb_search.frame_view(T, cam, F2)
    with orb_search.ResidentFrame(gpu_ctx.lib, gpu_ctx.handle, F2) as plain:
        for name, args in (("search_last_frame", (view, last)), ("search_local_points", (view, mp))):
            a, xa = getattr(built, name)(*args); b, xb = getattr(plain, name)(*args)
            assert a.n_matches == b.n_matches and a.n_matches > 50 and a.rounds == b.rounds, name
            for f in ("match", "best_dist", "second_dist", "removed", "owner"):
                assert np.array_equal(getattr(a, f), getattr(b, f)), f"{name}.{f}"
            if isinstance(xa, dict):
                assert np.array_equal(xa["in_view"], xb["in_view"])
                v = xa["in_view"] != 0
                for f in ("proj_uvr", "level", "view_cos"):
                    assert np.array_equal(bits(xa[f][v]), bits(xb[f][v])), f"{name}.{f}"
            else:
                assert np.array_equal(bits(xa), bits(xb)), name
    recs = []
    for tf in (DeviceTrackedFrame.from_stereo_build(gpu_ctx, built, cam), DeviceTrackedFrame(gpu_ctx, F2, cam)):
        with tf:
            tf.track_with_motion_model(T, last, ids)
            tf.track_local_map(mp, ids)
            recs.append(tf.download())
    for a, b in zip(*recs):
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], np.ndarray):
                g, e = a[k], b[k]
                assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, e.view(np.uint64) if e.dtype == np.float64 else e), k
            else:
                assert np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64), k
    assert recs[0][0]["n_search"] > 50 and recs[0][1]["n_inliers"] > 20


# ---------------------------------------------------------------------------------------------- ownership
def test_frame_survives_next_extract_and_the_extractor(gpu_ctx, small):
    s0, s1 = small[0], small[1]
    ex = ORBextractor(gpu_ctx, *SMALL, PATTERN, max_cols=W, max_rows=H, max_images=2)
    try:
        L, _ = ex([s0["sc"]["left"][0], s0["sc"]["right"][0]])
        built = ex.build_stereo_frame(L, s0["sc"]["mb"], s0["sc"]["mbf"])
        L1, _ = ex([s1["sc"]["left"][0], s1["sc"]["right"][0]])                   # overwrites the extractor's keypoints and pyramids
        assert not np.array_equal(L1.xy, L.xy)
        assert_same(built.download(), s0["exp"], "after the next extract")
        second = ex.build_stereo_frame(L1, s1["sc"]["mb"], s1["sc"]["mbf"])
    finally:
        ex.close()                                                                # the extractor goes first
    assert_same(second.download(), s1["exp"], "after the extractor")
    assert_same(built.download(), s0["exp"], "first frame, again")
    second.close(); built.close()


# ---------------------------------------------------------------------------------------------- arguments
def test_refusals(gpu_ctx, crafted, small):
    lib, ctx = gpu_ctx.lib, gpu_ctx.handle
    sc = crafted["sc"]; L, Rf = sc["L"], sc["R"]
    INV, UNS = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED

    def call(L=L, Rf=Rf, drop=None, **kw):
        kl, kr = orb_search.keypoints_struct(L), orb_search.keypoints_struct(Rf)
        P, keep = orb_search.pyramids_struct(sc["left"], sc["right"], L.scale, sc["inv_scale"])
        prm, keep2 = orb_search.frame_stereo_params(L, sc["mb"], sc["mbf"])
        for k, v in kw.items():
            setattr(P if k == "pyr_levels" else prm, "n_levels" if k == "pyr_levels" else k, v)
        a = dict(ctx=ctx, kl=kl, kr=kr, pyr=P, params=prm)
        if drop: a[drop] = None
        st, h = orb_search.build_stereo_frame_raw(lib, a["ctx"], a["kl"], a["kr"], a["pyr"], a["params"])
        if st == abi.LLD_OK:
            orb_search.StereoBuiltFrame(lib, ctx, L, h).close()
        else:
            assert not h.value
        return st

    for drop in ("ctx", "kl", "kr", "pyr", "params"):
        assert call(drop=drop) == INV, drop
    fn = lib.fn("frame_build_stereo_keypoints")
    assert fn(ctx, None, None, None, None, None) == INV                          # no place for the handle
    assert call(left_angle=None) == INV
    for nl in (0, -1, 17, 7):
        assert call(n_levels=nl) == INV, nl                                       # out of range, or not the pyramid's
    assert call(n_levels=17, pyr_levels=17) == INV
    for mb in (0.0, -0.5, float("nan")):
        assert call(mb=mb) == INV, mb
    for who, o in (("L", 8), ("L", -1), ("R", 8), ("R", -2)):
        F = sub(L if who == "L" else Rf, np.arange((L if who == "L" else Rf).n)); F.octave[5] = o
        assert call(**{"L" if who == "L" else "Rf": F}) == INV, (who, o)
    big = np.arange(orb_search.MAX_KEYPOINTS + 1) % 300
    assert call(L=sub(L, big)) == UNS and call(Rf=sub(Rf, big % Rf.n)) == UNS
    assert call(L=sub(L, big[:-1])) == abi.LLD_OK                                 # exactly LLD_ORB_MAX_KEYPOINTS is served
    assert call() == abi.LLD_OK                                                   # after the refusals, a valid call succeeds

    s = small[0]["sc"]
    with ORBextractor(gpu_ctx, *SMALL, PATTERN, max_cols=W, max_rows=H, max_images=2) as ex:
        prm, keep = orb_search.frame_stereo_params(small[0]["L"], s["mb"], s["mbf"])
        assert ex.build_stereo_frame_raw(0, 1, prm)[0] == INV                     # no successful extract yet
        Lx = ex(s["left"][0])                                                     # one image
        assert ex.build_stereo_frame_raw(0, 1, prm)[0] == INV                     # index outside the last call's n_images
        ex([s["left"][0], s["right"][0]])
        for li, ri in ((0, 2), (2, 1), (-1, 1), (0, -1), (0, 0), (1, 1)):
            assert ex.build_stereo_frame_raw(li, ri, prm)[0] == INV, (li, ri)
        assert ex.build_stereo_frame_raw(0, 1, None)[0] == INV
        bad, _ = orb_search.frame_stereo_params(small[0]["L"], 0.0, s["mbf"])
        assert ex.build_stereo_frame_raw(0, 1, bad)[0] == INV
        fb = lib.fn("frame_build_stereo")
        assert fb(None, 0, 1, C.byref(prm), C.byref(C.c_void_p())) == INV and fb(ex.handle, 0, 1, C.byref(prm), None) == INV
        built = ex.build_stereo_frame(small[0]["L"], s["mb"], s["mbf"])           # and then the valid call
        # a frame and a context that do not belong together
        other = Context(0)
        try:
            with pytest.raises(ValueError):
                DeviceTrackedFrame.from_stereo_build(other, built, (700.0, 700.0, W / 2.0, H / 2.0, float(s["mbf"])))
        finally:
            other.close()
        assert_same(built.download(), small[0]["exp"], "after the refusals")
        built.close()

    # lld_frame_stereo_download on a frame lld_frame_create made
    dl = lib.fn("frame_stereo_download"); dl.argtypes = [C.c_void_p, C.POINTER(orb_search.StereoResult)]; dl.restype = C.c_int
    with orb_search.ResidentFrame(lib, ctx, L) as plain:
        out = np.empty(L.n, np.float32); r = orb_search.StereoResult()
        r.u_right = out.ctypes.data_as(abi.c_float_p); r.depth = out.ctypes.data_as(abi.c_float_p)
        assert dl(plain.handle, C.byref(r)) == INV
    assert dl(None, C.byref(r)) == INV
