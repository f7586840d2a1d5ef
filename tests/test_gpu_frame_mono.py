"""lld_frame_build_mono / lld_frame_build_mono_keypoints / lld_frame_keypoints_download: the RGB-D and the monocular Frame built on the
device, against the numpy restatement tests/frame_mono_ref.py (which is not the reference) and, for "the frame is a frame", against
lld_frame_create on the downloaded arrays.  Everything bit for bit: floats as uint32, ids as integers.  The one concession: a NaN is
compared as "a NaN" (the restated arithmetic does not define which one), and only keypoints that are not finite produce one."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import frame_mono_ref as M
import orb_extract_ref as R
from lld_slam_amd import Context, abi, orb_search, synth
from lld_slam_amd.orb_extractor import ORBextractor
from lld_slam_amd.orb_search import Frame
from lld_slam_amd.tracking import DeviceTrackedFrame

pytestmark = pytest.mark.gpu

SMALL = (500, 1.2, 8, 12, 7)
PATTERN = R.seeded_pattern(7)
W, H = M.W, M.H                       # 416 x 240: the smallest size at which all eight levels stay >= 62 px
CAM, DIST5, MBF = M.CAM, M.DIST5, M.MBF
DIST4 = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)                  # a four-coefficient camera that stays tame over the image
CAM5 = CAM + (MBF,)
f32 = np.float32
INV, UNS, OK = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED, abi.LLD_OK


def bits(a):
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def bits_any(a):
    a = np.ascontiguousarray(a)
    return bits(a) if a.dtype == np.float32 else a


def assert_same(got, exp, what=""):
    """got: MonoKeypoints; exp: the restatement's dict."""
    for f in ("xy_un", "u_right", "depth"):
        g, e = bits(getattr(got, f)), bits(exp[f])
        assert g.shape == e.shape, f"{what} {f} {g.shape} vs {e.shape}"
        assert np.array_equal(g, e), f"{what} {f} differs at {np.argwhere(g != e)[:8].tolist()}"


TABLES = R.level_tables(*SMALL[:3])


def frame_of(kp, idx=None):
    idx = np.arange(kp["xy"].shape[0]) if idx is None else np.asarray(idx, np.int64)
    return Frame(desc=kp["desc"][idx].copy(), xy=kp["xy"][idx].copy(), octave=kp["octave"][idx].copy(), uright=np.full(len(idx), -1, f32),
                 angle=kp["angle"][idx].copy(), max_x=float(W), max_y=float(H), scale=TABLES["scale"], sigma2=TABLES["sigma2"],
                 inv_sigma2=TABLES["inv_sigma2"]).normalise()


@pytest.fixture(scope="module")
def crafted():
    """300 keypoints (the three out-of-grid ones first) and the depth images.  Computed once, never changed."""
    kp = M.crafted_keypoints()
    return dict(kp=kp, F=frame_of(kp), f32=M.depth_image("f32"), u16=M.depth_image("u16"), ramp=M.depth_ramp())


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view)).cuda()


def run(ctx, F, dist, depth=None, factor=1.0, device=False, cam=CAM, mbf=MBF):
    dev = None
    if device:
        import torch
        t = dict(xy=to_device(F.xy), desc=to_device(F.desc), angle=to_device(F.angle))
        torch.cuda.synchronize()
        dev = {k: v.data_ptr() for k, v in t.items()}
    built = orb_search.build_mono_frame_keypoints(ctx.lib, ctx.handle, F, cam, dist, mbf, depth=depth, depth_factor=factor, device=dev, image_size=(W, H))
    try:
        return built.download()
    finally:
        built.close()


# ---------------------------------------------------------------------------------------------- undistortion
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dist", [DIST5, DIST5[:4], DIST4, DIST4 + (0.05,), (0.0, -0.9, 0.01, 0.002, 1.1), (0.0, 0.5, 0.01, 0.002)],
                         ids=["k5", "k5-cut", "k4", "k4+k3", "k1=0,5", "k1=0,4"])
def test_undistortion(gpu_ctx, crafted, dist, device):
    F = crafted["F"]
    exp = M.build(F.xy, CAM, dist, MBF)
    got = run(gpu_ctx, F, dist, device=device)
    assert F.n == 300 and np.array_equal(F.xy[:3], M.OUT_OF_GRID)
    assert_same(got, exp, "undistortion")
    assert np.all(got.u_right == -1) and np.all(got.depth == -1)
    if dist[0] == 0.0:
        assert np.array_equal(got.xy_un.view(np.uint32), F.xy.view(np.uint32))          # the input, bit for bit
    else:
        assert np.abs(got.xy_un - F.xy).max() > 0.5
    if dist == DIST5:
        _, _, inside = M.grid_cell(got.xy_un, M.image_bounds(W, H, CAM, DIST5))
        assert not inside[:3].any() and inside[3:].sum() > 250


# ---------------------------------------------------------------------------------------------- depth
def depth_keypoints(crafted, cols, rows):
    """The crafted set with its tail replaced by the cases of the look-up, for a cols x rows depth image."""
    kp = {k: v.copy() for k, v in crafted["kp"].items()}
    c, r = float(cols), float(rows)
    special = f32([[10.99, 7.999], [-0.5, 12.0], [15.0, -0.999], [-0.25, -0.75], [-1.0, 30.0], [30.0, -1.0], [-1.0001, 5.0],
                   [c, 10.0], [10.0, r], [c - 0.001, r - 0.001], [np.nextafter(f32(c), f32(0)), 3.0], [c + 40.0, 5.0], [5.0, r + 1e6], [3e38, 1.0], [1.0, -3e38],
                   [np.nan, 5.0], [5.0, np.nan], [np.inf, 5.0], [5.0, -np.inf], [np.nan, np.nan], [0.0, 0.0], [-0.0, -0.0]])
    kp["xy"][-len(special):] = special
    return kp, len(special)


VARIANTS = {"f32,1": ("f32", 1.0), "f32,1+5e-6": ("f32", 1.0 + 5e-6), "f32,0.5": ("f32", 0.5), "u16,1/5000": ("u16", 1.0 / 5000.0), "u16,1": ("u16", 1.0)}


@pytest.mark.parametrize("shape", ["full", "padded", "smaller", "device"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_depth(gpu_ctx, crafted, variant, shape):
    kind, factor = VARIANTS[variant]
    img = crafted[kind]
    assert (img == 0).any() and (kind == "u16" or (np.isnan(img).any() and np.isposinf(img).any() and (img < 0).any()))
    if shape == "smaller":
        img = np.ascontiguousarray(img[:200, :300])
    rows, cols = img.shape
    kp, ns = depth_keypoints(crafted, cols, rows)
    F = frame_of(kp)
    exp = M.build(F.xy, CAM, DIST5, MBF, img, factor)
    arg, keep = img, None
    if shape in ("padded", "device"):
        wide = np.full((rows, cols + 7), 77, img.dtype)
        wide[:, :cols] = img
        if shape == "padded":
            arg = wide[:, :cols]
            assert arg.strides[0] == (cols + 7) * img.itemsize
        else:
            import torch
            keep = to_device(wide); torch.cuda.synchronize()
            arg = (keep.data_ptr(), cols, rows, (cols + 7) * img.itemsize, abi.DEPTH_F32 if kind == "f32" else abi.DEPTH_U16)
    got = run(gpu_ctx, F, DIST5, depth=arg, factor=factor, device=shape == "device")
    assert_same(got, exp, f"{variant} {shape}")
    # what the scene exercises, from the restatement alone
    has = exp["depth"] > 0
    assert has.sum() > 100 and (~has).sum() > 20
    sp = slice(F.n - ns, F.n)
    assert exp["depth"][sp][0] > 0 or img[7, 10] <= 0 or np.isnan(img[7, 10])               # (10.99, 7.999) reads pixel (10, 7)
    assert np.all(exp["depth"][sp][4:7] == -1) and np.all(exp["depth"][sp][7:9] == -1) and np.all(exp["depth"][sp][11:20] == -1)
    if kind == "f32":
        assert np.isposinf(exp["depth"]).any()
        i = int(np.nonzero(np.isposinf(exp["depth"]))[0][0])
        assert bits(got.u_right)[i] == bits(got.xy_un[:, 0])[i]                              # +inf: mvuRight = u_un
    if variant == "f32,1+5e-6":
        assert np.array_equal(bits(exp["depth"]), bits(M.build(F.xy, CAM, DIST5, MBF, img, 1.0)["depth"]))
    if variant == "u16,1":
        assert np.all(exp["depth"][has] == np.round(exp["depth"][has]))


def test_depth_is_sampled_at_the_distorted_position(gpu_ctx, crafted):
    F = crafted["F"]; ramp = crafted["ramp"]
    exp = M.build(F.xy, CAM, DIST5, MBF, ramp, 1.0)
    wrong, ok = M.sample_depth(np.nan_to_num(exp["xy_un"]), ramp, 1.0)
    both = ok & (exp["depth"] > 0)
    assert (wrong[both] != exp["depth"][both]).sum() > 0.5 * F.n                             # most keypoints would read another pixel
    assert_same(run(gpu_ctx, F, DIST5, depth=ramp), exp, "ramp")
    # without distortion the two positions coincide and the same kernel gives the plain look-up
    assert_same(run(gpu_ctx, F, (0.0, 0.0, 0.0, 0.0), depth=ramp), M.build(F.xy, CAM, (0, 0, 0, 0), MBF, ramp, 1.0), "ramp, no distortion")


def test_monocular(gpu_ctx, crafted):
    F = crafted["F"]
    for dist in (DIST5, (0.0, 0.0, 0.0, 0.0)):
        got = run(gpu_ctx, F, dist, depth=None)
        assert np.array_equal(got.u_right.view(np.uint32), np.full(F.n, -1, f32).view(np.uint32))
        assert np.array_equal(got.depth.view(np.uint32), np.full(F.n, -1, f32).view(np.uint32))
        assert_same(got, M.build(F.xy, CAM, dist, MBF), "monocular")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, orb_search.MAX_KEYPOINTS])
def test_counts(gpu_ctx, crafted, n):
    F = frame_of(crafted["kp"], np.arange(n) % 300)
    img = crafted["u16"]
    got = run(gpu_ctx, F, DIST5, depth=img, factor=1.0 / 5000.0)
    assert got.xy_un.shape == (n, 2) and got.u_right.shape == (n,)
    assert_same(got, M.build(F.xy, CAM, DIST5, MBF, img, 1.0 / 5000.0), f"n = {n}")


def raw_call(ctx, F, dist=DIST5, depth=None, factor=1.0, cam=CAM, mbf=MBF, drop=None, kp_edit=None, depth_edit=None, **prm_edit):
    """lld_frame_build_mono_keypoints with one argument spoiled: the status (a frame that was made is destroyed)."""
    lib = ctx.lib
    H_ = dataclasses.replace(F, min_x=-8.0, max_x=W + 8.0, min_y=-6.0, max_y=H + 6.0).normalise()
    kp = orb_search.keypoints_struct(F)
    prm, keep = orb_search.frame_mono_params(H_, cam, dist, mbf)
    for k, v in prm_edit.items():
        if k == "dist_at":
            prm.dist[v[0]] = v[1]
        else:
            setattr(prm, k, v)
    for k, v in (kp_edit or {}).items():
        setattr(kp, k, v)
    D, keep2 = orb_search.depth_image_struct(depth, factor)
    for k, v in (depth_edit or {}).items():
        setattr(D, k, v)
    a = dict(ctx=ctx.handle, kp=kp, params=prm)
    if drop: a[drop] = None
    st, h = orb_search.build_mono_frame_raw(lib, a["ctx"], a["kp"], D, a["params"])
    if st == OK:
        orb_search.MonoBuiltFrame(lib, ctx.handle, H_, h).close()
    else:
        assert not h.value
    return st


def test_one_more_than_the_limit_is_refused(gpu_ctx, crafted):
    big = np.arange(orb_search.MAX_KEYPOINTS + 1) % 300
    assert raw_call(gpu_ctx, frame_of(crafted["kp"], big)) == UNS
    assert raw_call(gpu_ctx, frame_of(crafted["kp"], big), depth=crafted["f32"]) == UNS
    assert raw_call(gpu_ctx, frame_of(crafted["kp"], big[:-1])) == OK


# ---------------------------------------------------------------------------------------------- extractor route
@pytest.fixture(scope="module")
def scene():
    """A 416x240 grey image, its CPU extraction, a depth image over it and the restatement's frame.  Computed once, never changed."""
    sc = synth.make_stereo_scene(0, width=W, height=H)
    grey, grey2 = sc["left"][0], sc["right"][0]
    e = R.extract(grey, *SMALL, PATTERN)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (1.5 + 2.5 * (yy / H) + 0.4 * np.sin(xx / 37.0)).astype(f32)
    rng = np.random.default_rng(11)
    m = rng.random((H, W))
    depth[m < 0.08] = 0.0; depth[(m >= 0.08) & (m < 0.1)] = np.nan
    raw16 = np.where(np.isfinite(depth), np.round(np.nan_to_num(depth) * 5000.0), 0).astype(np.uint16)
    return dict(grey=grey, grey2=grey2, e=e, depth=depth, raw16=raw16)


@pytest.fixture(scope="module")
def small_ex(gpu_ctx):
    with ORBextractor(gpu_ctx, *SMALL, PATTERN, max_cols=W, max_rows=H, max_images=2) as ex:
        yield ex


@pytest.mark.parametrize("kind", ["f32", "u16", "mono"])
def test_extractor_route(gpu_ctx, scene, small_ex, kind):
    depth, factor = {"f32": (scene["depth"], 1.0), "u16": (scene["raw16"], 1.0 / 5000.0), "mono": (None, 1.0)}[kind]
    L = small_ex(scene["grey"])
    assert L.n > 400 and np.array_equal(L.xy, scene["e"]["xy"]) and np.array_equal(L.desc, scene["e"]["desc"])
    built = small_ex.build_mono_frame(L, CAM, DIST5, MBF, depth=depth, depth_factor=factor)
    try:
        got = built.download()
        b = M.image_bounds(W, H, CAM, DIST5)
        assert (f32(built.F.min_x), f32(built.F.max_x), f32(built.F.min_y), f32(built.F.max_y)) == tuple(b)
    finally:
        built.close()
    exp = M.build(L.xy, CAM, DIST5, MBF, depth, factor)
    assert_same(got, exp, "restatement")
    via_kp = run(gpu_ctx, L, DIST5, depth=depth, factor=factor)
    assert_same(got, dataclasses.asdict(via_kp), "keypoint route")
    if kind != "mono":
        assert (got.depth > 0).sum() > 300 and (got.depth < 0).sum() > 10


def test_frame_survives_next_extract_and_the_extractor(gpu_ctx, scene):
    ex = ORBextractor(gpu_ctx, *SMALL, PATTERN, max_cols=W, max_rows=H, max_images=2)
    try:
        L = ex(scene["grey"])
        built = ex.build_mono_frame(L, CAM, DIST5, MBF, depth=scene["depth"])
        exp = M.build(L.xy, CAM, DIST5, MBF, scene["depth"], 1.0)
        L1 = ex(scene["grey2"])                                                 # overwrites the extractor's keypoints
        assert not np.array_equal(L1.xy[:50], L.xy[:50])
        assert_same(built.download(), exp, "after the next extract")
        second = ex.build_mono_frame(L1, CAM, DIST5, MBF, depth=scene["raw16"], depth_factor=1.0 / 5000.0)
        exp1 = M.build(L1.xy, CAM, DIST5, MBF, scene["raw16"], 1.0 / 5000.0)
    finally:
        ex.close()                                                              # the extractor goes first
    assert_same(second.download(), exp1, "after the extractor")
    assert_same(built.download(), exp, "first frame, again")
    # the frames kept their own descriptors, octaves and angles too: a search on them still works
    T = np.eye(4, dtype=f32)
    st = built.download()
    last, mp, ids = _queries(built.F, st, np.random.default_rng(2))
    out, _ = built.search_last_frame(orb_search.frame_view(T, CAM5, built.F), last, th=15.0)
    assert out.n_matches > 50
    second.close(); built.close()


# ---------------------------------------------------------------------------------------------- the frame is a frame
def _queries(F, st, rng):
    """MapPoints un-projected from the frame's own undistorted keypoints with depth (camera at the origin), descriptors with a few
    flipped bits.  F: the host Frame after download (xy = mvKeysUn)."""
    fx, fy, cx, cy = [f32(c) for c in CAM]
    idx = np.nonzero(np.isfinite(st.depth) & (st.depth > 0))[0]
    z = st.depth[idx].astype(f32)
    P = np.stack([(st.xy_un[idx, 0] - cx) * z / fx, (st.xy_un[idx, 1] - cy) * z / fy, z], 1).astype(f32)
    desc = F.desc[idx].copy()
    for r in range(len(idx)):
        for b in rng.integers(0, 256, 6):
            desc[r, b >> 5] ^= np.uint32(1) << np.uint32(b & 31)
    dist = np.linalg.norm(P, axis=1).astype(f32)
    maxd = (dist * F.scale[F.octave[idx]]).astype(f32)
    last = dict(world_pos=P, valid=np.ones(len(idx), np.uint8), octave=F.octave[idx].copy(), angle=F.angle[idx].copy(), desc=desc,
                has_obs=np.ones(len(idx), np.uint8))
    mp = dict(world_pos=P, normal=(P / dist[:, None]).astype(f32), max_distance=maxd, min_distance=(maxd / F.scale[-1]).astype(f32),
              desc=desc, has_obs=np.ones(len(idx), np.uint8), skip=np.zeros(len(idx), np.uint8))
    return last, mp, np.arange(len(idx), dtype=np.int32)


def with_out_of_grid(e, rng):
    """The extraction's keypoints followed by the three out-of-grid ones (which the ORB extractor, 19 px inside the image, never gives)."""
    k = len(M.OUT_OF_GRID)
    kp = dict(xy=np.concatenate([e["xy"], M.OUT_OF_GRID]), octave=np.concatenate([e["octave"], np.zeros(k, np.int32)]),
              angle=np.concatenate([e["angle"], f32([10.0, 100.0, 200.0])]),
              desc=np.concatenate([e["desc"], rng.integers(0, 2 ** 32, (k, 8), dtype=np.uint64).astype(np.uint32)]))
    return frame_of(kp)


def test_built_frame_is_a_frame(gpu_ctx, scene):
    F = with_out_of_grid(scene["e"], np.random.default_rng(4))
    n = F.n; oog = np.arange(n - 3, n)
    built = orb_search.build_mono_frame_keypoints(gpu_ctx.lib, gpu_ctx.handle, F, CAM, DIST5, MBF, depth=scene["depth"], image_size=(W, H))
    st = built.download()
    b = orb_search.image_bounds(gpu_ctx.lib, W, H, CAM, DIST5)
    _, _, inside = M.grid_cell(st.xy_un, b)
    assert not inside[oog].any() and inside[:n - 3].all() and np.all(st.depth[oog] > 0)
    # what the host would hand lld_frame_create: the downloaded arrays, the grid of lld_frame_image_bounds
    F2 = dataclasses.replace(F, xy=st.xy_un.copy(), uright=st.u_right.copy(), min_x=float(b[0]), max_x=float(b[1]), min_y=float(b[2]), max_y=float(b[3])).normalise()
    last, mp, ids = _queries(F2, st, np.random.default_rng(5))                 # the out-of-grid keypoints have depth: they are queried too
    assert len(ids) > 300
    T = np.eye(4, dtype=f32); T[:3, 3] = [0.01, -0.004, 0.008]
    view = orb_search.frame_view(T, CAM5, F2)
    with orb_search.ResidentFrame(gpu_ctx.lib, gpu_ctx.handle, F2) as plain:
        for name, args, kw in (("search_last_frame", (view, last), dict(th=15.0)), ("search_local_points", (view, mp), dict(th=3.0))):
            a, xa = getattr(built, name)(*args, **kw); c, xb = getattr(plain, name)(*args, **kw)
            assert a.n_matches == c.n_matches and a.n_matches > 50 and a.rounds == c.rounds, name
            for f in ("match", "best_dist", "second_dist", "removed", "owner"):
                assert np.array_equal(getattr(a, f), getattr(c, f)), f"{name}.{f}"
            assert np.all(a.owner[oog] == -1) and not np.isin(a.match, oog).any(), name      # no out-of-grid keypoint owns a match
            if isinstance(xa, dict):
                assert np.array_equal(xa["in_view"], xb["in_view"])
                v = xa["in_view"] != 0
                for f in ("proj_uvr", "level", "view_cos"):
                    assert np.array_equal(bits_any(xa[f][v]), bits_any(xb[f][v])), f"{name}.{f}"
            else:
                assert np.array_equal(bits(xa), bits(xb)), name
    recs = []
    for tf in (DeviceTrackedFrame.from_built(gpu_ctx, built, CAM5, th_motion=15.0, th_local=3.0),
               DeviceTrackedFrame(gpu_ctx, F2, CAM5, th_motion=15.0, th_local=3.0)):
        with tf:
            tf.track_with_motion_model(T, last, ids)
            tf.track_local_map(mp, ids)
            recs.append(tf.download())
    for a, c in zip(*recs):
        assert a.keys() == c.keys()
        for k in a:
            if isinstance(a[k], np.ndarray):
                g, e = a[k], c[k]
                assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, e.view(np.uint64) if e.dtype == np.float64 else e), k
            else:
                assert np.float64(a[k]).view(np.uint64) == np.float64(c[k]).view(np.uint64), k
        assert np.all(a["kp_point_id"][oog] == -1)
    assert recs[0][0]["n_search"] > 50 and recs[0][1]["n_inliers"] > 20


# ---------------------------------------------------------------------------------------------- arguments
def test_refusals(gpu_ctx, crafted, scene):
    lib, ctx = gpu_ctx.lib, gpu_ctx.handle
    F = crafted["F"]; d32, d16 = crafted["f32"], crafted["u16"]
    call = lambda **kw: raw_call(gpu_ctx, F, **kw)
    nan, inf = float("nan"), float("inf")

    for drop in ("ctx", "kp", "params"):
        assert call(drop=drop) == INV, drop
    fn = lib.fn("frame_build_mono_keypoints")
    assert fn(ctx, None, None, None, None) == INV                               # no place for the handle
    assert call(left_angle=None) == INV and call(level_scale=None) == INV and call(level_inv_sigma2=None) == INV
    assert call(kp_edit=dict(xy=None)) == INV and call(kp_edit=dict(desc=None)) == INV and call(kp_edit=dict(octave=None)) == INV
    assert call(kp_edit=dict(n=-1)) == INV
    for v in (0.0, -300.0, nan, inf):
        assert call(fx=v) == INV and call(fy=v) == INV, v
    assert call(cx=nan) == INV and call(cy=inf) == INV
    for nd in (0, 3, 6, -1):
        assert call(n_dist=nd) == INV, nd
    for at in range(5):
        assert call(dist_at=(at, nan)) == INV and call(dist_at=(at, -inf)) == INV, at
    assert call(dist=DIST5[:4], dist_at=(4, nan)) == OK                         # dist[4] is not a coefficient when n_dist = 4
    assert call(mbf=nan) == INV and call(mbf=inf) == INV
    for gc, gr in ((0, 48), (64, 0), (-1, 48), (128, 64), (8192, 1)):
        assert call(grid_cols=gc, grid_rows=gr) == INV, (gc, gr)
    for nl in (0, -1, 17):
        assert call(n_levels=nl) == INV, nl
    for o in (8, -1):
        G = frame_of(crafted["kp"]); G.octave[5] = o
        assert raw_call(gpu_ctx, G) == INV, o
    assert raw_call(gpu_ctx, F, n_levels=3) == INV                              # the crafted octaves reach 7
    # the depth image
    for edit in (dict(cols=0), dict(cols=-5), dict(cols=16384), dict(rows=0), dict(rows=16384), dict(step=W * 4 - 4), dict(step=W * 4 + 2), dict(step=0),
                 dict(type=2), dict(type=-1), dict(factor=nan), dict(factor=inf), dict(data=None)):
        assert call(depth=d32, depth_edit=edit) == INV, edit
    for edit in (dict(step=W * 2 - 2), dict(step=W * 2 + 1), dict(cols=16384, step=16384 * 2), dict(factor=-inf)):
        assert call(depth=d16, depth_edit=edit) == INV, edit
    assert call(depth=d32) == OK and call(depth=d16, factor=0.0) == OK and call(depth=d32, factor=-2.0) == OK
    assert raw_call(gpu_ctx, frame_of(crafted["kp"], [])) == OK                 # no keypoints: an empty frame (Frame.cc:184-185)
    assert call() == OK                                                         # after the refusals, a valid call succeeds

    with ORBextractor(gpu_ctx, *SMALL, PATTERN, max_cols=W, max_rows=H, max_images=2) as ex:
        Hf = orb_search.mono_host_frame(lib, scene_frame(scene), CAM, DIST5)
        prm, keep = orb_search.frame_mono_params(Hf, CAM, DIST5, MBF)
        D, keep2 = orb_search.depth_image_struct(scene["depth"], 1.0)
        assert ex.build_mono_frame_raw(0, D, prm)[0] == INV                     # no successful extract yet
        L = ex(scene["grey"])                                                   # one image
        for im in (1, 2, -1):
            assert ex.build_mono_frame_raw(im, D, prm)[0] == INV, im            # index outside the last call's n_images
        assert ex.build_mono_frame_raw(0, D, None)[0] == INV
        fb = lib.fn("frame_build_mono")
        assert fb(None, 0, C.byref(D), C.byref(prm), C.byref(C.c_void_p())) == INV and fb(ex.handle, 0, C.byref(D), C.byref(prm), None) == INV
        bad, _ = orb_search.frame_mono_params(Hf, (0.0,) + CAM[1:], DIST5, MBF)
        assert ex.build_mono_frame_raw(0, D, bad)[0] == INV
        bad, _ = orb_search.frame_mono_params(Hf, CAM, DIST5, MBF); bad.n_dist = 6
        assert ex.build_mono_frame_raw(0, D, bad)[0] == INV
        Dbad, _ = orb_search.depth_image_struct(scene["depth"], 1.0); Dbad.type = 7
        assert ex.build_mono_frame_raw(0, Dbad, prm)[0] == INV
        Dbad, _ = orb_search.depth_image_struct(scene["depth"], 1.0); Dbad.rows = 16384
        assert ex.build_mono_frame_raw(0, Dbad, prm)[0] == INV
        built = ex.build_mono_frame(L, CAM, DIST5, MBF, depth=scene["depth"])  # and then the valid call
        # a frame and a context that do not belong together
        other = Context(0)
        try:
            with pytest.raises(ValueError):
                DeviceTrackedFrame.from_built(other, built, CAM5)
        finally:
            other.close()
        assert_same(built.download(), M.build(L.xy, CAM, DIST5, MBF, scene["depth"], 1.0), "after the refusals")
        # lld_frame_stereo_download on a frame built here
        sd = lib.fn("frame_stereo_download"); sd.argtypes = [C.c_void_p, C.POINTER(orb_search.StereoResult)]; sd.restype = C.c_int
        out = np.empty(L.n, f32); r = orb_search.StereoResult()
        r.u_right = out.ctypes.data_as(abi.c_float_p); r.depth = out.ctypes.data_as(abi.c_float_p)
        assert sd(built.handle, C.byref(r)) == INV
        built.close()

    # lld_frame_keypoints_download on a frame lld_frame_create made, on a stereo-built one, on nothing
    dl = lib.fn("frame_keypoints_download"); dl.argtypes = [C.c_void_p, abi.c_float_p, abi.c_float_p, abi.c_float_p]; dl.restype = C.c_int
    xy = np.empty((4096, 2), f32); a = np.empty(4096, f32); b_ = np.empty(4096, f32)
    ptrs = (xy.ctypes.data_as(abi.c_float_p), a.ctypes.data_as(abi.c_float_p), b_.ctypes.data_as(abi.c_float_p))
    with orb_search.ResidentFrame(lib, ctx, F) as plain:
        assert dl(plain.handle, *ptrs) == INV
    sc = synth.make_stereo_scene(2, n=300, width=W, height=H)
    stereo = orb_search.build_stereo_frame_keypoints(lib, ctx, sc["L"], sc["R"], sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    try:
        assert dl(stereo.handle, *ptrs) == INV
        assert stereo.download().n_matches > 100                                # and the stereo frame is none the worse
    finally:
        stereo.close()
    assert dl(None, *ptrs) == INV
    # NULL outputs are allowed one by one
    built = orb_search.build_mono_frame_keypoints(lib, ctx, F, CAM, DIST5, MBF, depth=d32, image_size=(W, H))
    try:
        assert dl(built.handle, None, None, None) == OK and dl(built.handle, None, ptrs[1], None) == OK
        assert np.array_equal(bits(a[:F.n]), bits(M.build(F.xy, CAM, DIST5, MBF, d32, 1.0)["u_right"]))
    finally:
        built.close()


def scene_frame(scene):
    return frame_of(scene["e"])
