"""lld_orb_extract (ORBextractor::operator() on the device) against the CPU restatement tests/orb_extract_ref.py: keypoints (all six
fields, in order), descriptors, per-level statistics and every pyramid level, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import orb_extract_ref as R
import oracle_orbsearch as OS
from orb_scenes import scene
from lld_slam_amd import ORBmatcher, abi, synth
from lld_slam_amd.orb_extractor import (OrbExtractorParams, OrbFeatures, OrbImage, ORBextractor, compute_stereo_matches_device)

pytestmark = pytest.mark.gpu

KITTI = (2000, 1.2, 8, 12, 7)
PATTERN = R.seeded_pattern(7)


def _hip():
    return C.CDLL("libamdhip64.so")


def download(ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    hip = _hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, C.cast(ptr, C.c_void_p), nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def check_equal(got, exp, ex, image_index=None):
    for f in ("xy", "octave", "angle", "response", "size", "desc"):
        g, e = np.asarray(getattr(got, f)), exp[f]
        assert g.shape == e.shape, f"{f}: {g.shape} vs {e.shape}"
        if g.dtype.kind == "f":
            assert np.array_equal(g.view(np.uint32), e.view(np.uint32)), f"{f} differs at {np.nonzero(g != e)[0][:5]}"
        else:
            assert np.array_equal(g, e), f"{f} differs"
    assert np.array_equal(got.stats, exp["stats"]), f"stats\n{got.stats}\nvs\n{exp['stats']}"
    if image_index is not None:
        lv, cols, rows, step = ex.pyramid(image_index)
        for l, lev in enumerate(exp["levels"]):
            assert (rows[l], cols[l]) == lev.shape and step[l] == cols[l]
            dev = download(lv[l], int(rows[l]) * int(step[l])).reshape(rows[l], step[l])
            assert np.array_equal(dev, lev), f"pyramid level {l} differs"


@pytest.fixture(scope="module")
def kitti_ex(gpu_ctx):
    with ORBextractor(gpu_ctx, *KITTI, PATTERN, max_cols=1241, max_rows=376, max_images=2) as ex:
        yield ex


def test_level_tables(kitti_ex):
    T = R.level_tables(*KITTI[:3])
    assert np.array_equal(kitti_ex.scale_factors, T["scale"]) and np.array_equal(kitti_ex.inv_scale_factors, T["inv_scale"])
    assert np.array_equal(kitti_ex.level_sigma2, T["sigma2"]) and np.array_equal(kitti_ex.inv_level_sigma2, T["inv_sigma2"])
    assert np.array_equal(kitti_ex.features_per_level, T["per_level"]) and np.array_equal(kitti_ex.umax, T["umax"])
    assert kitti_ex.max_keypoints == 2000 + 3 * 8          # max(N + 3, 4 nIni) = N + 3 on every KITTI level


SCENES = {}


def _exp(kind, cols, rows, seed, params=KITTI):
    key = (kind, cols, rows, seed, params)
    if key not in SCENES:
        img = scene(kind, cols, rows, seed)
        SCENES[key] = (img, R.extract(img, *params, PATTERN))
    return SCENES[key]


@pytest.mark.parametrize("kind,seed", [("textured", 0), ("textured", 1), ("flat", 2), ("busy", 3)])
def test_kitti_size_bit_exact(kitti_ex, kind, seed):
    img, exp = _exp(kind, 1241, 376, seed)
    got = kitti_ex(img)
    check_equal(got, exp, kitti_ex, 0)


@pytest.mark.parametrize("cols,rows,kind", [(752, 480, "textured"), (701, 263, "textured"), (333, 517, "busy"), (640, 240, "flat")])
def test_other_sizes_bit_exact(gpu_ctx, cols, rows, kind):
    img, exp = _exp(kind, cols, rows, 11, KITTI)
    with ORBextractor(gpu_ctx, *KITTI, PATTERN, max_cols=800, max_rows=520, max_images=1) as ex:
        check_equal(ex(img), exp, ex, 0)


def test_small_nfeatures_overshoot(gpu_ctx):
    params = (60, 1.3, 4, 20, 7)
    img, exp = _exp("textured", 700, 250, 5, params)
    with ORBextractor(gpu_ctx, *params, PATTERN, max_cols=700, max_rows=250, max_images=1) as ex:
        check_equal(ex(img), exp, ex, 0)


def test_statistics_cover_every_path(kitti_ex):
    """The scenes above exercise the fallback threshold, empty cells, the sorted phase, the unchanged-size finish and levels that
    return more keypoints than mnFeaturesPerLevel.  Cell interiors (3 px inside each cell) tile the level exactly, so the 6-px cell
    overlap never hands a pixel to the octree twice; the duplicate path of the octree is checked on the restatement
    (tests/test_oracle_orb_extract.py)."""
    stats, dups = [], 0
    for kind, seed in [("textured", 0), ("flat", 2), ("busy", 3)]:
        img, exp = _exp(kind, 1241, 376, seed)
        st = kitti_ex(img).stats
        assert np.array_equal(st, exp["stats"])
        stats.append(st)
        for c in exp["candidates"]:
            xy = [(x, y) for x, y, _ in c]
            dups += len(xy) - len(set(xy))
    S = np.concatenate(stats)
    assert (S[:, 1] > 0).any(), "no cell used min_th_fast"
    assert (S[:, 2] > 0).any(), "no cell stayed empty"
    assert (S[:, 4] > 0).any(), "the sorted phase never ran"
    assert (S[:, 5] == 1).any(), "no level finished on an unchanged size"
    assert (S[:, 6] > S[:, 7]).any(), "no level returned more than mnFeaturesPerLevel"
    assert S[:, 0].max() > 10000, "no busy level 0"
    assert dups == 0


def test_two_images_one_call_equals_two_calls_and_repeat(kitti_ex):
    a, _ = _exp("textured", 1241, 376, 0)
    b, _ = _exp("busy", 1241, 376, 3)
    both = kitti_ex([a, b])
    ga, gb = kitti_ex(a), kitti_ex(b)
    again = kitti_ex([a, b])
    for x, y in [(both[0], ga), (both[1], gb), (again[0], ga), (again[1], gb)]:
        for f in ("xy", "octave", "angle", "response", "size", "desc", "stats"):
            assert np.array_equal(getattr(x, f), getattr(y, f)), f


def test_device_image_input(kitti_ex, gpu_ctx):
    import torch
    img, exp = _exp("textured", 1241, 376, 1)
    t = torch.from_numpy(img).to("cuda:0")
    torch.cuda.synchronize()
    got = kitti_ex((t.data_ptr(), 1241, 376, 1241))
    check_equal(got, exp, kitti_ex, 0)


def test_stereo_hand_off(gpu_ctx):
    sc = synth.make_stereo_scene(0)
    left, right = sc["left"][0], sc["right"][0]
    with ORBextractor(gpu_ctx, *KITTI, PATTERN, max_cols=1241, max_rows=376, max_images=2) as ex:
        L, Rf = ex([left, right])
        el, er = R.extract(left, *KITTI, PATTERN), R.extract(right, *KITTI, PATTERN)
        check_equal(L, el, ex, 0); check_equal(Rf, er, ex, 1)
        dev = compute_stereo_matches_device(gpu_ctx, L, Rf, ex, sc["mb"], sc["mbf"])
        host = ORBmatcher(gpu_ctx).ComputeStereoMatchesFull(L, Rf, el["levels"], er["levels"], ex.inv_scale_factors, sc["mb"], sc["mbf"])
        n, ur, dep, br, sad = OS.compute_stereo_matches(L, Rf, el["levels"], er["levels"], ex.inv_scale_factors, sc["mb"], sc["mbf"])
    assert dev.n_matches == host.n_matches == n and n > 20
    for f, e in (("u_right", ur), ("depth", dep), ("best_r", br), ("sad", sad)):
        assert np.array_equal(getattr(dev, f), getattr(host, f)) and np.array_equal(getattr(dev, f), e), f


def test_invalid_arguments(gpu_ctx, kitti_ex):
    lib = gpu_ctx.lib
    create = lib.fn("orb_extractor_create")
    create.argtypes = [C.c_void_p, C.POINTER(OrbExtractorParams), C.POINTER(C.c_void_p)]
    pat = np.ascontiguousarray(PATTERN.reshape(-1))
    bad = pat.copy(); bad[17] = 14

    def params(p=pat, **kw):
        P = OrbExtractorParams(2000, 1.2, 8, 20, 7, 1241, 376, 2, p.ctypes.data_as(abi.c_int32_p))
        for k, v in kw.items():
            setattr(P, k, v)
        return P
    h = C.c_void_p()
    assert create(gpu_ctx.handle, C.byref(params(bad)), C.byref(h)) == abi.LLD_ERR_INVALID
    assert create(gpu_ctx.handle, C.byref(params(n_levels=17)), C.byref(h)) == abi.LLD_ERR_INVALID
    assert create(gpu_ctx.handle, C.byref(params(min_th_fast=0)), C.byref(h)) == abi.LLD_ERR_INVALID
    assert create(gpu_ctx.handle, C.byref(params(max_cols=20000)), C.byref(h)) == abi.LLD_ERR_INVALID
    assert create(gpu_ctx.handle, None, C.byref(h)) == abi.LLD_ERR_INVALID
    P = params(); P.pattern = None
    assert create(gpu_ctx.handle, C.byref(P), C.byref(h)) == abi.LLD_ERR_INVALID
    img = scene("textured", 1241, 376, 0)
    assert kitti_ex.extract_raw([np.zeros((377, 1241), np.uint8)])[0] == abi.LLD_ERR_INVALID      # taller than max_rows
    assert kitti_ex.extract_raw([np.zeros((376, 1242), np.uint8)])[0] == abi.LLD_ERR_INVALID      # wider than max_cols
    assert kitti_ex.extract_raw([np.zeros((120, 400), np.uint8)])[0] == abi.LLD_ERR_INVALID       # level 7 too small for one cell
    assert kitti_ex.extract_raw([np.zeros((200, 640), np.uint8)])[0] == abi.LLD_ERR_INVALID       # level 7 is 179x56: nRows = 0
    assert kitti_ex.extract_raw([img, img, img])[0] == abi.LLD_ERR_INVALID                       # n_images > max_images
    assert kitti_ex.extract_raw([])[0] == abi.LLD_ERR_INVALID
    ext = lib.fn("orb_extract")
    ext.argtypes = [C.c_void_p, C.c_int, C.POINTER(OrbImage), C.POINTER(OrbFeatures)]
    assert ext(kitti_ex.handle, 1, None, None) == abi.LLD_ERR_INVALID
    ims = (OrbImage * 1)(OrbImage(None, 1241, 376, 1241, 0))
    outs = (OrbFeatures * 1)()
    assert ext(kitti_ex.handle, 1, ims, outs) == abi.LLD_ERR_INVALID
    ims = (OrbImage * 1)(OrbImage(img.ctypes.data_as(abi.c_uint8_p), 1241, 376, 1241, 0))
    assert ext(kitti_ex.handle, 1, ims, outs) == abi.LLD_ERR_INVALID                             # null output arrays
