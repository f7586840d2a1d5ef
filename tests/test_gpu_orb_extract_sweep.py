"""lld_orb_extract across its accepted parameters, image sizes, inputs and batches, against the CPU restatement
tests/orb_extract_ref.py through test_gpu_orb_extract.check_equal: all six keypoint fields by bit pattern, the descriptors, the
per-level statistics and every pyramid level.  Each test names the path of the restatement it reaches; the statistics columns
(n_candidates, cells_min_th, cells_empty, iterations, sorted_rounds, finish_unchanged, n_keypoints, features_wanted) show it is taken."""
import ctypes as C

import numpy as np
import pytest

import bow_ref as B
import orb_extract_ref as R
import oracle_orbsearch as OS
from lld_slam_amd import ORBmatcher, abi, synth
from lld_slam_amd import vocabulary as voc
from lld_slam_amd.orb_extractor import OrbFeatures, OrbImage, OrbLevelStats, ORBextractor, compute_stereo_matches_device
from orb_scenes import scene
from test_gpu_orb_extract import check_equal, download

pytestmark = pytest.mark.gpu

PATTERN = R.seeded_pattern(7)
KITTI = (2000, 1.2, 8, 20, 7)
EUROC = (1200, 1.2, 8, 20, 7)
TUM = (1000, 1.2, 8, 20, 7)
CNT, MIN_TH, EMPTY, ITER, SORTED, UNCHANGED, NKP, WANTED = range(8)

_CACHE = {}


def exp(kind, cols, rows, seed, params, pattern=None):
    """(image, restatement result), cached per (scene, parameters, pattern)."""
    pat = PATTERN if pattern is None else pattern
    key = (kind, cols, rows, seed, params, pat.tobytes())
    if key not in _CACHE:
        img = scene(kind, cols, rows, seed)
        _CACHE[key] = (img, R.extract(img, *params, pat))
    return _CACHE[key]


def run(ctx, params, kind, cols, rows, seed=0, pattern=None):
    """One image through a fresh extractor sized for it; checked bit for bit.  Returns (statistics, restatement result)."""
    img, e = exp(kind, cols, rows, seed, params, pattern)
    with ORBextractor(ctx, *params, PATTERN if pattern is None else pattern, max_cols=cols, max_rows=rows, max_images=1) as ex:
        check_equal(ex(img), e, ex, 0)
    return e["stats"], e


def need(params, cols, rows):
    """The output capacity lld_orb_extract requires for one image (include/lld_amd.h): sum over levels of max(N_l + 3, 4 nIni_l)."""
    T = R.level_tables(*params[:3])
    return sum(max(int(T["per_level"][l]) + 3, 4 * R.n_ini(*R.level_size(cols, rows, T["inv_scale"][l]))) for l in range(params[2]))


def call(ex, images, capacity):
    """lld_orb_extract with an explicit output capacity per image; returns the status."""
    n = len(images)
    ims, outs, keep = (OrbImage * n)(), (OrbFeatures * n)(), []
    for i, (a, cap) in enumerate(zip(images, capacity)):
        ims[i] = OrbImage(a.ctypes.data_as(abi.c_uint8_p) if a is not None else None, a.shape[1] if a is not None else 1241,
                          a.shape[0] if a is not None else 376, a.strides[0] if a is not None else 1241, 0)
        arrs = [np.zeros((max(cap, 1), w), t) for w, t in ((2, np.float32), (1, np.int32), (1, np.float32), (1, np.float32), (1, np.float32),
                                                            (8, np.uint32))]
        st = (OrbLevelStats * ex.n_levels)()
        keep += arrs + [st]
        outs[i] = OrbFeatures(cap, 0, *(x.ctypes.data_as(p) for x, p in zip(arrs, (abi.c_float_p, abi.c_int32_p, abi.c_float_p, abi.c_float_p,
                                                                                    abi.c_float_p, abi.c_uint32_p))),
                              C.cast(st, C.POINTER(OrbLevelStats)))
    return ex._extract(ex.handle, n, ims, outs)


# ------------------------------------------------------------------------------------------------ shipped configurations
@pytest.mark.parametrize("params,cols,rows", [(KITTI, 1241, 376), (EUROC, 752, 480), (TUM, 640, 480)], ids=["kitti", "euroc", "tum"])
@pytest.mark.parametrize("kind", ["textured", "busy"])
def test_shipped_configuration(gpu_ctx, params, cols, rows, kind):
    """iniThFAST = 20 / minThFAST = 7 as the shipped yaml files set them, at each dataset's size: the fallback threshold
    (cells_min_th > 0 on textured) and the sorted phase (busy)."""
    S, _ = run(gpu_ctx, params, kind, cols, rows, 21)
    assert (S[:, SORTED] > 0).any() if kind == "busy" else (S[:, MIN_TH] > 0).any()


# ------------------------------------------------------------------------------------------------ level count and scale
def test_one_level(gpu_ctx):
    """n_levels = 1: no resize launch, every keypoint on level 0, N = nfeatures on the one level."""
    S, e = run(gpu_ctx, (1000, 1.2, 1, 20, 7), "textured", 640, 480, 22)
    assert S.shape == (1, 8) and S[0, WANTED] == 1000 and len(e["octave"]) > 500 and np.all(e["octave"] == 0)


def test_sixteen_levels_at_scale_1_05(gpu_ctx):
    """n_levels = LLD_ORB_MAX_LEVELS at a scale barely above 1: sixteen levels of nearly the same size."""
    S, e = run(gpu_ctx, (2000, 1.05, 16, 20, 7), "textured", 1241, 376, 23)
    assert S.shape == (16, 8) and set(np.unique(e["octave"])) == set(range(16))


def test_scale_2_hits_cvround_ties(gpu_ctx):
    """scale 2.0 on odd sizes: cols * inv = 350.5 and rows * inv = 262.5 at level 1, ties that cvRound sends to the even neighbour."""
    params = (1000, 2.0, 4, 20, 7)
    inv = R.level_tables(*params[:3])["inv_scale"]
    assert [R.level_size(701, 525, inv[l]) for l in range(1, 4)] == [(350, 262), (175, 131), (88, 66)]
    run(gpu_ctx, params, "textured", 701, 525, 24)


@pytest.mark.parametrize("scale", [1.25, 1.5])
def test_scale_with_inexact_inverse(gpu_ctx, scale):
    """1/1.25 and 1/1.5 in float: the level sizes and the resize coefficients come from a rounded inverse."""
    run(gpu_ctx, (1500, scale, 5, 20, 7), "textured", 1000, 700, 25)


# ------------------------------------------------------------------------------------------------ feature counts
def test_nfeatures_zero_returns_the_initial_nodes(gpu_ctx):
    """nfeatures = 0: N = 0 on every level, the outer loop stops after its first pass with size >= N, so each level returns the
    non-empty children of its initial nodes."""
    S, e = run(gpu_ctx, (0, 1.2, 8, 20, 7), "textured", 1241, 376, 26)
    assert np.all(S[:, WANTED] == 0) and np.all(S[:, ITER] == 1) and len(e["octave"]) > 0


def test_nfeatures_one(gpu_ctx):
    """nfeatures = 1: every level but the first wants cvRound of a fraction."""
    S, e = run(gpu_ctx, (1, 1.2, 8, 20, 7), "textured", 1241, 376, 27)
    assert S[:, WANTED].sum() == 1 and len(e["octave"]) > 0


def test_nfeatures_far_above_the_candidate_supply(gpu_ctx):
    """nfeatures = 20000 at 1241x376: on every level with fewer candidates than N (levels 1-7 here) the octree splits until the size
    stops changing and every distinct candidate comes back."""
    S, _ = run(gpu_ctx, (20000, 1.2, 8, 20, 7), "textured", 1241, 376, 28)
    few = S[:, CNT] < S[:, WANTED]
    assert few.sum() >= 7 and np.all(S[few, UNCHANGED] == 1) and np.array_equal(S[few, NKP], S[few, CNT])


def test_panorama_capacity_is_4_nini(gpu_ctx):
    """4000x300 with nfeatures = 100: round(3968/268) = 15 initial nodes, so a level may return 4*nIni = 60 > N + 3 keypoints."""
    params = (100, 1.2, 4, 20, 7)
    assert R.n_ini(4000, 300) == 15
    S, _ = run(gpu_ctx, params, "textured", 4000, 300, 29)
    assert (S[:, NKP] > S[:, WANTED] + 3).any()


# ------------------------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("ini,mn", [(20, 20), (10, 40)], ids=["equal", "min_above_ini"])
def test_threshold_orders(gpu_ctx, ini, mn):
    """ini == min (the retry repeats the same test) and min > ini (the retry is stricter and finds nothing)."""
    S, _ = run(gpu_ctx, (1200, 1.2, 8, ini, mn), "textured", 752, 480, 30)
    assert (S[:, MIN_TH] > 0).any()
    if mn > ini:
        assert np.array_equal(S[:, MIN_TH], S[:, EMPTY])


def test_threshold_one_on_a_busy_image(gpu_ctx):
    """1/1 on pixel noise: the largest candidate counts, no cell falls back."""
    S, _ = run(gpu_ctx, (2000, 1.2, 8, 1, 1), "busy", 1241, 376, 31)
    assert S[0, CNT] > 30000 and np.all(S[:, MIN_TH] == 0)


def test_threshold_255_empties_every_cell(gpu_ctx):
    """255/255: no FAST score reaches 255, every cell falls back and stays empty, and no keypoint comes back."""
    S, e = run(gpu_ctx, (2000, 1.2, 8, 255, 255), "busy", 1241, 376, 32)
    assert len(e["octave"]) == 0 and np.all(S[:, CNT] == 0) and np.all(S[:, MIN_TH] > 0) and np.array_equal(S[:, MIN_TH], S[:, EMPTY])


# ------------------------------------------------------------------------------------------------ scenes
def test_constant_image(gpu_ctx):
    """No candidate at any level: every octree starts from empty initial nodes and returns nothing."""
    S, e = run(gpu_ctx, TUM, "constant", 640, 480, 33)
    assert np.all(S[:, CNT] == 0) and np.all(S[:, EMPTY] > 0) and len(e["octave"]) == 0


def test_one_corner(gpu_ctx):
    """One bright spot: exactly one candidate at level 0, which an initial node keeps on its own (bNoMore at size 1)."""
    S, e = run(gpu_ctx, EUROC, "corner", 752, 480, 34)
    assert S[0, CNT] == 1 and S[0, NKP] == 1


def test_checkerboard(gpu_ctx):
    """5-px squares: runs of equal FAST scores (the first of the greatest response stays) and nodes of equal size in the sorted
    phase (split in reverse creation order)."""
    S, e = run(gpu_ctx, KITTI, "checker", 1241, 376, 35)
    assert S[0, CNT] > 1000 and (S[:, SORTED] > 0).any()
    scores = [sc for _, _, sc in e["candidates"][0]]
    assert len(set(scores)) * 20 < len(scores)


@pytest.mark.parametrize("cols,rows,params", [(1280, 720, KITTI), (1920, 1080, (3000, 1.2, 8, 20, 7)), (4096, 2160, (3000, 1.2, 8, 20, 7))],
                         ids=["720p", "1080p", "4k"])
def test_large_frames(gpu_ctx, cols, rows, params):
    """Frames well above KITTI's size: level 0 has thousands of cells and more initial nodes."""
    S, _ = run(gpu_ctx, params, "textured", cols, rows, 36)
    assert S[0, CNT] > 2000


def test_the_size_that_found_the_candidate_capacity(gpu_ctx):
    """1143x933 on a handle of exactly that size: 37 cells of 31 columns (1147 > 1143) times 31 rows of 30 (930) need more
    candidate slots than the level has pixels.  The handle sized them as cols x rows and refused the image; 4096x2160 above was
    refused the same way."""
    _, _, n_cols, n_rows, w_cell, h_cell = R.level_grid(1143, 933)
    assert n_cols * w_cell * n_rows * h_cell > 1143 * 933
    S, _ = run(gpu_ctx, (1000, 1.2, 1, 20, 7), "textured", 1143, 933, 50)
    assert S[0, CNT] > 1000


# ------------------------------------------------------------------------------------------------ validity boundaries
def _smallest_side(params):
    inv = R.level_tables(*params[:3])["inv_scale"][-1]
    c = 62
    while R.level_size(c, c, inv)[0] < 62:
        c += 1
    return c


def test_smallest_accepted_size_and_one_pixel_less(gpu_ctx):
    """The smallest level-0 size whose last level is exactly 62 px (one FAST cell) is accepted and bit-exact; one pixel less in
    either direction is refused by the device and by the restatement."""
    params = TUM
    c = _smallest_side(params)
    inv = R.level_tables(*params[:3])["inv_scale"][-1]
    assert R.level_size(c, c, inv) == (62, 62)
    S, _ = run(gpu_ctx, params, "textured", c, c, 37)
    assert np.all(S[:, CNT] > 0)
    with ORBextractor(gpu_ctx, *params, PATTERN, max_cols=c, max_rows=c, max_images=1) as ex:
        for cc, rr in ((c - 1, c), (c, c - 1)):
            img = scene("textured", cc, rr, 37)
            assert ex.extract_raw([img])[0] == abi.LLD_ERR_INVALID
            with pytest.raises(ValueError):
                R.extract(img, *params, PATTERN)


def test_ratio_one_half_rounds_to_one_node(gpu_ctx):
    """(cols - 32) / (rows - 32) = 50/100 = 0.5 exactly: std::round gives one initial node (half-to-even would give 0 and be
    refused)."""
    assert R.n_ini(82, 132) == 1 and R.level_ok(82, 132) and not R.level_ok(81, 132)
    S, _ = run(gpu_ctx, (50, 1.2, 1, 20, 7), "busy", 82, 132, 38)
    assert S[0, CNT] > 0


def test_ratio_two_and_a_half_rounds_away_from_zero(gpu_ctx):
    """282x132: 250/100 = 2.5, nIni = 3 (half-to-even would give 2).  With nfeatures = 1 the first split of three initial nodes
    returns up to 12 = 4 nIni keypoints; more than 8 shows the third node."""
    assert R.n_ini(282, 132) == 3
    S, _ = run(gpu_ctx, (1, 1.2, 1, 20, 7), "busy", 282, 132, 39)
    assert 8 < S[0, NKP] <= 12


# ------------------------------------------------------------------------------------------------ batches and inputs
BATCH = [("textured", 1241, 376), ("busy", 752, 480), ("checker", 640, 480), ("textured", 333, 517), ("flat", 701, 263),
         ("corner", 300, 300), ("constant", 1000, 400), ("busy", 400, 250)]


def test_eight_mixed_images_in_one_call(gpu_ctx):
    """max_images = 8, eight sizes and kinds in one call (the mixed batch: each launch covers the largest level of the eight):
    each image equals the restatement, a one-image call, and the pyramid of its own index."""
    params = TUM
    E = [exp(k, c, r, 40 + i, params) for i, (k, c, r) in enumerate(BATCH)]
    with ORBextractor(gpu_ctx, *params, PATTERN, max_cols=1241, max_rows=517, max_images=8) as ex:
        got = ex([img for img, _ in E])
        for i, (g, (_, e)) in enumerate(zip(got, E)):
            check_equal(g, e, ex, i)
        for img, e in E:
            check_equal(ex(img), e, ex, 0)


def test_calls_in_sequence_leave_no_state(gpu_ctx):
    """Large busy, small flat, large textured on one handle: each equals a fresh handle's result, so nothing of a larger earlier
    call (cell counts, octree nodes, pyramid pixels) leaks into a smaller later one."""
    params = KITTI
    seq = [exp("busy", 1241, 376, 41, params), exp("flat", 640, 240, 42, params), exp("textured", 1241, 376, 43, params)]
    with ORBextractor(gpu_ctx, *params, PATTERN, max_cols=1241, max_rows=376, max_images=1) as ex:
        for img, e in seq:
            check_equal(ex(img), e, ex, 0)
    for img, e in seq:
        with ORBextractor(gpu_ctx, *params, PATTERN, max_cols=1241, max_rows=376, max_images=1) as fresh:
            check_equal(fresh(img), e, fresh, 0)


def test_strided_host_image(gpu_ctx):
    """A numpy view big[:, :cols]: the wrapper passes step = strides[0] > cols and the upload reads row by row."""
    img, e = exp("textured", 752, 480, 44, EUROC)
    big = np.full((480, 800), 7, np.uint8); big[:, :752] = img
    view = big[:, :752]
    assert view.strides[0] == 800
    with ORBextractor(gpu_ctx, *EUROC, PATTERN, max_cols=752, max_rows=480, max_images=1) as ex:
        check_equal(ex(view), e, ex, 0)


def test_device_image_with_a_wider_step(gpu_ctx):
    """A device image whose step (1024) is larger than its width (752), the padding filled with another value."""
    import torch
    img, e = exp("busy", 752, 480, 45, EUROC)
    t = torch.full((480, 1024), 255, dtype=torch.uint8, device="cuda:0")
    t[:, :752] = torch.from_numpy(img).to("cuda:0")
    torch.cuda.synchronize()
    with ORBextractor(gpu_ctx, *EUROC, PATTERN, max_cols=752, max_rows=480, max_images=1) as ex:
        check_equal(ex((t.data_ptr(), 752, 480, 1024)), e, ex, 0)


# ------------------------------------------------------------------------------------------------ output capacity
def test_output_capacity_is_exactly_the_header_formula(gpu_ctx):
    """A 3000x250 panorama on a handle sized 4000x300: need = sum of max(N + 3, 4 nIni) over the image's own levels (less than
    max_keypoints); capacity == need is accepted, need - 1 is refused."""
    params = (100, 1.2, 4, 20, 7)
    img, e = exp("textured", 3000, 250, 46, params)
    n = need(params, 3000, 250)
    with ORBextractor(gpu_ctx, *params, PATTERN, max_cols=4000, max_rows=300, max_images=1) as ex:
        assert n < ex.max_keypoints and n > sum(R.level_tables(*params[:3])["per_level"]) + 3 * 4
        assert call(ex, [img], [n - 1]) == abi.LLD_ERR_INVALID
        assert call(ex, [img], [n]) == abi.LLD_OK
        check_equal(ex(img), e, ex, 0)


# ------------------------------------------------------------------------------------------------ pattern reach
def test_pattern_at_plus_minus_13(gpu_ctx):
    """Every pattern coordinate at +-13: at angles near 45 degrees the rotated reads land round(13 sqrt 2) = 18 px from the keypoint,
    one inside EDGE_THRESHOLD."""
    pat = (13 * np.random.default_rng(47).choice([-1, 1], size=(256, 4))).astype(np.int32)
    S, e = run(gpu_ctx, EUROC, "textured", 752, 480, 47, pattern=pat)
    near45 = np.abs((e["angle"] % 90.0) - 45.0) < 1.0
    assert near45.sum() > 5


# ------------------------------------------------------------------------------------------------ a refused call keeps the handle
def _snapshot(ctx, ex, L, Rf, sc):
    pyr = []
    for i in (0, 1):
        lv, cols, rows, step = ex.pyramid(i)
        ptrs = [C.cast(p, C.c_void_p).value for p in lv]
        pix = [download(lv[l], int(rows[l]) * int(step[l])) for l in range(ex.n_levels)]
        pyr.append((ptrs, cols.copy(), rows.copy(), step.copy(), pix))
    desc = [voc.extractor_descriptors(ex, i) for i in (0, 1)]
    desc_pix = [download(p, n * 32) for p, n in desc]
    st = compute_stereo_matches_device(ctx, L, Rf, ex, sc["mb"], sc["mbf"])
    return pyr, desc, desc_pix, st


def test_a_refused_call_leaves_the_last_pyramid_and_descriptors(gpu_ctx):
    """After each kind of refusal (a bad image after a valid one of another size, a bad first image that fails at a deep level, an
    image wider than max_cols, a null image, too small an output capacity) the pyramid and descriptor getters return exactly what
    the last successful call returned, and the stereo hand-off on them is unchanged."""
    sc = synth.make_stereo_scene(0)
    left, right = sc["left"][0], sc["right"][0]
    small, bad_deep = scene("textured", 640, 300, 48), np.zeros((120, 400), np.uint8)
    with ORBextractor(gpu_ctx, *KITTI, PATTERN, max_cols=1241, max_rows=376, max_images=2) as ex:
        L, Rf = ex([left, right])
        before = _snapshot(gpu_ctx, ex, L, Rf, sc)
        assert before[3].n_matches > 20
        cap = ex.max_keypoints
        refusals = [([small, bad_deep], [cap, cap]),                               # image 1 refused after a valid 640x300 image 0
                    ([bad_deep, small], [cap, cap]),                               # level 7 of image 0 is too small
                    ([small, np.zeros((376, 1242), np.uint8)], [cap, cap]),        # wider than max_cols
                    ([small, None], [cap, cap]),                                   # null pixels
                    ([small, small], [cap, need(KITTI, 640, 300) - 1])]             # output capacity one short
        for images, caps in refusals:
            assert call(ex, images, caps) == abi.LLD_ERR_INVALID
            after = _snapshot(gpu_ctx, ex, L, Rf, sc)
            for (p0, c0, r0, s0, x0), (p1, c1, r1, s1, x1) in zip(before[0], after[0]):
                assert p0 == p1 and np.array_equal(c0, c1) and np.array_equal(r0, r1) and np.array_equal(s0, s1)
                assert all(np.array_equal(a, b) for a, b in zip(x0, x1))
            assert before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(before[2], after[2]))
            for f in ("u_right", "depth", "best_r", "sad"):
                assert np.array_equal(getattr(before[3], f), getattr(after[3], f)), f
            assert before[3].n_matches == after[3].n_matches


# ------------------------------------------------------------------------------------------------ hand-offs at other geometry
@pytest.mark.parametrize("n_levels", [1, 4])
def test_stereo_hand_off_at_scale_1_5(gpu_ctx, n_levels):
    """compute_stereo_matches_device on the extractor's own pyramid with 1 or 4 levels at scale 1.5 (level sizes and inverse
    scales the KITTI tables never give), against oracle_orbsearch.compute_stereo_matches on the restatement's pyramid."""
    params = (2000, 1.5, n_levels, 20, 7)
    sc = synth.make_stereo_scene(0)
    left, right = sc["left"][0], sc["right"][0]
    with ORBextractor(gpu_ctx, *params, PATTERN, max_cols=1241, max_rows=376, max_images=2) as ex:
        L, Rf = ex([left, right])
        el, er = R.extract(left, *params, PATTERN), R.extract(right, *params, PATTERN)
        check_equal(L, el, ex, 0); check_equal(Rf, er, ex, 1)
        dev = compute_stereo_matches_device(gpu_ctx, L, Rf, ex, sc["mb"], sc["mbf"])
        host = ORBmatcher(gpu_ctx).ComputeStereoMatchesFull(L, Rf, el["levels"], er["levels"], ex.inv_scale_factors, sc["mb"], sc["mbf"])
        n, ur, dep, br, sad = OS.compute_stereo_matches(L, Rf, el["levels"], er["levels"], ex.inv_scale_factors, sc["mb"], sc["mbf"])
    assert dev.n_matches == host.n_matches == n and n > 20
    for f, e in (("u_right", ur), ("depth", dep), ("best_r", br), ("sad", sad)):
        assert np.array_equal(getattr(dev, f), getattr(host, f)) and np.array_equal(getattr(dev, f), e), f


def test_bow_hand_off_at_other_parameters(gpu_ctx):
    """The device descriptors of a (1000, 1.5, 4, 12, 5) extraction go straight into lld_bow_transform (on_device = 1) and equal
    bow_ref.transform of the restatement's descriptors."""
    params = (1000, 1.5, 4, 12, 5)
    img, e = exp("textured", 752, 480, 49, params)
    V = B.make_vocab(21, k=7, L=6, p_full=0.3, p_early_leaf=0.12, p_stop=0.05, order="dfs")
    with ORBextractor(gpu_ctx, *params, PATTERN, max_cols=752, max_rows=480, max_images=1) as ex, \
            voc.ORBVocabulary.from_arrays(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], V["scoring"],
                                          V["weighting"]) as v:
        check_equal(ex(img), e, ex, 0)
        ptr, n = voc.extractor_descriptors(ex, 0)
        assert n == len(e["desc"]) > 500
        got = v.transform((ptr, n))
        ref = B.transform(B.Tree(V), e["desc"], 4)
    for f in ("word", "node", "node_start", "feature", "feature_word", "feature_nid"):
        assert np.array_equal(np.asarray(getattr(got, f)), ref[f]), f
    assert np.array_equal(got.value.view(np.uint64), ref["value"].view(np.uint64))
