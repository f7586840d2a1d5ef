"""The crafted stereo scenes (tests/stereo_scenes.py) do what they claim - proved here from the oracle alone, by the exit census of
oracle_orbsearch.compute_stereo_matches(..., want_exits=True).  No GPU.

The one exit of Frame::ComputeStereoMatches without a scene is `deltaR < -1 || deltaR > 1` (src/Frame.cc:672): dist2 is the FIRST strict
minimum of the eleven distances, so dist1 > dist2 and dist3 >= dist2, the denominator 2 * (dist1 + dist3 - 2 * dist2) is positive and
|deltaR| <= 0.5.  The census gives it code 13, and test_every_exit_occurs asserts that it never shows."""
import numpy as np
import pytest

import oracle_orbsearch as OS
import stereo_scenes as S

KEPT = (10, 11)
_cache = {}


def run(name):
    """(scene, left Frame, right Frame, oracle result with the census); computed once per scene, never changed."""
    if name not in _cache:
        sc = S.SCENES[name]()
        L, R = S.frames(sc)
        _cache[name] = (sc, L, R, OS.compute_stereo_matches(L, R, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"], want_exits=True))
    return _cache[name]


def exits_of(name, tag):
    sc, _, _, ref = run(name)
    return ref[5][np.array(sc["tags"][tag])]


@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_reaches_the_exits_it_names(name):
    sc, L, R, (n, ur, dep, br, sad, ex) = run(name)
    assert sc["name"] == name and L.n <= 600 and R.n <= 600 and L.n == ex.shape[0]
    count = np.bincount(ex, minlength=14)
    assert count[0] == 0 and count[13] == 0 and count.sum() == L.n, count
    for code in sc["exits"]:
        assert count[code] >= 3, f"{name}: exit {code} taken by {count[code]} left keypoints; census {count[1:13]}"
    # the census agrees with the outputs
    kept = np.isin(ex, KEPT)
    assert np.array_equal(ur >= 0, kept) and np.array_equal(dep > 0, kept) and n == int(kept.sum())
    assert np.array_equal(sad >= 0, np.isin(ex, KEPT + (12,))) and np.array_equal(br >= 0, ex >= 6)
    # determinism: a second build gives the same bytes
    again = S.SCENES[name]()
    for k in ("l_xy", "l_desc", "r_xy", "r_desc"):
        assert np.array_equal(again[k], sc[k])
    assert all(np.array_equal(a, b) for a, b in zip(again["right"], sc["right"]))


def test_every_exit_occurs():
    total = sum(np.bincount(run(name)[3][5], minlength=14) for name in S.SCENES)
    assert np.all(total[1:13] >= 3) and total[0] == 0 and total[13] == 0, total


def test_census_is_a_by_product():
    sc, L, R, ref = run("shifts")
    plain = OS.compute_stereo_matches(L, R, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    assert len(plain) == 5 and plain[0] == ref[0]
    for a, b in zip(plain[1:], ref[1:5]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_tall_matches_below_row_512():
    sc, L, R, (n, ur, dep, br, sad, ex) = run("tall")
    assert sc["left"][0].shape == (720, 160) and len(sc["left"]) == 8
    rows = L.xy[:, 1].astype(np.int64)
    assert rows.min() == 0 and rows.max() == 719 and set(range(500, 526)) <= set(rows.tolist())
    kept = np.isin(ex, KEPT)
    assert int((R.xy[br[kept], 1] >= 512).sum()) >= 20
    for o in range(8):                                                         # every octave has right keypoints at y >= 512
        assert np.any((R.octave == o) & (R.xy[:, 1] >= 512))
    across = np.array(sc["tags"]["across"])                                    # left row <= 511, its right keypoint at y >= 512
    hit = across[br[across] >= 0]
    assert hit.size >= 8 and np.all(L.xy[hit, 1] < 512) and np.all(R.xy[br[hit], 1] >= 512)


def test_level_counts():
    for name, n_levels, scale1 in (("levels_1", 1, None), ("levels_3", 3, 1.2), ("levels_16", 16, 1.1)):
        sc, L, R, ref = run(name)
        assert len(sc["left"]) == n_levels == L.scale.shape[0] and (scale1 is None or L.scale[1] == np.float32(scale1))
        assert set(L.octave.tolist()) == set(range(n_levels))
    sc, L, R, ref = run("levels_16")
    assert 8190 // 16 == 511 and int((R.xy[:, 1] >= 511).sum()) >= 50 and sc["left"][0].shape[0] == 540
    top0 = exits_of("levels_3", "top_0")                                       # octave 2 against a left octave 0: the gate, whatever else is in the row
    assert np.all(np.isin(top0, (4, 5))) and int((top0 == 4).sum()) >= 3 and np.all(np.isin(exits_of("levels_3", "top_1"), KEPT)) and np.all(np.isin(exits_of("levels_3", "top_2"), KEPT))


def test_patch_limits_pairs_part():
    sc, L, R, (n, ur, dep, br, sad, ex) = run("patch_limits")
    assert len(sc["pairs"]) == 5 * 4
    want_out = dict(xr=7, endu=6, x0_high=7, y0_low=7, y0_high=7)
    for what, level, inside, outside in sc["pairs"]:
        assert ex[inside] in KEPT and ex[outside] == want_out[what], (what, level, ex[inside], ex[outside])
    assert np.all(exits_of("patch_limits", "x0_low") == 7)                     # shadowed by xr - 10 >= 0, see the scene
    half = exits_of("patch_limits", "half")
    assert np.all(np.isin(half[:6], KEPT)) and half[6] == 7


def test_shifts_take_every_bestincR():
    for e in range(-6, 7):
        got = exits_of("shifts", "e%+d" % e)
        if abs(e) == 5:
            assert np.all(got == 8), (e, got)
        elif abs(e) < 5:
            assert np.all(np.isin(got, KEPT + (12,))), (e, got)
    assert np.all(np.isin(exits_of("shifts", "d74"), KEPT + (12,))) and np.all(exits_of("shifts", "d75") == 5)


def test_zero_and_max_disparity():
    sc, L, R, (n, ur, dep, br, sad, ex) = run("zero_disparity")
    zero = np.array(sc["tags"]["zero"])
    assert np.all(ex[zero] == 10) and np.all(sad[zero] == 0)
    assert np.array_equal(ur[zero], (L.xy[zero, 0].astype(np.float64) - 0.01).astype(np.float32))
    assert np.all(dep[zero] == np.float32(sc["mbf"]) / np.float32(0.01))
    sc, L, R, (n, ur, dep, br, sad, ex) = run("max_disparity")
    assert np.float32(sc["mbf"]) / np.float32(sc["mb"]) == 8.0
    assert np.all(exits_of("max_disparity", "below") == 4) and np.all(br[np.array(sc["tags"]["at"])] >= 0) and np.all(br[np.array(sc["tags"]["above"])] >= 0)
    reached = np.concatenate([exits_of("max_disparity", "at"), exits_of("max_disparity", "above")])
    assert int((reached == 9).sum()) >= 3 and int(np.isin(reached, KEPT).sum()) >= 3


def test_saturated_median():
    sc, L, R, (n, ur, dep, br, sad, ex) = run("saturated")
    pushed = np.sort(sad[sad >= 0])
    assert pushed.size >= 20 and pushed[0] > 2 ** 15 and pushed[pushed.size // 2] >= 32768 and pushed[-1] <= 121 * 510
    assert np.unique(pushed >> 8).size >= 5                                    # several bins of the radix select's first level


def test_median_cuts():
    for name, pushed, kept in (("median_1", [30], 1), ("median_2", [20, 50], 2), ("median_3", [20, 30, 70], 2), ("median_equal", [25] * 24, 24),
                               ("median_zero", [0] * 24, 0)):
        sc, L, R, (n, ur, dep, br, sad, ex) = run(name)
        assert sorted(sad[sad >= 0].tolist()) == pushed and n == kept, (name, sad[sad >= 0], n)
    assert 50 >= 2.1 * 20                                                      # median_2: the lower median would cut the 50


def test_row_outside():
    sc, L, R, (n, ur, dep, br, sad, ex) = run("row_outside")
    assert np.all(exits_of("row_outside", "below") == 1) and np.all(exits_of("row_outside", "above") == 1)
    assert np.all(exits_of("row_outside", "row0") == 7) and np.all(br[np.array(sc["tags"]["row0"])] >= 0)
    assert np.all(exits_of("row_outside", "empty_row") == 2) and np.all(exits_of("row_outside", "left_of_image") == 3)
    # the literal row test (no bounds check) would have found a candidate for these: a right keypoint of the same octave whose band holds the row
    for tag in ("below", "above"):
        for iL in sc["tags"][tag][:5 if tag == "above" else 4]:
            row = int(L.xy[iL, 1]); r = 2.0 * L.scale[R.octave[iL]]
            assert np.floor(R.xy[iL, 1] - r) <= row <= np.ceil(R.xy[iL, 1] + r)


def test_group_sizes():
    assert [run("groups_%d" % k)[1].n for k in S.GROUP_SIZES] == [1, 15, 16, 17, 255, 257]
