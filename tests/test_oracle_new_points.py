"""tests/newpoints_ref.py against hand-computed answers, against the points that generated its scenes, and its closed-form stereo
parallax cosine against the float libm chain; and the coverage condition the GPU tests rely on.  CPU only.

Recovery bar: on the noise-free scenes below (seeds 21, 22, 23: 3 x 6 x 200 matches) the worst |x3d - X| / |X - Ow1| over the
created points was measured at 8.7e-6 (float keypoints a few hundred pixels from the principal point carry 3e-5 px of rounding,
which small-parallax triangulations amplify).  The bar is 4 times that, 3.5e-5, to cover other seeds."""
import numpy as np
import pytest

import newpoints_ref as R
from newpoints_scenes import SEEDED, crafted, scene

RECOVERY_MEASURED = 8.7e-6
RECOVERY_BAR = 3.5e-5


def test_hand_computed_answer_for_every_status_and_source():
    seen_status, seen_source = set(), set()
    for pb, r, st, src, x in crafted():
        assert r["status"].tolist() == st
        assert r["source"].tolist() == src
        for i, X in x.items():
            assert np.allclose(r["x3d"][i], X, rtol=0, atol=2e-5), (i, r["x3d"][i])
        assert np.all(r["x3d"][r["status"] != R.NEW] == 0)
        seen_status |= set(st)
        seen_source |= {s for s, t in zip(src, st) if t == R.NEW}
    assert seen_status == set(range(11)) and seen_source == {0, 1, 2}
    pb, r = crafted()[0][:2]
    assert r["pair_status"].tolist() == [0, 0, 0, 0, 1] and r["n_new"].tolist() == [0, 1, 0, 2, 0]
    assert r["new_match"].tolist() == [1, 9, 10] and r["n_new_total"] == 3


def test_u2r_uses_the_current_keyframes_mbf():
    # match 9 of the crafted scene is a stereo keypoint of the neighbour; with another mbf on the NEIGHBOUR nothing changes,
    # with another mbf on keyframe 1 its right-image error appears (:407)
    pb = R.crafted_scenes()[0][0]
    base = R.triangulate(pb)["status"]
    pb["kf2"][3] = dict(pb["kf2"][3], mbf=np.float32(999.0))
    assert np.array_equal(R.triangulate(pb)["status"], base)
    pb["kf1"] = dict(pb["kf1"], mbf=np.float32(300.0))
    assert R.triangulate(pb)["status"][9] == R.REPROJ2


def test_both_stereo_computes_only_the_first_cosine():
    # :312-315: with both keypoints stereo cosParallaxStereo2 stays cosParallaxRays+1, so the neighbour's depth is never read
    pb = R.crafted_scenes()[0][0]
    ks = pb["key_start"][3]
    pb["keys2"]["ur"][ks + 1] = 600.0                                           # match 10: the neighbour's keypoint becomes stereo ..
    a = R.triangulate(pb)
    pb["keys2"]["depth"][ks + 1] = 0.01                                         # .. and its depth (a tiny one) changes nothing but u2_r
    b = R.triangulate(pb)
    assert a["source"][10] == b["source"][10] == R.SRC_STEREO1 and np.array_equal(a["x3d"][10], b["x3d"][10])


def test_noise_free_scenes_recover_the_generating_points():
    worst = 0.0
    for seed in (21, 22, 23):
        pb = R.make_scene(seed, [200] * 6, noise=0.0, p_outlier=0.0, p_octave=0.0, p_no_depth=0.0, p_stereo=0.0, enforce_margin=False)
        r = R.triangulate(pb)
        new = np.flatnonzero(r["status"] == R.NEW)
        assert len(new) > 600
        X = pb["X"][pb["matches"][new, 0]]
        Ow1 = R.derived(pb["kf1"])[1].astype(np.float64)
        worst = max(worst, float(np.max(np.linalg.norm(r["x3d"][new] - X, axis=1) / np.linalg.norm(X - Ow1, axis=1))))
    print("worst relative recovery error %.3g (bar %.3g)" % (worst, RECOVERY_BAR))
    assert worst <= RECOVERY_BAR


def test_closed_form_cosine_against_the_float_libm_chain():
    rng = np.random.default_rng(5)
    depth = np.exp(rng.uniform(np.log(0.3), np.log(300.0), 20000)).astype(np.float32)
    mb = np.float32(0.54)
    closed = R.cos_stereo(mb, depth)
    chain = np.cos(np.float32(2.0) * np.arctan2(mb / np.float32(2.0), depth)).astype(np.float32)
    exact = np.cos(2.0 * np.arctan2(np.float64(mb / np.float32(2.0)), depth.astype(np.float64)))
    assert np.array_equal(closed, exact.astype(np.float32))                     # the closed form is the correctly rounded value
    # the chain: numpy's float32 arctan2 and cos are each within 4 ulp (its documented bound for the vectorised float routines), the
    # doubling is exact; the closed form is within half an ulp
    theta = np.arctan2(np.float64(mb / np.float32(2.0)), depth.astype(np.float64))
    bound = np.abs(np.sin(2 * theta)) * 2 * 4 * np.spacing(theta.astype(np.float32)).astype(np.float64) + 4.5 * np.spacing(np.abs(closed))
    assert np.all(np.abs(chain.astype(np.float64) - closed) <= bound)
    assert np.max(np.abs(chain.astype(np.float64) - closed)) < 6e-7


def test_statuses_agree_with_the_libm_chain_beyond_two_ulp(monkeypatch):
    chain = lambda mb, d: np.cos(np.float32(2.0) * np.arctan2(np.float32(mb) / np.float32(2.0), np.asarray(d, np.float32))).astype(np.float32)
    checked = 0
    for name in ("stereo10", "skipped_second"):
        pb, r = scene(name)
        with monkeypatch.context() as m:
            m.setattr(R, "cos_stereo", chain)
            with np.errstate(all="ignore"):
                alt = R.triangulate(pb)
        far = np.abs(r["cos_rays"].astype(np.float64) - r["cos_stereo"]) > 2 * np.spacing(np.abs(r["cos_stereo"]))
        assert np.array_equal(alt["status"][far], r["status"][far]) and np.array_equal(alt["source"][far], r["source"][far])
        run = r["status"] != R.PAIR_SKIPPED
        assert far[run].sum() >= 0.99 * run.sum()                               # the condition leaves almost every match in
        checked += int(far[run].sum())
    assert checked > 2000


def test_coverage_condition():
    """Every status and source occurs over the fixed scenes, and no match is within 1e-5 of a threshold."""
    status, source = set(), set()
    for entry in [scene(n) for n in SEEDED] + [c[:2] for c in crafted()]:
        pb, r = entry
        assert np.all(R.margins(pb) > R.MARGIN)
        status |= set(r["status"].tolist())
        source |= set(r["source"][r["status"] == R.NEW].tolist())
    assert status == set(range(11)) and source == {0, 1, 2}


def test_seeded_scenes_have_the_shapes_their_names_promise():
    pb, r = scene("skipped_second")
    assert r["pair_status"].tolist() == [0, 1, 0, 0] and r["n_new"][1] == 0 and r["n_new"][2] > 0
    assert np.all(r["status"][pb["match_start"][1]:pb["match_start"][2]] == R.PAIR_SKIPPED)
    pb, r = scene("empty_middle")
    assert pb["match_start"].tolist() == [0, 70, 70, 160] and r["n_new"][1] == 0
    pb, r = scene("mono20")
    assert np.all(pb["keys1"]["ur"] < 0) and np.all(pb["keys2"]["ur"] < 0) and 1 in r["pair_status"].tolist()
    pb, r = scene("stereo10")
    m = pb["matches"]; ks = np.repeat(pb["key_start"][:-1], np.diff(pb["match_start"]))
    s1 = pb["keys1"]["ur"][m[:, 0]] >= 0; s2 = pb["keys2"]["ur"][ks + m[:, 1]] >= 0
    assert (s1 & s2).sum() > 100 and (s1 ^ s2).sum() > 100 and (~s1 & ~s2).sum() > 100
