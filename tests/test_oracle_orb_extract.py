"""Known answers and invariants of the CPU restatement of ORBextractor::operator() (tests/orb_extract_ref.py), the level tables, and
the ctypes mirrors of the lld_orb_extract structs.  No GPU needed."""
import ctypes
import math
import os
import subprocess

import numpy as np

import orb_extract_ref as R
from lld_slam_amd import orb_extractor as OX
from lld_slam_amd.orb_search import orb_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fast_score_known_answers():
    p = np.full((7, 7), 100, np.uint8)
    assert R.fast_score_patch(p) < 1                                  # flat: no corner at any threshold
    q = p.copy()
    arc = R.CIRCLE[:9]
    for dx, dy in arc:
        q[3 + dy, 3 + dx] = 140                                       # 9 contiguous pixels 40 brighter
    assert R.fast_score_patch(q) == 39
    q[3 + arc[4][1], 3 + arc[4][0]] = 125                             # the weakest of the nine decides
    assert R.fast_score_patch(q) == 24
    d = p.copy()
    for dx, dy in R.CIRCLE[5:14]:
        d[3 + dy, 3 + dx] = 70                                        # dark arc
    assert R.fast_score_patch(d) == 29
    e = p.copy()
    for dx, dy in R.CIRCLE[:8]:
        e[3 + dy, 3 + dx] = 200                                       # 8 contiguous: not a FAST-9 corner
    assert R.fast_score_patch(e) < 1
    # the map agrees with the patch form
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (20, 24)).astype(np.uint8)
    sm = R.fast_score_map(img)
    for y in range(3, 17):
        for x in range(3, 21):
            assert sm[y, x] == max(R.fast_score_patch(img[y - 3:y + 4, x - 3:x + 4]), 0)


def test_resize_and_blur_keep_a_constant_image():
    img = np.full((97, 131), 173, np.uint8)
    assert np.all(R.resize_linear(img, 109, 81) == 173)
    assert np.all(R.blur(img) == 173)
    assert R.GAUSS_Q8.sum() == 256 and np.array_equal(R.GAUSS_Q8, R.GAUSS_Q8[::-1])


def test_resize_of_a_ramp_is_the_ramp_at_the_source_coordinate():
    x = np.arange(240)
    img = np.tile(x.astype(np.uint8), (10, 1))
    out = R.resize_linear(img, 200, 10)
    src = (np.arange(200) + 0.5) * 1.2 - 0.5
    assert np.max(np.abs(out[0].astype(float) - np.clip(src, 0, 239))) <= 0.51


def test_ic_angle_of_a_ramp():
    umax = R.level_tables(2000, 1.2, 8)["umax"]
    yy, xx = np.mgrid[0:41, 0:41]
    for ang in (0.0, 30.0, 100.0, 200.0, 300.0):
        a = math.radians(ang)
        img = np.clip(128 + 3 * ((xx - 20) * math.cos(a) + (yy - 20) * math.sin(a)), 0, 255).astype(np.uint8)
        m01, m10 = R.ic_angle(img, 20, 20, umax)
        got = float(R.fast_atan2(np.float32(m01), np.float32(m10)))
        assert abs((got - ang + 180) % 360 - 180) < 1.0


def test_fast_atan2_is_within_0_3_degrees():
    rng = np.random.default_rng(2)
    y, x = rng.normal(size=(2, 20000)).astype(np.float32) * 1000
    got = R.fast_atan2(y, x)
    ref = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360
    assert np.all((got >= 0) & (got < 360))
    assert np.max(np.abs((got - ref + 180) % 360 - 180)) < 0.3


def test_level_tables_match_orb_levels_and_hand_computation():
    T = R.level_tables(2000, 1.2, 8)
    scale, sigma2, inv_sigma2 = orb_levels(1.2, 8)
    assert np.array_equal(T["scale"], scale) and np.array_equal(T["sigma2"], sigma2) and np.array_equal(T["inv_sigma2"], inv_sigma2)
    # nDesired = 2000 (1 - 1/1.2) / (1 - 1.2^-8) = 434.5..., then *= 1/1.2 per level, cvRound each, remainder to the last
    assert T["per_level"].tolist() == [434, 362, 302, 251, 209, 175, 145, 122]
    assert T["per_level"].sum() == 2000
    assert T["umax"].tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def _cands(rng, n, w, h):
    return [(int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(1, 60))) for _ in range(n)]


def test_octree_invariants():
    rng = np.random.default_rng(3)
    W, H = 1209, 344
    for n, N in [(3000, 434), (800, 300), (5000, 40), (200, 122)]:
        c = _cands(rng, n, W, H)
        st = {}
        out = R.distribute_oct_tree(c, 16, 16 + W, 16, 16 + H, N, st)
        assert len(out) <= max(N + 3, 4 * round(W / H))
        cs = set(c)
        assert all(o in cs for o in out)
        assert len(set(out)) == len(out)


def test_octree_returns_every_distinct_candidate_when_few():
    rng = np.random.default_rng(4)
    pts = set()
    while len(pts) < 150:
        pts.add((int(rng.integers(0, 1209)), int(rng.integers(0, 344))))
    c = [(x, y, int(rng.integers(1, 50))) for x, y in sorted(pts, key=lambda p: (p[1], p[0]))]
    st = {}
    out = R.distribute_oct_tree(c, 16, 1225, 16, 360, 434, st)
    assert sorted(out) == sorted(c) and st["finish_unchanged"] == 1


def test_octree_keeps_the_first_of_the_greatest_response():
    # two candidates in one node after one split, equal responses: the earlier one stays
    c = [(10, 10, 30), (11, 10, 30), (12, 11, 29), (700, 300, 5)]
    out = R.distribute_oct_tree(c, 16, 1225, 16, 360, 2, {})
    assert (10, 10, 30) in out and (11, 10, 30) not in out


def test_octree_reduces_a_duplicate_pair_to_one():
    c = [(100, 50, 20), (100, 50, 25), (900, 200, 7)]
    st = {}
    out = R.distribute_oct_tree(c, 16, 1225, 16, 360, 434, st)
    assert sorted(out) == [(100, 50, 25), (900, 200, 7)] and st["finish_unchanged"] == 1


def test_sorted_phase_ties_split_the_later_created_node_first():
    # four quadrant clusters of equal size; N lets the sorted phase split only one of them
    c = []
    for qx, qy in [(100, 50), (900, 50), (100, 300), (900, 300)]:
        c += [(qx, qy, 5), (qx + 40, qy + 20, 6)]
    st = {}
    out = R.distribute_oct_tree(c, 16, 16 + 1209, 16, 16 + 1209, 5, st)
    assert st["sorted_rounds"] >= 1 and len(out) >= 5


def test_pattern_helper_range():
    p = R.seeded_pattern(0)
    assert p.shape == (256, 4) and p.min() >= -13 and p.max() <= 12


def test_struct_layouts_match_the_header(tmp_path):
    names = [("lld_orb_extractor_params", OX.OrbExtractorParams), ("lld_orb_extractor_levels", OX.OrbExtractorLevels),
             ("lld_orb_image", OX.OrbImage), ("lld_orb_level_stats", OX.OrbLevelStats), ("lld_orb_features", OX.OrbFeatures)]
    body = "".join(f'printf("%zu\\n", sizeof({n}));' for n, _ in names)
    probes = [(n, c, f) for n, c in names for f, _ in c._fields_]
    body += "".join(f'printf("%zu\\n", offsetof({n}, {f}));' for n, _, f in probes)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(c) for _, c in names] + [getattr(c, f).offset for _, c, f in probes]


def test_glibc_sincosf_restatement_matches_libm_on_a_sample(tmp_path):
    """tools/check_sincosf.c compiles the device's sinf / cosf restatement on the host; here over a seeded sample of angles
    (the tool itself walks every float angle in [0, 360))."""
    exe = tmp_path / "chk"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "lld_slam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "check_sincosf.c"), "-o", str(exe), "-lm"])
    out = subprocess.check_output([str(exe), "997"]).decode()
    assert "cos_diff 0 sin_diff 0" in out, out


def test_level_tables_at_one_and_sixteen_levels_and_scale_2():
    T = R.level_tables(1000, 1.2, 1)                                  # one level: nothing divided, every feature on level 0
    assert T["scale"].tolist() == [1.0] and T["inv_scale"].tolist() == [1.0] and T["per_level"].tolist() == [1000]
    T = R.level_tables(1000, 2.0, 4)                                  # powers of two are exact in float
    assert T["scale"].tolist() == [1, 2, 4, 8] and T["inv_scale"].tolist() == [1, 0.5, 0.25, 0.125]
    assert T["sigma2"].tolist() == [1, 4, 16, 64] and T["inv_sigma2"].tolist() == [1, 0.25, 0.0625, 0.015625]
    # nDesired = 1000 (1 - 1/2) / (1 - 2^-4) = 533.3, then 266.7, 133.3: cvRound each, the remainder 67 to the last level
    assert T["per_level"].tolist() == [533, 267, 133, 67]
    T = R.level_tables(2000, 1.05, 16)
    s = [1.0]
    for _ in range(15):
        s.append(float(np.float32(np.float32(s[-1]) * np.float32(1.05))))
    assert T["scale"].tolist() == s and abs(s[-1] - 1.05 ** 15) < 1e-5
    f = 1 / 1.05
    nd = 2000 * (1 - f) / (1 - f ** 16)                               # 129.2, 123.1, ... in double: float rounding moves none of them
    assert T["per_level"][:15].tolist() == [round(nd * f ** l) for l in range(15)]
    assert T["per_level"].sum() == 2000 and T["per_level"][15] == 2000 - sum(round(nd * f ** l) for l in range(15))


def test_level_size_rounds_ties_to_even():
    """cvRound((float)cols * inv): an exact .5 goes to the even neighbour, down or up."""
    assert R.level_size(701, 525, np.float32(0.5)) == (350, 262)       # 350.5, 262.5 -> down
    assert R.level_size(703, 527, np.float32(0.5)) == (352, 264)       # 351.5, 263.5 -> up
    assert R.level_size(701, 525, np.float32(0.125)) == (88, 66)       # 87.625, 65.625: no tie
    assert R.level_size(6, 10, np.float32(0.25)) == (2, 2)             # 1.5 -> 2, 2.5 -> 2


def test_size_limits_are_the_headers():
    """62 px is the smallest level side with one FAST cell; round((cols - 32) / (rows - 32)) must be >= 1.  extract() accepts
    exactly the images image_ok() accepts."""
    assert R.level_ok(62, 62) and not R.level_ok(61, 62) and not R.level_ok(62, 61)
    T = R.level_tables(1000, 1.2, 8)
    inv = T["inv_scale"][-1]
    c = next(c for c in range(62, 400) if R.level_size(c, c, inv)[0] >= 62)
    assert R.level_size(c, c, inv) == (62, 62) and R.level_size(c - 1, c - 1, inv)[0] == 61
    assert R.image_ok(c, c, T) and not R.image_ok(c - 1, c, T) and not R.image_ok(c, c - 1, T)
    pat = R.seeded_pattern(0)
    for cols, rows in [(c, c), (c - 1, c), (c, c - 1), (c + 1, 2 * c), (c, 2 * c + 200), (400, 120), (640, 200)]:
        img = np.full((rows, cols), 9, np.uint8)
        if R.image_ok(cols, rows, T):
            R.extract(img, 1000, 1.2, 8, 20, 7, pat)
        else:
            try:
                R.extract(img, 1000, 1.2, 8, 20, 7, pat)
                raise AssertionError(f"{cols}x{rows} accepted")
            except ValueError:
                pass


def test_n_ini_rounds_halves_away_from_zero():
    """std::round in DistributeOctTree: (cols - 32) / (rows - 32) = k + 0.5 gives k + 1 (half-to-even would give k for even k)."""
    assert [R.n_ini(32 + w, 132) for w in (50, 150, 250, 350, 49, 51)] == [1, 2, 3, 4, 0, 1]
    assert R.level_ok(82, 132) and not R.level_ok(81, 132)
    st = {}                                     # three initial nodes over 250 px keep 80 and 90 apart; two would share one child
    out = R.distribute_oct_tree([(80, 5, 9), (90, 5, 9), (240, 5, 9)], 16, 266, 16, 116, 1, st)
    assert len(out) == 3 and st["iterations"] == 1
