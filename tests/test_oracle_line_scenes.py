"""CPU: the crafted line scenes of line_scenes.py are held to the properties they are named after, and the compiled oracle
(oracle/lldo_linematch.cpp) is held to the plain numpy reference of line_ref.py on every one of them.  No GPU."""
import numpy as np
import pytest

import line_ref as LR
import line_scenes as LS

# measured with sweeps_to_fixed_point: (Jacobi sweeps until no pick changes, lines that need more than their 8 best candidates)
GREEDY_PROPERTIES = {
    ("groups", 1): (2, 0), ("groups", 2): (3, 0), ("groups", 6): (7, 0), ("groups", 7): (8, 0), ("groups", 8): (9, 0), ("groups", 9): (10, 70),
    ("groups", 12): (13, 280), ("ladder",): (303, 592),
    ("ties", "lanes"): (12, 4), ("ties", "cut9"): (11, 3), ("ties", "cut10"): (12, 4), ("ties", "cut73"): (75, 67), ("ties", "lead5"): (16, 8),
    ("ties", "gated"): (10, 3), ("threshold",): (2, 0),
    ("edge", 1, 40): (2, 0), ("edge", 40, 1): (3, 0), ("edge", 30, 5): (4, 0), ("edge", 100, 63): (9, 42), ("edge", 100, 64): (10, 43),
    ("edge", 100, 65): (8, 38), ("edge", 255, 90): (12, 174), ("edge", 256, 90): (11, 177), ("edge", 257, 90): (11, 178), ("edge", 513, 65): (9, 442),
}


@pytest.mark.parametrize("name", LS.GREEDY_NAMES, ids=lambda n: "-".join(map(str, n)))
def test_greedy_scene_properties_and_oracle(oracle, name):
    s, D, ref = LS.greedy_scene(name)
    m, d = oracle.line_match_greedy(s["dl"], s["dr"], s["gate"], s["tau"])
    np.testing.assert_array_equal(m, ref)
    np.testing.assert_array_equal(d[ref >= 0], D[np.flatnonzero(ref >= 0), ref[ref >= 0]])
    sweeps, fixed, beyond = LR.sweeps_to_fixed_point(D, s["tau"], s["gate"])
    np.testing.assert_array_equal(fixed, ref)                               # the fixed point of the sweeps is the sequential answer
    assert (sweeps, beyond) == GREEDY_PROPERTIES[name]
    assert len(set(ref[ref >= 0])) == (ref >= 0).sum()


def test_greedy_scenes_cover_what_they_claim():
    # both sides of the device's cap of 8 rounds, with and without lines beyond the 8-entry list
    sw = {g: GREEDY_PROPERTIES[("groups", g)] for g in LS.GROUP_SIZES}
    assert [sw[g][0] for g in LS.GROUP_SIZES] == [2, 3, 7, 8, 9, 10, 13] and sw[8][1] == 0 and sw[9][1] == 70 and sw[12][1] == 280
    # groups: the k-th line of a group ends on the right line at distance k
    s, D, ref = LS.greedy_scene(("groups", 12))
    np.testing.assert_array_equal(D[np.arange(840), ref], np.arange(840) // 70)
    # ladder: j -> j up to 300, nothing after; three chunks of 256 lines, every line from the 9th on beyond its list
    s, D, ref = LS.greedy_scene(("ladder",))
    np.testing.assert_array_equal(ref, np.where(np.arange(600) <= 300, np.arange(600), -1))
    # ties on the lanes: the ten equal lines are handed out in ascending index, whatever lane they sit on
    s, D, ref = LS.greedy_scene(("ties", "lanes"))
    assert ref.tolist() == sorted(LS.TIE_LANES) + [-1, -1] and len({i % 64 for i in LS.TIE_LANES}) == 3
    for kind, n in (("cut9", 9), ("cut10", 10), ("cut73", 73)):
        s, D, ref = LS.greedy_scene(("ties", kind))
        idx = np.flatnonzero(D[0] < s["tau"])
        assert idx.size == n and np.all(D[:, idx] == 5.0) and ref.tolist() == idx.tolist() + [-1, -1]
    s, D, ref = LS.greedy_scene(("ties", "lead5"))
    row = np.sort(D[0][D[0] < s["tau"]])
    assert row.tolist() == [1, 2, 3, 4, 6] + [7] * 9                        # the tie group holds ranks 5 .. 13: the cut at 8 goes through it
    s, D, ref = LS.greedy_scene(("ties", "gated"))
    idx = np.flatnonzero(D[0] < s["tau"])
    assert s["gate"][0, idx[0]] == 0 and ref[0] == idx[1] and ref[1] == idx[0]          # line 0 may not take the lowest index, line 1 then does
    # threshold: one float32 step below tau matches, tau itself and one step above do not
    s, D, ref = LS.greedy_scene(("threshold",))
    assert D[0, 0] < s["tau"] == D[1, 1] < D[2, 2] and np.nextafter(np.float32(D[0, 0]), np.float32(np.inf)) == np.float32(s["tau"])
    assert ref.tolist() == [0, -1, -1]
    sizes = {LS.greedy_scene(n)[1].shape for n in LS.GREEDY_NAMES if n[0] == "edge"}
    assert {q for q, _ in sizes} >= {1, 255, 256, 257, 513} and {t for _, t in sizes} >= {1, 5, 63, 64, 65}


# ---------------------------------------------------------------- Hough-window scenes
def window_properties(rows, cells, col_ok, inside):
    """rows: the projected image line per row (None: the row is skipped); cells [n,2] (di, ai) per column; col_ok: columns that pass every
    other test; inside [rows][n]: the reference's window verdict."""
    seen = np.zeros((6, 6), int); outside = dict(ang_lo=0, ang_hi=0, dist_lo=0, dist_hi=0); seam = 0; decided = 0
    for i, l in enumerate(rows):
        if l is None:
            assert not inside[i].any()
            continue
        amin, dmin = LR.hough_window_origin(l, LS.SX, LS.SY)
        da = (cells[:, 1] - (amin - 2)) % 50; dd = cells[:, 0] - (dmin - 2)
        win = (da < 6) & (dd >= 0) & (dd < 6) & (cells[:, 0] < 49)
        np.testing.assert_array_equal(inside[i], win & col_ok)              # the literal lists of GetHoughCoordinates say the same
        for a, d in zip(da[win & col_ok], dd[win & col_ok]):
            seen[a, d] += 1
        in_d = (dd >= 0) & (dd < 6) & (cells[:, 0] < 49) & col_ok; in_a = (da < 6) & col_ok
        outside["ang_lo"] += int(np.sum(in_d & (da == 49))); outside["ang_hi"] += int(np.sum(in_d & (da == 6)))
        outside["dist_lo"] += int(np.sum(in_a & (dd == -1))); outside["dist_hi"] += int(np.sum(in_a & (dd == 6) & (cells[:, 0] < 49)))
        if amin - 2 < 0 or amin + 3 > 49:                                   # the window crosses the angle seam
            ai = cells[inside[i], 1]
            assert np.any(ai >= 44) and np.any(ai <= 5), i
            seam += 1
        decided += int(np.sum(col_ok & ~win))
    return seen, outside, seam, decided


def check_window_properties(seen, outside, seam, decided, inside, cells):
    assert np.all(seen > 0), seen                                           # all 36 positions of the window hold a passing column somewhere
    assert all(v > 0 for v in outside.values()), outside                    # and on each of the four sides a column sits one cell outside
    assert seam >= 20
    assert not inside[:, cells[:, 0] == 49].any() and np.sum(cells[:, 0] == 49) == 50          # distance row 49 never passes
    assert decided >= 1000
    assert sorted(set(map(tuple, cells))) == [(d, a) for d in LS.FRAME_DIST_ROWS for a in range(50)]


def test_window_track_scene(oracle):
    P, L, F, ref_m, ref_g = LS.window_track_scene()
    cells = LR.line_cells(F["left_lines"], P["sx"], P["sy"])
    np.testing.assert_array_equal(oracle.line_hough_cells(F["left_lines"], P["sx"], P["sy"]), cells[:, 0] * 50 + cells[:, 1])
    rows = [l for l, _ in LR.track_row_lines(P, L)]
    m_all, g_all = LR.track_naive(P, L, F, use_grid=False, want_gate=True)
    assert g_all.all()                                                      # the reprojection gate is vacuous: the window alone decides
    seen, outside, seam, decided = window_properties(rows, cells, np.ones(cells.shape[0], bool), ref_g.astype(bool))
    check_window_properties(seen, outside, seam, decided, ref_g.astype(bool), cells)
    assert decided == int(g_all.sum() - ref_g.sum()) == 67288
    # rows: every target cell with both signs of both residues
    got = {(LR._hough_centre(l, LS.SX, LS.SY)) for l in rows}
    for ai in LS.ROW_ANG:
        for di in LS.ROW_DIST:
            signs = {(sd, sa) for d_, sd, a_, sa in got if (d_, a_) == (di, ai)}
            assert {s for s, _ in signs} >= ({-1, 1} if di else {-1}) and {s for _, s in signs} >= ({-1, 1} if ai else {-1}), (di, ai, signs)
    om, od, og = oracle.line_track_match(P["K"], P["T_curr"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], L, F, want_gate=True)
    np.testing.assert_array_equal(om, ref_m)
    # the oracle records a gate for the pairs its loop reaches: the order-independent gate minus the columns taken by earlier rows
    taken = np.zeros(cells.shape[0], bool); exp = ref_g.copy()
    for i in range(exp.shape[0]):
        exp[i, taken] = 0
        if ref_m[i] >= 0:
            taken[ref_m[i]] = True
    np.testing.assert_array_equal(og, exp)
    assert (ref_m >= 0).sum() >= 100


def test_window_lastkf_scene(oracle):
    P, cur, last, ref_m = LS.window_lastkf_scene()
    cells = LR.line_cells(last["left_lines"], P["sx"], P["sy"])
    rows = [None if r is None else r[0] for r in LR.lastkf_row_lines(P, cur)]
    assert all(r is not None for r in rows)
    inside = np.stack([LR._window_mask(l, cells, P["sx"], P["sy"]) for l in rows])
    seen, outside, seam, decided = window_properties(rows, cells, np.ones(cells.shape[0], bool), inside)
    check_window_properties(seen, outside, seam, decided, inside, cells)
    assert decided == 67288
    # every match is the nearest descriptor INSIDE the window, and for most rows another line of the frame is nearer outside of it
    D = LR.dist_matrix(cur["desc"], last["desc"])
    assert all(ref_m[i] == (np.flatnonzero(inside[i])[np.argmin(D[i, inside[i]])] if inside[i].any() else -1) for i in range(len(rows)))
    assert np.sum(np.argmin(D, axis=1) != ref_m) >= 90
    om, oc, ox, od = oracle.line_match_last_frame(P["K"], P["T_curr"], P["T_last"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], cur, last, True)
    np.testing.assert_array_equal(om, ref_m)
    np.testing.assert_array_equal(oc, LR.lastkf_created(P, cur, last, ref_m))
    assert oc.sum() >= 40


# ---------------------------------------------------------------- gate scenes with the normal threshold
def test_gate_scene_counts_and_oracle(oracle):
    S = LS.gate_scene(8); P, cur, last, info = S["P"], S["cur"], S["last"], S["info"]
    cat = info["cat"]
    for use_grid in (False, True):
        m, over = LR.lastkf_naive(P, cur, last, use_grid)
        om, oc = oracle.line_match_last_frame(P["K"], P["T_curr"], P["T_last"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], cur, last, use_grid)[:2]
        np.testing.assert_array_equal(om, m)
        np.testing.assert_array_equal(oc, LR.lastkf_created(P, cur, last, m))
        assert oc.sum() >= 20
    m, over = LR.lastkf_naive(P, cur, last, False)
    src = info["cur_src"]; partner = np.where(src >= 0, info["last_of_rel"][np.maximum(src, 0)], -1)
    free = (cur["occupied"] == 0) & (cur["line_matches"] >= 0)
    below = {o: 0 for o in range(LS.N_OCT)}; above = dict(below); one_l = one_r = 0
    for i in np.flatnonzero((src >= 0) & free):
        c, o, side = cat[src[i]]
        if c == LS.K_BOTH and side == 0:
            assert m[i] == partner[i] and tuple(over[i]) == (False, False); below[o] += 1
        elif c == LS.K_BOTH:
            assert m[i] != partner[i]; above[o] += 1                       # 5 % above in both images: rejected
        elif c == LS.K_ONE_L:
            assert m[i] == partner[i] and tuple(over[i]) == (True, False); one_l += 1     # MatchLinesLastKF keeps it, and it wins its match
        elif c == LS.K_ONE_R:
            assert m[i] == partner[i] and tuple(over[i]) == (False, True); one_r += 1
        else:
            assert m[i] != partner[i]                                      # the partner is skipped or has no stereo partner
    assert min(below.values()) >= 1 and min(above.values()) >= 1 and one_l >= 20 and one_r >= 20
    assert np.all(m[~free] == -1) and np.sum(~free) == 4
    hit = m[m >= 0]
    assert len(hit) - len(set(hit)) >= 10                                   # several current lines share one line of the last frame
    # ---- the same pairs under AddLinesFrom: above in EITHER image drops
    for kw in (dict(use_grid=False), dict(use_grid=True), dict(use_grid=False, monocular=True)):
        Pt, L, F = LS.track_view(S)
        tm, tg = LR.track_naive(Pt, L, F, want_gate=True, **kw)
        om, od, og = oracle.line_track_match(Pt["K"], Pt["T_curr"], Pt["b"], Pt["thr_reproj_base"], Pt["md_thr"], Pt["sx"], Pt["sy"], L, F, want_gate=True, **kw)
        np.testing.assert_array_equal(om, tm)
        assert np.all(tg[og.astype(bool)] == 1)
        if kw.get("use_grid", True):
            continue
        msrc = info["map_src"]; mpartner = info["last_of_rel"][msrc]
        counts = {}
        for i in range(len(msrc)):
            c, o, side = cat[msrc[i]]
            g = tg[i, mpartner[i]]
            dead = L["skip"][i] or i >= len(msrc) - 3                       # skipped rows, rows with a main point behind the camera
            if dead:
                assert not tg[i].any() and tm[i] == -1
            elif c == LS.K_BOTH:
                assert g == (side == 0); counts[("both", o, side)] = counts.get(("both", o, side), 0) + 1
            elif c in (LS.K_ONE_L, LS.K_ONE_R):
                assert g == (1 if kw.get("monocular") and c == LS.K_ONE_R else 0)        # (monocular: the right image is not looked at)
                counts[c] = counts.get(c, 0) + 1
            elif c == LS.K_SKIP:
                assert g == 0                                               # the frame line is occupied
            else:
                assert g == (1 if kw.get("monocular") else 0)               # line_matches = -1 passes for a monocular frame only
                if kw.get("monocular") and i < info["n_rel"]:
                    assert tm[i] == mpartner[i]
        assert all(counts.get(("both", o, s_), 0) >= 1 for o in range(LS.N_OCT) for s_ in (0, 1)) and counts[LS.K_ONE_L] >= 20 and counts[LS.K_ONE_R] >= 20
        assert np.sum(tm[len(msrc) - 13: len(msrc) - 3] == -1) >= 5          # the rivals (duplicate map lines) lose their frame line to the first taker


@pytest.mark.parametrize("n_last", LS.N_LAST_SIZES)
def test_gate_scene_prefixes_of_the_last_frame(oracle, n_last):
    S = LS.gate_scene(8); P, cur = S["P"], S["cur"]; last = LS.truncate_last(S["last"], n_last)
    m, _ = LR.lastkf_naive(P, cur, last, False)
    om = oracle.line_match_last_frame(P["K"], P["T_curr"], P["T_last"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], cur, last, False)[0]
    np.testing.assert_array_equal(om, m)
    assert m.max() < n_last and ((m >= 0).sum() >= 1 or n_last == 1)


@pytest.mark.parametrize("dim", LS.LASTKF_DIMS)
def test_gate_scene_descriptor_lengths(oracle, dim):
    S = LS.gate_scene(dim); P, cur, last = S["P"], S["cur"], S["last"]
    assert cur["desc"].shape[1] == last["desc"].shape[1] == dim
    m, _ = LR.lastkf_naive(P, cur, last, False)
    om = oracle.line_match_last_frame(P["K"], P["T_curr"], P["T_last"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], cur, last, False)[0]
    np.testing.assert_array_equal(om, m)
    assert (m >= 0).sum() >= 60


@pytest.mark.parametrize("step", (-1, 0, 1))
def test_md_thr_is_inclusive(oracle, step):
    """A distance equal to md_thr is accepted by both Tracking routines (`md > mdThr` rejects), one float32 step above is not."""
    S = LS.gate_scene(1)
    P, cur, last, L, rows_c, rows_m = LS.threshold_descs(S, step)
    l0 = S["info"]["last_of_rel"][0]
    free = rows_c[(cur["occupied"][rows_c] == 0) & (cur["line_matches"][rows_c] >= 0)]
    d = LR.l2_rows(cur["desc"][free[0]], last["desc"][[l0]])[0]
    assert (d < P["md_thr"], d == P["md_thr"], d > P["md_thr"]) == (step < 0, step == 0, step > 0)
    m, _ = LR.lastkf_naive(P, cur, last, False)
    assert len(free) >= 2 and np.all(m[free] == (l0 if step <= 0 else -1))
    om = oracle.line_match_last_frame(P["K"], P["T_curr"], P["T_last"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], cur, last, False)[0]
    np.testing.assert_array_equal(om, m)
    Pt, _, F = LS.track_view(dict(S, P=P, last=last))
    tm = LR.track_naive(Pt, L, F, use_grid=False)
    assert tm[rows_m[0]] == (l0 if step <= 0 else -1) and np.all(tm[rows_m[1:]] == -1)
    om = oracle.line_track_match(Pt["K"], Pt["T_curr"], Pt["b"], Pt["thr_reproj_base"], Pt["md_thr"], Pt["sx"], Pt["sy"], L, F, use_grid=False)[0]
    np.testing.assert_array_equal(om, tm)


# ---------------------------------------------------------------- stereo
def test_stereo_scene_octaves_and_exact_length(oracle):
    s, jl, jr = LS.stereo_scene()
    assert np.hypot(*(s["left"][jl, :2] - s["left"][jl, 2:])) == 20.0 == np.hypot(*(s["right"][jr, :2] - s["right"][jr, 2:]))
    m1, g1 = LR.naive_match(s, 2.0, 20, is_stereo=True)
    m0, g0 = LR.naive_match(s, 2.0, 20, is_stereo=False)
    mism = s["left_octave"][:, None] != s["right_octave"][None, :]
    assert not g1[mism].any() and g0[mism].sum() >= 100 and np.array_equal(g0[~mism], g1[~mism])     # without is_stereo octave mismatches pass
    assert np.any(m0 != m1)
    assert g1[jl, jr] == 1 and m1[jl] == jr                                 # a length equal to min_line_length passes: the test is '<'
    assert LR.naive_match(s, 2.0, 21)[1][jl].sum() == 0
    om, od, og = oracle.line_match_stereo(s["K"], s["b"], 2.0, 20, s["left"], s["left_octave"], s["desc_left"], s["right"], s["right_octave"],
                                          s["desc_right"], want_gate=True)
    np.testing.assert_array_equal(og, g1); np.testing.assert_array_equal(om, m1)
