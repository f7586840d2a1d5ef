"""GPU parity: Tracking::AddLinesFrom through the C ABI (lld_line_track_match) vs the CPU oracle - matches and gates bit for bit."""
import numpy as np
import pytest

from lld_slam_amd import Tracking, synth

from line_ref import track_naive

pytestmark = pytest.mark.gpu


def run_both(gpu_ctx, oracle, P, L, F, **kw):
    trk = Tracking(gpu_ctx, P["K"], P["b"], 1.0 / P["sx"], 1.0 / P["sy"], mdThr=P["md_thr"], monocular=kw.get("monocular", False))
    g = trk.AddLinesFrom(L, P["T_curr"], P["thr_reproj_base"], F, use_grid=kw.get("use_grid", True), want_gate=True)
    o = oracle.line_track_match(P["K"], P["T_curr"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], L, F, want_gate=True, **kw)
    return g, o


@pytest.mark.parametrize("scene,kw", [(0, {}), (1, dict(monocular=True)), (2, dict(use_grid=False)), (3, dict(use_grid=False, monocular=True)),
                                      (5, {}), (6, dict(use_grid=False))])
def test_add_lines_from_matches_oracle(gpu_ctx, oracle, scene, kw):
    P, L, F = synth.make_line_track_scene(scene)
    (gm, gd, gg), (om, od, og) = run_both(gpu_ctx, oracle, P, L, F, **kw)
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gd[gm >= 0], od[om >= 0])                 # float difference, double accumulation in index order: identical
    # the oracle records a gate only for pairs its sequential loop reaches (a frame line taken earlier is skipped before the gates);
    # the device gate matrix is the order-independent part: it must contain every recorded pair and nothing on rows / columns that are excluded
    assert np.all(gg[og.astype(bool)] == 1)
    assert not np.any(gg[L["skip"].astype(bool)])
    assert not np.any(gg[:, F["occupied"].astype(bool)])
    # and it EQUALS the order-independent gate of the plain numpy restatement: an extra one from a missing or loosened gate fails here
    nm, ng = track_naive(P, L, F, want_gate=True, **kw)
    np.testing.assert_array_equal(gg, ng)
    np.testing.assert_array_equal(gm, nm)
    assert (gm >= 0).sum() > 10


def test_hough_cells_equal_the_oracle_fill(gpu_ctx, oracle):
    P, L, F = synth.make_line_track_scene(7, n_cur=500)
    trk = Tracking(gpu_ctx, P["K"], P["b"], 1.0 / P["sx"], 1.0 / P["sy"])
    np.testing.assert_array_equal(trk.HoughCells(F["left_lines"]), oracle.line_hough_cells(F["left_lines"], P["sx"], P["sy"]))


def test_rivals_chain_and_edge_cases(gpu_ctx, oracle):
    """Many map lines with one descriptor: the frame line goes to the first, the others fall back to their next candidate (the
    cut candidate lists must be refilled from the stored row); empty inputs; every frame line occupied."""
    P, L, F = synth.make_line_track_scene(8, n_map=300, n_cur=120)
    L["desc"][:] = L["desc"][0]; F["desc"][:] = L["desc"][0]               # all distances zero: pure order dependence
    (gm, _, _), (om, _, _) = run_both(gpu_ctx, oracle, P, L, F, use_grid=False)
    np.testing.assert_array_equal(gm, om)
    F2 = dict(F); F2["occupied"] = np.ones_like(F["occupied"])
    (gm, _, _), (om, _, _) = run_both(gpu_ctx, oracle, P, L, F2)
    assert np.all(gm == -1) and np.all(om == -1)
    empty = dict(left_lines=np.zeros((0, 4), np.float32), left_octave=np.zeros(0, np.int32), right_lines=np.zeros((0, 4), np.float32),
                 line_matches=np.zeros(0, np.int32), occupied=np.zeros(0, np.uint8), desc=np.zeros((0, 72), np.float32))
    trk = Tracking(gpu_ctx, P["K"], P["b"], 1.0 / P["sx"], 1.0 / P["sy"], mdThr=P["md_thr"])
    m, d = trk.AddLinesFrom(L, P["T_curr"], 2.0, empty)
    assert np.all(m == -1)


def test_malformed_arguments_are_refused(gpu_ctx):
    P, L, F = synth.make_line_track_scene(9, n_map=20, n_cur=30)
    trk = Tracking(gpu_ctx, P["K"], P["b"], 1.0 / P["sx"], 1.0 / P["sy"], mdThr=P["md_thr"])
    bad = dict(F); bad["line_matches"] = F["line_matches"].copy(); bad["line_matches"][0] = 10 ** 6          # partner index out of range
    with pytest.raises(RuntimeError):
        trk.AddLinesFrom(L, P["T_curr"], 2.0, bad)
    bad = dict(F); bad["left_octave"] = F["left_octave"].copy(); bad["left_octave"][0] = -1
    with pytest.raises(RuntimeError):
        trk.AddLinesFrom(L, P["T_curr"], 2.0, bad)


@pytest.mark.parametrize("scene,use_grid", [(0, True), (1, False), (2, True), (3, False)])
def test_match_lines_last_kf_matches_oracle(gpu_ctx, oracle, scene, use_grid):
    """Matches and the created flags bit for bit; X0 / direction to 1e-6 (the device takes the two well-conditioned eigen-directions of
    the normal matrix where the oracle, like the reference, solves the rank-deficient least squares by pivoted QR and projects)."""
    P, cur, last, _ = synth.make_two_frame_lines(scene)
    trk = Tracking(gpu_ctx, P["K"], P["b"], 1.0 / P["sx"], 1.0 / P["sy"], mdThr=P["md_thr"])
    gm, gc, gx, gd = trk.MatchLinesLastKF(P["T_curr"], P["T_last"], cur, last, P["thr_reproj_base"], use_grid)
    om, oc, ox, od = oracle.line_match_last_frame(P["K"], P["T_curr"], P["T_last"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], cur, last, use_grid)
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gc, oc)
    ok = oc.astype(bool)
    assert ok.sum() > 20
    np.testing.assert_allclose(gd[ok], od[ok], atol=1e-7)
    np.testing.assert_allclose(gx[ok], ox[ok], rtol=1e-6, atol=1e-6)
    assert np.all(gx[~ok] == 0) and np.all(gd[~ok] == 0)


def test_match_lines_last_kf_edge_cases(gpu_ctx, oracle):
    P, cur, last, _ = synth.make_two_frame_lines(4, n_lines=60)
    trk = Tracking(gpu_ctx, P["K"], P["b"], 1.0 / P["sx"], 1.0 / P["sy"], mdThr=P["md_thr"])
    none = dict(last); none["line_matches"] = -np.ones_like(last["line_matches"])            # no line of the last frame has a stereo partner
    m, c, _, _ = trk.MatchLinesLastKF(P["T_curr"], P["T_last"], cur, none)
    assert np.all(m == -1) and not c.any()
    empty = dict(left_lines=np.zeros((0, 4), np.float32), right_lines=np.zeros((0, 4), np.float32), line_matches=np.zeros(0, np.int32),
                 desc=np.zeros((0, 72), np.float32), left_octave=np.zeros(0, np.int32), skip=np.zeros(0, np.uint8))
    m, c, _, _ = trk.MatchLinesLastKF(P["T_curr"], P["T_last"], cur, empty)
    assert np.all(m == -1) and not c.any()
    bad = dict(cur); bad["line_matches"] = cur["line_matches"].copy(); bad["line_matches"][0] = 10 ** 6
    with pytest.raises(RuntimeError):
        trk.MatchLinesLastKF(P["T_curr"], P["T_last"], bad, last)


def test_degenerate_lines_take_the_documented_cell(gpu_ctx, oracle):
    """A KeyLine with coincident end points and a map line with a zero direction have no line equation (0/0): both sides treat them as the
    line y = 0 instead of indexing the grid with a NaN cast, and still agree on every match."""
    P, L, F = synth.make_line_track_scene(11, n_map=150, n_cur=200)
    F["left_lines"][::17, 2:] = F["left_lines"][::17, :2]
    L["dir"][::13] = 0.0
    trk = Tracking(gpu_ctx, P["K"], P["b"], 1.0 / P["sx"], 1.0 / P["sy"])
    cells = trk.HoughCells(F["left_lines"])
    np.testing.assert_array_equal(cells, oracle.line_hough_cells(F["left_lines"], P["sx"], P["sy"]))
    assert np.all(cells[::17] == 25)                                       # distance row 0, angle column 25 (pi/2)
    for kw in ({}, dict(use_grid=False)):
        (gm, gd, _), (om, od, _) = run_both(gpu_ctx, oracle, P, L, F, **kw)
        np.testing.assert_array_equal(gm, om)
        np.testing.assert_array_equal(gd[gm >= 0], od[om >= 0])
