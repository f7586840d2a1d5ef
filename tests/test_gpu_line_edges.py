"""GPU: the four line entry points (lld_line_match_greedy, lld_line_match_stereo, lld_line_track_match, lld_line_match_last_frame) on the
crafted scenes of line_scenes.py - windows, ties, thresholds, octaves, list cuts, chunk borders - against the plain numpy reference of
line_ref.py (integer outputs and distances exact, full gate matrices equal), the compiled oracle beside it on the larger scenes, and
every refusal with its status code, each followed by a valid call whose result is right."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lld_slam_amd import Tracking, TwoFrameLineMatcher, abi, host, synth

import line_ref as LR
import line_scenes as LS

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, OK = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED, abi.LLD_OK


def _tracking(ctx, P, **kw):
    return Tracking(ctx, P["K"], P["b"], 1.0 / P["sx"], 1.0 / P["sy"], mdThr=P["md_thr"], **kw)


def _oracle_lastkf(oracle, P, cur, last, use_grid):
    return oracle.line_match_last_frame(P["K"], P["T_curr"], P["T_last"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], cur, last, use_grid)


def _oracle_track(oracle, P, L, F, **kw):
    return oracle.line_track_match(P["K"], P["T_curr"], P["b"], P["thr_reproj_base"], P["md_thr"], P["sx"], P["sy"], L, F, want_gate=True, **kw)


def check_lastkf(gpu_ctx, oracle, P, cur, last, use_grid, ref_m=None):
    """match_last and created exact against the numpy reference and the oracle, X0 / dir against the oracle at the bars of test_gpu_linetrack.py."""
    if ref_m is None:
        ref_m = LR.lastkf_naive(P, cur, last, use_grid)[0]
    gm, gc, gx, gd = _tracking(gpu_ctx, P).MatchLinesLastKF(P["T_curr"], P["T_last"], cur, last, P["thr_reproj_base"], use_grid)
    om, oc, ox, od = _oracle_lastkf(oracle, P, cur, last, use_grid)
    np.testing.assert_array_equal(om, ref_m, err_msg="oracle vs numpy")
    np.testing.assert_array_equal(gm, ref_m, err_msg="device vs numpy")
    np.testing.assert_array_equal(oc, LR.lastkf_created(P, cur, last, ref_m), err_msg="oracle vs numpy (created)")
    np.testing.assert_array_equal(gc, oc)
    ok = oc.astype(bool)
    np.testing.assert_allclose(gd[ok], od[ok], atol=1e-7)
    np.testing.assert_allclose(gx[ok], ox[ok], rtol=1e-6, atol=1e-6)
    assert np.all(gx[~ok] == 0) and np.all(gd[~ok] == 0) and np.all(gc[gm < 0] == 0)
    return gm, gc


def check_track(gpu_ctx, oracle, P, L, F, ref=None, **kw):
    """matches and distances exact, the device gate EQUAL to the order-independent numpy gate."""
    ref_m, ref_g = ref if ref is not None else LR.track_naive(P, L, F, want_gate=True, **kw)
    trk = _tracking(gpu_ctx, P, monocular=kw.get("monocular", False))
    gm, gd, gg = trk.AddLinesFrom(L, P["T_curr"], P["thr_reproj_base"], F, use_grid=kw.get("use_grid", True), want_gate=True)
    om, od, og = _oracle_track(oracle, P, L, F, **kw)
    np.testing.assert_array_equal(om, ref_m, err_msg="oracle vs numpy")
    np.testing.assert_array_equal(gg, ref_g, err_msg="device gate vs numpy gate")
    np.testing.assert_array_equal(gm, ref_m, err_msg="device vs numpy")
    hit = np.flatnonzero(ref_m >= 0)
    exp_d = np.array([LR.l2_rows(L["desc"][i], F["desc"][[ref_m[i]]])[0] for i in hit])
    np.testing.assert_array_equal(gd[hit], exp_d)
    np.testing.assert_array_equal(gd[hit], od[hit])
    return gm, gg


# ---------------------------------------------------------------- lld_line_match_greedy
@pytest.mark.parametrize("name", LS.GREEDY_NAMES, ids=lambda n: "-".join(map(str, n)))
def test_greedy_scenes(gpu_ctx, oracle, name):
    s, D, ref = LS.greedy_scene(name)
    gm, gd = TwoFrameLineMatcher(gpu_ctx, s["tau"]).MatchLines(s["dl"], s["dr"], s["gate"])
    np.testing.assert_array_equal(gm, ref)
    hit = np.flatnonzero(ref >= 0)
    np.testing.assert_array_equal(gd[hit], D[hit, ref[hit]])
    assert np.all(gd[ref < 0] == np.finfo(np.float64).max)
    if D.shape[0] >= 500:                                                    # the larger scenes: the oracle as well, so a disagreement names its side
        om, od = oracle.line_match_greedy(s["dl"], s["dr"], s["gate"], s["tau"])
        np.testing.assert_array_equal(om, ref); np.testing.assert_array_equal(od[hit], gd[hit])


def test_greedy_is_deterministic_and_follows_the_order_of_its_input(gpu_ctx):
    tm = TwoFrameLineMatcher(gpu_ctx, 100.0)
    for name in (("groups", 12), ("ladder",)):
        s, D, ref = LS.greedy_scene(name)
        tm.tau = s["tau"]
        a = tm.MatchLines(s["dl"], s["dr"], s["gate"]); b = tm.MatchLines(s["dl"], s["dr"], s["gate"])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        np.testing.assert_array_equal(a[0], ref)
    s, D, ref = LS.greedy_scene(("groups", 9))
    perm = np.random.default_rng(5).permutation(D.shape[0])
    tm.tau = s["tau"]
    gm, gd = tm.MatchLines(s["dl"][perm], s["dr"], None)
    exp = LR.greedy_naive(D[perm], s["tau"])
    np.testing.assert_array_equal(gm, exp)
    assert not np.array_equal(exp, ref[perm])                               # the order of the left lines matters: rivals swap their right lines


# ---------------------------------------------------------------- the Hough window
def test_window_decides_add_lines_from(gpu_ctx, oracle):
    P, L, F, ref_m, ref_g = LS.window_track_scene()
    gm, gg = check_track(gpu_ctx, oracle, P, L, F, ref=(ref_m, ref_g))
    assert gg.sum() == ref_g.sum() > 2000 and (gm >= 0).sum() > 100
    trk = _tracking(gpu_ctx, P)
    cells = LR.line_cells(F["left_lines"], P["sx"], P["sy"])
    np.testing.assert_array_equal(trk.HoughCells(F["left_lines"]), cells[:, 0] * 50 + cells[:, 1])
    gm0, gd0, gg0 = trk.AddLinesFrom(L, P["T_curr"], P["thr_reproj_base"], F, use_grid=False, want_gate=True)
    assert gg0.all()                                                        # without the grid every pair passes: the window alone decided above


def test_window_decides_match_lines_last_kf(gpu_ctx, oracle):
    P, cur, last, ref_m = LS.window_lastkf_scene()
    gm, gc = check_lastkf(gpu_ctx, oracle, P, cur, last, True, ref_m)
    assert np.all(gm >= 0)
    gm0 = _tracking(gpu_ctx, P).MatchLinesLastKF(P["T_curr"], P["T_last"], cur, last, P["thr_reproj_base"], False)[0]
    np.testing.assert_array_equal(gm0, np.argmin(LR.dist_matrix(cur["desc"], last["desc"]), axis=1))
    assert np.sum(gm0 != gm) >= 90


# ---------------------------------------------------------------- gate scenes with the normal threshold
@pytest.mark.parametrize("kw", [dict(use_grid=False), dict(use_grid=True), dict(use_grid=False, monocular=True)], ids=["all", "grid", "monocular"])
def test_gate_scene_add_lines_from(gpu_ctx, oracle, kw):
    P, L, F = LS.track_view(LS.gate_scene(8))
    gm, gg = check_track(gpu_ctx, oracle, P, L, F, **kw)
    assert (gm >= 0).sum() >= 9 and not gg[L["skip"].astype(bool)].any() and not gg[-3:].any() and not gg[:, F["occupied"].astype(bool)].any()


@pytest.mark.parametrize("use_grid", [False, True])
def test_gate_scene_match_lines_last_kf(gpu_ctx, oracle, use_grid):
    S = LS.gate_scene(8)
    gm, gc = check_lastkf(gpu_ctx, oracle, S["P"], S["cur"], S["last"], use_grid)
    hit = gm[gm >= 0]
    assert len(hit) - len(set(hit)) >= 10 and gc.sum() >= 20                # not exclusive: several current lines share one last line


@pytest.mark.parametrize("n_last", LS.N_LAST_SIZES)
def test_last_frame_sizes(gpu_ctx, oracle, n_last):
    S = LS.gate_scene(8)
    check_lastkf(gpu_ctx, oracle, S["P"], S["cur"], LS.truncate_last(S["last"], n_last), False)
    P, L, F = LS.track_view(S, n_last)
    check_track(gpu_ctx, oracle, P, L, F, use_grid=False)


@pytest.mark.parametrize("dim", LS.LASTKF_DIMS)
def test_last_frame_descriptor_lengths(gpu_ctx, oracle, dim):
    S = LS.gate_scene(dim)
    gm, _ = check_lastkf(gpu_ctx, oracle, S["P"], S["cur"], S["last"], False)
    assert (gm >= 0).sum() >= 60


@pytest.mark.parametrize("step", (-1, 0, 1))
def test_md_thr_is_inclusive(gpu_ctx, oracle, step):
    S = LS.gate_scene(1)
    P, cur, last, L, rows_c, rows_m = LS.threshold_descs(S, step)
    l0 = S["info"]["last_of_rel"][0]
    gm, _ = check_lastkf(gpu_ctx, oracle, P, cur, last, False)
    free = rows_c[(cur["occupied"][rows_c] == 0) & (cur["line_matches"][rows_c] >= 0)]
    assert np.all(gm[free] == (l0 if step <= 0 else -1))
    Pt, _, F = LS.track_view(dict(S, P=P, last=last))
    tm, _ = check_track(gpu_ctx, oracle, Pt, L, F, use_grid=False)
    assert tm[rows_m[0]] == (l0 if step <= 0 else -1)


# ---------------------------------------------------------------- lld_line_match_stereo
@pytest.mark.parametrize("is_stereo", [True, False])
def test_stereo_octave_rule_and_exact_length(gpu_ctx, oracle, is_stereo):
    s, jl, jr = LS.stereo_scene()
    ref_m, ref_g = LR.naive_match(s, 2.0, 20, is_stereo=is_stereo)
    gm, gd, gg = host.line_stereo_call(gpu_ctx.lib, gpu_ctx.handle, s["K"], s["b"], 2.0, 20, s["left"], s["left_octave"], s["desc_left"], s["right"],
                                       s["right_octave"], s["desc_right"], is_stereo, True)
    np.testing.assert_array_equal(gg, ref_g)
    np.testing.assert_array_equal(gm, ref_m)
    hit = np.flatnonzero(ref_m >= 0)
    np.testing.assert_array_equal(gd[hit], np.array([LR.l2_rows(s["desc_left"][j], s["desc_right"][[ref_m[j]]])[0] for j in hit]))
    assert gg[jl, jr] == 1 and gm[jl] == jr                                 # length == min_line_length passes
    mism = s["left_octave"][:, None] != s["right_octave"][None, :]
    assert gg[mism].any() == (not is_stereo)
    if is_stereo:
        om, od, og = oracle.line_match_stereo(s["K"], s["b"], 2.0, 20, s["left"], s["left_octave"], s["desc_left"], s["right"], s["right_octave"],
                                              s["desc_right"], want_gate=True)
        np.testing.assert_array_equal(og, gg); np.testing.assert_array_equal(om, gm)
        g21 = host.line_stereo_call(gpu_ctx.lib, gpu_ctx.handle, s["K"], s["b"], 2.0, 21, s["left"], s["left_octave"], s["desc_left"], s["right"],
                                    s["right_octave"], s["desc_right"], True, True)[2]
        assert not g21[jl].any()


# ---------------------------------------------------------------- refusals, with the status code, each followed by a valid call
def _ptr(a):
    ct = {np.dtype(np.float32): C.c_float, np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32, np.dtype(np.uint8): C.c_uint8}[a.dtype]
    return a.ctypes.data_as(C.POINTER(ct))


class Raw:
    """One entry point with named arguments: call(**overrides) returns the status; arrays are kept alive here."""

    def __init__(self, fn, names, values):
        self.fn = fn; self.names = names; self.values = dict(zip(names, values))

    def call(self, **over):
        v = dict(self.values); v.update(over)
        return self.fn(*[(_ptr(x) if isinstance(x, np.ndarray) else x) for x in (v[n] for n in self.names)])


def run_refusals(raw, cases, valid):
    for over, status in cases:
        assert raw.call(**over) == status, (sorted(over), status)
        valid()                                                            # the context is still usable and the next valid call is right


def test_refusals_greedy(gpu_ctx):
    s, D, ref = LS.greedy_scene(("edge", 30, 5))
    nq, nt = D.shape
    m = np.empty(nq, np.int32); d = np.empty(nq, np.float64)
    raw = Raw(gpu_ctx.lib.fn("line_match_greedy"), ["ctx", "dl", "nq", "dr", "nt", "dim", "gate", "tau", "m", "d"],
              [gpu_ctx.handle, s["dl"], nq, s["dr"], nt, 3, None, s["tau"], m, d])

    def valid():
        m[:] = -7
        assert raw.call() == OK
        np.testing.assert_array_equal(m, ref)
    cases = [({k: None}, INVALID) for k in ("ctx", "dl", "dr", "m")] + [(dict(nq=-1), INVALID), (dict(nt=-1), INVALID), (dict(dim=0), INVALID),
                                                                         (dict(dim=-3), INVALID), (dict(dim=129), UNSUPPORTED)]
    run_refusals(raw, cases, valid)


def test_refusals_stereo(gpu_ctx):
    s = synth.make_stereo_lines(1, 40, 30)
    ref_m, ref_g = LR.naive_match(s, 2.0, 20)
    nq, nt = s["left"].shape[0], s["right"].shape[0]
    P = abi.LineStereoParams()
    for i, v in enumerate(s["K"].reshape(9)):
        P.K[i] = float(v)
    P.b = s["b"]; P.tau = 2.0; P.min_line_length = 20; P.is_stereo = 1
    m = np.empty(nq, np.int32); d = np.empty(nq, np.float64); g = np.empty((nq, nt), np.uint8)
    raw = Raw(gpu_ctx.lib.fn("line_match_stereo"), ["ctx", "prm", "ll", "lo", "dl", "nq", "rl", "ro", "dr", "nt", "dim", "m", "d", "g"],
              [gpu_ctx.handle, C.byref(P), s["left"], s["left_octave"], s["desc_left"], nq, s["right"], s["right_octave"], s["desc_right"], nt, 72, m, d, g])

    def valid():
        m[:] = -7; g[:] = 9
        assert raw.call() == OK
        np.testing.assert_array_equal(m, ref_m); np.testing.assert_array_equal(g, ref_g)
    cases = [({k: None}, INVALID) for k in ("ctx", "prm", "ll", "lo", "dl", "rl", "ro", "dr", "m")]
    cases += [(dict(nq=-1), INVALID), (dict(nt=-1), INVALID), (dict(dim=0), INVALID), (dict(dim=129), UNSUPPORTED)]
    run_refusals(raw, cases, valid)


def _track_params(P, **over):
    S = abi.LineTrackParams()
    for i, v in enumerate(np.asarray(P["K"], np.float64).reshape(9)):
        S.K[i] = float(v)
    for i, v in enumerate(np.asarray(P["T_curr"], np.float64).reshape(16)):
        S.T_curr[i] = float(v)
    S.b = P["b"]; S.thr_reproj_base = P["thr_reproj_base"]; S.md_thr = P["md_thr"]; S.sx = P["sx"]; S.sy = P["sy"]; S.monocular = 0; S.use_grid = 1
    for k, v in over.items():
        setattr(S, k, v)
    return S


def test_refusals_track(gpu_ctx):
    P, L, F = synth.make_line_track_scene(9, n_map=20, n_cur=30)
    ref_m, ref_g = LR.track_naive(P, L, F, want_gate=True)
    n_map, n_cur = 20, 30
    S = _track_params(P)
    m = np.empty(n_map, np.int32); d = np.empty(n_map, np.float64); g = np.empty((n_map, n_cur), np.uint8)
    names = ["ctx", "prm", "n_map", "x0", "dir", "x1", "x2", "skip", "mdesc", "n_cur", "ll", "lo", "n_right", "rl", "lm", "occ", "cdesc", "dim", "m", "d", "g"]
    c64 = lambda a: np.ascontiguousarray(a, np.float64)
    raw = Raw(gpu_ctx.lib.fn("line_track_match"), names,
              [gpu_ctx.handle, C.byref(S), n_map, c64(L["X0"]), c64(L["dir"]), c64(L["X1"]), c64(L["X2"]), L["skip"], L["desc"], n_cur, F["left_lines"],
               F["left_octave"], F["right_lines"].shape[0], F["right_lines"], F["line_matches"], F["occupied"], F["desc"], 72, m, d, g])

    def valid():
        m[:] = -7; g[:] = 9
        assert raw.call() == OK
        np.testing.assert_array_equal(m, ref_m); np.testing.assert_array_equal(g, ref_g)
    cases = [({k: None}, INVALID) for k in ("ctx", "prm", "x0", "dir", "x1", "x2", "mdesc", "ll", "lo", "lm", "cdesc", "m", "rl")]
    cases += [(dict(n_map=-1), INVALID), (dict(n_cur=-1), INVALID), (dict(n_right=-1), INVALID), (dict(dim=0), INVALID), (dict(dim=129), UNSUPPORTED)]
    for k, v in (("sx", 0.0), ("sx", -1.0), ("sx", float("nan")), ("sy", 0.0), ("sy", float("nan"))):
        cases.append((dict(prm=C.byref(_track_params(P, **{k: v}))), INVALID))
    for o in (-1, 65):
        lo = F["left_octave"].copy(); lo[n_cur - 1] = o
        cases.append((dict(lo=lo), INVALID))
    lm = F["line_matches"].copy(); lm[3] = F["right_lines"].shape[0]
    cases.append((dict(lm=lm), INVALID))
    run_refusals(raw, cases, valid)
    lo = F["left_octave"].copy(); lo[0] = 64                                # the largest octave that is taken: thr_base * 1.44^64
    assert raw.call(lo=lo) == OK
    F64 = dict(F, left_octave=lo)
    np.testing.assert_array_equal(m, LR.track_naive(P, L, F64)); np.testing.assert_array_equal(g, LR.track_naive(P, L, F64, want_gate=True)[1])


def test_refusals_last_frame(gpu_ctx):
    P, cur, last, _ = synth.make_two_frame_lines(4, n_lines=60)
    P = dict(P, md_thr=1e9)                                                 # every line that passes the gates matches: the gates decide
    ref_m = LR.lastkf_naive(P, cur, last, False)[0]
    n = 60
    S = abi.LineLastKfParams()

    def fill(S, **over):
        for i, v in enumerate(P["K"].reshape(9)):
            S.K[i] = float(v)
        for i, v in enumerate(P["T_curr"].reshape(16)):
            S.T_curr[i] = float(v)
        for i, v in enumerate(P["T_last"].reshape(16)):
            S.T_last[i] = float(v)
        S.b = P["b"]; S.thr_reproj_base = P["thr_reproj_base"]; S.md_thr = P["md_thr"]; S.sx = P["sx"]; S.sy = P["sy"]; S.use_grid = 0
        for k, v in over.items():
            setattr(S, k, v)
        return S
    fill(S)
    m = np.empty(n, np.int32); cre = np.empty(n, np.uint8); x0 = np.zeros((n, 3)); dr = np.zeros((n, 3))
    names = ["ctx", "prm", "n_cur", "cl", "n_cr", "cr", "clm", "cocc", "cdesc", "n_last", "ll", "lo", "n_lr", "lr", "llm", "lskip", "ldesc", "dim", "m", "cre", "x0", "dir"]
    raw = Raw(gpu_ctx.lib.fn("line_match_last_frame"), names,
              [gpu_ctx.handle, C.byref(S), n, cur["left_lines"], n, cur["right_lines"], cur["line_matches"], cur["occupied"], cur["desc"], n, last["left_lines"],
               last["left_octave"], n, last["right_lines"], last["line_matches"], last["skip"], last["desc"], 72, m, cre, x0, dr])

    def valid():
        m[:] = -7
        assert raw.call() == OK
        np.testing.assert_array_equal(m, ref_m)
    cases = [({k: None}, INVALID) for k in ("ctx", "prm", "cl", "cr", "clm", "cdesc", "ll", "lo", "lr", "llm", "ldesc", "m", "cre", "x0", "dir")]
    cases += [({k: -1}, INVALID) for k in ("n_cur", "n_cr", "n_last", "n_lr")] + [(dict(dim=0), INVALID), (dict(dim=-1), INVALID), (dict(dim=4097), UNSUPPORTED)]
    for k, v in (("sx", 0.0), ("sx", float("nan")), ("sy", -2.0), ("sy", float("nan"))):
        cases.append((dict(prm=C.byref(fill(abi.LineLastKfParams(), **{k: v}))), INVALID))
    for o in (-1, 65):
        lo = last["left_octave"].copy(); lo[n - 1] = o
        cases.append((dict(lo=lo), INVALID))
    a = cur["line_matches"].copy(); a[2] = n
    b = last["line_matches"].copy(); b[5] = n
    cases += [(dict(clm=a), INVALID), (dict(llm=b), INVALID)]
    run_refusals(raw, cases, valid)
    assert (ref_m >= 0).sum() > 10
    lo = last["left_octave"].copy(); lo[::3] = 64                            # the largest octave that is taken: 64 multiplications by 1.44
    assert raw.call(lo=lo) == OK
    exp = LR.lastkf_naive(P, cur, dict(last, left_octave=lo), False)[0]
    np.testing.assert_array_equal(m, exp)
    assert np.any(exp != ref_m)


# ---------------------------------------------------------------- the size ceilings of include/lld_amd.h, both sides
def _header_constants():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lld_amd.h")).read()
    out = {}
    for name in ("LLD_LINE_DIM_MAX", "LLD_LINE_LASTKF_DIM_MAX", "LLD_LINE_LDS_CEILING"):
        expr = re.search(r"#define\s+%s\s+\(?([0-9 *]+)\)?" % name, text).group(1)
        out[name] = int(np.prod([int(f) for f in expr.split("*")]))
    return out


def test_size_ceilings_both_sides(gpu_ctx):
    H = _header_constants()
    assert (H["LLD_LINE_DIM_MAX"], H["LLD_LINE_LASTKF_DIM_MAX"], H["LLD_LINE_LDS_CEILING"]) == (128, 4096, 150 * 1024)
    ceiling = H["LLD_LINE_LDS_CEILING"]
    fn = gpu_ctx.lib.fn("line_match_greedy")
    # one row of distances: columns * 8 + dim * 4 <= ceiling, nq = 2, dim = 72
    dim = 72; nt_max = (ceiling - dim * 4) // 8
    rng = np.random.default_rng(3)
    dl = rng.integers(0, 4, (2, dim)).astype(np.float32); dr = rng.integers(0, 4, (nt_max + 1, dim)).astype(np.float32)
    dr[nt_max - 1] = dl[0]; dr[7] = dl[1]                                    # the nearest right lines sit at the far end of the row and near its start
    m = np.full(2, -7, np.int32); d = np.zeros(2)
    assert fn(gpu_ctx.handle, _ptr(dl), 2, _ptr(dr), nt_max, dim, None, 1e9, _ptr(m), _ptr(d)) == OK          # ~150 KiB of dynamic LDS
    ref = LR.greedy_naive((dl, dr[:nt_max]), 1e9)
    np.testing.assert_array_equal(m, ref)
    assert m.tolist() == [nt_max - 1, 7] and d.tolist() == [0.0, 0.0]
    m[:] = -7
    assert fn(gpu_ctx.handle, _ptr(dl), 2, _ptr(dr), nt_max + 1, dim, None, 1e9, _ptr(m), _ptr(d)) == UNSUPPORTED
    assert m.tolist() == [-7, -7]                                           # nothing was written
    assert fn(gpu_ctx.handle, _ptr(dl), 2, _ptr(dr), 300, dim, None, 1e9, _ptr(m), _ptr(d)) == OK
    np.testing.assert_array_equal(m, LR.greedy_naive((dl, dr[:300]), 1e9))
    # blk + pick of the resolve: (rows + columns) * 4 + 16 <= ceiling, nt = 1, dim = 1
    n_max = (ceiling - 16) // 4
    dl = np.zeros((n_max, 1), np.float32); dr = np.zeros((1, 1), np.float32)
    m = np.full(n_max, -7, np.int32)
    assert fn(gpu_ctx.handle, _ptr(dl), n_max - 1, _ptr(dr), 1, 1, None, 1.0, _ptr(m), None) == OK
    assert m[0] == 0 and np.all(m[1:n_max - 1] == -1) and m[n_max - 1] == -7  # line 0 takes the only right line
    m[:] = -7
    assert fn(gpu_ctx.handle, _ptr(dl), n_max, _ptr(dr), 1, 1, None, 1.0, _ptr(m), None) == UNSUPPORTED
    assert np.all(m == -7)
    assert fn(gpu_ctx.handle, _ptr(dl), 5, _ptr(dr), 1, 1, None, 1.0, _ptr(m), None) == OK
    assert m[:6].tolist() == [0, -1, -1, -1, -1, -7]
    # the same two ceilings guard lld_line_track_match (rows = n_map, columns = n_cur): refused from the counts alone
    P, L, F = synth.make_line_track_scene(9, n_map=20, n_cur=30)
    S = _track_params(P)
    trk = gpu_ctx.lib.fn("line_track_match")
    c64 = lambda a: _ptr(np.ascontiguousarray(a, np.float64))
    big = n_max                                                            # n_map + n_cur over the resolve ceiling; n_cur alone under the row ceiling
    x = np.zeros((big, 3)); x[:, 2] = 5.0; dsc = np.zeros((big, 1), np.float32); mt = np.full(big, -7, np.int32)
    st = trk(gpu_ctx.handle, C.byref(S), big - 29, _ptr(x), _ptr(x), _ptr(x), _ptr(x), None, _ptr(dsc), 30, _ptr(F["left_lines"]), _ptr(F["left_octave"]),
             30, _ptr(F["right_lines"]), _ptr(F["line_matches"]), None, _ptr(dsc), 1, _ptr(mt), None, None)
    assert st == UNSUPPORTED and np.all(mt == -7)
    m2 = np.empty(20, np.int32)
    assert trk(gpu_ctx.handle, C.byref(S), 20, c64(L["X0"]), c64(L["dir"]), c64(L["X1"]), c64(L["X2"]), _ptr(L["skip"]), _ptr(L["desc"]), 30, _ptr(F["left_lines"]),
               _ptr(F["left_octave"]), 30, _ptr(F["right_lines"]), _ptr(F["line_matches"]), _ptr(F["occupied"]), _ptr(F["desc"]), 72, _ptr(m2), None, None) == OK
    np.testing.assert_array_equal(m2, LR.track_naive(P, L, F))
