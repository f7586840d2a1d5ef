"""lld_frame_build_lines / lld_frame_lines_download / lld_frame_new_map_lines: the stereo Frame's line association and MatchLinesLastKF on
resident frames, against the stand-alone device calls (lld_line_match_stereo + lld_frame_set_lines) and against the CPU oracle.
Integers and the stereo distances bit for bit; X0 / direction of a created line at the bar of tests/test_gpu_linetrack.py."""
import functools

import numpy as np
import pytest

import frame_lines_scenes as FS
from lld_slam_amd import abi, synth
from lld_slam_amd.tracking import DeviceTrackedFrame

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED


def lines_frame(ctx, L, **params):
    return DeviceTrackedFrame(ctx, FS.keypoint_frame(), FS.CAM, L, **params)


def check_build_against_both(gpu_ctx, oracle, L, is_stereo=1):
    L = dict(L, stereo=dict(L["stereo"], is_stereo=is_stereo))
    om, od, og = FS.oracle_stereo(oracle, L)
    with lines_frame(gpu_ctx, L) as tf:
        gm, gd = tf.lines_download()
    sm, sd = FS.device_stereo(gpu_ctx, L)
    print("matched %d of %d, rows with more than one gated candidate %d" % ((om >= 0).sum(), om.size, (og.sum(1) > 1).sum()))
    np.testing.assert_array_equal(gm, sm); np.testing.assert_array_equal(gd, sd)             # the stand-alone call on the same build
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gd[om >= 0], od[om >= 0])                                  # float difference, double accumulation in index order: identical
    assert np.all(gd[om < 0] == FS.DBL_MAX)
    return om, og


# ---------------------------------------------------------------------------------------------- 1. A against both references
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_build_lines_equals_stereo_matcher_on_wide_baseline_scenes(gpu_ctx, oracle, seed):
    om, og = check_build_against_both(gpu_ctx, oracle, FS.wide_stereo_scene(seed))
    assert (om >= 0).sum() * 5 >= om.size and (og.sum(1) > 1).sum() * 2 >= om.size             # the scene is what the test needs it to be


def test_build_lines_equals_stereo_matcher_on_the_kitti_scene(gpu_ctx, oracle):
    check_build_against_both(gpu_ctx, oracle, FS.kitti_stereo_scene())


def test_build_lines_without_the_octave_gate(gpu_ctx, oracle):
    """is_stereo = 0 drops the equal-octave gate.  The scenes give partners equal octaves, so here eight matched partners get another octave:
    with the gate their left lines lose them, without it they keep them."""
    L = FS.wide_stereo_scene(1)
    om = FS.oracle_stereo(oracle, L)[0]
    ro = L["right_octave"].copy(); ro[om[om >= 0][:8]] += 1
    L = dict(L, right_octave=ro)
    om1, _ = check_build_against_both(gpu_ctx, oracle, L, is_stereo=1)
    om0, _ = check_build_against_both(gpu_ctx, oracle, L, is_stereo=0)
    assert np.array_equal(om0, om) and (om1 != om0).sum() >= 8


def test_build_lines_with_an_empty_side(gpu_ctx, oracle):
    L = FS.wide_stereo_scene(0); dim = L["desc"].shape[1]
    none_r = dict(L, right_lines=np.zeros((0, 4), np.float32), right_octave=np.zeros(0, np.int32), desc_right=np.zeros((0, dim), np.float32))
    with lines_frame(gpu_ctx, none_r) as tf:
        m, d = tf.lines_download()
        assert m.size == 96 and np.all(m == -1) and np.all(d == FS.DBL_MAX)
    none_l = dict(L, left_lines=np.zeros((0, 4), np.float32), left_octave=np.zeros(0, np.int32), desc=np.zeros((0, dim), np.float32))
    with lines_frame(gpu_ctx, none_l) as tf:
        assert tf.n_lines == 0
        m, d = tf.lines_download()                                                          # a frame without lines: nothing to fetch
        assert m.size == 0
    with lines_frame(gpu_ctx, None) as tf:
        assert tf.lib.fn("frame_build_lines")(tf.res.handle, None) == abi.LLD_OK                # in == NULL: a frame without lines
        assert tf.lib.fn("frame_lines_download")(tf.res.handle, None, None) == abi.LLD_OK


def test_lines_download_on_a_frame_of_set_lines(gpu_ctx, oracle):
    L = FS.wide_stereo_scene(2)
    om, _, _ = FS.oracle_stereo(oracle, L)
    with lines_frame(gpu_ctx, dict(left_lines=L["left_lines"], left_octave=L["left_octave"], right_lines=L["right_lines"], right_octave=L["right_octave"],
                                   line_matches=om, desc=L["desc"])) as tf:
        m, d = tf.lines_download()
    np.testing.assert_array_equal(m, om)
    assert np.all(d == FS.DBL_MAX)


# ---------------------------------------------------------------------------------------------- 2. the chain after A = the chain after lld_frame_set_lines
@functools.lru_cache(maxsize=None)
def chain_scene():
    """One small tracking frame (200 keypoints, 96 lines) whose lines dict serves both routes: right descriptors = the partner's left
    descriptor plus noise, the rig's own K and baseline for the matcher."""
    sc = synth.make_tracking_scene(0, n_kp=200, n_map=260, n_last=120, n_lines=96, n_map_lines=120, n_last_lines=80, rot_deg=0.02, trans=0.001, line_depth=LINE_DEPTH, line_length=LINE_LENGTH)
    L = sc["lines"]; rng = np.random.default_rng(5)
    nr, dim = L["right_lines"].shape[0], L["desc"].shape[1]
    dr = rng.normal(size=(nr, dim)); dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    has = L["line_matches"] >= 0
    dr[L["line_matches"][has]] = L["desc"][has] + rng.normal(0, 0.05, (int(has.sum()), dim))
    fx, fy, cx, cy, bf = [float(np.float32(c)) for c in sc["cam"]]
    stereo = dict(K=np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]), b=float(np.float32(np.float32(bf) / np.float32(fx))), tau=FS.TAU, min_line_length=FS.MIN_LEN, is_stereo=1)
    return sc, dict(L, desc_right=dr.astype(np.float32), stereo=stereo)


LINE_DEPTH = (1.2, 2.3)
LINE_LENGTH = (0.15, 0.6)


def run_chain(tf, sc):
    tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc["last_lines"])
    tf.track_local_map(sc["map_points"], sc["map_ids"], sc["local_lines"])
    return tf.download()


def same_records(got, exp):
    for g, e in zip(got, exp):
        assert sorted(g) == sorted(e)
        for k in e:
            np.testing.assert_array_equal(g[k], e[k], err_msg=k)                            # every field and array, poses and chi2 included: the same kernels on the same bits


@pytest.fixture(scope="module")
def chain_reference(gpu_ctx, oracle):
    """The records of the chain on the frame whose lines lld_frame_set_lines set, with line_matches from the oracle."""
    sc, L = chain_scene()
    om, _, _ = FS.oracle_stereo(oracle, L)
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], dict(sc["lines"], line_matches=om)) as tf:
        ref = run_chain(tf, sc)
    assert ref[0]["n_lines_matched"] > 5 and ref[1]["n_lines_matched"] > 5
    return ref


def test_chain_after_build_lines_equals_chain_after_set_lines(gpu_ctx, chain_reference):
    sc, L = chain_scene()
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], L) as tf:
        same_records(run_chain(tf, sc), chain_reference)                                    # nothing waited between the build and the chain
        same_records(run_chain(tf, sc), chain_reference)
        tf._build_lines(L)                                                                  # on a frame that has a state: replaces it
        same_records(run_chain(tf, sc), chain_reference)


# ---------------------------------------------------------------------------------------------- 3. / 4. B against the oracle
def open_pair(gpu_ctx, oracle, seed):
    """Two resident frames built by lld_frame_build_lines and loaded with the scene's state; returns (S, cur, last, views, oracle partners)."""
    S = FS.last_kf_scene(seed)
    cur = lines_frame(gpu_ctx, S["cur"]); last = lines_frame(gpu_ctx, S["last"])
    vc = FS.set_line_state(cur, S["T_cur"], S["cur_state"]); vl = FS.set_line_state(last, S["T_last"], S["last_state"])
    return S, cur, last, (vc, vl), (FS.oracle_stereo(oracle, S["cur"])[0], FS.oracle_stereo(oracle, S["last"])[0])


def same_new_lines(g, o, first_new_id, n_held):
    om, oc, ox, od = o
    np.testing.assert_array_equal(g["match_last"], om)
    np.testing.assert_array_equal(g["created"], oc)
    ok = oc.astype(bool)
    assert g["n_created"] == int(ok.sum()) and g["n_held"] == n_held
    np.testing.assert_allclose(g["dir"][ok], od[ok], atol=1e-7)
    np.testing.assert_allclose(g["x0"][ok], ox[ok], rtol=1e-6, atol=1e-6)
    assert np.all(g["x0"][~ok] == 0) and np.all(g["dir"][~ok] == 0)
    want = np.full(ok.size, -1, np.int32); want[ok] = first_new_id + np.arange(int(ok.sum()))      # creation order: ascending i
    np.testing.assert_array_equal(g["new_id"], want)


@pytest.mark.parametrize("use_grid", [0, 1])
@pytest.mark.parametrize("seed", [0, 3, 5])
def test_new_map_lines_against_the_oracle(gpu_ctx, oracle, seed, use_grid):
    S, cur, last, (vc, vl), (lm_c, lm_l) = open_pair(gpu_ctx, oracle, seed)
    with cur, last:
        occ, skip = FS.host_flags(S["cur_state"], S["last_state"])
        o = FS.oracle_last_kf(oracle, vc, vl, S["cur"], S["last"], lm_c, lm_l, occ, skip, use_grid)
        print("created %d, matched %d, occupied %d, skipped %d" % (o[1].sum(), (o[0] >= 0).sum(), occ.sum(), skip.sum()))
        assert o[1].sum() >= 3 and skip.sum() >= 1 and occ.sum() >= 1
        first = 40000
        g = cur.new_map_lines(last, first, use_grid=use_grid)
        same_new_lines(g, o, first, int(occ.sum()))
        # the same call again: the created lines are held now, nothing else changed - nothing new, cnt0 grown by the lines made before
        g2 = cur.new_map_lines(last, first + 1000, use_grid=use_grid)
        assert g2["n_created"] == 0 and not g2["created"].any() and np.all(g2["new_id"] == -1)
        assert g2["n_held"] == g["n_held"] + g["n_created"]
        assert np.all(g2["match_last"][g["created"] != 0] == -1)


@pytest.mark.parametrize("use_grid", [0, 1])
def test_new_map_lines_leave_the_created_lines_in_the_frame(gpu_ctx, oracle, use_grid):
    """The roles advanced: a third frame as `cur`, the former `cur` - with the lines the first call created - as `last`.  The third frame
    tracked one of those new lines (its id is in the tracked list): that line must be skipped, by the id the device gave it."""
    S, cur, last, (vc, vl), (lm_c, lm_l) = open_pair(gpu_ctx, oracle, 0)
    first = 700
    with cur, last:
        g = cur.new_map_lines(last, first, use_grid=use_grid)
        made = np.flatnonzero(g["created"])
        assert made.size >= 3
        # the host's bookkeeping of what `cur` holds now
        c_id = S["cur_state"]["ln_line_id"].copy(); c_id[made] = g["new_id"][made]
        # the third frame sees what the last frame saw, from the last frame's pose; it holds two lines and tracked a created one and a held one
        third_state = dict(S["last_state"], ln_line_id=np.where(np.arange(96) % 40 == 7, FS.FOREIGN_ID0 + 100 + np.arange(96), -1).astype(np.int32),
                           tracked=np.array([g["new_id"][made[1]], FS.HELD_ID0 + int(np.flatnonzero(S["cur_state"]["ln_line_id"] >= 0)[0]), FS.FOREIGN_ID0 + 50], np.int32))
        with lines_frame(gpu_ctx, S["last"]) as third:
            v3 = FS.set_line_state(third, S["T_last"], third_state)
            occ3, skip3 = FS.host_flags(third_state, dict(ln_line_id=c_id))
            assert skip3[made[1]] == 1 and skip3.sum() == 2 and skip3[made[0]] == 0
            o = FS.oracle_last_kf(oracle, v3, vc, S["last"], S["cur"], lm_l, lm_c, occ3, skip3, use_grid)
            o_without = FS.oracle_last_kf(oracle, v3, vc, S["last"], S["cur"], lm_l, lm_c, occ3, np.zeros_like(skip3), use_grid)
            g3 = third.new_map_lines(cur, 9000, use_grid=use_grid)
            same_new_lines(g3, o, 9000, int(occ3.sum()))
            print("third frame: created %d, matched %d; without the skip flags matched %d" % (o[1].sum(), (o[0] >= 0).sum(), (o_without[0] >= 0).sum()))
            assert not np.any(g3["match_last"] == made[1])


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_build_lines_refusals_leave_the_frame_unchanged(gpu_ctx, chain_reference):
    sc, L = chain_scene()
    n = 96; dim = 72
    keep = [np.concatenate([[v], L[s][1:]]).astype(np.int32) for s in ("left_octave", "right_octave") for v in (-1, 65)]
    invalid = [dict(left=None), dict(left_octave=None), dict(desc_left=None), dict(right=None), dict(right_octave=None), dict(desc_right=None),
               dict(n_left=-1), dict(n_right=-1), dict(dim=0), dict(dim=-3), dict(sx=0.0), dict(sy=-1.0), dict(sx=float("nan"))]
    invalid += [dict(left_octave=keep[0].ctypes.data_as(abi.c_int32_p)), dict(left_octave=keep[1].ctypes.data_as(abi.c_int32_p)),
                dict(right_octave=keep[2].ctypes.data_as(abi.c_int32_p)), dict(right_octave=keep[3].ctypes.data_as(abi.c_int32_p))]
    # limits: one line more than the chain tracks next to 200 keypoints (8184), a descriptor wider than LLD_LINE_DIM_MAX, a row of distances
    # wider than the LDS ceiling (19 165 right lines at dim 72).  The second ceiling, (n_left + n_right) * 4 + 16 > 150 KiB, needs more than
    # 19 232 left lines next to 19 164 right ones and is always preceded by the line limit.
    big_l = dict(L, left_lines=np.zeros((8185, 4), np.float32), left_octave=np.zeros(8185, np.int32), desc=np.zeros((8185, dim), np.float32))
    big_r = dict(L, right_lines=np.zeros((19165, 4), np.float32), right_octave=np.zeros(19165, np.int32), desc_right=np.zeros((19165, dim), np.float32))
    wide = dict(L, desc=np.zeros((n, 129), np.float32), desc_right=np.zeros((L["right_lines"].shape[0], 129), np.float32))
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], L) as tf:
        assert tf.lib.fn("frame_build_lines")(None, None) == INVALID
        for over in invalid:
            assert FS.build_status(tf, L, **over) == INVALID, over
        for big in (big_l, big_r, wide):
            assert FS.build_status(tf, big) == UNSUPPORTED
        assert tf.lib.fn("frame_lines_download")(None, None, None) == INVALID
        assert tf.lib.fn("frame_lines_download")(tf.res.handle, None, None) == INVALID          # the frame has lines: line_matches is required
        same_records(run_chain(tf, sc), chain_reference)                                    # the frame still holds the lines of its valid build
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], None) as tf:                   # refused on a frame without a state, then a valid build
        assert FS.build_status(tf, L, dim=0) == INVALID and FS.build_status(tf, big_r) == UNSUPPORTED
        assert FS.build_status(tf, L) == abi.LLD_OK
        tf.n_lines = n
        same_records(run_chain(tf, sc), chain_reference)


def test_new_map_lines_refusals_leave_both_frames_unchanged(gpu_ctx, oracle):
    from lld_slam_amd import Context
    S, cur, last, (vc, vl), (lm_c, lm_l) = open_pair(gpu_ctx, oracle, 1)
    small = FS.two_frames(1, 96, 8)[2]
    with cur, last, lines_frame(gpu_ctx, None) as bare, lines_frame(gpu_ctx, S["last"]) as poseless, lines_frame(gpu_ctx, small) as dim8, Context(0) as other:
        FS.set_line_state(bare, S["T_last"], dict(ln_line_id=None, ln_x0=None, ln_dir=None, tracked=[]))      # a pose, but no lines
        FS.set_line_state(dim8, S["T_last"], dict(ln_line_id=None, ln_x0=None, ln_dir=None, tracked=[]))
        with lines_frame(other, S["last"]) as foreign:
            FS.set_line_state(foreign, S["T_last"], S["last_state"])
            for kw in (dict(cur_handle=None), dict(last_handle=None), dict(params=None), dict(want_out=False), dict(last_handle=cur.res.handle),
                       dict(last_handle=foreign.res.handle), dict(last_handle=dim8.res.handle), dict(last_handle=bare.res.handle), dict(cur_handle=bare.res.handle),
                       dict(last_handle=poseless.res.handle), dict(cur_handle=poseless.res.handle)):
                assert FS.new_lines_call(cur, last, 10, **kw) == INVALID, kw
            assert FS.new_lines_call(cur, last, -1) == INVALID
            assert FS.new_lines_call(cur, last, 2 ** 31 - 96) == INVALID                     # first_new_id + n_left = INT32_MAX + 1
        occ, skip = FS.host_flags(S["cur_state"], S["last_state"])
        o = FS.oracle_last_kf(oracle, vc, vl, S["cur"], S["last"], lm_c, lm_l, occ, skip, 1)
        first = 2 ** 31 - 1 - 96                                                              # the largest id the call takes
        same_new_lines(cur.new_map_lines(last, first), o, first, int(occ.sum()))
