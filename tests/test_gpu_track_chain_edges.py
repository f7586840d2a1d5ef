"""lld_frame_track_* at the edges of its rules and sizes, against the oracle's own run of the sequence (oracle/oracle_tracking.py), with the
records, tolerances and LM slack of tests/test_gpu_track_chain.py: every boundary scene of tests/track_scenes.py (the wide retry, the failure
exit, PoseOptimization's early return and line classification, the return values), a frame of LLD_ORB_MAX_KEYPOINTS keypoints, a frame without
keypoints, the most lines the chain accepts, the tracked-line list at capacity, and the calls the chain refuses before it queues anything."""
import ctypes as C

import numpy as np
import pytest

import oracle_tracking as OT
import track_scenes as TS
from lld_slam_amd import abi, orb_search, synth
from lld_slam_amd.tracking import DeviceTrackedFrame
from test_gpu_track_chain import _lm_count_log, run_device, same_record  # noqa: F401  (the LM count log covers these records too)

pytestmark = pytest.mark.gpu

MAX_KP = 4096                                                              # LLD_ORB_MAX_KEYPOINTS


def _same_stages(g, e):
    same_record(g[0], e[0]); same_record(g[1], e[1])


@pytest.mark.parametrize("name", TS.NAMES)
def test_boundary_scene(gpu_ctx, oracle, name):
    sc, params = TS.scene(name)
    key, want, _, _ = TS.BOUNDARIES[name]
    dev = {k: int(v) for k, v in params.items()}
    g = run_device(gpu_ctx, sc, **dev)
    e = OT.track_frame(sc, **params)
    assert e[0][key] == want
    _same_stages(g, e)


def test_max_keypoints_full_last_frame_and_local_map(gpu_ctx, oracle):
    # (seed 31's stage 2 ends its last LM round 4 iterations / 9 trials apart from the oracle's - over LM_IT_SLACK / LM_TRIAL_SLACK - with ids,
    # flags and pose equal: the last-bits effect tests/test_gpu_track_chain.py describes)
    sc = synth.make_tracking_scene(38, n_kp=MAX_KP, n_map=6000, n_last=MAX_KP)
    assert sc["frame"].n == MAX_KP and len(sc["last_ids"]) == MAX_KP
    g = run_device(gpu_ctx, sc)
    e = OT.track_frame(sc)
    _same_stages(g, e)
    assert e[0]["n_search"] > 1000 and e[1]["n_points"] > 2000


def _empty_frame(F):
    return orb_search.Frame(desc=np.zeros((0, 8), np.uint32), xy=np.zeros((0, 2), np.float32), octave=np.zeros(0, np.int32), uright=np.zeros(0, np.float32),
                            angle=np.zeros(0, np.float32), min_x=F.min_x, min_y=F.min_y, max_x=F.max_x, max_y=F.max_y, scale=F.scale, sigma2=F.sigma2,
                            inv_sigma2=F.inv_sigma2).normalise()


def test_frame_without_keypoints(gpu_ctx, oracle):
    """nt = 0: nothing to match; AddLinesFrom still runs and PoseOptimization returns before optimising in both stages."""
    sc = synth.make_tracking_scene(33, n_kp=600, n_map=700, n_last=300)
    sc["frame"] = _empty_frame(sc["frame"])
    g = run_device(gpu_ctx, sc)
    e = OT.track_frame(sc)
    _same_stages(g, e)
    assert e[0]["n_search"] == 0 and e[1]["n_search"] == 0 and e[1]["n_lines_matched"] > 0 and e[1]["n_point_edges"] == 0


MAX_LINES = 4088                                                          # include/lld_amd.h, lld_frame_set_lines: every nt <= 4096


def test_most_lines_the_chain_accepts(gpu_ctx, oracle):
    sc = synth.make_tracking_scene(32, n_kp=MAX_KP, n_map=4500, n_last=2000, n_lines=MAX_LINES, n_map_lines=4200, n_last_lines=2000)
    g = run_device(gpu_ctx, sc)
    e = OT.track_frame(sc)
    _same_stages(g, e)
    assert e[1]["n_lines_matched"] > 1000
    # one more line is refused by lld_frame_set_lines, before anything is built
    more = dict(sc["lines"])
    more["left_lines"] = np.concatenate([more["left_lines"], more["left_lines"][:1]]); more["left_octave"] = np.concatenate([more["left_octave"], more["left_octave"][:1]])
    more["line_matches"] = np.concatenate([more["line_matches"], [-1]]).astype(np.int32); more["desc"] = np.concatenate([more["desc"], more["desc"][:1]])
    with pytest.raises(RuntimeError, match="lld_frame_set_lines"):
        DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], more)
    # ... and with fewer keypoints the tables leave room for twice as many
    small = synth.make_tracking_scene(34, n_kp=1000, n_map=1200, n_last=600, n_lines=2 * MAX_LINES + 8, n_map_lines=300, n_last_lines=150)
    g = run_device(gpu_ctx, small)
    _same_stages(g, OT.track_frame(small))


def _capacity_scene(n=8, depth=(2.0, 4.0)):
    """Every frame line is tracked in TrackWithMotionModel, thrown out by its PoseOptimization and tracked again by TrackLocalMap: the tracked
    list holds 2 nl ids (tracked_cap = 2 nl + 16).  The frame's lines are seen at the TRUE pose; the last frame's MapLines are their
    back-projections through the PREDICTED pose (found by AddLinesFrom there, far off once the points have moved the pose), the local map's
    their back-projections through the true pose, under other ids."""
    sc = synth.make_tracking_scene(35, n_kp=600, n_map=700, n_last=300, rot_deg=0.25, trans=0.15)
    fx, fy, cx, cy, bf = [float(np.float32(c)) for c in sc["cam"]]
    b = bf / fx
    rng = np.random.default_rng(35)
    z = rng.uniform(*depth, (n, 2))
    px = np.stack([rng.uniform(200, 1000, n), rng.uniform(60, 300, n)], 1)
    ends = []
    for k in range(2):
        u = px[:, 0] + (k * 2 - 1) * rng.uniform(30, 60, n); v = px[:, 1] + (k * 2 - 1) * rng.uniform(10, 30, n)
        ends.append(np.stack([(u - cx) * z[:, k] / fx, (v - cy) * z[:, k] / fy, z[:, k]], 1))
    A, B = ends

    def proj(X, shift):
        return np.stack([fx * (X[:, 0] - shift) / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    left = np.concatenate([proj(A, 0.0), proj(B, 0.0)], 1).astype(np.float32)
    right = np.concatenate([proj(A, b), proj(B, b)], 1).astype(np.float32)
    dim = 72
    desc = rng.normal(size=(n, dim)); desc /= np.linalg.norm(desc, axis=1, keepdims=True)
    lines = dict(left_lines=left, left_octave=np.zeros(n, np.int32), right_lines=right, right_octave=np.zeros(n, np.int32),
                 line_matches=np.arange(n, dtype=np.int32), desc=desc.astype(np.float32))

    def world(T):
        T = np.asarray(T, np.float64); R, t = T[:3, :3], T[:3, 3]
        Aw, Bw = (R.T @ (A - t).T).T, (R.T @ (B - t).T).T
        d = (Bw - Aw) / np.linalg.norm(Bw - Aw, axis=1, keepdims=True)
        X0 = Aw - np.sum(Aw * d, axis=1, keepdims=True) * d
        return dict(X0=X0, dir=d, X1=Aw, X2=Bw, desc=desc.astype(np.float32), skip=np.zeros(n, np.uint8))
    sc["lines"] = lines
    sc["last_lines"] = dict(world(sc["Tcw_guess"]), id=np.arange(1000, 1000 + n, dtype=np.int32))
    sc["local_lines"] = dict(world(sc["Tcw_true"]), id=np.arange(2000, 2000 + n, dtype=np.int32))
    return sc


def test_tracked_lines_at_capacity(gpu_ctx, oracle):
    sc = _capacity_scene()
    e = OT.track_frame(sc)
    nl = len(sc["lines"]["left_lines"])
    assert e[0]["n_lines_matched"] == nl and e[0]["n_lines"] == 0 and e[1]["n_lines_matched"] == nl, \
        (e[0]["n_lines_matched"], e[0]["n_lines"], e[1]["n_lines_matched"])
    g = run_device(gpu_ctx, sc)
    _same_stages(g, e)


# ---------------------------------------------------------------------------------------------------- refusals
def _records(tf, sc):
    tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc["last_lines"])
    tf.track_local_map(sc["map_points"], sc["map_ids"], sc["local_lines"])
    return tf.download()


def _identical(a, b):
    for x, y in zip(a, b):
        same_record(x, y, exact_pose=True)


def test_refusals_leave_the_handle_as_a_fresh_one(gpu_ctx, oracle):
    """fx or fy <= 0 (lld_track_params_default leaves cam zeroed) and a frame without level_inv_sigma2 are refused by both stage-1 calls
    before anything is queued; the handle then tracks exactly as a fresh one."""
    sc = synth.make_tracking_scene(36, n_kp=800, n_map=1000, n_last=500)
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc["lines"]) as tf:
        fresh = _records(tf, sc)
    nt = sc["frame"].n
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], sc["lines"]) as tf:
        good = abi.Camera(*[float(np.float32(c)) for c in sc["cam"]])
        for bad in ((0.0, good.fy), (good.fx, -1.0), (float("nan"), good.fy)):
            tf.params.cam = abi.Camera(bad[0], bad[1], good.cx, good.cy, good.bf)
            with pytest.raises(RuntimeError, match="lld_frame_track_motion_model"):
                tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc["last_lines"])
            with pytest.raises(RuntimeError, match="lld_frame_track_set_state"):
                tf.set_state(sc["Tcw_guess"], np.full(nt, -1, np.int32), np.zeros((nt, 3), np.float32))
        tf.params.cam = good
        _identical(_records(tf, sc), fresh)
        # after a completed sequence, too
        tf.params.cam = abi.Camera(0.0, 0.0, 0.0, 0.0, 0.0)
        with pytest.raises(RuntimeError):
            tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"], sc["last_lines"])
        tf.params.cam = good
        _identical(_records(tf, sc), fresh)
    # a frame created without level_inv_sigma2
    with DeviceTrackedFrame(gpu_ctx, sc["frame"], sc["cam"], None) as tf:
        tf.res.close()
        p = orb_search.prepare(sc["frame"], np.zeros((0, 8), np.uint32), candidates=orb_search.CAND_GRID, accept_max=orb_search.TH_HIGH)
        p.s.level_inv_sigma2 = None
        h = C.c_void_p()
        fn = gpu_ctx.lib.fn("frame_create"); fn.argtypes = [C.c_void_p, C.POINTER(orb_search.OrbSearch), C.POINTER(C.c_void_p)]; fn.restype = C.c_int
        assert fn(gpu_ctx.handle, C.byref(p.s), C.byref(h)) == abi.LLD_OK
        tf.res.handle = h
        with pytest.raises(RuntimeError, match="lld_frame_track_motion_model"):
            tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"])
        with pytest.raises(RuntimeError, match="lld_frame_track_set_state"):
            tf.set_state(sc["Tcw_guess"], np.full(nt, -1, np.int32), np.zeros((nt, 3), np.float32))
