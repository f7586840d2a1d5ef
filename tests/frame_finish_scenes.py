"""Scenes for lld_frame_track_finish / lld_frame_create_stereo_points (a helper module, not a test file): seeded frames with crafted depth
lists around the close-100 rule, the state a frame holds when Tracking::Track reaches its tail, thin runners for the device and for the
restatement (tests/frame_finish_ref.py), and the scene file of examples/frame_finish_harness.  Deterministic and cached: a test must not
modify a scene (copy first)."""
import dataclasses
import functools

import numpy as np

import frame_finish_ref as REF
from lld_slam_amd import orb_search, synth

CAM = tuple(float(np.float32(c)) for c in synth.KITTI_CAM)
TH = np.float32(35.0)                                    # mThDepth of every crafted scene
FIRST_ID = 70000
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def keypoints(n, seed=0):
    F = synth.make_orb_frame(500 + seed, max(n, 1))
    if n == 0:
        idx = np.zeros(0, np.int64)
        F = dataclasses.replace(F, desc=F.desc[idx], xy=F.xy[idx], octave=F.octave[idx], uright=F.uright[idx], angle=F.angle[idx]).normalise()
    return F


def pose(seed):
    """A float mTcw a little off the identity (so that mRwc and mOw matter)."""
    rng = np.random.default_rng(9100 + seed)
    w = rng.normal(0, 0.05, 3); t = rng.normal(0, 0.4, 3)
    th = np.linalg.norm(w); k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T = np.eye(4, dtype=np.float32); T[:3, :3] = R.astype(np.float32); T[:3, 3] = t.astype(np.float32)
    return T


def random_state(n, seed, held=0.6, obs=0.75, outlier=0.2):
    """What a frame holds after TrackLocalMap: MapPoints on `held` of the keypoints, `obs` of those with observations, mvbOutlier set on
    `outlier` of ALL keypoints (a flag outlives the point it was raised for: TrackLocalMap takes the point and leaves the flag)."""
    rng = np.random.default_rng(9200 + seed)
    has = rng.random(n) < held
    return dict(kp_id=np.where(has, 1000 + np.arange(n), -1).astype(np.int32), kp_obs=(has & (rng.random(n) < obs)).astype(np.uint8),
                kp_outlier=(rng.random(n) < outlier).astype(np.uint8), kp_world=np.where(has[:, None], rng.normal(0, 5, (n, 3)), 0).astype(np.float32))


def _mix(rng, n, close=0, far=0, at_th=0, extra=()):
    """n depths: `close` in (0.5, 0.99 th), `far` in (1.01 th, 5 th), `at_th` equal to th, the values of `extra`, the rest -1; shuffled."""
    d = np.concatenate([rng.uniform(0.5, 0.99 * float(TH), close), rng.uniform(1.01 * float(TH), 5 * float(TH), far), np.full(at_th, float(TH)),
                        np.asarray(extra, np.float64)]).astype(np.float32)
    assert d.size <= n
    d = np.concatenate([d, np.full(n - d.size, -1, np.float32)])
    return d[rng.permutation(n)]


def _depths(name, rng):
    if name == "close99": return _mix(rng, 160, close=99, far=41)                  # 101 visited: the far entry at rank 99 does not stop the walk
    if name == "close100": return _mix(rng, 160, close=100, far=40)                # the first far entry is visited, the second is not
    if name == "close150": return _mix(rng, 220, close=150, far=50)                # 151 visited
    if name == "all_close": return _mix(rng, 200, close=200)                       # no break
    if name == "few": return _mix(rng, 128, close=30, far=30)                      # fewer than 101 positive depths: all visited
    if name == "at_threshold": return _mix(rng, 200, close=120, far=30, at_th=10)  # == th: not close, and no reason to stop
    if name == "ties":                                                             # twelve distinct values, th among them: ties across rank 100 and at th
        vals = np.float32([3, 7, 7.5, 11, 19, 23, 30, 35, 35.5, 41, 60, 90])
        return vals[rng.integers(0, len(vals), 240)].astype(np.float32)
    if name == "special":                                                          # +inf sorts last and is far; -1, 0, -0, NaN never enter; a denormal is close
        return _mix(rng, 190, close=105, far=20, extra=[INF] * 4 + [NAN] * 5 + [0.0] * 4 + [-0.0] * 2 + [1e-42] * 2 + [-INF])
    if name == "inf_breaks":                                                       # exactly 100 finite close depths, then only +inf: the first +inf stops the walk
        return _mix(rng, 130, close=100, extra=[INF] * 6)
    if name == "n1": return np.float32([12.5])
    if name == "n1_none": return np.float32([-1])
    if name == "n0": return np.zeros(0, np.float32)
    if name == "n1000": return _mix(rng, 1000, close=520, far=300)
    if name == "n2049": return _mix(rng, 2049, close=1100, far=700)
    if name == "n4096": return np.concatenate([rng.uniform(0.5, 0.99 * float(TH), 2500), rng.uniform(1.01 * float(TH), 200, 1596)]).astype(np.float32)[rng.permutation(4096)]
    raise KeyError(name)


NAMES = ("close99", "close100", "close150", "all_close", "few", "at_threshold", "ties", "special", "inf_breaks", "n0", "n1", "n1_none", "n1000", "n2049", "n4096")


@functools.lru_cache(maxsize=None)
def scene(name, seed=0):
    """dict(F, depth, state, T, p): a frame, its mvDepth, what it holds, its float mTcw, NeedNewKeyFrame's scalars (a keyframe is made)."""
    rng = np.random.default_rng(9000 + seed + sum(map(ord, name)))
    depth = _depths(name, rng)
    n = depth.size
    return dict(name=name, F=keypoints(n, seed), depth=depth, state=random_state(n, seed + sum(map(ord, name))), T=pose(seed), p=dict(REF.DECISION_DEFAULTS))


def view_of(sc, T=None):
    return orb_search.frame_view(sc["T"] if T is None else T, CAM, sc["F"])


def expect_finish(sc, force=-1, th=TH, first=FIRST_ID, **over):
    """The restatement on the scene: (state on exit, result)."""
    v = view_of(sc)
    return REF.track_finish(sc["state"], sc["depth"], sc["F"].xy, CAM, np.array(v.Rcw, np.float32), np.array(v.Ow, np.float32), th, first, dict(sc["p"], **over), force)


def load_state(tf, sc, state=None, T=None):
    st = sc["state"] if state is None else state
    return tf.set_state(sc["T"] if T is None else T, st["kp_id"], st["kp_world"], st["kp_obs"], st["kp_outlier"])[0]


def device_finish(ctx, sc, force=-1, th=TH, first=FIRST_ID, **over):
    """lld_frame_track_finish on a frame of lld_frame_create loaded with the scene's state; the depths travel with the call."""
    from lld_slam_amd.tracking import DeviceTrackedFrame
    with DeviceTrackedFrame(ctx, sc["F"], CAM) as tf:
        load_state(tf, sc)
        return tf.finish(th, first, depth=sc["depth"], force=force, **dict(sc["p"], **over))


SCALARS = ("n_tracked_close", "n_non_tracked_close", "need", "interrupt_ba", "made", "n_visited", "n_created")
ARRAYS = ("created", "new_id", "x3d", "kp_point_id", "order")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_result(g, e, what="", arrays=ARRAYS):
    for k in SCALARS:
        if k in e: assert g[k] == e[k], (what, k, g[k], e[k])
    for k in arrays:
        if k in e: np.testing.assert_array_equal(bits(g[k]), bits(e[k]), err_msg=f"{what} {k}")


# ---------------------------------------------------------------------------------------------- the chain scene
W, H = 416, 240


@functools.lru_cache(maxsize=None)
def chain_keypoints():
    """The 300-keypoint stereo scene the frame-build tests craft their cases on (synth.make_stereo_scene(2, n=300, 416 x 240))."""
    sc = synth.make_stereo_scene(2, n=300, width=W, height=H)
    # the image bounds of the frames the line scenes of tests/frame_lines_scenes.py were drawn for (the chain test gives this frame their lines)
    sc["L"] = dataclasses.replace(sc["L"], max_x=1241.0, max_y=376.0).normalise(); sc["R"] = dataclasses.replace(sc["R"], max_x=1241.0, max_y=376.0).normalise()
    return sc


def chain_cam(sc):
    fx = float(np.float32(sc["mbf"]) / np.float32(sc["mb"]))
    return (fx, fx, W / 2.0, H / 2.0, float(sc["mbf"]))


def chain_scene(u_right, depth, ss=None, cam=None):
    """A tracking scene (the dict DeviceTrackedFrame's stages and oracle_tracking.track_frame take) around the built stereo frame whose
    ComputeStereoMatches gave (u_right, depth): the MapPoints are the frame's own stereo keypoints un-projected from a camera at the origin,
    a seventh of them without observations (visual-odometry points of the last frame), a ninth displaced by 2.2 pixels (of their level) so that PoseOptimization
    throws them out; mThDepth is the median positive depth, so half of the candidates are far."""
    ss = chain_keypoints() if ss is None else ss; L = ss["L"]; cam = chain_cam(ss) if cam is None else cam
    rng = np.random.default_rng(31)
    F = dataclasses.replace(L, uright=np.asarray(u_right, np.float32).copy()).normalise()
    fx, fy, cx, cy, bf = [np.float32(c) for c in cam]
    idx = np.nonzero(depth > 0)[0]
    th = np.float32(np.median(depth[idx]))
    idx = idx[np.arange(len(idx)) % 5 != 1]                                               # a fifth of the stereo keypoints have no MapPoint yet
    z = depth[idx].astype(np.float32)
    P = np.stack([(L.xy[idx, 0] - cx) * z / fx, (L.xy[idx, 1] - cy) * z / fy, z], 1).astype(np.float32)
    off =np.arange(len(idx)) % 9 == 4
    shift = (np.float32(2.2) * L.scale[L.octave[idx]] * z / fx).astype(np.float32)      # 2.2 sigma in u, v and uR: inside SearchLocalPoints' window, chi2 = 14.5 > 7.815
    P[off, 0] += shift[off]; P[off, 1] += shift[off]
    desc = L.desc[idx].copy()
    for r in range(len(idx)):
        for b in rng.integers(0, 256, 6):
            desc[r, b >> 5] ^= np.uint32(1) << np.uint32(b & 31)
    obs = (np.arange(len(idx)) % 7 != 3).astype(np.uint8)
    dist = np.linalg.norm(P, axis=1).astype(np.float32)
    maxd = (dist * L.scale[L.octave[idx]]).astype(np.float32)
    ids = (100 + np.arange(len(idx))).astype(np.int32)
    half = np.arange(len(idx)) % 2 == 0
    last = dict(world_pos=P[half], valid=np.ones(int(half.sum()), np.uint8), octave=L.octave[idx][half].copy(), angle=L.angle[idx][half].copy(), desc=desc[half],
                has_obs=obs[half])
    mp = dict(world_pos=P, normal=(P / dist[:, None]).astype(np.float32), max_distance=maxd, min_distance=(maxd / L.scale[-1]).astype(np.float32), desc=desc,
              has_obs=obs, skip=np.zeros(len(idx), np.uint8))
    T = np.eye(4, dtype=np.float32); T[:3, 3] = [0.03, -0.01, 0.02]
    return dict(frame=F, cam=cam, Tcw_guess=T, last=last, last_ids=ids[half], map_points=mp, map_ids=ids, depth=np.asarray(depth, np.float32), th_depth=th,
                world_of=dict(zip(ids.tolist(), P)), obs_of=dict(zip(ids.tolist(), obs.tolist())))


def chain_entry_state(sc, rec2, rgbd):
    """mCurrentFrame as TrackLocalMap leaves it, from the stage's record (ids and flags as PoseOptimization left them, before the discard):
    RGB-D - no point leaves, mvbOutlier stays; STEREO - the flagged points leave (src/Tracking.cc:1171-1172), mvbOutlier stays."""
    ids = np.asarray(rec2["kp_point_id"], np.int32).copy(); out = np.asarray(rec2["kp_outlier"], np.uint8).copy()
    n = ids.size
    world = np.zeros((n, 3), np.float32); obs = np.zeros(n, np.uint8)
    for k in np.nonzero(ids >= 0)[0]:
        world[k] = sc["world_of"][int(ids[k])]; obs[k] = sc["obs_of"][int(ids[k])]
    if not rgbd:
        ids[out != 0] = -1
    return dict(kp_id=ids, kp_obs=np.where(ids >= 0, obs, 0).astype(np.uint8), kp_outlier=out, kp_world=world)


def chain_expect(lib, sc, rec2, rgbd, first=FIRST_ID, **over):
    """The restatement on the chain scene from a stage-2 record (the oracle's or the device's).  The frame's view is Frame::SetPose +
    UpdatePoseMatrices of the stage's optimised pose, formed as oracle_tracking forms it (`lib`: the library whose Converter narrows the pose)."""
    import oracle_tracking as OT
    from lld_slam_amd import host
    T = np.asarray(host.se3_to_tcw_f32(lib, np.asarray(rec2["pose_qt"], np.float64)), np.float32).reshape(4, 4)
    v = OT.pose_view(T, sc["cam"], sc["frame"])
    p = dict(REF.DECISION_DEFAULTS, n_matches_inliers=int(rec2["n_points_map"]), n_ref_matches=4 * int(rec2["n_points_map"]) + 40, **over)
    st = chain_entry_state(sc, rec2, rgbd)
    return st, REF.track_finish(st, sc["depth"], sc["frame"].xy, sc["cam"], np.array(v.Rcw, np.float32), np.array(v.Ow, np.float32), sc["th_depth"], first, p), p


# ---------------------------------------------------------------------------------------------- the scene file of examples/frame_finish_harness
def write_harness_scene(path, sc, force=-1, th=TH, first=FIRST_ID, mode=-1, **over):
    """A scene() dict as the flat binary examples/frame_finish_harness reads.  mode -1: lld_frame_track_finish; 0 / 1: lld_frame_create_stereo_points."""
    F = sc["F"]; st = sc["state"]; p = dict(sc["p"], **over)
    f32 = lambda a: np.ascontiguousarray(a, np.float32); i32 = lambda a: np.ascontiguousarray(a, np.int32); u8 = lambda a: np.ascontiguousarray(a, np.uint8)
    with open(path, "wb") as f:
        i32([F.n, F.scale.shape[0], int(first), int(force), int(mode), 0, 0, 0]).tofile(f)
        f32([F.min_x, F.min_y, F.max_x, F.max_y, F.width_inv, F.height_inv, float(th), 0.0]).tofile(f)
        f32(F.scale).tofile(f); f32(F.sigma2).tofile(f); f32(F.inv_sigma2).tofile(f)
        np.ascontiguousarray(CAM, np.float64).tofile(f)
        np.ascontiguousarray(F.desc, np.uint32).tofile(f); f32(F.xy).tofile(f); i32(F.octave).tofile(f); f32(F.uright).tofile(f); f32(F.angle).tofile(f)
        f.write(bytes(view_of(sc))); f32(sc["T"]).tofile(f)
        f32(sc["depth"]).tofile(f); i32(st["kp_id"]).tofile(f); f32(st["kp_world"]).tofile(f); u8(st["kp_obs"]).tofile(f); u8(st["kp_outlier"]).tofile(f)
        i32([p[k] for k in ("only_tracking", "mapper_stopped", "mapper_idle", "keyframes_in_queue", "set_not_stop_ok", "monocular", "max_frames", "min_frames",
                            "n_keyframes", "n_ref_matches", "n_matches_inliers")] + [p.get("sensor_rgbd", 0)]).tofile(f)
        np.ascontiguousarray([p["frame_id"], p["last_reloc_frame_id"], p["last_keyframe_id"]], np.int64).tofile(f)


def read_harness_result(path, n):
    """What examples/frame_finish_harness wrote: dict(hpp=result of lld_amd::TrackedFrame::Finish, adapter=result and object graph of
    FrameOnDevice::NeedNewKeyFrame + CreateNewKeyFrame, host=the host loops of the parent route on the same state, last_frame=the object graph
    of FrameOnDevice::UpdateLastFrame on the same frame)."""
    def result(f):
        d = dict(zip(SCALARS, (int(v) for v in np.fromfile(f, np.int32, 7))))
        d.update(created=np.fromfile(f, np.uint8, n), new_id=np.fromfile(f, np.int32, n), x3d=np.fromfile(f, np.float32, 3 * n).reshape(-1, 3),
                 kp_point_id=np.fromfile(f, np.int32, n), order=np.fromfile(f, np.int32, n))
        return d
    with open(path, "rb") as f:
        hpp = result(f)
        host = result(f)
        ad = dict(need=int(np.fromfile(f, np.int32, 1)[0]), interrupt_ba=int(np.fromfile(f, np.int32, 1)[0]), made=int(np.fromfile(f, np.int32, 1)[0]),
                  n_map_points=int(np.fromfile(f, np.int32, 1)[0]))
        ad.update(frame_ids=np.fromfile(f, np.int32, n), kf_ids=np.fromfile(f, np.int32, n), obs_index=np.fromfile(f, np.int32, n),
                  world=np.fromfile(f, np.float32, 3 * n).reshape(-1, 3), map_order=np.fromfile(f, np.int32, int(ad["n_map_points"])))
        n_tmp = int(np.fromfile(f, np.int32, 1)[0])
        last = dict(frame_ids=np.fromfile(f, np.int32, n), world=np.fromfile(f, np.float32, 3 * n).reshape(-1, 3), temporal_ids=np.fromfile(f, np.int32, n_tmp))
        assert f.read() == b""
    return dict(hpp=hpp, host=host, adapter=ad, last_frame=last)
