"""Scenes for lld_frame_build_lines / lld_frame_new_map_lines (a helper module, not a test file): wide-baseline stereo frames with both
descriptor sets, the pair of frames MatchLinesLastKF works on with the state each frame holds, and thin callers that fill the ABI structs
from those dicts.  Everything is deterministic and cached; a test must not modify a scene (copy first)."""
import ctypes as C
import functools

import numpy as np

from lld_slam_amd import abi, orb_search, synth
from lld_slam_amd.abi import c_double_p, c_float_p, c_int32_p, c_uint8_p

TAU, MIN_LEN = 0.9, 20
BASELINE = 2.0
DBL_MAX = np.finfo(np.float64).max
FX, FY, CX, CY = [float(np.float32(c)) for c in synth.KITTI_CAM[:4]]
# a rig whose Frame reports the scenes' 2 m baseline: mbf = b * fx, so that mb = mbf / fx (floats) is 2 again
CAM = (FX, FY, CX, CY, float(np.float32(BASELINE * FX)))
K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])
B = float(np.float32(np.float32(CAM[4]) / np.float32(FX)))
STEREO = dict(K=K, b=B, tau=TAU, min_line_length=MIN_LEN, is_stereo=1)


def _both_sides(fr, rng, dim):
    """Gives one frame of make_two_frame_lines what the stereo matcher reads: octaves (equal on partners) and right descriptors (the partner's
    left descriptor plus N(0, 0.05) noise; unit random vectors on right lines without a partner)."""
    n = fr["left_lines"].shape[0]; nr = fr["right_lines"].shape[0]
    lo = rng.integers(0, 3, n).astype(np.int32); ro = rng.integers(0, 3, nr).astype(np.int32)
    dr = rng.normal(size=(nr, dim)); dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    lm = fr["line_matches"]; has = lm >= 0
    ro[lm[has]] = lo[has]
    dr[lm[has]] = fr["desc"][has] + rng.normal(0, 0.05, (int(has.sum()), dim))
    return dict(left_lines=fr["left_lines"], left_octave=lo, right_lines=fr["right_lines"], right_octave=ro, desc=fr["desc"],
                desc_right=dr.astype(np.float32), stereo=STEREO)


@functools.lru_cache(maxsize=None)
def two_frames(seed, n=96, dim=72):
    """(P, cur, last, truth) of synth.make_two_frame_lines(seed, n) with `cur` and `last` completed by _both_sides: dicts a DeviceTrackedFrame
    takes as `lines` on the lld_frame_build_lines route."""
    P, cur, last, truth = synth.make_two_frame_lines(seed, n_lines=n, dim=dim, baseline=BASELINE)
    rng = np.random.default_rng(77000 + seed)
    c = _both_sides(cur, rng, dim); l = _both_sides(last, rng, dim)
    c["occupied"] = cur["occupied"]; l["skip"] = last["skip"]
    return P, c, l, truth


def wide_stereo_scene(seed, n=96, dim=72):
    """One wide-baseline stereo frame (the current frame of two_frames)."""
    return two_frames(seed, n, dim)[1]


def kitti_stereo_scene():
    """line_scenes.stereo_scene() under the names of the dicts above (KITTI's 0.54 m baseline, 91 x 81 lines)."""
    import line_scenes
    s = line_scenes.stereo_scene()[0]
    return dict(left_lines=s["left"], left_octave=s["left_octave"], right_lines=s["right"], right_octave=s["right_octave"], desc=s["desc_left"],
                desc_right=s["desc_right"], stereo=dict(K=s["K"], b=s["b"], tau=TAU, min_line_length=MIN_LEN, is_stereo=1))


def oracle_stereo(oracle, L, is_stereo=None):
    """TwoFrameLineMatcher::MatchLines of the CPU oracle on a lines dict: (line_matches, match_dist, gate)."""
    from lld_slam_amd import host
    s = L["stereo"]
    return host.line_stereo_call(oracle.lib(), None, s["K"], s["b"], s["tau"], s["min_line_length"], L["left_lines"], L["left_octave"], L["desc"],
                                 L["right_lines"], L["right_octave"], L["desc_right"], s["is_stereo"] if is_stereo is None else is_stereo, True)


def device_stereo(ctx, L, is_stereo=None):
    """lld_line_match_stereo, the stand-alone call, on the same dict: (line_matches, match_dist)."""
    from lld_slam_amd import host
    s = L["stereo"]
    return host.line_stereo_call(ctx.lib, ctx.handle, s["K"], s["b"], s["tau"], s["min_line_length"], L["left_lines"], L["left_octave"], L["desc"],
                                 L["right_lines"], L["right_octave"], L["desc_right"], s["is_stereo"] if is_stereo is None else is_stereo, False)


@functools.lru_cache(maxsize=None)
def keypoint_frame(n=200):
    """The keypoint side every line frame of these tests is created with (lld_frame_create needs one; the line routines do not read it)."""
    return synth.make_orb_frame(300, n)


def tcw_f32(T_cam_to_world):
    """mTcw (float) of a camera-to-world pose."""
    return np.linalg.inv(np.asarray(T_cam_to_world, np.float64)).astype(np.float32)


def build_struct(L, keep, F=None, **over):
    """lld_frame_lines_build of a lines dict; `over` replaces fields afterwards (None: a NULL pointer).  `keep` collects the arrays."""
    F = keypoint_frame() if F is None else F
    k = dict(left=np.ascontiguousarray(L["left_lines"], np.float32).reshape(-1, 4), lo=np.ascontiguousarray(L["left_octave"], np.int32),
             right=np.ascontiguousarray(L["right_lines"], np.float32).reshape(-1, 4), ro=np.ascontiguousarray(L["right_octave"], np.int32),
             dl=np.ascontiguousarray(L["desc"], np.float32), dr=np.ascontiguousarray(L["desc_right"], np.float32))
    keep.append(k)
    S = abi.FrameLinesBuild()
    S.n_left = k["left"].shape[0]; S.left = k["left"].ctypes.data_as(c_float_p); S.left_octave = k["lo"].ctypes.data_as(c_int32_p); S.desc_left = k["dl"].ctypes.data_as(c_float_p)
    S.n_right = k["right"].shape[0]; S.right = k["right"].ctypes.data_as(c_float_p); S.right_octave = k["ro"].ctypes.data_as(c_int32_p); S.desc_right = k["dr"].ctypes.data_as(c_float_p)
    S.dim = k["dl"].shape[1]; S.sx = 1.0 / float(F.max_x); S.sy = 1.0 / float(F.max_y)
    s = L["stereo"]
    S.stereo = abi.LineStereoParams((C.c_double * 9)(*np.asarray(s["K"], np.float64).ravel()), float(s["b"]), float(s["tau"]), int(s["min_line_length"]), int(s["is_stereo"]))
    for name, v in over.items():
        setattr(S, name, v)
    return S


def build_status(tf, L, **over):
    """Status of lld_frame_build_lines on the handle of DeviceTrackedFrame `tf`."""
    keep = []
    S = build_struct(L, keep, tf.F, **over)
    return tf.lib.fn("frame_build_lines")(tf.res.handle, C.byref(S))


# ---------------------------------------------------------------------------------------------- MatchLinesLastKF between two resident frames
HELD_ID0, LAST_ID0, FOREIGN_ID0 = 5000, 1000, 9000


@functools.lru_cache(maxsize=None)
def last_kf_scene(seed, n=96):
    """What the two frames of two_frames(seed, n) hold when CreateNewKeyFrame calls MatchLinesLastKF, as lld_frame_track_set_state takes it:
       cur   holds a line (id HELD_ID0 + i, some X0 / direction) on every line the scene marks occupied; its tracked list names the ids the
             last frame holds on the scene's skip lines, and FOREIGN ids nobody holds;
       last  holds a line (id LAST_ID0 + li) on every skip line and on every third other line.
    Returns dict(P, cur, last, cur_state, last_state, T_cur, T_last) - T_*: the float mTcw of the two frames."""
    P, cur, last, _ = two_frames(seed, n)
    rng = np.random.default_rng(88000 + seed)
    nl = cur["left_lines"].shape[0]; nll = last["left_lines"].shape[0]
    occ = cur["occupied"].astype(bool)
    c_id = np.where(occ, HELD_ID0 + np.arange(nl), -1).astype(np.int32)
    c_x0 = np.where(occ[:, None], rng.normal(0, 3, (nl, 3)), 0.0); c_dir = rng.normal(size=(nl, 3)); c_dir /= np.linalg.norm(c_dir, axis=1, keepdims=True)
    c_dir = np.where(occ[:, None], c_dir, 0.0)
    skip = last["skip"].astype(bool)
    l_has = skip | (np.arange(nll) % 3 == 0)
    l_id = np.where(l_has, LAST_ID0 + np.arange(nll), -1).astype(np.int32)
    l_x0 = np.where(l_has[:, None], rng.normal(0, 3, (nll, 3)), 0.0); l_dir = rng.normal(size=(nll, 3)); l_dir /= np.linalg.norm(l_dir, axis=1, keepdims=True)
    l_dir = np.where(l_has[:, None], l_dir, 0.0)
    tracked = np.concatenate([l_id[skip], FOREIGN_ID0 + np.arange(5)]).astype(np.int32)
    tracked = tracked[rng.permutation(tracked.size)]
    return dict(P=P, cur=cur, last=last, T_cur=tcw_f32(P["T_curr"]), T_last=tcw_f32(P["T_last"]),
                cur_state=dict(ln_line_id=c_id, ln_x0=c_x0, ln_dir=c_dir, tracked=tracked),
                last_state=dict(ln_line_id=l_id, ln_x0=l_x0, ln_dir=l_dir, tracked=np.zeros(0, np.int32)))


def set_line_state(tf, Tcw, st):
    """lld_frame_track_set_state with no MapPoints and the lines of `st`; returns the frame's view (orb_search.FrameView)."""
    nt = tf.F.n
    view, _ = tf.set_state(Tcw, np.full(nt, -1, np.int32), np.zeros((nt, 3), np.float32), ln_line_id=st["ln_line_id"], ln_x0=st["ln_x0"], ln_dir=st["ln_dir"],
                           tracked_line_id=st["tracked"])
    return view


def host_flags(cur_state, last_state):
    """occupied / skip as the host derives them from the same lists: the current frame's held lines; the last frame's held lines whose id the
    current frame tracked (a held line counts as tracked, src/Tracking.cc:1117)."""
    c_id = np.asarray(cur_state["ln_line_id"]); l_id = np.asarray(last_state["ln_line_id"])
    tracked = np.concatenate([c_id[c_id >= 0], np.asarray(cur_state["tracked"], np.int64)])
    return (c_id >= 0).astype(np.uint8), ((l_id >= 0) & np.isin(l_id, tracked)).astype(np.uint8)


def oracle_last_kf(oracle, view_cur, view_last, cur, last, cur_lm, last_lm, occupied, skip, use_grid, thr=6.0, md_thr=0.9):
    """oracle.line_match_last_frame with the cameras this build defines for resident frames ([Rwc | Ow] of each frame's view)."""
    import oracle_tracking as OT
    c = dict(left_lines=cur["left_lines"], right_lines=cur["right_lines"], line_matches=cur_lm, desc=cur["desc"], occupied=occupied)
    l = dict(left_lines=last["left_lines"], right_lines=last["right_lines"], line_matches=last_lm, desc=last["desc"], left_octave=last["left_octave"], skip=skip)
    F = keypoint_frame()
    return oracle.line_match_last_frame(K, OT.frame_lines_camera(view_cur), OT.frame_lines_camera(view_last), B, thr, md_thr, 1.0 / float(F.max_x), 1.0 / float(F.max_y),
                                        c, l, use_grid)


def new_lines_call(tf_cur, tf_last, first_new_id, use_grid=1, cur_handle=..., last_handle=..., params=..., want_out=True):
    """Status of lld_frame_new_map_lines with explicit control over every argument (for the refusals)."""
    n = tf_cur.n_lines
    a = dict(match_last=np.full(n, -1, np.int32), created=np.zeros(n, np.uint8), x0=np.zeros((n, 3)), dir=np.zeros((n, 3)), new_id=np.full(n, -1, np.int32))
    P = abi.FrameNewLinesParams(6.0, 0.9, int(use_grid), int(first_new_id))
    R = abi.FrameNewLinesResult(0, 0, a["match_last"].ctypes.data_as(c_int32_p), a["created"].ctypes.data_as(c_uint8_p), a["x0"].ctypes.data_as(c_double_p),
                                a["dir"].ctypes.data_as(c_double_p), a["new_id"].ctypes.data_as(c_int32_p))
    hc = tf_cur.res.handle if cur_handle is ... else cur_handle
    hl = tf_last.res.handle if last_handle is ... else last_handle
    return tf_cur.lib.fn("frame_new_map_lines")(hc, hl, C.byref(P) if params is ... else params, C.byref(R) if want_out else None)


# ---------------------------------------------------------------------------------------------- the scene file of examples/frame_lines_harness
def adapter_last_ids(S):
    """The last frame's MapLine ids for the object-graph route: what a frame tracked there is exactly what it holds (FrameOnDevice::SetFrameState),
    so the lines the last frame holds on its first skip lines ARE lines the current frame holds (the same MapLine in both frames)."""
    c_id = S["cur_state"]["ln_line_id"]; l_id = S["last_state"]["ln_line_id"].copy()
    held = c_id[c_id >= 0]; skip = np.flatnonzero(S["last"]["skip"])
    k = min(held.size, skip.size)
    l_id[skip[:k]] = held[:k]
    return l_id


def write_pair_scene(path, S, first_new_id):
    """last_kf_scene S as the flat binary examples/frame_lines_harness reads."""
    import oracle_tracking as OT
    F = keypoint_frame()
    f32 = lambda a: np.ascontiguousarray(a, np.float32); i32 = lambda a: np.ascontiguousarray(a, np.int32); f64 = lambda a: np.ascontiguousarray(a, np.float64)
    cur, last = S["cur"], S["last"]
    with open(path, "wb") as f:
        i32([F.n, F.scale.shape[0], cur["left_lines"].shape[0], cur["right_lines"].shape[0], last["left_lines"].shape[0], last["right_lines"].shape[0],
             cur["desc"].shape[1], first_new_id]).tofile(f)
        f32([F.min_x, F.min_y, F.max_x, F.max_y, F.width_inv, F.height_inv]).tofile(f)
        f32(F.scale).tofile(f); f32(F.sigma2).tofile(f); f32(F.inv_sigma2).tofile(f)
        f64(CAM).tofile(f); f64(list(K.ravel()) + [B, TAU, MIN_LEN]).tofile(f)
        np.ascontiguousarray(F.desc, np.uint32).tofile(f); f32(F.xy).tofile(f); i32(F.octave).tofile(f); f32(F.uright).tofile(f); f32(F.angle).tofile(f)
        for L, T, st, ids_adapter in ((cur, S["T_cur"], S["cur_state"], S["cur_state"]["ln_line_id"]), (last, S["T_last"], S["last_state"], adapter_last_ids(S))):
            view = orb_search.frame_view(T, CAM, F)
            f32(L["left_lines"]).tofile(f); i32(L["left_octave"]).tofile(f); f32(L["desc"]).tofile(f)
            f32(L["right_lines"]).tofile(f); i32(L["right_octave"]).tofile(f); f32(L["desc_right"]).tofile(f)
            f.write(bytes(view)); f32(T).tofile(f); f64(OT.frame_lines_camera(view)).tofile(f)
            i32(st["ln_line_id"]).tofile(f); i32(ids_adapter).tofile(f); f64(st["ln_x0"]).tofile(f); f64(st["ln_dir"]).tofile(f)
            i32([len(st["tracked"])]).tofile(f); i32(st["tracked"]).tofile(f)


def read_pair_result(path, n_cur, n_last):
    """What examples/frame_lines_harness wrote: dict(hpp=..., device=..., host=...)."""
    def graph(f):
        d = dict(ret=int(np.fromfile(f, np.int32, 1)[0]), n_map=int(np.fromfile(f, np.int32, 1)[0]), match_last=np.fromfile(f, np.int32, n_cur))
        d.update(created_id=np.fromfile(f, np.int32, n_cur), bookkeeping=np.fromfile(f, np.int32, n_cur), frame_ids=np.fromfile(f, np.int32, n_cur),
                 kf_ids=np.fromfile(f, np.int32, n_cur), x0=np.fromfile(f, np.float64, 3 * n_cur).reshape(-1, 3), dir=np.fromfile(f, np.float64, 3 * n_cur).reshape(-1, 3))
        return d
    with open(path, "rb") as f:
        hpp = dict(cur_matches=np.fromfile(f, np.int32, n_cur), last_matches=np.fromfile(f, np.int32, n_last))
        hpp["n_created"], hpp["n_held"], hpp["ret"] = [int(v) for v in np.fromfile(f, np.int32, 3)]
        hpp.update(match_last=np.fromfile(f, np.int32, n_cur), new_id=np.fromfile(f, np.int32, n_cur), created=np.fromfile(f, np.uint8, n_cur),
                   stage2_line_id=np.fromfile(f, np.int32, n_cur))
        dev_lm = np.fromfile(f, np.int32, n_cur); host_lm = np.fromfile(f, np.int32, n_cur)
        device = graph(f); host = graph(f)
        assert f.read() == b""
    return dict(hpp=hpp, ctor_matches=dev_lm, host_matches=host_lm, device=device, host=host)
