"""The Tracking thread's per-frame sequence on one Frame, over the C ABI (host-side mirror; no oracle, no CPU fallback).

The reference runs, on ONE `Frame` (stereo): `ORBmatcher::SearchByProjection(Current, Last, th, bMono)` (src/Tracking.cc:904),
`Optimizer::PoseOptimization` (:937) and the outlier discard (:940-958) of `TrackWithMotionModel`; then `SearchLocalPoints` (:1133) and
`Optimizer::PoseOptimization` (:1152) of `TrackLocalMap`.  `TrackedFrame` keeps what the reference keeps in the Frame between those calls -
`mvpMapPoints` (here: per keypoint the world position of its MapPoint and an id) and `mvbOutlier` - and issues the same calls; with
`resident=True` the frame's keypoints are uploaded once (`lld_frame_create`) and the two matchers move only their queries.
The line half of the sequence (`AddLinesFrom`, :924) and `ComputeStereoMatches` / `MatchLines` (src/Frame.cc:113,122) have their own entry
points (`lld_line_track_match`, `lld_compute_stereo_matches`, `lld_line_match_stereo`) and are not chained here."""
from __future__ import annotations

import numpy as np

from . import orb_search
from .host import Optimizer, PoseFrame


def pose_frame_from_matches(F: orb_search.Frame, cam, pose_qt, kp_world, kp_has) -> tuple[PoseFrame, np.ndarray]:
    """Optimizer::PoseOptimization's point edges from Frame::mvpMapPoints (src/Optimizer.cc:683-760): one edge per keypoint with a
    MapPoint, in keypoint order; stereo iff mvuRight[i] >= 0.  Returns the problem and the keypoint index of every edge."""
    idx = np.nonzero(kp_has)[0]
    uvr = np.stack([F.xy[idx, 0], F.xy[idx, 1], np.where(F.uright[idx] >= 0, F.uright[idx], -1.0)], 1).astype(np.float64)
    e = np.zeros((0, 3)); e4 = np.zeros((0, 4))
    f = PoseFrame(cam=cam, pose_qt=np.asarray(pose_qt, np.float64), pt_xw=kp_world[idx].astype(np.float64), pt_uvr=uvr,
                  pt_inv_sigma2=F.inv_sigma2[F.octave[idx]].astype(np.float64), ln_x0=e, ln_dir=e, ln_left=e4, ln_right=e4,
                  ln_octave=np.zeros((0, 2), np.int32))
    return f.normalise(), idx


def qt_to_tcw_f32(lib, qt) -> np.ndarray:
    """Converter::toCvMat(SE3Quat) (src/Converter.cc:49-70) through the ABI's own conversion."""
    import ctypes as C
    from .abi import c_double_p, c_float_p
    q = np.ascontiguousarray(qt, np.float64); T = np.zeros(16, np.float32)
    lib.fn("se3_to_tcw_f32")(q.ctypes.data_as(c_double_p), T.ctypes.data_as(c_float_p))
    return T.reshape(4, 4)


class TrackedFrame:
    def __init__(self, ctx, F: orb_search.Frame, cam, resident: bool = True):
        self.ctx, self.lib, self.F, self.cam = ctx, ctx.lib, F, cam
        self.res = orb_search.ResidentFrame(ctx.lib, ctx.handle, F) if resident else None
        self.kp_has = np.zeros(F.n, bool)                        # mvpMapPoints[i] != NULL
        self.kp_world = np.zeros((F.n, 3), np.float32)           # its GetWorldPos()
        self.kp_point = np.full(F.n, -1, np.int64)               # an id of the MapPoint (caller's numbering)
        self.kp_obs = np.zeros(F.n, bool)                        # its Observations() > 0: only such a MapPoint blocks its keypoint (src/ORBmatcher.cc:98-100)
        self.discarded = np.zeros(0, np.int64)                   # MapPoints dropped as outliers in this frame: mnLastFrameSeen = mnId (src/Tracking.cc:949)
        self.stages = {}                                         # what every stage returned, for the checker

    def close(self):
        if self.res is not None:
            self.res.close(); self.res = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def _view(self, pose_qt):
        return orb_search.frame_view(qt_to_tcw_f32(self.lib, pose_qt), self.cam, self.F)

    def _optimise(self, pose_qt, tag):
        prob, idx = pose_frame_from_matches(self.F, self.cam, pose_qt, self.kp_world, self.kp_has)
        out = Optimizer(self.ctx).PoseOptimization(prob, 0.5)
        self.stages[tag] = dict(problem=prob, edge_keypoint=idx, out=out)
        # the discard of src/Tracking.cc:940-958 / :1160-1178: an outlier edge's MapPoint leaves the frame
        bad = idx[out.pt_outlier != 0]
        self.discarded = np.concatenate([self.discarded, self.kp_point[bad]])
        self.kp_has[bad] = False; self.kp_point[bad] = -1
        return out.pose_qt

    def track_with_motion_model(self, pose_qt_guess, last: dict, last_ids, th=7.0, direction=0):
        """SearchByProjection(Current, Last) from the predicted pose, PoseOptimization on the matches, outlier discard."""
        view = self._view(pose_qt_guess)
        occ = (self.kp_has & self.kp_obs).astype(np.uint8)
        if self.res is not None:
            out, uvr = self.res.search_last_frame(view, last, occ, direction, th, True)
        else:
            out, uvr = orb_search.search_last_frame(self.lib, self.ctx.handle, self.F, view, last, occ, direction, th, True)
        self.stages["search_last_frame"] = dict(view=view, occupied=occ, out=out, uvr=uvr)
        ok = (out.match >= 0) & (out.removed == 0)
        # CurrentFrame.mvpMapPoints[bestIdx2] = pMP, later queries see it occupied; the orientation filter NULLs removed ones (:1452-1460)
        for q in np.nonzero(ok)[0]:
            k = int(out.match[q])
            if out.owner[k] == q:
                self.kp_has[k] = True; self.kp_world[k] = last["world_pos"][q]; self.kp_point[k] = last_ids[q]
                self.kp_obs[k] = True if last.get("has_obs") is None else bool(last["has_obs"][q])
        return self._optimise(pose_qt_guess, "pose_after_motion_model")

    def track_local_map(self, pose_qt, mp: dict, mp_ids, th=1.0, nnratio=0.8):
        """SearchLocalPoints (points the frame already holds are skipped, src/Tracking.cc:1620-1632) + PoseOptimization."""
        view = self._view(pose_qt)
        # mnLastFrameSeen == mCurrentFrame.mnId (:1640): the points the frame holds (:1629) AND those the discard after the first
        # PoseOptimization marked (:949) - the latter must not be projected and matched again in this frame
        held = np.isin(mp_ids, self.kp_point[self.kp_has]) | np.isin(mp_ids, self.discarded)
        skip = (np.asarray(mp["skip"]) != 0) | held
        mp2 = dict(mp, skip=skip.astype(np.uint8))
        occ = (self.kp_has & self.kp_obs).astype(np.uint8)
        if self.res is not None:
            out, fr = self.res.search_local_points(view, mp2, occ, th, nnratio)
        else:
            out, fr = orb_search.search_local_points(self.lib, self.ctx.handle, self.F, view, mp2, occ, th, nnratio)
        self.stages["search_local_points"] = dict(view=view, occupied=occ, points=mp2, out=out, frustum=fr)
        for q in np.nonzero(out.match >= 0)[0]:
            k = int(out.match[q])
            if out.owner[k] == q:
                self.kp_has[k] = True; self.kp_world[k] = mp["world_pos"][q]; self.kp_point[k] = mp_ids[q]
                self.kp_obs[k] = True if mp.get("has_obs") is None else bool(mp["has_obs"][q])
        return self._optimise(pose_qt, "pose_after_local_map")


# ------------------------------------------------------------------------------------------------ the device-resident chain (round 6)
import ctypes as C

from . import abi
from .abi import c_double_p, c_float_p, c_int32_p, c_uint8_p


class FrameLines(C.Structure):
    _fields_ = [("n_left", C.c_int32), ("left", c_float_p), ("left_octave", c_int32_p), ("n_right", C.c_int32), ("right", c_float_p),
                ("right_octave", c_int32_p), ("line_matches", c_int32_p), ("desc", c_float_p), ("dim", C.c_int32), ("reserved", C.c_int32),
                ("sx", C.c_double), ("sy", C.c_double)]


class MapLines(C.Structure):
    _fields_ = [("n", C.c_int32), ("x0", c_double_p), ("dir", c_double_p), ("x1", c_double_p), ("x2", c_double_p), ("skip", c_uint8_p),
                ("desc", c_float_p), ("id", c_int32_p)]


class TrackParams(C.Structure):
    _fields_ = [("cam", abi.Camera), ("pose", abi.PoseParams), ("th_motion", C.c_float), ("th_local", C.c_float), ("nnratio_local", C.c_float),
                ("viewing_cos_limit", C.c_float), ("direction", C.c_int32), ("check_orientation", C.c_int32), ("wide_retry", C.c_int32),
                ("monocular", C.c_int32), ("line_thr_reproj_base", C.c_double), ("line_md_thr", C.c_double), ("line_use_grid", C.c_int32),
                ("reserved", C.c_int32)]


class TrackResult(C.Structure):
    _fields_ = [("pose_qt", C.c_double * 7), ("chi2", C.c_double), ("n_inliers", C.c_int32), ("lm_iterations", C.c_int32), ("lm_trials", C.c_int32),
                ("n_edges", C.c_int32), ("n_search_first", C.c_int32), ("n_search", C.c_int32), ("used_wide", C.c_int32), ("n_points", C.c_int32),
                ("n_points_map", C.c_int32), ("n_lines_matched", C.c_int32), ("n_lines", C.c_int32), ("n_discarded", C.c_int32),
                ("n_point_edges", C.c_int32), ("n_in_view", C.c_int32),
                ("kp_point_id", c_int32_p), ("kp_outlier", c_uint8_p), ("ln_line_id", c_int32_p), ("ln_outlier", c_uint8_p), ("mp_in_view", c_uint8_p)]


class FrameHeld(C.Structure):
    """lld_frame_held (include/lld_amd.h): what a stage 1 that ran elsewhere left in the frame."""
    _fields_ = [("kp_point_id", c_int32_p), ("kp_world_pos", c_float_p), ("kp_has_obs", c_uint8_p), ("kp_outlier", c_uint8_p), ("n_seen", C.c_int32),
                ("seen_point_id", c_int32_p), ("ln_line_id", c_int32_p), ("ln_x0", c_double_p), ("ln_dir", c_double_p), ("ln_outlier", c_uint8_p),
                ("n_tracked", C.c_int32), ("tracked_line_id", c_int32_p)]


_COUNTERS = ("n_inliers", "lm_iterations", "lm_trials", "n_edges", "n_search_first", "n_search", "used_wide", "n_points", "n_points_map",
             "n_lines_matched", "n_lines", "n_discarded", "n_point_edges", "n_in_view")


def map_lines_struct(ml: dict | None):
    """lld_map_lines from a dict with X0, dir, X1, X2 [n,3], desc [n,dim], id [n] and optionally skip [n]; returns (struct, arrays kept alive)."""
    m = MapLines()
    if ml is None:
        return m, {}
    keep = dict(x0=np.ascontiguousarray(ml["X0"], np.float64).reshape(-1, 3), dir=np.ascontiguousarray(ml["dir"], np.float64).reshape(-1, 3),
                x1=np.ascontiguousarray(ml["X1"], np.float64).reshape(-1, 3), x2=np.ascontiguousarray(ml["X2"], np.float64).reshape(-1, 3),
                desc=np.ascontiguousarray(ml["desc"], np.float32), id=np.ascontiguousarray(ml["id"], np.int32),
                skip=None if ml.get("skip") is None else np.ascontiguousarray(ml["skip"], np.uint8))
    m.n = keep["x0"].shape[0]
    m.x0 = keep["x0"].ctypes.data_as(c_double_p); m.dir = keep["dir"].ctypes.data_as(c_double_p)
    m.x1 = keep["x1"].ctypes.data_as(c_double_p); m.x2 = keep["x2"].ctypes.data_as(c_double_p)
    m.skip = None if keep["skip"] is None else keep["skip"].ctypes.data_as(c_uint8_p)
    m.desc = keep["desc"].ctypes.data_as(c_float_p); m.id = keep["id"].ctypes.data_as(c_int32_p)
    return m, keep


def ref_keyframe_struct(kf: dict):
    """lld_ref_keyframe from a dict (see DeviceTrackedFrame.track_reference_keyframe); returns (struct, arrays kept alive)."""
    from .abi import c_uint32_p
    keep = dict(desc=np.ascontiguousarray(kf["desc"], np.uint32).reshape(-1, 8), angle=np.ascontiguousarray(kf["angle"], np.float32),
                point_id=np.ascontiguousarray(kf["point_id"], np.int32), world_pos=np.ascontiguousarray(kf["world_pos"], np.float32).reshape(-1, 3),
                has_obs=None if kf.get("has_obs") is None else np.ascontiguousarray(kf["has_obs"], np.uint8),
                node=np.ascontiguousarray(kf["node"], np.int32), node_start=np.ascontiguousarray(kf["node_start"], np.int32),
                feature=np.ascontiguousarray(kf["feature"], np.int32))
    K = abi.RefKeyFrame()
    K.n = keep["desc"].shape[0]
    K.desc = keep["desc"].ctypes.data_as(c_uint32_p); K.angle = keep["angle"].ctypes.data_as(c_float_p)
    K.point_id = keep["point_id"].ctypes.data_as(c_int32_p); K.world_pos = keep["world_pos"].ctypes.data_as(c_float_p)
    K.has_obs = None if keep["has_obs"] is None else keep["has_obs"].ctypes.data_as(c_uint8_p)
    K.n_nodes = keep["node"].shape[0]
    K.node = keep["node"].ctypes.data_as(c_int32_p); K.node_start = keep["node_start"].ctypes.data_as(c_int32_p)
    K.feature = keep["feature"].ctypes.data_as(c_int32_p)
    return K, keep


class DeviceTrackedFrame:
    """lld_frame_track_*: the whole per-frame sequence on the device (include/lld_amd.h).  `lines`: dict with left_lines [n,4], left_octave,
    right_lines, right_octave, line_matches, desc (the frame's mvLinesLeft / mvLinesRight / line_matches / mDescriptorsLines) or None.  A dict
    that carries desc_right and stereo (TwoFrameLineMatcher's parameters) instead of line_matches has its lines matched on the device
    (lld_frame_build_lines, see _build_lines)."""

    def __init__(self, ctx, F: orb_search.Frame, cam, lines: dict | None = None, gamma=0.5, **params):
        self.ctx, self.lib, self.F, self.cam = ctx, ctx.lib, F, cam
        self.res = orb_search.ResidentFrame(ctx.lib, ctx.handle, F)
        self._setup(lines, gamma, params)

    @classmethod
    def from_built(cls, ctx, built: "orb_search.ResidentFrame", cam, lines: dict | None = None, gamma=0.5, **params):
        """The chain on a frame the device built (orb_search.StereoBuiltFrame, or MonoBuiltFrame from ORBextractor.build_mono_frame /
        orb_search.build_mono_frame_keypoints): the handle is taken over (close() destroys it), nothing is uploaded again.  For an
        RGB-D frame pass th_motion=15, th_local=3 (Tracking.cc:901, :1657); for a monocular one th_motion=15 and monocular=1."""
        h_ctx = getattr(built.ctx, "value", built.ctx)
        if h_ctx != getattr(ctx.handle, "value", ctx.handle):
            raise ValueError("the built frame belongs to another context")
        self = cls.__new__(cls)
        self.ctx, self.lib, self.F, self.cam = ctx, ctx.lib, built.F, cam
        self.res = built
        self._setup(lines, gamma, params)
        return self

    @classmethod
    def from_stereo_build(cls, ctx, built: "orb_search.StereoBuiltFrame", cam, lines: dict | None = None, gamma=0.5, **params):
        """from_built on a stereo frame (ORBextractor.build_stereo_frame / orb_search.build_stereo_frame_keypoints)."""
        return cls.from_built(ctx, built, cam, lines, gamma, **params)

    def _setup(self, lines, gamma, params):
        lib, F = self.lib, self.F
        lib.fn("frame_set_lines").argtypes = [C.c_void_p, C.POINTER(FrameLines)]; lib.fn("frame_set_lines").restype = C.c_int
        lib.fn("track_params_default").argtypes = [C.POINTER(TrackParams)]; lib.fn("track_params_default").restype = None
        lib.fn("frame_track_motion_model").argtypes = [C.c_void_p, C.POINTER(TrackParams), C.POINTER(orb_search.FrameView), c_double_p,
                                                       C.POINTER(orb_search.LastFramePoints), c_int32_p, C.POINTER(MapLines)]
        lib.fn("frame_track_motion_model").restype = C.c_int
        lib.fn("frame_track_local_map").argtypes = [C.c_void_p, C.POINTER(TrackParams), C.POINTER(orb_search.MapPoints), c_int32_p, C.POINTER(MapLines)]
        lib.fn("frame_track_local_map").restype = C.c_int
        lib.fn("frame_track_download").argtypes = [C.c_void_p, C.POINTER(TrackResult), C.POINTER(TrackResult)]; lib.fn("frame_track_download").restype = C.c_int
        self.n_lines = 0; self.n_local_points = 0
        if lines is not None and lines.get("desc_right") is not None:
            self._build_lines(lines)
        elif lines is not None:
            k = dict(left=np.ascontiguousarray(lines["left_lines"], np.float32).reshape(-1, 4), lo=np.ascontiguousarray(lines["left_octave"], np.int32),
                     right=np.ascontiguousarray(lines["right_lines"], np.float32).reshape(-1, 4), ro=np.ascontiguousarray(lines["right_octave"], np.int32),
                     lm=np.ascontiguousarray(lines["line_matches"], np.int32), desc=np.ascontiguousarray(lines["desc"], np.float32))
            L = FrameLines()
            L.n_left = k["left"].shape[0]; L.left = k["left"].ctypes.data_as(c_float_p); L.left_octave = k["lo"].ctypes.data_as(c_int32_p)
            L.n_right = k["right"].shape[0]; L.right = k["right"].ctypes.data_as(c_float_p); L.right_octave = k["ro"].ctypes.data_as(c_int32_p)
            L.line_matches = k["lm"].ctypes.data_as(c_int32_p); L.desc = k["desc"].ctypes.data_as(c_float_p); L.dim = k["desc"].shape[1]
            L.sx = 1.0 / float(F.max_x); L.sy = 1.0 / float(F.max_y)
            self._check(lib.fn("frame_set_lines")(self.res.handle, C.byref(L)), "lld_frame_set_lines")
            self.n_lines = int(L.n_left)
        self.params = TrackParams()
        lib.fn("track_params_default")(C.byref(self.params))
        self.params.cam = abi.Camera(*[float(np.float32(c)) for c in self.cam])
        self.params.pose.gamma = gamma
        for k_, v in params.items():
            setattr(self.params, k_, v)

    def _build_lines(self, lines):
        """lld_frame_build_lines: `lines` carries desc_right [n_right, dim] and stereo = dict(K [3,3], b, tau, min_line_length, is_stereo)
        instead of line_matches; the stereo association is made on the device and stays there (lines_download() fetches it)."""
        F = self.F
        k = dict(left=np.ascontiguousarray(lines["left_lines"], np.float32).reshape(-1, 4), lo=np.ascontiguousarray(lines["left_octave"], np.int32),
                 right=np.ascontiguousarray(lines["right_lines"], np.float32).reshape(-1, 4), ro=np.ascontiguousarray(lines["right_octave"], np.int32),
                 dl=np.ascontiguousarray(lines["desc"], np.float32), dr=np.ascontiguousarray(lines["desc_right"], np.float32))
        sp = lines["stereo"]
        L = abi.FrameLinesBuild()
        L.n_left = k["left"].shape[0]; L.left = k["left"].ctypes.data_as(c_float_p); L.left_octave = k["lo"].ctypes.data_as(c_int32_p)
        L.desc_left = k["dl"].ctypes.data_as(c_float_p)
        L.n_right = k["right"].shape[0]; L.right = k["right"].ctypes.data_as(c_float_p); L.right_octave = k["ro"].ctypes.data_as(c_int32_p)
        L.desc_right = k["dr"].ctypes.data_as(c_float_p)
        L.dim = k["dl"].shape[1] if k["dl"].ndim == 2 else int(lines["dim"])
        L.sx = 1.0 / float(F.max_x); L.sy = 1.0 / float(F.max_y)
        L.stereo = abi.LineStereoParams((C.c_double * 9)(*np.asarray(sp["K"], np.float64).ravel()), float(sp["b"]), float(sp["tau"]),
                                        int(sp["min_line_length"]), int(sp.get("is_stereo", 1)))
        self._check(self.lib.fn("frame_build_lines")(self.res.handle, C.byref(L)), "lld_frame_build_lines")
        self.n_lines = int(L.n_left)

    def lines_download(self):
        """lld_frame_lines_download: waits for the frame's queued work; (line_matches [n_left] i32, match_dist [n_left] f64)."""
        lm = np.full(self.n_lines, -1, np.int32); md = np.zeros(self.n_lines, np.float64)
        self._check(self.lib.fn("frame_lines_download")(self.res.handle, lm.ctypes.data_as(c_int32_p), md.ctypes.data_as(c_double_p)), "lld_frame_lines_download")
        return lm, md

    def new_map_lines(self, last_frame: "DeviceTrackedFrame", first_new_id: int, thr_reproj_base=6.0, md_thr=None, use_grid=1):
        """lld_frame_new_map_lines: Tracking::MatchLinesLastKF between this frame and `last_frame`, both resident.  Returns a dict with
        n_created, n_held, match_last, created, x0, dir, new_id; the created lines have entered this frame's state."""
        n = self.n_lines
        a = dict(match_last=np.full(n, -1, np.int32), created=np.zeros(n, np.uint8), x0=np.zeros((n, 3)), dir=np.zeros((n, 3)), new_id=np.full(n, -1, np.int32))
        P = abi.FrameNewLinesParams(float(thr_reproj_base), float(self.params.line_md_thr if md_thr is None else md_thr), int(use_grid), int(first_new_id))
        R = abi.FrameNewLinesResult(0, 0, a["match_last"].ctypes.data_as(c_int32_p), a["created"].ctypes.data_as(c_uint8_p), a["x0"].ctypes.data_as(c_double_p),
                                    a["dir"].ctypes.data_as(c_double_p), a["new_id"].ctypes.data_as(c_int32_p))
        self._check(self.lib.fn("frame_new_map_lines")(self.res.handle, last_frame.res.handle, C.byref(P), C.byref(R)), "lld_frame_new_map_lines")
        return dict(a, n_created=int(R.n_created), n_held=int(R.n_held))

    def _finish_result(self):
        nt = self.F.n
        a = dict(created=np.zeros(nt, np.uint8), new_id=np.full(nt, -1, np.int32), x3d=np.zeros((nt, 3), np.float32), kp_point_id=np.full(nt, -1, np.int32),
                 order=np.full(nt, -1, np.int32))
        R = abi.FrameFinishResult()
        R.created = a["created"].ctypes.data_as(c_uint8_p); R.new_id = a["new_id"].ctypes.data_as(c_int32_p); R.x3d = a["x3d"].ctypes.data_as(c_float_p)
        R.kp_point_id = a["kp_point_id"].ctypes.data_as(c_int32_p); R.order = a["order"].ctypes.data_as(c_int32_p)
        return R, a

    @staticmethod
    def _finish_dict(R, a):
        return dict(a, n_tracked_close=int(R.n_tracked_close), n_non_tracked_close=int(R.n_non_tracked_close), need=int(R.need), interrupt_ba=int(R.interrupt_ba),
                    made=int(R.made), n_visited=int(R.n_visited), n_created=int(R.n_created))

    def finish(self, th_depth, first_new_id, depth=None, force=-1, **decision):
        """lld_frame_track_finish: the tail of Tracking::Track (src/Tracking.cc:429-476) on the frame stage 2 (or set_state) left on the device:
        clean VO matches, NeedNewKeyFrame's counts and decision, CreateNewKeyFrame's stereo points when a keyframe is made, the outlier drop.
        decision: the scalars of lld_frame_finish_params by name (only_tracking, mapper_stopped, mapper_idle, keyframes_in_queue, set_not_stop_ok,
        monocular, max_frames, min_frames, n_keyframes, n_ref_matches, n_matches_inliers [-1: the frame's own stage-2 record], frame_id,
        last_reloc_frame_id, last_keyframe_id).  depth: mvDepth [nt] for a frame lld_frame_create made.  Returns a dict: the scalars of
        lld_frame_finish_result and created, new_id, x3d, kp_point_id, order."""
        P = abi.FrameFinishParams()
        P.th_depth = float(th_depth); P.first_new_id = int(first_new_id); P.force = int(force); P.n_matches_inliers = -1
        for k_, v in decision.items():
            if k_ not in {n for n, _ in abi.FrameFinishParams._fields_}:
                raise TypeError(f"finish() got an unknown scalar {k_!r}")
            setattr(P, k_, int(v))
        d = None if depth is None else np.ascontiguousarray(depth, np.float32)
        P.depth = None if d is None else d.ctypes.data_as(c_float_p)
        R, a = self._finish_result()
        self._check(self.lib.fn("frame_track_finish")(self.res.handle, C.byref(P), C.byref(R)), "lld_frame_track_finish")
        return self._finish_dict(R, a)

    def create_stereo_points(self, mode, first_new_id, th_depth=0.0, Tcw_f32=None, depth=None):
        """lld_frame_create_stereo_points: mode abi.POINTS_LAST_FRAME - Tracking::UpdateLastFrame's temporal points (:830-882), Tcw_f32 (optional)
        the pose mLastFrame.SetPose receives (:825); mode abi.POINTS_INITIALIZATION - Tracking::StereoInitialization's points (:535-550), Tcw_f32
        the pose of the first frame (default: the identity).  Returns the dict of finish()."""
        from .host import se3_from_tcw_f32
        P = abi.FramePointsParams()
        P.mode = int(mode); P.th_depth = float(th_depth); P.first_new_id = int(first_new_id)
        if Tcw_f32 is None and mode == abi.POINTS_INITIALIZATION:
            Tcw_f32 = np.eye(4, dtype=np.float32)
        keep = []
        if Tcw_f32 is not None:
            T = np.ascontiguousarray(Tcw_f32, np.float32).reshape(4, 4)
            view = orb_search.frame_view(T, self.cam, self.F)
            qt = np.ascontiguousarray(se3_from_tcw_f32(self.lib, T), np.float64)
            keep += [view, qt]
            P.params = C.addressof(self.params); P.view = C.addressof(view); P.pose_qt = qt.ctypes.data_as(c_double_p)
        d = None if depth is None else np.ascontiguousarray(depth, np.float32)
        P.depth = None if d is None else d.ctypes.data_as(c_float_p)
        R, a = self._finish_result()
        self._check(self.lib.fn("frame_create_stereo_points")(self.res.handle, C.byref(P), C.byref(R)), "lld_frame_create_stereo_points")
        return self._finish_dict(R, a)

    def _check(self, st, what):
        if st != abi.LLD_OK:
            err = RuntimeError(f"{what} failed: {self.lib.fn('status_string')(st).decode()}")
            err.status = st
            raise err

    def close(self):
        if self.res is not None:
            self.res.close(); self.res = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def track_with_motion_model(self, Tcw_f32, last: dict, last_ids, last_lines: dict | None = None):
        """Queues stage 1 from the predicted float pose matrix (mVelocity * mLastFrame.mTcw); returns nothing (see download())."""
        from .host import se3_from_tcw_f32
        T = np.ascontiguousarray(Tcw_f32, np.float32).reshape(4, 4)
        view = orb_search.frame_view(T, self.cam, self.F)
        qt = np.ascontiguousarray(se3_from_tcw_f32(self.lib, T), np.float64)
        m, keep = orb_search.last_frame_struct(last)
        ids = np.ascontiguousarray(last_ids, np.int32)
        ml, keep2 = map_lines_struct(last_lines)
        self._check(self.lib.fn("frame_track_motion_model")(self.res.handle, C.byref(self.params), C.byref(view), qt.ctypes.data_as(c_double_p), C.byref(m),
                                                             ids.ctypes.data_as(c_int32_p), C.byref(ml) if last_lines is not None else None), "lld_frame_track_motion_model")
        return view, qt

    def compute_bow(self, voc, levelsup=4, host=False):
        """Frame::ComputeBoW on the resident descriptors (lld_frame_compute_bow): the FeatureVector stays in HBM with the frame.  host=True
        waits and returns the vocabulary.BowTransform (what a new keyframe hands lld_kfdb_add); otherwise the work is only queued."""
        from . import vocabulary as V
        fn = self.lib.fn("frame_compute_bow")
        if not host:
            self._check(fn(self.res.handle, voc.handle, int(levelsup), None), "lld_frame_compute_bow")
            return None
        n = self.F.n; m = max(n, 1)
        r = V.BowTransform(np.empty(m, np.int32), np.empty(m, np.float64), np.empty(m, np.int32), np.empty(m + 1, np.int32), np.empty(m, np.int32),
                           np.empty(m, np.int32), np.empty(m, np.int32))
        R = V.BowResult(0, r.word.ctypes.data_as(c_int32_p), r.value.ctypes.data_as(c_double_p), 0, r.node.ctypes.data_as(c_int32_p),
                        r.node_start.ctypes.data_as(c_int32_p), r.feature.ctypes.data_as(c_int32_p), r.feature_word.ctypes.data_as(c_int32_p),
                        r.feature_nid.ctypes.data_as(c_int32_p))
        self._check(fn(self.res.handle, voc.handle, int(levelsup), C.byref(R)), "lld_frame_compute_bow")
        nw, nn = R.n_words, R.n_nodes
        return V.BowTransform(r.word[:nw], r.value[:nw], r.node[:nn], r.node_start[:nn + 1], r.feature[:int(r.node_start[nn])], r.feature_word[:n], r.feature_nid[:n])

    def track_reference_keyframe(self, Tcw_last_f32, kf: dict):
        """Queues stage 1 as Tracking::TrackReferenceKeyFrame runs it (lld_frame_track_reference_keyframe), after compute_bow.  Tcw_last_f32:
        mLastFrame.mTcw.  kf: desc [n,8] u32, angle [n], point_id [n] (-1: no MapPoint or a bad one), world_pos [n,3], optionally has_obs
        [n], and mpReferenceKF's FeatureVector as node / node_start / feature (a BowTransform's fields)."""
        from .host import se3_from_tcw_f32
        T = np.ascontiguousarray(Tcw_last_f32, np.float32).reshape(4, 4)
        view = orb_search.frame_view(T, self.cam, self.F)
        qt = np.ascontiguousarray(se3_from_tcw_f32(self.lib, T), np.float64)
        K, keep = ref_keyframe_struct(kf)
        self._check(self.lib.fn("frame_track_reference_keyframe")(self.res.handle, C.byref(self.params), C.byref(view), qt.ctypes.data_as(c_double_p), C.byref(K)),
                    "lld_frame_track_reference_keyframe")
        return view, qt

    def relocalize(self, candidates, seeds=None, Tcw_f32=None, pnp_params=None):
        """Tracking::Relocalization as stage 1 (lld_frame_relocalize), after compute_bow: one call, synchronous.  candidates: vpCandidateKFs,
        each a dict as track_reference_keyframe takes it plus max_distance / min_distance [n] of its MapPoints, optionally point_desc [n,8]
        (pMP->GetDescriptor(); default: the keyframe's desc) and is_bad.  seeds: one per candidate (default: its index).  Tcw_f32: the
        pose the frame keeps when nothing matches (default: identity).  Returns the record as a dict; on matched, track_local_map can follow."""
        from .host import se3_from_tcw_f32
        from .abi import c_uint32_p
        K = len(candidates)
        T = np.eye(4, dtype=np.float32) if Tcw_f32 is None else np.ascontiguousarray(Tcw_f32, np.float32).reshape(4, 4)
        view = orb_search.frame_view(T, self.cam, self.F)
        qt = np.ascontiguousarray(se3_from_tcw_f32(self.lib, T), np.float64)
        kfs = (abi.RefKeyFrame * max(K, 1))(); ex = (abi.RelocCandidate * max(K, 1))(); keep = []
        for i, c in enumerate(candidates):
            k, kept = ref_keyframe_struct(c)
            kfs[i] = k
            maxd = None if c.get("max_distance") is None else np.ascontiguousarray(c["max_distance"], np.float32)
            mind = None if c.get("min_distance") is None else np.ascontiguousarray(c["min_distance"], np.float32)
            pd = None if c.get("point_desc") is None else np.ascontiguousarray(c["point_desc"], np.uint32).reshape(-1, 8)
            keep.append((kept, maxd, mind, pd))
            ex[i].max_distance = None if maxd is None else maxd.ctypes.data_as(c_float_p)
            ex[i].min_distance = None if mind is None else mind.ctypes.data_as(c_float_p)
            ex[i].point_desc = None if pd is None else pd.ctypes.data_as(c_uint32_p)
            ex[i].is_bad = int(bool(c.get("is_bad", False)))
            ex[i].seed = int(i if seeds is None else seeds[i]) & 0xFFFFFFFF
        prm = abi.PnPParams()
        self.lib.fn("pnp_params_default")(C.byref(prm))
        for k_, v in (pnp_params or {}).items():
            setattr(prm, k_, v)
        m = max(K, 1)
        a = dict(n_bow=np.zeros(m, np.int32), discarded=np.zeros(m, np.uint8), rounds=np.zeros(m, np.int32), n_good_last=np.zeros(m, np.int32),
                 rungs=np.zeros(m, np.int32), n_additional1=np.zeros(m, np.int32), n_additional2=np.zeros(m, np.int32))
        r = abi.RelocResult()
        for k_, v in a.items():
            setattr(r, k_, v.ctypes.data_as(c_uint8_p if v.dtype == np.uint8 else c_int32_p))
        self._check(self.lib.fn("frame_relocalize")(self.res.handle, C.byref(self.params), C.byref(view), qt.ctypes.data_as(c_double_p), K, kfs, ex, C.byref(prm),
                                                    C.byref(r)), "lld_frame_relocalize")
        out = {k_: v[:K].copy() for k_, v in a.items()}
        out.update(matched=int(r.matched), winner=int(r.winner), round=int(r.round), n_good=int(r.n_good), n_rounds=int(r.n_rounds), n_kept=int(r.n_kept),
                   Tcw=np.array(list(r.Tcw), np.float32).reshape(4, 4))
        return out

    def set_state(self, Tcw_f32, kp_point_id, kp_world_pos, kp_has_obs=None, kp_outlier=None, seen_point_id=(), ln_line_id=None, ln_x0=None, ln_dir=None,
                  ln_outlier=None, tracked_line_id=()):
        """lld_frame_track_set_state: stage 1 ran elsewhere (TrackReferenceKeyFrame / Relocalization); the frame's float pose and what it holds."""
        from .host import se3_from_tcw_f32
        fn = self.lib.fn("frame_track_set_state")
        fn.argtypes = [C.c_void_p, C.POINTER(TrackParams), C.POINTER(orb_search.FrameView), c_double_p, C.POINTER(FrameHeld)]; fn.restype = C.c_int
        T = np.ascontiguousarray(Tcw_f32, np.float32).reshape(4, 4)
        view = orb_search.frame_view(T, self.cam, self.F)
        qt = np.ascontiguousarray(se3_from_tcw_f32(self.lib, T), np.float64)
        H = FrameHeld(); keep = []

        def arr(a, dt, ptr):
            if a is None: return None
            a = np.ascontiguousarray(a, dt); keep.append(a)
            return a.ctypes.data_as(ptr)
        H.kp_point_id = arr(kp_point_id, np.int32, c_int32_p); H.kp_world_pos = arr(kp_world_pos, np.float32, c_float_p)
        H.kp_has_obs = arr(kp_has_obs, np.uint8, c_uint8_p); H.kp_outlier = arr(kp_outlier, np.uint8, c_uint8_p)
        H.n_seen = len(seen_point_id); H.seen_point_id = arr(seen_point_id if len(seen_point_id) else None, np.int32, c_int32_p)
        H.ln_line_id = arr(ln_line_id, np.int32, c_int32_p); H.ln_x0 = arr(ln_x0, np.float64, c_double_p); H.ln_dir = arr(ln_dir, np.float64, c_double_p)
        H.ln_outlier = arr(ln_outlier, np.uint8, c_uint8_p)
        H.n_tracked = len(tracked_line_id); H.tracked_line_id = arr(tracked_line_id if len(tracked_line_id) else None, np.int32, c_int32_p)
        self._check(fn(self.res.handle, C.byref(self.params), C.byref(view), qt.ctypes.data_as(c_double_p), C.byref(H)), "lld_frame_track_set_state")
        return view, qt

    def track_local_map(self, mp: dict, mp_ids, local_lines: dict | None = None):
        m, keep = orb_search.map_points_struct(mp)
        ids = np.ascontiguousarray(mp_ids, np.int32)
        self.n_local_points = int(m.n)
        ml, keep2 = map_lines_struct(local_lines)
        self._check(self.lib.fn("frame_track_local_map")(self.res.handle, C.byref(self.params), C.byref(m), ids.ctypes.data_as(c_int32_p),
                                                          C.byref(ml) if local_lines is not None else None), "lld_frame_track_local_map")

    def update_local_map(self, dmap):
        """Tracking::UpdateLocalMap on the device (lld_frame_track_update_local_map), queued behind stage 1.  dmap: device_map.DeviceMap."""
        fn = self.lib.fn("frame_track_update_local_map")
        fn.argtypes = [C.c_void_p, C.c_void_p]; fn.restype = C.c_int
        self._check(fn(self.res.handle, dmap.handle), "lld_frame_track_update_local_map")

    def track_local_map_resident(self, dmap):
        """Stage 2 on the lists update_local_map left in dmap (lld_frame_track_local_map_resident)."""
        fn = self.lib.fn("frame_track_local_map_resident")
        fn.argtypes = [C.c_void_p, C.POINTER(TrackParams), C.c_void_p]; fn.restype = C.c_int
        self._check(fn(self.res.handle, C.byref(self.params), dmap.handle), "lld_frame_track_local_map_resident")
        self.n_local_points = int(dmap.limits.max_local_points)

    def local_map_download(self, dmap, lists=True, stage2=True):
        """lld_frame_local_map_download: UpdateLocalMap's record as a dict (with the three lists when `lists`), plus 'stages': the records of
        download() fetched in the same synchronisation (stage 2 with mp_in_view per local point when it was queued)."""
        fn = self.lib.fn("frame_local_map_download")
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.LocalMapResult)]; fn.restype = C.c_int
        nt, nl, L = self.F.n, self.n_lines, dmap.limits
        R = abi.LocalMapResult()
        a = dict(local_keyframes=np.zeros(abi.MAP_MAX_LOCAL_KEYFRAMES, np.int32), local_points=np.zeros(max(L.max_local_points, 1), np.int32),
                 local_lines=np.zeros(max(L.max_local_lines, 1), np.int32))
        if lists:
            for k_, v in a.items(): setattr(R, k_, v.ctypes.data_as(c_int32_p))
        outs = []
        for st_ in range(2 if stage2 else 1):
            r = TrackResult()
            b = dict(kp_point_id=np.empty(nt, np.int32), kp_outlier=np.empty(nt, np.uint8), ln_line_id=np.empty(nl, np.int32), ln_outlier=np.empty(nl, np.uint8))
            r.kp_point_id = b["kp_point_id"].ctypes.data_as(c_int32_p); r.kp_outlier = b["kp_outlier"].ctypes.data_as(c_uint8_p)
            r.ln_line_id = b["ln_line_id"].ctypes.data_as(c_int32_p); r.ln_outlier = b["ln_outlier"].ctypes.data_as(c_uint8_p)
            outs.append((r, b))
        in_view = np.zeros(max(L.max_local_points, 1), np.uint8)
        R.mp_in_view = in_view.ctypes.data_as(c_uint8_p)
        R.stage1 = C.cast(C.pointer(outs[0][0]), C.c_void_p)
        if stage2: R.stage2 = C.cast(C.pointer(outs[1][0]), C.c_void_p)
        self._check(fn(self.res.handle, dmap.handle, C.byref(R)), "lld_frame_local_map_download")
        d = {k_: int(getattr(R, k_)) for k_ in ("status", "n_voted", "n_local_keyframes", "n_local_points", "n_local_lines", "n_bad_cleared", "ref_keyframe",
                                                "vote_empty", "stage2_ran")}
        if lists:
            d["local_keyframes"] = a["local_keyframes"][:min(d["n_local_keyframes"], abi.MAP_MAX_LOCAL_KEYFRAMES)].copy()
            ok = not (d["status"] & abi.LOCAL_MAP_KEYFRAME_OVERFLOW)
            d["local_points"] = a["local_points"][:d["n_local_points"]].copy() if ok and d["n_local_points"] <= L.max_local_points else None
            d["local_lines"] = a["local_lines"][:d["n_local_lines"]].copy() if ok and d["n_local_lines"] <= L.max_local_lines else None
        stages = []
        for r, b in outs:
            s_ = dict(b, pose_qt=np.array(list(r.pose_qt)), chi2=float(r.chi2))
            for c in _COUNTERS: s_[c] = int(getattr(r, c))
            stages.append(s_)
        if stage2: stages[1]["mp_in_view"] = in_view
        d["stages"] = stages
        return d

    def download(self, stage2=True):
        """One copy, one synchronisation: the records of stage 1 and (if queued) stage 2 as dicts."""
        nt, nl = self.F.n, self.n_lines
        outs = []
        for st_ in range(2):
            r = TrackResult()
            a = dict(kp_point_id=np.empty(nt, np.int32), kp_outlier=np.empty(nt, np.uint8), ln_line_id=np.empty(nl, np.int32), ln_outlier=np.empty(nl, np.uint8))
            r.kp_point_id = a["kp_point_id"].ctypes.data_as(c_int32_p); r.kp_outlier = a["kp_outlier"].ctypes.data_as(c_uint8_p)
            r.ln_line_id = a["ln_line_id"].ctypes.data_as(c_int32_p); r.ln_outlier = a["ln_outlier"].ctypes.data_as(c_uint8_p)
            if st_ == 1 and stage2:
                a["mp_in_view"] = np.zeros(self.n_local_points, np.uint8); r.mp_in_view = a["mp_in_view"].ctypes.data_as(c_uint8_p)
            outs.append((r, a))
        self._check(self.lib.fn("frame_track_download")(self.res.handle, C.byref(outs[0][0]), C.byref(outs[1][0]) if stage2 else None), "lld_frame_track_download")
        res = []
        for r, a in outs[:2 if stage2 else 1]:
            d = dict(a, pose_qt=np.array(list(r.pose_qt)), chi2=float(r.chi2))
            for c in _COUNTERS: d[c] = int(getattr(r, c))
            res.append(d)
        return res


# ------------------------------------------------------------------------------------------------ Relocalization, call by call
def relocalize_call_by_call(ctx, voc, levelsup, F: orb_search.Frame, cam, candidates, seeds=None, pnp_params=None, gamma=0.5, max_rounds=400):
    """Tracking::Relocalization (src/Tracking.cc:1837-1998) driven from the host one library call at a time - the alternative recipe of
    INTEGRATION.md section 11 - with the same arguments and the same record as DeviceTrackedFrame.relocalize: lld_bow_transform for the
    frame's FeatureVector (the candidates bring theirs), lld_orb_search_run's SearchByBoW per candidate, lld_pnp_batch_* with a download per round, lld_pose_opt and
    lld_orb_search_projected (LLD_ORB_PROJ_RELOC) per rung.  Returns the record plus what the frame holds at the end (kp_point_id,
    kp_outlier, kp_world_pos, kp_has_obs, Tcw) for lld_frame_track_set_state."""
    from types import SimpleNamespace
    from .host import ORBmatcher
    from .pnp import DEFAULT_PARAMS, PnPsolverBatch
    from .vocabulary import common_nodes
    K = len(candidates); nt = F.n
    seeds = list(range(K)) if seeds is None else list(seeds)
    names = ("probability", "min_inliers", "max_iterations", "min_set", "epsilon", "th2")
    prm = tuple((pnp_params or {}).get(k, d) for k, d in zip(names, DEFAULT_PARAMS))
    fvF = voc.transform(F.desc, levelsup)
    m1, m2 = ORBmatcher(ctx, 0.75, True), ORBmatcher(ctx, 0.9, True)
    n_bow = np.zeros(K, np.int32); discarded = np.zeros(K, np.uint8); slot = [None] * K; problems = []; which = []
    fx, fy, cx, cy = [float(np.float32(c)) for c in cam[:4]]
    for i, kf in enumerate(candidates):
        if kf.get("is_bad"):
            discarded[i] = 1; continue
        n = len(kf["angle"])
        KF = orb_search.Frame(desc=np.asarray(kf["desc"], np.uint32).reshape(-1, 8), xy=np.zeros((n, 2), np.float32), octave=np.zeros(n, np.int32),
                              uright=np.full(n, -1.0, np.float32), angle=np.asarray(kf["angle"], np.float32)).normalise()
        # pKF->mFeatVec exists since the keyframe was made (KeyFrame::ComputeBoW): the candidate's own CSR, as lld_frame_relocalize takes it
        fvK = SimpleNamespace(node=np.asarray(kf["node"], np.int32), node_start=np.asarray(kf["node_start"], np.int32), feature=np.asarray(kf["feature"], np.int32))
        out = m1.SearchByBoWFrame(KF, F, common_nodes(fvK, fvF), (np.asarray(kf["point_id"]) >= 0).astype(np.uint8))
        qk = out.query_kp if len(out.query_kp) else np.zeros(1, np.int64)
        slot[i] = np.where(out.owner >= 0, qk[np.maximum(out.owner, 0)], -1)
        n_bow[i] = out.n_matches
        if out.n_matches < 15:
            discarded[i] = 1; continue
        k = np.nonzero(slot[i] >= 0)[0]
        problems.append(dict(xyz=np.asarray(kf["world_pos"], np.float32)[slot[i][k]], uv=F.xy[k], sigma2=F.sigma2[F.octave[k]], kp_index=k, n_keypoints=nt,
                             fx=fx, fy=fy, cx=cx, cy=cy, seed=seeds[i]))
        which.append(i)
    n_kept = len(which)
    rounds = np.zeros(K, np.int32); good_last = np.full(K, -1, np.int32); rungs = np.zeros(K, np.int32); add1 = np.zeros(K, np.int32); add2 = np.zeros(K, np.int32)
    kp_has = np.zeros(nt, bool); kp_id = np.full(nt, -1, np.int64); kp_world = np.zeros((nt, 3), np.float32); kp_obs = np.zeros(nt, np.uint8); kp_out = np.zeros(nt, np.uint8)
    state = dict(T=None)
    opt = Optimizer(ctx)

    def optimise():
        prob, idx = pose_frame_from_matches(F, cam, state["qt"], kp_world, kp_has)
        o = opt.PoseOptimization(prob, gamma)
        kp_out[idx] = o.pt_outlier
        if len(idx) >= 3:
            state["T"] = qt_to_tcw_f32(ctx.lib, o.pose_qt)
            state["qt"] = se3_from_tcw(state["T"])
        return int(o.n_inliers)

    def se3_from_tcw(T):
        from .host import se3_from_tcw_f32
        return np.ascontiguousarray(se3_from_tcw_f32(ctx.lib, T), np.float64)

    def project(kf, found, th, dist):
        pid = np.asarray(kf["point_id"])
        desc = kf["point_desc"] if kf.get("point_desc") is not None else kf["desc"]
        mp = dict(world_pos=kf["world_pos"], max_distance=kf["max_distance"], min_distance=kf["min_distance"], desc=desc,
                  skip=((pid < 0) | np.isin(pid, list(found))).astype(np.uint8))
        out, _, _ = m2.SearchByProjectionRelocPoints(F, orb_search.frame_view(state["T"], cam, F), mp, kf["angle"], kp_has.astype(np.uint8), th, dist)
        obs = kf.get("has_obs") if kf.get("has_obs") is not None else np.ones(len(pid), np.uint8)
        for k in np.nonzero(out.owner >= 0)[0]:
            q = int(out.owner[k])
            kp_has[k] = True; kp_world[k] = np.asarray(kf["world_pos"], np.float32)[q]; kp_id[k] = int(pid[q]); kp_obs[k] = int(obs[q])
        return int(out.n_matches)

    def discard():
        bad = kp_has & (kp_out != 0)
        kp_has[bad] = False; kp_id[bad] = -1
    matched, winner, win_round, n_good, n_round = 0, -1, 0, 0, 0
    batch = PnPsolverBatch(ctx, problems, prm) if n_kept else None
    try:
        live = np.ones(n_kept, bool)
        while live.any() and not matched and n_round < max_rounds:
            n_round += 1
            res = batch.iterate(5, live)
            for s in range(n_kept):
                if not live[s]: continue
                i = which[s]; kf = candidates[i]; o = res[s]
                rounds[i] += 1
                if o.no_more: live[s] = False; discarded[i] = 1
                if o.Tcw is None: continue
                T = np.eye(4, dtype=np.float32); T[:3, :] = o.Tcw
                state["T"] = T; state["qt"] = se3_from_tcw(T)
                inl = o.inliers != 0
                pid = np.asarray(kf["point_id"]); q = np.maximum(slot[i], 0)
                obs = kf.get("has_obs") if kf.get("has_obs") is not None else np.ones(len(pid), np.uint8)
                kp_has[:] = inl; kp_id[:] = np.where(inl, pid[q], -1); kp_world[:] = np.where(inl[:, None], np.asarray(kf["world_pos"], np.float32)[q], 0)
                kp_obs[:] = np.where(inl, np.asarray(obs)[q], 0)
                found = set(int(x) for x in kp_id[inl])
                g = optimise(); mask = abi.RELOC_RUNG_POSE1; a1 = a2 = 0
                if g >= 10:
                    discard()
                    if g < 50:
                        a1 = project(kf, found, 10.0, 100); mask |= abi.RELOC_RUNG_SEARCH1
                        if a1 + g >= 50:
                            g = optimise(); mask |= abi.RELOC_RUNG_POSE2
                            if 30 < g < 50:
                                a2 = project(kf, set(int(x) for x in kp_id[kp_has]), 3.0, 64); mask |= abi.RELOC_RUNG_SEARCH2
                                if g + a2 >= 50:
                                    g = optimise(); mask |= abi.RELOC_RUNG_POSE3
                                    discard()
                good_last[i], rungs[i], add1[i], add2[i] = g, mask, a1, a2
                if g >= 50:
                    matched, winner, win_round, n_good = 1, i, n_round, g
                    break
    finally:
        if batch is not None and hasattr(batch, "close"): batch.close()
    if not matched:
        kp_has[:] = False; kp_id[:] = -1
    return dict(matched=matched, winner=winner, round=win_round, n_good=n_good, n_rounds=n_round, n_kept=n_kept, n_bow=n_bow, discarded=discarded, rounds=rounds,
                n_good_last=good_last, rungs=rungs, n_additional1=add1, n_additional2=add2, kp_point_id=np.where(kp_has, kp_id, -1).astype(np.int32),
                kp_outlier=np.where(kp_has, kp_out, 0).astype(np.uint8), kp_world_pos=np.where(kp_has[:, None], kp_world, 0).astype(np.float32),
                kp_has_obs=np.where(kp_has, kp_obs, 0).astype(np.uint8), Tcw=state["T"] if matched else None)


# ------------------------------------------------------------------------------------------------ flat files of examples/harness.cpp `track`
def write_harness_scene(path, sc: dict, repeats=1, download_between=False, gamma=0.5, thr_base=2.0, md_thr=0.9):
    """A make_tracking_scene dict as the flat binary `examples/harness track` reads (layout: run_track in examples/harness.cpp)."""
    F = sc["frame"]; lines = sc.get("lines")
    T = np.ascontiguousarray(sc["Tcw_guess"], np.float32).reshape(4, 4)
    view = orb_search.frame_view(T, sc["cam"], F)
    last, mp = sc["last"], sc["map_points"]
    n_last, n_mp = len(sc["last_ids"]), len(sc["map_ids"])
    nl = 0 if lines is None else np.asarray(lines["left_lines"]).reshape(-1, 4).shape[0]
    nr = 0 if lines is None else np.asarray(lines["right_lines"]).reshape(-1, 4).shape[0]
    dim = 1 if lines is None else np.asarray(lines["desc"]).shape[1]
    ll, ml = (sc.get("last_lines"), sc.get("local_lines")) if lines is not None else (None, None)
    n_ll = 0 if ll is None else len(ll["id"]); n_ml = 0 if ml is None else len(ml["id"])
    f32 = lambda a: np.ascontiguousarray(a, np.float32); i32 = lambda a: np.ascontiguousarray(a, np.int32); u8 = lambda a: np.ascontiguousarray(a, np.uint8)
    with open(path, "wb") as f:
        i32([F.n, F.scale.shape[0], n_last, n_mp, nl, nr, dim, n_ll, n_ml, repeats, int(download_between), 0, 0, 0, 0, 0]).tofile(f)
        f32([F.min_x, F.min_y, F.max_x, F.max_y, F.width_inv, F.height_inv]).tofile(f)
        f32(F.scale).tofile(f); f32(F.inv_sigma2).tofile(f)
        np.array([float(np.float32(c)) for c in sc["cam"]] + [gamma, thr_base, md_thr], np.float64).tofile(f)
        np.ascontiguousarray(F.desc, np.uint32).tofile(f); f32(F.xy).tofile(f); i32(F.octave).tofile(f); f32(F.uright).tofile(f); f32(F.angle).tofile(f)
        f.write(bytes(view)); f32(T).tofile(f)
        obs = last.get("has_obs") if last.get("has_obs") is not None else np.ones(n_last, np.uint8)
        f32(last["world_pos"]).tofile(f); u8(last["valid"]).tofile(f); i32(last["octave"]).tofile(f); f32(last["angle"]).tofile(f)
        np.ascontiguousarray(last["desc"], np.uint32).tofile(f); u8(obs).tofile(f); i32(sc["last_ids"]).tofile(f)
        mobs = mp.get("has_obs") if mp.get("has_obs") is not None else np.ones(n_mp, np.uint8)
        f32(mp["world_pos"]).tofile(f); f32(mp["normal"]).tofile(f); f32(mp["max_distance"]).tofile(f); f32(mp["min_distance"]).tofile(f)
        np.ascontiguousarray(mp["desc"], np.uint32).tofile(f); u8(mobs).tofile(f); u8(mp["skip"]).tofile(f); i32(sc["map_ids"]).tofile(f)
        if lines is not None:
            f32(lines["left_lines"]).tofile(f); i32(lines["left_octave"]).tofile(f); f32(lines["right_lines"]).tofile(f); i32(lines["right_octave"]).tofile(f)
            i32(lines["line_matches"]).tofile(f); f32(lines["desc"]).tofile(f)
        for L in (ll, ml):
            if L is None or len(L["id"]) == 0: continue
            for k in ("X0", "dir", "X1", "X2"): np.ascontiguousarray(L[k], np.float64).tofile(f)
            u8(L["skip"] if L.get("skip") is not None else np.zeros(len(L["id"]), np.uint8)).tofile(f); f32(L["desc"]).tofile(f); i32(L["id"]).tofile(f)
    return nl


def read_harness_result(path, nt, nl, repeats):
    """(record of stage 1, record of stage 2, dict of per-repeat host milliseconds) written by `examples/harness track`."""
    recs = []
    with open(path, "rb") as f:
        for _ in range(2):
            d = dict(pose_qt=np.fromfile(f, np.float64, 7), chi2=float(np.fromfile(f, np.float64, 1)[0]))
            c = np.fromfile(f, np.int32, 12)
            for k, v in zip(_COUNTERS[:12], c): d[k] = int(v)
            d["kp_point_id"] = np.fromfile(f, np.int32, nt); d["kp_outlier"] = np.fromfile(f, np.uint8, nt)
            d["ln_line_id"] = np.fromfile(f, np.int32, nl); d["ln_outlier"] = np.fromfile(f, np.uint8, nl)
            recs.append(d)
        ms = dict(total=np.fromfile(f, np.float64, repeats), queue_motion_model=np.fromfile(f, np.float64, repeats), queue_local_map=np.fromfile(f, np.float64, repeats))
    return recs[0], recs[1], ms


# ------------------------------------------------------------------------------------------------ flat files of examples/refkf_harness.cpp
def write_refkf_scene(path, sc: dict, kf: dict, Tcw_last, levelsup, gamma=0.5):
    """A make_tracking_scene dict (its lines are not written), mpReferenceKF as DeviceTrackedFrame.track_reference_keyframe takes it and
    mLastFrame.mTcw, as the flat binary `examples/refkf_harness` reads."""
    F = sc["frame"]; mp = sc["map_points"]
    T = np.ascontiguousarray(Tcw_last, np.float32).reshape(4, 4)
    view = orb_search.frame_view(T, sc["cam"], F)
    f32 = lambda a: np.ascontiguousarray(a, np.float32); i32 = lambda a: np.ascontiguousarray(a, np.int32); u8 = lambda a: np.ascontiguousarray(a, np.uint8)
    n_kf, n_mp = len(kf["angle"]), len(sc["map_ids"])
    with open(path, "wb") as f:
        i32([F.n, F.scale.shape[0], n_kf, len(kf["node"]), len(kf["feature"]), n_mp, int(levelsup), 0]).tofile(f)
        f32([F.min_x, F.min_y, F.max_x, F.max_y, F.width_inv, F.height_inv]).tofile(f)
        f32(F.scale).tofile(f); f32(F.sigma2).tofile(f); f32(F.inv_sigma2).tofile(f)
        np.array([float(np.float32(c)) for c in sc["cam"]] + [gamma], np.float64).tofile(f)
        np.ascontiguousarray(F.desc, np.uint32).tofile(f); f32(F.xy).tofile(f); i32(F.octave).tofile(f); f32(F.uright).tofile(f); f32(F.angle).tofile(f)
        f.write(bytes(view)); f32(T).tofile(f)
        obs = kf.get("has_obs") if kf.get("has_obs") is not None else np.ones(n_kf, np.uint8)
        np.ascontiguousarray(kf["desc"], np.uint32).tofile(f); f32(kf["angle"]).tofile(f); i32(kf["point_id"]).tofile(f); f32(kf["world_pos"]).tofile(f); u8(obs).tofile(f)
        i32(kf["node"]).tofile(f); i32(kf["node_start"]).tofile(f); i32(kf["feature"]).tofile(f)
        mobs = mp.get("has_obs") if mp.get("has_obs") is not None else np.ones(n_mp, np.uint8)
        f32(mp["world_pos"]).tofile(f); f32(mp["normal"]).tofile(f); f32(mp["max_distance"]).tofile(f); f32(mp["min_distance"]).tofile(f)
        np.ascontiguousarray(mp["desc"], np.uint32).tofile(f); u8(mobs).tofile(f); u8(mp["skip"]).tofile(f); i32(sc["map_ids"]).tofile(f)


def read_refkf_result(path, nt, n_kf):
    """What `examples/refkf_harness` wrote: dict(records=[stage 1, stage 2] of the lld_amd.hpp route, adapter=dict(...) of the object graph)."""
    def state(f):
        return dict(point_id=np.fromfile(f, np.int32, nt), outlier=np.fromfile(f, np.uint8, nt), Tcw=np.fromfile(f, np.float32, 16).reshape(4, 4))
    with open(path, "rb") as f:
        recs = []
        for _ in range(2):
            d = dict(pose_qt=np.fromfile(f, np.float64, 7), chi2=float(np.fromfile(f, np.float64, 1)[0]))
            for k, v in zip(_COUNTERS, np.fromfile(f, np.int32, 14)): d[k] = int(v)
            d["kp_point_id"] = np.fromfile(f, np.int32, nt); d["kp_outlier"] = np.fromfile(f, np.uint8, nt)
            recs.append(d)
        a = dict(returned=int(np.fromfile(f, np.int32, 1)[0]), after_stage1=state(f), seen=np.fromfile(f, np.uint8, n_kf), in_view=np.fromfile(f, np.uint8, n_kf))
        nn, nv = np.fromfile(f, np.int32, 2)
        a["feat_vec"] = dict(node=np.fromfile(f, np.int32, nn), node_start=np.fromfile(f, np.int32, nn + 1), feature=np.fromfile(f, np.int32, nv))
        a["inliers"] = int(np.fromfile(f, np.int32, 1)[0]); a["after_stage2"] = state(f)
    return dict(records=recs, adapter=a)


# ------------------------------------------------------------------------------------------------ flat files of examples/reloc_harness.cpp
def write_reloc_scene(path, F: orb_search.Frame, cam, candidates, seeds, Tcw0, levelsup, gamma=0.5):
    """A frame, the pose it carries and the candidates DeviceTrackedFrame.relocalize takes, as the flat binary `examples/reloc_harness` reads."""
    T = np.ascontiguousarray(Tcw0, np.float32).reshape(4, 4)
    view = orb_search.frame_view(T, cam, F)
    f32 = lambda a: np.ascontiguousarray(a, np.float32); i32 = lambda a: np.ascontiguousarray(a, np.int32); u8 = lambda a: np.ascontiguousarray(a, np.uint8)
    with open(path, "wb") as f:
        i32([F.n, F.scale.shape[0], len(candidates), int(levelsup)]).tofile(f)
        f32([F.min_x, F.min_y, F.max_x, F.max_y, F.width_inv, F.height_inv]).tofile(f)
        f32(F.scale).tofile(f); f32(F.sigma2).tofile(f); f32(F.inv_sigma2).tofile(f)
        np.array([float(np.float32(c)) for c in cam] + [gamma], np.float64).tofile(f)
        np.ascontiguousarray(F.desc, np.uint32).tofile(f); f32(F.xy).tofile(f); i32(F.octave).tofile(f); f32(F.uright).tofile(f); f32(F.angle).tofile(f)
        f.write(bytes(view)); f32(T).tofile(f)
        for kf, seed in zip(candidates, seeds):
            n = len(kf["angle"])
            obs = kf.get("has_obs") if kf.get("has_obs") is not None else np.ones(n, np.uint8)
            pdesc = kf["point_desc"] if kf.get("point_desc") is not None else kf["desc"]
            i32([n, len(kf["node"]), len(kf["feature"]), int(bool(kf.get("is_bad", False))), int(seed)]).tofile(f)
            np.ascontiguousarray(kf["desc"], np.uint32).tofile(f); np.ascontiguousarray(pdesc, np.uint32).tofile(f); f32(kf["angle"]).tofile(f); i32(kf["point_id"]).tofile(f)
            f32(kf["world_pos"]).tofile(f); u8(obs).tofile(f); f32(kf["max_distance"]).tofile(f); f32(kf["min_distance"]).tofile(f)
            i32(kf["node"]).tofile(f); i32(kf["node_start"]).tofile(f); i32(kf["feature"]).tofile(f)


def read_reloc_result(path, nt, K):
    """What `examples/reloc_harness` wrote: dict(returned, record, kp_point_id, kp_outlier) of the lld_amd.hpp route and adapter=dict(returned,
    point_id, outlier, Tcw) of the object graph."""
    with open(path, "rb") as f:
        out = dict(returned=int(np.fromfile(f, np.int32, 1)[0]))
        h = np.fromfile(f, np.int32, 6)
        rec = dict(zip(("matched", "winner", "round", "n_good", "n_rounds", "n_kept"), (int(x) for x in h)))
        rec["Tcw"] = np.fromfile(f, np.float32, 16).reshape(4, 4)
        for k, dt in (("n_bow", np.int32), ("discarded", np.uint8), ("rounds", np.int32), ("n_good_last", np.int32), ("rungs", np.int32), ("n_additional1", np.int32),
                      ("n_additional2", np.int32)):
            rec[k] = np.fromfile(f, dt, K)
        out["record"] = rec
        out["kp_point_id"] = np.fromfile(f, np.int32, nt); out["kp_outlier"] = np.fromfile(f, np.uint8, nt)
        out["adapter"] = dict(returned=int(np.fromfile(f, np.int32, 1)[0]), point_id=np.fromfile(f, np.int32, nt), outlier=np.fromfile(f, np.uint8, nt),
                              Tcw=np.fromfile(f, np.float32, 16).reshape(4, 4))
    return out
