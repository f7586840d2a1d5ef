"""Times the tail of Tracking::Track (clean VO matches, NeedNewKeyFrame, CreateNewKeyFrame's stereo points, the outlier drop) on the 2000-keypoint
stereo frame of synth.make_stereo_scene(0), built on the device, after both stages of the chain - two ways on the SAME library:
  new     lld_frame_track_finish, its one fetch included;
  parent  the only route the library offered before: lld_frame_track_download + lld_frame_stereo_download (the frame's state and mvDepth come to
          the host), the host loops in compiled C++ (examples/frame_finish_host.cpp, built here as a shared object), and lld_frame_track_set_state
          to bring the device state back in step with what the host made.
Before every window both stages run again on the frame (outside the window), so each window starts from what TrackLocalMap left.  Every struct
is filled before the timed window.  Each window is bracketed by two HIP events on the context's stream and by the host clock.  Medians and
quartiles of --reps windows after --warmup; the routes alternate in blocks of 20 so that a drift of the machine meets both.
Bar: the new median below the parent's by more than the larger interquartile range (HIP events), and both routes return the same integers
and positions.  Writes profiles/frame_finish_time.json when --out is given.  Needs an MI355X."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def quartiles(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(median_ms=float(med), q1_ms=float(q1), q3_ms=float(q3), iqr_ms=float(q3 - q1), min_ms=float(a[0]))


def host_loops():
    """examples/frame_finish_host.cpp as a shared object under build/ (host code only)."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libframe_finish_host.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "frame_finish_host.cpp"), "-o", so])
    return C.CDLL(so)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import frame_finish_ref as REF
    import frame_finish_scenes as FS
    from lld_slam_amd import Context, abi, orb_search, synth
    from lld_slam_amd.abi import c_float_p, c_int32_p, c_uint8_p
    from lld_slam_amd.tracking import DeviceTrackedFrame, FrameHeld, TrackParams, TrackResult
    ss = synth.make_stereo_scene(0)
    cam = tuple(float(np.float32(c)) for c in synth.KITTI_CAM)
    hl = host_loops()
    tail, state = hl.frame_finish_host_tail, hl.frame_finish_host_state
    state.restype = None; state.argtypes = [C.c_int, c_int32_p, c_uint8_p, c_float_p, c_uint8_p, c_int32_p, c_uint8_p, c_uint8_p, c_float_p]
    tail.restype = None
    tail.argtypes = [C.c_int, c_float_p, c_float_p, C.c_void_p, C.c_void_p, c_int32_p, c_uint8_p, c_uint8_p, c_float_p, C.c_void_p]
    res = {"reps": a.reps, "warmup": a.warmup, "library": os.path.relpath(abi.product_library_path(), ROOT),
           "timer": "HIP events on the context's stream around each window, and the host clock around the same calls"}
    with Context(0) as ctx:
        lib = ctx.lib
        hip = C.CDLL("libamdhip64.so")
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]; hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]; hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        stream = C.c_void_p(lib.fn("ctx_stream")(ctx.handle))
        sync = lib.fn("ctx_synchronize")
        built = orb_search.build_stereo_frame_keypoints(lib, ctx.handle, ss["L"], ss["R"], ss["left"], ss["right"], ss["inv_scale"], ss["mb"], ss["mbf"])
        st0 = built.download()
        sc = FS.chain_scene(st0.u_right, st0.depth, ss=ss, cam=cam)
        nt = sc["frame"].n
        th = float(sc["th_depth"])
        res["workload"] = ("synth.make_stereo_scene(0): %d keypoints, %d with depth, %d of them below mThDepth %.2f (the median depth); %d local MapPoints, %d of the last frame"
                           % (nt, int((st0.depth > 0).sum()), int(((st0.depth > 0) & (st0.depth < sc["th_depth"])).sum()), th, len(sc["map_ids"]), len(sc["last_ids"])))
        with DeviceTrackedFrame.from_stereo_build(ctx, built, cam) as tf:
            h = tf.res.handle

            def both_stages():
                tf.track_with_motion_model(sc["Tcw_guess"], sc["last"], sc["last_ids"])
                tf.track_local_map(sc["map_points"], sc["map_ids"])
                assert sync(ctx.handle) == 0

            both_stages()
            r2 = tf.download()[1]
            p = dict(REF.DECISION_DEFAULTS, n_matches_inliers=-1, n_ref_matches=4 * int(r2["n_points_map"]) + 40)
            # ---- new route: everything but the call itself is prepared here
            P = abi.FrameFinishParams()
            P.th_depth = th; P.first_new_id = FS.FIRST_ID; P.force = -1
            for k, v in p.items(): setattr(P, k, int(v))
            Rn, an = tf._finish_result()
            finish = lib.fn("frame_track_finish")

            def route_new():
                assert finish(h, C.byref(P), C.byref(Rn)) == 0

            # ---- parent route: the records and mvDepth to the host, the host loops, the state back to the device
            world_of = np.zeros((int(np.max(sc["map_ids"])) + 1, 3), np.float32); obs_of = np.zeros(world_of.shape[0], np.uint8)
            world_of[sc["map_ids"]] = sc["map_points"]["world_pos"]; obs_of[sc["map_ids"]] = sc["map_points"]["has_obs"]
            T1, T2 = TrackResult(), TrackResult()
            rec = dict(id1=np.empty(nt, np.int32), out1=np.empty(nt, np.uint8), id2=np.empty(nt, np.int32), out2=np.empty(nt, np.uint8))
            T1.kp_point_id = rec["id1"].ctypes.data_as(c_int32_p); T1.kp_outlier = rec["out1"].ctypes.data_as(c_uint8_p)
            T2.kp_point_id = rec["id2"].ctypes.data_as(c_int32_p); T2.kp_outlier = rec["out2"].ctypes.data_as(c_uint8_p)
            sd = dict(ur=np.empty(nt, np.float32), depth=np.empty(nt, np.float32), br=np.empty(nt, np.int32), sad=np.empty(nt, np.int32))
            SR = orb_search.StereoResult()
            SR.u_right = sd["ur"].ctypes.data_as(c_float_p); SR.depth = sd["depth"].ctypes.data_as(c_float_p)
            SR.best_r = sd["br"].ctypes.data_as(c_int32_p); SR.sad = sd["sad"].ctypes.data_as(c_int32_p)
            track_download = lib.fn("frame_track_download"); stereo_download = lib.fn("frame_stereo_download")
            stereo_download.argtypes = [C.c_void_p, C.POINTER(orb_search.StereoResult)]; stereo_download.restype = C.c_int
            set_state = lib.fn("frame_track_set_state")
            set_state.argtypes = [C.c_void_p, C.POINTER(TrackParams), C.POINTER(orb_search.FrameView), abi.c_double_p, C.POINTER(FrameHeld)]; set_state.restype = C.c_int
            Pp = abi.FrameFinishParams()
            C.memmove(C.byref(Pp), C.byref(P), C.sizeof(P))
            Rp, ap_ = tf._finish_result()
            hs = dict(id=np.empty(nt, np.int32), obs=np.empty(nt, np.uint8), out=np.empty(nt, np.uint8), world=np.empty((nt, 3), np.float32))
            H = FrameHeld()
            H.kp_point_id = hs["id"].ctypes.data_as(c_int32_p); H.kp_world_pos = hs["world"].ctypes.data_as(c_float_p)
            H.kp_has_obs = hs["obs"].ctypes.data_as(c_uint8_p); H.kp_outlier = hs["out"].ctypes.data_as(c_uint8_p)
            xy = np.ascontiguousarray(sc["frame"].xy, np.float32)
            import oracle_tracking as OT
            from lld_slam_amd import host

            T = np.asarray(host.se3_to_tcw_f32(lib, np.asarray(r2["pose_qt"], np.float64)), np.float32).reshape(4, 4)   # Frame::SetPose of the optimised pose: the same
            view = OT.pose_view(T, cam, sc["frame"])                                                                    # every window, formed once (a C++ caller spends nanoseconds on it)
            qt = np.ascontiguousarray(host.se3_from_tcw_f32(lib, T), np.float64)
            world_p = world_of.ctypes.data_as(c_float_p); obs_p = obs_of.ctypes.data_as(c_uint8_p); xy_p = xy.ctypes.data_as(c_float_p); qt_p = qt.ctypes.data_as(abi.c_double_p)

            def route_parent():
                assert track_download(h, C.byref(T1), C.byref(T2)) == 0 and stereo_download(h, C.byref(SR)) == 0
                state(nt, T2.kp_point_id, T2.kp_outlier, world_p, obs_p, H.kp_point_id, H.kp_has_obs, H.kp_outlier, H.kp_world_pos)
                Pp.n_matches_inliers = T2.n_points_map
                tail(nt, SR.depth, xy_p, C.addressof(view), C.addressof(Pp), H.kp_point_id, H.kp_has_obs, H.kp_outlier, H.kp_world_pos, C.addressof(Rp))
                assert set_state(h, C.byref(tf.params), C.byref(view), qt_p, C.byref(H)) == 0

            wall, dev = {}, {}

            def window(name, fn, keep_times):
                assert hip.hipEventRecord(e0, stream) == 0
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
                ms = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                if keep_times:
                    wall.setdefault(name, []).append((t1 - t0) * 1e3); dev.setdefault(name, []).append(float(ms.value))

            routes = {"parent": route_parent, "new": route_new}
            for name, fn in routes.items():
                for _ in range(a.warmup):
                    both_stages(); window(name, fn, False)
            for start in range(0, a.reps, 20):
                for name, fn in routes.items():
                    for _ in range(min(20, a.reps - start)):
                        both_stages(); window(name, fn, True)
            both_stages(); route_new(); both_stages(); route_parent()
            g = tf._finish_dict(Rn, an); e = tf._finish_dict(Rp, ap_)
            FS.same_result(g, e, "new route against the parent route")
            res.update(n_tracked_close=g["n_tracked_close"], n_non_tracked_close=g["n_non_tracked_close"], n_visited=g["n_visited"], n_created=g["n_created"], made=g["made"])
        for name in dev:
            res[name] = dict(hip_events=quartiles(dev[name]), host_wall=quartiles(wall[name]))
    pr, nw = res["parent"]["hip_events"], res["new"]["hip_events"]
    spread = max(pr["iqr_ms"], nw["iqr_ms"])
    res["bar"] = dict(rule="new median below the parent median by more than the larger interquartile range (HIP events); same integers and positions asserted",
                      larger_iqr_ms=spread, difference_ms=pr["median_ms"] - nw["median_ms"], met=bool(pr["median_ms"] - nw["median_ms"] > spread))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
