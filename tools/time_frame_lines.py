"""Times the line set-up of a stereo frame and Tracking::MatchLinesLastKF on 300 + 300 lines of dimension 72 (two wide-baseline frames of
tests/frame_lines_scenes.py), each two ways on the SAME library:
  (i)  lines of a fresh frame   parent: lld_line_match_stereo -> its host result -> lld_frame_set_lines;
                                new:    lld_frame_build_lines -> a stream synchronisation;
  (ii) new map lines            parent: lld_frame_track_download of both frames (the stage records a caller builds `occupied` and `skip` from) ->
                                        those two arrays on the host -> lld_line_match_last_frame with every input in host memory;
                                new:    lld_frame_new_map_lines on the two resident frames.
In (i) the frame (lld_frame_create) exists before the window and is destroyed after it, as one frame per image is; in (ii) both frames are
reset to the same state (lld_frame_track_set_state) before every window, because the new route changes what the current frame holds.
Every struct is filled before the timed window.  Each window is bracketed by two HIP events on the context's stream and by the host clock.
Medians and quartiles of --reps windows after --warmup; the routes alternate in blocks of 20 so that a drift of the machine meets both.
Bar: the new median below the parent's by more than the larger interquartile range, and both routes return the same integers.
Writes profiles/frame_lines_time.json when --out is given.  Needs an MI355X."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
N_LINES = 300


def quartiles(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(median_ms=float(med), q1_ms=float(q1), q3_ms=float(q3), iqr_ms=float(q3 - q1), min_ms=float(a[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import frame_lines_scenes as FS
    import oracle_tracking as OT
    from lld_slam_amd import Context, abi, host, orb_search
    from lld_slam_amd.tracking import DeviceTrackedFrame, FrameLines
    S = FS.last_kf_scene(0, N_LINES)
    cur, last = S["cur"], S["last"]
    F = FS.keypoint_frame()
    res = {"workload": "%d + %d lines of dimension %d per frame, two frames of synth.make_two_frame_lines (baseline 2 m), next to %d keypoints"
                       % (N_LINES, N_LINES, cur["desc"].shape[1], F.n),
           "reps": a.reps, "warmup": a.warmup, "library": os.path.relpath(abi.product_library_path(), ROOT),
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
        build = lib.fn("frame_build_lines")
        set_lines = lib.fn("frame_set_lines"); set_lines.argtypes = [C.c_void_p, C.POINTER(FrameLines)]; set_lines.restype = C.c_int
        wall, dev = {}, {}

        def window(name, fn, keep_times):
            assert hip.hipEventRecord(e0, stream) == 0
            t0 = time.perf_counter()
            out = fn()
            t1 = time.perf_counter()
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            if keep_times:
                wall.setdefault(name, []).append((t1 - t0) * 1e3); dev.setdefault(name, []).append(float(ms.value))
            return out

        def run(routes, before):
            for name, fn in routes.items():
                for _ in range(a.warmup):
                    before(); window(name, fn, False)
            for start in range(0, a.reps, 20):
                for name, fn in routes.items():
                    for _ in range(min(20, a.reps - start)):
                        before(); window(name, fn, True)

        # ---------------------------------------------------------------- (i) the lines of a fresh frame
        keep = []
        B = FS.build_struct(cur, keep, F)
        k = keep[0]
        sp = cur["stereo"]
        state = {}

        def fresh():
            if state.get("tf") is not None:
                state["tf"].close()
            state["tf"] = DeviceTrackedFrame(ctx, F, FS.CAM, None)              # lld_frame_create (synchronises itself)

        def lines_new():
            st = build(state["tf"].res.handle, C.byref(B)) | sync(ctx.handle)
            assert st == 0

        def lines_parent():
            m, _ = host.line_stereo_call(lib, ctx.handle, sp["K"], sp["b"], sp["tau"], sp["min_line_length"], k["left"], k["lo"], k["dl"], k["right"], k["ro"], k["dr"], True)
            L = FrameLines()
            L.n_left = k["left"].shape[0]; L.left = k["left"].ctypes.data_as(abi.c_float_p); L.left_octave = k["lo"].ctypes.data_as(abi.c_int32_p)
            L.n_right = k["right"].shape[0]; L.right = k["right"].ctypes.data_as(abi.c_float_p); L.right_octave = k["ro"].ctypes.data_as(abi.c_int32_p)
            L.line_matches = m.ctypes.data_as(abi.c_int32_p); L.desc = k["dl"].ctypes.data_as(abi.c_float_p); L.dim = k["dl"].shape[1]
            L.sx = B.sx; L.sy = B.sy
            assert set_lines(state["tf"].res.handle, C.byref(L)) == 0            # (synchronises itself)
            state["parent_matches"] = m

        run({"lines_parent": lines_parent, "lines_new": lines_new}, fresh)
        fresh(); lines_new(); state["tf"].n_lines = N_LINES
        got = state["tf"].lines_download()[0]
        fresh(); lines_parent()
        assert np.array_equal(got, state["parent_matches"])
        res["n_stereo_matches"] = int((got >= 0).sum())
        state["tf"].close()

        # ---------------------------------------------------------------- (ii) MatchLinesLastKF
        with DeviceTrackedFrame(ctx, F, FS.CAM, cur) as tc, DeviceTrackedFrame(ctx, F, FS.CAM, last) as tl:
            lm_c = tc.lines_download()[0]; lm_l = tl.lines_download()[0]
            views = {}

            def reset():
                views["c"] = FS.set_line_state(tc, S["T_cur"], S["cur_state"]); views["l"] = FS.set_line_state(tl, S["T_last"], S["last_state"])
                assert sync(ctx.handle) == 0

            reset()
            Tc, Tl = OT.frame_lines_camera(views["c"]), OT.frame_lines_camera(views["l"])
            tracked = np.asarray(S["cur_state"]["tracked"], np.int64)
            out = {}

            def kf_new():
                out["new"] = tc.new_map_lines(tl, 100000)

            def kf_parent():
                rc = tc.download(stage2=False)[0]; rl = tl.download(stage2=False)[0]        # the stage records: what the two frames hold
                c_id = np.asarray(S["cur_state"]["ln_line_id"]); l_id = np.asarray(S["last_state"]["ln_line_id"])
                del rc, rl                                                                  # (after set_state the records read as empty: the host's own lists stand in)
                occ = (c_id >= 0).astype(np.uint8)
                skip = ((l_id >= 0) & np.isin(l_id, np.concatenate([c_id[c_id >= 0], tracked]))).astype(np.uint8)
                c = dict(left_lines=cur["left_lines"], right_lines=cur["right_lines"], line_matches=lm_c, desc=cur["desc"], occupied=occ)
                l = dict(left_lines=last["left_lines"], right_lines=last["right_lines"], line_matches=lm_l, desc=last["desc"], left_octave=last["left_octave"], skip=skip)
                out["parent"] = host.line_lastkf_call(lib, ctx.handle, FS.K, Tc, Tl, FS.B, 6.0, 0.9, 1.0 / float(F.max_x), 1.0 / float(F.max_y), c, l, True)

            run({"new_lines_parent": kf_parent, "new_lines_new": kf_new}, reset)
            reset(); kf_new(); reset(); kf_parent()
            assert np.array_equal(out["new"]["match_last"], out["parent"][0]) and np.array_equal(out["new"]["created"], out["parent"][1])
            res["n_created"] = int(out["new"]["n_created"]); res["n_matched_last"] = int((out["new"]["match_last"] >= 0).sum())
        for name in dev:
            res[name] = dict(hip_events=quartiles(dev[name]), host_wall=quartiles(wall[name]))
    res["bar"] = {}
    for what in ("lines", "new_lines"):
        p, n = res[what + "_parent"]["hip_events"], res[what + "_new"]["hip_events"]
        spread = max(p["iqr_ms"], n["iqr_ms"])
        res["bar"][what] = dict(rule="new median below the parent median by more than the larger interquartile range (HIP events); same integers asserted",
                                larger_iqr_ms=spread, difference_ms=p["median_ms"] - n["median_ms"], met=bool(p["median_ms"] - n["median_ms"] > spread))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
