"""Times "grey image + depth image -> resident RGB-D frame ready for lld_frame_track_motion_model" on a 640x480 image with the TUM1
intrinsics and distortion coefficients, ORBextractor(1000, 1.2, 8, 20, 7) and a 16-bit depth image (factor 1/5000), two ways on the SAME
library:
  * parent route  lld_orb_extract -> its host results -> undistortion and depth look-up on the host (the numpy restatement
                  tests/frame_mono_ref.py, the only host code the project has for it) -> lld_frame_create: what a caller had before
                  lld_frame_build_mono existed;
  * new route     lld_orb_extract -> lld_frame_build_mono -> a stream synchronisation.
Every struct is filled before the timed window.  Each window is bracketed by two HIP events on the context's stream (the first recorded
before lld_orb_extract, the second after the last call of the route and waited for), and by the host clock.  Medians and quartiles of --reps
windows after --warmup; the routes alternate in blocks of 20 so that a drift of the machine meets both.  Bar: the new median below the parent's
by more than the larger interquartile range.  Writes profiles/frame_mono_time.json when --out is given.  Needs an MI355X."""
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
TUM1 = (1000, 1.2, 8, 20, 7)
W, H = 640, 480
CAM = (517.306408, 516.469215, 318.643040, 255.313989)
DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
MBF, FACTOR = 40.0, 1.0 / 5000.0


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
    import frame_mono_ref as M
    import orb_extract_ref as R
    from lld_slam_amd import Context, abi, orb_search, synth
    from lld_slam_amd.orb_extractor import ORBextractor
    grey = synth.make_stereo_scene(0, n=50, width=W, height=H)["left"][0]
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.round((1.5 + 2.5 * (yy / H) + 0.4 * np.sin(xx / 37.0)) * 5000.0).astype(np.uint16)
    depth[np.random.default_rng(1).random((H, W)) < 0.1] = 0
    res = {"workload": "640x480 grey image, ORBextractor(1000, 1.2, 8, 20, 7), TUM1 intrinsics and coefficients, uint16 depth image with factor 1/5000",
           "reps": a.reps, "warmup": a.warmup, "library": os.path.relpath(abi.product_library_path(), ROOT),
           "timer": "HIP events on the context's stream around each window (lld_orb_extract included), and the host clock around the same calls"}
    with Context(0) as ctx, ORBextractor(ctx, *TUM1, R.seeded_pattern(7), max_cols=W, max_rows=H, max_images=1) as ex:
        lib = ctx.lib
        hip = C.CDLL("libamdhip64.so")
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]; hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]; hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        stream = C.c_void_p(lib.fn("ctx_stream")(ctx.handle))
        sync = lib.fn("ctx_synchronize")
        destroy = lib.fn("frame_destroy"); destroy.argtypes = [C.c_void_p]; destroy.restype = None
        create = lib.fn("frame_create"); create.argtypes = [C.c_void_p, C.POINTER(orb_search.OrbSearch), C.POINTER(C.c_void_p)]; create.restype = C.c_int
        build = lib.fn("frame_build_mono")
        build.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.DepthImage), C.POINTER(abi.FrameMonoParams), C.POINTER(C.c_void_p)]; build.restype = C.c_int

        L = ex(grey)
        res["n_keypoints"] = L.n
        Hf = orb_search.mono_host_frame(lib, L, CAM, DIST)
        prm, keep = orb_search.frame_mono_params(Hf, CAM, DIST, MBF)
        D, keep2 = orb_search.depth_image_struct(depth, FACTOR)
        last = {}

        def new_route():
            h = C.c_void_p()
            L1 = ex(grey)                                                       # lld_orb_extract; its host results are not read
            st = build(ex.handle, 0, C.byref(D), C.byref(prm), C.byref(h))
            st |= sync(ctx.handle)
            assert st == 0
            return h

        def parent_route():
            h = C.c_void_p()
            L1 = ex(grey)                                                       # lld_orb_extract and its host results
            r = M.build(L1.xy, CAM, DIST, MBF, depth, FACTOR)                  # undistortion and depth look-up on the host
            F2 = orb_search.Frame(desc=L1.desc, xy=r["xy_un"], octave=L1.octave, uright=r["u_right"], angle=L1.angle, min_x=Hf.min_x, max_x=Hf.max_x,
                                  min_y=Hf.min_y, max_y=Hf.max_y, scale=L1.scale, sigma2=L1.sigma2, inv_sigma2=L1.inv_sigma2)
            prep = orb_search.prepare(F2, np.zeros((0, 8), np.uint32), candidates=orb_search.CAND_GRID, accept_max=orb_search.TH_HIGH)
            assert create(ctx.handle, C.byref(prep.s), C.byref(h)) == 0        # (synchronises itself)
            last["exp"] = r
            return h

        routes = {"parent": parent_route, "new": new_route}
        wall = {k: [] for k in routes}; dev = {k: [] for k in routes}

        def window(name, keep_times):
            assert hip.hipEventRecord(e0, stream) == 0
            t0 = time.perf_counter()
            h = routes[name]()
            t1 = time.perf_counter()
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            if keep_times:
                wall[name].append((t1 - t0) * 1e3); dev[name].append(float(ms.value))
            return h

        for name in routes:
            for _ in range(a.warmup):
                destroy(window(name, False))
        block = 20
        for start in range(0, a.reps, block):
            for name in routes:
                for _ in range(min(block, a.reps - start)):
                    destroy(window(name, True))
        # the two routes give the same frame
        built = orb_search.MonoBuiltFrame(lib, ctx.handle, Hf, new_route())
        got = built.download(); built.close()
        destroy(parent_route())
        for f in ("xy_un", "u_right", "depth"):
            assert np.array_equal(np.ascontiguousarray(getattr(got, f)).view(np.uint32), last["exp"][f].view(np.uint32)), f
        res["n_with_depth"] = int((got.depth > 0).sum())
        for name in routes:
            res[name] = dict(hip_events=quartiles(dev[name]), host_wall=quartiles(wall[name]))
    p, n = res["parent"]["hip_events"], res["new"]["hip_events"]
    spread = max(p["iqr_ms"], n["iqr_ms"])
    res["bar"] = dict(rule="new median below the parent median by more than the larger interquartile range (HIP events)", larger_iqr_ms=spread,
                      difference_ms=p["median_ms"] - n["median_ms"], met=bool(p["median_ms"] - n["median_ms"] > spread))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
