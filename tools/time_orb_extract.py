#!/usr/bin/env python3
"""Per-frame time of lld_orb_extract on a stereo pair at KITTI size and parameters (1241x376, ORBextractor(2000, 1.2, 8, 12, 7)):
host clock around synchronised calls after warm-up, (a) host images in, keypoints out; (b) images already in HBM, keypoints out.
The per-kernel split comes from a separate run under rocprofv3 --kernel-trace --stats (see tools/README.md).
    python tools/time_orb_extract.py [repeats=200]          (prints one JSON object)"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lld_slam_amd import Context, synth
from lld_slam_amd.orb_extractor import ORBextractor


def seeded_pattern(seed=0):
    return np.random.default_rng(seed).integers(-13, 13, size=(256, 4)).astype(np.int32)


def timed(fn, repeats, warm=10):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)   # lld_orb_extract returns after its stream sync
    t = np.array(t)
    return dict(min=round(float(t.min()), 4), median=round(float(np.median(t)), 4), p90=round(float(np.percentile(t, 90)), 4), repeats=repeats)


def main(repeats=200):
    import torch
    sc = synth.make_stereo_scene(0)
    left, right = np.ascontiguousarray(sc["left"][0]), np.ascontiguousarray(sc["right"][0])
    with Context(0) as ctx, ORBextractor(ctx, 2000, 1.2, 8, 12, 7, seeded_pattern(), max_cols=1241, max_rows=376, max_images=2) as ex:
        dl, dr = torch.from_numpy(left).to("cuda:0"), torch.from_numpy(right).to("cuda:0")
        torch.cuda.synchronize()
        dev = [(dl.data_ptr(), 1241, 376, 1241), (dr.data_ptr(), 1241, 376, 1241)]
        host_ms = timed(lambda: ex([left, right]), repeats)
        dev_ms = timed(lambda: ex(dev), repeats)
        L, R = ex([left, right])
        out = dict(image="1241x376 stereo pair (synth.make_stereo_scene(0))", params=[2000, 1.2, 8, 12, 7],
                   ms_per_frame_host_images=host_ms, ms_per_frame_device_images=dev_ms, keypoints=[int(L.n), int(R.n)],
                   level0_candidates=[int(L.stats[0, 0]), int(R.stats[0, 0])])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
