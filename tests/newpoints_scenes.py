"""The fixed scenes of the new-map-point tests, built once per process and shared (problem, reference result)."""
import functools

import newpoints_ref as R

# name -> (seed, matches per pair, monocular)
SEEDED = {
    "stereo10": (11, [300] * 10, False),          # 10 pairs in stereo mode: both-stereo, one-stereo and no-stereo keypoints
    "mono20": (12, [300] * 20, True),             # 20 pairs x 300 matches in mono mode
    "one": (13, [1], False),
    "w63": (14, [63], False), "w64": (15, [64], False), "w65": (16, [65], False),
    "empty_middle": (17, [70, 0, 90], False),     # 3 pairs, the middle one without a match
    "skipped_second": (18, [80, 50, 130, 20], False),   # 4 pairs, the second below the baseline gate
}


@functools.lru_cache(maxsize=None)
def scene(name):
    seed, nm, mono = SEEDED[name]
    pb = R.make_scene(seed, nm, monocular=mono)
    return pb, R.triangulate(pb)


@functools.lru_cache(maxsize=None)
def crafted():
    return [(pb, R.triangulate(pb), st, src, x) for pb, st, src, x in R.crafted_scenes()]
