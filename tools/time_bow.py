#!/usr/bin/env python3
"""Time of the DBoW2 vocabulary calls on the device (lld_bow_transform, lld_bow_score) with a synthetic vocabulary of ORBvoc's size
(tests/bow_ref.make_vocab: k = 10, L = 6, about 10^6 words), measured with HIP events on the context's stream after warm-up, medians
over repeated calls.  Each call returns with its results on the host, so a time covers upload, kernels and download.
  (a) 2000 descriptors from host memory; (b) the same count read from lld_orb_extract's device buffer (extractor_descriptors);
  (c) two sets of 2000 in one call; (d) one query against 1000 candidate BowVectors.
    python tools/time_bow.py [out.json] [repeats=200]      (prints and writes one JSON object)
The per-kernel split comes from a run of its own under rocprofv3 --kernel-trace --stats."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bow_ref as B  # noqa: E402
from lld_slam_amd import Context, synth  # noqa: E402
from lld_slam_amd import vocabulary as voc  # noqa: E402
from lld_slam_amd.orb_extractor import ORBextractor  # noqa: E402


class Events:
    """hipEventRecord on the context's stream around one call; elapsed in ms."""

    def __init__(self, stream):
        self.hip = C.CDLL("libamdhip64.so.7")      # the runtime liblld_amd.so and torch already share
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def time(self, fn):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value


def timed(ev, fn, repeats, warm=20):
    for _ in range(warm):
        fn()
    t, w = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        t.append(ev.time(fn))
        w.append((time.perf_counter() - t0) * 1e3)
    t, w = np.array(t), np.array(w)
    return dict(event_median_ms=round(float(np.median(t)), 4), event_min_ms=round(float(t.min()), 4),
                event_p90_ms=round(float(np.percentile(t, 90)), 4), host_median_ms=round(float(np.median(w)), 4), repeats=repeats)


def seeded_pattern(seed=0):
    return np.random.default_rng(seed).integers(-13, 13, size=(256, 4)).astype(np.int32)


def main(out_path=None, repeats=200):
    t0 = time.perf_counter()
    V = B.make_vocab(22, k=10, L=6, p_early_leaf=0.002, p_stop=0.02)
    gen_s = time.perf_counter() - t0
    n_words = int(V["is_leaf"].sum())
    sc = synth.make_stereo_scene(0)
    left, right = np.ascontiguousarray(sc["left"][0]), np.ascontiguousarray(sc["right"][0])
    with Context(0) as ctx, voc.ORBVocabulary.from_arrays(ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"],
                                                          max_sets=2) as v, \
            ORBextractor(ctx, 2000, 1.2, 8, 12, 7, seeded_pattern(), max_cols=1241, max_rows=376, max_images=2) as ex:
        ev = Events(ctx.stream())
        d1, d2 = B.random_desc(1, 2000), B.near_leaves(V, 2, 2000)[0]
        F = ex([left, right])
        dev = voc.extractor_descriptors(ex, 0)
        host = timed(ev, lambda: v.transform(d1), repeats)
        from_ex = timed(ev, lambda: v.transform(dev), repeats)
        two = timed(ev, lambda: v.transform([d1, d2]), repeats)
        q = v.transform(d1)
        rng = np.random.default_rng(3)
        cands = []
        for _ in range(1000):
            w = np.unique(np.concatenate([q.word[rng.random(len(q.word)) < 0.3], rng.integers(0, n_words, 1500)])).astype(np.int32)
            val = rng.random(len(w)); val /= val.sum()
            cands.append((w, val))
        start = np.zeros(1001, np.int32); start[1:] = np.cumsum([len(w) for w, _ in cands])
        words = np.concatenate([w for w, _ in cands]); values = np.concatenate([x for _, x in cands])
        res = np.empty(1000)
        score = timed(ev, lambda: v.score_raw(q.word, q.value, start, words, values, res), repeats)
        out = dict(vocabulary=dict(k=10, L=6, nodes=int(len(V["parent"])), words=n_words, generator="tests/bow_ref.make_vocab(22, k=10, L=6)",
                                   generate_s=round(gen_s, 2)),
                   transform_2000_host=host, transform_extractor_device=dict(from_ex, n=int(dev[1]), keypoints=[int(F[0].n), int(F[1].n)]),
                   transform_two_sets_2000=two, score_1_vs_1000=dict(score, candidate_words=int(start[-1]), query_words=int(len(q.word))),
                   words_2000=int(len(q.word)), nodes_2000=int(len(q.node)))
    s = json.dumps(out, indent=1)
    print(s)
    if out_path:
        with open(out_path, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 200)
