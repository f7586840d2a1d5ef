#!/usr/bin/env python3
"""Time of the device KeyFrameDatabase (lld_kfdb_*) on a synthetic vocabulary of ORBvoc's size (tests/bow_ref.make_vocab: k = 10,
L = 6, about 10^6 words), measured with HIP events on the context's stream after warm-up, medians over repeated calls.  Every call
returns with its results on the host, so a time covers upload, kernels and download.
  Databases of 1000 and 4000 keyframes of about 1500 words each, drawn Zipf-skewed (rank r ~ r^-1.1, through a fixed permutation
  of the word ids) plus words shared with the trajectory neighbours; each keyframe has up to 10 covisibles.
  (a) DetectRelocalizationCandidates and (b) DetectLoopCandidates (5 connected, minScore 0.01) of a frame near a stored keyframe,
  a fresh query id per call; (c) one add and (d) one erase of a 1500-word keyframe into the 4000-keyframe database.
    python tools/time_kfdb.py [out.json] [repeats=200]      (prints and writes one JSON object)
The per-kernel split comes from a run of its own under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bow_ref as B  # noqa: E402
from time_bow import Events, timed  # noqa: E402
from lld_slam_amd import Context  # noqa: E402
from lld_slam_amd import vocabulary as voc  # noqa: E402
from lld_slam_amd.keyframe_database import KeyFrameDatabase  # noqa: E402

WORDS_PER_KF = 1500


def keyframes(seed, n_kf, n_words):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_words)
    vecs, prev = [], None
    for i in range(n_kf):
        r = rng.zipf(1.1, 4 * WORDS_PER_KF) - 1
        w = np.unique(perm[r[r < n_words]])[: WORDS_PER_KF // 2]
        if prev is not None:                                  # about half the words shared with the previous keyframe
            w = np.union1d(w, prev[rng.random(len(prev)) < 0.5])
        w = np.union1d(w, rng.integers(0, n_words, max(0, WORDS_PER_KF - len(w))))[: int(WORDS_PER_KF * 1.1)]
        w = np.unique(w).astype(np.int32)
        v = rng.uniform(0.05, 3.0, len(w))
        vecs.append((w, v / v.sum()))
        prev = w
    return vecs


def main(out_path=None, repeats=200):
    t0 = time.perf_counter()
    V = B.make_vocab(22, k=10, L=6, p_early_leaf=0.002, p_stop=0.02)
    n_words = int(V["is_leaf"].sum())
    gen_s = time.perf_counter() - t0
    out = dict(vocabulary=dict(k=10, L=6, words=n_words, generator="tests/bow_ref.make_vocab(22, k=10, L=6)", generate_s=round(gen_s, 2)))
    rng = np.random.default_rng(9)
    with Context(0) as ctx, voc.ORBVocabulary.from_arrays(ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"]) as v:
        ev = Events(ctx.stream())
        for n_kf in (1000, 4000):
            vecs = keyframes(n_kf, n_kf, n_words)
            total = sum(len(w) for w, _ in vecs)
            with KeyFrameDatabase(v, max_keyframes=n_kf + 8, max_words=total + 4 * WORDS_PER_KF) as db:
                db.add(list(range(1, n_kf + 1)), vecs)
                db.set_covisibles({i: [j for j in range(max(1, i - 5), min(n_kf, i + 5) + 1) if j != i] for i in range(1, n_kf + 1)})
                qid = [10 ** 6]
                j = n_kf // 2
                qw, qv = vecs[j]
                keep = rng.random(len(qw)) < 0.8
                q = (qw[keep], qv[keep] / qv[keep].sum())

                def reloc():
                    qid[0] += 1
                    return db.detect_relocalization_candidates(qid[0], q)

                def loop():
                    qid[0] += 1
                    return db.detect_loop_candidates(qid[0], q, [j - 1, j, j + 1, j + 2, j + 3], 0.01)

                r, l = reloc(), loop()
                out[f"reloc_{n_kf}"] = dict(timed(ev, reloc, repeats), n_sharing=r.n_sharing, n_scored=r.n_scored,
                                            n_candidates=int(len(r.kf_id)))
                out[f"loop_{n_kf}"] = dict(timed(ev, loop, repeats), n_sharing=l.n_sharing, n_scored=l.n_scored,
                                           n_candidates=int(len(l.kf_id)))
                out[f"db_{n_kf}"] = dict(keyframes=n_kf, words=int(total), mean_words=round(total / n_kf, 1))
                if n_kf == 4000:
                    extra = keyframes(77, 1, n_words)[0]
                    ta, te = [], []
                    for k in range(20 + repeats):
                        a = ev.time(lambda: db.add(999999, extra))
                        e = ev.time(lambda: db.erase(999999))
                        if k >= 20:
                            ta.append(a); te.append(e)
                    out["add_1_into_4000"] = dict(event_median_ms=round(float(np.median(ta)), 4), event_min_ms=round(float(min(ta)), 4),
                                                  words=int(len(extra[0])), repeats=repeats)
                    out["erase_1_from_4000"] = dict(event_median_ms=round(float(np.median(te)), 4), event_min_ms=round(float(min(te)), 4),
                                                    repeats=repeats)
    s = json.dumps(out, indent=1)
    print(s)
    if out_path:
        with open(out_path, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 200)
