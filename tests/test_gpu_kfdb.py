"""lld_kfdb_* (the KeyFrameDatabase on the device) against the restatement tests/kfdb_ref.py: after every query the ids in order,
the full count, the four counters and the accScores as float32 bits must be equal.  Registers carried between queries are
covered by long interleaved sequences of add / erase / clear / set_covisibles and both queries."""
import numpy as np
import pytest

import bow_ref as B
import kfdb_ref as K
from kfdb_scenes import apply, check
from lld_slam_amd import abi
from lld_slam_amd import vocabulary as voc
from lld_slam_amd.keyframe_database import KeyFrameDatabase

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vocab(gpu_ctx):
    V = B.make_vocab(41, k=10, L=4, p_full=1.0)             # 10^4 words
    with voc.ORBVocabulary.from_arrays(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"]) as v:
        yield v


@pytest.mark.parametrize("name", sorted(K.SCENARIOS))
def test_known_answers_on_the_device(vocab, name):
    ops, exp = K.SCENARIOS[name]
    ref = K.KeyFrameDatabase(vocab.n_words)
    with KeyFrameDatabase(vocab, max_keyframes=64, max_words=4096) as dev:
        n = 0
        for op in ops:
            r = apply(dev, ref, op)
            if r is not None:
                check(r[0], r[1], f"{name} query {n}")
                if isinstance(exp[n], tuple):
                    assert list(r[0].kf_id) == exp[n][0]
                n += 1


def sequence(vocab, seed, n_kf, words_per_kf, n_queries, max_words, clear_at=None):
    """Walks a trajectory: adds keyframes with their covisibility, erases some, and interleaves reloc and loop queries (query ids
    repeat now and then).  Returns the number of pool words appended, for the compaction check."""
    ids, place, vecs = K.trajectory(seed, n_kf, vocab.n_words, words_per_kf=words_per_kf)
    cov = K.covisibility(ids, vecs)
    rng = np.random.default_rng(seed + 100)
    ref = K.KeyFrameDatabase(vocab.n_words, max_words=max_words)
    appended, live, queries, frame_id = 0, {}, 0, 1000
    query_every = max(1, n_kf // n_queries)
    with KeyFrameDatabase(vocab, max_keyframes=min(8192, n_kf + 16), max_words=max_words) as dev:
        for i, (kid, v) in enumerate(zip(ids, vecs)):
            if live and sum(len(x[0]) for x in live.values()) + len(v[0]) > max_words:
                for e in sorted(live)[: max(1, len(live) // 4)]:
                    dev.erase(e); ref.erase(e); live.pop(e)
            dev.add(kid, v); ref.add(kid, v)
            live[kid] = v
            appended += len(v[0])
            nb = [n for n in cov[kid] if n < kid]
            updates = {kid: nb}
            for n in nb[:3]:
                updates[n] = [m for m in cov[n] if m <= kid]
            dev.set_covisibles(updates)
            for a, b in updates.items():
                ref.set_covisibles(a, b)
            if rng.random() < 0.03 and len(live) > 5:
                e = int(rng.choice(sorted(live)))
                dev.erase(e); ref.erase(e); live.pop(e)
            if clear_at is not None and i == clear_at:
                dev.clear(); ref.clear(); live.clear()
            if i % query_every == 0 and i > 3:
                j = int(rng.integers(0, i + 1))
                q = vecs[j]
                if rng.random() < 0.5:                          # a frame near keyframe j: drop some words, renormalise
                    keep = rng.random(len(q[0])) < 0.8
                    q = K.normalized(q[0][keep], rng) if keep.any() else q
                if rng.random() < 0.1:
                    frame_id -= 1                               # a reloc query id used again
                frame_id += 1
                g, e = dev.detect_relocalization_candidates(frame_id, q), ref.detect_relocalization_candidates(frame_id, q)
                check(g, e, f"seed {seed} reloc at {i}")
                ms = float(np.float32(rng.choice([0.0, 0.01, 0.05, 0.2])))
                conn = cov[ids[j]][: int(rng.integers(0, 8))]
                g, e = dev.detect_loop_candidates(ids[j], vecs[j], conn, ms), ref.detect_loop_candidates(ids[j], vecs[j], conn, ms)
                check(g, e, f"seed {seed} loop at {i}")
                queries += 2
    return appended, queries


@pytest.mark.parametrize("seed,n_kf,wpk,n_queries", [(1, 300, 80, 150), (2, 1000, 60, 150), (3, 4000, 30, 100)])
def test_interleaved_sequences(vocab, seed, n_kf, wpk, n_queries):
    appended, queries = sequence(vocab, seed, n_kf, wpk, n_queries, max_words=1 << 22, clear_at=n_kf // 2 if seed == 1 else None)
    assert queries >= n_queries


def test_a_run_that_compacts(vocab):
    max_words = 6000
    appended, queries = sequence(vocab, 4, 600, 60, 200, max_words=max_words)
    assert appended > 3 * max_words and queries >= 200      # the pool was reused: compaction ran


def test_refusals_leave_the_database_unchanged(vocab):
    W = vocab.n_words
    ref = K.KeyFrameDatabase(W, max_keyframes=6, max_words=40)
    with KeyFrameDatabase(vocab, max_keyframes=6, max_words=40) as dev:
        for kid, d in ((1, {0: 0.5, 1: 0.5}), (2, {0: 0.25, 3: 0.75}), (3, {1: 0.5, 3: 0.5})):
            apply(dev, ref, ("add", kid, K._v(d)))
        apply(dev, ref, ("cov", 2, [1, 3]))
        q = K._v({0: 0.5, 1: 0.25, 3: 0.25})
        bad_words = (np.array([4, 2], np.int32), np.array([0.5, 0.5]))
        out_of_range = (np.array([W], np.int32), np.array([1.0]))
        refusals = [lambda: dev.add_raw([1], [K._v({5: 1.0})]),                       # already in the database
                    lambda: dev.add_raw([4, 4], [K._v({5: 1.0}), K._v({6: 1.0})]),    # twice in one call
                    lambda: dev.add_raw([4], [bad_words]), lambda: dev.add_raw([4], [out_of_range]),
                    lambda: dev.add_raw([4, 5, 6, 7], [K._v({5 + i: 1.0}) for i in range(4)]),    # slots
                    lambda: dev.add_raw([4], [K._v({10 + i: 1 / 40 for i in range(40)})]),       # words
                    lambda: dev.set_covisibles_raw([1], [[10, 11, 12, 13]]),                      # slots
                    lambda: dev.detect_relocalization_candidates_raw(9, bad_words)[0],
                    lambda: dev.detect_loop_candidates_raw(9, out_of_range, [], 0.0)[0]]
        for n, bad in enumerate(refusals):
            assert bad() == abi.LLD_ERR_INVALID, n
            r = apply(dev, ref, ("reloc", 100 + n, q))
            check(r[0], r[1], f"after refusal {n}")
            r = apply(dev, ref, ("loop", 200 + n, q, [3], 0.0))
            check(r[0], r[1], f"after refusal {n}")
        assert dev.erase_raw([77]) == abi.LLD_OK
        st, out, full = dev.detect_relocalization_candidates_raw(300, q, capacity=0)   # runs, stamps, reports the count
        e = ref.detect_relocalization_candidates(300, q)
        assert st == abi.LLD_OK and full == len(e[0]) and len(out.kf_id) == 0
        r = apply(dev, ref, ("reloc", 300, q))
        check(r[0], r[1], "after the capacity-0 query")


def test_end_to_end_from_descriptors(gpu_ctx):
    V = B.make_vocab(43, k=6, L=4, p_full=1.0)
    T = B.Tree(V)
    with voc.ORBVocabulary.from_arrays(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], max_sets=4) as v, \
            KeyFrameDatabase(v, max_keyframes=64, max_words=1 << 16) as dev:
        ref = K.KeyFrameDatabase(v.n_words)
        base = [B.near_leaves(V, 50 + p, 400)[0] for p in range(6)]
        rng = np.random.default_rng(5)
        bows = []
        for i in range(24):
            d = base[i % 6].copy()
            d[rng.random(len(d)) < 0.3] = B.random_desc(i, 1)[0]
            got = v.transform(d)
            exp = B.transform(T, d, 4)
            assert np.array_equal(got.word, exp["word"]) and np.array_equal(got.value.view(np.uint64), exp["value"].view(np.uint64))
            dev.add(i + 1, got); ref.add(i + 1, (exp["word"], exp["value"]))
            bows.append(exp)
            cov = [j + 1 for j in range(max(0, i - 3), i)][::-1]
            dev.set_covisibles(i + 1, cov); ref.set_covisibles(i + 1, cov)
        for qi in range(12):
            d = base[qi % 6].copy()
            d[rng.random(len(d)) < 0.4] = B.random_desc(100 + qi, 1)[0]
            got = v.transform(d)
            exp = B.transform(T, d, 4)
            q = (exp["word"], exp["value"])
            check(dev.detect_relocalization_candidates(qi + 1, got), ref.detect_relocalization_candidates(qi + 1, q), f"reloc {qi}")
            check(dev.detect_loop_candidates(100 + qi, got, [qi + 1], 0.01), ref.detect_loop_candidates(100 + qi, q, [qi + 1], 0.01),
                  f"loop {qi}")
