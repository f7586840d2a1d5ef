"""Keyframe-database scenes in which thousands of keyframes score: deterministic op lists (the format of kfdb_ref.run_ops, plus
("reloc_cap", query_id, bow, capacity) for a query through the *_raw call with a small result buffer) with the sizes each must
reach.  CPU only: the device tests replay a scene on the library, the CPU tests hold the restatement's answers to a dense
recomputation.  Also check() and apply(), shared with test_gpu_kfdb.py.

One place is 40 words drawn from the first 2000 of a 10^4-word vocabulary.  A keyframe of the place drops a few of them and adds
private words from the other 8000; the query holds the 40 words with equal values, so maxCommonWords = 40, minCommonWords = 32
and every keyframe that keeps more than 32 of them is scored."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import bow_ref
import kfdb_ref as K

N_WORDS = 10_000
PLACE_POOL = 2000
PLACE_WORDS = 40
QUERY_KINDS = ("reloc", "loop", "reloc_cap")


# ------------------------------------------------------------------------------------------------------------------ shared with test_gpu_kfdb

def check(got, exp, what=""):
    ids, acc, stats = exp
    assert list(got.kf_id) == ids, f"{what}: ids {list(got.kf_id)[:10]} vs {ids[:10]}"
    assert np.array_equal(np.asarray(got.acc_score, np.float32).view(np.uint32), np.asarray(acc, np.float32).view(np.uint32)), what
    assert dict(n_sharing=got.n_sharing, max_common_words=got.max_common_words, min_common_words=got.min_common_words,
                n_scored=got.n_scored) == stats, what


def apply(dev, ref, op):
    """One scenario operation on both; returns (device Candidates, restatement result) for a query, else None."""
    k = op[0]
    if k == "add":
        dev.add(op[1], op[2]); ref.add(op[1], op[2])
    elif k == "erase":
        dev.erase(op[1]); ref.erase(op[1])
    elif k == "clear":
        dev.clear(); ref.clear()
    elif k == "cov":
        dev.set_covisibles(op[1], op[2]); ref.set_covisibles(op[1], op[2])
    elif k == "reloc":
        return dev.detect_relocalization_candidates(op[1], op[2]), ref.detect_relocalization_candidates(op[1], op[2])
    elif k == "loop":
        return dev.detect_loop_candidates(op[1], op[2], op[3], op[4]), ref.detect_loop_candidates(op[1], op[2], op[3], op[4])
    return None


# ------------------------------------------------------------------------------------------------------------------ vectors

def bow(words, u):
    """(words ascending, values / their sum): the sum runs in word order, as BowVector::normalize."""
    words, u = np.asarray(words, np.int64), np.asarray(u, np.float64)
    o = np.argsort(words, kind="stable")
    words, u = words[o], u[o]
    assert len(words) == 0 or np.all(np.diff(words) > 0)
    norm = 0.0
    for x in u.tolist():
        norm += abs(x)
    return words.astype(np.int32), u / norm


def make_place(rng):
    return np.sort(rng.choice(PLACE_POOL, PLACE_WORDS, replace=False)).astype(np.int64)


def place_query(place, n=None):
    w = place[: n or len(place)]
    return bow(w, np.ones(len(w)))


def place_keyframe(rng, place, drop, n_private, spread=0.1, extra=()):
    """The place's words without those at the positions `drop`, n_private words of the other 8000, and `extra`."""
    keep = np.ones(len(place), bool)
    keep[np.asarray(drop, np.int64)] = False
    private = PLACE_POOL + rng.choice(N_WORDS - PLACE_POOL, n_private, replace=False)
    words = np.concatenate([place[keep], private, np.asarray(extra, np.int64)])
    return bow(words, rng.uniform(1.0 - spread, 1.0 + spread, len(words)))


@dataclass
class Scene:
    name: str
    ops: list
    max_keyframes: int
    max_words: int
    n_words: int = N_WORDS
    least: dict = field(default_factory=dict)       # query index -> the least n_scored / n_kept / n_retained / n_out it must reach
    dense: tuple = ()                                 # queries that meet clean registers: the dense recomputation applies
    notes: dict = field(default_factory=dict)         # what the hand-stated expectations of a scene need

    @property
    def queries(self):
        return [op for op in self.ops if op[0] in QUERY_KINDS]


def _adds(ids, vecs):
    return [("add", int(i), v) for i, v in zip(ids, vecs)]


# ------------------------------------------------------------------------------------------------------------------ scenes

def _retained_keyframes(seed, n):
    """n keyframes of one place that all pass 0.75f * best on their own score: 0-4 dropped words (the first keyframe none, so
    maxCommonWords is 40) and 8-12 private ones put every score between about 36/52 and 40/48 of the query's."""
    rng = np.random.default_rng(seed)
    place = make_place(rng)
    vecs = []
    for i in range(n):
        d = int(rng.integers(0, 5)) if i else 0
        vecs.append(place_keyframe(rng, place, rng.choice(PLACE_WORDS, d, replace=False), int(rng.integers(8, 13))))
    return place, [1000 + i for i in range(n)], vecs


def all_retained(n):
    place, ids, vecs = _retained_keyframes(1000 + n, n)
    q = place_query(place)
    ops = _adds(ids, vecs) + [("reloc", 1, q)]
    full = dict(n_scored=n, n_kept=n, n_retained=n, n_out=n)
    least, dense = {0: full}, (0,)
    if n == 8192:                                    # a used handle: a loop query that leaves 103 out, then half the place's words
        conn = ids[::80]
        ops += [("loop", 2, q, conn, 0.0), ("reloc", 3, place_query(place, 20))]
        m = n - len(conn)
        least.update({1: dict(n_scored=m, n_kept=m, n_retained=m, n_out=m), 2: dict(n_scored=8000, n_kept=8000)})   # a few lack 4 of the 20
        dense = (0, 1, 2)                            # no covisibles: no register of an earlier query is read
    return Scene(f"all_retained[{n}]", ops, max_keyframes=n, max_words=1 << 20, least=least, dense=dense,
                 notes=dict(connected=103 if n == 8192 else 0))


def groups(interleaved):
    """200 covisibility groups of 11; member 3 holds exactly the place's words (the hub).  Every member keeps the place's first
    word, so the list order is the add order and each group is first met at the member added first."""
    rng = np.random.default_rng(2002 if interleaved else 2001)
    place = make_place(rng)
    G, M = 200, 11
    ids = {(g, m): 1000 + g * M + m for g in range(G) for m in range(M)}
    vec = {}
    for g in range(G):
        for m in range(M):
            if m == 3:
                vec[g, m] = place_keyframe(rng, place, [], 0)
            else:
                d = int(rng.integers(0, 5))
                vec[g, m] = place_keyframe(rng, place, 1 + rng.choice(PLACE_WORDS - 1, d, replace=False), int(rng.integers(8, 13)))
    if interleaved:
        order = [(int(g), m) for m in range(M) for g in rng.permutation(G)]
    else:
        order = [(g, m) for g in range(G) for m in range(M)]
    first_met = [g for g, m in order if m == order[0][1]] if interleaved else list(range(G))
    q = place_query(place)
    ops = _adds([ids[k] for k in order], [vec[k] for k in order])
    ops += [("cov", ids[g, m], [ids[g, o] for o in range(M) if o != m]) for g in range(G) for m in range(M)]
    ops += [("reloc", 1, q)]
    least = {0: dict(n_scored=G * M, n_kept=G * M, n_retained=G * M, n_out=G)}
    hubs = [ids[g, 3] for g in first_met]
    if not interleaved:                              # a used handle: 50 hubs connected to the query, then half the place's words
        ops += [("loop", 2, q, hubs[::4], 0.0), ("reloc", 3, place_query(place, 20))]
    return Scene("groups_interleaved" if interleaved else "groups", ops, max_keyframes=G * M, max_words=1 << 18, least=least,
                 dense=(0, 1) if not interleaved else (0,), notes=dict(hubs=hubs, connected=0 if interleaved else 50))


def order():
    """3000 keyframes lacking the first 0-5 place words; ids are a permutation of the slots; 1000 are erased and added again, so
    neither the id nor the slot gives the list order."""
    rng = np.random.default_rng(3001)
    place = make_place(rng)
    n = 3000
    ids = (5000 + rng.permutation(n)).tolist()
    vecs = [place_keyframe(rng, place, np.arange(int(rng.integers(0, 6)) if i else 0), int(rng.integers(8, 13))) for i in range(n)]
    again = rng.permutation(rng.choice(n, 1000, replace=False)).tolist()
    ops = _adds(ids, vecs) + [("erase", ids[i]) for i in sorted(again)]
    ops += _adds([ids[i] for i in again], [vecs[i] for i in again]) + [("reloc", 1, place_query(place))]
    return Scene("order", ops, max_keyframes=n, max_words=1 << 18, dense=(0,),
                 least={0: dict(n_scored=n, n_kept=n, n_retained=n, n_out=n)}, notes=dict(slot={i: s for s, i in enumerate(ids)}))


def identical():
    """2000 keyframes with one BowVector, each listing the next 10: every score ties, so each entry is its own pBestKF.  The last
    8 have at most 7 neighbours and 8 * s is not above 0.75f * 11 * s."""
    rng = np.random.default_rng(4001)
    place = make_place(rng)
    n = 2000
    v = place_keyframe(rng, place, [], 10)
    ids = [1000 + i for i in range(n)]
    ops = _adds(ids, [v] * n) + [("cov", ids[i], ids[i + 1: i + 11]) for i in range(n)] + [("reloc", 1, place_query(place))]
    return Scene("identical", ops, max_keyframes=n, max_words=1 << 17, dense=(0,),
                 least={0: dict(n_scored=n, n_kept=n, n_retained=n - 8, n_out=n - 8)})


def _spread_database(seed):
    """3000 keyframes of one place with 0-59 private words, 0-5 dropped words and values in [0.5, 1.5]; every second one also
    holds 10 further words of the first 2000 (the A words).  300 far keyframes share 20-32 of the place's words: a place query
    lists them without scoring them.  Each place keyframe lists far, place, far, place, far as its covisibles."""
    rng = np.random.default_rng(seed)
    place = make_place(rng)
    a_words = np.setdiff1d(np.arange(PLACE_POOL), place)[rng.choice(PLACE_POOL - PLACE_WORDS, 10, replace=False)]
    n, n_far = 3000, 300
    ids = [1000 + i for i in range(n)]
    far = [9000 + j for j in range(n_far)]
    vecs = [place_keyframe(rng, place, rng.choice(PLACE_WORDS, int(rng.integers(0, 6)), replace=False), int(rng.integers(0, 60)),
                           spread=0.5, extra=a_words if i % 2 == 0 else ()) for i in range(n)]
    far_vecs = [place_keyframe(rng, place, rng.choice(PLACE_WORDS, PLACE_WORDS - int(rng.integers(20, 33)), replace=False), 20)
                for _ in range(n_far)]
    ops = _adds(ids + far, vecs + far_vecs)
    for i in range(n):
        f = rng.choice(n_far, 3, replace=False)
        p = rng.choice(n, 2, replace=False)
        ops.append(("cov", ids[i], [far[f[0]], ids[p[0]], far[f[1]], ids[p[1]], far[f[2]]]))
    for j in range(n_far):
        ops.append(("cov", far[j], [ids[k] for k in rng.choice(n, 3, replace=False)]))
    return rng, place, a_words, ids, far, vecs, far_vecs, ops


def retain_cut():
    rng, place, a_words, ids, far, vecs, far_vecs, ops = _spread_database(5001)
    ops.append(("reloc", 1, place_query(place)))
    # accScore is the sum of three scores between about 0.4 and 0.9 of the query's, so 0.75f of the largest cuts through the middle
    # of them: hundreds stay (several wavefronts of them, a sort of at least 512 keys) and thousands go
    return Scene("retain_cut", ops, max_keyframes=3300, max_words=1 << 19, dense=(0,),
                 least={0: dict(n_scored=3000, n_kept=3000, n_retained=500, n_out=300)}, notes=dict(n_sharing=3300))


def loop():
    """The retain_cut database under a loop query with 500 connected keyframes; min_score is the median score of the 2500 that
    are scored (the mean of the two middle ones, so no score equals it), then one above every score."""
    rng, place, a_words, ids, far, vecs, far_vecs, ops = _spread_database(5001)
    q = place_query(place)
    conn = sorted(int(ids[i]) for i in rng.choice(len(ids), 500, replace=False))
    left = set(conn)
    s = np.sort(np.array([K.F32(bow_ref.score(q, v)) for i, v in zip(ids, vecs) if i not in left], np.float32))
    assert len(s) == 2500
    lo, hi = s[1249], s[1250]
    ms = np.float32((np.float64(lo) + np.float64(hi)) / 2)
    assert np.nextafter(np.nextafter(lo, np.float32(2)), np.float32(2)) < ms < np.nextafter(np.nextafter(hi, np.float32(0)), np.float32(0))
    ops += [("loop", 1, q, conn, float(ms)), ("loop", 2, q, conn, 2.0)]
    return Scene("loop", ops, max_keyframes=3300, max_words=1 << 19, dense=(0, 1),
                 least={0: dict(n_scored=2500, n_kept=1250, n_retained=300, n_out=200), 1: dict(n_scored=2500)},
                 notes=dict(n_sharing=2800, connected=500, far=far, min_score=float(ms)))


def capacity():
    place, ids, vecs = _retained_keyframes(1000 + 3000, 3000)
    q = place_query(place)
    ops = _adds(ids, vecs)
    for k, cap in enumerate((0, 1, 1000, 2999, 3000)):
        ops += [("reloc_cap", 10 + 2 * k, q, cap), ("reloc", 11 + 2 * k, q)]
    full = dict(n_scored=3000, n_kept=3000, n_retained=3000, n_out=3000)
    return Scene("capacity", ops, max_keyframes=3000, max_words=1 << 18, dense=tuple(range(10)), least={k: full for k in range(10)})


def carry():
    """Registers carried between queries on the retain_cut kind of database (see the comments at each query)."""
    rng, place, a_words, ids, far, vecs, far_vecs, ops = _spread_database(6001)
    q = place_query(place)
    qa = bow(np.concatenate([place, a_words]), np.ones(50))
    s1 = sorted(int(ids[i]) for i in rng.choice(3000, 500, replace=False))
    s2 = sorted(s1[:250] + [int(ids[i]) for i in rng.choice(3000, 250, replace=False)])
    back = [i for i in reversed(range(3000)) if i % 3]
    ops += [("reloc", 100, q),                       # 0: a plain query: every place keyframe is scored
            ("reloc", 100, q),                       # 1: the id again: every register takes += cnt, nothing is listed
            ("reloc", 101, qa),                      # 2: 50 words: only the 1500 with the A words pass the gate of 40; the others
                                                     #    are listed, and their mRelocScore of query 0 enters the accumulation
            ("loop", 7, q, s1, 0.0),                 # 3
            ("loop", 7, qa, s2, 0.0),                # 4: only s1 - s2 is listed; neighbours stamped by query 3 hold its scores
            ("clear",)]
    ops += _adds([ids[i] for i in back] + far[::-1], [vecs[i] for i in back] + far_vecs[::-1])
    ops += [("reloc", 102, qa)]                      # 5: a used handle after clear(): registers kept, the lists rebuilt
    return Scene("carry", ops, max_keyframes=3300, max_words=1 << 19,
                 least={0: dict(n_scored=3000, n_kept=3000), 2: dict(n_scored=1500, n_kept=1500), 5: dict(n_scored=1000, n_kept=1000)},
                 notes=dict(s1=s1, s2=s2, ids=ids, connected=500))


LONG_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 1000, 4000)
LONG_N_WORDS = 12 ** 4


def long_vectors():
    """Per length L: a keyframe with ceil(0.9 L) of its words in the 8000-word query and one that shares only its last word.  After
    each pair is added a query runs: the gate comes from the longest keyframe so far, whose overlap is known."""
    rng = np.random.default_rng(7001)
    qw = np.sort(rng.choice(LONG_N_WORDS, 8000, replace=False))
    other = np.setdiff1d(np.arange(LONG_N_WORDS), qw)
    q = bow(qw, rng.uniform(0.05, 3.0, len(qw)))
    ops, overlap = [], []
    for k, L in enumerate(LONG_LENGTHS):
        c = -(-9 * L // 10)
        near = np.concatenate([rng.choice(qw, c, replace=False), rng.choice(other, L - c, replace=False)])
        last = int(rng.choice(qw[-800:]))
        below = other[other < last]
        lone = np.concatenate([rng.choice(below, L - 1, replace=False), [last]])
        ops += [("add", 100 + 2 * k, bow(near, rng.uniform(0.05, 3.0, L))), ("add", 101 + 2 * k, bow(lone, rng.uniform(0.05, 3.0, L))),
                ("reloc", 1 + k, q)]
        overlap.append(c)
    return Scene("long_vectors", ops, max_keyframes=2 * len(LONG_LENGTHS), max_words=1 << 14, n_words=LONG_N_WORDS,
                 dense=tuple(range(len(LONG_LENGTHS))), least={k: dict(n_scored=1, n_kept=1, n_retained=1, n_out=1) for k in range(9)},
                 notes=dict(overlap=overlap))


ALL_RETAINED_SIZES = (63, 64, 65, 1023, 1024, 1025, 2049, 4097, 8192)
BUILDERS = {f"all_retained[{n}]": functools.partial(all_retained, n) for n in ALL_RETAINED_SIZES}
BUILDERS.update({"groups": functools.partial(groups, False), "groups_interleaved": functools.partial(groups, True), "order": order,
                 "identical": identical, "retain_cut": retain_cut, "loop": loop, "capacity": capacity, "carry": carry,
                 "long_vectors": long_vectors})
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name):
    return BUILDERS[name]()


# ------------------------------------------------------------------------------------------------------------------ the restatement's answers

def batched(ops):
    """The op list with each run of adds, erases and covisibility updates as one call: ("add_many", ids, vecs),
    ("erase_many", ids), ("cov_many", {id: covisibles}); the other ops unchanged."""
    out = []
    for op in ops:
        k = op[0]
        if k == "add":
            if not out or out[-1][0] != "add_many":
                out.append(("add_many", [], []))
            out[-1][1].append(op[1]); out[-1][2].append(op[2])
        elif k == "erase":
            if not out or out[-1][0] != "erase_many":
                out.append(("erase_many", []))
            out[-1][1].append(op[1])
        elif k == "cov":
            if not out or out[-1][0] != "cov_many" or op[1] in out[-1][1]:
                out.append(("cov_many", {}))
            out[-1][1][op[1]] = list(op[2])
        else:
            out.append(op)
    return out


@dataclass
class Answer:
    ids: list
    acc: list
    stats: dict
    detail: dict                                     # kfdb_ref's last_detail: n_kept, n_retained, n_out
    scores: dict                                     # id -> the score register of the query's kind, for the keyframes in the database
    listed: list                                     # kfdb_ref's last_listed: the ids of lKFsSharingWords in list order
    capacity: int | None = None                      # of a reloc_cap query


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's answer to every query of the scene, computed once.  Treat it as read-only."""
    sc = scene(name)
    ref = K.KeyFrameDatabase(sc.n_words, max_keyframes=sc.max_keyframes, max_words=sc.max_words)
    out = []
    for op in batched(sc.ops):
        k = op[0]
        if k == "add_many":
            ref.add_many(op[1], op[2])
        elif k == "erase_many":
            for i in op[1]:
                ref.erase(i)
        elif k == "cov_many":
            for i, nb in op[1].items():
                ref.set_covisibles(i, nb)
        elif k == "clear":
            ref.clear()
        elif k in ("reloc", "reloc_cap"):
            r = ref.detect_relocalization_candidates(op[1], op[2])
            out.append(Answer(r[0], r[1], r[2], dict(ref.last_detail), {i: ref.kfs[i].mRelocScore for i in ref.in_db}, ref.last_listed,
                              op[3] if k == "reloc_cap" else None))
        elif k == "loop":
            r = ref.detect_loop_candidates(op[1], op[2], op[3], op[4])
            out.append(Answer(r[0], r[1], r[2], dict(ref.last_detail), {i: ref.kfs[i].mLoopScore for i in ref.in_db}, ref.last_listed))
    return tuple(out)
