"""The scenes of tests/kfdb_scenes.py on the CPU: each reaches the sizes it declares, and the restatement's answers (which the
device is held to bit for bit) agree with a dense numpy recomputation that shares no code with the restatement's list walk."""
import math

import numpy as np
import pytest

import kfdb_ref as K
import kfdb_scenes as S

F32 = np.float32


def ulps(a, b):
    """Distance in float32 steps between non-negative floats."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------------------------ declared sizes

@pytest.mark.parametrize("name", S.NAMES)
def test_scene_reaches_its_declared_sizes(name):
    sc, ans = S.scene(name), S.reference(name)
    assert len(ans) == len(sc.queries) and sc.least
    for k, least in sc.least.items():
        got = dict(ans[k].detail, n_scored=ans[k].stats["n_scored"])
        print(f"{name} query {k}: n_sharing {ans[k].stats['n_sharing']} n_scored {got['n_scored']} n_kept {got['n_kept']} "
              f"n_retained {got['n_retained']} n_out {got['n_out']}")
        for key, v in least.items():
            assert got[key] >= v, (name, k, key, got[key], v)
        assert got["n_out"] == len(ans[k].ids)


def test_the_scenes_reach_the_limits_of_the_kernels():
    """n_scored and n_out 8192 (LLD_KFDB_MAX_KEYFRAMES), 500 connected keyframes, 4000 words in a keyframe, and every size of
    the bitonic sort from 64 to 8192."""
    n_scored = max(a.stats["n_scored"] for n in S.NAMES for a in S.reference(n))
    n_out = max(a.detail["n_out"] for n in S.NAMES for a in S.reference(n))
    connected = max(len(op[3]) for n in S.NAMES for op in S.scene(n).ops if op[0] == "loop")
    words = max(len(op[2][0]) for n in S.NAMES for op in S.scene(n).ops if op[0] == "add")
    print(f"largest n_scored {n_scored} n_out {n_out} connected {connected} words per keyframe {words}")
    assert n_scored == 8192 and n_out == 8192 and connected == 500 and words == 4000
    npad = {1 << int(a.detail["n_out"] - 1).bit_length() for n in S.NAMES for a in S.reference(n) if a.detail["n_out"] > 1}
    assert {64, 128, 1024, 2048, 4096, 8192} <= npad
    assert any(a.detail["n_kept"] > 1024 and a.detail["n_retained"] < a.detail["n_kept"] and a.detail["n_out"] < a.detail["n_retained"]
               for n in S.NAMES for a in S.reference(n))


# ------------------------------------------------------------------------------------------------------------------ hand-stated expectations

def test_order_follows_neither_the_id_nor_the_slot():
    sc, (a,) = S.scene("order"), S.reference("order")
    ids = np.array(a.ids)
    slots = np.array([sc.notes["slot"][i] for i in a.ids])
    d_id, d_slot = int((np.diff(ids) < 0).sum()), int((np.diff(slots) < 0).sum())
    print(f"order: {d_id} descents in id, {d_slot} in slot")
    assert sorted(a.ids) == sorted(sc.notes["slot"]) and d_id > 100 and d_slot > 100
    assert not np.array_equal(np.argsort(ids), np.argsort(slots))


def test_groups_return_each_hub_once_where_its_group_is_first_met():
    for name in ("groups", "groups_interleaved"):
        sc, a = S.scene(name), S.reference(name)[0]
        assert a.ids == sc.notes["hubs"], name
        assert (a.ids == sorted(a.ids)) == (name == "groups")
    a = S.reference("groups")
    assert len(set(a[1].ids) & set(S.scene("groups").notes["hubs"][::4])) == 0 and len(a[1].ids) == 200


def test_identical_keyframes_keep_themselves():
    (a,) = S.reference("identical")
    assert a.ids == list(range(1000, 2992))
    assert len(set(np.asarray(list(a.scores.values()), F32).view(np.uint32).tolist())) == 1
    assert len(set(np.asarray(a.acc, F32).view(np.uint32).tolist())) == 3         # 11, 10 and 9 equal terms


def test_capacity_scene_repeats_one_answer():
    ans = S.reference("capacity")
    assert [a.capacity for a in ans] == [0, None, 1, None, 1000, None, 2999, None, 3000, None]
    assert all(a.ids == ans[0].ids and len(a.ids) == 3000 for a in ans)


def test_loop_scene_skips_listed_neighbours_that_were_not_scored():
    sc, ans = S.scene("loop"), S.reference("loop")
    far, conn = set(sc.notes["far"]), set(sc.queries[0][3])
    assert ans[0].stats["n_sharing"] == 2800 and len(conn) == 500
    named = set()
    for op in sc.ops:
        if op[0] == "cov" and op[1] not in far and op[1] not in conn:
            named |= far & set(op[2][:10])
    assert named == far                              # each is a covisible of a scored keyframe
    assert ans[1].ids == [] and ans[1].detail["n_kept"] == 0 and ans[1].stats["n_scored"] == 2500
    s = np.array([v for i, v in ans[0].scores.items() if i not in far and i not in conn], F32)
    assert (s >= F32(sc.notes["min_score"])).sum() == 1250 == ans[0].detail["n_kept"]


def test_carry_scene_by_hand():
    sc, ans = S.scene("carry"), S.reference("carry")
    s1, s2, ids = set(sc.notes["s1"]), set(sc.notes["s2"]), sc.notes["ids"]
    empty = dict(n_sharing=0, max_common_words=0, min_common_words=0, n_scored=0)
    assert ans[1].ids == [] and ans[1].stats == empty                       # the id again: nothing is listed
    assert ans[2].stats == dict(n_sharing=3300, max_common_words=50, min_common_words=40, n_scored=1500)
    # the same query on registers that no query has touched: the stale scores of query 0 are gone, the answer differs
    db = [op for op in sc.ops[: sc.ops.index(sc.queries[0])]]
    fresh = K.run_ops(K.KeyFrameDatabase(sc.n_words), db + [sc.queries[2]])[0]
    assert fresh[2] == ans[2].stats and (fresh[0] != ans[2].ids or fresh[1] != ans[2].acc)
    assert ans[3].stats["n_sharing"] == 2800
    assert ans[4].stats["n_sharing"] == len(s1 - s2) and len(s1 - s2) >= 200     # those query 3 left unstamped, unless connected again
    back = [i for i in reversed(range(3000)) if i % 3]
    assert ans[5].stats["n_sharing"] == len(back) + 300 and ans[5].stats["n_scored"] == sum(i % 2 == 0 for i in back)
    assert set(ans[5].ids) <= {ids[i] for i in back}


def test_long_vectors_gate():
    sc, ans = S.scene("long_vectors"), S.reference("long_vectors")
    c = sc.notes["overlap"]
    for k, a in enumerate(ans):
        gate = int(F32(c[k]) * F32(0.8))
        assert a.stats == dict(n_sharing=2 * (k + 1), max_common_words=c[k], min_common_words=gate,
                               n_scored=sum(x > gate for x in c[: k + 1]) + (k == 0)), k


# ------------------------------------------------------------------------------------------------------------------ dense cross-check

class Dense:
    """The database as a keyframe x query-word matrix.  A query is answered from matrix products and sorts: the common-word
    counts are a product with a vector of ones, the position in lKFsSharingWords is (first common query word, add order), the
    score is 1 - 0.5 * sum |q - v| over the union of the words by math.fsum.  Registers are taken as never touched: the query id
    is new, and a keyframe that is not scored holds the score 0."""

    def __init__(self):
        self.vec, self.seq, self.cov, self.adds = {}, {}, {}, 0

    def op(self, op):
        k = op[0]
        if k == "add":
            self.vec[op[1]] = (np.asarray(op[2][0], np.int64), np.asarray(op[2][1], np.float64))
            self.seq[op[1]] = self.adds
            self.adds += 1
        elif k == "erase":
            self.vec.pop(op[1], None)
        elif k == "clear":
            self.vec.clear()
        elif k == "cov":
            self.cov[op[1]] = list(op[2])[:10]

    def query(self, op):
        loop = op[0] == "loop"
        qw, qv = np.asarray(op[2][0], np.int64), np.asarray(op[2][1], np.float64)
        ids = np.array(sorted(self.vec), np.int64)
        n, nq = len(ids), len(qw)
        M = np.zeros((n, nq))
        rest = []
        for r, i in enumerate(ids.tolist()):
            w, v = self.vec[i]
            at = np.minimum(np.searchsorted(qw, w), nq - 1)
            hit = qw[at] == w
            M[r, at[hit]] = v[hit]
            rest.append(v[~hit])
        P = M > 0
        common = P.astype(np.int64) @ np.ones(nq, np.int64)
        listed = common > 0
        if loop:
            listed &= ~np.isin(ids, np.asarray(op[3], np.int64))
        out = dict(n_sharing=int(listed.sum()), max_common_words=0, min_common_words=0, n_scored=0, n_kept=0, n_retained=0, n_out=0,
                   ids=[], acc=[], scores={}, margin=1 << 30, listed=[])
        if not listed.any():
            return out
        seq = np.array([self.seq[i] for i in ids.tolist()])
        order = np.lexsort((seq, P.argmax(axis=1)))
        order = order[listed[order]]
        out["listed"] = ids[order].tolist()
        maxc = int(common[listed].max())
        minc = int(F32(maxc) * F32(0.8))
        scored = listed & (common > minc)
        score = np.zeros(n, F32)
        for r in np.flatnonzero(scored).tolist():
            score[r] = F32(1.0 - 0.5 * math.fsum(np.abs(qv - M[r]).tolist() + rest[r].tolist()))
        out.update(max_common_words=maxc, min_common_words=minc, n_scored=int(scored.sum()),
                   scores={int(ids[r]): score[r] for r in np.flatnonzero(scored).tolist()})
        kept = scored & (score >= F32(op[4])) if loop else scored
        if loop and scored.any():
            out["margin"] = int(ulps(score[scored], F32(op[4])).min())
        admitted = scored if loop else listed
        row = {int(i): r for r, i in enumerate(ids.tolist())}
        entries = [r for r in order.tolist() if kept[r]]
        if not entries:
            return out
        acc, best = [], []
        for r in entries:
            rows = [r] + [row[j] for j in self.cov.get(int(ids[r]), []) if j in row and admitted[row[j]]]
            terms = score[rows]
            acc.append(np.cumsum(terms, dtype=F32)[-1])
            best.append(rows[int(np.argmax(terms))])
        acc, best = np.array(acc, F32), np.array(best)
        thr = F32(0.75) * max(F32(op[4]) if loop else F32(0.0), acc.max())
        retained = acc > thr
        _, firsts = np.unique(best[retained], return_index=True)
        firsts = np.sort(firsts)
        out.update(n_kept=len(entries), n_retained=int(retained.sum()), n_out=len(firsts), ids=ids[best[retained][firsts]].tolist(),
                   acc=acc[retained][firsts], margin=min(out["margin"], int(ulps(acc, thr).min())))
        return out


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.BUILDERS[n] is not S.carry])
def test_restatement_against_the_dense_recomputation(name):
    sc, ans = S.scene(name), S.reference(name)
    assert sc.dense
    dense, k = Dense(), 0
    for op in sc.ops:
        if op[0] not in S.QUERY_KINDS:
            dense.op(op)
            continue
        if k in sc.dense:
            d, a = dense.query(op), ans[k]
            what = f"{name} query {k}"
            assert {key: d[key] for key in a.stats} == a.stats, what
            assert {key: d[key] for key in a.detail} == a.detail, what
            assert d["listed"] == a.listed, what
            # the two double sums differ by far less than a float step, so one rounding to float moves at most one step
            assert len(d["scores"]) == a.stats["n_scored"]
            if d["scores"]:
                assert int(ulps(list(d["scores"].values()), [a.scores[i] for i in d["scores"]]).max()) <= 1, what
            # no accScore within 2 steps of 0.75f * best, no score within 2 of minScore: no id hangs on the last bit
            assert d["margin"] > 2, what
            assert d["ids"] == a.ids, what
            if a.ids:
                assert int(ulps(d["acc"], a.acc).max()) <= 2, what
        k += 1
    assert k == len(ans)
