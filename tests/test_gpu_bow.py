"""lld_bow_* (DBoW2 vocabulary transform and L1 score on the device) against the numpy restatement tests/bow_ref.py, bit for bit:
f64 values are compared as uint64.  Vocabularies are generated (an irregular small one and one of ORBvoc's size); descriptors are
random (they tie constantly at ~128 bits, so the first-child rule is exercised), drawn near words, or extracted by lld_orb_extract."""
import ctypes as C

import numpy as np
import pytest

import bow_ref as B
import oracle_orbsearch as OS
import orb_extract_ref as R
from lld_slam_amd import ORBmatcher, abi
from lld_slam_amd import vocabulary as voc
from lld_slam_amd.orb_extractor import ORBextractor
from bow_ref import hand_queries, hand_tree

pytestmark = pytest.mark.gpu

CACHE = {}


def vocab_small(weighting=0):
    if "small" not in CACHE:
        CACHE["small"] = B.make_vocab(21, k=7, L=6, p_full=0.3, p_early_leaf=0.12, p_stop=0.05, order="dfs")
    return dict(CACHE["small"], weighting=weighting)


def vocab_big():
    if "big" not in CACHE:
        CACHE["big"] = B.make_vocab(22, k=10, L=6, p_early_leaf=0.002, p_stop=0.02)
    return CACHE["big"]


def tree(V):
    key = ("tree", id(V["parent"]), V["weighting"])
    if key not in CACHE:
        CACHE[key] = B.Tree(V)
    return CACHE[key]


def upload(ctx, V, **kw):
    return voc.ORBVocabulary.from_arrays(ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], V["scoring"],
                                         V["weighting"], **kw)


@pytest.fixture(scope="module")
def small(gpu_ctx):
    with upload(gpu_ctx, vocab_small()) as v:
        yield v


@pytest.fixture(scope="module")
def big(gpu_ctx):
    with upload(gpu_ctx, vocab_big(), max_sets=3) as v:
        yield v


def mixed_desc(V, seed, n):
    """Half random descriptors, half drawn near words."""
    r = B.random_desc(seed, n)
    near, _ = B.near_leaves(V, seed + 1, n)
    pick = np.random.default_rng(seed + 2).random(n) < 0.5
    return np.where(pick[:, None], near, r).astype(np.uint32)


def check(got: voc.BowTransform, exp: dict):
    for f in ("word", "node", "node_start", "feature", "feature_word", "feature_nid"):
        g = np.asarray(getattr(got, f))
        assert np.array_equal(g, exp[f]), f"{f} differs: {g[:8]} vs {exp[f][:8]}"
    assert got.value.dtype == np.float64
    assert np.array_equal(got.value.view(np.uint64), exp["value"].view(np.uint64)), "value differs"


def test_hand_tree_known_answers(gpu_ctx):
    V = hand_tree()
    with upload(gpu_ctx, V) as v:
        assert v.info["n_words"] == 7 and v.info["min_leaf_depth"] == 1 and v.info["max_depth"] == 2
        got = v.transform(hand_queries())
        check(got, B.transform(B.Tree(V), hand_queries(), 4))
        assert got.feature_nid[0] == 4 and got.feature_nid[10] == 3 and got.feature_word[9] == -1


@pytest.mark.parametrize("which", ["small", "big"])
@pytest.mark.parametrize("n", [0, 1, 2000, voc.MAX_FEATURES])
def test_transform_bit_exact(request, which, n):
    v = request.getfixturevalue(which)
    V = vocab_small() if which == "small" else vocab_big()
    d = mixed_desc(V, 100 + n, n) if n else np.zeros((0, 8), np.uint32)
    check(v.transform(d), B.transform(tree(V), d, 4))


def test_random_descriptors_tie(big):
    """Random descriptors: every level holds ties (checked on the restatement), the device follows the first-child rule."""
    V = vocab_big()
    d = B.random_desc(7, 2000)
    ch = tree(V).ch[0]
    ch = ch[ch >= 0]
    dist = B.distance(d[:, None, :], V["desc"][ch])
    assert ((dist == dist.min(axis=1, keepdims=True)).sum(axis=1) > 1).any()
    check(big.transform(d), B.transform(tree(V), d, 4))


@pytest.mark.parametrize("levelsup", [0, 4, 6, 7, 20, -2])
def test_levelsup(small, levelsup):
    V = vocab_small()
    d = mixed_desc(V, 5, 1500)
    check(small.transform(d, levelsup=levelsup), B.transform(tree(V), d, levelsup))


@pytest.mark.parametrize("weighting", [1, 2, 3])
def test_other_weightings(gpu_ctx, weighting):
    V = vocab_small(weighting)
    d = mixed_desc(V, 9, 3000)
    with upload(gpu_ctx, V) as v:
        check(v.transform(d), B.transform(B.Tree(V), d, 4))


def test_several_sets_in_one_call(big):
    V = vocab_big()
    sets = [mixed_desc(V, 31, 2000), np.zeros((0, 8), np.uint32), mixed_desc(V, 32, 777)]
    together = big.transform(sets)
    for s, got in zip(sets, together):
        check(got, B.transform(tree(V), s, 4))
        one = big.transform(s)
        for f in ("word", "node", "node_start", "feature", "feature_word", "feature_nid"):
            assert np.array_equal(getattr(one, f), getattr(got, f))
        assert np.array_equal(one.value.view(np.uint64), got.value.view(np.uint64))


def test_text_file_round_trip(gpu_ctx, tmp_path):
    V = vocab_small()
    p = tmp_path / "voc.txt"
    B.write_text(V, p, trailing_newline=True, blank_every=50)
    d = mixed_desc(V, 12, 2500)
    with voc.ORBVocabulary.from_text_file(gpu_ctx, p) as v:
        check(v.transform(d), B.transform(tree(V), d, 4))


def scene(cols, rows, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = 90 + 40 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
    for _ in range(80):
        cx, cy = rng.uniform(0, cols), rng.uniform(0, rows)
        w, h = rng.uniform(5, 60, 2)
        a = rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a); v = -(xx - cx) * np.sin(a) + (yy - cy) * np.cos(a)
        img[(np.abs(u) < w) & (np.abs(v) < h)] = rng.uniform(0, 255)
    img += rng.normal(0, 4, (rows, cols))
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def extracted(gpu_ctx):
    """A stereo-like pair: the right image is the left one shifted by 9 px plus fresh noise."""
    left = scene(1241, 376, 3)
    right = np.roll(left, -9, axis=1)
    right = np.clip(right.astype(np.int16) + np.random.default_rng(4).integers(-2, 3, right.shape), 0, 255).astype(np.uint8)
    ex = ORBextractor(gpu_ctx, 2000, 1.2, 8, 20, 7, R.seeded_pattern(7), max_cols=1241, max_rows=376, max_images=2)
    F = ex([left, right])
    yield ex, F
    ex.close()


def test_device_descriptors_from_the_extractor(big, extracted):
    ex, F = extracted
    V = vocab_big()
    dev = [voc.extractor_descriptors(ex, i) for i in (0, 1)]
    assert [n for _, n in dev] == [F[0].n, F[1].n] and F[0].n > 1000
    got_dev = big.transform(dev)                                           # on_device = 1: read in place
    got_host = big.transform([F[0].desc, F[1].desc])
    for gd, gh, f in zip(got_dev, got_host, F):
        check(gd, B.transform(tree(V), f.desc, 4))
        assert np.array_equal(gd.value.view(np.uint64), gh.value.view(np.uint64)) and np.array_equal(gd.feature, gh.feature)


def test_extract_transform_search_end_to_end(gpu_ctx, big, extracted):
    """extract -> transform (device descriptors) -> common nodes -> SearchByBoW on the device, against the oracle on the same lists."""
    ex, F = extracted
    t1, t2 = big.transform([voc.extractor_descriptors(ex, 0), voc.extractor_descriptors(ex, 1)])
    nd = voc.common_nodes(t1, t2)
    assert nd["n_nodes"] > 20
    # the lists are the FeatureVectors' own
    for j in range(nd["n_nodes"]):
        a = nd["idx1"][nd["start1"][j]:nd["start1"][j + 1]]
        assert len(set(t1.feature_nid[a].tolist())) == 1 and np.all(np.diff(a) > 0)
    F1, F2 = F
    valid = (np.random.default_rng(1).random(F1.n) < 0.9).astype(np.uint8)
    out = ORBmatcher(gpu_ctx, 0.7, True).SearchByBoWFrame(F1, F2, nd, valid)
    n_exp, fm = OS.search_by_bow_frame(F1, F2, nd["n_nodes"], nd["start1"], nd["idx1"], nd["start2"], nd["idx2"], valid, 0.7, True)
    assert out.n_matches == n_exp and n_exp > 50
    got = np.where(out.owner >= 0, out.query_kp[np.maximum(out.owner, 0)], -1)
    np.testing.assert_array_equal(got, fm)
    v2 = (np.random.default_rng(2).random(F2.n) < 0.9).astype(np.uint8)
    out = ORBmatcher(gpu_ctx, 0.75, True).SearchByBoWKF(F1, F2, nd, valid, v2)
    n_exp, m12 = OS.search_by_bow_kf(F1, F2, nd["n_nodes"], nd["start1"], nd["idx1"], nd["start2"], nd["idx2"], valid, v2, 0.75, True)
    assert out.n_matches == n_exp and n_exp > 50
    got = -np.ones(F1.n, np.int32); got[out.query_kp] = out.final_match()
    np.testing.assert_array_equal(got, m12)


def test_score_one_query_against_1000(big):
    V = vocab_big()
    W = big.n_words
    q = big.transform(mixed_desc(V, 40, 2000))
    rng = np.random.default_rng(41)
    cands = []
    for c in range(1000):
        if c == 0:
            cands.append((q.word, q.value))                               # itself
        elif c == 1:
            cands.append((np.empty(0, np.int32), np.empty(0)))            # empty
        elif c == 2:
            w = np.setdiff1d(np.arange(0, W, 97), q.word)[:500]           # disjoint: -0.0
            cands.append((w.astype(np.int32), np.full(len(w), 1.0 / len(w))))
        else:
            m = int(rng.integers(1, 2500))
            share = q.word[rng.random(len(q.word)) < rng.random()]
            w = np.unique(np.concatenate([share, rng.integers(0, W, m)])).astype(np.int32)
            val = rng.random(len(w)); val /= val.sum()
            cands.append((w, val))
    got = big.score_many(q, cands)
    exp = np.array([B.score((q.word, q.value), c) for c in cands])
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    assert got[0] == exp[0] and got.view(np.uint64)[2] == np.float64(-0.0).view(np.uint64)
    assert big.score(q, q) == B.score((q.word, q.value), (q.word, q.value))


def _create_status(ctx, V, **kw):
    d, keep = voc.desc_struct(V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"], V.get("scoring", 0),
                              V.get("weighting", 0), n_words=V.get("n_words"))
    h = C.c_void_p()
    f = ctx.lib.fn("bow_vocab_create")
    f.argtypes = [C.c_void_p, C.POINTER(voc.BowVocabDesc), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    st = f(ctx.handle, C.byref(d), kw.get("max_sets", 1), kw.get("max_features", 100), C.byref(h))
    if st == abi.LLD_OK:
        ctx.lib.fn("bow_vocab_destroy")(h)
    return st, h.value


def test_invalid_trees_are_refused(gpu_ctx):
    base = hand_tree()
    assert _create_status(gpu_ctx, base)[0] == abi.LLD_OK
    bad = []
    V = dict(base, parent=base["parent"].copy()); V["parent"][4] = 5; bad.append(V)              # parent after child
    V = dict(base, parent=base["parent"].copy()); V["parent"][0] = 0; bad.append(V)              # node 0 not the root
    V = dict(base, is_leaf=base["is_leaf"].copy()); V["is_leaf"][1] = 1; bad.append(V)           # flagged leaf with children
    V = dict(base, is_leaf=base["is_leaf"].copy()); V["is_leaf"][3] = 0; bad.append(V)           # childless non-word
    V = dict(base, n_words=6); bad.append(V)                                                      # count disagrees
    n = 66                                                                                        # 65 children of the root
    bad.append(dict(k=65, L=1, parent=np.r_[-1, np.zeros(n - 1)].astype(np.int32), is_leaf=np.r_[0, np.ones(n - 1)].astype(np.uint8),
                    desc=np.zeros((n, 8), np.uint32), weight=np.ones(n)))
    n = 19                                                                                        # a chain of depth 17 + a sibling leaf
    bad.append(dict(k=2, L=10, parent=np.r_[-1, np.arange(17), 0].astype(np.int32), is_leaf=np.r_[np.zeros(17), 1, 1].astype(np.uint8),
                    desc=np.zeros((n, 8), np.uint32), weight=np.ones(n)))
    bad.append(dict(base, parent=base["parent"][:1], is_leaf=base["is_leaf"][:1], desc=base["desc"][:1], weight=base["weight"][:1]))
    bad.append(dict(base, weighting=4))
    for i, V in enumerate(bad):
        st, h = _create_status(gpu_ctx, V)
        assert st == abi.LLD_ERR_INVALID and not h, i
    assert _create_status(gpu_ctx, dict(base, scoring=1))[0] == abi.LLD_ERR_UNSUPPORTED
    assert _create_status(gpu_ctx, base, max_features=voc.MAX_FEATURES + 1)[0] == abi.LLD_ERR_INVALID
    assert _create_status(gpu_ctx, base, max_sets=0)[0] == abi.LLD_ERR_INVALID
    # depth 16 exactly is accepted
    n = 18
    ok = dict(k=2, L=10, parent=np.r_[-1, np.arange(16), 0].astype(np.int32), is_leaf=np.r_[np.zeros(16), 1, 1].astype(np.uint8),
              desc=np.zeros((n, 8), np.uint32), weight=np.ones(n))
    assert _create_status(gpu_ctx, ok)[0] == abi.LLD_OK


def test_invalid_calls_are_refused_before_anything_is_queued(gpu_ctx, small):
    V = vocab_small()
    d = mixed_desc(V, 50, 300)
    before = small.transform(d)
    too_many = np.zeros((voc.MAX_FEATURES + 1, 8), np.uint32)
    assert small.transform_raw([too_many])[0] == abi.LLD_ERR_INVALID
    assert small.transform_raw([])[0] == abi.LLD_ERR_INVALID
    assert small.transform_raw([d] * (small.max_sets + 1))[0] == abi.LLD_ERR_INVALID
    assert small.transform_raw([(0, 5)])[0] == abi.LLD_ERR_INVALID                         # null device pointer with n > 0
    S = (voc.BowSet * 1)(); R_ = (voc.BowResult * 1)()
    S[0].n = 3; S[0].desc = d.ctypes.data_as(abi.c_uint32_p)
    assert small._transform(small.handle, 1, S, R_) == abi.LLD_ERR_INVALID                 # result arrays missing
    q = small.transform(d)
    out = np.zeros(2)
    W = small.n_words
    assert small.score_raw(q.word[::-1], q.value[::-1], [0, 0, 0], [], [], out) == abi.LLD_ERR_INVALID    # query not ascending
    assert small.score_raw(q.word, q.value, [0, 1, 2], [3, W], [0.5, 0.5], out) == abi.LLD_ERR_INVALID    # word out of range
    assert small.score_raw(q.word, q.value, [0, 2, 2], [5, 5], [0.5, 0.5], out) == abi.LLD_ERR_INVALID    # repeated word
    assert small.score_raw(q.word, q.value, [0, 2, 1], [5, 6], [0.5, 0.5], out) == abi.LLD_ERR_INVALID    # starts decrease
    assert small.score_raw(q.word, q.value, [-1, 0, 0], [5], [0.5], out) == abi.LLD_ERR_INVALID           # negative start
    after = small.transform(d)
    check(after, dict(word=before.word, value=before.value, node=before.node, node_start=before.node_start, feature=before.feature,
                      feature_word=before.feature_word, feature_nid=before.feature_nid))
    assert small.score(q, q) == B.score((q.word, q.value), (q.word, q.value))
