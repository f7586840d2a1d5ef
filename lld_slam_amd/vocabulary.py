"""DBoW2's ORBVocabulary on the device (lld_bow_*): ctypes mirrors of the structs of include/lld_amd.h and a class with the
reference's names: from_text_file (loadFromTextFile), transform (BowVector + FeatureVector) and score (L1Scoring::score)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import c_double_p, c_int32_p, c_uint8_p, c_uint32_p

MAX_FEATURES = 8192          # LLD_BOW_MAX_FEATURES
L1_NORM = 0
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3


class BowVocabDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("n_nodes", C.c_int32),
                ("n_words", C.c_int32), ("parent", c_int32_p), ("is_leaf", c_uint8_p), ("desc", c_uint32_p), ("weight", c_double_p)]


class BowVocabInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("k", "L", "scoring", "weighting", "n_nodes", "n_words", "min_leaf_depth", "max_depth",
                                          "max_sets", "max_features")]


class BowSet(C.Structure):
    _fields_ = [("desc", c_uint32_p), ("n", C.c_int32), ("on_device", C.c_int32), ("levelsup", C.c_int32), ("reserved", C.c_int32)]


class BowResult(C.Structure):
    _fields_ = [("n_words", C.c_int32), ("word", c_int32_p), ("value", c_double_p), ("n_nodes", C.c_int32), ("node", c_int32_p),
                ("node_start", c_int32_p), ("feature", c_int32_p), ("feature_word", c_int32_p), ("feature_nid", c_int32_p)]


class BowVector(C.Structure):
    _fields_ = [("n", C.c_int32), ("word", c_int32_p), ("value", c_double_p)]


@dataclass
class BowTransform:
    """One transform: the BowVector (`word` ascending, `value`), the FeatureVector as node-major CSR (`node` ascending,
    `node_start`, `feature`), and per feature the word id (-1 = stop word) and nid."""
    word: np.ndarray
    value: np.ndarray
    node: np.ndarray
    node_start: np.ndarray
    feature: np.ndarray
    feature_word: np.ndarray
    feature_nid: np.ndarray

    def feature_lists(self):
        """{node id: feature indices}, the shape of DBoW2::FeatureVector."""
        return {int(nd): self.feature[self.node_start[i]:self.node_start[i + 1]] for i, nd in enumerate(self.node)}


def _fn(lib, name, argtypes, restype=C.c_int):
    f = lib.fn(name)
    f.argtypes = argtypes
    f.restype = restype
    return f


def _status(lib, st):
    return f"{lib.fn('status_string')(st).decode()} (status {st})"


def read_text(path, lib=None):
    """lld_bow_vocab_read_text: (status, dict of k, L, scoring, weighting, parent, is_leaf, desc [n][8] u32, weight).  Host only."""
    lib = lib if lib is not None else abi.product()
    f = _fn(lib, "bow_vocab_read_text", [C.c_char_p, C.POINTER(BowVocabDesc)])
    d = BowVocabDesc()
    st = f(str(path).encode(), C.byref(d))
    if st != abi.LLD_OK:
        return st, None
    n = d.n_nodes
    out = dict(k=d.k, L=d.L, scoring=d.scoring, weighting=d.weighting, parent=np.empty(n, np.int32), is_leaf=np.empty(n, np.uint8),
               desc=np.empty((n, 8), np.uint32), weight=np.empty(n, np.float64))
    d.parent = out["parent"].ctypes.data_as(c_int32_p); d.is_leaf = out["is_leaf"].ctypes.data_as(c_uint8_p)
    d.desc = out["desc"].ctypes.data_as(c_uint32_p); d.weight = out["weight"].ctypes.data_as(c_double_p)
    st = f(str(path).encode(), C.byref(d))
    return st, (out if st == abi.LLD_OK else None)


def desc_struct(parent, is_leaf, desc, weight, k, L, scoring=L1_NORM, weighting=TF_IDF, n_words=None):
    """(struct, keep-alive) of an lld_bow_vocab_desc over numpy arrays."""
    keep = dict(parent=np.ascontiguousarray(parent, np.int32), is_leaf=np.ascontiguousarray(is_leaf, np.uint8),
                desc=np.ascontiguousarray(np.asarray(desc).reshape(-1, 8), np.uint32), weight=np.ascontiguousarray(weight, np.float64))
    d = BowVocabDesc(int(k), int(L), int(scoring), int(weighting), len(keep["parent"]),
                     int((keep["is_leaf"] > 0).sum()) if n_words is None else int(n_words),
                     keep["parent"].ctypes.data_as(c_int32_p), keep["is_leaf"].ctypes.data_as(c_uint8_p),
                     keep["desc"].ctypes.data_as(c_uint32_p), keep["weight"].ctypes.data_as(c_double_p))
    return d, keep


class ORBVocabulary:
    """TemplatedVocabulary<FORB::TDescriptor, FORB> uploaded to one context: `transform(desc or list of desc, levelsup=4)`
    returns BowTransform(s), `score(v1, v2)` / `score_many(query, candidates)` the L1 scores."""

    def __init__(self, ctx, parent, is_leaf, desc, weight, k, L, scoring=L1_NORM, weighting=TF_IDF, max_sets=4,
                 max_features=MAX_FEATURES):
        self.ctx = ctx
        self.lib = ctx.lib
        d, keep = desc_struct(parent, is_leaf, desc, weight, k, L, scoring, weighting)
        h = C.c_void_p()
        st = _fn(self.lib, "bow_vocab_create", [C.c_void_p, C.POINTER(BowVocabDesc), C.c_int, C.c_int, C.POINTER(C.c_void_p)])(
            ctx.handle, C.byref(d), int(max_sets), int(max_features), C.byref(h))
        if st != abi.LLD_OK:
            raise ValueError(f"lld_bow_vocab_create failed: {_status(self.lib, st)}")
        self.handle = h
        info = BowVocabInfo()
        _fn(self.lib, "bow_vocab_info_get", [C.c_void_p, C.POINTER(BowVocabInfo)])(h, C.byref(info))
        self.info = {f: getattr(info, f) for f, _ in BowVocabInfo._fields_}
        self.L, self.n_words, self.max_sets, self.max_features = info.L, info.n_words, info.max_sets, info.max_features
        self._transform = _fn(self.lib, "bow_transform", [C.c_void_p, C.c_int, C.POINTER(BowSet), C.POINTER(BowResult)])
        self._score = _fn(self.lib, "bow_score", [C.c_void_p, C.POINTER(BowVector), C.c_int, c_int32_p, c_int32_p, c_double_p,
                                                  c_double_p])

    @classmethod
    def from_arrays(cls, ctx, parent, is_leaf, desc, weight, k, L, scoring=L1_NORM, weighting=TF_IDF, **kw):
        return cls(ctx, parent, is_leaf, desc, weight, k, L, scoring, weighting, **kw)

    @classmethod
    def from_text_file(cls, ctx, path, **kw):
        """loadFromTextFile: raises ValueError where the reference returns false (or where its behaviour is undefined)."""
        st, d = read_text(path, ctx.lib)
        if st != abi.LLD_OK:
            raise ValueError(f"lld_bow_vocab_read_text({path}) failed: {_status(ctx.lib, st)}")
        return cls(ctx, d["parent"], d["is_leaf"], d["desc"], d["weight"], d["k"], d["L"], d["scoring"], d["weighting"], **kw)

    def transform_raw(self, sets, levelsup=4):
        """sets: list of [n][8] u32 host arrays or (device pointer, n) tuples.  Returns (status, list of BowTransform)."""
        ns = len(sets)
        S = (BowSet * max(ns, 1))()
        R = (BowResult * max(ns, 1))()
        keep, res = [], []
        for i, s in enumerate(sets):
            if isinstance(s, tuple):
                ptr, n = s
                S[i] = BowSet(C.cast(C.c_void_p(ptr), c_uint32_p), int(n), 1, int(levelsup), 0)
            else:
                a = np.ascontiguousarray(np.asarray(s, np.uint32).reshape(-1, 8))
                keep.append(a)
                n = len(a)
                S[i] = BowSet(a.ctypes.data_as(c_uint32_p), n, 0, int(levelsup), 0)
            m = max(n, 1)
            r = BowTransform(np.empty(m, np.int32), np.empty(m, np.float64), np.empty(m, np.int32), np.empty(m + 1, np.int32),
                             np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.int32))
            R[i] = BowResult(0, r.word.ctypes.data_as(c_int32_p), r.value.ctypes.data_as(c_double_p), 0, r.node.ctypes.data_as(c_int32_p),
                             r.node_start.ctypes.data_as(c_int32_p), r.feature.ctypes.data_as(c_int32_p),
                             r.feature_word.ctypes.data_as(c_int32_p), r.feature_nid.ctypes.data_as(c_int32_p))
            res.append((r, n))
        st = self._transform(self.handle, ns, S, R)
        out = []
        for i, (r, n) in enumerate(res):
            if st == abi.LLD_OK:
                nw, nn = R[i].n_words, R[i].n_nodes
                nv = int(r.node_start[nn])
                out.append(BowTransform(r.word[:nw], r.value[:nw], r.node[:nn], r.node_start[:nn + 1], r.feature[:nv], r.feature_word[:n],
                                        r.feature_nid[:n]))
        return st, out

    def transform(self, desc, levelsup=4):
        """TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) on one descriptor set ([n][8] u32, or a
        (device pointer, n) tuple) or a list of them (one sequence of launches)."""
        single = not isinstance(desc, list)
        st, out = self.transform_raw([desc] if single else desc, levelsup)
        if st != abi.LLD_OK:
            raise ValueError(f"lld_bow_transform failed: {_status(self.lib, st)}")
        return out[0] if single else out

    def score_many(self, query, candidates):
        """L1Scoring::score(query, c) for every candidate; query and candidates are BowTransforms or (word, value) pairs."""
        qw, qv = _wv(query)
        cw = [_wv(c) for c in candidates]
        start = np.zeros(len(cw) + 1, np.int32)
        start[1:] = np.cumsum([len(w) for w, _ in cw])
        words = np.concatenate([w for w, _ in cw] + [np.empty(0, np.int32)]).astype(np.int32)
        values = np.concatenate([v for _, v in cw] + [np.empty(0, np.float64)]).astype(np.float64)
        out = np.empty(len(cw), np.float64)
        st = self.score_raw(qw, qv, start, words, values, out)
        if st != abi.LLD_OK:
            raise ValueError(f"lld_bow_score failed: {_status(self.lib, st)}")
        return out

    def score_raw(self, qw, qv, start, words, values, out):
        qw = np.ascontiguousarray(qw, np.int32); qv = np.ascontiguousarray(qv, np.float64)
        start = np.ascontiguousarray(start, np.int32); words = np.ascontiguousarray(words, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        q = BowVector(len(qw), qw.ctypes.data_as(c_int32_p), qv.ctypes.data_as(c_double_p))
        return self._score(self.handle, C.byref(q), len(start) - 1, start.ctypes.data_as(c_int32_p), words.ctypes.data_as(c_int32_p),
                           values.ctypes.data_as(c_double_p), out.ctypes.data_as(c_double_p))

    def score(self, v1, v2):
        return float(self.score_many(v1, [v2])[0])

    def close(self):
        if getattr(self, "handle", None):
            _fn(self.lib, "bow_vocab_destroy", [C.c_void_p], None)(self.handle)
            self.handle = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()
    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _wv(v):
    if isinstance(v, BowTransform):
        return v.word, v.value
    w, val = v
    return np.asarray(w, np.int32), np.asarray(val, np.float64)


def common_nodes(fv1: BowTransform, fv2: BowTransform):
    """The nodes both FeatureVectors hold, ascending, as the CSR dict orb_search.search_by_bow_frame / _kf /
    search_for_triangulation take: n_nodes, start1, idx1, start2, idx2 (the node merge of ORBmatcher::SearchByBoW)."""
    common, i1, i2 = np.intersect1d(fv1.node, fv2.node, assume_unique=True, return_indices=True)
    start1, idx1, start2, idx2 = [0], [], [0], []
    for a, b in zip(i1, i2):
        idx1.extend(fv1.feature[fv1.node_start[a]:fv1.node_start[a + 1]].tolist()); start1.append(len(idx1))
        idx2.extend(fv2.feature[fv2.node_start[b]:fv2.node_start[b + 1]].tolist()); start2.append(len(idx2))
    return dict(n_nodes=len(common), start1=np.array(start1, np.int32), idx1=np.array(idx1, np.int32), start2=np.array(start2, np.int32),
                idx2=np.array(idx2, np.int32))


def extractor_descriptors(ex, image_index=0):
    """(device pointer, n) of the rBRIEF descriptors of image `image_index` of ex's last call (lld_orb_extractor_descriptors)."""
    p = c_uint32_p(); n = C.c_int32()
    st = _fn(ex.lib, "orb_extractor_descriptors", [C.c_void_p, C.c_int, C.POINTER(c_uint32_p), C.POINTER(C.c_int32)])(
        ex.handle, int(image_index), C.byref(p), C.byref(n))
    if st != abi.LLD_OK:
        raise ValueError(f"lld_orb_extractor_descriptors failed (status {st})")
    return C.cast(p, C.c_void_p).value or 0, int(n.value)
