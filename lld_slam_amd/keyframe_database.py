"""ORB-SLAM2's KeyFrameDatabase on the device (lld_kfdb_*): the keyframes' BowVectors, the inverted file, the covisibility lists
and the per-keyframe query registers stay in HBM; a query uploads the query vector and downloads the candidate ids.  The rules are
those of include/lld_amd.h."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import c_double_p, c_float_p, c_int32_p
from .vocabulary import BowTransform, BowVector

MAX_KEYFRAMES = 8192         # LLD_KFDB_MAX_KEYFRAMES
MAX_COVISIBLES = 10          # LLD_KFDB_MAX_COVISIBLES
c_uint64_p = C.POINTER(C.c_uint64)


class KfdbResult(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("n_candidates", C.c_int32), ("kf_id", c_uint64_p), ("acc_score", c_float_p),
                ("n_sharing", C.c_int32), ("max_common_words", C.c_int32), ("min_common_words", C.c_int32), ("n_scored", C.c_int32)]


@dataclass
class Candidates:
    """The candidate ids in the reference's return order, the accScore of the entry that produced each, and the counters of the
    query: lKFsSharingWords.size(), maxCommonWords, minCommonWords, nscores."""
    kf_id: np.ndarray
    acc_score: np.ndarray
    n_sharing: int
    max_common_words: int
    min_common_words: int
    n_scored: int


def _fn(lib, name, argtypes, restype=C.c_int):
    f = lib.fn(name)
    f.argtypes = argtypes
    f.restype = restype
    return f


def _wv(v):
    if isinstance(v, BowTransform):
        return np.ascontiguousarray(v.word, np.int32), np.ascontiguousarray(v.value, np.float64)
    w, val = v
    return np.ascontiguousarray(w, np.int32), np.ascontiguousarray(val, np.float64)


def _vec(v):
    w, val = _wv(v)
    return BowVector(len(w), w.ctypes.data_as(c_int32_p), val.ctypes.data_as(c_double_p)), (w, val)


def _ids(ids):
    return np.ascontiguousarray(np.asarray(ids, np.uint64).reshape(-1))


class KeyFrameDatabase:
    """KeyFrameDatabase(voc) on the vocabulary's context: add / erase / clear, set_covisibles (UpdateBestCovisibles), and the two
    queries.  BowVectors are (words, values) pairs or BowTransforms.  Methods raise ValueError where the library refuses; the
    *_raw methods return the status instead."""

    def __init__(self, vocabulary, max_keyframes=4096, max_words=8 << 20):
        self.voc = vocabulary
        self.lib = vocabulary.lib
        lib = self.lib
        h = C.c_void_p()
        st = _fn(lib, "kfdb_create", [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)])(vocabulary.handle, int(max_keyframes),
                                                                                                 int(max_words), C.byref(h))
        if st != abi.LLD_OK:
            raise ValueError(f"lld_kfdb_create failed (status {st})")
        self.handle = h
        self.max_keyframes = int(max_keyframes)
        self._add = _fn(lib, "kfdb_add", [C.c_void_p, C.c_int32, c_uint64_p, C.POINTER(BowVector)])
        self._erase = _fn(lib, "kfdb_erase", [C.c_void_p, C.c_int32, c_uint64_p])
        self._clear = _fn(lib, "kfdb_clear", [C.c_void_p])
        self._cov = _fn(lib, "kfdb_set_covisibles", [C.c_void_p, C.c_int32, c_uint64_p, c_int32_p, c_uint64_p])
        self._loop = _fn(lib, "kfdb_detect_loop_candidates", [C.c_void_p, C.c_uint64, C.POINTER(BowVector), C.c_int32, c_uint64_p,
                                                              C.c_float, C.POINTER(KfdbResult)])
        self._reloc = _fn(lib, "kfdb_detect_relocalization_candidates", [C.c_void_p, C.c_uint64, C.POINTER(BowVector),
                                                                         C.POINTER(KfdbResult)])

    @staticmethod
    def _check(st, what):
        if st != abi.LLD_OK:
            raise ValueError(f"lld_kfdb_{what} failed (status {st})")

    # ---------------------------------------------------------------------------------------------------------- mutations
    def add_raw(self, ids, vecs):
        ids = _ids(ids)
        vecs = list(vecs)
        V = (BowVector * max(1, len(vecs)))()
        keep = []
        for i, v in enumerate(vecs):
            V[i], k = _vec(v)
            keep.append(k)
        return self._add(self.handle, len(ids), ids.ctypes.data_as(c_uint64_p), V)

    def add(self, kf_id, vec=None):
        """add(id, bow) for one keyframe, or add(ids, bows) for several in order."""
        if vec is None or np.ndim(kf_id) == 0:
            ids, vecs = [kf_id], [vec]
        else:
            ids, vecs = kf_id, vec
        self._check(self.add_raw(ids, vecs), "add")

    def erase_raw(self, ids):
        ids = _ids(ids)
        return self._erase(self.handle, len(ids), ids.ctypes.data_as(c_uint64_p))

    def erase(self, ids):
        self._check(self.erase_raw([ids] if np.ndim(ids) == 0 else ids), "erase")

    def clear(self):
        self._check(self._clear(self.handle), "clear")

    def set_covisibles_raw(self, kf_ids, neighbours):
        kf_ids = _ids(kf_ids)
        lists = [_ids(n) for n in neighbours]
        start = np.zeros(len(lists) + 1, np.int32)
        start[1:] = np.cumsum([len(n) for n in lists])
        nb = np.ascontiguousarray(np.concatenate(lists + [np.empty(0, np.uint64)]).astype(np.uint64))
        return self._cov(self.handle, len(kf_ids), kf_ids.ctypes.data_as(c_uint64_p), start.ctypes.data_as(c_int32_p),
                         nb.ctypes.data_as(c_uint64_p))

    def set_covisibles(self, kf_id, neighbours=None):
        """set_covisibles(id, ordered covisibles) or set_covisibles({id: ordered covisibles})."""
        if neighbours is None:
            items = list(kf_id.items())
            self._check(self.set_covisibles_raw([k for k, _ in items], [v for _, v in items]), "set_covisibles")
        else:
            self._check(self.set_covisibles_raw([kf_id], [neighbours]), "set_covisibles")

    # ---------------------------------------------------------------------------------------------------------- queries
    def _result(self, capacity):
        cap = int(capacity)
        ids = np.zeros(max(cap, 1), np.uint64)
        acc = np.zeros(max(cap, 1), np.float32)
        R = KfdbResult(cap, 0, ids.ctypes.data_as(c_uint64_p), acc.ctypes.data_as(c_float_p), 0, 0, 0, 0)
        return R, ids, acc

    @staticmethod
    def _out(R, ids, acc):
        n = min(R.n_candidates, R.capacity)
        return Candidates(ids[:n].copy(), acc[:n].copy(), R.n_sharing, R.max_common_words, R.min_common_words, R.n_scored), \
            R.n_candidates

    def detect_loop_candidates_raw(self, query_id, bow, connected, min_score, capacity=None):
        """(status, Candidates, full count)."""
        q, keep = _vec(bow)
        conn = _ids(list(connected))
        R, ids, acc = self._result(self.max_keyframes if capacity is None else capacity)
        st = self._loop(self.handle, int(query_id), C.byref(q), len(conn), conn.ctypes.data_as(c_uint64_p), float(min_score), C.byref(R))
        return (st,) + self._out(R, ids, acc)

    def detect_loop_candidates(self, query_id, bow, connected, min_score):
        """DetectLoopCandidates(pKF, minScore): pKF's mnId, mBowVec and GetConnectedKeyFrames()."""
        st, out, _ = self.detect_loop_candidates_raw(query_id, bow, connected, min_score)
        self._check(st, "detect_loop_candidates")
        return out

    def detect_relocalization_candidates_raw(self, query_id, bow, capacity=None):
        q, keep = _vec(bow)
        R, ids, acc = self._result(self.max_keyframes if capacity is None else capacity)
        st = self._reloc(self.handle, int(query_id), C.byref(q), C.byref(R))
        return (st,) + self._out(R, ids, acc)

    def detect_relocalization_candidates(self, query_id, bow):
        """DetectRelocalizationCandidates(F): the frame's mnId and mBowVec."""
        st, out, _ = self.detect_relocalization_candidates_raw(query_id, bow)
        self._check(st, "detect_relocalization_candidates")
        return out

    def close(self):
        if getattr(self, "handle", None):
            _fn(self.lib, "kfdb_destroy", [C.c_void_p], None)(self.handle)
            self.handle = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()
    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
