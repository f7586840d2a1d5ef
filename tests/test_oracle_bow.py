"""DBoW2 vocabulary without a GPU: known answers of the numpy restatement (tests/bow_ref.py) on a hand-built 3-ary tree, the
library's text reader (lld_bow_vocab_read_text, host only) against the numpy parser, and the struct layouts of the lld_bow_* ABI."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import bow_ref as B
from bow_ref import W_OTHER, W_REPEAT, hand_queries, hand_tree
from lld_slam_amd import abi, vocabulary as voc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_hand_tree_known_answers():
    V = hand_tree()
    T = B.Tree(V)
    q = hand_queries()
    leaf, wid, w, nid = B.descend(T, q, 4)
    # the tie at level 1 goes to A; under A, bits 10/11/12 are each 1 away, node 4 (first) wins
    assert leaf[0] == 4 and nid[0] == 4
    np.testing.assert_array_equal(leaf[1:8], 4)
    assert leaf[8] == 5 and leaf[9] == 6 and leaf[10] == 3
    # word ids are the leaf lines in file order: 3 -> 0, 4 -> 1, ... 9 -> 6
    np.testing.assert_array_equal(B.word_ids(V)[3:], np.arange(7))
    # C is a leaf at depth 1, above nid level 2: it stands for itself (the documented deviation)
    assert nid[10] == 3
    r = B.transform(T, q, 4)
    # node 6 has weight 0: the stop word is in neither vector
    assert 3 not in r["word"] and 6 not in r["node"] and 9 not in r["feature"] and r["feature_word"][9] == -1
    np.testing.assert_array_equal(r["word"], [0, 1, 2])
    np.testing.assert_array_equal(r["node"], [3, 4, 5])
    np.testing.assert_array_equal(r["node_start"], [0, 1, 9, 10])
    np.testing.assert_array_equal(r["feature"], [10, 0, 1, 2, 3, 4, 5, 6, 7, 8])
    # eight hits of word 1 (the tie + seven): repeated addition, then the sequential L1 norm
    s = W_REPEAT
    for _ in range(7):
        s = s + W_REPEAT
    norm = 0.0
    for v in (2.0, s, W_OTHER):
        norm += v
    exp = [2.0 / norm, s / norm, W_OTHER / norm]
    assert [struct.pack("<d", x) for x in r["value"]] == [struct.pack("<d", x) for x in exp]
    # ... which is not count*w
    s7 = W_REPEAT
    for _ in range(6):
        s7 = s7 + W_REPEAT
    assert s7 != 7 * W_REPEAT
    assert s7 / (s7 + W_OTHER) != 7 * W_REPEAT / (7 * W_REPEAT + W_OTHER) or W_OTHER / (s7 + W_OTHER) != W_OTHER / (7 * W_REPEAT + W_OTHER)


def test_hand_tree_idf_keeps_the_first_weight():
    V = dict(hand_tree(), weighting=2)
    r = B.transform(B.Tree(V), hand_queries(), 4)
    norm = 0.0
    for v in (2.0, W_REPEAT, W_OTHER):
        norm += v
    np.testing.assert_array_equal(r["value"], [2.0 / norm, W_REPEAT / norm, W_OTHER / norm])


def test_levelsup_moves_nid():
    V = hand_tree()
    T = B.Tree(V)
    q = hand_queries()
    for levelsup, exp in ((5, 1), (6, 0), (9, 0), (4, 4), (0, 4), (-3, 4)):   # nid level 1, 0, <0, 2, 6 (> depth), 9
        _, _, _, nid = B.descend(T, q[:1], levelsup)
        assert nid[0] == exp, (levelsup, nid[0])


def test_score_known_answers():
    a = (np.array([1, 4, 9]), np.array([0.5, 0.25, 0.25]))
    b = (np.array([2, 4, 9, 11]), np.array([0.4, 0.1, 0.3, 0.2]))
    s = 0.0
    for vi, wi in ((0.25, 0.1), (0.25, 0.3)):
        s += abs(vi - wi) - abs(vi) - abs(wi)
    assert B.score(a, b) == -s / 2.0
    assert B.score(a, a) == 1.0
    d = B.score(a, (np.array([2, 3]), np.array([0.5, 0.5])))
    assert struct.pack("<d", d) == struct.pack("<d", -0.0)          # no common word: -0.0, bit for bit


def test_generator_properties():
    V = B.make_vocab(5, k=6, L=6, p_full=0.3, p_early_leaf=0.15, p_stop=0.05, order="dfs")
    ch = B.children(V)
    nch = np.array([len(c) for c in ch])
    assert nch.max() <= 6 and nch[nch > 0].min() >= 2
    depth = np.zeros(len(ch), np.int64)
    for i in range(1, len(ch)):
        assert V["parent"][i] < i
        depth[i] = depth[V["parent"][i]] + 1
    leaf_depths = set(depth[V["is_leaf"] > 0].tolist())
    assert min(leaf_depths) <= V["L"] - 4 and len(leaf_depths) >= 3
    assert (V["weight"][V["is_leaf"] > 0] == 0).any()                  # stop words
    assert not all(np.all(np.diff(c) == 1) for c in ch if len(c) > 1)   # preorder: siblings are not all adjacent lines
    q, src = B.near_leaves(V, 6, 2000)
    leaf, _, _, _ = B.descend(B.Tree(V), q, 4)
    assert (leaf == src).mean() > 0.99                                 # hierarchical: near a leaf means reaching it


def _lib_read(path):
    return voc.read_text(path, abi.product())


@pytest.mark.parametrize("trailing,blank", [(True, 0), (False, 0), (True, 7)])
def test_reader_matches_numpy_parser(tmp_path, trailing, blank):
    V = B.make_vocab(11, k=5, L=4, p_full=0.5, p_early_leaf=0.2, p_stop=0.1, order="dfs", weighting=1)
    p = tmp_path / "voc.txt"
    B.write_text(V, p, trailing_newline=trailing, blank_every=blank)
    exp = B.read_text(p)
    st, got = _lib_read(p)
    assert st == abi.LLD_OK
    for k in ("k", "L", "scoring", "weighting"):
        assert got[k] == exp[k] == V[k]
    for k in ("parent", "is_leaf", "desc", "weight"):
        np.testing.assert_array_equal(got[k], exp[k])
        np.testing.assert_array_equal(got[k], V[k])
    assert got["weight"].view(np.uint64).tolist() == V["weight"].view(np.uint64).tolist()


def test_reader_byte_values_and_spacing(tmp_path):
    """Bytes are (unsigned char) of the decimal int; any whitespace separates fields; CRLF is whitespace."""
    p = tmp_path / "v.txt"
    row = ["0", "1"] + [str(x) for x in [256 + 7, -1] + list(range(30))] + ["1.25"]
    p.write_text("2 1 0 0\r\n" + "\t".join(row) + "\r\n\n  \n" + " ".join(row[:1] + ["1"] + row[2:]) + "\n")
    exp = B.read_text(p)
    st, got = _lib_read(p)
    assert st == abi.LLD_OK and len(got["parent"]) == len(exp["parent"]) == 3
    np.testing.assert_array_equal(got["desc"], exp["desc"])
    assert got["desc"][1].view(np.uint8)[0] == 7 and got["desc"][1].view(np.uint8)[1] == 255


@pytest.mark.parametrize("header", ["21 6 0 0", "-1 6 0 0", "10 0 0 0", "10 11 0 0", "10 6 6 0", "10 6 -1 0", "10 6 0 4", "10 6 0",
                                    "ten 6 0 0", ""])
def test_reader_refuses_what_the_reference_refuses(tmp_path, header):
    p = tmp_path / "v.txt"
    p.write_text(header + "\n0 1 " + " ".join(["0"] * 32) + " 1.0\n")
    with pytest.raises(B.Refused):
        B.read_text(p)
    st, _ = _lib_read(p)
    assert st == abi.LLD_ERR_INVALID


@pytest.mark.parametrize("line", ["1 1 " + " ".join(["0"] * 32) + " 1.0",          # parent is not an earlier node
                                  "0 1 " + " ".join(["0"] * 31) + " 1.0",          # short line
                                  "0 1 " + " ".join(["x"] * 32) + " 1.0"])         # not an int
def test_reader_refuses_malformed_nodes(tmp_path, line):
    p = tmp_path / "v.txt"
    p.write_text("10 6 0 0\n" + line + "\n")
    with pytest.raises(B.Refused):
        B.read_text(p)
    assert _lib_read(p)[0] == abi.LLD_ERR_INVALID


def test_reader_missing_file_and_second_call_mismatch(tmp_path):
    assert _lib_read(tmp_path / "none.txt")[0] == abi.LLD_ERR_INVALID
    V = B.make_vocab(3, k=3, L=2)
    p = tmp_path / "v.txt"
    B.write_text(V, p)
    d = voc.BowVocabDesc()
    f = abi.product().fn("bow_vocab_read_text")
    f.argtypes = [ctypes.c_char_p, ctypes.POINTER(voc.BowVocabDesc)]
    assert f(str(p).encode(), ctypes.byref(d)) == abi.LLD_OK and d.n_nodes == len(V["parent"])
    small = len(V["parent"]) - 1                               # arrays one node too short: refused, not overrun
    arr = [np.zeros(small, np.int32), np.zeros(small, np.uint8), np.zeros((small, 8), np.uint32), np.zeros(small)]
    d.n_nodes = small
    d.parent = arr[0].ctypes.data_as(abi.c_int32_p); d.is_leaf = arr[1].ctypes.data_as(abi.c_uint8_p)
    d.desc = arr[2].ctypes.data_as(abi.c_uint32_p); d.weight = arr[3].ctypes.data_as(abi.c_double_p)
    assert f(str(p).encode(), ctypes.byref(d)) == abi.LLD_ERR_INVALID


def test_bow_struct_layouts_match_the_header(tmp_path):
    names = [("lld_bow_vocab_desc", voc.BowVocabDesc), ("lld_bow_vocab_info", voc.BowVocabInfo), ("lld_bow_set", voc.BowSet),
             ("lld_bow_result", voc.BowResult), ("lld_bow_vector", voc.BowVector)]
    probes = [("lld_bow_vocab_desc", voc.BowVocabDesc, f) for f in ("n_words", "parent", "is_leaf", "desc", "weight")] + \
             [("lld_bow_vocab_info", voc.BowVocabInfo, f) for f in ("min_leaf_depth", "max_features")] + \
             [("lld_bow_set", voc.BowSet, f) for f in ("n", "on_device", "levelsup")] + \
             [("lld_bow_result", voc.BowResult, f) for f in ("word", "value", "n_nodes", "node", "node_start", "feature",
                                                             "feature_word", "feature_nid")] + \
             [("lld_bow_vector", voc.BowVector, f) for f in ("word", "value")]
    body = "".join(f'printf("%zu\\n", sizeof({n}));' for n, _ in names)
    body += "".join(f'printf("%zu\\n", offsetof({n}, {f}));' for n, _, f in probes)
    body += 'printf("%d\\n", LLD_BOW_MAX_FEATURES);'
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/lld_amd.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(c) for _, c in names] + [getattr(c, f).offset for _, c, f in probes] + [voc.MAX_FEATURES]
