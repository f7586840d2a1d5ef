"""The C++ route to the vocabulary: examples/bow_harness (lld_amd::ORBVocabulary of include/lld_amd.hpp) loads a text vocabulary,
transforms two descriptor sets into std::map BowVector / FeatureVector and scores them; everything must equal tests/bow_ref.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bow_ref as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "bow_harness")


def read_vectors(f):
    n = struct.unpack("<i", f.read(4))[0]
    words, values = [], []
    for _ in range(n):
        w, v = struct.unpack("<id", f.read(12))
        words.append(w); values.append(v)
    n = struct.unpack("<i", f.read(4))[0]
    nodes, start, feat = [], [0], []
    for _ in range(n):
        nd, c = struct.unpack("<ii", f.read(8))
        nodes.append(nd); feat.extend(struct.unpack(f"<{c}i", f.read(4 * c))); start.append(len(feat))
    return dict(word=np.array(words, np.int32), value=np.array(values, np.float64), node=np.array(nodes, np.int32),
                node_start=np.array(start, np.int32), feature=np.array(feat, np.int32))


@pytest.mark.parametrize("levelsup", [4, 2])
def test_bow_harness_matches_the_restatement(tmp_path, levelsup):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "bow_harness"], check=True, capture_output=True)
    V = B.make_vocab(31, k=8, L=5, p_full=0.4, p_early_leaf=0.1, p_stop=0.05, order="dfs")
    B.write_text(V, tmp_path / "voc.txt")
    d1 = B.random_desc(1, 1800)
    d2 = np.where(np.random.default_rng(2).random((1800, 1)) < 0.5, d1, B.random_desc(3, 1800)).astype(np.uint32)
    with open(tmp_path / "in.bin", "wb") as f:
        for a in (np.array([levelsup], np.int32), np.array([len(d1)], np.int32), d1, np.array([len(d2)], np.int32), d2):
            a.astype(a.dtype.newbyteorder("<")).tofile(f)
    r = subprocess.run([HARNESS, str(tmp_path / "voc.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    T = B.Tree(B.read_text(tmp_path / "voc.txt"))
    exp = [B.transform(T, d, levelsup) for d in (d1, d2)]
    with open(tmp_path / "out.bin", "rb") as f:
        got = [read_vectors(f), read_vectors(f)]
        s = struct.unpack("<d", f.read(8))[0]
    for g, e in zip(got, exp):
        for k in ("word", "node", "node_start", "feature"):
            np.testing.assert_array_equal(g[k], e[k])
        assert np.array_equal(g["value"].view(np.uint64), e["value"].view(np.uint64))
    es = B.score((exp[0]["word"], exp[0]["value"]), (exp[1]["word"], exp[1]["value"]))
    assert struct.pack("<d", s) == struct.pack("<d", es) and 0.0 < es < 1.0


def test_bow_harness_refuses_a_bad_header(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "bow_harness"], check=True, capture_output=True)
    (tmp_path / "voc.txt").write_text("10 11 0 0\n0 1 " + " ".join(["0"] * 32) + " 1.0\n")
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([4, 0, 0], np.int32).tofile(f)
    r = subprocess.run([HARNESS, str(tmp_path / "voc.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 3 and "loadFromTextFile failed" in r.stderr
