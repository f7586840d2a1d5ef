"""The C++ route to the keyframe database: examples/kfdb_harness (lld_amd::KeyFrameDatabase of include/lld_amd.hpp) runs one
scripted sequence of add / erase / clear / covisibility updates and both queries; every query must equal tests/kfdb_ref.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bow_ref as B
import kfdb_ref as K
import kfdb_scenes as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "kfdb_harness")


def bow_bytes(v):
    return struct.pack("<i", len(v[0])) + b"".join(struct.pack("<id", int(w), float(x)) for w, x in zip(v[0], v[1]))


def script(ops):
    out = b""
    for op in ops:
        k = op[0]
        if k == "add":
            out += struct.pack("<iQ", 1, op[1]) + bow_bytes(op[2])
        elif k == "erase":
            out += struct.pack("<iQ", 2, op[1])
        elif k == "clear":
            out += struct.pack("<i", 3)
        elif k == "cov":
            out += struct.pack("<iQi", 4, op[1], len(op[2])) + b"".join(struct.pack("<Q", n) for n in op[2])
        elif k == "reloc":
            out += struct.pack("<iQ", 5, op[1]) + bow_bytes(op[2])
        elif k == "loop":
            out += struct.pack("<iQ", 6, op[1]) + bow_bytes(op[2]) + struct.pack("<i", len(op[3])) + \
                b"".join(struct.pack("<Q", c) for c in op[3]) + struct.pack("<f", op[4])
    return out + struct.pack("<i", 0)


def test_kfdb_harness_matches_the_restatement(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "kfdb_harness"], check=True, capture_output=True)
    V = B.make_vocab(33, k=8, L=4, p_full=1.0)
    B.write_text(V, tmp_path / "voc.txt")
    n_words = int(V["is_leaf"].sum())
    ids, _, vecs = K.trajectory(7, 120, n_words, words_per_kf=50)
    cov = K.covisibility(ids, vecs)
    rng = np.random.default_rng(8)
    ops = []
    for name in ("stale_reloc_score", "erase_then_readd"):
        ops += K.SCENARIOS[name][0] + [("clear",)]
    for i, (kid, v) in enumerate(zip(ids, vecs)):
        kid += 100
        ops.append(("add", kid, v))
        ops.append(("cov", kid, [n + 100 for n in cov[kid - 100] if n + 100 < kid]))
        if i % 17 == 16:
            ops.append(("erase", kid - 5))
        if i % 4 == 3:
            j = int(rng.integers(0, i + 1))
            ops.append(("reloc", 5000 + i, vecs[j]))
            ops.append(("loop", ids[j] + 100, vecs[j], [n + 100 for n in cov[ids[j]][:3]], 0.02))
    exp = K.run_ops(K.KeyFrameDatabase(n_words), ops)
    run_and_compare(tmp_path, ops, exp)
    assert len(exp) > 50


def run_and_compare(tmp_path, ops, exp, *limits):
    """Runs the harness on the script of ops (vocabulary in tmp_path/voc.txt); every query must equal exp's (ids, accs, stats)."""
    (tmp_path / "script.bin").write_bytes(script(ops))
    r = subprocess.run([HARNESS, str(tmp_path / "voc.txt"), str(tmp_path / "script.bin"), str(tmp_path / "out.bin"), *map(str, limits)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    data = (tmp_path / "out.bin").read_bytes()
    pos = 0
    for q, (eids, eacc, stats) in enumerate(exp):
        n = struct.unpack_from("<i", data, pos)[0]; pos += 4
        got_ids = list(struct.unpack_from(f"<{n}Q", data, pos)); pos += 8 * n
        got_acc = np.frombuffer(data, np.float32, n, pos); pos += 4 * n
        s = struct.unpack_from("<4i", data, pos); pos += 16
        assert got_ids == eids, q
        assert np.array_equal(got_acc.view(np.uint32), np.asarray(eacc, np.float32).view(np.uint32)), q
        assert s == (stats["n_sharing"], stats["max_common_words"], stats["min_common_words"], stats["n_scored"]), q
    assert pos == len(data)


@pytest.mark.parametrize("name", ["groups", "all_retained[1025]"])
def test_kfdb_harness_on_a_scene(tmp_path, name):
    """Scenes of tests/kfdb_scenes.py through the C++ wrapper, which sizes its own result buffers: 2200 entries de-duplicated to 200,
    and 1025 candidates, one more than a pass of the finish kernel."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "kfdb_harness"], check=True, capture_output=True)
    sc = S.scene(name)
    V = B.make_vocab(41, k=10, L=4, p_full=1.0)
    assert int(V["is_leaf"].sum()) == sc.n_words
    B.write_text(V, tmp_path / "voc.txt")
    run_and_compare(tmp_path, sc.ops, [(a.ids, a.acc, a.stats) for a in S.reference(name)], sc.max_keyframes, sc.max_words)
