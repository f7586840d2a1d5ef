"""The C++ route to the PnPsolver: examples/pnp_harness runs Tracking::Relocalization's iterate(5) rounds through the object adapter
(adapters/lld_pnp_adapter.cc, PnPsolver(F, vpMapPointMatches) on Frame / MapPoint test doubles with NULL matches and isBad()
points), then lld_amd::PnPsolver's iterate + find on candidate 0.  Every call must equal tests/pnp_ref.py on the same gather."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pnp_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "pnp_harness")
LEVEL_SIGMA2 = np.array([np.float32(np.float32(1.44) ** np.float32(l)) for l in range(8)], np.float32)


def make_relocalisation(seed, n_kp=400, n_cand=6):
    base = P.make_scene(seed, n_kp, 0.8, n_keypoints=n_kp)
    octave = np.array([int(np.argmin(np.abs(LEVEL_SIGMA2 - s))) for s in base["sigma2"]], np.int32)
    uv = np.empty((n_kp, 2), np.float32)
    uv[base["kp_index"]] = base["uv"]
    oc = np.empty(n_kp, np.int32)
    oc[base["kp_index"]] = octave
    xyz_true = np.empty((n_kp, 3), np.float32)
    xyz_true[base["kp_index"]] = base["xyz"]
    rng = np.random.default_rng(seed + 1)
    cands = []
    for c in range(n_cand):
        state = rng.choice([0, 1, 1, 1, 2], n_kp).astype(np.int32)          # NULL, good, isBad
        xyz = xyz_true.copy()
        wrong = rng.random(n_kp) < [0.1, 0.4, 0.7, 0.2, 0.9, 0.5][c % 6]
        xyz[wrong] = rng.uniform(-20, 20, (int(wrong.sum()), 3)).astype(np.float32)
        cands.append(dict(state=state, xyz=xyz, seed=int(rng.integers(0, 1 << 32))))
    return dict(uv=uv, octave=oc, cands=cands, fx=base["fx"], fy=base["fy"], cx=base["cx"], cy=base["cy"], n_kp=n_kp)


def scene_bytes(sc, max_rounds, n_it):
    out = struct.pack("<5i", len(sc["cands"]), sc["n_kp"], 8, max_rounds, n_it)
    out += struct.pack("<4f", sc["fx"], sc["fy"], sc["cx"], sc["cy"]) + LEVEL_SIGMA2.tobytes()
    for i in range(sc["n_kp"]):
        out += struct.pack("<2fi", float(sc["uv"][i, 0]), float(sc["uv"][i, 1]), int(sc["octave"][i]))
    for c in sc["cands"]:
        out += struct.pack("<I", c["seed"])
        for i in range(sc["n_kp"]):
            out += struct.pack("<i", int(c["state"][i]))
            if c["state"][i]:
                out += c["xyz"][i].astype(np.float32).tobytes()
    return out


def ref_solver(sc, c):
    cd = sc["cands"][c]
    keep = np.flatnonzero(cd["state"] == 1)                                  # NULL and isBad() skipped (PnPsolver.cc:83-86)
    return P.PnPsolverRef(cd["xyz"][keep], sc["uv"][keep], LEVEL_SIGMA2[sc["octave"][keep]], keep, sc["n_kp"], sc["fx"], sc["fy"],
                          sc["cx"], sc["cy"], cd["seed"])


def parse(line):
    f = line.split()
    tag, rnd, cand, has, no_more, n_in = f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5])
    T = np.array([int(x, 16) for x in f[7:19]], np.uint32).view(np.float32).reshape(3, 4)
    inl = [int(x) for x in f[19:]]
    return tag, rnd, cand, has, no_more, n_in, T, inl


def check(line, o, what):
    tag, rnd, cand, has, no_more, n_in, T, inl = parse(line)
    assert has == (o["Tcw"] is not None), what
    assert n_in == o["n_inliers"], what
    if tag != "F":
        assert no_more == int(o["no_more"]), what
    if has:
        assert np.array_equal(T.view(np.uint32), o["Tcw"].view(np.uint32)), what
        assert inl == list(np.flatnonzero(o["inliers"])), what
    else:
        assert inl == [], what


@pytest.mark.parametrize("seed", [1, 2])
def test_harness_rounds_equal_restatement(tmp_path, seed):
    assert os.path.exists(HARNESS), "examples/pnp_harness is built by build()"
    sc = make_relocalisation(seed)
    path = tmp_path / "scene.bin"
    path.write_bytes(scene_bytes(sc, 60, 5))
    out = subprocess.run([HARNESS, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    refs = [ref_solver(sc, c) for c in range(len(sc["cands"]))]
    rounds = P.relocalization_rounds(refs, n=5, max_rounds=60)
    exp = [(r, c, o) for r, row in enumerate(rounds) for c, o in enumerate(row) if o is not None]
    got = [l for l in lines if l.startswith("R ")]
    assert len(got) == len(exp)
    for l, (r, c, o) in zip(got, exp):
        assert parse(l)[1:3] == (r, c)
        check(l, o, f"round {r} candidate {c}")
    one = ref_solver(sc, 0)
    s_line = [l for l in lines if l.startswith("S ")][0]
    f_line = [l for l in lines if l.startswith("F ")][0]
    check(s_line, one.iterate(5), "single iterate")
    check(f_line, one.find(), "single find after iterate")
