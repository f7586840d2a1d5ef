"""The crafted scenes of tests/orbsearch_scenes.py on the CPU: every scene's witness holds (the edge it is named after is really in it),
the compiled oracle (oracle/lldo_orbsearch.cpp) equals the numpy reference, and every scene catches the mutations it lists - at least
one named one-line mutation of the numpy reference changes the answer, so a kernel with that mistake fails the scene.  No GPU."""
import numpy as np
import pytest

import oracle_orbsearch as OS
import orbsearch_ref as R
import orbsearch_scenes as SC
from lld_slam_amd import orb_search, synth


def bits_of(a): return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the window searches
@pytest.mark.parametrize("name", SC.NAMES)
def test_witness_holds(name):
    scene = SC.scenes()[name]
    ref, trace = scene.ref()
    assert scene.witness(ref, trace) >= 1


@pytest.mark.parametrize("name", SC.ROUTINE_NAMES)
def test_compiled_oracle_equals_the_numpy_reference(name):
    scene = SC.scenes()[name]
    ref, _ = scene.ref()
    got = getattr(OS, scene.routine)(*scene.args)
    got = got if isinstance(got, tuple) else (got,)
    exp = scene.routine_view(ref)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)


@pytest.mark.parametrize("name", SC.NAMES)
def test_scene_catches_its_mutations(name):
    scene = SC.scenes()[name]
    ref, _ = scene.ref()
    assert scene.mutations, "every scene needs a mutation it catches"
    for m in scene.mutations:
        assert m in R.MUTATIONS
        assert R.differs(R.search_ref(scene.p, m), ref), f"{name} does not notice: {R.MUTATIONS[m]}"


def test_every_family_and_mutation_is_used():
    scenes = list(SC.scenes().values()) + list(SC.projection_scenes().values())
    assert {s.family for s in scenes} == {"windows", "ties", "thresholds", "level", "gates", "occupancy", "takeover", "histogram", "projection"}
    used = {m for s in scenes for m in s.mutations}
    # a window outside the grid holds no keypoint either way: clamping in place of the early return cannot show
    assert used == (set(R.MUTATIONS) | set(R.PROJECTION_MUTATIONS)) - {"no_early_return"}, (set(R.MUTATIONS) | set(R.PROJECTION_MUTATIONS)) ^ used


def test_unmutated_reference_is_deterministic():
    for s in list(SC.scenes().values())[:10]:
        assert not R.differs(R.search_ref(s.p), s.ref()[0])


# ---------------------------------------------------------------------------------------------------------------- the projection loops
def oracle_projection(scene):
    """The compiled oracle's projection loop of the scene's routine, in the layout of ProjScene.project."""
    k = scene.kind
    if k == "local_points":
        _, inv, uvr, lvl, vc = OS.is_in_frustum(scene.view, scene.pts, 0.5)
        return dict(valid=inv, uv=uvr[:, :2], ur=uvr[:, 2], lvl=lvl, vc=vc)
    if k == "last_frame":
        valid, uv, ur = OS.project_last_frame(scene.view, scene.pts)
        return dict(valid=valid, uv=uv, ur=ur)
    if k == "fuse":
        valid, uv, ur, lvl = OS.project_fuse(scene.view, scene.pts)
        return dict(valid=valid, uv=uv, ur=ur, lvl=lvl)
    valid, uv, lvl = OS.project_general(scene.view, scene.pts, int(k[-1]), scene.sR, scene.t)
    return dict(valid=valid, uv=uv, lvl=lvl)


@pytest.mark.parametrize("name", SC.PROJ_NAMES)
def test_projection_witness_oracle_and_mutations(name):
    scene = SC.projection_scenes()[name]
    pr, out, trace = scene.ref()
    assert scene.witness((pr, out, trace), trace) >= 1
    got = oracle_projection(scene)
    np.testing.assert_array_equal(got["valid"] != 0, pr["valid"] != 0)
    m = pr["valid"] != 0
    for key, g in got.items():
        if key != "valid":
            np.testing.assert_array_equal(bits_of(g[m]) if g.dtype == np.float32 else g[m], bits_of(pr[key][m]) if g.dtype == np.float32 else pr[key][m], err_msg=key)
    assert scene.mutations
    for mname in scene.mutations:
        assert SC.proj_differs(scene.answer(mname), (pr, out)), f"{name} does not notice: {R.PROJECTION_MUTATIONS[mname]}"


def test_numpy_projection_loops_equal_the_compiled_oracle_on_a_seeded_scene():
    F = synth.make_orb_frame(3, 300); T, mp = synth.make_local_map(F, 3, 400)
    view = orb_search.frame_view(T, synth.KITTI_CAM, F)
    k, inv, uvr, lvl, vc = OS.is_in_frustum(view, mp)
    i2, u2, l2, v2, why = R.frustum_ref(view, mp)
    m = inv != 0
    np.testing.assert_array_equal(inv, i2); np.testing.assert_array_equal(bits_of(uvr[m]), bits_of(u2[m]))
    np.testing.assert_array_equal(lvl[m], l2[m]); np.testing.assert_array_equal(bits_of(vc[m]), bits_of(v2[m]))
    assert k == m.sum() and all(why.count(w) >= 5 for w in ("skip", "behind", "image", "dist", "angle", "ok"))
    sR = (0.9 * synth._rodrigues(np.array([0.02, -0.01, 0.03]))).astype(np.float32); t2 = np.array([0.1, -0.05, 0.2], np.float32)
    for routine in range(4):
        v, uv, l = OS.project_general(view, mp, routine, sR, t2)
        a = R.project_general_ref(view, mp, routine, sR, t2); m = v != 0
        np.testing.assert_array_equal(v, a[0]); np.testing.assert_array_equal(bits_of(uv[m]), bits_of(a[1][m])); np.testing.assert_array_equal(l[m], a[3][m])
        assert m.sum() > 200
