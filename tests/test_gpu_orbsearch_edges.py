"""GPU: the crafted scenes of tests/orbsearch_scenes.py (windows, visit-order ties, thresholds, gates, occupancy chains, the take-over
rule, the rotation histogram, the projection loops) on the device against the plain numpy reference of tests/orbsearch_ref.py.  Every
output is an integer, an index or a float compared as bits: exact equality, no tolerances.  Each search scene runs through the generic
lld_orb_search_run entry with its explicit flags, through the wrapper of the reference routine it restates (where there is one), and once
more inside one lld_orb_search_batch launch; each projection scene runs through the whole-routine entry point that projects on the device."""
import ctypes as C

import numpy as np
import pytest

import orbsearch_ref as R
import orbsearch_scenes as SC
from lld_slam_amd import abi, orb_search as S

pytestmark = pytest.mark.gpu


def bits_of(a): return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_prepared(ctx, p):
    """lld_orb_search_run on an already configured problem; the outputs are copied out of the problem's own buffers."""
    fn = ctx.lib.fn("orb_search_run")
    fn.argtypes = [C.c_void_p, C.POINTER(S.OrbSearch), C.POINTER(S.OrbSearchResult)]; fn.restype = C.c_int
    for a in (p.out.match, p.out.best_dist, p.out.second_dist, p.out.owner): a[...] = -77
    p.out.removed[...] = 77
    st = fn(ctx.handle, C.byref(p.s), C.byref(p.r))
    assert st == abi.LLD_OK, ctx.lib.fn("status_string")(st)
    return S.SearchOutput(p.out.match.copy(), p.out.best_dist.copy(), p.out.second_dist.copy(), p.out.removed.copy(), p.out.owner.copy(), p.r.n_matches, p.r.rounds)


@pytest.mark.parametrize("name", SC.NAMES)
def test_generic_entry_equals_the_numpy_reference(gpu_ctx, name):
    scene = SC.scenes()[name]
    R.assert_same(run_prepared(gpu_ctx, scene.p), scene.ref()[0], name)


@pytest.mark.parametrize("name", SC.ROUTINE_NAMES)
def test_routine_wrapper_equals_the_numpy_reference(gpu_ctx, name):
    scene = SC.scenes()[name]
    ref, _ = scene.ref()
    got = getattr(S, scene.routine)(gpu_ctx.lib, gpu_ctx.handle, *scene.device_args())
    exp = scene.routine_view(ref)
    if scene.routine == "search_for_initialization":                          # the wrapper returns the routine's own outputs
        assert len(got) == len(exp)
    else:
        R.assert_same(got, ref, name)
        got = scene.routine_view(got)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)


def test_all_scenes_in_one_batch_launch_equal_the_single_calls(gpu_ctx):
    scenes = list(SC.scenes().values())
    single = [run_prepared(gpu_ctx, s.p) for s in scenes]
    outs = S.run_batch(gpu_ctx.lib, gpu_ctx.handle, [s.p for s in scenes])
    for s, one, out in zip(scenes, single, outs):
        R.assert_same(out, s.ref()[0], s.name + " (batch)")
        R.assert_same(out, one, s.name + " (batch against single)")
        assert out.rounds == one.rounds


def test_rescans_and_rounds_are_reported(gpu_ctx):
    """The scenes built to force a long fixed-point chain do so on the device: query i of the occupancy chain learns in round i + 1 that its
    first choice is taken, so the chain needs more rounds than it has queries."""
    for nq in (1023, 1024, 1025):
        assert run_prepared(gpu_ctx, SC.scenes()["occ_chain_%d" % nq].p).rounds >= nq


def device_projection(ctx, scene):
    """The whole-routine entry point of the scene's kind: (search outputs, projection outputs in the layout of ProjScene.project)."""
    k, lib, h, p = scene.kind, ctx.lib, ctx.handle, scene.pts
    if k == "local_points":
        out, fr = S.search_local_points(lib, h, scene.F, scene.view, p, scene.occupied, scene.th, 0.8, 0.5)
        return out, dict(valid=fr["in_view"], uv=fr["proj_uvr"][:, :2], ur=fr["proj_uvr"][:, 2], lvl=fr["level"], vc=fr["view_cos"])
    if k == "last_frame":
        out, uvr = S.search_last_frame(lib, h, scene.F, scene.view, p, scene.occupied, 0, scene.th, True)
        return out, dict(uv=uvr[:, :2], ur=uvr[:, 2])
    if k == "fuse":
        out, uvr = S.fuse_search_points(lib, h, scene.F, scene.view, p, scene.th)
        return out, dict(uv=uvr[:, :2], ur=uvr[:, 2])
    routine = int(k[-1])
    out, uv, lvl = S.search_projected(lib, h, scene.F, scene.view, p, routine, scene.th, accept_max=64, check_orientation=routine == S.PROJ_RELOC,
                                      angle=np.zeros(scene.F.n, np.float32), occupied=scene.occupied, sR=scene.sR, t=scene.t)
    return out, dict(uv=uv, lvl=lvl)


@pytest.mark.parametrize("name", SC.PROJ_NAMES)
def test_whole_routine_projects_and_searches_like_the_numpy_reference(gpu_ctx, name):
    scene = SC.projection_scenes()[name]
    pr, ref, _ = scene.ref()
    out, got = device_projection(gpu_ctx, scene)
    m = pr["valid"] != 0
    if "valid" in got: np.testing.assert_array_equal(got.pop("valid") != 0, m)
    for key, g in got.items():                                                # values of points that do not reach the search are unspecified
        np.testing.assert_array_equal(bits_of(g[m]) if g.dtype == np.float32 else g[m], bits_of(pr[key][m]) if g.dtype == np.float32 else pr[key][m], err_msg=key)
    R.assert_same(out, ref, name)


@pytest.mark.parametrize("pre", ["exact_", "kitti_scan_", "all_skipped_"])
def test_search_by_sim3_whole_routine(gpu_ctx, pre):
    """ORBmatcher::SearchBySim3 in one call: both directions are the scene's SIM3_DIR problem (the same keyframe, points and transform on either
    side), so the agreement check keeps match[i] exactly where match[match[i]] == i."""
    scene = SC.projection_scenes()[pre + "proj3"]
    _, ref, _ = scene.ref()
    m = ref.match
    exp = np.array([m[i] if m[i] >= 0 and m[m[i]] == i else -1 for i in range(m.size)], np.int32)
    got, found = S.search_by_sim3_points(gpu_ctx.lib, gpu_ctx.handle, scene.F, scene.view, scene.pts, scene.F, scene.view, scene.pts,
                                         scene.sR, scene.t, scene.sR, scene.t, scene.th)
    np.testing.assert_array_equal(got, exp)
    assert found == int((exp >= 0).sum())
