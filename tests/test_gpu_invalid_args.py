"""Error behaviour of the newer entry points: malformed arguments are refused with a status, nothing is launched."""
import ctypes as C

import numpy as np
import pytest

from lld_slam_amd import abi, orb_search as S, synth

pytestmark = pytest.mark.gpu


def test_null_and_malformed_arguments_return_a_status(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    f = lib.fn("optimize_sim3"); f.argtypes = [C.c_void_p] * 4; f.restype = C.c_int
    assert f(h, None, None, None) != 0
    p = synth.make_sim3_pair(0, 30).to_c(); r = abi.Sim3Result()
    assert f(h, C.addressof(p), None, C.addressof(r)) != 0                      # result.dropped missing
    p.n = -1
    d = np.zeros(30, np.uint8); r.dropped = d.ctypes.data_as(abi.c_uint8_p)
    assert f(h, C.addressof(p), None, C.addressof(r)) != 0
    g = lib.fn("optimize_essential_graph"); g.argtypes = [C.c_void_p] * 4; g.restype = C.c_int
    assert g(h, None, None, None) != 0
    G = abi.PoseGraph(); G.n_vertices = 3; G.n_edges = 1                        # arrays missing
    o = np.zeros((3, 8)); R = abi.PoseGraphResult(); R.sim3 = o.ctypes.data_as(abi.c_double_p)
    assert g(h, C.addressof(G), None, C.addressof(R)) != 0
    k = lib.fn("compute_stereo_matches"); k.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]; k.restype = C.c_int
    assert k(h, None, None, None, 0.5, 380.0, None) != 0
    sc = synth.make_stereo_scene(6, 200, width=320, height=150)
    kl, kr = S.keypoints_struct(sc["L"]), S.keypoints_struct(sc["R"])
    P, keep = S.pyramids_struct(sc["left"], sc["right"], sc["L"].scale, sc["inv_scale"])
    res = S.StereoResult()                                                     # u_right / depth missing
    assert k(h, C.addressof(kl), C.addressof(kr), C.addressof(P), sc["mb"], sc["mbf"], C.addressof(res)) != 0
    bad_oct = sc["L"].octave.copy(); bad_oct[0] = 99
    kl.octave = bad_oct.ctypes.data_as(abi.c_int32_p)
    ur = np.zeros(200, np.float32); dp = np.zeros(200, np.float32)
    res.u_right = ur.ctypes.data_as(abi.c_float_p); res.depth = dp.ctypes.data_as(abi.c_float_p)
    assert k(h, C.addressof(kl), C.addressof(kr), C.addressof(P), sc["mb"], sc["mbf"], C.addressof(res)) != 0   # octave outside the pyramid
    # the context is still usable afterwards
    from lld_slam_amd import Optimizer
    assert Optimizer(gpu_ctx).OptimizeSim3(synth.make_sim3_pair(1, 60)).n_inliers > 10


def test_zero_iteration_rounds_are_refused(gpu_ctx):
    """optimize(0) would evaluate no error at all, and the outlier classification that follows would read g2o's uninitialised _error
    vectors (undefined behaviour in the reference): the parameter set is refused instead of being given a meaning of our own."""
    from lld_slam_amd import Optimizer
    w = synth.make_lba_small(12, n_free=4, n_fixed=2, n_points=60, n_lines=10)
    for kw in (dict(its_round1=0), dict(its_round2=0), dict(its_round1=0, its_round2=0)):
        with pytest.raises(RuntimeError):
            Optimizer(gpu_ctx).LocalBundleAdjustment(w, **kw)
    assert Optimizer(gpu_ctx).LocalBundleAdjustment(w, its_round1=1, its_round2=1).stats["lm_iterations"] == [1, 1]


def test_keypoint_side_refusals_of_the_projecting_searches(gpu_ctx):
    """Every entry point that takes a frame by its keypoints refuses a malformed keypoint side with the same status, before anything is queued:
    a 100-keypoint frame, 50 queries, one defect at a time.  Only the general problem (lld_orb_search_run) answers UNSUPPORTED to a level
    count above LLD_ORB_MAX_LEVELS, and that difference is part of the contract.  The valid call at the end, on the same context, equals the
    oracle's: the refusals left nothing behind."""
    import oracle_orbsearch as OS
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    INVALID, UNSUPPORTED = abi.LLD_ERR_INVALID, abi.LLD_ERR_UNSUPPORTED
    F = synth.make_orb_frame(210, 100)
    T, mp = synth.make_local_map(F, 210, 50)
    view = S.frame_view(T, synth.KITTI_CAM, F)
    last = dict(world_pos=mp["world_pos"], valid=np.ones(50, np.uint8), octave=F.octave[mp["src"]], angle=F.angle[mp["src"]], desc=mp["desc"], has_obs=mp["has_obs"])
    good = S.prepare(F, np.zeros((0, 8), np.uint32), candidates=S.CAND_GRID, accept_max=S.TH_HIGH, t_occupied=mp["occupied"])
    m, _keep_m = S.map_points_struct(mp)
    lf, _keep_l = S.last_frame_struct(last)
    pr = S.OrbProjection(); pr.routine, pr.th, pr.accept_max = S.PROJ_RELOC, 10.0, 100
    P = C.POINTER

    def fn(name, *argtypes):
        f = lib.fn(name); f.argtypes = [C.c_void_p, *argtypes]; f.restype = C.c_int
        return f
    create = fn("frame_create", P(S.OrbSearch), P(C.c_void_p))
    destroy = lib.fn("frame_destroy"); destroy.argtypes = [C.c_void_p]; destroy.restype = None
    local = fn("orb_search_local_points", P(S.OrbSearch), P(S.FrameView), P(S.MapPoints), C.c_float, C.c_float, C.c_float, P(S.FrustumResult), P(S.OrbSearchResult))
    lastf = fn("orb_search_last_frame", P(S.OrbSearch), P(S.FrameView), P(S.LastFramePoints), C.c_int, C.c_float, C.c_int, abi.c_float_p, P(S.OrbSearchResult))
    fuse = fn("orb_fuse_search", P(S.OrbSearch), P(S.FrameView), P(S.MapPoints), C.c_float, abi.c_float_p, P(S.OrbSearchResult))
    proj = fn("orb_search_projected", P(S.OrbSearch), P(S.FrameView), P(S.MapPoints), abi.c_float_p, P(S.OrbProjection), abi.c_float_p, abi.c_int32_p, P(S.OrbSearchResult))

    def call_create(s, v, r, l):
        out = C.c_void_p()
        st = create(h, C.byref(s), C.byref(out))
        if out.value: destroy(out)
        return st
    entry = {
        "lld_frame_create": call_create,
        "lld_orb_search_local_points": lambda s, v, r, l: local(h, C.byref(s), C.byref(v), C.byref(m), 0.5, 1.0, 0.8, None, C.byref(r)),
        "lld_orb_search_last_frame": lambda s, v, r, l: lastf(h, C.byref(s), C.byref(v), C.byref(l), 0, 7.0, 1, None, C.byref(r)),
        "lld_orb_fuse_search": lambda s, v, r, l: fuse(h, C.byref(s), C.byref(v), C.byref(m), 3.0, None, C.byref(r)),
        "lld_orb_search_projected": lambda s, v, r, l: proj(h, C.byref(s), C.byref(v), C.byref(m), None, C.byref(pr), None, None, C.byref(r)),
    }
    searching = [k for k in entry if k != "lld_frame_create"]

    res_arrays = [np.empty(50, np.int32), np.empty(50, np.int32), np.empty(50, np.int32), np.empty(50, np.uint8)]
    bad_octave = F.octave.copy(); bad_octave[7] = S.MAX_LEVELS
    bad_last_octave = last["octave"].astype(np.int32).copy(); bad_last_octave[3] = F.scale.shape[0]

    def fresh():
        s = S.OrbSearch.from_buffer_copy(good.s); v = S.FrameView.from_buffer_copy(view); l = S.LastFramePoints.from_buffer_copy(lf)
        r = S.OrbSearchResult()
        r.match = res_arrays[0].ctypes.data_as(abi.c_int32_p); r.best_dist = res_arrays[1].ctypes.data_as(abi.c_int32_p)
        r.second_dist = res_arrays[2].ctypes.data_as(abi.c_int32_p); r.removed = res_arrays[3].ctypes.data_as(abi.c_uint8_p)
        return dict(s=s, v=v, r=r, l=l)

    def grid(a, cols, rows): a["s"].grid_cols, a["s"].grid_rows = cols, rows
    keypoint_side = [
        ("nt = -1", lambda a: setattr(a["s"], "nt", -1), INVALID),
        ("nt = LLD_ORB_MAX_KEYPOINTS + 1", lambda a: setattr(a["s"], "nt", S.MAX_KEYPOINTS + 1), UNSUPPORTED),
        ("t_desc = NULL", lambda a: setattr(a["s"], "t_desc", None), INVALID),
        ("level_scale = NULL", lambda a: setattr(a["s"], "level_scale", None), INVALID),
        ("n_levels = 0", lambda a: setattr(a["s"], "n_levels", 0), INVALID),
        ("n_levels = LLD_ORB_MAX_LEVELS + 1", lambda a: setattr(a["s"], "n_levels", S.MAX_LEVELS + 1), INVALID),
        ("grid_cols = 0", lambda a: grid(a, 0, S.FRAME_GRID_ROWS), INVALID),
        ("grid_cols * grid_rows = 8192", lambda a: grid(a, 128, 64), INVALID),
        ("an octave = LLD_ORB_MAX_LEVELS", lambda a: setattr(a["s"], "t_octave", bad_octave.ctypes.data_as(abi.c_int32_p)), INVALID),
    ]
    query_side = [
        ("result.match = NULL", lambda a: setattr(a["r"], "match", None), INVALID),
        ("view.n_levels != frame.n_levels", lambda a: setattr(a["v"], "n_levels", a["s"].n_levels - 1), INVALID),
    ]
    table = [(name, what, defect, status) for name in entry for what, defect, status in keypoint_side]
    table += [(name, what, defect, status) for name in searching for what, defect, status in query_side]
    table.append(("lld_orb_fuse_search", "level_inv_sigma2 = NULL", lambda a: setattr(a["s"], "level_inv_sigma2", None), INVALID))
    table.append(("lld_orb_search_last_frame", "a last-frame octave = n_levels",
                  lambda a: setattr(a["l"], "octave", bad_last_octave.ctypes.data_as(abi.c_int32_p)), INVALID))
    got = []
    for name, what, defect, status in table:
        a = fresh(); defect(a)
        st = entry[name](a["s"], a["v"], a["r"], a["l"])
        if st != status: got.append((name, what, st, status))
    # the general problem: above the level limit is UNSUPPORTED, not INVALID
    g = S.prepare(F, mp["desc"], candidates=S.CAND_GRID, accept_max=S.TH_HIGH, q_uv=np.zeros((50, 2), np.float32), q_radius=np.ones(50, np.float32))
    g.s.n_levels = S.MAX_LEVELS + 1
    run = fn("orb_search_run", P(S.OrbSearch), P(S.OrbSearchResult))
    st = run(h, C.byref(g.s), C.byref(g.r))
    if st != UNSUPPORTED: got.append(("lld_orb_search_run", "n_levels = LLD_ORB_MAX_LEVELS + 1", st, UNSUPPORTED))
    assert not got, "(entry point, defect, status, expected): %r" % (got,)
    for name in entry:                                                          # the unspoilt arguments are accepted by every one of them
        a = fresh()
        assert entry[name](a["s"], a["v"], a["r"], a["l"]) == abi.LLD_OK, name
    out, fr = S.search_local_points(lib, h, F, view, mp, mp["occupied"], 1.0, 0.8)
    k, inv, uvr, lvl, vc = OS.is_in_frustum(view, mp)
    np.testing.assert_array_equal(fr["in_view"], inv)
    n_exp, slot = OS.search_by_projection_map(F, mp["desc"], inv, uvr[:, :2], uvr[:, 2], lvl, vc, mp["has_obs"], mp["occupied"], 1.0, 0.8)
    got_slot = np.where(out.owner >= 0, out.owner, np.where(mp["occupied"] != 0, 1 << 20, -1))
    assert out.n_matches == n_exp and n_exp > 0
    np.testing.assert_array_equal(got_slot, slot)
