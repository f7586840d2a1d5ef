"""Frame::ComputeStereoMatches on the crafted scenes of tests/stereo_scenes.py (what each is for: tests/test_oracle_stereo_exits.py), by
both device routes - lld_compute_stereo_matches (row-bucket stage 1 of orb_search_kernel) and lld_frame_build_stereo_keypoints
(stereo_rows_kernel) - against the oracle's literal restatement: u_right and depth as bit patterns, best_r, sad and n_matches, all equal.
The deltaR exit has no scene: it cannot be taken (see the header of tests/test_oracle_stereo_exits.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle_orbsearch as OS
import stereo_scenes as S
from lld_slam_amd import ORBmatcher, abi, orb_search
from lld_slam_amd.abi import c_float_p, c_int32_p, c_uint8_p, c_uint32_p

pytestmark = pytest.mark.gpu

_cache = {}


def scene(name):
    """(scene, left Frame, right Frame, the oracle's result); computed once per scene, never changed."""
    if name not in _cache:
        sc = S.SCENES[name]()
        L, R = S.frames(sc)
        _cache[name] = (sc, L, R, OS.compute_stereo_matches(L, R, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"]))
    return _cache[name]


def check(g, ref, what):
    """The comparison of tests/test_gpu_orbsearch.py's _check_stereo, with the place of the first difference in the message."""
    n, ur, dep, br, sad = ref
    for name, got, exp in (("best_r", g.best_r, br), ("sad", g.sad, sad), ("u_right", g.u_right.view(np.uint32), ur.view(np.uint32)),
                           ("depth", g.depth.view(np.uint32), dep.view(np.uint32))):
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}: {got[bad[:8]]} vs {exp[bad[:8]]}"
    assert g.n_matches == n, f"{what}: n_matches {g.n_matches} vs {n}"


def build_and_download(ctx, L, R, sc, **kw):
    built = orb_search.build_stereo_frame_keypoints(ctx.lib, ctx.handle, L, R, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"], **kw)
    try:
        return built.download()
    finally:
        built.close()


@pytest.mark.parametrize("name", list(S.SCENES))
def test_host_route(gpu_ctx, name):
    sc, L, R, ref = scene(name)
    g = ORBmatcher(gpu_ctx).ComputeStereoMatchesFull(L, R, sc["left"], sc["right"], sc["inv_scale"], sc["mb"], sc["mbf"])
    check(g, ref, f"{name}, lld_compute_stereo_matches")


@pytest.mark.parametrize("name", list(S.SCENES))
def test_device_route(gpu_ctx, name):
    sc, L, R, ref = scene(name)
    check(build_and_download(gpu_ctx, L, R, sc), ref, f"{name}, lld_frame_build_stereo_keypoints")


@pytest.mark.parametrize("name", ["tall", "patch_limits"])
def test_device_resident_inputs(gpu_ctx, name):
    """Pyramids (on_device = 1, with a row step larger than the width) and keypoints already in HBM: nothing but the left octaves is uploaded."""
    import torch
    sc, L, R, ref = scene(name)
    pad = lambda a: np.ascontiguousarray(np.pad(a, ((0, 0), (0, 13))))
    dl = [torch.from_numpy(pad(a)).cuda() for a in sc["left"]]; dr = [torch.from_numpy(pad(a)).cuda() for a in sc["right"]]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()
    t = dict(lxy=up(L.xy), ldesc=up(L.desc), langle=up(L.angle), rxy=up(R.xy), roct=up(R.octave), rdesc=up(R.desc))
    torch.cuda.synchronize()

    def device_pyramids():
        P, keep = orb_search.pyramids_struct(sc["left"], sc["right"], L.scale, sc["inv_scale"])
        keep["dlp"] = (c_uint8_p * len(dl))(*[C.cast(x.data_ptr(), c_uint8_p) for x in dl]); keep["drp"] = (c_uint8_p * len(dr))(*[C.cast(x.data_ptr(), c_uint8_p) for x in dr])
        keep["step"] = np.array([x.shape[1] for x in dl], np.int32)
        P.left = C.cast(keep["dlp"], C.POINTER(c_uint8_p)); P.right = C.cast(keep["drp"], C.POINTER(c_uint8_p))
        P.left_step = keep["step"].ctypes.data_as(c_int32_p); P.right_step = keep["step"].ctypes.data_as(c_int32_p); P.on_device = 1
        return P, keep

    # lld_compute_stereo_matches: keypoints from the host, pyramids in place
    kl, kr = orb_search.keypoints_struct(L), orb_search.keypoints_struct(R)
    P, keep = device_pyramids()
    n = L.n
    g = orb_search.StereoMatches(np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.int32), 0)
    r = orb_search.StereoResult(); r.u_right = g.u_right.ctypes.data_as(c_float_p); r.depth = g.depth.ctypes.data_as(c_float_p)
    r.best_r = g.best_r.ctypes.data_as(c_int32_p); r.sad = g.sad.ctypes.data_as(c_int32_p)
    fn = gpu_ctx.lib.fn("compute_stereo_matches")
    fn.argtypes = [C.c_void_p, C.POINTER(orb_search.Keypoints), C.POINTER(orb_search.Keypoints), C.POINTER(orb_search.StereoPyramids), C.c_float, C.c_float,
                   C.POINTER(orb_search.StereoResult)]
    fn.restype = C.c_int
    assert fn(gpu_ctx.handle, C.byref(kl), C.byref(kr), C.byref(P), sc["mb"], sc["mbf"], C.byref(r)) == abi.LLD_OK
    g.n_matches = r.n_matches
    check(g, ref, f"{name}, lld_compute_stereo_matches, pyramids in HBM")

    # lld_frame_build_stereo_keypoints: keypoints and pyramids in place
    kl, kr = orb_search.keypoints_struct(L), orb_search.keypoints_struct(R)
    kl.xy = C.cast(C.c_void_p(t["lxy"].data_ptr()), c_float_p); kl.desc = C.cast(C.c_void_p(t["ldesc"].data_ptr()), c_uint32_p)
    kr.xy = C.cast(C.c_void_p(t["rxy"].data_ptr()), c_float_p); kr.octave = C.cast(C.c_void_p(t["roct"].data_ptr()), c_int32_p)
    kr.desc = C.cast(C.c_void_p(t["rdesc"].data_ptr()), c_uint32_p)
    prm, keep2 = orb_search.frame_stereo_params(L, sc["mb"], sc["mbf"], angle=t["langle"].data_ptr(), keypoints_on_device=True)
    st, h = orb_search.build_stereo_frame_raw(gpu_ctx.lib, gpu_ctx.handle, kl, kr, P, prm)
    assert st == abi.LLD_OK
    built = orb_search.StereoBuiltFrame(gpu_ctx.lib, gpu_ctx.handle, L, h)
    try:
        got = built.download()
    finally:
        built.close()
    check(got, ref, f"{name}, lld_frame_build_stereo_keypoints, everything in HBM")
