"""Independent restatement of the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:245-262, :287-451) with the
numerics of include/lld_amd.h: DEVIATION 2 of the Initializer section (float products summed in double in index order and rounded
once, cv::norm in double, null vectors through the cyclic Jacobi on A^T A with the canonical sign) and the closed-form stereo
parallax cosine.  Written from LocalMapping.cc, KeyFrame.cc and the header text; imports nothing from lld_slam_amd.  The small
linear algebra comes from tests/initializer_ref.py.

Everything is numpy element-wise arithmetic over the matches of one pair: a float value lives in a float32 array, a float
operation is one float32 operation, a double operation one float64 operation (numpy never fuses a multiply and an add).

Also: the seeded scene generator make_scene (KITTI-like camera, mixed stereo and mono keypoints or a mono mode, neighbours at
several baselines including one the baseline gate skips), the hand-made scenes crafted_scenes (one match per status and source)
and margins(), the smallest relative distance of any compared quantity from its threshold."""
from __future__ import annotations

import numpy as np

from initializer_ref import CAM, F32, F64, _quiet, _rot, mm, norm3, null_vector_batch

(NEW, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, DIST_ZERO, SCALE, NO_DEPTH, PAIR_SKIPPED) = range(11)
SRC_TRIANGULATED, SRC_STEREO1, SRC_STEREO2 = range(3)
MARGIN = 1e-5


# ------------------------------------------------------------------ keyframes
def level_tables(n_levels=8, scale=1.2):
    """mvScaleFactors / mvLevelSigma2 as ORBextractor builds them, in float."""
    sf = np.ones(n_levels, F32)
    for i in range(1, n_levels):
        sf[i] = sf[i - 1] * F32(scale)
    return sf, (sf * sf).astype(F32)


def make_kf(R, t, fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"], mb=0.54, median_depth=0.0, n_levels=8):
    sf, s2 = level_tables(n_levels)
    return dict(Rcw=np.asarray(R, F32).reshape(3, 3).copy(), tcw=np.asarray(t, F32).reshape(3).copy(), fx=F32(fx), fy=F32(fy), cx=F32(cx),
                cy=F32(cy), mb=F32(mb), mbf=F32(F32(fx) * F32(mb)), scale_factor=F32(1.2), median_depth=F32(median_depth),
                scale_factors=sf, level_sigma2=s2)


@_quiet
def derived(kf):
    """Rwc, Ow = -Rwc*tcw (src/KeyFrame.cc:85), invfx, invfy (src/Frame.cc:150)."""
    Rwc = np.asarray(kf["Rcw"], F32).reshape(3, 3).T
    Ow = -mm(Rwc, np.asarray(kf["tcw"], F32))
    return Rwc, Ow.astype(F32), F32(1.0) / F32(kf["fx"]), F32(1.0) / F32(kf["fy"])


def _rel(a, b):
    a = np.asarray(a, F64); b = np.asarray(b, F64)
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
    return np.where(np.isnan(r), 0.0, r)


@_quiet
def pair_gate(kf1, kf2, monocular):
    """The baseline gate (:245-262): (skipped, relative distance of the compared quantity from its threshold)."""
    Ow1, Ow2 = derived(kf1)[1], derived(kf2)[1]
    baseline = F32(norm3((Ow2 - Ow1).astype(F32)))
    if not monocular:
        return bool(baseline < F32(kf2["mb"])), float(_rel(baseline, kf2["mb"]))
    ratio = F32(baseline / F32(kf2["median_depth"]))
    return bool(F64(ratio) < 0.01), float(_rel(ratio, 0.01))


@_quiet
def cos_stereo(mb, depth):
    """cos(2*atan2(mb/2, depth)) as (d^2 - a^2)/(d^2 + a^2) in double, rounded to float (the header's DEVIATION)."""
    a = F64(F32(mb) / F32(2.0)); d = np.asarray(depth, F32).astype(F64)
    return ((d * d - a * a) / (d * d + a * a)).astype(F32)


def _rowdot(R, r, x):
    Rd = np.asarray(R, F32).astype(F64); xd = x.astype(F64)
    s = Rd[r, 0] * xd[:, 0]
    s = s + Rd[r, 1] * xd[:, 1]
    return s + Rd[r, 2] * xd[:, 2]


@_quiet
def _unproject(kf, u, v, z):
    """KeyFrame::UnprojectStereo (src/KeyFrame.cc:638-654) without its z > 0 test."""
    Rwc, Ow, invfx, invfy = derived(kf)
    c = np.stack([(u - kf["cx"]) * z * invfx, (v - kf["cy"]) * z * invfy, z], 1).astype(F32)
    return (mm(Rwc[None], c[:, :, None])[:, :, 0] + Ow).astype(F32)


@_quiet
def _reproj(kf, x3d, z, kx, ky, ur, stereo, mbf):
    """(float error sum, double bound) of one reprojection gate (:364-388 / :391-414)."""
    x = (_rowdot(kf["Rcw"], 0, x3d) + F64(kf["tcw"][0])).astype(F32)
    y = (_rowdot(kf["Rcw"], 1, x3d) + F64(kf["tcw"][1])).astype(F32)
    invz = (1.0 / z.astype(F64)).astype(F32)
    u = kf["fx"] * x * invz + kf["cx"]
    v = kf["fy"] * y * invz + kf["cy"]
    ex = u - kx; ey = v - ky
    er = (u - F32(mbf) * invz) - ur
    e_mono = ex * ex + ey * ey
    e_st = ex * ex + ey * ey + er * er
    return np.where(stereo, e_st, e_mono).astype(F32)


@_quiet
def triangulate_pair(kf1, keys1, kf2, keys2, matches, monocular):
    """One neighbour: dict(pair_status, status, source, x3d, margin) over its matches."""
    matches = np.asarray(matches, np.int64).reshape(-1, 2)
    n = len(matches)
    skipped, gate_margin = pair_gate(kf1, kf2, monocular)
    if skipped or n == 0:
        return dict(pair_status=int(skipped), status=np.full(n, PAIR_SKIPPED if skipped else NEW, np.uint8), source=np.zeros(n, np.uint8),
                    x3d=np.zeros((n, 3), F32), margin=np.full(n, gate_margin))
    i1, i2 = matches[:, 0], matches[:, 1]
    xy1 = np.asarray(keys1["xy"], F32).reshape(-1, 2)[i1]; xy2 = np.asarray(keys2["xy"], F32).reshape(-1, 2)[i2]
    raw1 = xy1 if keys1.get("raw_xy") is None else np.asarray(keys1["raw_xy"], F32).reshape(-1, 2)[i1]
    raw2 = xy2 if keys2.get("raw_xy") is None else np.asarray(keys2["raw_xy"], F32).reshape(-1, 2)[i2]
    ur1 = np.asarray(keys1["ur"], F32)[i1]; ur2 = np.asarray(keys2["ur"], F32)[i2]
    d1 = np.asarray(keys1["depth"], F32)[i1]; d2 = np.asarray(keys2["depth"], F32)[i2]
    o1 = np.asarray(keys1["octave"])[i1]; o2 = np.asarray(keys2["octave"])[i2]
    Rwc1, Ow1, invfx1, invfy1 = derived(kf1)
    Rwc2, Ow2, invfx2, invfy2 = derived(kf2)
    st1 = ur1 >= 0; st2 = ur2 >= 0                                              # :294, :298
    one = np.ones(n, F32)
    xn1 = np.stack([(xy1[:, 0] - kf1["cx"]) * invfx1, (xy1[:, 1] - kf1["cy"]) * invfy1, one], 1).astype(F32)   # :301-302
    xn2 = np.stack([(xy2[:, 0] - kf2["cx"]) * invfx2, (xy2[:, 1] - kf2["cy"]) * invfy2, one], 1).astype(F32)
    ray1 = mm(Rwc1[None], xn1[:, :, None])[:, :, 0]                             # :304-305
    ray2 = mm(Rwc2[None], xn2[:, :, None])[:, :, 0]
    r1, r2 = ray1.astype(F64), ray2.astype(F64)
    dot = r1[:, 0] * r2[:, 0]
    dot = dot + r1[:, 1] * r2[:, 1]
    dot = dot + r1[:, 2] * r2[:, 2]
    cosR = (dot / (norm3(ray1) * norm3(ray2))).astype(F32)                      # :306
    cs1 = (cosR + F32(1.0)).astype(F32); cs2 = cs1.copy()                       # :308-310
    cs1 = np.where(st1, cos_stereo(kf1["mb"], d1), cs1)                         # :312-315: if / else if
    cs2 = np.where(~st1 & st2, cos_stereo(kf2["mb"], d2), cs2)
    cs = np.where(cs2 < cs1, cs2, cs1)                                          # std::min (:317)
    c_a = cosR < cs; c_b = cosR > F32(0.0); c_c = st1 | st2 | (cosR.astype(F64) < 0.9998)
    tri = c_a & c_b & c_c                                                       # :320
    un1 = ~tri & st1 & (cs1 < cs2)                                              # :341
    un2 = ~tri & ~un1 & st2 & (cs2 < cs1)                                       # :345
    low = ~tri & ~un1 & ~un2                                                    # :349
    margin = np.full(n, gate_margin)

    def reach(mask, a, b):
        margin[mask] = np.minimum(margin, _rel(a, b))[mask]

    everyone = np.ones(n, bool)
    reach(everyone, cosR, cs)
    reach(c_a, cosR, np.zeros(n))                                               # cosParallaxRays > 0: 1 unless it is zero
    reach(c_a & c_b & ~st1 & ~st2, cosR, 0.9998)
    reach(~tri & (st1 | st2), cs1, cs2)

    T1 = np.concatenate([kf1["Rcw"], kf1["tcw"][:, None]], 1).astype(F32)       # :323-327
    T2 = np.concatenate([kf2["Rcw"], kf2["tcw"][:, None]], 1).astype(F32)
    A = np.stack([xn1[:, 0, None] * T1[2] - T1[0], xn1[:, 1, None] * T1[2] - T1[1],
                  xn2[:, 0, None] * T2[2] - T2[0], xn2[:, 1, None] * T2[2] - T2[1]], 1).astype(F32)
    x = null_vector_batch(A)
    wzero = x[:, 3] == 0                                                        # :334
    inv = 1.0 / x[:, 3].astype(F64)
    p_tri = (x[:, :3].astype(F64) * inv[:, None]).astype(F32)                   # :338
    m_w = tri & ~wzero                                                          # x3D[3] != 0: a component of a unit vector
    margin[m_w] = np.minimum(margin, np.abs(x[:, 3]).astype(F64))[m_w]
    p_un1 = _unproject(kf1, raw1[:, 0], raw1[:, 1], d1)
    p_un2 = _unproject(kf2, raw2[:, 0], raw2[:, 1], d2)
    x3d = np.where(tri[:, None], p_tri, np.where(un1[:, None], p_un1, p_un2)).astype(F32)
    source = np.where(tri, SRC_TRIANGULATED, np.where(un1, SRC_STEREO1, np.where(un2, SRC_STEREO2, 0))).astype(np.uint8)
    status = np.full(n, NEW, np.uint8)
    alive = np.ones(n, bool)

    def leave(mask, code):
        nonlocal alive
        m = alive & mask
        status[m] = code
        alive = alive & ~m

    leave(low, LOW_PARALLAX)
    leave(tri & wzero, W_ZERO)
    leave((un1 & ~(d1 > 0)) | (un2 & ~(d2 > 0)), NO_DEPTH)
    # :355-361; the margin of a sign test is measured against the magnitudes that enter the sum
    z1 = (_rowdot(kf1["Rcw"], 2, x3d) + F64(kf1["tcw"][2])).astype(F32)
    mag1 = np.abs(kf1["Rcw"][2].astype(F64)) @ np.abs(x3d.astype(F64)).T + abs(F64(kf1["tcw"][2]))
    reach(alive, mag1 + np.abs(z1), mag1)
    leave(z1 <= 0, Z1)
    z2 = (_rowdot(kf2["Rcw"], 2, x3d) + F64(kf2["tcw"][2])).astype(F32)
    mag2 = np.abs(kf2["Rcw"][2].astype(F64)) @ np.abs(x3d.astype(F64)).T + abs(F64(kf2["tcw"][2]))
    reach(alive, mag2 + np.abs(z2), mag2)
    leave(z2 <= 0, Z2)
    e1 = _reproj(kf1, x3d, z1, xy1[:, 0], xy1[:, 1], ur1, st1, kf1["mbf"])
    th1 = np.where(st1, 7.8, 5.991) * np.asarray(kf1["level_sigma2"], F32)[o1].astype(F64)
    reach(alive, e1, th1)
    leave(e1.astype(F64) > th1, REPROJ1)
    e2 = _reproj(kf2, x3d, z2, xy2[:, 0], xy2[:, 1], ur2, st2, kf1["mbf"])     # QUIRK: keyframe 1's mbf (:407)
    th2 = np.where(st2, 7.8, 5.991) * np.asarray(kf2["level_sigma2"], F32)[o2].astype(F64)
    reach(alive, e2, th2)
    leave(e2.astype(F64) > th2, REPROJ2)
    dist1 = norm3((x3d - Ow1).astype(F32)).astype(F32)                          # :417-423
    dist2 = norm3((x3d - Ow2).astype(F32)).astype(F32)
    leave((dist1 == 0) | (dist2 == 0), DIST_ZERO)
    ratioDist = (dist2 / dist1).astype(F32)                                     # :426-431
    ratioOctave = (np.asarray(kf1["scale_factors"], F32)[o1] / np.asarray(kf2["scale_factors"], F32)[o2]).astype(F32)
    ratioFactor = F32(1.5) * F32(kf1["scale_factor"])
    lhs = (ratioDist * ratioFactor).astype(F32); rhs = (ratioOctave * ratioFactor).astype(F32)
    reach(alive, lhs, ratioOctave)
    reach(alive, ratioDist, rhs)
    leave((lhs < ratioOctave) | (ratioDist > rhs), SCALE)
    x3d = np.where((status == NEW)[:, None], x3d, F32(0.0)).astype(F32)
    return dict(pair_status=0, status=status, source=source, x3d=x3d, margin=margin, cos_rays=cosR, cos_stereo=cs)


def triangulate(pb):
    """The whole call on a problem in the form of lld_new_points_in (see make_scene): dict(status, source, x3d, pair_status,
    n_new, new_match, n_new_total, margin)."""
    ks, ms = np.asarray(pb["key_start"]), np.asarray(pb["match_start"])
    parts = []
    for p, kf2 in enumerate(pb["kf2"]):
        k2 = {k: (None if v is None else np.asarray(v)[ks[p]:ks[p + 1]]) for k, v in pb["keys2"].items()}
        parts.append(triangulate_pair(pb["kf1"], pb["keys1"], kf2, k2, np.asarray(pb["matches"]).reshape(-1, 2)[ms[p]:ms[p + 1]],
                                      pb["monocular"]))
    cat = lambda k, dt: np.concatenate([r[k] for r in parts]).astype(dt) if parts else np.zeros(0, dt)
    status = cat("status", np.uint8)
    return dict(status=status, source=cat("source", np.uint8), x3d=np.concatenate([r["x3d"] for r in parts]).astype(F32).reshape(-1, 3),
                margin=cat("margin", F64), pair_status=np.array([r["pair_status"] for r in parts], np.uint8),
                n_new=np.array([int((r["status"] == NEW).sum()) for r in parts], np.int32),
                new_match=np.flatnonzero(status == NEW).astype(np.int32), n_new_total=int((status == NEW).sum()),
                cos_rays=np.concatenate([r.get("cos_rays", np.zeros(len(r["status"]), F32)) for r in parts]),
                cos_stereo=np.concatenate([r.get("cos_stereo", np.zeros(len(r["status"]), F32)) for r in parts]))


def margins(pb):
    """Per match, the smallest relative distance |a - b| / max(|a|, |b|) of any quantity the match's path compares from what it is
    compared with: the baseline gate of its pair, the three tests of :320, :341 / :345, x3D[3] against 0 (as a component of a unit
    vector), z1 and z2 against 0 (against the magnitudes summed), both reprojection sums against their bounds and both scale
    tests.  The two `== 0` tests that come out TRUE (W_ZERO, DIST_ZERO) are left out: only exact structural zeros produce them
    (products by 0 and +-1, sums of equal terms), on which no rounding can differ."""
    return triangulate(pb)["margin"]


# ------------------------------------------------------------------ scenes
def problem(kf1, keys1, kf2, keys2_list, matches_list, monocular):
    key_start = np.concatenate([[0], np.cumsum([len(k["ur"]) for k in keys2_list])]).astype(np.int32)
    match_start = np.concatenate([[0], np.cumsum([len(m) for m in matches_list])]).astype(np.int32)
    cat = lambda k, dt, w: (np.concatenate([np.asarray(q[k], dt).reshape(-1, *w) for q in keys2_list]) if keys2_list else np.zeros((0, *w), dt))
    keys2 = dict(xy=cat("xy", F32, (2,)), raw_xy=cat("raw_xy", F32, (2,)), ur=cat("ur", F32, ()), depth=cat("depth", F32, ()),
                 octave=cat("octave", np.int32, ()))
    matches = (np.concatenate([np.asarray(m, np.int32).reshape(-1, 2) for m in matches_list]) if matches_list else np.zeros((0, 2), np.int32))
    return dict(kf1=kf1, keys1=keys1, kf2=list(kf2), key_start=key_start, keys2=keys2, match_start=match_start, matches=matches,
                monocular=bool(monocular))


def split(pb, p):
    """Pair p of a problem as a problem of its own."""
    ks, ms = pb["key_start"], pb["match_start"]
    k2 = {k: v[ks[p]:ks[p + 1]] for k, v in pb["keys2"].items()}
    return problem(pb["kf1"], pb["keys1"], [pb["kf2"][p]], [k2], [pb["matches"][ms[p]:ms[p + 1]]], pb["monocular"])


BASELINES = (0.9, 0.25, 1.6, 2.8, 0.7, 4.0, 1.2, 2.0, 0.55, 3.3)               # metres; 0.25 is below mb = 0.54


def _project(kf, X, rng, noise, p_stereo, monocular):
    """Keypoints of the world points X in keyframe kf: xy, raw_xy, ur, depth, octave-free; and the camera depth."""
    R, t = kf["Rcw"].astype(F64), kf["tcw"].astype(F64)
    Xc = X @ R.T + t
    z = Xc[:, 2]
    u = F64(kf["fx"]) * Xc[:, 0] / z + F64(kf["cx"]) + rng.normal(0, noise, len(X))
    v = F64(kf["fy"]) * Xc[:, 1] / z + F64(kf["cy"]) + rng.normal(0, noise, len(X))
    xy = np.stack([u, v], 1).astype(F32)
    raw = (xy + np.array([0.37, -0.21], F32)).astype(F32)                       # mvKeys differs from mvKeysUn
    stereo = (rng.random(len(X)) < p_stereo) & ~bool(monocular) & (z > 0.5)
    ur = np.where(stereo, u - F64(kf["mbf"]) / np.where(stereo, z, 1.0) + rng.normal(0, noise, len(X)), -1.0).astype(F32)
    with np.errstate(all="ignore"):
        depth = np.where(stereo, F32(kf["mbf"]) / (xy[:, 0] - ur), F32(-1.0)).astype(F32)   # mvDepth = mbf/disparity (Frame.cc)
    return xy, raw, ur, depth, z


def make_scene(seed, n_matches, monocular=False, n_keys1=None, noise=0.3, p_stereo=0.6, p_outlier=0.08, p_octave=0.06, p_no_depth=0.03, enforce_margin=True):
    """One keyframe and len(n_matches) neighbours at BASELINES (cycled), n_matches[p] matches each.  Every keypoint of keyframe 1
    observes its own world point 3 .. 60 m ahead; a neighbour's keypoint is that point projected there, with pixel noise, a share
    p_outlier displaced by 3 .. 40 px, octaves consistent with the distances except a share p_octave, and (stereo mode) a share
    p_no_depth of keyframe 1's stereo keypoints with depth -1.  Matches whose margins() is not above MARGIN are drawn again (a new
    neighbour keypoint for the same keypoint of keyframe 1), so the scene holds none (enforce_margin=False, for noise-free scenes whose
    keypoints cannot move, draws once).  Returns the problem plus X (the world
    point of every keypoint of keyframe 1)."""
    rng = np.random.default_rng(seed)
    n_matches = list(n_matches)
    n1 = n_keys1 or max(max(n_matches, default=1) + 40, 64)
    Rcw1 = _rot(rng.normal(0, 0.05, 3)); tcw1 = rng.normal(0, 2.0, 3)
    kf1 = make_kf(Rcw1, tcw1)
    u = rng.uniform(40, CAM["w"] - 40, n1); v = rng.uniform(20, CAM["h"] - 20, n1)
    depth = np.exp(rng.uniform(np.log(3.0), np.log(60.0), n1))
    Xc = np.stack([(u - CAM["cx"]) / CAM["fx"], (v - CAM["cy"]) / CAM["fy"], np.ones(n1)], 1) * depth[:, None]
    X = (Xc - kf1["tcw"].astype(F64)) @ kf1["Rcw"].astype(F64)                  # Rwc (Xc - t)
    xy1, raw1, ur1, d1, _ = _project(kf1, X, rng, noise, p_stereo, monocular)
    oct1 = rng.integers(0, 5, n1).astype(np.int32)
    nd = (ur1 >= 0) & (rng.random(n1) < p_no_depth)
    d1 = np.where(nd, F32(-1.0), d1).astype(F32)
    keys1 = dict(xy=xy1, raw_xy=raw1, ur=ur1, depth=d1, octave=oct1)
    C1 = derived(kf1)[1].astype(F64)
    kf2s, keys2s, matches = [], [], []
    for p, nm in enumerate(n_matches):
        b = BASELINES[p % len(BASELINES)] * (0.1 if monocular and p % len(BASELINES) == 1 else 1.0)
        d = rng.normal(0, 1, 3) * np.array([1.0, 0.15, 0.8]); d /= np.linalg.norm(d)
        R2 = _rot(rng.normal(0, 0.03, 3)) @ Rcw1
        C2 = C1 + b * (kf1["Rcw"].astype(F64).T @ d)
        kf2 = make_kf(R2, -R2 @ C2, median_depth=float(np.median(depth)))
        idx1 = rng.permutation(n1)[:nm]
        extra = 7
        pos2 = rng.permutation(nm + extra)[:nm]
        k2 = dict(xy=rng.uniform(0, 300, (nm + extra, 2)).astype(F32), raw_xy=None, ur=np.full(nm + extra, -1, F32),
                  depth=np.full(nm + extra, -1, F32), octave=np.zeros(nm + extra, np.int32))
        k2["raw_xy"] = k2["xy"].copy()
        todo = np.arange(nm)
        for rnd in range(50):
            if len(todo) == 0 or (rnd and not enforce_margin):
                break
            Xm = X[idx1[todo]]
            xy, raw, ur, dp, z2 = _project(kf2, Xm, rng, noise, p_stereo, monocular)
            out = rng.random(len(todo)) < p_outlier
            ang = rng.uniform(0, 2 * np.pi, len(todo)); r = rng.uniform(3, 40, len(todo))
            xy = np.where(out[:, None], xy + np.stack([r * np.cos(ang), r * np.sin(ang)], 1), xy).astype(F32)
            raw = (xy + np.array([0.37, -0.21], F32)).astype(F32)
            dist1 = np.linalg.norm(Xm - C1, axis=1); dist2 = np.linalg.norm(Xm - C2, axis=1)
            o2 = oct1[idx1[todo]] - np.rint(np.log(dist2 / dist1) / np.log(1.2)).astype(np.int64) + rng.integers(-1, 2, len(todo))
            o2 = np.where(rng.random(len(todo)) < p_octave, rng.integers(0, 8, len(todo)), o2)
            k2["xy"][pos2[todo]] = xy; k2["raw_xy"][pos2[todo]] = raw; k2["ur"][pos2[todo]] = ur; k2["depth"][pos2[todo]] = dp
            k2["octave"][pos2[todo]] = np.clip(o2, 0, 7)
            m = np.stack([idx1, pos2], 1).astype(np.int32)
            mg = triangulate_pair(kf1, keys1, kf2, k2, m, monocular)["margin"]
            todo = np.flatnonzero(~(mg > MARGIN)) if not pair_gate(kf1, kf2, monocular)[0] else np.zeros(0, np.int64)
        assert len(todo) == 0 or not enforce_margin, "make_scene could not move every match away from its thresholds"
        kf2s.append(kf2); keys2s.append(k2); matches.append(np.stack([idx1, pos2], 1).astype(np.int32))
    pb = problem(kf1, keys1, kf2s, keys2s, matches, monocular)
    pb["X"] = X
    return pb


def crafted_scenes():
    """Two hand-made problems on a power-of-two camera (fx = fy = 512, cx = 640, cy = 192, mb = 0.5, mbf = 256: 1/fx is exact)
    with identity rotations, and for every match the expected (status, source) worked out by hand - see the comments.
    Returns [(problem, expected status list, expected source list, notes)]."""
    cam = dict(fx=512.0, fy=512.0, cx=640.0, cy=192.0, mb=0.5)
    I = np.eye(3)
    kf = lambda R, C: make_kf(R, -np.asarray(R, F64) @ np.asarray(C, F64), **cam)

    def keys(rows):
        """rows: (x, y, ur, depth, octave)"""
        a = np.array(rows, F64).reshape(-1, 5)
        return dict(xy=a[:, :2].astype(F32), raw_xy=a[:, :2].astype(F32), ur=a[:, 2].astype(F32), depth=a[:, 3].astype(F32),
                    octave=a[:, 4].astype(np.int32))

    px = lambda X, C: (640.0 + 512.0 * (X[0] - C[0]) / (X[2] - C[2]), 192.0 + 512.0 * (X[1] - C[1]) / (X[2] - C[2]))
    P = (0.5, 0.0, 8.0)                                                         # the world point most matches look at
    Ca, Cb, Cc = (1.0, 0.0, 0.0), (1.0, 0.0, 10.0), (0.0, 0.0, 1.0)
    Q = (0.1, 0.0, 8.0)
    k1 = keys([
        (640, 192, 640 - 256 * 0.25, 4, 0),        # 0 DIST_ZERO: un-projects to (0,0,4), the centre of the scaled neighbour
        (*px(P, (0, 0, 0)), -1, -1, 0),            # 1 NEW by triangulation: X = (0.5, 0, 8)
        (608, 192, -1, -1, 0),                     # 2 Z1: rays swapped against 1, they meet at (0.5, 0, -8)
        (672, 195, -1, -1, 0),                     # 3 REPROJ1: 6 px of vertical disparity, 3 px of error on each side
        (672, 195, -1, -1, 4),                     # 4 REPROJ2: the same, but level 4 here allows 5.991*1.2^8 = 25.8 px^2
        (*px(P, (0, 0, 0)), -1, -1, 0),            # 5 SCALE: level 0 against level 5, equal distances
        (640, 192, -1, -1, 0),                     # 6 LOW_PARALLAX: 1 km away, two mono keypoints
        (600, 192, 590, 0, 0),                     # 7 NO_DEPTH: stereo keypoint with depth 0 (cosine -1), UnprojectStereo refuses
        (640, 192, -1, -1, 0),                     # 8 Z2: (0,0,4), in front of keyframe 1 and 6 m BEHIND the neighbour at (1,0,10)
        (*px(Q, (0, 0, 0)), -1, -1, 0),            # 9 NEW from the neighbour's stereo keypoint (forward motion: little parallax)
        (px(Q, (0, 0, 0))[0], 192, px(Q, (0, 0, 0))[0] - 32, 8, 0),   # 10 NEW from keyframe 1's stereo keypoint (depth 8)
        (700, 200, -1, -1, 0),                     # 11 in the skipped pair
    ])
    n0 = make_kf(2 * I, (0, 0, -2), **cam)                                      # NOT a rotation: Ow = -Rwc*tcw = (0,0,4), yet z2 = 2*4-2 = 6
    k2_0 = keys([(640, 192, -1, -1, 0)])
    k2_a = keys([(*px(P, Ca), -1, -1, 0), (672, 192, -1, -1, 0), (608, 189, -1, -1, 0), (608, 189, -1, -1, 0), (*px(P, Ca), -1, -1, 5),
                 (640 - 512 / 1000.0, 192, -1, -1, 0), (560, 192, -1, -1, 0)])
    k2_b = keys([(*px((0, 0, 4), Cb), -1, -1, 0)])
    qc = px(Q, Cc)
    k2_c = keys([(qc[0], qc[1], qc[0] - 256 / 7.0, 7, 0), (qc[0], qc[1], -1, -1, 0)])
    k2_d = keys([(690, 200, -1, -1, 0)])
    pb1 = problem(kf(I, (0, 0, 0)), k1, [n0, kf(I, Ca), kf(I, Cb), kf(I, Cc), kf(I, (0.25, 0, 0))], [k2_0, k2_a, k2_b, k2_c, k2_d],
                  [[(0, 0)], [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 6)], [(8, 0)], [(9, 0), (10, 1)], [(11, 0)]], False)
    st1 = [DIST_ZERO, NEW, Z1, REPROJ1, REPROJ2, SCALE, LOW_PARALLAX, NO_DEPTH, Z2, NEW, NEW, PAIR_SKIPPED]
    src1 = [SRC_STEREO1, 0, 0, 0, 0, 0, 0, SRC_STEREO1, 0, SRC_STEREO2, SRC_STEREO1, 0]
    x1 = {1: P, 9: Q, 10: Q}
    # W_ZERO: cameras at (-1,0,0) and (1,0,0), both keypoints in the same column (equal xn.x) 60 px apart vertically.  Column 3 of A
    # is (-1, 0, 1, 0), exactly orthogonal to the other three ((-1,0,-1,0), (0,-1,0,-1), (p,q1,p,q2)), so A^T A splits into a 3x3
    # block and the entry 2; the Jacobi never mixes them, the block holds the smallest eigenvalue and x3D[3] is exactly 0.
    k1w = keys([(740, 222, -1, -1, 0)])
    k2w = keys([(740, 162, -1, -1, 0)])
    pb2 = problem(kf(I, (-1, 0, 0)), k1w, [kf(I, (1, 0, 0))], [k2w], [[(0, 0)]], False)
    return [(pb1, st1, src1, x1), (pb2, [W_ZERO], [0], {})]
