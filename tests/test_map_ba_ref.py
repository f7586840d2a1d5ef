"""tests/map_ba_ref.py, the restatement the device window is held to, is itself held to two things here: a literal transcription of the
reference's walk (src/Optimizer.cc:938-1218 as adapters/lld_optimizer_adapter.cc:32-151 restates it) on objects with visit marks, and the
windows of tests/map_ba_scenes.py that were worked out by hand.  CPU only."""
import numpy as np
import pytest

import map_ba_ref as R
import map_ba_scenes as S
from lld_slam_amd import abi, host


def se3(T):
    return host.se3_from_tcw_f32(abi.product(), T)


# ---------------------------------------------------------------------------------------------------------------- the walk on objects
class Obj:
    def __init__(self, **kw):
        self.mnBALocalForKF = self.mnBAFixedForKF = None
        self.__dict__.update(kw)


def objects(m):
    """KeyFrame / MapPoint / MapLine objects of a map dict.  A slot never set is a NULL entry of a row (a point) or a bad object (a line, a
    keyframe).  GetObservations() iterates in the stored order."""
    K = {s: Obj(slot=s, mnId=k.get("mn_id", 0), bad=bool(k["bad"]), k=k) for s, k in m["keyframes"].items()}
    for o in list(m["points"].values()) + list(m["lines"].values()):
        for kf, _ in o["obs"] or ():
            if kf not in K:
                K[kf] = Obj(slot=kf, mnId=0, bad=True, k=dict(points=[], lines=[]))
    P = {s: Obj(slot=s, bad=bool(p["bad"]), p=p) for s, p in m["points"].items()}
    L = {s: Obj(slot=s, bad=bool(l["bad"]), l=l) for s, l in m["lines"].items()}
    for o in K.values():
        o.points = [P.get(p) if p >= 0 else None for p in o.k["points"]]
        o.lines = [L.get(l) if l >= 0 else None for l in o.k["lines"]]
    for o in list(P.values()) + list(L.values()):
        o.obs = [(K[kf], idx) for kf, idx in (o.p["obs"] if hasattr(o, "p") else o.l["obs"])]
    return K, P, L


def walk(m, kf_slots, sig):
    """The visit mark is a token of the call, not pKF->mnId: the reference's marks start at 0, so a call with pKF->mnId == 0 would find every
    object marked - LocalMapping never makes that call, and the library's marks are per call."""
    K, P, L = objects(m)
    pKF = K[kf_slots[0]]
    mark = object()
    lLocalKeyFrames = [pKF]
    pKF.mnBALocalForKF = mark
    for s in kf_slots[1:]:
        pKFi = K[s]
        pKFi.mnBALocalForKF = mark
        if not pKFi.bad:
            lLocalKeyFrames.append(pKFi)
    lLocalMapPoints, lLocalMapLines = [], []
    for kf in lLocalKeyFrames:
        for pMP in kf.points:
            if pMP is not None and not pMP.bad and pMP.mnBALocalForKF is not mark:
                lLocalMapPoints.append(pMP); pMP.mnBALocalForKF = mark
        for pML in kf.lines:
            if pML is None or pML.bad:
                continue
            if pML.l["n_obs"] < 4:
                continue
            if pML.mnBALocalForKF is not mark:
                lLocalMapLines.append(pML); pML.mnBALocalForKF = mark
    lFixedCameras = []
    for lm in lLocalMapPoints + lLocalMapLines:
        for pKFi, _ in lm.obs:
            if pKFi.mnBALocalForKF is not mark and pKFi.mnBAFixedForKF is not mark:
                pKFi.mnBAFixedForKF = mark
                if not pKFi.bad:
                    lFixedCameras.append(pKFi)
    cams = sorted((kf for kf in lLocalKeyFrames if kf.mnId != 0), key=lambda kf: kf.mnId)
    n_free = len(cams)
    cams += [kf for kf in lLocalKeyFrames if kf.mnId == 0]
    cams += lFixedCameras
    cam_index = {id(kf): i for i, kf in enumerate(cams)}
    w = dict(marked_bad=sorted(kf.slot for kf in K.values() if kf.bad and kf.mnBAFixedForKF is mark), n_free_cams=n_free, n_local_cams=len(lLocalKeyFrames), cam_slot=[kf.slot for kf in cams], cam_qt=[se3(kf.k["Tcw"]) for kf in cams],
             point_slot=[p.slot for p in lLocalMapPoints], pt_xyz=[], pt_obs_start=[0], pt_obs_cam=[], pt_obs_uvr=[], pt_obs_inv_sigma2=[],
             line_slot=[l.slot for l in lLocalMapLines], line_x0=[], line_dir=[], ln_obs_start=[0], ln_obs_cam=[], ln_obs_left=[], ln_obs_right=[], ln_obs_octave=[])
    for pMP in lLocalMapPoints:
        w["pt_xyz"].append([float(v) for v in np.asarray(pMP.p["pos"], np.float32)])
        for pKFi, idx in pMP.obs:
            if pKFi.bad:
                continue
            w["pt_obs_cam"].append(cam_index[id(pKFi)])
            w["pt_obs_uvr"].append([float(v) for v in pKFi.k["uvr"][idx]])
            w["pt_obs_inv_sigma2"].append(float(sig[pKFi.k["octave"][idx]]))
        w["pt_obs_start"].append(len(w["pt_obs_cam"]))
    for pML in lLocalMapLines:
        w["line_x0"].append(list(pML.l["x0"])); w["line_dir"].append(list(pML.l["dir"]))
        by_id = {}
        for pKFi, idx in pML.obs:
            if not pKFi.bad:
                by_id.setdefault(pKFi.mnId, (pKFi, idx))
        for mn in sorted(by_id):
            pKFcurr, idx = by_id[mn]
            w["ln_obs_cam"].append(cam_index[id(pKFcurr)])
            w["ln_obs_left"].append([float(v) for v in pKFcurr.k["kl_left"][idx]])
            w["ln_obs_right"].append([float(v) for v in pKFcurr.k["kl_right"][idx]])
            w["ln_obs_octave"].append([int(v) for v in pKFcurr.k["kl_octave"][idx]])
        w["ln_obs_start"].append(len(w["ln_obs_cam"]))
    return w


def same(ref, w):
    assert ref["status"] == 0 and ref["marked_bad"] == w["marked_bad"]
    assert (ref["n_free_cams"], ref["n_local_cams"]) == (w["n_free_cams"], w["n_local_cams"])
    for name in R.ARRAYS:
        got = ref[name]
        want = np.array(w[name], got.dtype).reshape(got.shape if got.size else (-1,) + got.shape[1:])
        assert got.shape == want.shape and np.array_equal(got, want), name
    assert (ref["n_cams"], ref["n_points"], ref["n_pt_obs"], ref["n_lines"], ref["n_ln_obs"]) == (
        len(w["cam_slot"]), len(w["point_slot"]), len(w["pt_obs_cam"]), len(w["line_slot"]), len(w["ln_obs_cam"]))


@pytest.mark.parametrize("seed", range(8))
def test_restatement_equals_the_walk_on_random_maps(seed):
    m, q = S.random_map(seed)
    ref = R.ba_window(m, q, S.SIGMA2, se3)
    same(ref, walk(m, q, S.SIGMA2))
    assert ref["n_points"] > 50 and ref["n_lines"] > 3 and ref["n_cams"] > ref["n_local_cams"] > 2     # the maps exercise every list


@pytest.mark.parametrize("name", sorted(S.NAMED))
def test_restatement_equals_the_walk_on_the_named_scenes(name):
    m, q = S.NAMED[name]()
    same(R.ba_window(m, q, S.SIGMA2, se3), walk(m, q, S.SIGMA2))


WIDE = [dict(n_points=257), dict(n_observers=65), dict(n_line_observers=65), dict(n_local=40), dict(n_points=8193), dict(n_points=8190, n_lines=5), dict(n_lines=257),
        dict(n_lines=513), dict(n_local_spread=600), dict(n_fixed=300)]


@pytest.mark.parametrize("kw", WIDE, ids=lambda k: "-".join("%s%d" % i for i in k.items()))
def test_restatement_equals_the_walk_on_the_wide_scenes(kw):
    m, q = S.wide(**kw)
    ref = R.ba_window(m, q, S.SIGMA2, se3)
    same(ref, walk(m, q, S.SIGMA2))
    # the scenes past the kernels' widths are as wide as they were made to be
    if kw.get("n_points", 0) > 8000: assert ref["n_points"] == kw["n_points"] and ref["n_lines"] == kw.get("n_lines", 0) and ref["marked_bad"] == [1]
    if "n_lines" in kw and "n_points" not in kw:
        assert ref["n_lines"] == kw["n_lines"] + 2 and len(m["keyframes"][0]["lines"]) > kw["n_lines"]
        local = set(ref["line_slot"].tolist())                       # every tile of 256 row entries adds local lines behind the tiles before it
        row = m["keyframes"][0]["lines"]
        assert all(len(local & set(row[t:t + 256]) - set(row[:t])) > 0 for t in range(0, len(row), 256)) and len(row) > 256 * (kw["n_lines"] // 256)
    if "n_local_spread" in kw: assert ref["n_local_cams"] > 512 and ref["n_points"] == 2 * ref["n_local_cams"] and ref["n_lines"] == ref["n_local_cams"]
    if "n_fixed" in kw: assert ref["n_cams"] - ref["n_local_cams"] > 256 and len(ref["marked_bad"]) > 16


@pytest.mark.parametrize("name", sorted(S.HAND))
def test_restatement_gives_the_windows_worked_out_by_hand(name):
    m, q = S.NAMED[name]()
    r = R.ba_window(m, q, S.SIGMA2, se3)
    e = S.HAND[name]
    assert r["status"] == 0
    for k in ("cam_slot", "point_slot", "pt_obs_start", "pt_obs_cam", "line_slot", "ln_obs_start", "ln_obs_cam"):
        assert r[k].tolist() == e[k], k
    assert (r["n_free_cams"], r["n_local_cams"]) == (e["n_free_cams"], e["n_local_cams"])
    assert r["pt_obs_uvr"][:, 0].tolist() == e["pt_u"] and r["pt_obs_inv_sigma2"].tolist() == e["pt_sig"]
    assert r["pt_obs_uvr"][:, 1].tolist() == [u + 0.5 for u in e["pt_u"]] and r["pt_obs_uvr"][:, 2].tolist() == [u - 2 for u in e["pt_u"]]
    assert r["cam_qt"].tolist() == [[0, 0, 0, 1, s, 2 * s, 3 * s] for s in e["cam_slot"]]
    assert r["pt_xyz"].tolist() == [[p, p + 0.5, p + 0.25] for p in e["point_slot"]]
    assert r["line_x0"].tolist() == [[l, 0.1 * l, 2.0] for l in e["line_slot"]] and r["line_dir"].tolist() == [[0.0, 1.0, 0.001 * l] for l in e["line_slot"]]
    if e["line_slot"]:
        assert r["ln_obs_left"][:, 0].tolist() == e["ln_left_xs"] and r["ln_obs_right"][:, 0].tolist() == e["ln_right_xs"]
        assert r["ln_obs_octave"].tolist() == e["ln_obs_octave"]


def test_status_and_refusals():
    m, q = S.bad_neighbour()
    for bad_q in ([], [0, 0], [0, 9], [-1], list(range(R.MAX_LOCAL + 1))):
        with pytest.raises(R.Refused):
            R.ba_window(m, bad_q, S.SIGMA2, se3)
    zero = dict({c: 0 for c in R.COUNTS}, status=R.NO_FEATURE_DATA)
    for spoil in ("features", "keypoints", "index", "octave", "unindexed", "line_row", "line_index"):
        m, q = S.fixed_through_line()
        if spoil == "features": del m["keyframes"][2]["uvr"]
        if spoil == "keypoints": m["keyframes"][2]["octave"] = None
        if spoil == "index": m["points"][0]["obs"][2] = (2, 2)
        if spoil == "octave": m["keyframes"][1]["octave"][0] = S.N_LEVELS
        if spoil == "unindexed": m["points"][0]["indexed"] = False
        if spoil == "line_row": m["lines"][0]["obs"] = None
        if spoil == "line_index": m["lines"][0]["obs"][0] = (3, 2)
        assert R.ba_window(m, q, S.SIGMA2, se3) == zero, spoil


def test_bad_keyframes_marked_fixed():
    """what lld_map_local_ba reports as marked_bad_slot: a bad neighbour is marked local and so is not among them; a bad observer and a
    slot never set are"""
    for name, want in (("bad_neighbour", []), ("bad_observer_inside", [1]), ("never_set_observer", [1, 4])):
        m, q = S.NAMED[name]()
        assert R.ba_window(m, q, S.SIGMA2, se3)["marked_bad"] == want, name
