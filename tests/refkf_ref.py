"""TEST INFRASTRUCTURE ONLY: Tracking::TrackReferenceKeyFrame (src/Tracking.cc:773-817) followed by TrackLocalMap on ONE Frame, on the CPU,
composed from what the other checkers already are: oracle_tracking's Frame, bow_ref's transform for both FeatureVectors, the oracle's
SearchByBoW(KeyFrame*, Frame&), its PoseOptimization and its TrackLocalMap.  Nothing of the device chain enters."""
from __future__ import annotations

import numpy as np

import bow_ref
import oracle_orbsearch as OS
import oracle_tracking as OT
import refkf_scenes as RS


def common_nodes(kf, fv):
    """The node merge of ORBmatcher.cc:180-264 as the CSR lists the oracle's search takes: the nodes both FeatureVectors hold, ascending."""
    common, ik, i_f = np.intersect1d(np.asarray(kf["node"]), np.asarray(fv["node"]), assume_unique=True, return_indices=True)
    ks, kidx, fs, fidx = [0], [], [0], []
    for a, b in zip(ik, i_f):
        kidx.extend(np.asarray(kf["feature"])[kf["node_start"][a]:kf["node_start"][a + 1]].tolist()); ks.append(len(kidx))
        fidx.extend(np.asarray(fv["feature"])[fv["node_start"][b]:fv["node_start"][b + 1]].tolist()); fs.append(len(fidx))
    return dict(n_nodes=len(common), start1=np.array(ks, np.int32), idx1=np.array(kidx, np.int32), start2=np.array(fs, np.int32), idx2=np.array(fidx, np.int32))


def frame_bow(S):
    """Frame::ComputeBoW of the scene's frame (bow_ref)."""
    return bow_ref.transform(S["tree"], S["sc"]["frame"].desc, S["levelsup"])


def search(S, check_orientation=True):
    """(nmatches, slot [nt]: keyframe keypoint whose MapPoint the frame's keypoint received, or -1)."""
    kf = S["kf"]
    nd = common_nodes(kf, frame_bow(S))
    valid = (np.asarray(kf["point_id"]) >= 0).astype(np.uint8)
    n, slot = OS.search_by_bow_frame(RS.keyframe_frame(kf), S["sc"]["frame"], nd["n_nodes"], nd["start1"], nd["idx1"], nd["start2"], nd["idx2"], valid, 0.7,
                                     check_orientation)
    return int(n), slot


def stage1(S, gamma=0.5):
    """TrackReferenceKeyFrame past its failure exit, like the device chain: (Frame, record of stage 1)."""
    sc, kf = S["sc"], S["kf"]
    fr = OT.new_frame(sc)
    n, slot = search(S)
    for k in np.nonzero(slot >= 0)[0]:
        q = int(slot[k])
        fr.kp_has[k] = True; fr.kp_world[k] = np.asarray(kf["world_pos"], np.float32)[q]; fr.kp_id[k] = int(kf["point_id"][q]); fr.kp_obs[k] = int(kf["has_obs"][q])
    fr.set_pose_matrix(S["Tcw_last"])                                     # mCurrentFrame.SetPose(mLastFrame.mTcw), :789
    out, n_edges = fr.pose_optimization(gamma)
    rec = fr.record(out, n_edges, dict(n_search_first=n, n_search=n, used_wide=0, n_point_edges=int(fr.problems[-1].n_points), n_in_view=0))
    bad = fr.kp_has & (fr.kp_out != 0)                                    # :796-814
    fr.seen_points.update(int(i) for i in fr.kp_id[bad])
    fr.kp_has[bad] = False; fr.kp_id[bad] = -1; fr.kp_out[bad] = 0
    rec.update(n_points=int(fr.kp_has.sum()), n_points_map=int((fr.kp_has & (fr.kp_obs != 0)).sum()), n_discarded=int(bad.sum()), n_lines=0)
    return fr, rec


def track(S, gamma=0.5):
    """(record of TrackReferenceKeyFrame, record of TrackLocalMap)."""
    fr, rec1 = stage1(S, gamma)
    rec2 = OT.track_local_map(S["sc"], fr, gamma)
    return rec1, rec2
