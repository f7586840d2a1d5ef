// lld_loopclosing_adapter.cc — see lld_loopclosing_adapter.h.
#include "lld_loopclosing_adapter.h"

#include <cstring>
#include <set>

namespace lld_adapter {

namespace {

// Keyframes numbered in std::less<KeyFrame*> order: the slots of one call
struct KfSlots {
  std::map<KeyFrame*, int32_t> slot;
  std::vector<KeyFrame*> kfs;
  void add(KeyFrame* pKF) { if (pKF) slot[pKF] = 0; }
  void number() { kfs.clear(); int32_t i = 0; for (std::map<KeyFrame*, int32_t>::iterator it = slot.begin(); it != slot.end(); ++it) { it->second = i++; kfs.push_back(it->first); } }
  int32_t of(KeyFrame* pKF) const { return slot.find(pKF)->second; }
};

void pose_rows(const lld_slam::Mat& T, float* out) { for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) out[4 * r + c] = T.at<float>(r, c); }
lld_slam::Mat pose_mat(const float* rows) {                   // cv::Mat::eye(4,4,CV_32F) with [R|t] on top (Converter::toCvSE3)
  lld_slam::Mat T(4, 4);
  for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) T.at<float>(r, c) = rows[4 * r + c];
  T.at<float>(3, 3) = 1.f;
  return T;
}
void sim3_flat(const Sim3& S, double* d) { for (int i = 0; i < 4; i++) d[i] = S.q[i]; for (int i = 0; i < 3; i++) d[4 + i] = S.t[i]; d[7] = S.s; }
Sim3 sim3_unflat(const double* d) { Sim3 S; for (int i = 0; i < 4; i++) S.q[i] = d[i]; for (int i = 0; i < 3; i++) S.t[i] = d[4 + i]; S.s = d[7]; return S; }

// The point table of lld_loop_correct / lld_essential_graph_apply for `pts`; `skip[i]`: the rule never reads point i's reference
// keyframe.  Every observing and reference keyframe must have a slot already.  out.* take the points' current values.
void gather_points(const std::vector<MapPoint*>& pts, const std::vector<uint8_t>& skip, const KfSlots& K, lld_amd::MapCorrPoints& P,
                   std::vector<float>& normal, std::vector<float>& mn, std::vector<float>& mx) {
  const size_t n = pts.size();
  P.pos.assign(3 * n, 0.f); P.bad.assign(n, 0); P.ref_kf.assign(n, 0); P.ref_level.assign(n, 0); P.obs_start.assign(1, 0); P.obs_kf.clear();
  normal.assign(3 * n, 0.f); mn.assign(n, 0.f); mx.assign(n, 0.f);
  KeyFrame* scales = nullptr;
  for (size_t i = 0; i < n; ++i) {
    MapPoint* pMP = pts[i];
    P.bad[i] = pMP->isBad() ? 1 : 0;
    const float* X = pMP->mWorldPos.ptr<float>();
    P.pos[3 * i] = X[0]; P.pos[3 * i + 1] = X[1]; P.pos[3 * i + 2] = X[2];
    if (!pMP->mNormalVector.empty()) std::memcpy(&normal[3 * i], pMP->mNormalVector.ptr<float>(), 12);
    mn[i] = pMP->mfMinDistance; mx[i] = pMP->mfMaxDistance;
    if (!P.bad[i]) {
      std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
      for (std::map<KeyFrame*, size_t>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) P.obs_kf.push_back(K.of(mit->first));
      KeyFrame* pRefKF = pMP->mpRefKF;
      if (!skip[i] && !observations.empty() && pRefKF) {
        P.ref_kf[i] = K.of(pRefKF);
        P.ref_level[i] = pRefKF->mvKeysUn[observations[pRefKF]].octave;   // operator[]: an absent pRefKF yields keypoint 0 (MapPoint.cc:361)
        if (!scales) scales = pRefKF;
      }
    }
    P.obs_start.push_back((int32_t)P.obs_kf.size());
  }
  if (scales) P.level_scale.assign(scales->mvScaleFactors.begin(), scales->mvScaleFactors.begin() + scales->mnScaleLevels);
  else P.level_scale.assign(1, 1.f);           // nothing reads it
}

void add_point_keyframes(MapPoint* pMP, KfSlots& K) {
  if (pMP->isBad()) return;
  const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
  for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit) K.add(mit->first);
  K.add(pMP->mpRefKF);
}

void scatter_normal(MapPoint* pMP, const float* normal, float mn, float mx) {   // MapPoint.cc:367-369
  pMP->mfMaxDistance = mx; pMP->mfMinDistance = mn; pMP->mNormalVector = lld_slam::Mat(3, 1, normal);
}

}  // namespace

int CorrectLoopPoses(const lld_amd::Context& ctx, KeyFrame* mpCurrentKF, const Sim3& mg2oScw, const std::vector<KeyFrame*>& mvpCurrentConnectedKFs,
                     KeyFrameAndPose& CorrectedSim3, KeyFrameAndPose& NonCorrectedSim3, std::vector<float>* scw_f32) {
  // the connected keyframes in the order CorrectedSim3 iterates: pointer order
  std::set<KeyFrame*> connected(mvpCurrentConnectedKFs.begin(), mvpCurrentConnectedKFs.end());
  connected.insert(mpCurrentKF);
  KfSlots K;
  std::map<MapPoint*, int32_t> point_slot;
  std::vector<MapPoint*> pts;
  lld_amd::LoopCorrectBatch b;
  b.kf_start.assign(1, 0);
  for (std::set<KeyFrame*>::iterator it = connected.begin(); it != connected.end(); ++it) {
    K.add(*it);
    const std::vector<MapPoint*> vpMPsi = (*it)->GetMapPointMatches();          // (:482)
    for (size_t iMP = 0; iMP < vpMPsi.size(); iMP++) {
      MapPoint* pMPi = vpMPsi[iMP];
      if (!pMPi) continue;
      std::map<MapPoint*, int32_t>::iterator f = point_slot.find(pMPi);
      if (f == point_slot.end()) { f = point_slot.insert(std::make_pair(pMPi, (int32_t)pts.size())).first; pts.push_back(pMPi); add_point_keyframes(pMPi, K); }
      b.kf_point.push_back(f->second);
    }
    b.kf_start.push_back((int32_t)b.kf_point.size());
  }
  K.number();
  b.cur = 0;
  for (std::set<KeyFrame*>::iterator it = connected.begin(); it != connected.end(); ++it) {
    if (*it == mpCurrentKF) b.cur = (int32_t)b.conn.size();
    b.conn.push_back(K.of(*it));
  }
  b.kf_tcw.resize(12 * K.kfs.size());
  for (size_t k = 0; k < K.kfs.size(); ++k) pose_rows(K.kfs[k]->GetPose(), &b.kf_tcw[12 * k]);
  sim3_flat(mg2oScw, b.scw);
  const size_t n = pts.size();
  b.already.resize(n);
  std::vector<uint8_t> skip(n);
  for (size_t i = 0; i < n; ++i) {
    b.already[i] = pts[i]->mnCorrectedByKF == mpCurrentKF->mnId ? 1 : 0;        // (:490)
    skip[i] = b.already[i] || pts[i]->isBad();
  }
  lld_amd::LoopCorrectOutput o;
  gather_points(pts, skip, K, b.points, o.normal, o.min_distance, o.max_distance);
  o.pos = b.points.pos;
  lld_amd::CorrectLoop(ctx, b, o);

  int corrected = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!(o.updated[i] & LLD_MAPCORR_MOVED)) continue;
    corrected++;
    pts[i]->SetWorldPos(lld_slam::Mat(3, 1, &o.pos[3 * i]));                   // (:499)
    pts[i]->mnCorrectedByKF = mpCurrentKF->mnId;                                // (:500)
    pts[i]->mnCorrectedReference = K.kfs[b.conn[o.corrected_by[i]]]->mnId;      // (:501)
    if (o.updated[i] & LLD_LANDMARK_NORMAL_DEPTH) scatter_normal(pts[i], &o.normal[3 * i], o.min_distance[i], o.max_distance[i]);   // (:502)
  }
  if (scw_f32) *scw_f32 = o.scw_f32;
  for (size_t r = 0; r < b.conn.size(); ++r) {
    KeyFrame* pKFi = K.kfs[b.conn[r]];
    CorrectedSim3[pKFi] = sim3_unflat(&o.corrected_sim3[8 * r]);                // (:441, :463)
    NonCorrectedSim3[pKFi] = sim3_unflat(&o.non_corrected_sim3[8 * r]);         // (:470)
    pKFi->SetPose(pose_mat(&o.tiw_corrected[12 * r]));                          // (:514)
    pKFi->Ow = lld_slam::Mat(3, 1, &o.ow_corrected[3 * r]);
  }
  return corrected;
}

int ApplyEssentialGraph(const lld_amd::Context& ctx, Map* pMap, KeyFrame* pCurKF, const KeyFrameAndPose& vScw, const KeyFrameAndPose& vCorrectedSiw) {
  const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
  KfSlots K;
  for (size_t i = 0; i < vpKFs.size(); ++i) K.add(vpKFs[i]);
  for (size_t i = 0; i < vpMPs.size(); ++i) add_point_keyframes(vpMPs[i], K);
  K.number();
  lld_amd::EssentialGraphApplyBatch b;
  const size_t nk = K.kfs.size(), n = vpMPs.size();
  b.sim3_before.resize(8 * nk); b.sim3_after.resize(8 * nk);
  for (size_t k = 0; k < nk; ++k) {             // every keyframe a live point reads, and every keyframe of the map, was a vertex
    KeyFrameAndPose::const_iterator bi = vScw.find(K.kfs[k]), ai = vCorrectedSiw.find(K.kfs[k]);
    if (bi == vScw.end() || ai == vCorrectedSiw.end()) return -1;   // its new centre would be unknown: nothing is called, nothing written
    sim3_flat(bi->second, &b.sim3_before[8 * k]);
    sim3_flat(ai->second, &b.sim3_after[8 * k]);
  }
  std::map<unsigned long, int32_t> slot_of_id;
  for (size_t k = 0; k < nk; ++k) slot_of_id[K.kfs[k]->mnId] = (int32_t)k;
  b.corr_kf.assign(n, 0);
  std::vector<uint8_t> skip(n);
  for (size_t i = 0; i < n; ++i) {
    MapPoint* pMP = vpMPs[i];
    skip[i] = pMP->isBad() ? 1 : 0;
    if (skip[i]) continue;
    if (pMP->mnCorrectedByKF == pCurKF->mnId) b.corr_kf[i] = slot_of_id[pMP->mnCorrectedReference];   // (:1631-1634)
    else b.corr_kf[i] = K.of(pMP->GetReferenceKeyFrame());                                            // (:1637-1638)
  }
  lld_amd::EssentialGraphApplyOutput o;
  gather_points(vpMPs, skip, K, b.points, o.normal, o.min_distance, o.max_distance);
  o.pos = b.points.pos;
  lld_amd::ApplyEssentialGraph(ctx, b, o);
  for (size_t k = 0; k < nk; ++k) {
    K.kfs[k]->SetPose(pose_mat(&o.tiw[12 * k]));                                // (:1619)
    K.kfs[k]->Ow = lld_slam::Mat(3, 1, &o.ow[3 * k]);
  }
  int corrected = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!(o.updated[i] & LLD_MAPCORR_MOVED)) continue;
    corrected++;
    vpMPs[i]->SetWorldPos(lld_slam::Mat(3, 1, &o.pos[3 * i]));                 // (:1650)
    if (o.updated[i] & LLD_LANDMARK_NORMAL_DEPTH) scatter_normal(vpMPs[i], &o.normal[3 * i], o.min_distance[i], o.max_distance[i]);   // (:1652)
  }
  return corrected;
}

int UpdateMapAfterGlobalBA(const lld_amd::Context& ctx, Map* pMap, unsigned long nLoopKF) {
  const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
  KfSlots K;
  for (size_t i = 0; i < vpKFs.size(); ++i) { K.add(vpKFs[i]); K.add(vpKFs[i]->GetParent()); }
  for (size_t i = 0; i < pMap->mvpKeyFrameOrigins.size(); ++i) K.add(pMap->mvpKeyFrameOrigins[i]);
  for (size_t i = 0; i < vpMPs.size(); ++i) if (!vpMPs[i]->isBad()) K.add(vpMPs[i]->GetReferenceKeyFrame());
  K.number();
  const size_t nk = K.kfs.size(), n = vpMPs.size();
  lld_amd::GlobalBAApplyBatch b;
  b.kf_tcw.resize(12 * nk); b.kf_tcw_gba.assign(12 * nk, 0.f); b.kf_in_gba.resize(nk); b.parent.resize(nk);
  for (size_t k = 0; k < nk; ++k) {
    KeyFrame* pKF = K.kfs[k];
    pose_rows(pKF->GetPose(), &b.kf_tcw[12 * k]);
    b.kf_in_gba[k] = pKF->mnBAGlobalForKF == nLoopKF ? 1 : 0;                   // (:689)
    if (b.kf_in_gba[k]) pose_rows(pKF->mTcwGBA, &b.kf_tcw_gba[12 * k]);
    b.parent[k] = pKF->GetParent() ? K.of(pKF->GetParent()) : -1;
  }
  for (size_t i = 0; i < pMap->mvpKeyFrameOrigins.size(); ++i) b.origins.push_back(K.of(pMap->mvpKeyFrameOrigins[i]));   // (:679)
  b.pos.assign(3 * n, 0.f); b.pos_gba.assign(3 * n, 0.f); b.bad.resize(n); b.in_gba.resize(n); b.ref_kf.assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    MapPoint* pMP = vpMPs[i];
    b.bad[i] = pMP->isBad() ? 1 : 0;
    b.in_gba[i] = pMP->mnBAGlobalForKF == nLoopKF ? 1 : 0;                      // (:714)
    std::memcpy(&b.pos[3 * i], pMP->mWorldPos.ptr<float>(), 12);
    if (b.in_gba[i]) std::memcpy(&b.pos_gba[3 * i], pMP->mPosGBA.ptr<float>(), 12);
    else if (!b.bad[i]) b.ref_kf[i] = K.of(pMP->GetReferenceKeyFrame());        // (:722)
  }
  lld_amd::GlobalBAApplyOutput o;
  o.pos = b.pos;
  lld_amd::ApplyGlobalBA(ctx, b, o);
  for (size_t k = 0; k < nk; ++k) {
    if (!o.visited[k]) continue;
    KeyFrame* pKF = K.kfs[k];
    if (!b.kf_in_gba[k]) { pKF->mTcwGBA = pose_mat(&o.tcw_new[12 * k]); pKF->mnBAGlobalForKF = nLoopKF; }   // (:692-693)
    pKF->mTcwBefGBA = pose_mat(&o.tcw_before[12 * k]);                          // (:699)
    pKF->SetPose(pKF->mTcwGBA);                                                 // (:700)
    pKF->Ow = lld_slam::Mat(3, 1, &o.ow_new[3 * k]);
  }
  int moved = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!o.moved[i]) continue;
    moved++;
    vpMPs[i]->SetWorldPos(lld_slam::Mat(3, 1, &o.pos[3 * i]));                 // (:717, :737)
  }
  return moved;
}

}  // namespace lld_adapter
