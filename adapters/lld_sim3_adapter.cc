// lld_sim3_adapter.cc — see lld_sim3_adapter.h.
#include "lld_sim3_adapter.h"

namespace lld_adapter {

lld_amd::Sim3Problem GatherSim3(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, bool bFixScale,
                                uint32_t seed) {
  lld_amd::Sim3Problem p;
  const std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
  const int mN1 = (int)vpMatched12.size();
  for (int i1 = 0; i1 < mN1; i1++) {                                         // Sim3Solver.cc:64-101
    if (!vpMatched12[i1]) continue;
    MapPoint* pMP1 = vpKeyFrameMP1[i1];
    MapPoint* pMP2 = vpMatched12[i1];
    if (!pMP1) continue;
    if (pMP1->isBad() || pMP2->isBad()) continue;
    const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
    const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (indexKF1 < 0 || indexKF2 < 0) continue;
    p.sigma2_1.push_back(pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave]);
    p.sigma2_2.push_back(pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave]);
    p.index1.push_back(i1);
    const Mat X1 = pMP1->GetWorldPos(), X2 = pMP2->GetWorldPos();
    for (int r = 0; r < 3; ++r) { p.xyz1.push_back(X1.at<float>(r)); p.xyz2.push_back(X2.at<float>(r)); }
  }
  p.n1 = mN1;
  const Mat R1 = pKF1->GetRotation(), t1 = pKF1->GetTranslation(), R2 = pKF2->GetRotation(), t2 = pKF2->GetTranslation();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) { p.Rcw1[3 * r + c] = R1.at<float>(r, c); p.Rcw2[3 * r + c] = R2.at<float>(r, c); }
    p.tcw1[r] = t1.at<float>(r); p.tcw2[r] = t2.at<float>(r);
  }
  const Mat& K1 = pKF1->mK;                                                  // mK1 = pKF1->mK (:105-106)
  const Mat& K2 = pKF2->mK;
  p.fx1 = K1.at<float>(0, 0); p.fy1 = K1.at<float>(1, 1); p.cx1 = K1.at<float>(0, 2); p.cy1 = K1.at<float>(1, 2);
  p.fx2 = K2.at<float>(0, 0); p.fy2 = K2.at<float>(1, 1); p.cx2 = K2.at<float>(0, 2); p.cy2 = K2.at<float>(1, 2);
  p.bFixScale = bFixScale;
  p.seed = seed;
  return p;
}

static std::vector<lld_amd::Sim3Problem> gather_all(KeyFrame* pKF1, const std::vector<KeyFrame*>& cands,
                                                    const std::vector<std::vector<MapPoint*> >& vv, bool bFixScale,
                                                    const std::vector<uint32_t>& seeds) {
  std::vector<lld_amd::Sim3Problem> out;
  for (size_t i = 0; i < cands.size(); ++i)
    out.push_back(GatherSim3(pKF1, cands[i], vv[i], bFixScale, seeds.empty() ? (uint32_t)i : seeds[i]));
  return out;
}

Sim3Solvers::Sim3Solvers(const lld_amd::Context& ctx, KeyFrame* pKF1, const std::vector<KeyFrame*>& candidates,
                         const std::vector<std::vector<MapPoint*> >& vv, bool bFixScale, const lld_sim3solver_params& params,
                         const std::vector<uint32_t>& seeds)
    : n_(candidates.size()), b_(ctx, gather_all(pKF1, candidates, vv, bFixScale, seeds), params), last_(candidates.size()) {}

void Sim3Solvers::iterate(int nIterations, const std::vector<uint8_t>& active, std::vector<Mat>& Scm, std::vector<bool>& bNoMore,
                          std::vector<std::vector<bool> >& vbInliers, std::vector<int>& nInliers) {
  last_ = b_.iterate(nIterations, active);
  Scm.assign(n_, Mat()); bNoMore.assign(n_, false); vbInliers.assign(n_, std::vector<bool>()); nInliers.assign(n_, 0);
  for (size_t i = 0; i < n_; ++i) {
    bNoMore[i] = last_[i].bNoMore;
    nInliers[i] = last_[i].nInliers;
    vbInliers[i] = last_[i].vbInliers;                                       // mN1 entries, false where no pose
    if (!last_[i].has_pose) continue;                                        // cv::Mat()
    Mat T(4, 4);                                                             // mBestT12: eye(4) with sR | t
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) T.at<float>(r, c) = last_[i].T12[4 * r + c];
    T.at<float>(3, 3) = 1.f;
    Scm[i] = T;
  }
}

Mat Sim3Solvers::GetEstimatedRotation(size_t i) const { return Mat(3, 3, last_[i].R); }

Mat Sim3Solvers::GetEstimatedTranslation(size_t i) const { return Mat(3, 1, last_[i].t); }

}  // namespace lld_adapter
