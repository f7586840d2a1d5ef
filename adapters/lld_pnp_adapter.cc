// lld_pnp_adapter.cc — see lld_pnp_adapter.h.
#include "lld_pnp_adapter.h"

namespace lld_adapter {

lld_amd::PnPProblem GatherPnP(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches, uint32_t seed) {
  lld_amd::PnPProblem p;
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {      // PnPsolver.cc:79-101
    MapPoint* pMP = vpMapPointMatches[i];
    if (!pMP || pMP->isBad()) continue;
    const lld_slam::KeyPoint& kp = F.mvKeysUn[i];
    p.uv.push_back(kp.pt.x);
    p.uv.push_back(kp.pt.y);
    p.sigma2.push_back(F.mvLevelSigma2[kp.octave]);
    Mat Pos = pMP->GetWorldPos();
    p.xyz.push_back(Pos.at<float>(0));
    p.xyz.push_back(Pos.at<float>(1));
    p.xyz.push_back(Pos.at<float>(2));
    p.kp_index.push_back((int32_t)i);
  }
  p.n_keypoints = (int32_t)vpMapPointMatches.size();
  p.fx = F.fx; p.fy = F.fy; p.cx = F.cx; p.cy = F.cy;                        // :104-107
  p.seed = seed;
  return p;
}

static std::vector<lld_amd::PnPProblem> gather_all(const Frame& F, const std::vector<std::vector<MapPoint*> >& vv,
                                                   const std::vector<uint32_t>& seeds) {
  std::vector<lld_amd::PnPProblem> out;
  for (size_t i = 0; i < vv.size(); ++i) out.push_back(GatherPnP(F, vv[i], seeds.empty() ? (uint32_t)i : seeds[i]));
  return out;
}

PnPsolvers::PnPsolvers(const lld_amd::Context& ctx, const Frame& F, const std::vector<std::vector<MapPoint*> >& vv,
                       const lld_pnp_params& params, const std::vector<uint32_t>& seeds)
    : n_(vv.size()), b_(ctx, gather_all(F, vv, seeds), params) {}

void PnPsolvers::iterate(int nIterations, const std::vector<uint8_t>& active, std::vector<Mat>& Tcw, std::vector<bool>& bNoMore,
                         std::vector<std::vector<bool> >& vbInliers, std::vector<int>& nInliers) {
  std::vector<lld_amd::PnPOutput> o = b_.iterate(nIterations, active);
  Tcw.assign(n_, Mat()); bNoMore.assign(n_, false); vbInliers.assign(n_, std::vector<bool>()); nInliers.assign(n_, 0);
  for (size_t i = 0; i < n_; ++i) {
    bNoMore[i] = o[i].bNoMore;
    nInliers[i] = o[i].nInliers;
    if (!o[i].has_pose) continue;                                            // cv::Mat() and an empty vbInliers
    Mat T(4, 4);                                                             // mBestTcw / mRefinedTcw: eye(4) with R | t
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) T.at<float>(r, c) = o[i].Tcw[4 * r + c];
    T.at<float>(3, 3) = 1.f;
    Tcw[i] = T;
    vbInliers[i] = o[i].vbInliers;
  }
}

}  // namespace lld_adapter
