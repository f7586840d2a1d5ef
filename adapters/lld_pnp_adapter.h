// lld_pnp_adapter.h — host adapter for Tracking::Relocalization's PnPsolvers on live SLAM objects:
//   PnPsolver::PnPsolver(const Frame&, const vector<MapPoint*>&)   src/PnPsolver.cc:66-110
//   PnPsolver::iterate(nIterations, bNoMore, vbInliers, nInliers)  src/PnPsolver.cc:165-258
// One PnPsolvers object holds every candidate of one relocalisation as a device batch (lld_pnp_*, include/lld_amd.h); iterate()
// runs iterate(n) on every candidate still in play at once, which gives what the reference's round robin (Tracking.cc:1894-1916)
// gives for each (one rand() stream per candidate).  Same object model switch as lld_optimizer_adapter.h (LLD_ADAPTER_OBJECTS_HEADER).
#ifndef LLD_PNP_ADAPTER_H
#define LLD_PNP_ADAPTER_H

#include <vector>

#include "../include/lld_amd.hpp"

#ifndef LLD_ADAPTER_OBJECTS_HEADER
#define LLD_ADAPTER_OBJECTS_HEADER "lld_slam_objects.h"
#endif
#include LLD_ADAPTER_OBJECTS_HEADER

namespace lld_adapter {

using lld_slam::Frame;
using lld_slam::MapPoint;
using lld_slam::Mat;

// The constructor's gather: NULL and isBad() matches skipped; mvKeysUn[i].pt, mvLevelSigma2[octave], GetWorldPos(),
// mvKeyPointIndices = i; fu, fv, uc, vc = F.fx, fy, cx, cy.
lld_amd::PnPProblem GatherPnP(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches, uint32_t seed);

class PnPsolvers {
 public:
  // One solver per entry of vvpMapPointMatches (the candidates of Tracking.cc:1864-1873, in order), with SetRansacParameters(params).
  // seeds: one per candidate; empty = the candidate's position i (the documented default).
  PnPsolvers(const lld_amd::Context& ctx, const Frame& F, const std::vector<std::vector<MapPoint*> >& vvpMapPointMatches,
             const lld_pnp_params& params = lld_amd::PnPsolverBatch::defaults(), const std::vector<uint32_t>& seeds = {});
  // iterate(nIterations, bNoMore, vbInliers, nInliers) on every candidate with active[i] (empty: all); Tcw[i] is the 4x4 CV_32F pose
  // the reference returns, or an empty Mat.  Inactive candidates keep their previous outputs.
  void iterate(int nIterations, const std::vector<uint8_t>& active, std::vector<Mat>& Tcw, std::vector<bool>& bNoMore,
               std::vector<std::vector<bool> >& vbInliers, std::vector<int>& nInliers);
  size_t size() const { return n_; }
 private:
  size_t n_;
  lld_amd::PnPsolverBatch b_;
};

}  // namespace lld_adapter
#endif
