// lld_sim3_adapter.h — host adapter for LoopClosing::ComputeSim3's Sim3Solvers on live SLAM objects:
//   Sim3Solver::Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale)      src/Sim3Solver.cc:37-112
//   Sim3Solver::iterate(nIterations, bNoMore, vbInliers, nInliers)   src/Sim3Solver.cc:140-207
// One Sim3Solvers object holds every loop candidate of one ComputeSim3 as a device batch (lld_sim3solver_*, include/lld_amd.h);
// iterate() runs iterate(n) on every candidate still in play at once, which gives what the reference's round robin
// (LoopClosing.cc:289-342) gives for each (one rand() stream per candidate).  Same object model switch as lld_optimizer_adapter.h
// (LLD_ADAPTER_OBJECTS_HEADER).
#ifndef LLD_SIM3_ADAPTER_H
#define LLD_SIM3_ADAPTER_H

#include <vector>

#include "../include/lld_amd.hpp"

#ifndef LLD_ADAPTER_OBJECTS_HEADER
#define LLD_ADAPTER_OBJECTS_HEADER "lld_slam_objects.h"
#endif
#include LLD_ADAPTER_OBJECTS_HEADER

namespace lld_adapter {

using lld_slam::KeyFrame;
using lld_slam::MapPoint;
using lld_slam::Mat;

// The constructor's gather: an entry is skipped when vpMatched12[i1] or pKF1->GetMapPointMatches()[i1] is NULL, either point
// isBad(), or either GetIndexInKeyFrame is < 0; world points, mvLevelSigma2[octave] of both keypoints, index1 = i1, both poses
// and both mK.
lld_amd::Sim3Problem GatherSim3(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, bool bFixScale,
                                uint32_t seed);

class Sim3Solvers {
 public:
  // One solver per candidate pKF2 = candidates[i] with vpMatched12 = vvpMatched12[i] (LoopClosing.cc:262-281, in order), with
  // SetRansacParameters(params).  seeds: one per candidate; empty = the candidate's position i.
  Sim3Solvers(const lld_amd::Context& ctx, KeyFrame* pKF1, const std::vector<KeyFrame*>& candidates,
              const std::vector<std::vector<MapPoint*> >& vvpMatched12, bool bFixScale,
              const lld_sim3solver_params& params = lld_amd::Sim3SolverBatch::defaults(), const std::vector<uint32_t>& seeds = {});
  // iterate(nIterations, bNoMore, vbInliers, nInliers) on every candidate with active[i] (empty: all); Scm[i] is the 4x4 CV_32F
  // T12 the reference returns, or an empty Mat.  Inactive candidates keep their previous outputs.
  void iterate(int nIterations, const std::vector<uint8_t>& active, std::vector<Mat>& Scm, std::vector<bool>& bNoMore,
               std::vector<std::vector<bool> >& vbInliers, std::vector<int>& nInliers);
  // GetEstimatedRotation (3x3) / Translation (3x1) / Scale of candidate i after the last iterate call: its best hypothesis.
  Mat GetEstimatedRotation(size_t i) const;
  Mat GetEstimatedTranslation(size_t i) const;
  float GetEstimatedScale(size_t i) const { return last_[i].s; }
  size_t size() const { return n_; }
 private:
  size_t n_;
  lld_amd::Sim3SolverBatch b_;
  std::vector<lld_amd::Sim3Output> last_;
};

}  // namespace lld_adapter
#endif
