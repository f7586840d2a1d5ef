// lld_localmapping_adapter.h — host adapter for LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:208-453) on live SLAM objects.
// The neighbour loop stays on the host and stays sequential: a point created at idx1 for neighbour i makes
// ORBmatcher::SearchForTriangulation skip that keypoint for neighbour i+1 (the pMP1 test of src/ORBmatcher.cc:699-708), so the
// neighbours cannot be batched without changing the result.  Per neighbour: the baseline gate (:245-262), ComputeF12 (:537-554) on the
// host, the SearchForTriangulation adapter (lld_matcher_adapter), ONE lld_new_points_triangulate call with one pair for the loop
// body (:287-432), then the reference's bookkeeping (:435-450) for every created point in its order.  The per-point
// ComputeDistinctiveDescriptors / UpdateNormalAndDepth (:443-445) become one RefreshMapPoints (lld_landmark_adapter) for all new
// points at the end - also before an early return: with exactly two observations and fixed poses the result does not depend on when
// it runs.  Same object model switch as lld_optimizer_adapter.h (LLD_ADAPTER_OBJECTS_HEADER).
#ifndef LLD_LOCALMAPPING_ADAPTER_H
#define LLD_LOCALMAPPING_ADAPTER_H

#include <functional>
#include <list>
#include <vector>

#include "lld_landmark_adapter.h"
#include "lld_matcher_adapter.h"

namespace lld_adapter {

using lld_slam::Map;

// What one call did (optional; the tests read it, a live system passes nullptr): one entry per neighbour visited.
struct NewPointsTrace {
  std::vector<int> skipped, n_matches, n_new;                       // the baseline gate, vMatchedIndices.size(), points created
  bool returned_early = false;                                     // CheckNewKeyFrames() fired at some i > 0
};

// cv::Mat LocalMapping::ComputeF12(KeyFrame *&pKF1, KeyFrame *&pKF2) (:537-554).  Products by DEVIATION 2 of include/lld_amd.h
// (float products summed in double in index order, rounded once; a chain A*B*C is (A*B)*C; then the float + t1w), K1.t().inv() and
// K2.inv() by its cofactor rule.
lld_slam::Mat ComputeF12(KeyFrame*& pKF1, KeyFrame*& pKF2);

// void LocalMapping::CreateNewMapPoints() with its members as arguments.  CheckNewKeyFrames is asked before every neighbour but the
// first (:240-241).  Returns nnew.
int CreateNewMapPoints(const lld_amd::Context& ctx, KeyFrame* mpCurrentKeyFrame, Map* mpMap, bool mbMonocular,
                       std::list<MapPoint*>& mlpRecentAddedMapPoints, const std::function<bool()>& CheckNewKeyFrames,
                       NewPointsTrace* trace = nullptr);

}  // namespace lld_adapter
#endif
