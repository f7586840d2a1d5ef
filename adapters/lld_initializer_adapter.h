// lld_initializer_adapter.h — host adapter for Tracking::MonocularInitialization's Initializer on live SLAM objects:
//   Initializer::Initializer(ReferenceFrame, sigma, iterations)                              src/Initializer.cc:33-42
//   Initializer::Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated)        src/Initializer.cc:44-121
// The object holds the reference frame's mK and mvKeysUn on the device (lld_initializer_*, include/lld_amd.h) for as long as the
// reference's Initializer lives.  Same object model switch as lld_optimizer_adapter.h (LLD_ADAPTER_OBJECTS_HEADER).
#ifndef LLD_INITIALIZER_ADAPTER_H
#define LLD_INITIALIZER_ADAPTER_H

#include <vector>

#include "../include/lld_amd.hpp"

#ifndef LLD_ADAPTER_OBJECTS_HEADER
#define LLD_ADAPTER_OBJECTS_HEADER "lld_slam_objects.h"
#endif
#include LLD_ADAPTER_OBJECTS_HEADER

namespace lld_adapter {

using lld_slam::Frame;
using lld_slam::Mat;
using lld_slam::Point3f;

class Initializer {
 public:
  // mK = ReferenceFrame.mK.clone(); mvKeys1 = ReferenceFrame.mvKeysUn.  seed: srand(seed) of every call's stream (DEVIATION 1).
  Initializer(const lld_amd::Context& ctx, const Frame& ReferenceFrame, float sigma = 1.0f, int iterations = 200, uint32_t seed = 0);
  // Returns the reference's bool.  On success R21 (3x3 CV_32F), t21 (3x1), vP3D and vbTriangulated (mvKeys1.size() entries each)
  // are filled; on failure they are left as they were.  Neither frame is written.
  bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, Mat& R21, Mat& t21, std::vector<Point3f>& vP3D,
                  std::vector<bool>& vbTriangulated);
  // every output of the last call (diagnostics)
  const lld_amd::InitializerOutput& last() const { return ini_.last(); }
 private:
  lld_amd::Initializer ini_;
};

}  // namespace lld_adapter
#endif
