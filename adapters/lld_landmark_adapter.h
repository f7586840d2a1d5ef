// lld_landmark_adapter.h — host adapter for the per-landmark refresh on live SLAM objects:
//   MapPoint::ComputeDistinctiveDescriptors()   src/MapPoint.cc:242-307
//   MapPoint::UpdateNormalAndDepth()            src/MapPoint.cc:330-371
//   MapLine::ComputeDistinctiveDescriptors()    src/MapLine.cc:133-201
// for a whole vector of landmarks in one device call each (lld_mappoint_refresh / lld_mapline_distinctive, include/lld_amd.h).
// Both gather the observations in std::map order, make one call and scatter into mDescriptor / mNormalVector / mfMinDistance /
// mfMaxDistance; a landmark the reference would return early on is left exactly as it was.  Same object model switch as
// lld_optimizer_adapter.h (LLD_ADAPTER_OBJECTS_HEADER).
#ifndef LLD_LANDMARK_ADAPTER_H
#define LLD_LANDMARK_ADAPTER_H

#include <vector>

#include "../include/lld_amd.hpp"

#ifndef LLD_ADAPTER_OBJECTS_HEADER
#define LLD_ADAPTER_OBJECTS_HEADER "lld_slam_objects.h"
#endif
#include LLD_ADAPTER_OBJECTS_HEADER

namespace lld_adapter {

using lld_slam::KeyFrame;
using lld_slam::MapLine;
using lld_slam::MapPoint;

// flags: LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH (ProcessNewKeyFrame, SearchInNeighbors) or LLD_LANDMARK_NORMAL_DEPTH
// alone (the tail of LocalBundleAdjustment, CorrectLoop).  A nullptr entry is skipped.  The scale table is the one of the first
// reference keyframe met (DEVIATION (scales) of include/lld_amd.h).  Returns the number of points with anything written.
int RefreshMapPoints(const lld_amd::Context& ctx, const std::vector<MapPoint*>& vpMapPoints,
                     unsigned flags = LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH);
// Returns the number of lines whose mDescriptor was written.
int ComputeDistinctiveDescriptors(const lld_amd::Context& ctx, const std::vector<MapLine*>& vpMapLines);

}  // namespace lld_adapter
#endif
